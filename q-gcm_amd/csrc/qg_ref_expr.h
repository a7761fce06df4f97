// qg_ref_expr.h - the reference expressions of the tendency kernels, each written ONCE, in the reference's association
// order (built with -ffp-contract=off: these lines make qgostep bit-identical to the CPU reference).  Two forms of one
// text: QG_XXX(..), an expression macro - to the compiler the text it replaced, the form of the tile
// kernels (k_tend_body.inc, tend_edge, k_qocdiag.h, k_cyclic.h), where a function around a single expression changes the
// schedule and the code length - and qg_xxx(..), a forced-inline function defined by the macro, for the kernel that
// compiles to the same code either way (k_tend_rows.h).  Arguments are named by compass point around the centre c0:
// S / N rows j-1 / j+1, W / E columns i-1 / i+1.
#pragma once
#include "qgcm_dev.h"

// Five-point sum: the bracket of Del^2 (src/qgosubs.F:116-117), Del^4 (:330-331), Del^6 (:354-355, :375-376) and of
// qocdiag_out's copies (src/qocdiag.F:417-540).  The factor dxom2 is the caller's: the reference multiplies from
// either side, the bits are equal, but the operand order reaches the instruction stream.
#define QG_FIVE_POINT(cS, cW, cE, cN, c0) ((cS) + (cW) + (cE) + (cN) - 4.0 * (c0))
// Mixed boundary condition at a wall point (src/qgosubs.F:98-99,112,125; :311-312,326,339).  The inner neighbour is N on
// the S wall row, S on the N wall row, E on the W wall column, W on the E wall column; rows before columns at the corners.
#define QG_WALL_RULE(bcf, inner, c0) ((bcf) * ((inner) - (c0)))
// Arakawa Jacobian J(q, p) without adfaco (src/qgosubs.F:379-388; cyclic W column :358-367): ten terms left to right, in
// two halves (k_tend_body.inc keeps a compiler barrier between them).  QG_JAC_TAIL(QG_JAC_HEAD(..), ..) parses as
// (((((((((t1 + t2) + t3) - t4) - t5) + t6) + t7) - t8) - t9) + t10): the reference's single expression.
#define QG_JAC_HEAD(qS, qW, qE, qN, pS, pW, pE, pN, pSW, pSE, pNW, pNE)                                               \
  (((qE) - (qW)) * ((pN) - (pS)) + ((qS) - (qN)) * ((pE) - (pW)) + (qE) * ((pNE) - (pSE)) - (qW) * ((pNW) - (pSW)) - \
   (qN) * ((pNE) - (pNW)) + (qS) * ((pSE) - (pSW)))
#define QG_JAC_TAIL(jac, pS, pW, pE, pN, qSW, qSE, qNW, qNE) \
  ((jac) + (pN) * ((qNE) - (qNW)) - (pS) * ((qSE) - (qSW)) - (pE) * ((qNE) - (qSE)) + (pW) * ((qNW) - (qSW)))

__device__ __forceinline__ double qg_five_point(double cS, double cW, double cE, double cN, double c0) {
  return QG_FIVE_POINT(cS, cW, cE, cN, c0);
}
__device__ __forceinline__ double qg_wall_rule(double bcf, double inner, double c0) { return QG_WALL_RULE(bcf, inner, c0); }
__device__ __forceinline__ double qg_jac_head(double qS, double qW, double qE, double qN, double pS, double pW, double pE,
                                              double pN, double pSW, double pSE, double pNW, double pNE) {
  return QG_JAC_HEAD(qS, qW, qE, qN, pS, pW, pE, pN, pSW, pSE, pNW, pNE);
}
__device__ __forceinline__ double qg_jac_tail(double jac, double pS, double pW, double pE, double pN, double qSW, double qSE,
                                              double qNW, double qNE) {
  return QG_JAC_TAIL(jac, pS, pW, pE, pN, qSW, qSE, qNW, qNE);
}
