// qg_ref_expr.h - the reference expressions of the step, each written ONCE, in the reference's association order (built
// with -ffp-contract=off: these lines make qgostep, ocinvq and ocqbdy bit-identical to the CPU reference).  Two forms of
// one text: QG_XXX(..), an expression macro - to the compiler the text it replaced, the form of the tile
// kernels (k_tend_body.inc, tend_edge, k_qocdiag.h, k_cyclic.h), where a function around a single expression changes the
// schedule and the code length - and qg_xxx(..), a forced-inline function defined by the macro, for the sites that
// compile to the same code either way (k_tend_rows.h; in section 2 qg_hom_box, qg_modes_to_layer and qg_bdy_q).
#pragma once
#include "qgcm_dev.h"

// ---- 1. the tendency kernels; arguments by compass point around the centre c0: S / N rows j-1 / j+1, W / E columns i-1 / i+1
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

// ---- 2. the epilogue of the inversion (k_unpack_box, k_ocqbdy, k_unpack_cyc, k_dst64_unpack, k_rfft64_unpack,
// k_rfft3_unpack) and the y-slab halo messages; operands are arguments: a register array, LDS or a global field alike
// Homogeneous part of mode m = 1 .. nl-1.  Box (src/ocisubs.F:388): pm(m) = wrk(i,j,m) + hclco(m-1) * ochom(i,j,m-1).
// Channel (:307, :310): homcor(1) = c3 * pbh(j), homcor(m) = c1(m-1) * pch1(j,m-1) + c2(m-1) * pch2(j,m-1); c1, c2 count
// from 0, pch1 / pch2 are [mode - 1][ny], j is a local row from 1.
#define QG_HOM_BOX(wv, hc, oh) ((wv) + (hc) * (oh))
#define QG_HOM_CHANNEL0(c3, pbh, j) ((c3) * (pbh)[(j) - 1])
#define QG_HOM_CHANNEL(c1, c2, pch1, pch2, ny, j, m) \
  ((c1)[(m) - 1] * (pch1)[((j) - 1) + (long)(ny) * ((m) - 1)] + (c2)[(m) - 1] * (pch2)[((j) - 1) + (long)(ny) * ((m) - 1)])
// Modes -> layers (src/ocisubs.F:318-322, 392-396; :258-261): pl = 0.0, then pl = pl + ctm2l(m,k) * pm(m) for each m in
// turn; ctm2l(m,k) sits at m + nl * k.  k_rfft3_unpack, which mixes before the transform, uses the term alone.
#define QG_CTM2L(ctm2l, nl, m, k) ((ctm2l)[(m) + (nl) * (k)])
#define QG_M2L_TERM(ctm2l, nl, m, k, pm) (QG_CTM2L(ctm2l, nl, m, k) * (pm))
// Vertical coupling of layer k at a boundary point (src/vorsubs.F:245-388): ap = sum of f0 A(k,l) p(l) over l = k-1, k,
// k+1, left to right, without the layer that does not exist; f0A(k,l) sits at k + nl * l.  pkm / pk0 / pkp: the pressure
// of layers k-1 / k / k+1 at the point; only the operands of the case taken are evaluated.
#define QG_AP_TERM(f0A, nl, k, l, p) ((f0A)[(k) + (nl) * (l)] * (p))
#define QG_AP_TOP(f0A, nl, pk0, pkp) (QG_AP_TERM(f0A, nl, 0, 0, pk0) + QG_AP_TERM(f0A, nl, 0, 1, pkp))
#define QG_AP_BOTTOM(f0A, nl, k, pkm, pk0) (QG_AP_TERM(f0A, nl, k, (k) - 1, pkm) + QG_AP_TERM(f0A, nl, k, k, pk0))
#define QG_AP_INTERIOR(f0A, nl, k, pkm, pk0, pkp) (QG_AP_TERM(f0A, nl, k, (k) - 1, pkm) + QG_AP_TERM(f0A, nl, k, k, pk0) + QG_AP_TERM(f0A, nl, k, (k) + 1, pkp))
#define QG_AP(f0A, nl, k, pkm, pk0, pkp) \
  ((k) == 0 ? QG_AP_TOP(f0A, nl, pk0, pkp) : (k) == (nl) - 1 ? QG_AP_BOTTOM(f0A, nl, k, pkm, pk0) : QG_AP_INTERIOR(f0A, nl, k, pkm, pk0, pkp))
// atqzbd's exception (src/vorsubs.F:470): on the southern boundary the atmosphere's top layer (k = nl - 1 here) takes
// layer k from row 2, the inward neighbour pin; it replaces QG_AP's value there
#define QG_AP_ATQZBD(f0A, nl, k, pkm, pin) QG_AP_BOTTOM(f0A, nl, k, pkm, pin)
// Boundary PV (src/vorsubs.F:268 and each side's lines): q = bcfaco_f0 * (pin - pw) - ap + by, that is ((bcf * (pin -
// pw)) - ap) + by; pw the wall value, pin its inward neighbour, by = beta * yporel(j).  Then q = q + ddyn(i,j), the
// topography, in one layer only: the ocean's bottom layer, the atmosphere's first.
#define QG_BDY_Q(bcf, pin, pw, ap, by) ((bcf) * ((pin) - (pw)) - (ap) + (by))
#define QG_TOPO_LAYER(atm, nl) ((atm) ? 0 : (nl) - 1)
// Halo message of one direction: [k][3 rows][ldx] of p, then [k][ldx] of q; offset of a row's first column (a long).
// p row r = 0 .. 2 is owned row jlo + r (to the lower neighbour) or jhi - 2 + r (to the upper), the q row is jlo / jhi.
// The length is where a q row of layer nl would begin; the host sizes its buffers by it (halo_msg_len).
#define QG_HALO_P(k, r, ldx) (((long)(k) * 3 + (r)) * (ldx))
#define QG_HALO_Q(nl, k, ldx) (((long)(nl) * 3 + (k)) * (ldx))
#define QG_HALO_LEN(nl, ldx) ((size_t)QG_HALO_Q(nl, nl, ldx))
__device__ __forceinline__ double qg_hom_box(double wv, double hc, double oh) { return QG_HOM_BOX(wv, hc, oh); }
template <int NL>
__device__ __forceinline__ double qg_modes_to_layer(const double *ctm2l, int k, const double *pm) {
  double v = 0.0;
#pragma unroll
  for (int m = 0; m < NL; ++m) v = v + QG_M2L_TERM(ctm2l, NL, m, k, pm[m]);
  return v;
}
__device__ __forceinline__ double qg_bdy_q(double bcf, double pin, double pw, double ap, double by) { return QG_BDY_Q(bcf, pin, pw, ap, by); }
