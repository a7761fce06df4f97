// k_tend.h - K1: PV tendency + leapfrog + layer->mode projection, one pass.
//
// Replaces, per ocean step (reference file:line):
//   del2p = Del^2(pom) with mixed BCs            src/qgosubs.F:86-130
//   ocadif: d4p, d6p, Arakawa 9-pt J(q,p), dqdt  src/qgosubs.F:306-400
//   forcing / bottom drag / leapfrog             src/qgosubs.F:173-219
//   ocinvq projection onto modes                 src/ocisubs.F:117-139
//
// One workgroup owns a TX x TY tile of p-points for ALL layers.  Per layer
// the radius-3 halo of pom and the radius-1 halos of po, qo are staged in
// LDS, Del^2 / Del^4 are built in LDS with the reference's boundary rules,
// and each thread finishes Del^6 + Jacobian for its points in registers.
// The global loads of layer k+1 (and of the point-wise epilogue operands) are
// issued into registers before layer k is computed, so a workgroup always
// has loads in flight (software pipelining across layers).
// Workgroups are renumbered so that each XCD (blockIdx mod 8) sweeps a
// contiguous band of tile rows: the halo rows re-read by vertically adjacent
// tiles then hit that XCD's own L2 instead of being re-fetched.
// Tile shape: 16 x 16 points, 256 threads, one point per thread (72 VGPRs, 12 KB LDS: 7 workgroups per CU). The
// kernel is bound by its chain of barrier-separated phases, so resident workgroups matter more than halo
// re-reads: measured at 5 km 64x8 (2 points per thread, 5 per CU) 38.4 us, 32x8 35.0, 16x16 33.3, 16x8 35.1,
// 32x16/512 threads 35.3, 16x32/512 36.2.
// Expression association order is the reference's, and the library is built
// with -ffp-contract=off, so qgostep reproduces the CPU reference bit for bit.
//
// Algorithmic HBM traffic: read pom,po,qo,qom (4 nl) + wekpo,entoc,ddynoc (3),
// write qo (nl) + wrk (nl)  ->  (6 nl + 3) N doubles = 21 N for nl = 3
// (SURVEY 8d counts 24 N because the reference also rewrites qom; here the
// q buffers rotate instead).  Where the host knows entoc and / or ddynoc to be
// all zero, k_tend_z does not read them: 19 N with both zero (flat bottom,
// mixed layer off - the flagship), 20 N with one.
// The kernels' body is k_tend_body.inc (shared by k_tend and k_tend_z).
#pragma once
#include "qgcm_dev.h"
#include "qg_ref_expr.h" // the five-point sum, the wall rule, the Jacobian
#include "k_misc.h" // constr_dpi_update
#include "k_cyclic.h" // cyc_bsums_block
#include "k_oml.h" // oml_final_block

#ifndef TEND_TX
#define TEND_TX 16
#endif
#ifndef TEND_TY
#define TEND_TY 16
#endif
#ifndef TEND_NT
#define TEND_NT 256
#endif

// Tiles of the HBM-bound sizes (the instantiations without write-through stores, WTQ = false): twice as wide.  A row of a
// 32-wide tile is two whole 128-byte lines per field instead of one, the radius-3 halo columns weigh half as much, and
// at SOcn 5 km / the slabs of NAtl 1 km the kernel's reads come from HBM, not from the Infinity Cache: measured at
// SOcn 5 km (profiles/r4_tend_shapes_socn5.log) 16 x 16: 100.6 us, 32 x 16 (256 threads, two rows per thread): 94.7,
// 32 x 16 / 512 threads: 95.0, 64 x 8: 94.7, 64 x 4: 96.2, 32 x 8: 96.3, 16 x 32: 100.4 (+), 32 x 32: 101.2.  At NAtl 5 km
// (cache resident, write-through pairs) the 16 x 16 tile stays: resident workgroups matter more there (see above).
#ifndef TEND_TX_WIDE
#define TEND_TX_WIDE 32
#endif
static_assert(TEND_TX % 2 == 0 && TEND_TX_WIDE % 2 == 0, "tend_point<.., PAIR> stores the new qo in pairs of neighbouring columns: tiles start on odd columns");

template <bool CYC>
__device__ __forceinline__ int tend_wrap(int gi, int nxt) {
  if (CYC) {
    if (gi < 1) gi += nxt;
    else if (gi > nxt) gi -= nxt;
  }
  return gi;
}

// tiles cover i = 1..imax, local rows jlo..jmax; what is left (E wall column, N wall row) is edge work
struct TendTiling {
  int gx, gy, imax, jmax;
  int ecol, erow; // 1 if the E wall column / N wall row is peeled off
  int nedge;      // edge workgroups
};

template <bool CYC, int TX = TEND_TX>
__host__ __device__ __forceinline__ TendTiling tend_tiling(const QgGeom &g) {
  TendTiling T;
  const int rows = g.jhi - g.jlo + 1;
  T.ecol = (!CYC && g.nx % TX == 1 && g.nx > 1) ? 1 : 0;
  T.erow = (!CYC && rows % TEND_TY == 1 && rows > 1 && g.jhi + g.joff == g.nyg) ? 1 : 0;
  T.gx = T.ecol ? g.nx / TX : (g.nx + TX - 1) / TX;
  T.gy = T.erow ? rows / TEND_TY : (rows + TEND_TY - 1) / TEND_TY;
  T.imax = T.ecol ? g.nx - 1 : g.nx;
  T.jmax = T.erow ? g.jhi - 1 : g.jhi;
  const int npts = T.ecol * rows + T.erow * T.imax;
  T.nedge = (npts + TEND_NT - 1) / TEND_NT;
  return T;
}

// Point-wise part of the step for one p-point and all layers (qgosubs.F:173-219, ocisubs.F:117-139):
// dq = dqdt of the point (0 outside the interior), d2bot = Del^2(pom) of the bottom layer,
// qm / qo = old qom / qo of the point (qo: only read on rows that are not stepped, and with AVG).
// PAIR (the tile kernel's epilogue: EVERY lane of the wave calls, `valid` says whether its point exists): the new qo
// and the work array leave as 16-byte write-through stores of two neighbouring columns (qgcm_dev.h: the 44 MB this
// kernel writes no longer wait, dirty in L2, for the end-of-kernel flush); !PAIR: plain stores (edge workgroups).
// AVG: the leapfrog averaging that follows this step (src/q-gcm.F:1345-1351) is folded into the store of the new qo:
// 0.5*(new qo + qo); the projection keeps the un-averaged value.  A template flag: as a kernel argument the extra
// branches cost the other 24 steps of 25 more than the averaging pass had (measured: +0.5 us per step at 5 km).
template <int NL, bool CYC, bool PAIR = false, bool AVG = false>
__device__ __forceinline__ void tend_point(const QgTendParams &P, int gi, int gj, const double *dq, double d2bot,
                                           const double *qm, const double *qo, double wek, double ent, double ddy,
                                           bool valid = true) {
  const long fs = P.g.fstride;
  const long o = (long)(gj - 1) * P.g.ldx + (gi - 1);
  const bool wallrow = (gj + P.g.joff == 1 || gj + P.g.joff == P.g.nyg);
  if (!PAIR && wallrow) {
    // rows not stepped: the new-qo buffer keeps qo (qgosubs.F:214-219)
#pragma unroll
    for (int k = 0; k < NL; ++k) P.qnew[fs * k + o] = qo[k];
    return;
  }
  double qdot[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) qdot[k] = dq[k];
  if (CYC && P.g.atm) {
    // atmosphere (src/qgasubs.F:128-131): entrainment and Ekman pumping act on the bottom layer 1 with the
    // opposite sign, there is no drag term
    qdot[0] = dq[0] + P.fohfac[0] * (ent - wek);
    qdot[1] = dq[1] - P.fohfac[1] * ent;
  } else {
    qdot[0] = dq[0] + P.fohfac[0] * (wek - ent);
    qdot[1] = dq[1] + P.fohfac[1] * ent;
    qdot[NL - 1] = qdot[NL - 1] - P.bdrfac * d2bot;
  }
  double ql[NL];
  double betay = P.beta * P.yporel[gj - 1];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    double qn = qm[k] + P.tdto * qdot[k]; // qom + tdto*qdot
    // sponge layer of the k247 fork (src/qgosubs.F:203-205), association as written there; a wave-uniform branch on a
    // kernel argument, not taken in any BASELINE configuration
    if (P.rspl) qn = qn + P.tdc1 * P.rspl[valid ? o : 0] * (qm[k] - betay);
    const double qs = AVG ? 0.5 * (qn + qo[k]) : qn;
    if (PAIR) {
      // (rows not stepped keep qo, qgosubs.F:214-219; o is even on even lanes: the tile starts at an odd column)
      qg_pair_store_wt(P.qnew + fs * k + o, wallrow ? qo[k] : qs, valid);
    } else {
      P.qnew[fs * k + o] = qs;
    }
    ql[k] = qn - betay;
  }
  if (CYC && P.g.atm) ql[0] = ql[0] - ddy; // topography under layer 1, src/atisubs.F:117
  else ql[NL - 1] = ql[NL - 1] - ddy;
  int c = CYC ? gi - 1 : gi - 2;
  const bool cok = c >= 0 && c < P.g.nk && !wallrow;
  if (PAIR || cok) {
#pragma unroll
    for (int m = 0; m < NL; ++m) {
      double qmm = 0.0;
#pragma unroll
      for (int k = 0; k < NL; ++k) qmm = qmm + P.ctl2m[k + NL * m] * ql[k];
      // (plain stores: the box ocean's column c = gi - 2 is even on ODD lanes, and pairs that start on odd lanes leave
      //  lanes 0 and 15 of every tile row with single elements.  Measured: those as 8-byte plain stores into lines the
      //  16-byte write-through stores keep dropping from L2: kernel 29.6 -> 82 us; as 8-byte sc1 stores: 33.3 us.)
      if (valid && cok) P.wrk[P.g.wstride * m + (long)(gj - 1) * P.g.ldw + c] = P.fnot * qmm;
    }
  }
}

// Edge work of the box ocean: the E wall column (dqdt = 0, qgosubs.F:371,397; Del^2 of the bottom layer by
// the wall rule :112,125) and the N wall row (not stepped), one point per thread.
// ZM: the zero-field mask of k_tend_z below (bit 0: entoc, bit 1: ddynoc are all zero and not read).
template <int NL, bool AVG = false, int ZM = 0>
__device__ __forceinline__ void tend_edge(const QgTendParams &P, const TendTiling &T, int eblock) {
  const QgGeom &g = P.g;
  const int rows = g.jhi - g.jlo + 1;
  const int t = eblock * TEND_NT + (int)threadIdx.x;
  int gi, gj;
  if (t < T.ecol * rows) {
    gi = g.nx;
    gj = g.jlo + t;
  } else {
    const int u = t - T.ecol * rows;
    if (!T.erow || u >= T.imax) return;
    gi = 1 + u;
    gj = g.jhi;
  }
  const long fs = g.fstride;
  const long o = (long)(gj - 1) * g.ldx + (gi - 1);
  const bool wallrow = (gj + g.joff == 1 || gj + g.joff == g.nyg);
  double dq[NL], qm[NL], qo[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    dq[k] = 0.0;
    qm[k] = wallrow ? 0.0 : P.qnew[fs * k + o];
    qo[k] = (wallrow || AVG) ? P.qo[fs * k + o] : 0.0; // (AVG: tend_point stores 0.5*(new qo + qo))
  }
  double d2bot = 0.0, wek = 0.0, ent = 0.0, ddy = 0.0;
  if (!wallrow) { // then gi == nx: E wall column of a stepped row
    const double *pb = P.pom + fs * (NL - 1) + o;
    d2bot = QG_WALL_RULE(P.bcfaco, pb[-1], pb[0]);
    wek = P.wekpo[o];
    if (!(ZM & 1)) ent = P.entoc[o];
    if (!(ZM & 2)) ddy = P.ddynoc[o];
  }
  tend_point<NL, false, false, AVG>(P, gi, gj, dq, d2bot, qm, qo, wek, ent, ddy);
}

// WTQ: the epilogue stores the new qo in write-through pairs (tend_point<.., PAIR>) - worth 1 us per step while the
// step's working set stays in the Infinity Cache (NAtl 5 km), but it costs 6 VGPRs (78: six waves per SIMD instead of
// seven) and at HBM-bound sizes, where L2's own full-line evictions already spread the writes over the kernel, it made
// the kernel slower (SOcn 5 km 95 -> 103 us, written through or not): the host picks the instantiation by size.
template <int NL, bool CYC, bool WTQ, bool AVG = false>
#ifndef TEND_WAVES_PER_EU
#define TEND_WAVES_PER_EU 4
#endif
#ifndef TEND_WAVES_WTQ
#define TEND_WAVES_WTQ 4
#endif
__global__ __launch_bounds__(TEND_NT, (WTQ && NL <= 4) ? TEND_WAVES_WTQ : TEND_WAVES_PER_EU) void k_tend(QG_TEND_ARGS, const QgTendParams P,
                                                                     const QgCycSumParams S, const QgOmlFinal F) {
  constexpr int ZM = 0; // reads entoc and ddynoc
#include "k_tend_body.inc"
}

// Zero-field variants: the same kernel for a handle whose entoc (ZM bit 0) and / or ddynoc (ZM bit 1) is known on the
// host to be all +0.0 (qgcm_hip.hip: tend_zmask).  A field whose bit is set is neither loaded nor given a prefetch
// register; the epilogue computes with a literal 0.0 in its place, expression by expression as written in tend_point,
// so signed zeros and rounding are the reading kernel's.  A second kernel name: k_tend<NL, CYC, WTQ, AVG> keeps its
// name, its template list and its code (ZM = 0).  Instantiated for NL = 2, 3, 4; NL > 4 keeps reading the fields.
template <int NL, bool CYC, bool WTQ, bool AVG, int ZM>
__global__ __launch_bounds__(TEND_NT, (WTQ && NL <= 4) ? TEND_WAVES_WTQ : TEND_WAVES_PER_EU) void k_tend_z(QG_TEND_ARGS, const QgTendParams P,
                                                                       const QgCycSumParams S, const QgOmlFinal F) {
  static_assert(ZM >= 1 && ZM <= 3 && NL <= 4, "ZM = 0 is k_tend");
#include "k_tend_body.inc"
}
