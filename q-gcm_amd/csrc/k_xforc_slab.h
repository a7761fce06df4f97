// k_xforc_slab.h - xforc for an ocean held as y-slabs under a replicated whole-domain atmosphere.  Compiled
// in k_xforc_slab.hip only.  The atmosphere side runs the kernels of k_xforc.h unchanged on every rank's replica; here is
// what the ocean side adds:
//
//   k_xf_wekpo_slab       k_wekpo (k_setup.h) on the slab's local p rows: a row is a zonal boundary by its GLOBAL index
//   k_xf_lines_oc_slab    cyclic ocean: txisoc, txinoc from the replicated fine stress rows (raoro * txf formed inline:
//                         the operands of tauxo), in k_xf_lines' order - every rank holds the bits of the whole-domain call
//   k_xf_heat_oc_slab     k_xf_heat_oc on the slab's T rows: fnetoc pointwise on every local T row; per atmosphere cell the
//                         sums over the OWNED points only, lane / point order of k_xf_heat_oc and the xor butterfly, into
//                         the message (4, ncell): fnetat sum, arocsm, slhfsm, oradsm; +0.0 for a cell the slab does not own a
//                         point of
//   k_xf_heat_combine     cell sums and monitor partials = the ranks' messages added in rank order (the same on every rank)
//
// and, for the banded mode (rank r runs the atmosphere side on the fine rows its band of atmosphere p rows and
// its slab need, instead of on the whole replica), what the atmosphere side becomes:
//
//   k_xf_*_win            the atmosphere-side kernels of k_xforc.h on the rows j0 .. j0 + gridDim.y - 1: the same text
//                         (k_xforc_rows.inc), so a row holds the bits the whole-domain launch gives it
//   k_xf_band_pack        the band's rows of tauxa, tauya, uekat, vekat, wekta, wekpa and the line sums the rank owns
//                         -> the message's momentum block
//   k_xf_band_scatter     every rank's rows and line sums -> the replica's arrays and scalars: a copy, no sum
//
// and, for tau_udiff (the basin's pom(:,:,1) assembled on every rank ahead of the atmosphere side, which then
// runs k_xf_fine / k_xf_fine_win with P.udiff = 1 on the assembled array, their text unchanged):
//
//   k_xf_pom_pack         the slab's OWNED p rows of layer 1 of the lagged pressure -> the message
//   k_xf_pom_assemble     every rank's rows -> the assembled array (nxpo, nypo): a copy, one writer per point
//
// and, for tau_udiff without that gather (every rank forms the fine stress above the rows it OWNS and the ranks
// exchange rank-ordered partial sums of the coarse fields):
//
//   k_xf_edge_pack        the first 4 and the last 4 OWNED p rows of layer 1 of the lagged pressure -> the edge message
//   k_xf_edge_assemble    the slab's owned rows and the 4 rows beyond each seam (the direct neighbours' edges) -> the
//                         basin-sized array of 6q: rows g0 - 4 .. g1 + 4 are the basin's bits, the rest is not written
//   k_xf_sums_atm         coarse rows a0 .. : tauxa, tauya, vekat where the rank owns the sampled fine row (k_xf_atm's
//                         expressions) and the terms of uekat's meridional line that lie in the owned fine rows
//   k_xf_sums_wekpa       the rows of wekpa's box that lie in the owned fine T rows: the numerator, k_xf_wekpa's order
//   k_xf_sums_combine     samples and line sums from their one owner; uekat, wekpa from the contributing ranks' partials,
//                         the first one's value then the others added in rank order
//
// A cell wholly inside one slab keeps the bits of the whole-domain sum (x + 0.0 = x); a cell a seam cuts is a sum of the
// same terms in another order.  No atomics; every sum has a fixed tree.
#pragma once
#include "qgcm_dev.h"
#include "k_xf_heat_params.h"
#include "k_xforc_rows.h" // QgXfParams, xf_point

#define XFS_NT 256

struct QgXfSlabParams {
  int nx, nxt, nyl, joff, nyg; // local p rows nyl; global row = local row + joff; nyg rows in the basin
  int ldx, ldt, ldf;           // pitches: ocean p grid, ocean T grid (wekto), fine atmosphere p grid
  int cyc, iocoff, jocoff;     // (iocoff, jocoff): the ocean's GLOBAL offset in the fine grid
  const double *txf;           // tauxaor
  const double *wekto;         // local T rows (nyl - 1)
  double *wekpo;
  QgScalars *sco;              // the cyclic ocean's device scalars
  double raoro, dxo;
  int lines;                   // k_xf_lines_oc_slab: bit 0 txisoc, bit 1 txinoc (replicated: 3; banded: what the slab's rows hold)
};

// the window of a k_xf_*_win launch
struct QgXfWin {
  int j0;     // the row of blockIdx.y = 0
  int jumax;  // k_xf_atm_win: the last row that forms uekat (the row past a band is computed for its vekat alone)
  int lines;  // k_xf_lines_win: bit 0 txisat, bit 1 txinat
};

// The momentum block of a banded rank's message: XFB_HDR doubles - a0, a1 (the band, p rows of the atmosphere), own
// (bit 0 txisat, 1 txinat, 2 txisoc, 3 txinoc: the line sums this rank formed), 0, then the four sums (0.0 where not
// owned) - and six fields of nrow rows (the longest band) by nxpa columns: tauxa, tauya, uekat, vekat, wekta, wekpa from
// row a0 on, 0.0 past the band, past a field's last row (uekat, wekta: nyta) and past its last column (vekat, wekta: nxta).
#define XFB_HDR 8
#define XFB_NF 6
struct QgXfBandMsg {
  int nxpa, nxta, nypa, nyta, lda, ldta;
  int a0, a1, own, nrow;  // pack: this rank's band
  int nranks;             // scatter
  long stride;            // scatter: rank r's message starts at gath + r * stride
  double *fld[XFB_NF];    // tauxa, tauya, uekat, vekat, wekta, wekpa
  QgScalars *sca, *sco;   // (sco: the cyclic ocean's, or nullptr)
  double *msg;            // pack
  const double *gath;     // scatter
};
static inline long xfb_mom_len(int nrow, int nxpa) { return XFB_HDR + (long)XFB_NF * nrow * nxpa; }

// The message of the surface pressure: XFP_HDR doubles - g0, g1 (the global p rows the slab owns), nxpo,
// zeros - then nrow rows (the longest owned range of any rank) of nxpo columns from row g0 on, +0.0 past row g1.
#define XFP_HDR 8
struct QgXfPomMsg {
  int nxpo, nypo;      // the BASIN's p grid
  int ldo, lda;        // pitches: the slab's p grid, the assembled array
  int g0, g1, jlo;     // pack: the owned global rows and the local row of g0
  int nrow, nranks;    // (nranks: assemble)
  long stride;         // assemble: rank r's message starts at gath + r * stride
  const double *pom;   // pack: layer 1 of the slab's lagged pressure (local rows)
  double *msg;         // pack
  const double *gath;  // assemble
  double *all;         // assemble: (lda, nypo)
};
static inline long xfp_len(int nrow, int nxpo) { return XFP_HDR + (long)nrow * nxpo; }

// ---- owner-computed sums -----------------------------------------------------------------------------------------
// The edge message: XFE_HDR doubles - g0, g1 (the global p rows the slab owns), nxpo, zeros - then 2 * XFE_ROWS rows of
// nxpo columns: rows g0 .. g0 + 3, then rows g1 - 3 .. g1 (a slab owns at least 4 rows).
#define XFE_HDR 8
#define XFE_ROWS 4
struct QgXfEdgeMsg {
  int nxpo, nypo;      // the BASIN's p grid
  int ldo, lda;        // pitches: the slab's p grid, the basin-sized array
  int g0, g1, jlo;     // the owned global rows and the local row of g0
  int rank, nranks;    // assemble: the neighbours are ranks rank - 1 and rank + 1
  long stride;         // assemble: rank r's message starts at gath + r * stride
  const double *pom;   // layer 1 of the slab's lagged pressure (local rows)
  double *msg;         // pack
  const double *gath;  // assemble
  double *all;         // assemble: (lda, nypo)
};
static inline long xfe_len(int nxpo) { return XFE_HDR + 2L * XFE_ROWS * nxpo; }

// The momentum block of a rank's message in this mode: XFS_HDR doubles - f0, f1 (the fine p rows the rank owns), a0 (the
// first coarse row of the fields), own (the line sums it formed: the bits of QgXfBandMsg), then the four sums (0.0
// where not owned) - and five fields of nrow rows by nxpa columns from coarse row a0 on: tauxa, tauya, vekat (0.0 where
// the rank does not own the sampled fine row), the partial uekat line (without the factor -uvekfc) and the partial
// wekpa numerator; 0.0 past the rank's range, past a field's last row and past its last column.
#define XFS_HDR 8
#define XFS_NF 5
struct QgXfSumMsg {
  int nxpa, nxta, nypa, nyta, lda, ldta, ldf, ldtf;
  int ndxr, ndxodd, nijwid, nxtaor, nytaor, nypaor;
  int f0, f1, t0, t1, a0, a1, own, nrow; // the part: this rank's plan (t0 .. t1: the owned fine T rows)
  int nranks;                            // combine
  long stride;                           // combine: rank r's message starts at gath + r * stride
  const double *txf, *tyf, *wf;          // the part
  double *tauxa, *tauya, *uekat, *vekat, *wekpa; // combine
  double uvekfc;
  QgScalars *sca, *sco;                  // (sco: the cyclic ocean's, or nullptr)
  double *msg;                           // the part
  const double *gath;                    // combine
};
static inline long xfs_mom_len(int nrow, int nxpa) { return XFS_HDR + (long)XFS_NF * nrow * nxpa; }

struct QgXfHeatSlabParams {
  QgXfHeatParams h;   // nyto and the tables: the GLOBAL ocean's; sstm, fnetoc, ldto: the slab's local T rows
  int joff, nytl;     // local T row (1-based) = global T row - joff; nytl local T rows
  int jT0, jT1;       // owned local T rows
  double *msg;        // (4, ncell)
};

// The kernels: only where k_xforc_slab.hip asks for them (qgcm_hip.hip includes this file for the parameter structs).
#ifdef QG_XFORC_SLAB_KERNELS
// grid: (ceil(nx/256), nyl).  The expressions of k_wekpo; row jo (local) is global row jg = jo + joff.  The outermost
// halo row towards a neighbour has no T row beyond it: left as it is (no kernel reads wekpo there).
__global__ __launch_bounds__(XFS_NT) void k_xf_wekpo_slab(const QgXfSlabParams P) {
  const int io = blockIdx.x * blockDim.x + threadIdx.x + 1, jo = blockIdx.y + 1;
  const int nx = P.nx, nxt = P.nxt, nytl = P.nyl - 1, jg = jo + P.joff;
  if (io > nx || jo > P.nyl) return;
  auto W = [&](int i, int j) { return P.wekto[(long)(j - 1) * P.ldt + (i - 1)]; };
  const bool cyc = P.cyc != 0;
  int ic = io;
  if (cyc && io == nx) ic = 1; // wekpo(nxpo, j) = wekpo(1, j)
  double v;
  if (jg >= 2 && jg <= P.nyg - 1) {
    if (jo < 2 || jo > nytl) return; // seam halo row
    if (ic == 1) v = cyc ? 0.25 * (W(nxt, jo - 1) + W(nxt, jo) + W(1, jo - 1) + W(1, jo)) : 0.5 * (W(1, jo - 1) + W(1, jo));
    else if (ic == nx) v = 0.5 * (W(nxt, jo - 1) + W(nxt, jo));
    else v = 0.25 * (W(ic - 1, jo - 1) + W(ic - 1, jo) + W(ic, jo - 1) + W(ic, jo));
  } else {
    const int jt = (jg == 1) ? 1 : nytl; // (global row 1 is local row 1; global row nyg is local row nyl)
    if (ic == 1) v = cyc ? 0.5 * (W(nxt, jt) + W(1, jt)) : W(1, jt);
    else if (ic == nx) v = W(nxt, jt);
    else v = 0.5 * (W(ic - 1, jt) + W(ic, jt));
  }
  P.wekpo[(long)(jo - 1) * P.ldx + (io - 1)] = v;
}

// One workgroup of 256: sums 2 and 3 of k_xf_lines (tauxo rows 1 + 2 and nypo-1 + nypo of the GLOBAL ocean), thread-strided
// along the row, wave butterfly, waves left to right.  P.lines: which of the two; the other's rows are not read.
__global__ __launch_bounds__(XFS_NT) void k_xf_lines_oc_slab(const QgXfSlabParams P) {
  __shared__ double red[2][XFS_NT / 64];
  const int tid = threadIdx.x;
  double s[2] = {0.0, 0.0};
  for (int i = 1 + tid; i <= P.nx; i += XFS_NT) {
    const double w = (i == 1 || i == P.nx) ? 0.5 : 1.0;
    const double *c = P.txf + (long)P.jocoff * P.ldf + (P.iocoff + i - 1); // fine row of ocean row 1
    if (P.lines & 1) {
      const double a0 = P.raoro * c[0], a1 = P.raoro * c[P.ldf];
      s[0] += w * (a0 + a1);
    }
    if (P.lines & 2) {
      const double b0 = P.raoro * c[(long)(P.nyg - 2) * P.ldf], b1 = P.raoro * c[(long)(P.nyg - 1) * P.ldf];
      s[1] += w * (b0 + b1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int v = 0; v < 2; ++v) s[v] += __shfl_xor(s[v], off);
  if ((tid & 63) == 0)
#pragma unroll
    for (int v = 0; v < 2; ++v) red[v][tid >> 6] = s[v];
  __syncthreads();
  if (tid == 0) {
    double t[2];
    for (int v = 0; v < 2; ++v) {
      t[v] = 0.0;
      for (int w = 0; w < XFS_NT / 64; ++w) t[v] += red[v][w];
    }
    if (P.lines & 1) P.sco->txisoc = 0.5 * P.dxo * t[0];
    if (P.lines & 2) P.sco->txinoc = 0.5 * P.dxo * t[1];
  }
}

// grid: (nxaooc, nyaooc), block 64: one wave per atmosphere cell above the ocean
__global__ __launch_bounds__(64) void k_xf_heat_oc_slab(const QgXfHeatSlabParams S) {
  const QgXfHeatParams &P = S.h;
  const int ca = blockIdx.x, cb = blockIdx.y, lane = threadIdx.x, ndxr = P.ndxr;
  const long lda = P.ldta;
  double s[4] = {0.0, 0.0, 0.0, 0.0}; // the owned points' part of the cell's fnetat sum, arocsm, slhfsm, oradsm
  for (int p = lane; p < ndxr * ndxr; p += 64) {
    const int io = ca * ndxr + p % ndxr, jo = cb * ndxr + p / ndxr; // 0-based GLOBAL ocean T point
    const int jl = jo + 1 - S.joff;                                   // local T row, 1-based
    if (jl < 1 || jl > S.nytl) continue;
    const int im = P.ix[io] - 1, ip = P.ix[P.nxto + io] - 1, jm = P.iy[jo] - 1, jp = P.iy[P.nyto + jo] - 1;
    const double wmx = P.wx[io], wpx = P.wx[P.nxto + io], wmy = P.wy[jo], wpy = P.wy[P.nyto + jo];
    // bilint's four terms in its order, fmult = 1 (:985-988)
    const double asto = 1.0 * (wmx * wmy * P.astm[jm * lda + im] + wpx * wmy * P.astm[jm * lda + ip] +
                               wmx * wpy * P.astm[jp * lda + im] + wpx * wpy * P.astm[jp * lda + ip]);
    const long o = (long)(jl - 1) * P.ldto + io;
    const double sst = P.sstm[o];
    const double ocnrad = P.D0up * sst;           // :800
    const double slhf = P.xlamda * (sst - asto);  // :803
    const double atmrad = P.Dmdown * asto;        // :807
    P.fnetoc[o] = -P.fso[jo] - atmrad - ocnrad - slhf; // :810
    if (jl < S.jT0 || jl > S.jT1) continue;       // a halo row: its part of the sums is the neighbour's
    const double atmrad2 = P.dmdu * asto;         // :815, dmdu = Dmdown - Dmup
    s[0] += P.ocfrac * (ocnrad + atmrad2 + slhf); // :816-817
    s[1] += atmrad;
    s[2] += slhf;
    s[3] += ocnrad;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off);
  if (lane == 0) {
    const int c = cb * P.nxaooc + ca;
#pragma unroll
    for (int q = 0; q < 4; ++q) S.msg[q * P.ncell + c] = s[q];
  }
}

// grid: ceil(ncell/256): thread c adds the ranks' four partials of cell c in rank order; rank r's heat block (4, ncell)
// starts at gath + r * stride + off (replicated: stride 4 * ncell, off 0; banded: behind the momentum block)
__global__ __launch_bounds__(XFS_NT) void k_xf_heat_combine(const double *gath, int nranks, int ncell, long stride, long off,
                                                            double *cell, double *part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double *g = gath + off + (long)q * ncell + c;
    double s = g[0];
    for (int r = 1; r < nranks; ++r) s += g[r * stride];
    if (q == 0) cell[c] = s;
    else part[(q - 1) * ncell + c] = s;
  }
}

// ---- banded mode -------------------------------------------------------------------------------------------
// The atmosphere-side kernels on a window of rows: the text of k_xforc.h's kernels with the row of blockIdx.y = 0, the
// last uekat row and the choice of line sums taken from W.
#define XF_K(name) name##_win
#define XF_WIN_ARG , const QgXfWin W
#define XF_J0 W.j0
#define XF_JUMAX W.jumax
#define XF_SOUTH ((W.lines & 1) != 0)
#define XF_NORTH ((W.lines & 2) != 0)
#define XF_LINES_OC false
#define XF_WINDOWED 1
#include "k_xforc_rows.inc"
#undef XF_K
#undef XF_WIN_ARG
#undef XF_J0
#undef XF_JUMAX
#undef XF_SOUTH
#undef XF_NORTH
#undef XF_LINES_OC
#undef XF_WINDOWED

// field f of the message: its width, its height and its pitch in the replica
__device__ __forceinline__ void xfb_field(const QgXfBandMsg &B, int f, int &w, int &h, int &ld) {
  const bool tcol = f == 3 || f == 4, trow = f == 2 || f == 4; // vekat, wekta: nxta columns; uekat, wekta: nyta rows
  w = tcol ? B.nxta : B.nxpa;
  h = trow ? B.nyta : B.nypa;
  ld = tcol ? B.ldta : B.lda;
}

// grid: (ceil(nxpa/256), nrow, XFB_NF): message row jr of field f = the replica's row a0 + jr, or 0.0
__global__ __launch_bounds__(XFS_NT) void k_xf_band_pack(const QgXfBandMsg B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y, f = blockIdx.z;
  if (i == 0 && jr == 0 && f == 0) {
    double *h = B.msg;
    h[0] = (double)B.a0; h[1] = (double)B.a1; h[2] = (double)B.own; h[3] = 0.0;
    h[4] = (B.own & 1) ? B.sca->txisoc : 0.0;
    h[5] = (B.own & 2) ? B.sca->txinoc : 0.0;
    h[6] = (B.own & 4) ? B.sco->txisoc : 0.0;
    h[7] = (B.own & 8) ? B.sco->txinoc : 0.0;
  }
  if (i >= B.nxpa) return;
  int w, h, ld;
  xfb_field(B, f, w, h, ld);
  const int ja = B.a0 + jr;
  double v = 0.0;
  if (ja <= B.a1 && ja <= h && i < w) v = B.fld[f][(long)(ja - 1) * ld + i];
  B.msg[XFB_HDR + ((long)f * B.nrow + jr) * B.nxpa + i] = v;
}

// grid: (ceil(nxpa/256), nrow, XFB_NF * nranks): rank r's message row jr of field f -> the replica's row a0(r) + jr.  The
// bands tile the rows, so every point has one writer; a header that does not describe a band inside the grid writes nothing.
__global__ __launch_bounds__(XFS_NT) void k_xf_band_scatter(const QgXfBandMsg B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y, r = blockIdx.z / XFB_NF, f = blockIdx.z % XFB_NF;
  const double *m = B.gath + (long)r * B.stride;
  const int a0 = (int)m[0], a1 = (int)m[1], own = (int)m[2];
  if (a0 < 1 || a1 > B.nypa || a1 < a0 || a1 - a0 + 1 > B.nrow) return;
  if (i == 0 && jr == 0 && f == 0) {
    if (own & 1) B.sca->txisoc = m[4];
    if (own & 2) B.sca->txinoc = m[5];
    if (B.sco && (own & 4)) B.sco->txisoc = m[6];
    if (B.sco && (own & 8)) B.sco->txinoc = m[7];
  }
  int w, h, ld;
  xfb_field(B, f, w, h, ld);
  const int ja = a0 + jr;
  if (i >= w || ja > a1 || ja > h) return;
  B.fld[f][(long)(ja - 1) * ld + i] = m[XFB_HDR + ((long)f * B.nrow + jr) * B.nxpa + i];
}

// ---- tau_udiff ---------------------------------------------------------------------------------------------
// grid: (ceil(nxpo/256), nrow): message row jr = the slab's owned row g0 + jr (local row jlo + jr), or +0.0 past g1.  Halo
// rows are never read.  Consecutive lanes, consecutive doubles on both sides.
__global__ __launch_bounds__(XFS_NT) void k_xf_pom_pack(const QgXfPomMsg M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y;
  if (i == 0 && jr == 0) {
    double *h = M.msg;
    h[0] = (double)M.g0; h[1] = (double)M.g1; h[2] = (double)M.nxpo;
#pragma unroll
    for (int k = 3; k < XFP_HDR; ++k) h[k] = 0.0;
  }
  if (i >= M.nxpo) return;
  double v = 0.0;
  if (M.g0 + jr <= M.g1) v = M.pom[(long)(M.jlo - 1 + jr) * M.ldo + i];
  M.msg[XFP_HDR + (long)jr * M.nxpo + i] = v;
}

// grid: (ceil(nxpo/256), nrow, nranks): rank r's message row jr -> row g0(r) + jr of the assembled array.  The owned
// ranges tile 1 .. nypo, so every point has one writer; a header that does not describe rows inside the basin (or
// another row length) writes nothing.
__global__ __launch_bounds__(XFS_NT) void k_xf_pom_assemble(const QgXfPomMsg M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y, r = blockIdx.z;
  const double *m = M.gath + (long)r * M.stride;
  const int g0 = (int)m[0], g1 = (int)m[1], nx = (int)m[2];
  if (g0 < 1 || g1 > M.nypo || g1 < g0 || g1 - g0 + 1 > M.nrow || nx != M.nxpo) return;
  const int g = g0 + jr;
  if (i >= M.nxpo || g > g1) return;
  M.all[(long)(g - 1) * M.lda + i] = m[XFP_HDR + (long)jr * M.nxpo + i];
}
// ---- owner-computed sums -----------------------------------------------------------------------------------------
// grid: (ceil(nxpo/256), 2 * XFE_ROWS): message row jr = owned row g0 + jr (jr < 4) or g1 - 7 + jr.  Halo rows are never
// read.  Consecutive lanes, consecutive doubles on both sides.
__global__ __launch_bounds__(XFS_NT) void k_xf_edge_pack(const QgXfEdgeMsg M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y;
  if (i == 0 && jr == 0) {
    double *h = M.msg;
    h[0] = (double)M.g0; h[1] = (double)M.g1; h[2] = (double)M.nxpo;
#pragma unroll
    for (int k = 3; k < XFE_HDR; ++k) h[k] = 0.0;
  }
  if (i >= M.nxpo) return;
  const int g = jr < XFE_ROWS ? M.g0 + jr : M.g1 - (2 * XFE_ROWS - 1) + jr;
  M.msg[XFE_HDR + (long)jr * M.nxpo + i] = M.pom[(long)(M.jlo - 1 + g - M.g0) * M.ldo + i];
}

// grid: (ceil(nxpo/256), own + 2 * XFE_ROWS), own = g1 - g0 + 1: rows jr < own copy the slab's owned row g0 + jr; the next
// four are rows g0 - 4 .. g0 - 1 from the last four rows of rank - 1's message, the last four rows g1 + 1 .. g1 + 4 from
// the first four of rank + 1's.  One writer per point.  A neighbour's header that does not describe at least 4 rows
// inside 1 .. nypo that end (begin) at this slab's seam, or another row length, writes nothing.
__global__ __launch_bounds__(XFS_NT) void k_xf_edge_assemble(const QgXfEdgeMsg M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, jr = blockIdx.y, own = M.g1 - M.g0 + 1;
  if (i >= M.nxpo) return;
  if (jr < own) {
    M.all[(long)(M.g0 + jr - 1) * M.lda + i] = M.pom[(long)(M.jlo - 1 + jr) * M.ldo + i];
    return;
  }
  const int k = jr - own;
  const bool south = k < XFE_ROWS;
  const int r = south ? M.rank - 1 : M.rank + 1;
  if (r < 0 || r >= M.nranks) return;
  const double *m = M.gath + (long)r * M.stride;
  const int h0 = (int)m[0], h1 = (int)m[1], nx = (int)m[2];
  if (h0 < 1 || h1 > M.nypo || h1 - h0 + 1 < XFE_ROWS || nx != M.nxpo) return;
  if (south ? h1 != M.g0 - 1 : h0 != M.g1 + 1) return;
  const int g = south ? M.g0 - XFE_ROWS + k : M.g1 + 1 + (k - XFE_ROWS); // (inside h0 .. h1, hence inside the basin)
  const int mr = south ? XFE_ROWS + k : k - XFE_ROWS;
  M.all[(long)(g - 1) * M.lda + i] = m[XFE_HDR + (long)mr * M.nxpo + i];
}

// grid: (ceil(nxpa/256), nrow): coarse row ja = a0 + jr.  k_xf_atm's expressions and order; the line's terms k = 0 .. ndxr
// (fine rows joff + k, end weights 0.5) restricted to the owned fine rows f0 .. f1, ascending, the first term starting
// the sum.  A line inside f0 .. f1 is k_xf_atm's sum.
__global__ __launch_bounds__(XFS_NT) void k_xf_sums_atm(const QgXfSumMsg B) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, jr = blockIdx.y, ja = B.a0 + jr;
  if (ia == 1 && jr == 0) {
    double *h = B.msg;
    h[0] = (double)B.f0; h[1] = (double)B.f1; h[2] = (double)B.a0; h[3] = (double)B.own;
    h[4] = (B.own & 1) ? B.sca->txisoc : 0.0;
    h[5] = (B.own & 2) ? B.sca->txinoc : 0.0;
    h[6] = (B.own & 4) ? B.sco->txisoc : 0.0;
    h[7] = (B.own & 8) ? B.sco->txinoc : 0.0;
  }
  if (ia > B.nxpa) return;
  const int ndxr = B.ndxr, ldf = B.ldf;
  double tx = 0.0, ty = 0.0, ve = 0.0, up = 0.0;
  if (ja <= B.a1 && ja <= B.nypa) {
    const int joff = 1 + (ja - 1) * ndxr;
    if (joff >= B.f0 && joff <= B.f1) { // the sampled fine row is this rank's
      const long o = (long)(joff - 1) * ldf + (long)(ia - 1) * ndxr;
      tx = B.txf[o];
      ty = B.tyf[o];
      if (ia <= B.nxta) {
        const double *t = B.txf + o;
        double s = 0.5 * t[0];
        for (int i = 1; i < ndxr; ++i) s = s + t[i];
        s = s + 0.5 * t[ndxr];
        ve = B.uvekfc * s;
      }
    }
    if (ja <= B.nyta) {
      const int k0 = B.f0 - joff > 0 ? B.f0 - joff : 0, k1 = B.f1 - joff < ndxr ? B.f1 - joff : ndxr;
      if (k0 <= k1) {
        const int ic = (ia == B.nxpa) ? 1 : ia;
        const double *t = B.tyf + (long)(joff - 1) * ldf + (long)(ic - 1) * ndxr;
        auto term = [&](int k) { const double v = t[(long)k * ldf]; return (k == 0 || k == ndxr) ? 0.5 * v : v; };
        double s = term(k0);
        for (int k = k0 + 1; k <= k1; ++k) s = s + term(k);
        up = s;
      }
    }
  }
  double *f = B.msg + XFS_HDR + (long)jr * B.nxpa + (ia - 1);
  const long nf = (long)B.nrow * B.nxpa;
  f[0] = tx; f[nf] = ty; f[2 * nf] = ve; f[3 * nf] = up;
}

// grid: (ceil(nxpa/64), nrow), block 64: k_xf_wekpa's loops on the rows of the box that lie in the owned fine T rows
// t0 .. t1; wsum does not depend on the data and is the combine's.
__global__ __launch_bounds__(64) void k_xf_sums_wekpa(const QgXfSumMsg B) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, jr = blockIdx.y, ja = B.a0 + jr;
  if (ia > B.nxpa) return;
  const int ndxr = B.ndxr, nijwid = B.nijwid, nxtaor = B.nxtaor;
  auto wt = [&](int d) { return B.ndxodd ? ((d == 0 || d == ndxr) ? 0.5 : 1.0) : (d == ndxr ? 0.0 : 1.0); };
  double wtasum = 0.0;
  if (ja <= B.a1 && ja <= B.nypa) {
    const int jbeg = (ja - 1) * ndxr - (ndxr - 1) / 2;
    int jlo = jbeg > 1 ? jbeg : 1;
    int jhi = (jbeg + nijwid - 1 < B.nytaor) ? jbeg + nijwid - 1 : B.nytaor;
    if (jlo < B.t0) jlo = B.t0;
    if (jhi > B.t1) jhi = B.t1;
    const int ibeg = (ia - 1) * ndxr - (ndxr - 1) / 2;
    for (int j = jlo; j <= jhi; ++j) {
      const double wtj = wt(j - jbeg);
      const double *row = B.wf + (long)(j - 1) * B.ldtf;
      for (int d0 = 0; d0 < nijwid; d0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          int it = ibeg + d0 + u - 1; // 0-based cyclic column
          it = it < 0 ? it + nxtaor : (it >= nxtaor ? it - nxtaor : it);
          v[u] = d0 + u < nijwid ? row[it] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (d0 + u < nijwid) {
            const double w = wt(d0 + u) * wtj;
            wtasum = wtasum + w * v[u];
          }
      }
    }
  }
  B.msg[XFS_HDR + ((long)4 * B.nrow + jr) * B.nxpa + (ia - 1)] = wtasum;
}

// grid: (ceil(nxpa/256), nypa): thread (ia, ja) reads the ranks' messages in rank order.  Whether rank r holds the sample
// of row ja, terms of its uekat line or rows of its wekpa box is read from r's f0, f1; a header that does not describe
// fine rows inside 1 .. nypaor, or whose fields do not hold row ja, contributes nothing.  Every output point has one
// writer: this thread.
__global__ __launch_bounds__(XFS_NT) void k_xf_sums_combine(const QgXfSumMsg B) {
  const int ia = blockIdx.x * blockDim.x + threadIdx.x + 1, ja = blockIdx.y + 1;
  if (ia == 1 && ja == 1)
    for (int r = 0; r < B.nranks; ++r) {
      const double *m = B.gath + (long)r * B.stride;
      const int f0 = (int)m[0], f1 = (int)m[1], own = (int)m[3];
      if (f0 < 1 || f1 > B.nypaor || f1 < f0) continue;
      if (own & 1) B.sca->txisoc = m[4];
      if (own & 2) B.sca->txinoc = m[5];
      if (B.sco && (own & 4)) B.sco->txisoc = m[6];
      if (B.sco && (own & 8)) B.sco->txinoc = m[7];
    }
  if (ia > B.nxpa) return;
  const int ndxr = B.ndxr, nijwid = B.nijwid;
  const int joff = 1 + (ja - 1) * ndxr;
  const int jbeg = (ja - 1) * ndxr - (ndxr - 1) / 2;
  const int jlo = jbeg > 1 ? jbeg : 1;
  const int jhi = (jbeg + nijwid - 1 < B.nytaor) ? jbeg + nijwid - 1 : B.nytaor;
  const long nf = (long)B.nrow * B.nxpa;
  double us = 0.0, wp = 0.0;
  bool hu = false, hw = false;
  for (int r = 0; r < B.nranks; ++r) {
    const double *m = B.gath + (long)r * B.stride;
    const int f0 = (int)m[0], f1 = (int)m[1], a0 = (int)m[2];
    if (f0 < 1 || f1 > B.nypaor || f1 < f0) continue;
    const int jr = ja - a0;
    if (a0 < 1 || jr < 0 || jr >= B.nrow) continue;
    const int t1 = f1 < B.nytaor ? f1 : B.nytaor;
    const double *f = m + XFS_HDR + (long)jr * B.nxpa + (ia - 1);
    if (joff >= f0 && joff <= f1) {
      B.tauxa[(long)(ja - 1) * B.lda + (ia - 1)] = f[0];
      B.tauya[(long)(ja - 1) * B.lda + (ia - 1)] = f[nf];
      if (ia <= B.nxta) B.vekat[(long)(ja - 1) * B.ldta + (ia - 1)] = f[2 * nf];
    }
    if (ja <= B.nyta && joff <= f1 && joff + ndxr >= f0) {
      const double v = f[3 * nf];
      us = hu ? us + v : v;
      hu = true;
    }
    if (jlo <= t1 && jhi >= f0) {
      const double v = f[4 * nf];
      wp = hw ? wp + v : v;
      hw = true;
    }
  }
  if (hu) B.uekat[(long)(ja - 1) * B.lda + (ia - 1)] = -B.uvekfc * us;
  if (hw) {
    auto wt = [&](int d) { return B.ndxodd ? ((d == 0 || d == ndxr) ? 0.5 : 1.0) : (d == ndxr ? 0.0 : 1.0); };
    double wsum = 0.0; // k_xf_wekpa's own sum, term for term
    for (int j = jlo; j <= jhi; ++j) {
      const double wtj = wt(j - jbeg);
      for (int d = 0; d < nijwid; ++d) {
        const double w = wt(d) * wtj;
        wsum = wsum + w;
      }
    }
    B.wekpa[(long)(ja - 1) * B.lda + (ia - 1)] = wp / wsum;
  }
}
#endif // QG_XFORC_SLAB_KERNELS
