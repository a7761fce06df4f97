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
// A cell wholly inside one slab keeps the bits of the whole-domain sum (x + 0.0 = x); a cell a seam cuts is a sum of the
// same terms in another order.  No atomics; every sum has a fixed tree.
#pragma once
#include "qgcm_dev.h"
#include "k_xf_heat_params.h"

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
};

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
// along the row, wave butterfly, waves left to right.
__global__ __launch_bounds__(XFS_NT) void k_xf_lines_oc_slab(const QgXfSlabParams P) {
  __shared__ double red[2][XFS_NT / 64];
  const int tid = threadIdx.x;
  double s[2] = {0.0, 0.0};
  for (int i = 1 + tid; i <= P.nx; i += XFS_NT) {
    const double w = (i == 1 || i == P.nx) ? 0.5 : 1.0;
    const double *c = P.txf + (long)P.jocoff * P.ldf + (P.iocoff + i - 1); // fine row of ocean row 1
    const double a0 = P.raoro * c[0], a1 = P.raoro * c[P.ldf];
    const double b0 = P.raoro * c[(long)(P.nyg - 2) * P.ldf], b1 = P.raoro * c[(long)(P.nyg - 1) * P.ldf];
    s[0] += w * (a0 + a1);
    s[1] += w * (b0 + b1);
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
    P.sco->txisoc = 0.5 * P.dxo * t[0];
    P.sco->txinoc = 0.5 * P.dxo * t[1];
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

// grid: ceil(ncell/256): thread c adds the ranks' four partials of cell c in rank order
__global__ __launch_bounds__(XFS_NT) void k_xf_heat_combine(const double *gath, int nranks, int ncell, double *cell, double *part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double s = gath[q * ncell + c];
    for (int r = 1; r < nranks; ++r) s += gath[((long)r * 4 + q) * ncell + c];
    if (q == 0) cell[c] = s;
    else part[(q - 1) * ncell + c] = s;
  }
}
#endif // QG_XFORC_SLAB_KERNELS
