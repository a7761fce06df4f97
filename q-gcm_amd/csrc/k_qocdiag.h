// k_qocdiag.h - the ocean's periodic dumps on the device.
//
// Two routines the reference calls at every mod(ntdone,noutoc) == 0 and that otherwise need the whole state on the host:
//   * qocdiag_out (src/qocdiag.F:303-687): the vorticity budget of the step about to be taken - dqdt, the Arakawa
//     Jacobian qotjac, the Del-4th / Del-6th viscous terms qt2dif / qt4dif and the Ekman / entrainment / bottom-drag
//     term qotent - at the subsampled points (1+(i-1)*nsko, 1+(j-1)*nsko) of every layer;
//   * ocnc_out (src/nc_subs.F:837-1072): sst, po, qo, wekto, the interface displacement h, tauxo and tauyo at the
//     same subsampled points (T-grid fields on the T grid's own subsample).
//
//   k_qocdiag      one p point per lane in QD_TX x QD_TY tiles, one layer per grid z.  Del-sqd(pom) of the tile + a
//                  2-point halo goes to LDS (read from pom, which the tile's neighbours share through L2), then
//                  Del-4th of the tile + a 1-point halo, then Del-6th and the terms at the tile's points.  Only the
//                  subsampled points are stored; tiles without one return at once.
//   k_ocnc_sample  copies (or, for h, differences) of subsampled points, one plane per grid z.
//
// Every expression and its operand order is qocdiag_out's (built with -ffp-contract=off): bitwise the reference's
// numbers.  Boundary rules, verbatim, on GLOBAL rows (gj = j + joff): the bcfaco forms of del2p / del4p on rows 1 and
// nypo, and in the box on columns 1 and nxpo; there every term is zero and dqdt = rdto*(qo - qom).  Cyclic: the wrap
// of column 1 through nxpo-1 and column nxpo a copy of column 1.  In the cyclic case every column is evaluated at its
// canonical column c in 1..nxpo-1 (period nxpo-1): the reference's del2p / del4p / terms at nxpo are copies of those
// at 1, and the one quantity that is not - del2p(nxpo, 1 / nypo), from column nxpo's own pom - feeds only del4p(nxpo,
// 1 / nypo), which no output reads.
// No atomics, no scratch.  On a y-slab the owned rows are computed: Del-6th at owned row j reads pom on rows j-3 ..
// j+3, po / qo on rows j-1 .. j+1: the three halo rows that k_monslab_scan relies on.
#pragma once
#include "qgcm_dev.h"
#include "qg_ref_expr.h" // what qocdiag_out shares with qgostep: the five-point sum, the wall rule, the Jacobian

#define QD_TX 64 // tile width = one wave: lane = column
#define QD_TY 16
#define QD_NT 256 // 4 waves, 4 rows each
#define QD_NTERM 5 // dqdt, qotjac, qt2dif, qt4dif, qotent

struct QgQocdiagParams {
  QgGeom g;
  const double *pom, *po, *qo, *qom, *wekpo, *entoc; // p grid, ldx pitch
  double *out;                                       // [QD_NTERM][nl][jpn][ipwk]
  int nsko, ipwk, jpn, m0;                           // subsample: columns, rows of out, global subsample row of out's first
  int ntx;                                           // tiles along x
  int jlo, jhi;                                      // owned local rows
  double adfaco, bcfaco, dxom2, rdto, bdrfac;        // src/qocdiag.F:369-376
  double fohfac[2];                                  // fnot/hoc(1), fnot/hoc(2)
  double ah2fac[QG_MAXL], ah4fac[QG_MAXL];           // ah2oc(k)/fnot, ah4oc(k)/fnot
};

// canonical column of global column gi: the box's own (0 off the grid), or the cyclic image in 1..nx-1
template <bool CYC>
__device__ __forceinline__ int qd_col(int gi, int nx) {
  if (CYC) {
    const int n = nx - 1;
    return ((gi - 1) % n + n) % n + 1;
  }
  return (gi >= 1 && gi <= nx) ? gi : 0;
}

template <bool CYC>
__global__ __launch_bounds__(QD_NT) void k_qocdiag(const QgQocdiagParams P) {
  constexpr int W2 = QD_TX + 4, H2 = QD_TY + 4, W4 = QD_TX + 2, H4 = QD_TY + 2;
  __shared__ double d2[H2][W2], d4[H4][W4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nx = P.g.nx, ny = P.g.nyg, ldx = P.g.ldx, joff = P.g.joff, nsko = P.nsko;
  const int k = blockIdx.z, nl = P.g.nl;
  const long fs = P.g.fstride;
  const int tx = blockIdx.x % P.ntx, ty = blockIdx.x / P.ntx;
  const int i0 = tx * QD_TX + 1, j0 = P.jlo + ty * QD_TY; // first column (global), first row (local)
  // (uniform) nothing to store in this tile: no subsampled column or no owned subsampled row
  {
    const int ci = ((i0 - 1 + nsko - 1) / nsko) * nsko + 1;
    const int g0 = j0 + joff, g1 = min(j0 + QD_TY - 1, P.jhi) + joff;
    const int cj = ((g0 - 1 + nsko - 1) / nsko) * nsko + 1;
    if (ci > min(i0 + QD_TX - 1, nx) || cj > g1) return;
  }
  const double *pmk = P.pom + fs * k, *pk = P.po + fs * k, *qk = P.qo + fs * k;
  const double bcfaco = P.bcfaco, dxom2 = P.dxom2;
#define QD_AT(A, i, j) (A)[(long)((j) - 1) * ldx + ((i) - 1)]

  // Del-sqd(pom) at global columns i0-2 .. i0+QD_TX+1, local rows j0-2 .. j0+QD_TY+1 (src/qocdiag.F:405-438)
  for (int t = tid; t < W2 * H2; t += QD_NT) {
    const int a = t % W2, b = t / W2;
    const int c = qd_col<CYC>(i0 - 2 + a, nx), lj = j0 - 2 + b, gj = lj + joff;
    double v = 0.0;
    if (c >= 1 && gj >= 1 && gj <= ny && lj >= P.jlo - 2 && lj <= P.jhi + 2) {
      if (gj == 1) v = QG_WALL_RULE(bcfaco, QD_AT(pmk, c, lj + 1), QD_AT(pmk, c, lj));
      else if (gj == ny) v = QG_WALL_RULE(bcfaco, QD_AT(pmk, c, lj - 1), QD_AT(pmk, c, lj));
      else if (!CYC && c == 1) v = QG_WALL_RULE(bcfaco, QD_AT(pmk, 2, lj), QD_AT(pmk, 1, lj));
      else if (!CYC && c == nx) v = QG_WALL_RULE(bcfaco, QD_AT(pmk, nx - 1, lj), QD_AT(pmk, nx, lj));
      else {
        const int il = (CYC && c == 1) ? nx - 1 : c - 1;
        v = QG_FIVE_POINT(QD_AT(pmk, c, lj - 1), QD_AT(pmk, il, lj), QD_AT(pmk, c + 1, lj), QD_AT(pmk, c, lj + 1), QD_AT(pmk, c, lj)) * dxom2;
      }
    }
    d2[b][a] = v;
  }
  __syncthreads();
  // Del-4th at global columns i0-1 .. i0+QD_TX, local rows j0-1 .. j0+QD_TY (src/qocdiag.F:443-477); d2 centre (b+1, a+1)
  for (int t = tid; t < W4 * H4; t += QD_NT) {
    const int a = t % W4, b = t / W4;
    const int c = qd_col<CYC>(i0 - 1 + a, nx), lj = j0 - 1 + b, gj = lj + joff;
    double v = 0.0;
    if (c >= 1 && gj >= 1 && gj <= ny && lj >= P.jlo - 1 && lj <= P.jhi + 1) {
      const int A = a + 1, B = b + 1;
      if (gj == 1) v = QG_WALL_RULE(bcfaco, d2[B + 1][A], d2[B][A]);
      else if (gj == ny) v = QG_WALL_RULE(bcfaco, d2[B - 1][A], d2[B][A]);
      else if (!CYC && c == 1) v = QG_WALL_RULE(bcfaco, d2[B][A + 1], d2[B][A]);
      else if (!CYC && c == nx) v = QG_WALL_RULE(bcfaco, d2[B][A - 1], d2[B][A]);
      else v = QG_FIVE_POINT(d2[B - 1][A], d2[B][A - 1], d2[B][A + 1], d2[B + 1][A], d2[B][A]) * dxom2;
    }
    d4[b][a] = v;
  }
  __syncthreads();

  // the terms at the tile's subsampled points (src/qocdiag.F:479-606)
  const int gi = i0 + lane;
  if (gi > nx || (gi - 1) % nsko != 0) return;
  const int c = CYC ? qd_col<true>(gi, nx) : gi;
  const int il = (CYC && c == 1) ? nx - 1 : c - 1, ir = c + 1;
  const long plane = (long)P.jpn * P.ipwk;
  double *o = P.out + (long)k * plane + (gi - 1) / nsko;
  const long tstride = plane * nl;
  for (int r = wv; r < QD_TY; r += QD_NT / 64) {
    const int j = j0 + r, gj = j + joff;
    if (j > P.jhi || (gj - 1) % nsko != 0) continue;
    double dqdt, jac = 0.0, qt2 = 0.0, qt4 = 0.0, ent = 0.0;
    if (gj == 1 || gj == ny || (!CYC && (gi == 1 || gi == nx))) {
      dqdt = P.rdto * (QD_AT(qk, gi, j) - QD_AT(P.qom + fs * k, gi, j));
    } else {
      const int A = lane + 1, B = r + 1; // d4 centre; d2 centre (B + 1, A + 1)
      const double d6p = dxom2 * QG_FIVE_POINT(d4[B - 1][A], d4[B][A - 1], d4[B][A + 1], d4[B + 1][A], d4[B][A]);
      qt2 = P.ah2fac[k] * d4[B][A];
      qt4 = -(P.ah4fac[k] * d6p);
      jac = P.adfaco * QG_JAC_TAIL(
                QG_JAC_HEAD(QD_AT(qk, c, j - 1), QD_AT(qk, il, j), QD_AT(qk, ir, j), QD_AT(qk, c, j + 1),
                            QD_AT(pk, c, j - 1), QD_AT(pk, il, j), QD_AT(pk, ir, j), QD_AT(pk, c, j + 1),
                            QD_AT(pk, il, j - 1), QD_AT(pk, ir, j - 1), QD_AT(pk, il, j + 1), QD_AT(pk, ir, j + 1)),
                QD_AT(pk, c, j - 1), QD_AT(pk, il, j), QD_AT(pk, ir, j), QD_AT(pk, c, j + 1),
                QD_AT(qk, il, j - 1), QD_AT(qk, ir, j - 1), QD_AT(qk, il, j + 1), QD_AT(qk, ir, j + 1));
      if (k == 0) ent = P.fohfac[0] * (QD_AT(P.wekpo, c, j) - QD_AT(P.entoc, c, j));
      else if (k == 1) ent = P.fohfac[1] * QD_AT(P.entoc, c, j);
      else ent = 0.0;
      if (k == nl - 1) ent = ent - P.bdrfac * d2[B + 1][A + 1];
      dqdt = jac + qt2 + qt4 + ent;
    }
    const long row = (long)((gj - 1) / nsko - P.m0) * P.ipwk;
    o[row] = dqdt;
    o[tstride + row] = jac;
    o[2 * tstride + row] = qt2;
    o[3 * tstride + row] = qt4;
    o[4 * tstride + row] = ent;
  }
#undef QD_AT
}

// ocnc_out's subsample: plane z of out (ni x nj, i fastest) = src[z] at columns 1, 1+nsko, .. and local rows
// lj0, lj0+nsko, ..; with src2 (the interface displacement h) rg[z]*(src2[z] - src[z]), src/nc_subs.F:1021-1023
#define QD_SMP_MAXP QG_MAXL
struct QgSampleParams {
  const double *src[QD_SMP_MAXP], *src2[QD_SMP_MAXP];
  double rg[QD_SMP_MAXP];
  double *out;
  int ld, ni, nj, nsko, lj0;
};

__global__ __launch_bounds__(256) void k_ocnc_sample(const QgSampleParams P) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, z = blockIdx.z;
  if (i >= P.ni) return;
  const long o = (long)(P.lj0 - 1 + j * P.nsko) * P.ld + (long)i * P.nsko;
  const double v = P.src2[z] ? P.rg[z] * (P.src2[z][o] - P.src[z][o]) : P.src[z][o];
  P.out[((long)z * P.nj + j) * P.ni + i] = v;
}
