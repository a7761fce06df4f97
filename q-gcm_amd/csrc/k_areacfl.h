// k_areacfl.h - the area averages (areavg) and the CFL check (cfltry) on the device.
//
// Replaces `call areavg` (src/areasubs_diag.F:50-677, cpp option get_areav) and `call cfltry` (src/q-gcm.F:2121-2440),
// the last two periodic diagnostics of the main loop that needed sst / ast and po / pa on the host.
//
// Area averages: areint's weighted sum of sst (ocean handle) or ast (atmosphere handle) over up to nine rectangles of
// T cells, all areas of the handle in one pass (they may overlap).
//   k_arav_rows   one wave per (area, owned row of the area): the lanes stride the row segment i1..i2, with facw at
//                 i1 and face at i2 (i1 == i2: both, as areint's formula gives), and end in the butterfly.
//   k_arav_part   one workgroup, one wave per area: the interior rows j1+1..j2-1 this handle owns, lane-strided in
//                 row order, then the butterfly.  FINAL (whole domain): facs / facn on rows j1 and j2 (j1 == j2: both
//                 on the one row) and the division by the denominator.  Else the summary of a y-slab: the raw sums
//                 of rows j1 and j2 (0 where another rank owns them) and the interior sum, then the owned T rows.
//   k_arav_combine  the gathered summaries, added in rank order; checks that the T rows tile 1..nyto.
// The denominator depends on the tables alone: the host forms it at set-up in areint's serial order, so it is bitwise
// the reference's.  The numerator is a sum in another order than areint's: it agrees to rounding.  No atomics, every
// order fixed: bitwise the same from call to call and on every rank.
//
// CFL check: per quantity - the mixed layer's |u|, |v|, then |u|(k), then |v|(k), 2*(nl+1) in all - the maximum, its
// first location in the reference's scan order (j outer, i inner) and the number of points whose Courant number
// (dt/dx)*|.| is >= cflcrit.  The expressions keep the reference's operand order, uncontracted; a maximum, a count
// and a first location do not depend on the order of the reduction, so all three are exact.
//   k_cfl_scan    CFL_TX x CFL_TY tiles of p points, lane = column, all layers; each point reads its +i and +j
//                 neighbours (the tile's one-point halo; on a y-slab row j+1 of the last owned row is a halo row).
//                 Per workgroup and quantity: maximum, key = (j-1)*nx + (i-1) of its first point, count.
//   k_cfl_final   one workgroup, one wave per quantity over the workgroups' partials (PART: + the owned p rows).
//   k_cfl_combine the gathered summaries: the maximum, the earliest key among equal maxima, the counts added.
// There is no cyclic special case because the reference has none.  The key is an int: grids up to 46340 x 46340.
// The point-by-point listing of a failing run (`Bad |u|; CFL, i, j, k`) stays with the host, which pulls the state
// for it as it does for valids' neighbourhood print-out.
#pragma once
#include "qgcm_dev.h"

#define ARAV_MAXN 9                        // namxoc = namxat of areasubs_diag.F
#define ARAV_PART_LEN (3 * ARAV_MAXN + 2)  // per area: row j1, row j2, interior | owned T rows t0, t1
#define ARAV_OUT_LEN (3 * ARAV_MAXN + 1)   // averages | numerators | denominators | the combine's status

struct QgAravParams {
  const double *f;  // sst / ast at the current level, T grid
  int ld;           // its pitch
  int n;            // areas
  int i1[ARAV_MAXN], i2[ARAV_MAXN], j1[ARAV_MAXN], j2[ARAV_MAXN]; // T subscripts, 1-based, global rows
  double facw[ARAV_MAXN], face[ARAV_MAXN], facs[ARAV_MAXN], facn[ARAV_MAXN], den[ARAV_MAXN];
  int t0, t1;       // the global T rows this handle owns
  int joff;         // local row = global row - joff
  int nyt;          // T rows of the whole domain
  int rowcap;       // t1 - t0 + 1
  double *rows;     // (rowcap, n): the weighted sum of owned row t0 + r of area a at a * rowcap + r
  double *out;      // ARAV_OUT_LEN (FINAL, combine) or ARAV_PART_LEN (the summary)
  const double *gath;
  int nranks;
};

__device__ __forceinline__ double arav_wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// grid (most owned rows of any area, n), 64 threads
__global__ __launch_bounds__(64) void k_arav_rows(const QgAravParams P) {
  const int a = blockIdx.y, lane = threadIdx.x;
  const int r0 = max(P.j1[a], P.t0), r1 = min(P.j2[a], P.t1);
  const int gj = r0 + blockIdx.x;
  if (gj > r1) return;
  const int i1 = P.i1[a], i2 = P.i2[a];
  const double facw = P.facw[a], face = P.face[a];
  const double *row = P.f + (long)(gj - P.joff - 1) * P.ld;
  double s = 0.0;
  for (int i = i1 + lane; i <= i2; i += 64) {
    const double v = row[i - 1];
    double t = v;
    if (i == i1) t = facw * v;
    if (i == i2) t = i == i1 ? t + face * v : face * v;
    s += t;
  }
  s = arav_wave_sum(s);
  if (lane == 0) P.rows[(long)a * P.rowcap + (gj - P.t0)] = s;
}

// one workgroup of ARAV_MAXN waves
template <bool FINAL>
__global__ __launch_bounds__(64 * ARAV_MAXN) void k_arav_part(const QgAravParams P) {
  const int a = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double *o = P.out;
  if (!FINAL && threadIdx.x == 0) {
    o[3 * ARAV_MAXN] = (double)P.t0;
    o[3 * ARAV_MAXN + 1] = (double)P.t1;
  }
  if (a >= P.n) {
    if (!FINAL && lane < 3) o[3 * a + lane] = 0.0;
    return;
  }
  const int j1 = P.j1[a], j2 = P.j2[a], t0 = P.t0, t1 = P.t1;
  const double *rows = P.rows + (long)a * P.rowcap - t0; // rows[gj]
  double s = 0.0;
  for (int gj = max(j1 + 1, t0) + lane; gj <= min(j2 - 1, t1); gj += 64) s += rows[gj];
  s = arav_wave_sum(s);
  if (lane != 0) return;
  const double south = (j1 >= t0 && j1 <= t1) ? rows[j1] : 0.0, north = (j2 >= t0 && j2 <= t1) ? rows[j2] : 0.0;
  if (FINAL) {
    const double num = P.facs[a] * south + P.facn[a] * north + s;
    o[a] = num / P.den[a];
    o[ARAV_MAXN + a] = num;
    o[2 * ARAV_MAXN + a] = P.den[a];
  } else {
    o[3 * a] = south;
    o[3 * a + 1] = north;
    o[3 * a + 2] = s;
  }
}

// nranks gathered summaries (rank r at r * ARAV_PART_LEN) -> out as k_arav_part<true> writes it, then
// out[3 * ARAV_MAXN] = status: 0, or r + 1 when rank r is the first whose T rows do not continue the tiling of
// 1..nyto (nothing else is written then).  Rank order, no atomics: every rank computes bitwise the same numbers.
__global__ __launch_bounds__(64) void k_arav_combine(const QgAravParams P) {
  const int a = threadIdx.x, R = P.nranks;
  const double *G = P.gath;
  int bad = 0, next = 1;
  for (int r = 0; r < R && !bad; ++r) {
    const double g0 = G[(long)r * ARAV_PART_LEN + 3 * ARAV_MAXN], g1 = G[(long)r * ARAV_PART_LEN + 3 * ARAV_MAXN + 1];
    if (g0 != (double)next || g1 < g0 || g1 > (double)P.nyt || (r == R - 1 && g1 != (double)P.nyt)) bad = r + 1;
    else next = (int)g1 + 1;
  }
  if (a == 0) P.out[3 * ARAV_MAXN] = (double)bad;
  if (bad || a >= P.n) return;
  double south = G[3 * a], north = G[3 * a + 1], s = G[3 * a + 2];
  for (int r = 1; r < R; ++r) {
    const double *g = G + (long)r * ARAV_PART_LEN + 3 * a;
    south += g[0];
    north += g[1];
    s += g[2];
  }
  const double num = P.facs[a] * south + P.facn[a] * north + s;
  P.out[a] = num / P.den[a];
  P.out[ARAV_MAXN + a] = num;
  P.out[2 * ARAV_MAXN + a] = P.den[a];
}

// ---------------------------------------------------------------------------
// CFL check
// ---------------------------------------------------------------------------
#define CFL_TX 64  // tile width = one wave: lane = column
#define CFL_TY 16
#define CFL_NT 256 // 4 waves, 4 rows each
#define CFL_FT 1024
#define CFL_NQ(nl) (2 * ((nl) + 1))
#define CFL_LEN(nl) (3 * CFL_NQ(nl))          // maxima | keys | counts
#define CFL_PART_LEN(nl) (CFL_LEN(nl) + 2)    // ... | owned p rows g0, g1
#define CFL_EXTREM 1.0e30                     // the reference's starting value -extrem

struct QgCflParams {
  QgGeom g;
  const double *p;       // po / pa at the current level
  const double *sx, *sy; // ocean: tauxo, tauyo (p grid, ldx); atmosphere: uekat (nxpa, nyta; ldx), vekat (nxta, nypa; ldt)
  int ldt;
  int jlo, jhi;          // owned local p rows
  int ntx, nblk;
  double rdxf0, rhf0hm, dtdx, cflcrit;
  double *part;          // (CFL_LEN(nl), nblk)
  double *out;           // CFL_LEN(nl) (+ the combine's status) or CFL_PART_LEN(nl)
  const double *gath;
  int nranks;
};

// (value, key) a replaced by b when b is larger, or as large and earlier in the scan
__device__ __forceinline__ void cfl_take(double &v, int &k, double ov, int ok) {
  if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
}

template <int NL, bool ATM>
__global__ __launch_bounds__(CFL_NT) void k_cfl_scan(const QgCflParams P) {
  constexpr int NQ = CFL_NQ(NL);
  __shared__ double rv[NQ][CFL_NT / 64];
  __shared__ int rk[NQ][CFL_NT / 64], rc[NQ][CFL_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nx = P.g.nx, nyg = P.g.nyg, ldx = P.g.ldx, joff = P.g.joff, jhi = P.jhi;
  const long fs = P.g.fstride;
  const int b = blockIdx.x, tx = b % P.ntx, ty = b / P.ntx;
  const int i = tx * CFL_TX + 1 + lane, j0 = P.jlo + ty * CFL_TY;
  const double rdx = P.rdxf0, rh = P.rhf0hm, dtdx = P.dtdx, crit = P.cflcrit;
  double mv[NQ];
  int mk[NQ], mc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) { mv[q] = -CFL_EXTREM; mk[q] = 0x7fffffff; mc[q] = 0; }
  // a thread meets its points in scan order, so a strictly larger value is the first occurrence
#define CFL_UPD(q, val)                                  \
  do {                                                   \
    const double v_ = (val);                             \
    if (v_ > mv[q]) { mv[q] = v_; mk[q] = key; }         \
    if (dtdx * v_ >= crit) ++mc[q];                      \
  } while (0)
  for (int r = wv; r < CFL_TY; r += CFL_NT / 64) {
    const int j = j0 + r, gj = j + joff;
    if (i > nx || j > jhi) continue;
    const long o = (long)(j - 1) * ldx + (i - 1);
    const int key = (gj - 1) * nx + (i - 1);
    const bool hu = gj <= nyg - 1, hv = i <= nx - 1; // |u|: j = 1..ny-1, i = 1..nx; |v|: j = 1..ny, i = 1..nx-1
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const double *pk = P.p + fs * k;
      const double p = pk[o];
      if (hu) {
        const double d = pk[o + ldx] - p;
        CFL_UPD(2 + k, fabs(-rdx * d));
        if (k == 0) {
          if (ATM) CFL_UPD(0, fabs(-rdx * d + P.sx[o]));
          else CFL_UPD(0, fabs(-rdx * d + rh * (P.sy[o + ldx] + P.sy[o])));
        }
      }
      if (hv) {
        const double d = pk[o + 1] - p;
        CFL_UPD(2 + NL + k, fabs(rdx * d));
        if (k == 0) {
          if (ATM) CFL_UPD(1, fabs(rdx * d + P.sy[(long)(j - 1) * P.ldt + (i - 1)]));
          else CFL_UPD(1, fabs(rdx * d - rh * (P.sx[o + 1] + P.sx[o])));
        }
      }
    }
  }
#undef CFL_UPD
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      cfl_take(mv[q], mk[q], __shfl_xor(mv[q], off), __shfl_xor(mk[q], off));
      mc[q] += __shfl_xor(mc[q], off);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) { rv[q][wv] = mv[q]; rk[q][wv] = mk[q]; rc[q][wv] = mc[q]; }
  }
  __syncthreads();
  if (tid < NQ) {
    double v = rv[tid][0];
    int k = rk[tid][0], c = rc[tid][0];
    for (int w = 1; w < CFL_NT / 64; ++w) {
      cfl_take(v, k, rv[tid][w], rk[tid][w]);
      c += rc[tid][w];
    }
    const int nblk = P.nblk;
    P.part[(long)tid * nblk + b] = v;
    P.part[(long)(NQ + tid) * nblk + b] = (double)k;
    P.part[(long)(2 * NQ + tid) * nblk + b] = (double)c;
  }
}

// one workgroup: wave per quantity over the workgroups' partials; PART: the summary of a y-slab
template <bool PART>
__global__ __launch_bounds__(CFL_FT) void k_cfl_final(const QgCflParams P) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nq = CFL_NQ(P.g.nl), nblk = P.nblk;
  for (int q = wv; q < nq; q += CFL_FT / 64) {
    const double *pv = P.part + (long)q * nblk, *pk = P.part + (long)(nq + q) * nblk, *pc = P.part + (long)(2 * nq + q) * nblk;
    double v = -CFL_EXTREM, c = 0.0;
    int k = 0x7fffffff;
    for (int bb = lane; bb < nblk; bb += 64) {
      cfl_take(v, k, pv[bb], (int)pk[bb]);
      c += pc[bb]; // (whole numbers below 2^53: exact in any order)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      cfl_take(v, k, __shfl_xor(v, off), __shfl_xor(k, off));
      c += __shfl_xor(c, off);
    }
    if (lane == 0) {
      P.out[q] = v;
      P.out[nq + q] = (double)k;
      P.out[2 * nq + q] = c;
    }
  }
  if (PART && tid == 0) {
    P.out[3 * nq] = (double)(P.jlo + P.g.joff);
    P.out[3 * nq + 1] = (double)(P.jhi + P.g.joff);
  }
}

// nranks gathered summaries (rank r at r * CFL_PART_LEN) -> out as k_cfl_final<false> writes it, then
// out[CFL_LEN] = status: 0, or r + 1 when rank r is the first whose rows do not continue the tiling of 1..nypo
__global__ __launch_bounds__(64) void k_cfl_combine(const QgCflParams P) {
  const int q = threadIdx.x, R = P.nranks, nq = CFL_NQ(P.g.nl), L = 3 * nq + 2;
  const double *G = P.gath;
  int bad = 0, next = 1;
  for (int r = 0; r < R && !bad; ++r) {
    const double g0 = G[(long)r * L + L - 2], g1 = G[(long)r * L + L - 1];
    if (g0 != (double)next || g1 < g0 || g1 > (double)P.g.nyg || (r == R - 1 && g1 != (double)P.g.nyg)) bad = r + 1;
    else next = (int)g1 + 1;
  }
  if (q == 0) P.out[3 * nq] = (double)bad;
  if (bad || q >= nq) return;
  double v = G[q], c = G[2 * nq + q];
  int k = (int)G[nq + q];
  for (int r = 1; r < R; ++r) {
    const double *g = G + (long)r * L;
    cfl_take(v, k, g[q], (int)g[nq + q]);
    c += g[2 * nq + q];
  }
  P.out[q] = v;
  P.out[nq + q] = (double)k;
  P.out[2 * nq + q] = c;
}
