// k_cov.h - the covariance matrices of covaria_diag.F (covocn / covatm) on the device.
//
// One contribution subsamples layer 1 of p with psampl and the T field (sst / ast) with tsampl, then applies
// Algorithm AS 41 (dssp, wt = 1) to each: a mean update and a rank-1 update of the packed lower triangle
// cov(k), k = i(i+1)/2 + j (0-based, 0 <= j <= i < nvar).  Built with -ffp-contract=off, in the reference's operand
// order: bitwise the reference's numbers.  No atomics, no scratch.
//
// Row-sum form.  A sample depends on the field only through per-row sums over the columns of one block:
//   p grid (psampl):  r(is, j) = 0.5*p(id1,j) + p(id1+1,j) + .. + p(id2-1,j) + 0.5*p(id2,j),  id1 = 1+(is-1)*nsi,
//                     id2 = 1+is*nsi (the inner rows' sumi and the boundary rows' sums / sumn alike);
//                     u(ivs) = sumd + 0.5*(r(is,jd1) + r(is,jd2)),  sumd = 0 + r(is,jd1+1) + .. + r(is,jd2-1)
//   T grid (tsampl):  r(is, j) = 0 + t(id1,j) + .. + t(is*nsi,j);  u(ivs) = 0 + r(is,jd1) + .. + r(is,js*nsi)
// with ivs = (js-1)*(nx/nsi) + is.  A y-slab therefore sends the sums of its own rows ("part") and every rank forms
// the whole-domain sample from the gathered parts, bitwise the whole-domain handle's.
//
// Part layout (doubles): [0..3] = first and last global p row, first and last global T row (1-based), then the p
// rows' sums (nbx each, row by row), then the T rows' sums.  A whole-domain handle makes one part of all rows.
//
//   k_cov_rowsums   a workgroup per COV_RNT block columns of an owned p row / owned T row (staged in LDS)
//   k_cov_combine   u in the reference's order from the gathered parts (rank order, no atomics), then AS 41's mean
//                   update; writes the deviation d = u - mean (first sample: mean = u).  Fails (status word) when the
//                   parts do not tile the rows.
//   k_cov_rank1     cov(k) = cov(k) + (c*d(i))*d(j) over the packed range [k0, k1) of both matrices: pure HBM
//                   streaming, 16 B per lane per access, 64-bit indices; a lane finds the row of its first element by
//                   inverting the triangular number and walks forward across row ends.
#pragma once
#include "qgcm_dev.h"

#define COV_NT 256   // lanes per workgroup of k_cov_combine and k_cov_rank1
#define COV_U 4      // accesses of 2 elements per lane in k_cov_rank1
#define COV_TILE (2L * COV_NT * COV_U)
#define COV_HDR 4    // header doubles of a part
#define COV_RNT 64   // lanes per workgroup of k_cov_rowsums
#define COV_MAXNSI 32 // largest nsi (the row-sum kernel's LDS segment)
#define COV_MAXR 256 // ranks k_cov_combine takes (their headers are staged in LDS)

typedef double cov_d2 __attribute__((ext_vector_type(2)));

struct QgCovRowParams {
  const double *p, *t; // layer 1 of p (pitch ldx), the T field (pitch ldt); local rows
  int ldx, ldt, nsi, nbx;
  int jp0, nrp;        // first owned local p row, owned p rows
  int jt0, nrt;        // first owned local T row, owned T rows
  int joff;            // global row = local row + joff
  double *out;         // the part (header + sums)
};

struct QgCovCombParams {
  const double *gath; // nranks parts of part_len doubles, rank order
  long part_len;
  int nranks, nsi, nbx, nby, nyp, nyt;
  double *mean[2], *dev[2]; // p, T
  double b[2];              // AS 41's b = wt/sumwt of this contribution
  int first[2];             // nunit == 1: mean = u
  int *status;              // 0, or 1 + the first rank that does not continue the rows
};

struct QgCovR1Params {
  double *m[2];        // the matrices' local storage: element k at m[k - k0]
  const double *d[2];  // deviation vectors
  double c[2];         // AS 41's c = wt - b*wt
  long k0, n;          // first packed index held, elements held
};

// row i and column j of packed element k (0-based): the triangular root in double, then an exact integer correction
__device__ __host__ inline void cov_rowcol(long k, long &i, long &j) {
  long r = (long)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
  while (r > 0 && r * (r + 1) / 2 > k) --r;
  while ((r + 1) * (r + 2) / 2 <= k) ++r;
  i = r;
  j = k - r * (r + 1) / 2;
}

// a workgroup per segment of COV_RNT block columns of one row: the segment's points are staged in LDS with coalesced
// loads (several in flight per lane), then a lane sums one block column in order
__global__ __launch_bounds__(COV_RNT) void k_cov_rowsums(const QgCovRowParams P) {
  __shared__ double seg[COV_RNT * COV_MAXNSI + 1];
  const bool tgrid = (int)blockIdx.y >= P.nrp;
  const int r = tgrid ? (int)blockIdx.y - P.nrp : (int)blockIdx.y;
  const int jl = (tgrid ? P.jt0 : P.jp0) + r; // local row
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    P.out[0] = (double)(P.jp0 + P.joff);
    P.out[1] = (double)(P.jp0 + P.joff + P.nrp - 1);
    P.out[2] = (double)(P.jt0 + P.joff);
    P.out[3] = (double)(P.jt0 + P.joff + P.nrt - 1);
  }
  const int nsi = P.nsi, is0 = blockIdx.x * COV_RNT;
  const int nb = min(COV_RNT, P.nbx - is0);                 // block columns of this segment
  const int npts = nb * nsi + (tgrid ? 0 : 1);               // points it reads (p: the shared right edge too)
  const double *src = (tgrid ? P.t + (long)P.ldt * (jl - 1) : P.p + (long)P.ldx * (jl - 1)) + (long)is0 * nsi;
#pragma unroll 8
  for (int i = threadIdx.x; i < npts; i += COV_RNT) seg[i] = src[i];
  __syncthreads();
  if ((int)threadIdx.x >= nb) return;
  const double *row = seg + threadIdx.x * nsi;
  double s;
  if (tgrid) {
    s = 0.0;
    for (int i = 0; i < nsi; ++i) s = s + row[i];
  } else {
    s = 0.5 * row[0];
    for (int i = 1; i < nsi; ++i) s = s + row[i];
    s = s + 0.5 * row[nsi];
  }
  P.out[COV_HDR + (tgrid ? (long)P.nrp * P.nbx : 0) + (long)r * P.nbx + is0 + threadIdx.x] = s;
}

// the sums of global row jg (p grid: w = 0, T grid: w = 1) and block column is, found in the part that holds the row
// (hdr: the parts' first and last rows, staged in LDS by k_cov_combine)
__device__ inline double cov_r(const QgCovCombParams &P, const int (*hdr)[4], int w, int jg, int is) {
  int k = 0;
  while (k < P.nranks - 1 && jg > hdr[k][2 * w + 1]) ++k;
  const long nrp = hdr[k][1] - hdr[k][0] + 1;
  return P.gath[k * P.part_len + COV_HDR + (w ? nrp * P.nbx : 0) + (long)(jg - hdr[k][2 * w]) * P.nbx + is];
}

__global__ __launch_bounds__(COV_NT) void k_cov_combine(const QgCovCombParams P) {
  __shared__ int hdr[COV_MAXR][4];
  __shared__ int bad;
  for (int k = threadIdx.x; k < P.nranks; k += COV_NT)
    for (int q = 0; q < 4; ++q) hdr[k][q] = (int)P.gath[k * P.part_len + q];
  __syncthreads();
  if (threadIdx.x == 0) {
    // the parts must continue each other's rows in rank order and end at the last row of each grid
    int e = 0, np = 0, nt = 0;
    for (int k = 0; k < P.nranks && !e; ++k) {
      const int p0 = hdr[k][0], p1 = hdr[k][1], t0 = hdr[k][2], t1 = hdr[k][3];
      const long len = COV_HDR + ((long)(p1 - p0 + 1) + (t1 - t0 + 1)) * P.nbx;
      if (p0 != np + 1 || p1 < p0 || t0 != nt + 1 || t1 < t0 - 1 || len > P.part_len) e = k + 1;
      np = p1;
      nt = t1;
    }
    if (!e && (np != P.nyp || nt != P.nyt)) e = P.nranks;
    bad = e;
    if (blockIdx.x == 0) *P.status = e;
  }
  __syncthreads();
  if (bad) return;
  const int nvar = P.nbx * P.nby;
  const int e = blockIdx.x * COV_NT + threadIdx.x;
  if (e >= 2 * nvar) return;
  const int w = e >= nvar ? 1 : 0, v = e - w * nvar;
  const int js = v / P.nbx, is = v - js * P.nbx; // 0-based block row, column
  const int jd1 = 1 + js * P.nsi;
  double u, sumd = 0.0;
  // sumd over rows a..b in order; the row sums of four rows are requested before they are added
  auto rows = [&](int w_, int a, int b) {
    int jd = a;
    for (; jd + 3 <= b; jd += 4) {
      const double r0 = cov_r(P, hdr, w_, jd, is), r1 = cov_r(P, hdr, w_, jd + 1, is);
      const double r2 = cov_r(P, hdr, w_, jd + 2, is), r3 = cov_r(P, hdr, w_, jd + 3, is);
      sumd = sumd + r0;
      sumd = sumd + r1;
      sumd = sumd + r2;
      sumd = sumd + r3;
    }
    for (; jd <= b; ++jd) sumd = sumd + cov_r(P, hdr, w_, jd, is);
  };
  if (w == 0) {
    const double rs = cov_r(P, hdr, 0, jd1, is), rn = cov_r(P, hdr, 0, jd1 + P.nsi, is);
    rows(0, jd1 + 1, jd1 + P.nsi - 1);
    u = sumd + 0.5 * (rs + rn);
  } else {
    rows(1, jd1, jd1 + P.nsi - 1);
    u = sumd;
  }
  double *mean = P.mean[w];
  if (P.first[w]) {
    mean[v] = u;
  } else {
    const double d = u - mean[v];
    mean[v] = mean[v] + P.b[w] * d;
    P.dev[w][v] = d;
  }
}

template <bool NT>
__device__ inline cov_d2 cov_ld(const double *p) {
  if (NT) return __builtin_nontemporal_load((const cov_d2 *)p);
  return *(const cov_d2 *)p;
}
template <bool NT>
__device__ inline void cov_st(double *p, cov_d2 v) {
  if (NT) __builtin_nontemporal_store(v, (cov_d2 *)p);
  else *(cov_d2 *)p = v;
}

// Lane l of workgroup b updates elements (2l, 2l+1) + u*2*COV_NT of the tile at b*COV_TILE, u = 0..COV_U-1, in both
// matrices; the storage is allocated to an even count, so a pair load never leaves it (the element past n is stored
// back unchanged).  All COV_U pairs are loaded before the first is updated.
template <bool NT>
__global__ __launch_bounds__(COV_NT) void k_cov_rank1(const QgCovR1Params P) {
  const long base = (long)blockIdx.x * COV_TILE + 2 * (long)threadIdx.x;
  if (base >= P.n) return;
  long i, j;
  cov_rowcol(P.k0 + base, i, j);
  long ri[COV_U], rj[COV_U];
  cov_d2 a[COV_U], b[COV_U];
#pragma unroll
  for (int u = 0; u < COV_U; ++u) {
    ri[u] = i;
    rj[u] = j;
    const long loc = base + (long)u * 2 * COV_NT;
    if (loc < P.n) {
      a[u] = cov_ld<NT>(P.m[0] + loc);
      b[u] = cov_ld<NT>(P.m[1] + loc);
    }
    j += 2 * COV_NT; // walk to the element 2*COV_NT further on
    while (j > i) {
      j -= i + 1;
      ++i;
    }
  }
  const double *d0 = P.d[0], *d1 = P.d[1];
  const double c0 = P.c[0], c1 = P.c[1];
#pragma unroll
  for (int u = 0; u < COV_U; ++u) {
    const long loc = base + (long)u * 2 * COV_NT;
    if (loc >= P.n) break;
    long i0 = ri[u], j0 = rj[u];
    // xssp(k) = xssp(k) + c*x(i)*x(j): (c*x(i)) once per row, then *x(j), then the add
    a[u].x = a[u].x + (c0 * d0[i0]) * d0[j0];
    b[u].x = b[u].x + (c1 * d1[i0]) * d1[j0];
    if (loc + 1 < P.n) {
      if (++j0 > i0) {
        ++i0;
        j0 = 0;
      }
      a[u].y = a[u].y + (c0 * d0[i0]) * d0[j0];
      b[u].y = b[u].y + (c1 * d1[i0]) * d1[j0];
    }
    cov_st<NT>(P.m[0] + loc, a[u]);
    cov_st<NT>(P.m[1] + loc, b[u]);
  }
}
