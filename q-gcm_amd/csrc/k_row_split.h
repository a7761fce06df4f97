// k_row_split.h - cyclic rows longer than one LDS buffer (nxto > 5104: SOcn 4 km .. 1 km), DESIGN 3.5c.
//
// A real row of length N = P * L is transformed as P interleaved sub-rows of length L <= 5104, x_p[n] = x[p + P n].
// The sub-rows are transformed by the row kernels the library has (k_rfft_cyc on the scratch array, seen as P * nrows
// rows of length L); what is new is the radix-P pass through HBM in front of them (inverse) or behind them (forward),
// and the two copies.  W_N = exp(-2 pi i / N) comes from the table qgcm_hip_set_grid builds for length N.
//
//   forward (drfftf):  Y_p = rfft_L(x_p);  X[k] = sum_p W_N^{p k} Y_p[k mod L], k = 0 .. N/2, where Y_p[j] for
//                      j > L/2 is conj(Y_p[L - j])
//   inverse (drfftb):  Y_p[k] = sum_{q<P} W_N^{-p (k + L q)} X[k + L q], k = 0 .. L/2, where X[j] for j > N/2 is
//                      conj(X[N - j]);  x_p = rfftb_L(Y_p)   (unnormalised, as drfftb)
//
// Rows of wrk and sub-rows of the scratch array are in FFTPACK's half-complex order
//   r(1) = X_0, r(2k) = Re X_k, r(2k+1) = Im X_k, r(n) = X_{n/2}.
// Layout of the scratch array (one array of wrk's size): sub-row p of interior row r (0-based from jr0) of mode m at
// scr + wstride * m + (r * P + p) * L - the sub-rows of one mode are consecutive rows of pitch L, so the row kernels
// pair them as they pair rows of wrk; nrows * P * L = nrows * N <= ny * ldw = wstride, L even keeps 16-byte pairs.
//
// Four launches of (ceil(points / 256), nrows, layers) blocks of 256 threads, a thread per point or coefficient.
#pragma once
#include <hip/hip_runtime.h>

struct QgRowSplit {
  double *wrk;          // rows of the work array (in: forward physical / inverse spectral; out: the other)
  double *scr;          // the scratch array
  const double2 *twid;  // exp(-2 pi i t / N), t = 0 .. N-1
  long wstride;         // doubles between two modes, of wrk and of scr
  int ldw, jr0, nrows;  // pitch of wrk, its first interior row (1-based) and the number of interior rows
  int N, P, L;
  int layer0;
};

enum { SPLIT_GATHER = 0, SPLIT_FWD, SPLIT_INV, SPLIT_SCATTER }; // qg_launch_row_split's `which`
#define SPLIT_NT 256

// element j = 0 .. n/2 of a half-complex row of length n
__device__ __forceinline__ double2 split_hc_load(const double *r, int j, int n) {
  if (j == 0) return double2{r[0], 0.0};
  if (2 * j == n) return double2{r[n - 1], 0.0};
  return double2{r[2 * j - 1], r[2 * j]};
}
__device__ __forceinline__ void split_hc_store(double *r, int j, int n, double2 v) {
  if (j == 0) r[0] = v.x;
  else if (2 * j == n) r[n - 1] = v.x;
  else {
    r[2 * j - 1] = v.x;
    r[2 * j] = v.y;
  }
}

// x_p[n] = x[p + P n]: rows of wrk -> sub-rows of scr (GATHER), and back (SCATTER)
template <int P, bool SCATTER>
__global__ __launch_bounds__(SPLIT_NT) void k_split_copy(const QgRowSplit S) {
  const int i = blockIdx.x * SPLIT_NT + threadIdx.x, r = blockIdx.y;
  if (i >= S.N || r >= S.nrows) return;
  const long mo = S.wstride * (blockIdx.z + S.layer0);
  double *row = S.wrk + mo + (long)(S.jr0 - 1 + r) * S.ldw;
  double *sub = S.scr + mo + ((long)r * P + i % P) * S.L;
  if (SCATTER) row[i] = sub[i / P];
  else sub[i / P] = row[i];
}

// forward: the sub-rows' spectra in scr -> the row's spectrum in wrk
template <int P>
__global__ __launch_bounds__(SPLIT_NT) void k_split_fwd(const QgRowSplit S) {
  const int k = blockIdx.x * SPLIT_NT + threadIdx.x, r = blockIdx.y;
  const int N = S.N, L = S.L;
  if (2 * k > N || r >= S.nrows) return;
  const long mo = S.wstride * (blockIdx.z + S.layer0);
  const double *sub = S.scr + mo + (long)r * P * L;
  const int k0 = k % L;
  const bool cj = 2 * k0 > L;
  const int j = cj ? L - k0 : k0;
  double2 acc = split_hc_load(sub, j, L);
  if (cj) acc.y = -acc.y;
#pragma unroll
  for (int p = 1; p < P; ++p) {
    double2 y = split_hc_load(sub + (long)p * L, j, L);
    if (cj) y.y = -y.y;
    const double2 w = S.twid[(int)(((long)p * k) % N)];
    acc.x += w.x * y.x - w.y * y.y;
    acc.y += w.x * y.y + w.y * y.x;
  }
  split_hc_store(S.wrk + mo + (long)(S.jr0 - 1 + r) * S.ldw, k, N, acc);
}

// inverse: the row's spectrum in wrk -> the sub-rows' spectra in scr
template <int P>
__global__ __launch_bounds__(SPLIT_NT) void k_split_inv(const QgRowSplit S) {
  const int k = blockIdx.x * SPLIT_NT + threadIdx.x, r = blockIdx.y;
  const int N = S.N, L = S.L;
  if (2 * k > L || r >= S.nrows) return;
  const long mo = S.wstride * (blockIdx.z + S.layer0);
  const double *row = S.wrk + mo + (long)(S.jr0 - 1 + r) * S.ldw;
  double *sub = S.scr + mo + (long)r * P * L;
  double2 x[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int j = k + L * q; // < N
    const bool cj = 2 * j > N;
    x[q] = split_hc_load(row, cj ? N - j : j, N);
    if (cj) x[q].y = -x[q].y;
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double2 acc = x[0];
    if (p > 0) {
      const double2 w = S.twid[(int)(((long)p * k) % N)]; // times conj(w): W_N^{-p k}
      acc = double2{w.x * x[0].x + w.y * x[0].y, w.x * x[0].y - w.y * x[0].x};
    }
#pragma unroll
    for (int q = 1; q < P; ++q) {
      const double2 w = S.twid[(int)(((long)p * (k + L * q)) % N)];
      acc.x += w.x * x[q].x + w.y * x[q].y;
      acc.y += w.x * x[q].y - w.y * x[q].x;
    }
    split_hc_store(sub + (long)p * L, k, L, acc);
  }
}
