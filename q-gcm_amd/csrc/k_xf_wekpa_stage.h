// k_xf_wekpa_stage.h - the box average of xforc's momentum half (src/xfosubs.F:446-471) for wide boxes.
//
// k_xf_wekpa (k_xforc_rows.inc) gives every atmosphere p point one thread that fetches its box of nijwid^2 fine values
// from global memory itself: at ndxr = 16 neighbouring lanes read 128 bytes apart and a box is 256 values; at ndxr = 80
// they read 640 bytes apart, a box is 6400 values and every one of them is a dependent add behind a load of its own.
// Here a workgroup of XFW_NT threads owns XFW_G zonally adjacent p points of one atmosphere row.  Per fine T row of the
// box all its threads bring the (G - 1) * ndxr + nijwid values the G boxes span into LDS with coalesced loads (the
// cyclic wrap of the column is resolved there), the row after it being requested before this row is summed; lane g of
// the first wave then adds its nijwid values from LDS.
//
// Bitwise k_xf_wekpa: the same terms in the same order (d = 0 .. nijwid - 1 inside j = jlo .. jhi), wsum from the same
// wt(d) * wt(j - jbeg) products, the same division; the build has -ffp-contract=off.
//
// LDS: two row buffers.  Column c of the span (c = 0 at lane 0's first column) sits at (c / ndxr) * pitch + c % ndxr
// with pitch = ndxr | 1, so lane g reads g * pitch + d at step d (for odd ndxr the pitch is ndxr and d = ndxr is the
// next lane's d = 0: the same formula).  An odd pitch in doubles puts the 32 lanes of a ds_read_b64 group on 32
// different bank pairs; with pitch = ndxr = 80 they would share two (80 g mod 32 takes the values 0 and 16).
#pragma once
#include "k_xforc_rows.h" // QgXfParams

#define XFW_G 32   // p points per workgroup
#define XFW_NT 256 // threads per workgroup
#define XFW_NDXR_MAX 128
static_assert(XFW_G <= 64, "the sums run on the first wave");

// doubles of one row buffer: G lanes of `pitch` and the last lane's d = ndxr of an odd ndxr
__host__ __device__ inline int xfw_row_doubles(int ndxr) { return XFW_G * (ndxr | 1) + 1; }
__host__ __device__ inline size_t xfw_lds_bytes(int ndxr) { return 2 * (size_t)xfw_row_doubles(ndxr) * sizeof(double); }
// loads per thread and row: the widest span, XFW_G full boxes
__host__ __device__ inline int xfw_loads(int ndxr) { return ((XFW_G - 1) * ndxr + ndxr + ndxr % 2 + XFW_NT - 1) / XFW_NT; }

// grid: (ceil(nxpa/XFW_G), rows), block XFW_NT, dynamic LDS xfw_lds_bytes(ndxr); row blockIdx.y is ja = ja0 + blockIdx.y.
// U >= xfw_loads(ndxr): the loads a thread keeps in flight per row (all issued, the surplus ones on the span's last column)
template <int U>
__global__ __launch_bounds__(XFW_NT) void k_xf_wekpa_stage(const QgXfParams P, const int ja0) {
  extern __shared__ double xfw_lds[];
  const int tid = threadIdx.x, ia0 = blockIdx.x * XFW_G + 1, ja = blockIdx.y + ja0;
  const int ndxr = P.ndxr, nijwid = P.nijwid, nxtaor = P.nxtaor;
  const int pitch = ndxr | 1, rowd = xfw_row_doubles(ndxr);
  const int gact = (P.nxpa - ia0 + 1 < XFW_G) ? P.nxpa - ia0 + 1 : XFW_G; // p points of this workgroup
  const int span = (gact - 1) * ndxr + nijwid;
  auto wt = [&](int d) { return P.ndxodd ? ((d == 0 || d == ndxr) ? 0.5 : 1.0) : (d == ndxr ? 0.0 : 1.0); };
  const int jbeg = (ja - 1) * ndxr - (ndxr - 1) / 2;
  const int jlo = jbeg > 1 ? jbeg : 1;
  const int jhi = (jbeg + nijwid - 1 < P.nytaor) ? jbeg + nijwid - 1 : P.nytaor;
  const int ibeg0 = (ia0 - 1) * ndxr - (ndxr - 1) / 2; // lane 0's ibeg
  // this thread's columns of the span: where they come from (0-based cyclic column) and where they go
  int src[U], dst[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = tid + u * XFW_NT;
    const int cc = c < span ? c : span - 1;
    int it = ibeg0 + cc - 1; // it = 1 + mod(i-1+nxtaor, nxtaor), 0-based
    it = it < 0 ? it + nxtaor : (it >= nxtaor ? it - nxtaor : it);
    src[u] = it;
    const int q = cc / ndxr;
    dst[u] = c < span ? q * pitch + (cc - q * ndxr) : -1;
  }
  double v[U];
  {
    const double *row = P.wf + (long)(jlo - 1) * P.ldtf;
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = row[src[u]];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (dst[u] >= 0) xfw_lds[dst[u]] = v[u];
  }
  __syncthreads();
  double wsum = 0.0, wtasum = 0.0;
  for (int j = jlo; j <= jhi; ++j) {
    const double *buf = xfw_lds + ((j - jlo) & 1) * rowd;
    if (j < jhi) { // the next row, requested under the sums of this one
      const double *row = P.wf + (long)j * P.ldtf;
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = row[src[u]];
    }
    if (tid < gact) {
      const double wtj = wt(j - jbeg);
      const double *b = buf + tid * pitch;
      for (int d = 0; d < nijwid; ++d) { // the reference's order (d = i - ibeg)
        const double w = wt(d) * wtj;
        wsum = wsum + w;
        wtasum = wtasum + w * b[d];
      }
    }
    if (j < jhi) {
      double *nxt = xfw_lds + ((j - jlo + 1) & 1) * rowd;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (dst[u] >= 0) nxt[dst[u]] = v[u];
    }
    __syncthreads();
  }
  if (tid < gact) P.wekpa[(long)(ja - 1) * P.lda + (ia0 + tid - 1)] = wtasum / wsum;
}
