// k_misc.h - constraint solve, mode->layer unpack, boundary PV, LF averaging.
#pragma once
#include "qgcm_dev.h"
#include "qg_ref_expr.h" // the inversion epilogue, the halo-message layout

#define CS_NT 256

// ---------------------------------------------------------------------------
// K5+K6 (box): area integrals of the inhomogeneous solutions + mass
// constraints.  Reference: xintp per mode (src/ocisubs.F:160, src/intsubs.f:
// 78-133; boundary values of wrk are zero so the trapezoid weights reduce to
// the plain interior sum delivered per row by the inverse DST kernel), then
// dpioc update, rhs and the (nlo-1)x(nlo-1) solve with DGETRS + DGERFS
// (src/ocisubs.F:333-370).  One workgroup; fixed-order tree reduction, so
// the result is deterministic (the reference's OpenMP reduction is not).
// ---------------------------------------------------------------------------
__device__ inline void qg_lu_solve(int n, const double *lu, const int *piv, double *b) {
  for (int k = 0; k < n; ++k)
    if (piv[k] != k) {
      double t = b[k];
      b[k] = b[piv[k]];
      b[piv[k]] = t;
    }
  for (int k = 0; k < n; ++k)
    for (int i = k + 1; i < n; ++i) b[i] -= lu[i + n * k] * b[k];
  for (int k = n - 1; k >= 0; --k) {
    b[k] /= lu[k + n * k];
    for (int i = 0; i < k; ++i) b[i] -= lu[i + n * k] * b[k];
  }
}

__device__ inline double qg_block_sum(double v, double *red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int off = CS_NT / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  double r = red[0];
  __syncthreads();
  return r;
}

// Area integrals of the NL inhomogeneous solutions, xin(m) = dxo*dyo * sum_k wcot(k)*ksum(m,k), by ONE wave (every
// lane returns the same values): only odd wavenumbers (even 0-based index) contribute; four independent partial
// sums per lane keep four loads in flight (2400 terms per mode at 1 km); fixed order (s0 + s1) + (s2 + s3), then a
// butterfly - deterministic, unlike the reference's OpenMP reduction.
template <int NL, class PT>
__device__ __forceinline__ void constr_xin(const PT &P, int lane, double *xin) {
  double s[NL];
  double s4[4][NL];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int m = 0; m < NL; ++m) s4[u][m] = 0.0;
  for (int k0 = 2 * lane; k0 < P.g.nk; k0 += 512) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 128 * u;
      const double wk = k < P.g.nk ? P.wcot[k] : 0.0;
#pragma unroll
      for (int m = 0; m < NL; ++m) s4[u][m] += wk * (k < P.g.nk ? P.ksum[(long)m * P.g.ldw + k] : 0.0);
    }
  }
#pragma unroll
  for (int m = 0; m < NL; ++m) s[m] = (s4[0][m] + s4[1][m]) + (s4[2][m] + s4[3][m]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int m = 0; m < NL; ++m) s[m] += __shfl_xor(s[m], off);
  }
#pragma unroll
  for (int m = 0; m < NL; ++m) xin[m] = s[m] * P.dxo * P.dyo;
}

// Leapfrog update of the mass-constraint integrals, src/ocisubs.F:343-347 (aient = xon(1) across the first
// interface only). One thread.
template <int NL>
__device__ __forceinline__ void constr_dpi_update(QgScalars *sc, double tdto, const double *gpoc) {
#pragma unroll
  for (int k = 0; k < NL - 1; ++k) {
    double aient = (k == 0) ? sc->xon[0] : 0.0;
    double aitmp = sc->dpioc[k];
    sc->dpioc[k] = sc->dpiocp[k] - tdto * gpoc[k] * aient;
    sc->dpiocp[k] = aitmp;
  }
}

// rhs(k) = dpioc(k) - sum_m cdiffo(m,k)*xin(m) and the (nlo-1)x(nlo-1) solve with DGETRS + one DGERFS-style
// refinement loop (src/ocisubs.F:349-370), host-side LU factors; dpn = the NEW dpioc.  -> hclco(1..nlo-1) in x.
template <int NL, class PT>
__device__ __forceinline__ void constr_box_solve(const PT &P, const double *xin, const double *dpn, double *x) {
  constexpr int n1 = NL - 1;
  double rhs[n1], r[n1], w[n1];
#pragma unroll
  for (int k = 0; k < n1; ++k) {
    double rhsum = 0.0;
#pragma unroll
    for (int m = 0; m < NL; ++m) rhsum = rhsum + P.cs.cdiffo[m + NL * k] * xin[m];
    rhs[k] = dpn[k] - rhsum;
    x[k] = rhs[k];
  }
  // LU solve (DGETRS) with the host-side factors; pivots applied as selects
  auto lu_solve = [&](double *b) {
#pragma unroll
    for (int k = 0; k < n1; ++k) {
      const int pk = P.cs.ipiv[k];
#pragma unroll
      for (int i = 0; i < n1; ++i)
        if (i > k && i == pk) {
          double t = b[k];
          b[k] = b[i];
          b[i] = t;
        }
    }
#pragma unroll
    for (int k = 0; k < n1; ++k)
#pragma unroll
      for (int i = k + 1; i < n1; ++i) b[i] -= P.cs.cdhlu[i + n1 * k] * b[k];
#pragma unroll
    for (int k = n1 - 1; k >= 0; --k) {
      b[k] /= P.cs.cdhlu[k + n1 * k];
#pragma unroll
      for (int i = 0; i < k; ++i) b[i] -= P.cs.cdhlu[i + n1 * k] * b[k];
    }
  };
  lu_solve(x);
  // iterative refinement with DGERFS's stopping rule (ITMAX = 5)
  const double eps = 1.1102230246251565e-16, safmin = 2.2250738585072014e-308;
  const double safe1 = (n1 + 1) * safmin, safe2 = safe1 / eps;
  double lstres = 3.0;
  for (int count = 1;; ++count) {
#pragma unroll
    for (int i = 0; i < n1; ++i) {
      double sv = rhs[i], t = fabs(rhs[i]);
#pragma unroll
      for (int j = 0; j < n1; ++j) {
        sv -= P.cs.cdhoc[i + n1 * j] * x[j];
        t += fabs(P.cs.cdhoc[i + n1 * j]) * fabs(x[j]);
      }
      r[i] = sv;
      w[i] = t;
    }
    double berr = 0.0;
#pragma unroll
    for (int i = 0; i < n1; ++i) {
      double v = (w[i] > safe2) ? fabs(r[i]) / w[i] : (fabs(r[i]) + safe1) / (w[i] + safe1);
      if (v > berr) berr = v;
    }
    if (berr > eps && 2.0 * berr <= lstres && count <= 5) {
      lu_solve(r);
#pragma unroll
      for (int i = 0; i < n1; ++i) x[i] += r[i];
      lstres = berr;
    } else
      break;
  }
}

// area integrals only (homsol on y-slabs: qgcm_hip_area_integrals)
template <int NL>
__global__ __launch_bounds__(64) void k_xin_only(const QgConstrParams P) {
  double xin[NL];
  constr_xin<NL>(P, threadIdx.x, xin);
  if (threadIdx.x == 0)
#pragma unroll
    for (int m = 0; m < NL; ++m) P.sc->xinhom[m] = xin[m];
}

__global__ __launch_bounds__(256) void k_fill_rows(double *w, long wstride, int ldw, int nk, int j0, int j1, int nl, double v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y, m = blockIdx.z;
  if (c < nk && j <= j1 && m < nl) w[wstride * m + (long)(j - 1) * ldw + c] = v;
}

// One wavefront; NL is a template parameter so that every small array lives in
// registers (run-time indexed locals would go to scratch memory and turn this
// latency-bound kernel several times slower).  Inside qgcm_hip_steps the box ocean does without this launch:
// the same functions run in k_tend (dpioc update) and in every workgroup of k_dst64_unpack<.., CONSTR>.
template <int NL>
__device__ __forceinline__ void constr_box_all(const QgConstrParams &P, int lane) {
  constexpr int n1 = NL - 1;
  double xin[NL];
  constr_xin<NL>(P, lane, xin);
  if (lane != 0) return;
  QgScalars *sc = P.sc;
#pragma unroll
  for (int m = 0; m < NL; ++m) sc->xinhom[m] = xin[m];
  constr_dpi_update<NL>(sc, P.tdto, P.gpoc);
  double dpn[n1], x[n1];
#pragma unroll
  for (int k = 0; k < n1; ++k) dpn[k] = sc->dpioc[k];
  constr_box_solve<NL>(P, xin, dpn, x);
#pragma unroll
  for (int k = 0; k < n1; ++k) sc->hclco[k] = x[k];
}

// (rows of other sizes than 64*M: the same body rides as one extra workgroup of the inverse-row launch, k_dst_box)
template <int NL>
__global__ __launch_bounds__(64) void k_constr_box(const QgConstrParams P) {
  constr_box_all<NL>(P, threadIdx.x);
}

// ---------------------------------------------------------------------------
// K7: add homogeneous solutions, modes -> layers (src/ocisubs.F:377-401).
// The reference also copies po -> pom here; the p buffers rotate instead, so
// the new po is written over the old pom and the names are swapped by the host.
// Traffic: read wrk (nl) + ochom (nl-1), write po (nl).
// ---------------------------------------------------------------------------
template <int NL>
__device__ __forceinline__ void unpack_point(const QgUnpackParams &P, int gi, int gj, double *pl) {
  const int nx = P.g.nx;
  const long o = (long)(gj - 1) * P.g.ldx + (gi - 1);
  const int G = gj + P.g.joff; // global row
  const bool inner = (gi >= 2 && gi <= nx - 1 && G >= 2 && G <= P.g.nyg - 1);
  const long ow = (long)(gj - 1) * P.g.ldw + (gi - 2);
  double pm[NL];
  pm[0] = inner ? P.wrk[ow] : 0.0;
#pragma unroll
  for (int m = 1; m < NL; ++m) {
    double wv = inner ? P.wrk[P.g.wstride * m + ow] : 0.0;
    pm[m] = qg_hom_box(wv, P.sc->hclco[m - 1], P.ochom[P.g.fstride * (m - 1) + o]);
  }
#pragma unroll
  for (int k = 0; k < NL; ++k) pl[k] = qg_modes_to_layer<NL>(P.ctm2l, k, pm);
}

// BDY = true additionally writes the boundary PV of the new pressure (ocqbdy,
// src/vorsubs.F:245-388) from the same threads: qgcm_hip_steps uses it to save
// a launch; the stand-alone entry points keep unpack and ocqbdy separate.
template <int NL, bool BDY>
__global__ __launch_bounds__(256) void k_unpack_box(const QgUnpackParams P, const QgBdyParams B) {
  const int nx = P.g.nx;
  const int gi0 = blockIdx.x * blockDim.x + threadIdx.x + 1;
  const int gj = P.g.jlo + blockIdx.y; // owned local row
  if (gj > P.g.jhi) return;
  const bool valid = gi0 <= nx;
  const int gi = valid ? gi0 : nx; // (lanes past the row keep the wave whole for the pair stores; they write nothing)
  const int G = gj + P.g.joff, nyg = P.g.nyg;
  const long o = (long)(gj - 1) * P.g.ldx + (gi0 - 1);
  double pl[NL];
  unpack_point<NL>(P, gi, gj, pl);
#pragma unroll
  for (int k = 0; k < NL; ++k) qg_pair_store_wt(P.pnew + P.g.fstride * k + o, pl[k], valid); // (qgcm_dev.h)
  if (!valid) return;
  // y-slab halo messages (QG_HALO_P / QG_HALO_Q, qg_ref_expr.h), written here when the host passes the buffers (slab stage 2): the
  // first / last three owned rows of the new pressure, and below the edge row of q
  const bool qlo = BDY && P.msg_lo && gj == P.g.jlo, qhi = BDY && P.msg_hi && gj == P.g.jhi;
  if (BDY && P.msg_lo && gj - P.g.jlo < 3) {
#pragma unroll
    for (int k = 0; k < NL; ++k) P.msg_lo[QG_HALO_P(k, gj - P.g.jlo, P.g.ldx) + (gi - 1)] = pl[k];
  }
  if (BDY && P.msg_hi && P.g.jhi - gj < 3) {
#pragma unroll
    for (int k = 0; k < NL; ++k) P.msg_hi[QG_HALO_P(k, gj - (P.g.jhi - 2), P.g.ldx) + (gi - 1)] = pl[k];
  }
  if (BDY) {
    const bool ns = (G == 1 || G == nyg);
    const bool we = (gi == 1 || gi == nx);
    if ((qlo || qhi) && !(ns || we)) { // interior columns of the q row: set by k_tend
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const double q = B.qo[P.g.fstride * k + o];
        if (qlo) P.msg_lo[QG_HALO_Q(NL, k, P.g.ldx) + (gi - 1)] = q;
        if (qhi) P.msg_hi[QG_HALO_Q(NL, k, P.g.ldx) + (gi - 1)] = q;
      }
    }
    if (ns || we) {
      const int ii = ns ? gi : (gi == 1 ? 2 : nx - 1);
      const int jj = ns ? (G == 1 ? gj + 1 : gj - 1) : gj;
      double pin[NL];
      unpack_point<NL>(P, ii, jj, pin);
      const double by = B.beta * B.yporel[gj - 1];
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const double ap = QG_AP(B.f0A, NL, k, pl[k - 1], pl[k], pl[k + 1]);
        double q = qg_bdy_q(B.bcfaco_f0, pin[k], pl[k], ap, by);
        if (k == QG_TOPO_LAYER(false, NL)) q = q + B.ddynoc[o]; // (a box is an ocean)
        B.qo[P.g.fstride * k + o] = q;
        if (qlo) P.msg_lo[QG_HALO_Q(NL, k, P.g.ldx) + (gi - 1)] = q;
        if (qhi) P.msg_hi[QG_HALO_Q(NL, k, P.g.ldx) + (gi - 1)] = q;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K8: PV on the solid boundaries from the new pressure (src/vorsubs.F:245-388)
// grid: x covers max(nx,ny) points; blockIdx.y = side (0 S, 1 N, 2 W, 3 E); z = layer
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ocqbdy(const QgBdyParams P) {
  const int nx = P.g.nx, ny = P.g.ny, nl = P.g.nl, ldx = P.g.ldx;
  const long fs = P.g.fstride;
  const int t = blockIdx.x * blockDim.x + threadIdx.x + 1;
  const int side = blockIdx.y;
  const int k = blockIdx.z;
  int gi, gj, ii, jj; // boundary point, its inward neighbour
  if (side < 2) {
    if (t > nx) return;
    gi = t; ii = t;
    // only the rank that owns the global boundary row does it
    if (side == 0 && P.g.jlo + P.g.joff != 1) return;
    if (side == 1 && P.g.jhi + P.g.joff != P.g.nyg) return;
    gj = (side == 0) ? P.g.jlo : P.g.jhi;
    jj = (side == 0) ? gj + 1 : gj - 1;
  } else {
    if (P.g.cyc) return;
    if (t < P.g.jlo || t > P.g.jhi) return;
    if (t + P.g.joff < 2 || t + P.g.joff > P.g.nyg - 1) return;
    gj = t; jj = t;
    gi = (side == 2) ? 1 : nx;
    ii = (side == 2) ? 2 : nx - 1;
  }
  const long ob = (long)(gj - 1) * ldx + (gi - 1);
  const long oi = (long)(jj - 1) * ldx + (ii - 1);
  const double *po = P.po;
  double pb = po[fs * k + ob];
  double ap = QG_AP(P.f0A, nl, k, po[fs * (k - 1) + ob], pb, po[fs * (k + 1) + ob]);
  if (P.g.atm && k == nl - 1 && side == 0) ap = QG_AP_ATQZBD(P.f0A, nl, k, po[fs * (k - 1) + ob], po[fs * k + oi]);
  double q = qg_bdy_q(P.bcfaco_f0, po[fs * k + oi], pb, ap, P.beta * P.yporel[gj - 1]);
  if (k == QG_TOPO_LAYER(P.g.atm, nl)) q = q + P.ddynoc[ob];
  P.qo[fs * k + ob] = q;
}

// ---------------------------------------------------------------------------
// K9: leapfrog time-level averaging (src/q-gcm.F:1328-1366, ocean part)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lf_average(double *qo, const double *qom, double *po, const double *pom,
                                                     long n, QgScalars *sc, int nl, int cyc) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    qo[i] = 0.5 * (qo[i] + qom[i]);
    po[i] = 0.5 * (po[i] + pom[i]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int k = 0; k < nl - 1; ++k) sc->dpioc[k] = 0.5 * (sc->dpioc[k] + sc->dpiocp[k]);
    if (cyc)
      for (int k = 0; k < nl; ++k) {
        sc->ocncs[k] = 0.5 * (sc->ocncs[k] + sc->ocncsp[k]);
        sc->ocncn[k] = 0.5 * (sc->ocncn[k] + sc->ocncnp[k]);
      }
  }
}

// the scalar part alone: the fields were averaged by the step's own kernels (QgTendParams.avg, QgUnpackParams.pavg)
__global__ void k_lf_average_scalars(QgScalars *sc, int nl, int cyc) {
  if (threadIdx.x != 0) return;
  for (int k = 0; k < nl - 1; ++k) sc->dpioc[k] = 0.5 * (sc->dpioc[k] + sc->dpiocp[k]);
  if (cyc)
    for (int k = 0; k < nl; ++k) {
      sc->ocncs[k] = 0.5 * (sc->ocncs[k] + sc->ocncsp[k]);
      sc->ocncn[k] = 0.5 * (sc->ocncn[k] + sc->ocncnp[k]);
    }
}

// ---------------------------------------------------------------------------
// y-slab halo messages: 3 rows of po and 1 row of qo per layer and direction.
// message = [k][3 rows][ldx] of p, then [k][ldx] of q (QG_HALO_P / QG_HALO_Q, qg_ref_expr.h).   grid: (ceil(ldx/256), 4*nl, 2)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_halo_pack(QgGeom g, const double *po, const double *qo, double *to_lower,
                                                   double *to_upper) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.ldx) return;
  const int rr = blockIdx.y % 4, k = blockIdx.y / 4; // rr 0..2: p rows, 3: q row
  const int dir = blockIdx.z;                        // 0: to lower neighbour, 1: to upper
  double *msg = dir == 0 ? to_lower : to_upper;
  if (!msg) return;
  if (rr < 3) {
    const int j = dir == 0 ? g.jlo + rr : g.jhi - 2 + rr;
    msg[QG_HALO_P(k, rr, g.ldx) + i] = po[g.fstride * k + (long)(j - 1) * g.ldx + i];
  } else {
    const int j = dir == 0 ? g.jlo : g.jhi;
    msg[QG_HALO_Q(g.nl, k, g.ldx) + i] = qo[g.fstride * k + (long)(j - 1) * g.ldx + i];
  }
}

__global__ __launch_bounds__(256) void k_halo_unpack(QgGeom g, double *po, double *qo, const double *from_lower,
                                                     const double *from_upper) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.ldx) return;
  const int rr = blockIdx.y % 4, k = blockIdx.y / 4;
  const int dir = blockIdx.z; // 0: message from the lower neighbour (its top rows), 1: from the upper
  const double *msg = dir == 0 ? from_lower : from_upper;
  if (!msg) return;
  if (rr < 3) {
    const int j = dir == 0 ? g.jlo - 3 + rr : g.jhi + 1 + rr;
    po[g.fstride * k + (long)(j - 1) * g.ldx + i] = msg[QG_HALO_P(k, rr, g.ldx) + i];
  } else {
    const int j = dir == 0 ? g.jlo - 1 : g.jhi + 1;
    qo[g.fstride * k + (long)(j - 1) * g.ldx + i] = msg[QG_HALO_Q(g.nl, k, g.ldx) + i];
  }
}

// empty launch: calibrates the bracket overhead of the per-kernel HIP-event timing
__global__ void k_noop() {}

// device-to-device copy probe for the "measured peak" of the roofline
// Measurement only (bench.py): a pure streaming kernel with a given read : write mix - NR fields read, NW fields
// written, 16 bytes per lane, nothing else - on buffers of the workload's field size.  What the memory system gives
// this kernel is the practical ceiling for a kernel of the same mix (profiles/tools/membw_mix.hip).
template <int NR, int NW>
__global__ __launch_bounds__(256) void k_stream_mix(const double2 *__restrict__ src, double2 *__restrict__ dst, long nper) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nper; i += stride) {
    double2 v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = src[r * nper + i];
    double2 acc = v[0];
#pragma unroll
    for (int r = 1; r < NR; ++r) acc.x += v[r].x;
#pragma unroll
    for (int w = 0; w < NW; ++w) dst[w * nper + i] = double2{acc.x + w, acc.y};
  }
}

__global__ __launch_bounds__(256) void k_copy(const double2 *__restrict__ src, double2 *__restrict__ dst, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}
