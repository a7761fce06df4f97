// k_monitors.h - the ocean half of the monitoring diagnostics on the device.
//
// Replaces the ocean half of `call monnc_comp` (src/monitor_diag.F:479-832, with poref :173-182, del4bx :899-1020,
// del4ch :1026-1151, genint :1155-1209) and `call couroc` (:1450-1928).  On the host these need po, pom, qo every
// dgnday and ~30 passes per layer over them; here 19*nlo + 16 doubles come back (layout: include/qgcm_hip.h).
//   k_mon_scan   one pass over the p grid in MON_TX x MON_TY tiles, all layers.  Per layer the lagged geostrophic
//                velocities ugoc / vgoc of the tile + a 3-point halo go to LDS, then Del-sqd of them (2-point halo),
//                then Del-4th at the tile's points, with the one-sided boundary forms of del4bx or the periodic wrap
//                of del4ch.  Each workgroup writes its partial genint sums (edge weights facwe / facsn of the p, T
//                and mixed grids) and its partial minima (maxima as minima of the negated values, exact).
//   k_mon_jet    the zonal sums of ugeos behind the jet position ujeto, row by row in the reference's serial order.
//   k_mon_final  one workgroup: reduces the partials in a fixed order, the arg-max over the rows and the scalar
//                arithmetic of monnc_comp (ocnorm, rhooc, cpoc, Sverdrups, occtot) and couroc.
// No atomics: every sum has a fixed association order, so the result is bitwise the same from call to call.  The
// extrema (po, sst, couroc's velocities and Courant numbers), ocjpos and ocjval use the reference's expressions,
// uncontracted (-ffp-contract=off), and min / max do not depend on the order: against the golden values of the
// reference build (tests/golden/mon_*.npz) they are bitwise equal.  The genint integrals are sums in another order
// than the host's: they agree to rounding.
#pragma once
#include "qgcm_dev.h"

#define MON_TX 64           // tile width = one wave: lane = column
#define MON_TY 16
#define MON_NT 256          // 4 waves, 4 rows each
#define MON_FT 1024         // threads of k_mon_final (one wave per reduced quantity)
#define MON_NQ 13           // sums per batch (per layer; then the layer-independent ones)
#define MON_NMN 7           // minima per batch
#define MON_NS(nl) (MON_NQ * ((nl) + 1))
#define MON_NM(nl) (MON_NMN * ((nl) + 1))
#define MON_LEN(nl) (19 * (nl) + 16)
// per-rank summary of a y-slab (qgcm_hip_monitors_part; layout: include/qgcm_hip.h)
#define MON_PART_LEN(nl) (MON_NS(nl) + MON_NM(nl) + 4 * (nl) + 2)

// sums of layer k at MON_NQ*k + ...
enum { MS_P = 0, MS_Q, MS_U2D, MS_U4D, MS_UKE, MS_UKEDOT, MS_V2D, MS_V4D, MS_VKE, MS_VKEDOT, MS_ETA, MS_ETA2, MS_ETADOT };
// layer-independent sums at MON_NQ*nl + ...
enum { MS_WEKT = 0, MS_AWEKT, MS_WEKP, MS_AWEKP, MS_ENT, MS_AENT, MS_UTAUX, MS_VTAUY, MS_SSTWEK, MS_SST, MS_UBOT, MS_VBOT, MS_ETAENT };
// minima of layer k at MON_NMN*k + ...: pomin, -pomax, ugmin, -ugmax, vgmin, -vgmax, -vsqmax;
// layer-independent at MON_NMN*nl + ...: sstmin, -sstmax, ummin, -ummax, vmmin, -vmmax, -vsqmax (mixed layer)

struct QgMonParams {
  QgGeom g;
  const double *po, *pom, *qo, *wekpo, *entoc; // p grid, ldx pitch
  const double *taux, *tauy;                   // p grid, ldx pitch
  const double *wekto, *sst;                   // T grid, ldt pitch
  int ldt;
  int ntx, nblk;                               // tiles along x, tiles in all
  int jlo, jhi, njet;                          // owned local p rows; owned T rows (jet rows) = jlo .. jlo + njet - 1
  int sb, nb;                                  // the cpp options sb_hflux / nb_hflux of couroc's mixed layer
  double rdxof0, dxom2, hdxom1, dto, uvgfac, rhf0hm;
  double rgpoc[QG_MAXL];
  double ocnorm, rhooc, cpoc, fnot, delek;
  double hoc[QG_MAXL], gpoc[QG_MAXL], ah2oc[QG_MAXL], ah4oc[QG_MAXL];
  double *psum;  // (MON_NS, nblk)
  double *pmin;  // (MON_NM, nblk)
  double *ujet;  // (njet, nl): ujeto of every owned T row of every layer (k_mon_jet -> k_mon_final / k_monslab_part)
  double *out;   // MON_LEN(nl) (k_mon_final, k_monslab_combine; then the combine's status) or MON_PART_LEN(nl) (k_monslab_part)
  const double *gath; // k_monslab_combine: nranks summaries of MON_PART_LEN(nl), rank-major
  int nranks;
};

__device__ __forceinline__ int mon_wrap(int i, int n) { return ((i - 1) % n + n) % n + 1; }

// Del-sqd of a field tabulated on (N, M) at LDS position (a, b) = global point (gi, gj): the forms of del4bx
// (one-sided differences on the four edges) or, CYC, of del4ch (periodic in x; the halo holds periodic images).
template <bool CYC, int W>
__device__ __forceinline__ double mon_lap(const double (*A)[W], int a, int b, int gi, int gj, int N, int M, double f) {
  if (gj < 1 || gj > M || (!CYC && (gi < 1 || gi > N))) return 0.0;
  const bool yin = gj > 1 && gj < M;
  if (yin && (CYC || (gi > 1 && gi < N))) return f * (A[b - 1][a] + A[b][a - 1] + A[b][a + 1] + A[b + 1][a] - 4.0 * A[b][a]);
  double s;
  if (!CYC && gi == 1) s = A[b][a + 2] - 2.0 * A[b][a + 1] + A[b][a];
  else if (!CYC && gi == N) s = A[b][a] - 2.0 * A[b][a - 1] + A[b][a - 2];
  else s = A[b][a - 1] - 2.0 * A[b][a] + A[b][a + 1];
  if (gj == 1) s = s + A[b + 2][a] - 2.0 * A[b + 1][a] + A[b][a];
  else if (gj == M) s = s + A[b][a] - 2.0 * A[b - 1][a] + A[b - 2][a];
  else s = s + A[b - 1][a] - 2.0 * A[b][a] + A[b + 1][a];
  return f * s;
}

__device__ __forceinline__ double mon_min(double a, double b) { return b < a ? b : a; }

// a uniform value kept in a VGPR: k_mon_scan's scalar registers are full (kernel arguments, layer pointers); the
// slab's two row bounds as SGPRs spill them to scratch
__device__ __forceinline__ int mon_in_vgpr(int x) {
  int v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
  return v;
}

// one batch of MON_NQ sums + MON_NMN minima: wave butterfly, then the four waves left to right; partials of block b
__device__ __forceinline__ void mon_flush(double *s, double *m, double (*red)[MON_NT / 64], double *psum, double *pmin,
                                          int s0, int m0, int nblk, int b) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) s[q] += __shfl_xor(s[q], off);
#pragma unroll
    for (int q = 0; q < MON_NMN; ++q) m[q] = mon_min(m[q], __shfl_xor(m[q], off));
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) red[q][tid >> 6] = s[q];
#pragma unroll
    for (int q = 0; q < MON_NMN; ++q) red[MON_NQ + q][tid >> 6] = m[q];
  }
  __syncthreads();
  if (tid < MON_NQ) {
    double t = red[tid][0];
    for (int w = 1; w < MON_NT / 64; ++w) t += red[tid][w];
    psum[(long)(s0 + tid) * nblk + b] = t;
  } else if (tid < MON_NQ + MON_NMN) {
    double t = red[tid][0];
    for (int w = 1; w < MON_NT / 64; ++w) t = mon_min(t, red[tid][w]);
    pmin[(long)(m0 + tid - MON_NQ) * nblk + b] = t;
  }
  __syncthreads();
}

// SLAB: the owned rows of a y-slab (local rows jlo..jhi); else the whole domain (the same code with joff = 0, rows 1..ny)
template <int NL, bool CYC, bool SLAB>
__device__ __forceinline__ void mon_scan(const QgMonParams &P) {
  constexpr int UW = MON_TX + 6, UH = MON_TY + 6, DW = MON_TX + 4, DH = MON_TY + 4;
  __shared__ double ug[UH][UW], vg[UH][UW], d2u[DH][DW], d2v[DH][DW];
  __shared__ double red[MON_NQ + MON_NMN][MON_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // ny, nyt: rows of the BASIN (every boundary rule uses global rows gj = j + joff); j, j0: local rows of the arrays
  const int nx = P.g.nx, ny = P.g.nyg, nxt = P.g.nxt, nyt = ny - 1, ldx = P.g.ldx, ldt = P.ldt;
  const int joff = SLAB ? mon_in_vgpr(P.g.joff) : 0, jhi = SLAB ? mon_in_vgpr(P.jhi) : ny;
  const long fs = P.g.fstride;
  const int b = blockIdx.x, tx = b % P.ntx, ty = b / P.ntx;
  const int i0 = tx * MON_TX + 1, j0 = (SLAB ? P.jlo : 1) + ty * MON_TY;
  const int i = i0 + lane;
  const double rdxof0 = P.rdxof0, rdt = P.rdxof0 / P.dto, dxom2 = P.dxom2;
  const double BIG = HUGE_VAL;
  double si[MON_NQ], mi[MON_NMN];
#pragma unroll
  for (int q = 0; q < MON_NQ; ++q) si[q] = 0.0;
#pragma unroll
  for (int q = 0; q < MON_NMN; ++q) mi[q] = BIG;

#pragma unroll   // (k static: the k == 0 / k == NL - 1 terms and rgpoc[k] resolve at compile time)
  for (int k = 0; k < NL; ++k) {
    const double *pk = P.po + fs * k, *pmk = P.pom + fs * k, *qk = P.qo + fs * k;
    // lagged geostrophic velocities (:627-646): ugoc on (nxpo, nyto), vgoc on (nxto, nypo); 0 off the grid.  On a
    // y-slab, 0 also more than two rows beyond the last owned row, where no owned point's Del-4th reaches: pom is read
    // on local rows >= j0 - 3 >= jlo - 3 and <= jhi + 3, which the 3 halo rows hold (a whole domain: jhi = ny)
    for (int t = tid; t < UW * UH; t += MON_NT) {
      const int a = t % UW, bb = t / UW;
      const int gi = i0 - 3 + a, lj = j0 - 3 + bb, gj = lj + joff;
      double u = 0.0, v = 0.0;
      const int iu = CYC ? mon_wrap(gi, nx) : gi, iv = CYC ? mon_wrap(gi, nxt) : gi;
      if (gj >= 1 && gj <= nyt && (!SLAB || lj <= jhi + 2) && iu >= 1 && iu <= nx) {
        const long o = (long)(lj - 1) * ldx + (iu - 1);
        u = -rdxof0 * (pmk[o + ldx] - pmk[o]);
      }
      if (gj >= 1 && gj <= ny && (!SLAB || lj <= jhi + 3) && iv >= 1 && iv <= nxt) {
        const long o = (long)(lj - 1) * ldx + (iv - 1);
        v = rdxof0 * (pmk[o + 1] - pmk[o]);
      }
      ug[bb][a] = u;
      vg[bb][a] = v;
    }
    __syncthreads();
    for (int t = tid; t < DW * DH; t += MON_NT) {
      const int a = t % DW, bb = t / DW;
      const int gi = i0 - 2 + a, gj = j0 - 2 + bb + joff;
      d2u[bb][a] = mon_lap<CYC, UW>(ug, a + 1, bb + 1, gi, gj, nx, nyt, dxom2);
      d2v[bb][a] = mon_lap<CYC, UW>(vg, a + 1, bb + 1, gi, gj, nxt, ny, dxom2);
    }
    __syncthreads();

    double s[MON_NQ], m[MON_NMN];
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) s[q] = 0.0;
#pragma unroll
    for (int q = 0; q < MON_NMN; ++q) m[q] = BIG;
    const double rg = k < NL - 1 ? P.rgpoc[k] : 0.0, rgdt = rg / P.dto;
    for (int r = wv; r < MON_TY; r += MON_NT / 64) {
      const int j = j0 + r, gj = j + joff;
      if (i <= nx && j <= jhi) {
        const long o = (long)(j - 1) * ldx + (i - 1);
        const double wx = (i == 1 || i == nx) ? 0.5 : 1.0, wy = (gj == 1 || gj == ny) ? 0.5 : 1.0, wp = wx * wy;
        const double p = pk[o];
        // p grid (genint 0.5, 0.5): pint, qint (:729-730), eta terms (:557-590), extrema of po (:655-666)
        s[MS_P] += wp * p;
        s[MS_Q] += wp * qk[o];
        m[0] = mon_min(m[0], p);
        m[1] = mon_min(m[1], -p);
        if (k < NL - 1) {
          const double pn = pk[fs + o];
          const double eta = rg * (pn - p);
          const double etadot = rgdt * (p - pn - pmk[o] + pmk[fs + o]);
          s[MS_ETA] += wp * eta;
          s[MS_ETA2] += wp * (eta * eta);
          s[MS_ETADOT] += wp * (eta * etadot);
          if (k == 0) si[MS_ETAENT] += wp * (eta * P.entoc[o]);
        }
        if (k == 0) {
          const double we = P.wekpo[o], en = P.entoc[o];
          si[MS_WEKP] += wp * we;
          si[MS_AWEKP] += wp * fabs(we);
          si[MS_ENT] += wp * en;
          si[MS_AENT] += wp * fabs(en);
        }
        // u points (genint 0.5, 1.0): (nxpo, nyto)
        if (gj <= nyt) {
          const double ugeos = -rdxof0 * (pk[o + ldx] - p);
          const double ugdot = -rdt * (pk[o + ldx] - pmk[o] - pmk[o + ldx] + pmk[o]); // (sic, :679-680)
          const double d2 = d2u[r + 2][lane + 2];
          const double d4 = mon_lap<CYC, DW>(d2u, lane + 2, r + 2, i, gj, nx, nyt, dxom2);
          s[MS_U2D] += wx * (ugeos * d2);
          s[MS_U4D] += wx * (ugeos * d4);
          s[MS_UKE] += wx * (ugeos * ugeos);
          s[MS_UKEDOT] += wx * (ugeos * ugdot);
          if (k == 0) si[MS_UTAUX] += wx * (ugeos * (0.5 * (P.taux[o + ldx] + P.taux[o])));
          if (k == NL - 1) {
            const double ul = ug[r + 3][lane + 3];
            si[MS_UBOT] += wx * (ul * ul);
          }
        }
        // v points (genint 1.0, 0.5): (nxto, nypo)
        if (i <= nxt) {
          const double vgeos = rdxof0 * (pk[o + 1] - p);
          const double vgdot = rdt * (pk[o + 1] - p - pmk[o + 1] + pmk[o]);
          const double d2 = d2v[r + 2][lane + 2];
          const double d4 = mon_lap<CYC, DW>(d2v, lane + 2, r + 2, i, gj, nxt, ny, dxom2);
          s[MS_V2D] += wy * (vgeos * d2);
          s[MS_V4D] += wy * (vgeos * d4);
          s[MS_VKE] += wy * (vgeos * vgeos);
          s[MS_VKEDOT] += wy * (vgeos * vgdot);
          if (k == 0) si[MS_VTAUY] += wy * (vgeos * (0.5 * (P.tauy[o + 1] + P.tauy[o])));
          if (k == NL - 1) {
            const double vl = vg[r + 3][lane + 3];
            si[MS_VBOT] += wy * (vl * vl);
          }
        }
        // T cells (i, j): couroc's velocities on the cell faces (:1753-1925), in the Q-G layer ...
        if (i <= nxt && gj <= nyt) {
          const long o1 = o + 1, on = o + ldx, on1 = on + 1;
          const double um = (!CYC && i == 1) ? 0.0 : -rdxof0 * (pk[on] - pk[o]);
          const double up = (!CYC && i == nxt) ? 0.0 : -rdxof0 * (pk[on1] - pk[o1]);
          const double vm = gj == 1 ? 0.0 : rdxof0 * (pk[o1] - pk[o]);
          const double vp = gj == nyt ? 0.0 : rdxof0 * (pk[on1] - pk[on]);
          if (i == 1) { m[2] = mon_min(m[2], um); m[3] = mon_min(m[3], -um); }
          m[2] = mon_min(m[2], up);
          m[3] = mon_min(m[3], -up);
          m[4] = mon_min(m[4], mon_min(vm, vp));
          m[5] = mon_min(m[5], mon_min(-vm, -vp));
          m[6] = mon_min(m[6], -((um + up) * (um + up) + (vm + vp) * (vm + vp)));
          if (k == 0) {
            // ... and in the mixed layer (:1492-1744), with the Ekman part of the stress; T-grid integrals (:786-807)
            const double uv = P.uvgfac, rh = P.rhf0hm;
            const double *tx = P.taux, *ty = P.tauy;
            const double mum = (!CYC && i == 1) ? 0.0 : -uv * (pk[on] - pk[o]) + rh * (ty[on] + ty[o]);
            const double mup = (!CYC && i == nxt) ? 0.0 : -uv * (pk[on1] - pk[o1]) + rh * (ty[on1] + ty[o1]);
            const double mvm = gj == 1 ? (P.sb ? -rh * (tx[o1] + tx[o]) : 0.0) : uv * (pk[o1] - pk[o]) - rh * (tx[o1] + tx[o]);
            const double mvp = gj == nyt ? (P.nb ? -rh * (tx[on1] + tx[on]) : 0.0) : uv * (pk[on1] - pk[on]) - rh * (tx[on1] + tx[on]);
            if (i == 1 && gj > 1 && gj < nyt) { mi[2] = mon_min(mi[2], mum); mi[3] = mon_min(mi[3], -mum); } // (the corner rows start at up)
            mi[2] = mon_min(mi[2], mup);
            mi[3] = mon_min(mi[3], -mup);
            mi[4] = mon_min(mi[4], mon_min(mvm, mvp));
            mi[5] = mon_min(mi[5], mon_min(-mvm, -mvp));
            mi[6] = mon_min(mi[6], -((mum + mup) * (mum + mup) + (mvm + mvp) * (mvm + mvp)));
            const long ot = (long)(j - 1) * ldt + (i - 1);
            const double wt = P.wekto[ot], ss = P.sst[ot];
            si[MS_WEKT] += wt;
            si[MS_AWEKT] += fabs(wt);
            si[MS_SSTWEK] += ss * wt;
            si[MS_SST] += ss;
            mi[0] = mon_min(mi[0], ss);
            mi[1] = mon_min(mi[1], -ss);
          }
        }
      }
    }
    mon_flush(s, m, red, P.psum, P.pmin, MON_NQ * k, MON_NMN * k, P.nblk, b);
  }
  mon_flush(si, mi, red, P.psum, P.pmin, MON_NQ * NL, MON_NMN * NL, P.nblk, b);
}

template <int NL, bool CYC>
__global__ __launch_bounds__(MON_NT) void k_mon_scan(const QgMonParams P) { mon_scan<NL, CYC, false>(P); }

// the scan over the owned rows of a y-slab (qgcm_hip_monitors_part)
template <int NL, bool CYC>
__global__ __launch_bounds__(MON_NT) void k_monslab_scan(const QgMonParams P) { mon_scan<NL, CYC, true>(P); }

// ujeto(j) of layer k (:671-688) in the reference's order: one wave per (row, layer) puts the row's ugeos into LDS
// (dynamic, min(nxpo, MON_JET_CHUNK) doubles: launch_monitors), then one lane sums i = 1..nxpo serially and subtracts
// ugeos(nxpo), as the Fortran loop does - bitwise the reference's ujeto, so ocjpos / ocjval are too.  A row longer than
// MON_JET_CHUNK (the split rows of DESIGN 3.5c: 11521 and 23041 points) passes through the same LDS chunk by chunk; the
// one lane keeps its running sum across the chunks, so the order of the additions is that of one pass.  Every row of
// at most MON_JET_CHUNK points is one pass with the barriers it always had.  grid (owned T rows njet, nlo), 64 threads.
#define MON_JET_CHUNK 8192 // ugeos values per LDS pass: 64 KiB, the most a launch gets without an attribute
__global__ __launch_bounds__(64) void k_mon_jet(const QgMonParams P) {
  extern __shared__ double urow[];
  const int j = blockIdx.x + P.jlo, k = blockIdx.y, nx = P.g.nx;
  const double *pk = P.po + P.g.fstride * k + (long)(j - 1) * P.g.ldx;
  double ujet = 0.0, last = 0.0;
  for (int c0 = 0; c0 < nx; c0 += MON_JET_CHUNK) {
    const int n = nx - c0 < MON_JET_CHUNK ? nx - c0 : MON_JET_CHUNK;
    if (c0) __syncthreads(); // the one lane has read the chunk before
    for (int i = threadIdx.x; i < n; i += 64) urow[i] = -P.rdxof0 * (pk[P.g.ldx + c0 + i] - pk[c0 + i]);
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < n; ++i) ujet = ujet + urow[i];
      last = urow[n - 1];
    }
  }
  if (threadIdx.x != 0) return;
  ujet = ujet - last;
  P.ujet[(long)k * P.njet + blockIdx.x] = fabs(ujet) / (double)P.g.nxt;
}

// The partials of this handle in a fixed order (all MON_FT threads): the sums and minima of every workgroup -> rs, rm,
// and per layer the largest ujeto of the owned T rows with its GLOBAL row (the first row that reaches it; 0, 0 when
// all are zero) (:690-698) -> jv, jp.
template <int NL>
__device__ __forceinline__ void mon_reduce(const QgMonParams &P, double *rs, double *rm, double *jv, int *jp) {
  constexpr int NS = MON_NS(NL), NM = MON_NM(NL);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nblk = P.nblk;
  const int njet = P.njet, jrow0 = P.jlo - 1 + P.g.joff; // ujet index j - 1 is global T row j + jrow0
  for (int q = wv; q < NS + NM; q += MON_FT / 64) {
    const bool sum = q < NS;
    const double *src = sum ? P.psum + (long)q * nblk : P.pmin + (long)(q - NS) * nblk;
    // four independent chains per lane (four loads in flight), combined in a fixed order
    const double z = sum ? 0.0 : HUGE_VAL;
    double a[4] = {z, z, z, z};
    int bb = lane;
    for (; bb + 192 < nblk; bb += 256)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = sum ? a[r] + src[bb + 64 * r] : mon_min(a[r], src[bb + 64 * r]);
    for (; bb < nblk; bb += 64) a[0] = sum ? a[0] + src[bb] : mon_min(a[0], src[bb]);
    double v = sum ? (a[0] + a[1]) + (a[2] + a[3]) : mon_min(mon_min(a[0], a[1]), mon_min(a[2], a[3]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double w = __shfl_xor(v, off);
      v = sum ? v + w : mon_min(v, w);
    }
    if (lane == 0) {
      if (sum) rs[q] = v;
      else rm[q - NS] = v;
    }
  }
  // position and value of the largest ujeto (the first row that reaches it; 0, 0 when all are zero) (:690-698)
  for (int k = wv; k < NL; k += MON_FT / 64) {
    double bv = 0.0;
    int bj = 0;
    for (int j = lane + 1; j <= njet; j += 64) {
      const double u = P.ujet[(long)k * njet + j - 1];
      if (u > bv) { bv = u; bj = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off);
      const int oj = __shfl_xor(bj, off);
      if (ov > bv || (ov == bv && ov > 0.0 && oj < bj)) { bv = ov; bj = oj; }
    }
    if (lane == 0) { jv[k] = bv; jp[k] = bj > 0 ? bj + jrow0 : 0; }
  }
}

// The scalar arithmetic of monnc_comp and couroc on the reduced basin-wide numbers (one thread); pos[k], pon[k] =
// po(1, 1, k), po(1, nypo, k) (poref, osfmin / osfmax, occirc).
template <int NL>
__device__ __forceinline__ void mon_finish(const QgMonParams &P, const double *rs, const double *rm, const double *jv,
                                           const int *jp, const double *pos, const double *pon, double *out) {
  const double on = P.ocnorm, rho = P.rhooc, fnot = P.fnot;
  const double *I = rs + MON_NQ * NL, *X = rm + MON_NMN * NL;
  double *o = out;
  *o++ = I[MS_WEKT] * on;   // wetmoc
  *o++ = I[MS_AWEKT] * on;  // watmoc
  *o++ = I[MS_WEKP] * on;   // wepmoc
  *o++ = I[MS_AWEKP] * on;  // wapmoc
  *o++ = I[MS_ENT] * on;    // entmoc
  *o++ = I[MS_AENT] * on;   // enamoc
  for (int k = 0; k < NL - 1; ++k) *o++ = rs[MON_NQ * k + MS_ETA] * on;                         // etamoc
  for (int k = 0; k < NL - 1; ++k) *o++ = rs[MON_NQ * k + MS_ETA2] * on;                        // et2moc
  for (int k = 0; k < NL - 1; ++k) *o++ = rho * P.gpoc[k] * rs[MON_NQ * k + MS_ETADOT];        // ddtpeoc (no ocnorm, :581)
  *o++ = rho * P.gpoc[0] * I[MS_ETAENT] * on;                                                     // pkenoc
  *o++ = rho * (I[MS_VTAUY] + I[MS_UTAUX]) * on;                                                  // utauoc
  double occ[NL];
  for (int k = 0; k < NL; ++k) {
    const double *S = rs + MON_NQ * k, *M = rm + MON_NMN * k, h = P.hoc[k];
    const double pomin = M[0], pomax = -M[1];
    const double poref = fnot > 0.0 ? pos[k] : (fnot < 0.0 ? pon[k] : 0.0);
    const double pmin_f = pomin / fnot, pmax_f = pomax / fnot;
    occ[k] = 1.0e-6 * h * (pos[k] - pon[k]) / fnot;
    o[0 * NL + k] = S[MS_P] * on;                                                        // pavgoc
    o[1 * NL + k] = S[MS_Q] * on;                                                        // qavgoc
    o[2 * NL + k] = -rho * P.ah2oc[k] * h * (S[MS_U2D] + S[MS_V2D]) * on;               // ah2doc
    o[3 * NL + k] = rho * P.ah4oc[k] * h * (S[MS_U4D] + S[MS_V4D]) * on;                // ah4doc
    o[4 * NL + k] = 0.5 * rho * h * (S[MS_UKE] + S[MS_VKE]) * on;                       // kealoc
    o[5 * NL + k] = rho * h * (S[MS_UKEDOT] + S[MS_VKEDOT]) * on;                       // ddtkeoc
    o[6 * NL + k] = 1.0e-6 * h * ((pmin_f < pmax_f ? pmin_f : pmax_f) - poref / fnot);  // osfmin
    o[7 * NL + k] = 1.0e-6 * h * ((pmin_f > pmax_f ? pmin_f : pmax_f) - poref / fnot);  // osfmax
    o[8 * NL + k] = occ[k];                                                              // occirc
    o[9 * NL + k] = (double)jp[k];                                                       // ocjpos
    o[10 * NL + k] = jv[k];                                                              // ocjval
  }
  o += 11 * NL;
  *o++ = 0.5 * rho * P.delek * fabs(fnot) * (I[MS_UBOT] + I[MS_VBOT]) * on;  // btdgoc
  *o++ = X[0];                                                                // sstmin
  *o++ = -X[1];                                                               // sstmax
  *o++ = I[MS_SST] * on;                                                      // tmlmoc
  *o++ = rho * P.cpoc * I[MS_SSTWEK] * on;                                    // hfmloc
  double tot = 0.0;
  for (int k = 0; k < NL; ++k) tot += occ[k];
  *o++ = tot;                                                                 // occtot
  const double cfac = P.hdxom1 * P.dto;
  *o++ = X[2];                       // umminoc
  *o++ = -X[3];                      // ummaxoc
  *o++ = X[4];                       // vmminoc
  *o++ = -X[5];                      // vmmaxoc
  *o++ = cfac * sqrt(-X[6]);         // cnmloc
  for (int k = 0; k < NL; ++k) {
    const double *M = rm + MON_NMN * k;
    o[k] = M[2];                     // ugminoc
    o[NL + k] = -M[3];               // ugmaxoc
    o[2 * NL + k] = M[4];            // vgminoc
    o[3 * NL + k] = -M[5];           // vgmaxoc
    o[4 * NL + k] = cfac * sqrt(-M[6]); // cnqgoc
  }
}

template <int NL>
__global__ __launch_bounds__(MON_FT) void k_mon_final(const QgMonParams P) {
  constexpr int NS = MON_NS(NL), NM = MON_NM(NL);
  __shared__ double rs[NS], rm[NM], jv[NL], pos[NL], pon[NL];
  __shared__ int jp[NL];
  mon_reduce<NL>(P, rs, rm, jv, jp);
  const long fs = P.g.fstride, onorth = (long)(P.jhi - 1) * P.g.ldx; // (a whole-domain handle: jhi = nypo)
  if (threadIdx.x < NL) {
    pos[threadIdx.x] = P.po[fs * threadIdx.x];
    pon[threadIdx.x] = P.po[fs * threadIdx.x + onorth];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  mon_finish<NL>(P, rs, rm, jv, jp, pos, pon, P.out);
}

// ---- y-slabs: per-rank summary + combine (the pattern of the Thomas summaries: one all-gather in between) ----------
// summary of MON_PART_LEN(nl) doubles (include/qgcm_hip.h): sums (MON_NS) | minima (MON_NM) | ujeto max (nl) | its
// global T row (nl) | po(1, g0, k) (nl) | po(1, g1, k) (nl) | g0 | g1      (g0..g1: the global p rows this rank owns)
template <int NL>
__global__ __launch_bounds__(MON_FT) void k_monslab_part(const QgMonParams P) {
  constexpr int NS = MON_NS(NL), NM = MON_NM(NL);
  __shared__ double rs[NS], rm[NM], jv[NL];
  __shared__ int jp[NL];
  mon_reduce<NL>(P, rs, rm, jv, jp);
  __syncthreads();
  const int tid = threadIdx.x;
  double *o = P.out;
  for (int q = tid; q < NS; q += MON_FT) o[q] = rs[q];
  for (int q = tid; q < NM; q += MON_FT) o[NS + q] = rm[q];
  o += NS + NM;
  const long fs = P.g.fstride, ol = (long)(P.jlo - 1) * P.g.ldx, oh = (long)(P.jhi - 1) * P.g.ldx;
  if (tid < NL) {
    o[tid] = jv[tid];
    o[NL + tid] = (double)jp[tid];
    o[2 * NL + tid] = P.po[fs * tid + ol];
    o[3 * NL + tid] = P.po[fs * tid + oh];
  }
  if (tid == 0) {
    o[4 * NL] = (double)(P.jlo + P.g.joff);
    o[4 * NL + 1] = (double)(P.jhi + P.g.joff);
  }
}

// nranks gathered summaries (rank r at r * MON_PART_LEN) -> the vector of k_mon_final, then out[MON_LEN] = status: 0,
// or r + 1 when rank r is the first whose rows do not continue the tiling of 1..nypo (nothing else is written then).
// Sums and minima over the ranks in rank order; the jet moves to a later rank only with a strictly larger ujeto (the
// reference's first occurrence).  One workgroup, no atomics: every rank computes bitwise the same vector.
template <int NL>
__global__ __launch_bounds__(256) void k_monslab_combine(const QgMonParams P) {
  constexpr int NS = MON_NS(NL), NM = MON_NM(NL), L = MON_PART_LEN(NL);
  __shared__ double rs[NS], rm[NM], jv[NL], pos[NL], pon[NL];
  __shared__ int jp[NL], st;
  const int tid = threadIdx.x, R = P.nranks;
  const double *G = P.gath;
  for (int q = tid; q < NS + NM; q += 256) {
    double v = G[q];
    for (int r = 1; r < R; ++r) v = q < NS ? v + G[(long)r * L + q] : mon_min(v, G[(long)r * L + q]);
    if (q < NS) rs[q] = v;
    else rm[q - NS] = v;
  }
  if (tid < NL) {
    const int k = tid, J = NS + NM;
    double bv = 0.0;
    int bj = 0;
    for (int r = 0; r < R; ++r) {
      const double v = G[(long)r * L + J + k];
      if (v > bv) { bv = v; bj = (int)G[(long)r * L + J + NL + k]; }
    }
    jv[k] = bv;
    jp[k] = bj;
    pos[k] = G[J + 2 * NL + k];
    pon[k] = G[(long)(R - 1) * L + J + 3 * NL + k];
  }
  if (tid == 0) {
    int bad = 0, next = 1;
    for (int r = 0; r < R && !bad; ++r) {
      const double g0 = G[(long)r * L + L - 2], g1 = G[(long)r * L + L - 1];
      if (g0 != (double)next || g1 < g0 || g1 > (double)P.g.nyg || (r == R - 1 && g1 != (double)P.g.nyg)) bad = r + 1;
      else next = (int)g1 + 1;
    }
    st = bad;
    P.out[MON_LEN(NL)] = (double)bad;
  }
  __syncthreads();
  if (tid == 0 && st == 0) mon_finish<NL>(P, rs, rm, jv, jp, pos, pon, P.out);
}
