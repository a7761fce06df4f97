// k_atm_monitors.h - the atmosphere half of the monitoring diagnostics on the device.
//
// Replaces the atmosphere half of `call monnc_comp` (src/monitor_diag.F:160-172 and 185-475, with del4ch :1026-1151
// and genint :1155-1209) and `call courat` (:1213-1444), and the atmospheric half of `call valids` (src/valsubs.F:
// 120-269).  18*nla + 11 doubles come back (layout: include/qgcm_hip.h) instead of pa, pam, qa.
//   k_atmon_scan   one pass over the p grid in MON_TX x MON_TY tiles, all layers (the tile scheme of k_mon_scan, cyclic):
//                  per layer the lagged ugat / vgat of the tile + a 3-point halo (periodic images) go to LDS, then
//                  Del-sqd of them, then Del-4th at the tile's points, with del4ch's periodic wrap as the reference calls
//                  it (ugat with period nxpa, vgat with period nxta).  Each workgroup writes its partial genint sums and
//                  its partial minima (maxima as minima of the negated values, exact) through mon_flush.
//   k_atmon_chain  the serial chains: the zonal sums behind ujeta (one workgroup per row and layer, the reference's
//                  order), and in one more workgroup the sum of ast over the cells above the ocean (tmaooc).
//   k_atmon_final  one workgroup: reduces the partials in a fixed order, the arg-max over the rows and the scalar
//                  arithmetic of monnc_comp (atnorm, rhoat, cpat, olrtop) and courat.
//   k_atval        one workgroup: the twelve extrema of the atmospheric valids.
// No atomics: every sum has a fixed association order, so a call is bitwise reproducible.  The extrema, Courant numbers,
// atstpos / atstval and tmaooc use the reference's expressions uncontracted (-ffp-contract=off) and are bitwise the
// reference's (tests/golden/atmon_*.npz); the genint integrals are sums in another order and agree to rounding.
#pragma once
#include "k_monitors.h" // the tile constants, mon_lap (del4ch), mon_min, mon_flush, mon_wrap

#define ATMON_LEN(nl) (18 * (nl) + 11)
#define ATMON_CHUNK 2048 // ast values per LDS pass of the tmaooc chain
#define ATVAL_N 12       // min, max of pa, qa, ast, wekta, tauxa, tauya

// sums of layer k at MON_NQ*k + ...  (AS_VD2: vkedot is the genint of Del-sqd(lagged v), which del4ch leaves in attwk3:
// the reference computes vgdot but never stores it, src/monitor_diag.F:399-409)
enum { AS_P = 0, AS_Q, AS_U4D, AS_UKE, AS_UKEDOT, AS_V4D, AS_VKE, AS_VD2, AS_ETA, AS_ETA2, AS_ETADOT };
// layer-independent sums at MON_NQ*nl + ...
enum { AS_WEKT = 0, AS_AWEKT, AS_WEKP, AS_AWEKP, AS_ENT, AS_AENT, AS_ETAENT, AS_UTAUX, AS_VTAUY, AS_AST, AS_HMIX, AS_ASTH };
// minima of layer k at MON_NMN*k + ...: ugmin, -ugmax, vgmin, -vgmax, -vsqmax;
// layer-independent at MON_NMN*nl + ...: astmin, -astmax, ummin, -ummax, vmmin, -vmmax, -vsqmax (mixed layer)

struct QgAtmonParams {
  QgGeom g;                                        // the atmosphere: nx, ny = nxpa, nypa
  const double *pa, *pam, *qa, *wekpa, *entat;     // p grid, ldx pitch
  const double *tauxa, *tauya;                     // p grid, ldx pitch
  const double *uekat;                             // (nxpa, nyta), ldx pitch
  const double *wekta, *ast, *hmixa;               // T grid, ldt pitch
  const double *vekat;                             // (nxta, nypa), ldt pitch
  int ldt;
  int ntx, nblk;                                   // tiles along x, tiles in all
  int nx1, ny1, nxaooc, nyaooc;                    // the ocean's cells on the atmosphere's T grid (tmaooc)
  double rdxaf0, dxam2, hdxam1, dta, atnorm;
  double rhoat, cpat, hmat, davgat, bup, cup, dup;
  double aup[QG_MAXL - 1];
  double rgpat[QG_MAXL], gpat[QG_MAXL], hat[QG_MAXL], ah4at[QG_MAXL];
  double *psum;  // (MON_NS, nblk)
  double *pmin;  // (MON_NM, nblk)
  double *chain; // ujeta (nyta, nl), then tmaooc
  double *out;   // ATMON_LEN(nl) (k_atmon_final) or ATVAL_N (k_atval)
};

template <int NL>
__global__ __launch_bounds__(MON_NT) void k_atmon_scan(const QgAtmonParams P) {
  constexpr int UW = MON_TX + 6, UH = MON_TY + 6, DW = MON_TX + 4, DH = MON_TY + 4;
  __shared__ double ug[UH][UW], vg[UH][UW], d2u[DH][DW], d2v[DH][DW];
  __shared__ double red[MON_NQ + MON_NMN][MON_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nx = P.g.nx, ny = P.g.ny, nxt = nx - 1, nyt = ny - 1, ldx = P.g.ldx, ldt = P.ldt;
  const long fs = P.g.fstride;
  const int b = blockIdx.x, tx = b % P.ntx, ty = b / P.ntx;
  const int i0 = tx * MON_TX + 1, j0 = ty * MON_TY + 1;
  const int i = i0 + lane;
  const double rdx = P.rdxaf0, rdt = P.rdxaf0 / P.dta, dxm2 = P.dxam2;
  const double BIG = HUGE_VAL;
  double si[MON_NQ], mi[MON_NMN];
#pragma unroll
  for (int q = 0; q < MON_NQ; ++q) si[q] = 0.0;
#pragma unroll
  for (int q = 0; q < MON_NMN; ++q) mi[q] = BIG;

#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const double *pk = P.pa + fs * k, *pmk = P.pam + fs * k, *qk = P.qa + fs * k;
    // lagged geostrophic velocities (:320-338): ugat on (nxpa, nyta), vgat on (nxta, nypa); 0 off the grid in y
    for (int t = tid; t < UW * UH; t += MON_NT) {
      const int a = t % UW, bb = t / UW;
      const int gi = i0 - 3 + a, gj = j0 - 3 + bb;
      const int iu = mon_wrap(gi, nx), iv = mon_wrap(gi, nxt);
      double u = 0.0, v = 0.0;
      if (gj >= 1 && gj <= nyt) {
        const long o = (long)(gj - 1) * ldx + (iu - 1);
        u = -rdx * (pmk[o + ldx] - pmk[o]);
      }
      if (gj >= 1 && gj <= ny) {
        const long o = (long)(gj - 1) * ldx + (iv - 1);
        v = rdx * (pmk[o + 1] - pmk[o]);
      }
      ug[bb][a] = u;
      vg[bb][a] = v;
    }
    __syncthreads();
    for (int t = tid; t < DW * DH; t += MON_NT) {
      const int a = t % DW, bb = t / DW;
      const int gi = i0 - 2 + a, gj = j0 - 2 + bb;
      d2u[bb][a] = mon_lap<true, UW>(ug, a + 1, bb + 1, gi, gj, nx, nyt, dxm2);
      d2v[bb][a] = mon_lap<true, UW>(vg, a + 1, bb + 1, gi, gj, nxt, ny, dxm2);
    }
    __syncthreads();

    double s[MON_NQ], m[MON_NMN];
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) s[q] = 0.0;
#pragma unroll
    for (int q = 0; q < MON_NMN; ++q) m[q] = BIG;
    const double rg = k < NL - 1 ? P.rgpat[k] : 0.0, rgdt = rg / P.dta;
    for (int r = wv; r < MON_TY; r += MON_NT / 64) {
      const int j = j0 + r;
      if (i <= nx && j <= ny) {
        const long o = (long)(j - 1) * ldx + (i - 1);
        const double wx = (i == 1 || i == nx) ? 0.5 : 1.0, wy = (j == 1 || j == ny) ? 0.5 : 1.0, wp = wx * wy;
        const double p = pk[o];
        // p grid (genint 0.5, 0.5): pint, qint (:414-415), eta terms (:253-285), Ekman velocity and entrainment
        s[AS_P] += wp * p;
        s[AS_Q] += wp * qk[o];
        if (k < NL - 1) {
          const double pn = pk[fs + o];
          const double eta = rg * (p - pn);
          const double etadot = rgdt * (p - pn - pmk[o] + pmk[fs + o]);
          s[AS_ETA] += wp * eta;
          s[AS_ETA2] += wp * (eta * eta);
          s[AS_ETADOT] += wp * (eta * etadot);
          if (k == 0) si[AS_ETAENT] += wp * (eta * P.entat[o]);
        }
        if (k == 0) {
          const double we = P.wekpa[o], en = P.entat[o];
          si[AS_WEKP] += wp * we;
          si[AS_AWEKP] += wp * fabs(we);
          si[AS_ENT] += wp * en;
          si[AS_AENT] += wp * fabs(en);
        }
        // u points (genint 0.5, 1.0): (nxpa, nyta)
        if (j <= nyt) {
          const double ugeos = -rdx * (pk[o + ldx] - p);
          const double ugdot = -rdt * (pk[o + ldx] - p - pmk[o + ldx] + pmk[o]);
          const double d4 = mon_lap<true, DW>(d2u, lane + 2, r + 2, i, j, nx, nyt, dxm2);
          s[AS_U4D] += wx * (ugeos * d4);
          s[AS_UKE] += wx * (ugeos * ugeos);
          s[AS_UKEDOT] += wx * (ugeos * ugdot);
          if (k == 0) si[AS_UTAUX] += wx * (ugeos * (0.5 * (P.tauxa[o + ldx] + P.tauxa[o])));
        }
        // v points (genint 1.0, 0.5): (nxta, nypa)
        if (i <= nxt) {
          const double vgeos = rdx * (pk[o + 1] - p);
          const double d4 = mon_lap<true, DW>(d2v, lane + 2, r + 2, i, j, nxt, ny, dxm2);
          s[AS_V4D] += wy * (vgeos * d4);
          s[AS_VKE] += wy * (vgeos * vgeos);
          s[AS_VD2] += wy * d2v[r + 2][lane + 2];
          if (k == 0) si[AS_VTAUY] += wy * (vgeos * (0.5 * (P.tauya[o + 1] + P.tauya[o])));
        }
        // T cells (i, j): courat's velocities on the cell faces in the Q-G layer (:1355-1434) ...
        if (i <= nxt && j <= nyt) {
          const long o1 = o + 1, on = o + ldx, on1 = on + 1;
          const double um = -rdx * (pk[on] - pk[o]);
          const double up = -rdx * (pk[on1] - pk[o1]);
          const double vm = j == 1 ? 0.0 : rdx * (pk[o1] - pk[o]);
          const double vp = j == nyt ? 0.0 : rdx * (pk[on1] - pk[on]);
          // every row starts its recurrence with the western u, which enters the extrema
          if (i == 1) { m[0] = mon_min(m[0], um); m[1] = mon_min(m[1], -um); }
          m[0] = mon_min(m[0], up);
          m[1] = mon_min(m[1], -up);
          m[2] = mon_min(m[2], mon_min(vm, vp));
          m[3] = mon_min(m[3], mon_min(-vm, -vp));
          m[4] = mon_min(m[4], -((um + up) * (um + up) + (vm + vp) * (vm + vp)));
          if (k == 0) {
            // ... and in the mixed layer (:1247-1345): + the Ekman velocities; vekat itself on the zonal boundaries
            const long ot = (long)(j - 1) * ldt + (i - 1);
            const double mum = um + P.uekat[o], mup = up + P.uekat[o1];
            const double mvm = j == 1 ? P.vekat[ot] : vm + P.vekat[ot];
            const double mvp = j == nyt ? P.vekat[ot + ldt] : vp + P.vekat[ot + ldt];
            if (i == 1) { mi[2] = mon_min(mi[2], mum); mi[3] = mon_min(mi[3], -mum); }
            mi[2] = mon_min(mi[2], mup);
            mi[3] = mon_min(mi[3], -mup);
            mi[4] = mon_min(mi[4], mon_min(mvm, mvp));
            mi[5] = mon_min(mi[5], mon_min(-mvm, -mvp));
            mi[6] = mon_min(mi[6], -((mum + mup) * (mum + mup) + (mvm + mvp) * (mvm + mvp)));
            // T-grid integrals (genint 1.0, 1.0: plain sums) and the extrema of ast (:190-199, 440-452)
            const double wt = P.wekta[ot], as = P.ast[ot], hm = P.hmixa[ot];
            si[AS_WEKT] += wt;
            si[AS_AWEKT] += fabs(wt);
            si[AS_AST] += as;
            si[AS_HMIX] += hm;
            si[AS_ASTH] += as * hm;
            mi[0] = mon_min(mi[0], as);
            mi[1] = mon_min(mi[1], -as);
          }
        }
      }
    }
    mon_flush(s, m, red, P.psum, P.pmin, MON_NQ * k, MON_NMN * k, P.nblk, b);
  }
  mon_flush(si, mi, red, P.psum, P.pmin, MON_NQ * NL, MON_NMN * NL, P.nblk, b);
}

// The serial chains, dynamic LDS of max(nxpa, ATMON_CHUNK) doubles, 64 threads.  Workgroup (j - 1) + nyta*k: ujeta(j)
// of layer k (:343-365) - the row's ugeos into LDS, then one lane sums i = 1..nxpa and subtracts ugeos(nxpa), as the
// Fortran loop does.  Workgroup nyta*nla: tmaooc (:456-462), the cells j = ny1.., i = nx1.. row by row into LDS in
// chunks, one lane adds them in the reference's order.
__global__ __launch_bounds__(64) void k_atmon_chain(const QgAtmonParams P) {
  extern __shared__ double buf[];
  const int tid = threadIdx.x, nx = P.g.nx, nyt = P.g.ny - 1, ldx = P.g.ldx;
  const int b = blockIdx.x;
  if (b < nyt * P.g.nl) {
    const int j = b % nyt + 1, k = b / nyt;
    const double *pk = P.pa + P.g.fstride * k + (long)(j - 1) * ldx;
    for (int i = tid; i < nx; i += 64) buf[i] = -P.rdxaf0 * (pk[ldx + i] - pk[i]);
    __syncthreads();
    if (tid != 0) return;
    double ujet = 0.0;
    for (int i = 0; i < nx; ++i) ujet = ujet + buf[i];
    ujet = ujet - buf[nx - 1];
    P.chain[b] = fabs(ujet) / (double)(nx - 1);
    return;
  }
  const int w = P.nxaooc, n = P.nxaooc * P.nyaooc;
  const double *a0 = P.ast + (long)(P.ny1 - 1) * P.ldt + (P.nx1 - 1);
  double t = 0.0;
  for (int c0 = 0; c0 < n; c0 += ATMON_CHUNK) {
    const int c1 = n < c0 + ATMON_CHUNK ? n : c0 + ATMON_CHUNK;
    for (int q = c0 + tid; q < c1; q += 64) buf[q - c0] = a0[(long)(q / w) * P.ldt + q % w];
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < c1 - c0; ++q) t = t + buf[q];
    __syncthreads();
  }
  if (tid == 0) P.chain[nyt * P.g.nl] = t / (double)n;
}

// The partials in a fixed order (all MON_FT threads: one wave per quantity, four chains per lane), the jet position
// (the first row that reaches the largest ujeta; 0, 0 when all are zero, :368-375), then the scalar arithmetic on one
// thread.
template <int NL>
__global__ __launch_bounds__(MON_FT) void k_atmon_final(const QgAtmonParams P) {
  constexpr int NS = MON_NS(NL), NM = MON_NM(NL);
  __shared__ double rs[NS], rm[NM], jv[NL];
  __shared__ int jp[NL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nblk = P.nblk, nyt = P.g.ny - 1;
  for (int q = wv; q < NS + NM; q += MON_FT / 64) {
    const bool sum = q < NS;
    const double *src = sum ? P.psum + (long)q * nblk : P.pmin + (long)(q - NS) * nblk;
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
  for (int k = wv; k < NL; k += MON_FT / 64) {
    double bv = 0.0;
    int bj = 0;
    for (int j = lane + 1; j <= nyt; j += 64) {
      const double u = P.chain[(long)k * nyt + j - 1];
      if (u > bv) { bv = u; bj = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off);
      const int oj = __shfl_xor(bj, off);
      if (ov > bv || (ov == bv && ov > 0.0 && oj < bj)) { bv = ov; bj = oj; }
    }
    if (lane == 0) { jv[k] = bv; jp[k] = bj; }
  }
  __syncthreads();
  if (tid != 0) return;

  const double on = P.atnorm, rho = P.rhoat;
  const double *I = rs + MON_NQ * NL, *X = rm + MON_NMN * NL;
  double *o = P.out;
  *o++ = I[AS_WEKT] * on;   // wetmat
  *o++ = I[AS_AWEKT] * on;  // watmat
  *o++ = I[AS_WEKP] * on;   // wepmat
  *o++ = I[AS_AWEKP] * on;  // wapmat
  for (int k = 0; k < NL - 1; ++k) *o++ = k == 0 ? I[AS_ENT] * on : 0.0;                    // entmat (interface 1 only)
  for (int k = 0; k < NL - 1; ++k) *o++ = k == 0 ? I[AS_AENT] * on : 0.0;                   // enamat
  double etam[NL];
  for (int k = 0; k < NL - 1; ++k) *o++ = etam[k] = rs[MON_NQ * k + AS_ETA] * on;           // etamat
  for (int k = 0; k < NL - 1; ++k) *o++ = rs[MON_NQ * k + AS_ETA2] * on;                    // et2mat
  for (int k = 0; k < NL - 1; ++k) *o++ = rho * P.gpat[k] * rs[MON_NQ * k + AS_ETADOT];    // ddtpeat (no atnorm, :282)
  for (int k = 0; k < NL - 1; ++k) *o++ = k == 0 ? rho * P.gpat[0] * I[AS_ETAENT] * on : 0.0; // pkenat
  *o++ = rho * (I[AS_VTAUY] + I[AS_UTAUX]) * on;                                            // utauat
  for (int k = 0; k < NL; ++k) {
    const double *S = rs + MON_NQ * k, h = P.hat[k];
    o[0 * NL + k] = S[AS_P] * on;                                          // pavgat
    o[1 * NL + k] = S[AS_Q] * on;                                          // qavgat
    o[2 * NL + k] = rho * P.ah4at[k] * h * (S[AS_U4D] + S[AS_V4D]) * on;   // ah4dat
    o[3 * NL + k] = 0.5 * rho * h * (S[AS_UKE] + S[AS_VKE]) * on;          // kealat
    o[4 * NL + k] = rho * h * (S[AS_UKEDOT] + S[AS_VD2]) * on;             // ddtkeat
    o[5 * NL + k] = (double)jp[k];                                         // atstpos
    o[6 * NL + k] = jv[k];                                                 // atstval
  }
  o += 7 * NL;
  const double tmlmat = I[AS_AST] * on, hmlmat = I[AS_HMIX] * on;
  *o++ = tmlmat;                                  // tmlmat
  *o++ = hmlmat;                                  // hmlmat
  *o++ = X[0];                                    // astmin
  *o++ = -X[1];                                   // astmax
  *o++ = rho * P.cpat * I[AS_ASTH] * on;          // hcmlat
  *o++ = P.chain[nyt * NL];                       // tmaooc
  double olr = P.bup * (hmlmat - P.hmat) + P.cup * P.davgat + P.dup * tmlmat;
  for (int k = 0; k < NL - 1; ++k) olr = olr + P.aup[k] * etam[k];
  *o++ = olr;                                     // olrtop
  const double cfac = P.hdxam1 * P.dta;
  *o++ = X[2];                       // umminat
  *o++ = -X[3];                      // ummaxat
  *o++ = X[4];                       // vmminat
  *o++ = -X[5];                      // vmmaxat
  *o++ = cfac * sqrt(-X[6]);         // cnmlat
  for (int k = 0; k < NL; ++k) {
    const double *M = rm + MON_NMN * k;
    o[k] = M[0];                     // ugminat
    o[NL + k] = -M[1];               // ugmaxat
    o[2 * NL + k] = M[2];            // vgminat
    o[3 * NL + k] = -M[3];           // vgmaxat
    o[4 * NL + k] = cfac * sqrt(-M[4]); // cnqgat
  }
}

// The extrema of the atmospheric valids (src/valsubs.F:120-180): one workgroup of MON_FT threads, minima of the values
// and of their negations, then out = min, max of pa, qa, ast, wekta, tauxa, tauya.  Order-independent: bitwise.
__global__ __launch_bounds__(MON_FT) void k_atval(const QgAtmonParams P) {
  __shared__ double red[2 * 6][MON_FT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nx = P.g.nx, ny = P.g.ny, nxt = nx - 1, nyt = ny - 1, ldx = P.g.ldx, ldt = P.ldt;
  double m[2 * 6];
#pragma unroll
  for (int q = 0; q < 2 * 6; ++q) m[q] = HUGE_VAL;
  for (int t = tid; t < nx * ny; t += MON_FT) {
    const long o = (long)(t / nx) * ldx + t % nx;
    for (int k = 0; k < P.g.nl; ++k) {
      const double p = P.pa[P.g.fstride * k + o], q = P.qa[P.g.fstride * k + o];
      m[0] = mon_min(m[0], p); m[1] = mon_min(m[1], -p);
      m[2] = mon_min(m[2], q); m[3] = mon_min(m[3], -q);
    }
    const double x = P.tauxa[o], y = P.tauya[o];
    m[8] = mon_min(m[8], x); m[9] = mon_min(m[9], -x);
    m[10] = mon_min(m[10], y); m[11] = mon_min(m[11], -y);
  }
  for (int t = tid; t < nxt * nyt; t += MON_FT) {
    const long o = (long)(t / nxt) * ldt + t % nxt;
    const double a = P.ast[o], w = P.wekta[o];
    m[4] = mon_min(m[4], a); m[5] = mon_min(m[5], -a);
    m[6] = mon_min(m[6], w); m[7] = mon_min(m[7], -w);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int q = 0; q < 2 * 6; ++q) m[q] = mon_min(m[q], __shfl_xor(m[q], off));
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 2 * 6; ++q) red[q][wv] = m[q];
  __syncthreads();
  if (tid < 2 * 6) {
    double v = red[tid][0];
    for (int w = 1; w < MON_FT / 64; ++w) v = mon_min(v, red[tid][w]);
    P.out[tid] = (tid & 1) ? -v : v;
  }
}
