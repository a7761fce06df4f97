// k_tavg.h - the ocean's time averages on the device.
//
// Two products of the reference that otherwise need the whole state on the host:
//   * the fork's running mean of po (-Docnc_avg_k247): avg_ocn_k247 (src/timavge.F:624-662) adds po into po_avg on
//     every ocean step, right after ocqbdy (src/q-gcm.F:1250-1252), i.e. BEFORE the step's leapfrog averaging;
//     ocnc_avgout_k247 (src/nc_subs.F:1944-2052) scales by rnsum = 1/nsum_ocavg, writes and resets.
//   * tavocn / tavout, ocean half (src/timavge.F:425-619, 667-880): sums of the wind stress, wekpo, wekto, fnetoc,
//     sst, po, qo and of the mixed layer's C-grid advection terms uufo .. vtvfo; tavout scales them by
//     rnsoc = 1/nsumoc (0 when nsumoc = 0) and derives the eddy fluxes uptpoc / vptpoc.
// Everything is elementwise with the reference's expressions in the reference's order (built with
// -ffp-contract=off): bitwise the reference's numbers.
//
// Sum layout (QgTavParams.sum, all fields with the p grid's pitch ldx and fstride): field index
//   TAV_TX, TAV_TY, TAV_WP (nxpo,nypo) | TAV_WT, TAV_FM, TAV_SST (nxto,nyto) | pocav (nl) | qocav (nl) |
//   uufo, tufo, utufo (nxpo,nyto) | vvfo, tvfo, vtvfo (nxto,nypo); the means add uptpoc (nxpo,nyto), vptpoc (nxto,nypo).
//   T row j lives in (p) row j of its array.
//
//   k_poavg_add     po_avg += po over the owned rows, 16 bytes per lane
//   k_tav_accum     one tavocn contribution over the owned rows (templated on box / cyclic, sb_hflux, nb_hflux)
//   k_tav_mean      tavout's scaling and eddy fluxes into a separate buffer (the sums stay)
#pragma once
#include "qgcm_dev.h"

#define TAV_NT 256
enum { TAV_TX = 0, TAV_TY, TAV_WP, TAV_WT, TAV_FM, TAV_SST, TAV_P0 };
// index of the sums after pocav, qocav; the means append uptpoc, vptpoc
#define TAV_UU(nl) (TAV_P0 + 2 * (nl))
#define TAV_NSUM(nl) (TAV_UU(nl) + 6)
#define TAV_NMEAN(nl) (TAV_NSUM(nl) + 2)

// po_avg(:, jlo..jhi, k) += po(:, jlo..jhi, k): per layer one contiguous run of nrow * ldx doubles (ldx is a
// multiple of 16, so every run starts 128-B aligned); the row padding is summed too and never read.
__global__ __launch_bounds__(TAV_NT) void k_poavg_add(double *__restrict__ sum, const double *__restrict__ po, long off,
                                                       long n2, long fstride) {
  const long base = off + (long)blockIdx.y * fstride;
  const double2 *s = reinterpret_cast<const double2 *>(po + base);
  double2 *d = reinterpret_cast<double2 *>(sum + base);
  for (long t = (long)blockIdx.x * TAV_NT + threadIdx.x; t < n2; t += (long)gridDim.x * TAV_NT) {
    const double2 a = d[t], b = s[t];
    d[t] = double2{a.x + b.x, a.y + b.y};
  }
}

struct QgTavParams {
  QgGeom g;
  const double *po, *qo, *wekpo;        // (ldx, ny, nl) / (ldx, ny)
  const double *taux, *tauy;            // (ldx, ny)
  const double *sst, *wekto, *fnet;     // T grid, pitch ldt; fnet nullptr = zero (never set, mixed layer off)
  int ldt;
  int jlo, jhi, jt1;                    // owned local p rows jlo..jhi, owned T rows jlo..jt1
  double uvgfac, rhf0hm, tsbdy, tnbdy;  // src/timavge.F:447-448
  double *sum;                          // TAV_NSUM(nl) fields of fstride
  // k_tav_mean
  double *mean;                         // TAV_NMEAN(nl) fields of fstride
  double rnsoc;
  unsigned mask;                        // bit f: compute mean field f (uptpoc / vptpoc: bits TAV_NSUM, TAV_NSUM + 1)
};

// One thread per p point (i, j) of an owned row j: the p-grid sums and vvfo .. vtvfo (i <= nxto) of p row j; when T
// row j is owned also the T-grid sums (i <= nxto) and uufo .. utufo of T row j.  The neighbours a slab edge reads
// (po, tauyo row jhi + 1; sst T row jlo - 1) are halo rows: current after a step's averaging and halo exchange.
template <int NL, bool CYC, bool SB, bool NB>
__global__ __launch_bounds__(TAV_NT) void k_tav_accum(const QgTavParams P) {
  const int nx = P.g.nx, nxt = P.g.nxt, ldx = P.g.ldx, ldt = P.ldt, nyg = P.g.nyg;
  const long fs = P.g.fstride;
  const int i = blockIdx.x * TAV_NT + threadIdx.x + 1; // 1-based
  const int j = blockIdx.y + P.jlo;                   // local p row
  if (i > nx || j > P.jhi) return;
  const int gj = j + P.g.joff;
  const long ip = (long)(i - 1) + (long)ldx * (j - 1);
  double *S = P.sum;
  // wind stress and wekpo (p grid), po and qo
  S[TAV_TX * fs + ip] = S[TAV_TX * fs + ip] + P.taux[ip];
  S[TAV_TY * fs + ip] = S[TAV_TY * fs + ip] + P.tauy[ip];
  S[TAV_WP * fs + ip] = S[TAV_WP * fs + ip] + P.wekpo[ip];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    S[(TAV_P0 + k) * fs + ip] = S[(TAV_P0 + k) * fs + ip] + P.po[k * fs + ip];
    S[(TAV_P0 + NL + k) * fs + ip] = S[(TAV_P0 + NL + k) * fs + ip] + P.qo[k * fs + ip];
  }
  const double *sst = P.sst;
  const long it = (long)(i - 1) + (long)ldt * (j - 1); // T point (i, j)
  // meridional advection at p row j (T columns i = 1..nxto)
  if (i <= nxt) {
    double vvf, tvf, vtvf;
    if (gj == 1) {
      if (SB) {
        vvf = -(P.rhf0hm * (P.taux[ip + 1] + P.taux[ip]));
        tvf = 0.5 * (sst[it] + P.tsbdy);
        vtvf = vvf * tvf;
      } else {
        vvf = 0.0;
        tvf = sst[it];
        vtvf = 0.0;
      }
    } else if (gj == nyg) { // T row nyto = local row j - 1
      if (NB) {
        vvf = -(P.rhf0hm * (P.taux[ip + 1] + P.taux[ip]));
        tvf = 0.5 * (sst[it - ldt] + P.tnbdy);
        vtvf = vvf * tvf;
      } else {
        vvf = 0.0;
        tvf = sst[it - ldt];
        vtvf = 0.0;
      }
    } else {
      vvf = P.uvgfac * (P.po[ip + 1] - P.po[ip]) - P.rhf0hm * (P.taux[ip + 1] + P.taux[ip]);
      tvf = 0.5 * (sst[it] + sst[it - ldt]);
      vtvf = vvf * tvf;
    }
    const int u = TAV_UU(NL);
    S[(u + 3) * fs + ip] = S[(u + 3) * fs + ip] + vvf;
    S[(u + 4) * fs + ip] = S[(u + 4) * fs + ip] + tvf;
    S[(u + 5) * fs + ip] = S[(u + 5) * fs + ip] + vtvf;
  }
  if (j > P.jt1) return;
  // T-grid fields of T row j
  if (i <= nxt) {
    S[TAV_WT * fs + ip] = S[TAV_WT * fs + ip] + P.wekto[it];
    S[TAV_FM * fs + ip] = S[TAV_FM * fs + ip] + (P.fnet ? P.fnet[it] : 0.0);
    S[TAV_SST * fs + ip] = S[TAV_SST * fs + ip] + sst[it];
  }
  // zonal advection at T row j (p columns i = 1..nxpo); cyclic: column nxpo repeats column 1
  double uuf, tuf, utuf;
  const int ic = (CYC && i == nx) ? 1 : i;
  if (!CYC && (i == 1 || i == nx)) {
    uuf = 0.0;
    tuf = sst[(i == 1 ? 0 : nxt - 1) + (long)ldt * (j - 1)];
    utuf = 0.0;
  } else {
    const long pc = (long)(ic - 1) + (long)ldx * (j - 1), row = (long)ldt * (j - 1);
    uuf = -(P.uvgfac * (P.po[pc + ldx] - P.po[pc])) + P.rhf0hm * (P.tauy[pc + ldx] + P.tauy[pc]);
    // sst(i, j) + sst(i - 1, j); cyclic at i = 1: sst(1, j) + sst(nxto, j)
    tuf = 0.5 * (sst[row + ic - 1] + sst[row + (ic == 1 ? nxt - 1 : ic - 2)]);
    utuf = uuf * tuf;
  }
  const int u = TAV_UU(NL);
  S[u * fs + ip] = S[u * fs + ip] + uuf;
  S[(u + 1) * fs + ip] = S[(u + 1) * fs + ip] + tuf;
  S[(u + 2) * fs + ip] = S[(u + 2) * fs + ip] + utuf;
}

// tavout's arithmetic (src/timavge.F:721-727, 804-870) into P.mean; fields whose mask bit is clear are skipped.
template <int NL>
__global__ __launch_bounds__(TAV_NT) void k_tav_mean(const QgTavParams P) {
  const int nx = P.g.nx, nxt = P.g.nxt, ldx = P.g.ldx;
  const long fs = P.g.fstride;
  const int i = blockIdx.x * TAV_NT + threadIdx.x + 1;
  const int j = blockIdx.y + P.jlo;
  if (i > nx || j > P.jhi) return;
  const long ip = (long)(i - 1) + (long)ldx * (j - 1);
  const double r = P.rnsoc;
  const double *S = P.sum;
  double *M = P.mean;
  const unsigned m = P.mask;
  const bool trow = j <= P.jt1;
  for (int f = 0; f < TAV_UU(NL); ++f) {
    if (!(m >> f & 1u)) continue;
    const bool tgrid = f == TAV_WT || f == TAV_FM || f == TAV_SST;
    if (tgrid && (!trow || i > nxt)) continue;
    M[f * fs + ip] = r * S[f * fs + ip];
  }
  const int u = TAV_UU(NL), e = TAV_NSUM(NL);
  if (trow && (m & (0x7u << u | 1u << e))) {
    const double uu = r * S[u * fs + ip], tu = r * S[(u + 1) * fs + ip], ut = r * S[(u + 2) * fs + ip];
    if (m >> u & 1u) M[u * fs + ip] = uu;
    if (m >> (u + 1) & 1u) M[(u + 1) * fs + ip] = tu;
    if (m >> (u + 2) & 1u) M[(u + 2) * fs + ip] = ut;
    if (m >> e & 1u) M[e * fs + ip] = ut - uu * tu;
  }
  if (i <= nxt && (m & (0x7u << (u + 3) | 1u << (e + 1)))) {
    const double vv = r * S[(u + 3) * fs + ip], tv = r * S[(u + 4) * fs + ip], vt = r * S[(u + 5) * fs + ip];
    if (m >> (u + 3) & 1u) M[(u + 3) * fs + ip] = vv;
    if (m >> (u + 4) & 1u) M[(u + 4) * fs + ip] = tv;
    if (m >> (u + 5) & 1u) M[(u + 5) * fs + ip] = vt;
    if (m >> (e + 1) & 1u) M[(e + 1) * fs + ip] = vt - vv * tv;
  }
}
