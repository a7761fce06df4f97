// k_aml.h - atmospheric mixed layer on the device.
//
// Replaces `call aml` of the reference main program (src/q-gcm.F:1260):
//   amladf  advective + diffusive tendencies of the mixed-layer temperature and thickness: second-order C-grid advection
//           by the geostrophic velocity of layer 1 plus the Ekman velocity uekat / vekat of xforc, Del^2 and Del^4
//           diffusion of the lagged temperature (no flux through the zonal walls), Del^2 diffusion of the lagged
//           thickness (hmat outside the walls); zonally cyclic                        src/amlsubs.F:246-563
//   aml     leapfrog step of hmixa (7.16) with the diabatic term, the hmamin floor and the astm > diabcr reset, of ast
//           (7.17), entrainment at T points (7.18), convective correction (7.19), averaging onto the p grid plus the
//           eta and topography terms (entat), xan(1) = area integral, boundary line integrals enisat(1) / eninat(1),
//           monitors cfraat / centat                                                   src/amlsubs.F:47-238
//
// Two launches, after the pattern of k_oml.h (the T grid is 384 x 96 at the coupled double-gyre size: launch latency, not
// bandwidth, is what this costs):
//   k_aml_step   one thread per T point, operand fields staged through LDS (astm with halo 2; ast, hmixa, hmixam with
//                halo 1; pa(1) on the cell corners): both tendencies, the step with its three branches, the new ast and
//                hmixa into the spare buffers (three buffers each rotate: new -> ast, ast -> astm), raw entrainment xfa,
//                per-workgroup partial sums of the monitors
//   k_aml_entat  one thread per p point: entat, partials of xintp and of the two line sums
// The final reduction is oml_final_block of k_oml.h (the sums, their places in QgScalars and their scalings are the
// ocean's under other names): in workgroup 0 of the tendency launch that follows inside qgcm_hip_steps, in a
// one-workgroup launch after a stand-alone qgcm_hip_aml.
// Every expression keeps the reference's operand order (contraction off): ast, astm, hmixa, hmixam, entat are bitwise
// the reference's.  The sums run in a fixed tree: reproducible, equal to the reference's to rounding; cfraat is a sum
// of zeros and ones and therefore exact.
#pragma once
#include "qgcm_dev.h"
#include "k_oml.h" // tile constants, oml_block_sums

#define AML_SH 8 // tile rows of k_aml_step (64 x 8 T points per workgroup, 33 KB of LDS)

struct QgAmlParams {
  int nxt, nyt, nx, ny, nl; // T grid nxta x nyta, p grid nxpa x nypa, layers
  int ldt, ldx;
  long fstride;                          // doubles between two layers of pa / pam
  const double *ast, *astm, *hm, *hmm;   // T grid, pitch ldt
  double *astn, *hmn;                    // the spare buffers: new ast, new hmixa
  const double *fnet, *wekta, *xc1;      // T grid, pitch ldt
  const double *uekat;                   // (nxpa, nyta), pitch ldx
  const double *vekat;                   // (nxta, nypa), pitch ldt
  const double *pa, *pam, *dtop;         // p grid, pitch ldx (dtop: nullptr = zero topography)
  double *xfa, *entat;
  double *partA; // (3, nblkA): unused, cfrasm, centsm per workgroup of k_aml_step (the layout oml_final_block reads)
  double *partB; // (3, nblkB): xintp sum, S / N line sums per workgroup of k_aml_entat
  int nblkA, nblkB;
  double rdxaf0, hdxam1, d2tfac, d4tfac, hmdfac, hmat, hmamin, hmainv, hdrcdt, diabcr, entfac, xbfac, dface, cface, xcexp,
         tat1, tdta, rrcpat;
  double afacdp[QG_MAXL];
};

// grid: (ceil(nxt/64), ceil(nyt/AML_SH)), block 256 = 64 x 4; thread rows j0 + ty + 4 r
__global__ __launch_bounds__(OML_NT) void k_aml_step(const QgAmlParams P) {
  constexpr int TH = AML_SH, RPT = TH / OML_TY;
  constexpr int MW = OML_TX + 4, MH = TH + 4; // astm tile, halo 2: local (lx, ly) <-> T point (i0 - 2 + lx, j0 - 2 + ly)
  constexpr int SW = OML_TX + 2, SH = TH + 2; // ast, hmixa, hmixam tiles, halo 1
  constexpr int PW = OML_TX + 1, PH = TH + 1; // p-grid tile: p points (i0 + lx, j0 + ly)
  constexpr int DW = OML_TX + 2, DH = TH + 2; // del2t tile, halo 1
  __shared__ double sM[MH * MW], sS[SH * SW], sH[SH * SW], sL[SH * SW], sP[PH * PW], sD[DH * DW];
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * OML_TX + 1, j0 = blockIdx.y * TH + 1;
  const int lx0 = tid % OML_TX, ly0 = tid / OML_TX;
  const int i = i0 + lx0;
  const int nxt = P.nxt, nyt = P.nyt;
  const long ldt = P.ldt, ldx = P.ldx;
  // the T column a column position stands for (zonal wrap; modulo: the last tile reaches past the edge - those
  // positions are never used, but their addresses must stay inside the row), rows clamped (value unused)
  auto tcol = [&](int gi) { return ((gi - 1) % nxt + nxt) % nxt + 1; };
  auto trow = [&](int gj) { return gj < 1 ? 1 : (gj > nyt ? nyt : gj); };
  // ---- stage: all loads of a thread in flight together
  {
    constexpr int NM = (MH * MW + OML_NT - 1) / OML_NT, NS = (SH * SW + OML_NT - 1) / OML_NT, NP = (PH * PW + OML_NT - 1) / OML_NT;
    double vm[NM], vs[NS], vh[NS], vl[NS], vp[NP];
#pragma unroll
    for (int e = 0; e < NM; ++e) {
      const int idx = tid + e * OML_NT, lx = idx % MW, ly = idx / MW;
      vm[e] = P.astm[(long)(trow(j0 - 2 + (ly < MH ? ly : 0)) - 1) * ldt + (tcol(i0 - 2 + lx) - 1)];
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) {
      const int idx = tid + e * OML_NT, lx = idx % SW, ly = idx / SW;
      const long o = (long)(trow(j0 - 1 + (ly < SH ? ly : 0)) - 1) * ldt + (tcol(i0 - 1 + lx) - 1);
      vs[e] = P.ast[o];
      vh[e] = P.hm[o];
      vl[e] = P.hmm[o];
    }
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const int idx = tid + e * OML_NT, lx = idx % PW, ly = idx / PW;
      const int pi = i0 + lx > P.nx ? P.nx : i0 + lx, pj0 = j0 + (ly < PH ? ly : 0), pj = pj0 > P.ny ? P.ny : pj0;
      vp[e] = P.pa[(long)(pj - 1) * ldx + (pi - 1)];
    }
#pragma unroll
    for (int e = 0; e < NM; ++e) {
      const int idx = tid + e * OML_NT;
      if (idx < MH * MW) sM[idx] = vm[e];
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) {
      const int idx = tid + e * OML_NT;
      if (idx < SH * SW) {
        sS[idx] = vs[e];
        sH[idx] = vh[e];
        sL[idx] = vl[e];
      }
    }
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const int idx = tid + e * OML_NT;
      if (idx < PH * PW) sP[idx] = vp[e];
    }
  }
  // pointwise operands of this thread's own points, requested before the barrier
  double e_fnet[RPT], e_wk[RPT], e_xc[RPT], e_uw[RPT], e_ue[RPT], e_vs[RPT], e_vn[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int j = j0 + ly0 + OML_TY * r;
    const bool in = i <= nxt && j <= nyt;
    const long o = in ? (long)(j - 1) * ldt + (i - 1) : 0, ou = in ? (long)(j - 1) * ldx + (i - 1) : 0;
    e_fnet[r] = P.fnet[o];
    e_wk[r] = P.wekta[o];
    e_xc[r] = P.xc1 ? P.xc1[o] : 0.0;
    e_uw[r] = P.uekat[ou];     // uekat(i, j), uekat(i+1, j): i + 1 <= nxpa
    e_ue[r] = P.uekat[ou + 1];
    e_vs[r] = P.vekat[o];      // vekat(i, j), vekat(i, j+1): j + 1 <= nypa
    e_vn[r] = P.vekat[o + (in ? ldt : 0)];
  }
  __syncthreads();
  // ---- del2t of the tile and its halo, each value once, from the astm tile: src/amlsubs.F:314-315 (W), 338-339,
  // 363-364 (E), 403-404 / 422-423 (S / N rows), 455-456, 476-477, 497-498, 519-520 (corners) - one operand order per
  // row kind, the zonal neighbours wrapped; the dummy columns (:372-373, 457, 478, 499, 521) are the wrapped columns
  for (int idx = tid; idx < DH * DW; idx += OML_NT) {
    const int lx = idx % DW, gj = j0 - 1 + idx / DW;
    double val = 0.0;
    if (gj >= 1 && gj <= nyt) {
      const double *T = &sM[(gj - (j0 - 2)) * MW + (lx + 1)];
      const double cc = T[0], w = T[-1], e = T[1];
      if (gj == 1) val = w + e + T[MW] - 3.0 * cc;
      else if (gj == nyt) val = T[-MW] + w + e - 3.0 * cc;
      else val = T[-MW] + w + e + T[MW] - 4.0 * cc;
    }
    sD[idx] = val;
  }
  __syncthreads();
  const double rdxaf0 = P.rdxaf0, hdxam1 = P.hdxam1, hmat = P.hmat;
  double scfr = 0.0, scen = 0.0;
  // local accessors: p points (ii, jj) with ii in i .. i+1, jj in j .. j+1; T points (i + di, jj) within one of (i, j)
#define PA1(ii, jj) sP[((jj)-j0) * PW + ((ii)-i0)]
#define ASL(di, jj) sS[((jj)-(j0 - 1)) * SW + (lx0 + 1 + (di))]
#define HML(di, jj) sH[((jj)-(j0 - 1)) * SW + (lx0 + 1 + (di))]
#define HMM(di, jj) sL[((jj)-(j0 - 1)) * SW + (lx0 + 1 + (di))]
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int ly = ly0 + OML_TY * r;
    const int j = j0 + ly;
    if (i > nxt || j > nyt) continue;
    // ---- amladf: advection (the recurrences um = up, tm = tp of :323-325 are the same sums: a + b = b + a) ----
    const double um = -rdxaf0 * (PA1(i, j + 1) - PA1(i, j)) + e_uw[r];
    const double up = -rdxaf0 * (PA1(i + 1, j + 1) - PA1(i + 1, j)) + e_ue[r];
    const double tm = ASL(-1, j) + ASL(0, j), tp = ASL(0, j) + ASL(1, j);
    const double hm = HML(-1, j) + HML(0, j), hp = HML(0, j) + HML(1, j);
    const double xadvt = hdxam1 * (up * tp - um * tm);
    const double xadvh = hdxam1 * (up * hp - um * hm);
    double yadvt, yadvh, lap;
    const double hc = HMM(0, j), hw = HMM(-1, j), he = HMM(1, j);
    if (j == 1) { // :397-407 (and the corners :449-460, 470-481)
      const double vm = e_vs[r];
      const double vp = rdxaf0 * (PA1(i + 1, 2) - PA1(i, 2)) + e_vn[r];
      yadvt = hdxam1 * vp * (ASL(0, 2) + ASL(0, 1));
      yadvh = hdxam1 * (vp * (HML(0, 2) + HML(0, 1)) - vm * (HML(0, 1) + hmat));
      lap = hmat + hw + he + HMM(0, 2) - 4.0 * hc;
    } else if (j == nyt) { // :416-427 (:491-503, 513-525)
      const double vm = rdxaf0 * (PA1(i + 1, j) - PA1(i, j)) + e_vs[r];
      const double vp = e_vn[r];
      yadvt = hdxam1 * (-vm * (ASL(0, j) + ASL(0, j - 1)));
      yadvh = hdxam1 * (vp * (hmat + HML(0, j)) - vm * (HML(0, j) + HML(0, j - 1)));
      lap = HMM(0, j - 1) + hw + he + hmat - 4.0 * hc;
    } else { // :307-318, 331-342, 356-367
      const double vm = rdxaf0 * (PA1(i + 1, j) - PA1(i, j)) + e_vs[r];
      const double vp = rdxaf0 * (PA1(i + 1, j + 1) - PA1(i, j + 1)) + e_vn[r];
      yadvt = hdxam1 * (vp * (ASL(0, j + 1) + ASL(0, j)) - vm * (ASL(0, j) + ASL(0, j - 1)));
      yadvh = hdxam1 * (vp * (HML(0, j + 1) + HML(0, j)) - vm * (HML(0, j) + HML(0, j - 1)));
      lap = HMM(0, j - 1) + hw + he + HMM(0, j + 1) - 4.0 * hc;
    }
    double tmrhs = -(xadvt + yadvt);
    const double hmrhs = -(xadvh + yadvh) + P.hmdfac * lap;
    // ---- Del-sqd and Del-4th terms, :539-557 ----
    const double *d = &sD[(ly + 1) * DW + (lx0 + 1)];
    const double dc = d[0], dw = d[-1], de = d[1];
    if (j == 1) tmrhs = tmrhs + P.d2tfac * dc - P.d4tfac * (dw + de + d[DW] - 3.0 * dc);
    else if (j == nyt) tmrhs = tmrhs + P.d2tfac * dc - P.d4tfac * (d[-DW] + dw + de - 3.0 * dc);
    else tmrhs = tmrhs + P.d2tfac * dc - P.d4tfac * (d[-DW] + dw + de + d[DW] - 4.0 * dc);
    // ---- aml, :119-164 ----
    const double am = sM[(ly + 2) * MW + (lx0 + 2)]; // astm(i, j)
    double hnew, dtfix;
    if (am <= P.diabcr) {
      const double dhdiab = P.hdrcdt * (hc - hmat) / (P.tat1 - am);
      hnew = hc + P.tdta * hmrhs - dhdiab;
      const double dhfix = fmax(P.hmamin - hnew, 0.0);
      hnew = hnew + dhfix;
      dtfix = dhfix * (P.tat1 - am) / hc;
    } else {
      hnew = hmat;
      dtfix = 0.0;
    }
    const double trhtot = tmrhs + P.rrcpat * e_fnet[r] / hc - P.hmainv * e_wk[r] * am;
    double astnew = am + P.tdta * trhtot + dtfix;
    const double xfaent = P.xbfac * (hc - hmat) + P.dface * (P.xcexp * am + e_xc[r]);
    const double dtanew = P.tat1 - astnew;
    const double conena = P.entfac * HML(0, j) * fmin(0.0, dtanew);
    const long o = (long)(j - 1) * ldt + (i - 1);
    P.xfa[o] = xfaent - P.xcexp * conena;
    astnew = astnew + fmin(0.0, dtanew);
    P.astn[o] = astnew;
    P.hmn[o] = hnew;
    scfr += (0.5 - copysign(0.5, dtanew));
    scen -= conena;
  }
#undef PA1
#undef ASL
#undef HML
#undef HMM
  const int b = blockIdx.y * gridDim.x + blockIdx.x;
  double t[2] = {scfr, scen};
  oml_block_sums<2>(t, red, tid);
  if (tid == 0) {
    P.partA[b] = 0.0;
    P.partA[P.nblkA + b] = t[0];
    P.partA[2 * P.nblkA + b] = t[1];
  }
}

// grid: (ceil(nx/64), ceil(ny/16)), block 256 = 64 x 4, thread rows j0 + ty + 4 r
__global__ __launch_bounds__(OML_NT) void k_aml_entat(const QgAmlParams P) {
  __shared__ double red[12];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * OML_TX + (tid % OML_TX) + 1;
  const int nx = P.nx, ny = P.ny, nxt = P.nxt;
  const long ldt = P.ldt, ldx = P.ldx;
  double t[3] = {0.0, 0.0, 0.0}; // xintp sum, S and N line sums
#pragma unroll
  for (int r = 0; r < OML_RPT; ++r) {
    const int j = blockIdx.y * (OML_TY * OML_RPT) + (tid / OML_TX) + OML_TY * r + 1;
    if (i > nx || j > ny) continue;
    // the T cells west / east of the p column (column 1 and its copy nxpa: cells nxta and 1, src/amlsubs.F:175-181)
    const int iw = (i == 1 || i == nx) ? nxt : i - 1, ie = (i == 1 || i == nx) ? 1 : i;
    double en;
    if (j >= 2 && j <= ny - 1) {
      const double *lo = P.xfa + (long)(j - 2) * ldt, *hi = lo + ldt;
      en = 0.25 * (lo[iw - 1] + lo[ie - 1] + hi[iw - 1] + hi[ie - 1]);
    } else { // :187-194
      const double *row = P.xfa + (long)(j == 1 ? 0 : ny - 2) * ldt;
      en = 0.5 * (row[iw - 1] + row[ie - 1]);
    }
    // eta and topography contributions, :201-212
    const long o = (long)(j - 1) * ldx + (i - 1);
    double adpsum = 0.0;
    for (int l = 0; l < P.nl - 1; ++l) adpsum = adpsum + P.afacdp[l] * (P.pam[o + l * P.fstride] - P.pam[o + (l + 1) * P.fstride]);
    en = en + adpsum + P.cface * (P.dtop ? P.dtop[o] : 0.0);
    P.entat[o] = en;
    const double wx = (i == 1 || i == nx) ? 0.5 : 1.0, wy = (j == 1 || j == ny) ? 0.5 : 1.0; // xintp, src/intsubs.f:78-133
    t[0] += wx * wy * en;
    if (j == 1) t[1] += wx * en;  // :227-236
    if (j == ny) t[2] += wx * en;
  }
  const int b = blockIdx.y * gridDim.x + blockIdx.x;
  oml_block_sums<3>(t, red, tid);
  if (tid == 0) {
    P.partB[b] = t[0];
    P.partB[P.nblkB + b] = t[1];
    P.partB[2 * P.nblkB + b] = t[2];
  }
}

// leapfrog averaging of the mixed-layer temperature and thickness, src/q-gcm.F:1388-1394
__global__ __launch_bounds__(256) void k_aml_average(double *ast, const double *astm, double *hm, const double *hmm, long n) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    ast[t] = 0.5 * (ast[t] + astm[t]);
    hm[t] = 0.5 * (hm[t] + hmm[t]);
  }
}
