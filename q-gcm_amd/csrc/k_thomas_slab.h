// k_thomas_slab.h - a y-slab whose rows are cut into segments (more than 2048 rows, or QGCM_HIP_THOMAS_SLAB_SEG_ROWS):
// the segments of k_thomas.h nested inside the slab's summary.  The slab still publishes ONE (Cf, Cb, S0) per step and
// ONE (D, E, SP, SQ) per set-up, in the layout of every other slab: the other ranks cannot tell.
//
// Per wavenumber and mode a run of rows maps its inflows (u_in from below, v_in from above) as
//     u_out = Cf + D u_in,   v_out = Cb + E u_in + D v_in,   colsum = S0 + SP u_in + SQ v_in       (k_thomas_corr.inc)
// so with the slab's segments s = 1..S, south to north, the value entering segment s from below is
//     alpha_s + delta_s u_in:        alpha_1 = 0, delta_1 = 1,  alpha_{s+1} = Cf_s + D_s alpha_s,  delta_{s+1} = D_s delta_s
// and, north to south, the value entering it from above is
//     beta_s + eps_s u_in + gamma_s v_in:   beta_S = eps_S = 0, gamma_S = 1,
//         beta_{s-1} = Cb_s + E_s alpha_s + D_s beta_s,  eps_{s-1} = E_s delta_s + D_s eps_s,  gamma_{s-1} = D_s gamma_s.
// The slab's own summary is
//     Cf' = alpha_{S+1},  Cb' = beta_0,   S0' = sum_s S0_s + SP_s alpha_s + SQ_s beta_s        (every solve)
//     D' = delta_{S+1},   E' = eps_0,     SP' = sum_s SP_s delta_s + SQ_s eps_s,  SQ' = sum_s SQ_s gamma_s   (set-up)
//
// PHASE 1 (before the exchange): k_thomas_seg<R, 1, 8> over the slab's segments (zero-inflow solutions in place, the
//          segments' summaries into seg.msg), then k_thomas_fold<false>: (Cf', Cb', S0') into the slab's message, alpha_s
//          and beta_s into a device buffer.
// PHASE 2 (after it): k_thomas_corr_slab composes all RANKS' summaries as k_thomas_corr does (the same text), turns the
//          slab's inflows (uin, vin) into every segment's, and adds the segment's responses as k_thomas_corr_seg does.
// Set-up: k_thomas_fold<true> once (delta, eps, gamma per segment; D', E', SP', SQ' into slabDE).
#pragma once
#include "k_thomas.h"

// One lane per wavenumber walks the two chains over the segments (S <= 64 steps of a multiply-add, operands from L2).  The
// forward walk leaves alpha_s / delta_s in the table; the backward walk reads them back (the lane's own stores).
// SETUP: the right-hand-side independent half.  grid: (ceil(nk/64), nl), 64 threads
template <bool SETUP>
__global__ __launch_bounds__(64) void k_thomas_fold(const QgThomasFold F) {
  const int k = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y;
  if (k >= F.nk) return;
  const long mk = (long)m * F.ldw + k, per = (long)F.nl * F.ldw, plane = (long)F.S * per;
  const double *msg = F.msg + TH_MSG * mk, *cst = F.cst + TH_CST * mk; // + s * TH_MSG * per / s * TH_CST * per
  if (SETUP) {
    double *dl = F.coef + mk, *ep = dl + plane, *ga = ep + plane; // + s * per
    double d = 1.0;
    for (int s = 0; s < F.S; ++s) {
      dl[s * per] = d;
      d = cst[s * TH_CST * per] * d;
    }
    double e = 0.0, g = 1.0, sp = 0.0, sq = 0.0;
    for (int s = F.S - 1; s >= 0; --s) {
      const double *c = cst + s * TH_CST * per;
      const double ds = dl[s * per];
      ep[s * per] = e;
      ga[s * per] = g;
      sp += c[2] * ds + c[3] * e;
      sq += c[3] * g;
      e = c[1] * ds + c[0] * e;
      g = c[0] * g;
    }
    double *out = F.slabDE + TH_CST * mk;
    out[0] = d;
    out[1] = e;
    out[2] = sp;
    out[3] = sq;
  } else {
    double *al = F.ab + mk, *be = al + plane;
    // the chains of k_thomas_corr.inc, one level down: segments for ranks
    double u = 0.0;
    for (int s = 0; s < F.S; ++s) {
      al[s * per] = u;
      u = __builtin_fma(cst[s * TH_CST * per], u, msg[s * TH_MSG * per]);
    }
    double v = 0.0, term = 0.0;
    for (int s = F.S - 1; s >= 0; --s) {
      const double *gs = msg + s * TH_MSG * per, *gc = cst + s * TH_CST * per;
      const double us = al[s * per];
      be[s * per] = v;
      term += gs[2] + us * gc[2] + v * gc[3];
      v = __builtin_fma(gc[0], v, gs[1] + gc[1] * us);
    }
    double *out = F.send + TH_MSG * mk;
    out[0] = u;
    out[1] = v;
    out[2] = term;
  }
}

// blockIdx.z = segment * nslice + slice, as k_thomas_corr_seg; P.rank / P.nranks / P.gath / P.cgath are the RANKS', as
// k_thomas_corr's; T0's np / nq / poff / qoff are the first segment's.  Every segment's slice 0 composes the ranks' chain;
// segment 0's publishes ksum (and ybnd).  grid: (nblk, nlayers, S * nslice), dynamic LDS as k_thomas_corr
__global__ __launch_bounds__(THC_NT) void k_thomas_corr_slab(const QgThomasParams P, const QgThomasCorr T0, const QgThomasSegRec *segs,
                                                             const QgThomasFold F, const int nslice) {
  const int seg = blockIdx.z / nslice;
  const unsigned slice = blockIdx.z - seg * nslice;
  const QgThomasSegRec sg = segs[seg];
  const QgThomasCorr T = {T0.ptab, T0.qtab, T0.np + sg.tb0, T0.nq + sg.tb0, T0.poff + sg.tb0, T0.qoff + sg.tb0};
  const int rank = P.rank, jr0 = sg.jr0, jr1 = sg.jr1;
  const bool owner = seg == 0 && slice == 0;
  // the segment's five coefficients, requested before anything else (the lanes that run the ranks' chain)
  double fa = 0.0, fb = 0.0, fd = 1.0, fe = 0.0, fg = 1.0;
  if (threadIdx.x < TH_KW) {
    const long per = (long)F.nl * F.ldw, plane = (long)F.S * per;
    const long e = seg * per + (long)(blockIdx.y + P.layer0) * F.ldw + blockIdx.x * TH_KW + threadIdx.x; // (< ldw: a multiple of TH_KW)
    fa = F.ab[e];
    fb = F.ab[plane + e];
    fd = F.coef[e];
    fe = F.coef[plane + e];
    fg = F.coef[2 * plane + e];
  }
  // the slab's inflows -> the segment's: alpha + delta uin, beta + eps uin + gamma vin
#define THC_INFLOWS(u, v)                      \
  do {                                         \
    const double uin_ = (u);                   \
    (u) = __builtin_fma(fd, uin_, fa);         \
    (v) = __builtin_fma(fg, (v), fb + fe * uin_); \
  } while (0)
#include "k_thomas_corr.inc"
#undef THC_INFLOWS
}
