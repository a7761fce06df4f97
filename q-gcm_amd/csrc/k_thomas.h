// k_thomas.h - K4: batched constant-coefficient tridiagonal solves along y.
//
// Reference: for every wavenumber i the system
//     aoc*u(j-1) + boc(i)*u(j) + aoc*u(j+1) = rhs(i,j),  j = 2..nypo-1
// is solved by the Thomas algorithm (src/ocisubs.F:470-488 box, 575-593
// cyclic) and scaled by ftnorm.  The pivots betinv(j) = 1/(boc - aoc*gam(j))
// depend only on (boc, j), and the recurrence reaches a bitwise fixed point after
// a few rows (median 15 at 5 km; the lowest wavenumbers of the barotropic mode
// never do).  The host runs the recurrence once (same operations and rounding as the
// reference) and tabulates, per block of 16 wavenumbers, the pivots of the rows before
// the block's last wavenumber has become stationary (< 1 MB at 5 km) plus the
// stationary value per wavenumber: no divide is left in the kernel.  (Round 1
// re-ran the recurrence per thread: the 16 IEEE divides of the never-stationary
// block made that workgroup - and with it the launch - 4 us longer than the rest.)
//
// Parallel formulation: both sweeps are first-order linear recurrences
//     forward : u_r = (w_r - aoc*u_{r-1}) * bet_r     = fma(-g_r, u_{r-1}, w_r*bet_r),  g_r = aoc*bet_r
//     backward: v_r = u_r - aoc*bet_r * v_{r+1}       = fma(-g_r, v_{r+1}, u_r)
// (one fused multiply-add per row and sweep: the chain of dependent operations per row is 1 instead of 3, 16 -> 10
// VALU instructions per row in all, and with w*bet and g held in place of w and bet the kernel needs 92 VGPRs
// instead of 124.  The reference's rounding sequence is not kept - no chunked evaluation can keep it - the
// difference stays at the rounding level: tests/test_gpu_parity.py compares with the reference at 1e-12.)
// The rows are cut into 64 chunks of R rows; lanes hold 16 consecutive
// wavenumbers (one 128-B line) x 4 chunks per wave, a workgroup of 1024
// threads covers a whole column block.  Each thread keeps its R rows in
// registers, computes the chunk's affine map (C, D) with zero inflow, the
// maps are composed by a wave scan, and the sweep is re-run from the true
// inflow - so each row is read once and written once (PHASE 0).
//
// y-slab decomposition: the same idea one level up, see the PHASE list below: each
// rank reduces its slab to four numbers per wavenumber, ONE all-gather of
// 4*nk*nl doubles replaces the all-to-all transposes of the whole array.
//
// Algorithmic traffic: read w + write u (16 B per point) for PHASE 0.
#pragma once
#include "qgcm_dev.h"
#include "k_cyclic.h" // constr_cyc_partA

#define TH_KW 16   // wavenumbers per workgroup (128-B line)
#define TH_NC 64   // chunks per column
#define TH_NT (TH_KW * TH_NC)
static_assert(TH_NC == 64, "the chunk scan maps the 64 chunks of a wavenumber to the lanes of one wave");

// Inclusive scan of affine maps over the 64 lanes of a wave (lane = position in
// sweep order).  On return (Cs, Ds) is the composition of positions 0..lane.
// DPP moves instead of ds_bpermute shuffles (VALU only, a few cycles instead of an LDS-pipe round trip per step):
// shifts by 1, 2, 4, 8 inside each row of 16 lanes, then lane 15 of rows 0 / 2 into rows 1 / 3, then lane 31 into rows
// 2 and 3.  The composition is not commutative: the map taken from the lower lanes is always applied first.
template <int CTRL>
__device__ __forceinline__ double th_dpp(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ void th_scan_step(double &Cs, double &Ds, bool take) {
  const double Cp = th_dpp<CTRL>(Cs), Dp = th_dpp<CTRL>(Ds);
  if (take) {
    Cs = Cs + Ds * Cp;
    Ds = Ds * Dp;
  }
}
__device__ __forceinline__ void affine_scan(double &Cs, double &Ds, int lane) {
  const int rl = lane & 15;
  th_scan_step<0x111>(Cs, Ds, rl >= 1);        // row_shr:1
  th_scan_step<0x112>(Cs, Ds, rl >= 2);        // row_shr:2
  th_scan_step<0x114>(Cs, Ds, rl >= 4);        // row_shr:4
  th_scan_step<0x118>(Cs, Ds, rl >= 8);        // row_shr:8
  th_scan_step<0x142>(Cs, Ds, (lane & 16) != 0); // row_bcast:15 -> rows 1 and 3
  th_scan_step<0x143>(Cs, Ds, lane >= 32);     // row_bcast:31 -> rows 2 and 3
}

// PHASE 0  whole column in this handle: zero inflow at both ends, 1 read + 1 write.
// y-slab decomposition (one exchange per step, ONE pass over the work array):
//   u = u0 + uin*P,  v = B(u) + vin*Q  are linear in the values uin / vin that enter
//   the slab from the ranks below / above, so a slab is summarised by
//     Cf  = last value of the zero-inflow forward sweep,
//     Cb  = first value of the zero-inflow backward sweep applied to u0,
//     D   = product of (-a*bet) over the slab (forward AND backward gain),
//     E   = first value of the backward sweep applied to the unit forward response P.
//   D and E do not depend on the right-hand side (PHASE 4 computes them once).
// Area integrals (xintp of the solution, src/ocisubs.F:160 + src/intsubs.f:78-133) are taken in
// spectral space: the solution vanishes on the four walls, so xintp is the plain sum over the
// interior, and the sum over i of sin(k i pi/n) is cot(k pi/2n) for odd k, 0 for even k. Hence
//     xintp(wrk_m) = sum_k wcot(k) * ksum(m,k),   ksum(m,k) = ftnorm * sum_j v_j(k),
// and ksum is a by-product of the backward sweep (no pass over the transformed field, and the
// constraint solve no longer waits for the inverse row transform).  For y-slabs the column sum is
// linear in the inflows too:  sum_j v_j = S0 + uin*SP + vin*SQ  (S0: zero-inflow sum, SP / SQ:
// sums of the unit responses, right-hand-side independent), so every rank forms the basin-wide
// ksum from the one all-gather of the slab summaries - bitwise the same on every rank.
// PHASE 1  the slab's ZERO-INFLOW solution, written in place (1 read + 1 write, the same work as
//          PHASE 0), and (Cf, Cb, S0) per wavenumber published.  Rounds 1-3 published the summary
//          WITHOUT writing and ran both sweeps again from the true inflows after the exchange (a
//          second read + write of the whole array: NAtl 1 km 21 + 47 us per slab for one solve).
//          Now what is left after the exchange is k_thomas_corr below: the full responses to the
//          inflows, uin*Pv_r + vin*Qv_r, are ADDED to the rows they reach - they decay like
//          lambda^distance from the slab's ends, so for all but the lowest wavenumbers that is a few
//          rows (tables of Pv / Qv up to where they drop below 1e-19 of the inflow, built once at
//          set-up from PHASE 4 / 5's own output, QgThomasParams.corr*).
// PHASE 4  set-up: D, E and SP of this slab (input column = 0, unit inflow from below); the
//          response Pv is left in the work array for the table build.
// PHASE 5  set-up: SQ (input column = 0, unit inflow from above); Qv left in the work array.
// per-step message of one rank: TH_MSG doubles (Cf, Cb, S0) at TH_MSG*(m*ldw + k); the right-hand-side independent
// part (D, E, SP, SQ: TH_CST doubles, the layout of slabDE) is exchanged ONCE after set-up (cgath)
// grid: (ceil(nk/16), nlayers)
#define TH_MSG 3
#define TH_CST 4
// CYCA: the instantiation of the zonally cyclic geometries: it leaves the zonal-mean solution next to the boundaries in
// ybnd, and its grid carries one extra workgroup for part A of the cyclic / atmospheric constraint algebra (a template
// flag, not a run-time test: inlined into the plain instantiation the extra code cost it 11 spilled VGPRs at R = 16)
// KW: wavenumbers per workgroup = waves per workgroup.  16 (a 128-byte line per row, 1024 threads, 128 VGPRs) up to
// 16 rows per thread; 8 (512 threads, 256 VGPRs) for the long columns - R >= 20 keeps 4R doubles of rows and pivots in
// registers and spilled 100-800 B per lane under the 128-VGPR limit.
template <int R, int PHASE, bool CYCA = false, int KW = TH_KW>
// (second launch bound = waves per SIMD: 512-thread workgroups of 8 wavenumbers share a CU in pairs at 128 VGPRs)
__global__ __launch_bounds__(KW * TH_NC, (KW == 8 && R <= 16) ? 4 : 1) void k_thomas(QG_TH_ARGS, const QgThomasParams P) {
  const int *poff = P.poff;
  double *send = P.send, *slabDE = P.slabDE;
#include "k_thomas_solve.inc"
}

// ---------------------------------------------------------------------------------------------------------------
// Columns of more than 2048 rows in ONE handle: the column is cut into S segments (qgcm_hip_thomas_segments), each a
// "slab" of the y-slab algebra above that lives in the same work array.  k_thomas_seg runs PHASE 1 over all segments
// at once - the segment is the grid's z index, its rows and the origins of its tables, of its summary and of its
// constants come from a device table - and k_thomas_corr_seg below composes all segments' inflows and adds the
// responses.  (Set-up: the plain k_thomas<R, 4 / 5> once per segment, build_thomas_tables in qgcm_hip.hip - the set-up
// of the column that is not cut too, which is a plan of one segment.)  Two launches, 2 reads + 2 writes of the rows
// within reach against 1 + 1 of PHASE 0; the summaries never leave the device.  grid: (ceil(nk/KW), nlayers, S)
struct QgThomasSegRec {
  int jr0, jr1; // the segment's first / last local row (1-based, as QgGeom::jr0 / jr1)
  int tb0;      // offset of its (nblk, nlayers) entries in rcb / poff and in the response tables' np / nq / poff / qoff
  int pad;
  long b0;      // ... of its (ldw, nlayers) stationary pivots in binf
  long msg0;    // ... of its TH_MSG * (ldw, nlayers) summaries (the layout of the gathered slab messages)
  long cst0;    // ... of its TH_CST * (ldw, nlayers) constants (the layout of cgath)
};
// ... and of a y-slab cut into segments (k_thomas_slab.h): what folds the segments' summaries into the slab's own
struct QgThomasFold {
  const double *msg; // (Cf, Cb, S0) of every segment, segment-major (k_thomas_seg's output)
  const double *cst; // (D, E, SP, SQ) of every segment, segment-major
  double *coef;      // (3, S, nl, ldw): delta_s, eps_s, gamma_s (set-up)
  double *ab;        // (2, S, nl, ldw): alpha_s, beta_s (every solve)
  double *send;      // the slab's message: TH_MSG doubles per (mode, wavenumber)
  double *slabDE;    // the slab's constants: TH_CST doubles per (mode, wavenumber)
  int S, nl, ldw, nk;
};
template <int R, int PHASE, int KW>
__global__ __launch_bounds__(KW * TH_NC, (KW == 8 && R <= 16) ? 4 : 1) void k_thomas_seg(double *wrk, const QgThomasSegRec *segs, long wstride,
                                                                                         int ldw, int nk, int layer0, int nblk,
                                                                                         const QgThomasParams P) {
  static_assert(PHASE == 1, "the per-step phase only: the set-up runs k_thomas<R, 4 / 5> once per segment");
  constexpr bool CYCA = false;
  const QgThomasSegRec sg = segs[blockIdx.z];
  const double *binf = P.binf + sg.b0;
  const int *rcb = P.rcb + sg.tb0, *poff = P.poff + sg.tb0;
  double *send = P.send + sg.msg0, *slabDE = P.slabDE + sg.cst0;
  const int jr0 = sg.jr0, jr1 = sg.jr1;
#include "k_thomas_solve.inc"
}

// ---------------------------------------------------------------------------------------------------------------
// y-slabs, after the exchange of the slab summaries: k_thomas_corr.
//   1. composes all ranks' summaries (lanes = ranks, two affine scans per wavenumber) into the values uin / vin that
//      enter THIS slab from below / above, the basin-wide column sums ksum (bitwise the same on every rank) and, for
//      the zonally cyclic oceans, the zonal-mean solution next to the two zonal boundaries (ybnd);
//   2. adds the slab's full responses to those inflows to the zero-inflow solution PHASE 1 left in the work array:
//          v_r += uin * Pv_r  (rows r < np of the block)  +  vin * Qv_r  (the last nq rows),
//      Pv / Qv from the tables built at set-up.  Everything is scaled by ftnorm, as the stored rows are.
// Workgroup = one block of TH_KW wavenumbers (a 128-byte line per row): 256 threads; in step 2 a thread owns a pair
// of neighbouring wavenumbers (16-byte loads / stores) in every 32nd row.  grid: (ceil(nk/16), nlayers).
// The rows are independent of one another here - no sweep, no scan, no divide: the pass is bound by the bytes it
// touches, 2 x 8 B per corrected element + 8 B of table (NAtl 1 km, 600-row slabs: ~ 20 % of the rows on average).
struct QgThomasCorr {
  const double *ptab, *qtab; // responses, TH_KW doubles per row: block b of layer m starts at row poff / qoff of its table
  const int *np, *nq;        // (nblk, nlayers) rows within reach of the lower / upper inflow (0: no neighbour on that side)
  const int *poff, *qoff;
};
#define THC_NT 256
#ifndef THC_UNR
#define THC_UNR 4 // rows in flight per thread and trip of the correction loop
#endif
#define THC_PER ((TH_MSG + TH_CST) * TH_KW) // doubles per rank and block: summaries + constants of 16 wavenumbers
#define THC_LDS (THC_PER + TH_KW + 1)       // ... + the inflow per wavenumber (+ 1: bank spread between ranks)
__global__ __launch_bounds__(THC_NT) void k_thomas_corr(const QgThomasParams P, const QgThomasCorr T) {
  const int rank = P.rank, jr0 = P.g.jr0, jr1 = P.g.jr1;
  const unsigned slice = blockIdx.z;
  const bool owner = blockIdx.z == 0;
#include "k_thomas_corr.inc"
}
// ... over all segments of a tall column at once: blockIdx.z = segment * nslice + slice; P.gath / P.cgath = the summaries
// k_thomas_seg<.., 1, ..> has just written / the constants of the set-up, segment-major; T's np / nq / poff / qoff are
// the first segment's (the others' follow at QgThomasSegRec::tb0).  Every segment's slice 0 composes the chain for its own
// inflows; segment 0's publishes ksum (and ybnd).  grid: (nblk, nlayers, S * nslice), dynamic LDS as k_thomas_corr
__global__ __launch_bounds__(THC_NT) void k_thomas_corr_seg(const QgThomasParams P, const QgThomasCorr T0, const QgThomasSegRec *segs,
                                                            const int nslice) {
  const int rank = blockIdx.z / nslice;
  const unsigned slice = blockIdx.z - rank * nslice;
  const QgThomasSegRec sg = segs[rank];
  const QgThomasCorr T = {T0.ptab, T0.qtab, T0.np + sg.tb0, T0.nq + sg.tb0, T0.poff + sg.tb0, T0.qoff + sg.tb0};
  const int jr0 = sg.jr0, jr1 = sg.jr1;
  const bool owner = rank == 0 && slice == 0;
#include "k_thomas_corr.inc"
}

// set-up of the tables: how far a unit inflow reaches into the slab.  The work array holds PHASE 4's (from_top = 0:
// the response decays upwards from row 0) or PHASE 5's (from_top = 1: downwards from the last row) output, scaled by
// ftnorm; per block of TH_KW wavenumbers the number of rows up to the last one with an entry above tol.
// grid: (nblk, nlayers), 256 threads
__global__ __launch_bounds__(256) void k_thomas_reach(const QgThomasParams P, int from_top, double tol, int *reach) {
  __shared__ int smax[256];
  const int tid = threadIdx.x, kk = tid % TH_KW, c = tid / TH_KW;
  const int bx = blockIdx.x, m = blockIdx.y;
  const int nr = P.g.jr1 - P.g.jr0 + 1;
  const int k = bx * TH_KW + kk;
  const double *wb = P.wrk + P.g.wstride * m + (long)(P.g.jr0 - 1) * P.g.ldw + k;
  int far = 0; // rows counted from the end the inflow enters at
  if (k < P.g.nk)
    for (int r = c; r < nr; r += 256 / TH_KW) {
      const double v = wb[(long)r * P.g.ldw];
      if (!(fabs(v) <= tol)) { // (a NaN counts as "reaches")
        const int d = from_top ? nr - r : r + 1;
        far = d > far ? d : far;
      }
    }
  smax[tid] = far;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) smax[tid] = smax[tid] > smax[tid + s] ? smax[tid] : smax[tid + s];
    __syncthreads();
  }
  if (tid == 0) reach[m * P.nblk + bx] = smax[0];
}

// ... and the copy of those rows into the packed table, divided by ftnorm (the stored rows carry it, the tables do
// not: k_thomas_corr multiplies the inflows by it).  grid: (nblk, nlayers), 256 threads
__global__ __launch_bounds__(256) void k_thomas_pack(const QgThomasParams P, int from_top, const int *reach, const int *off,
                                                     double *tab) {
  const int tid = threadIdx.x, kk = tid % TH_KW, c = tid / TH_KW;
  const int bx = blockIdx.x, m = blockIdx.y;
  const int nr = P.g.jr1 - P.g.jr0 + 1;
  const int k = bx * TH_KW + kk;
  const int n = reach[m * P.nblk + bx];
  const int r0 = from_top ? nr - n : 0;
  const double *wb = P.wrk + P.g.wstride * m + (long)(P.g.jr0 - 1) * P.g.ldw + k;
  double *t = tab + (long)off[m * P.nblk + bx] * TH_KW + kk;
  for (int r = c; r < n; r += 256 / TH_KW) t[(long)r * TH_KW] = (k < P.g.nk) ? wb[(long)(r0 + r) * P.g.ldw] / P.ftnorm : 0.0;
}
