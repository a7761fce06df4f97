// k_tend_rows.h - K1 + K3 (forward) in one launch for the 5 km box ocean (nxto = 960): PV tendency, leapfrog and
// layer->mode projection by ROW BANDS, whose epilogue runs the forward DST-I of the band's rows.
//
// k_tend writes the modal right-hand side to wrk and k_dst64 reads it straight back (6 of the 25 fields the two
// launches move), across the longest kernel boundary of the step.  A workgroup that steps whole rows needs nothing from
// any other workgroup to transform them, so here
//
//   * one workgroup owns a band of B consecutive interior rows over the full width and all layers;
//   * phase 1 (tendency): each WAVE takes strips of TR_SW = 56 columns, lane = column with 4 halo lanes on either side
//     (the cascade Del^2 -> Del^4 -> Del^6 has radius 3; 4 keeps the owned columns starting on an odd column, so that the
//     even lane of a lane pair is 16-byte aligned for qg_pair_store_wt).  East / west neighbours come from DPP wave
//     shifts, north / south neighbours are the rows the lane holds in registers.  The wave walks the layers of its strip
//     one after the other (the loads of layer k+1 are requested before layer k is computed), keeps dqdt of all layers in
//     registers and finishes with the point-wise part (forcing, drag, leapfrog, projection) - the five-point sum, the
//     wall rule and the Jacobian are qg_ref_expr.h's, the point-wise expressions tend_point's, contraction off.  The new qo
//     leaves in 16-byte write-through pairs; the modal right-hand side fnot * qmm goes to LDS, one row per (row, mode).
//     A strip out of reach of every wall - all but 2 of 240 bands, all but 2 of 18 strips at NAtl 5 km - takes a body
//     without the wall rule, the clamps and the wall-column masks (k_tend_rows_strip.inc, one text included twice);
//   * ONE workgroup barrier;
//   * phase 2 (forward rows): the last B/2 x NL waves run dst64_front / dst64_back (k_dst64.h) on one (row pair, mode)
//     each, reading the rows from LDS, and store the spectral rows to wrk as k_dst64 does.  The transform buffer F of a
//     wave lies over the two right-hand-side rows that this wave alone reads: dst64_front has all its row loads in
//     registers before it writes F.  The tables of the front half are requested in FRONT of the barrier (see there).
// What a wave waits on: vmcnt counts loads and stores alike and retires them in order, and the compiler does not count
// the write-through stores (inline asm) - a wait it places for one load behind such a store waits for the store's
// acknowledgement too.  So no vector-memory wait stands between a strip's first store and its end, and none of phase
// 2's global loads behind the barrier (tests/test_band_rows_epilogue_asm.py reads both off the assembly).
// No workgroup waits for another one: no flags, no counters.
// The wall rows (not stepped: the new-qo buffer keeps qo) are copied by the first and the last band.
#pragma once
#include "k_tend.h"
#include "k_dst64.h"

#define TR_SW 56 // columns owned by a strip (64 lanes - 2 x 4 halo lanes)
#define TR_HL 4  // halo lanes on either side

// value of the lane to the west (lane - 1) / east (lane + 1); lanes 0 / 63 receive 0 (halo lanes)
template <int CTRL>
__device__ __forceinline__ double tr_dpp(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
#define TR_WEST(v) tr_dpp<0x138>(v) // wave_shr:1
#define TR_EAST(v) tr_dpp<0x130>(v) // wave_shl:1

// element at byte offset `off` (32-bit, per lane) behind the wave-uniform pointer `base`: keeps the address in the "scalar
// base + 32-bit lane offset" form of global_load (no 64-bit address arithmetic in VGPRs).  `base` is the pointer of ONE
// layer: the launcher refuses grids whose layer reaches 2^32 bytes (ny * ldx >= 2^29)
__device__ __forceinline__ double tr_ld(const double *base, unsigned off) {
  return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + off);
}

struct TrRules {
  bool isW, isE; // this lane is the W / E wall column
  int nyg;
  int vz; // 0, in a VGPR the compiler cannot see through
  double bcf, dxom2;
};

// Five-point operator of one row with the reference's mixed boundary rule (qg_ref_expr.h: interior sum, wall rule and
// which neighbour is the inner one; the corners follow the row rule, as the i2 / i4 offsets of k_tend_body.inc).  gj: row
// of c0 - the same in every lane, but held in a VGPR (TrRules.vz): on a scalar row number the compiler branches around
// each rule, and the web of blocks that makes of the unrolled cascade ends in scratch; on a vector one both rules are
// evaluated and selected, as k_tend_body.inc does.
__device__ __forceinline__ double tr_lap(const TrRules &R, double cS, double c0, double cN, int gj) {
  const double cW = TR_WEST(c0), cE = TR_EAST(c0);
  const double vi = qg_five_point(cS, cW, cE, cN, c0) * R.dxom2;
  const bool wS = gj == 1, wN = gj == R.nyg;
  double in = cW; // (a flat chain of selects, the last one wins: rows before columns, S before N)
  in = R.isW ? cE : in;
  in = wN ? cS : in;
  in = wS ? cN : in;
  const double vw = qg_wall_rule(R.bcf, in, c0);
  const bool wall = wS | wN | R.isW | R.isE;
  return wall ? vw : vi;
}
// the same operator where no wall is in reach: tr_lap's `vi`, which its last select returns there
__device__ __forceinline__ double tr_lap_interior(double dxom2, double cS, double c0, double cN) {
  const double cW = TR_WEST(c0), cE = TR_EAST(c0);
  return qg_five_point(cS, cW, cE, cN, c0) * dxom2;
}

// The kernel's arguments as the kernarg segment lays them out: where the by-value P lies in it.  A strip reads P's
// scalars and pointers from there (scalar loads, under its own arithmetic) instead of holding them in SGPRs from the
// kernel's head on: held, they and the band's row offsets are ~200 SGPRs the compiler spills to VGPR lanes before the first
// load is requested and moves back lane by lane inside every strip.
struct TrKernArgs {
  const double *pom; const double2 *twid; const double *sintab;
  int nx, ny, ldx, side;
  QgTendParams P;
};
typedef const __attribute__((address_space(4))) QgTendParams *TrParamPtr;
// a table in global memory that no kernel of a step writes (yporel), seen through the constant address space: scalar loads
typedef const __attribute__((address_space(4))) double *TrConstRow;

// Phase stamps (development builds only, -DQG_STAMPS; qgcm_dev.h, profiles/tools/stamps_band.py), kernel slot 3 of this
// translation unit's own table.  Thread 0 (wave 0, which has two strips at NAtl 5 km): 0 / 10 kernel entry, 1 first strip
// done, 2 last strip done, in front of the barrier.  Lane 0 of the first transform wave: 3 its strips done, 4 tables in,
// 5 past the barrier, 9 front half done, 6 transform done, 7 stores issued, 8 stores drained.
#ifdef QG_STAMPS
#define TR_STAMP(thread, i)                                                                                         \
  do {                                                                                                              \
    if (threadIdx.x == (thread) && blockIdx.x < QG_STAMP_BLOCKS) qg_stamps[3][blockIdx.x][i] = wall_clock64();       \
  } while (0)
// lane 0 of EVERY wave, kernel slots 1 / 0 of the table, one stamp per wave number: its first strip done / all its
// strips done, in front of the barrier - which wave the barrier waits for
#define TR_STAMP_W(kern, w)                                                                                         \
  do {                                                                                                              \
    static_assert(TrCfg<B>::NW <= QG_NSTAMP, "a stamp per wave");                                                   \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < QG_STAMP_BLOCKS) qg_stamps[kern][blockIdx.x][w] = wall_clock64();    \
  } while (0)
#else
#define TR_STAMP(thread, i) do { } while (0)
#define TR_STAMP_W(kern, w) do { } while (0)
#endif

#define TR_WAVES_PER_EU 3// the transform waves need ~146 VGPRs (k_dst64): three waves per SIMD
// rows per band.  Measured at NAtl 5 km: 2 (two six-wave workgroups per CU): 71.9 us per step, 4 (one
// twelve-wave workgroup per CU): 59.4; the parent 61.9.
constexpr int TR_BAND = 4;
template <int B>
struct TrCfg {
  static constexpr int NW = 3 * B;                 // waves per workgroup: three per SIMD at two (B = 2) / one (B = 4) workgroups per CU
  static constexpr int NT = 64 * NW;
  static constexpr int REG = 15 * D64_ROW * 2 + 128; // doubles per (row pair, mode): F (over the two rows), then W64
  static_assert(B % 2 == 0 && NT <= 1024, "whole row pairs; a workgroup has at most 1024 threads");
  static_assert((B / 2) * 3 * REG * 8 <= 160 * 1024, "three modes per row pair: the band's rows must fit the CU's 160 KB of LDS");
};

// grid: 8 * ceil(nbands / 8) workgroups of 64 * 3 B threads; whole-domain handle (joff = 0, rows 1..ny), NL = 3
template <int NL, int B, int ZM>
__global__ __launch_bounds__(TrCfg<B>::NT, TR_WAVES_PER_EU) void k_tend_rows(const double *pom, const double2 *twid, const double *sintab,
                                                                  int nx, int ny, int ldx, int side, const QgTendParams P) {
  TR_STAMP(0, 10);
  TR_STAMP(0, 0);
  constexpr int M = 15, N = 64 * M, NW = TrCfg<B>::NW, REG = TrCfg<B>::REG, NPW = B / 2;
  static_assert(B % 2 == 0 && NPW * NL <= NW, "a wave per (row pair, mode)");
  static_assert(2 * N <= M * D64_ROW * 2, "the two right-hand-side rows lie inside the transform buffer");
  constexpr bool ENT = !(ZM & 1), DDY = !(ZM & 2); // the field is read
  __shared__ __align__(16) double lds[NPW * NL * REG];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long fs = P.g.fstride;
  const int jr1 = ny - 1; // interior rows 2 .. ny - 1
  const int nbands = (jr1 - 1 + B - 1) / B;
  const int per_xcd = (nbands + 7) / 8;
  if ((side & 2) && blockIdx.x == 0 && tid == 0) constr_dpi_update<NL>(P.sc, P.tdto, P.gpoc); // see QgTendParams
  // XCD-aware numbering: each XCD (blockIdx mod 8) sweeps a contiguous run of bands, neighbours in time and in rows
  const int band = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (band >= nbands) return;
  const int j0 = 2 + band * B; // first row of the band
  const double *po0 = P.po, *qo0 = P.qo;

  // ---- wall rows (not stepped): the new-qo buffer keeps qo (qgosubs.F:214-219) -----------------------------------
  if (band == 0 || band == nbands - 1) {
#pragma unroll 1
    for (int w = 0; w < 2; ++w) {
      if ((w == 0 && band != 0) || (w == 1 && band != nbands - 1)) continue;
      const long ow = (long)(w == 0 ? 0 : ny - 1) * ldx;
      for (int i = tid; i < nx; i += TrCfg<B>::NT) {
#pragma unroll
        for (int k = 0; k < NL; ++k) P.qnew[fs * k + ow + i] = qo0[fs * k + ow + i];
      }
    }
  }

  TrRules R;
  R.nyg = ny; R.bcf = P.bcfaco; R.dxom2 = P.dxom2;
  asm volatile("v_mov_b32 %0, 0" : "=v"(R.vz));
  const double dxom2 = P.dxom2;

  // ---- phase 1: the tendency of the band, strip by strip ----------------------------------------------------------
  // Two bodies of one text (k_tend_rows_strip.inc), chosen per strip by a scalar branch.  A band is out of reach of the
  // wall ROWS iff every row on which the cascade forms the five-point operator is an interior row: the widest level,
  // Del^2, covers rows j0-2 .. j0+B+1 (with B = 4: band >= 1 && ny >= 4 band + 8; not "neither first nor last" - the band
  // before a short last band reaches row ny; a partial band never is).  A strip is out of reach of the wall COLUMNS iff
  // no lane of it is column 1 or nx.  At NAtl 5 km 2 of 240 bands and 2 of 18 strips take the body with the wall rule.
  const bool band_free = j0 - 2 >= 2 && j0 + B + 1 <= ny - 1;
  const int nstrips = (nx + TR_SW - 1) / TR_SW;
  // (TR_FENCE: a scheduling fence.  Left to itself the compiler requests the rows of all layers at once and forms every
  //  DPP shift of the Jacobian before the first product: 600 bytes of scratch per lane.  Between the fences the order is
  //  the one written in the strip body: the pom rows of layer k + 1 are requested once Del^2 of layer k has consumed those
  //  of layer k, its po / qo rows once the Jacobian has - so each request flies during the arithmetic that follows it,
  //  and a lane never holds more than one layer's rows.  TR_PIN: the value exists HERE - pure arithmetic is otherwise
  //  sunk past the fences to its use in the epilogue, and the DPP shifts it reads, which cannot move, stay live until then.)
#define TR_PIN(x) asm volatile("" : "+v"(x))
#define TR_STR_(x) #x
#define TR_STR(x) TR_STR_(x)
#define TR_FENCE()                       \
  do {                                   \
    asm volatile("" ::: "memory");       \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
#pragma unroll 1
  for (int strip = wv; strip < nstrips; strip += NW) {
    // What does not change from strip to strip is made to look as if it did (an empty asm the compiler cannot see
    // through): the band's first row - the row offsets are then formed on the scalar unit inside the strip instead of
    // being held, and spilled, across the loop - and the address of P in the kernarg segment (TrKernArgs above).
    int jb = j0;
    asm volatile("" : "+s"(jb));
    TrParamPtr pe = (TrParamPtr)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() +
                                 offsetof(TrKernArgs, P));
    asm volatile("" : "+s"(pe));
#define PE (*pe)
    const int g0 = strip * TR_SW + 1 - TR_HL; // column of lane 0
    const bool strip_free = g0 >= 2 && g0 + 63 <= nx - 1;
    if (band_free && strip_free) {
#define TR_WALLS 0
#include "k_tend_rows_strip.inc"
#undef TR_WALLS
    } else {
#define TR_WALLS 1
#include "k_tend_rows_strip.inc"
#undef TR_WALLS
    }
#undef PE
    if (strip < NW) {
      TR_STAMP(0, 1);
      TR_STAMP_W(1, wv);
    }
  }
#undef TR_FENCE
  TR_STAMP(0, 2);
  TR_STAMP_W(0, wv);
  // ---- phase 2: forward DST-I of the band's rows, a wave per (row pair, mode), as k_dst64 --------------------------
  // The transforms run on the LAST NPW * NL waves: with 18 strips on 12 waves those have one strip, reach the barrier
  // a strip ahead of the others, and the acknowledgements of their write-through stores are long in.  What the front
  // half reads from global tables - twid[lane], this wave's W64 row, the dsint sine factors: no address depends on
  // phase 1 - they request HERE, in front of the barrier, and write W64 to LDS (past the two right-hand-side rows of
  // their region, which phase 1 is still filling).  Behind the barrier these loads were a global round trip on the
  // critical path of every band, queued - vmcnt retires in order - behind whatever stores the wave still had in flight;
  // stand-alone k_dst64 never sees it (there the tables travel with the row loads).  The LDS region and the (pair, mode)
  // follow from the transform index tx, not from the wave number.  Every wave reaches the barrier exactly once; a
  // transform wave whose pair is absent (a partial last band) has requested its tables like the others and leaves.
  constexpr int TW0 = NW - NPW * NL; // first transform wave
  static_assert(M * D64_ROW * 2 >= 2 * N && M * D64_ROW * 2 + 2 * 64 <= REG,
                "a region's W64 row lies past its two right-hand-side rows and inside the region");
  const int tx = wv - TW0; // = pair * NL + m; negative: a wave without a transform
  double *reg = lds + (tx < 0 ? 0 : tx) * REG;
  cplx *F = reinterpret_cast<cplx *>(reg);
  cplx *W64 = reinterpret_cast<cplx *>(reg + M * D64_ROW * 2);
  D64Tables<M> tab;
  if (tx >= 0) {
    TR_STAMP(64 * TW0, 3);
    dst64_tables<M>(twid, sintab, W64, lane, tab);
    // in hand before the barrier (the wait is hidden behind the other waves' second strip)
    TR_PIN(tab.w1.x);
    TR_PIN(tab.w1.y);
#pragma unroll
    for (int n1 = 0; n1 <= M / 2; ++n1) TR_PIN(tab.sn[n1]);
    TR_STAMP(64 * TW0, 4);
  }
#undef TR_PIN
#undef TR_STR
#undef TR_STR_
  __syncthreads();
  if (tx < 0) return;
  TR_STAMP(64 * TW0, 5);
  const int pair = tx / NL, m = tx - pair * NL;
  const int ja = j0 + 2 * pair;
  if (ja > jr1) return;
  const bool has_b = (ja + 1 <= jr1);
  double *rowa = P.wrk + P.g.wstride * m + (long)(ja - 1) * P.g.ldw;
  double *rowb = rowa + P.g.ldw;
  double rsa, rsb;
  dst64_front<M, true>(twid, sintab, reg, reg + N, has_b, F, W64, lane, &tab);
  TR_STAMP(64 * TW0, 9);
  dst64_back<M>(F, W64, lane, rsa, rsb);
  TR_STAMP(64 * TW0, 6);
  const double *raw = reg;
#include "k_dst64_store.inc"
  TR_STAMP(64 * TW0, 7);
  QG_STAMP_DRAIN();
  TR_STAMP(64 * TW0, 8);
}
