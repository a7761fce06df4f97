// qgcm_hip.hip - C ABI (include/qgcm_hip.h) over the gfx950 kernels.
//
// One HIP stream per handle; state stays resident in HBM; the q and p time
// levels rotate between two buffers each instead of being copied
// (reference: qom<-qo in src/qgosubs.F:201-206, pom<-po in src/ocisubs.F:392).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <vector>

#include "qgcm_dev.h"
#include "k_tend.h"
#include "k_dst.h"
#include "k_fft3.h"
// the row lengths with a three-stage plan: NAtl 1 km (4800), SOcn 5 km (4608), and two more for the tests
#ifndef FFT3_NT
#define FFT3_NT 256
#endif
// (4800 = 12 * 20 * 20: the cheap radix takes the stage with two rounds of butterflies - profiles/r4_fft_plan_4800.log)
#ifdef FFT3_4800_OLD // (A/B: the round-2 plan of the 4800-point rows)
#define QG_FFT3_PLANS(X) X(1, 15, 16, 20) X(2, 16, 16, 18) X(3, 16, 16, 16) X(4, 12, 15, 16)
#else
#define QG_FFT3_PLANS(X) X(1, 12, 20, 20) X(2, 16, 16, 18) X(3, 16, 16, 16) X(4, 12, 15, 16)
#endif
#include "k_dst64.h"
#include "k_thomas.h"
#include "k_misc.h"
#include "k_cyclic.h"
#include "k_rfft64.h"
#include "k_fft3_unpack.h"
#include "k_oml.h"
#include "k_aml.h"
#include "k_valids.h"
#include "k_monitors.h"
#include "k_atm_monitors.h"
#include "k_tavg.h"
#include "k_atm_tavg.h"
#include "k_cov.h"
#include "k_areacfl.h"
#include "k_qocdiag.h"
#include "k_setup.h"
#include "k_xforc.h"
#include "k_xforc_slab.h" // (the parameter structs; the kernels are k_xforc_slab.hip's)
#include "k_row_split.h"

// kernels that are templates on the number of layers: instantiated for nlo = 2 .. QGCM_HIP_MAXL (8); the fused fast
// paths (k_dst64_unpack, k_rfft64_unpack, k_rfft3_unpack, the riding constraint solves) stay with nlo <= 4
static_assert(QG_MAXL == 8, "QG_SWITCH_NL lists the cases");
#define QG_SWITCH_NL(nl, X, what)                    \
  switch (nl) {                                      \
    case 2: X(2); break;                             \
    case 3: X(3); break;                             \
    case 4: X(4); break;                             \
    case 5: X(5); break;                             \
    case 6: X(6); break;                             \
    case 7: X(7); break;                             \
    case 8: X(8); break;                             \
    default: QG_FAIL(what ": unsupported nlo");      \
  }

static thread_local char g_err[512] = "";

#define QG_FAIL(...)                             \
  do {                                           \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
    return 1;                                    \
  } while (0)

#define HIPCHECK(expr)                                                                          \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) QG_FAIL("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Device allocations held through QgBuf in this process (qgcm_hip_debug_live_allocs).
static std::atomic<long> g_live_blocks{0};
static std::atomic<size_t> g_live_bytes{0};

// Move-only owner of n elements of device memory (PINNED: of page-locked host memory, which is not counted above).
// Converts to T *, so kernel-parameter fills and launches read as with a raw pointer.  Every device or pinned
// allocation of the library is one of these: a member of the handle, or a local for scratch.  Members that point into
// memory owned elsewhere stay raw pointers and say so.
template <typename T, bool PINNED = false>
class QgBuf {
  T *p_ = nullptr;
  size_t n_ = 0;

 public:
  QgBuf() = default;
  QgBuf(QgBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  QgBuf &operator=(QgBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~QgBuf() { reset(); }
  operator T *() const { return p_; }
  size_t size() const { return n_; }
  // frees; the caller has made sure that no launch still uses the memory
  void reset() {
    if (!p_) return;
    if (PINNED) (void)hipHostFree(p_);
    else {
      (void)hipFree(p_);
      g_live_blocks -= 1;
      g_live_bytes -= n_ * sizeof(T);
    }
    p_ = nullptr, n_ = 0;
  }
  // n elements in place of what was held, device memory zeroed; a failure names `what` and the bytes
  int alloc(size_t n, const char *what) {
    reset();
    const size_t bytes = n * sizeof(T);
    const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError(); // (the runtime's sticky error: later calls must not report it)
      p_ = nullptr;
      QG_FAIL("allocating %s (%zu bytes, %.2f GB) failed", what, bytes, bytes / 1e9);
    }
    if (!p_) return 0; // (nothing asked for)
    n_ = n;
    if (PINNED) return 0;
    g_live_blocks += 1;
    g_live_bytes += bytes;
    // The zero fill runs on the NULL stream, and a device memset need not have finished when hipMemset returns; the
    // handle's stream is non-blocking (not ordered against the null stream), so work queued on it right after an
    // allocation - the copy in qgcm_hip_set_thomas_consts, the all-gather in qgcm_hip_comm_init - could be overtaken
    // by the fill and zeroed. Seen as wrong slab constants with three one-process-per-slab ranks. Wait for the fill.
    HIPCHECK(hipMemset(p_, 0, bytes));
    HIPCHECK(hipStreamSynchronize(nullptr));
    return 0;
  }
  int ensure(size_t n, const char *what) { return p_ ? 0 : alloc(n, what); }           // allocated on first use
  int grow(size_t n, const char *what) { return p_ && n <= n_ ? 0 : alloc(n, what); }  // reallocated when too small
};
typedef QgBuf<double> QgDbl;

// a pair of scratch events of one call, destroyed at scope exit
struct QgEventPair {
  hipEvent_t a = nullptr, b = nullptr;
  int create() {
    HIPCHECK(hipEventCreate(&a));
    HIPCHECK(hipEventCreate(&b));
    return 0;
  }
  ~QgEventPair() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
};

#include "slab_comm.h"

enum { KN_TEND = 0, KN_BSUMS, KN_DSTF, KN_THOMAS, KN_DSTI, KN_CONSTR, KN_UNPACK, KN_OCQBDY, KN_LFAVG, KN_OML, KN_OML_ENTOC, KN_NOOP, KN_NOOP_TRAIN, KN_POAVG, KN_TAVAT, KN_COV, KN_AML, KN_AML_ENTAT, KN_COUNT };
// (k_oml = k_oml_step, the sst step + raw entrainment; k_oml_entoc = the entrainment on the p grid; k_aml = k_aml_step)
static const char *kKernelNames[KN_COUNT] = {"k_tend",   "k_cyc_bsums", "k_dst_fwd", "k_thomas", "k_dst_inv",
                                             "k_constr", "k_unpack",  "k_ocqbdy", "k_lf_average", "k_oml", "k_oml_entoc", "k_noop", "k_noop_train",
                                             "k_poavg_add", "k_tavat_accum", "k_cov", "k_aml", "k_aml_entat"};

// Device copy of the Thomas pivot tables of one set of diagonals (see QgThomasParams / build_pivots).
struct QgThomasTab {
  QgDbl binf, ptab;
  QgBuf<int> rcb, poff;
};

// A schedule: step s is due when every > 0 and s % every == phase.
struct QgSched { int every = 0, phase = 0; };
static const int kNeverDue = 1 << 30;
static bool sched_due(QgSched k, int s) { return k.every > 0 && s % k.every == k.phase; }
// due steps among s0 .. s0+n-1
static long sched_count(QgSched k, int s0, int n) {
  if (k.every <= 0 || n <= 0) return 0;
  auto upto = [k](long x) { return x < k.phase ? 0L : (x - k.phase) / k.every + 1; }; // due steps in 0..x
  return upto((long)s0 + n - 1) - upto((long)s0 - 1);
}
// steps from s to the next due step (0: s is due; kNeverDue without a schedule)
static int sched_dist(QgSched k, int s) { return k.every > 0 ? (k.phase - s % k.every + k.every) % k.every : kNeverDue; }
// the (every, phase) a caller `who` asks for into k
static int sched_set(QgSched &k, int every, int phase, const char *who) {
  if (every < 0) QG_FAIL("%s: every = %d (need >= 0; 0 removes the schedule)", who, every);
  if (every > 0 && (phase < 0 || phase >= every)) QG_FAIL("%s: phase = %d outside [0, %d)", who, phase, every);
  k.every = every;
  k.phase = every > 0 ? phase : 0;
  return 0;
}
enum { SCH_DUMP = 0, SCH_TAVATM, SCH_COV, SCH_COUNT };

struct qgcm_hip_ctx {
  qgcm_hip_params prm;
  QgGeom g;
  int device;
  hipStream_t stream = nullptr;
  QgDbl p[2], q[2];
  int ip, iq; // p[ip] = po, p[ip^1] = pom ; q[iq] = qo, q[iq^1] = qom
  QgDbl wekpo, entoc, ddynoc, ochom, yporel;
  QgDbl rspl; // sponge-layer ramp r_spl (qgcm_hip_set_sponge), or empty
  double c1_spl = 0.0;
  QgDbl wrk, rowsum;
  QgDbl ybnd;                              // cyclic y-slabs: (2, nl) zonal-mean solution next to the zonal boundaries (k_thomas PHASE 2)
  const double *slab_gath = nullptr;       // not owned - cyclic y-slabs: the gathered step messages of the last thomas phase 2
  int slab_nranks = 1;
  const double *oml_gath = nullptr;        // not owned - y-slabs: the gathered sums of the mixed layer's stage 10 (3, nranks)
  // The Thomas solve's plan and tables (build_thomas_tables).  The plan cuts the interior rows into S >= 1 segments: one
  // for every column up to 2048 rows (the single-segment kernels k_thomas / k_thomas_corr; the plan of one segment is
  // the slab itself), more for a taller ocean - a whole-domain handle's (k_thomas.h: k_thomas_seg, k_thomas_corr_seg)
  // or a y-slab's (k_thomas_slab.h: the segments folded into the slab's one summary).  Per set of diagonals - [0] the
  // modal solves of set_grid, [1] the last qgcm_hip_helmholtz - every segment's pivot tables, response tables and
  // constants, segment-major.  With S = 1 a set holds its pivots and, in [0], meta and the two response tables (a
  // single row towards a side without a neighbour); the slab's constants are slabDE itself.
  struct {
    int S = 1, R = 0, maxlen = 0;           // segments, rows per thread of the Thomas kernel (its chunk), longest segment
    int seg_rows = 0;                       // QGCM_HIP_THOMAS_SEG_ROWS (a y-slab: .._SLAB_SEG_ROWS) as set_grid read it (0: unset)
    std::vector<int> first, count;          // interior rows [first, first + count) of each segment
    QgDbl msg;                              // S > 1: (Cf, Cb, S0) of every segment, segment-major: the gathered slab messages' layout
    QgDbl coef, ab;                         // S > 1: the slab phases of the modal solves (QgThomasFold): (delta, eps, gamma) of
                                            // the set-up and (alpha, beta) of the last phase 1, (S, nl, ldw) each
    struct Set {
      QgThomasTab tab;                      // pivots
      QgBuf<QgThomasSegRec> recs;           // S > 1
      QgDbl ptab, qtab, cst;                // responses; S > 1: (D, E, SP, SQ) segment-major (cgath's layout)
      QgBuf<int> meta;                      // np, nq, poff, qoff: (nblk, layers, S) each
      std::vector<double> boc;              // [1], S > 1: the diagonal the tables were built for
    } set[2];
  } seg;
  QgDbl slabDE;                            // y-slab summary constants (D, E, SP, SQ) per (mode, wavenumber)
  QgDbl th_cgath;                          // all ranks' slabDE (rank-major), exchanged once (qgcm_hip_set_thomas_consts)
  int th_cgath_ranks = 0;
  QgDbl ksum, wcot;                        // spectral column sums of the solution and their cot weights (k_thomas.h)
  QgDbl bpart;                             // cyclic: partial boundary line sums (k_tend's extra workgroups -> constraint algebra)
  QgBuf<QgConstrParams> d_boxq;            // box: device copy of the constraint parameters (generic inverse rows' extra workgroup)
  QgBuf<QgCycConstrParams> d_cycq;         // cyclic: device copy of the constraint parameters (fused step path)
  QgDbl pch1, pch2, pbh;
  QgBuf<QgScalars> sc;
  QgBuf<double2> twid;
  QgDbl sintab;
  int fftN, nfac, fac[QG_MAXFAC]; // fftN = nxto; the factors (and dst_single, dst_lds, fft3 below) belong to the length the
                                  // row kernels transform: nxto, or split.L on a handle that splits its rows
  // Cyclic ocean rows longer than one LDS buffer (nxto > 5104, or QGCM_HIP_ROW_SPLIT; k_row_split.h): the
  // plan nxto = P * L of qgcm_hip_row_split, the table exp(-2 pi i t / L) of the sub-transforms and the scratch array
  // of wrk's size - both allocated on handles that split only.  P = 1: the rows are transformed whole.
  struct {
    int P = 1, L = 0;
    QgBuf<double2> twid;
    QgDbl scr;
  } split;
  QgConstr cs;
  bool grid_set, homog_set;
  bool geom_set = false; // yporel / ddynoc are on the device (qgcm_hip_set_geometry or set_grid)
  bool whole; // the handle owns the whole domain (no y-slab neighbours)
  bool dst_single = false; // generic row kernels run single-buffer (in-place) stages
  int fft3 = 0;            // long rows: three-stage register-radix plan of k_fft3.h (0 = none; index into QG_FFT3_PLANS)
  size_t fft3_lds = 0;
  bool force_generic_dst; // QGCM_HIP_GENERIC_DST=1: use the generic Stockham row kernel (A/B + tests)
  bool no_fused_unpack;   // QGCM_HIP_NO_FUSED_UNPACK=1: separate inverse transform and unpack launches (A/B + tests)
  int cu_first = 0, cu_count = 0; // qgcm_hip_set_cu_range: the CUs this handle's stream may use (0: all)
  bool no_fused_avg;      // QGCM_HIP_NO_FUSED_AVG=1: leapfrog averaging as a launch of its own inside qgcm_hip_steps (A/B + tests)
  bool no_fused_constr;   // QGCM_HIP_NO_FUSED_CONSTR=1: keep the k_constr_box launch inside qgcm_hip_steps (A/B + tests)
  bool tend_wide;         // QGCM_HIP_TEND_WIDE=1: the tendency kernel's HBM-bound instantiation (32-wide tiles, plain stores) at any size (tests)
  // The device buffer holds +0.0 everywhere (bit patterns: -0.0 does not count), known on the host: set by the zero fill
  // of the allocation and by the scan of every host array handed in (set_forcing; set_geometry / set_grid), cleared by
  // every device-side writer of entoc (the mixed layers).  tend_zmask turns them into k_tend_z's ZM.
  bool entoc_zero = false, ddynoc_zero = false;
  bool no_band_rows;      // QGCM_HIP_NO_BAND_ROWS=1: the 5 km step keeps k_tend + k_dst64 instead of the row-band kernel k_tend_rows (A/B + tests)
  bool beside = false;    // qgcm_hip_coupled_steps: an atmosphere handle steps beside this ocean on the same GPU (step_plan: band_rows)
  bool read_zero_fields;  // QGCM_HIP_READ_ZERO_FIELDS=1: the tendency kernel reads entoc and ddynoc whatever they hold (A/B + tests)
  std::vector<double> bd2oc;
  // profiling
  hipError_t timer_err = hipSuccess;
  int timer_err_at = 0;
  bool profiling;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> evpool; // pairs, drained once per step (no host sync between kernels)
  std::vector<int> evkid;
  double kms[KN_COUNT];
  int klaunch[KN_COUNT];
  // graphs keyed by (ip, iq, phase)
  struct GraphEntry { hipGraphExec_t exec; unsigned long used; }; // used: the steps_impl call that last replayed it
  std::map<long long, GraphEntry> graphs;
  unsigned long graph_call = 0;
  int avg_period = 25; // time levels are averaged after steps s with (s-1) mod avg_period == 0: ocean 25, atmosphere 100
  // ocean mixed layer (qgcm_hip_oml_init): three rotating sst buffers (is = sst, ism = sstm, spare = 3-is-ism)
  struct {
    bool on = false;
    qgcm_hip_oml_params prm;
    int ldt = 0, is = 0, ism = 1, nblkA = 0, nblkB = 0;
    QgDbl sst[3];
    QgDbl fnet, wekto, xfo, taux, tauy;
    QgDbl partA, partB, diag;
  } oml;
  // atmospheric mixed layer (qgcm_hip_aml_init, k_aml.h; atmosphere handles): ast and hmixa in three rotating buffers
  // each (ia = the current level, iam = the lagged one, spare = 3-ia-iam); atmon.ast / atmon.hmixa always point at the
  // current ones, so every diagnostic reads the stepped fields.  fnetat is tav.fnet, wekta / uekat / vekat are atmon's.
  struct {
    bool on = false;
    qgcm_hip_aml_params prm;
    int ldt = 0, ia = 0, iam = 1, nblkA = 0, nblkB = 0;
    QgDbl ast[3], hm[3];
    QgDbl xfa, xc1, dtop, partA, partB, diag;
  } aml;
  // validity scan (qgcm_hip_valids): partials, results, optional bottom topography
  QgDbl val_part, val_out, dtopoc;
  QgDbl val_sum, prs_out; // y-slab prsamp: this rank's valids summary (sst), combined result
  QgDbl area_part, area_out; // trapezoid area integrals of po, pom, qo (k_setup.h)
  // ocean monitors (qgcm_hip_monitors, k_monitors.h): constants, the fields that do not evolve on the device without
  // the mixed layer (qgcm_hip_set_monitor_fields), partials and the pinned result, all allocated on first use
  struct {
    bool prm_set = false;
    qgcm_hip_mon_params prm;
    int ldt = 0;
    QgDbl taux, tauy, wekto, sst;
    QgDbl psum, pmin, ujet, out;
    QgBuf<double, true> hout; // pinned host copy of out
  } mon;
  // atmosphere monitors and valids (qgcm_hip_atm_monitors / _atm_valids, k_atm_monitors.h): constants, the fields
  // xforc / aml leave on the host (qgcm_hip_set_atm_monitor_fields), partials and the pinned result
  struct {
    bool prm_set = false;
    qgcm_hip_atm_mon_params prm;
    int ldt = 0;
    QgDbl wekta, tauxa, tauya, uekat, vekat;
    // what every diagnostic reads, not owned: ast_own / hmixa_own (the fields of qgcm_hip_set_atm_monitor_fields) until
    // qgcm_hip_aml_init, the mixed layer's current level from then on (aml_set_idx)
    double *ast = nullptr, *hmixa = nullptr;
    QgDbl ast_own, hmixa_own;
    QgDbl psum, pmin, chain, out;
    QgBuf<double, true> hout; // pinned host copy of out
  } atmon;
  // running mean of po (qgcm_hip_poavg_enable, k_tavg.h): the sum over the owned rows and its count; while `on`
  // every step of qgcm_hip_steps / the slab stage 2 adds its po before the leapfrog averaging
  struct {
    bool on = false;
    QgDbl sum;
    long n = 0;
  } poavg;
  // tavocn / tavatm and tavout (qgcm_hip_tavocn / _tavatm, k_tavg.h, k_atm_tavg.h) for the handle's fluid: sums (the
  // atmosphere's in the ocean's layout), means (allocated on first use), fnetoc without the mixed layer / fnetat
  struct {
    bool prm_set = false;
    qgcm_hip_tav_params prm; // (ocean only: the atmosphere's hmat comes with qgcm_hip_set_atm_mon_params)
    QgDbl sum, mean, fnet;
    long n = 0;
  } tav;
  // covariance matrices (qgcm_hip_cov_*, k_cov.h): covini's state for the handle's fluid - the packed rows [k0, k1)
  // of the p and T matrices this handle holds, both means, the deviation vectors, this handle's row-sum part, the
  // counts nunit / sumwt of dssp (host) and the combine's status word
  struct {
    int nsi = 0, nbx = 0, nby = 0, nvar = 0;
    bool nt = false; // non-temporal loads / stores in k_cov_rank1 (matrices past the Infinity Cache, QGCM_HIP_COV_NT)
    long nmat = 0, k0 = 0, k1 = 0, part_len = 0;
    QgDbl mat[2], mean[2], dev[2];
    QgDbl part;
    QgBuf<int> status;
    long nu[2] = {0, 0};
    double swt[2] = {0.0, 0.0};
  } cov;
  // area averages and CFL check (qgcm_hip_areavg* / qgcm_hip_cfl*, k_areacfl.h): the tables of qgcm_hip_areavg_init
  // (tab.n = 0: not set up), the row sums and the result; the CFL partials and result, allocated on first use
  struct {
    QgAravParams tab = {};
    QgDbl rows, out;
    QgDbl cfl_part, cfl_out;
  } ac;
  // periodic dumps (qgcm_hip_qocdiag / _ocnc_sample / _atnc_sample, k_qocdiag.h): device result buffer (grown on
  // demand); the scheduled dump of qgcm_hip_qocdiag_schedule: a ring of `cap` snapshots of `len` doubles, oldest at `head`
  struct {
    QgDbl buf;
    int nsko = 0, cap = 0, head = 0, count = 0;
    size_t len = 0;
    QgDbl ring;
    std::vector<int> steps; // step number of each ring slot
  } qd;
  // what qgcm_hip_steps does on its own at scheduled steps: the dump of qgcm_hip_qocdiag_schedule inside the step, the
  // contributions of qgcm_hip_tavatm_schedule and qgcm_hip_cov_schedule after it, in this order
  QgSched sched[SCH_COUNT];
  // momentum half of xforc (qgcm_hip_xforc_init, k_xforc.h), held by the ATMOSPHERE handle: the constants, the ocean
  // handle it was set up with (or nullptr: atmos_only), the scratch (coarse velocities, the fine stress and the fine
  // Ekman velocity), the transposed weight tables and the two events that order the streams
  struct {
    bool on = false, coupled = false; // coupled: qgcm_hip_coupled_steps calls xforc before every ocean step
    bool slab = false;                // set up by qgcm_hip_xforc_slab_init: `oc` is a y-slab, this atmosphere a replica
    qgcm_hip_xforc_params prm;
    qgcm_hip_ctx *oc = nullptr; // not owned
    int ldf = 0, ldtf = 0;
    bool wekpa_stage = false; // wekpa by k_xf_wekpa_stage: ndxr above 64, or QGCM_HIP_XF_WEKPA_STAGE=1
    QgDbl u1at, v1at, txf, tyf, wf, tab;
    hipEvent_t ev_oc = nullptr, ev_atm = nullptr;
    // heat half (qgcm_hip_xforc_heat_init): constants, the two fsprim tables, bilint's index / weight tables, the
    // per-cell sums above the ocean, the partial sums of the four monitors and their results
    struct {
      bool on = false;
      qgcm_hip_xforc_heat_params prm;
      QgDbl fsa, fso, wx, wy, cell, part, scal;
      QgBuf<int> ix, iy;
      int nblkL = 0;
    } heat;
    // heat half without an ocean (qgcm_hip_xforc_sst_init; atmos_only): the prescribed SST (nxaooc*ndxr, nyaooc*ndxr)
    // with its own pitch and the spacing of its grid.  The constants, tables, sums and results are `heat`'s, whose
    // `on` stays false: the two set-ups exclude each other (xf.oc != nullptr / == nullptr).
    struct {
      bool on = false;
      int ldt = 0;
      double dxo = 0.0, dyo = 0.0;
      QgDbl sst;
    } sst;
    // banded mode of the slab set-up (qgcm_hip_xforc_slab_bands): this rank's band and windows, the common
    // row count of the message and the rank count the plan was made for
    struct {
      bool on = false, poison = false; // poison: QGCM_HIP_XF_POISON=1 - NaN bytes into the fine arrays before every part
      int nranks = 0;
      qgcm_hip_xforc_band plan;
    } bands;
    // tau_udiff on a slab set-up (qgcm_hip_xforc_slab_udiff): the basin's pom(:,:,1) assembled from every
    // rank's owned rows (nxpo, nyg; pitch ld), the common row count of the message and the rank count; fresh: an
    // assemble has run since the last qgcm_hip_xforc_slab_part
    struct {
      bool on = false, fresh = false, poison = false; // poison: QGCM_HIP_XF_POISON=1 - NaN bytes before every assemble
      int nrow = 0, nranks = 0, ld = 0;
      QgDbl pom;
    } udiff;
    // tau_udiff by owner-computed sums (qgcm_hip_xforc_slab_sums): this rank's part of the ownership plan
    // and the rank count; the basin-sized array is udiff.pom (udiff.on stays false: the modes exclude each other), of
    // which an edge assemble fills rows g0 - 4 .. g1 + 4; fresh: one has run since the last qgcm_hip_xforc_slab_part
    struct {
      bool on = false, fresh = false, poison = false; // poison: QGCM_HIP_XF_POISON=1 - NaN bytes before every assemble / part
      int rank = 0, nranks = 0;
      qgcm_hip_xforc_sum plan;
    } sums;
  } xf;
  // y-slab exchanges over RCCL (qgcm_hip_comm_init); slab-step graphs keyed like `graphs`
  QgSlabComm *sc_comm = nullptr;
  QgSlabCoupled *sc_cpl = nullptr; // the coupled window's exchange buffers (qgcm_hip_slab_coupled_init)
  std::map<long long, hipGraphExec_t> slab_graphs;
  bool slab_graph_mode = false; // QGCM_HIP_SLAB_GRAPH=1: capture 50 distributed steps (collectives included)
  size_t dst_lds;

  qgcm_hip_ctx() = default;
  qgcm_hip_ctx(const qgcm_hip_ctx &) = delete;
  // What is not memory.  The stream is drained first and the communicator goes before its buffers (~QgSlabComm); the
  // members then free the memory, after the stream has gone idle.
  ~qgcm_hip_ctx() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto &kv : graphs) hipGraphExecDestroy(kv.second.exec);
    for (auto &kv : slab_graphs) hipGraphExecDestroy(kv.second);
    delete sc_comm;
    delete sc_cpl;
    if (xf.ev_oc) hipEventDestroy(xf.ev_oc);
    if (xf.ev_atm) hipEventDestroy(xf.ev_atm);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    for (hipEvent_t e : evpool) hipEventDestroy(e);
    if (stream) hipStreamDestroy(stream);
  }
};

static const int kGraphBlock = 50; // steps per captured block (qgcm_hip_steps: get_graph; y-slabs: qgcm_hip_slab_steps)

extern "C" const char *qgcm_hip_last_error(void) { return g_err; }
extern "C" int qgcm_hip_abi_version(void) { return QGCM_HIP_ABI_VERSION; }

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Captured step graphs hold kernel parameters by value and raw device pointers: every call that changes
// either (tables, homogeneous solutions, mixed-layer parameters, slab constants) drops them.
// The stream is drained even when no graph exists: the callers go on to overwrite device tables with blocking copies
// on the null stream, which the handle's non-blocking stream does not wait for - eager steps still in flight would
// read half-updated tables (all callers are set-up calls: the wait costs nothing that matters).
static void drop_graphs(qgcm_hip_ctx *c) {
  (void)hipStreamSynchronize(c->stream);
  if (c->graphs.empty() && c->slab_graphs.empty()) return;
  for (auto &kv : c->graphs) hipGraphExecDestroy(kv.second.exec);
  for (auto &kv : c->slab_graphs) hipGraphExecDestroy(kv.second);
  c->graphs.clear();
  c->slab_graphs.clear();
}

static int factorize(int n, int *fac) {
  int nf = 0;
  static const int tr[5] = {8, 4, 2, 3, 5}; // fewest passes through LDS (FFTPACK's own order is 4,2,3,5)
  for (int t = 0; t < 5; ++t)
    while (n % tr[t] == 0) {
      fac[nf++] = tr[t];
      n /= tr[t];
    }
  for (int p = 7; n > 1; p += 2)
    while (n % p == 0) {
      fac[nf++] = p;
      n /= p;
    }
  return nf;
}

// pitched host <-> device copies of (nx, rows) Fortran blocks
static int upload2d(qgcm_hip_ctx *c, double *dst, int ld, const double *src, int nx, long rows) {
  HIPCHECK(hipMemcpy2DAsync(dst, (size_t)ld * 8, src, (size_t)nx * 8, (size_t)nx * 8, (size_t)rows,
                            hipMemcpyHostToDevice, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}
static int download2d(qgcm_hip_ctx *c, double *dst, const double *src, int ld, int nx, long rows) {
  HIPCHECK(hipMemcpy2DAsync(dst, (size_t)nx * 8, src, (size_t)ld * 8, (size_t)nx * 8, (size_t)rows,
                            hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// every element of a host array is +0.0 (bit patterns: -0.0 is not, the kernels' arithmetic tells the two apart)
static bool all_plus_zero(const double *a, size_t n) {
  unsigned long long any = 0;
  for (size_t i = 0; i < n; ++i) {
    unsigned long long b;
    memcpy(&b, a + i, sizeof(b));
    any |= b;
  }
  return any == 0;
}

// k_tend_z's mask for the next tendency launch: bit 0 = entoc, bit 1 = ddynoc need not be read (k_tend.h).  Every
// launch goes through launch_tend, which asks here; the graph keys carry the mask (get_graph, get_slab_graph).
static int tend_zmask(const qgcm_hip_ctx *c) {
  if (c->read_zero_fields || c->g.nl > 4) return 0;
  return (c->entoc_zero && !c->oml.on && !c->aml.on ? 1 : 0) | (c->ddynoc_zero ? 2 : 0);
}

// a host field a set_* call hands over (nullptr: not this time) into dst, allocated (ld, rows) on first use
static int upload_field(qgcm_hip_ctx *c, QgDbl &dst, int ld, const double *src, int nx, long rows) {
  if (!src) return 0;
  if (dst.ensure((size_t)ld * rows, "a field handed over by the host")) return 1;
  return upload2d(c, dst, ld, src, nx, rows);
}

extern "C" int qgcm_hip_create(qgcm_hip_handle *h, const qgcm_hip_params *prm, int device) {
  if (!h || !prm) QG_FAIL("qgcm_hip_create: null argument");
  *h = nullptr;
  if (prm->nlo < 2 || prm->nlo > QG_MAXL) QG_FAIL("qgcm_hip_create: nlo=%d outside 2..%d", prm->nlo, QG_MAXL);
  if (prm->nxpo < 4 || prm->nypo < 4) QG_FAIL("qgcm_hip_create: grid too small");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) QG_FAIL("qgcm_hip_create: no HIP device (%s) - there is no CPU fallback", hipGetErrorString(e));
  if (device >= 0) HIPCHECK(hipSetDevice(device));
  std::unique_ptr<qgcm_hip_ctx> c(new qgcm_hip_ctx()); // (a failure below leaves nothing behind, and *h null)
  memset(&c->prm, 0, sizeof(c->prm));
  c->prm = *prm;
  HIPCHECK(hipGetDevice(&c->device));
  QgGeom &g = c->g;
  g.nx = prm->nxpo; g.nl = prm->nlo; g.cyc = prm->cyclic;
  g.atm = prm->atmos ? 1 : 0;
  if (g.atm && !g.cyc) QG_FAIL("qgcm_hip_create: the atmosphere is a zonally periodic channel (atmos = 1 needs cyclic = 1)");
  if (g.atm) {
    c->avg_period = 100;   // src/q-gcm.F:1370
    c->prm.delek = 0.0;    // no drag layer and no Del-4th term in qgastep / atadif
    for (int k = 0; k < QG_MAXL; ++k) c->prm.ah2oc[k] = 0.0;
  }
  g.nyg = prm->nypo;
  {
    // y-slab view: owned global rows g0..g1 (+ 3 halo rows towards each neighbour)
    int g0 = prm->slab_g0, g1 = prm->slab_g1;
    if (g0 == 0 && g1 == 0) { g0 = 1; g1 = g.nyg; }
    if (g0 < 1 || g1 > g.nyg || g1 - g0 + 1 < 4) QG_FAIL("qgcm_hip_create: bad slab %d..%d of %d rows (need >= 4 rows)", g0, g1, g.nyg);
    const int hlo = g0 > 1 ? 3 : 0, hhi = g1 < g.nyg ? 3 : 0;
    g.ny = (g1 - g0 + 1) + hlo + hhi;
    g.joff = g0 - hlo - 1;
    g.jlo = hlo + 1;
    g.jhi = hlo + (g1 - g0 + 1);
    g.jr0 = (g0 == 1) ? g.jlo + 1 : g.jlo;       // rows 2..nyg-1 of the global grid that this slab owns
    g.jr1 = (g1 == g.nyg) ? g.jhi - 1 : g.jhi;
    c->whole = (g0 == 1 && g1 == g.nyg);
    if (prm->atmos && !c->whole) QG_FAIL("qgcm_hip_create: y-slabs are implemented for the oceans only");
  }
  g.nxt = g.nx - 1;
  g.nk = g.cyc ? g.nxt : g.nxt - 1;
  g.ldx = round_up(g.nx, 16);
  g.ldw = round_up(g.nxt + 1, 16);
  g.fstride = (long)g.ldx * g.ny;
  g.wstride = (long)g.ldw * g.ny;
  // Layout invariants of the 16-byte write-through pair stores (qg_store16_wt / qg_pair_store_wt, qgcm_dev.h): pairs
  // start on 16-byte boundaries (even pitches and strides), an odd row length leaves a padding column for the last
  // pair's second half, and the work array has one behind the last coefficient.  They hold for the pitches chosen
  // above; a later change of the layout must not break them silently.  (Row padding then holds garbage: nothing may
  // read or reduce over columns >= nx resp. >= nk.)
  if (g.ldx % 2 || g.ldw % 2 || g.fstride % 2 || g.wstride % 2 || (g.nx % 2 && g.ldx <= g.nx) || g.ldw <= g.nk)
    QG_FAIL("qgcm_hip_create: row pitches ldx=%d ldw=%d break the alignment / padding rules of the paired stores", g.ldx, g.ldw);
  if ((double)g.fstride * g.nl >= 2147483647.0 || (double)g.wstride * g.nl >= 2147483647.0)
    QG_FAIL("qgcm_hip_create: %ld x %d elements per field exceed the kernels' 32-bit element offsets", g.fstride, g.nl);
  HIPCHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t F = (size_t)g.fstride, W = (size_t)g.wstride;
  for (int i = 0; i < 2; ++i) {
    if (c->p[i].alloc(F * g.nl, "a time level of p")) return 1;
    if (c->q[i].alloc(F * g.nl, "a time level of q")) return 1;
  }
  c->ip = c->iq = 0;
  if (c->wekpo.alloc(F, "wekpo") || c->entoc.alloc(F, "entoc") || c->ddynoc.alloc(F, "ddynoc")) return 1;
  c->entoc_zero = c->ddynoc_zero = true; // (alloc fills with zeros)
  if (c->ochom.alloc(F * (g.nl - 1), "the homogeneous solutions")) return 1;
  if (c->yporel.alloc(g.ny, "yporel")) return 1;
  if (c->wrk.alloc(W * g.nl, "the spectral work array")) return 1;
  if (c->slabDE.alloc((size_t)4 * g.ldw * g.nl, "the slab constants")) return 1;
  if (g.cyc && c->ybnd.alloc(2 * QG_MAXL, "ybnd")) return 1;
  if (c->ksum.alloc((size_t)g.ldw * g.nl, "ksum")) return 1;
  if (c->wcot.alloc((size_t)g.ldw, "wcot")) return 1;
  if (c->bpart.alloc((size_t)5 * BSUM_NB * 2 * g.nl, "the boundary line sums")) return 1;
  if (c->rowsum.alloc((size_t)g.ny * g.nl, "the row sums")) return 1;
  if (c->pch1.alloc((size_t)g.ny * g.nl, "pch1") || c->pch2.alloc((size_t)g.ny * g.nl, "pch2") || c->pbh.alloc(g.ny, "pbh")) return 1;
  if (c->sc.alloc(1, "the step's scalars")) return 1;
  c->grid_set = c->homog_set = false;
  {
    const char *e = getenv("QGCM_HIP_GENERIC_DST");
    c->force_generic_dst = e && e[0] == '1';
    const char *f = getenv("QGCM_HIP_NO_FUSED_UNPACK");
    c->no_fused_unpack = f && f[0] == '1';
    const char *fc = getenv("QGCM_HIP_NO_FUSED_CONSTR");
    c->no_fused_constr = fc && fc[0] == '1';
    const char *tw = getenv("QGCM_HIP_TEND_WIDE");
    c->tend_wide = tw && tw[0] == '1';
    const char *fa = getenv("QGCM_HIP_NO_FUSED_AVG");
    c->no_fused_avg = fa && fa[0] == '1';
    const char *rz = getenv("QGCM_HIP_READ_ZERO_FIELDS");
    c->read_zero_fields = rz && rz[0] == '1';
    const char *br = getenv("QGCM_HIP_NO_BAND_ROWS");
    c->no_band_rows = br && br[0] == '1';
  }
  c->profiling = false;
  HIPCHECK(hipEventCreate(&c->ev0));
  HIPCHECK(hipEventCreate(&c->ev1));
  memset(&c->cs, 0, sizeof(c->cs));
  HIPCHECK(hipDeviceSynchronize()); // the zero fills above ran on the null stream
  *h = c.release();
  return 0;
}

extern "C" int qgcm_hip_destroy(qgcm_hip_handle c) {
  delete c; // (~qgcm_hip_ctx; a null handle is fine)
  return 0;
}

extern "C" int qgcm_hip_debug_live_allocs(long *blocks, size_t *bytes) {
  if (blocks) *blocks = g_live_blocks.load();
  if (bytes) *bytes = g_live_bytes.load();
  return 0;
}

// rows per thread the Thomas kernel is instantiated for; 10 / 20: the 600- and 1200-row slabs of NAtl 1 km
#define QG_TH_ROWS(X) X(1) X(2) X(4) X(8) X(10) X(12) X(16) X(20) X(24) X(32)
static int thomas_rows_per_chunk(int nrows) {
  const int need = (nrows + TH_NC - 1) / TH_NC;
#define QG_TH_FITS(RV) if (need <= RV) return RV;
  QG_TH_ROWS(QG_TH_FITS)
#undef QG_TH_FITS
  return -1;
}

// The segment plan of a column of nrows interior rows (pure host code): S = ceil(nrows / max) balanced segments, the
// first nrows % S one row longer.  max_rows <= 0: no maximum given - one segment up to QGCM_HIP_THOMAS_MAX_ROWS rows (the
// single-segment kernel), segments of at most QGCM_HIP_THOMAS_SEG_DEFAULT rows beyond (1024: 16 rows per thread, the
// 128-VGPR form - measured on NAtl 1 km against 2048 and 640).  A maximum below 2 * MIN - 1 could leave a
// segment shorter than the slab minimum (nrows = max + 1 gives two halves): refused.
extern "C" int qgcm_hip_thomas_segments(int nrows, int max_rows, int *nseg, int *first, int *count) {
  if (!nseg) QG_FAIL("qgcm_hip_thomas_segments: null argument");
  if (nrows < 1) QG_FAIL("qgcm_hip_thomas_segments: nrows = %d", nrows);
  int cap = QGCM_HIP_THOMAS_SEG_DEFAULT;
  if (max_rows > 0) {
    if (max_rows < 2 * QGCM_HIP_THOMAS_SEG_MIN - 1)
      QG_FAIL("qgcm_hip_thomas_segments: a maximum of %d rows per segment is below %d (segments of at least %d rows)", max_rows,
              2 * QGCM_HIP_THOMAS_SEG_MIN - 1, QGCM_HIP_THOMAS_SEG_MIN);
    cap = max_rows < QGCM_HIP_THOMAS_MAX_ROWS ? max_rows : QGCM_HIP_THOMAS_MAX_ROWS;
  }
  const int S = (max_rows <= 0 && nrows <= QGCM_HIP_THOMAS_MAX_ROWS) ? 1 : (nrows + cap - 1) / cap;
  if (S > QGCM_HIP_THOMAS_MAX_SEG)
    QG_FAIL("qgcm_hip_thomas_segments: %d rows in segments of at most %d rows are more than %d segments", nrows, cap, QGCM_HIP_THOMAS_MAX_SEG);
  *nseg = S;
  const int base = nrows / S, extra = nrows % S;
  for (int s = 0, at = 0; s < S; ++s) {
    const int n = base + (s < extra ? 1 : 0);
    if (first) first[s] = at;
    if (count) count[s] = n;
    at += n;
  }
  return 0;
}

extern "C" int qgcm_hip_thomas_plan(qgcm_hip_handle c, int *nseg, int *first, int *count) {
  if (!c || !nseg) QG_FAIL("qgcm_hip_thomas_plan: null argument");
  if (!c->grid_set) QG_FAIL("qgcm_hip_thomas_plan: the plan is made by qgcm_hip_set_grid");
  const int S = c->seg.S;
  *nseg = S;
  for (int s = 0; s < S; ++s) {
    if (first) first[s] = c->seg.first[s];
    if (count) count[s] = c->seg.count[s];
  }
  return 0;
}

// The generic row kernels' LDS (k_dst.h): two ping-pong buffers, or ONE buffer with in-place stages for long rows whose
// factors all have an in-place stage
static bool row_single_buffer(int N) {
  if (N < DST_SINGLE_MINN || N > DST_SINGLE_MAXN || N % 2) return false;
  int fac[64]; // (2^31 has 31 factors)
  const int nf = factorize(N, fac);
  for (int f = 0; f < nf; ++f)
    if (fac[f] != 2 && fac[f] != 3 && fac[f] != 4 && fac[f] != 5 && fac[f] != 8) return false;
  return true;
}
static size_t row_lds_bytes(int N, bool cyc, bool single) {
  if (single) return (size_t)N * sizeof(cplx) + 2 * (RFFT_NT / 64) * sizeof(double); // RFFT_NT == DST_NT_BIG
  return (size_t)2 * N * sizeof(cplx) + 2 * (cyc ? RFFT_NT : (N >= DST_BIG_N ? DST_NT_BIG : DST_NT)) * sizeof(double);
}
static const size_t kRowLdsMax = 160 * 1024;

// The row plan of a zonally cyclic ocean with rows of nxto points (pure host code): nxto = P * L, P interleaved
// sub-rows of length L per row (k_row_split.h).  forced_P <= 0: P = 1 up to DST_SINGLE_MAXN = 5104 points; beyond, the
// smallest P in 2 .. 5 that divides nxto and leaves an even L <= 5104 which the generic cyclic row kernel holds in LDS.
// forced_P > 0 (QGCM_HIP_ROW_SPLIT): that P, at any length, under the same conditions.
extern "C" int qgcm_hip_row_split(int nxto, int forced_P, int *P, int *L) {
  if (!P || !L) QG_FAIL("qgcm_hip_row_split: null argument");
  if (nxto < 2) QG_FAIL("qgcm_hip_row_split: nxto = %d", nxto);
  auto fits = [&](int p) {
    if (nxto % p) return false;
    const int l = nxto / p;
    return l % 2 == 0 && l <= DST_SINGLE_MAXN && row_lds_bytes(l, true, row_single_buffer(l)) <= kRowLdsMax;
  };
  if (forced_P > 0) {
    if (forced_P < 2 || forced_P > QGCM_HIP_ROW_SPLIT_MAX_P)
      QG_FAIL("qgcm_hip_row_split: QGCM_HIP_ROW_SPLIT=%d is outside 2 .. %d", forced_P, QGCM_HIP_ROW_SPLIT_MAX_P);
    if (nxto % forced_P) QG_FAIL("qgcm_hip_row_split: QGCM_HIP_ROW_SPLIT=%d does not divide nxto=%d", forced_P, nxto);
    if ((nxto / forced_P) % 2) QG_FAIL("qgcm_hip_row_split: QGCM_HIP_ROW_SPLIT=%d leaves sub-rows of an odd length %d (nxto=%d)", forced_P, nxto / forced_P, nxto);
    if (!fits(forced_P))
      QG_FAIL("qgcm_hip_row_split: QGCM_HIP_ROW_SPLIT=%d leaves sub-rows of %d points, more than the row kernels hold (<= %d)", forced_P, nxto / forced_P, DST_SINGLE_MAXN);
    *P = forced_P;
    *L = nxto / forced_P;
    return 0;
  }
  if (nxto <= DST_SINGLE_MAXN) {
    *P = 1;
    *L = nxto;
    return 0;
  }
  for (int p = 2; p <= QGCM_HIP_ROW_SPLIT_MAX_P; ++p)
    if (fits(p)) {
      *P = p;
      *L = nxto / p;
      return 0;
    }
  QG_FAIL("qgcm_hip_row_split: nxto=%d is longer than one row transform (<= %d points) and no P in 2 .. %d splits it into even sub-rows of at most %d points "
          "that the row kernels hold; supported: nxto = P * L with L even, L <= %d",
          nxto, DST_SINGLE_MAXN, QGCM_HIP_ROW_SPLIT_MAX_P, DST_SINGLE_MAXN, DST_SINGLE_MAXN);
}

extern "C" int qgcm_hip_row_plan(qgcm_hip_handle c, int *P, int *L) {
  if (!c || !P || !L) QG_FAIL("qgcm_hip_row_plan: null argument");
  if (!c->grid_set) QG_FAIL("qgcm_hip_row_plan: the plan is made by qgcm_hip_set_grid");
  *P = c->split.P;
  *L = c->split.P > 1 ? c->split.L : c->g.nxt;
  return 0;
}

// per-step message of one slab: the summaries of the two y sweeps; a cyclic ocean appends its boundary line sums
static inline size_t slab_msg_len(const QgGeom &g) {
  return (size_t)TH_MSG * g.nl * g.ldw + (g.cyc ? (size_t)5 * BSUM_NB * 2 * g.nl : 0);
}
// ... and, with the mixed layer on the device, the three sums of its entoc pass at the very end
static inline size_t slab_msg_len_oml(const qgcm_hip_ctx *c) { return slab_msg_len(c->g) + (c->oml.on ? 3 : 0); }
// halo message per direction: 3 rows of po + 1 row of qo per layer, + 3 rows of the new sst with the mixed layer on
static inline size_t halo_msg_len(const qgcm_hip_ctx *c) {
  return QG_HALO_LEN(c->g.nl, c->g.ldx) + (c->oml.on ? (size_t)3 * c->oml.ldt : 0); // (qg_ref_expr.h: the kernels' layout)
}

// Thomas pivots, exactly the recurrence of src/ocisubs.F:472-477 (box) / 577-582 (cyclic), run once on the host.
// The recurrence reaches a bitwise fixed point after a few rows for most spectral indices; per block of TH_KW indices
// the pivots of the local rows before the block's slowest index is stationary are tabulated (rows of TH_KW doubles),
// plus the stationary pivot per index.  Appends the tables of one layer (set of diagonals) to T.
struct ThomasTabHost {
  std::vector<double> binf, ptab;
  std::vector<int> rcb, poff;
};
static void build_pivots(const QgGeom &g, double aoc, const double *boc /* per spectral index */, ThomasTabHost &T) {
  const int nr = g.jr1 - g.jr0 + 1;         // rows of this slab
  const int rg0 = g.jr0 + g.joff - 2;       // global interior-row index of the slab's first row
  const int nblk = (g.nk + TH_KW - 1) / TH_KW;
  const size_t b0 = T.binf.size();
  T.binf.resize(b0 + g.ldw, 0.0);
  std::vector<double> piv((size_t)TH_KW * nr);
  for (int bx = 0; bx < nblk; ++bx) {
    int rcb = 1; // at least one row, so that the kernel's clamped table read is always in bounds
    std::fill(piv.begin(), piv.end(), 0.0);
    for (int kk = 0; kk < TH_KW; ++kk) {
      const int k = bx * TH_KW + kk;
      if (k >= g.nk) continue;
      double betinv = 1.0 / boc[k]; // global interior row 0
      int gconv = rg0 + nr;         // first global row whose pivot equals its predecessor's (bitwise)
      for (int rg = 0; rg < rg0 + nr; ++rg) {
        if (rg > 0) {
          double gam = aoc * betinv;
          double nb = 1.0 / (boc[k] - aoc * gam);
          if (nb == betinv && gconv == rg0 + nr) gconv = rg;
          betinv = nb;
        }
        if (rg >= rg0) piv[(size_t)(rg - rg0) * TH_KW + kk] = betinv;
      }
      T.binf[b0 + k] = betinv; // the stationary value (or, if never stationary, unused: rcb = nr then)
      int lc = gconv - rg0;
      lc = lc < 0 ? 0 : (lc > nr ? nr : lc);
      if (lc > rcb) rcb = lc;
    }
    T.rcb.push_back(rcb);
    T.poff.push_back((int)(T.ptab.size() / TH_KW));
    T.ptab.insert(T.ptab.end(), piv.begin(), piv.begin() + (size_t)rcb * TH_KW);
  }
}

// (re)allocates the device tables as needed and uploads T (blocking copies: T may die at the caller's scope exit)
static int upload_pivots(qgcm_hip_ctx *c, QgThomasTab &D, const ThomasTabHost &T) {
  HIPCHECK(hipStreamSynchronize(c->stream)); // no launch may still be reading the old tables
  if (D.binf.grow(T.binf.size(), "the stationary pivots") || D.ptab.grow(T.ptab.size(), "the pivot tables") ||
      D.rcb.grow(T.rcb.size(), "the pivot tables' row counts") || D.poff.grow(T.poff.size(), "the pivot tables' offsets"))
    return 1;
  HIPCHECK(hipMemcpy(D.binf, T.binf.data(), T.binf.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(D.ptab, T.ptab.data(), T.ptab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(D.rcb, T.rcb.data(), T.rcb.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(D.poff, T.poff.data(), T.poff.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// the y-slab arguments of a Thomas phase (qgcm_hip_thomas_phase); the default is a lone slab
struct QgThomasSlabArgs {
  const double *gath = nullptr; // phase 2: all ranks' gathered step messages
  double *send = nullptr;       // phase 1: this slab's message
  int rank = 0, nranks = 1;
};
static int launch_thomas(qgcm_hip_ctx *c, int which, int nlayers, int phase, const QgThomasSlabArgs &slab = {}, bool cyc_part_a = false);

static int launch_thomas_rows(qgcm_hip_ctx *c, const QgThomasParams &P, int phase, bool cyca, int nlayers, hipStream_t st);
static int launch_thomas_seg_rows(qgcm_hip_ctx *c, const QgThomasParams &P, const QgThomasSegRec *recs, int nlayers, hipStream_t st);
static int launch_thomas_seg(qgcm_hip_ctx *c, QgThomasParams &P, int which, int nlayers, hipStream_t st);
static int launch_thomas_slab_seg(qgcm_hip_ctx *c, QgThomasParams &P, int which, int phase, int nlayers, hipStream_t st);
// The kernels of a y-slab cut into segments and their launches live in k_thomas_slab.hip, a device code object of its
// own (as k_tend_rows.hip): this file compiles to the device code it had without them.
hipError_t qg_launch_thomas_fold(bool setup, hipStream_t st, const QgThomasFold &F);
hipError_t qg_launch_thomas_corr_slab(hipStream_t st, const QgThomasParams &P, const QgThomasCorr &T, const QgThomasSegRec *segs,
                                      const QgThomasFold &F, int nslice, int nlayers);
static QgThomasFold thomas_fold_params(const qgcm_hip_ctx *c, double *send);

// which: the set of diagonals (seg.set) whose pivots the solve reads; always the whole work array from its first layer
static void fill_thomas_params(qgcm_hip_ctx *c, QgThomasParams &P, int which, int nlayers) {
  const QgGeom &g = c->g;
  const QgThomasTab &tab = c->seg.set[which].tab;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.gath_stride = (long)slab_msg_len_oml(c);
  P.slabDE = c->slabDE;
  P.ksum = c->ksum;
  P.wrk = c->wrk;
  P.binf = tab.binf; P.ptab = tab.ptab; P.rcb = tab.rcb; P.poff = tab.poff;
  P.nblk = (g.nk + TH_KW - 1) / TH_KW;
  P.aoc = c->prm.aoc;
  P.ftnorm = g.cyc ? 1.0 / g.nxt : 0.5 / g.nxt; // src/ocisubs.F:440, 547
  P.nlayers = nlayers;
  P.layer0 = 0;
  P.nranks = 1;
}

// Set-up of the Thomas solve for one set of diagonals (which = 0: the modal solves, boc = nlo diagonals; 1:
// qgcm_hip_helmholtz's, one diagonal) under the handle's plan of S >= 1 segments; a plan of one segment is the slab
// itself.  Every segment's pivots - the recurrence depends on its first global row - go segment-major into the set's
// pivot tables.  A whole column solved in one piece with another diagonal (which = 1, S = 1) needs nothing else: PHASE 0
// has no inflows.  Otherwise PHASE 4 / 5 run once per segment (k_thomas.h: they give the segment's gain and response
// sums - with S = 1 straight into slabDE - and leave the responses Pv / Qv to unit inflows in the segment's own rows of
// the work array, which is overwritten), then the responses are tabulated per block of TH_KW wavenumbers as far as they
// reach (above 1e-19 of the inflow).  A segment's neighbours are the segments next to it, and at the slab's two ends the
// neighbouring ranks, where there are any; towards a side without a neighbour nothing ever enters: reach 0.  The modal
// set of S > 1 segments then folds the segments' constants into the slab's own (k_thomas_slab.h): slabDE and the
// per-segment coefficients of the slab phases - on a whole-domain handle too, which is a lone slab (nranks = 1) to
// qgcm_hip_thomas_phase.  (One segment is not folded: the fold of one is not bound to give PHASE 4 / 5's bits.)
static int build_thomas_tables(qgcm_hip_ctx *c, int which, const std::vector<std::vector<double>> &boc) {
  const QgGeom &g = c->g;
  auto &sg = c->seg;
  auto &ss = sg.set[which];
  const int S = sg.S, nlt = (int)boc.size(), nblk = (g.nk + TH_KW - 1) / TH_KW, nmt = nblk * nlt;
  std::vector<QgThomasSegRec> recs(S);
  {
    ThomasTabHost T;
    for (int s = 0; s < S; ++s) {
      QgGeom gs = g;
      gs.jr0 = g.jr0 + sg.first[s];
      gs.jr1 = gs.jr0 + sg.count[s] - 1;
      recs[s] = QgThomasSegRec{gs.jr0, gs.jr1, s * nmt, 0, (long)s * nlt * g.ldw, (long)s * TH_MSG * nlt * g.ldw, (long)s * TH_CST * g.nl * g.ldw};
      for (int m = 0; m < nlt; ++m) build_pivots(gs, c->prm.aoc, boc[m].data(), T);
    }
    if (upload_pivots(c, ss.tab, T)) return 1; // (waits for the stream: nothing reads the old tables any more)
  }
  if (which != 0 && S == 1) return 0;
  if (S > 1) { // (one segment: no device records, its summary is the slab's message and its constants are slabDE)
    if (sg.msg.ensure((size_t)TH_MSG * g.nl * g.ldw * S, "the segments' messages")) return 1;
    if (ss.cst.ensure((size_t)TH_CST * g.nl * g.ldw * S, "the segments' constants")) return 1;
    if (ss.recs.ensure(S, "the segment records")) return 1;
    HIPCHECK(hipMemcpy(ss.recs, recs.data(), sizeof(QgThomasSegRec) * S, hipMemcpyHostToDevice));
  }
  if (ss.meta.ensure((size_t)4 * S * nmt, "the segments' reach")) return 1;
  std::vector<int> meta((size_t)4 * S * nmt, 0);
  HIPCHECK(hipMemcpy(ss.meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice)); // (ends without a neighbour: reach 0)
  QgThomasParams P0;
  fill_thomas_params(c, P0, which, nlt);
  auto seg_params = [&](int s) {
    QgThomasParams P = P0;
    P.g.jr0 = recs[s].jr0; P.g.jr1 = recs[s].jr1;
    P.binf += recs[s].b0; P.rcb += recs[s].tb0; P.poff += recs[s].tb0;
    if (S > 1) P.slabDE = ss.cst + recs[s].cst0;
    return P;
  };
  const double tol = 1.0e-19 * P0.ftnorm; // three orders below the rounding of the inflow itself
  const bool nb_lo = g.joff + g.jlo > 1, nb_hi = g.joff + g.jhi < g.nyg; // a neighbouring rank below / above
  auto closed = [&](int side, int s) { return side ? (s == S - 1 && !nb_hi) : (s == 0 && !nb_lo); }; // nothing ever enters there
  for (int side = 0; side < 2; ++side) { // 0: inflow from below (PHASE 4, Pv), 1: from above (PHASE 5, Qv)
    QgDbl &rtab = side ? ss.qtab : ss.ptab;
    rtab.reset();
    int *d_reach = ss.meta + side * S * nmt, *d_off = ss.meta + (2 + side) * S * nmt;
    int *h_reach = meta.data() + side * S * nmt, *h_off = meta.data() + (2 + side) * S * nmt;
    for (int s = 0; s < S; ++s) {
      const QgThomasParams P = seg_params(s);
      if (launch_thomas_rows(c, P, 4 + side, false, nlt, c->stream)) return 1;
      if (closed(side, s)) continue;
      hipLaunchKernelGGL(k_thomas_reach, dim3(nblk, nlt), dim3(256), 0, c->stream, P, side, tol, d_reach + s * nmt);
      HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemcpyAsync(h_reach, d_reach, sizeof(int) * S * nmt, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    size_t off = 0;
    for (int i = 0; i < S * nmt; ++i) {
      h_off[i] = (int)off;
      off += h_reach[i];
    }
    // The kernels index the table with 32-bit offsets.  A block's reach is at most its segment's rows, so the table has
    // at most nblk * nlt * nrows rows of TH_KW doubles, and TH_KW * nblk <= ldw, nlt <= nlo, nrows < ny: fewer elements
    // than the ldw * ny * nlo of the work array, which qgcm_hip_create keeps below 2^31 - for one segment as for many,
    // this cannot trip on a grid the library accepts.
    if ((double)off * TH_KW >= 2147483647.0) QG_FAIL("qgcm_hip_set_grid: the segments' response tables exceed 32-bit offsets");
    if (rtab.alloc((size_t)TH_KW * (off ? off : 1), "the segments' response table")) return 1;
    HIPCHECK(hipMemcpyAsync(d_off, h_off, sizeof(int) * S * nmt, hipMemcpyHostToDevice, c->stream));
    for (int s = 0; s < S; ++s) {
      if (closed(side, s)) continue;
      const QgThomasParams P = seg_params(s);
      hipLaunchKernelGGL(k_thomas_pack, dim3(nblk, nlt), dim3(256), 0, c->stream, P, side, (const int *)(d_reach + s * nmt),
                         (const int *)(d_off + s * nmt), rtab);
      HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
  }
  if (which == 0 && S > 1) {
    const size_t per = (size_t)S * g.nl * g.ldw;
    if (sg.coef.ensure(3 * per, "the segments' fold coefficients") || sg.ab.ensure(2 * per, "the segments' inflows")) return 1;
    HIPCHECK(qg_launch_thomas_fold(true, c->stream, thomas_fold_params(c, nullptr)));
    HIPCHECK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

extern "C" int qgcm_hip_set_geometry(qgcm_hip_handle c, const double *yporel, const double *ddynoc) {
  if (!c || !yporel) QG_FAIL("qgcm_hip_set_geometry: null argument");
  const QgGeom &g = c->g;
  drop_graphs(c);
  HIPCHECK(hipMemcpy(c->yporel, yporel, sizeof(double) * g.ny, hipMemcpyHostToDevice));
  if (ddynoc) {
    c->ddynoc_zero = false; // (a failed copy leaves the buffer unknown)
    if (upload2d(c, c->ddynoc, g.ldx, ddynoc, g.nx, g.ny)) return 1;
    c->ddynoc_zero = all_plus_zero(ddynoc, (size_t)g.nx * g.ny); // (the row padding keeps the allocation's zeros; nothing reads it)
  }
  c->geom_set = true;
  return 0;
}

extern "C" int qgcm_hip_set_grid(qgcm_hip_handle c, const double *yporel, const double *bd2oc, const double *ddynoc) {
  if (!c || !yporel || !bd2oc) QG_FAIL("qgcm_hip_set_grid: null argument");
  const QgGeom &g = c->g;
  if (qgcm_hip_set_geometry(c, yporel, ddynoc)) return 1;
  c->bd2oc.assign(bd2oc, bd2oc + g.nxt);
  // Thomas diagonal + chunk-entry pivots per mode: boc = bd2oc - rdm2oc(m)   (src/ocisubs.F:148-150)
  // an ocean cuts a column of more than 2048 rows (or, with QGCM_HIP_THOMAS_SEG_ROWS - a y-slab: with
  // QGCM_HIP_THOMAS_SLAB_SEG_ROWS - set, any column longer than that) into segments; the atmosphere keeps the
  // single-segment kernel
  {
    const int nrows = g.jr1 - g.jr0 + 1;
    auto &sg = c->seg;
    int S = 1, first[QGCM_HIP_THOMAS_MAX_SEG] = {0}, count[QGCM_HIP_THOMAS_MAX_SEG] = {nrows}; // (the atmosphere's plan)
    if (!g.atm) {
      // QGCM_HIP_THOMAS_SEG_ROWS (whole-domain handles) / QGCM_HIP_THOMAS_SLAB_SEG_ROWS (y-slabs): the longest segment; read
      // here, at every set_grid.  Anything but a positive integer is refused: a typing error must not silently mean "unset"
      const char *var = c->whole ? "QGCM_HIP_THOMAS_SEG_ROWS" : "QGCM_HIP_THOMAS_SLAB_SEG_ROWS";
      sg.seg_rows = 0;
      if (const char *sr = getenv(var)) {
        char *end = nullptr;
        const long v = strtol(sr, &end, 10);
        if (end == sr || *end != '\0' || v < 1 || v > 1000000) QG_FAIL("qgcm_hip_set_grid: %s=\"%s\" is not a positive number of rows", var, sr);
        sg.seg_rows = (int)v;
      }
      if (qgcm_hip_thomas_segments(nrows, sg.seg_rows, &S, first, count)) return 1;
    }
    sg.first.assign(first, first + S);
    sg.count.assign(count, count + S);
    sg.maxlen = count[0];
    if (S != sg.S) { // (a second set_grid under another plan: the per-segment buffers are sized by S)
      HIPCHECK(hipStreamSynchronize(c->stream));
      sg.msg.reset();
      sg.coef.reset();
      sg.ab.reset();
      for (auto &ss : sg.set) { // (the pivot tables stay: upload_pivots grows them where the new plan needs more)
        ss.recs.reset();
        ss.ptab.reset();
        ss.qtab.reset();
        ss.cst.reset();
        ss.meta.reset();
      }
    }
    sg.set[1].boc.clear();
    sg.S = S;
    sg.R = thomas_rows_per_chunk(sg.maxlen);
    if (sg.R < 0) // (an ocean of that height has a segment plan: the atmosphere only)
      QG_FAIL("qgcm_hip_set_grid: %d rows of an atmosphere handle exceed the single-segment Thomas kernel (<= 2048); only ocean handles solve taller columns", nrows);
  }
  std::vector<std::vector<double>> bocs(g.nl, std::vector<double>(g.nk));
  for (int m = 0; m < g.nl; ++m)
    for (int k = 0; k < g.nk; ++k) bocs[m][k] = bd2oc[k] - c->prm.rdm2oc[m];
  // FFT tables: complex length N = nxto (box DST-I of length nxto-1)
  const int N = g.nxt;
  // The row plan (qgcm_hip_row_split): a zonally cyclic ocean transforms rows of more than 5104 points - or, with
  // QGCM_HIP_ROW_SPLIT=<P> set, rows of any length - as P interleaved sub-rows of length Ls = N / P; every other handle
  // transforms its rows whole (Ls = N) and does not read the variable.
  int splitP = 1, Ls = N;
  if (g.cyc && !g.atm) {
    int forced = 0;
    if (const char *sp = getenv("QGCM_HIP_ROW_SPLIT")) {
      char *end = nullptr;
      const long v = strtol(sp, &end, 10);
      if (end == sp || *end != '\0' || v < 1 || v > 1000000) QG_FAIL("qgcm_hip_set_grid: QGCM_HIP_ROW_SPLIT=\"%s\" is not a positive number of sub-rows", sp);
      forced = (int)v;
    }
    if (qgcm_hip_row_split(N, forced, &splitP, &Ls)) return 1;
  } else if (N > DST_SINGLE_MAXN) {
    QG_FAIL("qgcm_hip_set_grid: nxto=%d is longer than one row transform (<= %d points); only zonally cyclic ocean handles split longer rows "
            "(box oceans and atmosphere handles: nxto <= %d)", N, DST_SINGLE_MAXN, DST_SINGLE_MAXN);
  }
  c->fftN = N;
  c->nfac = factorize(Ls, c->fac);
  if (c->nfac > QG_MAXFAC) QG_FAIL("qgcm_hip_set_grid: too many FFT factors");
  std::vector<double2> tw(N);
  const double twopi = 6.28318530717958647692528676655900577;
  for (int t = 0; t < N; ++t) {
    double ang = -twopi * (double)t / (double)N;
    tw[t].x = cos(ang);
    tw[t].y = sin(ang);
  }
  std::vector<double> st(N / 2 + 2);
  const double pi = 3.14159265358979323846264338327950288;
  for (int k = 0; k <= N / 2 + 1; ++k) st[k] = 2.0 * sin((double)k * (pi / (double)N)); // dsinti.f:20-24
  if (c->twid.alloc(N, "the twiddle factors") || c->sintab.alloc(st.size(), "the sine table")) return 1;
  HIPCHECK(hipMemcpy(c->twid, tw.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(c->sintab, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice));
  // a handle that splits its rows: the sub-transforms' table exp(-2 pi i t / Ls) = every P-th entry of the table above,
  // and the scratch array; a handle that does not holds neither
  if (splitP != c->split.P || Ls != c->split.L) HIPCHECK(hipStreamSynchronize(c->stream));
  c->split.P = splitP;
  c->split.L = Ls;
  if (splitP > 1) {
    std::vector<double2> tws(Ls);
    for (int t = 0; t < Ls; ++t) tws[t] = tw[(size_t)t * splitP];
    if (c->split.twid.alloc(Ls, "the sub-rows' twiddle factors") || c->split.scr.grow((size_t)g.wstride * g.nl, "the split rows' scratch array")) return 1;
    HIPCHECK(hipMemcpy(c->split.twid, tws.data(), sizeof(double2) * Ls, hipMemcpyHostToDevice));
  } else {
    c->split.twid.reset();
    c->split.scr.reset();
  }
  // generic row kernels (of length Ls): two ping-pong buffers, or ONE buffer with in-place stages for long rows
  c->dst_single = row_single_buffer(Ls) && !getenv("QGCM_HIP_NO_SINGLE_BUFFER");
  c->dst_lds = row_lds_bytes(Ls, g.cyc, c->dst_single);
  if (c->dst_lds > kRowLdsMax) QG_FAIL("qgcm_hip_set_grid: nxto=%d needs %zu B of LDS per row pair (> 160 KiB)", Ls, c->dst_lds);
  HIPCHECK(hipFuncSetAttribute((const void *)k_dst_box<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dst_lds));
  HIPCHECK(hipFuncSetAttribute((const void *)k_dst_box<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dst_lds));
  HIPCHECK(hipFuncSetAttribute((const void *)k_dst_box<false, DST_NT_BIG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dst_lds));
  HIPCHECK(hipFuncSetAttribute((const void *)k_rfft_cyc<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dst_lds));
  HIPCHECK(hipFuncSetAttribute((const void *)k_rfft_cyc<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->dst_lds));
  // long rows: the three-stage register-radix plans of k_fft3.h (QGCM_HIP_NO_FFT3=1: the Stockham plan, for A/B + tests)
  c->fft3 = 0;
  if (!getenv("QGCM_HIP_NO_FFT3")) {
#define QG_FFT3_SETUP(ID, R1, R2, R3)                                                                                        \
    if (Ls == R1 * R2 * R3) {                                                                                                \
      typedef Fft3Plan<R1, R2, R3> PL;                                                                                       \
      c->fft3 = ID;                                                                                                          \
      c->fft3_lds = (size_t)PL::LDS_CPLX * sizeof(cplx) + 2 * (FFT3_NT / 64) * sizeof(double);                               \
      HIPCHECK(hipFuncSetAttribute((const void *)k_dst_box<false, FFT3_NT, PL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->fft3_lds)); \
      HIPCHECK(hipFuncSetAttribute((const void *)k_rfft_cyc<false, PL, FFT3_NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->fft3_lds)); \
      HIPCHECK(hipFuncSetAttribute((const void *)k_rfft_cyc<true, PL, FFT3_NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->fft3_lds)); \
      HIPCHECK(hipFuncSetAttribute((const void *)k_rfft3_unpack<PL, 3, FFT3_NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->fft3_lds)); \
      HIPCHECK(hipFuncSetAttribute((const void *)k_rfft3_unpack<PL, 3, FFT3_NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->fft3_lds)); \
    }
    QG_FFT3_PLANS(QG_FFT3_SETUP)
#undef QG_FFT3_SETUP
  }
  c->grid_set = true;
  // the pivots, and the slab summary constants (gain, backward image and column sums of the unit responses), once
  if (build_thomas_tables(c, 0, bocs)) return 1;
  {
    // weights of the spectral area integral (k_thomas.h): sum_{i=1}^{n-1} 2 sin(k i pi/n) = 2 cot(k pi/2n), k odd
    std::vector<double> wc((size_t)g.ldw, 0.0);
    if (!g.cyc)
      for (int k = 1; k <= g.nk; k += 2) {
        const double h = (double)k * (pi / (2.0 * (double)N));
        wc[k - 1] = 2.0 * cos(h) / sin(h);
      }
    HIPCHECK(hipMemcpyAsync(c->wcot, wc.data(), wc.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

static int lu_factor(int n, double *a, int *piv) {
  for (int k = 0; k < n; ++k) {
    int p = k;
    double mx = fabs(a[k + n * k]);
    for (int i = k + 1; i < n; ++i)
      if (fabs(a[i + n * k]) > mx) {
        mx = fabs(a[i + n * k]);
        p = i;
      }
    piv[k] = p;
    if (mx == 0.0) return k + 1;
    if (p != k)
      for (int j = 0; j < n; ++j) {
        double t = a[k + n * j];
        a[k + n * j] = a[p + n * j];
        a[p + n * j] = t;
      }
    for (int i = k + 1; i < n; ++i) {
      a[i + n * k] /= a[k + n * k];
      for (int j = k + 1; j < n; ++j) a[i + n * j] -= a[i + n * k] * a[k + n * j];
    }
  }
  return 0;
}

// what the box and the cyclic constraint parameters share (QgConstrParams, QgCycConstrParams)
template <class T>
static void fill_constr_common(const qgcm_hip_ctx *c, T &P) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.ksum = c->ksum;
  P.wrk = c->wrk;
  P.sc = c->sc;
  P.cs = c->cs;
  P.dxo = pr.dxo; P.dyo = pr.dyo; P.tdto = pr.tdto; P.fnot = pr.fnot;
  for (int k = 0; k < g.nl; ++k) {
    P.gpoc[k] = pr.gpoc[k];
    P.hoc[k] = pr.hoc[k];
  }
  for (int i = 0; i < g.nl * g.nl; ++i) {
    P.ctl2m[i] = pr.ctl2moc[i];
    P.ctm2l[i] = pr.ctm2loc[i];
  }
}

static void fill_constr_params(const qgcm_hip_ctx *c, QgConstrParams &P) {
  fill_constr_common(c, P);
  P.rowsum = c->rowsum;
  P.wcot = c->wcot;
}

// ... packed for the extra wave of k_dst64_unpack (nlo <= 4, qgcm_dev.h)
static void fill_constr_lite(const qgcm_hip_ctx *c, QgConstrLite &C) {
  memset(&C, 0, sizeof(C));
  C.g = c->g; C.ksum = c->ksum; C.wcot = c->wcot; C.sc = c->sc;
  C.dxo = c->prm.dxo; C.dyo = c->prm.dyo;
  for (int i = 0; i < 16; ++i) { C.cs.cdiffo[i] = c->cs.cdiffo[i]; C.cs.cdhoc[i] = c->cs.cdhoc[i]; C.cs.cdhlu[i] = c->cs.cdhlu[i]; }
  for (int i = 0; i < 4; ++i) C.cs.ipiv[i] = c->cs.ipiv[i];
}

static void fill_cyc_constr_params(const qgcm_hip_ctx *c, QgCycConstrParams &Q) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  fill_constr_common(c, Q);
  Q.bpart = Q.bpart_n = c->bpart;
  Q.ybnd = c->ybnd; // k_thomas (PHASE 0 and PHASE 2 alike) leaves the zonal-mean rows next to the boundaries there
  if (c->slab_gath) {
    // y-slab stages: the boundary line sums travel at the end of the step messages (rank 0 owns the southern boundary,
    // the last rank the northern one); the solution next to the boundaries comes from k_thomas PHASE 2
    const size_t off = (size_t)TH_MSG * g.nl * g.ldw;
    Q.bpart = c->slab_gath + off;
    Q.bpart_n = c->slab_gath + (size_t)(c->slab_nranks - 1) * slab_msg_len_oml(c) + off;
  }
  Q.adfaco = 1.0 / (12.0 * pr.dxo * pr.dyo * pr.fnot);
  Q.delek_sgn = 0.5 * (pr.fnot >= 0.0 ? 1.0 : -1.0) * pr.delek;
  for (int k = 0; k < g.nl; ++k) {
    Q.ah2oc[k] = pr.ah2oc[k];
    Q.ah4oc[k] = pr.ah4oc[k];
  }
}

extern "C" int qgcm_hip_set_homog_box(qgcm_hip_handle c, const double *ochom, const double *cdiffo, const double *cdhoc) {
  if (!c || !ochom || !cdiffo || !cdhoc) QG_FAIL("qgcm_hip_set_homog_box: null argument");
  if (c->g.cyc) QG_FAIL("qgcm_hip_set_homog_box: handle is cyclic");
  drop_graphs(c);
  const QgGeom &g = c->g;
  const int nl = g.nl, n1 = nl - 1;
  if (upload2d(c, c->ochom, g.ldx, ochom, g.nx, (long)g.ny * n1)) return 1;
  memcpy(c->cs.cdiffo, cdiffo, sizeof(double) * nl * n1);
  memcpy(c->cs.cdhoc, cdhoc, sizeof(double) * n1 * n1);
  memcpy(c->cs.cdhlu, cdhoc, sizeof(double) * n1 * n1);
  int info = lu_factor(n1, c->cs.cdhlu, c->cs.ipiv); // DGETRF, src/conhoms.F:627
  if (info) QG_FAIL("qgcm_hip_set_homog_box: cdhoc is singular (info=%d)", info);
  c->homog_set = true;
  {
    // device copy of the constraint parameters for the extra workgroup of the generic inverse rows
    QgConstrParams Q;
    fill_constr_params(c, Q);
    if (c->d_boxq.ensure(1, "the constraint parameters")) return 1;
    HIPCHECK(hipMemcpy(c->d_boxq, &Q, sizeof(Q), hipMemcpyHostToDevice));
  }
  return 0;
}

extern "C" int qgcm_hip_set_homog_cyc(qgcm_hip_handle c, const double *pch1oc, const double *pch2oc, const double *pbhoc,
                                      const double *aipcho, const double *hc1soc, const double *hc2soc, const double *hc1noc,
                                      const double *hc2noc, double hbsioc, double aipbho) {
  if (!c || !pch1oc || !pch2oc || !pbhoc || !aipcho || !hc1soc || !hc2soc || !hc1noc || !hc2noc)
    QG_FAIL("qgcm_hip_set_homog_cyc: null argument");
  if (!c->g.cyc) QG_FAIL("qgcm_hip_set_homog_cyc: handle is a box ocean");
  drop_graphs(c);
  const QgGeom &g = c->g;
  const int n1 = g.nl - 1;
  HIPCHECK(hipMemcpy(c->pch1, pch1oc, sizeof(double) * g.ny * n1, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(c->pch2, pch2oc, sizeof(double) * g.ny * n1, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(c->pbh, pbhoc, sizeof(double) * g.ny, hipMemcpyHostToDevice));
  for (int m = 0; m < n1; ++m) {
    c->cs.aipcho[m] = aipcho[m];
    c->cs.hc1soc[m] = hc1soc[m];
    c->cs.hc2soc[m] = hc2soc[m];
    c->cs.hc1noc[m] = hc1noc[m];
    c->cs.hc2noc[m] = hc2noc[m];
  }
  c->cs.hbsioc = hbsioc;
  c->cs.aipbho = aipbho;
  c->homog_set = true;
  {
    // device copy of the constraint parameters for the fused step path (k_thomas's extra workgroup, k_rfft64_unpack)
    QgCycConstrParams Q;
    fill_cyc_constr_params(c, Q);
    if (c->d_cycq.ensure(1, "the constraint parameters")) return 1;
    HIPCHECK(hipMemcpy(c->d_cycq, &Q, sizeof(Q), hipMemcpyHostToDevice));
  }
  return 0;
}

extern "C" int qgcm_hip_set_state(qgcm_hip_handle c, const double *po, const double *pom, const double *qo, const double *qom) {
  if (!c) QG_FAIL("qgcm_hip_set_state: null handle");
  const QgGeom &g = c->g;
  const long rows = (long)g.ny * g.nl;
  if (po && upload2d(c, c->p[c->ip], g.ldx, po, g.nx, rows)) return 1;
  if (pom && upload2d(c, c->p[c->ip ^ 1], g.ldx, pom, g.nx, rows)) return 1;
  if (qo && upload2d(c, c->q[c->iq], g.ldx, qo, g.nx, rows)) return 1;
  if (qom && upload2d(c, c->q[c->iq ^ 1], g.ldx, qom, g.nx, rows)) return 1;
  return 0;
}

extern "C" int qgcm_hip_get_state(qgcm_hip_handle c, double *po, double *pom, double *qo, double *qom) {
  if (!c) QG_FAIL("qgcm_hip_get_state: null handle");
  const QgGeom &g = c->g;
  const long rows = (long)g.ny * g.nl;
  if (po && download2d(c, po, c->p[c->ip], g.ldx, g.nx, rows)) return 1;
  if (pom && download2d(c, pom, c->p[c->ip ^ 1], g.ldx, g.nx, rows)) return 1;
  if (qo && download2d(c, qo, c->q[c->iq], g.ldx, g.nx, rows)) return 1;
  if (qom && download2d(c, qom, c->q[c->iq ^ 1], g.ldx, g.nx, rows)) return 1;
  return 0;
}

extern "C" int qgcm_hip_set_forcing(qgcm_hip_handle c, const double *wekpo, const double *entoc, const double *xon) {
  if (!c) QG_FAIL("qgcm_hip_set_forcing: null handle");
  const QgGeom &g = c->g;
  if (wekpo && upload2d(c, c->wekpo, g.ldx, wekpo, g.nx, g.ny)) return 1;
  if (entoc) { // (NULL leaves the buffer and what is known about it as they were)
    c->entoc_zero = false;
    if (upload2d(c, c->entoc, g.ldx, entoc, g.nx, g.ny)) return 1;
    // no drop_graphs: the graph keys carry the mask, a captured block of the other variant stays valid for its mask
    c->entoc_zero = all_plus_zero(entoc, (size_t)g.nx * g.ny);
  }
  if (xon) {
    HIPCHECK(hipMemcpyAsync((char *)(QgScalars *)c->sc + offsetof(QgScalars, xon), xon, sizeof(double) * (g.nl - 1), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

extern "C" int qgcm_hip_tend_zero_mask(qgcm_hip_handle c) { return c ? tend_zmask(c) : -1; }

// The fork's sponge layer (-Dsponge_layer_k247): r_spl(nxpo,nypo) of MODULE occonst (set by the main program,
// src/q-gcm.F:1154-1168) and the compile-time constant c1_spl (src/parameters_data.F:144).  NULL switches the term off.
extern "C" int qgcm_hip_set_sponge(qgcm_hip_handle c, const double *r_spl, double c1_spl) {
  if (!c) QG_FAIL("qgcm_hip_set_sponge: null handle");
  if (c->g.atm) QG_FAIL("qgcm_hip_set_sponge: the atmosphere has no sponge term (src/qgasubs.F)");
  drop_graphs(c); // captured steps hold the kernel parameters by value
  const QgGeom &g = c->g;
  if (!r_spl) {
    c->rspl.reset();
    c->c1_spl = 0.0;
    return 0;
  }
  if (g.cyc) {
    // A periodic channel needs a ramp that is periodic in x (the fork's option nospl_in_ewbdy_k247: N / S boundaries
    // only).  The reference steps the duplicate column nxpo by itself (src/qgosubs.F:181), so with the full ramp of
    // src/q-gcm.F:1164-1166, whose values at i = 1 and i = nxpo differ, its qo(nxpo,j) drifts away from qo(1,j); on
    // the device column nxpo IS column 1 - refuse instead of differing silently.
    for (int j = 0; j < g.ny; ++j)
      if (r_spl[(size_t)j * g.nx] != r_spl[(size_t)j * g.nx + g.nx - 1])
        QG_FAIL("qgcm_hip_set_sponge: r_spl(1,%d) != r_spl(nxpo,%d) - a zonally cyclic ocean needs a ramp that is periodic in x (build with -Dnospl_in_ewbdy_k247)", j + 1, j + 1);
  }
  if (c->rspl.ensure((size_t)g.fstride, "the sponge ramp")) return 1;
  c->c1_spl = c1_spl;
  return upload2d(c, c->rspl, g.ldx, r_spl, g.nx, g.ny);
}

extern "C" int qgcm_hip_set_cyc_forcing(qgcm_hip_handle c, double txisoc, double txinoc, const double *enisoc,
                                        const double *eninoc) {
  if (!c) QG_FAIL("qgcm_hip_set_cyc_forcing: null handle");
  if (!c->g.cyc) QG_FAIL("qgcm_hip_set_cyc_forcing: handle is a box ocean");
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  h.txisoc = txisoc;
  h.txinoc = txinoc;
  for (int k = 0; k < c->g.nl - 1; ++k) {
    if (enisoc) h.enisoc[k] = enisoc[k];
    if (eninoc) h.eninoc[k] = eninoc[k];
  }
  HIPCHECK(hipMemcpyAsync(c->sc, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_set_scalars(qgcm_hip_handle c, const double *s) {
  if (!c || !s) QG_FAIL("qgcm_hip_set_scalars: null argument");
  const int nl = c->g.nl, o = 2 * (nl - 1);
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < nl - 1; ++k) {
    h.dpioc[k] = s[k];
    h.dpiocp[k] = s[nl - 1 + k];
  }
  for (int k = 0; k < nl; ++k) {
    h.ocncs[k] = s[o + k];
    h.ocncn[k] = s[o + nl + k];
    h.ocncsp[k] = s[o + 2 * nl + k];
    h.ocncnp[k] = s[o + 3 * nl + k];
  }
  HIPCHECK(hipMemcpyAsync(c->sc, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_get_scalars(qgcm_hip_handle c, double *s) {
  if (!c || !s) QG_FAIL("qgcm_hip_get_scalars: null argument");
  const int nl = c->g.nl, o = 2 * (nl - 1);
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < nl - 1; ++k) {
    s[k] = h.dpioc[k];
    s[nl - 1 + k] = h.dpiocp[k];
  }
  for (int k = 0; k < nl; ++k) {
    s[o + k] = c->g.cyc ? h.ocncs[k] : 0.0;
    s[o + nl + k] = c->g.cyc ? h.ocncn[k] : 0.0;
    s[o + 2 * nl + k] = c->g.cyc ? h.ocncsp[k] : 0.0;
    s[o + 3 * nl + k] = c->g.cyc ? h.ocncnp[k] : 0.0;
  }
  return 0;
}

extern "C" int qgcm_hip_get_inv_diag(qgcm_hip_handle c, double *xinhom, double *coef) {
  if (!c) QG_FAIL("qgcm_hip_get_inv_diag: null handle");
  const int nl = c->g.nl;
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (xinhom)
    for (int m = 0; m < nl; ++m) xinhom[m] = h.xinhom[m];
  if (coef) {
    if (c->g.cyc) {
      for (int m = 0; m < nl - 1; ++m) {
        coef[m] = h.c1[m];
        coef[nl - 1 + m] = h.c2[m];
      }
      coef[2 * (nl - 1)] = h.c3;
    } else {
      for (int m = 0; m < nl - 1; ++m) coef[m] = h.hclco[m];
    }
  }
  return 0;
}

extern "C" int qgcm_hip_get_monitors(qgcm_hip_handle c, double *ermas, double *emfr) {
  if (!c) QG_FAIL("qgcm_hip_get_monitors: null handle");
  if (!c->g.cyc) QG_FAIL("qgcm_hip_get_monitors: the box ocean has no continuity monitors (src/ocisubs.F:268-283 is cyclic_ocean code)");
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < c->g.nl - 1; ++k) {
    if (ermas) ermas[k] = h.ermas[k];
    if (emfr) emfr[k] = h.emfr[k];
  }
  return 0;
}

// ---------------------------------------------------------------------------
// kernel launches
// ---------------------------------------------------------------------------
// Profiling mode: a HIP event pair brackets every kernel launch on the stream; the
// pairs are drained once per step so the queue stays busy between kernels.
struct KTimer {
  qgcm_hip_ctx *c;
  size_t slot;
  hipStream_t st;
  KTimer(qgcm_hip_ctx *c_, int id, hipStream_t st_ = nullptr) : c(c_), slot(0), st(st_ ? st_ : c_->stream) {
    if (c->profiling) {
      slot = c->evkid.size();
      if (c->evpool.size() < 2 * (slot + 1)) {
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        c->evpool.push_back(a);
        c->evpool.push_back(b);
      }
      c->evkid.push_back(id);
      note(hipEventRecord(c->evpool[2 * slot], st), 0);
    }
  }
  ~KTimer() {
    if (c->profiling)
      note(hipEventRecord(c->evpool[2 * slot + 1], st), 1);
  }
  void note(hipError_t e, int which) {
    if (e != hipSuccess && c->timer_err == hipSuccess) {
      c->timer_err = e;
      c->timer_err_at = 2 * (int)slot + which;
    }
  }
};

static void drain_timers(qgcm_hip_ctx *c) {
  if (c->evkid.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  for (size_t i = 0; i < c->evkid.size(); ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->evpool[2 * i], c->evpool[2 * i + 1]);
    c->kms[c->evkid[i]] += ms;
    c->klaunch[c->evkid[i]] += 1;
  }
  c->evkid.clear();
}

static void fill_oml_final(qgcm_hip_ctx *c, QgOmlFinal &F, bool on) {
  memset(&F, 0, sizeof(F));
  if (c->aml.on) { // the atmosphere's mixed layer: the same sums under other names (xan, enisat / eninat, cfraat, centat)
    const auto &a = c->aml;
    F.partA = a.partA; F.partB = a.partB; F.nblkA = a.nblkA; F.nblkB = a.nblkB; F.diag = a.diag;
  } else {
    const auto &o = c->oml;
    F.partA = o.partA; F.partB = o.partB; F.nblkA = o.nblkA; F.nblkB = o.nblkB; F.diag = o.diag;
  }
  F.cyc = c->g.cyc; F.on = on ? 1 : 0;
  F.sc = c->sc;
  F.ocnorm = 1.0 / ((double)c->g.nxt * (double)(c->g.nyg - 1)); // src/parameters_data.F:88
  F.dxo = c->prm.dxo; F.dyo = c->prm.dyo;
}

// part: TEND_ALL = the whole launch; TEND_INNER = the tile rows whose stencils stay inside the owned rows (they need no
// halo row: y-slabs run them while the halo exchange of the previous step is still under way) plus the one-thread /
// one-workgroup riders of workgroup 0; TEND_OUTER = the first and the last tile row plus the edge / line-sum workgroups.
// INNER followed by OUTER writes what ALL writes, bit for bit (tiles are independent).
enum { TEND_ALL = 0, TEND_INNER = 1, TEND_OUTER = 2 };
static bool tend_can_split(const qgcm_hip_ctx *c) {
  const TendTiling T = c->g.cyc ? tend_tiling<true>(c->g) : tend_tiling<false>(c->g);
  return T.gy >= 3;
}

// The step plan: which launches one inversion makes, derived in ONE place from the geometry and the handle's switches
// (DESIGN 3.5 has the table).  ocinvq_impl, one_step, launch_tend, launch_dst and the slab stages 1 / 2 read it.
enum { ROWS_GENERIC = 0, ROWS_DST64, ROWS_RFFT64, ROWS_FFT3, ROWS_SPLIT };        // the row kernels' family
enum { INV_PLAIN = 0, INV_DST64_UNPACK, INV_RFFT64_UNPACK, INV_FFT3_UNPACK };      // inverse rows: alone, or fused with the unpack
enum { CONSTR_OWN = 0, CONSTR_INV_WAVE, CONSTR_BOX_WG, CONSTR_AB };                // where the constraint solve runs
struct QgStepPlan {
  int rows;     // ROWS_GENERIC: k_dst_box / k_rfft_cyc (Stockham); ROWS_DST64 / ROWS_RFFT64: a wave per row pair (k_dst64.h,
                // k_rfft64.h); ROWS_FFT3: the three-stage plans of k_fft3.h; ROWS_SPLIT: P sub-rows per row through the
                // scratch array (k_row_split.h), three launches per transform
  int m64;      // wave-per-row-pair families: nxto = 64 * m64
  int inv;      // INV_PLAIN: launch_dst + launch_unpack; else k_dst64_unpack / k_rfft64_unpack / k_rfft3_unpack
  int constr;   // CONSTR_OWN: a launch of its own (k_constr_box / k_constr_cyc); CONSTR_INV_WAVE: the extra wave of
                // k_dst64_unpack; CONSTR_BOX_WG: the extra workgroup of the generic box inverse rows; CONSTR_AB: part A in
                // the Thomas launch, part B in the inverse launch (cyclic)
  bool upd_dpi; // k_tend steps dpioc / dpiocp (the constraint solve of CONSTR_INV_WAVE starts from the stepped values)
  bool wtq;     // k_tend: write-through pair stores of the new qo and 16-wide tiles
  bool avg_ok;  // a leapfrog-averaging step may be fused into k_tend and the fused inverse kernel
  bool band_rows; // one_step's plain steps run k_tend_rows (k_tend_rows.h: tendency by bands of so many rows, whose
                // epilogue is the forward row transform) in place of launch_tend + the forward launch_dst
};

// in_step: inside qgcm_hip_steps (k_tend has stepped dpioc where the plan says so, the boundary PV is fused into the
// unpack); slab: the stages 1 / 2 of qgcm_hip_slab_stage
static QgStepPlan step_plan(const qgcm_hip_ctx *c, bool in_step = false, bool slab = false) {
  const QgGeom &g = c->g;
  QgStepPlan pl;
  // the row lengths with a wave-per-row-pair kernel: an in-register M-point DFT exists for M = 3, 15 and (k_rfft64.h) 6
  const int N = c->fftN;
  pl.m64 = c->force_generic_dst ? 0 : (N == 64 * 3 ? 3 : N == 64 * 15 ? 15 : (g.cyc && N == 64 * 6) ? 6 : 0);
  pl.rows = (c->fft3 && !c->force_generic_dst) ? ROWS_FFT3 : pl.m64 ? (g.cyc ? ROWS_RFFT64 : ROWS_DST64) : ROWS_GENERIC;
  // split rows (cyclic oceans): the unfused inverse rows + k_unpack_cyc and the stand-alone k_constr_cyc, as a column
  // cut into segments has them - every fused or riding form below asks for another row family
  if (c->split.P > 1) {
    pl.rows = ROWS_SPLIT;
    pl.m64 = 0;
  }
  // inverse rows + homogeneous corrections + modes -> layers (+ boundary PV) in one launch, 2 .. 4 layers:
  // box (k_dst64_unpack); cyclic / atmosphere, whole domain (k_rfft64_unpack; the slab stages keep the plain rows);
  // long cyclic ocean rows of three layers (k_fft3_unpack.h: it reads the solved modes once, the boundary PV always fused)
  pl.inv = INV_PLAIN;
  if (!c->no_fused_unpack) {
    if (pl.rows == ROWS_DST64 && g.nl <= 4) pl.inv = INV_DST64_UNPACK;
    if (pl.rows == ROWS_RFFT64 && g.nl <= 4 && c->whole && !slab) pl.inv = INV_RFFT64_UNPACK;
    if (pl.rows == ROWS_FFT3 && g.cyc && !g.atm && g.nl == 3 && g.ldx % 2 == 0) pl.inv = INV_FFT3_UNPACK;
  }
  pl.constr = CONSTR_OWN;
  if (!c->no_fused_constr) {
    if (g.cyc) {
      // inside qgcm_hip_steps part A of the constraint algebra rides in the Thomas launch and part B in the inverse
      // launch: the extra wave of k_rfft64_unpack, every workgroup of k_rfft3_unpack, the extra workgroup of the generic
      // rows (SOcn 5 km; it reads ksum and ybnd, not wrk) - the riding parts exist for nlo <= 4.  (The wave-per-row-pair
      // kernels of k_rfft64.h have no such extra workgroup: they are fused with the unpack unless that is switched off,
      // and then keep the stand-alone constraint launch.)
      // (a column cut into segments launches no k_thomas<R, 0, true>, whose extra workgroup part A rides in: the
      //  stand-alone k_constr_cyc there)
      if (in_step && !slab && g.nl <= 4 && c->seg.S == 1 && pl.rows != ROWS_SPLIT && (pl.inv == INV_RFFT64_UNPACK || pl.rows != ROWS_RFFT64)) pl.constr = CONSTR_AB;
    } else if (pl.inv == INV_DST64_UNPACK) {
      // (y-slabs with the mixed layer on: xon(1) is only complete after the all-gather of stage 2 - no riding solve)
      if (in_step && !(slab && c->oml.on)) pl.constr = CONSTR_INV_WAVE;
    } else if (pl.rows != ROWS_DST64 && g.nl <= 3) {
      pl.constr = CONSTR_BOX_WG; // 2 or 3 layers, see k_dst_box
    }
  }
  // whole-domain inversions use k_rfft3_unpack only where its workgroups evaluate part B themselves
  if (pl.inv == INV_FFT3_UNPACK && !slab && pl.constr != CONSTR_AB) pl.inv = INV_PLAIN;
  pl.upd_dpi = pl.constr == CONSTR_INV_WAVE;
  // write-through pair stores of the new qo (and 16-wide tiles) while the fields fit the Infinity Cache; plain stores and
  // 32-wide tiles beyond (k_tend.h)
  pl.wtq = (double)g.fstride * 8.0 * (7 * g.nl - 1) < 200.0e6 && !c->tend_wide;
  // the fused kernels that can store the averaged time level: k_tend<.., AVG> with k_dst64_unpack<.., AVG> (write-through
  // tiles only) or with k_rfft3_unpack<.., AVG>.  (While the po sum is on, the averaging step runs unfused: the sum must
  // see this step's po before it is averaged.)
  pl.avg_ok = in_step && !slab && !c->no_fused_avg && !c->poavg.on &&
              ((pl.constr == CONSTR_INV_WAVE && pl.wtq) || pl.inv == INV_FFT3_UNPACK);
  // the 5 km box ocean inside qgcm_hip_steps: tendency and forward rows in one launch.  The kernel exists for three
  // layers, 960-point rows, entoc and ddynoc both read or both all zero; it carries neither the mixed layers' riders nor
  // the sponge term.  (The running mean of po adds its launch after the step either way: the same plan on or off.)
  // Not where the ocean shares the GPU with an atmosphere (qgcm_hip_coupled_steps) or has a CU range: the kernel's 240
  // workgroups want a whole CU each (768 threads, 110 KB of LDS) and one generation of them - with 192 CUs, or with CUs
  // that hold the atmosphere's waves, the coupled ocean step was 4.5 us slower than with the two launches.
  const int zm = tend_zmask(c);
  pl.band_rows = (!c->no_band_rows && !g.cyc && pl.rows == ROWS_DST64 && pl.m64 == 15 && g.nl == 3 && in_step && !slab &&
                  c->whole && c->seg.S == 1 && pl.wtq && pl.constr == CONSTR_INV_WAVE && (zm == 0 || zm == 3) &&
                  !c->oml.on && !c->aml.on && !(const double *)c->rspl && !c->beside && c->cu_count == 0);
  return pl;
}

// The zero-field variants of the tendency kernel (k_tend.h: k_tend_z; zm = 1, 2, 3, nl <= 4).  Defined at the END of this
// file, and on purpose: kernels land in the code object in the order of their first use in this translation unit, so the
// variants follow every kernel the parent library had, which keep their code AND their place (where a kernel lies moves
// the 5 km step by +-0.7 us).
static void launch_tend_z(int zm, int nl, bool cyc, bool wtq, bool avg, dim3 grid, hipStream_t stream, const QgTendParams &P,
                          const QgCycSumParams &S, const QgOmlFinal &F);
// The row-band kernel of the 5 km box ocean (k_tend_rows.h; step_plan's band_rows).  The kernel and its launch live in
// k_tend_rows.hip, a device code object of its own: this file compiles to the device code it had without the kernel.
void qg_launch_tend_rows(int zm, hipStream_t st, const QgTendParams &P, const double2 *twid, const double *sintab);
static int launch_tend_rows(qgcm_hip_ctx *c, bool upd_dpi);

// what the tendency kernels read (launch_tend, launch_tend_rows)
static void fill_tend_params(const qgcm_hip_ctx *c, QgTendParams &P, bool upd_dpi) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.pom = c->p[c->ip ^ 1];
  P.po = c->p[c->ip];
  P.qo = c->q[c->iq];
  P.qnew = c->q[c->iq ^ 1];
  P.wekpo = c->wekpo; P.entoc = c->entoc; P.ddynoc = c->ddynoc; P.yporel = c->yporel;
  P.wrk = c->wrk; P.sc = c->sc; P.bsum = nullptr;
  // scalar prologue of qgostep, src/qgosubs.F:76-82, and ocadif, :276-277
  P.adfaco = 1.0 / (12.0 * pr.dxo * pr.dyo * pr.fnot);
  P.dxom2 = 1.0 / (pr.dxo * pr.dxo);
  P.bcfaco = pr.bccooc * P.dxom2 / (0.5 * pr.bccooc + 1.0);
  P.tdto = pr.tdto;
  P.bdrfac = 0.5 * (pr.fnot >= 0.0 ? 1.0 : -1.0) * pr.delek / pr.hoc[g.nl - 1];
  P.fnot = pr.fnot; P.beta = pr.beta;
  for (int k = 0; k < g.nl; ++k) {
    P.fohfac[k] = pr.fnot / pr.hoc[k];
    P.ah2fac[k] = pr.ah2oc[k] / pr.fnot;
    P.ah4fac[k] = pr.ah4oc[k] / pr.fnot;
  }
  for (int i = 0; i < g.nl * g.nl; ++i) P.ctl2m[i] = pr.ctl2moc[i];
  P.upd_dpi = upd_dpi ? 1 : 0;
  P.rspl = c->rspl;
  P.tdc1 = pr.tdto * c->c1_spl; // tdto*c1_spl, src/qgosubs.F:204
  for (int k = 0; k < g.nl; ++k) P.gpoc[k] = pr.gpoc[k];
}

// avg: the launch stores the averaged time level (one_step); bpart: where the extra workgroups put the boundary line
// sums (nullptr: c->bpart; y-slabs: the tail of the step message); st: nullptr = the handle's stream
static int launch_tend(qgcm_hip_ctx *c, bool upd_dpi = false, bool oml_final = false, int part = TEND_ALL, bool avg = false,
                       double *bpart = nullptr, hipStream_t st = nullptr) {
  if (!st) st = c->stream;
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  QgTendParams P;
  fill_tend_params(c, P, upd_dpi);
  // write-through pair stores of the new qo and 16-wide tiles while the step's working set (~ 7 nl - 1 fields) stays in the
  // 256 MiB Infinity Cache (NAtl 5 km: 150 MB: -1 us per step; SOcn 5 km's 425 MB: +8 us); plain stores and 32-wide
  // tiles at the HBM-bound sizes (k_tend.h)
  const QgStepPlan pl = step_plan(c, true);
  const bool wtq = pl.wtq;
  if (avg && (part != TEND_ALL || !pl.avg_ok)) QG_FAIL("k_tend: the fused leapfrog averaging belongs to whole-domain steps of the fused inverse-row kernels");
  const TendTiling T = g.cyc ? (wtq ? tend_tiling<true, TEND_TX>(g) : tend_tiling<true, TEND_TX_WIDE>(g))
                             : (wtq ? tend_tiling<false, TEND_TX>(g) : tend_tiling<false, TEND_TX_WIDE>(g));
  if (part != TEND_ALL && T.gy < 3) QG_FAIL("k_tend: a slab of fewer than three tile rows cannot be split");
  if (part == TEND_INNER) { P.trow0 = 1; P.trows = T.gy - 2; P.tstride = 1; }
  if (part == TEND_OUTER) { P.trow0 = 0; P.trows = 2; P.tstride = T.gy - 1; P.upd_dpi = 0; }
  const int ntiles = T.gx * (part == TEND_ALL ? T.gy : P.trows);
  // cyclic: the boundary line sums for the momentum constraints (state before the step) ride as extra workgroups
  QgCycSumParams S;
  memset(&S, 0, sizeof(S));
  if (g.cyc) {
    S.g = g;
    S.pom = P.pom; S.po = P.po; S.qo = P.qo;
    S.part = bpart ? bpart : c->bpart;
    S.bcfaco = P.bcfaco; S.dxom2 = P.dxom2; S.adfaco = P.adfaco; S.fnot = pr.fnot;
    S.dxo = pr.dxo; S.dyo = pr.dyo;
  }
  QgOmlFinal F;
  fill_oml_final(c, F, oml_final && (c->oml.on || c->aml.on) && part != TEND_OUTER);
  const int nextra = part == TEND_INNER ? 0 : (g.cyc ? g.nl * 2 * BSUM_NB : T.nedge);
  dim3 grid(8 * ((ntiles + 7) / 8) + nextra); // 1-D: the kernel maps blockIdx -> tile per XCD band, then edge / line-sum work
  KTimer t(c, KN_TEND, st);
  // the ONE place that picks between k_tend and its zero-field variants: qgostep, one_step, the slab stages (whole,
  // inner and outer tile windows) and qgastep all launch from here
  const int zm = tend_zmask(c);
#define QG_TEND(NLV)                                                                                       \
  if (g.cyc && wtq) hipLaunchKernelGGL((k_tend<NLV, true, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); \
  else if (g.cyc) hipLaunchKernelGGL((k_tend<NLV, true, false>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); \
  else if (wtq) hipLaunchKernelGGL((k_tend<NLV, false, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); \
  else hipLaunchKernelGGL((k_tend<NLV, false, false>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F)
  if (zm) { // (tend_zmask: nl <= 4) the same choice of NL, CYC, WTQ, AVG as below, among the variants
    launch_tend_z(zm, g.nl, g.cyc, wtq, avg, grid, st, P, S, F);
  } else if (avg && g.cyc) { // (long-row cyclic oceans: k_rfft3_unpack<.., AVG> does the rest)
    if (wtq) hipLaunchKernelGGL((k_tend<3, true, true, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F);
    else hipLaunchKernelGGL((k_tend<3, true, false, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F);
  } else if (avg) { // the step before a leapfrog averaging stores the averaged qo itself (one_step)
    switch (g.nl) {
      case 2: hipLaunchKernelGGL((k_tend<2, false, true, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); break;
      case 3: hipLaunchKernelGGL((k_tend<3, false, true, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); break;
      default: hipLaunchKernelGGL((k_tend<4, false, true, true>), grid, dim3(TEND_NT), 0, st, QG_TEND_VALS(P, F), P, S, F); break;
    }
  } else {
    QG_SWITCH_NL(g.nl, QG_TEND, "k_tend");
  }
#undef QG_TEND
  HIPCHECK(hipGetLastError());
  return 0;
}

// what the row kernels read, the fused inverse kernels included (they never look at the Stockham factor list)
static void fill_dst_params(const qgcm_hip_ctx *c, QgDstParams &D, double *wrk, int nlayers, int layer0) {
  memset(&D, 0, sizeof(D));
  D.g = c->g;
  D.wrk = wrk;
  D.twid = c->twid;
  D.sintab = c->sintab;
  D.rowsum = nullptr; // area / line integrals come from k_thomas (ksum and the k = 0 column)
  D.N = c->fftN;
  D.nfac = c->nfac;
  for (int f = 0; f < c->nfac; ++f) D.fac[f] = c->fac[f];
  D.nlayers = nlayers;
  D.layer0 = layer0;
  D.single = c->dst_single ? 1 : 0;
}

// The radix-P pass and the copies of split rows live in k_row_split.hip, a device code object of its own (as
// k_tend_rows.hip): this file compiles to the device code it had without them.
hipError_t qg_launch_row_split(int which, hipStream_t st, const QgRowSplit &S, int nlayers);
static int launch_dst(qgcm_hip_ctx *c, double *wrk, int nlayers, bool inverse, int layer0, hipStream_t st, bool cyc_part_b,
                      bool box_constr, bool sub);

// ROWS_SPLIT (k_row_split.h): forward = sub-rows out of the rows, their transforms, the radix-P pass into the rows;
// inverse = the radix-P pass out of the rows, the sub-rows' transforms, the sub-rows back into the rows.  Three
// launches, each counted in the transform's class.
static int launch_dst_split(qgcm_hip_ctx *c, double *wrk, int nlayers, bool inverse, int layer0, hipStream_t st) {
  const QgGeom &g = c->g;
  QgRowSplit S;
  memset(&S, 0, sizeof(S));
  S.wrk = wrk; S.scr = c->split.scr; S.twid = c->twid;
  S.wstride = g.wstride; S.ldw = g.ldw; S.jr0 = g.jr0; S.nrows = g.jr1 - g.jr0 + 1;
  S.N = c->fftN; S.P = c->split.P; S.L = c->split.L;
  S.layer0 = layer0;
  if (!S.scr || S.P * S.L != S.N || S.N > g.ldw) QG_FAIL("launch_dst: the handle has no split-row plan");
  const int kn = inverse ? KN_DSTI : KN_DSTF;
  {
    KTimer t(c, kn, st);
    HIPCHECK(qg_launch_row_split(inverse ? SPLIT_INV : SPLIT_GATHER, st, S, nlayers));
  }
  if (launch_dst(c, c->split.scr, nlayers, inverse, layer0, st, false, false, true)) return 1;
  KTimer t(c, kn, st);
  HIPCHECK(qg_launch_row_split(inverse ? SPLIT_SCATTER : SPLIT_FWD, st, S, nlayers));
  return 0;
}

// sub: the sub-rows of split rows - wrk = the scratch array, seen as P * nrows rows of length and pitch L per mode
static int launch_dst(qgcm_hip_ctx *c, double *wrk, int nlayers, bool inverse, int layer0 = 0, hipStream_t st = nullptr,
                      bool cyc_part_b = false, bool box_constr = false, bool sub = false) {
  if (!st) st = c->stream;
  const QgGeom &g = c->g;
  QgStepPlan pl = step_plan(c);
  if (pl.rows == ROWS_SPLIT && !sub) {
    if (cyc_part_b || box_constr) QG_FAIL("launch_dst: no constraint solve rides in split rows");
    return launch_dst_split(c, wrk, nlayers, inverse, layer0, st);
  }
  QgDstParams P;
  fill_dst_params(c, P, wrk, nlayers, layer0);
  int nrows = g.jr1 - g.jr0 + 1;
  if (sub) { // (the row kernels read N, ldw, wstride, jr0, jr1 of their parameters; ny only with row sums, which are off)
    pl.rows = (c->fft3 && !c->force_generic_dst) ? ROWS_FFT3 : ROWS_GENERIC;
    nrows *= c->split.P;
    P.N = c->split.L;
    P.twid = c->split.twid;
    P.g.ldw = c->split.L;
    P.g.jr0 = 1;
    P.g.jr1 = nrows;
  }
  const int npairs = (nrows + 1) / 2;
  dim3 grid(npairs, nlayers);
  dim3 grid64((npairs + D64_WAVES - 1) / D64_WAVES, nlayers);
  if (cyc_part_b) { // generic cyclic inverse rows: one extra workgroup runs part B of the constraint algebra
    if (!inverse || !g.cyc || !c->d_cycq || g.nl > 4) QG_FAIL("launch_dst: part B rides in the inverse rows of a cyclic ocean with homogeneous solutions, nlo <= 4");
    P.cycq = c->d_cycq;
    grid.x += 1;
  }
  if (box_constr) { // generic box inverse rows: one extra workgroup runs the constraint solve (k_constr_box's body)
    if (!inverse || g.cyc || !c->d_boxq || pl.rows == ROWS_DST64 || g.nl > 3) QG_FAIL("launch_dst: the box constraint solve rides in the generic inverse rows of a box ocean with homogeneous solutions");
    P.boxq = c->d_boxq;
    grid.x += 1;
  }
  KTimer t(c, inverse ? KN_DSTI : KN_DSTF, st);
  if (pl.rows == ROWS_FFT3) {
    // long rows: three in-place register-radix stages (k_fft3.h)
#define QG_FFT3_LAUNCH(ID, R1, R2, R3)                                                                                     \
    if (c->fft3 == ID) {                                                                                                   \
      typedef Fft3Plan<R1, R2, R3> PL;                                                                                     \
      if (!g.cyc) hipLaunchKernelGGL((k_dst_box<false, FFT3_NT, PL>), grid, dim3(FFT3_NT), c->fft3_lds, st, P);            \
      else if (inverse) hipLaunchKernelGGL((k_rfft_cyc<true, PL, FFT3_NT>), grid, dim3(FFT3_NT), c->fft3_lds, st, P);      \
      else hipLaunchKernelGGL((k_rfft_cyc<false, PL, FFT3_NT>), grid, dim3(FFT3_NT), c->fft3_lds, st, P);                  \
    }
    QG_FFT3_PLANS(QG_FFT3_LAUNCH)
#undef QG_FFT3_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
  }
  if (g.cyc) {
    // wave-per-row-pair fast path when nxto = 64*M (k_rfft64.h); the generic Stockham kernel otherwise
    const int M64 = pl.m64;
#define QG_RF(MV)                                                                           \
  if (inverse) hipLaunchKernelGGL((k_rfft64<MV, true>), grid64, dim3(D64_NT), 0, st, P);    \
  else hipLaunchKernelGGL((k_rfft64<MV, false>), grid64, dim3(D64_NT), 0, st, P)
    if (M64 == 3) { QG_RF(3); }
    else if (M64 == 6) { QG_RF(6); }
    else if (M64 == 15) { QG_RF(15); }
    else if (inverse) hipLaunchKernelGGL((k_rfft_cyc<true>), grid, dim3(RFFT_NT), c->dst_lds, st, P);
    else hipLaunchKernelGGL((k_rfft_cyc<false>), grid, dim3(RFFT_NT), c->dst_lds, st, P);
#undef QG_RF
    HIPCHECK(hipGetLastError());
    return 0;
  }
  // wave-per-row-pair fast path when nxto = 64*M with an in-register M-point DFT available
  if (pl.m64 == 15) {
    hipLaunchKernelGGL((k_dst64<15, false>), grid64, dim3(D64_NT), 0, st, QG_ROW_VALS(P), P);
  } else if (pl.m64 == 3) {
    hipLaunchKernelGGL((k_dst64<3, false>), grid64, dim3(D64_NT), 0, st, QG_ROW_VALS(P), P);
  } else if (c->fftN >= DST_BIG_N) hipLaunchKernelGGL((k_dst_box<false, DST_NT_BIG>), grid, dim3(DST_NT_BIG), c->dst_lds, st, P);
  else hipLaunchKernelGGL((k_dst_box<false>), grid, dim3(DST_NT), c->dst_lds, st, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

// the response tables of set `which` as the three correction kernels read them: np, nq, poff, qoff are the quarters of meta
static QgThomasCorr thomas_corr_tables(const qgcm_hip_ctx *c, int which) {
  const auto &ss = c->seg.set[which];
  const int nm = (c->g.nk + TH_KW - 1) / TH_KW * (which ? 1 : c->g.nl) * c->seg.S;
  QgThomasCorr T;
  T.ptab = ss.ptab; T.qtab = ss.qtab;
  T.np = ss.meta; T.nq = ss.meta + nm; T.poff = ss.meta + 2 * nm; T.qoff = ss.meta + 3 * nm;
  return T;
}
// slices (blockIdx.z) the correction kernels cut a slab or segment of nrows rows into
static int thomas_corr_slices(int nrows) {
  const int per = THC_UNR * (THC_NT / 8); // rows per slice
  return (nrows + per - 1) / per;
}
// a correction kernel of this file with lds bytes for its ranks' or segments' inflows: more than 31 of them are beyond
// the default dynamic-LDS limit of a launch
static int thomas_corr_allow_lds(const void *kernel, size_t lds) {
  if (lds > 32 * 1024) HIPCHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

// The solve of set `which` of diagonals (seg.set) over the whole work array.  phase 0: whole column; 1: the slab's
// zero-inflow solution + its summary (slab.send); 2: after the exchange - the inflows composed from all ranks' summaries
// (slab.gath) and their responses added (k_thomas_corr)
static int launch_thomas(qgcm_hip_ctx *c, int which, int nlayers, int phase, const QgThomasSlabArgs &slab, bool cyc_part_a) {
  hipStream_t st = c->stream;
  const QgGeom &g = c->g;
  const int nranks = slab.nranks;
  if (!c->seg.set[which].tab.binf) QG_FAIL("k_thomas: the pivot tables have not been built (qgcm_hip_set_grid)");
  QgThomasParams P;
  fill_thomas_params(c, P, which, nlayers);
  P.gath = slab.gath; P.send = slab.send; P.rank = slab.rank; P.nranks = nranks;
  if (phase == 2) {
    if (g.cyc) P.ybnd = c->ybnd;
    c->slab_gath = slab.gath; // (the cyclic constraint algebra reads the boundary line sums at the end of the step messages)
    c->slab_nranks = nranks;
    P.cgath = (nranks == 1) ? c->slabDE : c->th_cgath; // a lone slab is its own rank 0
    if (nranks > 1 && (!c->th_cgath || c->th_cgath_ranks != nranks))
      QG_FAIL("qgcm_hip_thomas_phase: the set-up constants of the %d slabs have not been exchanged (qgcm_hip_set_thomas_consts)", nranks);
  }
  if (c->seg.S > 1) {
    if (phase == 1 || phase == 2) return launch_thomas_slab_seg(c, P, which, phase, nlayers, st);
    if (phase != 0 || !c->whole) QG_FAIL("k_thomas: phase %d on a column in %d segments", phase, c->seg.S);
    if (cyc_part_a) QG_FAIL("k_thomas: part A of the constraint algebra does not ride in the segmented solve");
    return launch_thomas_seg(c, P, which, nlayers, st);
  }
  if (phase == 2) {
    if (which != 0 || !c->seg.set[0].meta) QG_FAIL("k_thomas_corr: the response tables belong to the modal solves of qgcm_hip_set_grid");
    const QgThomasCorr T = thomas_corr_tables(c, 0);
    KTimer t(c, KN_THOMAS, st);
    const size_t lds = sizeof(double) * THC_LDS * nranks;
    if (thomas_corr_allow_lds((const void *)k_thomas_corr, lds)) return 1;
    hipLaunchKernelGGL(k_thomas_corr, dim3(P.nblk, nlayers, thomas_corr_slices(c->seg.maxlen)), dim3(THC_NT), lds, st, P, T);
    HIPCHECK(hipGetLastError());
    return 0;
  }
  if (phase == 0) {
    c->slab_gath = nullptr; // whole-column solve: the constraint algebra reads bpart
    if (g.cyc && nlayers == g.nl) P.ybnd = c->ybnd; // ... and the zonal-mean rows next to the boundaries from here
  }
  // zonally cyclic geometries use the CYCA instantiation for the whole-column solve: it fills ybnd, and its extra
  // workgroup runs part A of the constraint algebra when asked to (inside qgcm_hip_steps)
  const bool cyca = (phase == 0 && g.cyc);
  if (cyc_part_a && (phase != 0 || !c->d_cycq || g.nl > 4)) QG_FAIL("k_thomas: part A of the constraint algebra needs the homogeneous solutions and nlo <= 4");
  if (cyca) P.cycq = cyc_part_a ? c->d_cycq : nullptr; // (its extra workgroup is added to the grid below)
  return launch_thomas_rows(c, P, phase, cyca, nlayers, st);
}

// the k_thomas instantiation of the plan's rows per thread for the rows P.g.jr0 .. jr1; phases 4 / 5: set-up (k_thomas.h)
static int launch_thomas_rows(qgcm_hip_ctx *c, const QgThomasParams &P, int phase, bool cyca, int nlayers, hipStream_t st) {
  const QgGeom &g = c->g;
  KTimer t(c, KN_THOMAS, st);
#define QG_TH(RV, KWV)                                                                                                  \
  {                                                                                                                      \
    dim3 gridk((g.nk + KWV - 1) / KWV + (cyca ? 1 : 0), nlayers);                                                        \
    switch (phase) {                                                                                                     \
      case 0:                                                                                                            \
        if (cyca) hipLaunchKernelGGL((k_thomas<RV, 0, true, KWV>), gridk, dim3(KWV * TH_NC), 0, st, QG_TH_VALS(P), P); \
        else hipLaunchKernelGGL((k_thomas<RV, 0, false, KWV>), gridk, dim3(KWV * TH_NC), 0, st, QG_TH_VALS(P), P); \
        break;                                                                                                           \
      case 1: hipLaunchKernelGGL((k_thomas<RV, 1, false, KWV>), gridk, dim3(KWV * TH_NC), 0, st, QG_TH_VALS(P), P); break; \
      case 4: hipLaunchKernelGGL((k_thomas<RV, 4, false, KWV>), gridk, dim3(KWV * TH_NC), 0, st, QG_TH_VALS(P), P); break; \
      default: hipLaunchKernelGGL((k_thomas<RV, 5, false, KWV>), gridk, dim3(KWV * TH_NC), 0, st, QG_TH_VALS(P), P); break; \
    }                                                                                                                    \
  }
  // 8 .. 16 rows per thread: 512-thread workgroups of 8 wavenumbers, two per CU (128 VGPRs), the pair that shares the
  // 128-byte lines of a 16-wavenumber block on ONE XCD (k_thomas.h; r3: NAtl 5 km 10.6 -> 9.9 us against 1024-thread
  // workgroups); long columns (>= 20 rows per thread): 512 threads, 256 VGPRs
  switch (c->seg.R) {
    // (short columns too: 1024-thread workgroups of 16 wavenumbers measured slower everywhere - atmosphere 22.1 -> 21.3 us
    //  per step, 27.9 -> 26.3 on the two XCDs of a coupled run: profiles/r4_coupled_cu_masks.log)
#define QG_TH_CASE(RV) case RV: QG_TH(RV, 8); break;
    QG_TH_ROWS(QG_TH_CASE)
#undef QG_TH_CASE
    default: QG_FAIL("k_thomas: too many rows for the single-segment kernel");
  }
#undef QG_TH
  HIPCHECK(hipGetLastError());
  return 0;
}

// PHASE 1 of every segment at once (k_thomas_seg): P.send = the segments' summaries, the tables P's
static int launch_thomas_seg_rows(qgcm_hip_ctx *c, const QgThomasParams &P, const QgThomasSegRec *recs, int nlayers, hipStream_t st) {
  const QgGeom &g = c->g;
  KTimer t(c, KN_THOMAS, st);
  dim3 gridk((g.nk + 7) / 8, nlayers, c->seg.S);
  switch (c->seg.R) {
#define QG_TH_CASE(RV) case RV: hipLaunchKernelGGL((k_thomas_seg<RV, 1, 8>), gridk, dim3(8 * TH_NC), 0, st, P.wrk, recs, g.wstride, g.ldw, g.nk, P.layer0, P.nblk, P); break;
    QG_TH_ROWS(QG_TH_CASE)
#undef QG_TH_CASE
    default: QG_FAIL("k_thomas_seg: no instantiation for %d rows per thread", c->seg.R);
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

// The whole column of a handle whose plan has S > 1 segments, two launches with nothing of the host in between:
// k_thomas_seg (PHASE 1 of every segment, summaries into seg.msg) and k_thomas_corr_seg (inflows composed from seg.msg
// and the set-up constants, responses added, ksum / ybnd published).  P: launch_thomas's; which: the set of diagonals
static int launch_thomas_seg(qgcm_hip_ctx *c, QgThomasParams &P, int which, int nlayers, hipStream_t st) {
  const QgGeom &g = c->g;
  const auto &sg = c->seg;
  const auto &ss = sg.set[which];
  const int nlt = which ? 1 : g.nl, S = sg.S;
  if (!ss.recs || !ss.meta || !ss.ptab || !ss.qtab) QG_FAIL("k_thomas_seg: the segments' tables have not been built for these diagonals");
  if (nlayers > nlt) QG_FAIL("k_thomas_seg: %d layers asked of tables of %d", nlayers, nlt);
  P.send = sg.msg; P.gath = sg.msg; P.gath_stride = (long)TH_MSG * nlt * g.ldw;
  P.slabDE = ss.cst; P.cgath = ss.cst;
  P.rank = 0; P.nranks = S;
  c->slab_gath = nullptr; // whole-column solve: the constraint algebra reads bpart
  if (g.cyc && nlayers == g.nl) P.ybnd = c->ybnd;
  if (launch_thomas_seg_rows(c, P, ss.recs, nlayers, st)) return 1;
  {
    const QgThomasCorr T = thomas_corr_tables(c, which);
    KTimer t(c, KN_THOMAS, st);
    const size_t lds = sizeof(double) * THC_LDS * S;
    if (thomas_corr_allow_lds((const void *)k_thomas_corr_seg, lds)) return 1;
    const int nslice = thomas_corr_slices(sg.maxlen);
    hipLaunchKernelGGL(k_thomas_corr_seg, dim3(P.nblk, nlayers, S * nslice), dim3(THC_NT), lds, st, P, T, (const QgThomasSegRec *)ss.recs, nslice);
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

// The slab phases of a handle whose plan has S > 1 segments (k_thomas_slab.h), two launches each with nothing of the host
// in between.  1: k_thomas_seg (the segments' summaries into seg.msg) and k_thomas_fold (the slab's ONE summary into
// P.send, every segment's zero-inflow inflows into seg.ab); 2: k_thomas_corr_slab.  P: launch_thomas's, for phase 2
// with the ranks' summaries and constants in place
static QgThomasFold thomas_fold_params(const qgcm_hip_ctx *c, double *send) {
  const auto &sg = c->seg;
  QgThomasFold F;
  F.msg = sg.msg; F.cst = sg.set[0].cst; F.coef = sg.coef; F.ab = sg.ab;
  F.send = send; F.slabDE = c->slabDE;
  F.S = sg.S; F.nl = c->g.nl; F.ldw = c->g.ldw; F.nk = c->g.nk;
  return F;
}
static int launch_thomas_slab_seg(qgcm_hip_ctx *c, QgThomasParams &P, int which, int phase, int nlayers, hipStream_t st) {
  const QgGeom &g = c->g;
  const auto &sg = c->seg;
  const auto &ss = sg.set[0];
  if (which != 0 || nlayers != g.nl) QG_FAIL("qgcm_hip_thomas_phase: a column in segments folds all modal solves at once");
  if (!ss.recs || !ss.meta || !sg.coef || !sg.ab) QG_FAIL("qgcm_hip_thomas_phase: the segments' tables have not been built (qgcm_hip_set_grid)");
  const QgThomasFold F = thomas_fold_params(c, P.send);
  if (phase == 1) {
    P.send = sg.msg; P.slabDE = ss.cst;
    if (launch_thomas_seg_rows(c, P, ss.recs, nlayers, st)) return 1;
    KTimer t(c, KN_THOMAS, st);
    HIPCHECK(qg_launch_thomas_fold(false, st, F));
    return 0;
  }
  const QgThomasCorr T = thomas_corr_tables(c, 0);
  KTimer t(c, KN_THOMAS, st);
  HIPCHECK(qg_launch_thomas_corr_slab(st, P, T, ss.recs, F, thomas_corr_slices(sg.maxlen), nlayers));
  return 0;
}

static int launch_constr(qgcm_hip_ctx *c) {
  const QgGeom &g = c->g;
  if (g.cyc) {
    QgCycConstrParams Q;
    fill_cyc_constr_params(c, Q);
    KTimer t(c, KN_CONSTR);
#define QG_CONSTR_CYC(NLV) hipLaunchKernelGGL((k_constr_cyc<NLV>), dim3(1), dim3(64), 0, c->stream, Q)
    QG_SWITCH_NL(g.nl, QG_CONSTR_CYC, "k_constr_cyc");
#undef QG_CONSTR_CYC
    HIPCHECK(hipGetLastError());
    return 0;
  }
  QgConstrParams P;
  fill_constr_params(c, P);
  KTimer t(c, KN_CONSTR);
#define QG_CONSTR_BOX(NLV) hipLaunchKernelGGL((k_constr_box<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_CONSTR_BOX, "k_constr");
#undef QG_CONSTR_BOX
  HIPCHECK(hipGetLastError());
  return 0;
}

static void fill_bdy_params(qgcm_hip_ctx *c, QgBdyParams &P) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.po = c->p[c->ip];
  P.qo = c->q[c->iq];
  P.ddynoc = c->ddynoc;
  P.yporel = c->yporel;
  const double dxom2 = 1.0 / (pr.dxo * pr.dxo);
  P.bcfaco_f0 = pr.bccooc * dxom2 / (0.5 * pr.bccooc + 1.0) / pr.fnot; // src/vorsubs.F:268
  P.beta = pr.beta;
  for (int k = 0; k < g.nl; ++k)
    for (int l = 0; l < g.nl; ++l) P.f0A[k + g.nl * l] = pr.fnot * pr.amatoc[k + g.nl * l];
}

// The kernel arguments of the four unpack launchers below, filled once: D for the row kernels (null: the stand-alone
// unpack), P for the unpack kernels, B for the boundary PV (B.qo = current qo; B.po unused by the fused kernels).  msg_lo /
// msg_hi: the y-slab halo messages written by the same threads (the slab's solve and unpack).  avg: an averaging step of
// one_step, the launch stores the averaged level; avg_ok: this launch is the fused whole-domain kernel that can (`who` names it otherwise)
static int fill_inv_args(qgcm_hip_ctx *c, QgDstParams *D, QgUnpackParams &P, QgBdyParams &B, double *msg_lo, double *msg_hi, const char *who, bool avg, bool avg_ok) {
  const QgGeom &g = c->g;
  if (D) fill_dst_params(c, *D, c->wrk, g.nl, 0);
  fill_bdy_params(c, B);
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.wrk = c->wrk;
  P.ochom = c->ochom;
  P.pnew = c->p[c->ip ^ 1];
  P.sc = c->sc;
  P.pch1 = c->pch1; P.pch2 = c->pch2; P.pbh = c->pbh;
  P.msg_lo = msg_lo;
  P.msg_hi = msg_hi;
  for (int i = 0; i < g.nl * g.nl; ++i) P.ctm2l[i] = c->prm.ctm2loc[i];
  if (avg) {
    if (msg_lo || msg_hi || !avg_ok) QG_FAIL("%s: the fused leapfrog averaging belongs to whole-domain steps", who);
    P.pavg = c->p[c->ip];     // this step's po (the launch writes the old pom buffer)
    P.qavg = c->q[c->iq ^ 1]; // this step's qo (iq already points at the new qo)
  }
  return 0;
}

static int launch_unpack(qgcm_hip_ctx *c, bool fuse_bdy, double *msg_lo = nullptr, double *msg_hi = nullptr, bool avg = false) {
  const QgGeom &g = c->g;
  if ((msg_lo || msg_hi) && (!fuse_bdy || g.jhi - g.jlo + 1 < 3)) QG_FAIL("k_unpack: halo messages need the fused boundary PV and three owned rows");
  QgUnpackParams P;
  QgBdyParams B;
  if (fill_inv_args(c, nullptr, P, B, msg_lo, msg_hi, "k_unpack", avg, false)) return 1;
  dim3 grid((g.nx + 255) / 256, g.jhi - g.jlo + 1);
  KTimer t(c, KN_UNPACK);
#define QG_UNPACK(NLV)                                                                                   \
  if (g.cyc && fuse_bdy) hipLaunchKernelGGL((k_unpack_cyc<NLV, true>), grid, dim3(256), 0, c->stream, P, B);       \
  else if (g.cyc) hipLaunchKernelGGL((k_unpack_cyc<NLV, false>), grid, dim3(256), 0, c->stream, P, B);             \
  else if (fuse_bdy) hipLaunchKernelGGL((k_unpack_box<NLV, true>), grid, dim3(256), 0, c->stream, P, B); \
  else hipLaunchKernelGGL((k_unpack_box<NLV, false>), grid, dim3(256), 0, c->stream, P, B)
  QG_SWITCH_NL(g.nl, QG_UNPACK, "k_unpack");
#undef QG_UNPACK
  HIPCHECK(hipGetLastError());
  return 0;
}

// cyclic / atmosphere fast path: inverse rows + homogeneous corrections + modes -> layers (+ zonal-boundary PV) in
// one launch (k_rfft64_unpack), nxto = 64 * {3, 6, 15}: step_plan's INV_RFFT64_UNPACK
static int launch_rfft_unpack(qgcm_hip_ctx *c, bool fuse_bdy, bool constr, bool avg = false) {
  const QgGeom &g = c->g;
  QgDstParams D;
  QgUnpackParams P;
  QgBdyParams B;
  if (fill_inv_args(c, &D, P, B, nullptr, nullptr, "k_rfft64_unpack", avg, false)) return 1;
  if (constr && !c->d_cycq) QG_FAIL("k_rfft64_unpack: homogeneous solutions not set");
  QgCycConstrParams Qv; // by value: kernel arguments (k_rfft64.h)
  fill_cyc_constr_params(c, Qv);
  const int nrows = g.jr1 - g.jr0 + 1;
  dim3 grid((nrows + 1) / 2);
  KTimer t(c, KN_DSTI);
#define QG_RU(MV, NLV)                                                                                                        \
  if (fuse_bdy && constr) hipLaunchKernelGGL((k_rfft64_unpack<MV, NLV, true, true>), grid, dim3(64 * (NLV + 1)), 0, c->stream, D, P, B, Qv); \
  else if (fuse_bdy) hipLaunchKernelGGL((k_rfft64_unpack<MV, NLV, true, false>), grid, dim3(64 * NLV), 0, c->stream, D, P, B, Qv); \
  else hipLaunchKernelGGL((k_rfft64_unpack<MV, NLV, false, false>), grid, dim3(64 * NLV), 0, c->stream, D, P, B, Qv)
#define QG_RU_NL(MV)                 \
  switch (g.nl) {                    \
    case 2: QG_RU(MV, 2); break;     \
    case 3: QG_RU(MV, 3); break;     \
    default: QG_RU(MV, 4); break;    \
  }
  switch (step_plan(c).m64) {
    case 15: QG_RU_NL(15) break;
    case 6: QG_RU_NL(6) break;
    default: QG_RU_NL(3) break;
  }
#undef QG_RU_NL
#undef QG_RU
  HIPCHECK(hipGetLastError());
  return 0;
}

// long rows (three-stage plans): inverse rows + homogeneous corrections + modes -> layers + boundary PV in one launch
// that reads the solved modes once (k_fft3_unpack.h); nlo = 3, the boundary PV always fused: step_plan's INV_FFT3_UNPACK
// (own_constr: every workgroup evaluates part B of the constraint algebra for itself)
static bool can_fuse_fft3_unpack(const qgcm_hip_ctx *c) { return step_plan(c, true, true).inv == INV_FFT3_UNPACK; } // (the slab stages' plan: wherever the kernel exists)

static int launch_fft3_unpack(qgcm_hip_ctx *c, bool own_constr, double *msg_lo = nullptr, double *msg_hi = nullptr, bool avg = false) {
  const QgGeom &g = c->g;
  if (!can_fuse_fft3_unpack(c)) QG_FAIL("k_fft3_unpack: not a long-row configuration of three layers");
  if ((msg_lo || msg_hi) && g.jhi - g.jlo + 1 < 3) QG_FAIL("k_fft3_unpack: halo messages need three owned rows");
  QgDstParams D;
  QgUnpackParams P;
  QgBdyParams B;
  if (fill_inv_args(c, &D, P, B, msg_lo, msg_hi, "k_rfft3_unpack", avg, own_constr)) return 1;
  const int npairs = (g.jr1 - g.jr0 + 2) / 2;
  dim3 grid(8 * ((npairs + 7) / 8) * g.nl);
  KTimer t(c, KN_DSTI);
  QgCycConstrParams Q;
  fill_cyc_constr_params(c, Q);
#define QG_FFT3U_LAUNCH(ID, R1, R2, R3)                                                                                   \
  if (c->fft3 == ID) {                                                                                                    \
    typedef Fft3Plan<R1, R2, R3> PL;                                                                                      \
    if (avg) hipLaunchKernelGGL((k_rfft3_unpack<PL, 3, FFT3_NT, true>), grid, dim3(FFT3_NT), c->fft3_lds, c->stream, D, P, B, Q, 1); \
    else hipLaunchKernelGGL((k_rfft3_unpack<PL, 3, FFT3_NT>), grid, dim3(FFT3_NT), c->fft3_lds, c->stream, D, P, B, Q, own_constr ? 1 : 0); \
  }
  QG_FFT3_PLANS(QG_FFT3U_LAUNCH)
#undef QG_FFT3U_LAUNCH
  HIPCHECK(hipGetLastError());
  return 0;
}

// box fast path: inverse row transform + modes -> layers (+ boundary PV) in one launch (k_dst64_unpack): step_plan's
// INV_DST64_UNPACK
static int launch_dst_unpack(qgcm_hip_ctx *c, bool fuse_bdy, double *msg_lo = nullptr, double *msg_hi = nullptr,
                             bool constr = false, bool avg = false) {
  const QgGeom &g = c->g;
  QgDstParams D;
  QgUnpackParams P;
  QgBdyParams B;
  if (fill_inv_args(c, &D, P, B, msg_lo, msg_hi, "k_dst64_unpack", avg, fuse_bdy && constr)) return 1;
  QgConstrLite C;
  fill_constr_lite(c, C);
  const int nrows = g.jr1 - g.jr0 + 1;
  dim3 grid((nrows + 1) / 2);
  KTimer t(c, KN_DSTI);
#define QG_DU(MV, NLV)                                                                                                  \
  if (avg) hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, true, false, true, true>), grid, dim3(64 * (NLV + 1)), 0, c->stream, QG_ROW_VALS(D), P, B, C); \
  else if ((msg_lo || msg_hi) && constr) hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, true, true, true>), grid, dim3(64 * (NLV + 1)), 0, c->stream, QG_ROW_VALS(D), P, B, C); \
  else if (msg_lo || msg_hi) hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, true, true, false>), grid, dim3(64 * NLV), 0, c->stream, QG_ROW_VALS(D), P, B, C); \
  else if (fuse_bdy && constr) hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, true, false, true>), grid, dim3(64 * (NLV + 1)), 0, c->stream, QG_ROW_VALS(D), P, B, C); \
  else if (fuse_bdy) hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, true, false, false>), grid, dim3(64 * NLV), 0, c->stream, QG_ROW_VALS(D), P, B, C); \
  else hipLaunchKernelGGL((k_dst64_unpack<MV, NLV, false, false, false>), grid, dim3(64 * NLV), 0, c->stream, QG_ROW_VALS(D), P, B, C)
#define QG_DU_NL(MV)                 \
  switch (g.nl) {                    \
    case 2: QG_DU(MV, 2); break;     \
    case 3: QG_DU(MV, 3); break;     \
    default: QG_DU(MV, 4); break;    \
  }
  if (step_plan(c).m64 == 15) {
    QG_DU_NL(15)
  } else {
    QG_DU_NL(3)
  }
#undef QG_DU_NL
#undef QG_DU
  HIPCHECK(hipGetLastError());
  return 0;
}

// the boundary PV of pressure po into qo, device fields of the handle's shape (of the epilogue's arguments, B alone)
static int launch_ocqbdy_on(qgcm_hip_ctx *c, const double *po, double *qo) {
  const QgGeom &g = c->g;
  QgBdyParams P;
  fill_bdy_params(c, P);
  P.po = po; P.qo = qo;
  const int nmax = g.nx > g.ny ? g.nx : g.ny;
  dim3 grid((nmax + 255) / 256, g.cyc ? 2 : 4, g.nl);
  hipLaunchKernelGGL(k_ocqbdy, grid, dim3(256), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

static int launch_ocqbdy(qgcm_hip_ctx *c) {
  KTimer t(c, KN_OCQBDY);
  return launch_ocqbdy_on(c, c->p[c->ip], c->q[c->iq]);
}

static int launch_lfavg(qgcm_hip_ctx *c) {
  const QgGeom &g = c->g;
  const long n = g.fstride * g.nl;
  KTimer t(c, KN_LFAVG);
  hipLaunchKernelGGL(k_lf_average, dim3(2048), dim3(256), 0, c->stream, c->q[c->iq], c->q[c->iq ^ 1], c->p[c->ip],
                     c->p[c->ip ^ 1], n, c->sc, g.nl, g.cyc);
  HIPCHECK(hipGetLastError());
  return 0;
}

static int check_ready(qgcm_hip_ctx *c, const char *who) {
  if (!c) QG_FAIL("%s: null handle", who);
  if (!c->grid_set) QG_FAIL("%s: qgcm_hip_set_grid has not been called", who);
  return 0;
}

extern "C" int qgcm_hip_qgostep(qgcm_hip_handle c) {
  if (check_ready(c, "qgcm_hip_qgostep")) return 1;
  if (launch_tend(c)) return 1;
  c->iq ^= 1; // the old qom buffer now holds qo; the old qo is qom
  return 0;
}

// The plan's inverse rows and unpack, fused or not, with the constraint parts the plan lets ride in them.  A whole-domain
// inversion (ocinvq_impl) has no halo messages and lets every workgroup of k_rfft3_unpack evaluate part B for itself
// (own_constr); a slab's solve and unpack (slab_solve_unpack) passes the messages the unpack threads also write.
static int launch_inverse(qgcm_hip_ctx *c, const QgStepPlan &pl, bool fuse_bdy, double *msg_lo, double *msg_hi, bool own_constr, bool avg) {
  switch (pl.inv) {
    case INV_DST64_UNPACK: return launch_dst_unpack(c, fuse_bdy, msg_lo, msg_hi, pl.constr == CONSTR_INV_WAVE, avg);
    case INV_RFFT64_UNPACK: return launch_rfft_unpack(c, fuse_bdy, pl.constr == CONSTR_AB, avg); // (3 launches after k_tend instead of 5)
    case INV_FFT3_UNPACK: return launch_fft3_unpack(c, own_constr, msg_lo, msg_hi, avg);
    default:
      if (launch_dst(c, c->wrk, c->g.nl, true, 0, nullptr, pl.constr == CONSTR_AB, pl.constr == CONSTR_BOX_WG)) return 1;
      return launch_unpack(c, fuse_bdy, msg_lo, msg_hi, avg);
  }
}

// in_step: called from qgcm_hip_steps, where k_tend has already stepped dpioc / dpiocp where the plan says so
// (launch_tend(c, pl.upd_dpi)) and ocqbdy is fused into the unpack; the launches are step_plan's.  avg: one_step's
// averaging step, the fused inverse kernel stores the averaged level
static int ocinvq_impl(qgcm_hip_ctx *c, bool in_step = false, bool avg = false, bool fwd_done = false) {
  if (check_ready(c, "qgcm_hip_ocinvq")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_ocinvq: this handle is a y-slab; drive it with the slab building blocks");
  if (!c->homog_set) QG_FAIL("qgcm_hip_ocinvq: homogeneous solutions not set");
  const QgStepPlan pl = step_plan(c, in_step);
  // (A per-mode side-stream variant of this chain was measured slower - 140 vs 116 us/step at 5 km - and removed.)
  if (!fwd_done && launch_dst(c, c->wrk, c->g.nl, false)) return 1; // (fwd_done: k_tend_rows has left the spectral rows in wrk)
  if (launch_thomas(c, 0, c->g.nl, 0, {}, pl.constr == CONSTR_AB)) return 1;
  // area (and, cyclic, line) integrals are a by-product of the y sweeps: the constraints precede the inverse transform
  if (pl.constr == CONSTR_OWN && launch_constr(c)) return 1;
  if (launch_inverse(c, pl, in_step, nullptr, nullptr, true, avg)) return 1; // (fuse_bdy = in_step)
  c->ip ^= 1; // new po sits in the old pom buffer; the old po is pom
  return 0;
}

extern "C" int qgcm_hip_ocinvq(qgcm_hip_handle c) { return ocinvq_impl(c); }

extern "C" int qgcm_hip_ocqbdy(qgcm_hip_handle c) {
  if (check_ready(c, "qgcm_hip_ocqbdy")) return 1;
  return launch_ocqbdy(c);
}

// ocqbdy / atqzbd on host arrays (start-up calls of the main program, src/q-gcm.F:724-725, 743-744)
extern "C" int qgcm_hip_ocqbdy_host(qgcm_hip_handle c, double *q, const double *p) {
  if (!c) QG_FAIL("qgcm_hip_ocqbdy_host: null handle");
  if (!c->geom_set) QG_FAIL("qgcm_hip_ocqbdy_host: neither qgcm_hip_set_geometry nor qgcm_hip_set_grid has been called");
  if (!q || !p) QG_FAIL("qgcm_hip_ocqbdy_host: null argument");
  if (!c->whole) QG_FAIL("qgcm_hip_ocqbdy_host: only for a handle that owns the whole domain");
  const QgGeom &g = c->g;
  const size_t n = (size_t)g.fstride * g.nl;
  QgDbl dp, dq; // scratch
  if (dp.alloc(n, "the scratch copy of p") || dq.alloc(n, "the scratch copy of q")) return 1;
  const long rows = (long)g.ny * g.nl;
  int rc = upload2d(c, dp, g.ldx, p, g.nx, rows) || upload2d(c, dq, g.ldx, q, g.nx, rows);
  if (!rc && (rc = launch_ocqbdy_on(c, dp, dq))) snprintf(g_err, sizeof(g_err), "qgcm_hip_ocqbdy_host: launch failed");
  if (!rc) rc = download2d(c, q, dq, g.ldx, g.nx, rows);
  return rc;
}

static int launch_aml(qgcm_hip_ctx *c, bool with_final);
static int launch_aml_average(qgcm_hip_ctx *c);

// ---------------------------------------------------------------------------
// ocean mixed layer
// ---------------------------------------------------------------------------
extern "C" int qgcm_hip_oml_init(qgcm_hip_handle c, const qgcm_hip_oml_params *p) {
  if (check_ready(c, "qgcm_hip_oml_init")) return 1;
  if (!p) QG_FAIL("qgcm_hip_oml_init: null parameters");
  if (c->sc_comm) QG_FAIL("qgcm_hip_oml_init: call before qgcm_hip_comm_init (the step and halo messages grow by the mixed layer's parts)");
  if (!(p->hmoc > 0.0) || p->toc1 == p->toc2) QG_FAIL("qgcm_hip_oml_init: need hmoc > 0 and toc(1) != toc(2)");
  const QgGeom &g = c->g;
  const int nxt = g.nxt, nyt = g.ny - 1;
  if (nxt < 3 || nyt < 3) QG_FAIL("qgcm_hip_oml_init: grid too small");
  auto &o = c->oml;
  drop_graphs(c);
  o.prm = *p;
  if (!o.diag) { // (the last of the buffers: a call that failed half-way is made good by the next)
    o.ldt = round_up(nxt, 16);
    const size_t nT = (size_t)o.ldt * nyt, nP = (size_t)g.ldx * g.ny;
    o.nblkA = ((nxt + OML_TX - 1) / OML_TX) * ((nyt + OML_SH - 1) / OML_SH);
    o.nblkB = ((g.nx + OML_TX - 1) / OML_TX) * ((g.ny + OML_TY * OML_RPT * OML_ERR - 1) / (OML_TY * OML_RPT * OML_ERR));
    struct { QgDbl *buf; size_t n; } bufs[] = {{&o.sst[0], nT}, {&o.sst[1], nT}, {&o.sst[2], nT}, {&o.fnet, nT}, {&o.wekto, nT},
                                               {&o.xfo, nT}, {&o.taux, nP}, {&o.tauy, nP}, {&o.partA, (size_t)3 * o.nblkA},
                                               {&o.partB, (size_t)3 * o.nblkB}, {&o.diag, 2}};
    for (auto &b : bufs)
      if (b.buf->ensure(b.n, "a buffer of the ocean mixed layer")) return 1;
    o.is = 0;
    o.ism = 1;
  }
  o.on = true;
  c->entoc_zero = false; // the mixed layer writes entoc every step from now on (tend_zmask: never skipped again)
  return 0;
}

static int oml_ready(qgcm_hip_ctx *c, const char *who) {
  if (check_ready(c, who)) return 1;
  if (!c->oml.on) QG_FAIL("%s: qgcm_hip_oml_init has not been called", who);
  return 0;
}

extern "C" int qgcm_hip_oml_set_state(qgcm_hip_handle c, const double *sst, const double *sstm) {
  if (oml_ready(c, "qgcm_hip_oml_set_state")) return 1;
  const int nxt = c->g.nxt, nyt = c->g.ny - 1;
  if (sst && upload2d(c, c->oml.sst[c->oml.is], c->oml.ldt, sst, nxt, nyt)) return 1;
  if (sstm && upload2d(c, c->oml.sst[c->oml.ism], c->oml.ldt, sstm, nxt, nyt)) return 1;
  return 0;
}

extern "C" int qgcm_hip_oml_get_state(qgcm_hip_handle c, double *sst, double *sstm) {
  if (oml_ready(c, "qgcm_hip_oml_get_state")) return 1;
  const int nxt = c->g.nxt, nyt = c->g.ny - 1;
  if (sst && download2d(c, sst, c->oml.sst[c->oml.is], c->oml.ldt, nxt, nyt)) return 1;
  if (sstm && download2d(c, sstm, c->oml.sst[c->oml.ism], c->oml.ldt, nxt, nyt)) return 1;
  return 0;
}

extern "C" int qgcm_hip_oml_set_forcing(qgcm_hip_handle c, const double *fnetoc, const double *wekto, const double *tauxo,
                                        const double *tauyo) {
  if (oml_ready(c, "qgcm_hip_oml_set_forcing")) return 1;
  const QgGeom &g = c->g;
  const int nxt = g.nxt, nyt = g.ny - 1;
  if (fnetoc && upload2d(c, c->oml.fnet, c->oml.ldt, fnetoc, nxt, nyt)) return 1;
  if (wekto && upload2d(c, c->oml.wekto, c->oml.ldt, wekto, nxt, nyt)) return 1;
  if (tauxo && upload2d(c, c->oml.taux, g.ldx, tauxo, g.nx, g.ny)) return 1;
  if (tauyo && upload2d(c, c->oml.tauy, g.ldx, tauyo, g.nx, g.ny)) return 1;
  return 0;
}

static void fill_oml_params(qgcm_hip_ctx *c, QgOmlParams &P) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  auto &o = c->oml;
  const qgcm_hip_oml_params &q = o.prm;
  memset(&P, 0, sizeof(P));
  P.nxt = g.nxt; P.nyt = g.ny - 1; P.nx = g.nx; P.ny = g.ny; P.cyc = g.cyc; P.sb = q.sb_hflux; P.nb = q.nb_hflux;
  P.ldt = o.ldt; P.ldx = g.ldx;
  // y-slab view (k_oml.h): T row j lies between p rows j and j+1
  P.joff = g.joff; P.nyg = g.nyg; P.nytg = g.nyg - 1;
  P.jP0 = g.jlo; P.jP1 = g.jhi;
  P.jT0 = g.jlo; P.jT1 = (g.jhi + g.joff == g.nyg) ? g.jhi - 1 : g.jhi;
  P.jX0 = (g.jlo + g.joff > 1) ? P.jT0 - 1 : P.jT0;
  const int spare = 3 - o.is - o.ism;
  P.sst = o.sst[o.is]; P.sstm = o.sst[o.ism]; P.sstn = o.sst[spare];
  P.fnet = o.fnet; P.wekto = o.wekto; P.xfo = o.xfo;
  P.po1 = c->p[c->ip]; P.taux = o.taux; P.tauy = o.tauy;
  P.entoc = c->entoc;
  P.partA = o.partA; P.partB = o.partB;
  P.nblkA = ((P.nxt + OML_TX - 1) / OML_TX) * ((P.jT1 - P.jX0 + 1 + OML_SH - 1) / OML_SH);
  P.nblkB = ((P.nx + OML_TX - 1) / OML_TX) * ((P.jP1 - P.jP0 + 1 + OML_TY * OML_RPT * OML_ERR - 1) / (OML_TY * OML_RPT * OML_ERR));
  P.sc = c->sc; P.diag = o.diag;
  const double dxom2 = 1.0 / (pr.dxo * pr.dxo), rdxof0 = 1.0 / (pr.dxo * pr.fnot); // src/q-gcm.F:435
  P.uvgfac = q.ycexp * rdxof0;           // src/omlsubs.F:274-277
  P.rhf0hm = 0.5 / (pr.fnot * q.hmoc);
  P.d2tfac = q.st2d * dxom2;
  P.d4tfac = q.st4d * (dxom2 * dxom2);
  P.hdxom1 = 0.5 / pr.dxo;
  P.hmoinv = 1.0 / q.hmoc;               // src/omlsubs.F:78-80
  P.dtoinv = 1.0 / (q.toc1 - q.toc2);
  P.entfac = q.hmoc * P.dtoinv / pr.tdto;
  P.tdto = pr.tdto; P.rrcpoc = q.rrcpoc; P.toc1 = q.toc1; P.tsbdy = q.tsbdy; P.tnbdy = q.tnbdy;
  P.ocnorm = 1.0 / ((double)P.nxt * (double)P.nytg); // src/parameters_data.F:88
  P.dxo = pr.dxo; P.dyo = pr.dyo;
}

// first half of `oml`: new sst, raw entrainment, per-workgroup partial sums.  send3 (y-slabs): this slab's three sums
static int launch_oml_a(qgcm_hip_ctx *c, double *send3) {
  QgOmlParams P;
  fill_oml_params(c, P);
  dim3 gA((P.nxt + OML_TX - 1) / OML_TX, (P.jT1 - P.jX0 + 1 + OML_SH - 1) / OML_SH);
  hipLaunchKernelGGL(k_oml_step, gA, dim3(OML_NT), 0, c->stream, P);
  if (send3) hipLaunchKernelGGL(k_oml_sum3, dim3(1), dim3(OML_NT), 0, c->stream, (const double *)P.partA, P.nblkA, send3);
  HIPCHECK(hipGetLastError());
  return 0;
}

// second half: entoc from the entrainment minus its basin-wide mean (gath3 (3, nranks): every slab's sums, or nullptr
// for a handle that owns the whole domain), then the rotation of the sst buffers
static int launch_oml_b(qgcm_hip_ctx *c, const double *gath3, int nranks) {
  auto &o = c->oml;
  QgOmlParams P;
  fill_oml_params(c, P);
  P.mean_gath = gath3;
  P.nranks = nranks;
  dim3 gB((P.nx + OML_TX - 1) / OML_TX, (P.jP1 - P.jP0 + 1 + OML_TY * OML_RPT * OML_ERR - 1) / (OML_TY * OML_RPT * OML_ERR));
  c->entoc_zero = false; // (k_oml_entoc writes entoc)
  hipLaunchKernelGGL(k_oml_entoc, gB, dim3(OML_NT), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  // rotation: sstm <- sst, sst <- new (src/omlsubs.F:125-126)
  const int spare = 3 - o.is - o.ism;
  o.ism = o.is;
  o.is = spare;
  return 0;
}

// with_final = false: the final reduction rides in workgroup 0 of the tendency launch that follows (one_step)
static int launch_oml(qgcm_hip_ctx *c, bool with_final = true) {
  {
    KTimer t(c, KN_OML);
    if (launch_oml_a(c, nullptr)) return 1;
  }
  {
    KTimer t(c, KN_OML_ENTOC);
    if (launch_oml_b(c, nullptr, 1)) return 1;
  }
  if (with_final) {
    QgOmlFinal F;
    fill_oml_final(c, F, true);
    hipLaunchKernelGGL(k_oml_final, dim3(1), dim3(OML_NT), 0, c->stream, F);
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_oml(qgcm_hip_handle c) {
  if (oml_ready(c, "qgcm_hip_oml")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_oml: this handle is a y-slab; the mixed layer steps with the slab stages 10 / 11");
  return launch_oml(c);
}

static int launch_oml_average(qgcm_hip_ctx *c) {
  const long n = (long)c->oml.ldt * (c->g.ny - 1);
  hipLaunchKernelGGL(k_oml_average, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->oml.sst[c->oml.is],
                     (const double *)c->oml.sst[c->oml.ism], n);
  HIPCHECK(hipGetLastError());
  return 0;
}

// the whole ocean part of the averaging block src/q-gcm.F:1328-1366: po, qo, constraint scalars and - when the
// mixed layer lives on the device - sst
extern "C" int qgcm_hip_lf_average(qgcm_hip_handle c) {
  if (check_ready(c, "qgcm_hip_lf_average")) return 1;
  if (launch_lfavg(c)) return 1;
  if (c->oml.on && launch_oml_average(c)) return 1;
  if (c->aml.on && launch_aml_average(c)) return 1; // ast, hmixa: src/q-gcm.F:1388-1394
  return 0;
}

extern "C" int qgcm_hip_oml_get_diag(qgcm_hip_handle c, double *entoc, double *diag) {
  if (oml_ready(c, "qgcm_hip_oml_get_diag")) return 1;
  const QgGeom &g = c->g;
  if (entoc && download2d(c, entoc, c->entoc, g.ldx, g.nx, g.ny)) return 1;
  if (diag) {
    QgScalars h;
    double d[2];
    HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(d, c->oml.diag, sizeof(d), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    diag[0] = h.xon[0]; diag[1] = d[0]; diag[2] = d[1];
    diag[3] = g.cyc ? h.enisoc[0] : 0.0; diag[4] = g.cyc ? h.eninoc[0] : 0.0;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// the on-device diagnostics: valids, monitors, start-up arithmetic, time averages, dumps, covariances
// ---------------------------------------------------------------------------
#include "diag_host.h"

// The accumulations qgcm_hip_steps launches after a scheduled step, in the reference's order (tavatm, then covocn /
// covatm: src/q-gcm.F:1477-1489): the schedule, the check that every input is there, the contribution
static const struct {
  int sched;
  int (*inputs)(qgcm_hip_ctx *, const char *);
  int (*launch)(qgcm_hip_ctx *, const char *);
  const char *who;
} kAccum[] = {{SCH_TAVATM, tavatm_inputs, launch_tavatm, "qgcm_hip_steps (qgcm_hip_tavatm_schedule)"},
              {SCH_COV, cov_inputs, launch_cov, "qgcm_hip_steps (qgcm_hip_cov_schedule)"}};

// the contributions due after step s (asynchronous, never captured)
static int launch_accums(qgcm_hip_ctx *c, int s) {
  for (const auto &a : kAccum)
    if (sched_due(c->sched[a.sched], s) && a.launch(c, "qgcm_hip_steps")) return 1;
  return 0;
}

// How many of the n steps from s may run as one block: up to, not including, the next dump step (it records inside
// the step) and up to and including the next accumulation step (its contribution follows the step)
static int sched_block(const qgcm_hip_ctx *c, int s, int n) {
  for (int i = 0; i < SCH_COUNT; ++i) n = std::min(n, sched_dist(c->sched[i], s) + (i == SCH_DUMP ? 0 : 1));
  return n;
}

static int avg_phase(const qgcm_hip_ctx *c, int s) { return (s - 1) % c->avg_period; }
static bool avg_after(const qgcm_hip_ctx *c, int s) { return avg_phase(c, s) == 0; } // step s ends with a leapfrog averaging

static int one_step(qgcm_hip_ctx *c, int s) {
  if (c->oml.on && launch_oml(c, false)) return 1; // src/q-gcm.F:1232; its final reduction rides in launch_tend
  if (c->aml.on && launch_aml(c, false)) return 1; // src/q-gcm.F:1260, immediately before qgastep; likewise
  if (sched_due(c->sched[SCH_DUMP], s) && qd_record(c, s)) return 1; // qocdiag_out after oml, before qgostep (src/q-gcm.F:1234-1239)
  if (check_ready(c, "qgcm_hip_steps")) return 1;
  const QgStepPlan pl = step_plan(c, true);
  // Leapfrog averaging (src/q-gcm.F:1345-1351) after this step: where the box ocean's fused kernels run, they store the
  // averaged level themselves - k_tend the interior qo (both levels are in its registers), k_dst64_unpack the new po and
  // the boundary qo (one extra read of this step's po) - instead of a pass of its own over six fields (133 MB at 5 km,
  // 21 us every 25 steps); the integrals dpioc follow in a one-thread launch.  Same expressions: bitwise the same fields.
  const bool avg = avg_after(c, s);
  const bool avg_fused = avg && pl.avg_ok; // (long-row cyclic oceans: k_rfft3_unpack<.., AVG> does what k_dst64_unpack does for the box)
  // (the 5 km box ocean's plain steps: tendency and forward rows in one launch; averaging steps keep the two)
  const bool rows_fused = pl.band_rows && !avg;
  if (rows_fused ? launch_tend_rows(c, pl.upd_dpi) : launch_tend(c, pl.upd_dpi, c->oml.on || c->aml.on, TEND_ALL, avg_fused)) return 1;
  c->iq ^= 1; // as qgcm_hip_qgostep
  if (ocinvq_impl(c, true, avg_fused, rows_fused)) return 1; // ocqbdy fused into the unpack kernel
  if (c->poavg.on && launch_poavg(c)) return 1; // avg_ocn_k247 right after ocqbdy, src/q-gcm.F:1250-1252
  if (avg_fused) {
    KTimer t(c, KN_LFAVG);
    hipLaunchKernelGGL(k_lf_average_scalars, dim3(1), dim3(64), 0, c->stream, c->sc, c->g.nl, c->g.cyc ? 1 : 0);
    HIPCHECK(hipGetLastError());
    if (c->oml.on && launch_oml_average(c)) return 1; // the mixed-layer temperature keeps its own (one-field) pass
    if (c->aml.on && launch_aml_average(c)) return 1;
  } else if (avg) {
    if (qgcm_hip_lf_average(c)) return 1; // incl. sst when the mixed layer is on
  }
  if (c->profiling) {
    // an empty launch bracketed like the kernels (see qgcm_hip_profile_steps)
    KTimer t(c, KN_NOOP);
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, c->stream);
  }
  if (c->evkid.size() > 4000) drain_timers(c); // bounds the event pool on long profiling runs
  return 0;
}

// the buffer rotation; atmon.ast / atmon.hmixa follow the current level
static void aml_set_idx(qgcm_hip_ctx *c, int ia, int iam) {
  c->aml.ia = ia;
  c->aml.iam = iam;
  c->atmon.ast = c->aml.ast[ia];
  c->atmon.hmixa = c->aml.hm[ia];
}

// three buffers rotate with period 3 (current -> lagged -> spare -> current), one position per step
static void rotate3(int &cur, int &lag, int nsteps) {
  for (int r = 0; r < nsteps % 3; ++r) {
    const int spare = 3 - cur - lag;
    lag = cur;
    cur = spare;
  }
}
// where the mixed layer's buffers (the ocean's sst; the atmosphere's ast / hmixa) stand nsteps later
static void ml_rotate(qgcm_hip_ctx *c, int nsteps) {
  if (c->oml.on) rotate3(c->oml.is, c->oml.ism, nsteps);
  if (c->aml.on) {
    int ia = c->aml.ia, iam = c->aml.iam;
    rotate3(ia, iam, nsteps);
    aml_set_idx(c, ia, iam);
  }
}

// The rotation state a block of steps moves.  Capturing a block and the dry pass of steps_impl execute nothing: they
// put it back to that of the block's first step.
struct QgRotState {
  int ip, iq, is, ism, ia, iam;
  long pn;
  void save(const qgcm_hip_ctx *c) {
    ip = c->ip; iq = c->iq; is = c->oml.is; ism = c->oml.ism; ia = c->aml.ia; iam = c->aml.iam; pn = c->poavg.n;
  }
  void restore(qgcm_hip_ctx *c) const {
    c->ip = ip; c->iq = iq; c->oml.is = is; c->oml.ism = ism; c->poavg.n = pn;
    if (c->aml.on) aml_set_idx(c, ia, iam);
  }
};

// What `body` launches on the handle's stream, captured and instantiated as an executable graph
template <class Body>
static int capture_block(qgcm_hip_ctx *c, bool upload, hipGraphExec_t *exec, Body body) {
  QgRotState st;
  st.save(c);
  hipGraph_t graph;
  HIPCHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  hipError_t e = hipStreamEndCapture(c->stream, &graph);
  st.restore(c); // capture does not execute
  if (rc) return 1;
  HIPCHECK(e);
  HIPCHECK(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
  HIPCHECK(hipGraphDestroy(graph));
  // (the first replay of a fresh executable graph otherwise pays for its upload inside the caller's window)
  if (upload && hipGraphUpload(*exec, c->stream) != hipSuccess) (void)hipGetLastError();
  return 0;
}

// One captured block of B consecutive steps. B is even, so both buffer rotations are back where they started
// after the block; the key carries everything else a captured step depends on: the position in the averaging
// cycle and the sst rotation. 50-step blocks serve long runs (one graph for the ocean: 50 = 2 x 25); what is left
// (< 50 steps) goes out as ONE more block of the largest even length - a run of n steps is n / 50 + 1 graph
// launches and at most one eager step (round 2 cut the tail into 10-step blocks: two replays for the driver's
// 20-step window, each paying the ~10-16 us host-side floor of a replay).  The cache is bounded: a caller
// that asks for ever new block lengths / phases evicts everything once kMaxGraphs is reached.
static const size_t kMaxGraphs = 96;

// the key of a captured block of B steps from s0, in both caches (graphs, slab_graphs)
static long long graph_key(const qgcm_hip_ctx *c, int s0, int B) {
  // mixed layer on/off and its buffer rotation (an ocean handle has the ocean's, an atmosphere handle the atmosphere's)
  const int omk = c->oml.on ? 1 + 3 * c->oml.is + c->oml.ism : c->aml.on ? 1 + 3 * c->aml.ia + c->aml.iam : 0;
  // ... and which tendency kernel the block launches (tend_zmask: set_forcing changes it without dropping the graphs;
  // omk < 16, so bits 28-29 are free)
  // (bit 30: step_plan's band_rows depends on whether an atmosphere steps beside the ocean)
  return ((long long)B << 32) | ((long long)c->poavg.on << 31) | ((long long)c->beside << 30) | ((long long)tend_zmask(c) << 28) | (omk << 24) | (c->ip << 16) |
         (c->iq << 8) | avg_phase(c, s0);
}

static int get_graph(qgcm_hip_ctx *c, int s0, int B, hipGraphExec_t *out) {
  const long long key = graph_key(c, s0, B);
  auto it = c->graphs.find(key);
  if (it != c->graphs.end()) {
    it->second.used = c->graph_call;
    *out = it->second.exec;
    return 0;
  }
  if (c->graphs.size() >= kMaxGraphs) {
    // evict what the CURRENT call has not touched (a dry pass that builds the graphs of a timed call must not lose
    // them to its own later blocks); least recently used first, down to half the cache
    HIPCHECK(hipStreamSynchronize(c->stream)); // replays of the graphs about to be destroyed may still be queued
    std::vector<std::pair<unsigned long, long long>> old;
    for (auto &kv : c->graphs)
      if (kv.second.used != c->graph_call) old.push_back({kv.second.used, kv.first});
    std::sort(old.begin(), old.end());
    for (size_t i = 0; i < old.size() && c->graphs.size() > kMaxGraphs / 2; ++i) {
      hipGraphExecDestroy(c->graphs[old[i].second].exec);
      c->graphs.erase(old[i].second);
    }
  }
  if (sched_block(c, s0, B) < B) // (steps_impl cuts)
    QG_FAIL("qgcm_hip_steps: internal: a graph block would hold a dump step or an accumulation step");
  hipGraphExec_t exec;
  if (capture_block(c, true, &exec, [&]() {
        int rc = 0;
        for (int s = s0; s < s0 + B && !rc; ++s) rc = one_step(c, s);
        return rc;
      }))
    return 1;
  c->graphs[key] = {exec, c->graph_call};
  *out = exec;
  return 0;
}

// dry = true only instantiates the graphs the run will replay (so that a timed region does not pay for it)
// With a dump schedule (qgcm_hip_qocdiag_schedule) the graph blocks end before every dump step, and the dump step (and
// a single step left before one) runs eagerly: the blocks of the other steps are the graphs of a run without one.
// With an accumulation schedule (qgcm_hip_tavatm_schedule) the graph blocks end after every accumulation step, and the
// contribution is launched on the stream between two replays (never captured); a single step left before one runs
// eagerly.  The dry pass cuts in the same places.  A covariance schedule (qgcm_hip_cov_schedule) cuts the same way; its
// contribution follows a tavatm contribution of the same step (src/q-gcm.F:1477-1488).
static int steps_impl(qgcm_hip_ctx *c, int s0, int n, bool dry) {
  int s = s0;
  if (!dry) { // the ring has room and every input of the contributions is there before anything is launched
    const long d = sched_count(c->sched[SCH_DUMP], s0, n);
    if (d > c->qd.cap - c->qd.count)
      QG_FAIL("qgcm_hip_steps: steps %d..%d would record %ld dumps, the ring has room for %d (qgcm_hip_qocdiag_read)",
              s0, s0 + n - 1, d, c->qd.cap - c->qd.count);
    for (const auto &a : kAccum)
      if (sched_count(c->sched[a.sched], s0, n) > 0 && a.inputs(c, a.who)) return 1;
    c->graph_call++; // (a dry pass belongs to the call that follows it: qgcm_hip_time_steps, prepare + steps)
  }
  QgRotState st0;
  st0.save(c);
  while (n > 0) {
    const int m = sched_block(c, s, n);
    if (!c->profiling && m >= 2) {
      const int B = m >= kGraphBlock ? kGraphBlock : (m & ~1);
      hipGraphExec_t ge;
      if (get_graph(c, s, B, &ge)) return 1;
      if (!dry) HIPCHECK(hipGraphLaunch(ge, c->stream));
      if (!dry && c->poavg.on) c->poavg.n += B;
      s += B;
      n -= B;
      ml_rotate(c, B); // the p and q rotations are back where they started, the mixed layer's has moved on
      if (!dry && launch_accums(c, s - 1)) return 1; // after the block's last step
      continue;
    }
    // a dump step, an accumulation step, the single step before one, the last odd step or a profiled step: eagerly (a
    // dry pass follows the rotations it would make)
    if (!dry) {
      if (one_step(c, s) || launch_accums(c, s)) return 1; // after the step's averaging (src/q-gcm.F:1477-1489)
    } else {
      c->ip ^= 1;
      c->iq ^= 1;
      ml_rotate(c, 1);
    }
    ++s;
    --n;
  }
  if (dry) st0.restore(c);
  return 0;
}

extern "C" int qgcm_hip_steps(qgcm_hip_handle c, int s0, int n) {
  if (check_ready(c, "qgcm_hip_steps")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_steps: this handle is a y-slab; drive it with the slab building blocks");
  if (s0 < 1 || n < 0) QG_FAIL("qgcm_hip_steps: bad step range");
  return steps_impl(c, s0, n, false);
}

// ---------------------------------------------------------------------------
// atmosphere: the same kernels under the reference's names
// ---------------------------------------------------------------------------
static int check_atm(qgcm_hip_ctx *c, const char *who) {
  if (check_ready(c, who)) return 1;
  if (!c->g.atm) QG_FAIL("%s: the handle was not created with qgcm_hip_params.atmos = 1", who);
  return 0;
}

extern "C" int qgcm_hip_qgastep(qgcm_hip_handle c) {
  if (check_atm(c, "qgcm_hip_qgastep")) return 1;
  return qgcm_hip_qgostep(c);
}

extern "C" int qgcm_hip_atinvq(qgcm_hip_handle c) {
  if (check_atm(c, "qgcm_hip_atinvq")) return 1;
  return ocinvq_impl(c);
}

extern "C" int qgcm_hip_atqzbd(qgcm_hip_handle c) {
  if (check_atm(c, "qgcm_hip_atqzbd")) return 1;
  return launch_ocqbdy(c);
}

extern "C" int qgcm_hip_get_bsums(qgcm_hip_handle c, double *b) {
  if (check_ready(c, "qgcm_hip_get_bsums")) return 1;
  if (!b) QG_FAIL("qgcm_hip_get_bsums: null argument");
  if (!c->g.cyc) QG_FAIL("qgcm_hip_get_bsums: only the zonally cyclic ocean and the atmosphere have boundary line sums");
  QgScalars h;
  HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const int nl = c->g.nl;
  for (int k = 0; k < nl; ++k) {
    b[k] = h.ajisoc[k];
    b[nl + k] = h.ajinoc[k];
    b[2 * nl + k] = h.ap5soc[k];
    b[3 * nl + k] = h.ap5noc[k];
  }
  return 0;
}

// ---------------------------------------------------------------------------
// atmospheric mixed layer: src/amlsubs.F on the device, kernels in k_aml.h
// ---------------------------------------------------------------------------
// the handles the mixed layer's entry points serve: whole-domain atmosphere handles
static int aml_handle(qgcm_hip_ctx *c, const char *who) {
  if (!c) QG_FAIL("%s: null handle", who);
  if (!c->g.atm) QG_FAIL("%s: the handle is an ocean (its mixed layer is qgcm_hip_oml_*)", who);
  if (!c->whole) QG_FAIL("%s: the handle is a y-slab (the atmospheric mixed layer needs the whole domain)", who);
  return check_ready(c, who);
}

static int aml_ready(qgcm_hip_ctx *c, const char *who) {
  if (aml_handle(c, who)) return 1;
  if (!c->aml.on) QG_FAIL("%s: qgcm_hip_aml_init has not been called", who);
  return 0;
}

extern "C" int qgcm_hip_aml_init(qgcm_hip_handle c, const qgcm_hip_aml_params *p) {
  const char *who = "qgcm_hip_aml_init";
  if (aml_handle(c, who)) return 1;
  if (!p) QG_FAIL("%s: null parameters", who);
  if (!(p->hmat > 0.0) || !(p->hmamin > 0.0) || p->tat1 == p->tat2) QG_FAIL("%s: need hmat > 0, hmamin > 0 and tat(1) != tat(2)", who);
  const QgGeom &g = c->g;
  const int nxt = g.nxt, nyt = g.ny - 1;
  if (nxt < 3 || nyt < 3) QG_FAIL("%s: grid too small", who);
  auto &a = c->aml;
  auto &m = c->atmon;
  drop_graphs(c);
  if (!a.diag) { // (the last of the buffers: a call that failed half-way is made good by the next)
    if (!m.ldt) m.ldt = round_up(nxt, 16);
    a.ldt = m.ldt;
    const size_t nT = (size_t)a.ldt * nyt, nP = (size_t)g.ldx * g.ny;
    a.nblkA = ((nxt + OML_TX - 1) / OML_TX) * ((nyt + AML_SH - 1) / AML_SH);
    a.nblkB = ((g.nx + OML_TX - 1) / OML_TX) * ((g.ny + OML_TY * OML_RPT - 1) / (OML_TY * OML_RPT));
    // the mixed layer's own buffers, then the inputs that others write: fnetat (xforc's heat half or
    // qgcm_hip_set_atm_tav_fields), wekta, uekat, vekat
    struct { QgDbl *buf; size_t n; } bufs[] = {{&a.ast[0], nT}, {&a.ast[1], nT}, {&a.ast[2], nT}, {&a.hm[0], nT}, {&a.hm[1], nT},
                                               {&a.hm[2], nT}, {&a.xfa, nT}, {&a.xc1, nT}, {&a.dtop, nP},
                                               {&a.partA, (size_t)3 * a.nblkA}, {&a.partB, (size_t)3 * a.nblkB},
                                               {&c->tav.fnet, nT}, {&m.wekta, nT}, {&m.uekat, (size_t)g.ldx * nyt},
                                               {&m.vekat, (size_t)m.ldt * g.ny}, {&a.diag, 2}};
    for (auto &b : bufs)
      if (b.buf->ensure(b.n, "a buffer of the atmospheric mixed layer")) return 1;
    // what qgcm_hip_set_atm_monitor_fields was given before becomes the current level: copy, give the old owners'
    // memory back, point atmon.ast / atmon.hmixa at the rotating buffers
    if (m.ast_own) HIPCHECK(hipMemcpy(a.ast[0], m.ast_own, nT * sizeof(double), hipMemcpyDeviceToDevice));
    if (m.hmixa_own) HIPCHECK(hipMemcpy(a.hm[0], m.hmixa_own, nT * sizeof(double), hipMemcpyDeviceToDevice));
    m.ast_own.reset();
    m.hmixa_own.reset();
    aml_set_idx(c, 0, 1);
  }
  a.prm = *p;
  a.prm.xc1ast = a.prm.dtopat = nullptr; // (host pointers are not kept)
  const size_t nT = (size_t)a.ldt * nyt, nP = (size_t)g.ldx * g.ny;
  if (p->xc1ast) { if (upload2d(c, a.xc1, a.ldt, p->xc1ast, nxt, nyt)) return 1; }
  else HIPCHECK(hipMemset(a.xc1, 0, nT * sizeof(double)));
  if (p->dtopat) { if (upload2d(c, a.dtop, g.ldx, p->dtopat, g.nx, g.ny)) return 1; }
  else HIPCHECK(hipMemset(a.dtop, 0, nP * sizeof(double)));
  HIPCHECK(hipDeviceSynchronize());
  a.on = true;
  c->entoc_zero = false; // the mixed layer writes entat (the handle's entoc buffer) every step from now on
  return 0;
}

extern "C" int qgcm_hip_aml_set_state(qgcm_hip_handle c, const double *ast, const double *astm, const double *hmixa,
                                      const double *hmixam) {
  if (aml_ready(c, "qgcm_hip_aml_set_state")) return 1;
  const auto &a = c->aml;
  const int nxt = c->g.nxt, nyt = c->g.ny - 1;
  if (ast && upload2d(c, a.ast[a.ia], a.ldt, ast, nxt, nyt)) return 1;
  if (astm && upload2d(c, a.ast[a.iam], a.ldt, astm, nxt, nyt)) return 1;
  if (hmixa && upload2d(c, a.hm[a.ia], a.ldt, hmixa, nxt, nyt)) return 1;
  if (hmixam && upload2d(c, a.hm[a.iam], a.ldt, hmixam, nxt, nyt)) return 1;
  return 0;
}

extern "C" int qgcm_hip_aml_get_state(qgcm_hip_handle c, double *ast, double *astm, double *hmixa, double *hmixam) {
  if (aml_ready(c, "qgcm_hip_aml_get_state")) return 1;
  const auto &a = c->aml;
  const int nxt = c->g.nxt, nyt = c->g.ny - 1;
  if (ast && download2d(c, ast, a.ast[a.ia], a.ldt, nxt, nyt)) return 1;
  if (astm && download2d(c, astm, a.ast[a.iam], a.ldt, nxt, nyt)) return 1;
  if (hmixa && download2d(c, hmixa, a.hm[a.ia], a.ldt, nxt, nyt)) return 1;
  if (hmixam && download2d(c, hmixam, a.hm[a.iam], a.ldt, nxt, nyt)) return 1;
  return 0;
}

static void fill_aml_params(qgcm_hip_ctx *c, QgAmlParams &P) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  const auto &a = c->aml;
  const qgcm_hip_aml_params &q = a.prm;
  memset(&P, 0, sizeof(P));
  P.nxt = g.nxt; P.nyt = g.ny - 1; P.nx = g.nx; P.ny = g.ny; P.nl = g.nl;
  P.ldt = a.ldt; P.ldx = g.ldx; P.fstride = g.fstride;
  const int spare = 3 - a.ia - a.iam;
  P.ast = a.ast[a.ia]; P.astm = a.ast[a.iam]; P.astn = a.ast[spare];
  P.hm = a.hm[a.ia]; P.hmm = a.hm[a.iam]; P.hmn = a.hm[spare];
  P.fnet = c->tav.fnet; P.wekta = c->atmon.wekta; P.xc1 = a.xc1; P.uekat = c->atmon.uekat; P.vekat = c->atmon.vekat;
  P.pa = c->p[c->ip]; P.pam = c->p[c->ip ^ 1]; P.dtop = a.dtop;
  P.xfa = a.xfa; P.entat = c->entoc;
  P.partA = a.partA; P.partB = a.partB; P.nblkA = a.nblkA; P.nblkB = a.nblkB;
  // MODULE atconst as src/q-gcm.F:392-441 derives it, then the scalar prologues of aml (src/amlsubs.F:78-90) and amladf (:277-279)
  const double dxa = pr.dxo, dxam2 = 1.0 / (dxa * dxa);
  P.rdxaf0 = 1.0 / (dxa * pr.fnot);
  P.hdxam1 = 0.5 / dxa;
  P.d2tfac = q.at2d * dxam2;
  P.d4tfac = q.at4d * (dxam2 * dxam2);
  P.hmdfac = q.ahmd * dxam2;
  P.hmat = q.hmat; P.hmamin = q.hmamin;
  P.hmainv = 1.0 / q.hmat;
  P.hdrcdt = q.hmadmp * q.rrcpat * pr.tdto;
  P.diabcr = q.tat1 - 2.0 * P.hdrcdt;
  P.entfac = 1.0 / (pr.tdto * (q.tat2 - q.tat1));
  P.xbfac = q.xcexp * q.bface;
  for (int l = 0; l < g.nl - 1; ++l) P.afacdp[l] = q.aface[l] / pr.gpoc[l];
  P.dface = q.dface; P.cface = q.cface; P.xcexp = q.xcexp; P.tat1 = q.tat1; P.tdta = pr.tdto; P.rrcpat = q.rrcpat;
}

// with_final = false: the final reduction rides in workgroup 0 of the tendency launch that follows (one_step)
static int launch_aml(qgcm_hip_ctx *c, bool with_final) {
  QgAmlParams P;
  fill_aml_params(c, P);
  dim3 gA((P.nxt + OML_TX - 1) / OML_TX, (P.nyt + AML_SH - 1) / AML_SH);
  dim3 gB((P.nx + OML_TX - 1) / OML_TX, (P.ny + OML_TY * OML_RPT - 1) / (OML_TY * OML_RPT));
  {
    KTimer t(c, KN_AML);
    hipLaunchKernelGGL(k_aml_step, gA, dim3(OML_NT), 0, c->stream, P);
  }
  {
    KTimer t(c, KN_AML_ENTAT);
    c->entoc_zero = false; // (k_aml_entat writes entat, the handle's entoc buffer)
    hipLaunchKernelGGL(k_aml_entat, gB, dim3(OML_NT), 0, c->stream, P);
  }
  if (with_final) {
    QgOmlFinal F;
    fill_oml_final(c, F, true);
    hipLaunchKernelGGL(k_oml_final, dim3(1), dim3(OML_NT), 0, c->stream, F);
  }
  HIPCHECK(hipGetLastError());
  // rotation: astm <- ast, ast <- new; likewise hmixa (src/amlsubs.F:161-164)
  aml_set_idx(c, 3 - c->aml.ia - c->aml.iam, c->aml.ia);
  return 0;
}

extern "C" int qgcm_hip_aml(qgcm_hip_handle c) {
  if (aml_ready(c, "qgcm_hip_aml")) return 1;
  return launch_aml(c, true);
}

static int launch_aml_average(qgcm_hip_ctx *c) {
  const auto &a = c->aml;
  const long n = (long)a.ldt * (c->g.ny - 1);
  hipLaunchKernelGGL(k_aml_average, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a.ast[a.ia],
                     (const double *)a.ast[a.iam], a.hm[a.ia], (const double *)a.hm[a.iam], n);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_aml_get_diag(qgcm_hip_handle c, double *entat, double *diag) {
  if (aml_ready(c, "qgcm_hip_aml_get_diag")) return 1;
  const QgGeom &g = c->g;
  if (entat && download2d(c, entat, c->entoc, g.ldx, g.nx, g.ny)) return 1;
  if (diag) {
    QgScalars h;
    double d[2];
    HIPCHECK(hipMemcpyAsync(&h, c->sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(d, c->aml.diag, sizeof(d), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    const int ni = g.nl - 1; // interfaces: the vectors whole, so that a host can see that only their first entries move
    for (int k = 0; k < ni; ++k) {
      diag[k] = h.xon[k];
      diag[ni + k] = h.enisoc[k];
      diag[2 * ni + k] = h.eninoc[k];
    }
    diag[3 * ni] = d[0];
    diag[3 * ni + 1] = d[1];
  }
  return 0;
}

// ---------------------------------------------------------------------------
// momentum half of xforc: src/xfosubs.F:137-709 on the device, kernels in k_xforc.h
// ---------------------------------------------------------------------------
// xforc is off until qgcm_hip_xforc_init has gone through (it replaces the buffers)
static void xf_off(qgcm_hip_ctx *a) {
  auto &x = a->xf;
  x.on = x.coupled = x.slab = x.bands.on = x.udiff.on = x.udiff.fresh = x.sums.on = x.sums.fresh = false;
  x.oc = nullptr;
  x.heat.on = false; // (set up against the geometry qgcm_hip_xforc_init was given: qgcm_hip_xforc_heat_init again)
  x.sst.on = false;  // (likewise qgcm_hip_xforc_sst_init)
}

// k_xf_wekpa_stage and its launch live in k_xf_wekpa_stage.hip, a device code object of its own as k_tend_rows.hip
hipError_t qg_setup_xf_wekpa_stage(int ndxr);
hipError_t qg_launch_xf_wekpa_stage(hipStream_t st, const QgXfParams &P, int ja0, int nrow);

// slab: the set-up of qgcm_hip_xforc_slab_init - the ocean handle holds rows of a basin of g.nyg rows
static int xf_init(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const qgcm_hip_xforc_params *p, const char *who, bool slab) {
  if (!atm || !p) QG_FAIL("%s: null atmosphere handle or parameters", who);
  if (slab && !oc) QG_FAIL("%s: null ocean handle", who);
  if (check_atm(atm, who)) return 1;
  if (!atm->whole) QG_FAIL("%s: the atmosphere handle is a y-slab (xforc needs the whole domain)", who);
  if (oc) {
    if (oc->g.atm) QG_FAIL("%s: the first handle is an atmosphere (pass the ocean, or NULL for atmos_only)", who);
    if (!slab && !oc->whole) QG_FAIL("%s: the ocean handle is a y-slab (xforc needs the whole domain)", who);
    if (check_ready(oc, who)) return 1;
    if (oc->device != atm->device) QG_FAIL("%s: the two handles live on different devices (%d, %d)", who, oc->device, atm->device);
  }
  if (p->tau_udiff && !oc) QG_FAIL("%s: tau_udiff needs an ocean (the reference ignores it when atmos_only)", who);
  if (p->tau_udiff && slab)
    QG_FAIL("%s: tau_udiff is not available with a y-slab ocean (the fine stress above the sea would need every slab's pom on every rank)", who);
  if (!p->stbbb || !p->stbus || !p->stbvs || !p->stbun || !p->stbvn) QG_FAIL("%s: a weight table is NULL", who);
  const int ndxr = p->ndxr, nxta = atm->g.nxt, nyta = atm->g.ny - 1;
  if (ndxr < 1 || ndxr > 128) QG_FAIL("%s: ndxr = %d outside 1..128", who, ndxr);
  if (nxta < 4 || nyta < 2) QG_FAIL("%s: atmosphere of %d x %d cells is too small", who, nxta, nyta);
  if ((double)nxta * ndxr >= 1.0e6 || (long)nyta * ndxr >= 65535)
    QG_FAIL("%s: the fine grid %d*%d x %d*%d exceeds the kernels' launch limits", who, nxta, ndxr, nyta, ndxr);
  // (the kernels index the fine arrays with int products of a row and a pitch where the row is not cast: DESIGN 6s)
  if ((double)round_up(nxta * ndxr + 1, 16) * (double)(nyta * ndxr + 1) > 2147483647.0)
    QG_FAIL("%s: the fine grid's padded arrays of %d x %d elements pass 2^31 - 1 elements", who, round_up(nxta * ndxr + 1, 16),
            nyta * ndxr + 1);
  if (!(p->hmat > 0.0) || !(p->cdat > 0.0)) QG_FAIL("%s: need hmat > 0 and cdat > 0", who);
  if (oc) {
    const int nxto = oc->g.nxt, nyto = (slab ? oc->g.nyg : oc->g.ny) - 1;
    if (!(p->hmoc > 0.0)) QG_FAIL("%s: need hmoc > 0", who);
    if (p->nxaooc < 1 || p->nyaooc < 1 || nxto != p->nxaooc * ndxr || nyto != p->nyaooc * ndxr)
      QG_FAIL("%s: mismatched geometry: the ocean has %d x %d T cells, nxaooc*ndxr x nyaooc*ndxr = %d*%d x %d*%d", who, nxto,
              nyto, p->nxaooc, ndxr, p->nyaooc, ndxr);
    if (p->nx1 < 1 || p->ny1 < 1 || p->nx1 + p->nxaooc - 1 > nxta || p->ny1 + p->nyaooc - 1 > nyta)
      QG_FAIL("%s: the ocean (nx1 = %d, ny1 = %d, nxaooc = %d, nyaooc = %d) does not lie inside the atmosphere's %d x %d cells",
              who, p->nx1, p->ny1, p->nxaooc, p->nyaooc, nxta, nyta);
    if (oc->g.cyc && (p->nxaooc != nxta || p->nx1 != 1))
      QG_FAIL("%s: a zonally cyclic ocean needs nxaooc = nxta (%d, %d) and nx1 = 1", who, p->nxaooc, nxta);
    if (oc->prm.fnot != atm->prm.fnot) QG_FAIL("%s: the handles differ in fnot", who);
  }
  auto &x = atm->xf;
  HIPCHECK(hipStreamSynchronize(atm->stream));
  xf_off(atm);
  x.prm = *p;
  x.prm.stbbb = x.prm.stbus = x.prm.stbvs = x.prm.stbun = x.prm.stbvn = nullptr; // (host pointers are not kept)
  const QgGeom &g = atm->g;
  const int nxpaor = nxta * ndxr + 1, nypaor = nyta * ndxr + 1;
  x.ldf = round_up(nxpaor, 16);
  x.ldtf = round_up(nxpaor - 1, 16);
  const size_t nfine = (size_t)x.ldf * nypaor, npl = (size_t)(ndxr + 1) * ndxr;
  if (x.u1at.alloc((size_t)g.ldx * g.ny, "xforc's u1at") || x.v1at.alloc((size_t)g.ldx * g.ny, "xforc's v1at") ||
      x.txf.alloc(nfine, "xforc's fine stress") || x.tyf.alloc(nfine, "xforc's fine stress") ||
      x.wf.alloc((size_t)x.ldtf * (nypaor - 1), "xforc's fine Ekman velocity") || x.tab.alloc(5 * 16 * npl, "xforc's weight tables"))
    return 1;
  {
    // MODULE xfosubs holds stb**(16, 0:ndxr, 0:ndxr); the kernels read tab[k][jj][ii], ii = 0..ndxr-1 (k_xforc.h)
    std::vector<double> t(5 * 16 * npl);
    const double *src[5] = {p->stbbb, p->stbus, p->stbvs, p->stbun, p->stbvn};
    for (int m = 0; m < 5; ++m)
      for (int k = 0; k < 16; ++k)
        for (int jj = 0; jj <= ndxr; ++jj)
          for (int ii = 0; ii < ndxr; ++ii)
            t[((size_t)m * 16 + k) * npl + (size_t)jj * ndxr + ii] = src[m][k + 16 * ((size_t)ii + (size_t)(ndxr + 1) * jj)];
    HIPCHECK(hipMemcpy(x.tab, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  // the destinations beside wekpa / wekpo: the atmosphere's monitor fields and the ocean's (zero until the first call)
  auto &m = atm->atmon;
  if (!m.ldt) m.ldt = round_up(nxta, 16);
  struct { QgDbl *buf; size_t n; } dst[] = {{&m.wekta, (size_t)m.ldt * nyta}, {&m.tauxa, (size_t)g.ldx * g.ny},
                                            {&m.tauya, (size_t)g.ldx * g.ny}, {&m.uekat, (size_t)g.ldx * nyta},
                                            {&m.vekat, (size_t)m.ldt * g.ny}};
  for (auto &d : dst)
    if (d.buf->ensure(d.n, "an atmosphere monitor field")) return 1;
  if (oc) {
    auto &mo = oc->mon;
    const QgGeom &go = oc->g;
    if (!mo.ldt) mo.ldt = round_up(go.nxt, 16);
    if (mo.taux.ensure((size_t)go.ldx * go.ny, "an ocean monitor field") ||
        mo.tauy.ensure((size_t)go.ldx * go.ny, "an ocean monitor field") ||
        mo.wekto.ensure((size_t)mo.ldt * (go.ny - 1), "an ocean monitor field"))
      return 1;
  }
  {
    // the form of the box average: k_xf_wekpa up to ndxr = 64, k_xf_wekpa_stage above; QGCM_HIP_XF_WEKPA_STAGE
    // = 0 / 1 forces the plain / the staged form at any ndxr
    const char *e = getenv("QGCM_HIP_XF_WEKPA_STAGE");
    x.wekpa_stage = e && *e ? atoi(e) != 0 : ndxr > XF_WEKPA_STAGE_ABOVE;
    if (x.wekpa_stage) HIPCHECK(qg_setup_xf_wekpa_stage(ndxr));
  }
  if (!x.ev_oc) HIPCHECK(hipEventCreateWithFlags(&x.ev_oc, hipEventDisableTiming));
  if (!x.ev_atm) HIPCHECK(hipEventCreateWithFlags(&x.ev_atm, hipEventDisableTiming));
  x.oc = oc;
  x.slab = slab;
  x.on = true;
  return 0;
}

extern "C" int qgcm_hip_xforc_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_params *p) {
  return xf_init(oc, atm, p, "qgcm_hip_xforc_init", false);
}

// slab: one of the qgcm_hip_xforc_slab_* calls (their set-up and the whole-domain one exclude each other)
static int xf_ready(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const char *who, bool slab = false) {
  if (!atm) QG_FAIL("%s: null atmosphere handle", who);
  if (check_atm(atm, who)) return 1;
  if (slab) {
    if (!atm->xf.on || !atm->xf.slab) QG_FAIL("%s: qgcm_hip_xforc_slab_init has not been called for this atmosphere", who);
    if (!oc || atm->xf.oc != oc) QG_FAIL("%s: the ocean handle is not the one qgcm_hip_xforc_slab_init was called with", who);
    return 0;
  }
  if (!atm->xf.on) QG_FAIL("%s: qgcm_hip_xforc_init has not been called for this atmosphere", who);
  if (atm->xf.slab) QG_FAIL("%s: this atmosphere's xforc was set up for a y-slab ocean (qgcm_hip_xforc_slab_init): use the qgcm_hip_xforc_slab_ calls", who);
  if (atm->xf.oc != oc) QG_FAIL("%s: the ocean handle is not the one qgcm_hip_xforc_init was called with", who);
  return 0;
}

static void xf_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, QgXfParams &P) {
  const auto &x = atm->xf;
  const qgcm_hip_xforc_params &p = x.prm;
  const QgGeom &g = atm->g;
  memset(&P, 0, sizeof(P));
  const int ndxr = p.ndxr;
  P.ndxr = ndxr; P.nxta = g.nxt; P.nyta = g.ny - 1; P.nxpa = g.nx; P.nypa = g.ny;
  P.nxtaor = P.nxta * ndxr; P.nytaor = P.nyta * ndxr; P.nxpaor = P.nxtaor + 1; P.nypaor = P.nytaor + 1;
  P.ndxodd = ndxr % 2; P.nijwid = ndxr + ndxr % 2;
  P.lda = g.ldx; P.ldta = atm->atmon.ldt; P.ldf = x.ldf; P.ldtf = x.ldtf;
  P.pam = atm->p[atm->ip ^ 1];
  P.u1at = x.u1at; P.v1at = x.v1at; P.txf = x.txf; P.tyf = x.tyf; P.wf = x.wf;
  const size_t tn = (size_t)16 * (ndxr + 1) * ndxr;
  P.tbb = x.tab; P.tus = x.tab + tn; P.tvs = x.tab + 2 * tn; P.tun = x.tab + 3 * tn; P.tvn = x.tab + 4 * tn;
  const auto &m = atm->atmon;
  P.tauxa = m.tauxa; P.tauya = m.tauya; P.uekat = m.uekat; P.vekat = m.vekat; P.wekta = m.wekta; P.wekpa = atm->wekpo;
  P.sca = atm->sc;
  // constants as src/xfosubs.F:137-155, 185, 249 with dxa = ndxr*dxo, rdxaf0, rdxof0 of src/q-gcm.F:380, 435-436
  const double fnot = atm->prm.fnot, dxa = atm->prm.dxo, dxo = oc ? oc->prm.dxo : dxa / (double)ndxr;
  const double rdxaf0 = 1.0 / (dxa * fnot), rdxof0 = 1.0 / (dxo * fnot);
  P.dxo = dxo;
  P.hxafac = 0.5 * rdxaf0; P.hxofac = 0.5 * rdxof0;
  P.zbfcat = rdxaf0 / (0.5 * p.bccoat + 1.0);
  P.zbfcoc = rdxof0 / (0.5 * p.bccooc + 1.0);
  P.uvekfc = 1.0 / (p.hmat * fnot * (double)ndxr);
  P.hmrdxa = p.hmat / dxa;
  const double cdhfaa = (p.cdat / fnot) / p.hmat;
  P.cdrfaa = p.cdat / fabs(cdhfaa);
  P.qu2faa = 4.0 * cdhfaa * cdhfaa;
  P.raoro = p.raoro;
  P.udiff = p.tau_udiff ? 1 : 0;
  if (oc) {
    const double cdhfab = (p.cdat / fnot) * (1.0 / p.hmat + p.raoro / p.hmoc);
    P.cdrfab = p.cdat / fabs(cdhfab);
    P.qu2fab = 4.0 * cdhfab * cdhfab;
    P.nxpo = oc->g.nx; P.nypo = oc->g.ny; P.ldo = oc->g.ldx; P.cyc_oc = oc->g.cyc;
    P.iocoff = (p.nx1 - 1) * ndxr; P.jocoff = (p.ny1 - 1) * ndxr;
    P.pom = oc->p[oc->ip ^ 1];
    P.tauxo = oc->mon.taux; P.tauyo = oc->mon.tauy;
    P.sco = oc->g.cyc ? oc->sc : nullptr;
  }
}

static int launch_xf_heat(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm);
static int launch_xf_heat_sst(qgcm_hip_ctx *atm);
// k_xf_heat_sst and its launch live in k_xf_heat_sst.hip, a device code object of its own (as k_tend_rows.hip): this file
// compiles to the device code it had without the kernel.
hipError_t qg_launch_xf_heat_sst(hipStream_t st, const QgXfHeatParams &P);

// the atmosphere side of the momentum half up to wekpa: the fine stress and every product that depends on pam only
// (stage: wekpa by k_xf_wekpa_stage)
static hipError_t launch_xf_atmos(const QgXfParams &P, hipStream_t st, bool stage) {
  const dim3 b(XF_NT);
  hipLaunchKernelGGL(k_xf_coarse, dim3((P.nxpa + XF_NT - 1) / XF_NT, P.nypa), b, 0, st, P);
  hipLaunchKernelGGL(k_xf_fine, dim3((P.nxta + XF_CX - 1) / XF_CX, P.nyta), b, 0, st, P);
  hipLaunchKernelGGL(k_xf_atm, dim3((P.nxpa + XF_NT - 1) / XF_NT, P.nypa), b, 0, st, P);
  hipLaunchKernelGGL(k_xf_wekta, dim3((P.nxta + XF_NT - 1) / XF_NT, P.nyta), b, 0, st, P);
  hipLaunchKernelGGL(k_xf_wektaor, dim3((P.nxtaor + XF_NT - 1) / XF_NT, P.nytaor), b, 0, st, P);
  if (stage) return qg_launch_xf_wekpa_stage(st, P, 1, P.nypa);
  hipLaunchKernelGGL(k_xf_wekpa, dim3((P.nxpa + 63) / 64, P.nypa), dim3(64), 0, st, P);
  return hipGetLastError();
}

// One `call xforc` on the atmosphere's stream, ordered against the ocean's stream by two events: the momentum half and,
// once qgcm_hip_xforc_heat_init (without an ocean: qgcm_hip_xforc_sst_init) has set it up, the heat half.
extern "C" int qgcm_hip_xforc(qgcm_hip_handle oc, qgcm_hip_handle atm) {
  if (xf_ready(oc, atm, "qgcm_hip_xforc")) return 1;
  auto &x = atm->xf;
  hipStream_t st = atm->stream;
  QgXfParams P;
  xf_fill(oc, atm, P);
  if (oc) { // pom and the ocean's forcing buffers: after everything queued on the ocean's stream
    HIPCHECK(hipEventRecord(x.ev_oc, oc->stream));
    HIPCHECK(hipStreamWaitEvent(st, x.ev_oc, 0));
  }
  const dim3 b(XF_NT);
  HIPCHECK(launch_xf_atmos(P, st, x.wekpa_stage));
  if (oc) {
    const QgGeom &go = oc->g;
    auto &mo = oc->mon;
    hipLaunchKernelGGL(k_xf_tauo, dim3((P.nxpo + XF_NT - 1) / XF_NT, P.nypo), b, 0, st, P);
    QgWekParams W;
    memset(&W, 0, sizeof(W));
    W.g = go; W.taux = mo.taux; W.tauy = mo.tauy; W.wekto = mo.wekto; W.wekpo = oc->wekpo; W.ldt = mo.ldt;
    W.hxofac = P.hxofac;
    hipLaunchKernelGGL(k_wekto, dim3((go.nxt + 255) / 256, go.ny - 1), dim3(256), 0, st, W);
    hipLaunchKernelGGL(k_wekpo, dim3((go.nx + 255) / 256, go.ny), dim3(256), 0, st, W);
    if (oc->oml.on) { // the mixed layer's own forcing buffers (same pitches)
      auto &o = oc->oml;
      const size_t nP = (size_t)go.ldx * go.ny * sizeof(double), nT = (size_t)o.ldt * (go.ny - 1) * sizeof(double);
      HIPCHECK(hipMemcpyAsync(o.taux, mo.taux, nP, hipMemcpyDeviceToDevice, st));
      HIPCHECK(hipMemcpyAsync(o.tauy, mo.tauy, nP, hipMemcpyDeviceToDevice, st));
      HIPCHECK(hipMemcpyAsync(o.wekto, mo.wekto, nT, hipMemcpyDeviceToDevice, st));
    }
  }
  hipLaunchKernelGGL(k_xf_lines, dim3(1), b, 0, st, P);
  HIPCHECK(hipGetLastError());
  if (x.heat.on && launch_xf_heat(oc, atm)) return 1; // the heat half, src/xfosubs.F:711-853
  if (x.sst.on && launch_xf_heat_sst(atm)) return 1;  // ... as -Datmos_only builds it, from the prescribed SST
  if (oc) { // the ocean's next step reads wekpo, the stress and the line integrals
    HIPCHECK(hipEventRecord(x.ev_atm, st));
    HIPCHECK(hipStreamWaitEvent(oc->stream, x.ev_atm, 0));
  }
  return 0;
}

// (an ocean's fields come with the rows its handle holds: a y-slab's local rows for qgcm_hip_xforc_slab_get)
static int xf_get(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, double *tauxa, double *tauya, double *uekat, double *vekat, double *wekta,
                  double *wekpa, double *tauxo, double *tauyo, double *wekto, double *wekpo, double *txi) {
  const QgGeom &g = atm->g;
  const auto &m = atm->atmon;
  const int nxt = g.nxt, nyt = g.ny - 1;
  if (tauxa && download2d(atm, tauxa, m.tauxa, g.ldx, g.nx, g.ny)) return 1;
  if (tauya && download2d(atm, tauya, m.tauya, g.ldx, g.nx, g.ny)) return 1;
  if (uekat && download2d(atm, uekat, m.uekat, g.ldx, g.nx, nyt)) return 1;
  if (vekat && download2d(atm, vekat, m.vekat, m.ldt, nxt, g.ny)) return 1;
  if (wekta && download2d(atm, wekta, m.wekta, m.ldt, nxt, nyt)) return 1;
  if (wekpa && download2d(atm, wekpa, atm->wekpo, g.ldx, g.nx, g.ny)) return 1;
  if ((tauxo || tauyo || wekto || wekpo) && !oc) QG_FAIL("qgcm_hip_xforc_get: an ocean field was asked for without an ocean");
  if (oc) {
    const QgGeom &go = oc->g;
    const auto &mo = oc->mon;
    HIPCHECK(hipStreamSynchronize(atm->stream)); // (xforc ran on the atmosphere's stream)
    if (tauxo && download2d(oc, tauxo, mo.taux, go.ldx, go.nx, go.ny)) return 1;
    if (tauyo && download2d(oc, tauyo, mo.tauy, go.ldx, go.nx, go.ny)) return 1;
    if (wekto && download2d(oc, wekto, mo.wekto, mo.ldt, go.nxt, go.ny - 1)) return 1;
    if (wekpo && download2d(oc, wekpo, oc->wekpo, go.ldx, go.nx, go.ny)) return 1;
  }
  if (txi) {
    QgScalars h;
    HIPCHECK(hipMemcpyAsync(&h, atm->sc, sizeof(h), hipMemcpyDeviceToHost, atm->stream));
    HIPCHECK(hipStreamSynchronize(atm->stream));
    txi[0] = h.txisoc;
    txi[1] = h.txinoc;
    txi[2] = txi[3] = 0.0;
    if (oc && oc->g.cyc) {
      HIPCHECK(hipMemcpyAsync(&h, oc->sc, sizeof(h), hipMemcpyDeviceToHost, atm->stream));
      HIPCHECK(hipStreamSynchronize(atm->stream));
      txi[2] = h.txisoc;
      txi[3] = h.txinoc;
    }
  }
  return 0;
}

extern "C" int qgcm_hip_xforc_get(qgcm_hip_handle oc, qgcm_hip_handle atm, double *tauxa, double *tauya, double *uekat,
                                  double *vekat, double *wekta, double *wekpa, double *tauxo, double *tauyo, double *wekto,
                                  double *wekpo, double *txi) {
  if (xf_ready(oc, atm, "qgcm_hip_xforc_get")) return 1;
  return xf_get(oc, atm, tauxa, tauya, uekat, vekat, wekta, wekpa, tauxo, tauyo, wekto, wekpo, txi);
}

// ---------------------------------------------------------------------------
// heat half of xforc: src/xfosubs.F:711-853 on the device, kernels in k_xforc.h
// ---------------------------------------------------------------------------
// bilint's index and weight tables, as the reference computes them (src/xfosubs.F:916-980): ix = iam, iap (2, nxto),
// iy = jam, jap (2, nyto), 1-based; wx = wmx, wpx; wy = wmy, wpy.  Host side only; refuses a coordinate that xta / yta
// does not cover.
static int xf_bilint_tables(const char *who, int nxta, int nyta, int nxto, int nyto, double dxa, double dya, const double *xta,
                            const double *yta, const double *xto, const double *yto, std::vector<int> &ix, std::vector<int> &iy,
                            std::vector<double> &wx, std::vector<double> &wy) {
  const double dxainv = 1.0 / dxa, dyainv = 1.0 / dya;
  ix.assign(2 * (size_t)nxto, 0);
  iy.assign(2 * (size_t)nyto, 0);
  wx.assign(2 * (size_t)nxto, 0.0);
  wy.assign(2 * (size_t)nyto, 0.0);
  for (int io = 0; io < nxto; ++io) {
    int iam = (int)(1.0 + dxainv * (xto[io] - xta[0]));
    int iap = iam + 1;
    if (iam > nxta) QG_FAIL("%s: the atmosphere's xta does not cover ocean column %d", who, io + 1);
    const double xam = iam >= 1 ? xta[iam - 1] : xta[0] - dxa;
    wx[nxto + io] = dxainv * (xto[io] - xam);
    wx[io] = 1.0 - wx[nxto + io];
    iam = 1 + (iam + nxta - 1) % nxta; // (both pointers mended for the cyclic T grid)
    iap = 1 + (iap + nxta - 1) % nxta;
    if (iam < 1 || iap < 1) QG_FAIL("%s: the atmosphere's xta does not cover ocean column %d", who, io + 1);
    ix[io] = iam;
    ix[nxto + io] = iap;
  }
  for (int jo = 0; jo < nyto; ++jo) {
    int jam = (int)(1.0 + dyainv * (yto[jo] - yta[0]));
    int jap = jam + 1;
    jam = std::max(jam, 1);
    jap = std::min(jap, nyta);
    if (jam > nyta || jap < 1) QG_FAIL("%s: the atmosphere's yta does not cover ocean row %d", who, jo + 1);
    wy[nyto + jo] = dyainv * (yto[jo] - yta[jam - 1]);
    wy[jo] = 1.0 - wy[nyto + jo];
    iy[jo] = jam;
    iy[nyto + jo] = jap;
  }
  return 0;
}

// slab: the set-up of qgcm_hip_xforc_heat_slab_init - the tables cover the whole basin's T rows (g.nyg - 1), which the
// kernels of k_xforc_slab.h index by global row
static int xf_heat_init(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const qgcm_hip_xforc_heat_params *p, const char *who, bool slab) {
  if (!atm || !p) QG_FAIL("%s: null atmosphere handle or parameters", who);
  if (!oc) QG_FAIL("%s: the heat half needs an ocean (oc = NULL)", who);
  if (!atm->g.atm) QG_FAIL("%s: the second handle is an ocean (pass the atmosphere)", who);
  if (oc->g.atm) QG_FAIL("%s: the first handle is an atmosphere (pass the ocean)", who);
  if (!atm->whole || (!slab && !oc->whole)) QG_FAIL("%s: the %s handle is a y-slab (xforc needs the whole domain)", who, atm->whole ? "ocean" : "atmosphere");
  if (xf_ready(oc, atm, who, slab)) return 1;
  if (!atm->aml.on) QG_FAIL("%s: qgcm_hip_aml_init has not been called for this atmosphere", who);
  if (!oc->oml.on) QG_FAIL("%s: qgcm_hip_oml_init has not been called for this ocean", who);
  if (!p->fsa || !p->fso || !p->xta || !p->yta || !p->xto || !p->yto) QG_FAIL("%s: a table or a coordinate array is NULL", who);
  const qgcm_hip_xforc_params &x = atm->xf.prm;
  const int nxta = atm->g.nxt, nyta = atm->g.ny - 1, nxto = oc->g.nxt, nyto = (slab ? oc->g.nyg : oc->g.ny) - 1;
  std::vector<int> ix, iy;
  std::vector<double> wx, wy;
  if (xf_bilint_tables(who, nxta, nyta, nxto, nyto, atm->prm.dxo, atm->prm.dyo, p->xta, p->yta, p->xto, p->yto, ix, iy, wx, wy))
    return 1;
  HIPCHECK(hipStreamSynchronize(atm->stream));
  auto &h = atm->xf.heat;
  h.on = false; // (until this call has gone through: it replaces the buffers)
  const int ncell = x.nxaooc * x.nyaooc;
  h.nblkL = ((nxta + 63) / 64) * ((nyta + 3) / 4);
  if (h.fsa.alloc(nyta, "fsprim of the atmosphere") || h.fso.alloc(nyto, "fsprim of the ocean") ||
      h.wx.alloc(2 * (size_t)nxto, "bilint's x weights") || h.wy.alloc(2 * (size_t)nyto, "bilint's y weights") ||
      h.cell.alloc(ncell, "the per-cell sums") || h.part.alloc(3 * (size_t)ncell + h.nblkL, "the heat half's partial sums") ||
      h.scal.alloc(4, "the heat half's results") || h.ix.alloc(2 * (size_t)nxto, "bilint's x indices") ||
      h.iy.alloc(2 * (size_t)nyto, "bilint's y indices"))
    return 1;
  HIPCHECK(hipMemcpy(h.fsa, p->fsa, nyta * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.fso, p->fso, nyto * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.wx, wx.data(), wx.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.wy, wy.data(), wy.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.ix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.iy, iy.data(), iy.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipDeviceSynchronize());
  h.prm = *p;
  h.prm.fsa = h.prm.fso = h.prm.xta = h.prm.yta = h.prm.xto = h.prm.yto = nullptr; // (host pointers are not kept)
  h.on = true;
  return 0;
}

extern "C" int qgcm_hip_xforc_heat_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_heat_params *p) {
  return xf_heat_init(oc, atm, p, "qgcm_hip_xforc_heat_init", false);
}

// oc = nullptr: the set-up of qgcm_hip_xforc_sst_init - the SST grid is the atmosphere handle's own buffer, there is no
// fnetoc and no fso (k_xf_heat_sst reads neither)
static void xf_heat_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, QgXfHeatParams &P) {
  const auto &h = atm->xf.heat;
  const auto &ss = atm->xf.sst;
  const qgcm_hip_xforc_heat_params &q = h.prm;
  const qgcm_hip_xforc_params &x = atm->xf.prm;
  const auto &a = atm->aml;
  memset(&P, 0, sizeof(P));
  P.nxta = atm->g.nxt; P.nyta = atm->g.ny - 1;
  P.nxto = oc ? oc->g.nxt : x.nxaooc * x.ndxr; P.nyto = oc ? oc->g.nyg - 1 : x.nyaooc * x.ndxr; // (a y-slab: the basin's rows)
  P.ndxr = x.ndxr; P.nx1 = x.nx1; P.ny1 = x.ny1; P.nxaooc = x.nxaooc; P.nyaooc = x.nyaooc;
  P.ldta = a.ldt; P.lda = atm->g.ldx; P.ldto = oc ? oc->oml.ldt : ss.ldt; P.fstride = atm->g.fstride;
  P.astm = a.ast[a.iam]; P.hmm = a.hm[a.iam]; P.pam = atm->p[atm->ip ^ 1]; P.dtop = a.dtop;
  P.sstm = oc ? (const double *)oc->oml.sst[oc->oml.ism] : (const double *)ss.sst;
  P.fsa = h.fsa; P.fso = oc ? (const double *)h.fso : nullptr; P.ix = h.ix; P.iy = h.iy; P.wx = h.wx; P.wy = h.wy;
  P.fnetoc = oc ? (double *)oc->oml.fnet : nullptr; P.fnetat = atm->tav.fnet;
  P.cell = h.cell; P.part = h.part; P.scal = h.scal;
  P.ncell = x.nxaooc * x.nyaooc; P.nblkL = h.nblkL; P.natlan = P.nxta * P.nyta - P.ncell;
  // the scalar prologue, src/xfosubs.F:774-777
  const double dxo = oc ? oc->prm.dxo : ss.dxo, dyo = oc ? oc->prm.dyo : ss.dyo, dxa = atm->prm.dxo, dya = atm->prm.dyo;
  P.D0up = q.D0up; P.xlamda = q.xlamda; P.Dmdown = q.Dmdown; P.Dmup = q.Dmup; P.dmdu = q.Dmdown - q.Dmup;
  P.ocfrac = dxo * dyo / (dxa * dya);
  P.fmafac = q.Adown11 * 0.25 / atm->prm.gpoc[0];
  P.fmatop = 0.25 * (q.Cmup + q.C1down);
  P.hmafac = -q.hmadmp - q.Bmup - q.B1down;
  P.hmat = q.hmat;
  P.ocnorm = 1.0 / ((double)P.nxto * (double)P.nyto); // src/parameters_data.F:88
}

static int launch_xf_heat(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm) {
  QgXfHeatParams P;
  xf_heat_fill(oc, atm, P);
  hipStream_t st = atm->stream;
  hipLaunchKernelGGL(k_xf_heat_oc, dim3(P.nxaooc, P.nyaooc), dim3(64), 0, st, P);
  hipLaunchKernelGGL(k_xf_heat_atm, dim3((P.nxta + 63) / 64, (P.nyta + 3) / 4), dim3(OML_NT), 0, st, P);
  hipLaunchKernelGGL(k_xf_heat_final, dim3(1), dim3(OML_NT), 0, st, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

// (fnetoc comes with the T rows the ocean handle holds: a y-slab's local rows for qgcm_hip_xforc_slab_get)
static int xf_heat_get(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, double *fnetoc, double *fnetat, double *scal) {
  HIPCHECK(hipStreamSynchronize(atm->stream)); // (xforc ran on the atmosphere's stream)
  if (fnetoc && download2d(oc, fnetoc, oc->oml.fnet, oc->oml.ldt, oc->g.nxt, oc->g.ny - 1)) return 1;
  if (fnetat && download2d(atm, fnetat, atm->tav.fnet, atm->aml.ldt, atm->g.nxt, atm->g.ny - 1)) return 1;
  if (scal) {
    HIPCHECK(hipMemcpyAsync(scal, atm->xf.heat.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, atm->stream));
    HIPCHECK(hipStreamSynchronize(atm->stream));
  }
  return 0;
}

extern "C" int qgcm_hip_xforc_heat_get(qgcm_hip_handle oc, qgcm_hip_handle atm, double *fnetoc, double *fnetat, double *scal) {
  const char *who = "qgcm_hip_xforc_heat_get";
  if (!oc) QG_FAIL("%s: the heat half needs an ocean (oc = NULL)", who);
  if (xf_ready(oc, atm, who)) return 1;
  if (!atm->xf.heat.on) QG_FAIL("%s: qgcm_hip_xforc_heat_init has not been called", who);
  return xf_heat_get(oc, atm, fnetoc, fnetat, scal);
}

// ---------------------------------------------------------------------------
// xforc for an ocean held as y-slabs under a replicated whole-domain atmosphere: every rank holds its slab
// and, on the same device, a replica of the atmosphere that it steps redundantly.  With tau_udiff off the fine stress
// and every atmosphere-side product depend on pam only: the kernels of k_xforc.h run unchanged on the replica.  The
// ocean side is local to the slab's rows (k_xf_tauo at the slab's global row offset, k_wekto, k_xforc_slab.h); the
// cells' heat sums are partial sums over the owned points, all-gathered by the caller between _part and _combine and
// added in rank order on every rank, so the replicas stay bitwise identical.
// ---------------------------------------------------------------------------
hipError_t qg_launch_xf_slab_ocean(hipStream_t st, const QgXfSlabParams &P);
hipError_t qg_launch_xf_heat_oc_slab(hipStream_t st, const QgXfHeatSlabParams &S);
hipError_t qg_launch_xf_heat_combine(hipStream_t st, const double *gath, int nranks, int ncell, long stride, long off, double *cell,
                                     double *part);
hipError_t qg_launch_xf_win_fine(hipStream_t st, const QgXfParams &P, int c0, int c1);
hipError_t qg_launch_xf_win_band(hipStream_t st, const QgXfParams &P, int a0, int a1, int t0, int t1, int lines, bool stage);
hipError_t qg_launch_xf_band_pack(hipStream_t st, const QgXfBandMsg &B);
hipError_t qg_launch_xf_band_scatter(hipStream_t st, const QgXfBandMsg &B);

extern "C" int qgcm_hip_xforc_slab_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_params *p) {
  return xf_init(oc, atm, p, "qgcm_hip_xforc_slab_init", true);
}

extern "C" int qgcm_hip_xforc_heat_slab_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_heat_params *p) {
  return xf_heat_init(oc, atm, p, "qgcm_hip_xforc_heat_slab_init", true);
}

// ---- the band plan, host code without a device -----------------------------------------------------------------
// One rank's windows from its band a0 .. a1 of atmosphere p rows and the global ocean p rows g0 .. g1 its slab owns (it
// holds three halo rows more towards each neighbour: qgcm_hip_create); nyg: the basin's p rows.  The fine p rows the band's outputs, the line sums the rank owns and the
// slab's k_xf_tauo read are two intervals (read off k_xforc_rows.inc); each becomes the cell rows that hold it.
static void xf_band_windows(int nyta, int ndxr, int ny1, int nyg, int a0, int a1, int g0, int g1, qgcm_hip_xforc_band *b) {
  const int n = ndxr, nypa = nyta + 1, nytaor = nyta * n, nypaor = nytaor + 1, odd = n % 2, nijwid = n + odd;
  const int slo = g0 - 3 > 1 ? g0 - 3 : 1, shi = g1 + 3 < nyg ? g1 + 3 : nyg; // the rows the slab holds
  memset(b, 0, sizeof(*b));
  b->a0 = a0; b->a1 = a1;
  // a line sum belongs to the rank that owns its outer row: one owner each
  b->own = (a0 == 1 ? 1 : 0) | (a1 == nypa ? 2 : 0) | (g0 == 1 ? 4 : 0) | (g1 == nyg ? 8 : 0);
  // tauxa, tauya, vekat at ja: fine row 1 + (ja-1) n, on a0 .. min(a1+1, nypa); uekat at ja <= nyta: that row and the n above
  int lo = 1 + (a0 - 1) * n, hi = 1 + (a1 < nyta ? a1 : nyta) * n;
  // wekpa at ja: fine T rows jbeg .. jbeg + nijwid - 1 clipped to 1 .. nytaor; T row j reads p rows j, j + 1
  const int jb0 = (a0 - 1) * n - (n - 1) / 2, jb1 = (a1 - 1) * n - (n - 1) / 2;
  b->t0 = jb0 > 1 ? jb0 : 1;
  b->t1 = jb1 + nijwid - 1 < nytaor ? jb1 + nijwid - 1 : nytaor;
  if (b->t0 < lo) lo = b->t0;
  if (b->t1 + 1 > hi) hi = b->t1 + 1;
  // the atmosphere's line sums: rows jsou (odd n: and jsou + 1), jnor (and jnor - 1)
  const int jsou = 1 + n / 2, jnor = nypaor - n / 2;
  if (b->own & 1) { if (jsou < lo) lo = jsou; if (jsou + odd > hi) hi = jsou + odd; }
  if (b->own & 2) { if (jnor - odd < lo) lo = jnor - odd; if (jnor > hi) hi = jnor; }
  auto cell = [&](int f) { const int c = (f - 1) / n + 1; return c < nyta ? c : nyta; }; // (fine row nypaor: cell row nyta)
  const int ca0 = cell(lo), ca1 = cell(hi);
  // the slab: k_xf_tauo at local row j reads the fine row jocoff + joff + j; the cyclic ocean's line sums read the fine
  // rows of ocean rows 1, 2 (the slab that owns row 1) and nyg - 1, nyg (the slab that owns row nyg): among them
  const int jocoff = (ny1 - 1) * n, cb0 = cell(jocoff + slo), cb1 = cell(jocoff + shi);
  if (cb0 <= ca1 + 1 && ca0 <= cb1 + 1) { // they touch: one interval
    b->nseg = 1;
    b->c0[0] = ca0 < cb0 ? ca0 : cb0;
    b->c1[0] = ca1 > cb1 ? ca1 : cb1;
  } else {
    b->nseg = 2;
    const bool af = ca0 < cb0;
    b->c0[0] = af ? ca0 : cb0; b->c1[0] = af ? ca1 : cb1;
    b->c0[1] = af ? cb0 : ca0; b->c1[1] = af ? cb1 : ca1;
  }
  for (int s = 0; s < b->nseg; ++s) { // the fine p rows k_xf_fine writes on these cell rows
    b->f0[s] = 1 + (b->c0[s] - 1) * n;
    b->f1[s] = b->c1[s] == nyta ? nypaor : b->c1[s] * n;
  }
}

// the bands: atmosphere p rows 1 .. nypa split evenly, the first nypa % nranks bands one row longer
static void xf_band_of(int nypa, int rank, int nranks, int *a0, int *a1) {
  const int base = nypa / nranks, rem = nypa % nranks;
  *a0 = 1 + rank * base + (rank < rem ? rank : rem);
  *a1 = *a0 + base + (rank < rem ? 1 : 0) - 1;
}

extern "C" int qgcm_hip_xforc_bands(int nxpa, int nyta, int ndxr, int ny1, int nyaooc, int nranks, const int *slab_lo,
                                    const int *slab_hi, qgcm_hip_xforc_band *out) {
  const char *who = "qgcm_hip_xforc_bands";
  if (!slab_lo || !slab_hi || !out) QG_FAIL("%s: null argument", who);
  if (nxpa < 2 || nyta < 2 || ndxr < 1 || ny1 < 1 || nyaooc < 1 || ny1 + nyaooc - 1 > nyta)
    QG_FAIL("%s: bad geometry (nxpa %d, nyta %d, ndxr %d, ny1 %d, nyaooc %d)", who, nxpa, nyta, ndxr, ny1, nyaooc);
  const int nypa = nyta + 1, nyg = nyaooc * ndxr + 1;
  if (nranks < 1 || nranks > nypa) QG_FAIL("%s: %d ranks for %d atmosphere rows (every rank needs a band)", who, nranks, nypa);
  for (int r = 0; r < nranks; ++r)
    if (slab_lo[r] < 1 || slab_hi[r] > nyg || slab_hi[r] < slab_lo[r])
      QG_FAIL("%s: rank %d owns ocean rows %d..%d outside 1..%d", who, r, slab_lo[r], slab_hi[r], nyg);
  const int nrow = (nypa + nranks - 1) / nranks; // the longest band
  for (int r = 0; r < nranks; ++r) {
    int a0, a1;
    xf_band_of(nypa, r, nranks, &a0, &a1);
    xf_band_windows(nyta, ndxr, ny1, nyg, a0, a1, slab_lo[r], slab_hi[r], &out[r]);
    out[r].nrow = nrow;
    out[r].mom_len = (int)xfb_mom_len(nrow, nxpa);
  }
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_bands(qgcm_hip_handle oc, qgcm_hip_handle atm, int a0, int a1, int nrow, int nranks) {
  const char *who = "qgcm_hip_xforc_slab_bands";
  if (xf_ready(oc, atm, who, true)) return 1;
  auto &x = atm->xf;
  if (x.sums.on) QG_FAIL("%s: this pair runs the owner-computed sums (qgcm_hip_xforc_slab_sums): the modes exclude each other", who);
  const int nypa = atm->g.ny;
  if (a0 < 1 || a1 > nypa || a1 < a0) QG_FAIL("%s: the band %d..%d lies outside the atmosphere's rows 1..%d", who, a0, a1, nypa);
  if (nranks < 1 || nranks > nypa) QG_FAIL("%s: %d ranks for %d atmosphere rows", who, nranks, nypa);
  if (nrow < a1 - a0 + 1 || nrow > nypa) QG_FAIL("%s: the common row count %d does not hold the band %d..%d (or exceeds %d)", who, nrow, a0, a1, nypa);
  if ((long)XFB_NF * nranks > 65535) QG_FAIL("%s: %d ranks exceed the scatter's launch limit", who, nranks);
  const QgGeom &go = oc->g;
  HIPCHECK(hipStreamSynchronize(atm->stream));
  xf_band_windows(nypa - 1, x.prm.ndxr, x.prm.ny1, go.nyg, a0, a1, go.joff + go.jlo, go.joff + go.jhi, &x.bands.plan);
  x.bands.plan.nrow = nrow;
  x.bands.plan.mom_len = (int)xfb_mom_len(nrow, atm->g.nx);
  x.bands.nranks = nranks;
  const char *e = getenv("QGCM_HIP_XF_POISON");
  x.bands.poison = e && atoi(e) == 1;
  x.bands.on = true;
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_msg_len(qgcm_hip_handle atm) {
  if (!atm || !atm->xf.on || !atm->xf.slab) return 0;
  const int heat = atm->xf.heat.on ? 4 * atm->xf.prm.nxaooc * atm->xf.prm.nyaooc : 0;
  if (atm->xf.bands.on) return atm->xf.bands.plan.mom_len + heat; // the momentum block, then the heat block
  if (atm->xf.sums.on) return atm->xf.sums.plan.mom_len + heat;
  return heat; // (replicated: the momentum half alone exchanges nothing)
}

// ---- tau_udiff on a slab set-up ----------------------------------------------------------------------------------
// The ocean enters the momentum half at one place, xf_point (k_xforc_rows.h), which reads pom(:,:,1) around a fine point
// above the sea.  Every rank assembles the basin's pom(:,:,1) from the ranks' owned rows ahead of the atmosphere side
// (pack, the caller's all-gather, assemble); the stress kernels then run unchanged with P.udiff = 1 on the assembled
// array.  No sum changes its order: the results are the whole-domain call's bits on any rank count.  The drag constants
// of the sea (cdrfab, qu2fab) and zbfcoc, hxofac are xf_fill's, from the constants the set-up kept, as the whole-domain
// set-up with tau_udiff has them.
hipError_t qg_launch_xf_pom_pack(hipStream_t st, const QgXfPomMsg &M);
hipError_t qg_launch_xf_pom_assemble(hipStream_t st, const QgXfPomMsg &M);

extern "C" int qgcm_hip_xforc_slab_udiff(qgcm_hip_handle oc, qgcm_hip_handle atm, int nrow, int nranks) {
  const char *who = "qgcm_hip_xforc_slab_udiff";
  if (xf_ready(oc, atm, who, true)) return 1;
  auto &x = atm->xf;
  const QgGeom &go = oc->g;
  const int own = go.jhi - go.jlo + 1;
  if (nranks < 1 || nranks > 65535) QG_FAIL("%s: nranks = %d outside 1..65535", who, nranks);
  if (x.sums.on) QG_FAIL("%s: this pair runs the owner-computed sums (qgcm_hip_xforc_slab_sums): the modes exclude each other", who);
  if (nrow < own || nrow > go.nyg)
    QG_FAIL("%s: the common row count %d does not hold this slab's %d owned rows (or exceeds the basin's %d)", who, nrow, own, go.nyg);
  HIPCHECK(hipStreamSynchronize(atm->stream));
  const int ld = round_up(go.nx, 16);
  const size_t n = (size_t)ld * go.nyg;
  if (x.udiff.pom.grow(n, "xforc's assembled surface pressure")) return 1;
  HIPCHECK(hipMemsetAsync(x.udiff.pom, 0, n * sizeof(double), atm->stream));
  x.udiff.ld = ld;
  x.udiff.nrow = nrow;
  x.udiff.nranks = nranks;
  const char *e = getenv("QGCM_HIP_XF_POISON");
  x.udiff.poison = e && atoi(e) == 1;
  x.udiff.fresh = false;
  x.udiff.on = true;
  return 0;
}

static int xf_udiff_ready(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const char *who) {
  if (xf_ready(oc, atm, who, true)) return 1;
  if (!atm->xf.udiff.on) QG_FAIL("%s: qgcm_hip_xforc_slab_udiff has not been called for this pair", who);
  return 0;
}

static void xf_pom_msg_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, QgXfPomMsg &M) {
  const QgGeom &go = oc->g;
  const auto &u = atm->xf.udiff;
  memset(&M, 0, sizeof(M));
  M.nxpo = go.nx; M.nypo = go.nyg; M.ldo = go.ldx; M.lda = u.ld;
  M.g0 = go.joff + go.jlo; M.g1 = go.joff + go.jhi; M.jlo = go.jlo;
  M.nrow = u.nrow; M.nranks = u.nranks;
  M.stride = xfp_len(u.nrow, go.nx);
}

extern "C" int qgcm_hip_xforc_slab_pom_len(qgcm_hip_handle oc, qgcm_hip_handle atm, long *n) {
  const char *who = "qgcm_hip_xforc_slab_pom_len";
  if (!n) QG_FAIL("%s: null argument", who);
  if (xf_udiff_ready(oc, atm, who)) return 1;
  *n = xfp_len(atm->xf.udiff.nrow, oc->g.nx);
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_pom_pack(qgcm_hip_handle oc, qgcm_hip_handle atm, double *send_dev) {
  const char *who = "qgcm_hip_xforc_slab_pom_pack";
  if (xf_udiff_ready(oc, atm, who)) return 1;
  if (!send_dev) QG_FAIL("%s: send_dev must hold qgcm_hip_xforc_slab_pom_len doubles", who);
  auto &x = atm->xf;
  hipStream_t st = atm->stream;
  QgXfPomMsg M;
  xf_pom_msg_fill(oc, atm, M);
  M.pom = oc->p[oc->ip ^ 1]; // layer 1 of the lagged pressure, as xf_fill's P.pom
  M.msg = send_dev;
  HIPCHECK(hipEventRecord(x.ev_oc, oc->stream)); // after everything queued on the slab's stream, as the part waits
  HIPCHECK(hipStreamWaitEvent(st, x.ev_oc, 0));
  HIPCHECK(qg_launch_xf_pom_pack(st, M));
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_pom_assemble(qgcm_hip_handle oc, qgcm_hip_handle atm, const double *gath_dev, int nranks) {
  const char *who = "qgcm_hip_xforc_slab_pom_assemble";
  if (xf_udiff_ready(oc, atm, who)) return 1;
  auto &x = atm->xf;
  if (!gath_dev) QG_FAIL("%s: gath_dev must hold nranks messages of qgcm_hip_xforc_slab_pom_len doubles", who);
  if (nranks != x.udiff.nranks)
    QG_FAIL("%s: nranks = %d, the shear term was set up for %d ranks (qgcm_hip_xforc_slab_udiff)", who, nranks, x.udiff.nranks);
  hipStream_t st = atm->stream;
  QgXfPomMsg M;
  xf_pom_msg_fill(oc, atm, M);
  M.gath = gath_dev;
  M.all = x.udiff.pom;
  if (x.udiff.poison) // a row no rank owns, or one the copy misses, shows in the stress above it
    HIPCHECK(hipMemsetAsync(x.udiff.pom, 0xFF, (size_t)x.udiff.ld * M.nypo * sizeof(double), st));
  HIPCHECK(qg_launch_xf_pom_assemble(st, M));
  x.udiff.fresh = true;
  return 0;
}

// ---- tau_udiff by owner-computed sums -----------------------------------------------------------------------------
// xf_point reads pom at ocean rows jo - 1 .. jo + 1 of a fine point above the sea, so the fine stress on a fine row needs
// three ocean rows: a rank forms it above the rows it owns from its own pressure and four rows beyond each seam, which the
// direct neighbours send (pack, a small all-gather by the caller, assemble).  Of the coarse products only uekat's
// meridional lines and wekpa's boxes are sums a seam can cut: they travel as partial sums and are added in rank order.
hipError_t qg_launch_xf_edge_pack(hipStream_t st, const QgXfEdgeMsg &M);
hipError_t qg_launch_xf_edge_assemble(hipStream_t st, const QgXfEdgeMsg &M);
hipError_t qg_launch_xf_sums_wektaor(hipStream_t st, const QgXfParams &P, int t0, int t1);
hipError_t qg_launch_xf_sums_part(hipStream_t st, const QgXfParams &P, const QgXfSumMsg &B);
hipError_t qg_launch_xf_sums_combine(hipStream_t st, const QgXfSumMsg &B);

// The ownership plan, host code without a device: the windows are read off the kernels' index expressions
// (k_xforc_rows.inc, k_xforc_slab.h), as xf_band_windows' are.
static int xf_sums_plan(const char *who, int nxpa, int nyta, int ndxr, int ny1, int nyaooc, int nranks, const int *lo, const int *hi,
                        qgcm_hip_xforc_sum *out) {
  if (!lo || !hi || !out) QG_FAIL("%s: null argument", who);
  if (nxpa < 2 || nyta < 2 || ndxr < 1 || ny1 < 1 || nyaooc < 1 || ny1 + nyaooc - 1 > nyta)
    QG_FAIL("%s: bad geometry (nxpa %d, nyta %d, ndxr %d, ny1 %d, nyaooc %d)", who, nxpa, nyta, ndxr, ny1, nyaooc);
  if (nranks < 1) QG_FAIL("%s: nranks = %d, need at least one rank", who, nranks);
  const int n = ndxr, nypa = nyta + 1, nytaor = nyta * n, nypaor = nytaor + 1, odd = n % 2, nijwid = n + odd;
  const int nyg = nyaooc * n + 1, jocoff = (ny1 - 1) * n;
  for (int r = 0; r < nranks; ++r) {
    const int want = r ? hi[r - 1] + 1 : 1;
    if (lo[r] != want || hi[r] < lo[r] || hi[r] > nyg)
      QG_FAIL("%s: the owned rows do not tile 1..%d: rank %d owns %d..%d, its range must begin at %d", who, nyg, r, lo[r], hi[r], want);
  }
  if (hi[nranks - 1] != nyg) QG_FAIL("%s: the owned rows do not tile 1..%d: the last rank's end at %d", who, nyg, hi[nranks - 1]);
  for (int r = 0; r < nranks; ++r)
    if (hi[r] - lo[r] + 1 < 4)
      QG_FAIL("%s: rank %d owns %d ocean rows, fewer than 4 (the rows beyond a seam come from the direct neighbours' edges only)", who,
              r, hi[r] - lo[r] + 1);
  auto cell = [&](int f) { const int c = (f - 1) / n + 1; return c < nyta ? c : nyta; }; // (fine row nypaor: cell row nyta)
  const int jsou = 1 + n / 2, jnor = nypaor - n / 2;
  int nrow = 0;
  for (int r = 0; r < nranks; ++r) {
    qgcm_hip_xforc_sum &s = out[r];
    memset(&s, 0, sizeof(s));
    s.g0 = lo[r]; s.g1 = hi[r];
    s.f0 = r == 0 ? 1 : jocoff + lo[r];
    s.f1 = r == nranks - 1 ? nypaor : jocoff + hi[r];
    s.t0 = s.f0; s.t1 = s.f1 < nytaor ? s.f1 : nytaor; // T row j reads p rows j, j + 1
    // the stress the rank holds correct: its own rows, row f1 + 1 for its last T row, and the fine rows under the three
    // halo rows of its slab (k_xf_tauo)
    s.w0 = s.f0 - 3 > 1 ? s.f0 - 3 : 1;
    s.w1 = s.f1 + 3 < nypaor ? s.f1 + 3 : nypaor;
    s.c0 = cell(s.w0); s.c1 = cell(s.w1);
    s.u0 = s.c0 > 1 ? s.c0 - 1 : 1; s.u1 = s.c1 + 2 < nypa ? s.c1 + 2 : nypa; // (qg_launch_xf_win_fine)
    // a line sum belongs to the rank whose rows hold its outer row; odd ndxr: the partner row must be that rank's too
    if (jsou >= s.f0 && jsou <= s.f1) {
      if (odd && jsou + 1 > s.f1)
        QG_FAIL("%s: txisat reads the fine rows %d and %d, which rank %d (fine rows %d..%d) and the next would share", who, jsou,
                jsou + 1, r, s.f0, s.f1);
      s.own |= 1;
    }
    if (jnor >= s.f0 && jnor <= s.f1) {
      if (odd && jnor - 1 < s.f0)
        QG_FAIL("%s: txinat reads the fine rows %d and %d, which rank %d (fine rows %d..%d) and the one before would share", who,
                jnor - 1, jnor, r, s.f0, s.f1);
      s.own |= 2;
    }
    s.own |= (lo[r] == 1 ? 4 : 0) | (hi[r] == nyg ? 8 : 0);
    // the coarse rows whose sample (fine row joff), uekat line (joff .. joff + n) or wekpa box (fine T rows) meets the rank's
    s.a0 = 0;
    for (int ja = 1; ja <= nypa; ++ja) {
      const int joff = 1 + (ja - 1) * n;
      const int jbeg = (ja - 1) * n - (n - 1) / 2;
      const int jlo = jbeg > 1 ? jbeg : 1, jhi = jbeg + nijwid - 1 < nytaor ? jbeg + nijwid - 1 : nytaor;
      const bool hit = (joff >= s.f0 && joff <= s.f1) || (ja <= nyta && joff <= s.f1 && joff + n >= s.f0) || (jlo <= s.t1 && jhi >= s.t0);
      if (!hit) continue;
      if (!s.a0) s.a0 = ja;
      s.a1 = ja;
    }
    if (s.a1 - s.a0 + 1 > nrow) nrow = s.a1 - s.a0 + 1;
  }
  for (int r = 0; r < nranks; ++r) {
    out[r].nrow = nrow;
    out[r].mom_len = (int)xfs_mom_len(nrow, nxpa);
  }
  return 0;
}

extern "C" int qgcm_hip_xforc_sums(int nxpa, int nyta, int ndxr, int ny1, int nyaooc, int nranks, const int *slab_lo,
                                   const int *slab_hi, qgcm_hip_xforc_sum *out) {
  return xf_sums_plan("qgcm_hip_xforc_sums", nxpa, nyta, ndxr, ny1, nyaooc, nranks, slab_lo, slab_hi, out);
}

extern "C" int qgcm_hip_xforc_slab_sums(qgcm_hip_handle oc, qgcm_hip_handle atm, int rank, int nranks, const int *slab_lo,
                                        const int *slab_hi) {
  const char *who = "qgcm_hip_xforc_slab_sums";
  if (xf_ready(oc, atm, who, true)) return 1;
  auto &x = atm->xf;
  const QgGeom &go = oc->g;
  if (x.bands.on) QG_FAIL("%s: this pair runs the banded atmosphere side (qgcm_hip_xforc_slab_bands): the modes exclude each other", who);
  if (x.udiff.on) QG_FAIL("%s: this pair gathers the surface pressure (qgcm_hip_xforc_slab_udiff): the modes exclude each other", who);
  if (nranks < 1 || nranks > 65535) QG_FAIL("%s: nranks = %d outside 1..65535", who, nranks);
  if (rank < 0 || rank >= nranks) QG_FAIL("%s: rank %d outside 0..%d", who, rank, nranks - 1);
  std::vector<qgcm_hip_xforc_sum> plan(nranks);
  if (xf_sums_plan(who, atm->g.nx, atm->g.ny - 1, x.prm.ndxr, x.prm.ny1, x.prm.nyaooc, nranks, slab_lo, slab_hi, plan.data())) return 1;
  if (slab_lo[rank] != go.joff + go.jlo || slab_hi[rank] != go.joff + go.jhi)
    QG_FAIL("%s: rank %d of the plan owns ocean rows %d..%d, this slab owns %d..%d", who, rank, slab_lo[rank], slab_hi[rank],
            go.joff + go.jlo, go.joff + go.jhi);
  if (go.jhi - go.jlo + 1 + 2 * XFE_ROWS > 65535) QG_FAIL("%s: %d owned rows exceed the assemble's launch limit", who, go.jhi - go.jlo + 1);
  HIPCHECK(hipStreamSynchronize(atm->stream));
  const int ld = round_up(go.nx, 16);
  const size_t n = (size_t)ld * go.nyg;
  if (x.udiff.pom.grow(n, "xforc's assembled surface pressure")) return 1;
  HIPCHECK(hipMemsetAsync(x.udiff.pom, 0, n * sizeof(double), atm->stream));
  x.udiff.ld = ld;
  x.sums.plan = plan[rank];
  x.sums.rank = rank;
  x.sums.nranks = nranks;
  const char *e = getenv("QGCM_HIP_XF_POISON");
  x.sums.poison = e && atoi(e) == 1;
  x.sums.fresh = false;
  x.sums.on = true;
  return 0;
}

static int xf_sums_ready(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const char *who) {
  if (xf_ready(oc, atm, who, true)) return 1;
  if (!atm->xf.sums.on) QG_FAIL("%s: qgcm_hip_xforc_slab_sums has not been called for this pair", who);
  return 0;
}

static void xf_edge_msg_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, QgXfEdgeMsg &M) {
  const QgGeom &go = oc->g;
  const auto &x = atm->xf;
  memset(&M, 0, sizeof(M));
  M.nxpo = go.nx; M.nypo = go.nyg; M.ldo = go.ldx; M.lda = x.udiff.ld;
  M.g0 = go.joff + go.jlo; M.g1 = go.joff + go.jhi; M.jlo = go.jlo;
  M.rank = x.sums.rank; M.nranks = x.sums.nranks;
  M.stride = xfe_len(go.nx);
  M.pom = oc->p[oc->ip ^ 1]; // layer 1 of the lagged pressure, as xf_fill's P.pom
}

extern "C" int qgcm_hip_xforc_slab_edge_len(qgcm_hip_handle oc, qgcm_hip_handle atm, long *n) {
  const char *who = "qgcm_hip_xforc_slab_edge_len";
  if (!n) QG_FAIL("%s: null argument", who);
  if (xf_sums_ready(oc, atm, who)) return 1;
  *n = xfe_len(oc->g.nx);
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_edge_pack(qgcm_hip_handle oc, qgcm_hip_handle atm, double *send_dev) {
  const char *who = "qgcm_hip_xforc_slab_edge_pack";
  if (xf_sums_ready(oc, atm, who)) return 1;
  if (!send_dev) QG_FAIL("%s: send_dev must hold qgcm_hip_xforc_slab_edge_len doubles", who);
  auto &x = atm->xf;
  hipStream_t st = atm->stream;
  QgXfEdgeMsg M;
  xf_edge_msg_fill(oc, atm, M);
  M.msg = send_dev;
  HIPCHECK(hipEventRecord(x.ev_oc, oc->stream)); // after everything queued on the slab's stream, as the part waits
  HIPCHECK(hipStreamWaitEvent(st, x.ev_oc, 0));
  HIPCHECK(qg_launch_xf_edge_pack(st, M));
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_edge_assemble(qgcm_hip_handle oc, qgcm_hip_handle atm, const double *gath_dev, int nranks) {
  const char *who = "qgcm_hip_xforc_slab_edge_assemble";
  if (xf_sums_ready(oc, atm, who)) return 1;
  auto &x = atm->xf;
  if (!gath_dev) QG_FAIL("%s: gath_dev must hold nranks messages of qgcm_hip_xforc_slab_edge_len doubles", who);
  if (nranks != x.sums.nranks)
    QG_FAIL("%s: nranks = %d, the sums were set up for %d ranks (qgcm_hip_xforc_slab_sums)", who, nranks, x.sums.nranks);
  hipStream_t st = atm->stream;
  QgXfEdgeMsg M;
  xf_edge_msg_fill(oc, atm, M);
  M.gath = gath_dev;
  M.all = x.udiff.pom;
  HIPCHECK(hipEventRecord(x.ev_oc, oc->stream)); // (the owned rows are read from the slab's pressure once more)
  HIPCHECK(hipStreamWaitEvent(st, x.ev_oc, 0));
  if (x.sums.poison) // a row the rank does not hold shows in the stress above it
    HIPCHECK(hipMemsetAsync(x.udiff.pom, 0xFF, (size_t)x.udiff.ld * M.nypo * sizeof(double), st));
  HIPCHECK(qg_launch_xf_edge_assemble(st, M));
  x.sums.fresh = true;
  return 0;
}

static void xf_sum_msg_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const QgXfParams &P, QgXfSumMsg &B) {
  const auto &s = atm->xf.sums.plan;
  memset(&B, 0, sizeof(B));
  B.nxpa = P.nxpa; B.nxta = P.nxta; B.nypa = P.nypa; B.nyta = P.nyta; B.lda = P.lda; B.ldta = P.ldta; B.ldf = P.ldf; B.ldtf = P.ldtf;
  B.ndxr = P.ndxr; B.ndxodd = P.ndxodd; B.nijwid = P.nijwid; B.nxtaor = P.nxtaor; B.nytaor = P.nytaor; B.nypaor = P.nypaor;
  B.f0 = s.f0; B.f1 = s.f1; B.t0 = s.t0; B.t1 = s.t1; B.a0 = s.a0; B.a1 = s.a1; B.nrow = s.nrow;
  B.own = oc->g.cyc ? s.own : (s.own & 3); // (a box ocean has no line sums)
  B.txf = P.txf; B.tyf = P.tyf; B.wf = P.wf;
  B.tauxa = P.tauxa; B.tauya = P.tauya; B.uekat = P.uekat; B.vekat = P.vekat; B.wekpa = P.wekpa;
  B.uvekfc = P.uvekfc;
  B.sca = atm->sc;
  B.sco = oc->g.cyc ? oc->sc : nullptr;
}

// the pack's / the scatter's view of the replica
static void xf_band_msg_fill(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, QgXfBandMsg &B) {
  const auto &m = atm->atmon;
  const QgGeom &g = atm->g;
  const auto &b = atm->xf.bands.plan;
  memset(&B, 0, sizeof(B));
  B.nxpa = g.nx; B.nxta = g.nxt; B.nypa = g.ny; B.nyta = g.ny - 1; B.lda = g.ldx; B.ldta = m.ldt;
  B.a0 = b.a0; B.a1 = b.a1; B.nrow = b.nrow;
  B.own = oc->g.cyc ? b.own : (b.own & 3); // (a box ocean has no line sums)
  B.fld[0] = m.tauxa; B.fld[1] = m.tauya; B.fld[2] = m.uekat; B.fld[3] = m.vekat; B.fld[4] = m.wekta; B.fld[5] = atm->wekpo;
  B.sca = atm->sc;
  B.sco = oc->g.cyc ? oc->sc : nullptr;
}

// the ocean's next step reads wekpo, the stress, the line integrals and the mixed layer's forcing
static int xf_slab_handover(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm) {
  HIPCHECK(hipEventRecord(atm->xf.ev_atm, atm->stream));
  HIPCHECK(hipStreamWaitEvent(oc->stream, atm->xf.ev_atm, 0));
  return 0;
}

extern "C" int qgcm_hip_xforc_slab_part(qgcm_hip_handle oc, qgcm_hip_handle atm, double *send_dev) {
  const char *who = "qgcm_hip_xforc_slab_part";
  if (xf_ready(oc, atm, who, true)) return 1;
  auto &x = atm->xf;
  if (x.heat.on && !send_dev) QG_FAIL("%s: the heat half is set up: send_dev must hold qgcm_hip_xforc_slab_msg_len doubles", who);
  const bool banded = x.bands.on;
  if (banded && !send_dev) QG_FAIL("%s: the bands are set up: send_dev must hold qgcm_hip_xforc_slab_msg_len doubles", who);
  if (x.udiff.on && !x.udiff.fresh)
    QG_FAIL("%s: the surface pressure has not been assembled for this call (qgcm_hip_xforc_slab_pom_pack, the all-gather, qgcm_hip_xforc_slab_pom_assemble)", who);
  x.udiff.fresh = false;
  const bool sums = x.sums.on;
  if (sums && !send_dev) QG_FAIL("%s: the sums are set up: send_dev must hold qgcm_hip_xforc_slab_msg_len doubles", who);
  if (sums && !x.sums.fresh)
    QG_FAIL("%s: the edge rows have not been assembled for this call (qgcm_hip_xforc_slab_edge_pack, the all-gather, qgcm_hip_xforc_slab_edge_assemble)", who);
  x.sums.fresh = false;
  hipStream_t st = atm->stream;
  QgXfParams P;
  xf_fill(oc, atm, P);
  const QgGeom &go = oc->g;
  auto &mo = oc->mon;
  // Two parameter blocks.  PA, the atmosphere side's (k_xf_fine, k_xf_fine_win: xf_point): with tau_udiff the BASIN's
  // ocean grid, offsets and the assembled pom(:,:,1); without it no kernel of that side reads the ocean's
  // entries.  P, the ocean side's (k_xf_tauo): the slab's local rows at the slab's offset.
  QgXfParams PA = P;
  PA.sco = nullptr;
  if (x.udiff.on || sums) { // (sums: rows g0 - 4 .. g1 + 4 of the array hold the basin's bits)
    PA.udiff = 1;
    PA.nypo = go.nyg;
    PA.ldo = x.udiff.ld;
    PA.pom = x.udiff.pom;
  }
  // the slab's rows of the ocean: local row j is row j + joff of the basin (k_xf_tauo reads the fine row jocoff + j)
  P.jocoff += go.joff;
  P.sco = nullptr; // (k_xf_lines: the atmosphere's two sums; the cyclic ocean's are k_xf_lines_oc_slab's)
  HIPCHECK(hipEventRecord(x.ev_oc, oc->stream));
  HIPCHECK(hipStreamWaitEvent(st, x.ev_oc, 0));
  const dim3 b(XF_NT);
  if (banded) { // the atmosphere side on this rank's windows only
    const auto &bp = x.bands.plan;
    if (x.bands.poison) { // a read outside the computed windows shows in the results
      const size_t nf = (size_t)x.ldf * P.nypaor * sizeof(double);
      HIPCHECK(hipMemsetAsync(x.txf, 0xFF, nf, st));
      HIPCHECK(hipMemsetAsync(x.tyf, 0xFF, nf, st));
      HIPCHECK(hipMemsetAsync(x.wf, 0xFF, (size_t)x.ldtf * P.nytaor * sizeof(double), st));
    }
    for (int s = 0; s < bp.nseg; ++s) HIPCHECK(qg_launch_xf_win_fine(st, PA, bp.c0[s], bp.c1[s]));
    HIPCHECK(qg_launch_xf_win_band(st, PA, bp.a0, bp.a1, bp.t0, bp.t1, bp.own & 3, x.wekpa_stage));
  } else if (sums) { // the fine stress on the plan's one window, wektaor on the owned T rows
    const auto &sp = x.sums.plan;
    if (x.sums.poison) {
      const size_t nf = (size_t)x.ldf * P.nypaor * sizeof(double);
      HIPCHECK(hipMemsetAsync(x.txf, 0xFF, nf, st));
      HIPCHECK(hipMemsetAsync(x.tyf, 0xFF, nf, st));
      HIPCHECK(hipMemsetAsync(x.wf, 0xFF, (size_t)x.ldtf * P.nytaor * sizeof(double), st));
    }
    HIPCHECK(qg_launch_xf_win_fine(st, PA, sp.c0, sp.c1));
    HIPCHECK(qg_launch_xf_sums_wektaor(st, PA, sp.t0, sp.t1));
  } else
    HIPCHECK(launch_xf_atmos(PA, st, x.wekpa_stage));
  hipLaunchKernelGGL(k_xf_tauo, dim3((P.nxpo + XF_NT - 1) / XF_NT, P.nypo), b, 0, st, P);
  QgWekParams W;
  memset(&W, 0, sizeof(W));
  W.g = go; W.taux = mo.taux; W.tauy = mo.tauy; W.wekto = mo.wekto; W.wekpo = oc->wekpo; W.ldt = mo.ldt;
  W.hxofac = P.hxofac;
  hipLaunchKernelGGL(k_wekto, dim3((go.nxt + 255) / 256, go.ny - 1), dim3(256), 0, st, W);
  QgXfSlabParams S;
  memset(&S, 0, sizeof(S));
  S.nx = go.nx; S.nxt = go.nxt; S.nyl = go.ny; S.joff = go.joff; S.nyg = go.nyg;
  S.ldx = go.ldx; S.ldt = mo.ldt; S.ldf = x.ldf;
  S.cyc = go.cyc; S.iocoff = P.iocoff; S.jocoff = P.jocoff - go.joff;
  S.txf = x.txf; S.wekto = mo.wekto; S.wekpo = oc->wekpo; S.sco = oc->sc;
  S.raoro = P.raoro; S.dxo = P.dxo;
  S.lines = banded ? (x.bands.plan.own >> 2) & 3 : sums ? (x.sums.plan.own >> 2) & 3 : 3; // only the sums whose ocean rows this slab holds
  HIPCHECK(qg_launch_xf_slab_ocean(st, S));
  if (oc->oml.on) { // the mixed layer's own forcing buffers (same pitches)
    auto &o = oc->oml;
    const size_t nP = (size_t)go.ldx * go.ny * sizeof(double), nT = (size_t)o.ldt * (go.ny - 1) * sizeof(double);
    HIPCHECK(hipMemcpyAsync(o.taux, mo.taux, nP, hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemcpyAsync(o.tauy, mo.tauy, nP, hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemcpyAsync(o.wekto, mo.wekto, nT, hipMemcpyDeviceToDevice, st));
  }
  if (banded) { // the message's momentum block (the atmosphere's line sums were k_xf_lines_win's, on the ranks that own them)
    QgXfBandMsg B;
    xf_band_msg_fill(oc, atm, B);
    B.msg = send_dev;
    HIPCHECK(qg_launch_xf_band_pack(st, B));
  } else if (sums) { // the line sums this rank owns, its samples and its partial sums -> the message's momentum block
    QgXfSumMsg B;
    xf_sum_msg_fill(oc, atm, PA, B);
    B.msg = send_dev;
    HIPCHECK(qg_launch_xf_sums_part(st, PA, B));
  } else
    hipLaunchKernelGGL(k_xf_lines, dim3(1), b, 0, st, P);
  HIPCHECK(hipGetLastError());
  if (x.heat.on) { // fnetoc on the slab's T rows and this rank's partial cell sums (src/xfosubs.F:774-817)
    QgXfHeatSlabParams H;
    memset(&H, 0, sizeof(H));
    xf_heat_fill(oc, atm, H.h);
    H.joff = go.joff; H.nytl = go.ny - 1;
    H.jT0 = go.jlo; H.jT1 = (go.jhi + go.joff == go.nyg) ? go.jhi - 1 : go.jhi; // T row j lies between p rows j and j+1
    H.msg = send_dev + (banded ? x.bands.plan.mom_len : sums ? x.sums.plan.mom_len : 0);
    HIPCHECK(qg_launch_xf_heat_oc_slab(st, H));
  }
  return xf_slab_handover(oc, atm);
}

extern "C" int qgcm_hip_xforc_slab_combine(qgcm_hip_handle oc, qgcm_hip_handle atm, const double *gath_dev, int nranks) {
  const char *who = "qgcm_hip_xforc_slab_combine";
  if (xf_ready(oc, atm, who, true)) return 1;
  auto &x = atm->xf;
  const bool banded = x.bands.on, sums = x.sums.on;
  if (!x.heat.on && !banded && !sums) QG_FAIL("%s: qgcm_hip_xforc_heat_slab_init has not been called (the momentum half has nothing to combine)", who);
  if (!gath_dev || nranks < 1) QG_FAIL("%s: null buffer or nranks = %d", who, nranks);
  if (banded && nranks != x.bands.nranks)
    QG_FAIL("%s: nranks = %d, the bands were set up for %d ranks (qgcm_hip_xforc_slab_bands)", who, nranks, x.bands.nranks);
  if (sums && nranks != x.sums.nranks)
    QG_FAIL("%s: nranks = %d, the sums were set up for %d ranks (qgcm_hip_xforc_slab_sums)", who, nranks, x.sums.nranks);
  hipStream_t st = atm->stream;
  const long mom = banded ? x.bands.plan.mom_len : sums ? x.sums.plan.mom_len : 0;
  if (sums) { // samples and line sums from their owners, the cut sums added in rank order; then wekta on the whole grid
    QgXfParams P;
    xf_fill(oc, atm, P);
    QgXfSumMsg B;
    xf_sum_msg_fill(oc, atm, P, B);
    B.gath = gath_dev;
    B.nranks = nranks;
    B.stride = qgcm_hip_xforc_slab_msg_len(atm);
    HIPCHECK(qg_launch_xf_sums_combine(st, B));
    hipLaunchKernelGGL(k_xf_wekta, dim3((P.nxta + XF_NT - 1) / XF_NT, P.nyta), dim3(XF_NT), 0, st, P);
    HIPCHECK(hipGetLastError());
    if (!x.heat.on) return xf_slab_handover(oc, atm);
  }
  if (banded) { // every rank's rows and line sums into this replica (a copy: no sum changes its order)
    QgXfBandMsg B;
    xf_band_msg_fill(oc, atm, B);
    B.gath = gath_dev;
    B.nranks = nranks;
    B.stride = qgcm_hip_xforc_slab_msg_len(atm);
    HIPCHECK(qg_launch_xf_band_scatter(st, B));
    if (!x.heat.on) return xf_slab_handover(oc, atm);
  }
  QgXfHeatParams P;
  xf_heat_fill(oc, atm, P);
  HIPCHECK(qg_launch_xf_heat_combine(st, gath_dev, nranks, P.ncell, mom + 4L * P.ncell, mom, P.cell, P.part));
  hipLaunchKernelGGL(k_xf_heat_atm, dim3((P.nxta + 63) / 64, (P.nyta + 3) / 4), dim3(OML_NT), 0, st, P);
  hipLaunchKernelGGL(k_xf_heat_final, dim3(1), dim3(OML_NT), 0, st, P);
  HIPCHECK(hipGetLastError());
  return xf_slab_handover(oc, atm);
}

extern "C" int qgcm_hip_xforc_slab_get(qgcm_hip_handle oc, qgcm_hip_handle atm, double *tauxa, double *tauya, double *uekat,
                                       double *vekat, double *wekta, double *wekpa, double *tauxo, double *tauyo, double *wekto,
                                       double *wekpo, double *txi, double *fnetoc, double *fnetat, double *scal) {
  const char *who = "qgcm_hip_xforc_slab_get";
  if (xf_ready(oc, atm, who, true)) return 1;
  if ((fnetoc || fnetat || scal) && !atm->xf.heat.on) QG_FAIL("%s: qgcm_hip_xforc_heat_slab_init has not been called", who);
  if (xf_get(oc, atm, tauxa, tauya, uekat, vekat, wekta, wekpa, tauxo, tauyo, wekto, wekpo, txi)) return 1;
  return (fnetoc || fnetat || scal) ? xf_heat_get(oc, atm, fnetoc, fnetat, scal) : 0;
}

// ---------------------------------------------------------------------------
// heat half of xforc without an ocean: what a -Datmos_only build of src/xfosubs.F:711-853 runs, from an SST
// that is read once and held (src/q-gcm.F:753-786)
// ---------------------------------------------------------------------------
static int xf_sst_ready(qgcm_hip_ctx *atm, const char *who) {
  if (xf_ready(nullptr, atm, who)) return 1;
  if (!atm->xf.sst.on) QG_FAIL("%s: qgcm_hip_xforc_sst_init has not been called", who);
  return 0;
}

extern "C" int qgcm_hip_xforc_sst_init(qgcm_hip_handle atm, const qgcm_hip_xforc_sst_params *p) {
  const char *who = "qgcm_hip_xforc_sst_init";
  if (!atm || !p) QG_FAIL("%s: null atmosphere handle or parameters", who);
  if (check_atm(atm, who)) return 1;
  if (!atm->whole) QG_FAIL("%s: the atmosphere handle is a y-slab (xforc needs the whole domain)", who);
  if (!atm->xf.on) QG_FAIL("%s: qgcm_hip_xforc_init has not been called for this atmosphere", who);
  if (atm->xf.oc) QG_FAIL("%s: this atmosphere's xforc was set up with an ocean: its heat half is qgcm_hip_xforc_heat_init", who);
  if (!atm->aml.on) QG_FAIL("%s: qgcm_hip_aml_init has not been called for this atmosphere", who);
  if (!p->fsa || !p->xta || !p->yta || !p->xto || !p->yto || !p->sst) QG_FAIL("%s: a table, a coordinate array or the SST is NULL", who);
  const qgcm_hip_xforc_params &x = atm->xf.prm;
  const int nxta = atm->g.nxt, nyta = atm->g.ny - 1;
  // (qgcm_hip_xforc_init checks the position of the sea only against an ocean handle)
  if (x.nxaooc < 1 || x.nyaooc < 1 || x.nx1 < 1 || x.ny1 < 1 || x.nx1 + x.nxaooc - 1 > nxta || x.ny1 + x.nyaooc - 1 > nyta)
    QG_FAIL("%s: the sea (nx1 = %d, ny1 = %d, nxaooc = %d, nyaooc = %d) does not lie inside the atmosphere's %d x %d cells", who,
            x.nx1, x.ny1, x.nxaooc, x.nyaooc, nxta, nyta);
  if (!(p->dxo > 0.0) || !(p->dyo > 0.0)) QG_FAIL("%s: need dxo > 0 and dyo > 0", who);
  const int nxto = x.nxaooc * x.ndxr, nyto = x.nyaooc * x.ndxr;
  std::vector<int> ix, iy;
  std::vector<double> wx, wy;
  if (xf_bilint_tables(who, nxta, nyta, nxto, nyto, atm->prm.dxo, atm->prm.dyo, p->xta, p->yta, p->xto, p->yto, ix, iy, wx, wy))
    return 1;
  HIPCHECK(hipStreamSynchronize(atm->stream));
  auto &h = atm->xf.heat;
  auto &ss = atm->xf.sst;
  ss.on = false; // (until this call has gone through: it replaces the buffers)
  const int ncell = x.nxaooc * x.nyaooc;
  h.nblkL = ((nxta + 63) / 64) * ((nyta + 3) / 4);
  ss.ldt = round_up(nxto, 16);
  if (h.fsa.alloc(nyta, "fsprim of the atmosphere") || h.wx.alloc(2 * (size_t)nxto, "bilint's x weights") ||
      h.wy.alloc(2 * (size_t)nyto, "bilint's y weights") || h.cell.alloc(ncell, "the per-cell sums") ||
      h.part.alloc(3 * (size_t)ncell + h.nblkL, "the heat half's partial sums") || h.scal.alloc(4, "the heat half's results") ||
      h.ix.alloc(2 * (size_t)nxto, "bilint's x indices") || h.iy.alloc(2 * (size_t)nyto, "bilint's y indices") ||
      ss.sst.alloc((size_t)ss.ldt * nyto, "the prescribed SST"))
    return 1;
  HIPCHECK(hipMemcpy(h.fsa, p->fsa, nyta * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.wx, wx.data(), wx.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.wy, wy.data(), wy.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.ix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h.iy, iy.data(), iy.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(ss.sst, 0, (size_t)ss.ldt * nyto * sizeof(double)));
  HIPCHECK(hipMemset(h.scal, 0, 4 * sizeof(double)));
  HIPCHECK(hipDeviceSynchronize());
  if (upload2d(atm, ss.sst, ss.ldt, p->sst, nxto, nyto)) return 1;
  memset(&h.prm, 0, sizeof(h.prm)); // (the constants; no host pointer is kept)
  h.prm.xlamda = p->xlamda; h.prm.D0up = p->D0up; h.prm.Dmup = p->Dmup; h.prm.Dmdown = p->Dmdown; h.prm.Adown11 = p->Adown11;
  h.prm.Bmup = p->Bmup; h.prm.B1down = p->B1down; h.prm.Cmup = p->Cmup; h.prm.C1down = p->C1down;
  h.prm.hmadmp = p->hmadmp; h.prm.hmat = p->hmat;
  ss.dxo = p->dxo;
  ss.dyo = p->dyo;
  ss.on = true;
  return 0;
}

static int launch_xf_heat_sst(qgcm_hip_ctx *atm) {
  QgXfHeatParams P;
  xf_heat_fill(nullptr, atm, P);
  hipStream_t st = atm->stream;
  HIPCHECK(qg_launch_xf_heat_sst(st, P));
  hipLaunchKernelGGL(k_xf_heat_atm, dim3((P.nxta + 63) / 64, (P.nyta + 3) / 4), dim3(OML_NT), 0, st, P);
  hipLaunchKernelGGL(k_xf_heat_final, dim3(1), dim3(OML_NT), 0, st, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_xforc_sst_set(qgcm_hip_handle atm, const double *sst) {
  const char *who = "qgcm_hip_xforc_sst_set";
  if (xf_sst_ready(atm, who)) return 1;
  if (!sst) QG_FAIL("%s: null argument", who);
  const qgcm_hip_xforc_params &x = atm->xf.prm;
  return upload2d(atm, atm->xf.sst.sst, atm->xf.sst.ldt, sst, x.nxaooc * x.ndxr, x.nyaooc * x.ndxr);
}

extern "C" int qgcm_hip_xforc_sst_get(qgcm_hip_handle atm, double *fnetat, double *scal) {
  if (xf_sst_ready(atm, "qgcm_hip_xforc_sst_get")) return 1;
  if (fnetat && download2d(atm, fnetat, atm->tav.fnet, atm->aml.ldt, atm->g.nxt, atm->g.ny - 1)) return 1;
  if (scal) {
    HIPCHECK(hipMemcpyAsync(scal, atm->xf.heat.scal, 4 * sizeof(double), hipMemcpyDeviceToHost, atm->stream));
    HIPCHECK(hipStreamSynchronize(atm->stream));
  }
  return 0;
}

extern "C" int qgcm_hip_coupled_set_xforc(qgcm_hip_handle oc, qgcm_hip_handle atm, int on) {
  if (!on) {
    if (atm) atm->xf.coupled = false;
    return 0;
  }
  if (xf_ready(oc, atm, "qgcm_hip_coupled_set_xforc")) return 1;
  atm->xf.coupled = true;
  return 0;
}

// Coupled run with the forcing held between calls: the main loop of src/q-gcm.F:1220-1268 without xforc / oml / aml.
// The ocean steps of the window are queued on the ocean handle's stream and the atmospheric steps on the
// atmosphere's: with the forcing frozen the two halves do not exchange data inside the window, so the streams need
// no cross dependencies and the GPU overlaps the atmosphere's small kernels with the ocean's.
// Two handles that step side by side on one GPU (qgcm_hip_coupled_steps: the ocean and the atmosphere of a coupled run)
// queue for the same wave slots: the atmosphere's twelve small dependent launches per ocean step then advance only as
// slots of the ocean's chip-filling launches retire (107 us per ocean step at NAtl 5 km, where the ocean alone takes 68
// and the atmosphere's three steps alone 67).  Given disjoint CU ranges (hipExtStreamCreateWithCUMask) each half keeps
// its own pace: 94.6 us with 96 CUs for the atmosphere and 160 for the ocean (profiles/r4_coupled_cu_masks.log).
// The handle's stream is REPLACED (not a second stream beside it: the runtime multiplexes streams onto few hardware
// queues, and masked streams that share one ran four times slower); count = 0 gives the unrestricted stream back.
extern "C" int qgcm_hip_set_cu_range(qgcm_hip_handle c, int first, int count) {
  if (!c) QG_FAIL("qgcm_hip_set_cu_range: null handle");
  if (c->sc_comm) QG_FAIL("qgcm_hip_set_cu_range: not for a handle with a communicator (its exchanges are ordered on the stream it has)");
  int ncu = 0, dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  if (first < 0 || count < 0 || first + count > ncu || ncu > 1024) QG_FAIL("qgcm_hip_set_cu_range: CUs %d..%d outside 0..%d", first, first + count - 1, ncu - 1);
  if (first == c->cu_first && count == c->cu_count) return 0;
  HIPCHECK(hipStreamSynchronize(c->stream));
  drop_graphs(c); // (executable graphs are uploaded to the stream they replay on)
  hipStream_t ns = nullptr;
  if (count > 0) {
    uint32_t mask[32];
    memset(mask, 0, sizeof(mask));
    for (int i = first; i < first + count; ++i) mask[i / 32] |= 1u << (i % 32);
    HIPCHECK(hipExtStreamCreateWithCUMask(&ns, (uint32_t)((ncu + 31) / 32), mask));
  } else
    HIPCHECK(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
  HIPCHECK(hipStreamDestroy(c->stream));
  c->stream = ns;
  c->cu_first = first;
  c->cu_count = count;
  return 0;
}

extern "C" int qgcm_hip_coupled_steps(qgcm_hip_handle oc, qgcm_hip_handle atm, int nt0, int n, int nstr) {
  if (nt0 < 1 || n < 0 || nstr < 1) QG_FAIL("qgcm_hip_coupled_steps: bad step range");
  if (oc && check_ready(oc, "qgcm_hip_coupled_steps")) return 1;
  if (atm && check_atm(atm, "qgcm_hip_coupled_steps")) return 1;
  if (oc && (oc->g.atm || !oc->whole)) QG_FAIL("qgcm_hip_coupled_steps: first handle must be a whole-domain ocean");
  if (oc) oc->beside = atm != nullptr; // (part of the graph key)
  if (atm && atm->xf.coupled) {
    // qgcm_hip_coupled_set_xforc: the reference's order (src/q-gcm.F:1222-1268) - at every nt with mod(nt,nstr) == 1
    // xforc, then the ocean step, then the atmospheric steps up to the next such nt.  The events of qgcm_hip_xforc
    // order the two streams; xforc is launched between the step graphs' replays.
    if (xf_ready(oc, atm, "qgcm_hip_coupled_steps")) return 1;
    const int end = nt0 + n; // one past the last step
    for (int nt = nt0; nt < end;) {
      int next = end;
      if (nstr > 1) {
        if (nt % nstr == 1) {
          if (qgcm_hip_xforc(oc, atm)) return 1;
          if (oc && steps_impl(oc, (nt - 1) / nstr + 1, 1, false)) return 1;
        }
        const int nn = nt + (nstr - (nt - 1) % nstr); // the next nt with mod(nt,nstr) == 1
        if (nn < end) next = nn;
      }
      if (steps_impl(atm, nt, next - nt, false)) return 1;
      nt = next;
    }
    return 0;
  }
  if (oc && n > 0) {
    // ocean steps s with nt = 1 + (s-1)*nstr in [nt0, nt0+n-1]   (mod(nt,nstr) == 1, src/q-gcm.F:1222; nstr = 1 never
    // steps the ocean in the reference - SURVEY 8d caveat - and neither does this)
    if (nstr > 1) {
      const int sfirst = (nt0 - 1 + nstr - 1) / nstr + 1; // smallest s with 1+(s-1)*nstr >= nt0
      const int slast = (nt0 + n - 2) / nstr + 1;         // largest s with 1+(s-1)*nstr <= nt0+n-1
      if (slast >= sfirst && steps_impl(oc, sfirst, slast - sfirst + 1, false)) return 1;
    }
  }
  if (atm && n > 0 && steps_impl(atm, nt0, n, false)) return 1;
  return 0;
}

extern "C" int qgcm_hip_sync(qgcm_hip_handle c) {
  if (!c) QG_FAIL("qgcm_hip_sync: null handle");
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_helmholtz(qgcm_hip_handle c, double *wrk, const double *boc) {
  if (check_ready(c, "qgcm_hip_helmholtz")) return 1;
  if (!wrk || !boc) QG_FAIL("qgcm_hip_helmholtz: null argument");
  if (!c->whole) QG_FAIL("qgcm_hip_helmholtz: only for a handle that owns the whole domain");
  const QgGeom &g = c->g;
  // pivots for this boc (box: boc(i-1) multiplies sine wavenumber i-1, src/ocisubs.F:470-478)
  // a column in segments builds the responses of every segment for THIS diagonal too: the last one's are kept
  auto &ss = c->seg.set[1];
  const bool kept = c->seg.S > 1 && ss.boc.size() == (size_t)g.nk && !memcmp(ss.boc.data(), boc, sizeof(double) * g.nk);
  if (!kept) {
    ss.boc.clear();
    if (build_thomas_tables(c, 1, {std::vector<double>(boc, boc + g.nk)})) return 1;
    ss.boc.assign(boc, boc + g.nk);
  }
  // box: interior columns i=2..nx-1 of every row -> wrk(c = i-2, j); cyclic: columns 1..nxto -> wrk(c = i-1, j)
  const int coff = g.cyc ? 0 : 1;
  HIPCHECK(hipMemcpy2DAsync(c->wrk, (size_t)g.ldw * 8, wrk + coff, (size_t)g.nx * 8, (size_t)g.nk * 8, (size_t)g.ny,
                            hipMemcpyHostToDevice, c->stream));
  if (launch_dst(c, c->wrk, 1, false)) return 1;
  if (launch_thomas(c, 1, 1, 0)) return 1;
  if (launch_dst(c, c->wrk, 1, true)) return 1;
  HIPCHECK(hipMemcpy2DAsync(wrk + coff, (size_t)g.nx * 8, c->wrk, (size_t)g.ldw * 8, (size_t)g.nk * 8, (size_t)g.ny,
                            hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  // box: solid-boundary values are zero (src/ocisubs.F:496-509); cyclic: E = W (:604)
  for (int j = 0; j < g.ny; ++j) {
    if (g.cyc) {
      wrk[(size_t)j * g.nx + g.nx - 1] = wrk[(size_t)j * g.nx];
    } else {
      wrk[(size_t)j * g.nx] = 0.0;
      wrk[(size_t)j * g.nx + g.nx - 1] = 0.0;
    }
  }
  for (int i = 0; i < g.nx; ++i) {
    wrk[i] = 0.0;
    wrk[(size_t)(g.ny - 1) * g.nx + i] = 0.0;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// y-slab building blocks
// ---------------------------------------------------------------------------
extern "C" int qgcm_hip_local_rows(qgcm_hip_handle c, int *nyl, int *joff, int *jlo, int *jhi) {
  if (!c) QG_FAIL("qgcm_hip_local_rows: null handle");
  if (nyl) *nyl = c->g.ny;
  if (joff) *joff = c->g.joff;
  if (jlo) *jlo = c->g.jlo;
  if (jhi) *jhi = c->g.jhi;
  return 0;
}

extern "C" int qgcm_hip_row_transform(qgcm_hip_handle c, int inverse) {
  if (check_ready(c, "qgcm_hip_row_transform")) return 1;
  return launch_dst(c, c->wrk, c->g.nl, inverse != 0);
}

extern "C" int qgcm_hip_wrk_fill(qgcm_hip_handle c, double value) {
  if (check_ready(c, "qgcm_hip_wrk_fill")) return 1;
  const QgGeom &g = c->g;
  HIPCHECK(hipMemsetAsync(c->wrk, 0, sizeof(double) * g.wstride * g.nl, c->stream));
  hipLaunchKernelGGL(k_fill_rows, dim3((g.nk + 255) / 256, g.jr1 - g.jr0 + 1, g.nl), dim3(256), 0, c->stream, c->wrk,
                     g.wstride, g.ldw, g.nk, g.jr0, g.jr1, g.nl, value);
  HIPCHECK(hipGetLastError());
  return 0;
}

// counterpart of qgcm_hip_wrk_get: the rows jr0..jr1 of a (nxpo, nyl, nlo) host block into the work array (box: the
// interior columns 2..nxpo-1; cyclic: columns 1..nxto), everything else of the work array zero
extern "C" int qgcm_hip_wrk_set(qgcm_hip_handle c, const double *wrk) {
  if (check_ready(c, "qgcm_hip_wrk_set")) return 1;
  if (!wrk) QG_FAIL("qgcm_hip_wrk_set: null argument");
  const QgGeom &g = c->g;
  HIPCHECK(hipMemsetAsync(c->wrk, 0, sizeof(double) * g.wstride * g.nl, c->stream));
  const int coff = g.cyc ? 0 : 1;
  for (int m = 0; m < g.nl; ++m)
    HIPCHECK(hipMemcpy2DAsync(c->wrk + g.wstride * m + (size_t)(g.jr0 - 1) * g.ldw, (size_t)g.ldw * 8,
                              wrk + (size_t)g.nx * g.ny * m + (size_t)(g.jr0 - 1) * g.nx + coff, (size_t)g.nx * 8, (size_t)g.nk * 8,
                              (size_t)(g.jr1 - g.jr0 + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_wrk_get(qgcm_hip_handle c, double *wrk) {
  if (check_ready(c, "qgcm_hip_wrk_get")) return 1;
  if (!wrk) QG_FAIL("qgcm_hip_wrk_get: null argument");
  const QgGeom &g = c->g;
  memset(wrk, 0, sizeof(double) * (size_t)g.nx * g.ny * g.nl);
  const int coff = g.cyc ? 0 : 1;
  for (int m = 0; m < g.nl; ++m)
    HIPCHECK(hipMemcpy2DAsync(wrk + (size_t)g.nx * g.ny * m + (size_t)(g.jr0 - 1) * g.nx + coff, (size_t)g.nx * 8,
                              c->wrk + g.wstride * m + (size_t)(g.jr0 - 1) * g.ldw, (size_t)g.ldw * 8, (size_t)g.nk * 8,
                              (size_t)(g.jr1 - g.jr0 + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (g.cyc)
    for (int m = 0; m < g.nl; ++m)
      for (int j = 0; j < g.ny; ++j) wrk[((size_t)m * g.ny + j) * g.nx + g.nx - 1] = wrk[((size_t)m * g.ny + j) * g.nx];
  return 0;
}

extern "C" int qgcm_hip_area_integrals(qgcm_hip_handle c, double *xin) {
  if (check_ready(c, "qgcm_hip_area_integrals")) return 1;
  if (!xin) QG_FAIL("qgcm_hip_area_integrals: null argument");
  if (c->g.cyc) QG_FAIL("qgcm_hip_area_integrals: box ocean only (spectral area integrals of the sine series)");
  QgConstrParams P;
  fill_constr_params(c, P);
#define QG_XIN(NLV) hipLaunchKernelGGL((k_xin_only<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(c->g.nl, QG_XIN, "k_xin_only");
#undef QG_XIN
  HIPCHECK(hipGetLastError());
  return qgcm_hip_get_inv_diag(c, xin, nullptr);
}

extern "C" int qgcm_hip_thomas_msg_len(qgcm_hip_handle c) { return c ? (int)slab_msg_len_oml(c) : 0; }
extern "C" int qgcm_hip_oml_msg_len(qgcm_hip_handle c) { return c ? 3 : 0; }

extern "C" int qgcm_hip_thomas_const_len(qgcm_hip_handle c) { return c ? TH_CST * c->g.nl * c->g.ldw : 0; }

extern "C" int qgcm_hip_thomas_consts(qgcm_hip_handle c, double *dst_dev) {
  if (check_ready(c, "qgcm_hip_thomas_consts")) return 1;
  if (!dst_dev) QG_FAIL("qgcm_hip_thomas_consts: null buffer");
  HIPCHECK(hipMemcpyAsync(dst_dev, c->slabDE, sizeof(double) * TH_CST * c->g.nl * c->g.ldw, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

extern "C" int qgcm_hip_set_thomas_consts(qgcm_hip_handle c, const double *gath_dev, int nranks) {
  if (check_ready(c, "qgcm_hip_set_thomas_consts")) return 1;
  if (!gath_dev || nranks < 1 || nranks > 64) QG_FAIL("qgcm_hip_set_thomas_consts: bad argument");
  const size_t n = (size_t)TH_CST * c->g.nl * c->g.ldw * nranks;
  drop_graphs(c);
  if (c->th_cgath_ranks != nranks) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    c->th_cgath_ranks = 0;
    if (c->th_cgath.alloc(n, "all ranks' slab constants")) return 1;
    c->th_cgath_ranks = nranks;
  }
  HIPCHECK(hipMemcpyAsync(c->th_cgath, gath_dev, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

extern "C" int qgcm_hip_thomas_phase(qgcm_hip_handle c, int phase, const double *gath_dev, double *send_dev, int rank,
                                     int nranks) {
  if (check_ready(c, "qgcm_hip_thomas_phase")) return 1;
  if (phase < 1 || phase > 2) QG_FAIL("qgcm_hip_thomas_phase: phase must be 1 or 2");
  if ((phase == 1 && !send_dev) || (phase == 2 && !gath_dev)) QG_FAIL("qgcm_hip_thomas_phase: missing buffer");
  if (nranks > 64) QG_FAIL("qgcm_hip_thomas_phase: at most 64 slabs");
  return launch_thomas(c, 0, c->g.nl, phase, {gath_dev, send_dev, rank, nranks});
}

extern "C" int qgcm_hip_constr(qgcm_hip_handle c) {
  if (check_ready(c, "qgcm_hip_constr")) return 1;
  if (!c->homog_set) QG_FAIL("qgcm_hip_constr: homogeneous solutions not set");
  return launch_constr(c);
}

extern "C" int qgcm_hip_unpack(qgcm_hip_handle c, int fuse_ocqbdy) {
  if (check_ready(c, "qgcm_hip_unpack")) return 1;
  if (launch_unpack(c, fuse_ocqbdy != 0)) return 1;
  c->ip ^= 1;
  return 0;
}

extern "C" int qgcm_hip_halo_msg_len(qgcm_hip_handle c) { return c ? (int)halo_msg_len(c) : 0; }

extern "C" int qgcm_hip_halo_pack(qgcm_hip_handle c, double *to_lower_dev, double *to_upper_dev) {
  if (check_ready(c, "qgcm_hip_halo_pack")) return 1;
  const QgGeom &g = c->g;
  dim3 grid((g.ldx + 255) / 256, 4 * g.nl, 2);
  hipLaunchKernelGGL(k_halo_pack, grid, dim3(256), 0, c->stream, g, (const double *)c->p[c->ip],
                     (const double *)c->q[c->iq], to_lower_dev, to_upper_dev);
  HIPCHECK(hipGetLastError());
  return 0;
}

// st (here and below): the stream of the launches, nullptr = the handle's
static int launch_halo_unpack(qgcm_hip_ctx *c, const double *from_lo, const double *from_hi, hipStream_t st = nullptr) {
  if (check_ready(c, "qgcm_hip_halo_unpack")) return 1;
  const QgGeom &g = c->g;
  if ((from_lo && g.jlo < 4) || (from_hi && g.ny - g.jhi < 3)) QG_FAIL("qgcm_hip_halo_unpack: no halo rows on that side");
  dim3 grid((g.ldx + 255) / 256, 4 * g.nl, 2);
  hipLaunchKernelGGL(k_halo_unpack, grid, dim3(256), 0, st ? st : c->stream, g, c->p[c->ip], c->q[c->iq], from_lo, from_hi);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_halo_unpack(qgcm_hip_handle c, const double *from_lo, const double *from_hi) { return launch_halo_unpack(c, from_lo, from_hi); }

// edge rows of the new sst, appended to the halo messages: the first / last three owned T rows out (to_lo / to_hi), or
// the neighbours' rows in (from_lo / from_hi)
static int launch_oml_halo(qgcm_hip_ctx *c, double *to_lo, double *to_hi, const double *from_lo, const double *from_hi, hipStream_t st = nullptr) {
  if (!c->oml.on || (!to_lo && !to_hi && !from_lo && !from_hi)) return 0;
  const size_t off = (size_t)4 * c->g.nl * c->g.ldx;
  const int jT1 = (c->g.jhi + c->g.joff == c->g.nyg) ? c->g.jhi - 1 : c->g.jhi;
  hipLaunchKernelGGL(k_oml_halo, dim3((c->g.nxt + 255) / 256, 3, 2), dim3(256), 0, st ? st : c->stream, c->oml.sst[c->oml.is],
                     c->oml.ldt, c->g.nxt, c->g.ny - 1, c->g.jlo, jT1, to_lo ? to_lo + off : nullptr, to_hi ? to_hi + off : nullptr,
                     from_lo ? from_lo + off : nullptr, from_hi ? from_hi + off : nullptr, from_lo || from_hi ? 1 : 0);
  HIPCHECK(hipGetLastError());
  return 0;
}

// The communication-free pieces of a y-slab step: qgcm_hip_slab_stage runs them by stage number (the Python driver
// SlabOcean.step), slab_step calls them between its exchanges.  First the tendency tiles of a slab: all of them, or the
// inner / the outer tile rows (launch_tend's part); send: the step message (cyclic: the boundary line sums go into its tail)
static int slab_tend(qgcm_hip_ctx *c, int part, double *send, hipStream_t st = nullptr) {
  // box fast path: as in qgcm_hip_steps the leapfrog of dpioc is done by the tendency launch and the constraint
  // solve by the extra wave of the fused inverse-transform kernel of slab_solve_unpack (no k_constr_box launch)
  // (with the mixed layer on, xon(1) is only complete after the all-gather: dpioc is stepped in slab_solve_unpack then)
  const bool upd_dpi = step_plan(c, true, true).upd_dpi;
  double *bpart = c->g.cyc && part != TEND_INNER ? send + (size_t)TH_MSG * c->g.nl * c->g.ldw : nullptr;
  return launch_tend(c, upd_dpi, false, part, false, bpart, st);
}

// forward rows and the slab summary of the two y sweeps into the step message (after all the tendency tiles)
static int slab_forward(qgcm_hip_ctx *c, double *send, int rank, int nranks) {
  c->iq ^= 1; // as qgcm_hip_qgostep
  if (qgcm_hip_row_transform(c, 0) || qgcm_hip_thomas_phase(c, 1, nullptr, send, rank, nranks)) return 1;
  if (c->oml.on) { // the three sums of this slab's entoc pass (launch_oml_b) ride at the end of the step message
    QgOmlParams OP;
    fill_oml_params(c, OP);
    hipLaunchKernelGGL(k_oml_sum3, dim3(1), dim3(OML_NT), 0, c->stream, (const double *)OP.partB, OP.nblkB, send + slab_msg_len(c->g));
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

// both sweeps from the gathered step messages, constraints, inverse rows, modes -> layers + boundary PV; the unpack
// launch, fused or not, also writes the halo messages (first / last three owned rows of po, edge row of qo)
static int slab_solve_unpack(qgcm_hip_ctx *c, double *gath, double *to_lo, double *to_hi, int rank, int nranks) {
  if (qgcm_hip_thomas_phase(c, 2, gath, nullptr, rank, nranks)) return 1;
  if (c->oml.on) { // xon(1), enisoc(1) / eninoc(1), monitors from every rank's sums, before the constraints use them
    if (!c->oml_gath) QG_FAIL("qgcm_hip_slab_stage: the mixed layer's stages 10 / 11 have not run this step");
    QgOmlFinal F;
    fill_oml_final(c, F, true);
    hipLaunchKernelGGL(k_oml_final_slab, dim3(1), dim3(64), 0, c->stream, c->oml_gath, (const double *)(gath + slab_msg_len(c->g)),
                       (long)slab_msg_len_oml(c), nranks, F);
    HIPCHECK(hipGetLastError());
  }
  const QgStepPlan pl = step_plan(c, true, true);
  if (nranks == 1) to_lo = to_hi = nullptr;
  if (pl.constr == CONSTR_OWN && qgcm_hip_constr(c)) return 1; // area integrals of the whole basin came with the slab summaries
  if (launch_inverse(c, pl, true, to_lo, to_hi, false, false)) return 1;
  c->ip ^= 1;
  if (launch_poavg(c)) return 1; // the new po of the owned rows, before slab_halo_in averages it
  return launch_oml_halo(c, to_lo, to_hi, nullptr, nullptr);
}

// the neighbours' edge rows in (with the mixed layer on, those of the new sst sit at the end of the halo messages),
// then the leapfrog averaging where the step ends with one (always on the handle's stream)
static int slab_halo_in(qgcm_hip_ctx *c, const double *from_lo, const double *from_hi, int nranks, bool avg, hipStream_t st = nullptr) {
  if (nranks > 1 && (launch_halo_unpack(c, from_lo, from_hi, st) || launch_oml_halo(c, nullptr, nullptr, from_lo, from_hi, st))) return 1;
  return avg ? qgcm_hip_lf_average(c) : 0;
}

// Stages 4 - 7 are stage 1 in pieces: 4 = the inner tile rows of the tendency launch (they need no halo row), 6 = the
// outer tile rows + edge work, 7 = forward rows and summary sweep (after 4 AND 6), 5 = 6 + 7.
extern "C" int qgcm_hip_slab_stage(qgcm_hip_handle c, int stage, double *a, double *b, double *cc, int rank, int nranks,
                                   int flags) {
  switch (stage) {
    case 1: case 4: case 5: case 6: case 7:
      if (stage != 4 && !a) QG_FAIL("qgcm_hip_slab_stage: stage %d needs the send buffer", stage);
      if (check_ready(c, "qgcm_hip_slab_stage")) return 1;
      if (stage != 1 && (c->oml.on || !tend_can_split(c)))
        QG_FAIL("qgcm_hip_slab_stage: stages 4 - 7 need a slab of at least three tile rows (%d rows each) and the mixed layer off", TEND_TY);
      if (!c->homog_set) QG_FAIL("qgcm_hip_slab_stage: homogeneous solutions not set");
      if (stage != 7 && slab_tend(c, stage == 1 ? TEND_ALL : stage == 4 ? TEND_INNER : TEND_OUTER, a)) return 1;
      return stage == 4 || stage == 6 ? 0 : slab_forward(c, a, rank, nranks);
    case 2: return slab_solve_unpack(c, a, b, cc, rank, nranks); // a = the gathered step messages, b / cc = the halo messages out
    case 3: return slab_halo_in(c, a, b, nranks, (flags & 1) != 0); // a / b = the halo messages in; flags & 1: leapfrog averaging
    // ---- ocean mixed layer on y-slabs: `call oml` (src/q-gcm.F:1232) comes before qgostep and needs the basin-wide
    // mean entrainment half way through - one more (three numbers per rank) all-gather per step
    case 10: // new sst, raw entrainment; a = this slab's three sums (send buffer of the mixed layer's all-gather)
      if (oml_ready(c, "qgcm_hip_slab_stage")) return 1;
      if (!a) QG_FAIL("qgcm_hip_slab_stage: stage 10 needs the send buffer");
      return launch_oml_a(c, a);
    case 11: // a = the gathered sums (3, nranks): entoc, rotation of the sst buffers
      if (oml_ready(c, "qgcm_hip_slab_stage")) return 1;
      if (!a) QG_FAIL("qgcm_hip_slab_stage: stage 11 needs the gathered sums");
      c->oml_gath = a;
      return launch_oml_b(c, a, nranks);
    default: QG_FAIL("qgcm_hip_slab_stage: stage must be 1..7, 10 or 11");
  }
}

// ---------------------------------------------------------------------------
// y-slab steps with the exchanges issued from here (RCCL on the library's stream)
// ---------------------------------------------------------------------------
#define NCCLCHECK(m, expr)                                                                           \
  do {                                                                                               \
    ncclResult_t r_ = (expr);                                                                        \
    if (r_ != ncclSuccess) QG_FAIL("%s failed: %s (%s:%d)", #expr, (m)->GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

extern "C" int qgcm_hip_comm_unique_id(char *id, int nbytes) {
  if (!id || nbytes < (int)sizeof(ncclUniqueId)) QG_FAIL("qgcm_hip_comm_unique_id: need a buffer of %d bytes", (int)sizeof(ncclUniqueId));
  QgRccl *api = qg_rccl(g_err, sizeof(g_err));
  if (!api) return 1;
  ncclUniqueId u;
  NCCLCHECK(api, api->GetUniqueId(&u));
  memcpy(id, &u, sizeof(u));
  return 0;
}

extern "C" int qgcm_hip_comm_init(qgcm_hip_handle c, const char *id, int nbytes, int rank, int nranks) {
  if (check_ready(c, "qgcm_hip_comm_init")) return 1;
  if (!id || nbytes < (int)sizeof(ncclUniqueId)) QG_FAIL("qgcm_hip_comm_init: need the %d-byte id of qgcm_hip_comm_unique_id", (int)sizeof(ncclUniqueId));
  if (nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks) QG_FAIL("qgcm_hip_comm_init: bad rank %d of %d (at most 64 slabs)", rank, nranks);
  if (c->sc_comm) QG_FAIL("qgcm_hip_comm_init: this handle already has a communicator");
  const QgGeom &g = c->g;
  // the slab must be the rank-th piece of the basin: first rank owns global row 1, last rank row nyg
  if ((rank == 0) != (g.joff + g.jlo == 1) || (rank == nranks - 1) != (g.joff + g.jhi == g.nyg))
    QG_FAIL("qgcm_hip_comm_init: slab rows %d..%d of %d do not fit rank %d of %d", g.joff + g.jlo, g.joff + g.jhi, g.nyg, rank, nranks);
  QgRccl *api = qg_rccl(g_err, sizeof(g_err));
  if (!api) return 1;
  HIPCHECK(hipSetDevice(c->device));
  std::unique_ptr<QgSlabComm> m(new QgSlabComm); // (a failure below leaves the handle without a communicator)
  m->api = api;
  m->rank = rank;
  m->nranks = nranks;
  const char *hp = getenv("QGCM_HIP_HALO_P2P");
  m->halo_p2p = hp ? atoi(hp) != 0 : true; // default: the two neighbours only (an all-gather moves nranks x the bytes)
  m->th_len = slab_msg_len_oml(c);
  m->halo_len = halo_msg_len(c);
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  NCCLCHECK(api, api->CommInitRank(&m->comm, nranks, u, rank));
  struct { QgDbl *buf; size_t n; } bufs[] = {{&m->th_send, m->th_len}, {&m->th_gath, m->th_len * nranks},
                                             {&m->h_send, 2 * m->halo_len}, {&m->h_gath, 2 * m->halo_len * nranks},
                                             {&m->oml_send, 4}, {&m->oml_gath, (size_t)4 * nranks}};
  for (auto &b : bufs)
    if (b.buf->alloc(b.n, "an exchange buffer")) return 1;
  // the right-hand-side independent part of the slab summaries (D, E, SP, SQ) is exchanged once
  if (nranks > 1) {
    const size_t nc = (size_t)TH_CST * g.nl * g.ldw;
    c->th_cgath_ranks = 0;
    if (c->th_cgath.alloc(nc * nranks, "all ranks' slab constants")) return 1;
    c->th_cgath_ranks = nranks;
    NCCLCHECK(api, api->AllGather(c->slabDE, c->th_cgath, nc, ncclDouble, m->comm, c->stream));
  }
  HIPCHECK(hipStreamSynchronize(c->stream));
  const char *gm = getenv("QGCM_HIP_SLAB_GRAPH");
  c->slab_graph_mode = gm && atoi(gm) != 0;
  c->sc_comm = m.release(); // owned by the handle from here on (~qgcm_hip_ctx)
  return 0;
}

extern "C" int qgcm_hip_comm_set_halo_p2p(qgcm_hip_handle c, int on) {
  if (!c || !c->sc_comm) QG_FAIL("qgcm_hip_comm_set_halo_p2p: no communicator (qgcm_hip_comm_init)");
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (c->sc_comm->halo_p2p != (on != 0)) drop_graphs(c); // captured steps contain the old exchange
  c->sc_comm->halo_p2p = (on != 0);
  return 0;
}

// Halo exchange of step s overlapped with the inner tile rows of step s+1's tendency launch: the exchange and the halo
// unpack go to a second stream; the handle's stream runs k_tend's inner tile rows (stage 4), waits for the halo rows,
// and goes on with the outer tile rows (stage 5).  Same results, bit for bit.  Not with the mixed layer on (its first
// stage needs the neighbours' sst rows), not across a leapfrog averaging, not for slabs of fewer than three tile rows:
// those steps keep the plain order.
extern "C" int qgcm_hip_comm_set_overlap(qgcm_hip_handle c, int on) {
  if (!c || !c->sc_comm) QG_FAIL("qgcm_hip_comm_set_overlap: no communicator (qgcm_hip_comm_init)");
  QgSlabComm *m = c->sc_comm;
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (m->overlap != (on != 0)) drop_graphs(c); // captured steps contain the old order
  if (on && !m->cstream) {
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamCreateWithFlags(&m->cstream, hipStreamNonBlocking));
    HIPCHECK(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&m->ev_halo, hipEventDisableTiming));
  }
  m->overlap = (on != 0);
  return 0;
}

// Measurement aid: the step's collectives issued back to back on the handle's stream, HIP-event timed
// (collective over all ranks). us[0] = all-gather of the slab summaries, us[1] = halo rows as one all-gather,
// us[2] = halo rows as grouped send/recv with the two neighbours.
extern "C" int qgcm_hip_comm_probe(qgcm_hip_handle c, int reps, double *us) {
  if (!c || !c->sc_comm) QG_FAIL("qgcm_hip_comm_probe: no communicator (qgcm_hip_comm_init)");
  if (!us || reps < 1) QG_FAIL("qgcm_hip_comm_probe: bad argument");
  QgSlabComm *m = c->sc_comm;
  const int r = m->rank, P = m->nranks;
  const size_t n = m->halo_len;
  QgEventPair ev;
  if (ev.create()) return 1;
  const hipEvent_t a = ev.a, b = ev.b;
  for (int which = 0; which < 3; ++which) {
    for (int pass = 0; pass < 2; ++pass) { // pass 0 warms the algorithm / channel set-up
      const int nrep = pass ? reps : 3;
      HIPCHECK(hipEventRecord(a, c->stream));
      for (int i = 0; i < nrep; ++i) {
        if (which == 0) {
          NCCLCHECK(m->api, m->api->AllGather(m->th_send, m->th_gath, m->th_len, ncclDouble, m->comm, c->stream));
        } else if (which == 1) {
          NCCLCHECK(m->api, m->api->AllGather(m->h_send, m->h_gath, 2 * n, ncclDouble, m->comm, c->stream));
        } else if (P > 1) {
          double *rl = m->h_gath + (size_t)(2 * (r > 0 ? r - 1 : 0) + 1) * n, *rh = m->h_gath + (size_t)(2 * (r < P - 1 ? r + 1 : 0)) * n;
          NCCLCHECK(m->api, m->api->GroupStart());
          if (r > 0) {
            NCCLCHECK(m->api, m->api->Send(m->h_send, n, ncclDouble, r - 1, m->comm, c->stream));
            NCCLCHECK(m->api, m->api->Recv(rl, n, ncclDouble, r - 1, m->comm, c->stream));
          }
          if (r < P - 1) {
            NCCLCHECK(m->api, m->api->Send(m->h_send + n, n, ncclDouble, r + 1, m->comm, c->stream));
            NCCLCHECK(m->api, m->api->Recv(rh, n, ncclDouble, r + 1, m->comm, c->stream));
          }
          NCCLCHECK(m->api, m->api->GroupEnd());
        }
      }
      HIPCHECK(hipEventRecord(b, c->stream));
      HIPCHECK(hipEventSynchronize(b));
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, a, b));
      if (pass) us[which] = 1e3 * ms / nrep;
    }
  }
  return 0;
}

// The edge rows of a step to both neighbours, on stream xs: grouped send/recv with the neighbours alone (p2p; the
// receive areas are the neighbour's slots of h_gath, as with the all-gather) or one all-gather of every rank's pair.
static int slab_halo_exchange(QgSlabComm *m, bool p2p, hipStream_t xs) {
  const int r = m->rank, P = m->nranks;
  const size_t n = m->halo_len;
  if (!p2p) {
    NCCLCHECK(m->api, m->api->AllGather(m->h_send, m->h_gath, 2 * n, ncclDouble, m->comm, xs));
    return 0;
  }
  double *to_lo = m->h_send, *to_hi = m->h_send + n;
  double *rl = m->h_gath + (size_t)(2 * (r > 0 ? r - 1 : 0) + 1) * n, *rh = m->h_gath + (size_t)(2 * (r < P - 1 ? r + 1 : 0)) * n;
  NCCLCHECK(m->api, m->api->GroupStart());
  if (r > 0) {
    NCCLCHECK(m->api, m->api->Send(to_lo, n, ncclDouble, r - 1, m->comm, xs));
    NCCLCHECK(m->api, m->api->Recv(rl, n, ncclDouble, r - 1, m->comm, xs));
  }
  if (r < P - 1) {
    NCCLCHECK(m->api, m->api->Send(to_hi, n, ncclDouble, r + 1, m->comm, xs));
    NCCLCHECK(m->api, m->api->Recv(rh, n, ncclDouble, r + 1, m->comm, xs));
  }
  NCCLCHECK(m->api, m->api->GroupEnd());
  return 0;
}

// where the neighbours' edge rows lie after either exchange (nullptr towards a wall)
static void slab_halo_from(QgSlabComm *m, const double *&from_lo, const double *&from_hi) {
  const int r = m->rank, P = m->nranks;
  const size_t n = m->halo_len;
  from_lo = r > 0 ? m->h_gath + (size_t)(2 * (r - 1) + 1) * n : nullptr; // what the lower neighbour sent upwards
  from_hi = r < P - 1 ? m->h_gath + (size_t)(2 * (r + 1)) * n : nullptr; // what the upper neighbour sent downwards
}

// one distributed ocean step: the communication-free pieces above (what SlabOcean.step runs through
// qgcm_hip_slab_stage) and two exchanges, all ordered on c->stream; no host synchronisation
// next_follows: step s + 1 is executed by the same qgcm_hip_slab_steps call / captured block (its tendency may be started);
// forked: set once this step has sent work to the exchange's stream (slab_step joins it if the step fails)
static int slab_step_issue(qgcm_hip_ctx *c, int s, bool next_follows, bool &forked) {
  QgSlabComm *m = c->sc_comm;
  const int r = m->rank, P = m->nranks;
  const size_t n = m->halo_len;
  if (m->th_len != slab_msg_len_oml(c) || n != halo_msg_len(c))
    QG_FAIL("qgcm_hip_slab_steps: the mixed layer was switched on after qgcm_hip_comm_init (message sizes differ)");
  // 0. mixed layer (`call oml` precedes qgostep): new sst + raw entrainment, every slab's sums, entoc
  if (c->oml.on) {
    if (launch_oml_a(c, m->oml_send)) return 1;
    NCCLCHECK(m->api, m->api->AllGather(m->oml_send, m->oml_gath, 3, ncclDouble, m->comm, c->stream));
    c->oml_gath = m->oml_gath; // (slab_solve_unpack reads it)
    if (launch_oml_b(c, m->oml_gath, P)) return 1;
  }
  // 1. tendency, forward row transform, slab summary of the two y sweeps
  if (m->pending) {
    // the halo rows of the previous step are still on their way (second stream): inner tile rows first
    if (slab_tend(c, TEND_INNER, nullptr)) return 1;
    HIPCHECK(hipStreamWaitEvent(c->stream, m->ev_halo, 0));
    m->pending = false;
    // the outer tile rows have run on the exchange's stream right behind the halo rows, beside the inner ones (below)
    if (!m->outer_done && slab_tend(c, TEND_OUTER, m->th_send)) return 1;
    m->outer_done = false;
  } else if (slab_tend(c, TEND_ALL, m->th_send)) return 1;
  if (slab_forward(c, m->th_send, r, P)) return 1;
  NCCLCHECK(m->api, m->api->AllGather(m->th_send, m->th_gath, m->th_len, ncclDouble, m->comm, c->stream));
  // 2. both sweeps from the composed inflows (+ basin-wide area integrals), constraints, inverse row transform,
  //    modes -> layers + boundary PV, edge rows out
  double *to_lo = r > 0 ? m->h_send : nullptr, *to_hi = r < P - 1 ? m->h_send + n : nullptr;
  if (slab_solve_unpack(c, m->th_gath, to_lo, to_hi, r, P)) return 1;
  const bool avg = avg_after(c, s);
  // overlapped: the exchange and the halo unpack on the second stream; the next step's inner tile rows do not wait for them
  const bool ov = m->overlap && !avg && !c->oml.on && tend_can_split(c);
  hipStream_t xs = c->stream;
  if (ov) {
    HIPCHECK(hipEventRecord(m->ev_fork, c->stream));
    forked = true;
    HIPCHECK(hipStreamWaitEvent(m->cstream, m->ev_fork, 0));
    xs = m->cstream;
  }
  const double *from_lo = nullptr, *from_hi = nullptr;
  if (P > 1 || ov) { // (one rank, overlapped: the all-gather is a local copy - it keeps the one-GPU tests on this path)
    if (slab_halo_exchange(m, m->halo_p2p && P > 1, xs)) return 1;
    slab_halo_from(m, from_lo, from_hi);
  }
  // 3. edge rows in, behind the exchange on its stream (+ leapfrog averaging: never overlapped, xs is the handle's stream)
  if ((P > 1 || avg) && slab_halo_in(c, from_lo, from_hi, P, avg, xs)) return 1;
  if (ov) {
    // The outer tile rows of step s + 1's tendency launch go out on the exchange's stream, right behind the halo rows
    // they need: they run BESIDE the inner tile rows the handle's stream is computing (disjoint tiles of the same
    // launch) instead of as a launch of their own after them - which cost a whole extra single-generation kernel per
    // step (round 3: +23 us on one rank).  Only when step s + 1 belongs to this call: a caller that stops here may
    // read the state, and the outer rows write into the buffer that holds qom.
    m->outer_done = false;
    if (next_follows) {
      if (slab_tend(c, TEND_OUTER, m->th_send, xs)) return 1;
      m->outer_done = true;
    }
    HIPCHECK(hipEventRecord(m->ev_halo, m->cstream));
    m->pending = true;
  }
  return 0;
}

// The one exit of a step.  A step that fails leaves nothing forked and no overlap state behind: the handle's stream
// waits for what the exchange's stream was given, by this step or (still pending) by the one before.
static int slab_step(qgcm_hip_ctx *c, int s, bool next_follows) {
  QgSlabComm *m = c->sc_comm;
  bool forked = false;
  if (!slab_step_issue(c, s, next_follows, forked)) return 0;
  if (forked && !m->pending) (void)hipEventRecord(m->ev_halo, m->cstream); // (failed before the step recorded it)
  if (forked || m->pending) (void)hipStreamWaitEvent(c->stream, m->ev_halo, 0);
  m->pending = m->outer_done = false;
  return 1;
}

// the second stream joins the handle's stream (end of a qgcm_hip_slab_steps call, end of a captured block)
static int slab_join(qgcm_hip_ctx *c) {
  QgSlabComm *m = c->sc_comm;
  if (m && m->pending) {
    m->pending = false;
    HIPCHECK(hipStreamWaitEvent(c->stream, m->ev_halo, 0));
  }
  return 0;
}

static int get_slab_graph(qgcm_hip_ctx *c, int s0, hipGraphExec_t *out) {
  const long long key = graph_key(c, s0, kGraphBlock); // (no eviction here, and 50-step blocks only)
  auto it = c->slab_graphs.find(key);
  if (it != c->slab_graphs.end()) {
    *out = it->second;
    return 0;
  }
  hipGraphExec_t exec;
  if (capture_block(c, false, &exec, [&]() {
        int rc = 0;
        for (int k = 0; k < kGraphBlock && !rc; ++k) rc = slab_step(c, s0 + k, k + 1 < kGraphBlock);
        return rc ? rc : slab_join(c);
      }))
    return 1;
  c->slab_graphs[key] = exec;
  *out = exec;
  return 0;
}

extern "C" int qgcm_hip_slab_steps(qgcm_hip_handle c, int s0, int n) {
  if (check_ready(c, "qgcm_hip_slab_steps")) return 1;
  if (!c->sc_comm) QG_FAIL("qgcm_hip_slab_steps: no communicator (qgcm_hip_comm_init)");
  if (!c->homog_set) QG_FAIL("qgcm_hip_slab_steps: homogeneous solutions not set");
  if (s0 < 1 || n < 0) QG_FAIL("qgcm_hip_slab_steps: bad step range");
  int s = s0;
  while (c->slab_graph_mode && n >= kGraphBlock) {
    hipGraphExec_t ge;
    if (get_slab_graph(c, s, &ge)) return 1;
    HIPCHECK(hipGraphLaunch(ge, c->stream));
    if (c->poavg.on) c->poavg.n += kGraphBlock;
    ml_rotate(c, kGraphBlock); // the p and q rotations are back where they started, sst has moved on
    s += kGraphBlock; // 50 steps: both rotations are back where they started
    n -= kGraphBlock;
  }
  for (; n > 0; --n, ++s)
    if (slab_step(c, s, n > 1)) return 1;
  return slab_join(c);
}

// ---------------------------------------------------------------------------
// the coupled window on a y-slab ocean: SlabOcean.coupled_steps with the library as the driver
// ---------------------------------------------------------------------------
static const char *const kCplNames[QGCM_HIP_CPL_NCODES] = {
    "", "xforc_edge_pack", "gather_edge", "xforc_edge_assemble", "xforc_pom_pack", "gather_pom", "xforc_pom_assemble",
    "xforc_part", "gather_xforc", "xforc_combine", "oml_a", "gather_oml", "oml_b", "stage1", "gather_summary", "stage2",
    "halo_gather", "halo_p2p", "stage3", "stage3_avg", "atm_step"};

extern "C" const char *qgcm_hip_slab_coupled_code_name(int code) {
  return code > 0 && code < QGCM_HIP_CPL_NCODES ? kCplNames[code] : "";
}

// The window's order, once: host code without a handle.  `emit` receives every operation in turn.
template <class Emit>
static int cpl_plan(const char *who, const qgcm_hip_slab_coupled_switches &sw, int nranks, int nt0, int n, int nstr, int xforc,
                    Emit emit) {
  if (nt0 < 1 || n < 0 || nstr < 1) QG_FAIL("%s: bad step range", who);
  if (nranks < 1) QG_FAIL("%s: nranks = %d, need at least one rank", who, nranks);
  if (sw.udiff_sums && (sw.bands || sw.udiff_gather))
    QG_FAIL("%s: udiff_sums excludes bands and udiff_gather (qgcm_hip_xforc_slab_sums)", who);
  const bool xf_gather = sw.heat || sw.bands || sw.udiff_sums; // (replicated, momentum half alone: nothing to exchange)
  struct { bool used; long len; const char *what; } need[] = {
      {xforc && xf_gather, sw.xforc_len, "xforc_len"},    {xforc && sw.udiff_gather, sw.pom_len, "pom_len"},
      {xforc && sw.udiff_sums, sw.edge_len, "edge_len"}, {sw.oml != 0, sw.oml_len, "oml_len"},
      {true, sw.summary_len, "summary_len"},             {nranks > 1, sw.halo_len, "halo_len"}};
  for (const auto &q : need)
    if (q.used && q.len < 1) QG_FAIL("%s: %s = %ld, but the window exchanges that message", who, q.what, q.len);
  const int ocean_avg_period = 25; // the leapfrog averaging of an ocean handle (qgcm_hip_ctx::avg_period)
  const int end = nt0 + n;         // one past the last step
  for (int nt = nt0; nt < end;) {
    int next = end;
    if (nstr > 1) { // (nstr = 1 never steps the ocean in the reference)
      if (nt % nstr == 1) {
        if (xforc) { // `call xforc`, in the mode set up (SlabOcean.xforc)
          if (sw.udiff_sums) { // the 4 rows beyond each seam onto the neighbours first
            emit(QGCM_HIP_CPL_XF_EDGE_PACK, 0L);
            emit(QGCM_HIP_CPL_GATHER_EDGE, sw.edge_len);
            emit(QGCM_HIP_CPL_XF_EDGE_ASSEMBLE, 0L);
          }
          if (sw.udiff_gather) { // the basin's pom(:,:,1) onto every rank first
            emit(QGCM_HIP_CPL_XF_POM_PACK, 0L);
            emit(QGCM_HIP_CPL_GATHER_POM, sw.pom_len);
            emit(QGCM_HIP_CPL_XF_POM_ASSEMBLE, 0L);
          }
          emit(QGCM_HIP_CPL_XF_PART, 0L);
          if (xf_gather) {
            emit(QGCM_HIP_CPL_GATHER_XFORC, sw.xforc_len);
            emit(QGCM_HIP_CPL_XF_COMBINE, 0L);
          }
        }
        const int s = (nt - 1) / nstr + 1; // the ocean step
        if (sw.oml) {                      // `call oml` precedes qgostep (src/q-gcm.F:1232)
          emit(QGCM_HIP_CPL_OML_A, 0L);
          emit(QGCM_HIP_CPL_GATHER_OML, sw.oml_len);
          emit(QGCM_HIP_CPL_OML_B, 0L);
        }
        emit(QGCM_HIP_CPL_STAGE1, 0L);
        emit(QGCM_HIP_CPL_GATHER_SUMMARY, sw.summary_len);
        emit(QGCM_HIP_CPL_STAGE2, 0L);
        if (nranks > 1) {
          if (sw.halo_p2p) emit(QGCM_HIP_CPL_HALO_P2P, sw.halo_len);
          else emit(QGCM_HIP_CPL_HALO_GATHER, 2 * sw.halo_len);
        }
        const bool avg = (s - 1) % ocean_avg_period == 0;
        if (nranks > 1 || avg) emit(avg ? QGCM_HIP_CPL_STAGE3_AVG : QGCM_HIP_CPL_STAGE3, 0L);
      }
      const int nn = nt + (nstr - (nt - 1) % nstr); // the next nt with mod(nt,nstr) == 1
      if (nn < end) next = nn;
    }
    for (; nt < next; ++nt) emit(QGCM_HIP_CPL_ATM_STEP, 0L);
  }
  return 0;
}

extern "C" int qgcm_hip_slab_coupled_plan(const qgcm_hip_slab_coupled_switches *sw, int nranks, int nt0, int n, int nstr, int xforc,
                                          long cap, int *codes, long *lens, long *count) {
  const char *who = "qgcm_hip_slab_coupled_plan";
  if (!sw || !count || cap < 0 || (cap > 0 && (!codes || !lens))) QG_FAIL("%s: null argument", who);
  long k = 0;
  if (cpl_plan(who, *sw, nranks, nt0, n, nstr, xforc, [&](int code, long len) {
        if (k < cap) {
          codes[k] = code;
          lens[k] = len;
        }
        ++k;
      }))
    return 1;
  *count = k;
  if (cap > 0 && k > cap) QG_FAIL("%s: the plan has %ld operations, the arrays hold %ld", who, k, cap);
  return 0;
}

// what both handle calls check first
static int cpl_ready(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const char *who) {
  if (!oc || !atm) QG_FAIL("%s: null handle", who);
  if (check_ready(oc, who)) return 1;
  if (oc->g.atm) QG_FAIL("%s: the first handle must be a y-slab ocean", who);
  if (oc->device != atm->device)
    QG_FAIL("%s: the slab lives on device %d, the atmosphere on device %d: a replica steps beside its slab", who, oc->device, atm->device);
  if (xf_ready(oc, atm, who, true)) return 1;
  if (!oc->sc_comm) QG_FAIL("%s: no communicator (qgcm_hip_comm_init)", who);
  if (oc->sc_comm->overlap)
    QG_FAIL("%s: the overlapped halo exchange is switched on (qgcm_hip_comm_set_overlap): the window runs the plain stage order", who);
  return 0;
}

// the switches and message lengths of a pair as it is set up now
static int cpl_switches(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, qgcm_hip_slab_coupled_switches &sw) {
  const auto &x = atm->xf;
  memset(&sw, 0, sizeof(sw));
  sw.oml = oc->oml.on;
  sw.heat = x.heat.on;
  sw.bands = x.bands.on;
  sw.udiff_gather = x.udiff.on;
  sw.udiff_sums = x.sums.on;
  sw.halo_p2p = oc->sc_comm->halo_p2p;
  sw.xforc_len = qgcm_hip_xforc_slab_msg_len(atm);
  if (x.udiff.on && qgcm_hip_xforc_slab_pom_len(oc, atm, &sw.pom_len)) return 1;
  if (x.sums.on && qgcm_hip_xforc_slab_edge_len(oc, atm, &sw.edge_len)) return 1;
  sw.oml_len = qgcm_hip_oml_msg_len(oc);
  sw.summary_len = qgcm_hip_thomas_msg_len(oc);
  sw.halo_len = qgcm_hip_halo_msg_len(oc);
  return 0;
}

extern "C" int qgcm_hip_slab_coupled_init(qgcm_hip_handle oc, qgcm_hip_handle atm) {
  const char *who = "qgcm_hip_slab_coupled_init";
  if (cpl_ready(oc, atm, who)) return 1;
  qgcm_hip_slab_coupled_switches sw;
  if (cpl_switches(oc, atm, sw)) return 1;
  const int P = oc->sc_comm->nranks;
  HIPCHECK(hipSetDevice(oc->device));
  // a window queued earlier may still read the buffers this call replaces, on either stream
  HIPCHECK(hipStreamSynchronize(oc->stream));
  HIPCHECK(hipStreamSynchronize(atm->stream));
  delete oc->sc_cpl;
  oc->sc_cpl = nullptr;
  std::unique_ptr<QgSlabCoupled> k(new QgSlabCoupled); // (a failure below leaves the handle without the buffers)
  k->atm = atm;
  k->xf_len = sw.xforc_len;
  k->pom_len = sw.pom_len;
  k->edge_len = sw.edge_len;
  struct { QgDbl *buf; size_t n; } bufs[] = {{&k->xf_send, (size_t)k->xf_len},     {&k->xf_gath, (size_t)k->xf_len * P},
                                             {&k->pom_send, (size_t)k->pom_len},   {&k->pom_gath, (size_t)k->pom_len * P},
                                             {&k->edge_send, (size_t)k->edge_len}, {&k->edge_gath, (size_t)k->edge_len * P}};
  for (auto &b : bufs) {
    if (!b.n) continue;
    if (b.buf->alloc(b.n, "an exchange buffer of the coupled window")) return 1;
    HIPCHECK(hipMemsetAsync(*b.buf, 0, b.n * sizeof(double), oc->stream));
  }
  HIPCHECK(hipEventCreateWithFlags(&k->ev_msg, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&k->ev_gath, hipEventDisableTiming));
  HIPCHECK(hipStreamSynchronize(oc->stream));
  oc->sc_cpl = k.release(); // owned by the handle from here on (~qgcm_hip_ctx)
  return 0;
}

// One all-gather of the window's xforc messages.  The message was written on the replica's stream and the gathered
// messages are read there; the collective runs on the slab's stream, like every other one of this communicator.
static int cpl_gather(qgcm_hip_ctx *oc, qgcm_hip_ctx *atm, const double *send, double *gath, long len) {
  QgSlabComm *m = oc->sc_comm;
  QgSlabCoupled *k = oc->sc_cpl;
  HIPCHECK(hipEventRecord(k->ev_msg, atm->stream));
  HIPCHECK(hipStreamWaitEvent(oc->stream, k->ev_msg, 0));
  NCCLCHECK(m->api, m->api->AllGather(send, gath, (size_t)len, ncclDouble, m->comm, oc->stream));
  HIPCHECK(hipEventRecord(k->ev_gath, oc->stream));
  HIPCHECK(hipStreamWaitEvent(atm->stream, k->ev_gath, 0));
  return 0;
}

extern "C" int qgcm_hip_slab_coupled_steps(qgcm_hip_handle oc, qgcm_hip_handle atm, int nt0, int n, int nstr, int xforc) {
  const char *who = "qgcm_hip_slab_coupled_steps";
  if (cpl_ready(oc, atm, who)) return 1;
  QgSlabCoupled *k = oc->sc_cpl;
  if (!k || k->atm != atm) QG_FAIL("%s: qgcm_hip_slab_coupled_init has not been called for this slab and atmosphere", who);
  if (!oc->homog_set) QG_FAIL("%s: homogeneous solutions not set", who);
  QgSlabComm *m = oc->sc_comm;
  const int r = m->rank, P = m->nranks;
  qgcm_hip_slab_coupled_switches sw;
  if (cpl_switches(oc, atm, sw)) return 1;
  if (sw.xforc_len != k->xf_len || sw.pom_len != k->pom_len || sw.edge_len != k->edge_len)
    QG_FAIL("%s: xforc's set-up changed after qgcm_hip_slab_coupled_init (message sizes differ): call it again", who);
  if ((long)m->th_len != sw.summary_len || (long)m->halo_len != sw.halo_len)
    QG_FAIL("%s: the mixed layer was switched on after qgcm_hip_comm_init (message sizes differ)", who);
  std::vector<std::pair<int, long>> plan;
  if (cpl_plan(who, sw, P, nt0, n, nstr, xforc, [&](int code, long len) { plan.push_back({code, len}); })) return 1;
  const size_t nh = m->halo_len;
  double *to_lo = r > 0 ? (double *)m->h_send : nullptr, *to_hi = r < P - 1 ? m->h_send + nh : nullptr;
  const double *from_lo = nullptr, *from_hi = nullptr;
  if (P > 1) slab_halo_from(m, from_lo, from_hi);
  int nt = nt0; // the next atmospheric step
  for (size_t i = 0; i < plan.size(); ++i) {
    const long len = plan[i].second;
    switch (plan[i].first) {
      case QGCM_HIP_CPL_XF_EDGE_PACK:
        if (qgcm_hip_xforc_slab_edge_pack(oc, atm, k->edge_send)) return 1;
        break;
      case QGCM_HIP_CPL_GATHER_EDGE:
        if (cpl_gather(oc, atm, k->edge_send, k->edge_gath, len)) return 1;
        break;
      case QGCM_HIP_CPL_XF_EDGE_ASSEMBLE:
        if (qgcm_hip_xforc_slab_edge_assemble(oc, atm, k->edge_gath, P)) return 1;
        break;
      case QGCM_HIP_CPL_XF_POM_PACK:
        if (qgcm_hip_xforc_slab_pom_pack(oc, atm, k->pom_send)) return 1;
        break;
      case QGCM_HIP_CPL_GATHER_POM:
        if (cpl_gather(oc, atm, k->pom_send, k->pom_gath, len)) return 1;
        break;
      case QGCM_HIP_CPL_XF_POM_ASSEMBLE:
        if (qgcm_hip_xforc_slab_pom_assemble(oc, atm, k->pom_gath, P)) return 1;
        break;
      case QGCM_HIP_CPL_XF_PART: // (ends with the hand-over: the slab's stream waits for it)
        if (qgcm_hip_xforc_slab_part(oc, atm, k->xf_len ? (double *)k->xf_send : nullptr)) return 1;
        break;
      case QGCM_HIP_CPL_GATHER_XFORC:
        if (cpl_gather(oc, atm, k->xf_send, k->xf_gath, len)) return 1;
        break;
      case QGCM_HIP_CPL_XF_COMBINE: // (likewise)
        if (qgcm_hip_xforc_slab_combine(oc, atm, k->xf_gath, P)) return 1;
        break;
      case QGCM_HIP_CPL_OML_A:
        if (launch_oml_a(oc, m->oml_send)) return 1;
        break;
      case QGCM_HIP_CPL_GATHER_OML:
        NCCLCHECK(m->api, m->api->AllGather(m->oml_send, m->oml_gath, (size_t)len, ncclDouble, m->comm, oc->stream));
        break;
      case QGCM_HIP_CPL_OML_B:
        oc->oml_gath = m->oml_gath; // (slab_solve_unpack reads it)
        if (launch_oml_b(oc, m->oml_gath, P)) return 1;
        break;
      case QGCM_HIP_CPL_STAGE1:
        if (slab_tend(oc, TEND_ALL, m->th_send) || slab_forward(oc, m->th_send, r, P)) return 1;
        break;
      case QGCM_HIP_CPL_GATHER_SUMMARY:
        NCCLCHECK(m->api, m->api->AllGather(m->th_send, m->th_gath, (size_t)len, ncclDouble, m->comm, oc->stream));
        break;
      case QGCM_HIP_CPL_STAGE2:
        if (slab_solve_unpack(oc, m->th_gath, to_lo, to_hi, r, P)) return 1;
        break;
      case QGCM_HIP_CPL_HALO_GATHER:
      case QGCM_HIP_CPL_HALO_P2P:
        if (slab_halo_exchange(m, plan[i].first == QGCM_HIP_CPL_HALO_P2P, oc->stream)) return 1;
        break;
      case QGCM_HIP_CPL_STAGE3:
      case QGCM_HIP_CPL_STAGE3_AVG:
        if (slab_halo_in(oc, from_lo, from_hi, P, plan[i].first == QGCM_HIP_CPL_STAGE3_AVG)) return 1;
        break;
      case QGCM_HIP_CPL_ATM_STEP: { // a run of them is one call: the replica's own graphs, averaging and schedules
        int cnt = 1;
        while (i + 1 < plan.size() && plan[i + 1].first == QGCM_HIP_CPL_ATM_STEP) ++i, ++cnt;
        if (steps_impl(atm, nt, cnt, false)) return 1;
        nt += cnt;
        break;
      }
      default: QG_FAIL("%s: internal: the plan holds the unknown operation %d", who, plan[i].first);
    }
  }
  return 0;
}

// Instantiate (and upload) the graphs qgcm_hip_steps(s0, n) will replay, without running anything: a caller that
// times a window with its own clock calls this first, so that capture + instantiation stay outside the window.
extern "C" int qgcm_hip_prepare_steps(qgcm_hip_handle c, int s0, int n) {
  if (check_ready(c, "qgcm_hip_prepare_steps")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_prepare_steps: this handle is a y-slab");
  if (s0 < 1 || n < 0) QG_FAIL("qgcm_hip_prepare_steps: bad step range");
  if (steps_impl(c, s0, n, true)) return 1;
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_time_steps(qgcm_hip_handle c, int s0, int n, float *ms) {
  if (check_ready(c, "qgcm_hip_time_steps")) return 1;
  QgEventPair ev;
  if (ev.create()) return 1;
  const hipEvent_t a = ev.a, b = ev.b;
  // instantiate the graphs the run replays outside the timed region
  if (steps_impl(c, s0, n, true)) return 1;
  HIPCHECK(hipEventRecord(a, c->stream));
  if (qgcm_hip_steps(c, s0, n)) return 1;
  HIPCHECK(hipEventRecord(b, c->stream));
  // (polling, not hipEventSynchronize: a caller that times the call with its own clock should not pay the wake-up
  //  latency of a blocking wait - tens of microseconds on a window of 20 steps)
  for (;;) {
    const hipError_t q = hipEventQuery(b);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) HIPCHECK(q);
  }
  (void)hipGetLastError(); // (hipErrorNotReady of the polls is not an error to report later)
  float t = 0.f;
  HIPCHECK(hipEventElapsedTime(&t, a, b));
  if (ms) *ms = t;
  return 0;
}

extern "C" int qgcm_hip_profile_steps(qgcm_hip_handle c, int s0, int n, double *ms, int *launches, const char **names, int *nk) {
  if (check_ready(c, "qgcm_hip_profile_steps")) return 1;
  if (!nk || *nk < KN_COUNT) QG_FAIL("qgcm_hip_profile_steps: need room for %d kernels", KN_COUNT);
  for (int i = 0; i < KN_COUNT; ++i) {
    c->kms[i] = 0.0;
    c->klaunch[i] = 0;
  }
  HIPCHECK(hipStreamSynchronize(c->stream));
  c->profiling = true;
  c->timer_err = hipSuccess;
  // Calibration of the brackets. An event record is a packet of its own on the stream, so a
  // bracket reads (kernel + its two records). "k_noop" is an empty launch bracketed like the
  // kernels; "k_noop_train" is a long train of empty launches inside ONE bracket, i.e. what an
  // empty launch costs on the stream by itself. Their difference is the cost of a bracket.
  const int ntrain = 512;
  {
    KTimer t(c, KN_NOOP_TRAIN);
    for (int i = 0; i < ntrain; ++i) hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, c->stream);
  }
  // all brackets of the n steps are queued without a host synchronisation in between (the
  // stream stays busy, as in the timed region) and read at the end
  int rc = qgcm_hip_steps(c, s0, n);
  drain_timers(c);
  c->profiling = false;
  if (rc) return 1;
  if (c->timer_err != hipSuccess) QG_FAIL("qgcm_hip_profile_steps: event record failed: %s", hipGetErrorName(c->timer_err));
  c->klaunch[KN_NOOP_TRAIN] = ntrain;
  for (int i = 0; i < KN_COUNT; ++i) {
    if (ms) ms[i] = c->kms[i];
    if (launches) launches[i] = c->klaunch[i];
    if (names) names[i] = kKernelNames[i];
  }
  *nk = KN_COUNT;
  return 0;
}

extern "C" int qgcm_hip_copy_bandwidth(qgcm_hip_handle c, size_t bytes, int reps, double *gbps) {
  if (!c || !gbps) QG_FAIL("qgcm_hip_copy_bandwidth: null argument");
  QgBuf<double2> a, b; // scratch
  const long n = (long)(bytes / sizeof(double2));
  if (a.alloc(n, "the probe's source") || b.alloc(n, "the probe's destination")) return 1;
  HIPCHECK(hipMemset(a, 1, n * sizeof(double2)));
  QgEventPair ev;
  if (ev.create()) return 1;
  const hipEvent_t e0 = ev.a, e1 = ev.b;
  hipLaunchKernelGGL(k_copy, dim3(2048), dim3(256), 0, c->stream, a, b, n);
  HIPCHECK(hipEventRecord(e0, c->stream));
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_copy, dim3(2048), dim3(256), 0, c->stream, a, b, n);
  HIPCHECK(hipEventRecord(e1, c->stream));
  HIPCHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  *gbps = 2.0 * (double)n * sizeof(double2) * reps / (ms * 1e-3) / 1e9;
  return 0;
}

// Rate (GB/s of read + written bytes) of a pure streaming kernel that reads nr fields and writes nw fields of
// field_bytes each (the mixes of the hot kernels: 15:6 tendency, 3:3 rows / sweep, 5:3 fused inverse rows, 1:1 the
// covariances' rank-1 update).
extern "C" int qgcm_hip_stream_mix_bandwidth(qgcm_hip_handle c, int nr, int nw, size_t field_bytes, int reps, double *gbps) {
  if (!c || !gbps) QG_FAIL("qgcm_hip_stream_mix_bandwidth: null argument");
  field_bytes = field_bytes / 4096 * 4096;
  if (field_bytes == 0 || reps < 1) QG_FAIL("qgcm_hip_stream_mix_bandwidth: bad size / repetitions");
  QgBuf<double2> a, b; // scratch
  const long nper = (long)(field_bytes / sizeof(double2));
  if (a.alloc((size_t)nper * nr, "the probe's sources") || b.alloc((size_t)nper * (nw > 0 ? nw : 1), "the probe's destinations"))
    return 1;
  QgEventPair ev;
  if (ev.create()) return 1;
  const hipEvent_t e0 = ev.a, e1 = ev.b;
  auto launch = [&]() -> int {
    const dim3 grid(2048), block(256);
    if (nr == 15 && nw == 6) hipLaunchKernelGGL((k_stream_mix<15, 6>), grid, block, 0, c->stream, a, b, nper);
    else if (nr == 3 && nw == 3) hipLaunchKernelGGL((k_stream_mix<3, 3>), grid, block, 0, c->stream, a, b, nper);
    else if (nr == 5 && nw == 3) hipLaunchKernelGGL((k_stream_mix<5, 3>), grid, block, 0, c->stream, a, b, nper);
    else if (nr == 1 && nw == 1) hipLaunchKernelGGL((k_stream_mix<1, 1>), grid, block, 0, c->stream, a, b, nper);
    else return 1;
    return 0;
  };
  int rc = 0;
  for (int w = 0; w < 3 && !rc; ++w) rc = launch();
  if (!rc) {
    HIPCHECK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; ++r) launch();
    HIPCHECK(hipEventRecord(e1, c->stream));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    *gbps = (double)field_bytes * (nr + nw) * reps / (ms * 1e-3) / 1e9;
  }
  if (rc) QG_FAIL("qgcm_hip_stream_mix_bandwidth: supported mixes are 15:6, 3:3, 5:3 and 1:1");
  return 0;
}

extern "C" void *qgcm_hip_stream(qgcm_hip_handle c) { return c ? (void *)c->stream : nullptr; }

#ifdef QG_STAMPS
// development builds only (scratch/stamps.py): the phase stamps of the last launch of each instrumented kernel
extern "C" int qgcm_hip_debug_stamps(long long *out, size_t nbytes) {
  if (nbytes > sizeof(qg_stamps)) nbytes = sizeof(qg_stamps);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(qg_stamps), nbytes, 0, hipMemcpyDeviceToHost));
  return 0;
}
#endif

// ---------------------------------------------------------------------------
// The zero-field variants of the tendency kernel.  LAST in the file: see the declaration in front of launch_tend.
// ---------------------------------------------------------------------------
template <int NL, bool CYC, bool WTQ, bool AVG>
static void tend_z_go(int zm, dim3 grid, hipStream_t stream, const QgTendParams &P, const QgCycSumParams &S, const QgOmlFinal &F) {
  switch (zm) {
    case 3: hipLaunchKernelGGL((k_tend_z<NL, CYC, WTQ, AVG, 3>), grid, dim3(TEND_NT), 0, stream, QG_TEND_VALS(P, F), P, S, F); break;
    case 2: hipLaunchKernelGGL((k_tend_z<NL, CYC, WTQ, AVG, 2>), grid, dim3(TEND_NT), 0, stream, QG_TEND_VALS(P, F), P, S, F); break;
    default: hipLaunchKernelGGL((k_tend_z<NL, CYC, WTQ, AVG, 1>), grid, dim3(TEND_NT), 0, stream, QG_TEND_VALS(P, F), P, S, F); break;
  }
}

// launch_tend's choice of NL, CYC, WTQ, AVG, mirrored (the 5 km box ocean first: its variants lead the group)
static void launch_tend_z(int zm, int nl, bool cyc, bool wtq, bool avg, dim3 grid, hipStream_t stream, const QgTendParams &P,
                          const QgCycSumParams &S, const QgOmlFinal &F) {
#define QG_TEND_Z(NLV)                                                         \
  if (cyc && wtq) tend_z_go<NLV, true, true, false>(zm, grid, stream, P, S, F); \
  else if (cyc) tend_z_go<NLV, true, false, false>(zm, grid, stream, P, S, F);  \
  else if (wtq) tend_z_go<NLV, false, true, false>(zm, grid, stream, P, S, F);  \
  else tend_z_go<NLV, false, false, false>(zm, grid, stream, P, S, F)
  if (!cyc && wtq && nl == 3) { // (first in the group whatever happens to the other variants: its place stays put)
    if (avg) tend_z_go<3, false, true, true>(zm, grid, stream, P, S, F);
    else tend_z_go<3, false, true, false>(zm, grid, stream, P, S, F);
  } else if (avg && cyc) {
    if (wtq) tend_z_go<3, true, true, true>(zm, grid, stream, P, S, F);
    else tend_z_go<3, true, false, true>(zm, grid, stream, P, S, F);
  } else if (avg) {
    switch (nl) {
      case 3: tend_z_go<3, false, true, true>(zm, grid, stream, P, S, F); break;
      case 2: tend_z_go<2, false, true, true>(zm, grid, stream, P, S, F); break;
      default: tend_z_go<4, false, true, true>(zm, grid, stream, P, S, F); break;
    }
  } else {
    switch (nl) {
      case 3: QG_TEND_Z(3); break;
      case 2: QG_TEND_Z(2); break;
      default: QG_TEND_Z(4); break;
    }
  }
#undef QG_TEND_Z
}

// ---------------------------------------------------------------------------
// The row-band kernel: tendency + forward rows of the 5 km box ocean in one launch (k_tend_rows.h, k_tend_rows.hip).
// ---------------------------------------------------------------------------
static int launch_tend_rows(qgcm_hip_ctx *c, bool upd_dpi) {
  const QgGeom &g = c->g;
  QgTendParams P;
  fill_tend_params(c, P, upd_dpi);
  const int zm = tend_zmask(c);
  // (ny * ldx < 2^29: the kernel forms 32-bit byte offsets inside a layer)
  if (g.cyc || g.nl != 3 || g.nxt != 960 || !c->whole || g.joff != 0 || g.jlo != 1 || g.jhi != g.ny || g.nyg != g.ny || g.ny < 3 ||
      (long)g.ny * g.ldx >= (1L << 29) || (zm != 0 && zm != 3) || P.rspl)
    QG_FAIL("k_tend_rows: the row-band kernel belongs to whole-domain steps of the three-layer box ocean with 960-point rows");
  KTimer t(c, KN_TEND, c->stream);
  qg_launch_tend_rows(zm, c->stream, P, c->twid, c->sintab);
  HIPCHECK(hipGetLastError());
  return 0;
}
