/* qgcm_hip.h - C ABI of the MI355X-native Q-GCM ocean PV-advance / inversion path.
 *
 * Drop-in boundary for the three argument-less calls the reference main
 * program makes once per ocean step (src/q-gcm.F:1243-1249):
 *
 *     call qgostep          -> qgcm_hip_qgostep()   (src/qgosubs.F:45-221 + ocadif 231-446)
 *     call ocinvq           -> qgcm_hip_ocinvq()    (src/ocisubs.F:64-407, hsbxoc 415-512, hscyoc 521-618)
 *     call ocqbdy (qo, po)  -> qgcm_hip_ocqbdy()    (src/vorsubs.F:245-388)
 *
 * plus the leapfrog time-level averaging block (src/q-gcm.F:1328-1366), the
 * Helmholtz solver that homsol calls at start-up (src/conhoms.F:454-455,572)
 * and the data movement that replaces the reference's shared module arrays
 * (ocstate: src/ocstate_data.F:39-42; occonst: src/occonst_data.F:36-44;
 * ochomog: src/ochomog_data.F:44-68; ocisubs: src/ocisubs.F:51-55).
 *
 * Conventions
 *  - plain C: raw double pointers + sizes, no Fortran descriptors, no torch types.
 *  - every host array is Fortran ordered exactly as the reference declares
 *    it, e.g. po(nxpo,nypo,nlo): element (i,j,k) 1-based at
 *    (i-1) + nxpo*((j-1) + nypo*(k-1)).  Host buffers are caller-owned and
 *    never retained.
 *  - the device owns the authoritative po,pom,qo,qom between set_state and
 *    get_state; all kernels run on one HIP stream owned by the handle.
 *  - every entry point returns 0 on success, non-zero on failure;
 *    qgcm_hip_last_error() returns a static description.  The reference's
 *    own convention is print + stop (e.g. src/ocisubs.F:361-365); the Fortran
 *    shim (q-gcm_amd/fortran) restores that behaviour.
 *  - one host thread per handle (the reference is called from its single
 *    main thread); calls are asynchronous until qgcm_hip_sync / a get_*.
 *  - there is NO CPU fallback: without a HIP device create() fails.
 */
#ifndef QGCM_HIP_H
#define QGCM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QGCM_HIP_MAXL 8 /* max number of QG layers supported: 2 <= nlo <= 8 (kernels instantiated for every count;
                           the fused single-launch forms of the inversion for nlo <= 4) */
/* 2: qgcm_hip_params.atmos + the atmosphere entry points
 * 3: qgcm_hip_get_monitors (required by the Fortran shim), qgcm_hip_prepare_steps, qgcm_hip_stream_mix_bandwidth,
 *    qgcm_hip_set_sponge, qgcm_hip_set_cu_range; halo rows of qgcm_hip_slab_steps default to neighbour send/recv
 *    (entry points added since keep the number - there is no minor version: qgcm_hip_slab_coupled_plan / _init / _steps
 *    the latest) */
#define QGCM_HIP_ABI_VERSION 3

typedef struct qgcm_hip_ctx *qgcm_hip_handle;

/* Scalars + small matrices of MODULE parameters / occonst / ochomog that the
 * path reads (src/parameters_data.F:23-147, src/occonst_data.F:36-44).
 * Matrices are Fortran ordered with leading dimension nlo, packed. */
typedef struct qgcm_hip_params {
  int nxpo, nypo, nlo; /* p-grid size, layers */
  int cyclic;          /* 1 = -Dcyclic_ocean (hscyoc path), 0 = box (hsbxoc) */
  double fnot, beta;   /* parameters_data.F: fnot, beta */
  double dxo, dyo;     /* occonst: grid spacing (dyo = dxo in the reference) */
  double tdto;         /* occonst: 2*dto */
  double delek;        /* bottom Ekman layer thickness */
  double bccooc;       /* mixed BC coefficient */
  double ah2oc[QGCM_HIP_MAXL];
  double ah4oc[QGCM_HIP_MAXL];
  double hoc[QGCM_HIP_MAXL];
  double gpoc[QGCM_HIP_MAXL];                        /* nlo-1 used */
  double amatoc[QGCM_HIP_MAXL * QGCM_HIP_MAXL];      /* amatoc(nlo,nlo)   eigmode.f:131-144 */
  double ctl2moc[QGCM_HIP_MAXL * QGCM_HIP_MAXL];     /* ctl2moc(nlo,nlo)  eigmode.f:420-428 */
  double ctm2loc[QGCM_HIP_MAXL * QGCM_HIP_MAXL];     /* ctm2loc(nlo,nlo) */
  double rdm2oc[QGCM_HIP_MAXL];                      /* 1/Rd^2 per mode */
  double aoc;                                        /* ocisubs: 1/dyo^2 (q-gcm.F:932) */
  /* y-slab decomposition (no counterpart in the reference, which is single-process):
   * this handle owns the global rows slab_g0..slab_g1 (1-based, inclusive) of the
   * nypo rows; 0,0 = the whole domain.  In slab mode every host array passed to
   * set_/get_* is the LOCAL block (nxpo, nyl, .) with nyl = owned rows + a 3-row
   * halo on each side that has a neighbour (qgcm_hip_local_rows). */
  int slab_g0, slab_g1;
  /* 1 = the handle is the ATMOSPHERIC channel of a coupled run: qgastep / atinvq / atqzbd
   * (src/qgasubs.F:45-317, src/atisubs.F:60-395, src/vorsubs.F:396-480).  Zonally periodic (cyclic must be 1);
   * the fields of this struct then carry MODULE atconst / parameters values under the ocean's names:
   * nxpo,nypo,nlo = nxpa,nypa,nla; dxo,dyo = dxa,dya; tdto = tdta; bccooc = bccoat; ah4oc = ah4at; hoc = hat;
   * gpoc = gpat; amatoc.. = amatat, ctl2mat, ctm2lat, rdm2at; aoc = aat; delek and ah2oc are ignored.
   * Differences from the cyclic ocean that the kernels honour: layer 1 is the bottom layer (topography term
   * in layer 1), forcing signs of src/qgasubs.F:128-131, no drag and no Del-4th term, constraint right-hand
   * sides of src/atisubs.F:177-196, dpiat = integral of pa(k)-pa(k+1), src/vorsubs.F:470 as written,
   * time levels averaged when mod(nt-1,100) == 0 (src/q-gcm.F:1370). */
  int atmos;
} qgcm_hip_params;

/* ---- life cycle -------------------------------------------------------- */
/* device < 0: use the current HIP device. */
int qgcm_hip_create(qgcm_hip_handle *h, const qgcm_hip_params *prm, int device);
int qgcm_hip_destroy(qgcm_hip_handle h);
const char *qgcm_hip_last_error(void);
int qgcm_hip_abi_version(void);

/* yporel(nypo), bd2oc(nxto) [reference/FFTPACK ordering, q-gcm.F:933-954],
 * ddynoc(nxpo,nypo).  Builds the device-side Thomas tables.
 *
 * Column height.  The whole-column tridiagonal kernel holds a column of at most QGCM_HIP_THOMAS_MAX_ROWS = 2048 interior
 * rows (nypo - 2).  A WHOLE-DOMAIN OCEAN handle, box or zonally cyclic, with a taller column (NAtl 2 km: 2401 rows,
 * NAtl 1 km: 4801) cuts it into balanced segments - qgcm_hip_thomas_segments gives the plan - and solves it in two
 * launches per inversion instead of one.  Every entry point that wants a whole-domain handle accepts such a handle;
 * run on one so far (README): qgcm_hip_steps and its graphs, the three stand-alone calls, helmholtz, oml, valids, prsamp;
 * accepted but not yet run on one: qgcm_hip_coupled_steps, xforc, the monitors, time averages, dumps and covariances.
 * A Y-SLAB of an ocean with more than 2048 interior rows takes a plan by the same rule.  It solves its segments in two
 * launches before the exchange of the slab summaries and one after it, and still publishes ONE summary per step and
 * ONE set of set-up constants, in the layout and lengths of every other slab (qgcm_hip_thomas_msg_len / _const_len):
 * the other ranks cannot tell, and ranks with different plans mix freely.  Every slab entry point drives such a handle
 * unchanged.  A whole-domain handle in segments is a lone slab (nranks = 1) to qgcm_hip_thomas_phase and
 * qgcm_hip_slab_steps.  An atmosphere handle of more than 2048 rows is refused by this call.
 * QGCM_HIP_THOMAS_SEG_ROWS=<n> (environment, read by this call for WHOLE-DOMAIN handles) and
 * QGCM_HIP_THOMAS_SLAB_SEG_ROWS=<n> (read for Y-SLABS, i.e. handles that own part of the rows): the longest segment,
 * 2 * QGCM_HIP_THOMAS_SEG_MIN - 1 <= n; columns of ANY height longer than n are then cut (n > 2048 counts as 2048) -
 * tests force segments on small basins with them.  Anything but a positive integer is refused.  Unset, columns of up
 * to 2048 rows take the single launch.  Neither variable is read for the other kind of handle. */
int qgcm_hip_set_grid(qgcm_hip_handle h, const double *yporel, const double *bd2oc,
                      const double *ddynoc);
#define QGCM_HIP_THOMAS_MAX_ROWS 2048 /* rows of one segment = of a column solved by the single-segment kernel */
#define QGCM_HIP_THOMAS_SEG_MIN 4     /* no segment is shorter (the minimum of a y-slab, qgcm_hip_create) */
#define QGCM_HIP_THOMAS_MAX_SEG 64    /* segments per column */
#define QGCM_HIP_THOMAS_SEG_DEFAULT 1024 /* longest segment of a column of more than 2048 rows when no maximum is given */
/* The segment plan of a column of nrows interior rows; pure host code, no handle and no device needed.
 * max_rows > 0: no segment is longer than min(max_rows, 2048); max_rows <= 0: one segment up to 2048 rows, segments
 * of at most QGCM_HIP_THOMAS_SEG_DEFAULT = 1024 rows beyond.  *nseg = S = the fewest segments that respect the maximum; segment s covers the interior rows
 * first[s] .. first[s] + count[s] - 1 (0-based, in order, each row once); the lengths differ by at most one (the longer
 * ones first).  first / count (QGCM_HIP_THOMAS_MAX_SEG ints each) may be NULL.  Fails (non-zero) for nrows < 1, for a
 * maximum below 2 * QGCM_HIP_THOMAS_SEG_MIN - 1 (it could leave a segment shorter than the minimum) and for more than
 * QGCM_HIP_THOMAS_MAX_SEG segments. */
int qgcm_hip_thomas_segments(int nrows, int max_rows, int *nseg, int *first, int *count);
/* The plan the handle actually uses (after qgcm_hip_set_grid): *nseg segments, segment s = the handle's interior rows
 * first[s] .. first[s] + count[s] - 1 (0-based from its first interior row; QGCM_HIP_THOMAS_MAX_SEG ints each, may be
 * NULL).  One segment of all interior rows for a handle on the single-segment kernel, the atmosphere included. */
int qgcm_hip_thomas_plan(qgcm_hip_handle h, int *nseg, int *first, int *count);
/* Row length.  The row kernels hold a row pair of at most 5104 points in LDS.  A ZONALLY CYCLIC OCEAN handle (whole
 * domain or y-slab) with longer rows (the reference's SOcn 4 km .. 1 km: nxto = 5760, 7680, 11520, 23040) transforms
 * each row as P interleaved sub-rows of length L = nxto / P through one scratch array of the work array's size, three
 * launches per transform instead of one; every entry point drives such a handle unchanged.  qgcm_hip_row_split gives
 * the plan: P = 1 (L = nxto) up to 5104 points; beyond, the smallest P in 2 .. QGCM_HIP_ROW_SPLIT_MAX_P that divides
 * nxto and leaves an even L <= 5104 the row kernels take (5760 = 2 x 2880, 7680 = 2 x 3840, 11520 = 3 x 3840,
 * 23040 = 5 x 4608).  forced_P > 0: that P at any length, under the same conditions.  Pure host code, no handle and no
 * device needed.  Fails (non-zero, the message names the limit) when no P qualifies (an odd nxto > 5104, say) and for a
 * forced_P outside 2 .. 5, one that does not divide nxto or one that leaves an odd or too long L.
 * QGCM_HIP_ROW_SPLIT=<P> (environment, read by qgcm_hip_set_grid for zonally cyclic OCEAN handles only) forces the
 * split on rows of any length - tests use it on small basins; anything but a positive integer is refused.
 * Box oceans and atmosphere handles with nxto > 5104 are refused by qgcm_hip_set_grid. */
#define QGCM_HIP_ROW_SPLIT_MAX_P 5
int qgcm_hip_row_split(int nxto, int forced_P, int *P, int *L);
/* The row plan the handle uses (after qgcm_hip_set_grid): *P sub-rows of length *L per row; (1, nxto) for a handle that
 * transforms its rows whole. */
int qgcm_hip_row_plan(qgcm_hip_handle h, int *P, int *L);
/* The part of set_grid that does not need bd2oc: yporel and ddynoc only.  The main program calls ocqbdy / atqzbd on
 * host arrays (src/q-gcm.F:724-725, 743-744) before it computes bd2oc (:932-972); qgcm_hip_ocqbdy_host needs no more
 * than this.  The stepping entry points still require qgcm_hip_set_grid. */
int qgcm_hip_set_geometry(qgcm_hip_handle h, const double *yporel, const double *ddynoc);

/* Products of homsol (src/conhoms.F:544-641 box / 376-543 cyclic).
 * box:    ochom(nxpo,nypo,nlo-1), cdiffo(nlo,nlo-1), cdhoc(nlo-1,nlo-1)
 *         (the LU factors cdhlu/ipivch are recomputed internally).
 * cyclic: pch1oc(nypo,nlo-1), pch2oc(nypo,nlo-1), pbhoc(nypo), aipcho(nlo-1),
 *         hc1soc, hc2soc, hc1noc, hc2noc (nlo-1 each), hbsioc, aipbho. */
int qgcm_hip_set_homog_box(qgcm_hip_handle h, const double *ochom, const double *cdiffo,
                           const double *cdhoc);
int qgcm_hip_set_homog_cyc(qgcm_hip_handle h, const double *pch1oc, const double *pch2oc,
                           const double *pbhoc, const double *aipcho, const double *hc1soc,
                           const double *hc2soc, const double *hc1noc, const double *hc2noc,
                           double hbsioc, double aipbho);

/* ---- state (MODULE ocstate) -------------------------------------------- */
/* Any pointer may be NULL to skip that field. */
int qgcm_hip_set_state(qgcm_hip_handle h, const double *po, const double *pom,
                       const double *qo, const double *qom);
int qgcm_hip_get_state(qgcm_hip_handle h, double *po, double *pom, double *qo, double *qom);
/* wekpo(nxpo,nypo), entoc(nxpo,nypo), xon(nlo-1)  (written by xforc / oml) */
int qgcm_hip_set_forcing(qgcm_hip_handle h, const double *wekpo, const double *entoc,
                         const double *xon);
/* Which fields the next tendency launch of the handle leaves out because the library knows them to hold +0.0
 * everywhere: bit 0 = entoc (entat), bit 1 = ddynoc; 0 = both are read; -1 for a NULL handle.  The library scans the
 * host arrays of qgcm_hip_set_forcing / _set_geometry / _set_grid (bit patterns: a -0.0 counts as non-zero) and knows
 * that a fresh handle's buffers are zero; a mixed layer on the device (qgcm_hip_oml_init / _aml_init) writes entoc
 * every step, which clears bit 0 for good.  The results do not depend on the mask, bit for bit;
 * QGCM_HIP_READ_ZERO_FIELDS=1 (read by qgcm_hip_create) keeps it at 0, as does nlo > 4. */
int qgcm_hip_tend_zero_mask(qgcm_hip_handle h);
/* The fork's sponge layer (cpp option sponge_layer_k247): the leapfrog step of qgostep gains
 *   + tdto*c1_spl*r_spl(i,j)*(qom(i,j,k) - beta*yporel(j))            src/qgosubs.F:203-205
 * r_spl(nxpo,nypo): the ramp of MODULE occonst (src/occonst_data.F:100-105) as the main program sets it
 * (src/q-gcm.F:1154-1168; a y-slab handle takes its local rows); c1_spl: src/parameters_data.F:144.
 * NULL switches the term off again (the default: no BASELINE configuration defines the option). */
int qgcm_hip_set_sponge(qgcm_hip_handle h, const double *r_spl, double c1_spl);
/* cyclic only: txisoc, txinoc (xforc), enisoc/eninoc(nlo-1) (oml) */
int qgcm_hip_set_cyc_forcing(qgcm_hip_handle h, double txisoc, double txinoc,
                             const double *enisoc, const double *eninoc);
/* constraint scalars of MODULE ochomog:
 *   scal[0 .. nlo-2]        dpioc
 *   scal[nlo-1 .. 2nlo-3]   dpiocp
 *   then (cyclic) ocncs, ocncn, ocncsp, ocncnp (nlo each); box: ignored/zero.
 * length 2*(nlo-1) + 4*nlo. */
int qgcm_hip_set_scalars(qgcm_hip_handle h, const double *scal);
int qgcm_hip_get_scalars(qgcm_hip_handle h, double *scal);
/* diagnostics of the last ocinvq: xinhom(nlo); coef = hclco(nlo-1) [box] or
 * c1(nlo-1), c2(nlo-1), c3 [cyclic] */
int qgcm_hip_get_inv_diag(qgcm_hip_handle h, double *xinhom, double *coef);
/* Continuity monitors of the last ocinvq / atinvq of a zonally cyclic handle (MODULE monitor: ermaso, emfroc,
 * src/ocisubs.F:268-283; ermasa, emfrat, src/atisubs.F:236-248): nlo-1 doubles each.  Synchronous. */
int qgcm_hip_get_monitors(qgcm_hip_handle h, double *ermas, double *emfr);

/* ---- the path ----------------------------------------------------------- */
int qgcm_hip_qgostep(qgcm_hip_handle h);    /* replaces "call qgostep"        q-gcm.F:1243 */
int qgcm_hip_ocinvq(qgcm_hip_handle h);     /* replaces "call ocinvq"         q-gcm.F:1246 */
int qgcm_hip_ocqbdy(qgcm_hip_handle h);     /* replaces "call ocqbdy (qo,po)" q-gcm.F:1249 */
int qgcm_hip_lf_average(qgcm_hip_handle h); /* ocean part of q-gcm.F:1328-1366 (incl. sst once qgcm_hip_oml_init was called) */
/* "call ocqbdy (q, p)" / "call atqzbd (q, p)" on HOST arrays, as the main program does at start-up for both time
 * levels before the device owns the state (src/q-gcm.F:724-725, 743-744): p(nxpo,nypo,nlo) is uploaded to scratch,
 * the boundary PV kernel runs, and the boundary ring of q(nxpo,nypo,nlo) is written back (interior untouched).
 * Does not touch the device-resident state. Synchronous. */
int qgcm_hip_ocqbdy_host(qgcm_hip_handle h, double *q, const double *p);
/* n whole ocean steps starting at 1-based ocean step index s0: qgostep, ocinvq,
 * ocqbdy and, when mod(s-1,25)==0, the averaging (nt = 1+(s-1)*nstr in
 * q-gcm.F:1222,1328).  Uses captured HIP graphs. */
int qgcm_hip_steps(qgcm_hip_handle h, int s0, int n);
int qgcm_hip_sync(qgcm_hip_handle h);

/* ---- the atmosphere path (handles created with atmos = 1) ------------------
 * One-for-one replacements of the three calls the main program makes every atmospheric step
 * (src/q-gcm.F:1262-1268).  State and inputs move through the calls above under the ocean's names:
 *   set_/get_state     pa, pam, qa, qam (nxpa,nypa,nla)                        MODULE atstate
 *   set_forcing        wekpa, entat (nxpa,nypa), xan(nla-1)                    atstate / athomog (written by xforc / aml)
 *   set_cyc_forcing    txisat, txinat, enisat(nla-1), eninat(nla-1)            athomog
 *   set_/get_scalars   dpiat, dpiatp (nla-1), atmcs, atmcn, atmcsp, atmcnp (nla)
 *   set_homog_cyc      pch1at, pch2at, pbhat, aipcha, hc1sat, hc2sat, hc1nat, hc2nat, hbsiat, aipbha
 *   set_grid           yparel(nypa), bd2at(nxta) [FFTPACK order, src/q-gcm.F:961-970], ddynat(nxpa,nypa)
 *   helmholtz          hscyat (src/atisubs.F:298-395) for homsol (src/conhoms.F:678-679)
 *   lf_average         atmospheric half of the averaging block, src/q-gcm.F:1370-1404
 *   steps(nt0, n)      n atmospheric steps nt = nt0.., averaging after the steps with mod(nt-1,100) == 0 */
int qgcm_hip_qgastep(qgcm_hip_handle h);    /* replaces "call qgastep"          q-gcm.F:1262 */
int qgcm_hip_atinvq(qgcm_hip_handle h);     /* replaces "call atinvq"           q-gcm.F:1265 */
int qgcm_hip_atqzbd(qgcm_hip_handle h);     /* replaces "call atqzbd (qa, pa)"  q-gcm.F:1268 */
/* boundary line sums of the last qgastep / cyclic qgostep, as the reference leaves them in MODULE athomog /
 * ochomog: b = ajis, ajin, ap5s, ap5n (nlo each).  They are formed by the constraint kernel, i.e. valid after
 * the atinvq / ocinvq that follows the step.  Synchronous. */
int qgcm_hip_get_bsums(qgcm_hip_handle h, double *b);
/* A coupled run with the forcing held between calls (xforc / oml / aml stay with the host):
 * atmospheric steps nt = nt0 .. nt0+n-1 on `atm`, and on `oc` one ocean step before every atmospheric step with
 * mod(nt,nstr) == 1 (src/q-gcm.F:1220-1268), each with its own averaging rule.  The two handles run on
 * their own HIP streams, so the small atmospheric kernels overlap the ocean's. Either handle may be NULL. */
int qgcm_hip_coupled_steps(qgcm_hip_handle oc, qgcm_hip_handle atm, int nt0, int n, int nstr);
/* Two handles that step side by side on one GPU (the ocean and the atmosphere under qgcm_hip_coupled_steps) can be
 * given disjoint ranges of compute units: the handle's HIP stream is replaced by one that may use the CUs
 * first .. first+count-1 only (count = 0: all of them again).  Without it the atmosphere's small dependent launches
 * queue behind the ocean's chip-filling ones.  Not for handles with a communicator.  Synchronous; no reference
 * counterpart (the reference runs both halves on the same OpenMP threads, src/q-gcm.F:1220-1268). */
int qgcm_hip_set_cu_range(qgcm_hip_handle h, int first, int count);

/* Helmholtz solve for homsol: wrk(nxpo,nypo) in/out, boc(nxto)
 * (replaces hsbxoc / hscyoc, src/ocisubs.F:415-618). Synchronous.  Any diagonal, not only the modal ones: a handle
 * whose column is cut into segments (see qgcm_hip_set_grid) builds the segments' response tables for this boc on the
 * call and keeps them until another boc arrives. */
int qgcm_hip_helmholtz(qgcm_hip_handle h, double *wrk, const double *boc);

/* ---- y-slab building blocks (multi-GPU; one handle per slab) -------------
 * A distributed step is: qgostep | row_transform(0) | thomas_phase 1, exchange,
 * 2 | constr | row_transform(1) | unpack | halo_pack, exchange, halo_unpack.
 * Two exchanges per step. All buffers named *_dev are DEVICE pointers owned by
 * the caller (e.g. torch tensors used with torch.distributed); every call is
 * asynchronous on the handle's stream. */
int qgcm_hip_local_rows(qgcm_hip_handle h, int *nyl, int *joff, int *jlo, int *jhi);
int qgcm_hip_row_transform(qgcm_hip_handle h, int inverse);
/* number of doubles of one per-step slab summary message: 3 * nlo * ldw (+ the boundary line sums of a cyclic ocean,
 * + 3 sums of the mixed layer once qgcm_hip_oml_init was called - query after it) */
int qgcm_hip_thomas_msg_len(qgcm_hip_handle h);
/* The right-hand-side independent part of the summaries (gains and unit-response sums, 4 * nlo * ldw doubles per
 * slab) is exchanged ONCE after qgcm_hip_set_grid: every rank copies its own with qgcm_hip_thomas_consts, the host
 * all-gathers them (rank-major) and hands the result to qgcm_hip_set_thomas_consts. qgcm_hip_comm_init does this
 * by itself for the library-issued exchanges; a lone slab (nranks = 1) needs nothing. */
int qgcm_hip_thomas_const_len(qgcm_hip_handle h);
int qgcm_hip_thomas_consts(qgcm_hip_handle h, double *dst_dev);
int qgcm_hip_set_thomas_consts(qgcm_hip_handle h, const double *gath_dev, int nranks);
/* phase 1: this slab's summary of the two y sweeps -> send_dev: per mode and wavenumber the zero-inflow
 *          end values of both sweeps and the zero-inflow column sum behind the area integrals
 *          (xintp, src/ocisubs.F:160) - 3 numbers.
 * phase 2: gath_dev = all ranks' phase-1 messages (rank-major) -> both sweeps finished, and the
 *          basin-wide area integrals known on every rank (bitwise the same). */
int qgcm_hip_thomas_phase(qgcm_hip_handle h, int phase, const double *gath_dev, double *send_dev,
                          int rank, int nranks);
/* mass-constraint solve (src/ocisubs.F:329-370) from the area integrals thomas_phase 2 left behind */
int qgcm_hip_constr(qgcm_hip_handle h);
int qgcm_hip_unpack(qgcm_hip_handle h, int fuse_ocqbdy);
/* halo messages: (3 rows of po + 1 row of qo) * nlo rows of ldx doubles each (+ 3 rows of sst with the mixed layer on) */
int qgcm_hip_halo_msg_len(qgcm_hip_handle h);
int qgcm_hip_halo_pack(qgcm_hip_handle h, double *to_lower_dev, double *to_upper_dev);
int qgcm_hip_halo_unpack(qgcm_hip_handle h, const double *from_lower_dev, const double *from_upper_dev);

/* homsol on y-slabs (src/conhoms.F:549-601 needs hsbxoc on the whole basin): the modal Helmholtz problems of a
 * step ARE homsol's (boc = bd2oc - rdm2oc(m)), so the same distributed solve serves - fill the work array with the
 * right-hand side 1 (qgcm_hip_wrk_fill), row_transform(0), thomas_phase 1 | exchange | 2, row_transform(1), read the
 * solutions of the local rows back (qgcm_hip_wrk_get: (nxpo, nyl, nlo) block, walls and halo rows zero) and their
 * basin-wide area integrals dxo*dyo*xintp(wrk_m) (qgcm_hip_area_integrals, from the spectral column sums of
 * thomas_phase 2 / a whole-domain sweep; nlo doubles, synchronous).  No host-side solver is involved. */
int qgcm_hip_wrk_fill(qgcm_hip_handle h, double value);
int qgcm_hip_wrk_get(qgcm_hip_handle h, double *wrk);
/* rows of a (nxpo, nyl, nlo) host block into the work array (the counterpart of qgcm_hip_wrk_get; walls ignored):
 * with qgcm_hip_row_transform this exposes the row transforms that replace FFTPACK's dsint / drfftf / drfftb
 * (src/ocisubs.F:461-463, 494-499, 566-568, 601-605) by themselves - forward: dsint resp. drfftf, unnormalised, the
 * cyclic spectrum in FFTPACK's half-complex order; inverse: dsint resp. drfftb.  Synchronous. */
int qgcm_hip_wrk_set(qgcm_hip_handle h, const double *wrk);
int qgcm_hip_area_integrals(qgcm_hip_handle h, double *xin);

/* One call per communication-free stage of a distributed step (fewer host round trips):
 *   stage 1: qgostep, row_transform(0), thomas_phase(1)                          a = summary send buffer
 *   stage 2: thomas_phase(2), constr, row_transform(1), unpack(+ocqbdy), halo_pack
 *                                                      a = summary gather buffer, b/c = halo to-lower/to-upper
 *   stage 3: halo_unpack, optional lf_average (flags & 1)                        a/b = halo from-lower/from-upper
 *   stage 4 + stage 5 = stage 1 in two parts, for drivers that overlap the halo exchange with compute: stage 4 is the
 *            part of the tendency launch that reads no halo row (all but the first and last 16-row tile row; it may
 *            run before stage 3 of the previous step), stage 5 the rest of stage 1 (a = summary send buffer).  Needs
 *            at least three tile rows per slab and the mixed layer off.
 *   stage 6 + stage 7 = stage 5 in two parts: stage 6 the outer tile rows + edge work of the tendency launch alone (it
 *            may run on another stream BESIDE stage 4 - disjoint tiles - as soon as the halo rows are in: what
 *            qgcm_hip_slab_steps does on the exchange's stream), stage 7 the forward rows and the summary sweep (after
 *            stages 4 and 6; a = summary send buffer in both).
 * With the ocean mixed layer on the device (qgcm_hip_oml_init on every slab, before the buffers are sized) `call oml`
 * (src/q-gcm.F:1232) runs before stage 1, in two halves around ONE more all-gather of qgcm_hip_oml_msg_len() doubles
 * per rank (the mean entrainment is a basin-wide number, src/omlsubs.F:153):
 *   stage 10: new sst, raw entrainment, this slab's sums                         a = send buffer (3 doubles)
 *   stage 11: entoc from entrainment minus mean, sst buffer rotation             a = gathered sums (3 * nranks)
 * xon(1) and the boundary line integrals of entoc then travel at the end of the stage-1 message, the edge rows of sst
 * at the end of the halo messages. */
int qgcm_hip_oml_msg_len(qgcm_hip_handle h);
int qgcm_hip_slab_stage(qgcm_hip_handle h, int stage, double *a_dev, double *b_dev, double *c_dev,
                        int rank, int nranks, int flags);

/* The same distributed step with the exchanges issued by the library itself: RCCL calls on the
 * handle's stream between the four stages, no host language in the loop. RCCL is bound at run
 * time (dlopen), a single-GPU process never loads it.
 *   qgcm_hip_comm_unique_id : rank 0 obtains the QGCM_HIP_COMM_ID_BYTES-byte rendezvous id and hands
 *                             it to the other ranks by whatever the host has (MPI_Bcast, torch.distributed)
 *   qgcm_hip_comm_init      : collective over the nranks handles (one process per GPU); rank r must own the
 *                             r-th slab (slab_g0/slab_g1 of qgcm_hip_params); allocates the exchange buffers
 *   qgcm_hip_slab_steps     : n whole steps from step s0 (collective). Per step: all-gather of the slab
 *                             summaries (3*nlo*ldw doubles) and the edge rows (3 of po + 1 of qo per layer) to
 *                             both neighbours as one all-gather, or as send/recv with QGCM_HIP_HALO_P2P=1.
 *                             QGCM_HIP_SLAB_GRAPH=1 replays 50-step HIP graphs that contain the collectives.
 * The communicator is released by qgcm_hip_destroy. */
#define QGCM_HIP_COMM_ID_BYTES 128
int qgcm_hip_comm_unique_id(char *id, int nbytes);
int qgcm_hip_comm_init(qgcm_hip_handle h, const char *id, int nbytes, int rank, int nranks);
int qgcm_hip_slab_steps(qgcm_hip_handle h, int s0, int n);
/* edge rows as grouped send/recv with the two neighbours (1) or as one all-gather (0); collective:
 * every rank must make the same choice */
int qgcm_hip_comm_set_halo_p2p(qgcm_hip_handle h, int on);
/* on = 1: the halo exchange of step s (and the halo unpack) run on a second stream while the handle's stream already
 * computes the tile rows of step s+1's tendency launch that need no halo row (stage 4); the outer tile rows follow
 * the halo rows on that second stream (stage 6), the handle's stream waits for them and goes on (stage 7).  Bitwise the same results.  Steps followed by a leapfrog averaging, the mixed layer and slabs of fewer
 * than three 16-row tile rows keep the plain order.  Collective choice, like the one above. */
int qgcm_hip_comm_set_overlap(qgcm_hip_handle h, int on);
/* measurement aid (collective): the step's exchanges back to back, microseconds each:
 * us[0] summaries all-gather, us[1] halo rows as all-gather, us[2] halo rows as send/recv */
int qgcm_hip_comm_probe(qgcm_hip_handle h, int reps, double *us);

/* ---- the coupled window on a y-slab ocean, driven by the library ------------------------------------------
 * What SlabOcean.coupled_steps issues call by call - xforc in the mode set up with its one or two all-gathers, the
 * mixed layer's two halves, the four stages of the slab step, the replica's atmospheric steps - issued from here: every
 * collective an RCCL call on the slab's stream, every dependency between the slab's stream and the replica's an event,
 * no host wait.  The order exists once, as a plan of (code, doubles per rank) pairs:
 *
 * qgcm_hip_slab_coupled_plan(sw, nranks, nt0, n, nstr, xforc, cap, codes, lens, count): host code without a handle or a
 *   device, a pure function of its arguments.  sw: the switches and the message lengths of the run.  Writes the window's
 *   operations in order into codes[] / lens[] (cap entries each; NULL with cap = 0 only counts) and their number into
 *   *count; lens[k] is the doubles per rank an exchange moves (HALO_GATHER: both edge messages, HALO_P2P: one of them)
 *   and 0 for everything else.  The plan does not depend on the rank: ranks that pass the same arguments issue the same
 *   collectives with the same lengths in the same order.  Refuses a bad step range, nranks < 1, an exchange of the
 *   chosen mode with a length < 1, udiff_sums together with bands or udiff_gather, and cap < *count (after setting it).
 * qgcm_hip_slab_coupled_init(oc, atm): after qgcm_hip_comm_init(oc), qgcm_hip_xforc_slab_init(oc, atm) and whichever of
 *   _heat_slab_init, _slab_bands, _slab_udiff, _slab_sums, qgcm_hip_oml_init, qgcm_hip_aml_init the run uses.  Allocates
 *   the exchange buffers of xforc's all-gathers (qgcm_hip_xforc_slab_msg_len, _pom_len, _edge_len doubles per rank; the
 *   step's and the mixed layer's are the communicator's), owned by the slab's handle and released by qgcm_hip_destroy.
 *   Refuses, by name: handles on different devices, an atmosphere not set up for this slab, a missing communicator, a
 *   handle with qgcm_hip_comm_set_overlap on (the window runs the plain stage order).  Call it again after a set-up call
 *   changed the mode; qgcm_hip_slab_coupled_steps refuses when the lengths no longer match.
 * qgcm_hip_slab_coupled_steps(oc, atm, nt0, n, nstr, xforc): collective.  n atmospheric steps nt = nt0 .. on the replica
 *   with one slab ocean step before every nt with mod(nt, nstr) == 1 (src/q-gcm.F:1220-1268; nstr = 1 never steps the
 *   ocean), xforc != 0: xforc before each ocean step.  It executes qgcm_hip_slab_coupled_plan's sequence for the handles'
 *   own switches and lengths; the leapfrog averaging follows every 25th ocean step, the atmosphere's every 100th of its
 *   own, as in qgcm_hip_steps.  Asynchronous like qgcm_hip_slab_steps: it returns with the work queued.  The replica's
 *   steps wait only for what xforc left them, so they may run beside the ocean step; the results do not depend on it. */
enum {
  QGCM_HIP_CPL_XF_EDGE_PACK = 1,    /* qgcm_hip_xforc_slab_edge_pack */
  QGCM_HIP_CPL_GATHER_EDGE = 2,     /* all-gather, qgcm_hip_xforc_slab_edge_len doubles per rank */
  QGCM_HIP_CPL_XF_EDGE_ASSEMBLE = 3,
  QGCM_HIP_CPL_XF_POM_PACK = 4,     /* qgcm_hip_xforc_slab_pom_pack */
  QGCM_HIP_CPL_GATHER_POM = 5,      /* all-gather, qgcm_hip_xforc_slab_pom_len */
  QGCM_HIP_CPL_XF_POM_ASSEMBLE = 6,
  QGCM_HIP_CPL_XF_PART = 7,         /* qgcm_hip_xforc_slab_part */
  QGCM_HIP_CPL_GATHER_XFORC = 8,    /* all-gather, qgcm_hip_xforc_slab_msg_len */
  QGCM_HIP_CPL_XF_COMBINE = 9,      /* qgcm_hip_xforc_slab_combine */
  QGCM_HIP_CPL_OML_A = 10,          /* slab stage 10 */
  QGCM_HIP_CPL_GATHER_OML = 11,     /* all-gather, qgcm_hip_oml_msg_len */
  QGCM_HIP_CPL_OML_B = 12,          /* slab stage 11 */
  QGCM_HIP_CPL_STAGE1 = 13,         /* slab stage 1 */
  QGCM_HIP_CPL_GATHER_SUMMARY = 14, /* all-gather, qgcm_hip_thomas_msg_len */
  QGCM_HIP_CPL_STAGE2 = 15,         /* slab stage 2 */
  QGCM_HIP_CPL_HALO_GATHER = 16,    /* edge rows as one all-gather, 2 * qgcm_hip_halo_msg_len */
  QGCM_HIP_CPL_HALO_P2P = 17,       /* edge rows as grouped send/recv with the neighbours, qgcm_hip_halo_msg_len each */
  QGCM_HIP_CPL_STAGE3 = 18,         /* slab stage 3 */
  QGCM_HIP_CPL_STAGE3_AVG = 19,     /* slab stage 3 with the leapfrog averaging */
  QGCM_HIP_CPL_ATM_STEP = 20,       /* one atmospheric step on the replica: (aml;) qgastep; atinvq; atqzbd */
  QGCM_HIP_CPL_NCODES = 21
};
typedef struct qgcm_hip_slab_coupled_switches {
  int oml;          /* the ocean mixed layer steps on the slabs (qgcm_hip_oml_init) */
  int heat;         /* xforc's heat half (qgcm_hip_xforc_heat_slab_init) */
  int bands;        /* qgcm_hip_xforc_slab_bands */
  int udiff_gather; /* qgcm_hip_xforc_slab_udiff */
  int udiff_sums;   /* qgcm_hip_xforc_slab_sums */
  int halo_p2p;     /* qgcm_hip_comm_set_halo_p2p */
  long xforc_len, pom_len, edge_len, oml_len, summary_len, halo_len; /* doubles per rank, the calls named above */
} qgcm_hip_slab_coupled_switches;
const char *qgcm_hip_slab_coupled_code_name(int code);
int qgcm_hip_slab_coupled_plan(const qgcm_hip_slab_coupled_switches *sw, int nranks, int nt0, int n, int nstr, int xforc,
                               long cap, int *codes, long *lens, long *count);
int qgcm_hip_slab_coupled_init(qgcm_hip_handle oc_slab, qgcm_hip_handle atm);
int qgcm_hip_slab_coupled_steps(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, int nt0, int n, int nstr, int xforc);

/* ---- ocean mixed layer -----------------------------------
 * `call oml` (src/q-gcm.F:1232; body src/omlsubs.F:47-236 + omladf 244-763) on the device: steps the
 * mixed-layer temperature on the T grid (nxto,nyto) = (nxpo-1,nypo-1), and produces what the PV path
 * consumes - entoc on the p grid, xon(1) and (cyclic) enisoc(1)/eninoc(1) - without leaving the GPU.
 * Only for a handle that owns the whole domain. */
typedef struct qgcm_hip_oml_params {
  double hmoc;         /* mixed layer thickness                 (MODULE intrfac, input.params) */
  double toc1, toc2;   /* toc(1), toc(2)                        (MODULE occonst) */
  double st2d, st4d;   /* Del-sqd / Del-4th sst diffusivities   (MODULE intrfac) */
  double ycexp;        /* sst advection coupling coefficient    (MODULE occonst) */
  double rrcpoc;       /* 1/(rhooc*cpoc), src/q-gcm.F:438       (MODULE radiate) */
  double tsbdy, tnbdy; /* boundary temperatures of the options below */
  int sb_hflux;        /* the reference's cpp options sb_hflux / nb_hflux as run-time flags */
  int nb_hflux;
} qgcm_hip_oml_params;
/* allocates the mixed-layer state and switches it on: qgcm_hip_steps then runs oml before qgostep in
 * every step and averages sst with the other fields (src/q-gcm.F:1345-1351).  On a y-slab handle (arrays = local rows
 * incl. halos, T row j between p rows j and j+1) call it before qgcm_hip_comm_init / before sizing the message buffers;
 * qgcm_hip_slab_steps / the slab stages 10, 11 then step it. */
int qgcm_hip_oml_init(qgcm_hip_handle h, const qgcm_hip_oml_params *p);
/* sst, sstm (MODULE intrfac), dense (nxto,nyto) Fortran order; NULL = leave unchanged / do not fetch */
int qgcm_hip_oml_set_state(qgcm_hip_handle h, const double *sst, const double *sstm);
int qgcm_hip_oml_get_state(qgcm_hip_handle h, double *sst, double *sstm);
/* fnetoc(nxto,nyto) (intrfac), wekto(nxto,nyto) (ocstate), tauxo, tauyo(nxpo,nypo) (intrfac); NULL = unchanged */
int qgcm_hip_oml_set_forcing(qgcm_hip_handle h, const double *fnetoc, const double *wekto,
                             const double *tauxo, const double *tauyo);
int qgcm_hip_oml(qgcm_hip_handle h);          /* replaces "call oml", src/q-gcm.F:1232 */
/* entoc(nxpo,nypo) (or NULL) and diag[5] = xon(1), cfraoc, centoc, enisoc(1), eninoc(1); synchronous */
int qgcm_hip_oml_get_diag(qgcm_hip_handle h, double *entoc, double *diag);

/* ---- validity scan -----------------------------------------
 * Ocean part of "call valids (solnok)" (src/q-gcm.F:1278; src/valsubs.F:272-527) on the device: instead of
 * pulling po, qo (44 MB at 5 km) every valday, 14 + nlo doubles and the verdict come back.
 *   out[0..13]  min, max of po, qo, sst, wekto, full layer thickness top / intermediate / bottom
 *   out[14..]   hfbad(1..nlo): per cent of the basin where layer k is thinner than thkmin = 100 m
 *               (evaluated, as in the reference, only when some thickness is <= thkmin; else 0)
 *   *solnok     0 if |po| >= 1e4, |qo| >= 0.05, |sst| >= 75, |wekto| >= 1e-3 or hfbad(k) > 20 (the reference's
 *               limits, src/valsubs.F:78-97), else 1.  sst / wekto are scanned when the mixed layer is
 *               initialised (their entries stay at +/-1e30 otherwise).
 * Bitwise the reference's numbers (min / max / quarter-integer sums are order independent). The
 * neighbourhood print-out of a failing run stays on the host (pull the state, call the reference's valids).
 * qgcm_hip_set_dtopoc: bottom topography dtopoc(nxpo,nypo) of MODULE occonst (NULL = flat). Synchronous. */
int qgcm_hip_set_dtopoc(qgcm_hip_handle h, const double *dtopoc);
int qgcm_hip_valids(qgcm_hip_handle h, double *out, int *solnok);

/* ---- ocean monitors ----------------------------------------
 * The ocean half of "call monnc_comp" (src/monitor_diag.F:479-832 with poref :173-182, del4bx / del4ch, genint) and
 * "call couroc" (:1450-1928) on the device: instead of pulling po, pom, qo every dgnday, qgcm_hip_monitor_len(h) =
 * 19*nlo + 16 doubles come back.  It reads the time levels qgcm_hip_get_state would return at that point (after an
 * averaging step the averaged ones), and changes no state.  Whole-domain ocean handles (y-slabs: below).
 * qgcm_hip_set_mon_params: the constants the handle does not hold (dto = tdto/2 and the rest of MODULE occonst are
 *   derived from qgcm_hip_params as src/q-gcm.F:414-436 does).
 * qgcm_hip_set_monitor_fields: tauxo, tauyo (nxpo,nypo) (intrfac), wekto (nxto,nyto) (ocstate), sst (nxto,nyto)
 *   (intrfac): the fields that do not evolve on the device without the mixed layer.  NULL = leave unchanged.  With the
 *   mixed layer on (qgcm_hip_oml_init) the monitors read its own stress, wekto and sst instead.  Without it,
 *   qgcm_hip_monitors fails, naming the field, if one was never given.  Synchronous.
 * qgcm_hip_monitors: out, in this order (names of MODULE monitor, src/monitor_data.F:50-71):
 *     wetmoc, watmoc, wepmoc, wapmoc, entmoc, enamoc
 *     etamoc(nlo-1), et2moc(nlo-1), ddtpeoc(nlo-1), pkenoc, utauoc
 *     pavgoc, qavgoc, ah2doc, ah4doc, kealoc, ddtkeoc, osfmin, osfmax, occirc, ocjpos, ocjval   (nlo each)
 *     btdgoc, sstmin, sstmax, tmlmoc, hfmloc, occtot
 *     umminoc, ummaxoc, vmminoc, vmmaxoc, cnmloc                                                (couroc, mixed layer)
 *     ugminoc, ugmaxoc, vgminoc, vgmaxoc, cnqgoc                                                (nlo each)
 *   Extrema, the transports and the jet position and value (serial zonal sums, as in the reference) use the reference's
 *   expressions uncontracted and are bitwise the golden values of the reference build (tests/golden/mon_*.npz);
 *   the genint integrals agree to rounding (another summation order).  All of it is bitwise reproducible from call
 *   to call.  Runs on the handle's stream; synchronous. */
typedef struct qgcm_hip_mon_params {
  double rhooc, cpoc;   /* ocean density, specific heat              (MODULE occonst) */
  double hmoc, ycexp;   /* mixed layer thickness, sst advection coupling (couroc's mixed layer: intrfac, occonst) */
  int sb_hflux;         /* the reference's cpp options sb_hflux / nb_hflux (couroc's mixed layer at the */
  int nb_hflux;         /* southern / northern boundary) as run-time flags */
} qgcm_hip_mon_params;
int qgcm_hip_monitor_len(qgcm_hip_handle h);
int qgcm_hip_set_mon_params(qgcm_hip_handle h, const qgcm_hip_mon_params *p);
int qgcm_hip_set_monitor_fields(qgcm_hip_handle h, const double *tauxo, const double *tauyo, const double *wekto,
                                const double *sst);
int qgcm_hip_monitors(qgcm_hip_handle h, double *out);

/* ---- the three diagnostics on y-slabs: per-rank summary, one all-gather, combine ----------------------------
 * qgcm_hip_monitors, qgcm_hip_valids and qgcm_hip_prsamp refuse y-slab handles.  On slabs each rank writes a
 * fixed-size summary of the rows it owns into a device buffer (_part), the caller all-gathers the summaries (rank r's
 * at r * len, as comm.all_gather produces them) and every rank combines the gathered buffer (_combine): bitwise the
 * same result on every rank, in the layout of the whole-domain call.
 *   Ownership: p rows g0..g1 of the slab (local jlo..jhi); T rows g0..g1, or g0..g1-1 on the rank that owns row
 *   nypo.  Every boundary rule (genint's edge weights, del4bx's one-sided forms, couroc's sb_hflux / nb_hflux rows,
 *   the trapezoid weights) uses global rows.  Del-4th of ugoc / vgoc at an owned row reads pom up to 3 rows beyond
 *   the owned ones: the halo rows must be current (they are between the slab step calls).
 *   _part_len(h): doubles per summary.  _part(h, send_dev): asynchronous on the handle's stream, like
 *   qgcm_hip_thomas_phase.  _combine(h, gath_dev, nranks, ...): synchronous; fails when the gathered g0, g1 do not
 *   tile rows 1..nypo in rank order.  On a whole-domain handle _part + _combine with nranks = 1 work as well.
 *   Extrema, ocjpos / ocjval, osfmin / osfmax, occirc and everything of valids are bitwise the whole-domain values;
 *   the integrals (sums over the ranks in rank order) agree to rounding.
 * Summary layouts (nl = nlo; "rows" = the global rows g0, g1 as doubles):
 *   monitors  sums (13*(nl+1)) | minima, maxima negated (7*(nl+1)) | per layer the largest ujeto of the owned T rows
 *             (nl) | its global T row, first occurrence, 0 = none (nl) | po(1,g0,k) (nl) | po(1,g1,k) (nl) | g0, g1
 *             = 24*nl + 22 doubles.  The combine keeps a later rank's jet only if it is strictly larger.
 *   valids    min / max as out[0..13] of qgcm_hip_valids | thin-point weights (nl) | g0, g1  = 16 + nl doubles
 *   prsamp    po, qo at the basin centre (nl each; 0 on the ranks that do not own row (nypo+1)/2) | xintp of po, qo
 *             over the owned rows (nl each) | min, max of sst (+-1e30 without the mixed layer) | 1 if the rank owns
 *             the centre row | g0, g1  = 4*nl + 5 doubles
 * qgcm_hip_set_monitor_fields and qgcm_hip_set_dtopoc take a slab's local rows, halo rows included (as
 * qgcm_hip_oml_set_forcing). */
int qgcm_hip_monitor_part_len(qgcm_hip_handle h);
int qgcm_hip_monitors_part(qgcm_hip_handle h, double *send_dev);
int qgcm_hip_monitors_combine(qgcm_hip_handle h, const double *gath_dev, int nranks, double *out);
int qgcm_hip_valids_part_len(qgcm_hip_handle h);
int qgcm_hip_valids_part(qgcm_hip_handle h, double *send_dev);
int qgcm_hip_valids_combine(qgcm_hip_handle h, const double *gath_dev, int nranks, double *out, int *solnok);
int qgcm_hip_prsamp_part_len(qgcm_hip_handle h);
int qgcm_hip_prsamp_part(qgcm_hip_handle h, double *send_dev);
int qgcm_hip_prsamp_combine(qgcm_hip_handle h, const double *gath_dev, int nranks, double *out);

/* ---- atmosphere monitors and valids -----------------------------------------------------------
 * The atmosphere half of "call monnc_comp" (src/monitor_diag.F:160-172, 185-475 with del4ch and genint), "call courat"
 * (:1213-1444) and the atmospheric half of "call valids" (src/valsubs.F:120-269) on an atmosphere handle
 * (qgcm_hip_params.atmos = 1) that owns the whole domain.  They read pa, pam, qa at the time levels qgcm_hip_get_state
 * would return (after an averaging step the averaged ones), wekpa and entat of qgcm_hip_set_forcing and the fields
 * below, and change no state.  dta = tdta/2, gpat, hat, ah4at, rdxaf0, hdxam1 and atnorm = 1/(nxta*nyta) come from
 * qgcm_hip_params.  Every entry point refuses an ocean handle and a y-slab handle, naming which.
 * qgcm_hip_set_atm_mon_params: the constants the handle does not hold (struct below); fails when the ocean's cells
 *   do not lie on the atmosphere's T grid.
 * qgcm_hip_set_atm_monitor_fields: what xforc / aml leave in MODULE intrfac / atstate on the host: wekta, ast, hmixa
 *   (nxta,nyta), tauxa, tauya (nxpa,nypa), uekat (nxpa,nyta), vekat (nxta,nypa).  NULL = leave unchanged.  Synchronous.
 * qgcm_hip_atm_monitor_len(h) = 18*nla + 11 (-1 for an ocean handle).  qgcm_hip_atm_monitors(h, out) fails,
 *   naming what is missing, before qgcm_hip_set_atm_mon_params or when one of the seven fields was never given.
 *   Out, in this order (names of MODULE monitor, src/monitor_data.F):
 *     wetmat, watmat, wepmat, wapmat
 *     entmat(nla-1), enamat(nla-1), etamat(nla-1), et2mat(nla-1), ddtpeat(nla-1), pkenat(nla-1)
 *     utauat
 *     pavgat(nla), qavgat(nla), ah4dat(nla), kealat(nla), ddtkeat(nla), atstpos(nla), atstval(nla)
 *     tmlmat, hmlmat, astmin, astmax, hcmlat, tmaooc, olrtop
 *     umminat, ummaxat, vmminat, vmmaxat, cnmlat                                   (courat, mixed layer)
 *     ugminat(nla), ugmaxat(nla), vgminat(nla), vgmaxat(nla), cnqgat(nla)        (courat, Q-G layers)
 *   As the reference writes them: ddtpeat without the atnorm factor, entmat / enamat / pkenat zero beyond interface 1,
 *   vkedot (in ddtkeat) the integral of Del-sqd(lagged v).  Extrema, Courant numbers, atstpos / atstval (serial
 *   zonal sums) and tmaooc (serial sum) are bitwise the reference's; the genint integrals agree to rounding.  Bitwise
 *   reproducible from call to call.  Runs on the handle's stream; synchronous.
 * qgcm_hip_atm_valids(h, out, solnok): out[12] = min, max of pa, qa, ast, wekta, tauxa, tauya (bitwise);
 *   *solnok = 0 if |pa| >= 1e7, |qa| >= 0.05, |ast| >= 90, |wekta| >= 1, |tauxa| or |tauya| >= 10 (the reference's
 *   limits), else 1.  Needs wekta, tauxa, tauya, ast.  The neighbourhood print-out stays on the host.  Synchronous. */
typedef struct qgcm_hip_atm_mon_params {
  double rhoat, cpat;       /* atmospheric density, specific heat          (MODULE atconst) */
  double hmat, davgat;      /* fixed mixed layer depth, mean topography    (MODULE atconst) */
  double aup[QGCM_HIP_MAXL - 1]; /* Aup(nla, 1..nla-1)                     (MODULE radiate) */
  double bup, cup, dup;     /* Bup(nla), Cup(nla), Dup(nla)                (MODULE radiate) */
  int nx1, ny1;             /* first atmosphere T cell above the ocean     (MODULE parameters) */
  int nxaooc, nyaooc;       /* atmosphere T cells above the ocean          (MODULE parameters) */
} qgcm_hip_atm_mon_params;
int qgcm_hip_set_atm_mon_params(qgcm_hip_handle h, const qgcm_hip_atm_mon_params *p);
int qgcm_hip_set_atm_monitor_fields(qgcm_hip_handle h, const double *wekta, const double *tauxa, const double *tauya,
                                    const double *ast, const double *hmixa, const double *uekat, const double *vekat);
int qgcm_hip_atm_monitor_len(qgcm_hip_handle h);
int qgcm_hip_atm_monitors(qgcm_hip_handle h, double *out);
int qgcm_hip_atm_valids(qgcm_hip_handle h, double *out, int *solnok);

/* ---- start-up / restart arithmetic and the progress sample on the device ------------
 * qgcm_hip_init_from_p: the start-up sequence of the main program (src/q-gcm.F:711-731; atmosphere :738-749) from
 *   the po, pom ALREADY on the device (qgcm_hip_set_state with qo = qom = NULL, e.g. after a restart read):
 *   constr (dpioc, dpiocp and, cyclic / atmosphere, ocncs, ocncn, ocncsp, ocncnp: src/conhoms.F:93-300), qcomp
 *   (src/vorsubs.F:49-138), ocqbdy / atqzbd, merqcy (src/vorsubs.F:142-239) for both time levels.  qcomp / merqcy /
 *   ocqbdy are bitwise the reference; the constraint integrals agree to rounding (parallel sums).
 * qgcm_hip_wekpo_from_tau: ocean-only Ekman pumping from the wind stress tauxo, tauyo (nxpo,nypo) - wekto on the
 *   T grid and its p-grid average wekpo (src/xfosubs.F:138, 566-645) - into the forcing the path reads (and
 *   into the mixed layer's wekto / stress once qgcm_hip_oml_init was called).  Synchronous.
 * qgcm_hip_prsamp: the ocean numbers of the progress print-out prsamp (src/q-gcm.F:1933-2066) without pulling the
 *   state: out = po(k), qo(k) at the basin centre ((nxpo+1)/2, (nypo+1)/2), the layer averages pavgoc(k), qavgoc(k)
 *   (src/monitor_diag.F:729-739), then min, max of sst (+-1e30 without the device mixed layer): 4*nlo + 2 doubles.
 *   Synchronous. */
int qgcm_hip_init_from_p(qgcm_hip_handle h);
int qgcm_hip_wekpo_from_tau(qgcm_hip_handle h, const double *tauxo, const double *tauyo);
int qgcm_hip_prsamp(qgcm_hip_handle h, double *out);

/* ---- time averages of the ocean -----------------------------------------------------------------
 * Running mean of po (the fork's -Docnc_avg_k247: avg_ocn_k247, src/timavge.F:624-662; ocnc_avgout_k247,
 * src/nc_subs.F:1944-2052):
 * qgcm_hip_poavg_enable(h, on): on = 1 starts a sum at zero (unless it is on already); while it is on, every step of
 *   qgcm_hip_steps (graphs included) and every slab stage 2 (qgcm_hip_slab_steps) adds the step's new po - after
 *   ocqbdy, BEFORE the step's leapfrog averaging - and counts it.  on = 0 stops adding; the sum stays readable.  Off
 *   (the default), the step's launches are exactly those without this feature.
 * qgcm_hip_poavg_out(h, po_avg, nsum, reset): po_avg (nxpo, rows, nlo) = rnsum * sum with rnsum = 1/nsum (the
 *   reference's one reciprocal, then a multiply; fails when nothing has been summed); NULL = do not fetch.  *nsum
 *   (may be NULL) = the count.  reset != 0 then zeroes sum and count.  Synchronous.
 * tavocn / tavout, ocean half (src/timavge.F:425-619, 667-880):
 * qgcm_hip_set_tav_params: hmoc, ycexp, tsbdy, tnbdy and the sb_hflux / nb_hflux branches of tavocn.  Without it the
 *   mixed layer's parameters are used (qgcm_hip_oml_init); with neither, qgcm_hip_tavocn fails.
 * qgcm_hip_set_tav_fields: fnetoc (nxto,nyto) for a handle without the mixed layer (zero if never given; with the
 *   mixed layer on, its own fnetoc is read).  tauxo, tauyo, wekto, sst come from the mixed layer when it is on, else
 *   from qgcm_hip_set_monitor_fields, as for the monitors.  NULL = unchanged.  Synchronous.
 * qgcm_hip_tavocn(h): adds one contribution from the state on the device (the time levels qgcm_hip_get_state would
 *   return, i.e. after a step's averaging) and counts it; asynchronous.
 * qgcm_hip_tav_reset(h): tavini - zeroes the sums and the count.
 * qgcm_hip_tav_out(h, fields, nsumoc): tavout's arithmetic (rnsoc = 1/nsumoc, 0 when nsumoc = 0) into
 *   fields[0 .. QGCM_HIP_TAV_NOUT-1], dense Fortran order, NULL = skip (only requested fields are computed and
 *   copied): txocav, tyocav, wpocav (nxpo,nypo) | wtocav, fmocav, sstav (nxto,nyto) | pocav, qocav (nxpo,nypo,nlo) |
 *   uufo, tufo, utufo (nxpo,nyto) | vvfo, tvfo, vtvfo (nxto,nypo) | uptpoc (nxpo,nyto) | vptpoc (nxto,nypo).  The sums
 *   are not changed.  *nsumoc (may be NULL) = the count.  Synchronous.
 * On a y-slab handle every call acts on the owned rows: p rows g0..g1, T rows g0..g1 (g0..g1-1 on the rank that owns
 * row nypo); the outputs have that many rows.  The flux terms at a slab edge read the halo rows of po, tauyo and sst,
 * which are current between slab steps.  Bitwise the reference's arithmetic (elementwise, uncontracted). */
#define QGCM_HIP_TAV_NOUT 16
typedef struct qgcm_hip_tav_params {
  double hmoc, ycexp;   /* mixed layer thickness, sst advection coupling (intrfac, occonst) */
  double tsbdy, tnbdy;  /* boundary temperatures of the options below (intrfac) */
  int sb_hflux;         /* the reference's cpp options sb_hflux / nb_hflux as run-time flags */
  int nb_hflux;
} qgcm_hip_tav_params;
int qgcm_hip_poavg_enable(qgcm_hip_handle h, int on);
int qgcm_hip_poavg_out(qgcm_hip_handle h, double *po_avg, int *nsum, int reset);
int qgcm_hip_set_tav_params(qgcm_hip_handle h, const qgcm_hip_tav_params *p);
int qgcm_hip_set_tav_fields(qgcm_hip_handle h, const double *fnetoc);
int qgcm_hip_tavocn(qgcm_hip_handle h);
int qgcm_hip_tav_reset(qgcm_hip_handle h);
int qgcm_hip_tav_out(qgcm_hip_handle h, double *const *fields, int *nsumoc);

/* ---- periodic ocean dumps ------------------------------------------------------------------------------
 * The reference's qocdiag_out (src/qocdiag.F:303-687) and ocnc_out (src/nc_subs.F:837-1072), called at every
 * mod(ntdone,noutoc) == 0, at the subsampled points (1+(i-1)*nsko, 1+(j-1)*nsko); a subsample of n points has
 * min(mod(n,nsko),1) + (n-mod(n,nsko))/nsko of them (ipwk, jpwk on the p grid, itwk, jtwk on the T grid).
 * qgcm_hip_qocdiag_len(h, nsko): the doubles qgcm_hip_qocdiag writes (-1 on error).
 * qgcm_hip_qocdiag(h, nsko, out): the vorticity budget from the state on the device - po, pom, qo, qom, the forcing's
 *   wekpo and the entoc on the device - as out[term][k][jp][ip] (ip fastest; terms dqdt, qotjac, qt2dif, qt4dif,
 *   qotent; per layer exactly what the reference hands nf_put_vara_double).  qt2dif is always produced (zero when every
 *   ah2oc is 0; the reference then skips writing it).  Equals the reference's dump when called between qgcm_hip_oml
 *   and qgcm_hip_qgostep, or at any time with the mixed layer off.  Synchronous.
 * qgcm_hip_qocdiag_schedule(h, nsko, every, capacity): while set, qgcm_hip_steps records the budget of every step s
 *   with (s-1) % every == 0 after the step's oml and before its tendency (the reference's mod(ntdone,noutoc) == 0 with
 *   ntdone = s-1, every = noutoc/nstr) into a device ring of `capacity` snapshots of qgcm_hip_qocdiag_len doubles.  A
 *   qgcm_hip_steps call that would record more snapshots than the ring has free fails before it launches anything.
 *   every = 0 removes the schedule and frees the ring.  Whole-domain handles only.  Other steps issue the launches of a
 *   run without a schedule, and the state is bitwise the same.
 * qgcm_hip_qocdiag_read(h, out, steps_out, max, nread): the unread snapshots, oldest first, at most max of them, into
 *   out (consecutive snapshots) and their step numbers into steps_out (may be NULL); frees them; *nread = how many.
 *   max <= 0: *nread = the number unread, nothing is copied.  Synchronous.
 * qgcm_hip_ocnc_sample_len(h, nsko, outfloc) / qgcm_hip_ocnc_sample(h, nsko, outfloc, out): ocnc_out's fields, the
 *   selected ones concatenated in its order: sst (itwk, jtwk) | po (ipwk, jpwk, nlo) | qo (ipwk, jpwk, nlo) |
 *   wekto (itwk, jtwk) | h = (po(k+1)-po(k))/gpoc(k) (ipwk, jpwk, nlo-1) | tauxo, tauyo (ipwk, jpwk each).  outfloc is the
 *   reference's 7-flag vector (1 = write; outfloc(6) selects tauxo and tauyo, outfloc(7) is not read).  sst, wekto,
 *   tauxo and tauyo come from the mixed layer when it is on, else from qgcm_hip_set_monitor_fields (the call fails,
 *   naming the field, if a requested one was never given).  Synchronous.
 * qgcm_hip_subsample_rows(h, nsko, mp0, mp1, mt0, mt1): on a y-slab handle the calls above compute the subsample rows
 *   [mp0, mp1) of the p grid and [mt0, mt1) of the T grid (0-based: global row 1 + m*nsko) that the rank owns (T rows
 *   as the slab monitors own them); a whole-domain handle gets [0, jpwk) and [0, jtwk).  NULL = not wanted.
 * Bitwise the reference's arithmetic (-ffp-contract=off); every boundary rule uses global rows. */
long qgcm_hip_qocdiag_len(qgcm_hip_handle h, int nsko);
int qgcm_hip_qocdiag(qgcm_hip_handle h, int nsko, double *out);
int qgcm_hip_qocdiag_schedule(qgcm_hip_handle h, int nsko, int every, int capacity);
int qgcm_hip_qocdiag_read(qgcm_hip_handle h, double *out, int *steps_out, int max, int *nread);
long qgcm_hip_ocnc_sample_len(qgcm_hip_handle h, int nsko, const int *outfloc);
int qgcm_hip_ocnc_sample(qgcm_hip_handle h, int nsko, const int *outfloc, double *out);
int qgcm_hip_subsample_rows(qgcm_hip_handle h, int nsko, int *mp0, int *mp1, int *mt0, int *mt1);

/* ---- time averages and periodic dump of the atmosphere --------------------------------------------------
 * tavatm / tavout, atmosphere half (src/timavge.F:278-421, 715-801), and atnc_out (src/nc_subs.F:1077-1326) on an
 * atmosphere handle (qgcm_hip_params.atmos = 1).  They read pa, qa at the time levels qgcm_hip_get_state would return
 * (after an averaging step the averaged ones), tauxa, tauya, wekta, ast, hmixa of qgcm_hip_set_atm_monitor_fields, hmat
 * of qgcm_hip_set_atm_mon_params, gpat and rdxaf0 = 1/(dxa*fnot) from qgcm_hip_params.  Every entry point refuses an
 * ocean handle; the ocean's qgcm_hip_tavocn / _tav_out / _tav_reset / _set_tav_fields refuse an atmosphere handle.
 * qgcm_hip_set_atm_tav_fields(h, fnetat): fnetat (nxta,nyta) of MODULE intrfac.  NULL = leave unchanged.  Synchronous.
 * qgcm_hip_tavatm(h): adds one contribution to the 14 sums and counts it (nsumat); asynchronous.  Fails, naming what is
 *   missing, before qgcm_hip_set_atm_mon_params (hmat), before tauxa, tauya, wekta, ast were given, or before fnetat.
 * qgcm_hip_atm_tav_reset(h): tavini's atmosphere half - zeroes the sums and the count.
 * qgcm_hip_atm_tav_out(h, fields, nsumat): tavout's arithmetic (rnsat = 1/nsumat, 0 when nsumat = 0) into
 *   fields[0 .. QGCM_HIP_ATM_TAV_NOUT-1], dense Fortran order, NULL = skip (only requested means are computed and
 *   copied): txatav, tyatav (nxpa,nypa) | wtatav, fmatav, astav (nxta,nyta) | patav, qatav (nxpa,nypa,nla) |
 *   uufa, tufa, utufa (nxpa,nyta) | vvfa, tvfa, vtvfa (nxta,nypa) | uptpat (nxpa,nyta) | vptpat (nxta,nypa).  The sums
 *   are not changed.  *nsumat (may be NULL) = the count.  Synchronous.
 * qgcm_hip_tavatm_schedule(h, every, phase): while set, qgcm_hip_steps and qgcm_hip_coupled_steps add one contribution
 *   after every atmospheric step nt with nt % every == phase - after the step's own averaging at mod(nt-1,100) == 0, as
 *   the reference orders them (src/q-gcm.F:1370-1405 before 1477-1479) - and count it like an explicit call: the result
 *   is that of qgcm_hip_tavatm between two windows that end at nt.  The reference's cadence is every = ntavat,
 *   phase = mod(nmidat + nsteps0, ntavat).  Inside a coupled window the forcing is held: a scheduled contribution reads
 *   the fields as they were last set.  A call whose steps hold a contribution fails before it launches anything when an
 *   input is missing.  Graph blocks end after scheduled steps; the contribution is launched on the handle's stream
 *   between replays (never captured) and the step kernels are those of a run without a schedule (qgcm_hip_prepare_steps
 *   / _time_steps cut in the same places; qgcm_hip_profile_steps counts one k_tavat_accum launch per scheduled step).
 *   every = 0 removes the schedule (the default: launches and graphs are then exactly those without this feature).
 *   Refuses every < 0 and phase outside [0, every).
 * qgcm_hip_atnc_sample_len(h, nska, outflat) (-1 on error) / qgcm_hip_atnc_sample(h, nska, outflat, out): atnc_out's
 *   fields at the points (1+(i-1)*nska, 1+(j-1)*nska), the selected ones concatenated in its order, each plane with i
 *   fastest, as the reference hands nf_put_vara_double: ast (itwk, jtwk) | pa (ipwk, jpwk, nla) | qa (ipwk, jpwk, nla) |
 *   wekta (itwk, jtwk) | ha = (pa(k)-pa(k+1))/gpat(k) (ipwk, jpwk, nla-1) | tauxa, tauya (ipwk, jpwk each) | hmixa
 *   (itwk, jtwk).  outflat is the reference's 7-flag vector (1 = write; outflat(6) selects tauxa and tauya).  A grid of
 *   n points has min(mod(n,nska),1) + (n-mod(n,nska))/nska of them.  Refuses nska < 1, a NULL outflat and a selected
 *   field that was never given (unselected ones need not be set).  Synchronous.
 * Bitwise the reference's arithmetic (elementwise, uncontracted). */
#define QGCM_HIP_ATM_TAV_NOUT 15
int qgcm_hip_set_atm_tav_fields(qgcm_hip_handle h, const double *fnetat);
int qgcm_hip_tavatm(qgcm_hip_handle h);
int qgcm_hip_atm_tav_reset(qgcm_hip_handle h);
int qgcm_hip_atm_tav_out(qgcm_hip_handle h, double *const *fields, int *nsumat);
int qgcm_hip_tavatm_schedule(qgcm_hip_handle h, int every, int phase);
long qgcm_hip_atnc_sample_len(qgcm_hip_handle h, int nska, const int *outflat);
int qgcm_hip_atnc_sample(qgcm_hip_handle h, int nska, const int *outflat, double *out);

/* ---- covariance matrices ---------------------------------------------------------------------------------
 * covini / covocn / covatm of src/covaria_diag.F (-Dget_covar) on the handle's fluid: an ocean handle subsamples
 * po(:,:,1) with psampl and sst with tsampl (covocn), an atmosphere handle pa(:,:,1) and ast (covatm); each vector then
 * goes through dssp (Algorithm AS 41, wt = 1): mean update and rank-1 update of a packed lower triangle of
 * nmat = nvar(nvar+1)/2 entries, nvar = (nxt/nsi)*(nyt/nsi).  Packed index k = i(i+1)/2 + j (0-based, j <= i), the
 * reference's i(i-1)/2 + j less one.  Lengths and indices are 64-bit.  Bitwise the reference's arithmetic.
 * qgcm_hip_cov_init(h, nsi, rank, nranks): covini for this handle: allocates and zeroes two matrices (only the packed
 *   rows this rank holds), two means and the counts.  nsi = 0 frees everything (the schedule too).  Refuses nsi < 2 and
 *   an nsi that does not divide nxto and nyto (nxta, nyta), the rule of src/parameters_data.F:126-127.  A whole-domain
 *   handle is rank 0 of 1; rank r of nranks y-slabs holds matrix rows [i_r, i_{r+1}), i_r the smallest i with
 *   i(i+1)/2 >= floor(r*nmat/nranks) (whole rows, balanced by element count; together they tile [0, nmat)).  A failed
 *   allocation fails with its byte count.  QGCM_HIP_COV_NT=1 in the environment at this call selects non-temporal
 *   loads and stores in the rank-1 update (the same numbers).
 * qgcm_hip_cov_size(h, &nvar, &nmat, &k0, &k1): the sizes and the packed range [k0, k1) this handle holds (NULL = skip).
 * qgcm_hip_cov_add(h): one covocn / covatm (whole-domain handles) from the state at the time levels
 *   qgcm_hip_get_state returns; sst comes from the device mixed layer when it is on, else from
 *   qgcm_hip_set_monitor_fields; ast from qgcm_hip_set_atm_monitor_fields.  Fails, naming the field, when one was never
 *   given.  Asynchronous.
 * qgcm_hip_cov_reset(h): covini again on the same sizes (matrices, means and counts to zero).
 * qgcm_hip_cov_out(h, which, avg, swt, nunit, k0, count, cov): which = 0: p (avgpo / swtpo / nupo / covpo, or the
 *   atmosphere's pa names), 1: T (sst / ast).  avg (nvar), swt, nunit and the packed entries k0 .. k0+count-1 (must lie
 *   in this handle's range) into cov; any pointer may be NULL.  Synchronous.
 * qgcm_hip_cov_schedule(h, every, phase): while set, qgcm_hip_steps and qgcm_hip_coupled_steps add one contribution
 *   after every step s with s % every == phase, after the step's averaging and after a scheduled tavatm contribution of
 *   the same step (src/q-gcm.F:1477-1489).  The reference's cadence: atmosphere (steps nt) every = ntcovat,
 *   phase = mod(nsteps0, ntcovat); ocean (ocean steps s, nt = 1 + (s-1)*nstr, in plain and coupled windows alike)
 *   every = ntcovoc/nstr, phase = mod((nsteps0 + nstr - 1)/nstr, every): covocn at nt reads the state of the last
 *   ocean step at or before nt.  Graph blocks end after scheduled steps; the contribution is launched between replays
 *   (never captured), and qgcm_hip_profile_steps counts one "k_cov" per contribution.  every = 0 removes the schedule
 *   (launches and graphs are then exactly those without this feature).  A window whose steps hold a contribution fails
 *   before it launches anything when an input is missing.  Refuses y-slab handles, every < 0 and phase outside
 *   [0, every).
 * y-slabs: qgcm_hip_cov_part_len(h) (-1 on error) = doubles of one rank's row sums (the same on every rank);
 *   qgcm_hip_cov_part(h, send_dev) writes this rank's row sums (asynchronous); after an all-gather of the parts in
 *   rank order, qgcm_hip_cov_combine(h, gath_dev, nranks) forms the whole-domain vectors and means on every rank
 *   (bitwise those of a whole-domain handle) and updates the rows this rank holds.  It waits for the combine and fails
 *   when the gathered row ranges do not tile the rows. */
int qgcm_hip_cov_init(qgcm_hip_handle h, int nsi, int rank, int nranks);
int qgcm_hip_cov_size(qgcm_hip_handle h, long *nvar, long *nmat, long *k0, long *k1);
int qgcm_hip_cov_add(qgcm_hip_handle h);
int qgcm_hip_cov_reset(qgcm_hip_handle h);
int qgcm_hip_cov_out(qgcm_hip_handle h, int which, double *avg, double *swt, long *nunit, long k0, long count, double *cov);
int qgcm_hip_cov_schedule(qgcm_hip_handle h, int every, int phase);
long qgcm_hip_cov_part_len(qgcm_hip_handle h);
int qgcm_hip_cov_part(qgcm_hip_handle h, double *send_dev);
int qgcm_hip_cov_combine(qgcm_hip_handle h, const double *gath_dev, int nranks);

/* ---- area averages and the CFL check: areavg and cfltry ------------------------------------------
 * "call areavg" (src/areasubs_diag.F:50-677, cpp option get_areav) and "call cfltry" (src/q-gcm.F:2121-2440) on the
 * device, for an ocean handle (sst; po, tauxo, tauyo, hmoc) or a whole-domain atmosphere handle (ast; pa, uekat,
 * vekat).  Both read the levels qgcm_hip_get_state / _oml_get_state / _aml_get_state would return at that point (after
 * an averaging step the averaged ones) and change no state; a handle that never calls them runs exactly as before.
 * The fields are the ones the monitors read: the mixed layer's own sst / ast and stress when it is on, else what
 * qgcm_hip_set_monitor_fields / qgcm_hip_set_atm_monitor_fields gave; uekat, vekat are those xforc writes.
 *
 * qgcm_hip_areavg_init(h, n, i1, i2, j1, j2, facw, face, facs, facn): the finished tables of areavg's first call for
 *   the T grid - 1-based subscripts (global rows, also on a y-slab) and the four boundary weights of n <= 9 areas
 *   (namxoc = namxat = 9); qgcm_hip.hostinit.area_limits restates the reference's arithmetic from the limits in
 *   metres.  Areas may overlap.  Refuses, naming the area and changing nothing: n outside 1..9, a subscript outside
 *   the T grid (the reference's own check), i1 > i2, j1 > j2.  i1 == i2 and j1 == j2 follow areint's formula as
 *   written (west and east weight on the one column, south and north row both contribute).  The denominator of
 *   areint depends on the tables alone: it is formed here, on the host, in the reference's serial order - bitwise
 *   the reference's.  May be called again with other tables.  qgcm_hip_areavg_count(h): n (0 before the set-up).
 * qgcm_hip_areavg(h, avg, num, den): tavoc / tavat (n) of one call of areavg; num, den (n each, may be NULL) are
 *   areint's numerator and denominator.  One pass over the areas' rows, no atomics and a fixed order: bitwise the
 *   same from call to call; the numerator is a sum in another order than areint's and agrees with it to rounding
 *   (2 N 2^-53 sum|terms| for an area of N points).  Fails, naming the field, if sst / ast was never given.
 *   Whole-domain handles; synchronous.
 * qgcm_hip_cfl_len(h) = 2*(nl+1) quantities, in this order: the mixed layer's |u|, |v|, then |u|(k), k = 1..nl, then
 *   |v|(k).  qgcm_hip_cfl(h, cflcrit, maxima, nbad, loc): per quantity the maximum (uabmax / vabmax, uamaxo / vamaxo
 *   and the atmosphere's), the number of lines "Bad ...; CFL, i, j[, k]" the reference would print - the points with
 *   (dt/dx)*|.| >= cflcrit where max*dt/dx >= cflcrit, else 0 - and loc[2q], loc[2q+1] = (i, j) of the maximum, its
 *   first occurrence in the reference's scan order (j outer, i inner).  nbad, loc may be NULL.  cflcrit: the
 *   reference's parameter is 0.8.  The expressions keep the reference's operand order, uncontracted, and maxima,
 *   counts and first locations do not depend on the order of a reduction: all are exact.  The Courant numbers
 *   max*dt/dx are the caller's to form (dt = tdto/2, dx = dxo).  There is no cyclic special case, as in the
 *   reference.  The point-by-point listing itself stays with the host, which pulls the state for a failing run as it
 *   does for valids.  Fails, naming it, if a stress, uekat / vekat or hmoc (qgcm_hip_set_mon_params, else
 *   qgcm_hip_oml_init) was never given.  Whole-domain handles; synchronous.
 * Y-slabs (ocean): the triples of the other diagnostics - _part_len(h) doubles per summary, _part(h, .., send_dev)
 *   asynchronous on the handle's stream, _combine(h, gath_dev, nranks, ..) synchronous, failing when the gathered rows
 *   do not tile the domain in rank order; they also serve a whole-domain ocean with nranks = 1 and refuse an
 *   atmosphere, as the whole-domain calls refuse a y-slab.
 *   areavg  per area the raw sums of rows j1 and j2 (0 on the ranks that do not own them) and the sum of the owned
 *           interior rows (3*9) | the owned global T rows t0, t1  = 29 doubles.  Ownership as above: T rows g0..g1,
 *           g1-1 on the rank that owns row nypo.  The combine adds in rank order, then applies facs / facn and
 *           divides: bitwise the same on every rank, within the reordering bound of the whole-domain value.
 *   cfl     maxima | keys (j-1)*nxpo + (i-1) of their first points, global rows | counts (2*(nl+1) each) | the owned
 *           p rows g0, g1  = 6*(nl+1) + 2 doubles.  The |u| forms read row j+1: a halo row, current between the slab
 *           step calls; the rank that owns row nypo stops at nypo-1.  The combine keeps the largest maximum and among
 *           equal ones the earliest key, and adds the counts: bitwise the whole-domain result. */
int qgcm_hip_areavg_init(qgcm_hip_handle h, int n, const int *i1, const int *i2, const int *j1, const int *j2,
                         const double *facw, const double *face, const double *facs, const double *facn);
int qgcm_hip_areavg_count(qgcm_hip_handle h);
int qgcm_hip_areavg(qgcm_hip_handle h, double *avg, double *num, double *den);
int qgcm_hip_areavg_part_len(qgcm_hip_handle h);
int qgcm_hip_areavg_part(qgcm_hip_handle h, double *send_dev);
int qgcm_hip_areavg_combine(qgcm_hip_handle h, const double *gath_dev, int nranks, double *avg, double *num, double *den);
int qgcm_hip_cfl_len(qgcm_hip_handle h);
int qgcm_hip_cfl(qgcm_hip_handle h, double cflcrit, double *maxima, int *nbad, int *loc);
int qgcm_hip_cfl_part_len(qgcm_hip_handle h);
int qgcm_hip_cfl_part(qgcm_hip_handle h, double cflcrit, double *send_dev);
int qgcm_hip_cfl_combine(qgcm_hip_handle h, const double *gath_dev, int nranks, double cflcrit, double *maxima, int *nbad,
                         int *loc);

/* ---- momentum half of xforc -----------------------------------------------------------------------
 * "call xforc" (src/q-gcm.F:1226) as far as the momentum goes (src/xfosubs.F:137-709): the atmosphere's geostrophic
 * velocity from pam(:,:,1), its bicubic interpolation to ocean resolution (auvbcu), the optional shear against the
 * ocean's geostrophic velocity from pom(:,:,1) (the cpp option tau_udiff as a run-time flag), the quadratic drag law,
 * the Ekman velocities on both grids and the stress line integrals of the momentum constraints.  The thermodynamic
 * half (:711-853: fnetoc, fnetat and the arlaav / slhfav / oradav / arocav sums) runs in the same call once
 * qgcm_hip_xforc_heat_init has set it up (below); until then fnetoc and fnetat keep coming from the setters.
 * qgcm_hip_xforc_init(oc, atm, p): oc = the whole-domain ocean handle, or NULL for the atmos_only half; atm = the
 *   whole-domain atmosphere handle, which keeps the set-up.  dxa, fnot come from the atmosphere's qgcm_hip_params
 *   (dxo), dxo from the ocean's (dxa / ndxr without one).  The five weight tables are host pointers laid out as
 *   MODULE xfosubs holds them, (16, 0:ndxr, 0:ndxr) Fortran order (qgcm_hip.hostinit.bcuini restates bcuini).  Refuses,
 *   naming the reason and changing nothing: a y-slab handle, an ocean whose T grid is not nxaooc*ndxr x nyaooc*ndxr,
 *   an ocean that does not lie inside the atmosphere, a cyclic ocean with nxaooc != nxta, tau_udiff without an ocean,
 *   ndxr outside 1..128, a fine grid whose padded arrays pass 2^31 - 1 elements.  Above ndxr = 64 the box average wekpa
 *   is formed by k_xf_wekpa_stage (QGCM_HIP_XF_WEKPA_STAGE=0/1, read here, forces either form at any ndxr).
 *   Allocates the scratch (two fine p-grid stress arrays and the fine T-grid Ekman velocity; u1ator / v1ator are never
 *   stored) and, where they do not exist yet, the buffers of qgcm_hip_set_atm_monitor_fields (wekta, tauxa, tauya,
 *   uekat, vekat) and of qgcm_hip_set_monitor_fields (tauxo, tauyo, wekto).
 * qgcm_hip_xforc(oc, atm): one call, asynchronous, on the atmosphere's stream; that stream first waits for what is
 *   queued on the ocean's, and the ocean's stream afterwards waits for the results.  It reads the lagged time levels
 *   (pam, pom: what qgcm_hip_get_state returns as pom) and writes
 *     wekpa, txisat, txinat  where qgastep / atinvq read them (qgcm_hip_set_forcing / _set_cyc_forcing's places)
 *     wekpo, txisoc, txinoc  likewise for the ocean (txis / txin: cyclic ocean only)
 *     tauxo, tauyo, wekto    the buffers of qgcm_hip_set_monitor_fields and, after qgcm_hip_oml_init, the mixed layer's
 *     tauxa, tauya, uekat, vekat, wekta   the buffers of qgcm_hip_set_atm_monitor_fields (they count as given)
 *   Every field is bitwise the reference's (same operand order, contraction off); the four line integrals are
 *   parallel sums with a fixed tree: reproducible from call to call, equal to the reference to rounding.
 * qgcm_hip_xforc_get: synchronous copies, dense Fortran order: tauxa, tauya, wekpa (nxpa,nypa), uekat (nxpa,nyta),
 *   vekat (nxta,nypa), wekta (nxta,nyta), tauxo, tauyo, wekpo (nxpo,nypo), wekto (nxto,nyto), txi[4] = txisat, txinat,
 *   txisoc, txinoc (0 for a box ocean or none).  NULL skips a field.
 * qgcm_hip_coupled_set_xforc(oc, atm, on): while on, qgcm_hip_coupled_steps(oc, atm, ...) runs the reference's order
 *   (src/q-gcm.F:1222-1268): at every nt with mod(nt,nstr) == 1 xforc, then the ocean step, then the atmospheric
 *   steps up to the next such nt.  Off (the default) a window's launches, streams and graphs are those without this
 *   feature. */
typedef struct qgcm_hip_xforc_params {
  int ndxr;                 /* dxa/dxo                                       (MODULE parameters) */
  int nx1, ny1;             /* first atmosphere T cell above the ocean */
  int nxaooc, nyaooc;       /* atmosphere T cells above the ocean */
  double cdat, raoro;       /* drag coefficient, density ratio rhoat/rhooc   (MODULE intrfac) */
  double hmat, hmoc;        /* mixed layer thicknesses                       (MODULE intrfac) */
  double bccoat, bccooc;    /* mixed boundary condition coefficients         (MODULE atconst / occonst) */
  int tau_udiff;            /* the reference's cpp option tau_udiff as a run-time flag */
  const double *stbbb, *stbus, *stbvs, *stbun, *stbvn; /* (16, 0:ndxr, 0:ndxr) each */
} qgcm_hip_xforc_params;
int qgcm_hip_xforc_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_params *p);
int qgcm_hip_xforc(qgcm_hip_handle oc, qgcm_hip_handle atm);
int qgcm_hip_xforc_get(qgcm_hip_handle oc, qgcm_hip_handle atm, double *tauxa, double *tauya, double *uekat,
                       double *vekat, double *wekta, double *wekpa, double *tauxo, double *tauyo, double *wekto,
                       double *wekpo, double *txi);
int qgcm_hip_coupled_set_xforc(qgcm_hip_handle oc, qgcm_hip_handle atm, int on);

/* ---- atmospheric mixed layer ------------------------------------------------------------------------
 * "call aml" (src/q-gcm.F:1260; src/amlsubs.F) on the device, for a whole-domain atmosphere handle.
 * qgcm_hip_aml_init(atm, p): from then on the handle owns ast, astm, hmixa, hmixam (nxta,nyta), in rotating buffers:
 *   ast and hmixa ARE the buffers of qgcm_hip_set_atm_monitor_fields (what was given before is kept), so the
 *   atmosphere monitors, qgcm_hip_atm_valids, tavatm, covatm and the periodic dump read the stepped fields; they count
 *   as given.  The init also allocates, as zeros, the inputs nobody has given yet - fnetat (the buffer of
 *   qgcm_hip_set_atm_tav_fields) and wekta, uekat, vekat (qgcm_hip_set_atm_monitor_fields) - so these count as given
 *   too from then on: the diagnostics' "was never given" checks no longer catch a missing xforc / setter for them.
 *   Every atmospheric step of qgcm_hip_steps / qgcm_hip_coupled_steps then runs aml immediately before
 *   qgastep, on the handle's stream and inside the step's graph, and the averaging at mod(nt-1,100) == 0 also averages
 *   ast and hmixa with their lagged levels (src/q-gcm.F:1388-1394).  Without it nothing changes.
 *   tdta, dxa, dya, gpat, fnot come from the handle's qgcm_hip_params; radiat stays on the host and hands in its
 *   coefficients.  xc1ast (nxta,nyta) and dtopat (nxpa,nypa) are host arrays, dense Fortran order; NULL = zeros.
 * qgcm_hip_aml(atm): one call, asynchronous.  Reads fnetat (the buffer of qgcm_hip_set_atm_tav_fields), wekta, uekat,
 *   vekat (qgcm_hip_set_atm_monitor_fields; xforc writes them), pa layer 1 (current level) and pam; writes the new
 *   levels, entat, xan(1), enisat(1), eninat(1) where qgastep reads them (the places of qgcm_hip_set_forcing /
 *   _set_cyc_forcing; later entries of xan, enisat, eninat are not touched) and the monitors cfraat, centat.
 *   ast, astm, hmixa, hmixam, entat are bitwise the reference's; the sums are parallel with a fixed tree:
 *   reproducible from call to call, equal to the reference to rounding; cfraat is exact.
 * qgcm_hip_aml_set_state / _get_state: dense Fortran order, NULL = leave / skip, synchronous.
 * qgcm_hip_aml_get_diag: entat (nxpa,nypa; NULL skips) and diag[3*(nla-1) + 2] = xan(1:nla-1), enisat(1:nla-1),
 *   eninat(1:nla-1), cfraat, centat (aml writes the first entry of each vector; the others are what the setters gave). */
typedef struct qgcm_hip_aml_params {
  double hmat, hmamin, hmadmp;   /* mixed layer thickness, its floor, its damping constant   (MODULE intrfac) */
  double rrcpat;                 /* 1/(rhoat*cpat)                                           (MODULE radiate) */
  double tat1, tat2;             /* temperature anomalies of layers 1, 2                     (MODULE atconst) */
  double xcexp;                  /* coupling coefficient x                                   (MODULE atconst) */
  double at2d, at4d, ahmd;       /* diffusivities of ast (Del-sqd, Del-4th) and of hmixa     (MODULE intrfac) */
  double aface[QGCM_HIP_MAXL - 1], bface, cface, dface; /* entrainment factors of radiat     (MODULE radiate) */
  const double *xc1ast;          /* (nxta,nyta) or NULL */
  const double *dtopat;          /* (nxpa,nypa) or NULL */
} qgcm_hip_aml_params;
int qgcm_hip_aml_init(qgcm_hip_handle atm, const qgcm_hip_aml_params *p);
int qgcm_hip_aml_set_state(qgcm_hip_handle atm, const double *ast, const double *astm, const double *hmixa, const double *hmixam);
int qgcm_hip_aml_get_state(qgcm_hip_handle atm, double *ast, double *astm, double *hmixa, double *hmixam);
int qgcm_hip_aml(qgcm_hip_handle atm);
int qgcm_hip_aml_get_diag(qgcm_hip_handle atm, double *entat, double *diag);

/* ---- heat half of xforc -----------------------------------------------------------------------------
 * src/xfosubs.F:711-853 with bilint (:891-993): fnetoc = -fsprim - atmrad - ocnrad - slhf at every ocean T point from
 * the mixed layer's lagged sstm and asto, the bilinear interpolant of the atmosphere's lagged astm (computed where it
 * is used, never stored); fnetat = the land value -fsprim - Dmup*astm, over the cells above the ocean the sum of
 * ocfrac*(ocnrad + atmrad + slhf) over each cell's ndxr x ndxr ocean points (one wave per cell, fixed order, no
 * atomics), plus the pointwise eta / topography / hmixam terms; the monitors arlaav, slhfav, oradav, arocav.
 * qgcm_hip_xforc_heat_init(oc, atm, p): after qgcm_hip_xforc_init(oc, atm), qgcm_hip_aml_init(atm) and
 *   qgcm_hip_oml_init(oc); refuses, naming the reason and changing nothing, when one of them is missing, when oc is
 *   NULL or is not the handle qgcm_hip_xforc_init was given.  fsa[nyta] = fsprim(ytarel), fso[nyto] = fsprim(ytorel)
 *   are host tables (sin is evaluated on the host, where the reference evaluates it); xta, yta, xto, yto are the
 *   T-point coordinates of both grids, from which bilint's index and weight tables are built once, as the reference
 *   computes them.  Adown11 = Adown(1,1); dtopat is the one given to qgcm_hip_aml_init.
 * qgcm_hip_xforc(oc, atm) then runs the heat half after the momentum half, on the same stream and inside the same
 *   waits, and writes fnetoc into the mixed layer's own forcing (the buffer of qgcm_hip_oml_set_forcing) and fnetat
 *   into the buffer of qgcm_hip_set_atm_tav_fields (it counts as given), where aml reads it.  fnetoc is bitwise the
 *   reference's, fnetat over land too; above the ocean and in the four monitors the sums run in a fixed tree:
 *   reproducible, equal to the serial reference to rounding.
 * qgcm_hip_xforc_heat_get: synchronous copies, dense Fortran order, NULL skips: fnetoc (nxto,nyto), fnetat
 *   (nxta,nyta), scal[4] = arlaav, slhfav, oradav, arocav. */
typedef struct qgcm_hip_xforc_heat_params {
  double xlamda, D0up, Dmup, Dmdown, Adown11, Bmup, B1down, Cmup, C1down; /* MODULE radiate */
  double hmadmp, hmat;                                                     /* MODULE intrfac */
  const double *fsa, *fso;             /* fsprim(ytarel(1:nyta)), fsprim(ytorel(1:nyto)) */
  const double *xta, *yta, *xto, *yto; /* T-point coordinates (nxta), (nyta), (nxto), (nyto) */
} qgcm_hip_xforc_heat_params;
int qgcm_hip_xforc_heat_init(qgcm_hip_handle oc, qgcm_hip_handle atm, const qgcm_hip_xforc_heat_params *p);
int qgcm_hip_xforc_heat_get(qgcm_hip_handle oc, qgcm_hip_handle atm, double *fnetoc, double *fnetat, double *scal);

/* ---- heat half of xforc without an ocean: atmos_only -------------------------------------------------
 * What a -Datmos_only build of the reference runs of src/xfosubs.F:711-853: the sea below the atmosphere is an SST that
 * is read once and held (src/q-gcm.F:753-786, sstm = sst), fnetoc and arocsm are skipped (:805-812).  The atmosphere
 * handle owns the SST, (nxto, nyto) = (nxaooc*ndxr, nyaooc*ndxr), at the position qgcm_hip_xforc_init was given.
 * With it qgcm_hip_coupled_steps(NULL, atm, ...) after qgcm_hip_coupled_set_xforc(NULL, atm, 1) is the reference's
 * atmos_only sequence xforc; (aml; qgastep; atinvq; atqzbd) x nstr without a host transfer.
 * qgcm_hip_xforc_sst_init(atm, p): after qgcm_hip_xforc_init(NULL, atm, ...) and qgcm_hip_aml_init(atm).  The radiation
 *   constants, fsa and the T-point coordinates are those of qgcm_hip_xforc_heat_params (bilint's tables are built by the
 *   same code); dxo, dyo are the spacings of the SST grid (ocfrac = dxo*dyo/(dxa*dya), ocnorm = 1/(nxto*nyto));
 *   sst (nxto, nyto) is a host array, dense Fortran order.  Refuses, naming the reason and changing nothing: a NULL
 *   argument, a handle that is not a whole-domain atmosphere, qgcm_hip_xforc_init missing or called WITH an ocean (the
 *   heat half of such an atmosphere is qgcm_hip_xforc_heat_init), qgcm_hip_aml_init missing, a sea that does not lie
 *   inside the atmosphere, a coordinate that xta / yta does not cover.
 * qgcm_hip_xforc(NULL, atm) then runs this heat half after the momentum half, on the same stream: fnetat into the
 *   buffer of qgcm_hip_set_atm_tav_fields (it counts as given), where aml reads it; bitwise the reference's over land,
 *   above the sea and in slhfav / oradav / arlaav equal to the serial reference to rounding (one wave per cell, fixed
 *   order, no atomics: reproducible); arocav = 0 exactly.
 * qgcm_hip_xforc_sst_set(atm, sst): replaces the held SST; a synchronous upload, ordered after what is queued on the
 *   handle's stream.
 * qgcm_hip_xforc_sst_get: synchronous copies, NULL skips: fnetat (nxta,nyta), scal[4] = arlaav, slhfav, oradav, arocav. */
typedef struct qgcm_hip_xforc_sst_params {
  double xlamda, D0up, Dmup, Dmdown, Adown11, Bmup, B1down, Cmup, C1down; /* MODULE radiate */
  double hmadmp, hmat;                                                     /* MODULE intrfac */
  const double *fsa;                   /* fsprim(ytarel(1:nyta)) */
  const double *xta, *yta, *xto, *yto; /* T-point coordinates (nxta), (nyta), (nxto), (nyto) */
  double dxo, dyo;                     /* spacing of the SST grid */
  const double *sst;                   /* (nxto, nyto) */
} qgcm_hip_xforc_sst_params;
int qgcm_hip_xforc_sst_init(qgcm_hip_handle atm, const qgcm_hip_xforc_sst_params *p);
int qgcm_hip_xforc_sst_set(qgcm_hip_handle atm, const double *sst);
int qgcm_hip_xforc_sst_get(qgcm_hip_handle atm, double *fnetat, double *scal);

/* ---- xforc on a y-slab ocean under a replicated atmosphere -------------------------------------------
 * Every rank holds its ocean slab and, on the same device, a whole-domain atmosphere handle: a replica, stepped
 * redundantly on every rank.  The replicas stay bitwise identical: everything one reads is computed from replicated
 * data by the same kernels, or added from an all-gathered buffer in rank order on every rank.  With tau_udiff off the
 * fine stress and tauxa, tauya, uekat, vekat, wekta, wekpa, txisat, txinat depend on pam only, so the atmosphere side
 * is the whole-domain call's, unchanged, on each replica.  The ocean side is local: tauxo, tauyo, wekto on every local
 * row of the slab (owned and halo) from the fine rows at the slab's global offset; wekpo on every local row but the
 * outermost halo row towards a neighbour (the T row beyond it is not held; no kernel reads wekpo there); txisoc /
 * txinoc of a cyclic ocean from the replicated fine rows on every rank, the whole-domain call's bits.  The heat half
 * computes fnetoc pointwise on every local T row and, per atmosphere cell above the ocean, the sums over the points
 * the slab OWNS (T rows g0..g1, g1-1 on the rank that owns row nypo) in the whole-domain kernel's order; the message
 * is (4, nxaooc*nyaooc): the cell's fnetat sum and its arocav / slhfav / oradav parts, +0.0 for a cell the slab owns no
 * point of.  The caller all-gathers the messages (rank-major); the combine adds them in rank order, then runs the
 * whole-domain call's tail.  A cell inside one slab keeps the whole-domain bits; a cell a seam cuts, and the three
 * monitors, agree to the rounding of a reordered sum.  With one rank every output is bitwise the whole-domain call's.
 * qgcm_hip_xforc_slab_init(oc_slab, atm, p) / qgcm_hip_xforc_heat_slab_init(oc_slab, atm, p): as qgcm_hip_xforc_init /
 *   _heat_init (same structs; fso, yto and nyaooc*ndxr describe the WHOLE basin's nypo - 1 T rows), for an ocean
 *   handle that holds a slab - or the whole domain, as a lone slab.  Refuse, naming the reason and changing nothing: an
 *   atmosphere handle that is not a whole-domain atmosphere, handles on different devices, tau_udiff (the fine stress
 *   above the sea would need every slab's pom on every rank), geometry that does not match the slab's global grid, the
 *   heat half before qgcm_hip_oml_init on the slab or qgcm_hip_aml_init on the atmosphere.  An atmosphere set up this
 *   way is refused by qgcm_hip_xforc, _xforc_get, _xforc_heat_init / _get and qgcm_hip_coupled_set_xforc, and the
 *   other way round.
 * qgcm_hip_xforc_slab_msg_len(atm): doubles per rank's message: 4*nxaooc*nyaooc with the heat half, else 0 (banded,
 *   below: the momentum block in front).
 * qgcm_hip_xforc_slab_part(oc_slab, atm, send_dev): asynchronous, on the atmosphere's stream, ordered against the
 *   slab's stream as qgcm_hip_xforc is: the momentum half, fnetoc and the message into send_dev (device; may be NULL
 *   without the heat half).  Results land where the whole-domain call puts them: wekpo, txisoc / txinoc where the slab
 *   stages read them, tauxo, tauyo, wekto in the buffers of qgcm_hip_set_monitor_fields and the mixed layer's own,
 *   fnetoc in the mixed layer's, the atmosphere's in its usual places.
 * qgcm_hip_xforc_slab_combine(oc_slab, atm, gath_dev, nranks): heat half only (banded, below: always); the rank-ordered sums of nranks
 *   messages, then fnetat and the four monitors as the whole-domain call computes them; the slab's stream then waits.
 * qgcm_hip_xforc_slab_get: synchronous copies, NULL skips: what qgcm_hip_xforc_get and qgcm_hip_xforc_heat_get return,
 *   the ocean's fields with the slab's LOCAL rows: tauxo, tauyo, wekpo (nxpo, nyl), wekto, fnetoc (nxto, nyl-1).
 * Not extended to the library's own RCCL exchanges (qgcm_hip_slab_steps): the caller carries the message. */
int qgcm_hip_xforc_slab_init(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, const qgcm_hip_xforc_params *p);
int qgcm_hip_xforc_heat_slab_init(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, const qgcm_hip_xforc_heat_params *p);
int qgcm_hip_xforc_slab_msg_len(qgcm_hip_handle atm);
int qgcm_hip_xforc_slab_part(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, double *send_dev);
int qgcm_hip_xforc_slab_combine(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, const double *gath_dev, int nranks);
int qgcm_hip_xforc_slab_get(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, double *tauxa, double *tauya, double *uekat,
                            double *vekat, double *wekta, double *wekpa, double *tauxo, double *tauyo, double *wekto,
                            double *wekpo, double *txi, double *fnetoc, double *fnetat, double *scal);

/* ---- the atmosphere side of the slab xforc split by bands of atmosphere rows ---------------------------
 * An opt-in mode of the calls above.  The default stays the replicated path: every rank runs the atmosphere side on
 * the whole fine grid.  Banded, rank r owns a band a0..a1 of the atmosphere's p rows ja = 1..nypa and runs the
 * atmosphere side only on the fine rows that band's outputs, the line sums it owns and its slab's rows of tauxo / tauyo
 * read: row-windowed launches of the same kernel text, so a row holds the bits the replicated call gives it.  The
 * ranks' bands of tauxa, tauya, uekat, vekat, wekta, wekpa and the four line sums travel in front of the heat block in
 * the ONE all-gather; the combine copies every rank's rows into the replica (no sum, no atomics), then runs the heat
 * tail.  Every replica ends with the arrays of the replicated call, bitwise.  The fine arrays keep their full height;
 * outside a rank's windows they hold stale values that nothing reads.
 * qgcm_hip_xforc_bands: the plan, host code without a device; a pure function of its arguments.  Bands: rows 1..nypa
 *   (nypa = nyta + 1) split evenly, the first nypa % nranks bands one row longer.  slab_lo[r]..slab_hi[r]: the global
 *   ocean p rows rank r's slab OWNS (it holds three halo rows more towards each neighbour).  out[r], per rank:
 *     a0, a1       the band
 *     own          the line sums the rank forms: bit 0 txisat (a0 = 1), 1 txinat (a1 = nypa), 2 txisoc (the slab owns
 *                  ocean row 1), 3 txinoc (it owns row nypo); bits 2, 3 matter for a cyclic ocean only
 *     nseg, c0, c1 one or two intervals of cell rows (1-based, inclusive) k_xf_fine runs on: the band's and the slab's,
 *                  one where they touch
 *     f0, f1       the fine p rows those cell rows cover: the rank's fine-row window
 *     t0, t1       the fine T rows of wektaor that wekpa on the band reads
 *     nrow         rows per field in the message: the longest band
 *     mom_len      doubles of the message's momentum block: 8 + 6 * nrow * nxpa - a0, a1, own, 0, the four line sums
 *                  (0.0 where not owned), then tauxa, tauya, uekat, vekat, wekta, wekpa as (nrow, nxpa) from row a0
 *                  on, 0.0 past the band, past a field's last row and past its last column
 *   Refuses nranks outside 1..nypa and slab rows outside 1..nyaooc*ndxr+1.
 * qgcm_hip_xforc_slab_bands(oc_slab, atm, a0, a1, nrow, nranks): after qgcm_hip_xforc_slab_init, switches the pair to
 *   bands: this rank's band, the common row count and the rank count of the plan (the caller takes them from
 *   qgcm_hip_xforc_bands; the library derives the windows from the band and the slab's own rows with the same code).
 *   Refuses, naming the reason and changing nothing: a pair not set up by qgcm_hip_xforc_slab_init, a band outside
 *   1..nypa, nrow shorter than the band.  qgcm_hip_xforc_slab_init again returns the pair to the replicated path.
 *   Reads QGCM_HIP_XF_POISON (INTEGRATION): 1 = every _slab_part first fills the fine arrays with NaN bytes.
 * Banded, qgcm_hip_xforc_slab_msg_len is mom_len plus the heat block's 4*nxaooc*nyaooc (0 without the heat half),
 *   qgcm_hip_xforc_slab_part needs send_dev, and qgcm_hip_xforc_slab_combine is required without the heat half too:
 *   the scatter, then the heat tail if the heat half is on; it refuses an nranks other than the plan's.
 * Handles of one pair on different devices are refused as before; ranks on different GPUs are untested. */
typedef struct qgcm_hip_xforc_band {
  int a0, a1, own, nseg;
  int c0[2], c1[2], f0[2], f1[2];
  int t0, t1, nrow, mom_len;
} qgcm_hip_xforc_band;
int qgcm_hip_xforc_bands(int nxpa, int nyta, int ndxr, int ny1, int nyaooc, int nranks, const int *slab_lo,
                         const int *slab_hi, qgcm_hip_xforc_band *out);
int qgcm_hip_xforc_slab_bands(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, int a0, int a1, int nrow, int nranks);

/* ---- tau_udiff on a y-slab ocean: the surface pressure gathered ahead of xforc ----------------------
 * The ocean enters the momentum half at one place: the fine stress above the sea subtracts the ocean's geostrophic
 * surface velocity, formed from pom(:,:,1).  Before the atmosphere side runs, every rank assembles the basin's
 * pom(:,:,1) from the ranks' OWNED rows: pack, one all-gather by the caller (rank-major), assemble.  The stress kernels
 * then run unchanged on the assembled array, replicated or banded, and no sum changes its order: every momentum
 * output is bitwise the whole-domain qgcm_hip_xforc set up with tau_udiff = 1, on any rank count.  The heat half keeps
 * its statement above.  All four calls come after qgcm_hip_xforc_slab_init with tau_udiff = 0 in its struct (which,
 * like tau_udiff = 1 there, keeps its meaning: the shear-free path, and the refusal).
 * qgcm_hip_xforc_slab_udiff(oc_slab, atm, nrow, nranks): switches the shear term on for this pair.  nrow: the longest
 *   owned p-row range of any rank; nranks: the rank count.  Allocates the assembled array (nxpo x nypo of the basin,
 *   its own pitch) in the atmosphere handle.  The drag constants of the sea and the ocean's velocity factors are those
 *   of the whole-domain set-up with tau_udiff.  Refuses, naming the reason and changing nothing: a pair not set up by
 *   qgcm_hip_xforc_slab_init, nrow smaller than this slab's owned rows (or larger than the basin), nranks < 1.
 *   qgcm_hip_xforc_slab_init again returns the pair to the shear-free path.  Composes with qgcm_hip_xforc_slab_bands
 *   in either order.  Reads QGCM_HIP_XF_POISON (INTEGRATION): 1 = every assemble first fills the assembled array with
 *   NaN bytes, so a row no rank owns, or one the copy misses, shows.
 * qgcm_hip_xforc_slab_pom_len(oc_slab, atm, &n): n = 8 + nrow * nxpo doubles per rank's message.
 * qgcm_hip_xforc_slab_pom_pack(oc_slab, atm, send_dev): asynchronous, on the atmosphere's stream after everything
 *   queued on the slab's stream: a header of 8 doubles - g0, g1 (the global p rows the slab owns), nxpo, zeros - then
 *   rows g0 .. g1 of layer 1 of the lagged pressure (what the whole-domain call would read) as (nrow, nxpo) row-major,
 *   +0.0 past the slab's rows.  Halo rows are never packed.
 * qgcm_hip_xforc_slab_pom_assemble(oc_slab, atm, gath_dev, nranks): every rank's rows copied into the assembled
 *   array, one writer per point, no atomics; a header that does not describe rows inside 1 .. nypo writes nothing;
 *   refuses an nranks other than the set-up's.
 * With the shear term on, qgcm_hip_xforc_slab_part refuses unless an assemble has run since the last part ("the
 *   surface pressure has not been assembled for this call"); a part that goes through clears the flag.
 * Every rank receives nranks * (8 + nrow * nxpo) doubles per xforc: this is the exact form, not the scalable one
 * (DESIGN 6q).  Ranks on different GPUs are untested. */
int qgcm_hip_xforc_slab_udiff(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, int nrow, int nranks);
int qgcm_hip_xforc_slab_pom_len(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, long *n);
int qgcm_hip_xforc_slab_pom_pack(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, double *send_dev);
int qgcm_hip_xforc_slab_pom_assemble(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, const double *gath_dev, int nranks);

/* ---- tau_udiff on a y-slab ocean without the gather: owner-computed sums -------------------------------
 * A third opt-in mode of the slab calls, beside the bands and the gather above; it excludes both and implies the shear
 * term.  Rank r forms the fine stress only above the ocean rows it OWNS (the land south of the sea is rank 0's, the land
 * north of it the last rank's), from its own rows of pom(:,:,1) and the 4 rows beyond each seam, which the direct
 * neighbours send: one small all-gather of 8 + 8 * nxpo doubles per rank.  tauxa, tauya, vekat and the line sums have
 * one owner each; uekat's meridional lines and wekpa's boxes are sent as partial sums over the owned fine rows and added
 * in rank order by the combine, which every replica runs alike.  A line or box inside one rank's rows keeps the bits
 * of the whole-domain call; one that a seam cuts is a sum of the same terms in another order.
 * qgcm_hip_xforc_sums: the ownership plan, host code without a device; a pure function of its arguments.
 *   slab_lo[r]..slab_hi[r]: the global ocean p rows rank r owns.  out[r], per rank:
 *     g0, g1       the owned ocean p rows
 *     f0, f1       the owned fine p rows (fine row jocoff + g above ocean row g, jocoff = (ny1 - 1) * ndxr); the ranks'
 *                  intervals tile 1 .. nypaor in rank order
 *     t0, t1       the owned fine T rows: T row j belongs to the owner of p row j
 *     w0, w1       the fine p rows whose stress the rank holds correct: max(1, f0 - 3) .. min(nypaor, f1 + 3)
 *     c0, c1       the cell rows k_xf_fine runs on (they cover w0 .. w1); u0, u1: the coarse rows of u1at / v1at
 *     a0, a1       the coarse rows whose sample, uekat line or wekpa box meets f0 .. f1
 *     own          the line sums the rank forms: the bits of qgcm_hip_xforc_band
 *     nrow         rows per field in the message: the longest a0 .. a1 of any rank
 *     mom_len      doubles of the message's momentum block: 8 + 5 * nrow * nxpa - f0, f1, a0, own, the four line sums
 *                  (0.0 where not owned), then tauxa, tauya, vekat, the partial uekat line (without -uvekfc) and the
 *                  partial wekpa numerator as (nrow, nxpa) from row a0 on
 *   Refuses, naming the reason: nranks < 1, owned ranges that do not tile 1 .. nypo, a rank that owns fewer than 4
 *   ocean rows, and (odd ndxr) a line sum whose two fine rows two ranks would share.
 * qgcm_hip_xforc_slab_sums(oc_slab, atm, rank, nranks, slab_lo, slab_hi): after qgcm_hip_xforc_slab_init with
 *   tau_udiff = 0, switches the pair to this mode; the library derives the plan with the same code and keeps entry
 *   `rank`, whose rows must be the slab's.  Refuses a pair in the banded or the gather mode.  qgcm_hip_xforc_slab_init
 *   again returns the pair to the replicated, shear-free path.  Reads QGCM_HIP_XF_POISON (INTEGRATION): 1 = NaN bytes
 *   into the basin-sized array before every edge assemble and into the fine arrays before every part.
 * qgcm_hip_xforc_slab_edge_len(oc_slab, atm, &n): n = 8 + 8 * nxpo doubles.
 * qgcm_hip_xforc_slab_edge_pack(oc_slab, atm, send_dev): a header - g0, g1, nxpo, zeros - then owned rows g0 .. g0 + 3
 *   and g1 - 3 .. g1 of layer 1 of the lagged pressure.  Halo rows are never packed.
 * qgcm_hip_xforc_slab_edge_assemble(oc_slab, atm, gath_dev, nranks): the slab's owned rows (a local copy) and the 4 rows
 *   beyond each seam from the neighbours' messages into the basin-sized array; rows g0 - 4 .. g1 + 4 are then the
 *   basin's bits, everything else is stale (or NaN bytes).  A neighbour's header that does not fit writes nothing.
 * In this mode qgcm_hip_xforc_slab_part refuses without a fresh edge assemble and needs send_dev;
 *   qgcm_hip_xforc_slab_msg_len is mom_len plus the heat block; qgcm_hip_xforc_slab_combine is required without the
 *   heat half too and refuses an nranks other than the plan's.  Ranks on different GPUs are untested. */
typedef struct qgcm_hip_xforc_sum {
  int g0, g1, f0, f1, t0, t1, w0, w1;
  int c0, c1, u0, u1, a0, a1, own, nrow;
  int mom_len, pad;
} qgcm_hip_xforc_sum;
int qgcm_hip_xforc_sums(int nxpa, int nyta, int ndxr, int ny1, int nyaooc, int nranks, const int *slab_lo,
                        const int *slab_hi, qgcm_hip_xforc_sum *out);
int qgcm_hip_xforc_slab_sums(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, int rank, int nranks, const int *slab_lo,
                             const int *slab_hi);
int qgcm_hip_xforc_slab_edge_len(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, long *n);
int qgcm_hip_xforc_slab_edge_pack(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, double *send_dev);
int qgcm_hip_xforc_slab_edge_assemble(qgcm_hip_handle oc_slab, qgcm_hip_handle atm, const double *gath_dev, int nranks);

/* ---- measurement -------------------------------------------------------- */
/* Runs n steps like qgcm_hip_steps and returns the HIP-event time (ms) of
 * the whole region, measured on the handle's stream. */
int qgcm_hip_time_steps(qgcm_hip_handle h, int s0, int n, float *ms);
/* Captures, instantiates and uploads the HIP graphs qgcm_hip_steps(s0, n) will replay (50-step blocks + one block
 * for the even part of the remainder) without running a step, so that a caller timing a window with its own clock
 * keeps graph construction outside it.  Synchronous; the state is untouched. */
int qgcm_hip_prepare_steps(qgcm_hip_handle h, int s0, int n);
/* Runs n steps eagerly with HIP events around every kernel launch and
 * accumulates per-kernel totals: ms[i], launches[i] for i < *nk (in: capacity,
 * out: number of kernel slots).  names[i] points to static strings. */
int qgcm_hip_profile_steps(qgcm_hip_handle h, int s0, int n, double *ms, int *launches,
                           const char **names, int *nk);
/* device copy bandwidth probe (GB/s of read+write traffic) used as the
 * "measured peak" beside the nominal 8 TB/s. */
int qgcm_hip_copy_bandwidth(qgcm_hip_handle h, size_t bytes, int reps, double *gbps);
/* Rate (GB/s of read + written bytes) of a pure streaming kernel that reads nr fields and writes nw fields of
 * field_bytes each, 16 bytes per lane: the practical ceiling for a kernel of that read : write mix on buffers of
 * that size (15:6 = the tendency kernel, 3:3 = row transforms / Thomas sweep, 5:3 = fused inverse rows). */
int qgcm_hip_stream_mix_bandwidth(qgcm_hip_handle h, int nr, int nw, size_t field_bytes, int reps, double *gbps);
/* HIP stream of the handle as an opaque pointer (hipStream_t). */
void *qgcm_hip_stream(qgcm_hip_handle h);
/* Debug aid: the device allocations the library holds in this process at the moment, over all handles and scratch -
 * their number and their bytes (either pointer may be NULL).  Every allocation of the library is counted where it is
 * made and where it is freed, so a handle that has been destroyed leaves both figures where they were before it was
 * created.  Process-local and exact, unlike the device's free memory, which other work on the GPU moves. */
int qgcm_hip_debug_live_allocs(long *blocks, size_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* QGCM_HIP_H */
