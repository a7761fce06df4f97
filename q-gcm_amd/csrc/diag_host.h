// Host side of the on-device diagnostics: the validity scan, the ocean and atmosphere monitors, the start-up / restart
// arithmetic, the time averages, the periodic dumps, the covariance matrices, the area averages and the CFL check
// (DESIGN 6e-6j, 6m).  Parameter fillers,
// launches and C ABI entry points only; the kernels are in the k_*.h headers.  Part of qgcm_hip.hip's translation unit:
// included there once, after the handle and the step's building blocks and before one_step.
#pragma once

// ---------------------------------------------------------------------------
// validity scan
// ---------------------------------------------------------------------------
extern "C" int qgcm_hip_set_dtopoc(qgcm_hip_handle c, const double *dtopoc) {
  if (check_ready(c, "qgcm_hip_set_dtopoc")) return 1;
  const QgGeom &g = c->g;
  if (!dtopoc) {
    c->dtopoc.reset();
    return 0;
  }
  return upload_field(c, c->dtopoc, g.ldx, dtopoc, g.nx, g.ny);
}

// last owned T row (local): the T rows of a slab are jlo..jhi, and jlo..jhi-1 on the rank that owns row nypo
static int owned_t1(const QgGeom &g) { return (g.jhi + g.joff == g.nyg) ? g.jhi - 1 : g.jhi; }

// the scan of qgcm_hip_valids over the owned rows -> c->val_part (asynchronous)
static int launch_valids_scan(qgcm_hip_ctx *c, QgValidsParams &P, const char *who) {
  if (check_ready(c, who)) return 1;
  const QgGeom &g = c->g;
  if (g.nl < 2 || g.nl > QG_MAXL) QG_FAIL("%s: unsupported nlo", who);
  if (c->val_part.ensure((size_t)(2 * VAL_NMM + QG_MAXL) * VAL_NB, "the validity scan's partials") ||
      c->val_out.ensure((size_t)2 * VAL_NMM + QG_MAXL + 2, "the validity scan's result"))
    return 1;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.po = c->p[c->ip];
  P.qo = c->q[c->iq];
  if (c->oml.on) {
    P.sst = c->oml.sst[c->oml.is];
    P.wekto = c->oml.wekto;
    P.ldt = c->oml.ldt;
  }
  P.dtopoc = c->dtopoc;
  P.jlo = g.jlo;
  P.nrow = g.jhi - g.jlo + 1;
  P.nrowt = owned_t1(g) - g.jlo + 1;
  for (int k = 0; k < g.nl - 1; ++k) P.rgpoc[k] = 1.0 / c->prm.gpoc[k]; // src/valsubs.F:390-392
  for (int k = 0; k < g.nl; ++k) P.hoc[k] = c->prm.hoc[k];
  P.part = c->val_part;
  P.out = c->val_out;
  P.ocnorm = 1.0 / ((double)g.nxt * (double)(g.nyg - 1));
#define QG_VALIDS(NLV) hipLaunchKernelGGL((k_valids_scan<NLV>), dim3(VAL_NB), dim3(VAL_NT), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_VALIDS, "k_valids");
#undef QG_VALIDS
  HIPCHECK(hipGetLastError());
  return 0;
}

// out[0 .. nres-2], *solnok from the device vector at c->val_out
static int valids_fetch(qgcm_hip_ctx *c, int nres, double *out, int *solnok, double *status) {
  double h[2 * VAL_NMM + QG_MAXL + 2];
  HIPCHECK(hipMemcpyAsync(h, c->val_out, sizeof(double) * (nres + (status ? 1 : 0)), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (status) {
    *status = h[nres];
    if (h[nres] != 0.0) return 0;
  }
  if (out)
    for (int q = 0; q < nres - 1; ++q) out[q] = h[q];
  if (solnok) *solnok = h[nres - 1] > 0.5 ? 1 : 0;
  return 0;
}

extern "C" int qgcm_hip_valids(qgcm_hip_handle c, double *out, int *solnok) {
  if (check_ready(c, "qgcm_hip_valids")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_valids: only for a handle that owns the whole domain (y-slabs: qgcm_hip_valids_part / _combine)");
  QgValidsParams P;
  if (launch_valids_scan(c, P, "qgcm_hip_valids")) return 1;
#define QG_VALIDS(NLV) hipLaunchKernelGGL((k_valids_final<NLV>), dim3(1), dim3(VAL_NT), 0, c->stream, P)
  QG_SWITCH_NL(c->g.nl, QG_VALIDS, "k_valids");
#undef QG_VALIDS
  HIPCHECK(hipGetLastError());
  return valids_fetch(c, 2 * VAL_NMM + c->g.nl + 1, out, solnok, nullptr);
}

extern "C" int qgcm_hip_valids_part_len(qgcm_hip_handle c) { return c ? VAL_PART_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_valids_part(qgcm_hip_handle c, double *send_dev) {
  if (check_ready(c, "qgcm_hip_valids_part")) return 1;
  if (!send_dev) QG_FAIL("qgcm_hip_valids_part: null argument");
  QgValidsParams P;
  if (launch_valids_scan(c, P, "qgcm_hip_valids_part")) return 1;
  P.out = send_dev;
#define QG_VALIDS(NLV) hipLaunchKernelGGL((k_valids_part<NLV>), dim3(1), dim3(VAL_NT), 0, c->stream, P)
  QG_SWITCH_NL(c->g.nl, QG_VALIDS, "k_valids");
#undef QG_VALIDS
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_valids_combine(qgcm_hip_handle c, const double *gath_dev, int nranks, double *out, int *solnok) {
  if (check_ready(c, "qgcm_hip_valids_combine")) return 1;
  if (!gath_dev || nranks < 1) QG_FAIL("qgcm_hip_valids_combine: need the gathered summaries and nranks >= 1");
  const QgGeom &g = c->g;
  if (g.nl < 2 || g.nl > QG_MAXL) QG_FAIL("qgcm_hip_valids_combine: unsupported nlo");
  if (c->val_out.ensure((size_t)2 * VAL_NMM + QG_MAXL + 2, "the validity scan's result")) return 1;
  QgValidsParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  if (c->oml.on) P.sst = c->oml.sst[c->oml.is]; // (only whether sst is scanned: the same on every rank)
  P.out = c->val_out;
  P.gath = gath_dev;
  P.nranks = nranks;
  P.ocnorm = 1.0 / ((double)g.nxt * (double)(g.nyg - 1)); // src/parameters_data.F:88
#define QG_VALIDS(NLV) hipLaunchKernelGGL((k_valids_combine<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_VALIDS, "k_valids");
#undef QG_VALIDS
  HIPCHECK(hipGetLastError());
  double st = 0.0;
  if (valids_fetch(c, 2 * VAL_NMM + g.nl + 1, out, solnok, &st)) return 1;
  if (st != 0.0)
    QG_FAIL("qgcm_hip_valids_combine: the gathered summaries do not tile rows 1..%d (rank %d of %d does not continue them)",
            g.nyg, (int)st - 1, nranks);
  return 0;
}

// ---------------------------------------------------------------------------
// ocean monitors: the ocean half of monnc_comp and couroc
// ---------------------------------------------------------------------------
extern "C" int qgcm_hip_monitor_len(qgcm_hip_handle c) { return c ? MON_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_set_mon_params(qgcm_hip_handle c, const qgcm_hip_mon_params *p) {
  if (!c || !p) QG_FAIL("qgcm_hip_set_mon_params: null argument");
  c->mon.prm = *p;
  c->mon.prm_set = true;
  return 0;
}

extern "C" int qgcm_hip_set_monitor_fields(qgcm_hip_handle c, const double *tauxo, const double *tauyo, const double *wekto,
                                           const double *sst) {
  if (check_ready(c, "qgcm_hip_set_monitor_fields")) return 1;
  const QgGeom &g = c->g; // (a y-slab: the local rows, halo rows included)
  const int nyt = g.ny - 1;
  auto &m = c->mon;
  if (!m.ldt) m.ldt = round_up(g.nxt, 16);
  return upload_field(c, m.taux, g.ldx, tauxo, g.nx, g.ny) || upload_field(c, m.tauy, g.ldx, tauyo, g.nx, g.ny) ||
         upload_field(c, m.wekto, m.ldt, wekto, g.nxt, nyt) || upload_field(c, m.sst, m.ldt, sst, g.nxt, nyt);
}

// The surface fields the ocean's diagnostics read: the mixed layer's own stress, wekto and sst when it is on, else the
// monitor fields (qgcm_hip_set_monitor_fields).  `need` lists the fields the caller reads, in the order it reports
// them, up to SF_END: fails, naming the first of them that was never given.
enum { SF_TAUX = 0, SF_TAUY, SF_WEKTO, SF_SST, SF_END };
static const int kSurfAll[] = {SF_TAUX, SF_TAUY, SF_WEKTO, SF_SST, SF_END};
struct QgSurf { const double *taux, *tauy, *wekto, *sst; int ldt; };
static int surf_fields(const qgcm_hip_ctx *c, const int *need, QgSurf &S, const char *who) {
  if (c->oml.on) {
    S = {c->oml.taux, c->oml.tauy, c->oml.wekto, c->oml.sst[c->oml.is], c->oml.ldt};
    return 0;
  }
  const auto &m = c->mon;
  S = {m.taux, m.tauy, m.wekto, m.sst, m.ldt};
  const double *given[SF_END] = {m.taux, m.tauy, m.wekto, m.sst};
  static const char *name[SF_END] = {"tauxo", "tauyo", "wekto", "sst"};
  for (; *need != SF_END; ++need)
    if (!given[*need])
      QG_FAIL("%s: %s was never given (qgcm_hip_set_monitor_fields) and the mixed layer is off", who, name[*need]);
  return 0;
}

// the parameters of the monitor kernels (partials over this handle's owned rows); allocates on first use
static int mon_params(qgcm_hip_ctx *c, QgMonParams &P, const char *who) {
  if (check_ready(c, who)) return 1;
  if (c->g.atm) QG_FAIL("%s: the handle is an atmosphere (only the ocean half of monnc_comp is implemented)", who);
  auto &m = c->mon;
  if (!m.prm_set) QG_FAIL("%s: qgcm_hip_set_mon_params has not been called", who);
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  const int nl = g.nl;
  QgSurf S;
  if (surf_fields(c, kSurfAll, S, who)) return 1;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.taux = S.taux; P.tauy = S.tauy; P.wekto = S.wekto; P.sst = S.sst; P.ldt = S.ldt;
  // the time levels qgcm_hip_get_state hands out at this point of the loop (after an averaging step: the averaged ones)
  P.po = c->p[c->ip]; P.pom = c->p[c->ip ^ 1]; P.qo = c->q[c->iq];
  P.wekpo = c->wekpo; P.entoc = c->entoc;
  // the owned rows: p rows jlo..jhi, T (jet) rows jlo..owned_t1 (a whole-domain handle: 1..nypo, 1..nyto)
  P.jlo = g.jlo; P.jhi = g.jhi; P.njet = owned_t1(g) - g.jlo + 1;
  P.ntx = (g.nx + MON_TX - 1) / MON_TX;
  P.nblk = P.ntx * ((g.jhi - g.jlo + 1 + MON_TY - 1) / MON_TY);
  if (m.psum.ensure((size_t)MON_NS(nl) * P.nblk, "the monitors' partial sums") ||
      m.pmin.ensure((size_t)MON_NM(nl) * P.nblk, "the monitors' partial extrema") ||
      m.ujet.ensure((size_t)P.njet * nl, "the monitors' jet rows") || m.out.ensure(MON_LEN(nl) + 1, "the monitors' result") ||
      m.hout.ensure(MON_LEN(nl) + 1, "the monitors' pinned result"))
    return 1;
  P.psum = m.psum; P.pmin = m.pmin; P.ujet = m.ujet; P.out = m.out;
  P.sb = m.prm.sb_hflux; P.nb = m.prm.nb_hflux;
  // MODULE occonst as src/q-gcm.F:414-436 derives it; dto = tdto/2 exactly
  P.dto = 0.5 * pr.tdto;
  P.rdxof0 = 1.0 / (pr.dxo * pr.fnot);
  P.dxom2 = 1.0 / (pr.dxo * pr.dxo);
  P.hdxom1 = 0.5 / pr.dxo;
  P.uvgfac = m.prm.ycexp * P.rdxof0;           // src/monitor_diag.F:1493-1494
  P.rhf0hm = 0.5 / (pr.fnot * m.prm.hmoc);
  for (int k = 0; k < nl - 1; ++k) P.rgpoc[k] = 1.0 / pr.gpoc[k];
  P.ocnorm = 1.0 / ((double)g.nxt * (double)(g.nyg - 1)); // src/parameters_data.F:88
  P.rhooc = m.prm.rhooc; P.cpoc = m.prm.cpoc; P.fnot = pr.fnot; P.delek = pr.delek;
  for (int k = 0; k < nl; ++k) {
    P.hoc[k] = pr.hoc[k]; P.gpoc[k] = pr.gpoc[k]; P.ah2oc[k] = pr.ah2oc[k]; P.ah4oc[k] = pr.ah4oc[k];
  }
  return 0;
}

// the scan and the jet rows over the owned rows; then `last` (k_mon_final or k_monslab_part) reduces them
static int launch_monitors(qgcm_hip_ctx *c, const QgMonParams &P, bool part) {
  const QgGeom &g = c->g;
  // k_mon_jet's LDS: the row when it fits MON_JET_CHUNK, else one chunk (the kernel then takes the row in passes)
  static_assert(sizeof(double) * MON_JET_CHUNK <= 65536, "k_mon_jet's chunk exceeds the LDS a launch gets by default");
  const size_t jet_lds = sizeof(double) * (g.nx < MON_JET_CHUNK ? g.nx : MON_JET_CHUNK);
#define QG_MON(NLV)                                                                                      \
  if (c->whole && g.cyc) hipLaunchKernelGGL((k_mon_scan<NLV, true>), dim3(P.nblk), dim3(MON_NT), 0, c->stream, P);  \
  else if (c->whole) hipLaunchKernelGGL((k_mon_scan<NLV, false>), dim3(P.nblk), dim3(MON_NT), 0, c->stream, P);      \
  else if (g.cyc) hipLaunchKernelGGL((k_monslab_scan<NLV, true>), dim3(P.nblk), dim3(MON_NT), 0, c->stream, P);      \
  else hipLaunchKernelGGL((k_monslab_scan<NLV, false>), dim3(P.nblk), dim3(MON_NT), 0, c->stream, P);                \
  hipLaunchKernelGGL(k_mon_jet, dim3(P.njet, g.nl), dim3(64), jet_lds, c->stream, P);                       \
  if (part) hipLaunchKernelGGL((k_monslab_part<NLV>), dim3(1), dim3(MON_FT), 0, c->stream, P);                 \
  else hipLaunchKernelGGL((k_mon_final<NLV>), dim3(1), dim3(MON_FT), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_MON, "k_mon");
#undef QG_MON
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_monitors(qgcm_hip_handle c, double *out) {
  if (check_ready(c, "qgcm_hip_monitors")) return 1;
  if (!out) QG_FAIL("qgcm_hip_monitors: null argument");
  if (!c->whole)
    QG_FAIL("qgcm_hip_monitors: only for a handle that owns the whole domain (y-slabs: qgcm_hip_monitors_part / _combine)");
  QgMonParams P;
  if (mon_params(c, P, "qgcm_hip_monitors") || launch_monitors(c, P, false)) return 1;
  auto &m = c->mon;
  const int nl = c->g.nl;
  HIPCHECK(hipMemcpyAsync(m.hout, m.out, sizeof(double) * MON_LEN(nl), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  memcpy(out, m.hout, sizeof(double) * MON_LEN(nl));
  return 0;
}

extern "C" int qgcm_hip_monitor_part_len(qgcm_hip_handle c) { return c ? MON_PART_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_monitors_part(qgcm_hip_handle c, double *send_dev) {
  if (check_ready(c, "qgcm_hip_monitors_part")) return 1;
  if (!send_dev) QG_FAIL("qgcm_hip_monitors_part: null argument");
  QgMonParams P;
  if (mon_params(c, P, "qgcm_hip_monitors_part")) return 1;
  P.out = send_dev;
  return launch_monitors(c, P, true);
}

extern "C" int qgcm_hip_monitors_combine(qgcm_hip_handle c, const double *gath_dev, int nranks, double *out) {
  if (check_ready(c, "qgcm_hip_monitors_combine")) return 1;
  if (!gath_dev || !out || nranks < 1) QG_FAIL("qgcm_hip_monitors_combine: need the gathered summaries, out and nranks >= 1");
  QgMonParams P;
  if (mon_params(c, P, "qgcm_hip_monitors_combine")) return 1;
  P.gath = gath_dev;
  P.nranks = nranks;
  auto &m = c->mon;
  const int nl = c->g.nl;
#define QG_MON(NLV) hipLaunchKernelGGL((k_monslab_combine<NLV>), dim3(1), dim3(256), 0, c->stream, P)
  QG_SWITCH_NL(nl, QG_MON, "k_mon");
#undef QG_MON
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(m.hout, m.out, sizeof(double) * (MON_LEN(nl) + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (m.hout[MON_LEN(nl)] != 0.0)
    QG_FAIL("qgcm_hip_monitors_combine: the gathered summaries do not tile rows 1..%d (rank %d of %d does not continue them)",
            c->g.nyg, (int)m.hout[MON_LEN(nl)] - 1, nranks);
  memcpy(out, m.hout, sizeof(double) * MON_LEN(nl));
  return 0;
}

// ---------------------------------------------------------------------------
// atmosphere monitors and valids: the atmosphere half of monnc_comp, courat and valids
// ---------------------------------------------------------------------------
// the handles the atmosphere's entry points serve: whole-domain atmosphere handles only (`ocean`: the calls that
// serve an ocean handle instead)
static int atm_only(qgcm_hip_ctx *c, const char *who, const char *ocean = "qgcm_hip_monitors / qgcm_hip_valids") {
  if (!c) QG_FAIL("%s: null handle", who);
  if (!c->g.atm) QG_FAIL("%s: the handle is an ocean (%s serve it)", who, ocean);
  if (!c->whole) QG_FAIL("%s: the handle is a y-slab (the atmosphere's diagnostics need the whole domain)", who);
  return check_ready(c, who);
}

extern "C" int qgcm_hip_atm_monitor_len(qgcm_hip_handle c) { return c && c->g.atm ? ATMON_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_set_atm_mon_params(qgcm_hip_handle c, const qgcm_hip_atm_mon_params *p) {
  if (atm_only(c, "qgcm_hip_set_atm_mon_params")) return 1;
  if (!p) QG_FAIL("qgcm_hip_set_atm_mon_params: null argument");
  const int nxt = c->g.nx - 1, nyt = c->g.ny - 1;
  if (p->nxaooc < 1 || p->nyaooc < 1 || p->nx1 < 1 || p->ny1 < 1 || p->nx1 + p->nxaooc - 1 > nxt ||
      p->ny1 + p->nyaooc - 1 > nyt)
    QG_FAIL("qgcm_hip_set_atm_mon_params: the ocean's cells nx1 = %d, ny1 = %d, nxaooc = %d, nyaooc = %d do not lie "
            "on the atmosphere's %d x %d T grid", p->nx1, p->ny1, p->nxaooc, p->nyaooc, nxt, nyt);
  c->atmon.prm = *p;
  c->atmon.prm_set = true;
  return 0;
}

extern "C" int qgcm_hip_set_atm_monitor_fields(qgcm_hip_handle c, const double *wekta, const double *tauxa,
                                               const double *tauya, const double *ast, const double *hmixa,
                                               const double *uekat, const double *vekat) {
  if (atm_only(c, "qgcm_hip_set_atm_monitor_fields")) return 1;
  const QgGeom &g = c->g;
  const int nxt = g.nx - 1, nyt = g.ny - 1;
  auto &m = c->atmon;
  if (!m.ldt) m.ldt = round_up(nxt, 16);
  // (field, device buffer, pitch, width, rows)
  struct F { const double *src; QgDbl *dst; int ld, nx, ny; } fs[] = {
      {wekta, &m.wekta, m.ldt, nxt, nyt}, {tauxa, &m.tauxa, g.ldx, g.nx, g.ny}, {tauya, &m.tauya, g.ldx, g.nx, g.ny},
      {uekat, &m.uekat, g.ldx, g.nx, nyt}, {vekat, &m.vekat, m.ldt, nxt, g.ny}};
  for (const F &f : fs)
    if (upload_field(c, *f.dst, f.ld, f.src, f.nx, f.ny)) return 1;
  // ast and hmixa: with the mixed layer on the device they go into its current level (what m.ast / m.hmixa point at),
  // without it into buffers of the monitors' own
  if (c->aml.diag) return (ast && upload2d(c, m.ast, m.ldt, ast, nxt, nyt)) || (hmixa && upload2d(c, m.hmixa, m.ldt, hmixa, nxt, nyt));
  if (upload_field(c, m.ast_own, m.ldt, ast, nxt, nyt) || upload_field(c, m.hmixa_own, m.ldt, hmixa, nxt, nyt)) return 1;
  m.ast = m.ast_own;
  m.hmixa = m.hmixa_own;
  return 0;
}

// the kernel parameters; `mon`: the monitors (constants, every field), else the valids (pa, qa, wekta, tauxa, tauya,
// ast).  Allocates the partials on first use.
static int atmon_params(qgcm_hip_ctx *c, QgAtmonParams &P, bool mon, const char *who) {
  if (atm_only(c, who)) return 1;
  auto &m = c->atmon;
  if (mon && !m.prm_set) QG_FAIL("%s: qgcm_hip_set_atm_mon_params has not been called", who);
  const char *miss = !m.wekta ? "wekta" : !m.tauxa ? "tauxa" : !m.tauya ? "tauya" : !m.ast ? "ast" : nullptr;
  if (!miss && mon) miss = !m.hmixa ? "hmixa" : !m.uekat ? "uekat" : !m.vekat ? "vekat" : nullptr;
  if (miss) QG_FAIL("%s: %s was never given (qgcm_hip_set_atm_monitor_fields)", who, miss);
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  const int nl = g.nl, nyt = g.ny - 1;
  if ((size_t)(g.nx > ATMON_CHUNK ? g.nx : ATMON_CHUNK) * sizeof(double) > 65536)
    QG_FAIL("%s: nxpa = %d exceeds the LDS row of k_atmon_chain", who, g.nx);
  memset(&P, 0, sizeof(P));
  P.g = g;
  // the time levels qgcm_hip_get_state hands out at this point of the loop (after an averaging step: the averaged ones)
  P.pa = c->p[c->ip]; P.pam = c->p[c->ip ^ 1]; P.qa = c->q[c->iq];
  P.wekpa = c->wekpo; P.entat = c->entoc;
  P.wekta = m.wekta; P.tauxa = m.tauxa; P.tauya = m.tauya; P.ast = m.ast; P.hmixa = m.hmixa; P.uekat = m.uekat;
  P.vekat = m.vekat;
  P.ldt = m.ldt;
  P.ntx = (g.nx + MON_TX - 1) / MON_TX;
  P.nblk = P.ntx * ((g.ny + MON_TY - 1) / MON_TY);
  if (m.psum.ensure((size_t)MON_NS(nl) * P.nblk, "the monitors' partial sums") ||
      m.pmin.ensure((size_t)MON_NM(nl) * P.nblk, "the monitors' partial extrema") ||
      m.chain.ensure((size_t)nyt * nl + 1, "the monitors' chain") || m.out.ensure(ATMON_LEN(nl), "the monitors' result") ||
      m.hout.ensure(ATMON_LEN(nl), "the monitors' pinned result"))
    return 1;
  P.psum = m.psum; P.pmin = m.pmin; P.chain = m.chain; P.out = m.out;
  // MODULE atconst as src/q-gcm.F:392-441 derives it; dta = tdta/2 exactly; atnorm: src/parameters_data.F:87
  P.dta = 0.5 * pr.tdto;
  P.rdxaf0 = 1.0 / (pr.dxo * pr.fnot);
  P.dxam2 = 1.0 / (pr.dxo * pr.dxo);
  P.hdxam1 = 0.5 / pr.dxo;
  P.atnorm = 1.0 / (double)((g.nx - 1) * nyt);
  const qgcm_hip_atm_mon_params &q = m.prm;
  P.rhoat = q.rhoat; P.cpat = q.cpat; P.hmat = q.hmat; P.davgat = q.davgat;
  P.bup = q.bup; P.cup = q.cup; P.dup = q.dup;
  P.nx1 = q.nx1; P.ny1 = q.ny1; P.nxaooc = q.nxaooc; P.nyaooc = q.nyaooc;
  for (int k = 0; k < nl - 1; ++k) { P.aup[k] = q.aup[k]; P.rgpat[k] = 1.0 / pr.gpoc[k]; P.gpat[k] = pr.gpoc[k]; }
  for (int k = 0; k < nl; ++k) { P.hat[k] = pr.hoc[k]; P.ah4at[k] = pr.ah4oc[k]; }
  return 0;
}

extern "C" int qgcm_hip_atm_monitors(qgcm_hip_handle c, double *out) {
  if (atm_only(c, "qgcm_hip_atm_monitors")) return 1;
  if (!out) QG_FAIL("qgcm_hip_atm_monitors: null argument");
  QgAtmonParams P;
  if (atmon_params(c, P, true, "qgcm_hip_atm_monitors")) return 1;
  const QgGeom &g = c->g;
  const int nl = g.nl, nyt = g.ny - 1;
  const size_t lds = sizeof(double) * (g.nx > ATMON_CHUNK ? g.nx : ATMON_CHUNK);
#define QG_ATMON(NLV)                                                                                 \
  hipLaunchKernelGGL((k_atmon_scan<NLV>), dim3(P.nblk), dim3(MON_NT), 0, c->stream, P);               \
  hipLaunchKernelGGL(k_atmon_chain, dim3(nyt * nl + 1), dim3(64), lds, c->stream, P);                 \
  hipLaunchKernelGGL((k_atmon_final<NLV>), dim3(1), dim3(MON_FT), 0, c->stream, P)
  QG_SWITCH_NL(nl, QG_ATMON, "k_atmon");
#undef QG_ATMON
  HIPCHECK(hipGetLastError());
  auto &m = c->atmon;
  HIPCHECK(hipMemcpyAsync(m.hout, m.out, sizeof(double) * ATMON_LEN(nl), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  memcpy(out, m.hout, sizeof(double) * ATMON_LEN(nl));
  return 0;
}

extern "C" int qgcm_hip_atm_valids(qgcm_hip_handle c, double *out, int *solnok) {
  if (atm_only(c, "qgcm_hip_atm_valids")) return 1;
  if (!out || !solnok) QG_FAIL("qgcm_hip_atm_valids: null argument");
  QgAtmonParams P;
  if (atmon_params(c, P, false, "qgcm_hip_atm_valids")) return 1;
  hipLaunchKernelGGL(k_atval, dim3(1), dim3(MON_FT), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  auto &m = c->atmon;
  HIPCHECK(hipMemcpyAsync(m.hout, m.out, sizeof(double) * ATVAL_N, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  memcpy(out, m.hout, sizeof(double) * ATVAL_N);
  // the limits of src/valsubs.F:78-97: patext, qatext, astext, wtaext, tauext (tauxa and tauya share theirs)
  static const double ext[6] = {1.0e7, 0.05, 90.0, 1.0, 10.0, 10.0};
  int ok = 1;
  for (int f = 0; f < 6; ++f)
    if (fabs(out[2 * f]) >= ext[f] || fabs(out[2 * f + 1]) >= ext[f]) ok = 0;
  *solnok = ok;
  return 0;
}

// ---------------------------------------------------------------------------
// start-up / restart arithmetic and the progress sample on the device
// ---------------------------------------------------------------------------
// the trapezoid sums over the owned rows (k_area_partial); with `final` also their reduction into c->area_out
static int launch_area_sums(qgcm_hip_ctx *c, bool final = true) {
  const QgGeom &g = c->g;
  if (c->area_part.ensure((size_t)AREA_NB * 3 * QG_MAXL, "the area integrals' partials") ||
      c->area_out.ensure((size_t)3 * QG_MAXL, "the area integrals"))
    return 1;
  QgAreaParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.f[0] = c->p[c->ip]; P.f[1] = c->p[c->ip ^ 1]; P.f[2] = c->q[c->iq];
  P.part = c->area_part; P.out = c->area_out;
  P.jlo = g.jlo; P.jhi = g.jhi;
#define QG_AREA(NLV)                                                                          \
  hipLaunchKernelGGL((k_area_partial<NLV>), dim3(AREA_NB), dim3(AREA_NT), 0, c->stream, P);     \
  if (final) hipLaunchKernelGGL((k_area_final<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_AREA, "k_area");
#undef QG_AREA
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_init_from_p(qgcm_hip_handle c) {
  if (check_ready(c, "qgcm_hip_init_from_p")) return 1;
  if (!c->whole) QG_FAIL("qgcm_hip_init_from_p: only for a handle that owns the whole domain");
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  // constr: src/q-gcm.F:711
  if (launch_area_sums(c)) return 1;
  {
    QgConstrInitParams P;
    memset(&P, 0, sizeof(P));
    P.g = g;
    P.po = c->p[c->ip]; P.pom = c->p[c->ip ^ 1]; P.area = c->area_out; P.sc = c->sc;
    P.dxo = pr.dxo; P.dyo = pr.dyo; P.fnot = pr.fnot;
    for (int i = 0; i < g.nl * g.nl; ++i) P.amat[i] = pr.amatoc[i];
#define QG_CINIT(NLV) hipLaunchKernelGGL((k_constr_init<NLV>), dim3(1), dim3(64), 0, c->stream, P)
    QG_SWITCH_NL(g.nl, QG_CINIT, "k_constr_init");
#undef QG_CINIT
    HIPCHECK(hipGetLastError());
  }
  // qcomp, ocqbdy / atqzbd, merqcy for both time levels: src/q-gcm.F:719-731, 738-749
  for (int t = 0; t < 2; ++t) {
    QgQcompParams Q;
    memset(&Q, 0, sizeof(Q));
    Q.g = g;
    Q.p = c->p[t ? c->ip ^ 1 : c->ip];
    Q.q = c->q[t ? c->iq ^ 1 : c->iq];
    Q.ddyn = c->ddynoc; Q.yporel = c->yporel;
    Q.dx2fac = (1.0 / (pr.dxo * pr.dxo)) / pr.fnot;
    Q.beta = pr.beta; Q.fnot = pr.fnot;
    for (int i = 0; i < g.nl * g.nl; ++i) Q.amat[i] = pr.amatoc[i];
    Q.ktopo = g.atm ? 0 : g.nl - 1;
    hipLaunchKernelGGL(k_qcomp, dim3((g.nx + 255) / 256, g.ny - 2, g.nl), dim3(256), 0, c->stream, Q);
    QgBdyParams B;
    fill_bdy_params(c, B);
    B.po = Q.p;
    B.qo = Q.q;
    const int nmax = g.nx > g.ny ? g.nx : g.ny;
    hipLaunchKernelGGL(k_ocqbdy, dim3((nmax + 255) / 256, g.cyc ? 2 : 4, g.nl), dim3(256), 0, c->stream, B);
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

extern "C" int qgcm_hip_wekpo_from_tau(qgcm_hip_handle c, const double *tauxo, const double *tauyo) {
  if (check_ready(c, "qgcm_hip_wekpo_from_tau")) return 1;
  if (!tauxo || !tauyo) QG_FAIL("qgcm_hip_wekpo_from_tau: null argument");
  if (!c->whole) QG_FAIL("qgcm_hip_wekpo_from_tau: only for a handle that owns the whole domain");
  const QgGeom &g = c->g;
  const int nyt = g.ny - 1;
  QgWekParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  QgDbl stx, sty, swt; // scratch without the device mixed layer: with it the stress and wekto live in its arrays
  double *tx, *ty, *wt;
  if (!c->oml.on) {
    P.ldt = round_up(g.nxt, 16);
    if (stx.alloc((size_t)g.ldx * g.ny, "the scratch stress") || sty.alloc((size_t)g.ldx * g.ny, "the scratch stress") ||
        swt.alloc((size_t)P.ldt * nyt, "the scratch wekto"))
      return 1;
    tx = stx; ty = sty; wt = swt;
  } else {
    tx = c->oml.taux; ty = c->oml.tauy; wt = c->oml.wekto;
    P.ldt = c->oml.ldt;
  }
  int rc = upload2d(c, tx, g.ldx, tauxo, g.nx, g.ny) || upload2d(c, ty, g.ldx, tauyo, g.nx, g.ny);
  if (!rc) {
    P.taux = tx; P.tauy = ty; P.wekto = wt; P.wekpo = c->wekpo;
    P.hxofac = 0.5 * (1.0 / (c->prm.dxo * c->prm.fnot)); // src/xfosubs.F:138 with rdxof0 of src/q-gcm.F:435
    hipLaunchKernelGGL(k_wekto, dim3((g.nxt + 255) / 256, nyt), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(k_wekpo, dim3((g.nx + 255) / 256, g.ny), dim3(256), 0, c->stream, P);
    rc = hipGetLastError() != hipSuccess;
    if (rc) snprintf(g_err, sizeof(g_err), "qgcm_hip_wekpo_from_tau: launch failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = 1;
  }
  return rc;
}

extern "C" int qgcm_hip_prsamp(qgcm_hip_handle c, double *out) {
  if (check_ready(c, "qgcm_hip_prsamp")) return 1;
  if (!out) QG_FAIL("qgcm_hip_prsamp: null argument");
  if (!c->whole) QG_FAIL("qgcm_hip_prsamp: only for a handle that owns the whole domain (y-slabs: qgcm_hip_prsamp_part / _combine)");
  const QgGeom &g = c->g;
  const int nl = g.nl;
  if (launch_area_sums(c)) return 1;
  double area[3 * QG_MAXL];
  HIPCHECK(hipMemcpyAsync(area, c->area_out, sizeof(double) * 3 * nl, hipMemcpyDeviceToHost, c->stream));
  const int nxco = (g.nx + 1) / 2, nyco = (g.ny + 1) / 2; // src/q-gcm.F:1974-1975
  const long oc = (long)(nyco - 1) * g.ldx + (nxco - 1);
  for (int k = 0; k < nl; ++k) {
    HIPCHECK(hipMemcpyAsync(out + k, c->p[c->ip] + g.fstride * k + oc, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(out + nl + k, c->q[c->iq] + g.fstride * k + oc, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHECK(hipStreamSynchronize(c->stream));
  const double ocnorm = 1.0 / ((double)g.nxt * (double)(g.ny - 1)); // src/parameters_data.F:88
  for (int k = 0; k < nl; ++k) {
    out[2 * nl + k] = area[k] * ocnorm;          // pavgoc
    out[3 * nl + k] = area[2 * nl + k] * ocnorm; // qavgoc
  }
  out[4 * nl] = 1.0e30;
  out[4 * nl + 1] = -1.0e30;
  if (c->oml.on) {
    double v[14 + QG_MAXL];
    int ok = 0;
    if (qgcm_hip_valids(c, v, &ok)) return 1;
    out[4 * nl] = v[4];     // min, max of sst (layout of qgcm_hip_valids)
    out[4 * nl + 1] = v[5];
  }
  return 0;
}

extern "C" int qgcm_hip_prsamp_part_len(qgcm_hip_handle c) { return c ? PRS_PART_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_prsamp_part(qgcm_hip_handle c, double *send_dev) {
  if (check_ready(c, "qgcm_hip_prsamp_part")) return 1;
  if (!send_dev) QG_FAIL("qgcm_hip_prsamp_part: null argument");
  const QgGeom &g = c->g;
  if (g.nl < 2 || g.nl > QG_MAXL) QG_FAIL("qgcm_hip_prsamp_part: unsupported nlo");
  if (launch_area_sums(c, false)) return 1;
  QgPrsampParams P;
  memset(&P, 0, sizeof(P));
  if (c->oml.on) { // min, max of sst: this rank's valids summary
    QgValidsParams V;
    if (launch_valids_scan(c, V, "qgcm_hip_prsamp_part")) return 1;
    if (c->val_sum.ensure((size_t)VAL_PART_LEN(QG_MAXL), "the valids summary")) return 1;
    V.out = c->val_sum;
#define QG_VALIDS(NLV) hipLaunchKernelGGL((k_valids_part<NLV>), dim3(1), dim3(VAL_NT), 0, c->stream, V)
    QG_SWITCH_NL(g.nl, QG_VALIDS, "k_valids");
#undef QG_VALIDS
    P.vsum = c->val_sum;
  }
  P.g = g;
  P.po = c->p[c->ip];
  P.qo = c->q[c->iq];
  P.area_part = c->area_part;
  P.jlo = g.jlo; P.jhi = g.jhi;
  P.out = send_dev;
#define QG_PRS(NLV) hipLaunchKernelGGL((k_prsamp_part<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_PRS, "k_prsamp");
#undef QG_PRS
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_prsamp_combine(qgcm_hip_handle c, const double *gath_dev, int nranks, double *out) {
  if (check_ready(c, "qgcm_hip_prsamp_combine")) return 1;
  if (!gath_dev || !out || nranks < 1) QG_FAIL("qgcm_hip_prsamp_combine: need the gathered summaries, out and nranks >= 1");
  const QgGeom &g = c->g;
  const int nl = g.nl;
  if (nl < 2 || nl > QG_MAXL) QG_FAIL("qgcm_hip_prsamp_combine: unsupported nlo");
  if (c->prs_out.ensure((size_t)4 * QG_MAXL + 3, "prsamp's result")) return 1;
  QgPrsampParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.out = c->prs_out;
  P.gath = gath_dev;
  P.nranks = nranks;
  P.ocnorm = 1.0 / ((double)g.nxt * (double)(g.nyg - 1)); // src/parameters_data.F:88
#define QG_PRS(NLV) hipLaunchKernelGGL((k_prsamp_combine<NLV>), dim3(1), dim3(64), 0, c->stream, P)
  QG_SWITCH_NL(nl, QG_PRS, "k_prsamp");
#undef QG_PRS
  HIPCHECK(hipGetLastError());
  double h[4 * QG_MAXL + 3];
  HIPCHECK(hipMemcpyAsync(h, c->prs_out, sizeof(double) * (4 * nl + 3), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (h[4 * nl + 2] != 0.0)
    QG_FAIL("qgcm_hip_prsamp_combine: the gathered summaries do not tile rows 1..%d (rank %d of %d does not continue them)",
            g.nyg, (int)h[4 * nl + 2] - 1, nranks);
  memcpy(out, h, sizeof(double) * (4 * nl + 2));
  return 0;
}

// ---------------------------------------------------------------------------
// time averages of the ocean (k_tavg.h): the fork's running mean of po (avg_ocn_k247 / ocnc_avgout_k247)
// and tavocn / tavout.  A y-slab handle sums and returns its owned rows.
// ---------------------------------------------------------------------------
static int tav_ready(qgcm_hip_ctx *c, const char *who) {
  if (check_ready(c, who)) return 1;
  if (c->g.atm) QG_FAIL("%s: the handle is an atmosphere (only the ocean's time averages are implemented)", who);
  return 0;
}

// po(:, owned rows, :) into the sum (asynchronous); counts the contribution.  Nothing while the sum is off.
static int launch_poavg(qgcm_hip_ctx *c) {
  if (!c->poavg.on) return 0;
  const QgGeom &g = c->g;
  const long n2 = (long)(g.jhi - g.jlo + 1) * g.ldx / 2;
  const unsigned nb = (unsigned)std::min<long>((n2 + TAV_NT - 1) / TAV_NT, 4096);
  KTimer t(c, KN_POAVG);
  hipLaunchKernelGGL(k_poavg_add, dim3(nb, g.nl), dim3(TAV_NT), 0, c->stream, c->poavg.sum, (const double *)c->p[c->ip],
                     (long)(g.jlo - 1) * g.ldx, n2, g.fstride);
  HIPCHECK(hipGetLastError());
  c->poavg.n++;
  return 0;
}

extern "C" int qgcm_hip_poavg_enable(qgcm_hip_handle c, int on) {
  if (tav_ready(c, "qgcm_hip_poavg_enable")) return 1;
  auto &a = c->poavg;
  if (on && !a.on) { // the sum starts at zero
    const size_t n = (size_t)c->g.fstride * c->g.nl;
    if (a.sum.ensure(n, "the running sum of po")) return 1;
    HIPCHECK(hipMemsetAsync(a.sum, 0, n * sizeof(double), c->stream));
    a.n = 0;
  }
  a.on = on != 0;
  return 0;
}

// owned rows of `nf` fields of fstride doubles at src into dense (nx_out, rows, nf) host arrays
static int download_owned(qgcm_hip_ctx *c, double *dst, const double *src, int nx_out, int j0, int rows, int nf) {
  const QgGeom &g = c->g;
  for (int k = 0; k < nf; ++k)
    if (download2d(c, dst + (size_t)k * nx_out * rows, src + (size_t)k * g.fstride + (size_t)(j0 - 1) * g.ldx, g.ldx,
                   nx_out, rows))
      return 1;
  return 0;
}

extern "C" int qgcm_hip_poavg_out(qgcm_hip_handle c, double *po_avg, int *nsum, int reset) {
  if (tav_ready(c, "qgcm_hip_poavg_out")) return 1;
  auto &a = c->poavg;
  if (po_avg) {
    if (!a.sum || a.n == 0) QG_FAIL("qgcm_hip_poavg_out: no step has been summed (qgcm_hip_poavg_enable)");
    const QgGeom &g = c->g;
    const int rows = g.jhi - g.jlo + 1;
    if (download_owned(c, po_avg, a.sum, g.nx, g.jlo, rows, g.nl)) return 1;
    const double rnsum = 1.0 / (double)a.n; // src/nc_subs.F: rnsum = 1.0d0 / dble( nsum_ocavg ), then rnsum * po_avg
    const size_t n = (size_t)g.nx * rows * g.nl;
    for (size_t i = 0; i < n; ++i) po_avg[i] = rnsum * po_avg[i];
  }
  if (nsum) *nsum = (int)a.n;
  if (reset && a.sum) {
    HIPCHECK(hipMemsetAsync(a.sum, 0, (size_t)c->g.fstride * c->g.nl * sizeof(double), c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    a.n = 0;
  }
  return 0;
}

extern "C" int qgcm_hip_set_tav_params(qgcm_hip_handle c, const qgcm_hip_tav_params *p) {
  if (!c || !p) QG_FAIL("qgcm_hip_set_tav_params: null argument");
  if (!(p->hmoc > 0.0)) QG_FAIL("qgcm_hip_set_tav_params: need hmoc > 0");
  c->tav.prm = *p;
  c->tav.prm_set = true;
  return 0;
}

// fnetoc / fnetat (T grid) for a handle whose fluid has no mixed layer on the device
static int tav_set_fnet(qgcm_hip_ctx *c, const double *fnet, int ldt) {
  return upload_field(c, c->tav.fnet, ldt, fnet, c->g.nxt, c->g.ny - 1);
}

extern "C" int qgcm_hip_set_tav_fields(qgcm_hip_handle c, const double *fnetoc) {
  if (tav_ready(c, "qgcm_hip_set_tav_fields")) return 1;
  return tav_set_fnet(c, fnetoc, round_up(c->g.nxt, 16));
}

// the rows and the sums of one contribution (tavocn or tavatm); allocates the sums on first use
static int tav_accum_params(qgcm_hip_ctx *c, QgTavParams &P) {
  const QgGeom &g = c->g;
  // the time levels qgcm_hip_get_state hands out here: after an averaging step, the averaged ones
  P.po = c->p[c->ip]; P.qo = c->q[c->iq];
  P.jlo = g.jlo; P.jhi = g.jhi; P.jt1 = owned_t1(g); // (a whole-domain handle: 1, ny, ny - 1)
  if (!c->tav.sum) {
    if (c->tav.sum.alloc((size_t)TAV_NSUM(g.nl) * g.fstride, "the time averages' sums")) return 1;
    c->tav.n = 0;
  }
  P.sum = c->tav.sum;
  return 0;
}

static int tav_params(qgcm_hip_ctx *c, QgTavParams &P, const char *who) {
  if (tav_ready(c, who)) return 1;
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  memset(&P, 0, sizeof(P));
  P.g = g;
  qgcm_hip_tav_params q;
  if (c->tav.prm_set) {
    q = c->tav.prm;
  } else if (c->oml.on) {
    const qgcm_hip_oml_params &o = c->oml.prm;
    q.hmoc = o.hmoc; q.ycexp = o.ycexp; q.tsbdy = o.tsbdy; q.tnbdy = o.tnbdy; q.sb_hflux = o.sb_hflux; q.nb_hflux = o.nb_hflux;
  } else {
    QG_FAIL("%s: qgcm_hip_set_tav_params has not been called and the mixed layer is off", who);
  }
  QgSurf S;
  if (surf_fields(c, kSurfAll, S, who)) return 1;
  P.taux = S.taux; P.tauy = S.tauy; P.wekto = S.wekto; P.sst = S.sst; P.ldt = S.ldt;
  // fnetoc: the mixed layer's own, else that of qgcm_hip_set_tav_fields (zero if never set)
  P.fnet = c->oml.on ? c->oml.fnet : c->tav.fnet;
  P.wekpo = c->wekpo;
  const double rdxof0 = 1.0 / (pr.dxo * pr.fnot); // src/q-gcm.F:436
  P.uvgfac = q.ycexp * rdxof0;                    // src/timavge.F:447-448
  P.rhf0hm = 0.5 / (pr.fnot * q.hmoc);
  P.tsbdy = q.tsbdy; P.tnbdy = q.tnbdy;
  if (tav_accum_params(c, P)) return 1;
  // (the flags select the template; kept here so that launch_tavocn needs nothing else)
  P.mask = (q.sb_hflux ? 1u : 0u) | (q.nb_hflux ? 2u : 0u);
  return 0;
}

extern "C" int qgcm_hip_tavocn(qgcm_hip_handle c) {
  QgTavParams P;
  if (tav_params(c, P, "qgcm_hip_tavocn")) return 1;
  const QgGeom &g = c->g;
  const bool sb = P.mask & 1u, nb = P.mask & 2u;
  P.mask = 0;
  const dim3 grid((g.nx + TAV_NT - 1) / TAV_NT, g.jhi - g.jlo + 1);
#define QG_TAV3(NLV, CY)                                                                                   \
  if (sb && nb) hipLaunchKernelGGL((k_tav_accum<NLV, CY, true, true>), grid, dim3(TAV_NT), 0, c->stream, P);       \
  else if (sb) hipLaunchKernelGGL((k_tav_accum<NLV, CY, true, false>), grid, dim3(TAV_NT), 0, c->stream, P);       \
  else if (nb) hipLaunchKernelGGL((k_tav_accum<NLV, CY, false, true>), grid, dim3(TAV_NT), 0, c->stream, P);       \
  else hipLaunchKernelGGL((k_tav_accum<NLV, CY, false, false>), grid, dim3(TAV_NT), 0, c->stream, P)
#define QG_TAV(NLV)         \
  if (g.cyc) {              \
    QG_TAV3(NLV, true);     \
  } else {                  \
    QG_TAV3(NLV, false);    \
  }
  QG_SWITCH_NL(g.nl, QG_TAV, "k_tav_accum");
#undef QG_TAV
#undef QG_TAV3
  HIPCHECK(hipGetLastError());
  c->tav.n++; // nsumoc = nsumoc + 1
  return 0;
}

// the sums and their count back to zero
static int tav_reset(qgcm_hip_ctx *c) {
  if (c->tav.sum) HIPCHECK(hipMemsetAsync(c->tav.sum, 0, (size_t)TAV_NSUM(c->g.nl) * c->g.fstride * sizeof(double), c->stream));
  c->tav.n = 0;
  return 0;
}

extern "C" int qgcm_hip_tav_reset(qgcm_hip_handle c) { return tav_ready(c, "qgcm_hip_tav_reset") || tav_reset(c); }

// tavout for the handle's fluid: the means of the selected outputs (the rows this handle owns) and the count
static int tav_out(qgcm_hip_ctx *c, double *const *fields, int *nsum) {
  if (nsum) *nsum = (int)c->tav.n;
  if (!fields) return 0;
  const QgGeom &g = c->g;
  const int nl = g.nl;
  // the ocean's 16 outputs -> (first field of the mean buffer, number of fields, p or T rows, columns); the
  // atmosphere's 15 are these without wekpo (tavatm keeps no Ekman-pumping sum, k_atm_tavg.h)
  struct Out { int f, nf; bool trow; int nx; };
  const int u = TAV_UU(nl), e = TAV_NSUM(nl);
  const Out all[QGCM_HIP_TAV_NOUT] = {{TAV_TX, 1, false, g.nx}, {TAV_TY, 1, false, g.nx}, {TAV_WP, 1, false, g.nx},
                                      {TAV_WT, 1, true, g.nxt}, {TAV_FM, 1, true, g.nxt}, {TAV_SST, 1, true, g.nxt},
                                      {TAV_P0, nl, false, g.nx}, {TAV_P0 + nl, nl, false, g.nx},
                                      {u, 1, true, g.nx}, {u + 1, 1, true, g.nx}, {u + 2, 1, true, g.nx},
                                      {u + 3, 1, false, g.nxt}, {u + 4, 1, false, g.nxt}, {u + 5, 1, false, g.nxt},
                                      {e, 1, true, g.nx}, {e + 1, 1, false, g.nxt}};
  Out map[QGCM_HIP_TAV_NOUT];
  int nout = 0;
  for (const Out &o : all)
    if (!(g.atm && o.f == TAV_WP)) map[nout++] = o;
  unsigned mask = 0;
  for (int o = 0; o < nout; ++o)
    if (fields[o])
      for (int k = 0; k < map[o].nf; ++k) mask |= 1u << (map[o].f + k);
  if (!mask) return 0;
  if (c->tav.mean.ensure((size_t)TAV_NMEAN(nl) * g.fstride, "the time averages' means")) return 1;
  if (c->tav.sum.ensure((size_t)TAV_NSUM(nl) * g.fstride, "the time averages' sums")) return 1;
  QgTavParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.jlo = g.jlo; P.jhi = g.jhi; P.jt1 = owned_t1(g);
  P.sum = c->tav.sum; P.mean = c->tav.mean; P.mask = mask;
  P.rnsoc = c->tav.n == 0 ? 0.0 : 1.0 / (double)c->tav.n; // rnsoc, src/timavge.F:723-727; rnsat, src/timavge.F:716-720
  const int np = g.jhi - g.jlo + 1, nt = owned_t1(g) - g.jlo + 1;
  const dim3 grid((g.nx + TAV_NT - 1) / TAV_NT, np);
#define QG_TAVM(NLV) hipLaunchKernelGGL((k_tav_mean<NLV>), grid, dim3(TAV_NT), 0, c->stream, P)
  QG_SWITCH_NL(nl, QG_TAVM, "k_tav_mean");
#undef QG_TAVM
  HIPCHECK(hipGetLastError());
  for (int o = 0; o < nout; ++o)
    if (fields[o] && download_owned(c, fields[o], c->tav.mean + (size_t)map[o].f * g.fstride, map[o].nx, g.jlo,
                                    map[o].trow ? nt : np, map[o].nf))
      return 1;
  return 0;
}

extern "C" int qgcm_hip_tav_out(qgcm_hip_handle c, double *const *fields, int *nsumoc) {
  return tav_ready(c, "qgcm_hip_tav_out") || tav_out(c, fields, nsumoc);
}

// ---------------------------------------------------------------------------
// periodic ocean dumps (k_qocdiag.h): qocdiag_out's vorticity budget and ocnc_out's subsample.  A y-slab
// handle computes the subsample rows it owns.
// ---------------------------------------------------------------------------
// points of a subsample of n points: the reference's min(mod(n,nsko),1) + (n-mod(n,nsko))/nsko (src/qocdiag.F:360-363)
static int qd_count(int n, int nsko) {
  const int m = n % nsko;
  return std::min(m, 1) + (n - m) / nsko;
}

// subsample rows [m0, m1) (0-based: global row 1 + m*nsko) among the global rows g0..g1
static void qd_rows(int g0, int g1, int nsko, int *m0, int *m1) {
  *m0 = (g0 - 1 + nsko - 1) / nsko;
  *m1 = std::max(*m0, (g1 - 1) / nsko + 1);
}

static int qd_ready(qgcm_hip_ctx *c, int nsko, const char *who) {
  if (check_ready(c, who)) return 1;
  if (c->g.atm) QG_FAIL("%s: the handle is an atmosphere (only the ocean's dumps are implemented)", who);
  if (nsko < 1) QG_FAIL("%s: nsko = %d (need >= 1)", who, nsko);
  return 0;
}

static size_t qd_len(const qgcm_hip_ctx *c, int nsko) {
  const QgGeom &g = c->g;
  int m0, m1;
  qd_rows(g.jlo + g.joff, g.jhi + g.joff, nsko, &m0, &m1);
  return (size_t)QD_NTERM * g.nl * (m1 - m0) * qd_count(g.nx, nsko);
}

// the dumps' result buffer, grown on demand (the stream is drained first: a dump in flight may still write the old one)
static int qd_grow(qgcm_hip_ctx *c, size_t n) {
  if (c->qd.buf.size() < n) HIPCHECK(hipStreamSynchronize(c->stream));
  return c->qd.buf.grow(n, "the dumps' result buffer");
}

// the budget of the state on the device into out (device, qd_len doubles); asynchronous
static int launch_qocdiag(qgcm_hip_ctx *c, int nsko, double *out) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  QgQocdiagParams P;
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.pom = c->p[c->ip ^ 1]; P.po = c->p[c->ip]; P.qo = c->q[c->iq]; P.qom = c->q[c->iq ^ 1];
  P.wekpo = c->wekpo; P.entoc = c->entoc; P.out = out;
  int m0, m1;
  qd_rows(g.jlo + g.joff, g.jhi + g.joff, nsko, &m0, &m1);
  if (m1 == m0) return 0; // no subsample row on this slab
  P.nsko = nsko; P.ipwk = qd_count(g.nx, nsko); P.jpn = m1 - m0; P.m0 = m0;
  P.jlo = g.jlo; P.jhi = g.jhi;
  // scalar prologue, src/qocdiag.F:369-380 (dxom2 = 1/dxo**2 of occonst, rdto = 1/dto with dto = tdto/2 exactly)
  P.adfaco = 1.0 / (12.0 * pr.dxo * pr.dyo * pr.fnot);
  P.dxom2 = 1.0 / (pr.dxo * pr.dxo);
  P.bcfaco = pr.bccooc * P.dxom2 / (0.5 * pr.bccooc + 1.0);
  P.fohfac[0] = pr.fnot / pr.hoc[0];
  P.fohfac[1] = pr.fnot / pr.hoc[1];
  P.bdrfac = 0.5 * (pr.fnot >= 0.0 ? 1.0 : -1.0) * pr.delek / pr.hoc[g.nl - 1];
  P.rdto = 1.0 / (0.5 * pr.tdto);
  for (int k = 0; k < g.nl; ++k) {
    P.ah2fac[k] = pr.ah2oc[k] / pr.fnot;
    P.ah4fac[k] = pr.ah4oc[k] / pr.fnot;
  }
  P.ntx = (g.nx + QD_TX - 1) / QD_TX;
  const int nty = (g.jhi - g.jlo + 1 + QD_TY - 1) / QD_TY;
  const dim3 grid(P.ntx * nty, 1, g.nl);
  if (g.cyc) hipLaunchKernelGGL(k_qocdiag<true>, grid, dim3(QD_NT), 0, c->stream, P);
  else hipLaunchKernelGGL(k_qocdiag<false>, grid, dim3(QD_NT), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int qgcm_hip_subsample_rows(qgcm_hip_handle c, int nsko, int *mp0, int *mp1, int *mt0, int *mt1) {
  if (qd_ready(c, nsko, "qgcm_hip_subsample_rows")) return 1;
  const QgGeom &g = c->g;
  int a, b;
  qd_rows(g.jlo + g.joff, g.jhi + g.joff, nsko, &a, &b);
  if (mp0) *mp0 = a;
  if (mp1) *mp1 = b;
  qd_rows(g.jlo + g.joff, owned_t1(g) + g.joff, nsko, &a, &b);
  if (mt0) *mt0 = a;
  if (mt1) *mt1 = b;
  return 0;
}

extern "C" long qgcm_hip_qocdiag_len(qgcm_hip_handle c, int nsko) {
  if (qd_ready(c, nsko, "qgcm_hip_qocdiag_len")) return -1;
  return (long)qd_len(c, nsko);
}

extern "C" int qgcm_hip_qocdiag(qgcm_hip_handle c, int nsko, double *out) {
  if (qd_ready(c, nsko, "qgcm_hip_qocdiag")) return 1;
  if (!out) QG_FAIL("qgcm_hip_qocdiag: null argument");
  const size_t n = qd_len(c, nsko);
  if (n == 0) return 0;
  if (qd_grow(c, n) || launch_qocdiag(c, nsko, c->qd.buf)) return 1;
  HIPCHECK(hipMemcpyAsync(out, c->qd.buf, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// one_step of a dump step: the budget after the step's oml, before its tendency, into the next ring slot
static int qd_record(qgcm_hip_ctx *c, int s) {
  auto &q = c->qd;
  if (q.count >= q.cap) QG_FAIL("qgcm_hip_steps: the dump ring is full at step %d", s); // (steps_impl checks first)
  const int slot = (q.head + q.count) % q.cap;
  if (launch_qocdiag(c, q.nsko, q.ring + (size_t)slot * q.len)) return 1;
  q.steps[slot] = s;
  q.count++;
  return 0;
}

extern "C" int qgcm_hip_qocdiag_schedule(qgcm_hip_handle c, int nsko, int every, int capacity) {
  if (check_ready(c, "qgcm_hip_qocdiag_schedule")) return 1;
  auto &q = c->qd;
  if (every != 0) {
    if (qd_ready(c, nsko, "qgcm_hip_qocdiag_schedule")) return 1;
    if (!c->whole) QG_FAIL("qgcm_hip_qocdiag_schedule: this handle is a y-slab; the scheduled dump is whole-domain only (call qgcm_hip_qocdiag between slab steps)");
    if (every < 0 || capacity < 1) QG_FAIL("qgcm_hip_qocdiag_schedule: need every >= 0 and capacity >= 1");
  }
  // the old schedule goes, with what its ring still holds (a dump in flight may still write the ring: drained first)
  if (q.ring) HIPCHECK(hipStreamSynchronize(c->stream));
  c->sched[SCH_DUMP] = {};
  q.cap = q.head = q.count = q.nsko = 0;
  q.len = 0;
  q.steps.clear();
  if (every == 0) {
    q.ring.reset();
    return 0;
  }
  const size_t len = qd_len(c, nsko);
  if (q.ring.grow(len * (size_t)capacity, "the dump ring")) return 1;
  q.nsko = nsko; q.cap = capacity; q.len = len;
  c->sched[SCH_DUMP] = {every, 1 % every}; // after every step s with (s - 1) % every == 0
  q.steps.assign(capacity, 0);
  return 0;
}

extern "C" int qgcm_hip_qocdiag_read(qgcm_hip_handle c, double *out, int *steps_out, int max, int *nread) {
  if (check_ready(c, "qgcm_hip_qocdiag_read")) return 1;
  if (!nread) QG_FAIL("qgcm_hip_qocdiag_read: null argument");
  auto &q = c->qd;
  if (max <= 0) { // a query: how many snapshots are unread
    *nread = q.count;
    return 0;
  }
  if (!out) QG_FAIL("qgcm_hip_qocdiag_read: null argument");
  const int n = std::min(max, q.count);
  for (int r = 0; r < n; ++r) {
    const int slot = (q.head + r) % q.cap;
    HIPCHECK(hipMemcpyAsync(out + (size_t)r * q.len, q.ring + (size_t)slot * q.len, q.len * sizeof(double),
                            hipMemcpyDeviceToHost, c->stream));
    if (steps_out) steps_out[r] = q.steps[slot];
  }
  HIPCHECK(hipStreamSynchronize(c->stream));
  q.head = q.cap ? (q.head + n) % q.cap : 0;
  q.count -= n;
  *nread = n;
  return 0;
}

// The fields of ocnc_out and atnc_out (src/nc_subs.F:1133-1322) in their order - sst, po, qo, wekto, h, tauxo, tauyo,
// and for the atmosphere hmixa - as (T grid?, planes; 0 planes: not selected).  The flags are outfloc(1..6) resp.
// outflat(1..7): the two stresses share flag 6, and ocnc_out does not read outfloc(7) (src/nc_subs.F:1067).
struct QdField { bool tgrid; int nplanes; };
enum { DUMP_MAXF = 8 };
static int dump_fields(const qgcm_hip_ctx *c, const int *flags, QdField f[DUMP_MAXF]) {
  const int nl = c->g.nl, nf = c->g.atm ? 8 : 7;
  const QdField all[DUMP_MAXF] = {{true, 1}, {false, nl}, {false, nl}, {true, 1}, {false, nl - 1}, {false, 1}, {false, 1}, {true, 1}};
  static const int flag[DUMP_MAXF] = {0, 1, 2, 3, 4, 5, 5, 6};
  for (int n = 0; n < nf; ++n) {
    f[n] = all[n];
    if (flags[flag[n]] != 1) f[n].nplanes = 0;
  }
  return nf;
}

// doubles of the selected fields' subsample on the rows this handle owns
static size_t dump_len(const qgcm_hip_ctx *c, int nsk, const int *flags) {
  const QgGeom &g = c->g;
  QdField f[DUMP_MAXF];
  const int nf = dump_fields(c, flags, f);
  int p0, p1, t0, t1;
  qd_rows(g.jlo + g.joff, g.jhi + g.joff, nsk, &p0, &p1);
  qd_rows(g.jlo + g.joff, owned_t1(g) + g.joff, nsk, &t0, &t1);
  const size_t np = (size_t)qd_count(g.nx, nsk) * (p1 - p0), nt = (size_t)qd_count(g.nxt, nsk) * (t1 - t0);
  size_t n = 0;
  for (int k = 0; k < nf; ++k) n += (size_t)f[k].nplanes * (f[k].tgrid ? nt : np);
  return n;
}

extern "C" long qgcm_hip_ocnc_sample_len(qgcm_hip_handle c, int nsko, const int *outfloc) {
  if (qd_ready(c, nsko, "qgcm_hip_ocnc_sample_len")) return -1;
  if (!outfloc) { snprintf(g_err, sizeof(g_err), "qgcm_hip_ocnc_sample_len: null argument"); return -1; }
  return (long)dump_len(c, nsko, outfloc);
}

extern "C" int qgcm_hip_ocnc_sample(qgcm_hip_handle c, int nsko, const int *outfloc, double *out) {
  if (qd_ready(c, nsko, "qgcm_hip_ocnc_sample")) return 1;
  if (!outfloc || !out) QG_FAIL("qgcm_hip_ocnc_sample: null argument");
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  QdField f[DUMP_MAXF];
  const int nf = dump_fields(c, outfloc, f);
  // the surface fields among the selected ones, in ocnc_out's order
  static const int surf[4][2] = {{0, SF_SST}, {3, SF_WEKTO}, {5, SF_TAUX}, {6, SF_TAUY}};
  int need[5], nn = 0;
  for (const auto &sf : surf)
    if (f[sf[0]].nplanes) need[nn++] = sf[1];
  need[nn] = SF_END;
  QgSurf F;
  if (surf_fields(c, need, F, "qgcm_hip_ocnc_sample")) return 1;
  const size_t n = dump_len(c, nsko, outfloc);
  if (n == 0) return 0;
  if (qd_grow(c, n)) return 1;
  int p0, p1, t0, t1;
  qd_rows(g.jlo + g.joff, g.jhi + g.joff, nsko, &p0, &p1);
  qd_rows(g.jlo + g.joff, owned_t1(g) + g.joff, nsko, &t0, &t1);
  const double *po = c->p[c->ip], *qo = c->q[c->iq];
  size_t off = 0;
  for (int k = 0; k < nf; ++k) {
    if (!f[k].nplanes) continue;
    QgSampleParams S;
    memset(&S, 0, sizeof(S));
    S.nsko = nsko;
    S.ni = qd_count(f[k].tgrid ? g.nxt : g.nx, nsko);
    S.nj = f[k].tgrid ? t1 - t0 : p1 - p0;
    S.ld = f[k].tgrid ? F.ldt : g.ldx;
    S.lj0 = 1 + (f[k].tgrid ? t0 : p0) * nsko - g.joff; // T row j lives in local row j of its array
    S.out = c->qd.buf + off;
    for (int z = 0; z < f[k].nplanes; ++z) {
      switch (k) {
        case 0: S.src[z] = F.sst; break;
        case 1: S.src[z] = po + z * g.fstride; break;
        case 2: S.src[z] = qo + z * g.fstride; break;
        case 3: S.src[z] = F.wekto; break;
        case 4: // h = rgpoc*(po(k+1) - po(k)), rgpoc = 1/gpoc(k) (src/nc_subs.F:1014-1023)
          S.src[z] = po + z * g.fstride; S.src2[z] = po + (z + 1) * g.fstride; S.rg[z] = 1.0 / pr.gpoc[z];
          break;
        case 5: S.src[z] = F.taux; break;
        default: S.src[z] = F.tauy; break;
      }
    }
    if (S.nj > 0) {
      hipLaunchKernelGGL(k_ocnc_sample, dim3((S.ni + 255) / 256, S.nj, f[k].nplanes), dim3(256), 0, c->stream, S);
      HIPCHECK(hipGetLastError());
    }
    off += (size_t)f[k].nplanes * S.ni * S.nj;
  }
  HIPCHECK(hipMemcpyAsync(out, c->qd.buf, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// time averages and periodic dump of the atmosphere (k_atm_tavg.h): tavatm, tavout's atmosphere half and
// atnc_out on a whole-domain atmosphere handle.  The fields xforc / aml leave on the host come from
// qgcm_hip_set_atm_monitor_fields, hmat from qgcm_hip_set_atm_mon_params, fnetat from qgcm_hip_set_atm_tav_fields.
// ---------------------------------------------------------------------------
static const char kOcnTavCalls[] = "qgcm_hip_tavocn / qgcm_hip_ocnc_sample"; // what serves an ocean handle instead

extern "C" int qgcm_hip_set_atm_tav_fields(qgcm_hip_handle c, const double *fnetat) {
  if (atm_only(c, "qgcm_hip_set_atm_tav_fields", kOcnTavCalls)) return 1;
  auto &m = c->atmon;
  if (!m.ldt) m.ldt = round_up(c->g.nxt, 16); // (the pitch of the other T-grid fields, qgcm_hip_set_atm_monitor_fields)
  return tav_set_fnet(c, fnetat, m.ldt);
}

// the parameters of one contribution; fails, naming it, when an input was never given.  Allocates the sums.
static int atav_params(qgcm_hip_ctx *c, QgTavParams &P, const char *who) {
  if (atm_only(c, who, kOcnTavCalls)) return 1;
  const auto &m = c->atmon;
  if (!m.prm_set) QG_FAIL("%s: hmat is missing (qgcm_hip_set_atm_mon_params has not been called)", who);
  if (!(m.prm.hmat > 0.0)) QG_FAIL("%s: hmat = %g (need > 0, qgcm_hip_set_atm_mon_params)", who, m.prm.hmat);
  const char *miss = !m.tauxa ? "tauxa" : !m.tauya ? "tauya" : !m.wekta ? "wekta" : !m.ast ? "ast" : nullptr;
  if (miss) QG_FAIL("%s: %s was never given (qgcm_hip_set_atm_monitor_fields)", who, miss);
  if (!c->tav.fnet) QG_FAIL("%s: fnetat was never given (qgcm_hip_set_atm_tav_fields)", who);
  const qgcm_hip_params &pr = c->prm;
  memset(&P, 0, sizeof(P));
  P.g = c->g;
  P.taux = m.tauxa; P.tauy = m.tauya; P.wekto = m.wekta; P.sst = m.ast; P.fnet = c->tav.fnet; P.ldt = m.ldt;
  P.uvgfac = 1.0 / (pr.dxo * pr.fnot);           // rdxaf0 of MODULE atconst (src/q-gcm.F:392-441)
  P.rhf0hm = 0.5 / (pr.fnot * m.prm.hmat);       // src/timavge.F:301
  return tav_accum_params(c, P);
}

// every input of a scheduled contribution is there (checked before a window launches anything)
static int tavatm_inputs(qgcm_hip_ctx *c, const char *who) {
  QgTavParams P;
  return atav_params(c, P, who);
}

// one contribution from the state on the device (asynchronous); counts it
static int launch_tavatm(qgcm_hip_ctx *c, const char *who) {
  QgTavParams P;
  if (atav_params(c, P, who)) return 1;
  const QgGeom &g = c->g;
  const dim3 grid((g.nx + TAV_NT - 1) / TAV_NT, g.ny);
  KTimer t(c, KN_TAVAT);
#define QG_ATAV(NLV) hipLaunchKernelGGL((k_tavat_accum<NLV>), grid, dim3(TAV_NT), 0, c->stream, P)
  QG_SWITCH_NL(g.nl, QG_ATAV, "k_tavat_accum");
#undef QG_ATAV
  HIPCHECK(hipGetLastError());
  c->tav.n++; // nsumat = nsumat + 1
  return 0;
}

extern "C" int qgcm_hip_tavatm(qgcm_hip_handle c) { return launch_tavatm(c, "qgcm_hip_tavatm"); }

extern "C" int qgcm_hip_atm_tav_reset(qgcm_hip_handle c) {
  return atm_only(c, "qgcm_hip_atm_tav_reset", kOcnTavCalls) || tav_reset(c);
}

extern "C" int qgcm_hip_atm_tav_out(qgcm_hip_handle c, double *const *fields, int *nsumat) {
  return atm_only(c, "qgcm_hip_atm_tav_out", kOcnTavCalls) || tav_out(c, fields, nsumat);
}

extern "C" int qgcm_hip_tavatm_schedule(qgcm_hip_handle c, int every, int phase) {
  if (atm_only(c, "qgcm_hip_tavatm_schedule", kOcnTavCalls)) return 1;
  return sched_set(c->sched[SCH_TAVATM], every, phase, "qgcm_hip_tavatm_schedule");
}

extern "C" long qgcm_hip_atnc_sample_len(qgcm_hip_handle c, int nska, const int *outflat) {
  if (atm_only(c, "qgcm_hip_atnc_sample_len", kOcnTavCalls)) return -1;
  if (!outflat) { snprintf(g_err, sizeof(g_err), "qgcm_hip_atnc_sample_len: null argument"); return -1; }
  if (nska < 1) { snprintf(g_err, sizeof(g_err), "qgcm_hip_atnc_sample_len: nska = %d (need >= 1)", nska); return -1; }
  return (long)dump_len(c, nska, outflat);
}

extern "C" int qgcm_hip_atnc_sample(qgcm_hip_handle c, int nska, const int *outflat, double *out) {
  if (atm_only(c, "qgcm_hip_atnc_sample", kOcnTavCalls)) return 1;
  if (!outflat || !out) QG_FAIL("qgcm_hip_atnc_sample: null argument");
  if (nska < 1) QG_FAIL("qgcm_hip_atnc_sample: nska = %d (need >= 1)", nska);
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  const auto &m = c->atmon;
  QdField f[DUMP_MAXF];
  const int nf = dump_fields(c, outflat, f);
  const double *fld[DUMP_MAXF] = {m.ast, nullptr, nullptr, m.wekta, nullptr, m.tauxa, m.tauya, m.hmixa};
  static const char *names[DUMP_MAXF] = {"ast", "pa", "qa", "wekta", "ha", "tauxa", "tauya", "hmixa"};
  for (int k = 0; k < nf; ++k)
    if (f[k].nplanes && k != 1 && k != 2 && k != 4 && !fld[k])
      QG_FAIL("qgcm_hip_atnc_sample: %s was never given (qgcm_hip_set_atm_monitor_fields)", names[k]);
  const size_t n = dump_len(c, nska, outflat);
  if (n == 0) return 0;
  if (qd_grow(c, n)) return 1;
  QgAtncParams S;
  memset(&S, 0, sizeof(S));
  S.nska = nska;
  S.out = c->qd.buf;
  const double *pa = c->p[c->ip], *qa = c->q[c->iq];
  const int ip = qd_count(g.nx, nska), jp = qd_count(g.ny, nska), it = qd_count(g.nxt, nska), jt = qd_count(g.ny - 1, nska);
  int z = 0;
  long off = 0;
  for (int k = 0; k < nf; ++k)
    for (int p = 0; p < f[k].nplanes; ++p, ++z) {
      if (z >= ATNC_MAXP) QG_FAIL("qgcm_hip_atnc_sample: internal: more than %d planes", ATNC_MAXP);
      const bool t = f[k].tgrid;
      S.ni[z] = t ? it : ip;
      S.nj[z] = t ? jt : jp;
      S.ld[z] = t ? m.ldt : g.ldx;
      S.off[z] = off;
      switch (k) {
        case 1: S.src[z] = pa + p * g.fstride; break;
        case 2: S.src[z] = qa + p * g.fstride; break;
        case 4: S.src[z] = pa + p * g.fstride; S.src2[z] = pa + (p + 1) * g.fstride; S.gp[z] = pr.gpoc[p]; break;
        default: S.src[z] = fld[k]; break;
      }
      off += (long)S.ni[z] * S.nj[z];
    }
  hipLaunchKernelGGL(k_atnc_sample, dim3((ip + 255) / 256, jp, z), dim3(256), 0, c->stream, S);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(out, c->qd.buf, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// covariance matrices (k_cov.h): covini / covocn / covatm of src/covaria_diag.F for the handle's fluid
// (an ocean handle: po and sst, covocn; an atmosphere handle: pa and ast, covatm).  The matrices are split across
// y-slab ranks by whole matrix rows; a whole-domain handle holds them all.
// ---------------------------------------------------------------------------
// the covariances off: the state back to its defaults (which gives the memory back)
static void cov_off(qgcm_hip_ctx *c) {
  c->cov = {};
  c->sched[SCH_COV] = {}; // (the schedule goes with the matrices)
}

static int cov_ready(qgcm_hip_ctx *c, const char *who) {
  if (check_ready(c, who)) return 1;
  if (c->cov.nsi == 0) QG_FAIL("%s: the covariances are off (qgcm_hip_cov_init)", who);
  return 0;
}

// the first packed row of rank r's share: the smallest i with i(i+1)/2 >= r*nmat/nranks (whole rows, balanced by
// element count; rank 0 starts at 0, rank nranks ends at nvar)
static long cov_row_split(long nvar, int r, int nranks) {
  const long nmat = nvar * (nvar + 1) / 2;
  const long t = (long)((__int128)nmat * r / nranks);
  long i = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i > 0 && (i - 1) * i / 2 >= t) --i;
  while (i * (i + 1) / 2 < t) ++i;
  return i;
}

extern "C" int qgcm_hip_cov_init(qgcm_hip_handle c, int nsi, int rank, int nranks) {
  if (check_ready(c, "qgcm_hip_cov_init")) return 1;
  const QgGeom &g = c->g;
  if (nsi == 0) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    cov_off(c);
    return 0;
  }
  const int nyt = g.nyg - 1;
  if (nsi < 2 || g.nxt % nsi != 0 || nyt % nsi != 0)
    QG_FAIL("qgcm_hip_cov_init: nsi = %d must be >= 2 and divide %s = %d and %s = %d (src/parameters_data.F:126-127)",
            nsi, g.atm ? "nxta" : "nxto", g.nxt, g.atm ? "nyta" : "nyto", nyt);
  if (nsi > COV_MAXNSI) QG_FAIL("qgcm_hip_cov_init: nsi = %d exceeds the row-sum kernel's %d", nsi, COV_MAXNSI);
  if (nranks < 1 || rank < 0 || rank >= nranks) QG_FAIL("qgcm_hip_cov_init: rank %d of %d", rank, nranks);
  if (c->whole && nranks != 1)
    QG_FAIL("qgcm_hip_cov_init: a whole-domain handle holds the whole matrices (rank 0 of 1, not %d of %d)", rank, nranks);
  HIPCHECK(hipStreamSynchronize(c->stream));
  cov_off(c);
  auto &v = c->cov;
  v.nbx = g.nxt / nsi;
  v.nby = nyt / nsi;
  v.nvar = v.nbx * v.nby;
  v.nmat = (long)v.nvar * (v.nvar + 1) / 2;
  const long i0 = cov_row_split(v.nvar, rank, nranks), i1 = cov_row_split(v.nvar, rank + 1, nranks);
  v.k0 = i0 * (i0 + 1) / 2;
  v.k1 = i1 * (i1 + 1) / 2;
  v.part_len = COV_HDR + (long)(g.nyg + nyt) * v.nbx; // the whole domain's rows: any slab's fit
  const size_t nm = (size_t)((v.k1 - v.k0 + 1) & ~1L); // even: k_cov_rank1 moves pairs
  // non-temporal loads / stores when the two matrices cannot stay in the 256 MiB Infinity Cache between contributions
  // (measured faster at SOcn 5 km and 385 x 97, slower at NAtl 5 km); QGCM_HIP_COV_NT=0 / 1 forces
  const char *env = getenv("QGCM_HIP_COV_NT");
  v.nt = (env && (env[0] == '0' || env[0] == '1')) ? env[0] == '1' : 2.0 * 8.0 * (double)(v.k1 - v.k0) > 256.0 * (1 << 20);
  int rc = 0;
  for (int w = 0; w < 2 && !rc; ++w)
    rc = (nm && v.mat[w].alloc(nm, w ? "the T covariance matrix" : "the p covariance matrix")) ||
         v.mean[w].alloc(v.nvar, "a covariance mean") || v.dev[w].alloc(v.nvar, "a covariance deviation vector");
  if (!rc) rc = v.part.alloc(v.part_len, "the covariances' row sums") || v.status.alloc(1, "the covariances' status word");
  if (rc) { // (nothing of a multi-gigabyte attempt stays behind; the message is alloc's)
    cov_off(c);
    return 1;
  }
  v.nsi = nsi;
  return 0;
}

extern "C" int qgcm_hip_cov_size(qgcm_hip_handle c, long *nvar, long *nmat, long *k0, long *k1) {
  if (cov_ready(c, "qgcm_hip_cov_size")) return 1;
  const auto &v = c->cov;
  if (nvar) *nvar = v.nvar;
  if (nmat) *nmat = v.nmat;
  if (k0) *k0 = v.k0;
  if (k1) *k1 = v.k1;
  return 0;
}

extern "C" int qgcm_hip_cov_reset(qgcm_hip_handle c) {
  if (cov_ready(c, "qgcm_hip_cov_reset")) return 1;
  auto &v = c->cov;
  const size_t nm = (size_t)((v.k1 - v.k0 + 1) & ~1L);
  for (int w = 0; w < 2; ++w) {
    if (nm) HIPCHECK(hipMemsetAsync(v.mat[w], 0, nm * sizeof(double), c->stream));
    HIPCHECK(hipMemsetAsync(v.mean[w], 0, (size_t)v.nvar * sizeof(double), c->stream));
    v.nu[w] = 0;
    v.swt[w] = 0.0;
  }
  return 0;
}

// the T field a contribution reads (nullptr: missing, named in g_err)
static const double *cov_tfield(qgcm_hip_ctx *c, int *ldt, const char *who) {
  if (c->g.atm) {
    if (!c->atmon.ast) { snprintf(g_err, sizeof(g_err), "%s: ast was never given (qgcm_hip_set_atm_monitor_fields)", who); return nullptr; }
    *ldt = c->atmon.ldt;
    return c->atmon.ast;
  }
  QgSurf S;
  static const int need[] = {SF_SST, SF_END};
  if (surf_fields(c, need, S, who)) return nullptr;
  *ldt = S.ldt;
  return S.sst;
}

// everything a scheduled contribution needs is there (checked before a window launches anything)
static int cov_inputs(qgcm_hip_ctx *c, const char *who) {
  if (cov_ready(c, who)) return 1;
  int ldt = 0;
  return cov_tfield(c, &ldt, who) ? 0 : 1;
}

// this handle's row sums into out (part_len doubles, device); fails, naming it, when the T field is missing
static int launch_cov_rowsums(qgcm_hip_ctx *c, double *out, const char *who) {
  if (cov_ready(c, who)) return 1;
  const QgGeom &g = c->g;
  QgCovRowParams R;
  memset(&R, 0, sizeof(R));
  if (!(R.t = cov_tfield(c, &R.ldt, who))) return 1;
  R.p = c->p[c->ip]; // layer 1 at the time level qgcm_hip_get_state hands out
  R.ldx = g.ldx;
  R.nsi = c->cov.nsi;
  R.nbx = c->cov.nbx;
  R.jp0 = g.jlo;
  R.nrp = g.jhi - g.jlo + 1;
  R.jt0 = g.jlo;
  R.nrt = owned_t1(g) - g.jlo + 1;
  R.joff = g.joff;
  R.out = out;
  hipLaunchKernelGGL(k_cov_rowsums, dim3((R.nbx + COV_RNT - 1) / COV_RNT, R.nrp + R.nrt), dim3(COV_RNT), 0, c->stream, R);
  HIPCHECK(hipGetLastError());
  return 0;
}

// dssp on both vectors from the gathered parts: the combine (mean update, deviations), then the rank-1 update of the
// rows this handle holds.  check: wait for the combine and fail when the parts do not tile the rows.
static int cov_update(qgcm_hip_ctx *c, const double *gath, int nranks, bool check, const char *who) {
  auto &v = c->cov;
  const QgGeom &g = c->g;
  QgCovCombParams Q;
  memset(&Q, 0, sizeof(Q));
  Q.gath = gath;
  Q.part_len = v.part_len;
  Q.nranks = nranks;
  Q.nsi = v.nsi;
  Q.nbx = v.nbx;
  Q.nby = v.nby;
  Q.nyp = g.nyg;
  Q.nyt = g.nyg - 1;
  Q.status = v.status;
  const double wt = 1.0; // covocn / covatm call dssp with wt = 1.0d0
  long nu[2];
  double swt[2];
  QgCovR1Params R;
  memset(&R, 0, sizeof(R));
  for (int w = 0; w < 2; ++w) {
    nu[w] = v.nu[w] + 1;    // nunit = nunit+1
    swt[w] = v.swt[w] + wt; // sumwt = sumwt+wt
    Q.b[w] = wt / swt[w];   // b = wt/sumwt
    Q.first[w] = nu[w] == 1;
    Q.mean[w] = v.mean[w];
    Q.dev[w] = v.dev[w];
    R.m[w] = v.mat[w];
    R.d[w] = v.dev[w];
    R.c[w] = wt - Q.b[w] * wt; // c = wt - b*wt
  }
  KTimer t(c, KN_COV);
  hipLaunchKernelGGL(k_cov_combine, dim3((2 * v.nvar + COV_NT - 1) / COV_NT), dim3(COV_NT), 0, c->stream, Q);
  HIPCHECK(hipGetLastError());
  if (check) {
    int st = 0;
    HIPCHECK(hipMemcpyAsync(&st, v.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    if (st)
      QG_FAIL("%s: the gathered row sums do not tile p rows 1..%d and T rows 1..%d (rank %d of %d does not continue them)",
              who, g.nyg, g.nyg - 1, st - 1, nranks);
  }
  // nunit == 1: the matrix is zero (covini / reset) and stays so; later samples update the rows held here
  R.k0 = v.k0;
  R.n = v.k1 - v.k0;
  if (nu[0] > 1 && R.n > 0) {
    const dim3 grid((unsigned)((R.n + COV_TILE - 1) / COV_TILE));
    if (v.nt) hipLaunchKernelGGL((k_cov_rank1<true>), grid, dim3(COV_NT), 0, c->stream, R);
    else hipLaunchKernelGGL((k_cov_rank1<false>), grid, dim3(COV_NT), 0, c->stream, R);
    HIPCHECK(hipGetLastError());
  }
  for (int w = 0; w < 2; ++w) {
    v.nu[w] = nu[w];
    v.swt[w] = swt[w];
  }
  return 0;
}

// one covocn / covatm from the device state (whole-domain handle; asynchronous)
static int launch_cov(qgcm_hip_ctx *c, const char *who) {
  if (cov_ready(c, who)) return 1;
  if (!c->whole) QG_FAIL("%s: the handle is a y-slab (qgcm_hip_cov_part / _combine serve it)", who);
  if (launch_cov_rowsums(c, c->cov.part, who)) return 1;
  return cov_update(c, c->cov.part, 1, false, who);
}

extern "C" int qgcm_hip_cov_add(qgcm_hip_handle c) { return launch_cov(c, "qgcm_hip_cov_add"); }

extern "C" long qgcm_hip_cov_part_len(qgcm_hip_handle c) {
  if (cov_ready(c, "qgcm_hip_cov_part_len")) return -1;
  return c->cov.part_len;
}

extern "C" int qgcm_hip_cov_part(qgcm_hip_handle c, double *send_dev) {
  if (cov_ready(c, "qgcm_hip_cov_part")) return 1;
  if (!send_dev) QG_FAIL("qgcm_hip_cov_part: null argument");
  return launch_cov_rowsums(c, send_dev, "qgcm_hip_cov_part");
}

extern "C" int qgcm_hip_cov_combine(qgcm_hip_handle c, const double *gath_dev, int nranks) {
  if (cov_ready(c, "qgcm_hip_cov_combine")) return 1;
  if (!gath_dev || nranks < 1 || nranks > COV_MAXR)
    QG_FAIL("qgcm_hip_cov_combine: need the gathered row sums and 1 <= nranks <= %d (not %d)", COV_MAXR, nranks);
  return cov_update(c, gath_dev, nranks, true, "qgcm_hip_cov_combine");
}

extern "C" int qgcm_hip_cov_out(qgcm_hip_handle c, int which, double *avg, double *swt, long *nunit, long k0, long count,
                                double *cov) {
  if (cov_ready(c, "qgcm_hip_cov_out")) return 1;
  const auto &v = c->cov;
  if (which != 0 && which != 1) QG_FAIL("qgcm_hip_cov_out: which = %d (0 = p, 1 = T)", which);
  if (cov && (count < 0 || k0 < v.k0 || k0 + count > v.k1))
    QG_FAIL("qgcm_hip_cov_out: entries %ld..%ld outside the range %ld..%ld this handle holds", k0, k0 + count - 1, v.k0,
            v.k1 - 1);
  if (swt) *swt = v.swt[which];
  if (nunit) *nunit = v.nu[which];
  if (avg) HIPCHECK(hipMemcpyAsync(avg, v.mean[which], (size_t)v.nvar * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cov && count > 0)
    HIPCHECK(hipMemcpyAsync(cov, v.mat[which] + (k0 - v.k0), (size_t)count * sizeof(double), hipMemcpyDeviceToHost,
                            c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int qgcm_hip_cov_schedule(qgcm_hip_handle c, int every, int phase) {
  if (check_ready(c, "qgcm_hip_cov_schedule")) return 1;
  if (!c->whole)
    QG_FAIL("qgcm_hip_cov_schedule: the handle is a y-slab; the scheduled contribution is whole-domain only (call "
            "qgcm_hip_cov_part / _combine between slab steps)");
  if (cov_ready(c, "qgcm_hip_cov_schedule")) return 1;
  return sched_set(c->sched[SCH_COV], every, phase, "qgcm_hip_cov_schedule");
}

// ---------------------------------------------------------------------------
// area averages and the CFL check: areavg and cfltry
// ---------------------------------------------------------------------------
// The handles these entry points serve.  part: the y-slab triple (_part / _combine), which an atmosphere does not
// have; else the whole-domain call, which a y-slab cannot answer.  `other`: the calls that serve the refused handle.
static int ac_handle(qgcm_hip_ctx *c, bool part, const char *who, const char *other) {
  if (!c) QG_FAIL("%s: null handle", who);
  if (part && c->g.atm) QG_FAIL("%s: the handle is an atmosphere, which has no y-slabs (%s serves it)", who, other);
  if (!part && !c->whole) QG_FAIL("%s: the handle is a y-slab (%s serve it)", who, other);
  return check_ready(c, who);
}

extern "C" int qgcm_hip_areavg_init(qgcm_hip_handle c, int n, const int *i1, const int *i2, const int *j1, const int *j2,
                                    const double *facw, const double *face, const double *facs, const double *facn) {
  const char *who = "qgcm_hip_areavg_init";
  if (check_ready(c, who)) return 1;
  if (c->g.atm && !c->whole) QG_FAIL("%s: the handle is an atmosphere's y-slab (the atmosphere's diagnostics need the whole domain)", who);
  if (n < 1 || n > ARAV_MAXN)
    QG_FAIL("%s: %d areas (need 1 .. %d = namxoc, namxat of src/areasubs_diag.F)", who, n, ARAV_MAXN);
  if (!i1 || !i2 || !j1 || !j2 || !facw || !face || !facs || !facn) QG_FAIL("%s: null argument", who);
  const QgGeom &g = c->g;
  const int nxt = g.nx - 1, nyt = g.nyg - 1;
  const char *fluid = g.atm ? "atmos." : "ocean";
  QgAravParams T = {};
  T.n = n;
  for (int a = 0; a < n; ++a) {
    // the reference's subscript checks (src/areasubs_diag.F:312-325), then what areint's loops assume
    if (i1[a] < 1 || i1[a] > nxt || i2[a] < 1 || i2[a] > nxt)
      QG_FAIL("%s: invalid subscript for %s area m = %d: i1t, i2t = %d, %d outside 1..%d", who, fluid, a + 1, i1[a], i2[a], nxt);
    if (j1[a] < 1 || j1[a] > nyt || j2[a] < 1 || j2[a] > nyt)
      QG_FAIL("%s: invalid subscript for %s area m = %d: j1t, j2t = %d, %d outside 1..%d", who, fluid, a + 1, j1[a], j2[a], nyt);
    if (i1[a] > i2[a]) QG_FAIL("%s: %s area m = %d has i1t = %d > i2t = %d", who, fluid, a + 1, i1[a], i2[a]);
    if (j1[a] > j2[a]) QG_FAIL("%s: %s area m = %d has j1t = %d > j2t = %d", who, fluid, a + 1, j1[a], j2[a]);
    T.i1[a] = i1[a]; T.i2[a] = i2[a]; T.j1[a] = j1[a]; T.j2[a] = j2[a];
    T.facw[a] = facw[a]; T.face[a] = face[a]; T.facs[a] = facs[a]; T.facn[a] = facn[a];
    // areint's weight sums in its serial order (:621-675): the same wsumi for every row
    double wsumi = facw[a];
    for (int i = i1[a] + 1; i <= i2[a] - 1; ++i) wsumi = wsumi + 1.0;
    wsumi = wsumi + face[a];
    double wtsum = 0.0;
    for (int j = j1[a] + 1; j <= j2[a] - 1; ++j) wtsum = wtsum + wsumi;
    T.den[a] = facs[a] * wsumi + facn[a] * wsumi + wtsum;
  }
  auto &m = c->ac;
  const int rowcap = owned_t1(g) - g.jlo + 1;
  if (m.rows.ensure((size_t)ARAV_MAXN * rowcap, "the area averages' row sums") || m.out.ensure(ARAV_PART_LEN, "the area averages"))
    return 1;
  HIPCHECK(hipStreamSynchronize(c->stream)); // (no call that reads the old tables is still in flight)
  m.tab = T;
  return 0;
}

// the kernel parameters: the tables, the field at its current level, the owned T rows
static int arav_params(qgcm_hip_ctx *c, QgAravParams &P, const char *who) {
  auto &m = c->ac;
  if (m.tab.n == 0) QG_FAIL("%s: qgcm_hip_areavg_init has not been called", who);
  const QgGeom &g = c->g;
  P = m.tab;
  if (g.atm) {
    if (!c->atmon.ast)
      QG_FAIL("%s: ast was never given (qgcm_hip_set_atm_monitor_fields) and the mixed layer is off", who);
    P.f = c->atmon.ast;
    P.ld = c->atmon.ldt;
  } else {
    static const int need[] = {SF_SST, SF_END};
    QgSurf S;
    if (surf_fields(c, need, S, who)) return 1;
    P.f = S.sst;
    P.ld = S.ldt;
  }
  P.t0 = g.jlo + g.joff;
  P.t1 = owned_t1(g) + g.joff;
  P.joff = g.joff;
  P.nyt = g.nyg - 1;
  P.rowcap = P.t1 - P.t0 + 1;
  P.rows = m.rows;
  P.out = m.out;
  return 0;
}

// the row sums of every area over the owned rows, then the handle's part of the sums (FINAL: the averages)
static int launch_arav(qgcm_hip_ctx *c, const QgAravParams &P, bool final) {
  int maxrows = 0;
  for (int a = 0; a < P.n; ++a)
    maxrows = std::max(maxrows, std::min(P.j2[a], P.t1) - std::max(P.j1[a], P.t0) + 1);
  if (maxrows > 0) hipLaunchKernelGGL(k_arav_rows, dim3(maxrows, P.n), dim3(64), 0, c->stream, P);
  if (final) hipLaunchKernelGGL(k_arav_part<true>, dim3(1), dim3(64 * ARAV_MAXN), 0, c->stream, P);
  else hipLaunchKernelGGL(k_arav_part<false>, dim3(1), dim3(64 * ARAV_MAXN), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

// avg, num, den (each may be null) from the device vector at c->ac.out; *status = the combine's
static int arav_fetch(qgcm_hip_ctx *c, int n, double *avg, double *num, double *den, double *status) {
  double h[ARAV_OUT_LEN];
  HIPCHECK(hipMemcpyAsync(h, c->ac.out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (status) {
    *status = h[3 * ARAV_MAXN];
    if (*status != 0.0) return 0;
  }
  for (int a = 0; a < n; ++a) {
    if (avg) avg[a] = h[a];
    if (num) num[a] = h[ARAV_MAXN + a];
    if (den) den[a] = h[2 * ARAV_MAXN + a];
  }
  return 0;
}

extern "C" int qgcm_hip_areavg_count(qgcm_hip_handle c) { return c ? c->ac.tab.n : -1; }

extern "C" int qgcm_hip_areavg(qgcm_hip_handle c, double *avg, double *num, double *den) {
  const char *who = "qgcm_hip_areavg";
  if (ac_handle(c, false, who, "qgcm_hip_areavg_part / _combine")) return 1;
  if (!avg) QG_FAIL("%s: null argument", who);
  QgAravParams P;
  if (arav_params(c, P, who) || launch_arav(c, P, true)) return 1;
  return arav_fetch(c, P.n, avg, num, den, nullptr);
}

extern "C" int qgcm_hip_areavg_part_len(qgcm_hip_handle c) { return c ? ARAV_PART_LEN : -1; }

extern "C" int qgcm_hip_areavg_part(qgcm_hip_handle c, double *send_dev) {
  const char *who = "qgcm_hip_areavg_part";
  if (ac_handle(c, true, who, "qgcm_hip_areavg")) return 1;
  if (!send_dev) QG_FAIL("%s: null argument", who);
  QgAravParams P;
  if (arav_params(c, P, who)) return 1;
  P.out = send_dev;
  return launch_arav(c, P, false);
}

extern "C" int qgcm_hip_areavg_combine(qgcm_hip_handle c, const double *gath_dev, int nranks, double *avg, double *num,
                                       double *den) {
  const char *who = "qgcm_hip_areavg_combine";
  if (ac_handle(c, true, who, "qgcm_hip_areavg")) return 1;
  if (!gath_dev || !avg || nranks < 1) QG_FAIL("%s: need the gathered summaries, avg and nranks >= 1", who);
  auto &m = c->ac;
  if (m.tab.n == 0) QG_FAIL("%s: qgcm_hip_areavg_init has not been called", who);
  QgAravParams P = m.tab;
  P.nyt = c->g.nyg - 1;
  P.out = m.out;
  P.gath = gath_dev;
  P.nranks = nranks;
  hipLaunchKernelGGL(k_arav_combine, dim3(1), dim3(64), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  double st = 0.0;
  if (arav_fetch(c, P.n, avg, num, den, &st)) return 1;
  if (st != 0.0)
    QG_FAIL("%s: the gathered summaries do not tile T rows 1..%d (rank %d of %d does not continue them)", who, P.nyt,
            (int)st - 1, nranks);
  return 0;
}

// the parameters of the CFL kernels (partials over this handle's owned rows); allocates on first use
static int cfl_params(qgcm_hip_ctx *c, QgCflParams &P, double cflcrit, const char *who) {
  const QgGeom &g = c->g;
  const qgcm_hip_params &pr = c->prm;
  if (g.nl < 2 || g.nl > QG_MAXL) QG_FAIL("%s: unsupported number of layers", who);
  if (!(cflcrit == cflcrit)) QG_FAIL("%s: cflcrit is not a number", who);
  memset(&P, 0, sizeof(P));
  P.g = g;
  P.p = c->p[c->ip]; // the level qgcm_hip_get_state hands out as po / pa
  if (g.atm) {
    const auto &m = c->atmon;
    const char *miss = !m.uekat ? "uekat" : !m.vekat ? "vekat" : nullptr;
    if (miss) QG_FAIL("%s: %s was never given (qgcm_hip_set_atm_monitor_fields, qgcm_hip_xforc)", who, miss);
    P.sx = m.uekat; P.sy = m.vekat; P.ldt = m.ldt;
  } else {
    static const int need[] = {SF_TAUX, SF_TAUY, SF_END};
    QgSurf S;
    if (surf_fields(c, need, S, who)) return 1;
    P.sx = S.taux; P.sy = S.tauy; P.ldt = S.ldt;
    // hmoc where the monitors take it (qgcm_hip_set_mon_params), else the mixed layer's own
    if (!c->mon.prm_set && !c->oml.on)
      QG_FAIL("%s: hmoc was never given (qgcm_hip_set_mon_params or qgcm_hip_oml_init)", who);
    const double hmoc = c->mon.prm_set ? c->mon.prm.hmoc : c->oml.prm.hmoc;
    P.rhf0hm = 0.5 / (pr.fnot * hmoc); // src/q-gcm.F:2174
  }
  P.jlo = g.jlo; P.jhi = g.jhi;
  P.ntx = (g.nx + CFL_TX - 1) / CFL_TX;
  P.nblk = P.ntx * ((g.jhi - g.jlo + 1 + CFL_TY - 1) / CFL_TY);
  auto &m = c->ac;
  if (m.cfl_part.ensure((size_t)CFL_LEN(QG_MAXL) * P.nblk, "the CFL check's partials") ||
      m.cfl_out.ensure(CFL_PART_LEN(QG_MAXL), "the CFL check's result"))
    return 1;
  P.part = m.cfl_part;
  P.out = m.cfl_out;
  // MODULE occonst / atconst as src/q-gcm.F derives them; dto = tdto/2 exactly
  P.rdxf0 = 1.0 / (pr.dxo * pr.fnot);
  P.dtdx = (0.5 * pr.tdto) / pr.dxo;
  P.cflcrit = cflcrit;
  return 0;
}

static int launch_cfl(qgcm_hip_ctx *c, const QgCflParams &P, bool part) {
#define QG_CFL(NLV)                                                                                      \
  if (c->g.atm) hipLaunchKernelGGL((k_cfl_scan<NLV, true>), dim3(P.nblk), dim3(CFL_NT), 0, c->stream, P); \
  else hipLaunchKernelGGL((k_cfl_scan<NLV, false>), dim3(P.nblk), dim3(CFL_NT), 0, c->stream, P)
  QG_SWITCH_NL(c->g.nl, QG_CFL, "k_cfl");
#undef QG_CFL
  if (part) hipLaunchKernelGGL(k_cfl_final<true>, dim3(1), dim3(CFL_FT), 0, c->stream, P);
  else hipLaunchKernelGGL(k_cfl_final<false>, dim3(1), dim3(CFL_FT), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  return 0;
}

// maxima, nbad (nq each) and loc (i, j per quantity) from the device vector at c->ac.cfl_out.  The count is the
// reference's: its second scan runs only where the printed Courant number max*dt/dx reaches cflcrit.
static int cfl_fetch(qgcm_hip_ctx *c, const QgCflParams &P, double *maxima, int *nbad, int *loc, double *status) {
  const int nq = CFL_NQ(c->g.nl);
  double h[CFL_PART_LEN(QG_MAXL)];
  HIPCHECK(hipMemcpyAsync(h, c->ac.cfl_out, sizeof(double) * (3 * nq + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (status) {
    *status = h[3 * nq];
    if (*status != 0.0) return 0;
  }
  const double dt = 0.5 * c->prm.tdto, dx = c->prm.dxo;
  for (int q = 0; q < nq; ++q) {
    const int key = (int)h[nq + q];
    if (maxima) maxima[q] = h[q];
    if (nbad) nbad[q] = h[q] * dt / dx >= P.cflcrit ? (int)h[2 * nq + q] : 0;
    if (loc) { loc[2 * q] = key % c->g.nx + 1; loc[2 * q + 1] = key / c->g.nx + 1; }
  }
  return 0;
}

extern "C" int qgcm_hip_cfl_len(qgcm_hip_handle c) { return c ? CFL_NQ(c->g.nl) : -1; }

extern "C" int qgcm_hip_cfl(qgcm_hip_handle c, double cflcrit, double *maxima, int *nbad, int *loc) {
  const char *who = "qgcm_hip_cfl";
  if (ac_handle(c, false, who, "qgcm_hip_cfl_part / _combine")) return 1;
  if (!maxima) QG_FAIL("%s: null argument", who);
  QgCflParams P;
  if (cfl_params(c, P, cflcrit, who) || launch_cfl(c, P, false)) return 1;
  return cfl_fetch(c, P, maxima, nbad, loc, nullptr);
}

extern "C" int qgcm_hip_cfl_part_len(qgcm_hip_handle c) { return c ? CFL_PART_LEN(c->g.nl) : -1; }

extern "C" int qgcm_hip_cfl_part(qgcm_hip_handle c, double cflcrit, double *send_dev) {
  const char *who = "qgcm_hip_cfl_part";
  if (ac_handle(c, true, who, "qgcm_hip_cfl")) return 1;
  if (!send_dev) QG_FAIL("%s: null argument", who);
  QgCflParams P;
  if (cfl_params(c, P, cflcrit, who)) return 1;
  P.out = send_dev;
  return launch_cfl(c, P, true);
}

extern "C" int qgcm_hip_cfl_combine(qgcm_hip_handle c, const double *gath_dev, int nranks, double cflcrit, double *maxima,
                                    int *nbad, int *loc) {
  const char *who = "qgcm_hip_cfl_combine";
  if (ac_handle(c, true, who, "qgcm_hip_cfl")) return 1;
  if (!gath_dev || !maxima || nranks < 1) QG_FAIL("%s: need the gathered summaries, maxima and nranks >= 1", who);
  QgCflParams P;
  if (cfl_params(c, P, cflcrit, who)) return 1;
  P.gath = gath_dev;
  P.nranks = nranks;
  hipLaunchKernelGGL(k_cfl_combine, dim3(1), dim3(64), 0, c->stream, P);
  HIPCHECK(hipGetLastError());
  double st = 0.0;
  if (cfl_fetch(c, P, maxima, nbad, loc, &st)) return 1;
  if (st != 0.0)
    QG_FAIL("%s: the gathered summaries do not tile rows 1..%d (rank %d of %d does not continue them)", who, c->g.nyg,
            (int)st - 1, nranks);
  return 0;
}
