"""OceanModel - Python mirror of the reference's operator interface for the ocean
hot path.  The reference exposes three argument-less module procedures acting on
MODULE ocstate / ochomog arrays (src/q-gcm.F:1243-1249):

    call qgostep ; call ocinvq ; call ocqbdy (qo, po)

Here the same three names are methods, the module arrays are device resident,
and ``po / pom / qo / qom`` are fetched on demand (properties).  Everything that
computes goes through the C ABI of include/qgcm_hip.h; nothing here falls back
to numpy for the per-step path.
"""
import ctypes as C

import numpy as np

from . import hostinit
from .handle import (COV_NAMES_ATM, COV_NAMES_OCN, OCNC_FIELDS, QOCDIAG_TERMS, TAV_LAYOUT, Handle, _dp, _f,  # noqa: F401
                     read_dump, read_means, subsample_count, unpack_budget)
from .lib import QgcmHipError, check


# layout of qgcm_hip_monitors (include/qgcm_hip.h): (name, length in units of nlo: 0 = scalar, -1 = nlo-1, 1 = nlo)
MONITOR_LAYOUT = ([(n, 0) for n in ("wetmoc", "watmoc", "wepmoc", "wapmoc", "entmoc", "enamoc")]
                  + [(n, -1) for n in ("etamoc", "et2moc", "ddtpeoc")] + [("pkenoc", 0), ("utauoc", 0)]
                  + [(n, 1) for n in ("pavgoc", "qavgoc", "ah2doc", "ah4doc", "kealoc", "ddtkeoc", "osfmin", "osfmax",
                                      "occirc", "ocjpos", "ocjval")]
                  + [(n, 0) for n in ("btdgoc", "sstmin", "sstmax", "tmlmoc", "hfmloc", "occtot",
                                      "umminoc", "ummaxoc", "vmminoc", "vmmaxoc", "cnmloc")]
                  + [(n, 1) for n in ("ugminoc", "ugmaxoc", "vgminoc", "vgmaxoc", "cnqgoc")])


# layout of qgcm_hip_atm_monitors (include/qgcm_hip.h), as MONITOR_LAYOUT: (name, length in units of nla)
ATM_MONITOR_LAYOUT = ([(n, 0) for n in ("wetmat", "watmat", "wepmat", "wapmat")]
                      + [(n, -1) for n in ("entmat", "enamat", "etamat", "et2mat", "ddtpeat", "pkenat")]
                      + [("utauat", 0)]
                      + [(n, 1) for n in ("pavgat", "qavgat", "ah4dat", "kealat", "ddtkeat", "atstpos", "atstval")]
                      + [(n, 0) for n in ("tmlmat", "hmlmat", "astmin", "astmax", "hcmlat", "tmaooc", "olrtop",
                                          "umminat", "ummaxat", "vmminat", "vmmaxat", "cnmlat")]
                      + [(n, 1) for n in ("ugminat", "ugmaxat", "vgminat", "vgmaxat", "cnqgat")])

# the twelve numbers of qgcm_hip_atm_valids
ATM_VALIDS_NAMES = ("pamin", "pamax", "qamin", "qamax", "astmin", "astmax", "wekmin", "wekmax", "txamin", "txamax",
                    "tyamin", "tyamax")


def unpack_atm_monitors(v, nl):
    """dict name -> float or array from the packed vector of qgcm_hip_atm_monitors; atstpos as int (0: none)."""
    return _unpack(v, nl, ATM_MONITOR_LAYOUT, "atstpos")


def _unpack(v, nl, layout, posname):
    out, i = {}, 0
    for name, kind in layout:
        n = {0: 1, -1: nl - 1, 1: nl}[kind]
        x = np.array(v[i:i + n], dtype=np.float64)
        out[name] = float(x[0]) if kind == 0 else (x.astype(np.int64) if name == posname else x)
        i += n
    if i != len(v):
        raise QgcmHipError("monitor vector has %d entries, the layout %d" % (len(v), i))
    return out


def atm_mon_params(acfg, ocean=None, rhoat=1.0, cpat=1.0e3, hmat=1000.0, davgat=0.0, aup=None, bup=0.0, cup=0.0,
                   dup=0.0, nx1=None, ny1=None, nxaooc=None, nyaooc=None):
    """struct qgcm_hip_atm_mon_params for the atmosphere `acfg` (an AtmosConfig).  rhoat, cpat, hmat default to
    examples/double_gyre_coupled's input.params (1.0 kg m^-3, 1.0e3 J kg^-1 K^-1, 1000 m); davgat = 0 is a flat
    atmosphere.  aup (= Aup(nla, 1..nla-1)), bup, cup, dup (= Bup(nla), Cup(nla), Dup(nla)) are computed by radiate
    at start-up, not read from input.params: they default to 0 (olrtop = 0).  The ocean's cells: nxaooc, nyaooc from
    `ocean` (an OceanConfig) or given; nx1, ny1 default to src/parameters_data.F:86, 1 + (nxta - nxaooc)/2."""
    from .lib import AtmMonParams
    nxa = ocean.nxaooc if nxaooc is None and ocean is not None else nxaooc
    nya = ocean.nyaooc if nyaooc is None and ocean is not None else nyaooc
    if nxa is None or nya is None:
        raise QgcmHipError("atm_mon_params: give the ocean's configuration or nxaooc, nyaooc")
    p = AtmMonParams()
    p.rhoat, p.cpat, p.hmat, p.davgat = float(rhoat), float(cpat), float(hmat), float(davgat)
    a = np.zeros(acfg.nla - 1) if aup is None else np.asarray(aup, dtype=np.float64)
    if len(a) != acfg.nla - 1:
        raise QgcmHipError("aup needs nla-1 = %d values" % (acfg.nla - 1))
    for k, v in enumerate(a):
        p.aup[k] = float(v)
    p.bup, p.cup, p.dup = float(bup), float(cup), float(dup)
    p.nxaooc, p.nyaooc = int(nxa), int(nya)
    p.nx1 = 1 + (acfg.nxta - p.nxaooc) // 2 if nx1 is None else int(nx1)
    p.ny1 = 1 + (acfg.nyta - p.nyaooc) // 2 if ny1 is None else int(ny1)
    return p


def unpack_monitors(v, nl):
    """dict name -> float or array from the packed vector of qgcm_hip_monitors; ocjpos as int (1-based row, 0: none)."""
    return _unpack(v, nl, MONITOR_LAYOUT, "ocjpos")


def prsamp_dict(out, nl):
    """dict of the packed result of qgcm_hip_prsamp (4*nlo + 2 doubles)."""
    return dict(po_centre=out[:nl].copy(), qo_centre=out[nl:2 * nl].copy(), pavgoc=out[2 * nl:3 * nl].copy(),
                qavgoc=out[3 * nl:4 * nl].copy(), sstmin=out[4 * nl], sstmax=out[4 * nl + 1])


# the atmosphere's time averages and dump (qgcm_hip_atm_tav_out / qgcm_hip_atnc_sample): outputs of
# qgcm_hip_atm_tav_out in ABI order (names of MODULE timavge / tavout) and their grids, as TAV_LAYOUT:
# p = (nxpa, nypa), t = (nxta, nyta), p3 = (nxpa, nypa, nla), u = (nxpa, nyta), v = (nxta, nypa)
ATM_TAV_LAYOUT = (("txatav", "p"), ("tyatav", "p"), ("wtatav", "t"), ("fmatav", "t"), ("astav", "t"), ("patav", "p3"),
                  ("qatav", "p3"), ("uufa", "u"), ("tufa", "u"), ("utufa", "u"), ("vvfa", "v"), ("tvfa", "v"),
                  ("vtvfa", "v"), ("uptpat", "u"), ("vptpat", "v"))
# atnc_out's fields in its order: (name, grid, planes in units of nla: 0 = one plane, 1 = nla, -1 = nla-1, flag index)
# (tauxa and tauya share outflat(6))
ATNC_FIELDS = (("ast", "t", 0, 0), ("pa", "p", 1, 1), ("qa", "p", 1, 2), ("wekta", "t", 0, 3), ("ha", "p", -1, 4),
               ("tauxa", "p", 0, 5), ("tauya", "p", 0, 5), ("hmixa", "t", 0, 6))


def cov_row_split(nvar, r, nranks):
    """First packed matrix row of rank r of nranks (qgcm_hip_cov_init): the smallest i with i(i+1)/2 >= r*nmat//nranks."""
    nmat = nvar * (nvar + 1) // 2
    t = nmat * r // nranks
    i = int((np.sqrt(8.0 * t + 1.0) - 1.0) * 0.5)
    while i > 0 and (i - 1) * i // 2 >= t:
        i -= 1
    while i * (i + 1) // 2 < t:
        i += 1
    return i


def cfl_names(nl):
    """The quantities of qgcm_hip_cfl in its order: ml_u, ml_v, u1..u<nl>, v1..v<nl>."""
    return ["ml_u", "ml_v"] + ["u%d" % (k + 1) for k in range(nl)] + ["v%d" % (k + 1) for k in range(nl)]


def cfl_dict(cfg, maxima, nbad, loc):
    """What cfl() returns: maxima, Courant numbers max*dt/dx (formed here, as the reference prints them), the counts
    of points at or above cflcrit and the 1-based (i, j) of every maximum, arrays over cfl_names(nl)."""
    return {"names": cfl_names(len(maxima) // 2 - 1), "maxima": maxima, "courant": maxima * cfg.dto / cfg.dxo,
            "nbad": nbad, "loc": loc.reshape(-1, 2)}


class OceanModel(Handle):
    """One ocean configuration on one MI355X: the handle that owns the whole domain.

    Start-up follows src/q-gcm.F:380-976 for the ocean: grid, eigmod, tridiagonal
    coefficients, homsol (its Helmholtz solves run on the GPU through
    qgcm_hip_helmholtz).  A caller that already has the reference's constants
    (the Fortran host) can pass them in ``consts`` to skip that arithmetic.
    """

    def __init__(self, cfg, ddynoc=None, device=-1, consts=None):
        self.yporel = cfg.yporel()
        self.ddynoc = np.zeros((cfg.nxpo, cfg.nypo), order="F") if ddynoc is None else _f(ddynoc)
        atmos = bool(getattr(cfg, "atmos", False))
        if consts is None:
            A, rdm2, cl2m, cm2l = hostinit.eigmod(cfg.gpoc, cfg.hoc, cfg.fnot, atmos=atmos)
        else:
            A, rdm2, cl2m, cm2l = (consts[k] for k in ("amatoc", "rdm2oc", "ctl2moc", "ctm2loc"))
        self.amatoc, self.rdm2oc, self.ctl2moc, self.ctm2loc = A, rdm2, cl2m, cm2l
        self.aoc, self.bd2oc = hostinit.bd2oc(cfg)
        Handle.__init__(self, cfg, dict(amatoc=A, rdm2oc=rdm2, ctl2moc=cl2m, ctm2loc=cm2l, aoc=self.aoc, bd2oc=self.bd2oc,
                                        yporel=self.yporel, ddynoc=self.ddynoc), device, atmos=atmos)
        # homsol
        if consts is not None and ("ochom" in consts or "pch1oc" in consts):
            self.homog = consts
        elif cfg.cyclic:
            self.homog = hostinit.homsol_cyc(cfg, rdm2, self.bd2oc, self.yporel, self.helmholtz)
        else:
            self.homog = hostinit.homsol_box(cfg, rdm2, cm2l, self.bd2oc, self.helmholtz)
        if cfg.cyclic:
            self.set_homog_cyc(self.homog)
        else:
            self.set_homog_box(self.homog)
        self.step_index = 1  # next 1-based ocean step
        if getattr(cfg, "l_spl", 0.0) > 0.0:  # a -Dsponge_layer_k247 configuration
            self.set_sponge(hostinit.sponge_ramp(cfg), cfg.c1_spl)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ----------------------------------------------------------------
    def set_p(self, po, pom=None):
        """Load pressures and derive q and the constraint scalars as the reference
        does at start-up (src/q-gcm.F:711-731: constr, qcomp, ocqbdy, merqcy)."""
        c = self.cfg
        po = _f(po)
        pom = po.copy(order="F") if pom is None else _f(pom)
        qo = hostinit.q_from_p(c, self.amatoc, self.yporel, self.ddynoc, po)
        qom = hostinit.q_from_p(c, self.amatoc, self.yporel, self.ddynoc, pom)
        self.set_state(po, pom, qo, qom)
        self.set_scalars(hostinit.constr(c, self.amatoc, po, pom))

    def init_from_p(self, po, pom=None):
        """The same start-up sequence ON THE DEVICE (qgcm_hip_init_from_p): only po, pom cross PCIe - the restart
        path of a host that keeps no q (restart dumps carry po, pom only, src/q-gcm.F:3076-3086)."""
        po = _f(po)
        pom = po if pom is None else _f(pom)
        self.set_state(po, pom, None, None)
        check(self.L.qgcm_hip_init_from_p(self.h))

    def wekpo_from_tau(self, tauxo, tauyo):
        """Ocean-only Ekman pumping from the wind stress on the device (src/xfosubs.F:566-645)."""
        check(self.L.qgcm_hip_wekpo_from_tau(self.h, _dp(_f(tauxo)), _dp(_f(tauyo))))

    def prsamp(self):
        """The ocean numbers of the reference's progress print-out (src/q-gcm.F:1933-2066) without pulling the state:
        dict(po_centre, qo_centre, pavgoc, qavgoc: nlo each; sstmin, sstmax)."""
        nl = self.cfg.nlo
        out = np.zeros(4 * nl + 2)
        check(self.L.qgcm_hip_prsamp(self.h, _dp(out)))
        return prsamp_dict(out, nl)

    po = property(lambda self: self.get_state()[0])
    pom = property(lambda self: self.get_state()[1])
    qo = property(lambda self: self.get_state()[2])
    qom = property(lambda self: self.get_state()[3])

    def tend_zero_mask(self):
        """Which of entoc (bit 0) and ddynoc (bit 1) the next tendency launch leaves out because the library knows
        them to be all zero (qgcm_hip_tend_zero_mask); the results do not depend on it."""
        return int(self.L.qgcm_hip_tend_zero_mask(self.h))

    def get_bsums(self):
        """ajisoc, ajinoc, ap5soc, ap5noc (nlo each): the boundary line sums of the last qgostep of a zonally cyclic
        ocean (valid after the following ocinvq).  On an atmosphere: ajisat, ajinat, ap5sat, ap5nat (nla each) of the
        last qgastep (valid after the following atinvq)."""
        b = np.zeros(4 * self.cfg.nlo)
        check(self.L.qgcm_hip_get_bsums(self.h, _dp(b)))
        return b

    def get_inv_diag(self):
        nl = self.cfg.nlo
        x = np.zeros(nl)
        cf = np.zeros(2 * nl + 1)
        check(self.L.qgcm_hip_get_inv_diag(self.h, _dp(x), _dp(cf)))
        n = 2 * (nl - 1) + 1 if self.cfg.cyclic else nl - 1
        return x, cf[:n].copy()

    # -- the path (same names as the reference's module procedures) ------------
    def ocinvq(self):
        check(self.L.qgcm_hip_ocinvq(self.h))

    def ocqbdy(self):
        check(self.L.qgcm_hip_ocqbdy(self.h))

    def ocqbdy_host(self, q, p):
        """`call ocqbdy (q, p)` / `call atqzbd (q, p)` on host arrays (start-up use, src/q-gcm.F:724-725, 743-744):
        returns q with its boundary ring recomputed from p; the device-resident state is not touched."""
        q = np.array(q, dtype=np.float64, order="F", copy=True)
        check(self.L.qgcm_hip_ocqbdy_host(self.h, _dp(q), _dp(_f(p))))
        return q

    def steps(self, n, s0=None):
        """n whole ocean steps (q-gcm.F:1243-1249 + the averaging of :1328)."""
        s0 = self.step_index if s0 is None else int(s0)
        check(self.L.qgcm_hip_steps(self.h, s0, int(n)))
        self.step_index = s0 + int(n)

    # -- validity scan (`call valids (solnok)`, src/q-gcm.F:1278) --
    def valids(self):
        """(solnok, out): out = min/max of po, qo, sst, wekto, layer thickness top/intermediate/bottom,
        then hfbad(1..nlo) in per cent (src/valsubs.F:272-527)."""
        out = np.zeros(14 + self.cfg.nlo)
        ok = C.c_int()
        check(self.L.qgcm_hip_valids(self.h, _dp(out), C.byref(ok)))
        return bool(ok.value), out

    # -- ocean monitors (ocean half of `call monnc_comp` + couroc, src/monitor_diag.F) --
    def monitor_vector(self):
        """The packed result of qgcm_hip_monitors (order: include/qgcm_hip.h)."""
        out = np.zeros(self.L.qgcm_hip_monitor_len(self.h))
        check(self.L.qgcm_hip_monitors(self.h, _dp(out)))
        return out

    def monitors(self):
        """The ocean variables of MODULE monitor that monnc_comp / couroc compute (src/monitor_data.F:50-71), from
        the device state without pulling it: dict of scalars and per-layer / per-interface numpy arrays."""
        return unpack_monitors(self.monitor_vector(), self.cfg.nlo)

    # -- area averages and the CFL check (`call areavg`, `call cfltry`) ---------------------------------
    def area_averages(self, parts=False):
        """tavoc (tavat on an atmosphere) of one `call areavg`: the weighted averages of sst (ast) at its current
        level over the areas of set_areas, from the device.  parts: (averages, numerators, denominators) of areint."""
        n = self.L.qgcm_hip_areavg_count(self.h)
        avg, num, den = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
        check(self.L.qgcm_hip_areavg(self.h, _dp(avg), _dp(num), _dp(den)))
        return (avg[:n], num[:n], den[:n]) if parts else avg[:n]

    def cfl(self, cflcrit=0.8):
        """`call cfltry` without its print-out: dict of names, maxima (the largest |u|, |v| of the mixed layer with its
        Ekman part, then the geostrophic ones per layer), courant = maxima*dt/dx, nbad (the points the reference would
        list as Bad: Courant number >= cflcrit) and loc (1-based i, j of each maximum, first in scan order)."""
        nq = self.L.qgcm_hip_cfl_len(self.h)
        mx, nb, loc = np.zeros(nq), np.zeros(nq, dtype=np.int32), np.zeros(2 * nq, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        check(self.L.qgcm_hip_cfl(self.h, float(cflcrit), _dp(mx), nb.ctypes.data_as(ip), loc.ctypes.data_as(ip)))
        return cfl_dict(self.cfg, mx, nb, loc)

    # -- time averages (avg_ocn_k247 / ocnc_avgout_k247, tavocn / tavout) --------------------------
    def po_mean(self, reset=False, count=False):
        """po_avg * (1/nsum) (nxpo, nypo, nlo), as ocnc_avgout_k247 scales it; reset=True then zeroes sum and count.
        count=True returns (mean, nsum)."""
        a, n = Handle.po_mean(self, reset)
        return (a, n) if count else a

    def time_means(self, names=None):
        """tavout's means (src/timavge.F:667-880) keyed by the reference's names (TAV_LAYOUT), plus "nsumoc".  The
        sums are not changed.  names: the subset to compute and copy (None = all)."""
        out, n = Handle.time_means(self, names)
        out["nsumoc"] = n
        return out

    # -- periodic ocean dumps (qocdiag_out, ocnc_out) ---------------------------------------------------
    def schedule_vorticity_budget(self, nsko, every, capacity=1):
        """Record the budget inside steps() on every step s with (s-1) % every == 0, after the step's oml and before
        its tendency, into a device ring of `capacity` snapshots.  every = 0 removes the schedule."""
        check(self.L.qgcm_hip_qocdiag_schedule(self.h, int(nsko), int(every), int(capacity)))
        self._qd_nsko = int(nsko)

    def read_vorticity_budgets(self):
        """The unread scheduled snapshots, oldest first, as a list of (step, dict); they are freed."""
        n = C.c_int()
        check(self.L.qgcm_hip_qocdiag_read(self.h, None, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        nsko = self._qd_nsko
        ln = self.L.qgcm_hip_qocdiag_len(self.h, nsko)
        out = np.zeros(n.value * ln)
        st = (C.c_int * n.value)()
        got = C.c_int()
        check(self.L.qgcm_hip_qocdiag_read(self.h, _dp(out), st, n.value, C.byref(got)))
        ip = subsample_count(self.cfg.nxpo, nsko)
        return [(st[r], unpack_budget(out[r * ln:(r + 1) * ln], self.cfg.nlo, ip)) for r in range(got.value)]

    # -- ocean mixed layer (`call oml`, src/q-gcm.F:1232) -------
    def oml(self):
        check(self.L.qgcm_hip_oml(self.h))

    def oml_get_diag(self):
        """entoc(nxpo,nypo) and (xon(1), cfraoc, centoc, enisoc(1), eninoc(1))."""
        e = np.zeros((self.cfg.nxpo, self.cfg.nypo), order="F")
        d = np.zeros(5)
        check(self.L.qgcm_hip_oml_get_diag(self.h, _dp(e), _dp(d)))
        return e, d

    # -- the work array and the Helmholtz solve by themselves ---------------------------------------------------
    def wrk_set(self, wrk):
        w = _f(wrk)
        assert w.shape == (self.cfg.nxpo, self.cfg.nypo, self.cfg.nlo)
        check(self.L.qgcm_hip_wrk_set(self.h, _dp(w)))

    def helmholtz(self, wrk, boc):
        """hsbxoc / hscyoc replacement (src/ocisubs.F:415-618); returns the solution."""
        w = np.array(wrk, dtype=np.float64, order="F", copy=True)
        b = np.ascontiguousarray(boc, dtype=np.float64)
        check(self.L.qgcm_hip_helmholtz(self.h, _dp(w), _dp(b)))
        return w

    # -- measurement ------------------------------------------------------------
    def time_steps(self, n, s0=None):
        """HIP-event time (ms) of n steps on the handle's stream."""
        s0 = self.step_index if s0 is None else int(s0)
        ms = C.c_float()
        check(self.L.qgcm_hip_time_steps(self.h, s0, int(n), C.byref(ms)))
        self.step_index = s0 + int(n)
        return ms.value

    def prepare_steps(self, n, s0=None):
        """Build the HIP graphs steps(n, s0) will replay (nothing runs): keeps graph capture / instantiation out of a
        window the caller times with its own clock."""
        s0 = self.step_index if s0 is None else int(s0)
        check(self.L.qgcm_hip_prepare_steps(self.h, s0, int(n)))

    # -- covariance matrices (covini / covocn and covout's arrays, src/covaria_diag.F) ---------------------
    def covocn(self):
        """One covocn contribution from the device state (po layer 1; sst of the mixed layer, else of
        set_monitor_fields)."""
        check(self.L.qgcm_hip_cov_add(self.h))

    def schedule_covariance(self, every, phase=0):
        """Add a contribution inside steps() / coupled_steps() after every step s with s % every == phase (after the
        step's averaging and a scheduled tavatm).  Reference cadence: ocean every = ntcovoc // nstr,
        phase = ((nsteps0 + nstr - 1) // nstr) % every; atmosphere every = ntcovat, phase = nsteps0 % ntcovat.
        every = 0 removes the schedule."""
        check(self.L.qgcm_hip_cov_schedule(self.h, int(every), int(phase)))

    def profile_steps(self, n, s0=None):
        """Per-kernel HIP-event totals over n eagerly launched steps:
        {name: (total_ms, launches)}."""
        s0 = self.step_index if s0 is None else int(s0)
        cap = 32
        ms = (C.c_double * cap)()
        ln = (C.c_int * cap)()
        names = (C.c_char_p * cap)()
        nk = C.c_int(cap)
        check(self.L.qgcm_hip_profile_steps(self.h, s0, int(n), ms, ln, names, C.byref(nk)))
        self.step_index = s0 + int(n)
        return {names[i].decode(): (ms[i], ln[i]) for i in range(nk.value)}

    def stream_mix_bandwidth(self, nr, nw, field_bytes, reps=20):
        """GB/s of a pure streaming kernel reading nr and writing nw fields of field_bytes (the practical ceiling for a
        kernel of that mix at that size)."""
        g = C.c_double()
        check(self.L.qgcm_hip_stream_mix_bandwidth(self.h, int(nr), int(nw), C.c_size_t(int(field_bytes)), int(reps), C.byref(g)))
        return g.value

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        g = C.c_double()
        check(self.L.qgcm_hip_copy_bandwidth(self.h, C.c_size_t(nbytes), int(reps), C.byref(g)))
        return g.value


_ATM_NAMES = {"amatat": "amatoc", "rdm2at": "rdm2oc", "ctl2mat": "ctl2moc", "ctm2lat": "ctm2loc",
              "pch1at": "pch1oc", "pch2at": "pch2oc", "pbhat": "pbhoc", "aipcha": "aipcho", "hc1sat": "hc1soc",
              "hc2sat": "hc2soc", "hc1nat": "hc1noc", "hc2nat": "hc2noc", "hbsiat": "hbsioc", "aipbha": "aipbho"}


class AtmosModel(OceanModel):
    """The atmospheric channel of a coupled run on the GPU.  The reference steps it with

        call qgastep ; call atinvq ; call atqzbd (qa, pa)          (src/q-gcm.F:1262-1268)

    on MODULE atstate / athomog arrays; the same three names are methods here.  ``cfg`` is an AtmosConfig; the
    inherited accessors carry the atmosphere's arrays: get_state() = pa, pam, qa, qam; get_scalars() = dpiat,
    dpiatp, atmcs, atmcn, atmcsp, atmcnp; steps(n) averages the time levels when mod(nt-1,100) == 0
    (src/q-gcm.F:1370).  ``consts`` may carry the reference's own eigmod / homsol products under their atmosphere
    names (amatat, ctl2mat, ..., pch1at, ...), as a drop-in host would pass them."""

    def __init__(self, cfg, ddynat=None, device=-1, consts=None):
        if consts is not None:
            consts = {_ATM_NAMES.get(k, k): v for k, v in consts.items()}
        OceanModel.__init__(self, cfg, ddynoc=ddynat, device=device, consts=consts)

    def set_forcing(self, wekpa=None, entat=None, xan=None, txis=None, txin=None, enis=None, enin=None):
        """wekpa, entat (p grid), xan(nla-1) and the line integrals txisat, txinat, enisat, eninat that
        xforc / aml leave in MODULE atstate / athomog."""
        OceanModel.set_forcing(self, wekpa, entat, xan)
        if txis is not None or txin is not None or enis is not None or enin is not None:
            self.set_cyc_forcing(0.0 if txis is None else txis, 0.0 if txin is None else txin, enis, enin)

    def qgastep(self):
        check(self.L.qgcm_hip_qgastep(self.h))

    def atinvq(self):
        check(self.L.qgcm_hip_atinvq(self.h))

    def atqzbd(self):
        check(self.L.qgcm_hip_atqzbd(self.h))

    # -- atmosphere monitors and valids (atmosphere half of `call monnc_comp` + courat, valids) ---------
    def set_atm_monitor_params(self, ocean=None, **kw):
        """Constants of MODULE atconst / radiate / parameters that monnc_comp reads and the handle does not hold;
        keywords and defaults: qgcm_hip.model.atm_mon_params (rhoat = 1.0, cpat = 1.0e3, hmat = 1000 as in
        examples/double_gyre_coupled's input.params; davgat, aup, bup, cup, dup = 0; nxaooc, nyaooc from `ocean`,
        an OceanConfig, and nx1, ny1 centred as src/parameters_data.F places the ocean)."""
        p = atm_mon_params(self.cfg, ocean, **kw)
        check(self.L.qgcm_hip_set_atm_mon_params(self.h, C.byref(p)))

    def set_atm_monitor_fields(self, wekta=None, tauxa=None, tauya=None, ast=None, hmixa=None, uekat=None, vekat=None):
        """wekta, ast, hmixa (nxta,nyta), tauxa, tauya (nxpa,nypa), uekat (nxpa,nyta), vekat (nxta,nypa): what xforc /
        aml leave on the host.  None = leave unchanged."""
        a = [_f(x) for x in (wekta, tauxa, tauya, ast, hmixa, uekat, vekat)]
        check(self.L.qgcm_hip_set_atm_monitor_fields(self.h, *[_dp(x) for x in a]))

    def monitor_vector(self):
        """The packed result of qgcm_hip_atm_monitors (order: include/qgcm_hip.h)."""
        out = np.zeros(self.L.qgcm_hip_atm_monitor_len(self.h))
        check(self.L.qgcm_hip_atm_monitors(self.h, _dp(out)))
        return out

    def monitors(self):
        """The atmosphere variables of MODULE monitor that monnc_comp / courat compute, from the device state without
        pulling it: dict keyed by the reference's names (ATM_MONITOR_LAYOUT)."""
        return unpack_atm_monitors(self.monitor_vector(), self.cfg.nla)

    def atm_valids(self):
        """(solnok, out): out = min, max of pa, qa, ast, wekta, tauxa, tauya (src/valsubs.F:120-269)."""
        out = np.zeros(len(ATM_VALIDS_NAMES))
        ok = C.c_int()
        check(self.L.qgcm_hip_atm_valids(self.h, _dp(out), C.byref(ok)))
        return bool(ok.value), out

    # -- time averages and periodic dump (tavatm / tavout's atmosphere half, atnc_out) ---------------------
    # (tavocn() stays the ocean's and refuses this handle)
    def set_time_mean_fields(self, fnetat=None):
        """fnetat (nxta, nyta) that tavatm sums (MODULE intrfac).  None = leave unchanged."""
        check(self.L.qgcm_hip_set_atm_tav_fields(self.h, _dp(_f(fnetat))))

    def tavatm(self):
        """One tavatm contribution from the device state (src/timavge.F:278-421); tauxa, tauya, wekta, ast come from
        set_atm_monitor_fields, hmat from set_atm_monitor_params, fnetat from set_time_mean_fields."""
        check(self.L.qgcm_hip_tavatm(self.h))

    def time_means(self, names=None):
        """tavout's atmosphere means (src/timavge.F:715-801) keyed by the reference's names (ATM_TAV_LAYOUT), plus
        "nsumat".  The sums are not changed.  names: the subset to compute and copy (None = all)."""
        from .lib import ATM_TAV_NOUT
        unknown = set(names or ()) - set(n for n, _ in ATM_TAV_LAYOUT)
        if unknown:
            raise QgcmHipError("unknown time means %s (ATM_TAV_LAYOUT)" % sorted(unknown))
        nxp, nyp, nl = self.cfg.nxpa, self.cfg.nypa, self.cfg.nla
        shape = dict(p=(nxp, nyp), t=(nxp - 1, nyp - 1), p3=(nxp, nyp, nl), u=(nxp, nyp - 1), v=(nxp - 1, nyp))
        out, n = read_means(ATM_TAV_LAYOUT, self.L.qgcm_hip_atm_tav_out, ATM_TAV_NOUT, self.h, shape, names)
        out["nsumat"] = n
        return out

    def reset_time_means(self):
        """tavini's atmosphere half: zero the sums and the count."""
        check(self.L.qgcm_hip_atm_tav_reset(self.h))

    def schedule_time_means(self, every, phase=0):
        """Add a tavatm contribution inside steps() / coupled_steps() after every step nt with nt % every == phase
        (after the step's averaging); the reference's cadence is every = ntavat, phase = (nmidat + nsteps0) % ntavat.
        every = 0 removes the schedule."""
        check(self.L.qgcm_hip_tavatm_schedule(self.h, int(every), int(phase)))

    def atmos_dump(self, nska=1, outflat=(1, 1, 1, 1, 1, 1, 1)):
        """atnc_out's subsampled fields (the selected ones): ast, wekta, hmixa (jtwk, itwk); tauxa, tauya (jpwk, ipwk);
        pa, qa (nla, jpwk, ipwk); ha = (pa(k)-pa(k+1))/gpat(k) (nla-1, jpwk, ipwk)."""
        c, L = self.cfg, self.L
        counts = lambda: dict(p=(subsample_count(c.nypa, nska), subsample_count(c.nxpa, nska)),
                              t=(subsample_count(c.nypa - 1, nska), subsample_count(c.nxpa - 1, nska)))
        return read_dump(ATNC_FIELDS, L.qgcm_hip_atnc_sample_len, L.qgcm_hip_atnc_sample, self.h, nska, outflat, c.nla,
                          counts)

    # -- covariance matrices (covatm): pa layer 1 and ast of set_atm_monitor_fields -------------------------
    _COV_NAMES = COV_NAMES_ATM

    def enable_covariance(self, nsi=2):
        """covini's atmosphere half (nsi = nscvat)."""
        OceanModel.enable_covariance(self, nsi)

    def covatm(self):
        """One covatm contribution from the device state (pa layer 1, ast)."""
        check(self.L.qgcm_hip_cov_add(self.h))

    def covocn(self):
        raise QgcmHipError("covocn is the ocean's; an atmosphere handle accumulates with covatm()")

    # -- atmospheric mixed layer (`call aml`, src/q-gcm.F:1260) -----------------------------------------
    def aml_init(self, am, xc1ast=None, dtopat=None):
        """Switch the mixed layer on (am: qgcm_hip.config.AmlConfig; xc1ast (nxta,nyta), dtopat (nxpa,nypa): None =
        zeros): the model then owns ast, astm, hmixa, hmixam; steps() / coupled_steps() run aml before qgastep in every
        step and average ast, hmixa with the other fields; the monitors, atm_valids, tavatm, covatm and atmos_dump read
        the stepped ast / hmixa (what set_atm_monitor_fields gave before is kept as the current level)."""
        from .lib import AmlParams
        c = self.cfg
        p = AmlParams()
        p.hmat, p.hmamin, p.hmadmp, p.rrcpat = am.hmat, am.hmamin, am.hmadmp, am.rrcpat
        p.tat1, p.tat2, p.xcexp = am.tat[0], am.tat[1], am.xcexp
        p.at2d, p.at4d, p.ahmd = am.at2d, am.at4d, am.ahmd
        if len(am.aface) != c.nla - 1:
            raise QgcmHipError("aml_init: aface has %d entries, need nla - 1 = %d" % (len(am.aface), c.nla - 1))
        for l, v in enumerate(am.aface):
            p.aface[l] = v
        p.bface, p.cface, p.dface = am.bface, am.cface, am.dface
        x, d = _f(xc1ast), _f(dtopat)
        if x is not None and x.shape != (c.nxta, c.nyta):
            raise QgcmHipError("aml_init: xc1ast has shape %s, need (%d, %d)" % (x.shape, c.nxta, c.nyta))
        if d is not None and d.shape != (c.nxpa, c.nypa):
            raise QgcmHipError("aml_init: dtopat has shape %s, need (%d, %d)" % (d.shape, c.nxpa, c.nypa))
        p.xc1ast, p.dtopat = _dp(x), _dp(d)
        check(self.L.qgcm_hip_aml_init(self.h, C.byref(p)))
        self.aml_cfg = am

    def aml_set_state(self, ast=None, astm=None, hmixa=None, hmixam=None):
        a = [_f(x) for x in (ast, astm, hmixa, hmixam)]
        for x in a:
            assert x is None or x.shape == (self.cfg.nxta, self.cfg.nyta)
        check(self.L.qgcm_hip_aml_set_state(self.h, *[_dp(x) for x in a]))

    def aml_get_state(self):
        """ast, astm, hmixa, hmixam (nxta, nyta)."""
        a = [np.zeros((self.cfg.nxta, self.cfg.nyta), order="F") for _ in range(4)]
        check(self.L.qgcm_hip_aml_get_state(self.h, *[_dp(x) for x in a]))
        return a

    def aml(self):
        """One `call aml` from the device state; asynchronous."""
        check(self.L.qgcm_hip_aml(self.h))

    def aml_get_diag(self):
        """entat (nxpa, nypa) and dict(xan, enisat, eninat, cfraat, centat): the first entries of xan, enisat, eninat
        where qgastep reads them and the two monitors; xan_v, enisat_v, eninat_v: the whole vectors (nla-1) - aml
        writes their first entries only."""
        ni = self.cfg.nla - 1
        e = np.zeros((self.cfg.nxpa, self.cfg.nypa), order="F")
        d = np.zeros(3 * ni + 2)
        check(self.L.qgcm_hip_aml_get_diag(self.h, _dp(e), _dp(d)))
        out = dict(xan=float(d[0]), enisat=float(d[ni]), eninat=float(d[2 * ni]), cfraat=float(d[3 * ni]),
                   centat=float(d[3 * ni + 1]))
        out.update(xan_v=tuple(d[:ni]), enisat_v=tuple(d[ni:2 * ni]), eninat_v=tuple(d[2 * ni:3 * ni]))
        return e, out

    pa = OceanModel.po
    pam = OceanModel.pom
    qa = OceanModel.qo
    qam = OceanModel.qom


def share_gpu(ocean, atmos, atmos_cus=None):
    """Give the two halves of a coupled run disjoint CU ranges of the GPU they share (qgcm_hip_set_cu_range): the
    atmosphere the first atmos_cus compute units (default 2/8 of the device: 64 of an MI355X's 256 = two XCDs), the ocean the rest;
    atmos_cus = 0 returns both to unrestricted streams.  Call before coupled_steps."""
    import torch
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    acu = ncu // 4 if atmos_cus is None else int(atmos_cus)
    if acu == 0:
        check(ocean.L.qgcm_hip_set_cu_range(ocean.h, 0, 0))
        check(atmos.L.qgcm_hip_set_cu_range(atmos.h, 0, 0))
    else:
        check(atmos.L.qgcm_hip_set_cu_range(atmos.h, 0, acu))
        check(ocean.L.qgcm_hip_set_cu_range(ocean.h, acu, ncu - acu))
    return acu


XFORC_FIELDS = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa", "tauxo", "tauyo", "wekto", "wekpo")
XFORC_INTEGRALS = ("txisat", "txinat", "txisoc", "txinoc")


def xforc_setup(ocean, atmos, cdat=1.3e-3, rhoat=1.0, rhooc=1.0e3, hmat=1000.0, hmoc=100.0, tau_udiff=False,
                tables=None, ndxr=None, nxaooc=None, nyaooc=None, nx1=None, ny1=None):
    """Set up the momentum half of xforc on the device (qgcm_hip_xforc_init) for the whole-domain models
    `ocean` (or None: the atmos_only half) and `atmos`.  cdat, hmat, hmoc and raoro = rhoat/rhooc default to the
    double-gyre input.params; bccoat / bccooc come from the configurations.  tau_udiff: the reference's cpp option.
    tables: the five bicubic weight tables {"stbbb", "stbus", "stbvs", "stbun", "stbvn"}, (16, ndxr+1, ndxr+1) each;
    default hostinit.bcuini.  The position of the ocean defaults to MODULE parameters' centring,
    nx1 = 1 + (nxta - nxaooc)/2 (likewise ny1)."""
    from .lib import XforcParams
    acfg = atmos.cfg
    if ocean is not None:
        oc = ocean.cfg
        ndxr = oc.ndxr if ndxr is None else ndxr
        nxaooc = oc.nxaooc if nxaooc is None else nxaooc
        nyaooc = oc.nyaooc if nyaooc is None else nyaooc
    elif ndxr is None:
        raise QgcmHipError("xforc_setup: without an ocean give ndxr")
    nxaooc = acfg.nxta if nxaooc is None else int(nxaooc)
    nyaooc = acfg.nyta if nyaooc is None else int(nyaooc)
    ndxr = int(ndxr)
    if tables is None:
        if ndxr < 1:
            raise QgcmHipError("xforc_setup: ndxr = %d" % ndxr)
        tables = hostinit.bcuini(ndxr, acfg.bccoat, acfg.dya)
    keep = [np.asfortranarray(tables[k], dtype=np.float64) for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")]
    for t in keep:
        if t.shape != (16, ndxr + 1, ndxr + 1):
            raise QgcmHipError("xforc_setup: a weight table has shape %s, need (16, %d, %d)" % (t.shape, ndxr + 1, ndxr + 1))
    p = XforcParams()
    p.ndxr, p.nxaooc, p.nyaooc = ndxr, int(nxaooc), int(nyaooc)
    p.nx1 = 1 + (acfg.nxta - p.nxaooc) // 2 if nx1 is None else int(nx1)
    p.ny1 = 1 + (acfg.nyta - p.nyaooc) // 2 if ny1 is None else int(ny1)
    p.cdat, p.raoro, p.hmat, p.hmoc = float(cdat), float(rhoat) / float(rhooc), float(hmat), float(hmoc)
    p.bccoat = float(acfg.bccoat)
    p.bccooc = float(ocean.cfg.bccooc) if ocean is not None else 0.0
    p.tau_udiff = int(bool(tau_udiff))
    p.stbbb, p.stbus, p.stbvs, p.stbun, p.stbvn = [_dp(t) for t in keep]
    check(atmos.L.qgcm_hip_xforc_init(ocean.h if ocean is not None else None, atmos.h, C.byref(p)))
    atmos.xforc_origin = (int(p.nx1), int(p.ny1))  # (where xforc_heat_setup finds the ocean)


def xforc(ocean, atmos):
    """One `call xforc` (momentum half) from the lagged pressures on the device; asynchronous (qgcm_hip_xforc)."""
    check(atmos.L.qgcm_hip_xforc(ocean.h if ocean is not None else None, atmos.h))


def xforc_get(ocean, atmos, names=None):
    """The outputs of the last xforc as a dict: XFORC_FIELDS (the ocean's only with an ocean) and XFORC_INTEGRALS."""
    a = atmos.cfg
    shapes = dict(tauxa=(a.nxpa, a.nypa), tauya=(a.nxpa, a.nypa), uekat=(a.nxpa, a.nyta), vekat=(a.nxta, a.nypa),
                  wekta=(a.nxta, a.nyta), wekpa=(a.nxpa, a.nypa))
    if ocean is not None:
        o = ocean.cfg
        shapes.update(tauxo=(o.nxpo, o.nypo), tauyo=(o.nxpo, o.nypo), wekto=(o.nxto, o.nyto), wekpo=(o.nxpo, o.nypo))
    want = [n for n in XFORC_FIELDS if n in shapes and (names is None or n in names)]
    out = {n: np.zeros(shapes[n], order="F") for n in want}
    txi = np.zeros(4)
    check(atmos.L.qgcm_hip_xforc_get(ocean.h if ocean is not None else None, atmos.h,
                                     *[_dp(out.get(n)) for n in XFORC_FIELDS], _dp(txi)))
    for k, n in enumerate(XFORC_INTEGRALS):
        if names is None or n in names:
            out[n] = float(txi[k])
    return out


HEAT_SCALARS = ("arlaav", "slhfav", "oradav", "arocav")


def _heat_params(who, p, atmos, ocean_cfg, heat, hmadmp, hmat, coords, **fs):
    """What xforc_heat_setup and xforc_sst_setup (`who`, for the messages) share: fills into `p` (XforcHeatParams /
    XforcSstParams) the radiation constants of `heat`, hmadmp, hmat (default: what aml_init was given), the tables
    fs = fsa[, fso] (None: hostinit.fsprim) and the coordinates xta, yta, xto, yto of hostinit.grid_coordinates with the
    ocean where xforc_setup placed it, overridden by `coords`.  Returns the arrays `p` points to: keep them until the
    library has copied them."""
    am = getattr(atmos, "aml_cfg", None)
    if (hmadmp is None or hmat is None) and am is None:
        raise QgcmHipError("%s: call atmos.aml_init first (qgcm_hip_aml_init has not been called)" % who)
    nx1, ny1 = getattr(atmos, "xforc_origin", (None, None))  # the position xforc_setup was given
    G = hostinit.grid_coordinates(atmos.cfg, ocean_cfg, nx1=nx1, ny1=ny1)
    if coords is not None:
        G = dict(G, **coords)
    for name, rel in (("fsa", "ytarel"), ("fso", "ytorel")):
        if name in fs:
            G[name] = hostinit.fsprim(G[rel], heat.fspco, G["yla"]) if fs[name] is None else fs[name]
    a, o = atmos.cfg, ocean_cfg
    want = dict(fsa=a.nyta, fso=o.nyto, xta=a.nxta, yta=a.nyta, xto=o.nxto, yto=o.nyto)
    keep = []
    for name in list(fs) + ["xta", "yta", "xto", "yto"]:
        v = np.ascontiguousarray(G[name], dtype=np.float64)
        if v.shape != (want[name],):
            raise QgcmHipError("%s: %s has shape %s, need (%d,)" % (who, name, v.shape, want[name]))
        setattr(p, name, _dp(v))
        keep.append(v)
    for k in ("xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup", "C1down"):
        setattr(p, k, float(getattr(heat, k)))
    p.hmadmp = float(am.hmadmp if hmadmp is None else hmadmp)
    p.hmat = float(am.hmat if hmat is None else hmat)
    return keep


def _heat_out(sc, **fields):
    """dict of the fields and the HEAT_SCALARS `sc` of qgcm_hip_xforc_heat_get / qgcm_hip_xforc_sst_get."""
    return dict(fields, **{k: float(v) for k, v in zip(HEAT_SCALARS, sc)})


def xforc_heat_setup(ocean, atmos, heat, hmadmp=None, hmat=None, fsa=None, fso=None, coords=None):
    """Set up the heat half of xforc on the device (qgcm_hip_xforc_heat_init) after xforc_setup(ocean,
    atmos), atmos.aml_init and ocean.oml_init: xforc() and coupled_steps(..., xforc=True) then also compute fnetoc
    (into the ocean mixed layer's forcing) and fnetat (where aml reads it).  heat: qgcm_hip.config.HeatConfig; hmadmp,
    hmat default to the values aml_init was given.  fsa / fso: the tables fsprim(ytarel(1:nyta)) / fsprim(ytorel(1:nyto))
    (default hostinit.fsprim); coords: dict(xta, yta, xto, yto), default hostinit.grid_coordinates with the ocean
    placed where xforc_setup placed it (its nx1, ny1)."""
    from .lib import XforcHeatParams
    p = XforcHeatParams()
    if ocean is None:  # (the library's own refusal: no coordinate can be derived without an ocean, so nothing else is passed)
        check(atmos.L.qgcm_hip_xforc_heat_init(None, atmos.h, C.byref(p)))
    keep = _heat_params("xforc_heat_setup", p, atmos, ocean.cfg, heat, hmadmp, hmat, coords, fsa=fsa, fso=fso)
    check(atmos.L.qgcm_hip_xforc_heat_init(ocean.h, atmos.h, C.byref(p)))
    del keep  # (copied by now)


def xforc_heat_get(ocean, atmos):
    """The outputs of the heat half of the last xforc: dict(fnetoc (nxto,nyto), fnetat (nxta,nyta), arlaav, slhfav,
    oradav, arocav)."""
    o, a = ocean.cfg, atmos.cfg
    fo, fa, sc = np.zeros((o.nxto, o.nyto), order="F"), np.zeros((a.nxta, a.nyta), order="F"), np.zeros(4)
    check(atmos.L.qgcm_hip_xforc_heat_get(ocean.h if ocean is not None else None, atmos.h, _dp(fo), _dp(fa), _dp(sc)))
    return _heat_out(sc, fnetoc=fo, fnetat=fa)


def xforc_sst_setup(atmos, ocean_cfg, heat, sst, hmadmp=None, hmat=None, fsa=None, coords=None):
    """Set up the heat half of xforc WITHOUT an ocean (qgcm_hip_xforc_sst_init, DESIGN 6n: the reference's atmos_only
    build) after xforc_setup(None, atmos, ndxr=..., nxaooc=..., nyaooc=...) and atmos.aml_init: xforc(None, atmos) and
    coupled_steps(None, atmos, ..., xforc=True) then also compute fnetat (where aml reads it) from the prescribed,
    held `sst` (nxto, nyto).  ocean_cfg: an OceanConfig used for the geometry of the sea only (nxaooc, nyaooc, ndxr,
    dxo, dyo); no OceanModel is needed.  heat: qgcm_hip.config.HeatConfig; hmadmp, hmat default to the values aml_init
    was given.  fsa: the table fsprim(ytarel(1:nyta)) (default hostinit.fsprim); coords: dict(xta, yta, xto, yto),
    default hostinit.grid_coordinates with the sea placed where xforc_setup placed it (its nx1, ny1)."""
    from .lib import XforcSstParams
    p = XforcSstParams()
    keep = _heat_params("xforc_sst_setup", p, atmos, ocean_cfg, heat, hmadmp, hmat, coords, fsa=fsa)
    s = _f(sst)
    if s is None or s.shape != (ocean_cfg.nxto, ocean_cfg.nyto):
        raise QgcmHipError("xforc_sst_setup: sst has shape %s, need (%d, %d)" % (None if s is None else s.shape,
                                                                                 ocean_cfg.nxto, ocean_cfg.nyto))
    p.dxo, p.dyo = float(ocean_cfg.dxo), float(ocean_cfg.dyo)
    p.sst = _dp(s)
    check(atmos.L.qgcm_hip_xforc_sst_init(atmos.h, C.byref(p)))
    del keep  # (copied by now)
    atmos.sst_shape = (int(ocean_cfg.nxto), int(ocean_cfg.nyto))


def xforc_sst_set(atmos, sst):
    """Replace the SST that xforc_sst_setup gave (qgcm_hip_xforc_sst_set): (nxto, nyto), held until the next call."""
    shape = getattr(atmos, "sst_shape", None)
    if shape is None:
        raise QgcmHipError("xforc_sst_set: qgcm_hip_xforc_sst_init has not been called (xforc_sst_setup first)")
    s = _f(sst)
    if s is None or s.shape != shape:
        raise QgcmHipError("xforc_sst_set: sst has shape %s, need (%d, %d)" % ((None if s is None else s.shape,) + shape))
    check(atmos.L.qgcm_hip_xforc_sst_set(atmos.h, _dp(s)))


def xforc_sst_get(atmos):
    """The outputs of the heat half of the last xforc(None, atmos): dict(fnetat (nxta,nyta), arlaav, slhfav, oradav,
    arocav); arocav is 0: the reference does not accumulate it when atmos_only."""
    a = atmos.cfg
    fa, sc = np.zeros((a.nxta, a.nyta), order="F"), np.zeros(4)
    check(atmos.L.qgcm_hip_xforc_sst_get(atmos.h, _dp(fa), _dp(sc)))
    return _heat_out(sc, fnetat=fa)


def coupled_steps(ocean, atmos, nt0, n, nstr, xforc=False):
    """n atmospheric steps nt = nt0.. with one ocean step before every one with mod(nt,nstr) == 1
    (src/q-gcm.F:1220-1268); either model may be None.  xforc = False: the forcing is held.  xforc = True (after
    xforc_setup): xforc runs on the device before every ocean step, in the reference's order - the momentum half and,
    after xforc_heat_setup, the heat half.  After atmos.aml_init every atmospheric step runs aml before qgastep, and
    after ocean.oml_init every ocean step runs oml: with all of them the window is the reference's full sequence
    xforc; oml; qgostep ...; (aml; qgastep ...) x nstr without a host transfer."""
    L = (ocean or atmos).L
    oh, ah = ocean.h if ocean is not None else None, atmos.h if atmos is not None else None
    if xforc or atmos is not None:
        check(L.qgcm_hip_coupled_set_xforc(oh, ah, 1 if xforc else 0))
    check(L.qgcm_hip_coupled_steps(oh, ah, int(nt0), int(n), int(nstr)))
    if atmos is not None:
        atmos.step_index = int(nt0) + int(n)
