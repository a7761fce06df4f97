"""Handle - what OceanModel (a handle that owns the whole domain) and HipSlab (a handle that owns a y-slab) share.

The library makes no distinction between the two: every entry point bound here takes a ``qgcm_hip_handle`` and works on
the rows that handle holds.  A Handle therefore carries a row view - the global p rows and T rows it stores, the number
of local rows and the counts of the rows it owns - and every method is written once against that view.  Arguments are
either LOCAL blocks (the handle's own rows: set_state, get_state, set_forcing, oml_get_state, wrk_get) or GLOBAL arrays
of which the stored rows are cut out here (oml_set_state, oml_set_forcing, set_monitor_fields, set_time_mean_fields,
set_dtopoc, set_sponge); for a whole-domain handle the cut is the identity.  None for a field means "leave unchanged"
(NULL to the library).
"""
import ctypes as C

import numpy as np

from .config import OmlConfig
from .hostinit import area_limits
from .lib import MAXL, TAV_NOUT, MonParams, OmlParams, Params, QgcmHipError, TavParams, check, load_library, row_plan, thomas_plan


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _f(a):
    return None if a is None else np.asfortranarray(a, dtype=np.float64)


def _cut(a, rows, shape=None):
    """The rows `rows` (axis 1) of the GLOBAL array `a` as a Fortran-ordered float64 block; no copy where `a` already
    is one and every row is taken.  shape: the global shape `a` must have."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    assert shape is None or a.shape == shape, "array of shape %s, need %s" % (a.shape, shape)
    return np.asfortranarray(a[:, rows])


def fill_params(cfg, consts, atmos=False, g=None):
    """struct qgcm_hip_params of the configuration `cfg` and the start-up constants `consts` (aoc, rdm2oc, amatoc,
    ctl2moc, ctm2loc); g = (g0, g1): the global rows of a y-slab (1-based, inclusive), None: the whole domain."""
    nl = cfg.nlo
    if nl > MAXL:
        raise QgcmHipError("nlo=%d exceeds QGCM_HIP_MAXL" % nl)
    p = Params()
    p.nxpo, p.nypo, p.nlo, p.cyclic, p.atmos = cfg.nxpo, cfg.nypo, nl, int(cfg.cyclic), int(atmos)
    p.fnot, p.beta, p.dxo, p.dyo = cfg.fnot, cfg.beta, cfg.dxo, cfg.dyo
    p.tdto, p.delek, p.bccooc, p.aoc = cfg.tdto, cfg.delek, cfg.bccooc, consts["aoc"]
    if g is not None:
        p.slab_g0, p.slab_g1 = g
    for k in range(nl):
        p.ah2oc[k], p.ah4oc[k], p.hoc[k], p.rdm2oc[k] = cfg.ah2oc[k], cfg.ah4oc[k], cfg.hoc[k], consts["rdm2oc"][k]
    for k in range(nl - 1):
        p.gpoc[k] = cfg.gpoc[k]
    for name in ("amatoc", "ctl2moc", "ctm2loc"):
        arr = getattr(p, name)
        for i, v in enumerate(np.asarray(consts[name]).ravel(order="F")):
            arr[i] = v
    return p


def mon_params(oml=None, rhooc=None, cpoc=None, hmoc=None, ycexp=None, sb_hflux=None, nb_hflux=None):
    """struct qgcm_hip_mon_params: the given values, the others from `oml` (a qgcm_hip.OmlConfig; its defaults are the
    examples' input.params values)."""
    om = OmlConfig() if oml is None else oml
    pick = lambda v, d: d if v is None else v
    p = MonParams()
    p.rhooc, p.cpoc = float(pick(rhooc, om.rhooc)), float(pick(cpoc, om.cpoc))
    p.hmoc, p.ycexp = float(pick(hmoc, om.hmoc)), float(pick(ycexp, om.ycexp))
    p.sb_hflux, p.nb_hflux = int(pick(sb_hflux, om.sb_hflux)), int(pick(nb_hflux, om.nb_hflux))
    return p


# outputs of qgcm_hip_tav_out in ABI order (names of MODULE timavge / tavout) and their grids: p = (nxpo, p rows),
# t = (nxto, T rows), p3 = (nxpo, p rows, nlo), u = (nxpo, T rows), v = (nxto, p rows)
TAV_LAYOUT = (("txocav", "p"), ("tyocav", "p"), ("wpocav", "p"), ("wtocav", "t"), ("fmocav", "t"), ("sstav", "t"),
              ("pocav", "p3"), ("qocav", "p3"), ("uufo", "u"), ("tufo", "u"), ("utufo", "u"), ("vvfo", "v"),
              ("tvfo", "v"), ("vtvfo", "v"), ("uptpoc", "u"), ("vptpoc", "v"))


def tav_params(oml=None, hmoc=None, ycexp=None, tsbdy=None, tnbdy=None, sb_hflux=None, nb_hflux=None):
    """struct qgcm_hip_tav_params: the given values, the others from `oml` (a qgcm_hip.OmlConfig)."""
    om = OmlConfig() if oml is None else oml
    pick = lambda v, d: d if v is None else v
    p = TavParams()
    p.hmoc, p.ycexp = float(pick(hmoc, om.hmoc)), float(pick(ycexp, om.ycexp))
    p.tsbdy, p.tnbdy = float(pick(tsbdy, om.tsbdy)), float(pick(tnbdy, om.tnbdy))
    p.sb_hflux, p.nb_hflux = int(pick(sb_hflux, om.sb_hflux)), int(pick(nb_hflux, om.nb_hflux))
    return p


def read_means(layout, entry, nout, h, shape, names):
    """The means `entry` (qgcm_hip_tav_out / qgcm_hip_atm_tav_out, `nout` outputs in `layout`'s order) returns for the
    given names (None = all): (dict name -> array, number of contributions).  shape: grid -> array shape."""
    want = [n for n, _ in layout] if names is None else list(names)
    out, ptrs = {}, (C.POINTER(C.c_double) * nout)()
    for i, (name, grid) in enumerate(layout):
        if name in want:
            out[name] = np.zeros(shape[grid], order="F")
            ptrs[i] = _dp(out[name])
    n = C.c_int()
    check(entry(h, ptrs, C.byref(n)))
    return out, n.value


# periodic ocean dumps (qgcm_hip_qocdiag / qgcm_hip_ocnc_sample)
QOCDIAG_TERMS = ("dqdt", "qotjac", "qt2dif", "qt4dif", "qotent")
# ocnc_out's fields in its order: (name, grid, planes in units of nlo: 0 = one plane, 1 = nlo, -1 = nlo-1, flag index)
# (tauxo and tauyo share outfloc(6))
OCNC_FIELDS = (("sst", "t", 0, 0), ("po", "p", 1, 1), ("qo", "p", 1, 2), ("wekto", "t", 0, 3), ("h", "p", -1, 4),
               ("tauxo", "p", 0, 5), ("tauyo", "p", 0, 5))


def subsample_count(n, nsko):
    """Points of a subsample: min(mod(n,nsko),1) + (n-mod(n,nsko))/nsko (src/qocdiag.F:360-363)."""
    m = n % nsko
    return min(m, 1) + (n - m) // nsko


def unpack_budget(v, nl, ipwk):
    """dict term -> (nlo, rows, ipwk) array from the packed out[term][k][jp][ip] of qgcm_hip_qocdiag."""
    a = v.reshape(len(QOCDIAG_TERMS), nl, -1, ipwk)
    return {t: a[n].copy() for n, t in enumerate(QOCDIAG_TERMS)}


def read_dump(fields, length, sample, h, nsk, flags, nl, counts):
    """The selected fields of `fields` (OCNC_FIELDS / ATNC_FIELDS) from the packed result of `sample`: dict name ->
    (planes, rows, columns) array, (rows, columns) for the one-plane fields.  counts(): grid -> (rows, columns)."""
    fl = (C.c_int * 7)(*[int(x) for x in flags])
    n = length(h, int(nsk), fl)
    if n < 0:
        check(1)
    out = np.zeros(n)
    check(sample(h, int(nsk), fl, _dp(out)))
    cnt, res, o = counts(), {}, 0
    for name, grid, planes, flag in fields:
        if int(flags[flag]) != 1:
            continue
        shp = ({0: 1, 1: nl, -1: nl - 1}[planes],) + cnt[grid]
        m = int(np.prod(shp))
        a = out[o:o + m].reshape(shp)
        res[name] = a[0] if planes == 0 else a
        o += m
    assert o == n
    return res


# covariance matrices (qgcm_hip_cov_*): covout's arrays under the reference's names, p-grid vector first
COV_NAMES_OCN = ("covpo", "avgpo", "swtpo", "nupo", "covto", "avgto", "swtto", "nuto")
COV_NAMES_ATM = ("covpa", "avgpa", "swtpa", "nupa", "covta", "avgta", "swtta", "nuta")


class Handle:
    """One qgcm_hip_handle: created here from `cfg` and the start-up constants `consts` on the GLOBAL grid (those of
    fill_params, yporel, bd2oc, ddynoc).  g = (g0, g1) and p_rows (the 0-based slice of the global p rows stored:
    owned rows and halo rows) make it a y-slab, rank `rank` of `nranks`; without them it owns the whole domain.

    The row view: p_rows, t_rows (slices of the global p / T rows stored; T row j lies between p rows j and j+1),
    nyl (local p rows), own_p, own_t (owned p / T rows: one T row fewer on the handle that owns row nypo)."""

    _COV_NAMES = COV_NAMES_OCN

    def __init__(self, cfg, consts, device=-1, atmos=False, g=None, p_rows=None, rank=0, nranks=1):
        self.cfg, self.rank, self.nranks = cfg, rank, nranks
        self.L = load_library()
        self.h = C.c_void_p()
        g0, g1 = (1, cfg.nypo) if g is None else g
        self.p_rows = slice(0, cfg.nypo) if p_rows is None else p_rows
        self.t_rows = slice(self.p_rows.start, self.p_rows.stop - 1)
        self.nyl = self.p_rows.stop - self.p_rows.start
        self.own_p = g1 - g0 + 1
        self.own_t = self.own_p - (1 if g1 == cfg.nypo else 0)
        self.nscal = 2 * (cfg.nlo - 1) + 4 * cfg.nlo
        self.params = fill_params(cfg, consts, atmos, g)
        check(self.L.qgcm_hip_create(C.byref(self.h), C.byref(self.params), int(device)))
        yp = np.ascontiguousarray(consts["yporel"][self.p_rows])
        bd2 = np.ascontiguousarray(consts["bd2oc"])
        dd = _cut(consts["ddynoc"], self.p_rows)
        check(self.L.qgcm_hip_set_grid(self.h, _dp(yp), _dp(bd2), _dp(dd)))

    def set_homog(self, ochom_local, cdiffo, cdhoc):
        """The homogeneous solutions of a box: ochom on the LOCAL rows, cdiffo, cdhoc."""
        args = [_f(a) for a in (ochom_local, cdiffo, cdhoc)]
        check(self.L.qgcm_hip_set_homog_box(self.h, *[_dp(a) for a in args]))

    def set_homog_box(self, hg):
        """As set_homog from the GLOBAL products of homsol (hostinit.homsol_box)."""
        self.set_homog(np.asarray(hg["ochom"])[:, self.p_rows, :], hg["cdiffo"], hg["cdhoc"])

    def set_homog_cyc(self, hg):
        """The homogeneous solutions of a channel from the GLOBAL products of hostinit.homsol_cyc: they depend on y
        only (conhoms.F:376-543), so the stored rows and the global scalars."""
        sl = self.p_rows
        args = [_f(hg["pch1oc"][sl, :]), _f(hg["pch2oc"][sl, :]), np.ascontiguousarray(hg["pbhoc"][sl]),
                *[np.ascontiguousarray(hg[k], dtype=np.float64) for k in ("aipcho", "hc1soc", "hc2soc", "hc1noc", "hc2noc")]]
        check(self.L.qgcm_hip_set_homog_cyc(self.h, *[_dp(a) for a in args], float(hg["hbsioc"]), float(hg["aipbho"])))

    # -- life cycle ----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.L.qgcm_hip_destroy(self.h)
            self.h = C.c_void_p()

    def sync(self):
        check(self.L.qgcm_hip_sync(self.h))

    def _done(self):
        """Called after every call that launches work (HipSlab: a sync when sync_each_call is set)."""

    def thomas_plan(self):
        """[(first, count)] per segment of the handle's interior rows (lib.thomas_plan); one entry: the single launch."""
        return thomas_plan(self.h)

    def row_plan(self):
        """(P, L): the handle transforms each row as P interleaved sub-rows of length L (lib.row_plan); (1, nxto): whole."""
        return row_plan(self.h)

    # -- state (LOCAL blocks: the handle's rows, halo rows included) -------------
    def set_state(self, po=None, pom=None, qo=None, qom=None):
        a = [_f(x) for x in (po, pom, qo, qom)]
        check(self.L.qgcm_hip_set_state(self.h, *[_dp(x) for x in a]))

    def get_state(self):
        a = [np.zeros((self.cfg.nxpo, self.nyl, self.cfg.nlo), order="F") for _ in range(4)]
        check(self.L.qgcm_hip_get_state(self.h, *[_dp(x) for x in a]))
        return a

    def set_forcing(self, wekpo=None, entoc=None, xon=None):
        w, e = _f(wekpo), _f(entoc)
        x = None if xon is None else np.ascontiguousarray(xon, dtype=np.float64)
        check(self.L.qgcm_hip_set_forcing(self.h, _dp(w), _dp(e), _dp(x)))

    def set_cyc_forcing(self, txisoc, txinoc, enisoc=None, eninoc=None):
        nl = self.cfg.nlo
        es = np.zeros(nl - 1) if enisoc is None else np.ascontiguousarray(enisoc, dtype=np.float64)
        en = np.zeros(nl - 1) if eninoc is None else np.ascontiguousarray(eninoc, dtype=np.float64)
        check(self.L.qgcm_hip_set_cyc_forcing(self.h, float(txisoc), float(txinoc), _dp(es), _dp(en)))

    def set_sponge(self, r_spl, c1_spl):
        """The fork's sponge layer (src/qgosubs.F:203-205): the GLOBAL ramp r_spl(nxpo, nypo) and the constant c1_spl;
        r_spl = None switches the term off."""
        r = _cut(r_spl, self.p_rows, (self.cfg.nxpo, self.cfg.nypo))
        check(self.L.qgcm_hip_set_sponge(self.h, _dp(r), 0.0 if r is None else float(c1_spl)))

    def set_scalars(self, s):
        s = np.ascontiguousarray(s, dtype=np.float64)
        assert s.size == self.nscal
        check(self.L.qgcm_hip_set_scalars(self.h, _dp(s)))

    def get_scalars(self):
        s = np.zeros(self.nscal)
        check(self.L.qgcm_hip_get_scalars(self.h, _dp(s)))
        return s

    def get_monitors(self):
        """(ermaso, emfroc) of the last ocinvq / constraint solve of a zonally cyclic ocean (src/ocisubs.F:268-283;
        atmosphere: ermasa, emfrat): nlo-1 values each, the same on every rank."""
        e, f = np.zeros(self.cfg.nlo - 1), np.zeros(self.cfg.nlo - 1)
        check(self.L.qgcm_hip_get_monitors(self.h, _dp(e), _dp(f)))
        return e, f

    # -- kernels by themselves ----------------------------------------------------
    def qgostep(self):
        check(self.L.qgcm_hip_qgostep(self.h))
        self._done()

    def lf_average(self):
        check(self.L.qgcm_hip_lf_average(self.h))
        self._done()

    def row_transform(self, inverse):
        """The row transforms by themselves (replacements of FFTPACK's dsint / drfftf / drfftb)."""
        check(self.L.qgcm_hip_row_transform(self.h, int(inverse)))
        self._done()

    def wrk_get(self):
        w = np.zeros((self.cfg.nxpo, self.nyl, self.cfg.nlo), order="F")
        check(self.L.qgcm_hip_wrk_get(self.h, _dp(w)))
        return w

    # -- ocean mixed layer (`call oml`, src/q-gcm.F:1232) -------
    def oml_init(self, om):
        """Switch the mixed layer on (om: qgcm_hip.config.OmlConfig): steps() then runs oml before qgostep in every
        step and averages sst with the other fields."""
        p = OmlParams()
        p.hmoc, p.toc1, p.toc2, p.st2d, p.st4d = om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d
        p.ycexp, p.rrcpoc, p.tsbdy, p.tnbdy = om.ycexp, om.rrcpoc, om.tsbdy, om.tnbdy
        p.sb_hflux, p.nb_hflux = int(om.sb_hflux), int(om.nb_hflux)
        check(self.L.qgcm_hip_oml_init(self.h, C.byref(p)))

    def oml_set_state(self, sst=None, sstm=None):
        """sst, sstm: GLOBAL (nxto, nyto) arrays."""
        a = [_cut(x, self.t_rows, (self.cfg.nxto, self.cfg.nyto)) for x in (sst, sstm)]
        check(self.L.qgcm_hip_oml_set_state(self.h, *[_dp(x) for x in a]))

    def oml_get_state(self):
        """LOCAL (nxto, nyl-1) sst, sstm; on a slab the owned T rows are local rows jlo..(jhi, or jhi-1 on the last
        rank)."""
        a = [np.zeros((self.cfg.nxto, self.nyl - 1), order="F") for _ in range(2)]
        check(self.L.qgcm_hip_oml_get_state(self.h, *[_dp(x) for x in a]))
        return a

    def oml_set_forcing(self, fnetoc=None, wekto=None, tauxo=None, tauyo=None):
        """GLOBAL arrays: fnetoc, wekto on the T grid (nxto, nyto); tauxo, tauyo on the p grid (nxpo, nypo)."""
        a = [_cut(fnetoc, self.t_rows), _cut(wekto, self.t_rows), _cut(tauxo, self.p_rows), _cut(tauyo, self.p_rows)]
        check(self.L.qgcm_hip_oml_set_forcing(self.h, *[_dp(x) for x in a]))

    # -- what the diagnostics read (monnc_comp + couroc, valids, areavg) --------------
    def set_monitor_params(self, oml=None, rhooc=None, cpoc=None, hmoc=None, ycexp=None, sb_hflux=None, nb_hflux=None):
        """Constants of MODULE occonst / intrfac that monnc_comp and couroc read and the handle does not hold:
        rhooc, cpoc, and hmoc, ycexp, sb_hflux, nb_hflux of couroc's mixed-layer velocities.  Defaults come from
        `oml` (a qgcm_hip.OmlConfig; its defaults are the examples' input.params values)."""
        p = mon_params(oml, rhooc, cpoc, hmoc, ycexp, sb_hflux, nb_hflux)
        check(self.L.qgcm_hip_set_mon_params(self.h, C.byref(p)))

    def set_monitor_fields(self, tauxo=None, tauyo=None, wekto=None, sst=None):
        """GLOBAL tauxo, tauyo (nxpo,nypo), wekto, sst (nxto,nyto): the fields the monitors read that do not evolve on
        the device without the mixed layer (with it on, its own arrays are read).  None = leave unchanged."""
        a = [_cut(tauxo, self.p_rows), _cut(tauyo, self.p_rows), _cut(wekto, self.t_rows), _cut(sst, self.t_rows)]
        check(self.L.qgcm_hip_set_monitor_fields(self.h, *[_dp(x) for x in a]))

    def set_dtopoc(self, dtopoc):
        """GLOBAL bottom topography (nxpo, nypo) for valids, None = flat."""
        d = _cut(dtopoc, self.p_rows)
        check(self.L.qgcm_hip_set_dtopoc(self.h, _dp(d)))

    def set_areas(self, xlo=None, xhi=None, ylo=None, yhi=None, tables=None):
        """The areas of areavg (of the whole basin: global rows, the same on every rank): their limits in metres from
        the domain's south-west corner, as `areas.limits` gives them (hostinit.read_areas_limits; at most nine), or the
        finished `tables` of hostinit.area_limits.  Returns the tables (subscripts 1-based, weights)."""
        if tables is None:
            cfg = self.cfg
            tables = area_limits(xlo, xhi, ylo, yhi, cfg.dxo, cfg.dyo, cfg.nxto, cfg.nyto,
                                 fluid="atmos." if getattr(cfg, "atmos", False) else "ocean")
        ii = [np.ascontiguousarray(tables[k], dtype=np.int32) for k in ("i1", "i2", "j1", "j2")]
        ww = [np.ascontiguousarray(tables[k], dtype=np.float64) for k in ("facw", "face", "facs", "facn")]
        n = len(ii[0])
        if any(len(a) != n for a in ii + ww):
            raise ValueError("set_area_tables: the tables differ in length")
        ip = C.POINTER(C.c_int)
        check(self.L.qgcm_hip_areavg_init(self.h, n, *[a.ctypes.data_as(ip) for a in ii], *[_dp(a) for a in ww]))
        return tables

    # -- time averages of the owned rows (avg_ocn_k247 / ocnc_avgout_k247, tavocn / tavout) -----------------
    def enable_po_mean(self, on=True):
        """Start (at zero) or stop the running sum of po: while on, every step adds its po after ocqbdy and before the
        leapfrog averaging (avg_ocn_k247, src/q-gcm.F:1250-1252)."""
        check(self.L.qgcm_hip_poavg_enable(self.h, int(bool(on))))

    def po_mean(self, reset=False):
        """(po_avg * (1/nsum) of the owned rows (nxpo, own_p, nlo), as ocnc_avgout_k247 scales it, nsum); reset=True
        then zeroes sum and count."""
        a = np.zeros((self.cfg.nxpo, self.own_p, self.cfg.nlo), order="F")
        n = C.c_int()
        check(self.L.qgcm_hip_poavg_out(self.h, _dp(a), C.byref(n), int(bool(reset))))
        return a, n.value

    def set_time_mean_params(self, oml=None, **kw):
        """hmoc, ycexp, tsbdy, tnbdy, sb_hflux, nb_hflux of tavocn (defaults from `oml`, a qgcm_hip.OmlConfig).
        Without this call the mixed layer's parameters are used."""
        check(self.L.qgcm_hip_set_tav_params(self.h, C.byref(tav_params(oml, **kw))))

    def set_time_mean_fields(self, fnetoc=None):
        """GLOBAL fnetoc (nxto, nyto) for tavocn without the mixed layer (zero if never given)."""
        f = _cut(fnetoc, self.t_rows)
        check(self.L.qgcm_hip_set_tav_fields(self.h, _dp(f)))

    def tavocn(self):
        """One tavocn contribution from the device state (src/timavge.F:425-619)."""
        check(self.L.qgcm_hip_tavocn(self.h))
        self._done()

    def time_means(self, names=None):
        """(tavout's means (src/timavge.F:667-880) of the owned rows keyed by the reference's names (TAV_LAYOUT),
        nsumoc).  The sums are not changed.  names: the subset to compute and copy (None = all)."""
        c, rp, rt = self.cfg, self.own_p, self.own_t
        shape = dict(p=(c.nxpo, rp), t=(c.nxto, rt), p3=(c.nxpo, rp, c.nlo), u=(c.nxpo, rt), v=(c.nxto, rp))
        return read_means(TAV_LAYOUT, self.L.qgcm_hip_tav_out, TAV_NOUT, self.h, shape, names)

    def reset_time_means(self):
        """tavini: zero the sums and the count."""
        check(self.L.qgcm_hip_tav_reset(self.h))

    # -- periodic ocean dumps (qocdiag_out, ocnc_out) on the subsample rows the handle owns ---------------
    def subsample_rows(self, nsko):
        """(mp0, mp1, mt0, mt1): the p-grid subsample rows [mp0, mp1) and T-grid rows [mt0, mt1) this handle owns."""
        r = [C.c_int() for _ in range(4)]
        check(self.L.qgcm_hip_subsample_rows(self.h, int(nsko), *[C.byref(x) for x in r]))
        return tuple(x.value for x in r)

    def vorticity_budget(self, nsko=1):
        """qocdiag_out's terms from the device state (po, pom, qo, qom, the wekpo given, the entoc on the device):
        dict dqdt, qotjac, qt2dif, qt4dif, qotent of (nlo, jpwk, ipwk) arrays at the points (1+i*nsko, 1+j*nsko) of
        the owned rows.  The reference's dump when called between oml() and qgostep(), or at any time with the mixed
        layer off."""
        n = self.L.qgcm_hip_qocdiag_len(self.h, int(nsko))
        if n < 0:
            check(1)
        out = np.zeros(n)
        check(self.L.qgcm_hip_qocdiag(self.h, int(nsko), _dp(out)))
        return unpack_budget(out, self.cfg.nlo, subsample_count(self.cfg.nxpo, nsko))

    def ocean_dump(self, nsko=1, outfloc=(1, 1, 1, 1, 1, 1, 0)):
        """ocnc_out's subsampled fields (the selected ones) on the owned subsample rows: sst, wekto (jtwk, itwk);
        po, qo (nlo, jpwk, ipwk); h (nlo-1, jpwk, ipwk); tauxo, tauyo (jpwk, ipwk)."""
        c, L = self.cfg, self.L

        def counts():
            mp0, mp1, mt0, mt1 = self.subsample_rows(nsko)
            return dict(p=(mp1 - mp0, subsample_count(c.nxpo, nsko)), t=(mt1 - mt0, subsample_count(c.nxto, nsko)))
        return read_dump(OCNC_FIELDS, L.qgcm_hip_ocnc_sample_len, L.qgcm_hip_ocnc_sample, self.h, nsko, outfloc, c.nlo,
                         counts)

    # -- covariance matrices (covini / covocn and covout's arrays, src/covaria_diag.F) ---------------------
    def enable_covariance(self, nsi=16):
        """covini: allocate and zero the p and T matrices (nvar(nvar+1)/2 entries each, nvar = (nxt/nsi)*(nyt/nsi)),
        the means and the counts; a slab holds the matrix rows of its rank.  nsi = 0 frees them."""
        check(self.L.qgcm_hip_cov_init(self.h, int(nsi), int(self.rank), int(self.nranks)))

    def covariance_size(self):
        """qgcm_hip_cov_size: dict nvar, nmat, k0, k1 (the packed range [k0, k1) the handle holds)."""
        v = [C.c_long() for _ in range(4)]
        check(self.L.qgcm_hip_cov_size(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("nvar", "nmat", "k0", "k1"), (x.value for x in v)))

    def covariance(self, k0=None, count=None):
        """covout's arrays keyed by the reference's names (covpo, avgpo, swtpo, nupo, covto, ...); the matrices as the
        packed entries k0 .. k0+count-1 (default: all the handle holds; 0-based k = i(i+1)/2 + j, j <= i)."""
        sz = self.covariance_size()
        k0 = sz["k0"] if k0 is None else int(k0)
        count = sz["k1"] - k0 if count is None else int(count)
        out = {}
        for w in (0, 1):
            cov, avg, swt, nu = np.zeros(max(count, 0)), np.zeros(sz["nvar"]), C.c_double(), C.c_long()
            check(self.L.qgcm_hip_cov_out(self.h, w, _dp(avg), C.byref(swt), C.byref(nu), k0, count, _dp(cov)))
            out.update(zip(self._COV_NAMES[4 * w:4 * w + 4], (cov, avg, swt.value, nu.value)))
        return out

    def reset_covariance(self):
        """covini again: matrices, means and counts to zero."""
        check(self.L.qgcm_hip_cov_reset(self.h))
