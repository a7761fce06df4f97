"""xforc at refinements above 64 on the device: ndxr = 75, 80 and 128 against the reference's own results
(tests/golden/make_golden_wide_ndxr.py), with the box average in both its forms - k_xf_wekpa and k_xf_wekpa_stage,
chosen by QGCM_HIP_XF_WEKPA_STAGE, which the library reads at xforc's set-up: the variable is set before the models are
made - the staged form at small ndxr against the existing fixtures, the heat half, the slab modes on virtual ranks of
one GPU, atmos_only, the coupled window and the ends of the range.  The parent refuses every set-up here
(`ndxr = 80 outside 1..64`) except the small-ndxr cases, whose variable it does not know."""
import dataclasses
import os

import numpy as np
import pytest

import numpy_atmos_only as na
import numpy_heat as nh
import numpy_xforc as nx
import numpy_xforc_sums as ns
from qgcm_hip import config
from test_wide_ndxr_cpu import GPU_CASES, HEAT_CASE, nstates, restated, tables

pytestmark = pytest.mark.gpu

VAR = "QGCM_HIP_XF_WEKPA_STAGE"
SLAB_CASE = "xf_r80_ny2_ud"  # the xf_r80_ud geometry with nyaooc = 2 (no file: _slab_case)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.array_equal(_bits(a), _bits(b)), "%s: max |diff| %.3e, %d points differ" % (
        what, np.abs(np.asarray(a) - np.asarray(b)).max(), int((_bits(a) != _bits(b)).sum()))


def _configs(g, P, name):
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=name, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"])
    return oc, config.atmos_of(oc, bccoat=P["bccoat"])


def _kw(P):
    return dict(cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tau_udiff=bool(P["tau_udiff"]))


def _models(case):
    """Ocean and atmosphere models with a fixture's dimensions and constants; xforc set up with the tables xforc_setup
    builds itself (hostinit.bcuini: bitwise the reference's at these ndxr, tests/test_wide_ndxr_cpu.py)."""
    from qgcm_hip import AtmosModel, OceanModel, xforc_setup
    g = nx.load(case)
    P = nx.params(g)
    oc, at = _configs(g, P, case)
    o, a = OceanModel(oc), AtmosModel(at)
    try:
        xforc_setup(o, a, **_kw(P))
    except Exception:
        o.close()
        a.close()
        raise
    assert (at.nxta - oc.nxaooc) // 2 + 1 == P["nx1"] and (at.nyta - oc.nyaooc) // 2 + 1 == P["ny1"]
    return g, P, o, a


def _p3(f):
    p = np.zeros(f.shape + (3,), order="F")
    p[:, :, 0] = f
    return p


def _load_state(o, a, g, s):
    a.set_state(po=_p3(g["in%d_pam1" % s]), pom=_p3(g["in%d_pam1" % s]))
    o.set_state(po=_p3(g["in%d_pom1" % s]), pom=_p3(g["in%d_pom1" % s]))


class _env:
    """The variable set (or removed, for None) inside a with block."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(VAR)
        if self.value is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = self.old


_runs = {}


def _run(case, stage):
    """[(R, R2)] per state: xforc_get after one call and after a second one, with the variable set to `stage` before the
    models are made.  Computed once per (case, stage), shared, unchanged."""
    if (case, stage) not in _runs:
        from qgcm_hip import xforc, xforc_get
        with _env(stage):
            g, P, o, a = _models(case)
        try:
            out = []
            for s in range(nstates(case)):
                _load_state(o, a, g, s)
                xforc(o, a)
                R = xforc_get(o, a)
                xforc(o, a)
                out.append((R, xforc_get(o, a)))
            _runs[(case, stage)] = out
        finally:
            o.close()
            a.close()
    return _runs[(case, stage)]


@pytest.mark.parametrize("stage", ["0", "1"])
@pytest.mark.parametrize("case", GPU_CASES)
def test_golden(case, stage):
    """Every pointwise field of every state bitwise the reference's, with either form of the box average; the four line
    integrals within the worst case of reordering a sum of n terms, 2 n 2^-53 sum|terms| dxo (the derived bound of
    tests/test_gpu_xforc.py); a second call gives identical bits.  xf_r128n3_ud is the upper end of the range (xf_r128_ud, nypa = 3, is
    below the four p rows a device handle needs: tests/test_wide_ndxr_cpu.py holds it to the restatement)."""
    g = nx.load(case)
    P = nx.params(g)
    for s, (R, R2) in enumerate(_run(case, stage)):
        N = restated(case, s)
        for f in nx.POINTWISE:
            _same(R[f], g["out%d_%s" % (s, f)], "%s stage %s state %d %s" % (case, stage, s, f))
            _same(R[f], R2[f], f + " (repeat)")
        for f in nx.INTEGRALS:
            ref = float(g["out%d_%s" % (s, f)])
            bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * P["dxo"]
            print("%s stage %s state %d %s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (
                case, stage, s, f, R[f], ref, abs(R[f] - ref), bound))
            assert abs(R[f] - ref) <= bound, (f, R[f], ref, bound)
            assert R[f] == R2[f], f
            if f.endswith("at") or P["cyclic"]:
                assert ref != 0.0


@pytest.mark.parametrize("case", GPU_CASES)
def test_forms_agree(case):
    """wekpa of k_xf_wekpa and of k_xf_wekpa_stage bitwise each other (and so is every other output)."""
    for s, ((A, _), (B, _)) in enumerate(zip(_run(case, "0"), _run(case, "1"))):
        assert np.abs(A["wekpa"]).max() > 0.0
        for f in nx.POINTWISE:
            _same(A[f], B[f], "%s state %d %s, plain against staged" % (case, s, f))


@pytest.mark.parametrize("case", ["xf_odd5_ud", "xf_cpl_small_ud", "xf_wide_ud"])
def test_staged_form_at_small_ndxr(case, monkeypatch):
    """The staged form forced at ndxr = 5, 16 and 4 (xf_wide_ud: nxpa = 301, ten workgroups on a row, the wrap reached from
    the first and from the last): every pointwise field bitwise the existing fixtures."""
    from qgcm_hip import xforc, xforc_get
    from test_gpu_xforc import _load_state as load, _models as models
    monkeypatch.setenv(VAR, "1")
    g, P, o, a = models(case)
    try:
        for s in range(2):
            load(o, a, g, s)
            xforc(o, a)
            R = xforc_get(o, a)
            for f in nx.POINTWISE:
                _same(R[f], g["out%d_%s" % (s, f)], "%s state %d %s" % (case, s, f))
    finally:
        o.close()
        a.close()


def test_heat_chain():
    """heat_r80 call by call at the bars of tests/test_gpu_heat.py: every xforc from the reference's state before the
    cycle - fnetoc bitwise, fnetat bitwise over land and above the ocean within 2 ndxr^2 2^-53 sum|terms| of the cell
    plus one ulp of the value, the four monitors within 2 n 2^-53 sum|terms| - and every aml re-fed with the reference's
    inputs: the state and entat bitwise."""
    from qgcm_hip import xforc, xforc_heat_get
    from test_gpu_heat import STATE, _models as models, _state_before
    g, P, o, a = models(HEAT_CASE)
    R = nh.restated(HEAT_CASE)
    try:
        for c in range(P["K"]):
            a.aml_set_state(**_state_before(g, P, c, 0))
            xforc(o, a)
            H = xforc_heat_get(o, a)
            N = R[("x", c)]
            tag = "%s xforc %d " % (HEAT_CASE, c)
            _same(H["fnetoc"], g["x%d_fnetoc" % c], tag + "fnetoc")
            ref, oc = g["x%d_fnetat" % c], N["ocean"]
            _same(H["fnetat"][~oc], ref[~oc], tag + "fnetat over land")
            blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
            assert oc[blk].all() and oc.sum() == N["cell_abs"].size
            bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"] + np.spacing(np.abs(ref[blk]))
            diff = np.abs(H["fnetat"][blk] - ref[blk])
            print("%sfnetat above the ocean: max |diff| %.3e, largest |diff| / bound %.3f" % (tag, diff.max(), (diff / bound).max()))
            assert np.all(diff <= bound), (tag, diff.max(), (diff / bound).max())
            for f in nh.HEAT_SCALARS:
                r = float(g["x%d_%s" % (c, f)])
                b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
                print("%s%s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (tag, f, H[f], r, abs(H[f] - r), b))
                assert abs(H[f] - r) <= b, (tag, f, H[f], r, b)
            a.set_time_mean_fields(fnetat=g["x%d_fnetat" % c])
            a.set_atm_monitor_fields(wekta=g["x%d_wekta" % c], uekat=g["x%d_uekat" % c], vekat=g["x%d_vekat" % c])
            for s in range(P["nstr"]):
                a.aml_set_state(**_state_before(g, P, c, s))
                a.aml()
                for f, v in zip(STATE, a.aml_get_state()):
                    _same(v, g["a%d%d_%s" % (c, s, f)], "aml %d.%d %s" % (c, s, f))
                _same(a.aml_get_diag()[0], g["a%d%d_entat" % (c, s)], "aml %d.%d entat" % (c, s))
    finally:
        o.close()
        a.close()


# ---- slabs --------------------------------------------------------------------------------------------------------------
def _slab_case():
    """The xf_r80_ud geometry with nyaooc = 2 (nypo = 161: on 2 and on 3 ranks a seam falls inside an atmosphere cell) as an
    entry of numpy_xforc's fixture cache, so that the slab tests' own helpers (tests/test_gpu_slab_udiff.py,
    tests/test_gpu_xforc_sums.py) take it by name: xf_r80_ud's constants and atmospheric pressures, a smooth ocean
    pressure of the fixtures' magnitude, bcuini's tables.  No outputs: the oracle is the whole-domain device call."""
    if SLAB_CASE not in nx._cache:
        g = nx.load("xf_r80_ud")
        nxta, nyta, nxaooc, _, ndxr = (int(v) for v in g["c_dims"])
        d = {k: v for k, v in g.items() if k.startswith("c_") or k.endswith("_pam1")}
        d["c_dims"] = np.array((nxta, nyta, nxaooc, 2, ndxr), dtype=np.int64)
        d["c_ny1"] = np.int64(1 + (nyta - 2) // 2)
        x = np.arange(nxaooc * ndxr + 1)[:, None] / float(nxaooc * ndxr)
        y = np.arange(2 * ndxr + 1)[None, :] / float(2 * ndxr)
        for s in range(2):
            d["in%d_pom1" % s] = np.asfortranarray(5.0 * np.cos(np.pi * y) * (1.0 + 0.0 * x) + (1.5 + s) * np.sin(np.pi * (2 + s) * x + 0.4)
                                                   * np.cos(np.pi * (3 - s) * y + 1.1 + s))
        d.update({"tab_" + t: v for t, v in tables("xf_r80_ud").items()})
        nx._cache[SLAB_CASE] = d
    return SLAB_CASE


@pytest.fixture
def _poison(monkeypatch):
    monkeypatch.setenv("QGCM_HIP_XF_POISON", "1")  # NaN bytes in the fine arrays and the assembled pressure


@pytest.mark.parametrize("bands", [False, True], ids=["replicated", "banded"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs_gather(nranks, bands, _poison):
    """ndxr = 80 on 2 and 3 virtual ranks with udiff_gather = True, replicated and with bands = True: the second of two
    xforc() calls is bitwise the whole-domain device call (tests/test_gpu_slab_udiff.py:_check_momentum)."""
    import test_gpu_slab_coupled as tsc
    import test_gpu_slab_udiff as tud
    case = _slab_case()
    ref = tud._whole_ud(case)[1]
    g, P, so, reps = tud._slabs_ud(case, nranks, bands)
    try:
        M = tud._two_calls(so, reps, g)
        tud._check_momentum("%s, %d ranks, bands %s," % (case, nranks, bands), so, M, ref)
    finally:
        tsc._close(so, reps)
    assert not np.array_equal(ref["wekpa"], tud._whole_ud(case)[0]["wekpa"])


@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs_sums(nranks, _poison):
    """... and with udiff_sums = True: bitwise where no seam cuts a uekat line or a wekpa box, within DESIGN 6r's derived
    bounds where one does (tests/test_gpu_xforc_sums.py:_check_momentum; k_xf_sums_wekpa keeps its plain loops)."""
    import test_gpu_slab_coupled as tsc
    import test_gpu_slab_udiff as tud
    import test_gpu_xforc_sums as tgs
    from qgcm_hip.slab import partition
    case = _slab_case()
    ref = tud._whole_ud(case)[1]
    g, P, so, reps = tgs._slabs_sums(case, nranks)
    try:
        M = tud._two_calls(so, reps, g)
        B = tgs._bounds(P, partition(so.cfg.nypo, nranks), ns.fine(case, 1))
        tgs._check_momentum("%s, %d ranks," % (case, nranks), so, M, ref, B)
    finally:
        tsc._close(so, reps)


# ---- atmos_only -----------------------------------------------------------------------------------------------------------
def test_atmos_only():
    """xforc_setup(None, atmos, ndxr=80, ...) with heat_r80's SST prescribed, against the numpy restatements at the bars
    of tests/test_gpu_atmos_only.py: the six momentum fields bitwise, txisat / txinat within 2 n 2^-53 sum|terms| dxo;
    fnetat bitwise over land and above the sea within 2 ndxr^2 2^-53 sum|terms| plus one spacing of the value; slhfav,
    oradav, arlaav within 2 n 2^-53 sum|terms|; arocav = 0 exactly; a second call gives identical bits."""
    from qgcm_hip import AtmosModel, xforc, xforc_get, xforc_setup, xforc_sst_get, xforc_sst_setup
    from test_gpu_atmos_only import _aml_cfg, _heat_cfg
    g = nh.load(HEAT_CASE)
    P = nh.params(g)
    assert P["ndxr"] == 80
    oc = dataclasses.replace(config.preset("cpl_tiny"), name=HEAT_CASE, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"],
                             nyaooc=P["nyaooc"], ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    at = config.atmos_of(oc, bccoat=P["bccoat"], gpat=(P["gpat1"], P["gpat2"]))
    Pm = dict(P, tau_udiff=0, cyclic=0)
    from qgcm_hip import hostinit
    pom1 = np.zeros((P["nxaooc"] * P["ndxr"] + 1, P["nyaooc"] * P["ndxr"] + 1), order="F")
    M = nx.xforc(g["in_pam"][:, :, 0], pom1, hostinit.bcuini(P["ndxr"], P["bccoat"], P["dxa"]), Pm)
    N = na.heat_sst(g["in_astm"], g["in_hmixam"], g["in_sstm"], g["in_pam"], g["in_dtopat"], g["t_fsa"], nh.tables_of(g, P), P)
    a = AtmosModel(at)
    try:
        xforc_setup(None, a, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], ndxr=80,
                    nxaooc=P["nxaooc"], nyaooc=P["nyaooc"])
        assert a.xforc_origin == (P["nx1"], P["ny1"])
        a.aml_init(_aml_cfg(P), xc1ast=g["in_xc1ast"], dtopat=g["in_dtopat"])
        xforc_sst_setup(a, oc, _heat_cfg(P), g["in_sstm"], fsa=g["t_fsa"], coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
        a.set_state(po=g["in_pa"], pom=g["in_pam"])
        a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
        xforc(None, a)
        R, H = xforc_get(None, a), xforc_sst_get(a)
        xforc(None, a)
        R2, H2 = xforc_get(None, a), xforc_sst_get(a)
        for f in na.MOM_FIELDS:
            _same(R[f], M[f], "atmos_only " + f)
            _same(R[f], R2[f], f + " (repeat)")
            assert np.abs(M[f]).max() > 0.0
        # (the coupled reference's momentum fields of the same pam, where the shear term cannot reach them: uekat, vekat and
        #  wekta of heat_r80 were formed without tau_udiff)
        for f in ("uekat", "vekat", "wekta"):
            _same(R[f], g["x0_" + f], "atmos_only %s against the coupled reference" % f)
        for f in na.MOM_INTEGRALS:
            bound = 2.0 * M["n_" + f] * 2.0 ** -53 * M["abs_" + f] * P["dxo"]
            assert abs(R[f] - M[f]) <= bound and R[f] == R2[f] and M[f] != 0.0, (f, R[f], M[f], bound)
        ref, sea = N["fnetat"], N["ocean"]
        _same(H["fnetat"][~sea], ref[~sea], "fnetat over land")
        blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
        bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"] + np.spacing(np.abs(ref[blk]))
        diff = np.abs(H["fnetat"][blk] - ref[blk])
        print("fnetat above the sea: max |diff| %.3e, largest |diff| / bound %.3f" % (diff.max(), (diff / bound).max()))
        assert np.all(diff <= bound) and np.all(H["fnetat"][sea] != 0.0)
        _same(H["fnetat"], H2["fnetat"], "fnetat (repeat)")
        for f in na.SST_SCALARS:
            b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
            print("%s: device %.17e restated %.17e |diff| %.3e bound %.3e" % (f, H[f], N[f], abs(H[f] - N[f]), b))
            assert abs(H[f] - N[f]) <= b and H[f] == H2[f], (f, H[f], N[f], b)
        assert H["arocav"] == 0.0 and H["arlaav"] != 0.0
    finally:
        a.close()


# ---- the coupled window ---------------------------------------------------------------------------------------------------
def _coupled(share):
    from qgcm_hip import share_gpu
    g, P, o, a = _models("xf_r80_ud")
    pa, po = _p3(g["in0_pam1"]), _p3(g["in0_pom1"])
    o.set_p(po, po)
    a.set_p(pa, pa)
    zo, za = np.zeros((o.cfg.nxpo, o.cfg.nypo), order="F"), np.zeros((a.cfg.nxpa, a.cfg.nypa), order="F")
    o.set_forcing(zo, zo.copy(order="F"), np.zeros(o.cfg.nlo - 1))
    a.set_forcing(za, za.copy(order="F"), np.zeros(a.cfg.nla - 1), 0.0, 0.0, np.zeros(a.cfg.nla - 1), np.zeros(a.cfg.nla - 1))
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("share", [False, True])
def test_coupled_window(share):
    """The xf_r80_ud grid, nstr = 3: a window of two ocean steps (six atmospheric ones) with xforc=True is bitwise the
    explicit sequence xforc(); ocean.steps(1); atmos.steps(3) and differs from the window with the forcing held; the same
    with a CU range on both handles."""
    from qgcm_hip import coupled_steps, xforc
    nstr, n = 3, 6
    res = {}
    for mode in ("window", "explicit", "held"):
        o, a = _coupled(share)
        try:
            if mode == "explicit":
                for nt in range(1, n + 1, nstr):
                    xforc(o, a)
                    o.steps(1, s0=(nt - 1) // nstr + 1)
                    a.steps(nstr, s0=nt)
            else:
                coupled_steps(o, a, 1, n, nstr, xforc=(mode == "window"))
            o.sync()
            a.sync()
            res[mode] = [np.array(x) for x in o.get_state()] + [np.array(x) for x in a.get_state()]
            assert all(np.isfinite(x).all() for x in res[mode])
        finally:
            o.close()
            a.close()
    for k, (x, y) in enumerate(zip(res["window"], res["explicit"])):
        _same(x, y, "window against explicit, field %d" % k)
    assert not np.array_equal(res["window"][0], res["held"][0])  # po: the atmosphere drives the ocean
    assert not np.array_equal(res["window"][4], res["held"][4])  # pa: and is driven by its own stress


# ---- the ends of the range --------------------------------------------------------------------------------------------------
def test_refusals():
    """ndxr = 129 is refused with the range in the message, and so is a fine grid whose padded arrays pass 2^31 - 1
    elements; the refused calls change nothing: the standing set-up at ndxr = 128 gives the bits it gave before."""
    from qgcm_hip import AtmosModel, QgcmHipError, xforc, xforc_get, xforc_setup
    g, P, o, a = _models("xf_r128n3_ud")
    assert P["ndxr"] == 128
    b = c = None
    try:
        _load_state(o, a, g, 0)
        xforc(o, a)
        before = xforc_get(o, a)
        _same(before["wekpa"], g["out0_wekpa"], "wekpa at ndxr = 128")
        kw = dict(_kw(P), tau_udiff=False)
        b = AtmosModel(a.cfg)
        with pytest.raises(QgcmHipError, match=r"ndxr = 129 outside 1\.\.128"):
            xforc_setup(None, b, ndxr=129, nxaooc=1, nyaooc=1, **kw)
        with pytest.raises(QgcmHipError, match=r"ndxr = 129 outside 1\.\.128"):
            xforc_setup(None, a, ndxr=129, nxaooc=1, nyaooc=1, **kw)
        # 320 x 480 cells at ndxr = 128: 40976 x 61441 elements (below the launch limits of 10^6 columns and 65535 rows)
        big = dataclasses.replace(a.cfg, name="atm_big", nxta=320, nyta=480)
        c = AtmosModel(big)
        with pytest.raises(QgcmHipError, match=r"padded arrays of 40976 x 61441 elements pass 2\^31 - 1"):
            xforc_setup(None, c, ndxr=128, nxaooc=1, nyaooc=1, **kw)
        xforc(o, a)
        after = xforc_get(o, a)
        for f in nx.POINTWISE + nx.INTEGRALS:
            assert np.array_equal(np.asarray(before[f]), np.asarray(after[f])), f
    finally:
        for m in (b, c, o, a):
            if m is not None:
                m.close()
