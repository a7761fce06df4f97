"""The atmospheric mixed layer (qgcm_hip_aml) and the heat half of xforc on the device against the
reference's own results (tests/golden/heat_*.npz) and against themselves: golden comparison call by call, the chained
cycles, destinations, the coupled window, the averaging and the refusals."""
import dataclasses

import numpy as np
import pytest

import numpy_heat as nh
from common import atm_apply, load_golden, relerr
from qgcm_hip import config

pytestmark = pytest.mark.gpu

STATE = ("ast", "astm", "hmixa", "hmixam")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.array_equal(_bits(a), _bits(b)), "%s: max |diff| %.3e, %d points differ" % (
        what, np.abs(np.asarray(a) - np.asarray(b)).max(), int((_bits(a) != _bits(b)).sum()))


def _aml_cfg(P):
    return config.AmlConfig(tat=(P["tat1"], P["tat2"]), aface=(P["aface1"], P["aface2"]), bface=P["bface"],
                            cface=P["cface"], dface=P["dface"], hmat=P["hmat"], hmamin=P["hmamin"], hmadmp=P["hmadmp"],
                            xcexp=P["xcexp"], at2d=P["at2d"], at4d=P["at4d"], ahmd=P["ahmd"], rhoat=1.0,
                            cpat=1.0 / P["rrcpat"])


def _heat_cfg(P):
    return config.HeatConfig(**{k: P[k] for k in ("D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup", "C1down",
                                                  "xlamda", "fspco")})


def _models(case, heat=True):
    """Ocean and atmosphere models with a fixture's dimensions and constants: xforc's momentum half, both mixed layers
    and (heat) the heat half set up from the fixture's own tables; the fixture's pressures and sstm loaded."""
    from qgcm_hip import AtmosModel, OceanModel, oml_preset, xforc_heat_setup, xforc_setup
    g = nh.load(case)
    P = nh.params(g)
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    at = config.atmos_of(oc, bccoat=P["bccoat"], gpat=(P["gpat1"], P["gpat2"]))
    o, a = OceanModel(oc), AtmosModel(at)
    xforc_setup(o, a, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tau_udiff=False)
    o.oml_init(oml_preset(oc))
    a.aml_init(_aml_cfg(P), xc1ast=g["in_xc1ast"], dtopat=g["in_dtopat"])
    if heat:
        xforc_heat_setup(o, a, _heat_cfg(P), fsa=g["t_fsa"], fso=g["t_fso"],
                         coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    a.set_state(po=g["in_pa"], pom=g["in_pam"])
    pom = np.zeros(g["in_pom"].shape + (3,), order="F")
    pom[:, :, 0] = g["in_pom"]
    o.set_state(po=pom, pom=pom)
    o.oml_set_state(sst=g["in_sstm"], sstm=g["in_sstm"])
    return g, P, o, a


def _state_before(g, P, c, s):
    """The reference's mixed-layer state before aml s of cycle c."""
    k = c * P["nstr"] + s
    if k == 0:
        return {f: g["in_" + f] for f in STATE}
    c0, s0 = divmod(k - 1, P["nstr"])
    return {f: g["a%d%d_%s" % (c0, s0, f)] for f in STATE}


@pytest.mark.parametrize("case", nh.CASES)
def test_aml_golden(case):
    """Every recorded call re-fed with the reference's own inputs: ast, astm, hmixa, hmixam, entat bitwise; cfraat
    exact; xan(1), centat and the line sums within the worst case of reordering a sum of n terms, 2 n 2^-53 sum|terms|
    (dxa dya or dxa); a repeated call from the same state gives identical bits."""
    g, P, o, a = _models(case, heat=False)
    R = nh.restated(case)
    scale = dict(xan=P["dxa"] * P["dya"], centat=P["dxa"] * P["dya"], enisat=P["dxa"], eninat=P["dxa"])
    try:
        for c in range(P["K"]):
            a.set_time_mean_fields(fnetat=g["x%d_fnetat" % c])
            a.set_atm_monitor_fields(wekta=g["x%d_wekta" % c], uekat=g["x%d_uekat" % c], vekat=g["x%d_vekat" % c])
            for s in range(P["nstr"]):
                runs = []
                for rep in range(2):
                    a.aml_set_state(**_state_before(g, P, c, s))
                    a.aml()
                    runs.append((a.aml_get_state(), a.aml_get_diag()))
                (st, (entat, d)), (st2, (entat2, d2)) = runs
                tag = "%s aml %d.%d " % (case, c, s)
                for f, v, v2 in zip(STATE, st, st2):
                    _same(v, g["a%d%d_%s" % (c, s, f)], tag + f)
                    _same(v, v2, tag + f + " (repeat)")
                _same(entat, g["a%d%d_entat" % (c, s)], tag + "entat")
                _same(entat, entat2, tag + "entat (repeat)")
                assert d == d2, tag
                assert d["cfraat"] == float(g["a%d%d_cfraat" % (c, s)]), tag
                N = R[("a", c, s)]
                for f in nh.AML_SUMS:
                    ref = float(g["a%d%d_%s" % (c, s, f)])
                    bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * scale[f]
                    print("%s%s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (tag, f, d[f], ref, abs(d[f] - ref), bound))
                    assert abs(d[f] - ref) <= bound, (tag, f, d[f], ref, bound)
    finally:
        o.close()
        a.close()


@pytest.mark.parametrize("case", nh.CASES)
def test_heat_golden(case):
    """xforc from the reference's state before every cycle: fnetoc bitwise; fnetat bitwise over land and, above the
    ocean, within 2 n 2^-53 sum|terms| with n = ndxr^2 over the cell's flux terms, plus one ulp of the value itself: the
    pointwise tail (src/xfosubs.F:835-842) is added to the cell's sum afterwards, so two sums that differ within the
    bound are each rounded once more at the magnitude of the complete value, which may be larger than the sum's.  The
    four monitors within the bound with their own n; a second call gives identical bits."""
    from qgcm_hip import xforc, xforc_heat_get
    g, P, o, a = _models(case)
    R = nh.restated(case)
    try:
        for c in range(P["K"]):
            a.aml_set_state(**_state_before(g, P, c, 0))
            xforc(o, a)
            H = xforc_heat_get(o, a)
            xforc(o, a)
            H2 = xforc_heat_get(o, a)
            N = R[("x", c)]
            tag = "%s xforc %d " % (case, c)
            _same(H["fnetoc"], g["x%d_fnetoc" % c], tag + "fnetoc")
            ref, oc = g["x%d_fnetat" % c], N["ocean"]
            _same(H["fnetat"][~oc], ref[~oc], tag + "fnetat over land")
            # the block above the ocean as (nxaooc, nyaooc), cell (ca, cb) against its own cell_abs[ca, cb] (a boolean
            # mask would flatten it row by row, which no Fortran-order reshape undoes)
            blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
            assert oc[blk].all() and oc.sum() == N["cell_abs"].size
            bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"] + np.spacing(np.abs(ref[blk]))
            diff = np.abs(H["fnetat"][blk] - ref[blk])
            print("%sfnetat above the ocean: max |diff| %.3e, largest |diff| / bound %.3f" % (tag, diff.max(), (diff / bound).max()))
            assert np.all(diff <= bound), (tag, diff.max(), (diff / bound).max())
            assert np.all(H["fnetat"][oc] != 0.0)
            for f in ("fnetoc", "fnetat"):
                _same(H[f], H2[f], tag + f + " (repeat)")
            for f in nh.HEAT_SCALARS:
                r = float(g["x%d_%s" % (c, f)])
                b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
                print("%s%s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (tag, f, H[f], r, abs(H[f] - r), b))
                assert abs(H[f] - r) <= b, (tag, f, H[f], r, b)
                assert H[f] == H2[f], tag + f
    finally:
        o.close()
        a.close()


@pytest.mark.parametrize("case", nh.CASES)
def test_chained(case):
    """The fixture's K cycles on the device with nothing re-fed (xforc(); aml() x nstr): after the last cycle ast,
    hmixa, entat and fnetoc agree with the reference to 1e-13 of their maximum."""
    from qgcm_hip import xforc, xforc_heat_get
    g, P, o, a = _models(case)
    try:
        a.aml_set_state(**{f: g["in_" + f] for f in STATE})
        for c in range(P["K"]):
            xforc(o, a)
            if c == P["K"] - 1:
                fnetoc = xforc_heat_get(o, a)["fnetoc"]
            for s in range(P["nstr"]):
                a.aml()
        ast, _, hmixa, _ = a.aml_get_state()
        entat, _ = a.aml_get_diag()
        last = "a%d%d_" % (P["K"] - 1, P["nstr"] - 1)
        errs = dict(ast=relerr(ast, g[last + "ast"]), hmixa=relerr(hmixa, g[last + "hmixa"]),
                    entat=relerr(entat, g[last + "entat"]), fnetoc=relerr(fnetoc, g["x%d_fnetoc" % (P["K"] - 1)]))
        print(case, errs)
        for k, e in errs.items():
            assert e < 1e-13, (case, k, e)
    finally:
        o.close()
        a.close()


def test_destinations():
    """After xforc() + aml() the consumers read the stepped fields without a setter: atm_valids' ast extrema, tavatm
    with fnetat never set by hand, the mixed layer's fnetoc and entat / xan(1) / enisat(1) where qgastep reads them."""
    from qgcm_hip import xforc, xforc_heat_get
    g, P, o, a = _models("heat_cpl_tiny")
    try:
        a.aml_set_state(**{f: g["in_" + f] for f in STATE})
        xforc(o, a)
        H = xforc_heat_get(o, a)
        a.aml()
        ast, astm, hmixa, hmixam = a.aml_get_state()
        entat, d = a.aml_get_diag()
        assert d["xan"] != 0.0 and d["enisat"] != 0.0 and np.abs(entat).max() > 0.0
        # atm_valids: entries 4, 5 = min, max of ast
        _, av = a.atm_valids()
        assert av[4] == ast.min() and av[5] == ast.max() and av[4] < av[5]
        # the periodic dump reads the stepped ast and hmixa
        dump = a.atmos_dump(nska=1)
        _same(np.asarray(dump["ast"]).T, ast, "dump ast")
        _same(np.asarray(dump["hmixa"]).T, hmixa, "dump hmixa")
        # tavatm: fnetat was never set by hand; one contribution's mean of fnetat is the field xforc wrote
        a.set_atm_monitor_params(ocean=o.cfg, hmat=P["hmat"])
        a.tavatm()
        tm = a.time_means(names=("fmatav", "astav"))
        _same(tm["fmatav"], H["fnetat"], "fmatav")
        _same(tm["astav"], ast, "astav")
        # the mixed layer's own fnetoc: overwritten through oml_set_forcing, restored by the next xforc()
        o.oml_set_forcing(fnetoc=np.zeros((o.cfg.nxto, o.cfg.nyto), order="F"))
        assert not xforc_heat_get(o, a)["fnetoc"].any()
        a.aml_set_state(**{f: g["in_" + f] for f in STATE})
        xforc(o, a)
        _same(xforc_heat_get(o, a)["fnetoc"], H["fnetoc"], "fnetoc restored")
        # entat / xan(1) / enisat(1): overwritten through set_forcing / set_cyc_forcing, restored by the next aml()
        a.set_forcing(entat=np.zeros_like(entat), xan=np.array([1.0, 2.0]), enis=np.array([3.0, 4.0]), enin=np.array([5.0, 6.0]))
        e0, d0 = a.aml_get_diag()
        assert not e0.any() and d0["xan_v"] == (1.0, 2.0) and d0["enisat_v"] == (3.0, 4.0) and d0["eninat_v"] == (5.0, 6.0)
        a.aml()
        e1, d1 = a.aml_get_diag()
        _same(e1, entat, "entat restored")
        for k in ("xan", "enisat", "eninat", "cfraat", "centat"):
            assert d1[k] == d[k], k
        # ... and aml touches no entry of xan, enisat, eninat beyond the first
        assert d1["xan_v"] == (d["xan"], 2.0) and d1["enisat_v"] == (d["enisat"], 4.0) and d1["eninat_v"] == (d["eninat"], 6.0)
    finally:
        o.close()
        a.close()


def _cpl_tiny(share, mixed):
    """cpl_tiny as tests/test_gpu_xforc.py sets it up; mixed: both mixed layers and the heat half on, with the
    constants and the smooth mixed-layer state of the heat_cpl_tiny fixture (same dimensions)."""
    from qgcm_hip import AtmosModel, OceanModel, oml_preset, share_gpu, xforc_heat_setup, xforc_setup
    g = load_golden("cpl_tiny")
    h = nh.load("heat_cpl_tiny")
    P = nh.params(h)
    oc, at = config.preset("cpl_tiny"), config.atmos_preset("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(g["in_po"], g["in_pom"])
    o.set_forcing(g["in_wekpo"], np.zeros_like(g["in_wekpo"]), np.zeros(oc.nlo - 1))
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    o.oml_init(oml_preset(oc))
    sst = 22.0 + 0.5 * h["in_sstm"]  # (above toc(1) = 15: a stable ocean mixed layer, no convective reset of sst)
    o.oml_set_state(sst=sst, sstm=sst)
    if mixed:
        r = at.dxa / (P["ndxr"] * P["dxo"])
        am = dataclasses.replace(_aml_cfg(P), at2d=P["at2d"] * r * r, at4d=P["at4d"] * r ** 4, ahmd=P["ahmd"] * r * r)
        a.aml_init(am, xc1ast=h["in_xc1ast"], dtopat=h["in_dtopat"])
        a.aml_set_state(**{k: h["in_" + k] for k in STATE})
        xforc_heat_setup(o, a, _heat_cfg(P))
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("share", [False, True])
def test_coupled_window(share):
    """cpl_tiny, nstr = 3, 7 atmospheric steps, both mixed layers on: the window is bitwise the explicit sequence
    xforc(); ocean.steps(1); (aml(); atmos steps) ... and differs from the same window without aml / the heat half, in
    pa and in sst; the same with a CU range on both handles."""
    from qgcm_hip import coupled_steps, xforc
    nstr, n = 3, 7
    res = {}
    for mode in ("window", "explicit", "plain"):
        o, a = _cpl_tiny(share, mode != "plain")
        try:
            if mode == "explicit":
                nt = 1
                while nt <= n:
                    xforc(o, a)
                    o.steps(1, s0=(nt - 1) // nstr + 1)
                    for k in range(min(nstr, n - nt + 1)):
                        a.aml()
                        a.qgastep()
                        a.atinvq()
                        a.atqzbd()
                        if (nt - 1) % 100 == 0:
                            a.lf_average()
                        nt += 1
            else:
                coupled_steps(o, a, 1, n, nstr, xforc=True)
            o.sync()
            a.sync()
            res[mode] = ([np.array(x) for x in o.get_state()] + [np.array(x) for x in a.get_state()]
                         + [np.array(x) for x in o.oml_get_state()])
            if mode != "plain":
                res[mode] += [np.array(x) for x in a.aml_get_state()] + [a.aml_get_diag()[0]]
            assert all(np.isfinite(x).all() for x in res[mode])
        finally:
            o.close()
            a.close()
    assert len(res["window"]) == len(res["explicit"]) == 15
    for k, (x, y) in enumerate(zip(res["window"], res["explicit"])):
        _same(x, y, "window vs explicit, field %d" % k)
    assert not np.array_equal(res["window"][4], res["plain"][4])  # pa: entat drives the atmosphere
    assert not np.array_equal(res["window"][8], res["plain"][8])  # sst: fnetoc drives the ocean's mixed layer


def test_averaging():
    """Two atmospheres from one state: steps(1, s0=101) averages (mod(nt-1,100) == 0), steps(1, s0=102) does not.
    The averaged ast, hmixa are 0.5*(new + lagged) of the other, bitwise; the lagged levels are equal."""
    out = []
    for s0 in (101, 102):
        o, a = _cpl_tiny(False, True)
        try:
            a.steps(1, s0=s0)
            a.sync()
            out.append(a.aml_get_state() + a.get_state())
        finally:
            o.close()
            a.close()
    A, B = out
    _same(A[0], 0.5 * (B[0] + B[1]), "ast")
    _same(A[2], 0.5 * (B[2] + B[3]), "hmixa")
    _same(A[1], B[1], "astm")
    _same(A[3], B[3], "hmixam")
    assert not np.array_equal(A[0], B[0])
    _same(A[4], 0.5 * (B[4] + B[5]), "pa")  # (the pressures are averaged by the same step)


def test_refusals():
    """Every refusal names its reason and changes no state: afterwards the standing set-up gives the same bits."""
    from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, oml_preset, xforc, xforc_heat_get, xforc_heat_setup, xforc_setup
    from qgcm_hip.slab import HipSlab, global_consts, partition
    import ctypes
    from qgcm_hip.lib import AmlParams, XforcHeatParams, check
    g, P, o, a = _models("heat_cpl_tiny")
    extra = []
    try:
        st0 = {f: g["in_" + f] for f in STATE}
        a.aml_set_state(**st0)
        xforc(o, a)
        a.aml()
        before = (xforc_heat_get(o, a), a.aml_get_state(), a.aml_get_diag())
        hc, kw = _heat_cfg(P), dict(fsa=g["t_fsa"], fso=g["t_fso"])
        mkw = dict(cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"])
        # an atmosphere that was never set up: before xforc_init, then before aml_init
        b = AtmosModel(a.cfg)
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml_init has not been called"):
            b.aml()
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml_init has not been called"):
            b.aml_get_state()
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_init has not been called"):
            xforc_heat_setup(o, b, hc, hmadmp=P["hmadmp"], hmat=P["hmat"], **kw)
        o2 = OceanModel(o.cfg)
        extra.append(o2)
        xforc_setup(o2, b, **mkw)
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml_init has not been called"):
            xforc_heat_setup(o2, b, hc, hmadmp=P["hmadmp"], hmat=P["hmat"], **kw)
        # an ocean without its mixed layer
        b.aml_init(_aml_cfg(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_oml_init has not been called"):
            xforc_heat_setup(o2, b, hc, **kw)
        # no ocean; a handle other than the one of xforc_init
        with pytest.raises(QgcmHipError, match=r"qgcm_hip_xforc_heat_init: the heat half needs an ocean \(oc = NULL\)"):
            xforc_heat_setup(None, a, hc, **kw)
        with pytest.raises(QgcmHipError, match=r"qgcm_hip_xforc_heat_get: the heat half needs an ocean \(oc = NULL\)"):
            check(a.L.qgcm_hip_xforc_heat_get(None, a.h, None, None, None))
        with pytest.raises(QgcmHipError, match="not the one qgcm_hip_xforc_init was called with"):
            xforc_heat_setup(o2, a, hc, **kw)
        # an ocean handle where the atmosphere is needed; a y-slab handle
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml_init: the handle is an ocean"):
            check(o.L.qgcm_hip_aml_init(o.h, ctypes.byref(AmlParams())))
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml: the handle is an ocean"):
            AtmosModel.aml(o)
        with pytest.raises(QgcmHipError, match="the second handle is an ocean"):
            check(o.L.qgcm_hip_xforc_heat_init(o.h, o.h, ctypes.byref(XforcHeatParams())))
        (g0, g1), _ = partition(o.cfg.nypo, 2)
        sl = HipSlab(o.cfg, global_consts(o.cfg, o.helmholtz), g0, g1, 0, 2)
        extra.append(sl)
        with pytest.raises(QgcmHipError, match="y-slab"):
            xforc_heat_setup(sl, a, hc, **kw)
        # the refused calls changed nothing
        a.aml_set_state(**st0)
        xforc(o, a)
        a.aml()
        after = (xforc_heat_get(o, a), a.aml_get_state(), a.aml_get_diag())
        for f in ("fnetoc", "fnetat"):
            _same(after[0][f], before[0][f], f)
        assert all(after[0][f] == before[0][f] for f in nh.HEAT_SCALARS)
        for x, y in zip(after[1], before[1]):
            _same(x, y, "state")
        _same(after[2][0], before[2][0], "entat")
        assert after[2][1] == before[2][1]
    finally:
        for m in extra + [o, a]:
            m.close()
