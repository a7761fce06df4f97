"""Atmosphere-only runs on the device: xforc without an ocean - the momentum half with oc = NULL and the
heat half from a prescribed, held SST (qgcm_hip_xforc_sst_*) - against the reference built with -Datmos_only
(tests/golden/ato_*.npz) and against itself: golden comparison, the chained cycles, the atmos_only window of
coupled_steps, a replaced SST and the refusals."""
import dataclasses

import numpy as np
import pytest

import numpy_atmos_only as na
import numpy_xforc as nx
from common import relerr
from qgcm_hip import config

pytestmark = pytest.mark.gpu


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


def _configs(case):
    """The fixture, its constants, the OceanConfig that carries the geometry of the sea (no OceanModel is made of it)
    and the atmosphere's configuration."""
    g = na.load(case)
    P = na.params(g)
    oc = dataclasses.replace(config.preset("cpl_tiny"), name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"],
                             nyaooc=P["nyaooc"], ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    at = config.atmos_of(oc, bccoat=P["bccoat"], gpat=(P["gpat1"], P["gpat2"]))
    return g, P, oc, at


def _mom_kw(P):
    return dict(cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], ndxr=P["ndxr"],
                nxaooc=P["nxaooc"], nyaooc=P["nyaooc"])


def _sst_kw(g):
    return dict(fsa=g["t_fsa"], coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})


def _atmos(case, aml=True, sst=True):
    """An atmosphere with a fixture's dimensions and constants and no ocean: xforc's momentum half set up with
    oc = NULL, the mixed layer (aml) and the heat half from the fixture's SST (sst); the fixture's pressures loaded."""
    from qgcm_hip import AtmosModel, xforc_setup, xforc_sst_setup
    g, P, oc, at = _configs(case)
    a = AtmosModel(at)
    try:
        xforc_setup(None, a, tables=nx.tables(g), **_mom_kw(P))  # (the reference's own tables: bitwise at odd ndxr too)
        assert a.xforc_origin == (P["nx1"], P["ny1"])
        if aml:
            a.aml_init(_aml_cfg(P), xc1ast=g["in_xc1ast"], dtopat=g["in_dtopat"])
        if sst:
            xforc_sst_setup(a, oc, _heat_cfg(P), g["in_sstm"], **_sst_kw(g))
        a.set_state(po=g["in_pa"], pom=g["in_pam"])
    except Exception:
        a.close()
        raise
    return g, P, oc, a


_line_bounds = {}


def _line_bound(case):
    """2 n 2^-53 sum|terms| dxo of the two stress line integrals, the bound of tests/test_gpu_xforc.py: n and the sum of
    |terms| from the numpy restatement of the momentum half (no shear term, so the ocean's pressure is not read)."""
    if case not in _line_bounds:
        g = na.load(case)
        P = dict(na.params(g), tau_udiff=0, cyclic=0)
        pom1 = np.zeros((P["nxaooc"] * P["ndxr"] + 1, P["nyaooc"] * P["ndxr"] + 1), order="F")
        N = nx.xforc(g["in_pam"][:, :, 0], pom1, nx.tables(g), P)
        _line_bounds[case] = ({f: 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * P["dxo"] for f in na.MOM_INTEGRALS},
                              {f: N[f] for f in na.MOM_FIELDS})
    return _line_bounds[case]


@pytest.mark.parametrize("case", na.CASES)
def test_momentum_without_ocean(case):
    """qgcm_hip_xforc(NULL, atm), the momentum half alone, against the first xforc of an atmos_only reference: tauxa,
    tauya, uekat, vekat, wekta, wekpa bitwise; txisat, txinat within the worst case of reordering their sums; a second
    call gives identical bits."""
    from qgcm_hip import xforc, xforc_get
    g, P, oc, a = _atmos(case, aml=False, sst=False)
    try:
        xforc(None, a)
        R = xforc_get(None, a)
        xforc(None, a)
        R2 = xforc_get(None, a)
        assert not set(R) & {"tauxo", "tauyo", "wekto", "wekpo"}
        bound, _ = _line_bound(case)
        for f in na.MOM_FIELDS:
            _same(R[f], g["x0_" + f], "%s %s" % (case, f))
            _same(R[f], R2[f], "%s %s (repeat)" % (case, f))
            assert np.abs(g["x0_" + f]).max() > 0.0
        for f in na.MOM_INTEGRALS:
            ref = float(g["x0_" + f])
            print("%s %s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (case, f, R[f], ref, abs(R[f] - ref), bound[f]))
            assert abs(R[f] - ref) <= bound[f], (case, f, R[f], ref, bound[f])
            assert R[f] == R2[f] and ref != 0.0
        assert R["txisoc"] == 0.0 and R["txinoc"] == 0.0
    finally:
        a.close()


@pytest.mark.parametrize("case", na.CASES)
def test_heat_from_sst(case):
    """The heat half from the SST against the first xforc of the fixture: fnetat bitwise over land; above the sea within
    2 ndxr^2 2^-53 sum|terms| of the cell plus one spacing of the value (the pointwise tail is added to the cell's sum
    afterwards); slhfav, oradav, arlaav within 2 n 2^-53 sum|terms|; arocav = 0 exactly, on ato_allsea arlaav too; a
    second call gives identical bits."""
    from qgcm_hip import xforc, xforc_sst_get
    g, P, oc, a = _atmos(case)
    try:
        a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
        xforc(None, a)
        H = xforc_sst_get(a)
        xforc(None, a)
        H2 = xforc_sst_get(a)
        N = na.restated(case)[0]
        ref, sea = g["x0_fnetat"], N["ocean"]
        _same(H["fnetat"][~sea], ref[~sea], case + " fnetat over land")
        blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
        assert sea[blk].all() and sea.sum() == N["cell_abs"].size
        bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"] + np.spacing(np.abs(ref[blk]))
        diff = np.abs(H["fnetat"][blk] - ref[blk])
        print("%s fnetat above the sea: max |diff| %.3e, largest |diff| / bound %.3f" % (case, diff.max(), (diff / bound).max()))
        assert np.all(diff <= bound), (case, diff.max(), (diff / bound).max())
        assert np.all(H["fnetat"][sea] != 0.0)
        _same(H["fnetat"], H2["fnetat"], case + " fnetat (repeat)")
        for f in na.SST_SCALARS:
            r = float(g["x0_" + f])
            b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
            print("%s %s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (case, f, H[f], r, abs(H[f] - r), b))
            assert abs(H[f] - r) <= b, (case, f, H[f], r, b)
            assert H[f] == H2[f], (case, f)
        assert H["arocav"] == 0.0 and H2["arocav"] == 0.0 and float(g["x0_arocav"]) == 0.0
        if case == "ato_allsea":
            assert H["arlaav"] == 0.0 and not (~sea).any()
        else:
            assert H["arlaav"] != 0.0
        # the momentum half ran in the same call
        _same(xforc_get_field(a, "wekta"), g["x0_wekta"], case + " wekta")
    finally:
        a.close()


def xforc_get_field(a, name):
    from qgcm_hip import xforc_get
    return xforc_get(None, a, names=(name,))[name]


@pytest.mark.parametrize("case", na.CASES)
def test_chained(case):
    """The fixture's K cycles on the device from the initial state only (xforc(); aml() x nstr): after the last cycle
    ast, hmixa, entat and fnetat agree with the reference to 1e-13 of their maximum."""
    from qgcm_hip import xforc, xforc_sst_get
    g, P, oc, a = _atmos(case)
    try:
        a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
        for c in range(P["K"]):
            xforc(None, a)
            if c == P["K"] - 1:
                fnetat = xforc_sst_get(a)["fnetat"]
            for s in range(P["nstr"]):
                a.aml()
        ast, _, hmixa, _ = a.aml_get_state()
        entat, _ = a.aml_get_diag()
        last = "a%d%d_" % (P["K"] - 1, P["nstr"] - 1)
        errs = dict(ast=relerr(ast, g[last + "ast"]), hmixa=relerr(hmixa, g[last + "hmixa"]),
                    entat=relerr(entat, g[last + "entat"]), fnetat=relerr(fnetat, g["x%d_fnetat" % (P["K"] - 1)]))
        print(case, errs)
        for k, e in errs.items():
            assert e < 1e-13, (case, k, e)
    finally:
        a.close()


def _window_atmos(cus):
    from qgcm_hip.lib import check
    g, P, oc, a = _atmos("ato_tiny")
    try:
        a.set_p(g["in_pa"], g["in_pam"])
        nl = a.cfg.nla
        a.set_forcing(np.zeros((a.cfg.nxpa, a.cfg.nypa), order="F"), np.zeros((a.cfg.nxpa, a.cfg.nypa), order="F"),
                      np.zeros(nl - 1), 0.0, 0.0, np.zeros(nl - 1), np.zeros(nl - 1))
        a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
        if cus:
            check(a.L.qgcm_hip_set_cu_range(a.h, 0, cus))
    except Exception:
        a.close()
        raise
    return a


@pytest.mark.parametrize("cus", [0, 64])
def test_window(cus):
    """ato_tiny's atmosphere, nstr = 3, 7 steps: coupled_steps(None, a, 1, 7, 3, xforc=True) - the reference's
    atmos_only sequence xforc; (aml; qgastep; atinvq; atqzbd) x nstr - is bitwise the explicit xforc(None, a);
    a.steps(k, s0=nt), and differs from the same window with the forcing held; without and with a CU range."""
    from qgcm_hip import coupled_steps, xforc, xforc_sst_get
    nstr, n = 3, 7
    res = {}
    for mode in ("window", "explicit", "held"):
        a = _window_atmos(cus)
        try:
            if mode == "explicit":
                nt = 1
                while nt <= n:
                    k = min(nstr, n - nt + 1)
                    xforc(None, a)
                    a.steps(k, s0=nt)
                    nt += k
            else:
                coupled_steps(None, a, 1, n, nstr, xforc=(mode == "window"))
            a.sync()
            res[mode] = [np.array(x) for x in a.get_state()] + [np.array(x) for x in a.aml_get_state()] + [a.aml_get_diag()[0]]
            if mode != "held":
                res[mode].append(xforc_sst_get(a)["fnetat"])
            assert all(np.isfinite(x).all() for x in res[mode])
        finally:
            a.close()
    assert len(res["window"]) == len(res["explicit"]) == 10
    for k, (x, y) in enumerate(zip(res["window"], res["explicit"])):
        _same(x, y, "window vs explicit, field %d" % k)
    assert np.abs(res["window"][9]).max() > 0.0
    assert not np.array_equal(res["window"][0], res["held"][0])  # pa: wekpa and entat drive the atmosphere
    assert not np.array_equal(res["window"][4], res["held"][4])  # ast: fnetat drives the mixed layer


def test_sst_set():
    """A replaced SST changes fnetat in the cells above the sea only, and slhfav / oradav; the first SST set back
    restores the first call's bits."""
    from qgcm_hip import QgcmHipError, xforc, xforc_sst_get, xforc_sst_set
    g, P, oc, a = _atmos("ato_odd5")
    try:
        a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
        sea = na.restated("ato_odd5")[0]["ocean"]
        xforc(None, a)
        H0 = xforc_sst_get(a)
        xforc_sst_set(a, g["in_sstm"] + 1.5)
        xforc(None, a)
        H1 = xforc_sst_get(a)
        _same(H1["fnetat"][~sea], H0["fnetat"][~sea], "fnetat over land")
        assert np.all(H1["fnetat"][sea] != H0["fnetat"][sea])
        assert H1["slhfav"] != H0["slhfav"] and H1["oradav"] != H0["oradav"]
        assert H1["arlaav"] == H0["arlaav"] and H1["arocav"] == 0.0
        with pytest.raises(QgcmHipError, match="sst has shape"):
            xforc_sst_set(a, g["in_sstm"][:-1])
        xforc_sst_set(a, g["in_sstm"])
        xforc(None, a)
        H2 = xforc_sst_get(a)
        _same(H2["fnetat"], H0["fnetat"], "fnetat restored")
        assert all(H2[f] == H0[f] for f in na.SST_SCALARS + ("arocav",))
    finally:
        a.close()


def _standing(a, g):
    from qgcm_hip import xforc, xforc_sst_get
    a.aml_set_state(**{f: g["in_" + f] for f in na.STATE})
    xforc(None, a)
    a.aml()
    return xforc_sst_get(a), a.aml_get_state(), a.aml_get_diag()


def _unchanged(before, after):
    _same(after[0]["fnetat"], before[0]["fnetat"], "fnetat")
    assert all(after[0][f] == before[0][f] for f in na.SST_SCALARS + ("arocav",))
    for x, y in zip(after[1], before[1]):
        _same(x, y, "state")
    _same(after[2][0], before[2][0], "entat")
    assert after[2][1] == before[2][1]


def test_refused_with_ocean():
    """An atmosphere whose xforc was set up WITH an ocean has its heat half in qgcm_hip_xforc_heat_init."""
    from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, xforc_setup, xforc_sst_setup
    g, P, oc, a = _atmos("ato_tiny")
    extra = []
    try:
        before = _standing(a, g)
        o, b = OceanModel(oc), AtmosModel(a.cfg)
        extra += [o, b]
        kw = _mom_kw(P)
        xforc_setup(o, b, **{k: kw[k] for k in ("cdat", "rhoat", "rhooc", "hmat", "hmoc")})
        b.aml_init(_aml_cfg(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_init: this atmosphere's xforc was set up with an ocean: "
                                               "its heat half is qgcm_hip_xforc_heat_init"):
            xforc_sst_setup(b, oc, _heat_cfg(P), g["in_sstm"], **_sst_kw(g))
        _unchanged(before, _standing(a, g))
    finally:
        for m in extra + [a]:
            m.close()


def test_refused_before_setup():
    """Before xforc_setup, before aml_init, and xforc_sst_get before the set-up."""
    from qgcm_hip import AtmosModel, QgcmHipError, xforc_setup, xforc_sst_get, xforc_sst_setup
    g, P, oc, a = _atmos("ato_tiny")
    b = None
    try:
        before = _standing(a, g)
        b = AtmosModel(a.cfg)
        hc, kw = _heat_cfg(P), _sst_kw(g)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_init: qgcm_hip_xforc_init has not been called"):
            xforc_sst_setup(b, oc, hc, g["in_sstm"], hmadmp=P["hmadmp"], hmat=P["hmat"], **kw)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_get: qgcm_hip_xforc_init has not been called"):
            xforc_sst_get(b)
        xforc_setup(None, b, tables=nx.tables(g), **_mom_kw(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_init: qgcm_hip_aml_init has not been called"):
            xforc_sst_setup(b, oc, hc, g["in_sstm"], hmadmp=P["hmadmp"], hmat=P["hmat"], **kw)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_get: qgcm_hip_xforc_sst_init has not been called"):
            xforc_sst_get(b)
        _unchanged(before, _standing(a, g))
    finally:
        for m in (b, a):
            if m is not None:
                m.close()


def test_refused_arguments():
    """An SST of the wrong shape (refused on the Python side), a coordinate the atmosphere does not cover, and the
    heat half WITH an ocean handle still refusing oc = NULL in its own words."""
    from qgcm_hip import QgcmHipError, xforc_heat_setup, xforc_sst_setup
    g, P, oc, a = _atmos("ato_tiny")
    try:
        before = _standing(a, g)
        hc, kw = _heat_cfg(P), _sst_kw(g)
        with pytest.raises(QgcmHipError, match=r"xforc_sst_setup: sst has shape \(47, 36\), need \(48, 36\)"):
            xforc_sst_setup(a, oc, hc, g["in_sstm"][:-1], **kw)
        far = dict(kw["coords"], xto=kw["coords"]["xto"] + 1.0e9)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_sst_init: the atmosphere's xta does not cover ocean column 1"):
            xforc_sst_setup(a, oc, hc, g["in_sstm"], fsa=kw["fsa"], coords=far)
        with pytest.raises(QgcmHipError, match=r"qgcm_hip_xforc_heat_init: the heat half needs an ocean \(oc = NULL\)"):
            xforc_heat_setup(None, a, hc, fsa=kw["fsa"])
        _unchanged(before, _standing(a, g))
    finally:
        a.close()
