"""The momentum half of xforc on the device (qgcm_hip_xforc) against the reference's own results
(tests/golden/xf_*.npz) and against itself: golden comparison, repeatability, destinations, the coupled window and the
refusals."""
import dataclasses

import numpy as np
import pytest

import numpy_xforc as nx
from common import atm_apply, load_golden
from qgcm_hip import config

pytestmark = pytest.mark.gpu


def _setup_kw(P):
    """The constants of a fixture as keyword arguments of xforc_setup (raoro = rhoat / rhooc)."""
    return dict(cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tau_udiff=bool(P["tau_udiff"]))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _models(case):
    """Ocean and atmosphere models with a fixture's dimensions and constants, xforc set up with the fixture's tables."""
    from qgcm_hip import AtmosModel, OceanModel, xforc_setup
    g = nx.load(case)
    P = nx.params(g)
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"])
    at = config.atmos_of(oc, bccoat=P["bccoat"])
    o, a = OceanModel(oc), AtmosModel(at)
    xforc_setup(o, a, tables=nx.tables(g), **_setup_kw(P))
    assert (a.cfg.nxta - oc.nxaooc) // 2 + 1 == P["nx1"] and (a.cfg.nyta - oc.nyaooc) // 2 + 1 == P["ny1"]
    return g, P, o, a


def _load_state(o, a, g, s):
    """The fixture's lagged layer-1 pressures into both time levels (the other layers zero, as the generator's)."""
    for m, f in ((a, g["in%d_pam1" % s]), (o, g["in%d_pom1" % s])):
        p = np.zeros(f.shape + (3,), order="F")
        p[:, :, 0] = f
        m.set_state(po=p, pom=p)


@pytest.mark.parametrize("case", nx.CASES)
def test_golden(case):
    """Every pointwise field of both states bitwise the reference's; the four line integrals (parallel sums) within
    the worst case of reordering a sum of n terms, 2 n 2^-53 sum|terms| dxo; a second call gives identical bits."""
    from qgcm_hip import xforc, xforc_get
    g, P, o, a = _models(case)
    try:
        for s in range(2):
            _load_state(o, a, g, s)
            xforc(o, a)
            R = xforc_get(o, a)
            xforc(o, a)
            R2 = xforc_get(o, a)
            N = nx.restated(case, s)
            for f in nx.POINTWISE:
                ref = g["out%d_%s" % (s, f)]
                assert R[f].shape == ref.shape, f
                assert np.array_equal(_bits(R[f]), _bits(ref)), "%s state %d %s: max |diff| %.3e, %d points differ" % (
                    case, s, f, np.abs(R[f] - ref).max(), int((_bits(R[f]) != _bits(ref)).sum()))
                assert np.array_equal(_bits(R[f]), _bits(R2[f])), f
            for f in nx.INTEGRALS:
                ref = float(g["out%d_%s" % (s, f)])
                bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * P["dxo"]
                print("%s state %d %s: device %.17e reference %.17e |diff| %.3e bound %.3e" % (
                    case, s, f, R[f], ref, abs(R[f] - ref), bound))
                assert abs(R[f] - ref) <= bound, (f, R[f], ref, bound)
                assert R[f] == R2[f], f
                if f.endswith("at") or P["cyclic"]:
                    assert ref != 0.0
    finally:
        o.close()
        a.close()


@pytest.mark.parametrize("case", ["xf_cpl_tiny_ud", "xf_cyc4_ud", "xf_cycwide_ud"])
def test_destinations(case):
    """After xforc the consumers' own buffers hold what xforc_get reports: wekpa / wekpo where the steppers read them
    (the buffers of set_forcing), the scalars behind set_cyc_forcing, the mixed layer's wekto and stress (after
    oml_init; through valids' and the monitors' reads of them) and the atmosphere's monitor fields (through
    atm_valids' extrema)."""
    from qgcm_hip import oml_preset, xforc, xforc_get
    g, P, o, a = _models(case)
    try:
        om = oml_preset(o.cfg)
        o.oml_init(om)
        zt = np.zeros((o.cfg.nxto, o.cfg.nyto), order="F")
        o.oml_set_state(zt, zt)
        _load_state(o, a, g, 0)
        xforc(o, a)
        R = xforc_get(o, a)
        # the mixed layer's wekto: valids scans it (out[6], out[7] = min, max of wekto) when the mixed layer is on
        _, vo = o.valids()
        assert vo[6] == R["wekto"].min() and vo[7] == R["wekto"].max() and vo[6] < vo[7]
        # the mixed layer's stress: utauoc of the monitors is formed from tauxo, tauyo; zero stress gives zero
        o.set_monitor_params(oml=om)
        ut = o.monitors()["utauoc"]
        assert np.isfinite(ut) and ut != 0.0
        zp = np.zeros((o.cfg.nxpo, o.cfg.nypo), order="F")
        o.oml_set_forcing(tauxo=zp, tauyo=zp)
        assert o.monitors()["utauoc"] == 0.0
        xforc(o, a)
        assert o.monitors()["utauoc"] == ut
        # the atmosphere's monitor fields: min, max of wekta, tauxa, tauya are entries 6..11 of atm_valids
        a.set_atm_monitor_fields(ast=np.zeros((a.cfg.nxta, a.cfg.nyta), order="F"))
        _, av = a.atm_valids()
        for k, f in ((6, "wekta"), (8, "tauxa"), (10, "tauya")):
            assert av[k] == R[f].min() and av[k + 1] == R[f].max() and av[k] < av[k + 1], f
        # the scalars behind set_cyc_forcing: overwritten through the setter, restored by the next xforc
        a.set_cyc_forcing(123.0, 456.0)
        if P["cyclic"]:
            o.set_cyc_forcing(123.0, 456.0)
        z = xforc_get(o, a, names=nx.INTEGRALS)
        assert z["txisat"] == 123.0 and z["txinat"] == 456.0 and z["txisoc"] == (123.0 if P["cyclic"] else 0.0)
        # wekpa / wekpo: overwritten through set_forcing (what the steppers read), restored by the next xforc
        a.set_forcing(np.zeros_like(R["wekpa"]))
        o.set_forcing(np.zeros_like(R["wekpo"]))
        z = xforc_get(o, a, names=("wekpa", "wekpo"))
        assert not z["wekpa"].any() and not z["wekpo"].any()
        xforc(o, a)
        z = xforc_get(o, a)
        for f in ("wekpa", "wekpo") + nx.INTEGRALS:
            assert np.array_equal(np.asarray(z[f]), np.asarray(R[f])), f
    finally:
        o.close()
        a.close()


def _cpl_tiny(share):
    from qgcm_hip import AtmosModel, OceanModel, share_gpu, xforc_setup
    g = load_golden("cpl_tiny")
    oc, at = config.preset("cpl_tiny"), config.atmos_preset("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(g["in_po"], g["in_pom"])
    o.set_forcing(g["in_wekpo"], np.zeros_like(g["in_wekpo"]), np.zeros(oc.nlo - 1))
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("share", [False, True])
def test_coupled_window(share):
    """cpl_tiny, nstr = 3: a window of 7 atmospheric steps with xforc=True is bitwise the explicit sequence
    xforc(); ocean.steps(1); atmos.steps(3) and differs from the same window with the forcing held; the same with a
    CU range on both handles."""
    from qgcm_hip import coupled_steps, xforc
    nstr, n = 3, 7
    res = {}
    for mode in ("window", "explicit", "held"):
        o, a = _cpl_tiny(share)
        try:
            if mode == "explicit":
                nt = 1
                while nt <= n:
                    xforc(o, a)
                    o.steps(1, s0=(nt - 1) // nstr + 1)
                    k = min(nstr, n - nt + 1)
                    a.steps(k, s0=nt)
                    nt += k
            else:
                coupled_steps(o, a, 1, n, nstr, xforc=(mode == "window"))
            o.sync()
            a.sync()
            res[mode] = [np.array(x) for x in o.get_state()] + [np.array(x) for x in a.get_state()]
            assert all(np.isfinite(x).all() for x in res[mode])
        finally:
            o.close()
            a.close()
    for x, y in zip(res["window"], res["explicit"]):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(res["window"][0], res["held"][0])  # po: the atmosphere drives the ocean
    assert not np.array_equal(res["window"][4], res["held"][4])  # pa: and is driven by its own stress


def test_refusals():
    """Every refusal names its reason and changes no state."""
    from qgcm_hip import AtmosModel, QgcmHipError, xforc, xforc_get, xforc_setup
    from qgcm_hip.slab import HipSlab, global_consts, partition
    g, P, o, a = _models("xf_cpl_tiny_ud")
    b = sl = None
    try:
        _load_state(o, a, g, 0)
        xforc(o, a)
        before = xforc_get(o, a)
        kw = _setup_kw(P)
        T = nx.tables(g)
        # xforc before xforc_init (a second atmosphere that was never set up)
        b = AtmosModel(a.cfg)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_init has not been called"):
            xforc(o, b)
        # tau_udiff without an ocean
        with pytest.raises(QgcmHipError, match="tau_udiff needs an ocean"):
            xforc_setup(None, b, ndxr=P["ndxr"], tables=T, **kw)
        # mismatched geometry: a refinement the ocean's grid does not have; an ocean outside the atmosphere
        with pytest.raises(QgcmHipError, match="mismatched geometry"):
            xforc_setup(o, a, ndxr=P["ndxr"] // 2, **kw)
        with pytest.raises(QgcmHipError, match="does not lie inside"):
            xforc_setup(o, a, tables=T, nx1=P["nxta"], **kw)
        # a y-slab ocean handle
        (g0, g1), _ = partition(o.cfg.nypo, 2)
        sl = HipSlab(o.cfg, global_consts(o.cfg, o.helmholtz), g0, g1, 0, 2)
        with pytest.raises(QgcmHipError, match="y-slab"):
            xforc_setup(sl, a, tables=T, **kw)
        # a handle other than the one of the set-up
        with pytest.raises(QgcmHipError, match="not the one qgcm_hip_xforc_init was called with"):
            xforc(None, a)
        # the refused calls changed nothing: the set-up still stands and gives the same bits
        xforc(o, a)
        after = xforc_get(o, a)
        for f in nx.POINTWISE + nx.INTEGRALS:
            assert np.array_equal(np.asarray(before[f]), np.asarray(after[f])), f
    finally:
        for m in (sl, b, o, a):
            if m is not None:
                m.close()
