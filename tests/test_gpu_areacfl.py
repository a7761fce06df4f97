"""MI355X: the area averages (qgcm_hip_areavg*) and the CFL check (qgcm_hip_cfl*) of DESIGN 6m against the reference's
own results (tests/golden/areacfl_*.npz) and the numpy restatement tests/numpy_areacfl.py, which reproduces them
(tests/test_areacfl_cpu.py): whole-domain oceans and atmospheres, stepped handles, y-slabs as virtual ranks on one GPU,
the refusals and the absence of side effects.

Bars.  Area averages: the denominator bitwise the reference's serial one; the numerator - a sum in another order -
within 2 n 2^-53 sum|terms| of the restatement's (n = the area's points; the bound of a reordered sum, both orders
being within n 2^-53 sum|terms| of the exact value); the average is the device's own quotient of the two.  CFL: maxima,
counts and locations exactly the restatement's, and the reference's printed values at the 8 digits it prints."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime)

import numpy_areacfl as na
from common import OCEAN_LAYERS
from qgcm_hip import AtmosModel, OceanConfig, OceanModel, QgcmHipError
from qgcm_hip.config import atmos_of
from qgcm_hip.slab import global_consts, partition, slab_slice
from test_gpu_monitors import setup as stepped_setup
from test_gpu_slab_diagnostics import close as close_slabs, make_slabs

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def config(g, case):
    nxta, nyta, nxaooc, nyaooc, ndxr = (int(v) for v in g["c_dims"])
    nl = int(g["in_po"].shape[2])  # three, but for numpy_areacfl.CFL_LAYER_CASES
    assert nl == na.CFL_LAYER_CASES.get(case, 3)
    lay = OCEAN_LAYERS[nl] if nl != 3 else {}
    return OceanConfig("areacfl_" + case, nxta, nyta, nxaooc, nyaooc, ndxr, nl, fnot=float(g["c_fnot"]), beta=1.7536e-11,
                       cyclic=bool(g["c_cyclic"]), dxo=float(g["c_dxo"]), **lay)


_MODELS = {}


def model(case, fluid):
    """One model per (case, fluid) for the whole module, loaded with the fixture's fields; never stepped."""
    if (case, fluid) not in _MODELS:
        g = na.load(case)
        cfg = config(g, case)
        assert cfg.dto == float(g["c_dto"]) and cfg.dta == float(g["c_dta"])
        if fluid == "oc":
            m = OceanModel(cfg)
            po = np.asfortranarray(g["in_po"])
            m.set_state(po, po, po, po)
            m.set_monitor_params(hmoc=float(g["c_hmoc"]))
            m.set_monitor_fields(g["in_tauxo"], g["in_tauyo"], np.zeros_like(g["in_sst"]), g["in_sst"])
        else:
            m = AtmosModel(atmos_of(cfg))
            pa = np.asfortranarray(g["in_pa"])
            m.set_state(pa, pa, pa, pa)
            m.set_atm_monitor_fields(ast=g["in_ast"], uekat=g["in_uekat"], vekat=g["in_vekat"])
        _MODELS[(case, fluid)] = (m, g)
    return _MODELS[(case, fluid)]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m, _ in _MODELS.values():
        m.close()
    _MODELS.clear()


def check_areas(tag, got, field, T):
    """(avg, num, den) of the device against the restatement of `field`; prints every figure next to its bound."""
    avg, num, den = got
    ravg, rnum, rden, absum, npts = na.areavg(field, T)
    bound = na.reorder_bound(absum, npts)
    for m in range(len(avg)):
        print("%s area %d: n = %d  num %.17g  ref %.17g  |diff| %.3e  bound %.3e  den %.17g  avg %.17g  ref %.17g"
              % (tag, m + 1, npts[m], num[m], rnum[m], abs(num[m] - rnum[m]), bound[m], den[m], avg[m], ravg[m]))
    assert np.array_equal(bits(den), bits(rden)), (tag, den - rden)
    assert np.all(np.abs(num - rnum) <= bound), (tag, np.abs(num - rnum), bound)
    assert np.array_equal(bits(avg), bits(num / den)), tag
    return ravg


# 1. area averages against the fixtures --------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fluid", [("area_box", "oc"), ("area_atm", "at"), ("area_atm", "oc"), ("area_box", "at")])
def test_area_averages_against_the_reference(case, fluid):
    m, g = model(case, fluid)
    T = na.tables(g, fluid)
    lim = g[fluid + "_lim"]
    mine = m.set_areas(lim[:, 0], lim[:, 1], lim[:, 2], lim[:, 3])
    for k in T:
        assert np.array_equal(mine[k], T[k]), k
    got = m.area_averages(parts=True)
    ravg = check_areas("%s %s" % (case, fluid), got, g["in_sst" if fluid == "oc" else "in_ast"], T)
    assert np.array_equal(bits(ravg), bits(g[fluid + "_tav"]))  # the restatement is the reference, bit for bit
    again = m.area_averages(parts=True)
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(m.area_averages()), bits(got[0]))


@pytest.mark.parametrize("cfgname", ["box_seam", "cyc_72"])
def test_area_averages_follow_the_sst_rotation(cfgname):
    """A stepped mixed-layer handle, past the averaging step 26: the averages of the sst the device holds now."""
    m, om, f = stepped_setup(cfgname, True)
    try:
        cfg = m.cfg
        x, y = cfg.xlo, cfg.ylo
        T = m.set_areas([0.0, 0.13 * x, 0.4 * x], [x, 0.71 * x, 0.9 * x], [0.0, 0.22 * y, 0.5 * y], [y, 0.83 * y, y])
        before = m.area_averages()
        m.steps(30, s0=1)
        got = m.area_averages(parts=True)
        assert not np.array_equal(before, got[0])
        check_areas(cfgname + " stepped", got, m.oml_get_state()[0], T)
        assert np.array_equal(bits(m.area_averages()), bits(got[0]))
    finally:
        m.close()


# 2. CFL ------------------------------------------------------------------------------------------------------------------
def check_cfl(tag, got, want):
    for n, name in enumerate(want["names"]):
        print("%s %-5s max %.17g  ref %.17g  nbad %d  ref %d  loc %s  ref %s" % (
            tag, name, got["maxima"][n], want["maxima"][n], got["nbad"][n], want["nbad"][n], tuple(got["loc"][n]),
            tuple(want["loc"][n])))
    assert got["names"] == want["names"]
    assert np.array_equal(bits(got["maxima"]), bits(want["maxima"])), tag
    assert np.array_equal(got["nbad"], want["nbad"]), tag
    assert np.array_equal(got["loc"], want["loc"]), tag
    assert np.array_equal(bits(got["courant"]), bits(want["courant"])), tag


@pytest.mark.parametrize("case,fluid", [("cfl_box", "oc"), ("cfl_cyc", "oc"), ("cfl_atm", "at"), ("cfl_box", "at"),
                                        ("area_box", "oc"), ("area_atm", "at"), ("cfl_box2", "oc"), ("cfl_box5", "oc"),
                                        ("cfl_cyc6", "oc")])
def test_cfl_against_the_reference(case, fluid):
    m, g = model(case, fluid)
    want = na.cfl_of_fixture(g, fluid)
    got = m.cfl(float(g["c_cflcrit"]))
    check_cfl("%s %s" % (case, fluid), got, want)
    # the reference's print-out: 8 significant digits, every Bad line
    for a, ref in ((got["maxima"], g[fluid + "_max"]), (got["courant"], g[fluid + "_cfl"])):
        assert np.all(np.abs(a - ref) <= 0.5e-7 * 10.0 ** np.floor(np.log10(np.abs(ref))) * (1 + 1e-9))
    bad = g[fluid + "_bad"]
    assert np.array_equal(got["nbad"], [(bad[:, 0] == q).sum() for q in range(len(got["nbad"]))])
    assert got["nbad"].sum() > 0
    for q in np.nonzero(got["nbad"])[0]:
        rows = want["bad"][want["bad"][:, 0] == q]
        assert tuple(rows[np.argmax(rows[:, 3]), 1:3]) == tuple(got["loc"][q])
    again = m.cfl(float(g["c_cflcrit"]))
    for k in ("maxima", "nbad", "loc"):
        assert np.array_equal(got[k], again[k])
    # another criterion: nothing at or above it -> no offenders; a low one -> many
    assert m.cfl(1.0e3)["nbad"].sum() == 0
    if case in na.CFL_LAYER_CASES:  # the tie of the last layer's |v|: two Bad lines share the largest value, the first wins
        q = got["names"].index("v%d" % na.CFL_LAYER_CASES[case])
        rows = bad[bad[:, 0] == q]
        top = rows[rows[:, 3] == rows[:, 3].max()]
        assert len(top) == 2 and tuple(top[0, 1:3]) == tuple(got["loc"][q]) and top[0, 1] > top[1, 1] + 64
    low = 0.05
    check_cfl("%s %s crit %g" % (case, fluid, low), m.cfl(low), dict(na.cfl_of_fixture(dict(g, c_cflcrit=low), fluid)))


@pytest.mark.parametrize("cfgname", ["box_seam", "cyc_72"])
def test_cfl_of_a_stepped_handle(cfgname):
    m, om, f = stepped_setup(cfgname, True)
    try:
        cfg = m.cfg
        m.steps(30, s0=1)
        po = m.get_state()[0]
        kw = dict(rdxf0=1.0 / (cfg.dxo * cfg.fnot), dt=cfg.dto, dx=cfg.dxo, rhf0hm=0.5 / (cfg.fnot * om.hmoc))
        crit = 0.5 * na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=0.8, **kw)["courant"].max()
        want = na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=crit, **kw)
        assert want["nbad"].sum() > 0
        check_cfl(cfgname + " stepped", m.cfl(crit), want)
    finally:
        m.close()


# 3. y-slabs ------------------------------------------------------------------------------------------------------------
def slabs_of(case, parts):
    g = na.load(case)
    cfg = config(g, case)
    so = make_slabs(cfg, parts, global_consts(cfg))
    po = np.asfortranarray(g["in_po"])
    for x in so.slabs:
        sl = slab_slice(cfg.nypo, x.g0, x.g1)
        x.set_state(po[:, sl], po[:, sl], po[:, sl], po[:, sl])
        x.set_monitor_params(hmoc=float(g["c_hmoc"]))
        x.set_monitor_fields(g["in_tauxo"], g["in_tauyo"], np.zeros_like(g["in_sst"]), g["in_sst"])
    return so, g


def area_splits():
    T = na.tables(na.load("area_box"), "oc")
    j1, j2 = int(T["j1"][1]), int(T["j2"][1])  # the area on cell edges: T rows 11..30 of 40
    return {"halves": [(1, 20), (21, 41)],              # its south and north rows on different ranks
            "first_on_last_owned": [(1, j1), (j1 + 1, 41)],  # rank 0's last owned T row is the area's first
            "three": [(1, j1), (j1 + 1, j2), (j2 + 1, 41)],  # ... and its last row the middle rank's last
            "partition3": partition(41, 3)}


@pytest.mark.parametrize("split", ["halves", "first_on_last_owned", "three", "partition3"])
def test_slab_area_averages(split):
    parts = area_splits()[split]
    whole, g = model("area_box", "oc")
    T = na.tables(g, "oc")
    whole.set_areas(tables=T)
    wavg, wnum, wden = whole.area_averages(parts=True)
    if split != "partition3":
        assert (parts[0][1] < T["j2"][1]) and (T["j1"][1] <= parts[0][1])
    if split == "first_on_last_owned":
        assert parts[0][1] == T["j1"][1]
    so, _ = slabs_of("area_box", parts)
    try:
        so.set_areas(tables=T)
        res = so.diagnostic("areavg")
        for r in res[1:]:
            for a, b in zip(r, res[0]):
                assert np.array_equal(bits(a), bits(b))
        check_areas("area_box %s" % split, res[0], g["in_sst"], T)
        _, _, _, absum, npts = na.areavg(g["in_sst"], T)
        bound = na.reorder_bound(absum, npts)
        print("slab - whole numerators:", np.abs(res[0][1] - wnum), "bound", bound)
        assert np.all(np.abs(res[0][1] - wnum) <= bound) and np.array_equal(bits(res[0][2]), bits(wden))
        assert np.array_equal(bits(so.area_averages()), bits(res[0][0]))
    finally:
        close_slabs(so)


@pytest.mark.parametrize("case,nranks", [("cfl_box", 0), ("cfl_box", 2), ("cfl_box", 3), ("cfl_cyc", 2), ("cfl_cyc", 3),
                                         ("cfl_box2", 2), ("cfl_box5", 2), ("cfl_box5", 3), ("cfl_cyc6", 2), ("cfl_cyc6", 3)])
def test_slab_cfl(case, nranks):
    whole, g = model(case, "oc")
    crit = float(g["c_cflcrit"])
    want = whole.cfl(crit)
    if nranks == 0:  # the |u| maximum of layer 1 on a rank's last owned row: its row j+1 is a halo row
        j = int(want["loc"][want["names"].index("u1")][1])
        parts = [(1, j), (j + 1, int(g["in_po"].shape[1]))]
    else:
        parts = partition(int(g["in_po"].shape[1]), nranks)
    so, _ = slabs_of(case, parts)
    try:
        res = so.diagnostic("cfl", cflcrit=crit)
        for r in res:
            check_cfl("%s %s" % (case, parts), r, want)
        check_cfl("%s restated" % case, so.cfl(crit), na.cfl_of_fixture(g, "oc"))
    finally:
        close_slabs(so)


# 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_change_nothing():
    m, g = model("area_box", "oc")
    a, _ = model("area_atm", "at")
    T = na.tables(g, "oc")
    m.set_areas(tables=T)
    before = m.area_averages(parts=True)
    ten = {k: np.concatenate([v, v[:1]]) for k, v in T.items()}
    with pytest.raises(QgcmHipError, match="10 areas"):
        m.set_areas(tables=ten)
    bad = {k: v.copy() for k, v in T.items()}
    bad["i1"][2], bad["i2"][2] = T["i2"][2], T["i1"][2]
    with pytest.raises(QgcmHipError, match=r"area m = 3 has i1t = \d+ > i2t"):
        m.set_areas(tables=bad)
    bad = {k: v.copy() for k, v in T.items()}
    bad["j2"][4] = 41
    with pytest.raises(QgcmHipError, match=r"invalid subscript for ocean area m = 5"):
        m.set_areas(tables=bad)
    bad = {k: v.copy() for k, v in T.items()}
    bad["i1"][0] = 0
    with pytest.raises(QgcmHipError, match=r"invalid subscript for ocean area m = 1"):
        m.set_areas(tables=bad)
    with pytest.raises(ValueError, match="outside x range for ocean area m = 1"):
        m.set_areas([-1.0], [10.0], [0.0], [10.0])
    for x, y in zip(before, m.area_averages(parts=True)):
        assert np.array_equal(bits(x), bits(y))
    # the wrong kind of handle
    L = m.L
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    import ctypes
    ptr = ctypes.c_void_p(buf.data_ptr())
    assert L.qgcm_hip_cfl_part(a.h, 0.8, ptr) != 0
    assert "atmosphere" in L.qgcm_hip_last_error().decode() and "qgcm_hip_cfl_part" in L.qgcm_hip_last_error().decode()
    assert L.qgcm_hip_areavg_part(a.h, ptr) != 0 and "atmosphere" in L.qgcm_hip_last_error().decode()
    so, _ = slabs_of("cfl_box", partition(41, 2))
    try:
        x = so.slabs[0]
        out, nb = np.zeros(16), np.zeros(32, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        dp = ctypes.POINTER(ctypes.c_double)
        assert L.qgcm_hip_cfl(x.h, 0.8, out.ctypes.data_as(dp), nb.ctypes.data_as(ip), nb.ctypes.data_as(ip)) != 0
        assert "y-slab" in L.qgcm_hip_last_error().decode() and "qgcm_hip_cfl_part" in L.qgcm_hip_last_error().decode()
        assert L.qgcm_hip_areavg(x.h, out.ctypes.data_as(dp), None, None) != 0
        assert "y-slab" in L.qgcm_hip_last_error().decode()
    finally:
        close_slabs(so)
    # a missing field, a missing set-up
    cfg = config(g, "bare")
    bare = OceanModel(cfg)
    try:
        with pytest.raises(QgcmHipError, match="qgcm_hip_areavg_init has not been called"):
            bare.area_averages()
        bare.set_areas(tables=T)
        with pytest.raises(QgcmHipError, match="qgcm_hip_areavg: sst was never given"):
            bare.area_averages()
        with pytest.raises(QgcmHipError, match="qgcm_hip_cfl: tauxo was never given"):
            bare.cfl()
        bare.set_monitor_fields(tauxo=g["in_tauxo"])
        with pytest.raises(QgcmHipError, match="qgcm_hip_cfl: tauyo was never given"):
            bare.cfl()
        bare.set_monitor_fields(tauyo=g["in_tauyo"])
        with pytest.raises(QgcmHipError, match="qgcm_hip_cfl: hmoc was never given"):
            bare.cfl()
    finally:
        bare.close()
    ab = AtmosModel(atmos_of(cfg))
    try:
        ab.set_areas([0.0], [ab.cfg.xla], [0.0], [ab.cfg.yla])
        with pytest.raises(QgcmHipError, match="qgcm_hip_areavg: ast was never given"):
            ab.area_averages()
        with pytest.raises(QgcmHipError, match="qgcm_hip_cfl: uekat was never given"):
            ab.cfl()
    finally:
        ab.close()


# 5. no side effects -----------------------------------------------------------------------------------------------------
def test_set_up_areas_change_no_step():
    """A handle that set areas up and never calls the new entry points steps bitwise like one that did not; calling
    them changes no state either."""
    ms = [stepped_setup("box_seam", True)[0] for _ in range(3)]
    try:
        cfg = ms[0].cfg
        for m in ms[1:]:
            m.set_areas([0.0, 0.2 * cfg.xlo], [cfg.xlo, 0.7 * cfg.xlo], [0.0, 0.1 * cfg.ylo], [cfg.ylo, 0.6 * cfg.ylo])
        for n in (7, 23):
            for m in ms:
                m.steps(n)
            ms[2].area_averages()
            ms[2].cfl()
        ref = ms[0].get_state() + list(ms[0].oml_get_state())
        for m in ms[1:]:
            for a, b in zip(ref, m.get_state() + list(m.oml_get_state())):
                assert np.array_equal(bits(a), bits(b))
    finally:
        for m in ms:
            m.close()
