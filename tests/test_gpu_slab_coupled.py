"""xforc and the coupled window on a y-slab ocean under a replicated atmosphere: virtual ranks on one GPU
(HipSlab with sync_each_call - LocalComm copies on another stream - / SlabOcean / LocalComm), one whole-domain AtmosModel per rank.  Every case is held to the whole-domain device
result on the same data (computed once per fixture and shared) and, where the fixtures record a field, to the reference's
own results (tests/golden/heat_*.npz).  Fixtures: heat_cpl_tiny (ocean 49 x 37, ndxr = 12; three ranks cut atmosphere
cells), heat_cpl_small (97 x 81, ndxr = 16; five ranks: interior slabs with two halos), heat_cyc72 (a channel of
289 x 17, ndxr = 4: the line integrals on every rank, the cyclic wrap beside slab offsets)."""
import dataclasses

import numpy as np
import pytest

import numpy_heat as nh
from qgcm_hip import config

pytestmark = pytest.mark.gpu

STATE = ("ast", "astm", "hmixa", "hmixam")
ATM_FIELDS = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa")
CASES = [("heat_cpl_tiny", 1), ("heat_cpl_tiny", 2), ("heat_cpl_tiny", 3), ("heat_cpl_small", 5), ("heat_cyc72", 2),
         ("heat_cyc72", 3)]


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
    g = nh.load(case)
    P = nh.params(g)
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    return g, P, oc, config.atmos_of(oc, bccoat=P["bccoat"], gpat=(P["gpat1"], P["gpat2"]))


def _mkw(P):
    return dict(cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"])


def _hkw(g):
    return dict(fsa=g["t_fsa"], fso=g["t_fso"], coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})


def _atmos(g, P, at):
    from qgcm_hip import AtmosModel
    a = AtmosModel(at)
    a.aml_init(_aml_cfg(P), xc1ast=g["in_xc1ast"], dtopat=g["in_dtopat"])
    a.set_state(po=g["in_pa"], pom=g["in_pam"])
    a.aml_set_state(**{f: g["in_" + f] for f in STATE})
    return a


def _pom3(g):
    pom = np.zeros(g["in_pom"].shape + (3,), order="F")
    pom[:, :, 0] = g["in_pom"]
    return pom


def _whole(case, heat=True):
    """The whole-domain models of tests/test_gpu_heat.py (tau_udiff off) with the fixture's state loaded."""
    from qgcm_hip import OceanModel, oml_preset, xforc_heat_setup, xforc_setup
    g, P, oc, at = _configs(case)
    o = OceanModel(oc)
    a = _atmos(g, P, at)
    xforc_setup(o, a, tau_udiff=False, **_mkw(P))
    o.oml_init(oml_preset(oc))
    if heat:
        xforc_heat_setup(o, a, _heat_cfg(P), **_hkw(g))
    o.set_state(*_consts(case, oc)[1])
    o.set_scalars(_consts(case, oc)[2])
    o.oml_set_state(sst=g["in_sstm"], sstm=g["in_sstm"])
    return g, P, o, a


_cst = {}


def _consts(case, oc):
    """Once per fixture, from a whole-domain handle: the start-up constants on the global grid (a box basin's
    homogeneous solutions come from its Helmholtz solver) and the state po, pom, qo, qom with the fixture's pom in
    layer 1 at both levels, the vorticity and the constraint scalars that go with it (OceanModel.set_p)."""
    if case not in _cst:
        from qgcm_hip import OceanModel
        from qgcm_hip.slab import global_consts
        m = OceanModel(oc)
        try:
            consts = global_consts(oc) if oc.cyclic else global_consts(oc, m.helmholtz)
            pom = _pom3(nh.load(case))
            m.set_p(pom, pom)
            _cst[case] = (consts, [np.array(x) for x in m.get_state()], m.get_scalars())
        finally:
            m.close()
    return _cst[case]


def _slabbed(case, nranks, heat=True):
    """SlabOcean of `nranks` virtual ranks with one replica of the atmosphere each, the fixture's state loaded."""
    import torch
    from qgcm_hip import oml_preset
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, partition, slab_slice
    g, P, oc, at = _configs(case)
    consts, st, scal = _consts(case, oc)
    slabs = [HipSlab(oc, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.oml_init(oml_preset(oc))
    so = SlabOcean(oc, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
    for x in slabs:
        sl = slab_slice(oc.nypo, x.g0, x.g1)
        x.set_state(*[v[:, sl, :] for v in st])
        x.set_scalars(scal)
        x.oml_set_state(sst=g["in_sstm"], sstm=g["in_sstm"])
    reps = [_atmos(g, P, at) for _ in slabs]
    so.xforc_setup(reps, tau_udiff=False, **_mkw(P))
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), **_hkw(g))
    return g, P, so, reps


def _close(so, reps):
    for m in list(so.slabs) + list(reps):
        m.close()


_ref = {}


def _reference(case):
    """One whole-domain xforc() on the fixture's state: the outputs of both halves.  Computed once, shared, unchanged."""
    if case not in _ref:
        from qgcm_hip import xforc, xforc_get, xforc_heat_get
        g, P, o, a = _whole(case)
        try:
            xforc(o, a)
            _ref[case] = dict(xforc_get(o, a), **xforc_heat_get(o, a))
        finally:
            o.close()
            a.close()
    return _ref[case]


def _cut_cells(oc, P, nranks):
    """cut[cb]: the T rows of the cell row cb (0-based) are owned by more than one rank."""
    from qgcm_hip.slab import partition
    owner = np.zeros(oc.nyto, dtype=int)
    for r, (g0, g1) in enumerate(partition(oc.nypo, nranks)):
        owner[g0 - 1:min(g1, oc.nyto)] = r  # T rows g0..g1, g1-1 on the rank that owns row nypo
    n = P["ndxr"]
    return np.array([len(set(owner[cb * n:(cb + 1) * n])) > 1 for cb in range(P["nyaooc"])])


def _replicas_equal(reps, what):
    base = None
    for r, a in enumerate(reps):
        a.sync()
        st = a.get_state()
        ast, _, hmixa, _ = a.aml_get_state()
        cur = [st[0], ast, hmixa]
        if base is None:
            base = cur
        for k, (x, y) in enumerate(zip(cur, base)):
            _same(x, y, "%s: replica %d against replica 0, field %d" % (what, r, k))


def _check_xforc(case, nranks, so, reps, g, P):
    """One so.xforc() against the whole-domain call and the fixture (docstring of test_xforc_slab)."""
    oc = so.cfg
    ref = _reference(case)
    N = nh.restated(case)[("x", 0)]
    so.xforc()
    M, H = so.xforc_get(), so.xforc_heat_get()
    _replicas_equal(reps, case)
    cut = _cut_cells(oc, P, nranks)
    if nranks > 1:
        assert cut.any() and not cut.all(), cut
    else:
        assert not cut.any()
    blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
    land = ~N["ocean"]
    for r, (x, m, h) in enumerate(zip(so.slabs, M, H)):
        tag = "%s, %d ranks, rank %d: " % (case, nranks, r)
        for f in ATM_FIELDS:
            _same(m[f], ref[f], tag + f)
            _same(m[f], M[0][f], tag + f + " against rank 0")
        for f in ("uekat", "vekat", "wekta"):
            _same(m[f], g["x0_" + f], tag + f + " against the fixture")
        for f in ("txisat", "txinat", "txisoc", "txinoc"):
            assert m[f] == ref[f], (tag, f, m[f], ref[f])
        if oc.cyclic:
            assert m["txisoc"] != 0.0 and m["txinoc"] != 0.0
        # the slab's rows: local p row j is global row j + joff; T rows likewise
        pr, tr = slice(x.joff, x.joff + x.nyl), slice(x.joff, x.joff + x.nyl - 1)
        for f in ("tauxo", "tauyo"):
            _same(m[f], ref[f][:, pr], tag + f)
        _same(m["wekto"], ref["wekto"][:, tr], tag + "wekto")
        _same(h["fnetoc"], ref["fnetoc"][:, tr], tag + "fnetoc")
        _same(h["fnetoc"], g["x0_fnetoc"][:, tr], tag + "fnetoc against the fixture")
        # wekpo: every local row but the outermost halo row towards a neighbour (the T row beyond it is not held)
        lo = 1 if x.g0 > 1 else 0
        hi = x.nyl - (1 if x.g1 < oc.nypo else 0)
        assert lo <= x.jlo - 1 and hi >= x.jhi  # (the owned rows are among them)
        _same(m["wekpo"][:, lo:hi], ref["wekpo"][:, x.joff + lo:x.joff + hi], tag + "wekpo")
        # fnetat: land and the cells no seam cuts by bits; cut cells within the reordering bound of the cell's sum
        fa = h["fnetat"]
        _same(fa, H[0]["fnetat"], tag + "fnetat against rank 0")
        _same(fa[land], ref["fnetat"][land], tag + "fnetat over land")
        _same(fa[land], g["x0_fnetat"][land], tag + "fnetat over land against the fixture")
        _same(fa[blk][:, ~cut], ref["fnetat"][blk][:, ~cut], tag + "fnetat over the cells no seam cuts")
        if cut.any():
            bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"][:, cut]
            diff = np.abs(fa[blk][:, cut] - ref["fnetat"][blk][:, cut])
            print("%sfnetat over cut cells: max |diff| %.3e, largest |diff| / bound %.3f" % (tag, diff.max(), (diff / bound).max()))
            assert np.all(diff <= bound), (tag, diff.max(), (diff / bound).max())
        assert h["arlaav"] == ref["arlaav"], tag
        for f in ("slhfav", "oradav", "arocav"):
            b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
            print("%s%s: slabs %.17e whole domain %.17e |diff| %.3e bound %.3e" % (tag, f, h[f], ref[f], abs(h[f] - ref[f]), b))
            assert abs(h[f] - ref[f]) <= b, (tag, f, h[f], ref[f], b)
            assert abs(h[f] - float(g["x0_" + f])) <= b, (tag, f)
            assert h[f] == H[0][f], (tag, f)
        if nranks == 1:  # a lone slab: every output is the whole-domain call's, bit for bit
            _same(fa, ref["fnetat"], tag + "fnetat")
            _same(m["wekpo"], ref["wekpo"], tag + "wekpo")
            for f in nh.HEAT_SCALARS:
                assert h[f] == ref[f], (tag, f, h[f], ref[f])


@pytest.mark.parametrize("case,nranks", CASES)
def test_xforc_slab(case, nranks):
    """One xforc() on slabs.  Every slab's local rows of tauxo, tauyo, wekto, fnetoc (wekpo: but the outermost halo row
    of a seam) and the whole of tauxa, tauya, uekat, vekat, wekta, wekpa on every replica are the whole-domain device
    result by integer view; uekat, vekat, wekta, fnetoc and fnetat over land also the fixture's.  fnetat over the cells
    no seam cuts by integer view - the test computes which cells the partition cuts and needs one of each kind - and
    over cut cells within 2 n 2^-53 sum|terms|, n = ndxr^2, sum|terms| of the cell's own flux terms (the derivation of
    tests/common.py:oml_bounds: a sum of n terms in any order); slhfav, oradav, arocav within the same bound with
    n = nxto nyto; arlaav, the four line integrals and (one rank) everything by bits.  The replicas' pa, ast, hmixa,
    fnetat and wekpa are bit-equal across ranks."""
    g, P, so, reps = _slabbed(case, nranks)
    try:
        _check_xforc(case, nranks, so, reps, g, P)
    finally:
        _close(so, reps)


@pytest.mark.parametrize("var,val", [("QGCM_HIP_THOMAS_SLAB_SEG_ROWS", "7"), ("QGCM_HIP_ROW_SPLIT", "2")])
def test_xforc_slab_forced_plans(monkeypatch, var, val):
    """The channel on two ranks with the slabs' columns forced into segments, and with the rows forced into two
    sub-rows: the new calls drive such slabs unchanged (test_xforc_slab's assertions)."""
    case, nranks = "heat_cyc72", 2
    monkeypatch.setenv(var, val)  # read by qgcm_hip_set_grid
    g, P, so, reps = _slabbed(case, nranks)
    try:
        if var.endswith("SEG_ROWS"):
            # (segments hold 4 to 7 rows: the first slab's eight interior rows make two, the second's seven stay one)
            assert len(so.slabs[0].thomas_plan()) == 2, [x.thomas_plan() for x in so.slabs]
        else:
            assert all(x.row_plan() == (2, 144) for x in so.slabs), [x.row_plan() for x in so.slabs]
        _check_xforc(case, nranks, so, reps, g, P)
    finally:
        _close(so, reps)


NSTR, NWIN = 3, 9  # three ocean steps


def _collect(o_state, sst, a):
    a.sync()
    return dict(ocean=[np.array(x) for x in o_state], sst=[np.array(x) for x in sst],
                atmos=[np.array(x) for x in a.get_state()], aml=[np.array(x) for x in a.aml_get_state()],
                entat=np.array(a.aml_get_diag()[0]))


def _gather(so):
    """Global po, pom, qo, qom and sst, sstm from the slabs' owned rows."""
    oc = so.cfg
    st = [np.zeros((oc.nxpo, oc.nypo, oc.nlo)) for _ in range(4)]
    for g0, g1, fields in so.gather_local():
        for dst, src in zip(st, fields):
            dst[:, g0 - 1:g1, :] = src
    sst = [np.zeros((oc.nxto, oc.nyto)) for _ in range(2)]
    for x in so.slabs:
        t1 = min(x.g1, oc.nyto)
        for dst, src in zip(sst, x.oml_get_state()):
            dst[:, x.g0 - 1:t1] = src[:, x.g0 - 1 - x.joff:t1 - x.joff]
    return st, sst


_win = {}


def _cpl_tiny(nranks):
    """cpl_tiny as tests/test_gpu_heat.py:_cpl_tiny sets it up for its coupled window - the preset's own grid, time
    steps and coefficients, the true reference's state (tests/golden/cpl_tiny.npz), both mixed layers and the heat half
    with the constants and the smooth mixed-layer state of heat_cpl_tiny, the sst above toc(1) = 15 (a stable ocean
    mixed layer) - with tau_udiff off.  nranks = 0: (ocean, atmosphere); else (SlabOcean, replicas)."""
    import torch
    from common import atm_apply, load_golden
    from qgcm_hip import AtmosModel, OceanModel, oml_preset, xforc_heat_setup, xforc_setup
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    g, h = load_golden("cpl_tiny"), nh.load("heat_cpl_tiny")
    P = nh.params(h)
    oc, at = config.preset("cpl_tiny"), config.atmos_preset("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    sst = 22.0 + 0.5 * h["in_sstm"]
    zero, xon = np.zeros_like(g["in_wekpo"]), np.zeros(oc.nlo - 1)

    def atmos():
        a = AtmosModel(at, ddynat=f["ddynat"])
        atm_apply(a, f)
        r = at.dxa / (P["ndxr"] * P["dxo"])
        am = dataclasses.replace(_aml_cfg(P), at2d=P["at2d"] * r * r, at4d=P["at4d"] * r ** 4, ahmd=P["ahmd"] * r * r)
        a.aml_init(am, xc1ast=h["in_xc1ast"], dtopat=h["in_dtopat"])
        a.aml_set_state(**{k: h["in_" + k] for k in STATE})
        return a

    o = OceanModel(oc)
    o.set_p(g["in_po"], g["in_pom"])
    o.set_forcing(g["in_wekpo"], zero, xon)
    if nranks == 0:
        a = atmos()
        xforc_setup(o, a, tau_udiff=False)
        o.oml_init(oml_preset(oc))
        o.oml_set_state(sst=sst, sstm=sst)
        xforc_heat_setup(o, a, _heat_cfg(P))
        return o, a
    try:
        consts, st, scal = global_consts(oc, o.helmholtz), o.get_state(), o.get_scalars()
    finally:
        o.close()
    slabs = [HipSlab(oc, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.oml_init(oml_preset(oc))
    so = SlabOcean(oc, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
    so.scatter_state(st[0], st[1], st[2], st[3], g["in_wekpo"], zero, xon, scal)
    for x in slabs:
        x.oml_set_state(sst=sst, sstm=sst)
    reps = [atmos() for _ in slabs]
    so.xforc_setup(reps, tau_udiff=False)
    so.xforc_heat_setup(_heat_cfg(P))
    return so, reps


def _window(nranks, xforc=True):
    """coupled_steps over NWIN atmospheric steps on `nranks` slabs (0: the whole-domain models); computed once per
    (nranks, xforc) and shared."""
    key = (nranks, xforc)
    if key in _win:
        return _win[key]
    if nranks == 0:
        from qgcm_hip import coupled_steps
        o, a = _cpl_tiny(0)
        try:
            coupled_steps(o, a, 1, NWIN, NSTR, xforc=xforc)
            o.sync()
            res = _collect(o.get_state(), o.oml_get_state(), a)
        finally:
            o.close()
            a.close()
    else:
        so, reps = _cpl_tiny(nranks)
        try:
            so.coupled_steps(1, NWIN, NSTR, xforc=xforc)
            for x in so.slabs:
                x.sync()
            _replicas_equal(reps, "window on %d ranks" % nranks)
            if xforc:
                M, H = so.xforc_get(), so.xforc_heat_get()
                for m, h in zip(M, H):
                    _same(m["wekpa"], M[0]["wekpa"], "wekpa after the window, against rank 0")
                    _same(h["fnetat"], H[0]["fnetat"], "fnetat after the window, against rank 0")
            res = _collect(*_gather(so), reps[-1])
        finally:
            _close(so, reps)
    assert all(np.isfinite(v).all() for k in res for v in (res[k] if isinstance(res[k], list) else [res[k]]))
    _win[key] = res
    return res


def _relerr(x, y):
    return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))


def _window_close(got, ref, what):
    """The bars the slab tests already hold a stepped ocean to (tests/test_gpu_oml.py, the mixed layer on slabs: fields
    1e-10, sst 1e-12 of their maximum) and, for what the chain of xforc and aml produces (ast, hmixa, entat), the bar
    of tests/test_gpu_heat.py:test_chained: 1e-13 of the maximum."""
    errs = {}
    for k, x, y in [("ocean%d" % i, a, b) for i, (a, b) in enumerate(zip(got["ocean"], ref["ocean"]))]:
        errs[k] = (_relerr(x, y), 1e-10)
    for k, x, y in [("atmos%d" % i, a, b) for i, (a, b) in enumerate(zip(got["atmos"], ref["atmos"]))]:
        errs[k] = (_relerr(x, y), 1e-10)
    for i, (x, y) in enumerate(zip(got["sst"], ref["sst"])):
        errs["sst%d" % i] = (_relerr(x, y), 1e-12)
    for i, (x, y) in enumerate(zip(got["aml"], ref["aml"])):
        errs[STATE[i]] = (_relerr(x, y), 1e-13)
    errs["entat"] = (_relerr(got["entat"], ref["entat"]), 1e-13)
    print(what, {k: "%.2e" % e for k, (e, _) in errs.items()})
    for k, (e, bar) in errs.items():
        assert e <= bar, (what, k, e, bar)


@pytest.mark.parametrize("nranks", [1, 3])
def test_coupled_window_slabs(nranks):
    """cpl_tiny, SlabOcean.coupled_steps(1, 9, 3, xforc=True), both mixed layers and the heat half on: three ocean steps, nine
    atmospheric ones.  On one rank the window is bitwise the whole-domain coupled_steps (every field of the ocean, the
    atmosphere and both mixed layers).  On more ranks it agrees with it at the bars of _window_close; the replicas are
    bit-equal after the window; and the window moves what it should: without xforc the atmosphere's ast differs."""
    ref = _window(0)
    got = _window(nranks)
    if nranks == 1:
        for k in ("ocean", "sst", "atmos", "aml"):
            for i, (x, y) in enumerate(zip(got[k], ref[k])):
                _same(x, y, "window, one rank: %s %d" % (k, i))
        _same(got["entat"], ref["entat"], "entat")
    _window_close(got, ref, "window on %d ranks" % nranks)
    held = _window(nranks, xforc=False)
    assert not np.array_equal(got["aml"][0], held["aml"][0])


def test_golden_chain_slabs():
    """The golden chain of tests/test_gpu_heat.py:test_chained on three ranks: the fixture's K cycles with nothing
    re-fed (SlabOcean.xforc(); aml() x nstr on every replica); after the last cycle ast, hmixa, entat and every slab's
    rows of fnetoc agree with the reference at that test's bar, 1e-13 of their maximum."""
    case, nranks = "heat_cpl_tiny", 3
    g, P, so, reps = _slabbed(case, nranks)
    try:
        for c in range(P["K"]):
            so.xforc()
            if c == P["K"] - 1:
                H = so.xforc_heat_get()
            for s in range(P["nstr"]):
                for a in reps:
                    a.aml()
        _replicas_equal(reps, "chain")
        last = "a%d%d_" % (P["K"] - 1, P["nstr"] - 1)
        ast, _, hmixa, _ = reps[0].aml_get_state()
        entat, _ = reps[0].aml_get_diag()
        fo = g["x%d_fnetoc" % (P["K"] - 1)]
        errs = dict(ast=_relerr(ast, g[last + "ast"]), hmixa=_relerr(hmixa, g[last + "hmixa"]),
                    entat=_relerr(entat, g[last + "entat"]))
        for x, h in zip(so.slabs, H):
            errs["fnetoc%d" % x.rank] = float(np.abs(h["fnetoc"] - fo[:, x.joff:x.joff + x.nyl - 1]).max() / np.abs(fo).max())
        print(case, errs)
        for k, e in errs.items():
            assert e < 1e-13, (case, k, e)
    finally:
        _close(so, reps)


def test_held_forcing_is_the_explicit_sequence():
    """coupled_steps(..., xforc=False) on slabs is bitwise the explicit sequence of step() and the replicas' steps."""
    res = []
    for mode in ("window", "explicit"):
        so, reps = _cpl_tiny(2)
        try:
            so.xforc()  # (a forcing to hold)
            if mode == "window":
                so.coupled_steps(1, 7, NSTR, xforc=False)
            else:
                nt = 1
                while nt <= 7:
                    so.step((nt - 1) // NSTR + 1)
                    k = min(NSTR, 7 - nt + 1)
                    for a in reps:
                        a.steps(k, s0=nt)
                    nt += k
            for x in so.slabs:
                x.sync()
            res.append(_collect(*_gather(so), reps[0]))
        finally:
            _close(so, reps)
    for k in ("ocean", "sst", "atmos", "aml"):
        for i, (x, y) in enumerate(zip(*[r[k] for r in res])):
            _same(x, y, "%s %d" % (k, i))
    _same(res[0]["entat"], res[1]["entat"], "entat")


def test_refusals():
    """Every refusal of the set-up calls returns non-zero with its reason in qgcm_hip_last_error() and changes nothing:
    a following valid call works and gives the bits of a run that met no refusal; the whole-domain entry points refuse
    a slab set-up and the other way round."""
    import ctypes
    from qgcm_hip import AtmosModel, QgcmHipError, xforc, xforc_get
    from qgcm_hip.lib import XforcHeatParams, XforcParams, check
    case = "heat_cpl_tiny"
    g, P, so, reps = _slabbed(case, 2, heat=False)
    extra = []
    try:
        x, a = so.slabs[0], reps[0]
        L = x.L
        # an atmosphere handle that is not a whole-domain atmosphere: y-slabs of atmospheres do not exist, an ocean does
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_init: the handle was not created with qgcm_hip_params.atmos"):
            check(L.qgcm_hip_xforc_slab_init(x.h, so.slabs[1].h, ctypes.byref(XforcParams())))
        with pytest.raises(QgcmHipError, match="tau_udiff is not available with a y-slab ocean"):
            so.xforc_setup(reps, tau_udiff=True, **_mkw(P))
        # geometry that does not match the slab's GLOBAL grid: the slab's own 19 rows are not nyaooc * ndxr + 1
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_init: mismatched geometry"):
            so.xforc_setup(reps, tau_udiff=False, nyaooc=so.cfg.nyaooc - 1, **_mkw(P))
        # the heat half before oml_init on the slab: a lone slab without its mixed layer
        so2 = _slabbed_without_oml(case, extra)
        with pytest.raises(QgcmHipError, match="qgcm_hip_oml_init has not been called for this ocean"):
            so2.xforc_heat_setup(_heat_cfg(P), **_hkw(g))
        # ... before the momentum half's set-up, and before aml_init on the atmosphere
        b = AtmosModel(a.cfg)
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_heat_slab_init(x.h, b.h, ctypes.byref(XforcHeatParams())))
        so.xforc_setup([b, reps[1]], tau_udiff=False, **_mkw(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_aml_init has not been called for this atmosphere"):
            so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], **_hkw(g))
        so.xforc_setup(reps, tau_udiff=False, **_mkw(P))
        # the two set-ups exclude each other
        with pytest.raises(QgcmHipError, match="set up for a y-slab ocean"):
            xforc(x, a)
        with pytest.raises(QgcmHipError, match="set up for a y-slab ocean"):
            xforc_get(x, a)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_combine: qgcm_hip_xforc_heat_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_combine(x.h, a.h, None, 2))
        with pytest.raises(QgcmHipError, match="not the one qgcm_hip_xforc_slab_init was called with"):
            check(L.qgcm_hip_xforc_slab_part(so.slabs[1].h, a.h, None))
        # the refused calls changed nothing: the standing set-up gives the whole-domain bits
        so.xforc()
        ref = _reference(case)
        for y, m in zip(so.slabs, so.xforc_get()):
            _same(m["wekpa"], ref["wekpa"], "wekpa after the refusals")
            _same(m["tauxo"], ref["tauxo"][:, y.joff:y.joff + y.nyl], "tauxo after the refusals")
    finally:
        for m in extra:
            m.close()
        _close(so, reps)


def _slabbed_without_oml(case, extra):
    """A lone slab (the whole domain) without its mixed layer under an atmosphere with its own, momentum half set up."""
    import torch
    from qgcm_hip import AtmosModel
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean
    g, P, oc, at = _configs(case)
    x = HipSlab(oc, _consts(case, oc)[0], 1, oc.nypo, 0, 1, sync_each_call=True)
    extra.append(x)
    a = AtmosModel(at)
    a.aml_init(_aml_cfg(P))
    extra.append(a)
    so = SlabOcean(oc, [x], LocalComm(1, after=torch.cuda.synchronize))
    so.xforc_setup([a], tau_udiff=False, **_mkw(P))
    return so
