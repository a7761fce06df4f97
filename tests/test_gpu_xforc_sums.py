"""tau_udiff on a y-slab ocean by owner-computed sums on virtual ranks of one GPU: with udiff_sums = True every
rank forms the fine stress above the ocean rows it owns, from its own pressure and the 4 rows beyond each seam, and the
ranks exchange rank-ordered partial sums of uekat and wekpa.  The oracle is the whole-domain device call set up with
tau_udiff = True on the same data (tests/test_gpu_slab_udiff.py:_whole_ud), by integer view for everything but the
entries of uekat, wekpa, wekta that a seam cuts, which are held to bounds derived from the fine stress of the numpy
restatement (tests/numpy_xforc_sums.py:bounds, where the wekta bound is derived).  Every case runs under
QGCM_HIP_XF_POISON=1 (NaN bytes in the basin-sized pressure array before every edge assemble and in the fine arrays
before every part), on handles that never ran another mode, and is asserted on the SECOND of two xforc() calls, with the
fixture's two states.  Ranks on different GPUs are not tested here."""
import ctypes

import numpy as np
import pytest

import numpy_heat as nh
import numpy_xforc as nx
import numpy_xforc_sums as ns
import test_gpu_slab_coupled as tsc
import test_gpu_slab_udiff as tud
from numpy_slab_udiff import configs
from test_gpu_slab_coupled import NSTR, NWIN, _bits, _same

pytestmark = pytest.mark.gpu

EXACT = ("tauxa", "tauya", "vekat")
SUMS = ("uekat", "wekpa", "wekta")


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    monkeypatch.setenv("QGCM_HIP_XF_POISON", "1")  # read by qgcm_hip_xforc_slab_sums (and by the other modes' set-ups)


def _slabs_sums(case, nranks):
    """SlabOcean of `nranks` virtual ranks on fresh handles, one replica of the atmosphere each, the momentum half set up
    with the fixture's tables and the owner-computed sums."""
    import torch
    from qgcm_hip import AtmosModel
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, partition
    g, P, oc, at = configs(case)
    consts = tud._consts_ud(case, oc)
    slabs = [HipSlab(oc, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    so = SlabOcean(oc, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
    reps = [AtmosModel(at) for _ in slabs]
    so.xforc_setup(reps, tables=nx.tables(g), udiff_sums=True, **tud._kw(P))
    return g, P, so, reps


def _bounds(P, rows, stress):
    """numpy_xforc_sums.bounds for a cut `rows` of the geometry P on the fine stress (txf, tyf, wf, uvekfc)."""
    D = ns.dims(P["nyta"], P["ndxr"], P["ny1"], P["nyaooc"])
    txf, tyf, wf, uvekfc = stress
    return ns.bounds(D, P["nxta"], txf, tyf, wf, uvekfc, P["hmat"] / (P["ndxr"] * P["dxo"]), ns.owner_rows(D, rows)[0])


def _check_momentum(tag, so, M, ref, B, g=None, case=None, s=1):
    """Every field of xforc_get on every rank against the whole-domain result `ref`: tauxa, tauya, vekat and the four line
    integrals whole and by bits; the ocean's fields on the slab's rows by bits (wekpo: but the outermost halo row of a seam,
    which no kernel reads); uekat, wekpa, wekta by bits at every entry B says no seam cuts and within B's bound at the
    others; replicas bit-equal; no NaN.  With a fixture: the bitwise fields against it too, the integrals within
    test_golden's bound.

    The bounds (numpy_xforc_sums.bounds), from the fine stress of the numpy restatement, never from the device's output:
    a cut uekat line is the same ndxr + 1 terms in another order, each order's rounding at most (ndxr + 1) 2^-53 of the
    sum of the terms' magnitudes: 2 (ndxr + 1) 2^-53 uvekfc sum |w_k tyf_k|; a cut wekpa box likewise with its N terms:
    2 N 2^-53 sum |w wf| / wsum.  wekta = -hmrdxa (ue[i+1] - ue[i] + ve[j+1] - ve[j]) reads two uekat with bounds B[i+1],
    B[i] and a bitwise vekat: in exact arithmetic the two results differ by at most hmrdxa B, B = B[i+1] + B[i]; each
    result rounds three additions and one product, each by at most 2^-53 (1 + 3 2^-53) of a partial result no larger
    than S = |ue[i+1]| + |ue[i]| + |ve[j+1]| + |ve[j]| + B - eight roundings in the two results, taken as nine to cover
    the second-order terms: hmrdxa B + 9 2^-53 hmrdxa S.  wekta counts as cut where either uekat it reads is."""
    oc = so.cfg
    worst = {}
    for r, (x, m) in enumerate(zip(so.slabs, M)):
        t = "%s rank %d: " % (tag, r)
        pr, tr = slice(x.joff, x.joff + x.nyl), slice(x.joff, x.joff + x.nyl - 1)
        lo = 1 if x.g0 > 1 else 0
        hi = x.nyl - (1 if x.g1 < oc.nypo else 0)
        for f in EXACT + SUMS:
            assert not np.isnan(m[f]).any(), t + f + " holds a NaN"
            _same(m[f], M[0][f], t + f + " against rank 0")
        for f in EXACT:
            _same(m[f], ref[f], t + f)
        for f in SUMS:
            cut, bound = B[f]
            assert cut.shape == m[f].shape
            assert cut.any() == (so.P > 1) and not cut.all(), (t, f)
            _same(m[f][~cut], ref[f][~cut], t + f + " where no seam cuts")
            d = np.abs(m[f] - ref[f])
            if cut.any():
                ratio = float((d[cut] / bound[cut]).max())
                worst[f] = max(worst.get(f, 0.0), ratio)
                assert np.all(d[cut] <= bound[cut]), (t, f, ratio)
        for f in ("tauxo", "tauyo"):
            assert not np.isnan(m[f]).any(), t + f + " holds a NaN"
            _same(m[f], ref[f][:, pr], t + f)
        assert not np.isnan(m["wekto"]).any() and not np.isnan(m["wekpo"][:, lo:hi]).any(), t
        _same(m["wekto"], ref["wekto"][:, tr], t + "wekto")
        _same(m["wekpo"][:, lo:hi], ref["wekpo"][:, x.joff + lo:x.joff + hi], t + "wekpo")
        for f in tud.LINES:
            assert _bits(m[f]) == _bits(ref[f]), (t, f, m[f], ref[f])
        if oc.cyclic:
            assert m["txisoc"] != 0.0 and m["txinoc"] != 0.0
        if so.P == 1:
            _same(m["wekpo"], ref["wekpo"], t + "wekpo, a lone slab")
        if g is not None:
            N = nx.restated(case, s)
            for f in EXACT:
                _same(m[f], g["out%d_%s" % (s, f)], t + f + " against the fixture")
            for f in ("tauxo", "tauyo"):
                _same(m[f], g["out%d_%s" % (s, f)][:, pr], t + f + " against the fixture")
            _same(m["wekto"], g["out%d_wekto" % s][:, tr], t + "wekto against the fixture")
            _same(m["wekpo"][:, lo:hi], g["out%d_wekpo" % s][:, x.joff + lo:x.joff + hi], t + "wekpo against the fixture")
            for f in tud.LINES:
                fx = float(g["out%d_%s" % (s, f)])
                bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * nx.params(g)["dxo"]
                assert abs(m[f] - fx) <= bound, (t, f, m[f], fx, bound)
    print("%s largest |diff| / bound over the cut entries: %s" % (tag, {f: "%.3f" % v for f, v in worst.items()}))


def _run_case(case, nranks):
    from qgcm_hip.slab import partition
    ref = tud._whole_ud(case)[1]
    g, P, so, reps = _slabs_sums(case, nranks)
    try:
        assert [x.xforc_edge_len(a) for x, a in zip(so.slabs, reps)] == [8 + 8 * so.cfg.nxpo] * nranks
        assert [x.xforc_msg_len(a) for x, a in zip(so.slabs, reps)] == [so.xforc_plan[0]["mom_len"]] * nranks
        M = tud._two_calls(so, reps, g)
        B = _bounds(P, partition(so.cfg.nypo, nranks), ns.fine(case, 1))
        _check_momentum("%s, %d ranks," % (case, nranks), so, M, ref, B, g, case, 1)
        for a in reps[1:]:
            for u, v in zip(a.get_state(), reps[0].get_state()):
                _same(u, v, "the replicas' pressures")
    finally:
        tsc._close(so, reps)
    assert not np.array_equal(ref["wekpa"], tud._whole_ud(case)[0]["wekpa"])  # the second state moved the outputs


@pytest.mark.parametrize("case,nranks", ns.BOX)
def test_box(case, nranks):
    """xf_cpl_tiny_ud on 1, 2, 3 ranks, xf_cpl_small_ud (ndxr 16) on 5, xf_odd5_ud on 3 (_check_momentum); on one rank
    every output is the whole-domain call's bits."""
    _run_case(case, nranks)


@pytest.mark.parametrize("case,nranks", ns.WIDE)
def test_wide_and_cyclic(case, nranks):
    """xf_cyc4_ud and xf_cycwide_ud (cyclic: the east-column expression, txisoc / txinoc, the box's cyclic wrap) on 2 and 3
    ranks; xf_wide_ud and xf_edge_ud on 2 (nxpo = 321 and 257: second blocks of the copy kernels).  test_box's assertions."""
    _run_case(case, nranks)


# ---- the heat half on ---------------------------------------------------------------------------------------------
_hstress = {}


def _heat_stress(case, ref):
    """The fine stress of a heat fixture's state with the shear term, from numpy_xforc's text with the default weight
    tables (what xforc_setup builds without `tables`): the bounds' magnitudes.  Held to the whole-domain device call's
    uekat at 1e-9 of its maximum, so that the magnitudes are those of the run under test."""
    if case not in _hstress:
        from qgcm_hip import hostinit
        g, P, oc, at = tsc._configs(case)
        tabs = hostinit.bcuini(P["ndxr"], at.bccoat, at.dya)
        Px = dict(P, tau_udiff=1)
        txf, tyf, hxofac, uvekfc = ns._ns["_fine_stress"](g["in_pam"][:, :, 0], g["in_pom"], tabs, Px)
        D = ns.dims(P["nyta"], P["ndxr"], P["ny1"], P["nyaooc"])
        ue = ns.nx_coarse(D, P["nxta"], txf, tyf, uvekfc)["uekat"]
        assert np.abs(ue - ref["uekat"]).max() <= 1e-9 * np.abs(ref["uekat"]).max()
        _hstress[case] = (txf, tyf, ns.wektaor(txf, tyf, hxofac), uvekfc)
    return _hstress[case]


def _heat_slabs_sums(case, nranks):
    """test_gpu_slab_coupled._slabbed, then - before anything has run - the set-up again with the owner-computed sums."""
    g, P, so, reps = tsc._slabbed(case, nranks, heat=False)
    so.xforc_setup(reps, udiff_sums=True, **tsc._mkw(P))
    so.xforc_heat_setup(tsc._heat_cfg(P), **tsc._hkw(g))
    return g, P, so, reps


def _check_heat(case, nranks, so, reps, g, P):
    """Two xforc() calls; the second against the whole-domain call with tau_udiff = True: the momentum half as
    _check_momentum; the heat half at DESIGN 6o's bars (tests/test_gpu_slab_coupled.py:_check_xforc): fnetoc and the
    cells no seam cuts by bits, cut cells and the three monitors within 2 n 2^-53 sum|terms|, replicas bit-equal."""
    from qgcm_hip.slab import partition
    oc, ref = so.cfg, tud._whole_heat_ud(case)
    N = nh.restated(case)[("x", 0)]
    so.xforc()
    so.xforc()
    M, H = so.xforc_get(), so.xforc_heat_get()
    tsc._replicas_equal(reps, case)
    B = _bounds(P, partition(oc.nypo, nranks), _heat_stress(case, ref))
    _check_momentum("%s, %d ranks, heat half on," % (case, nranks), so, M, ref, B)
    cut = tsc._cut_cells(oc, P, nranks)
    assert (cut.any() and not cut.all()) if nranks > 1 else not cut.any()
    blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
    land = ~N["ocean"]
    for r, (x, h) in enumerate(zip(so.slabs, H)):
        tag = "%s, %d ranks, rank %d: " % (case, nranks, r)
        tr = slice(x.joff, x.joff + x.nyl - 1)
        _same(h["fnetoc"], ref["fnetoc"][:, tr], tag + "fnetoc")
        _same(h["fnetoc"], g["x0_fnetoc"][:, tr], tag + "fnetoc against the fixture")
        fa = h["fnetat"]
        assert not np.isnan(fa).any()
        _same(fa, H[0]["fnetat"], tag + "fnetat against rank 0")
        _same(fa[land], ref["fnetat"][land], tag + "fnetat over land")
        _same(fa[blk][:, ~cut], ref["fnetat"][blk][:, ~cut], tag + "fnetat over the cells no seam cuts")
        if cut.any():
            bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * N["cell_abs"][:, cut]
            diff = np.abs(fa[blk][:, cut] - ref["fnetat"][blk][:, cut])
            assert np.all(diff <= bound), (tag, diff.max(), (diff / bound).max())
        assert h["arlaav"] == ref["arlaav"], tag
        for f in ("slhfav", "oradav", "arocav"):
            b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
            assert abs(h[f] - ref[f]) <= b, (tag, f, h[f], ref[f], b)
            assert h[f] == H[0][f], (tag, f)


@pytest.mark.parametrize("case,nranks", [("heat_cpl_tiny", 3), ("heat_cyc72", 2)])
def test_heat_half_on(case, nranks):
    """The heat fixtures' geometry and state (their pom is not zero) with both halves on (_check_heat)."""
    g, P, so, reps = _heat_slabs_sums(case, nranks)
    try:
        _check_heat(case, nranks, so, reps, g, P)
    finally:
        tsc._close(so, reps)


@pytest.mark.parametrize("var,val", [("QGCM_HIP_THOMAS_SLAB_SEG_ROWS", "7"), ("QGCM_HIP_ROW_SPLIT", "2")])
def test_forced_layouts(monkeypatch, var, val):
    """The channel on two ranks with the slabs' columns forced into segments, and with the rows forced into two sub-rows:
    the edge pack and the local copy read such slabs' pressure as any other."""
    case, nranks = "heat_cyc72", 2
    ref = tud._whole_heat_ud(case)  # (the whole-domain oracle keeps its own layout: computed before the variable is set)
    monkeypatch.setenv(var, val)  # read by qgcm_hip_set_grid
    g, P, so, reps = _heat_slabs_sums(case, nranks)
    try:
        if var.endswith("SEG_ROWS"):
            assert len(so.slabs[0].thomas_plan()) == 2, [x.thomas_plan() for x in so.slabs]
        else:
            assert all(x.row_plan() == (2, 144) for x in so.slabs), [x.row_plan() for x in so.slabs]
        assert ref is tud._whole_heat_ud(case)
        _check_heat(case, nranks, so, reps, g, P)
    finally:
        tsc._close(so, reps)


# ---- a coupled window ---------------------------------------------------------------------------------------------
def _window_sums(nranks):
    """test_gpu_slab_udiff._window_ud with the owner-computed sums: cpl_tiny, both mixed layers and the heat half, NWIN
    atmospheric steps = three ocean steps."""
    P = nh.params(nh.load("heat_cpl_tiny"))
    so, reps = tsc._cpl_tiny(nranks)
    try:
        so.xforc_setup(reps, udiff_sums=True)
        so.xforc_heat_setup(tsc._heat_cfg(P))
        so.coupled_steps(1, NWIN, NSTR, xforc=True)
        for x in so.slabs:
            x.sync()
        tsc._replicas_equal(reps, "window on %d ranks" % nranks)
        res = tsc._collect(*tsc._gather(so), reps[-1])
    finally:
        tsc._close(so, reps)
    assert all(np.isfinite(v).all() for k in res for v in (res[k] if isinstance(res[k], list) else [res[k]]))
    return res


def test_coupled_window():
    """A window of three ocean steps with both mixed layers: on one rank bitwise the whole-domain coupled_steps with
    tau_udiff = True; on three ranks within the bars of test_gpu_slab_coupled.py:_window_close against the whole-domain
    window."""
    ref = tud._window_ud(0)
    one = _window_sums(1)
    for k in ("ocean", "sst", "atmos", "aml"):
        for i, (x, y) in enumerate(zip(one[k], ref[k])):
            _same(x, y, "window, one rank: %s %d" % (k, i))
    _same(one["entat"], ref["entat"], "entat")
    tsc._window_close(_window_sums(3), ref, "window with the owner-computed sums on 3 ranks")


# ---- the refusals, the way back, the lengths ------------------------------------------------------------------------------
def test_refusals_and_the_way_back():
    """The flag beside another mode, part before an edge assemble, assemble and combine with another nranks, the set-up on
    a pair that is banded or gathers, with a plan whose rows are not the slab's or with a rank of 3 rows, and the other
    modes' set-ups on a pair in this mode are refused, naming the reason; after the refusals a valid call gives the bits
    of a run that met none.  The edge message is shorter than the gather's on the same slabs.  Then xforc_setup without
    the flag on the same handles: the outputs are bitwise the whole-domain shear-free ones."""
    from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, xforc, xforc_get, xforc_setup
    from qgcm_hip.lib import check
    from qgcm_hip.slab import partition
    from test_gpu_xforc import _load_state, _setup_kw
    case, nranks = "xf_cpl_tiny_ud", 2
    g, P, so, reps = _slabs_sums(case, nranks)
    extra = []
    try:
        x, a = so.slabs[0], reps[0]
        L = x.L
        kw = dict(tables=nx.tables(g), **tud._kw(P))
        rows = partition(so.cfg.nypo, nranks)
        B = _bounds(P, rows, ns.fine(case, 1))
        for bad in (dict(bands=True), dict(udiff_gather=True), dict(tau_udiff=True)):
            with pytest.raises(ValueError, match="udiff_sums = True excludes"):
                so.xforc_setup(reps, udiff_sums=True, **dict(kw, **bad))
        send, gath = so._xf_bufs
        es, eg = so._xf_edge_bufs
        ps, pg, pe = [ctypes.c_void_p(t[0].data_ptr()) for t in (send, gath, eg)]
        tud._load(so, reps, g, 0)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_part: the edge rows have not been assembled for this call"):
            check(L.qgcm_hip_xforc_slab_part(x.h, a.h, ps))
        so.xforc()
        with pytest.raises(QgcmHipError, match="the edge rows have not been assembled for this call"):
            check(L.qgcm_hip_xforc_slab_part(x.h, a.h, ps))  # (the part cleared the flag)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_edge_assemble: nranks = 3, the sums were set up for 2 ranks"):
            check(L.qgcm_hip_xforc_slab_edge_assemble(x.h, a.h, pe, 3))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_combine: nranks = 3, the sums were set up for 2 ranks"):
            check(L.qgcm_hip_xforc_slab_combine(x.h, a.h, pg, 3))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_bands: this pair runs the owner-computed sums"):
            x.xforc_bands_init(a, (1, 5), 5)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_udiff: this pair runs the owner-computed sums"):
            x.xforc_udiff_init(a, 19, nranks)
        with pytest.raises(QgcmHipError, match="rank 0 of the plan owns ocean rows 1..18, this slab owns 1..19"):
            x.xforc_sums_init(a, [(1, 18), (19, 37)])
        with pytest.raises(QgcmHipError, match="rank 2 owns 3 ocean rows, fewer than 4"):
            x.xforc_sums_init(a, [(1, 19), (20, 34), (35, 37)])
        b = AtmosModel(a.cfg)
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_sums: qgcm_hip_xforc_slab_init has not been called"):
            x.xforc_sums_init(b, rows)
        o = OceanModel(so.cfg)
        extra.append(o)
        xforc_setup(o, b, tables=nx.tables(g), **_setup_kw(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_edge_pack: qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_edge_pack(o.h, b.h, pe))
        # the refused calls changed nothing: the standing set-up gives the bits of a run that met none
        tud._load(so, reps, g, 1)
        so.xforc()
        _check_momentum("after the refusals,", so, so.xforc_get(), tud._whole_ud(case)[1], B, g, case, 1)
        edge = x.xforc_edge_len(a)
        # the gather mode on the same slabs: its message is the longer one; the sums are refused beside it
        so.xforc_setup(reps, udiff_gather=True, **kw)
        assert so._xf_edge_bufs is None
        assert edge == 8 + 8 * so.cfg.nxpo < x.xforc_pom_len(a) == 8 + 19 * so.cfg.nxpo
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_sums: this pair gathers the surface pressure"):
            x.xforc_sums_init(a, rows)
        so.xforc_setup(reps, bands=True, **kw)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_sums: this pair runs the banded atmosphere side"):
            x.xforc_sums_init(a, rows)
        # the way back: the shear-free, replicated set-up on the same handles
        so.xforc_setup(reps, **kw)
        assert so._xf_edge_bufs is None and so.xforc_plan is None
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_sums has not been called for this pair"):
            x.xforc_edge_len(a)
        so.xforc()
        xforc_setup(o, b, tables=nx.tables(g), **dict(_setup_kw(P), tau_udiff=False))
        _load_state(o, b, g, 1)
        xforc(o, b)
        free = xforc_get(o, b)
        tud._check_momentum("shear-free again,", so, so.xforc_get(), free)
        assert not np.array_equal(free["tauxo"], tud._whole_ud(case)[1]["tauxo"])
    finally:
        for m in extra:
            m.close()
        tsc._close(so, reps)
