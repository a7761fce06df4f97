"""tau_udiff on a y-slab ocean on virtual ranks of one GPU: with udiff_gather = True every xforc() first
gathers the slabs' owned rows of pom(:,:,1) and assembles the basin's layer on every rank; the stress kernels then run on
it unchanged.  The oracle is the whole-domain device call set up with tau_udiff = True on the same data - itself pinned
bitwise to the reference by the _ud fixtures (tests/test_gpu_xforc.py) - by integer view; the pointwise fields are also
held to the fixtures, the line integrals to test_golden's bound.  Every case runs under QGCM_HIP_XF_POISON=1 (NaN bytes
in the assembled array before every assemble, and in the fine arrays of a banded part), on handles that never ran the
shear-free path, and is asserted on the SECOND of two xforc() calls, with the fixture's two states.  Ranks on different
GPUs are not tested here."""
import ctypes

import numpy as np
import pytest

import numpy_heat as nh
import numpy_xforc as nx
import test_gpu_slab_coupled as tsc
from numpy_slab_udiff import BOX, HDR, WIDE, configs
from test_gpu_slab_coupled import ATM_FIELDS, NSTR, NWIN, _bits, _same
from test_gpu_xforc import _load_state, _models, _setup_kw

pytestmark = pytest.mark.gpu

LINES = ("txisat", "txinat", "txisoc", "txinoc")


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    monkeypatch.setenv("QGCM_HIP_XF_POISON", "1")  # read by qgcm_hip_xforc_slab_udiff and qgcm_hip_xforc_slab_bands


_cst, _wref = {}, {}


def _consts_ud(case, oc):
    """Once per fixture: the start-up constants on the global grid (a box basin's homogeneous solutions from a
    whole-domain handle's Helmholtz solver)."""
    if case not in _cst:
        from qgcm_hip import OceanModel
        from qgcm_hip.slab import global_consts
        if oc.cyclic:
            _cst[case] = global_consts(oc)
        else:
            m = OceanModel(oc)
            try:
                _cst[case] = global_consts(oc, m.helmholtz)
            finally:
                m.close()
    return _cst[case]


def _whole_ud(case):
    """The whole-domain xforc with tau_udiff = True on the fixture's two states, one after the other: [R0, R1].  Computed
    once per fixture, shared, unchanged."""
    if case not in _wref:
        from qgcm_hip import xforc, xforc_get
        g, P, o, a = _models(case)
        assert P["tau_udiff"] == 1
        try:
            out = []
            for s in range(2):
                _load_state(o, a, g, s)
                xforc(o, a)
                out.append(xforc_get(o, a))
            _wref[case] = out
        finally:
            o.close()
            a.close()
    return _wref[case]


def _slabs_ud(case, nranks, bands, udiff=True):
    """SlabOcean of `nranks` virtual ranks on fresh handles, one replica of the atmosphere each, the momentum half set up
    with the fixture's tables."""
    import torch
    from qgcm_hip import AtmosModel
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, partition
    g, P, oc, at = configs(case)
    consts = _consts_ud(case, oc)
    slabs = [HipSlab(oc, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    so = SlabOcean(oc, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
    reps = [AtmosModel(at) for _ in slabs]
    so.xforc_setup(reps, tables=nx.tables(g), bands=bands, udiff_gather=udiff, **_kw(P))
    return g, P, so, reps


def _kw(P):
    kw = _setup_kw(P)
    del kw["tau_udiff"]
    return kw


def _load(so, reps, g, s):
    """State s of the fixture: the lagged layer-1 pressures into both time levels, the slabs' local rows of the ocean's."""
    from qgcm_hip.slab import slab_slice
    pa = np.zeros(g["in%d_pam1" % s].shape + (3,), order="F")
    pa[:, :, 0] = g["in%d_pam1" % s]
    po = np.zeros(g["in%d_pom1" % s].shape + (3,), order="F")
    po[:, :, 0] = g["in%d_pom1" % s]
    for a in reps:
        a.sync()
        a.set_state(po=pa, pom=pa)
    for x in so.slabs:
        x.sync()
        sl = slab_slice(so.cfg.nypo, x.g0, x.g1)
        x.set_state(po=po[:, sl, :], pom=po[:, sl, :])


def _two_calls(so, reps, g):
    _load(so, reps, g, 0)
    so.xforc()
    _load(so, reps, g, 1)
    so.xforc()
    return so.xforc_get()


def _check_momentum(tag, so, M, ref, g=None, case=None, s=1):
    """Every field of xforc_get on every rank against the whole-domain result `ref`: the atmosphere's fields and the four
    line integrals whole, the ocean's on the slab's rows (wekpo: but the outermost halo row of a seam, which no kernel
    reads); replicas bit-equal; no NaN.  With a fixture: the pointwise fields by integer view, the integrals within
    test_golden's bound 2 n 2^-53 sum|terms| dxo."""
    oc = so.cfg
    for r, (x, m) in enumerate(zip(so.slabs, M)):
        t = "%s rank %d: " % (tag, r)
        pr, tr = slice(x.joff, x.joff + x.nyl), slice(x.joff, x.joff + x.nyl - 1)
        lo = 1 if x.g0 > 1 else 0
        hi = x.nyl - (1 if x.g1 < oc.nypo else 0)
        assert lo <= x.jlo - 1 and hi >= x.jhi
        for f in ATM_FIELDS:
            assert not np.isnan(m[f]).any(), t + f + " holds a NaN"
            _same(m[f], ref[f], t + f)
            _same(m[f], M[0][f], t + f + " against rank 0")
        for f in ("tauxo", "tauyo"):
            assert not np.isnan(m[f]).any(), t + f + " holds a NaN"
            _same(m[f], ref[f][:, pr], t + f)
        assert not np.isnan(m["wekto"]).any() and not np.isnan(m["wekpo"][:, lo:hi]).any(), t
        _same(m["wekto"], ref["wekto"][:, tr], t + "wekto")
        _same(m["wekpo"][:, lo:hi], ref["wekpo"][:, x.joff + lo:x.joff + hi], t + "wekpo")
        for f in LINES:
            assert _bits(m[f]) == _bits(ref[f]), (t, f, m[f], ref[f])
        if oc.cyclic:
            assert m["txisoc"] != 0.0 and m["txinoc"] != 0.0
        if so.P == 1:
            _same(m["wekpo"], ref["wekpo"], t + "wekpo, a lone slab")
        if g is not None:
            N = nx.restated(case, s)
            for f in ATM_FIELDS:
                _same(m[f], g["out%d_%s" % (s, f)], t + f + " against the fixture")
            for f in ("tauxo", "tauyo"):
                _same(m[f], g["out%d_%s" % (s, f)][:, pr], t + f + " against the fixture")
            _same(m["wekto"], g["out%d_wekto" % s][:, tr], t + "wekto against the fixture")
            _same(m["wekpo"][:, lo:hi], g["out%d_wekpo" % s][:, x.joff + lo:x.joff + hi], t + "wekpo against the fixture")
            for f in LINES:
                fx = float(g["out%d_%s" % (s, f)])
                bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * nx.params(g)["dxo"]
                print("%s%s: slabs %.17e fixture %.17e |diff| %.3e bound %.3e" % (t, f, m[f], fx, abs(m[f] - fx), bound))
                assert abs(m[f] - fx) <= bound, (t, f, m[f], fx, bound)


def _run_case(case, nranks, bands):
    ref = _whole_ud(case)[1]
    g, P, so, reps = _slabs_ud(case, nranks, bands)
    try:
        nrow = max(x.g1 - x.g0 + 1 for x in so.slabs)
        assert [x.xforc_pom_len(a) for x, a in zip(so.slabs, reps)] == [HDR + nrow * so.cfg.nxpo] * nranks
        M = _two_calls(so, reps, g)
        _check_momentum("%s, %d ranks, bands %s," % (case, nranks, bands), so, M, ref, g, case, 1)
        for a in reps[1:]:
            for u, v in zip(a.get_state(), reps[0].get_state()):
                _same(u, v, "the replicas' pressures")
    finally:
        tsc._close(so, reps)
    # the second state moved the outputs: the first call's rows would not pass for the second's
    assert not np.array_equal(ref["wekpa"], _whole_ud(case)[0]["wekpa"])


@pytest.mark.parametrize("bands", [False, True], ids=["replicated", "banded"])
@pytest.mark.parametrize("case,nranks", BOX)
def test_box(case, nranks, bands):
    """xf_cpl_tiny_ud on 1, 2, 3 ranks, xf_cpl_small_ud (ndxr 16) on 5, xf_odd5_ud on 3, replicated and banded: every field
    of xforc_get bit-equal to the whole-domain device call with tau_udiff = True, slab rows against the matching rows;
    the pointwise fields bit-equal to the fixture, the integrals within test_golden's bound; replicas bit-equal; no NaN."""
    _run_case(case, nranks, bands)


@pytest.mark.parametrize("bands", [False, True], ids=["replicated", "banded"])
@pytest.mark.parametrize("case,nranks", WIDE)
def test_wide_and_cyclic(case, nranks, bands):
    """xf_cyc4_ud and xf_cycwide_ud (cyclic: the east-column expression, txisoc / txinoc) on 2 and 3 ranks; xf_wide_ud and
    xf_edge_ud on 2 (nxpo = 321 and 257: second blocks of the copy kernels).  test_box's assertions."""
    _run_case(case, nranks, bands)


# ---- the heat half on ---------------------------------------------------------------------------------------------
_href = {}


def _whole_heat_ud(case):
    """test_gpu_slab_coupled._whole with tau_udiff = True: one whole-domain xforc() on the heat fixture's state, whose pom
    is not zero; both halves' outputs.  Computed once, shared, unchanged."""
    if case not in _href:
        from qgcm_hip import OceanModel, oml_preset, xforc, xforc_get, xforc_heat_get, xforc_heat_setup, xforc_setup
        g, P, oc, at = tsc._configs(case)
        assert np.abs(g["in_pom"]).max() > 1.0
        o = OceanModel(oc)
        a = tsc._atmos(g, P, at)
        try:
            xforc_setup(o, a, tau_udiff=True, **tsc._mkw(P))
            o.oml_init(oml_preset(oc))
            xforc_heat_setup(o, a, tsc._heat_cfg(P), **tsc._hkw(g))
            o.set_state(*tsc._consts(case, oc)[1])
            o.set_scalars(tsc._consts(case, oc)[2])
            o.oml_set_state(sst=g["in_sstm"], sstm=g["in_sstm"])
            xforc(o, a)
            _href[case] = dict(xforc_get(o, a), **xforc_heat_get(o, a))
        finally:
            o.close()
            a.close()
    return _href[case]


def _heat_slabs_ud(case, nranks, bands):
    """test_gpu_slab_coupled._slabbed, then - before anything has run - the set-up again with the shear term."""
    g, P, so, reps = tsc._slabbed(case, nranks, heat=False)
    so.xforc_setup(reps, bands=bands, udiff_gather=True, **tsc._mkw(P))
    so.xforc_heat_setup(tsc._heat_cfg(P), **tsc._hkw(g))
    return g, P, so, reps


def _check_heat(case, nranks, so, reps, g, P):
    """Two xforc() calls; the second against the whole-domain call with tau_udiff = True: the momentum half by bits
    (_check_momentum); the heat half at DESIGN 6o's bars (tests/test_gpu_slab_coupled.py:_check_xforc): fnetoc and the
    cells no seam cuts by bits, cut cells and the three monitors within 2 n 2^-53 sum|terms|, replicas bit-equal."""
    oc, ref = so.cfg, _whole_heat_ud(case)
    N = nh.restated(case)[("x", 0)]
    so.xforc()
    so.xforc()
    M, H = so.xforc_get(), so.xforc_heat_get()
    tsc._replicas_equal(reps, case)
    _check_momentum("%s, %d ranks, heat half on," % (case, nranks), so, M, ref)
    assert not np.array_equal(ref["tauxo"], tsc._reference(case)["tauxo"])  # (the shear term is in the oracle)
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
            print("%sfnetat over cut cells: max |diff| %.3e, largest |diff| / bound %.3f" % (tag, diff.max(), (diff / bound).max()))
            assert np.all(diff <= bound), (tag, diff.max(), (diff / bound).max())
        assert h["arlaav"] == ref["arlaav"], tag
        for f in ("slhfav", "oradav", "arocav"):
            b = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f]
            print("%s%s: slabs %.17e whole domain %.17e |diff| %.3e bound %.3e" % (tag, f, h[f], ref[f], abs(h[f] - ref[f]), b))
            assert abs(h[f] - ref[f]) <= b, (tag, f, h[f], ref[f], b)
            assert h[f] == H[0][f], (tag, f)


@pytest.mark.parametrize("bands", [False, True], ids=["replicated", "banded"])
@pytest.mark.parametrize("case,nranks", [("heat_cpl_tiny", 3), ("heat_cyc72", 2)])
def test_heat_half_on(case, nranks, bands):
    """The heat fixtures' geometry and state (their pom is not zero) with both halves on (_check_heat)."""
    g, P, so, reps = _heat_slabs_ud(case, nranks, bands)
    try:
        _check_heat(case, nranks, so, reps, g, P)
    finally:
        tsc._close(so, reps)


@pytest.mark.parametrize("var,val", [("QGCM_HIP_THOMAS_SLAB_SEG_ROWS", "7"), ("QGCM_HIP_ROW_SPLIT", "2")])
def test_forced_layouts(monkeypatch, var, val):
    """The channel on two ranks with the slabs' columns forced into segments, and with the rows forced into two sub-rows
    (tests/test_gpu_slab_coupled.py:test_xforc_slab_forced_plans): the pack reads such slabs' pressure as any other."""
    case, nranks = "heat_cyc72", 2
    ref = _whole_heat_ud(case)  # (the whole-domain oracle keeps its own layout: computed before the variable is set)
    monkeypatch.setenv(var, val)  # read by qgcm_hip_set_grid
    g, P, so, reps = _heat_slabs_ud(case, nranks, False)
    try:
        if var.endswith("SEG_ROWS"):
            assert len(so.slabs[0].thomas_plan()) == 2, [x.thomas_plan() for x in so.slabs]
        else:
            assert all(x.row_plan() == (2, 144) for x in so.slabs), [x.row_plan() for x in so.slabs]
        assert ref is _whole_heat_ud(case)
        _check_heat(case, nranks, so, reps, g, P)
    finally:
        tsc._close(so, reps)


# ---- a coupled window ---------------------------------------------------------------------------------------------
_win = {}


def _window_ud(nranks, bands=False):
    """test_gpu_slab_coupled._window with the shear term: cpl_tiny, both mixed layers and the heat half, NWIN atmospheric
    steps = three ocean steps; nranks = 0: the whole-domain models with tau_udiff = True."""
    key = (nranks, bands)
    if key in _win:
        return _win[key]
    P = nh.params(nh.load("heat_cpl_tiny"))
    if nranks == 0:
        from qgcm_hip import coupled_steps, xforc_heat_setup, xforc_setup
        o, a = tsc._cpl_tiny(0)
        try:
            xforc_setup(o, a, tau_udiff=True)  # (set up again before anything has run)
            xforc_heat_setup(o, a, tsc._heat_cfg(P))
            coupled_steps(o, a, 1, NWIN, NSTR, xforc=True)
            o.sync()
            res = tsc._collect(o.get_state(), o.oml_get_state(), a)
        finally:
            o.close()
            a.close()
    else:
        so, reps = tsc._cpl_tiny(nranks)
        try:
            so.xforc_setup(reps, bands=bands, udiff_gather=True)
            so.xforc_heat_setup(tsc._heat_cfg(P))
            so.coupled_steps(1, NWIN, NSTR, xforc=True)
            for x in so.slabs:
                x.sync()
            tsc._replicas_equal(reps, "window on %d ranks" % nranks)
            res = tsc._collect(*tsc._gather(so), reps[-1])
        finally:
            tsc._close(so, reps)
    assert all(np.isfinite(v).all() for k in res for v in (res[k] if isinstance(res[k], list) else [res[k]]))
    _win[key] = res
    return res


def test_coupled_window():
    """A window of three ocean steps with both mixed layers: on one rank bitwise the whole-domain coupled_steps with
    tau_udiff = True; on three within the bars of test_gpu_slab_coupled's window test (_window_close), replicated and
    banded bit-equal to each other; and the shear term moves the window: the ocean differs from the shear-free one."""
    ref = _window_ud(0)
    one = _window_ud(1)
    for k in ("ocean", "sst", "atmos", "aml"):
        for i, (x, y) in enumerate(zip(one[k], ref[k])):
            _same(x, y, "window, one rank: %s %d" % (k, i))
    _same(one["entat"], ref["entat"], "entat")
    rep, ban = _window_ud(3), _window_ud(3, True)
    tsc._window_close(rep, ref, "window with the shear term on 3 ranks")
    for k in ("ocean", "sst", "atmos", "aml"):
        for i, (x, y) in enumerate(zip(ban[k], rep[k])):
            _same(x, y, "window, banded against replicated: %s %d" % (k, i))
    _same(ban["entat"], rep["entat"], "entat")
    free = tsc._window(0)
    assert not np.array_equal(ref["ocean"][0], free["ocean"][0])


# ---- the flag, the refusals, the way back -------------------------------------------------------------------------------
def test_the_shear_term_does_something():
    """xf_cpl_tiny_ud on two ranks: tauxo with udiff_gather = True differs from tauxo with the forcing set up shear-free
    at more than half the sea points (a silently ignored flag would pass every comparison of a zero pom)."""
    case, out = "xf_cpl_tiny_ud", []
    for udiff in (True, False):
        g, P, so, reps = _slabs_ud(case, 2, False, udiff=udiff)
        try:
            M = _two_calls(so, reps, g)
            out.append(np.concatenate([m["tauxo"][:, x.jlo - 1:x.jhi] for x, m in zip(so.slabs, M)], axis=1))
        finally:
            tsc._close(so, reps)
    assert out[0].shape == out[1].shape == (so.cfg.nxpo, so.cfg.nypo)
    frac = float((out[0] != out[1]).mean())
    print("tauxo differs at %.3f of the sea points" % frac)
    assert frac > 0.5
    _same(out[0], _whole_ud(case)[1]["tauxo"], "tauxo with the shear term")


def test_refusals_and_the_way_back():
    """tau_udiff = True alone is refused with the old text; part before assemble, assemble with another nranks, _udiff on
    a pair not set up for slabs and an nrow too small are refused, naming the reason; after the refusals a valid call
    gives the bits of a run that met none.  Then xforc_setup(..., udiff_gather=False) on the same handles: the outputs
    are bitwise the whole-domain shear-free ones, and no assemble is asked for."""
    from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, xforc, xforc_get, xforc_setup
    from qgcm_hip.lib import check
    case, nranks = "xf_cpl_tiny_ud", 2
    g, P, so, reps = _slabs_ud(case, nranks, False)
    extra = []
    try:
        x, a = so.slabs[0], reps[0]
        L = x.L
        send, gath = so._xf_pom_bufs
        ps, pg = [ctypes.c_void_p(t[0].data_ptr()) for t in (send, gath)]
        with pytest.raises(QgcmHipError, match="tau_udiff is not available with a y-slab ocean"):
            so.xforc_setup(reps, tables=nx.tables(g), tau_udiff=True, **_kw(P))
        with pytest.raises(ValueError, match="pass only udiff_gather"):
            so.xforc_setup(reps, tables=nx.tables(g), tau_udiff=True, udiff_gather=True, **_kw(P))
        _load(so, reps, g, 0)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_part: the surface pressure has not been assembled for this call"):
            check(L.qgcm_hip_xforc_slab_part(x.h, a.h, None))
        so.xforc()
        with pytest.raises(QgcmHipError, match="the surface pressure has not been assembled for this call"):
            check(L.qgcm_hip_xforc_slab_part(x.h, a.h, None))  # (the part cleared the flag)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_pom_assemble: nranks = 3, the shear term was set up for 2 ranks"):
            check(L.qgcm_hip_xforc_slab_pom_assemble(x.h, a.h, pg, 3))
        with pytest.raises(QgcmHipError, match="does not hold this slab's 19 owned rows"):
            check(L.qgcm_hip_xforc_slab_udiff(x.h, a.h, 18, nranks))
        with pytest.raises(QgcmHipError, match="nranks = 0"):
            check(L.qgcm_hip_xforc_slab_udiff(x.h, a.h, 19, 0))
        b = AtmosModel(a.cfg)
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_udiff: qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_udiff(x.h, b.h, 19, nranks))
        with pytest.raises(QgcmHipError, match="not the one qgcm_hip_xforc_slab_init was called with"):
            check(L.qgcm_hip_xforc_slab_udiff(so.slabs[1].h, a.h, 19, nranks))
        # a whole-domain pair is not set up for slabs
        o = OceanModel(so.cfg)
        extra.append(o)
        xforc_setup(o, b, tables=nx.tables(g), **_setup_kw(P))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_udiff: qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_udiff(o.h, b.h, 37, 1))
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_pom_pack: qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_pom_pack(o.h, b.h, ps))
        # the refused calls changed nothing: the standing set-up gives the whole-domain bits
        _load(so, reps, g, 1)
        so.xforc()
        _check_momentum("after the refusals,", so, so.xforc_get(), _whole_ud(case)[1], g, case, 1)
        # the way back: the shear-free set-up on the same handles
        so.xforc_setup(reps, tables=nx.tables(g), udiff_gather=False, **_kw(P))
        assert so._xf_pom_bufs is None
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_udiff has not been called for this pair"):
            x.xforc_pom_len(a)
        so.xforc()
        xforc_setup(o, b, tables=nx.tables(g), **dict(_setup_kw(P), tau_udiff=False))
        _load_state(o, b, g, 1)
        xforc(o, b)
        free = xforc_get(o, b)
        _check_momentum("shear-free again,", so, so.xforc_get(), free)
        assert not np.array_equal(free["tauxo"], _whole_ud(case)[1]["tauxo"])
    finally:
        for m in extra:
            m.close()
        tsc._close(so, reps)
