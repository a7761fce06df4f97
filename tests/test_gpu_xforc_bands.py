"""The banded slab xforc on virtual ranks of one GPU: with bands = True rank r runs the atmosphere side only
on the fine rows its band of atmosphere rows and its slab need, and the bands travel in the one all-gather.  The oracle
is the replicated slab path on the same rank count - the existing code - by integer view.  Every banded case runs under
QGCM_HIP_XF_POISON=1 (NaN bytes in the fine arrays before every part: a read outside the computed windows shows), on
handles that have never run the replicated path, and is asserted on the SECOND of two xforc() calls with different pam
(stale rows of the first call would show).

Grids, the smallest at which each path can still go wrong: heat_cpl_tiny (16 x 12 cells, ocean 49 x 37, ndxr 12) on 1, 2,
3 and 5 ranks (5: bands of 3 and 2 rows, windows mostly halo); heat_odd5 (the xf_odd5 geometry, ndxr 5: half weights,
nijwid = ndxr + 1, the second rows of the line sums) on 3; heat_cpl_small (32 x 20, ocean 97 x 81, ndxr 16) on 5 - the
windowed k_xf_fine walks the x direction exactly as the whole call does (ceil(nxta / 8) workgroups per cell row), so a
tail workgroup exists where the whole call has one; at 32 and at 16 cells there is none, at heat_cyc72's 72 cells neither;
heat_cyc72 (a channel of 289 x 17, ndxr 4) on 2 and 3: the cyclic ocean's line sums owned by the first and the last slab.
Ranks on different GPUs are not tested here."""
import ctypes

import numpy as np
import pytest

import numpy_heat as nh
from test_gpu_slab_coupled import (ATM_FIELDS, NSTR, NWIN, _atmos, _bits, _check_xforc, _close, _collect, _configs, _consts,
                                   _cpl_tiny, _gather, _heat_cfg, _hkw, _mkw, _reference, _replicas_equal, _same, _window)

pytestmark = pytest.mark.gpu

CASES = [("heat_cpl_tiny", 1), ("heat_cpl_tiny", 2), ("heat_cpl_tiny", 3), ("heat_cpl_tiny", 5), ("heat_odd5", 3),
         ("heat_cpl_small", 5), ("heat_cyc72", 2), ("heat_cyc72", 3)]
LINES = ("txisat", "txinat", "txisoc", "txinoc")
OCEAN = ("tauxo", "tauyo", "wekto", "wekpo")


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    monkeypatch.setenv("QGCM_HIP_XF_POISON", "1")  # read by qgcm_hip_xforc_slab_bands


def _slabbed(case, nranks, bands, heat=True):
    """test_gpu_slab_coupled._slabbed with the choice of the atmosphere side: fresh handles, the fixture's state."""
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
    so.xforc_setup(reps, tau_udiff=False, bands=bands, **_mkw(P))
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), **_hkw(g))
    return g, P, so, reps


def _second_pressure(g):
    """Another pa, pam for the second call: the fixture's plus a smooth pattern of a tenth of its size, periodic in x."""
    out = []
    for k, name in enumerate(("in_pa", "in_pam")):
        p = np.array(g[name])
        nx, ny, nl = p.shape
        i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        pat = np.sin(2.0 * np.pi * (2 + k) * i / (nx - 1)) * np.cos(3.0 * np.pi * j / (ny - 1) + 0.3 * k)
        out.append(np.asfortranarray(p + 0.1 * np.abs(p).max() * pat[:, :, None] * (1.0 + 0.25 * np.arange(nl))))
    return out


def _two_calls(case, nranks, bands):
    """xforc(), the second pressure on every replica, xforc(): the outputs of the second call per rank."""
    g, P, so, reps = _slabbed(case, nranks, bands)
    try:
        so.xforc()
        pa, pam = _second_pressure(g)
        for a in reps:
            a.sync()
            a.set_state(po=pa, pom=pam)
        so.xforc()
        out = [dict(m, **h) for m, h in zip(so.xforc_get(), so.xforc_heat_get())]
        _replicas_equal(reps, "%s on %d ranks, bands %s" % (case, nranks, bands))
        plan = so.xforc_plan
    finally:
        _close(so, reps)
    return out, plan


@pytest.mark.parametrize("case,nranks", CASES)
def test_banded_is_the_replicated_path(case, nranks):
    """The second of two xforc() calls, banded under poison against replicated, same rank count: tauxa, tauya, uekat,
    vekat, wekta, wekpa, txisat, txinat, txisoc, txinoc, tauxo, tauyo, wekto, wekpo, fnetoc, fnetat and the four
    monitors by integer view on every rank; the replicas' pa, ast, hmixa (state) and fnetat, wekpa (outputs) bit-equal
    across ranks; no NaN anywhere."""
    ref, none = _two_calls(case, nranks, False)
    got, plan = _two_calls(case, nranks, True)
    assert none is None and len(plan) == nranks
    if nranks == 5 and case == "heat_cpl_tiny":
        assert [p["band"][1] - p["band"][0] + 1 for p in plan] == [3, 3, 3, 2, 2]
    if case == "heat_cyc72":
        assert "txisoc" in plan[0]["own"] and "txinoc" in plan[-1]["own"]
        assert sum(len(p["own"]) for p in plan) == 4
    if nranks > 1:  # the mode computes less: no rank's window is the whole fine grid
        P = nh.params(nh.load(case))
        for p in plan:
            assert sum(f1 - f0 + 1 for f0, f1 in p["fine"]) < P["nyta"] * P["ndxr"] + 1, p
    for r, (m, o) in enumerate(zip(got, ref)):
        tag = "%s, %d ranks, rank %d: " % (case, nranks, r)
        for f in ATM_FIELDS + OCEAN + ("fnetoc", "fnetat"):
            assert not np.isnan(m[f]).any(), tag + f + " holds a NaN"
            _same(m[f], o[f], tag + f)
        for f in LINES + tuple(nh.HEAT_SCALARS):
            assert not np.isnan(m[f]), tag + f
            assert _bits(m[f]) == _bits(o[f]), (tag, f, m[f], o[f])
        for f in ("fnetat", "wekpa"):
            _same(m[f], got[0][f], tag + f + " against rank 0")
    if case == "heat_cyc72":
        assert got[0]["txisoc"] != 0.0 and got[0]["txinoc"] != 0.0
    # the second call moved the outputs: the first call's rows would not pass for the second's
    assert not np.array_equal(ref[0]["wekpa"], _reference(case)["wekpa"])


def test_banded_against_the_fixture():
    """heat_cpl_tiny on three banded ranks, the first call: test_gpu_slab_coupled's own assertions (_check_xforc) - the
    whole-domain device result by integer view, uekat, vekat, wekta, fnetoc and fnetat over land the fixture's by integer
    view, cut cells and monitors within their reordering bounds."""
    case, nranks = "heat_cpl_tiny", 3
    g, P, so, reps = _slabbed(case, nranks, True)
    try:
        _check_xforc(case, nranks, so, reps, g, P)
    finally:
        _close(so, reps)


def test_banded_window():
    """cpl_tiny, coupled_steps(1, 9, 3, xforc=True) with both mixed layers and the heat half on three banded ranks: the
    ocean state, the sst, pa, ast and every other field the window moves end bit-equal to the replicated window."""
    nranks = 3
    ref = _window(nranks)  # (test_gpu_slab_coupled's replicated window; computed once and shared)
    so, reps = _cpl_tiny(nranks)
    try:
        P = nh.params(nh.load("heat_cpl_tiny"))
        so.xforc_setup(reps, tau_udiff=False, bands=True)  # (set up again before anything has run)
        so.xforc_heat_setup(_heat_cfg(P))
        so.coupled_steps(1, NWIN, NSTR, xforc=True)
        for x in so.slabs:
            x.sync()
        _replicas_equal(reps, "banded window")
        got = _collect(*_gather(so), reps[-1])
    finally:
        _close(so, reps)
    for k in ("ocean", "sst", "atmos", "aml"):
        for i, (x, y) in enumerate(zip(got[k], ref[k])):
            assert np.isfinite(x).all()
            _same(x, y, "banded window: %s %d" % (k, i))
    _same(got["entat"], ref["entat"], "entat")


def test_refusals_and_default():
    """qgcm_hip_xforc_slab_bands refuses, naming the reason and changing nothing: a band outside 1 .. nypa, a row count
    shorter than the band, a pair that qgcm_hip_xforc_slab_init has not set up; the combine refuses a rank count other
    than the plan's; the part refuses a missing buffer.  bands = False still has no message without the heat half; the
    banded pair has one.  After the refusals the standing banded set-up gives the whole-domain bits."""
    from qgcm_hip import AtmosModel, QgcmHipError
    from qgcm_hip.lib import check
    case, nranks = "heat_cpl_tiny", 2
    g, P, so0, reps0 = _slabbed(case, nranks, False, heat=False)
    try:
        assert [x.xforc_msg_len(a) for x, a in zip(so0.slabs, reps0)] == [0, 0] and so0.xforc_plan is None
    finally:
        _close(so0, reps0)
    g, P, so, reps = _slabbed(case, nranks, True, heat=False)
    extra = []
    try:
        x, a = so.slabs[0], reps[0]
        L, nypa = x.L, a.cfg.nypa
        plan = so.xforc_plan
        mom = 8 + 6 * plan[0]["nrow"] * a.cfg.nxpa
        assert [y.xforc_msg_len(b) for y, b in zip(so.slabs, reps)] == [mom, mom] == [p["mom_len"] for p in plan]
        for a0, a1 in ((0, 3), (5, nypa + 1), (4, 3)):
            with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_bands: the band %d..%d lies outside" % (a0, a1)):
                check(L.qgcm_hip_xforc_slab_bands(x.h, a.h, a0, a1, plan[0]["nrow"], nranks))
        with pytest.raises(QgcmHipError, match="does not hold the band"):
            check(L.qgcm_hip_xforc_slab_bands(x.h, a.h, 1, 7, 6, nranks))
        b = AtmosModel(a.cfg)
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_xforc_slab_bands: qgcm_hip_xforc_slab_init has not been called"):
            check(L.qgcm_hip_xforc_slab_bands(x.h, b.h, 1, 7, 7, nranks))
        with pytest.raises(QgcmHipError, match="not the one qgcm_hip_xforc_slab_init was called with"):
            check(L.qgcm_hip_xforc_slab_bands(so.slabs[1].h, a.h, 1, 7, 7, nranks))
        send, gath = so._xf_bufs
        with pytest.raises(QgcmHipError, match="the bands were set up for 2 ranks"):
            check(L.qgcm_hip_xforc_slab_combine(x.h, a.h, ctypes.c_void_p(gath[0].data_ptr()), 3))
        with pytest.raises(QgcmHipError, match="the bands are set up: send_dev must hold"):
            check(L.qgcm_hip_xforc_slab_part(x.h, a.h, None))
        so.xforc()
        ref = _reference(case)
        for y, m in zip(so.slabs, so.xforc_get()):
            for f in ATM_FIELDS:
                _same(m[f], ref[f], f + " after the refusals")
            for f in ("txisat", "txinat"):
                assert m[f] == ref[f], f
            _same(m["tauxo"], ref["tauxo"][:, y.joff:y.joff + y.nyl], "tauxo after the refusals")
    finally:
        for m in extra:
            m.close()
        _close(so, reps)
