"""y-slabs whose rows are cut into segments (k_thomas_slab.h): slabs of more than 2048 interior rows, which
qgcm_hip_set_grid refused before, and - with QGCM_HIP_THOMAS_SLAB_SEG_ROWS - segments forced on the slabs of the small
basins the true reference pins.  The slabs are virtual ranks on one GPU (HipSlab / SlabOcean / LocalComm), the tall
basins the thin 49-column family of test_gpu_tall_columns.py, whose oracle runs are shared.  Every case asserts
thomas_plan() first: none can pass on the single-segment path.  Bars are those of the tests named in each docstring."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import test_gpu_areacfl as t_areacfl
import test_gpu_monitors as t_mon
from common import (FIELDS, GOLDEN, SNAPS, load_golden, make_oracle, preset, relerr, same_bits, scal_err, state_errs)
from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, config, hostinit, lib, oml_preset, synth
from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition, rccl_unique_id, slab_slice
from test_gpu_tall_columns import TOL_CALL, TOL_RUN, load_box, oracle_bsums, reference, tall_cfg

pytestmark = pytest.mark.gpu

VAR = "QGCM_HIP_THOMAS_SLAB_SEG_ROWS"


def interior_rows(cfg, g0, g1):
    """Rows of the slab g0..g1 that the tridiagonal solve owns: the two wall rows are nobody's."""
    return g1 - g0 + 1 - (1 if g0 == 1 else 0) - (1 if g1 == cfg.nypo else 0)


def make_slabs(cfg, consts, parts, seg_rows=0, **kw):
    """The slabs of `parts`, each asserted to be on the plan the rule gives for its rows - more than one segment, but
    for the one-segment ends of test_slab_tables_rebuilt_under_another_plan."""
    P = len(parts)
    slabs = []
    try:
        for r, (g0, g1) in enumerate(parts):
            slabs.append(HipSlab(cfg, consts, g0, g1, r, P, sync_each_call=kw.get("sync_each_call", True)))
            want = lib.thomas_segments(interior_rows(cfg, g0, g1), seg_rows)
            assert slabs[-1].thomas_plan() == want, (r, slabs[-1].thomas_plan(), want)
    except BaseException:
        for x in slabs:
            x.close()
        raise
    return slabs


def slab_ocean(cfg, slabs):
    return SlabOcean(cfg, slabs, LocalComm(len(slabs), after=torch.cuda.synchronize))


class Gathered:
    """What common.state_errs / scal_err ask of a model, from the slabs' owned rows."""

    def __init__(self, so):
        self.so = so

    def get_state(self):
        cfg = self.so.cfg
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in self.so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        return got

    def get_scalars(self):
        s = [x.get_scalars() for x in self.so.slabs]
        for other in s[1:]:
            assert np.array_equal(other, s[0])  # every rank runs the constraint algebra on the same numbers
        return s[0]


def close_all(slabs, *models):
    for x in slabs:
        x.close()
    for m in models:
        if m is not None:
            m.close()


def scatter_box(so, r, consts):
    cfg = r["cfg"]
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], r["po"])
    scal = hostinit.constr(cfg, consts["amatoc"], r["po"], r["po"])
    so.scatter_state(r["po"], r["po"], qo, qo, r["wek"], np.zeros_like(r["wek"]), np.zeros(cfg.nlo - 1), scal)


def check_vs_oracle(so, r, what):
    cfg = r["cfg"]
    g = Gathered(so)
    errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, g.get_state(), r["s12"])}
    se = scal_err(g, {"s12_scal": r["s12_scal"], "s12_po": r["s12"][0]}, "s12", cfg)
    print(what, "12 steps:", errs, "scalars %.3e" % se)
    assert all(v < TOL_RUN for v in errs.values()), errs
    assert se < 1e-11


# 1 - 3. slabs of more than 2048 rows -------------------------------------------------------------------------------------
def test_lone_tall_slab_vs_oracle():
    """tall_cfg(171), 2051 interior rows, as ONE slab (nranks = 1; the handle owns every row, so its plan is the
    whole-domain handle's three segments): 12 steps through the slab stages against the oracle at test_long_columns'
    1e-10 on the four fields, the constraint scalars by scal_err < 1e-11.  The slab phases refused such a handle."""
    r = reference(171)
    cfg = r["cfg"]
    slabs, m = [], OceanModel(cfg)
    try:
        consts = global_consts(cfg, m.helmholtz)
        slabs = make_slabs(cfg, consts, [(1, cfg.nypo)])
        assert [n for _, n in slabs[0].thomas_plan()] == [684, 684, 683]
        so = slab_ocean(cfg, slabs)
        scatter_box(so, r, consts)
        so.steps(12, s0=1)
        check_vs_oracle(so, r, "lone slab of 2053 rows,")
    finally:
        close_all(slabs, m)


def test_two_tall_slabs_vs_oracle_and_whole_handle():
    """tall_cfg(400), the 4801-row column of NAtl 1 km, as two slabs of 2401 / 2400 rows (2400 / 2399 interior: three
    segments each): one step against the whole-domain handle within 1e-10, as
    test_tall_column_whole_handle_vs_three_y_slabs asks, and 12 steps against the oracle at the bars above."""
    r = reference(400)
    cfg = r["cfg"]
    slabs, m = [], OceanModel(cfg)
    try:
        consts = global_consts(cfg, m.helmholtz)
        parts = partition(cfg.nypo, 2)
        assert [g1 - g0 + 1 for g0, g1 in parts] == [2401, 2400]
        slabs = make_slabs(cfg, consts, parts)
        assert [[n for _, n in x.thomas_plan()] for x in slabs] == [[800, 800, 800], [800, 800, 799]]
        so = slab_ocean(cfg, slabs)
        scatter_box(so, r, consts)
        load_box(m, r)
        m.steps(1, s0=1)
        so.steps(1, s0=1)
        errs = {f: (relerr(x, y), relerr(x, z)) for f, x, y, z in zip(FIELDS, Gathered(so).get_state(), m.get_state(), r["s1"])}
        print("one step, slabs vs whole handle, slabs vs oracle:", errs)
        assert all(a < 1e-10 and b < 1e-10 for a, b in errs.values()), errs
        so.steps(11, s0=2)
        check_vs_oracle(so, r, "two slabs of 4801 rows,")
    finally:
        close_all(slabs, m)


def test_a_tall_slab_among_ordinary_ones():
    """tall_cfg(342), 4105 rows, cut by hand into 2100 + 900 + 1105 rows: the first slab in segments (2099 interior rows
    under the default of 1024: three of 700 / 700 / 699), the second on 16 rows per thread, the third on the
    20-rows-per-thread form, each with its own plan around ONE exchange of unchanged length - the message format did
    not change.  12 steps against the oracle at the bars above."""
    r = reference(342)
    cfg = r["cfg"]
    slabs, m = [], OceanModel(cfg)
    try:
        consts = global_consts(cfg, m.helmholtz)
        parts = [(1, 2100), (2101, 3000), (3001, 4105)]
        assert cfg.nypo == 4105
        slabs = make_slabs(cfg, consts, parts)
        assert [len(x.thomas_plan()) for x in slabs] == [3, 1, 1]
        assert len({x.th_len for x in slabs}) == 1 and len({x.cst_len for x in slabs}) == 1
        assert slabs[0].th_len == 3 * cfg.nlo * (-(-(cfg.nxto + 1) // 16) * 16)  # TH_MSG * nl * ldw, as ever
        so = slab_ocean(cfg, slabs)
        scatter_box(so, r, consts)
        so.steps(12, s0=1)
        check_vs_oracle(so, r, "2100 + 900 + 1105 rows,")
    finally:
        close_all(slabs, m)


# 4. forced segments on the basins the true reference pins -------------------------------------------------------------------
# 37 rows as two slabs of 19 / 18: 18 / 17 interior rows.  7 = 2 * QGCM_HIP_THOMAS_SEG_MIN - 1, the smallest maximum the
# plan takes: three segments each (6, 6, 6 and 6, 6, 5); 10: two segments each, 9 + 9 and the unequal 9 + 8
@pytest.mark.parametrize("seg_rows", [7, 10])
@pytest.mark.parametrize("name", ["box_tiny", "box_tiny5", "cyc_tiny", "cyc_tiny6"])
def test_forced_segments_on_two_slabs_vs_reference(name, seg_rows, monkeypatch):
    """The committed snapshots of the true reference at the bars of test_forced_segments_whole_steps_vs_reference, on two
    slabs in forced segments.  Cyclic: the boundary line sums of qgcm_hip_get_bsums after the first step against the
    oracle (the bar of test_cyclic_column_past_2048_rows_vs_oracle: 1e-11 of each kind's maximum) on every rank."""
    cfg, g = preset(name), load_golden(name)
    monkeypatch.setenv(VAR, str(seg_rows))
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "not read by a slab")  # (a whole-domain handle would refuse it)
    nl = cfg.nlo
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, None if cfg.cyclic else o.helmholtz)
        parts = partition(cfg.nypo, 2)
        slabs = make_slabs(cfg, consts, parts, seg_rows)
        plans = [[n for _, n in x.thomas_plan()] for x in slabs]
        assert plans == ([[6, 6, 6], [6, 6, 5]] if seg_rows == 7 else [[9, 9], [9, 8]]), plans
        so = slab_ocean(cfg, slabs)
        po, pom = g["in_po"], g["in_pom"]
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
        scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
        so.scatter_state(po, pom, qo, qom, g["in_wekpo"], g["in_entoc"], g["in_xon"], scal)
        if cfg.cyclic:
            cyc = (float(g["in_txis"]), float(g["in_txin"]), g["in_enis"], g["in_enin"])
            for x in slabs:
                x.set_cyc_forcing(*cyc)
            o.set_p(po, pom)
            o.set_forcing(g["in_wekpo"], g["in_entoc"], g["in_xon"])
            o.set_cyc_forcing(*cyc)
            o.qgostep()
            o.ocinvq()
            want_b = oracle_bsums(o)
        done, got = 0, Gathered(so)
        for s in SNAPS[name]:
            so.steps(s - done, s0=done + 1)
            if cfg.cyclic and done == 0:
                for x in slabs:
                    b = np.zeros(4 * nl)
                    lib.check(x.L.qgcm_hip_get_bsums(x.h, b.ctypes.data_as(lib.C.POINTER(lib.C.c_double))))
                    for q in range(4):
                        u, v = b[q * nl:(q + 1) * nl], want_b[q * nl:(q + 1) * nl]
                        assert np.abs(u - v).max() <= 1e-11 * np.abs(v).max() + 1e-300, (x.rank, q)
            done = s
            e = state_errs(got, g, "steps%d" % s)
            se = scal_err(got, g, "steps%d" % s, cfg)
            print(name, seg_rows, "step", s, e, "scalars %.3e" % se)
            assert all(v < (TOL_CALL if s <= 2 else 1e-10) for v in e.values()), (s, e)
            assert se < 1e-11
    finally:
        close_all(slabs)
        o.close()


@pytest.mark.parametrize("seg_rows", [7, 10])
def test_forced_segments_cyclic_continuity_monitors(seg_rows, monkeypatch):
    """test_cyclic_continuity_monitors_on_two_y_slabs (the true reference's ermaso / emfroc after each of six steps,
    same bars, on every rank) with both slabs in forced segments."""
    spec = importlib.util.spec_from_file_location("make_golden_monitors", os.path.join(GOLDEN, "make_golden_monitors.py"))
    gm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gm)
    monkeypatch.setenv(VAR, str(seg_rows))
    g = load_golden("cyc_tiny_monitors")
    cfg = preset("cyc_tiny")
    po, wek, txis, txin = gm.inputs(cfg)
    pom = np.asfortranarray(0.98 * po)
    consts = global_consts(cfg)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
    slabs = make_slabs(cfg, consts, partition(cfg.nypo, 2), seg_rows)
    try:
        assert all(len(x.thomas_plan()) >= 2 for x in slabs)
        so = slab_ocean(cfg, slabs)
        so.scatter_state(po, pom, qo, qom, wek, np.zeros_like(wek), np.array(gm.XON), scal)
        for sl in slabs:
            sl.set_cyc_forcing(txis, txin, np.array(gm.ENIS), np.array(gm.ENIN))
        for s in range(1, gm.NSTEPS + 1):
            so.steps(1, s0=s)
            sr = g["step%d_scal" % s]
            scale = np.abs(sr[:cfg.nlo - 1]) + np.abs(sr[cfg.nlo - 1:2 * (cfg.nlo - 1)])
            for sl in slabs:
                e, f = sl.get_monitors()
                assert (np.abs(e - g["step%d_ermaso" % s]) / scale).max() < 1e-12, (s, e, g["step%d_ermaso" % s])
                assert np.abs(f - g["step%d_emfroc" % s]).max() < 1e-11, (s, f, g["step%d_emfroc" % s])
    finally:
        close_all(slabs)


# 5. homsol ---------------------------------------------------------------------------------------------------------------
def test_homsol_on_forced_segment_slabs(monkeypatch):
    """test_homsol_on_y_slabs (two ranks; same bars: the products of homsol within 1e-12 of the reference's, then five
    steps within 1e-11 of the oracle) with both slabs of box_small (40 / 39 interior rows) in three segments."""
    monkeypatch.setenv(VAR, "16")
    cfg = preset("box_small")
    g = load_golden("box_small")
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg)  # no helmholtz: no ochom
        assert "ochom" not in consts
        slabs = make_slabs(cfg, consts, partition(cfg.nypo, 2), 16)
        assert [len(x.thomas_plan()) for x in slabs] == [3, 3]
        so = slab_ocean(cfg, slabs)
        hom = so.homsol()
        for k in ("aipohs", "cdiffo", "cdhoc"):
            assert relerr(hom[k], g["h_" + k]) < 1e-12, k
        for x in slabs:
            sl = slab_slice(cfg.nypo, x.g0, x.g1)
            own = slice(x.jlo - 1, x.jhi)
            assert relerr(x.ochom_local[:, own, :], g["h_ochom"][:, sl, :][:, own, :]) < 1e-12
        po, pom = g["in_po"], g["in_pom"]
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
        scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
        so.scatter_state(po, pom, qo, qom, g["in_wekpo"], g["in_entoc"], g["in_xon"], scal)
        o.set_p(po, pom)
        o.set_forcing(g["in_wekpo"], g["in_entoc"], g["in_xon"])
        so.steps(5, s0=1)
        o.steps(1, 5)
        for f, x, y in zip(FIELDS, Gathered(so).get_state(), o.get_state()):
            assert relerr(x, y) < 1e-11, f
    finally:
        close_all(slabs)
        o.close()


# 6. the mixed layer: its three sums close the step message ------------------------------------------------------------------
def test_mixed_layer_on_forced_segment_slabs(monkeypatch):
    """The case ("box_small", 2, True, True) of test_gpu_oml.test_mixed_layer_on_y_slabs, its bars unchanged, with the
    variable set: 60 steps against the whole-domain handle (one segment: it does not read the slabs' variable)."""
    monkeypatch.setenv(VAR, "16")
    cfg = preset("box_small")
    om = oml_preset(cfg, sb_hflux=True, nb_hflux=True)
    m = OceanModel(cfg)
    slabs = []
    try:
        assert len(m.thomas_plan()) == 1
        consts = global_consts(cfg, m.helmholtz)
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        pom = np.asfortranarray(0.995 * po)
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=7)
        wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
        zero2, xon = np.zeros_like(wekpo), np.zeros(cfg.nlo - 1)
        m.oml_init(om)
        m.set_p(po, pom)
        m.set_forcing(wekpo, zero2, xon)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
        st, scal = m.get_state(), m.get_scalars()
        slabs = make_slabs(cfg, consts, partition(cfg.nypo, 2), 16)
        assert [len(x.thomas_plan()) for x in slabs] == [3, 3]
        for sl in slabs:
            sl.oml_init(om)
        so = slab_ocean(cfg, slabs)
        assert slabs[0].th_len == 3 * cfg.nlo * (-(-(cfg.nxto + 1) // 16) * 16) + 3  # ... + the mixed layer's three sums
        so.scatter_state(st[0], st[1], st[2], st[3], wekpo, zero2, xon, scal)
        for sl in slabs:
            sl.oml_set_state(sst, sstm)
            sl.oml_set_forcing(fnet, wekto, tx, ty)
        for nst in (1, 59):
            so.steps(nst)
            m.steps(nst)
            for f, x, y in zip(FIELDS, Gathered(so).get_state(), m.get_state()):
                assert relerr(x, y) < 1e-10, (f, nst)
            ga, gb = m.oml_get_state()
            for sl in slabs:
                la, lb = sl.oml_get_state()
                t1 = min(sl.g1, cfg.nypo - 1)  # owned T rows g0..t1 (global, 1-based)
                loc = slice(sl.g0 - 1 - sl.joff, t1 - sl.joff)
                if nst == 1:
                    assert np.array_equal(la[:, loc], ga[:, sl.g0 - 1:t1]), (sl.rank, "sst after the first step")
                    assert np.array_equal(lb[:, loc], gb[:, sl.g0 - 1:t1]), (sl.rank, "sstm after the first step")
                assert relerr(la[:, loc], ga[:, sl.g0 - 1:t1]) < 1e-12, (sl.rank, nst)
                assert relerr(lb[:, loc], gb[:, sl.g0 - 1:t1]) < 1e-12, (sl.rank, nst)
        for sl in slabs:
            assert np.array_equal(sl.get_scalars(), slabs[0].get_scalars())
    finally:
        close_all(slabs, m)


# 7. the library's own step loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seg_rows,graph", [("box_small", 30, False), ("box_small", 30, True), ("cyc_small", 20, False),
                                                 ("cyc_small", 20, True)])
def test_library_issued_exchanges_one_rank_in_segments(name, seg_rows, graph, monkeypatch):
    """test_gpu_parity.test_library_issued_exchanges_one_rank (same bar: the three drivers - stage by stage from Python,
    qgcm_hip_slab_steps with the library's own RCCL exchanges, and with the overlapped exchange - agree bit for bit;
    eager and as captured 50-step graphs) on a handle in forced segments.  The one rank of a one-rank communicator owns
    every row: such a handle reads QGCM_HIP_THOMAS_SEG_ROWS, and the slab phases fold its segments as a slab's."""
    monkeypatch.setenv("QGCM_HIP_SLAB_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", str(seg_rows))
    cfg = preset(name)
    want = lib.thomas_segments(cfg.nypo - 2, seg_rows)
    assert len(want) >= 3
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, o.helmholtz)
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        txis, txin = synth.tau_line_integrals(cfg, tx) if cfg.cyclic else (0.0, 0.0)
        zero2 = np.zeros((cfg.nxpo, cfg.nypo), order="F")
        xon = np.zeros(cfg.nlo - 1)
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        scal = hostinit.constr(cfg, consts["amatoc"], po, po)
        out = []
        for native in (False, True, "overlap"):
            sl = HipSlab(cfg, consts, 1, cfg.nypo, 0, 1, sync_each_call=not native)
            slabs.append(sl)
            assert sl.thomas_plan() == want
            so = slab_ocean(cfg, [sl])
            so.scatter_state(po, po, qo, qo, wek, zero2, xon, scal)
            if cfg.cyclic:
                sl.set_cyc_forcing(txis, txin)
            if native:
                so.use_library_exchanges(rccl_unique_id())
            if native == "overlap":
                sl.set_overlap(1)
            so.steps(57, s0=1)   # graph mode: a 50-step block + 7 eager steps
            sl.sync()
            out.append((sl.get_state(), sl.get_scalars()))
        assert all(np.isfinite(x).all() for x in out[0][0])
        for other in out[1:]:
            for x, y in zip(out[0][0], other[0]):
                assert np.array_equal(x, y)
            assert np.array_equal(out[0][1], other[1])
    finally:
        close_all(slabs)
        o.close()


# 7b. one set of tables, rebuilt under another plan --------------------------------------------------------------------------
def set_plan(monkeypatch, seg_rows):
    if seg_rows:
        monkeypatch.setenv(VAR, str(seg_rows))
    else:
        monkeypatch.delenv(VAR, raising=False)


def set_grid_again(sl):
    """qgcm_hip_set_grid once more with the arguments HipSlab's constructor gave it (the variable is read there)."""
    from qgcm_hip.model import _dp
    rows = slab_slice(sl.cfg.nypo, sl.g0, sl.g1)
    yp = np.ascontiguousarray(sl.consts["yporel"][rows])
    bd2 = np.ascontiguousarray(sl.consts["bd2oc"])
    dd = np.asfortranarray(sl.consts["ddynoc"][:, rows])
    lib.check(sl.L.qgcm_hip_set_grid(sl.h, _dp(yp), _dp(bd2), _dp(dd)))


@pytest.mark.parametrize("plans", [(0, 7, 0), (7, 0, 7)])
@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny"])
def test_slab_tables_rebuilt_under_another_plan(name, plans, monkeypatch):
    """A slab's one set of tables serves every plan: two slabs of the 37-row basins (18 / 17 interior rows) built under
    plans[0] (0: the variable unset, one segment; 7: three segments each), then taken by qgcm_hip_set_grid to plans[1] and
    back.  Only then are the set-up constants exchanged (SlabOcean); three steps from the golden state are bitwise -
    fields and constraint scalars - those of fresh slabs that never left that plan.  Cyclic: ybnd comes from the
    correction kernels' owner workgroup."""
    cfg, g = preset(name), load_golden(name)
    parts = partition(cfg.nypo, 2)
    o = make_oracle(cfg)
    consts = global_consts(cfg, None if cfg.cyclic else o.helmholtz)

    def run(seq):
        slabs = []
        try:
            set_plan(monkeypatch, seq[0])
            slabs = make_slabs(cfg, consts, parts, seq[0])
            for seg_rows in seq[1:]:
                set_plan(monkeypatch, seg_rows)
                for x, (g0, g1) in zip(slabs, parts):
                    set_grid_again(x)
                    assert x.thomas_plan() == lib.thomas_segments(interior_rows(cfg, g0, g1), seg_rows)
            assert [len(x.thomas_plan()) for x in slabs] == [3 if seq[-1] else 1] * 2
            so = slab_ocean(cfg, slabs)
            po, pom = g["in_po"], g["in_pom"]
            qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
            qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
            so.scatter_state(po, pom, qo, qom, g["in_wekpo"], g["in_entoc"], g["in_xon"], hostinit.constr(cfg, consts["amatoc"], po, pom))
            if cfg.cyclic:
                for x in slabs:
                    x.set_cyc_forcing(float(g["in_txis"]), float(g["in_txin"]), g["in_enis"], g["in_enin"])
            so.steps(3, s0=1)
            got = Gathered(so)
            return got.get_state(), got.get_scalars()
        finally:
            close_all(slabs)

    try:
        moved, fresh = run(plans), run(plans[-1:])
        assert all(np.isfinite(f).all() for f in fresh[0]) and np.isfinite(fresh[1]).all()
        assert not np.array_equal(fresh[0][0], g["in_po"])
        for f, x, y in zip(FIELDS, moved[0], fresh[0]):
            same_bits(x, y, f)
        same_bits(moved[1], fresh[1], "scalars")
    finally:
        o.close()


# 8. row numbers above 2048 on a slab -------------------------------------------------------------------------------------
def far_northern_eddy(cfg):
    """test_gpu_tall_diagnostics.northern_eddy moved to the 4801-row basin: the second eddy of layer 1 is centred on p row
    4797, so the jet position and the CFL locations of layer 1 are rows of the UPPER slab (2402..4801)."""
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    i = np.arange(cfg.nxpo, dtype=np.float64)[:, None]
    d = np.arange(cfg.nypo, dtype=np.float64)[None, :] - (cfg.nypo - 5.0)
    po[:, :, 0] += 8.0 * np.exp(-((i - 0.4 * cfg.nxto) / 6.0) ** 2) * np.exp(-(d / np.where(d < 0.0, 8.0, 1.5)) ** 2)
    return np.asfortranarray(po)


def test_monitors_and_cfl_of_two_tall_slabs():
    """SlabOcean.monitors() and cfl() on the two slabs of the 4801-row basin, holding what a whole-domain handle holds
    after 10 steps, against that handle at the bars of test_gpu_tall_diagnostics: the monitors as t_mon.compare takes
    them (the EXACT names bitwise, the integrals within 1e-12 of their scale), cfl as check_cfl takes it (bitwise).  The
    jet position and the CFL locations of layer 1 lie in the upper slab, past row 2048: both are asserted."""
    import test_gpu_slab_diagnostics as t_slab
    cfg = tall_cfg(400)
    m, om, f = t_mon.setup(cfg, False)
    so = None
    try:
        po = far_northern_eddy(cfg)
        m.set_p(po, po)
        m.steps(10, s0=1)
        whole = m.monitors()
        want, scales = t_mon.reference(m, om, f, False)
        t_mon.compare(whole, want, scales)
        parts = partition(cfg.nypo, 2)
        assert want["ocjpos"][0] > parts[1][0] > 2048
        so = t_slab.slabs_like(m, om, f, False, parts)
        assert [len(x.thomas_plan()) for x in so.slabs] == [3, 3]
        got = so.monitors()
        t_mon.compare(got, whole, scales)
        t_mon.compare(got, want, scales)
        crit = 0.5 * np.max(m.cfl(0.8)["courant"])
        a = m.cfl(crit)
        rows = dict(zip(a["names"], a["loc"][:, 1]))
        assert rows["u1"] > parts[1][0] and rows["v1"] > parts[1][0] and np.sum(a["nbad"]) > 0, (rows, a["nbad"])
        t_areacfl.check_cfl("two tall slabs", so.cfl(crit), a)
    finally:
        if so is not None:
            t_slab.close(so)
        m.close()


# 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    cfg = preset("box_tiny")
    consts = global_consts(cfg)
    (g0, g1), _ = partition(cfg.nypo, 2)
    for bad in ("abc", "0", "-5", "12rows"):
        monkeypatch.setenv(VAR, bad)
        with pytest.raises(QgcmHipError, match=VAR):
            HipSlab(cfg, consts, g0, g1, 0, 2)
        OceanModel(cfg).close()  # a whole-domain handle does not read it
    monkeypatch.setenv(VAR, "5")  # below 2 * 4 - 1: the plan refuses it
    with pytest.raises(QgcmHipError, match="segments of at least 4 rows"):
        HipSlab(cfg, consts, g0, g1, 0, 2)
    monkeypatch.delenv(VAR)
    # the whole-domain handles' variable alone leaves a slab on one segment
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "7")
    sl = HipSlab(cfg, consts, g0, g1, 0, 2)
    try:
        assert sl.thomas_plan() == [(0, interior_rows(cfg, g0, g1))]
    finally:
        sl.close()
    m = OceanModel(cfg)
    try:
        assert m.thomas_plan() == lib.thomas_segments(cfg.nypo - 2, 7) and len(m.thomas_plan()) == 5
    finally:
        m.close()
    monkeypatch.delenv("QGCM_HIP_THOMAS_SEG_ROWS")
    # an atmosphere of more than 2048 rows stays refused, and the refusal no longer speaks of slabs
    oc = dataclasses.replace(config.preset("cpl_tiny"), name="cpl_tall_atm", nxta=16, nyta=2052, nxaooc=4, nyaooc=4, ndxr=12)
    at = config.atmos_of(oc, ah4at=(1.5e14 * (oc.ndxr * oc.dxo / 8.0e4) ** 4,) * 3)
    assert at.nypa - 2 == 2051
    with pytest.raises(QgcmHipError, match="atmosphere handle exceed the single-segment Thomas kernel") as ei:
        AtmosModel(at)
    assert "slab" not in str(ei.value)
    small = AtmosModel(config.atmos_preset("cpl_tiny"))
    try:
        assert small.thomas_plan() == [(0, small.cfg.nypo - 2)]
    finally:
        small.close()
