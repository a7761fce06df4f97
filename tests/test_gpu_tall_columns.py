"""Whole-domain ocean handles whose column is cut into segments (k_thomas_seg + k_thomas_corr_seg):
columns of more than 2048 interior rows, which qgcm_hip_set_grid refused before, and - with QGCM_HIP_THOMAS_SEG_ROWS -
segments forced on the small basins the true reference pins.

The tall basins are thin, 49 x (12 nyaooc + 1) x 3 as in test_gpu_parity.test_long_columns: nyaooc = 171 gives 2053
rows, 2051 interior, the first basin of this family past the limit (three segments of 684 / 684 / 683 rows); nyaooc =
400 gives 4801 rows, the column of NAtl 1 km (five segments of 960 / 959).  The other side is the C oracle; its runs are made once
per basin and shared.  Tolerances are those of the tests named in each docstring."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import oracle_binding as ob
from common import (FIELDS, SNAPS, apply_inputs, load_golden, load_snapshot, make_oracle, oml_bounds, oml_check_sums,
                    oml_init_oracle, preset, relerr, same_bits, scal_err, state_errs)
from qgcm_hip import OceanModel, lib, oml_preset, synth
from qgcm_hip.config import OceanConfig

pytestmark = pytest.mark.gpu

TOL_CALL = 1e-12  # one Helmholtz solve (test_gpu_parity)
TOL_RUN = 1e-10   # po, pom, qo, qom after 12 steps (test_long_columns)
XON = (4.0e6, -1.5e6)  # per 36 cells of basin length, as tests/golden/make_golden_monitors.py prescribes for cyc_tiny
ENIS, ENIN = (1.0e-3, 2.0e-3), (2.0e-3, -1.0e-3)


def tall_cfg(nyaooc, cyclic=False):
    if cyclic:  # constants of the Southern Ocean presets (config._SOCN), nxto = 48
        return OceanConfig("tallcyc_%d" % nyaooc, 4, nyaooc + 4, 4, nyaooc, 12, 3, dxo=1.0e5, dta=720.0, ah4oc=(3.2e12,) * 3,
                           fnot=-1.19467e-04, beta=1.31301e-11, cyclic=True)
    return OceanConfig("tall_%d" % nyaooc, 8, nyaooc + 4, 4, nyaooc, 12, 3, dxo=1.0e5, dta=720.0, ah4oc=(3.2e12,) * 3,
                       fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)


_REF = {}


def oracle_bsums(o):
    """ajisoc, ajinoc, ap5soc, ap5noc of the oracle's last qgostep.  oracle_binding gives the accessor to its AtmosOracle
    only; the C function behind it (qgo_get_bsums) serves every zonally cyclic context, the ocean's included."""
    b = np.zeros(4 * o.nl)
    o.L.qgo_get_bsums(o.h, b.ctypes.data_as(ob.C.POINTER(ob.C.c_double)))
    return b


def reference(nyaooc, cyclic=False):
    """Inputs and the oracle's results of one tall basin, computed once: a Helmholtz solve with a diagonal that is no
    modal one, the state and scalars after steps 1 and 12 (box) / the per-step figures of the cyclic checks."""
    key = (nyaooc, cyclic)
    if key in _REF:
        return _REF[key]
    cfg = tall_cfg(nyaooc, cyclic)
    nl = cfg.nlo
    r = dict(cfg=cfg)
    o = make_oracle(cfg)
    try:
        c = o.get_consts()
        r["po"] = synth.gaussian_eddy(cfg, noise=1e-2)
        r["pom"] = np.asfortranarray(0.98 * r["po"]) if cyclic else r["po"]
        tx, ty = synth.wind_stress(cfg)
        _, r["wek"] = synth.wekpo_from_tau(cfg, tx, ty)
        rng = np.random.default_rng(nyaooc)
        rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
        if cyclic:
            rhs[-1, :] = rhs[0, :]
        r["rhs"] = rhs
        r["boc"] = c["bd2oc"] - 0.37 * c["rdm2oc"][1] - 0.21 * c["rdm2oc"][2]  # between the modal diagonals
        r["sol"] = o.helmholtz(rhs, r["boc"])
        r["boc0"] = c["bd2oc"] - c["rdm2oc"][0]  # the barotropic diagonal: pivots that never become stationary
        r["sol0"] = o.helmholtz(rhs, r["boc0"])
        o.set_p(r["po"], r["pom"])
        if cyclic:
            r["xon"] = np.array(XON) * (cfg.nyto / 36.0)
            r["cyc"] = synth.tau_line_integrals(cfg, tx) + (np.array(ENIS), np.array(ENIN))
            o.set_forcing(r["wek"], np.zeros_like(r["wek"]), r["xon"])
            o.set_cyc_forcing(*r["cyc"])
            # The oracle has no output for the continuity monitors, so the reference values are formed HERE, by the
            # reference's own expressions (src/ocisubs.F:268-283), from the oracle's scalars around each ocinvq:
            # est1 = the new dpioc, est2 = dpiocp - tdto gpoc xon, ermaso = est1 - est2, emfroc = 2 ermaso / (|est1| + |est2|)
            r["steps"] = []
            for s in range(1, 13):
                o.qgostep()
                before = o.get_scalars()
                o.ocinvq()
                after = o.get_scalars()
                bs = oracle_bsums(o)
                o.ocqbdy()
                if (s - 1) % 25 == 0:
                    o.lf_average()
                est1 = after[:nl - 1]
                est2 = before[nl - 1:2 * (nl - 1)] - cfg.tdto * np.array(cfg.gpoc) * r["xon"]
                r["steps"].append(dict(scal=after, bsums=bs, ermaso=est1 - est2,
                                       emfroc=2.0 * (est1 - est2) / (np.abs(est1) + np.abs(est2))))
            r["s12"], r["s12_scal"] = o.get_state(), o.get_scalars()
        else:
            o.set_forcing(r["wek"], np.zeros_like(r["wek"]), np.zeros(nl - 1))
            o.steps(1, 1)
            r["s1"] = o.get_state()
            o.steps(2, 11)
            r["s12"], r["s12_scal"] = o.get_state(), o.get_scalars()
    finally:
        o.close()
    _REF[key] = r
    return r


def load_box(m, r):
    m.set_p(r["po"], r["pom"])
    m.set_forcing(r["wek"], np.zeros_like(r["wek"]), np.zeros(r["cfg"].nlo - 1))


@pytest.mark.parametrize("nyaooc", [171, 400])
def test_columns_past_2048_rows_vs_oracle(nyaooc):
    """The sizes qgcm_hip_set_grid refused ("exceed the single-segment Thomas kernel (<= 2048)"): qgcm_hip_helmholtz
    with a diagonal that is not a modal one (the segments' responses are built for it on the call; a second call
    reuses them), and 12 steps of qgcm_hip_steps against the oracle; the constraint scalars as scal_err compares them."""
    r = reference(nyaooc)
    cfg = r["cfg"]
    nseg = len(lib.thomas_segments(cfg.nypo - 2))
    assert cfg.nypo == 12 * nyaooc + 1 and nseg == {171: 3, 400: 5}[nyaooc]
    m = OceanModel(cfg)
    try:
        for rep in range(2):
            e = relerr(m.helmholtz(r["rhs"], r["boc"]), r["sol"])
            print("helmholtz, %d rows, call %d: %.3e" % (cfg.nypo, rep, e))
            assert e < TOL_CALL
        e = relerr(m.helmholtz(r["rhs"], r["boc0"]), r["sol0"])
        print("helmholtz, barotropic diagonal: %.3e" % e)
        assert e < TOL_CALL
        load_box(m, r)
        m.steps(12, s0=1)
        errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, m.get_state(), r["s12"])}
        se = scal_err(m, {"s12_scal": r["s12_scal"], "s12_po": r["s12"][0]}, "s12", cfg)
        print("12 steps, %d rows:" % cfg.nypo, errs, "scalars %.3e" % se)
        assert all(v < TOL_RUN for v in errs.values()), errs
        assert se < 1e-11
    finally:
        m.close()


def test_cyclic_column_past_2048_rows_vs_oracle():
    """A zonally cyclic ocean of 2053 rows (part A of the constraint algebra runs in the stand-alone k_constr_cyc: the
    segmented solve has no extra workgroup for it): Helmholtz solve, then 12 steps against the oracle - state and
    constraint scalars at the end, the boundary line sums of qgcm_hip_get_bsums after the first step (the bar of
    test_gpu_atmos: 1e-11 of each kind's maximum, from identical states) and the continuity monitors after each of the
    first six steps at the bars of test_cyclic_continuity_monitors_vs_reference (six steps there too: ermaso within
    1e-12 of |dpioc| + |dpiocp|, emfroc within 1e-11)."""
    r = reference(171, cyclic=True)
    cfg = r["cfg"]
    nl = cfg.nlo
    assert cfg.cyclic and cfg.nxto == 48 and cfg.nypo == 2053
    m = OceanModel(cfg)
    try:
        e = relerr(m.helmholtz(r["rhs"], r["boc"]), r["sol"])
        print("helmholtz: %.3e" % e)
        assert e < TOL_CALL
        m.set_p(r["po"], r["pom"])
        m.set_forcing(r["wek"], np.zeros_like(r["wek"]), r["xon"])
        m.set_cyc_forcing(*r["cyc"])
        for s, ref in zip(range(1, 7), r["steps"]):
            m.steps(1, s0=s)
            em, fm = m.get_monitors()
            scale = np.abs(ref["scal"][:nl - 1]) + np.abs(ref["scal"][nl - 1:2 * (nl - 1)])
            de, df = (np.abs(em - ref["ermaso"]) / scale).max(), np.abs(fm - ref["emfroc"]).max()
            print("step %d: ermaso %.3e emfroc %.3e (|emfroc| >= %.2e)" % (s, de, df, np.abs(ref["emfroc"]).min()))
            assert de < 1e-12 and df < 1e-11, (s, em, ref["ermaso"], fm, ref["emfroc"])
            assert np.abs(ref["emfroc"]).min() > 1e-5  # not rounding noise
            if s == 1:  # the line sums of the first qgostep: both sides start from the same bits
                b = m.get_bsums()
                for q in range(4):
                    x, y = b[q * nl:(q + 1) * nl], ref["bsums"][q * nl:(q + 1) * nl]
                    print("bsums kind %d: %.3e" % (q, np.abs(x - y).max() / np.abs(y).max()))
                    assert np.abs(x - y).max() <= 1e-11 * np.abs(y).max() + 1e-300, q
        m.steps(6, s0=7)
        errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, m.get_state(), r["s12"])}
        se = scal_err(m, {"s12_scal": r["s12_scal"], "s12_po": r["s12"][0]}, "s12", cfg)
        print("12 steps:", errs, "scalars %.3e" % se)
        assert all(v < TOL_RUN for v in errs.values()), errs
        assert se < 1e-11
    finally:
        m.close()


# box_small: 79 interior rows, cyc_small: 63; 30 / 20 rows: three / four segments of unequal length (27, 26, 26 and
# 16, 16, 16, 15); 7 = 2 * QGCM_HIP_THOMAS_SEG_MIN - 1: the smallest maximum the plan takes
@pytest.mark.parametrize("name,seg_rows", [("box_small", 30), ("box_small", 7), ("cyc_small", 20), ("cyc_small", 7)])
def test_forced_segments_whole_steps_vs_reference(name, seg_rows, monkeypatch):
    """test_gpu_parity.test_whole_steps_vs_reference (committed snapshots of the true reference, same bars) with the
    column of a small basin cut into segments."""
    cfg, g = preset(name), load_golden(name)
    plan = [n for _, n in lib.thomas_segments(cfg.nypo - 2, seg_rows)]
    assert len(plan) >= 3 and (seg_rows == 7 or len(set(plan)) == 2) and min(plan) >= lib.THOMAS_SEG_MIN
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", str(seg_rows))  # read by qgcm_hip_set_grid
    m = OceanModel(cfg)
    try:
        apply_inputs(m, g, cfg)
        done = 0
        for s in SNAPS[name]:
            m.steps(s - done, s0=done + 1)
            done = s
            e = state_errs(m, g, "steps%d" % s)
            se = scal_err(m, g, "steps%d" % s, cfg)
            print(name, seg_rows, "step", s, e, "scalars %.3e" % se)
            assert all(v < (TOL_CALL if s <= 2 else 1e-10) for v in e.values()), (s, e)
            assert se < 1e-11
        # the launch plan of the segmented solve: two Thomas launches per step
        prof = m.profile_steps(2, s0=done + 1)
        assert prof["k_thomas"][1] == 4 and prof["k_tend"][1] == 2
    finally:
        m.close()


# the per-call snapshots test_ocinvq needs are stored for the tiny grids only (35 interior rows): 16 rows give three
# segments of 12, 12, 11, 7 rows five of 7
@pytest.mark.parametrize("name,seg_rows", [("box_tiny", 16), ("box_tiny", 7), ("cyc_tiny", 16), ("cyc_tiny", 7)])
def test_forced_segments_ocinvq_vs_reference(name, seg_rows, monkeypatch):
    """test_gpu_parity.test_ocinvq and test_helmholtz_vs_reference (same bars) with the column cut into segments."""
    cfg, g = preset(name), load_golden(name)
    plan = [n for _, n in lib.thomas_segments(cfg.nypo - 2, seg_rows)]
    assert len(plan) >= 3
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", str(seg_rows))
    m = OceanModel(cfg)
    try:
        assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc"]), g["helm_sol"]) < TOL_CALL
        assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc0"]), g["helm_sol0"]) < TOL_CALL
        apply_inputs(m, g, cfg)
        load_snapshot(m, g, "init")
        m.qgostep()
        m.ocinvq()
        e = state_errs(m, g, "ocinvq")
        se = scal_err(m, g, "ocinvq", cfg)
        print(name, seg_rows, e, "scalars %.3e" % se)
        assert e["pom"] == 0.0 and e["qo"] == 0.0 and e["qom"] == 0.0, e
        assert e["po"] < TOL_CALL, e
        assert se < 1e-13
        m.ocqbdy()
        e = state_errs(m, g, "ocqbdy")
        assert e["qo"] < TOL_CALL and e["po"] < TOL_CALL, e
    finally:
        m.close()


def test_graph_replay_equals_eager_on_a_tall_column():
    """test_gpu_parity.test_graph_replay_equals_eager on the 2053-row box: the two launches of the segmented solve are
    captured like any other (nothing of the host between them), so the replayed graphs give the bits of the eager
    calls.  The launches per step are those of box_tiny in test_gpu_launch_plan (generic box rows, three layers: the
    constraint solve rides in the inverse rows) with two Thomas launches instead of one."""
    r = reference(171)
    m = OceanModel(r["cfg"])
    try:
        load_box(m, r)
        m.steps(120, s0=1)  # 2 graph replays + 20 eager steps
        a, sa = m.get_state(), m.get_scalars()
        load_box(m, r)
        for s in range(1, 121):
            m.qgostep()
            m.ocinvq()
            m.ocqbdy()
            if (s - 1) % 25 == 0:
                m.lf_average()
        for f, x, y in zip(FIELDS, a, m.get_state()):
            same_bits(x, y, f)
        assert np.array_equal(sa, m.get_scalars())
        assert all(np.isfinite(x).all() for x in a)
        load_box(m, r)
        got = {k: n for k, (_, n) in m.profile_steps(30, s0=1).items() if n}
        print(got)
        assert got == {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 60, "k_dst_inv": 30, "k_unpack": 30, "k_lf_average": 2,
                       "k_noop": 30, "k_noop_train": 512}
    finally:
        m.close()


def test_mixed_layer_on_a_tall_column():
    """qgcm_hip_oml_init + qgcm_hip_steps on the 2053-row box against the oracle's mixed layer, compared as
    test_gpu_oml does: after the first step (oml from the inputs) sst and sstm by integer view, entoc and the reordered
    sums within common.oml_bounds; after three more the bars of test_coupled_steps_vs_reference."""
    r = reference(171)
    cfg = r["cfg"]
    om = oml_preset(cfg)
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    try:
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
        wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
        oml_init_oracle(o, om)
        m.oml_init(om)
        for mod in (o, m):
            mod.set_p(r["po"], r["po"])
            mod.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(cfg.nlo - 1))
        o.oml_set(sst, sstm, fnet, wekto, tx, ty)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
        o.steps_oml(1, 1)
        m.steps(1, s0=1)
        a, b, e, s = o.oml_get()
        xfo, coneno = o.oml_get_xfo()
        sa, sb = m.oml_get_state()
        ent, d = m.oml_get_diag()
        same_bits(sa, a, "sst after step 1")
        same_bits(sb, b, "sstm after step 1")
        ratios = oml_check_sums("tall box", cfg, oml_bounds(cfg, xfo, coneno, e), ent, d, e, s)
        print("largest |diff| / bound:", {k: round(v, 4) for k, v in ratios.items()})
        o.steps_oml(2, 3)
        m.steps(3, s0=2)
        a, b, e, s = o.oml_get()
        sa, sb = m.oml_get_state()
        ent, _ = m.oml_get_diag()
        errs = dict(sst=relerr(sa, a), sstm=relerr(sb, b), entoc=relerr(ent, e))
        errs.update({f: relerr(x, y) for f, x, y in zip(FIELDS, m.get_state(), o.get_state())})
        print("after step 4:", errs)
        assert errs["sst"] < 1e-13 and errs["sstm"] < 1e-13, errs
        assert all(errs[f] < 1e-10 for f in ("entoc",) + FIELDS), errs
    finally:
        m.close()
        o.close()


def test_tall_column_whole_handle_vs_three_y_slabs():
    """One step of the 2053-row box as ONE handle (three segments inside it) and as three virtual y-slabs of 684 / 685 rows
    (HipSlab / SlabOcean / LocalComm as test_long_columns builds them): the same algebra cut at other rows, within
    1e-10 as test_y_slab_decomposition_on_one_gpu asks between the two forms; both also against the oracle."""
    from qgcm_hip import hostinit
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    r = reference(171)
    cfg = r["cfg"]
    nranks = 3
    slabs = []
    m = OceanModel(cfg)
    try:
        load_box(m, r)
        m.steps(1, s0=1)
        whole = m.get_state()
        consts = global_consts(cfg, m.helmholtz)
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], r["po"])
        scal = hostinit.constr(cfg, consts["amatoc"], r["po"], r["po"])
        parts = partition(cfg.nypo, nranks)
        slabs = [HipSlab(cfg, consts, g0, g1, k, nranks, sync_each_call=True) for k, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(r["po"], r["po"], qo, qo, r["wek"], np.zeros_like(r["wek"]), np.zeros(cfg.nlo - 1), scal)
        so.steps(1, s0=1)
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        errs = {f: (relerr(x, y), relerr(x, z)) for f, x, y, z in zip(FIELDS, whole, got, r["s1"])}
        print("whole vs slabs, whole vs oracle:", errs)
        assert all(a < 1e-10 and b < 1e-10 for a, b in errs.values()), errs
    finally:
        for sl in slabs:
            sl.close()
        m.close()


def test_prsamp_and_valids_on_a_tall_column():
    """The two scans a run makes every few steps, on the 2053-row box after 12 steps: qgcm_hip_prsamp as
    test_gpu_setup.test_prsamp_numbers checks it (spot values bitwise the device state, layer averages = xintp * ocnorm
    within 1e-13 of the field maximum) and qgcm_hip_valids (extremes of po and qo bitwise those of the device state; the
    verdict that of the oracle's valids on the same state)."""
    from qgcm_hip import hostinit
    r = reference(171)
    cfg = r["cfg"]
    m = OceanModel(cfg)
    o = make_oracle(cfg)
    try:
        load_box(m, r)
        m.steps(12, s0=1)
        st = m.get_state()
        po, qo = st[0], st[2]
        s = m.prsamp()
        ic, jc = (cfg.nxpo + 1) // 2 - 1, (cfg.nypo + 1) // 2 - 1
        assert np.array_equal(s["po_centre"], po[ic, jc, :]) and np.array_equal(s["qo_centre"], qo[ic, jc, :])
        ocnorm = 1.0 / (cfg.nxto * cfg.nyto)
        for k in range(cfg.nlo):
            assert abs(s["pavgoc"][k] - hostinit.xintp(po[:, :, k]) * ocnorm) < 1e-13 * np.abs(po).max()
            assert abs(s["qavgoc"][k] - hostinit.xintp(qo[:, :, k]) * ocnorm) < 1e-13 * np.abs(qo).max()
        ok, out = m.valids()
        o.set_state(*st)
        ok_o, out_o = o.valids()
        print("valids:", ok, out[:4], "oracle:", ok_o, out_o[:4])
        assert ok == ok_o
        assert out[0] == po.min() and out[1] == po.max() and out[2] == qo.min() and out[3] == qo.max()
        assert np.array_equal(out[:4], out_o[:4])
    finally:
        m.close()
        o.close()


def test_more_segments_than_the_default_dynamic_lds_holds(monkeypatch):
    """63 segments of 32 / 33 rows on the 2053-row box (the plan allows 64): k_thomas_corr_seg then keeps 63 x 1032 B of
    summaries in dynamic LDS, past the 32 KiB a launch gets without asking and past 64 KiB - the branch that raises the
    kernel's limit.  Helmholtz solve and 12 steps against the oracle, the bars of test_columns_past_2048_rows_vs_oracle."""
    r = reference(171)
    cfg = r["cfg"]
    assert len(lib.thomas_segments(cfg.nypo - 2, 33)) == 63
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "33")
    m = OceanModel(cfg)
    try:
        e = relerr(m.helmholtz(r["rhs"], r["boc"]), r["sol"])
        print("helmholtz, 63 segments: %.3e" % e)
        assert e < TOL_CALL
        load_box(m, r)
        m.steps(12, s0=1)
        errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, m.get_state(), r["s12"])}
        se = scal_err(m, {"s12_scal": r["s12_scal"], "s12_po": r["s12"][0]}, "s12", cfg)
        print("12 steps, 63 segments:", errs, "scalars %.3e" % se)
        assert all(v < TOL_RUN for v in errs.values()), errs
        assert se < 1e-11
    finally:
        m.close()


def test_segment_length_must_be_a_positive_number(monkeypatch):
    from qgcm_hip import QgcmHipError
    for bad in ("abc", "0", "-5", "12rows"):
        monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", bad)
        with pytest.raises(QgcmHipError, match="QGCM_HIP_THOMAS_SEG_ROWS"):
            OceanModel(preset("box_tiny"))
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "5")  # below 2 * 4 - 1: the plan refuses it
    with pytest.raises(QgcmHipError, match="segments of at least 4 rows"):
        OceanModel(preset("box_tiny"))


@pytest.mark.parametrize("name", ["box_med", "cyc_med"])
def test_forced_segments_around_the_fused_fast_paths(name, monkeypatch):
    """nxto = 192: the wave-per-row-pair rows with the fused inverse launch.  box_med: the constraint solve rides in the
    extra wave of k_dst64_unpack and the leapfrog averaging is stored by k_tend / k_dst64_unpack themselves - both
    unchanged around the segmented solve: with four segments (95 interior rows, at most 25 per segment) the launches of
    30 steps are those test_gpu_launch_plan records for box_med with two Thomas launches per step, and the run with
    QGCM_HIP_NO_FUSED_AVG=1 gives the same bits (test_fused_leapfrog_average_is_bitwise's assertion).  cyc_med: part A of
    the constraint algebra cannot ride in the segmented solve (three segments here), so k_constr_cyc is a launch of its own before
    k_rfft64_unpack.  Both against the oracle after 30 steps at the bars of test_cyclic_fast_row_transform_vs_oracle."""
    cfg = preset(name)
    assert cfg.nxto == 192 and len(lib.thomas_segments(cfg.nypo - 2, 25)) >= 3
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "25")
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    pom = np.asfortranarray(0.98 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    nl = cfg.nlo

    def load(mod):
        mod.set_p(po, pom)
        mod.set_forcing(wek, np.zeros_like(wek), np.zeros(nl - 1))
        if cfg.cyclic:
            mod.set_cyc_forcing(*(synth.tau_line_integrals(cfg, tx) + (np.full(nl - 1, 1.0e-3), np.full(nl - 1, 2.0e-3))))
    o = make_oracle(cfg)
    try:
        load(o)
        o.steps(1, 30)
        want, want_scal = o.get_state(), o.get_scalars()
    finally:
        o.close()
    runs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("QGCM_HIP_NO_FUSED_AVG", flag)
        m = OceanModel(cfg)
        try:
            load(m)
            m.steps(30, s0=1)
            runs[flag] = (m.get_state(), m.get_scalars())
            if flag == "0":
                load(m)
                got = {k: n for k, (_, n) in m.profile_steps(30, s0=1).items() if n}
        finally:
            m.close()
    print(name, got)
    if cfg.cyclic:
        assert got["k_thomas"] == 60 and got["k_constr"] == 30 and got["k_tend"] == 30, got
    else:
        assert got == {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 60, "k_dst_inv": 30, "k_lf_average": 2, "k_noop": 30,
                       "k_noop_train": 512}, got
    for f, x, y in zip(FIELDS, runs["0"][0], runs["1"][0]):
        same_bits(x, y, "%s, fused averaging against the pass of its own" % f)
    assert np.array_equal(runs["0"][1], runs["1"][1])
    errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, runs["0"][0], want)}
    sm = runs["0"][1]
    se = float(np.abs(sm[:2 * (nl - 1)] - want_scal[:2 * (nl - 1)]).max() / (cfg.xlo * cfg.ylo * np.abs(po).max()))
    print(name, errs, "scalars %.3e" % se)
    assert all(v < 1e-10 for v in errs.values()), errs
    assert se < 1e-12
    if cfg.cyclic:
        assert relerr(sm[2 * (nl - 1):], want_scal[2 * (nl - 1):]) < 1e-9
