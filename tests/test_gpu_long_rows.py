"""Zonally cyclic oceans whose rows are longer than one row transform holds (nxto > 5104: the reference's SOcn 4 km,
3 km, 2 km, 1 km - 5760, 7680, 11520, 23040 points), which qgcm_hip_set_grid refused before ("needs ... B of LDS per row
pair"), and - with QGCM_HIP_ROW_SPLIT - the split forced on the small basins the true reference pins.  DESIGN 3.5c:
each row is transformed as P interleaved sub-rows through a scratch array (k_row_split.h), three launches per transform.

The long basins are thin channels of 33 rows (31 interior: the last row pair has one row, and an odd P leaves an odd
number of sub-rows).  The other side is the C oracle, FFTPACK's own vectors (tests/golden/fftpack_rows_<n>.npz) or the
committed snapshots of the true reference; the oracle's runs are made once per basin and shared.  Every bar is that of
the test named in the docstring."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import oracle_binding as ob
from common import (FIELDS, SNAPS, apply_inputs, load_golden, load_snapshot, make_oracle, oml_bounds, oml_check_sums,
                    oml_init_oracle, preset, relerr, same_bits, scal_err, state_errs)
from qgcm_hip import OceanModel, QgcmHipError, lib, oml_preset, synth
from qgcm_hip.config import _SOCN, OceanConfig

pytestmark = pytest.mark.gpu

TOL_CALL = 1e-12  # one Helmholtz solve (test_gpu_parity)
TOL_RUN = 1e-10   # po, pom, qo, qom after 12 steps (test_long_columns)
TOLF = 5e-14      # test_row_transforms_against_fftpack_vectors
LENGTHS = (5760, 7680, 11520, 23040)
PLANS = {5760: (2, 2880), 7680: (2, 3840), 11520: (3, 3840), 23040: (5, 4608)}
ENIS, ENIN = (1.0e-3, 2.0e-3), (2.0e-3, -1.0e-3)
SPLIT_LAUNCHES = dict(k_tend=1, k_dst_fwd=3, k_thomas=1, k_constr=1, k_dst_inv=3, k_unpack=1)  # per step, DESIGN 3.5


def long_cfg(nxto, nyaooc=2):
    """A thin channel with the constants of the Southern Ocean presets at 5 km: nxto columns, 16 nyaooc + 1 rows."""
    assert nxto % 16 == 0
    return OceanConfig("longrows_%d" % nxto, nxto // 16, 8, nxto // 16, nyaooc, 16, 3, dxo=5.0e3, **_SOCN)


def oracle_bsums(o):
    """ajisoc, ajinoc, ap5soc, ap5noc of the oracle's last qgostep (as test_gpu_tall_columns reads them)."""
    b = np.zeros(4 * o.nl)
    o.L.qgo_get_bsums(o.h, b.ctypes.data_as(ob.C.POINTER(ob.C.c_double)))
    return b


_REF = {}


def reference(cfg, steps=12):
    """Inputs and the oracle's results on one channel, computed once (the recipe of test_gpu_tall_columns.reference for
    a zonally cyclic basin): the state and scalars after step 1 and at the end, the per-step scalars, line sums and
    continuity monitors."""
    if cfg.name in _REF:
        return _REF[cfg.name]
    nl = cfg.nlo
    r = dict(cfg=cfg)
    o = make_oracle(cfg)
    try:
        r["po"] = synth.gaussian_eddy(cfg, noise=1e-2)
        r["pom"] = np.asfortranarray(0.98 * r["po"])
        tx, ty = synth.wind_stress(cfg)
        _, r["wek"] = synth.wekpo_from_tau(cfg, tx, ty)
        # the entrainment integrals of tests/golden/make_golden_monitors.py (4e6, -1.5e6 on cyc_tiny's 4800 km x 3600 km),
        # scaled to this basin's area
        r["xon"] = np.array((4.0e6, -1.5e6)) * (cfg.xlo * cfg.ylo / (4.8e6 * 3.6e6))
        r["cyc"] = synth.tau_line_integrals(cfg, tx) + (np.array(ENIS), np.array(ENIN))
        o.set_p(r["po"], r["pom"])
        o.set_forcing(r["wek"], np.zeros_like(r["wek"]), r["xon"])
        o.set_cyc_forcing(*r["cyc"])
        r["steps"] = []
        for s in range(1, steps + 1):
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
            if s == 1:
                r["s1"] = o.get_state()
        r["end"], r["end_scal"] = o.get_state(), o.get_scalars()
    finally:
        o.close()
    _REF[cfg.name] = r
    return r


def load(m, r):
    m.set_p(r["po"], r["pom"])
    m.set_forcing(r["wek"], np.zeros_like(r["wek"]), r["xon"])
    m.set_cyc_forcing(*r["cyc"])


def check_steps_vs_oracle(m, r, tag):
    """12 steps against the oracle as test_cyclic_column_past_2048_rows_vs_oracle checks them: the continuity monitors
    after each of the first six steps (ermaso within 1e-12 of |dpioc| + |dpiocp|, emfroc within 1e-11), the boundary line
    sums after the first (1e-11 of each kind's maximum), state (1e-10) and constraint scalars (1e-11) at the end."""
    cfg = r["cfg"]
    nl = cfg.nlo
    load(m, r)
    for s, ref in zip(range(1, 7), r["steps"]):
        m.steps(1, s0=s)
        em, fm = m.get_monitors()
        scale = np.abs(ref["scal"][:nl - 1]) + np.abs(ref["scal"][nl - 1:2 * (nl - 1)])
        de, df = (np.abs(em - ref["ermaso"]) / scale).max(), np.abs(fm - ref["emfroc"]).max()
        print("%s step %d: ermaso %.3e emfroc %.3e (|emfroc| >= %.2e)" % (tag, s, de, df, np.abs(ref["emfroc"]).min()))
        assert de < 1e-12 and df < 1e-11, (s, em, ref["ermaso"], fm, ref["emfroc"])
        if s == 1:
            b = m.get_bsums()
            for q in range(4):
                x, y = b[q * nl:(q + 1) * nl], ref["bsums"][q * nl:(q + 1) * nl]
                print("%s bsums kind %d: %.3e" % (tag, q, np.abs(x - y).max() / np.abs(y).max()))
                assert np.abs(x - y).max() <= 1e-11 * np.abs(y).max() + 1e-300, q
    m.steps(6, s0=7)
    errs = {f: relerr(x, y) for f, x, y in zip(FIELDS, m.get_state(), r["end"])}
    se = scal_err(m, {"s12_scal": r["end_scal"], "s12_po": r["end"][0]}, "s12", cfg)
    print("%s 12 steps:" % tag, errs, "scalars %.3e" % se)
    assert all(v < TOL_RUN for v in errs.values()), errs
    assert se < 1e-11


def check_launches(m, s0, nsteps=2):
    """The launches of the split row family, from profile_steps: three per transform, unfused inverse rows +
    k_unpack_cyc, the stand-alone k_constr_cyc."""
    prof = {k: n for k, (_, n) in m.profile_steps(nsteps, s0=s0).items() if n}
    print(prof)
    for k, n in SPLIT_LAUNCHES.items():
        assert prof[k] == n * nsteps, (k, prof)


@pytest.mark.parametrize("nxto", LENGTHS)
def test_long_row_transforms_against_fftpack_vectors(nxto):
    """test_gpu_parity.test_row_transforms_against_fftpack_vectors at the four new lengths: qgcm_hip_row_transform
    forward and inverse against drfftf / drfftb of the reference's FFTPACK, the known vector in an even and an odd row of
    a pair (17 rows, 15 interior: row ny - 2 is the lone row of the last pair), in two modes, random rows elsewhere."""
    g = load_golden("fftpack_rows_%d" % nxto)
    cfg = OceanConfig("rows_%d" % nxto, nxto // 8, 6, nxto // 8, 2, 8, 3, dxo=5.0e3, **_SOCN)
    assert cfg.nxto == nxto
    nx, ny, nl = cfg.nxpo, cfg.nypo, cfg.nlo
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == PLANS[nxto] == lib.row_split(nxto)
        rng = np.random.default_rng(nxto)
        w = np.asfortranarray(rng.standard_normal((nx, ny, nl)))
        x, f, b = g["drfft_in_%d" % nxto], g["drfftf_out_%d" % nxto], g["drfftb_out_%d" % nxto]
        cols = slice(0, nxto)
        where = [(1, 0), (2, 0), (ny - 2, 2), (4, 1)]
        for j, mm in where:
            w[cols, j, mm] = x
        m.wrk_set(w)
        m.row_transform(0)
        got = m.wrk_get()
        for j, mm in where:
            e = relerr(got[cols, j, mm], f)
            print("forward %d row %d mode %d: %.3e" % (nxto, j, mm, e))
            assert e < TOLF, ("forward", j, mm)
        for j, mm in where:
            w[cols, j, mm] = f
        m.wrk_set(w)
        m.row_transform(1)
        got = m.wrk_get()
        for j, mm in where:
            e = relerr(got[cols, j, mm], b)
            print("inverse %d row %d mode %d: %.3e" % (nxto, j, mm, e))
            assert e < TOLF, ("inverse", j, mm)
    finally:
        m.close()


@pytest.mark.parametrize("nxto", LENGTHS)
def test_long_row_helmholtz_vs_oracle(nxto):
    """test_gpu_parity.test_long_row_transform_sizes at the four new lengths: the Helmholtz solver (row transform,
    sweeps, row transform) against the CPU oracle on a 33-row channel, all three modal diagonals."""
    cfg = OceanConfig("long_%d" % nxto, nxto // 8, 6, nxto // 8, 4, 8, 3, dxo=5.0e3, **_SOCN)
    assert cfg.nxto == nxto and cfg.nyto == 32
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    try:
        rng = np.random.default_rng(nxto)
        rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
        rhs[-1, :] = rhs[0, :]
        for mode in range(cfg.nlo):
            boc = m.bd2oc - m.rdm2oc[mode]
            e = relerr(m.helmholtz(rhs, boc), o.helmholtz(rhs, boc))
            print("helmholtz %d mode %d: %.3e" % (nxto, mode, e))
            assert e < TOL_CALL, mode
    finally:
        m.close()
        o.close()


@pytest.mark.parametrize("nxto", [5760, 23040])
def test_long_rows_twelve_steps_vs_oracle(nxto):
    """Twelve steps of qgcm_hip_steps on a 33-row channel (31 interior rows; at 23040 = 5 x 4608 an odd number of
    sub-rows) against the oracle, the recipe and bars of test_cyclic_column_past_2048_rows_vs_oracle."""
    r = reference(long_cfg(nxto))
    m = OceanModel(r["cfg"])
    try:
        assert m.row_plan() == PLANS[nxto] and (r["cfg"].nypo - 2) % 2 == 1
        assert min(np.abs(s["emfroc"]).min() for s in r["steps"][:6]) > 1e-5  # not rounding noise
        check_steps_vs_oracle(m, r, "nxto %d" % nxto)
    finally:
        m.close()


@pytest.mark.parametrize("name,P", [("cyc_tiny", 2), ("cyc_tiny", 3), ("cyc_tiny", 4), ("cyc_small", 2), ("cyc_small", 4)])
def test_forced_split_whole_steps_vs_reference(name, P, monkeypatch):
    """test_gpu_parity.test_whole_steps_vs_reference (committed snapshots of the true reference, same bars, as
    test_forced_segments_whole_steps_vs_reference repeats them) with the rows of a small basin split; then the launch
    counts of the split row family."""
    cfg, g = preset(name), load_golden(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", str(P))  # read by qgcm_hip_set_grid
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == (P, cfg.nxto // P) == lib.row_split(cfg.nxto, P)
        apply_inputs(m, g, cfg)
        done = 0
        for s in SNAPS[name]:
            m.steps(s - done, s0=done + 1)
            done = s
            e = state_errs(m, g, "steps%d" % s)
            se = scal_err(m, g, "steps%d" % s, cfg)
            print(name, P, "step", s, e, "scalars %.3e" % se)
            assert all(v < (TOL_CALL if s <= 2 else 1e-10) for v in e.values()), (s, e)
            assert se < 1e-11
        check_launches(m, done + 1)
    finally:
        m.close()


@pytest.mark.parametrize("P", [2, 3, 4])
def test_forced_split_ocinvq_vs_reference(P, monkeypatch):
    """test_gpu_parity.test_ocinvq and test_helmholtz_vs_reference (same bars, as
    test_forced_segments_ocinvq_vs_reference repeats them) on cyc_tiny with its rows split."""
    name = "cyc_tiny"
    cfg, g = preset(name), load_golden(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", str(P))
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == (P, cfg.nxto // P)
        assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc"]), g["helm_sol"]) < TOL_CALL
        assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc0"]), g["helm_sol0"]) < TOL_CALL
        apply_inputs(m, g, cfg)
        load_snapshot(m, g, "init")
        m.qgostep()
        m.ocinvq()
        e = state_errs(m, g, "ocinvq")
        se = scal_err(m, g, "ocinvq", cfg)
        print(name, P, e, "scalars %.3e" % se)
        assert e["pom"] == 0.0 and e["qo"] == 0.0 and e["qom"] == 0.0, e
        assert e["po"] < TOL_CALL, e
        assert se < 1e-13
        m.ocqbdy()
        e = state_errs(m, g, "ocqbdy")
        assert e["qo"] < TOL_CALL and e["po"] < TOL_CALL, e
    finally:
        m.close()


def test_forced_split_of_five_vs_oracle(monkeypatch):
    """P = 5 on a channel of nxto = 160 (13 rows, 11 interior: 55 sub-rows per mode) the true reference has no build
    of: 12 steps against the oracle at the bars of test_long_rows_twelve_steps_vs_oracle."""
    cfg = OceanConfig("cyc_160", 40, 8, 40, 3, 4, 3, dxo=1.0e5, dta=720.0, ah4oc=(3.2e12,) * 3, **_SOCN)
    assert cfg.nxto == 160
    r = reference(cfg)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", "5")
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == (5, 32)
        check_steps_vs_oracle(m, r, "nxto 160 / 5")
        check_launches(m, 13)
    finally:
        m.close()


@pytest.mark.parametrize("nxto", [5760, 23040])
def test_long_rows_two_steps_vs_reference_sample(nxto):
    """The REFERENCE ITSELF at a real row length: tests/golden/longrows_<nxto>_sample.npz holds every 96th (384th) column
    of the true reference's state after steps 1 and 2 on the 33-row channel (make_golden_long_rows_sample.py, in the
    manner of make_golden_fullsize.py).  Bars of test_whole_steps_vs_reference: 1e-12 of each field's maximum, the
    constraint scalars within 1e-11 as scal_err compares them."""
    cfg = long_cfg(nxto)
    g = load_golden("longrows_%d_sample" % nxto)
    st = int(g["stride"])
    nl = cfg.nlo
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    assert np.array_equal(po[::st], g["in_po"]) and np.array_equal(wek[::st], g["in_wekpo"])
    txis, txin = synth.tau_line_integrals(cfg, tx)
    assert txis == float(g["in_txis"]) and txin == float(g["in_txin"])
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == PLANS[nxto]
        m.set_p(po, po)
        m.set_forcing(wek, np.zeros_like(wek), np.zeros(nl - 1))
        m.set_cyc_forcing(txis, txin, np.zeros(nl - 1), np.zeros(nl - 1))
        for s in (1, 2):
            m.steps(1, s0=s)
            errs = {f: float(np.abs(x[::st] - g["steps%d_%s" % (s, f)]).max() / float(g["steps%d_%s_max" % (s, f)]))
                    for f, x in zip(FIELDS, m.get_state())}
            sm, sr = m.get_scalars(), g["steps%d_scal" % s]
            se = np.abs(sm[:2 * (nl - 1)] - sr[:2 * (nl - 1)]).max() / (cfg.xlo * cfg.ylo * float(g["steps%d_po_max" % s]))
            se = max(se, np.abs(sm[2 * (nl - 1):] - sr[2 * (nl - 1):]).max() / np.abs(sr[2 * (nl - 1):]).max())
            print("nxto %d step %d:" % (nxto, s), errs, "scalars %.3e" % se)
            assert all(v < TOL_CALL for v in errs.values()), (s, errs)
            assert se < 1e-11
    finally:
        m.close()


def test_graph_replay_equals_eager_on_long_rows():
    """test_gpu_parity.test_graph_replay_equals_eager at nxto = 5760: the three launches of each split transform are
    captured like any other, so the replayed graphs give the bits of the eager calls."""
    r = reference(long_cfg(5760))
    m = OceanModel(r["cfg"])
    try:
        load(m, r)
        m.steps(120, s0=1)  # 2 graph replays + 20 eager steps
        a, sa = m.get_state(), m.get_scalars()
        load(m, r)
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
        load(m, r)
        check_launches(m, 1, nsteps=30)
    finally:
        m.close()


def test_long_rows_whole_handle_vs_three_y_slabs():
    """One step at nxto = 5760 as ONE handle and as three virtual y-slabs of 11 rows (10 / 11 / 10 interior rows: the
    middle slab's last row pair has one row), every slab with split rows: the comparison and bar of
    test_tall_column_whole_handle_vs_three_y_slabs (1e-10 between the two forms and against the oracle)."""
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    r = reference(long_cfg(5760))
    cfg = r["cfg"]
    nranks = 3
    slabs = []
    m = OceanModel(cfg)
    try:
        load(m, r)
        qo, qom = m.get_state()[2], m.get_state()[3]
        scal = m.get_scalars()
        m.steps(1, s0=1)
        whole = m.get_state()
        consts = global_consts(cfg)
        parts = partition(cfg.nypo, nranks)
        assert [g1 - g0 + 1 for g0, g1 in parts] == [11, 11, 11]
        slabs = [HipSlab(cfg, consts, g0, g1, k, nranks, sync_each_call=True) for k, (g0, g1) in enumerate(parts)]
        assert all(sl.row_plan() == PLANS[5760] for sl in slabs)
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(r["po"], r["pom"], qo, qom, r["wek"], np.zeros_like(r["wek"]), r["xon"], scal)
        for sl in slabs:
            sl.set_cyc_forcing(*r["cyc"])
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


def test_mixed_layer_on_long_rows():
    """qgcm_hip_oml_init + qgcm_hip_steps at nxto = 5760 against the oracle's mixed layer, the recipe and bounds of
    test_mixed_layer_on_a_tall_column: after the first step sst and sstm by integer view, entoc and the reordered sums
    within common.oml_bounds; after three more the bars of test_coupled_steps_vs_reference."""
    r = reference(long_cfg(5760))
    cfg = r["cfg"]
    nl = cfg.nlo
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
            mod.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(nl - 1))
            mod.set_cyc_forcing(*(synth.tau_line_integrals(cfg, tx) + (np.zeros(nl - 1), np.zeros(nl - 1))))
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
        ratios = oml_check_sums("long rows", cfg, oml_bounds(cfg, xfo, coneno, e), ent, d, e, s)
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


def test_split_rows_on_a_column_in_segments(monkeypatch):
    """The split together with QGCM_HIP_THOMAS_SEG_ROWS on cyc_small (SOcn 1 km needs both: 23040 points, 2879 interior
    rows): rows as 2 x 48, the column as four segments; the true reference's snapshots at the bars of
    test_whole_steps_vs_reference; two Thomas launches per step beside the split's."""
    name = "cyc_small"
    cfg, g = preset(name), load_golden(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", "2")
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "20")
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == (2, 48) and len(m.thomas_plan()) == 4
        apply_inputs(m, g, cfg)
        done = 0
        for s in SNAPS[name]:
            m.steps(s - done, s0=done + 1)
            done = s
            e = state_errs(m, g, "steps%d" % s)
            se = scal_err(m, g, "steps%d" % s, cfg)
            print(name, "step", s, e, "scalars %.3e" % se)
            assert all(v < (TOL_CALL if s <= 2 else 1e-10) for v in e.values()), (s, e)
            assert se < 1e-11
        prof = {k: n for k, (_, n) in m.profile_steps(2, s0=done + 1).items() if n}
        assert prof["k_thomas"] == 4 and prof["k_dst_fwd"] == 6 and prof["k_dst_inv"] == 6 and prof["k_constr"] == 2, prof
    finally:
        m.close()


def test_long_row_refusals(monkeypatch):
    """What stays refused, by name: box oceans and atmosphere handles with nxto > 5104, values of QGCM_HIP_ROW_SPLIT that
    are no number, do not divide nxto or leave an odd L; the variable is not read for a box ocean; an unsplit handle's
    plan is (1, nxto)."""
    from qgcm_hip import AtmosModel
    from qgcm_hip.config import _NATL, AtmosConfig
    box = OceanConfig("box_5760", 722, 6, 720, 2, 8, 3, dxo=5.0e3, **_NATL)
    assert box.nxto == 5760 and not box.cyclic
    with pytest.raises(QgcmHipError, match="only zonally cyclic ocean handles split longer rows"):
        OceanModel(box)
    atm = AtmosConfig("atm_5760", 5760, 16, _SOCN["fnot"], _SOCN["beta"], 8.0e4)
    with pytest.raises(QgcmHipError, match="only zonally cyclic ocean handles split longer rows"):
        AtmosModel(atm)
    for bad in ("abc", "0", "-2", "2x"):
        monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", bad)
        with pytest.raises(QgcmHipError, match="QGCM_HIP_ROW_SPLIT"):
            OceanModel(preset("cyc_tiny"))
    for bad, what in (("5", "does not divide nxto=48"), ("7", "outside 2 .. 5"), ("1", "outside 2 .. 5")):
        monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", bad)
        with pytest.raises(QgcmHipError, match=what):
            OceanModel(preset("cyc_tiny"))
    odd = OceanConfig("cyc_54", 9, 8, 9, 3, 6, 3, dxo=1.0e5, dta=720.0, ah4oc=(3.2e12,) * 3, **_SOCN)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", "2")
    with pytest.raises(QgcmHipError, match="odd length 27"):
        OceanModel(odd)
    m = OceanModel(preset("box_tiny"))  # a box ocean does not read the variable
    try:
        assert m.row_plan() == (1, preset("box_tiny").nxto)
    finally:
        m.close()
    monkeypatch.delenv("QGCM_HIP_ROW_SPLIT")
    m = OceanModel(preset("cyc_tiny"))
    try:
        assert m.row_plan() == (1, 48)
    finally:
        m.close()
