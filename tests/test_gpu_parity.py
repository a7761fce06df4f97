"""Parity tests proper: the HIP path (through the C ABI) against the golden
vectors of the true reference and against the CPU oracle.  Needs an MI355X."""
import os

import numpy as np
import pytest

from common import GOLDEN  # noqa: E402
from common import (BOX_NAMES, CONFIG_NAMES, FIELDS, SNAPS, apply_inputs, load_golden, load_snapshot, make_oracle,
                    preset, relerr, scal_err, state_errs)

pytestmark = pytest.mark.gpu

# fp64 tolerances: one call from identical state <= 1e-12 relative to the
# field max-norm; the pointwise kernels are built without FMA contraction and keep the
# reference's association order, so they are required to be bit exact.
TOL_CALL = 1e-12
TOL_60 = 1e-10
GPU_CONFIGS = CONFIG_NAMES  # box and cyclic oceans


@pytest.fixture(scope="module", params=GPU_CONFIGS)
def case(request):
    from qgcm_hip import OceanModel
    cfg = preset(request.param)
    g = load_golden(request.param)
    m = OceanModel(cfg)
    yield cfg, g, m
    m.close()


def test_native_library_is_loaded():
    from qgcm_hip import library_path
    maps = open("/proc/self/maps").read()
    from qgcm_hip import load_library
    load_library()
    maps = open("/proc/self/maps").read()
    assert library_path() in maps


def test_helmholtz_vs_reference(case):
    cfg, g, m = case
    if "helm_rhs" not in g:
        pytest.skip("the *_ah2 fixtures carry no Helmholtz vectors (the solver does not see ah2oc)")
    assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc"]), g["helm_sol"]) < TOL_CALL
    assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc0"]), g["helm_sol0"]) < TOL_CALL


def test_homsol_products(case):
    cfg, g, m = case
    if cfg.cyclic:
        big = max(np.abs(g["h_hc1soc"]).max(), np.abs(g["h_hc2noc"]).max())
        for k in ("pch1oc", "pch2oc", "pbhoc", "aipcho", "hbsioc", "aipbho"):
            assert relerr(m.homog[k], g["h_" + k]) < 1e-12, k
        for k in ("hc1soc", "hc2soc", "hc1noc", "hc2noc"):
            assert np.abs(m.homog[k] - g["h_" + k]).max() / big < 1e-12, k
        return
    for k in ("ochom", "aipohs", "cdiffo", "cdhoc"):
        assert relerr(m.homog[k], g["h_" + k]) < 1e-12, k


def test_qgostep_bit_exact(case):
    cfg, g, m = case
    if "qgostep_po" not in g:
        pytest.skip("per-call snapshots only stored for the tiny grids")
    apply_inputs(m, g, cfg)
    load_snapshot(m, g, "init")
    m.qgostep()
    e = state_errs(m, g, "qgostep")
    assert all(v == 0.0 for v in e.values()), e


def test_ocinvq(case):
    cfg, g, m = case
    if "qgostep_po" not in g:
        pytest.skip("per-call snapshots only stored for the tiny grids")
    # ocinvq consumes the projection written by the preceding qgostep kernel, so
    # replay qgostep from the init state instead of only loading its output
    apply_inputs(m, g, cfg)
    load_snapshot(m, g, "init")
    m.qgostep()
    m.ocinvq()
    e = state_errs(m, g, "ocinvq")
    assert e["pom"] == 0.0 and e["qo"] == 0.0 and e["qom"] == 0.0, e
    assert e["po"] < TOL_CALL, e
    assert scal_err(m, g, "ocinvq", cfg) < 1e-13
    m.ocqbdy()
    e = state_errs(m, g, "ocqbdy")
    assert e["qo"] < TOL_CALL and e["po"] < TOL_CALL, e


def test_ocqbdy_bit_exact(case):
    cfg, g, m = case
    if "ocinvq_po" not in g:
        pytest.skip("per-call snapshots only stored for the tiny grids")
    apply_inputs(m, g, cfg)
    load_snapshot(m, g, "ocinvq")
    m.ocqbdy()
    e = state_errs(m, g, "ocqbdy")
    assert all(v == 0.0 for v in e.values()), e


def test_whole_steps_vs_reference(case):
    cfg, g, m = case
    apply_inputs(m, g, cfg)
    done = 0
    for s in SNAPS[cfg.name]:
        m.steps(s - done, s0=done + 1)
        done = s
        e = state_errs(m, g, "steps%d" % s)
        tol = TOL_CALL if s <= 2 else TOL_60
        assert all(v < tol for v in e.values()), (s, e)
        assert scal_err(m, g, "steps%d" % s, cfg) < 1e-11


def test_graph_replay_equals_eager(case):
    """qgcm_hip_steps uses a captured 50-step HIP graph; results must be identical
    to the same steps launched one kernel at a time (determinism of every kernel)."""
    cfg, g, m = case
    apply_inputs(m, g, cfg)
    m.steps(120, s0=1)  # 2 graph replays + 20 eager steps
    a = m.get_state()
    sa = m.get_scalars()
    apply_inputs(m, g, cfg)
    for s in range(1, 121):
        m.qgostep()
        m.ocinvq()
        m.ocqbdy()
        if (s - 1) % 25 == 0:
            m.lf_average()
    b = m.get_state()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(sa, m.get_scalars())
    assert all(np.isfinite(x).all() for x in a)


def test_random_state_vs_oracle(case):
    """Seeded noisy state, 3 free-running steps, HIP vs the CPU oracle."""
    from qgcm_hip import synth
    cfg, g, m = case
    o = make_oracle(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=5e-2, seed=99, xc=0.6, yc=0.3)
        pom = synth.gaussian_eddy(cfg, noise=5e-2, seed=100, xc=0.6, yc=0.3)
        rng = np.random.default_rng(7)
        wek = np.asfortranarray(1e-6 * rng.standard_normal((cfg.nxpo, cfg.nypo)))
        ent = np.asfortranarray(1e-7 * rng.standard_normal((cfg.nxpo, cfg.nypo)))
        if cfg.cyclic:  # forcing fields of a periodic channel are periodic
            wek[-1, :], ent[-1, :] = wek[0, :], ent[0, :]
        for mod in (m, o):
            mod.set_p(po, pom)
            mod.set_forcing(wek, ent, np.full(cfg.nlo - 1, 5e2))
            if cfg.cyclic:
                mod.set_cyc_forcing(1.5e2, -0.5e2, np.full(cfg.nlo - 1, 1e-3), np.full(cfg.nlo - 1, -2e-3))
        m.steps(3, s0=5)
        o.steps(5, 3)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < TOL_CALL, f
    finally:
        o.close()


@pytest.mark.parametrize("nlo", [2, 3, 4])
def test_box_constraint_solve_rides_in_generic_inverse_rows(nlo, monkeypatch):
    """Box oceans whose rows are not 64*M long run k_dst_box; with 2 or 3 layers the constraint solve (k_constr_box's
    body) rides as one extra workgroup of the inverse-row launch instead of a launch of its own (4 layers keep the
    launch).  Same state and scalars, bit for bit, as a handle created with QGCM_HIP_NO_FUSED_CONSTR=1 (stand-alone
    launch), whole path and two y-slabs; and the oracle's trajectory."""
    import torch
    from qgcm_hip import OceanModel, synth
    from qgcm_hip.config import OceanConfig
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    lay = {2: dict(hoc=(500.0, 3500.0), gpoc=(0.02,), ah2oc=(0.0, 0.0), ah4oc=(1.2e10,) * 2),
           3: dict(hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3),
           4: dict(hoc=(300.0, 500.0, 1200.0, 2000.0), gpoc=(0.02, 0.01, 0.005), ah2oc=(0.0,) * 4, ah4oc=(1.2e10,) * 4),
           5: dict(hoc=(300.0, 400.0, 600.0, 1000.0, 1700.0), gpoc=(0.02, 0.012, 0.008, 0.005), ah2oc=(0.0,) * 5, ah4oc=(1.2e10,) * 5),
           6: dict(hoc=(250.0, 350.0, 500.0, 700.0, 1000.0, 1200.0), gpoc=(0.02, 0.015, 0.01, 0.007, 0.004), ah2oc=(0.0,) * 6,
                   ah4oc=(1.2e10,) * 6),
           8: dict(hoc=(200.0, 250.0, 300.0, 400.0, 500.0, 650.0, 800.0, 900.0), gpoc=(0.02, 0.016, 0.013, 0.01, 0.008, 0.006, 0.004),
                   ah2oc=(0.0,) * 8, ah4oc=(1.2e10,) * 8)}[nlo]
    cfg = OceanConfig("ride_nl%d" % nlo, 10, 8, 10, 6, 16, nlo, dxo=2.5e4, dta=240.0, fnot=9.37456e-05, beta=1.7536e-11,
                      cyclic=False, **lay)
    assert cfg.nxto % 64 != 0
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=5)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ent = np.zeros_like(wek)
    xon = np.zeros(nlo - 1)
    xon[0] = 2e2

    nconstr = []

    def run(whole_only=False):
        m = OceanModel(cfg)
        slabs = []
        try:
            m.set_p(po, pom)
            m.set_forcing(wek, ent, xon)
            st0, scal0 = m.get_state(), m.get_scalars()
            m.steps(30, s0=1)
            out = [m.get_state(), m.get_scalars()]
            prof = m.profile_steps(4, s0=31)  # (after the state was taken) launches per kernel of four eager steps
            nconstr.append(prof.get("k_constr", (0.0, 0))[1])
            if not whole_only:
                consts = global_consts(cfg)
                parts = partition(cfg.nypo, 2)
                slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
                so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
                so.homsol()
                so.scatter_state(st0[0], st0[1], st0[2], st0[3], wek, ent, xon, scal0)
                so.steps(30, s0=1)
                out.append([f.copy() for _, _, fs in so.gather_local() for f in fs])
                out.append(slabs[0].get_scalars())
            return out
        finally:
            m.close()
            for sl in slabs:
                sl.close()

    ride = run()
    monkeypatch.setenv("QGCM_HIP_NO_FUSED_CONSTR", "1")  # read when a handle is created
    launch = run()
    monkeypatch.delenv("QGCM_HIP_NO_FUSED_CONSTR")
    assert nconstr == [0 if nlo <= 3 else 4, 4], nconstr  # no launch of its own when it rides
    for x, y in zip(ride[0], launch[0]):
        assert np.array_equal(x, y), nlo
    assert np.array_equal(ride[1], launch[1])
    for x, y in zip(ride[2], launch[2]):
        assert np.array_equal(x, y), nlo
    assert np.array_equal(ride[3], launch[3])
    o = make_oracle(cfg)
    try:
        o.set_p(po, pom)
        o.set_forcing(wek, ent, xon)
        o.steps(1, 30)
        for f, x, y in zip(FIELDS, ride[0], o.get_state()):
            assert relerr(x, y) < 1e-10, (f, nlo)
    finally:
        o.close()


@pytest.mark.parametrize("nlo,cyclic", [(2, False), (4, False), (2, True), (4, True), (6, False), (5, True), (8, False), (8, True)])
def test_fast_kernels_with_two_and_four_layers(nlo, cyclic):
    """The wave-per-row-pair kernels (nxto = 192 = 64*3) and their fused inverse-transform / unpack / constraint-wave
    forms are templates on the number of layers; most presets carry nlo = 3.  Two and four layers (the range of the
    fused forms), box and cyclic, 30 steps incl. an averaging from a noisy state, whole path and graph replay vs the
    oracle; the box cases also as two y-slabs.  Five, six and eight layers (the maximum of the ABI): the same grid through
    the separate launches (row transforms, constraint solve, unpack), the oracle pinned to reference builds with
    nlo = 5 and 6 (tests/golden/box_tiny5.npz, cyc_tiny6.npz)."""
    import torch
    from qgcm_hip import OceanModel, hostinit, synth
    from qgcm_hip.config import OceanConfig
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    from common import layer_cfg
    cfg = layer_cfg(nlo, cyclic)  # nl<nlo>_box 193 x 97, nl<nlo>_cyc 193 x 65; layer tables: common.OCEAN_LAYERS
    assert cfg.nxto == 192
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    slabs = []
    try:
        po = synth.gaussian_eddy(cfg, noise=2e-2, seed=11)
        pom = np.asfortranarray(0.99 * po)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxto) * 2 * np.pi / cfg.nxto)[:, None] * np.ones(cfg.nypo)[None, :])
        ent = np.asfortranarray(np.vstack([ent, ent[:1]]))
        xon = np.zeros(nlo - 1)
        xon[0] = 3e2
        for mod in (m, o):
            mod.set_p(po, pom)
            mod.set_forcing(wek, ent, xon)
            if cyclic:
                mod.set_cyc_forcing(*synth.tau_line_integrals(cfg, tx), np.full(nlo - 1, 2e-4), np.full(nlo - 1, -1e-4))
        st0, scal0 = m.get_state(), m.get_scalars()
        m.steps(30, s0=1)
        o.steps(1, 30)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-10, (f, nlo, cyclic)
        if not cyclic:
            consts = global_consts(cfg, o.helmholtz)
            parts = partition(cfg.nypo, 2)
            slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
            so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
            so.scatter_state(st0[0], st0[1], st0[2], st0[3], wek, ent, xon, scal0)
            so.steps(30, s0=1)
            got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
            for g0, g1, fields in so.gather_local():
                for dst, src in zip(got, fields):
                    dst[:, g0 - 1:g1, :] = src
            for f, x, y in zip(FIELDS, got, o.get_state()):
                assert relerr(x, y) < 1e-10, (f, nlo, "slabs")
    finally:
        for sl in slabs:
            sl.close()
        m.close()
        o.close()


def test_fast_dst_grid_vs_oracle():
    """box_med has nxto = 192 = 64*3 and therefore runs the wave-per-row-pair DST
    kernel (k_dst64); check the solver and whole steps against the CPU oracle, and
    the generic Stockham kernel against the fast one."""
    import os
    from qgcm_hip import OceanModel, synth
    cfg = preset("box_med")
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    os.environ["QGCM_HIP_GENERIC_DST"] = "1"
    try:
        mg = OceanModel(cfg)
    finally:
        del os.environ["QGCM_HIP_GENERIC_DST"]
    try:
        rng = np.random.default_rng(21)
        rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
        for mode in range(cfg.nlo):
            boc = m.bd2oc - m.rdm2oc[mode]
            ref = o.helmholtz(rhs, boc)
            assert relerr(m.helmholtz(rhs, boc), ref) < TOL_CALL
            assert relerr(mg.helmholtz(rhs, boc), ref) < TOL_CALL
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        for mod in (m, mg, o):
            mod.set_p(po, 0.99 * po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        m.steps(30, s0=1)
        mg.steps(30, s0=1)
        o.steps(1, 30)
        for f, x, y, z in zip(FIELDS, m.get_state(), mg.get_state(), o.get_state()):
            assert relerr(x, z) < 1e-11, f
            assert relerr(y, z) < 1e-11, f
    finally:
        m.close()
        mg.close()
        o.close()


def test_dynamic_topography_and_entrainment_fields():
    """ddynoc != 0 (the reference's topography term, src/ocisubs.F:124, src/vorsubs.F:296) and entoc != 0: qgostep
    and ocqbdy stay bit exact against the oracle, whole steps within tolerance; then the same model with the
    fields reset to zero (forcing changed after graphs were captured)."""
    import oracle_binding as ob
    from qgcm_hip import OceanModel, synth
    cfg = preset("box_med")
    i = np.arange(cfg.nxpo)[:, None] / (cfg.nxpo - 1.0)
    j = np.arange(cfg.nypo)[None, :] / (cfg.nypo - 1.0)
    ddyn = np.asfortranarray(2.0e-6 * np.sin(3 * np.pi * i) * np.cos(2 * np.pi * j))
    ent = np.asfortranarray(1.0e-7 * np.cos(2 * np.pi * i) * np.sin(np.pi * j))
    o = ob.Oracle(cfg.nxpo, cfg.nypo, cfg.nlo, cfg.cyclic, cfg.fnot, cfg.beta, cfg.dxo, cfg.dto, cfg.delek, cfg.bccooc,
                  cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc, cfg.yporel(), ddyn)
    o0 = make_oracle(cfg)
    m = OceanModel(cfg, ddynoc=ddyn)
    m0 = OceanModel(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        xon = np.zeros(cfg.nlo - 1)
        for mod in (o, m):
            mod.set_p(po, 0.99 * po)
            mod.set_forcing(wek, ent, xon)
            mod.qgostep()
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert np.array_equal(x, y), f            # bit exact
        for mod in (o, m):
            mod.ocinvq()
            mod.ocqbdy()
            mod.steps(2, 60) if mod is o else mod.steps(60, s0=2)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-10, f
        # zero fields again (m0 never saw a non-zero field; m switches back)
        zero = np.zeros_like(ent)
        for mod in (o0, m0):
            mod.set_p(po, 0.99 * po)
            mod.set_forcing(wek, zero, xon)
        m0.steps(55, s0=1)
        o0.steps(1, 55)
        for f, x, y in zip(FIELDS, m0.get_state(), o0.get_state()):
            assert relerr(x, y) < 1e-10, f
        m.set_forcing(wek, zero, xon)
        m.set_p(po, 0.99 * po)
        o.set_forcing(wek, zero, xon)
        o.set_p(po, 0.99 * po)
        m.steps(55, s0=1)
        o.steps(1, 55)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-10, f
        m0.set_p(po, 0.99 * po)
        o0.set_p(po, 0.99 * po)
        m0.qgostep()
        o0.qgostep()
        for f, x, y in zip(FIELDS, m0.get_state(), o0.get_state()):
            assert np.array_equal(x, y), f
    finally:
        for mod in (m, m0, o, o0):
            mod.close()


@pytest.mark.parametrize("nxto,cyclic", [(3072, False), (4096, False), (5000, False), (2880, True), (4608, True), (2400, False), (4800, False),
                                         (4096, True), (2880, False)])
def test_long_row_transform_sizes(nxto, cyclic):
    """Generic row kernels on long rows: 2561 <= nxto <= 5104 runs the single-buffer in-place stages (two
    workgroups per CU), below that the two-buffer Stockham plan with 512 threads; radix mixes 8/4/2/3/5.
    The Helmholtz solver (row transform, sweeps, row transform) against the CPU oracle on a 33-row basin."""
    from qgcm_hip import OceanModel
    from qgcm_hip.config import OceanConfig
    base = dict(fnot=-1.19467e-04, beta=1.31301e-11, cyclic=True) if cyclic else dict(fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)
    nxa = nxto // 8
    cfg = OceanConfig("long_%d" % nxto, nxa if cyclic else nxa + 2, 6, nxa, 4, 8, 3, dxo=5.0e3, **base)
    assert cfg.nxto == nxto and cfg.nyto == 32
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    try:
        rng = np.random.default_rng(nxto)
        rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
        if cyclic:
            rhs[-1, :] = rhs[0, :]
        for mode in range(cfg.nlo):
            boc = m.bd2oc - m.rdm2oc[mode]
            assert relerr(m.helmholtz(rhs, boc), o.helmholtz(rhs, boc)) < TOL_CALL, mode
    finally:
        m.close()
        o.close()


@pytest.mark.parametrize("nxto,cyclic", [(960, False), (4800, False), (384, True), (960, True), (4608, True), (4800, True),
                                         (96, True), (48, False)])
def test_row_transforms_against_fftpack_vectors(nxto, cyclic):
    """The device row transforms BY THEMSELVES (qgcm_hip_wrk_set / qgcm_hip_row_transform / qgcm_hip_wrk_get) against
    known answers of FFTPACK itself (tests/golden/fftpack_eigmod.npz, fftpack_long.npz: dsint at n = nxto - 1, drfftf /
    drfftb at n = nxto, generated from the reference build): every kernel family - wave-per-row-pair (960 = 64*15,
    384), three-stage register radix (4608, 4800), generic Stockham (96, 48) - forward (unnormalised, the cyclic
    spectrum in FFTPACK's half-complex order) and inverse.  SURVEY 7 step 5."""
    from qgcm_hip import OceanModel
    from qgcm_hip.config import OceanConfig
    g = {**load_golden("fftpack_eigmod"), **load_golden("fftpack_long")}
    TOLF = 5e-14  # two factorisations of one transform, relative to the row's largest coefficient (CPU oracle: 1.6e-14 at 4800)
    base = dict(fnot=-1.19467e-04, beta=1.31301e-11, cyclic=True) if cyclic else dict(fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)
    nd = 8 if nxto % 8 == 0 and nxto >= 64 else 4
    nxa = nxto // nd
    cfg = OceanConfig("rows_%d" % nxto, nxa if cyclic else nxa + 2, 6, nxa, 2, nd, 3, dxo=5.0e3, **base)
    assert cfg.nxto == nxto
    nx, ny, nl = cfg.nxpo, cfg.nypo, cfg.nlo
    m = OceanModel(cfg)
    try:
        rng = np.random.default_rng(nxto)
        w = np.asfortranarray(rng.standard_normal((nx, ny, nl)))
        if cyclic:
            x, f, b = g["drfft_in_%d" % nxto], g["drfftf_out_%d" % nxto], g["drfftb_out_%d" % nxto]
            cols = slice(0, nxto)
        else:
            x = g["dsint_in_%d" % (nxto - 1)]
            f = g["dsint_out_%d" % (nxto - 1)]
            cols = slice(1, nxto)
        # the known vector in an even and an odd position of a row pair, in two modes; random rows elsewhere
        where = [(1, 0), (2, 0), (ny - 2, 2), (4, 1)]
        for j, mm in where:
            w[cols, j, mm] = x
        m.wrk_set(w)
        m.row_transform(0)
        got = m.wrk_get()
        for j, mm in where:
            assert relerr(got[cols, j, mm], f) < TOLF, ("forward", j, mm)
        if cyclic:  # inverse of FFTPACK's own spectrum: drfftb
            for j, mm in where:
                w[cols, j, mm] = f
            m.wrk_set(w)
            m.row_transform(1)
            got = m.wrk_get()
            for j, mm in where:
                assert relerr(got[cols, j, mm], b) < TOLF, ("inverse", j, mm)
        else:       # dsint is its own inverse up to 2 (n + 1)  (src/fftpack/newbihar/fft.doc:342-344)
            m.row_transform(1)
            back = m.wrk_get()
            for j, mm in where:
                assert relerr(back[cols, j, mm] / (2.0 * nxto), x) < 3 * TOLF, ("inverse of the forward", j, mm)  # two transforms
    finally:
        m.close()


@pytest.mark.parametrize("nyaooc,nranks", [(100, 1), (160, 1), (200, 2)])
def test_long_columns(nyaooc, nranks):
    """Columns of 1025..2048 interior rows per handle keep 20 / 24 / 32 rows per thread in the tridiagonal kernel: those
    instantiations run 512-thread workgroups of 8 wavenumbers (256 VGPRs; with 1024 threads they spilled 100-800 B per
    lane).  A tall thin basin, 49 x (12*nyaooc+1) x 3: the Helmholtz solver and 12 steps against the oracle; the tallest
    also as two y-slabs (1201 rows each: the summary phases at 20 rows per thread)."""
    import torch
    from qgcm_hip import OceanModel, hostinit, synth
    from qgcm_hip.config import OceanConfig
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = OceanConfig("tall_%d" % nyaooc, 8, nyaooc + 4, 4, nyaooc, 12, 3, dxo=1.0e5, dta=720.0, ah4oc=(3.2e12,) * 3,
                      fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)
    assert cfg.nxto == 48 and cfg.nypo == 12 * nyaooc + 1
    o = make_oracle(cfg)
    slabs = []
    m = OceanModel(cfg) if nranks == 1 else None
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        zero2, xon = np.zeros_like(wek), np.zeros(cfg.nlo - 1)
        o.set_p(po, po)
        o.set_forcing(wek, zero2, xon)
        if nranks == 1:
            rng = np.random.default_rng(nyaooc)
            rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
            boc = m.bd2oc - m.rdm2oc[1]
            assert relerr(m.helmholtz(rhs, boc), o.helmholtz(rhs, boc)) < TOL_CALL
            m.set_p(po, po)
            m.set_forcing(wek, zero2, xon)
            m.steps(12, s0=1)
            got = m.get_state()
        else:
            consts = global_consts(cfg, o.helmholtz)
            qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
            scal = hostinit.constr(cfg, consts["amatoc"], po, po)
            parts = partition(cfg.nypo, nranks)
            slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
            so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
            so.scatter_state(po, po, qo, qo, wek, zero2, xon, scal)
            so.steps(12, s0=1)
            got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
            for g0, g1, fields in so.gather_local():
                for dst, src in zip(got, fields):
                    dst[:, g0 - 1:g1, :] = src
        o.steps(1, 12)
        for f, x, y in zip(FIELDS, got, o.get_state()):
            assert relerr(x, y) < 1e-10, (f, nyaooc)
    finally:
        for sl in slabs:
            sl.close()
        if m is not None:
            m.close()
        o.close()


def test_fused_inverse_transform_unpack_bitwise():
    """k_dst64_unpack (inverse row transform + modes -> layers + boundary PV in one launch) against
    the separate k_dst64 / k_unpack_box (/ k_ocqbdy) launches: same expressions, so bitwise equal --
    through qgcm_hip_steps and through the one-for-one entry points ocinvq + ocqbdy."""
    import os
    from qgcm_hip import OceanModel, synth
    cfg = preset("box_med")
    mf = OceanModel(cfg)
    os.environ["QGCM_HIP_NO_FUSED_UNPACK"] = "1"
    try:
        ms = OceanModel(cfg)
    finally:
        del os.environ["QGCM_HIP_NO_FUSED_UNPACK"]
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        for mod in (mf, ms):
            mod.set_p(po, 0.99 * po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            mod.steps(27, s0=1)
            for _ in range(3):
                mod.qgostep(); mod.ocinvq(); mod.ocqbdy()
        for f, x, y in zip(FIELDS, mf.get_state(), ms.get_state()):
            assert np.array_equal(x, y), f
        assert np.array_equal(mf.get_scalars(), ms.get_scalars())
    finally:
        mf.close()
        ms.close()


def test_fused_long_row_unpack_vs_two_launches():
    """k_rfft3_unpack (long rows of a cyclic ocean: inverse rows + homogeneous corrections + modes -> layers + zonal
    boundary PV in one launch that mixes the modes BEFORE the transform) against k_rfft_cyc<true> + k_unpack_cyc: the
    same linear algebra in another order, so equal to rounding - through qgcm_hip_steps (30 steps, one averaging)."""
    import os
    from qgcm_hip import OceanModel, synth
    cfg = preset("cyc_2880")
    mf = OceanModel(cfg)
    os.environ["QGCM_HIP_NO_FUSED_UNPACK"] = "1"
    try:
        ms = OceanModel(cfg)
    finally:
        del os.environ["QGCM_HIP_NO_FUSED_UNPACK"]
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        for mod in (mf, ms):
            mod.set_p(po, 0.99 * po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            mod.set_cyc_forcing(*synth.tau_line_integrals(cfg, tx))
            mod.steps(30, s0=1)
        for f, x, y in zip(FIELDS, mf.get_state(), ms.get_state()):
            assert relerr(x, y) < 1e-12, f
        sf, ss = mf.get_scalars(), ms.get_scalars()
        assert np.abs(sf - ss).max() <= 1e-12 * np.abs(ss).max()
    finally:
        mf.close()
        ms.close()


@pytest.mark.parametrize("name,nranks", [("box_small", 1), ("box_small", 2), ("box_med", 3), ("box_med", 4)])
def test_y_slab_decomposition_on_one_gpu(name, nranks):
    """The multi-GPU path with all slabs as virtual ranks on this one GPU: the slab
    kernels (global-row boundary rules, phased Thomas, halo pack/unpack) and the
    orchestration, against the single-domain oracle.  Only the transport differs
    from a real multi-GPU run (torch.distributed is covered by the gloo CPU test)."""
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset(name)
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, o.helmholtz)
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        pom = np.asfortranarray(0.99 * po)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxpo) / 5.0)[:, None] * np.ones(cfg.nypo)[None, :])
        xon = np.zeros(cfg.nlo - 1)
        xon[0] = 5e2
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
        scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
        o.set_p(po, pom)
        o.set_forcing(wek, ent, xon)
        parts = partition(cfg.nypo, nranks)
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(po, pom, qo, qom, wek, ent, xon, scal)
        so.steps(30, s0=1)
        o.steps(1, 30)
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        for f, x, y in zip(FIELDS, got, o.get_state()):
            assert relerr(x, y) < 1e-10, (f, nranks)
        for sl in slabs:
            assert np.array_equal(sl.get_scalars(), slabs[0].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        o.close()


@pytest.mark.parametrize("name,nranks", [("cyc_small", 1), ("cyc_small", 2), ("cyc_med", 3), ("cyc_960", 4), ("cyc_2880", 3)])
def test_cyclic_y_slab_decomposition_on_one_gpu(name, nranks):
    """Zonally cyclic ocean on y-slabs (virtual ranks on this one GPU): the boundary line sums of the momentum
    constraints ride in the step message (rank 0 owns the southern, the last rank the northern boundary), the
    zonal-mean solution next to the boundaries comes out of the composed slab summaries - no second exchange -
    and every rank runs the constraint algebra redundantly.  Against the whole-domain model and the oracle."""
    import torch
    from qgcm_hip import OceanModel, hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset(name)
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    slabs = []
    try:
        consts = global_consts(cfg)  # homogeneous solutions of the channel from the 1-D column solver
        for k in ("pch1oc", "pch2oc"):
            assert relerr(consts[k], m.homog[k]) < 1e-12, k
        assert relerr(consts["aipcho"], m.homog["aipcho"]) < 1e-11
        # hc2soc / hc1noc are the exponentially small far-boundary responses: compare on the scale of the four together
        hscale = max(np.abs(m.homog[k]).max() for k in ("hc1soc", "hc2soc", "hc1noc", "hc2noc"))
        for k in ("hc1soc", "hc2soc", "hc1noc", "hc2noc"):
            assert np.abs(consts[k] - m.homog[k]).max() / hscale < 1e-11, k
        po = synth.gaussian_eddy(cfg, noise=1e-2)
        pom = np.asfortranarray(0.99 * po)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        txis, txin = synth.tau_line_integrals(cfg, tx)
        ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxpo - 1) * 2 * np.pi / (cfg.nxpo - 1))[:, None] * np.ones(cfg.nypo)[None, :])
        ent = np.asfortranarray(np.vstack([ent, ent[:1]]))  # periodic: column nxpo = column 1
        xon = np.zeros(cfg.nlo - 1)
        enis = np.full(cfg.nlo - 1, 3e-4)
        enin = np.full(cfg.nlo - 1, -2e-4)
        for mod in (m, o):
            mod.set_p(po, pom)
            mod.set_forcing(wek, ent, xon)
            mod.set_cyc_forcing(txis, txin, enis, enin)
        qo, qom = m.get_state()[2], m.get_state()[3]
        scal = m.get_scalars()
        parts = partition(cfg.nypo, nranks)
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(po, pom, qo, qom, wek, ent, xon, scal)
        for sl in slabs:
            sl.set_cyc_forcing(txis, txin, enis, enin)
        so.steps(30, s0=1)
        m.steps(30, s0=1)
        o.steps(1, 30)
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        for f, x, y, z in zip(FIELDS, got, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-10, (f, nranks, "vs whole-domain handle")
            assert relerr(x, z) < 1e-10, (f, nranks, "vs oracle")
        nl = cfg.nlo
        scale = cfg.xlo * cfg.ylo * np.abs(po).max()
        ss, sm = slabs[0].get_scalars(), m.get_scalars()
        assert np.abs(ss[:2 * (nl - 1)] - sm[:2 * (nl - 1)]).max() / scale < 1e-12
        assert relerr(ss[2 * (nl - 1):], sm[2 * (nl - 1):]) < 1e-9
        for sl in slabs:
            assert np.array_equal(sl.get_scalars(), slabs[0].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        m.close()
        o.close()


# ---------------------------------------------------------------------------
# BASELINE.json full size (NAtl 5 km, 961 x 961 x 3)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def natl5():
    from qgcm_hip import OceanModel, synth
    cfg = preset("natl5")
    m = OceanModel(cfg)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    yield cfg, m, wek
    m.close()


def helmholtz_residual(cfg, sol, rhs, boc_shift):
    """(Del^2_5pt - rdm2) sol - rhs on interior points, relative to max|rhs|."""
    dxom2 = 1.0 / (cfg.dxo * cfg.dxo)
    lap = dxom2 * (sol[1:-1, :-2] + sol[:-2, 1:-1] + sol[2:, 1:-1] + sol[1:-1, 2:] - 4.0 * sol[1:-1, 1:-1])
    res = lap - boc_shift * sol[1:-1, 1:-1] - rhs[1:-1, 1:-1]
    return np.abs(res).max() / np.abs(rhs).max()


def test_full_size_helmholtz_properties(natl5):
    cfg, m, _ = natl5
    rng = np.random.default_rng(1)
    rhs1 = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
    rhs2 = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
    for mode in (0, 1, 2):
        boc = m.bd2oc - m.rdm2oc[mode]
        s1, s2 = m.helmholtz(rhs1, boc), m.helmholtz(rhs2, boc)
        # solves the 5-point modified Helmholtz problem (size-independent property)
        assert helmholtz_residual(cfg, s1, rhs1, m.rdm2oc[mode]) < 1e-9
        # p = 0 on the solid boundary (src/ocisubs.F:496-509)
        assert s1[0, :].max() == 0 and s1[-1, :].max() == 0 and s1[:, 0].max() == 0 and s1[:, -1].max() == 0
        # linearity
        s12 = m.helmholtz(rhs1 + 2.0 * rhs2, boc)
        assert relerr(s12, s1 + 2.0 * s2) < 1e-12


def test_full_size_steps_vs_oracle(natl5):
    """NAtl 5 km, Gaussian-eddy IC + double-gyre wind: a few steps against the CPU oracle."""
    from qgcm_hip import synth
    cfg, m, wek = natl5
    o = make_oracle(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        for mod in (m, o):
            mod.set_p(po, po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        m.steps(4, s0=1)
        o.steps(1, 4)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < TOL_CALL, f
        sm, so = m.get_scalars(), o.get_scalars()
        scale = cfg.xlo * cfg.ylo * np.abs(po).max()
        assert np.abs(sm - so).max() / scale < 1e-13
        check_against_reference_sample(m, "natl5", cfg, po, wek)
    finally:
        o.close()


def check_against_reference_sample(m, name, cfg, po, wek, cyc=None):
    """The same steps against the REFERENCE ITSELF at this size: tests/golden/<name>_sample.npz holds every
    16th / 32nd row and column of the state after steps 1 and 4 of the true reference
    (tests/golden/make_golden_fullsize.py), from the same synthetic inputs."""
    g = load_golden(name + "_sample")
    st = int(g["stride"])
    assert np.array_equal(po[::st, ::st], g["in_po"]) and np.array_equal(wek[::st, ::st], g["in_wekpo"])
    m.set_p(po, po)
    m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
    if cyc is not None:
        assert cyc == (float(g["in_txis"]), float(g["in_txin"]))
        m.set_cyc_forcing(*cyc)
    done = 0
    for s in (1, 4):
        m.steps(s - done, s0=done + 1)
        done = s
        for i, f in enumerate(FIELDS):
            x = m.get_state()[i]
            err = np.abs(x[::st, ::st] - g["steps%d_%s" % (s, f)]).max() / float(g["steps%d_%s_max" % (s, f)])
            assert err < TOL_CALL, (name, s, f, err)
        sm, sr = m.get_scalars(), g["steps%d_scal" % s]
        nl = cfg.nlo
        scale = cfg.xlo * cfg.ylo * float(g["steps%d_po_max" % s])
        assert np.abs(sm[:2 * (nl - 1)] - sr[:2 * (nl - 1)]).max() / scale < 1e-12
        if cfg.cyclic:
            assert relerr(sm[2 * (nl - 1):], sr[2 * (nl - 1):]) < 1e-10


def test_full_size_long_run_is_finite_and_deterministic(natl5):
    from qgcm_hip import synth
    cfg, m, wek = natl5
    po = synth.gaussian_eddy(cfg)
    outs = []
    for _ in range(2):
        m.set_p(po, po)
        m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        m.steps(200, s0=1)
        outs.append(m.get_state())
    for x, y in zip(*outs):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y)
    # mass constraint: the interface-displacement integrals stay at their initial value
    # when there is no entrainment (src/ocisubs.F:342-345 with aient = 0)
    s = m.get_scalars()
    assert np.allclose(s[:cfg.nlo - 1], s[cfg.nlo - 1:2 * (cfg.nlo - 1)], rtol=0, atol=1e-6 * abs(s[0]) + 1e-3)


def test_full_size_socn5_cyclic_vs_oracle():
    """BASELINE configs[2]: Southern Ocean 5 km periodic channel, 4609 x 577 x 3
    (nxto = 4608 = 2^9 3^2 real-FFT rows, 149 KB of LDS per row pair)."""
    from qgcm_hip import OceanModel, synth
    cfg = preset("socn5")
    m = OceanModel(cfg)
    o = make_oracle(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        txis, txin = synth.tau_line_integrals(cfg, tx)
        for mod in (m, o):
            mod.set_p(po, po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            mod.set_cyc_forcing(txis, txin)
        m.steps(3, s0=1)
        o.steps(1, 3)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < TOL_CALL, f
        sm, so = m.get_scalars(), o.get_scalars()
        nl = cfg.nlo
        scale = cfg.xlo * cfg.ylo * np.abs(po).max()
        assert np.abs(sm[:2 * (nl - 1)] - so[:2 * (nl - 1)]).max() / scale < 1e-12
        assert relerr(sm[2 * (nl - 1):], so[2 * (nl - 1):]) < 1e-10
        m.steps(100, s0=4)  # exercises the graph path at this size
        assert all(np.isfinite(x).all() for x in m.get_state())
        check_against_reference_sample(m, "socn5", cfg, po, wek, cyc=(txis, txin))
    finally:
        m.close()
        o.close()


@pytest.mark.parametrize("name,graph,with_oml", [("box_small", False, False), ("box_small", True, False), ("cyc_small", False, False),
                                                 ("cyc_small", True, False), ("box_small", False, True), ("box_small", True, True)])
def test_library_issued_exchanges_one_rank(name, graph, with_oml, monkeypatch):
    """qgcm_hip_slab_steps: the distributed step with the RCCL exchanges issued by the library
    itself, on a real (one-rank) RCCL communicator -- all a one-GPU box can hold; eager and as
    50-step HIP graphs that contain the collectives.  Bitwise equal to the same slab kernels
    driven stage by stage from Python (the path the virtual-rank tests pin to the oracle).  Box and cyclic ocean,
    and with the ocean mixed layer on (its own small all-gather inside the step, three graphs for the sst rotation).
    Third run: qgcm_hip_comm_set_overlap - the halo exchange (here a one-rank all-gather) and stage 3 on a second stream,
    forked and joined by events (inside the captured graphs too), the tendency launch split into its inner and outer
    tile rows; with the mixed layer on the switch must change nothing."""
    import torch
    from qgcm_hip import hostinit, oml_preset, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, rccl_unique_id
    monkeypatch.setenv("QGCM_HIP_SLAB_GRAPH", "1" if graph else "0")
    cfg = preset(name)
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
        if with_oml:
            om = oml_preset(cfg, sb_hflux=True, nb_hflux=True)
            sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=3)
            wekto, wek = synth.wekpo_from_tau(cfg, tx, ty)
        for native in (False, True, "overlap"):
            sl = HipSlab(cfg, consts, 1, cfg.nypo, 0, 1, sync_each_call=not native)
            slabs.append(sl)
            if with_oml:
                sl.oml_init(om)
            so = SlabOcean(cfg, [sl], LocalComm(1, after=torch.cuda.synchronize))
            so.scatter_state(po, po, qo, qo, wek, zero2, xon, scal)
            if cfg.cyclic:
                sl.set_cyc_forcing(txis, txin)
            if with_oml:
                sl.oml_set_state(sst, sstm)
                sl.oml_set_forcing(fnet, wekto, tx, ty)
            if native:
                so.use_library_exchanges(rccl_unique_id())
            if native == "overlap":
                sl.set_overlap(1)
            so.steps(107 if with_oml else 57, s0=1)   # graph mode: 50-step block(s) + 7 eager steps
            sl.sync()
            out.append((sl.get_state() + (sl.oml_get_state() if with_oml else []), sl.get_scalars()))
        for other in out[1:]:
            for x, y in zip(out[0][0], other[0]):
                assert np.array_equal(x, y)
            assert np.array_equal(out[0][1], other[1])
    finally:
        for sl in slabs:
            sl.close()
        o.close()


@pytest.mark.parametrize("cyclic,nslab", [(False, 2), (False, 3), (True, 2)])
def test_inner_tendency_tiles_need_no_halo_rows(cyclic, nslab):
    """The order the overlapped halo exchange produces (qgcm_hip_comm_set_overlap), run sequentially on virtual ranks:
    stage 4 of step s+1 (inner tile rows of the tendency launch) BEFORE stage 3 of step s (halo rows in), then stage 5.
    If an inner tile read a halo row it would read the rows of the step before: the run must stay bitwise equal to
    the plain order.  60 steps from a noisy state, across the averaging steps (which keep the plain order)."""
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.config import OceanConfig
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    base = dict(fnot=-1.19467e-04, beta=1.31301e-11, cyclic=True) if cyclic else dict(fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)
    cfg = OceanConfig("early_%s" % ("cyc" if cyclic else "box"), 12 if cyclic else 16, 12, 12, 7, 16, 3, dxo=2.5e4, dta=240.0,
                      ah4oc=(1.2e10,) * 3, **base)
    assert cfg.nypo >= 33 * nslab  # at least three 16-row tile rows per slab
    consts = global_consts(cfg)
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=21)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ent = np.zeros_like(wek)
    xon = np.zeros(cfg.nlo - 1)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
    txis, txin = synth.tau_line_integrals(cfg, tx) if cyclic else (0.0, 0.0)
    outs = []
    for early in (False, True):
        slabs = [HipSlab(cfg, consts, g0, g1, r, nslab, sync_each_call=True) for r, (g0, g1) in enumerate(partition(cfg.nypo, nslab))]
        try:
            so = SlabOcean(cfg, slabs, LocalComm(nslab, after=torch.cuda.synchronize))
            so.early_tend = early
            if not cyclic:
                so.homsol()
            so.scatter_state(po, pom, qo, qom, wek, ent, xon, scal)
            for x in slabs:
                if cyclic:
                    x.set_cyc_forcing(txis, txin)
            so.steps(60, s0=1)
            outs.append(([f.copy() for _, _, fs in so.gather_local() for f in fs], slabs[0].get_scalars()))
        finally:
            for x in slabs:
                x.close()
    assert all(np.isfinite(f).all() for f in outs[0][0])
    for x, y in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(outs[0][1], outs[1][1])


def test_bench_n8_workload_as_virtual_ranks():
    """Exactly the decomposition bench.py --gpus 8 runs (weak scaling: a 961 x 7681 x 3 basin, eight
    NAtl-5km-shaped slabs), here with the eight slabs as virtual ranks on this one GPU; three steps against the
    single-domain CPU oracle.  Only the transport differs from the real 8-GPU run."""
    import dataclasses
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg5 = preset("natl5")
    nranks = 8
    cfg = dataclasses.replace(cfg5, name="natl5_x8", nyaooc=cfg5.nyaooc * nranks, nyta=cfg5.nyta * nranks)
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, lambda w, b: hostinit.helmholtz_box_host(cfg, w, b))
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        zero2 = np.zeros((cfg.nxpo, cfg.nypo), order="F")
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        scal = hostinit.constr(cfg, consts["amatoc"], po, po)
        o.set_p(po, po)
        o.set_forcing(wek, zero2, np.zeros(cfg.nlo - 1))
        parts = partition(cfg.nypo, nranks)
        assert all(abs((g1 - g0 + 1) - 960) <= 1 for g0, g1 in parts)
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(po, po, qo, qo, wek, zero2, np.zeros(cfg.nlo - 1), scal)
        so.steps(3, s0=1)
        o.steps(1, 3)
        ref = o.get_state()
        for g0, g1, fields in so.gather_local():
            for f, x, y in zip(FIELDS, fields, ref):
                assert relerr(x, y[:, g0 - 1:g1, :]) < 1e-11, (f, g0)
        for sl in slabs:
            assert np.array_equal(sl.get_scalars(), slabs[0].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        o.close()


def test_full_size_natl1_slabs_vs_oracle():
    """BASELINE configs[4]: NAtl 1 km (4801 x 4801 x 3) as y-slabs.  Four slabs run as
    virtual ranks on this one GPU (the 8-GPU run only changes the transport); two
    steps against the CPU oracle."""
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("natl1")
    nranks = 4
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, lambda w, b: hostinit.helmholtz_box_host(cfg, w, b))
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        zero2 = np.zeros((cfg.nxpo, cfg.nypo), order="F")
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        scal = hostinit.constr(cfg, consts["amatoc"], po, po)
        o.set_p(po, po)
        o.set_forcing(wek, zero2, np.zeros(cfg.nlo - 1))
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True)
                 for r, (g0, g1) in enumerate(partition(cfg.nypo, nranks))]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(po, po, qo, qo, wek, zero2, np.zeros(cfg.nlo - 1), scal)
        so.steps(2, s0=1)
        o.steps(1, 2)
        ref = o.get_state()
        for g0, g1, fields in so.gather_local():
            for f, x, y in zip(FIELDS, fields, ref):
                assert relerr(x, y[:, g0 - 1:g1, :]) < 1e-11, (f, g0)
    finally:
        for sl in slabs:
            sl.close()
        o.close()


@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny", "box_small", "box_tiny_spl"])
def test_wide_tendency_tiles_are_bit_exact(name, monkeypatch):
    """At the HBM-bound sizes (SOcn 5 km, the slabs of NAtl 1 km) the tendency kernel runs 32-wide tiles with plain stores
    (chosen by size in launch_tend); QGCM_HIP_TEND_WIDE=1 forces that instantiation at the fixture sizes: qgostep bit
    for bit the reference, whole steps as the default instantiation, two y-slabs with the split (inner / outer) launch."""
    import torch
    from qgcm_hip import OceanModel
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset(name)
    g = load_golden(name)
    ref = OceanModel(cfg)
    apply_inputs(ref, g, cfg)
    ref.steps(30, s0=1)
    want = ref.get_state()
    ref.close()
    monkeypatch.setenv("QGCM_HIP_TEND_WIDE", "1")
    m = OceanModel(cfg)
    slabs = []
    try:
        apply_inputs(m, g, cfg)
        if "qgostep_po" in g:
            load_snapshot(m, g, "init")
            m.qgostep()
            e = state_errs(m, g, "qgostep")
            assert all(v == 0.0 for v in e.values()), e
            apply_inputs(m, g, cfg)
        st0, sc0 = m.get_state(), m.get_scalars()
        m.steps(30, s0=1)
        for x, y in zip(m.get_state(), want):
            assert np.array_equal(x, y)
        if not cfg.cyclic and cfg.l_spl == 0.0:
            consts = global_consts(cfg)
            slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(partition(cfg.nypo, 2))]
            so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
            so.homsol()
            so.scatter_state(st0[0], st0[1], st0[2], st0[3], g["in_wekpo"], g["in_entoc"], g["in_xon"], sc0)
            so.steps(30, s0=1)
            got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
            for g0, g1, fields in so.gather_local():
                for dst, src in zip(got, fields):
                    dst[:, g0 - 1:g1, :] = src
            for f, x, y in zip(FIELDS, got, want):
                assert relerr(x, y) < 1e-10, f
    finally:
        for sl in slabs:
            sl.close()
        m.close()


def test_sponge_layer_on_y_slabs():
    """The sponge term (src/qgosubs.F:203-205) on the y-slab path: every slab takes its rows of the ramp
    (qgcm_hip_set_sponge on a slab handle); two slabs of the box_tiny_spl reference fixture against the reference itself."""
    import torch
    from qgcm_hip import hostinit
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("box_tiny_spl")
    g = load_golden("box_tiny_spl")
    consts = global_consts(cfg)
    slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(partition(cfg.nypo, 2))]
    try:
        so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
        so.homsol()
        for sl in slabs:
            sl.set_sponge(g["in_rspl"], float(g["in_c1spl"]))
        so.scatter_state(g["init_po"], g["init_pom"], g["init_qo"], g["init_qom"], g["in_wekpo"], g["in_entoc"], g["in_xon"], g["init_scal"])
        so.steps(26, s0=1)
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        for f, x in zip(FIELDS, got):
            assert relerr(x, g["steps26_" + f]) < TOL_60, f
        assert relerr(got[0], load_golden("box_tiny")["steps26_po"]) > 1e-4   # (the term is not a no-op in this fixture)
    finally:
        for sl in slabs:
            sl.close()


def test_natl5_long_run_within_the_references_own_thread_spread():
    """SURVEY 8(d)'s long-run tolerances at BASELINE's full size (NAtl 5 km, 961 x 961 x 3, configs[1]): after 160
    ocean steps <= 1e-9, after 1600 (ten model days) <= 1e-7 of the field's max-norm, against samples of the REFERENCE
    ITSELF (tests/golden/natl5_long_sample.npz, make_golden_longrun.py: 8 OpenMP threads).  The fixture also holds the
    reference's own 8- vs 1-thread difference over the full fields (its OpenMP sums depend on the thread count): the
    yardstick SURVEY prescribes - the device must not be further from the reference than ten times that, or the
    tolerance, whichever is larger."""
    from qgcm_hip import OceanModel, synth
    cfg = preset("natl5")
    g = load_golden("natl5_long_sample")
    st = int(g["stride"])
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    assert np.array_equal(po[::st, ::st], g["in_po"]) and np.array_equal(wek[::st, ::st], g["in_wekpo"])
    m = OceanModel(cfg)
    try:
        m.set_p(po, po)
        m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        done, log = 0, []
        for s, tol in ((160, 1e-9), (1600, 1e-7)):
            m.steps(s - done, s0=done + 1)
            done = s
            for i, n in enumerate(FIELDS):
                err = float(np.abs(m.get_state()[i][::st, ::st] - g["steps%d_%s" % (s, n)]).max() / float(g["steps%d_%s_max" % (s, n)]))
                spread = float(g["spread%d_%s" % (s, n)])
                log.append("step %d %s: device vs reference %.2e, reference 8 vs 1 threads %.2e" % (s, n, err, spread))
                assert err < max(tol, 10.0 * spread), log[-1]
            sr, s1, sm = g["steps%d_scal" % s], g["steps%d_scal_1thread" % s], m.get_scalars()
            scale = cfg.xlo * cfg.ylo * float(g["steps%d_po_max" % s])
            n1 = 2 * (cfg.nlo - 1)
            assert np.abs(sm[:n1] - sr[:n1]).max() / scale < max(tol, 10.0 * np.abs(s1[:n1] - sr[:n1]).max() / scale)
        try:
            with open(os.path.join(os.environ.get("GRAFT_REPO_ROOT", "."), "gpurun_out", "natl5_long_run_errors.log"), "w") as f:
                f.write("\n".join(log) + "\n")
        except OSError:
            pass
    finally:
        m.close()


def test_cyclic_continuity_monitors_vs_reference():
    """ermaso / emfroc of the zonally cyclic ocinvq (MODULE monitor, src/ocisubs.F:268-283; round 2 skipped them): the
    device values after each of six steps against the TRUE reference (tests/golden/cyc_tiny_monitors.npz,
    make_golden_monitors.py) for a prescribed entrainment integral that makes them O(1e-4) relative numbers, in the
    three stand-alone calls and inside qgcm_hip_steps."""
    import importlib.util
    from qgcm_hip import OceanModel
    spec = importlib.util.spec_from_file_location("make_golden_monitors", os.path.join(GOLDEN, "make_golden_monitors.py"))
    gm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gm)
    g = load_golden("cyc_tiny_monitors")
    cfg = preset("cyc_tiny")
    po, wek, txis, txin = gm.inputs(cfg)
    for fused in (False, True):
        m = OceanModel(cfg)
        try:
            m.set_p(po, 0.98 * po)
            m.set_forcing(wek, np.zeros_like(wek), np.array(gm.XON))
            m.set_cyc_forcing(txis, txin, np.array(gm.ENIS), np.array(gm.ENIN))
            for s in range(1, gm.NSTEPS + 1):
                if fused:
                    m.steps(1, s0=s)
                else:
                    m.qgostep()
                    m.ocinvq()
                    m.ocqbdy()
                    if (s - 1) % 25 == 0:
                        m.lf_average()
                e, f = m.get_monitors()
                sr = g["step%d_scal" % s]
                scale = np.abs(sr[:cfg.nlo - 1]) + np.abs(sr[cfg.nlo - 1:2 * (cfg.nlo - 1)])  # |dpioc| + |dpiocp| ~ esum
                assert (np.abs(e - g["step%d_ermaso" % s]) / scale).max() < 1e-12, (fused, s, e, g["step%d_ermaso" % s])
                assert np.abs(f - g["step%d_emfroc" % s]).max() < 1e-11, (fused, s, f, g["step%d_emfroc" % s])
                assert np.abs(g["step%d_emfroc" % s]).min() > 1e-5   # the fixture is not rounding noise
        finally:
            m.close()


def test_cyclic_continuity_monitors_on_two_y_slabs():
    """The same monitors on the y-slab path (two virtual ranks, the constraint algebra runs redundantly on every rank from
    the gathered step messages): every rank's ermaso / emfroc after each of six steps against the reference fixture."""
    import importlib.util
    import torch
    from qgcm_hip import hostinit
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    spec = importlib.util.spec_from_file_location("make_golden_monitors", os.path.join(GOLDEN, "make_golden_monitors.py"))
    gm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gm)
    g = load_golden("cyc_tiny_monitors")
    cfg = preset("cyc_tiny")
    po, wek, txis, txin = gm.inputs(cfg)
    pom = np.asfortranarray(0.98 * po)
    consts = global_consts(cfg)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
    nranks = 2
    slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(cfg.nypo, nranks))]
    try:
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
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
        for sl in slabs:
            sl.close()


def test_full_size_natl1_eight_slabs_vs_reference_sample():
    """BASELINE configs[4] in the decomposition the 8-GPU run uses: NAtl 1 km (4801 x 4801 x 3, dto = 180 s) cut into
    EIGHT y-slabs of 600 / 601 rows (virtual ranks on this one GPU: the 8-GPU run only changes the transport), homogeneous
    solutions by the distributed Helmholtz solve, two steps - against the REFERENCE ITSELF at this size:
    tests/golden/natl1_sample.npz holds every 64th row and column of the true reference's state after steps 1 and 2
    (built from src/parameters_data.F.NAtl.1km:45,50; tests/golden/make_golden_fullsize.py natl1)."""
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("natl1")
    nranks = 8
    g = load_golden("natl1_sample")
    st = int(g["stride"])
    slabs = []
    try:
        consts = global_consts(cfg)
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        assert np.array_equal(po[::st, ::st], g["in_po"]) and np.array_equal(wek[::st, ::st], g["in_wekpo"])
        zero2 = np.zeros((cfg.nxpo, cfg.nypo), order="F")
        qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
        scal = hostinit.constr(cfg, consts["amatoc"], po, po)
        parts = partition(cfg.nypo, nranks)
        assert sorted(set(g1 - g0 + 1 for g0, g1 in parts)) == [600, 601]
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.homsol()
        so.scatter_state(po, po, qo, qo, wek, zero2, np.zeros(cfg.nlo - 1), scal)
        del qo, zero2
        for s in (1, 2):
            so.steps(1, s0=s)
            worst = {}
            for g0, g1, fields in so.gather_local():
                rows = np.arange(0, cfg.nypo, st)
                rows = rows[(rows >= g0 - 1) & (rows <= g1 - 1)]     # sampled global rows (0-based) inside this slab
                for f, x in zip(FIELDS, fields):
                    ref = g["steps%d_%s" % (s, f)][:, rows // st, :]
                    err = np.abs(x[::st, rows - (g0 - 1), :] - ref).max() / float(g["steps%d_%s_max" % (s, f)])
                    worst[f] = max(worst.get(f, 0.0), float(err))
            for f in FIELDS:
                assert worst[f] < 1e-11, (s, worst)
            sm, sr = slabs[0].get_scalars(), g["steps%d_scal" % s]
            nl = cfg.nlo
            scale = cfg.xlo * cfg.ylo * float(g["steps%d_po_max" % s])
            assert np.abs(sm[:2 * (nl - 1)] - sr[:2 * (nl - 1)]).max() / scale < 1e-12
    finally:
        for sl in slabs:
            sl.close()


@pytest.mark.parametrize("name", ["cyc_med", "cyc_960"])
def test_cyclic_fast_row_transform_vs_oracle(name):
    """nxto = 64*3 / 64*15 zonally cyclic oceans: wave-per-row-pair real FFT rows (k_rfft64.h), constraint algebra split
    over the Thomas launch and the fused inverse-transform / unpack kernel - against the CPU oracle, and the fused
    step path against the stand-alone entry points (bitwise)."""
    from qgcm_hip import OceanModel, synth
    cfg = preset(name)
    m = OceanModel(cfg)
    o = make_oracle(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        tx, ty = synth.wind_stress(cfg)
        _, wek = synth.wekpo_from_tau(cfg, tx, ty)
        txis, txin = synth.tau_line_integrals(cfg, tx)
        enis, enin = np.full(cfg.nlo - 1, 1.0e-3), np.full(cfg.nlo - 1, 2.0e-3)
        for mod in (m, o):
            mod.set_p(po, 0.98 * po)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            mod.set_cyc_forcing(txis, txin, enis, enin)
        m.steps(30, s0=1)
        o.steps(1, 30)
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-10, f
        sm, so = m.get_scalars(), o.get_scalars()
        nl = cfg.nlo
        scale = cfg.xlo * cfg.ylo * np.abs(po).max()
        assert np.abs(sm[:2 * (nl - 1)] - so[:2 * (nl - 1)]).max() / scale < 1e-12
        assert relerr(sm[2 * (nl - 1):], so[2 * (nl - 1):]) < 1e-9
        a, sa = m.get_state(), m.get_scalars()
        m.set_p(po, 0.98 * po)
        for s in range(1, 31):
            m.qgostep()
            m.ocinvq()
            m.ocqbdy()
            if (s - 1) % 25 == 0:
                m.lf_average()
        for x, y in zip(a, m.get_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(sa, m.get_scalars())
        # Helmholtz solver alone (hscyoc) on a random right-hand side
        rng = np.random.default_rng(5)
        rhs = np.asfortranarray(rng.standard_normal((cfg.nxpo, cfg.nypo)))
        rhs[-1, :] = rhs[0, :]
        boc = m.bd2oc - m.rdm2oc[1]
        assert relerr(m.helmholtz(rhs, boc), o.helmholtz(rhs, boc)) < TOL_CALL
    finally:
        m.close()
        o.close()


@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_homsol_on_y_slabs(nranks):
    """homsol without a host-side solver: the distributed modal Helmholtz solve with right-hand side 1
    (SlabOcean.homsol: qgcm_hip_wrk_fill, row transforms, the two Thomas phases around one exchange) against the
    reference's ochom, aipohs, cdiffo, cdhoc (src/conhoms.F:549-611), then a few steps against the oracle."""
    import torch
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition, slab_slice
    cfg = preset("box_small")
    g = load_golden("box_small")
    o = make_oracle(cfg)
    slabs = []
    try:
        consts = global_consts(cfg)  # no helmholtz: no ochom
        assert "ochom" not in consts
        parts = partition(cfg.nypo, nranks)
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
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
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        for f, x, y in zip(FIELDS, got, o.get_state()):
            assert relerr(x, y) < 1e-11, (f, nranks)
    finally:
        for sl in slabs:
            sl.close()
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nlo", [2, 3, 4])
def test_fused_leapfrog_average_is_bitwise(nlo, monkeypatch):
    """Inside qgcm_hip_steps the box ocean's fused kernels store the averaged time level themselves on the steps that the
    reference follows with its leapfrog averaging (src/q-gcm.F:1345-1351): k_tend the interior qo, k_dst64_unpack the
    new po and the boundary qo, a one-thread launch the integrals dpioc.  QGCM_HIP_NO_FUSED_AVG=1 keeps the pass of its
    own (k_lf_average, the form the reference fixtures of test_whole_steps_vs_reference pin at the generic sizes): the
    two are bit for bit the same after 1, 26 and 60 steps (averaging after steps 1, 26, 51), graph replay and eager."""
    from qgcm_hip import OceanModel, synth
    from qgcm_hip.config import OceanConfig
    lay = {2: dict(hoc=(500.0, 3500.0), gpoc=(0.02,), ah2oc=(0.0, 0.0), ah4oc=(1.2e10,) * 2),
           3: dict(hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3),
           4: dict(hoc=(300.0, 500.0, 1200.0, 2000.0), gpoc=(0.02, 0.01, 0.005), ah2oc=(0.0,) * 4, ah4oc=(1.2e10,) * 4)}[nlo]
    cfg = OceanConfig("nl%d_box_avg" % nlo, 16, 10, 12, 6, 16, nlo, dxo=2.5e4, dta=240.0, fnot=9.37456e-05, beta=1.7536e-11,
                      cyclic=False, **lay)
    assert cfg.nxto == 192  # the wave-per-row-pair kernels
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=5)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    xon = np.zeros(nlo - 1)
    xon[0] = 3e2
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("QGCM_HIP_NO_FUSED_AVG", flag)
        m = OceanModel(cfg)
        try:
            m.set_p(po, pom)
            m.set_forcing(wek, np.zeros_like(wek), xon)
            snaps = []
            m.steps(1, s0=1)   # one eager step, followed by the averaging
            snaps.append((m.get_state(), m.get_scalars()))
            m.steps(25, s0=2)  # ... step 26 averages again
            snaps.append((m.get_state(), m.get_scalars()))
            m.steps(34, s0=27)  # a captured block across the averaging after step 51
            snaps.append((m.get_state(), m.get_scalars()))
            out[flag] = snaps
        finally:
            m.close()
    for (sa, ca), (sb, cb) in zip(out["1"], out["0"]):
        for f, x, y in zip(FIELDS, sa, sb):
            assert np.array_equal(x, y), f
        assert np.array_equal(np.asarray(ca), np.asarray(cb))


@pytest.mark.gpu
def test_fused_leapfrog_average_long_cyclic_rows_is_bitwise(monkeypatch):
    """The same for the long rows of a cyclic ocean (k_tend<3, true, .., AVG> + k_rfft3_unpack<.., AVG>: new po, the PV of
    the zonal boundary rows, and the integrals dpioc / ocncs / ocncn in the one-thread launch): bit for bit the fields and
    scalars of the run that keeps k_lf_average (QGCM_HIP_NO_FUSED_AVG=1), eager and graph replay, 1 + 25 + 34 steps."""
    from qgcm_hip import OceanModel, synth
    cfg = preset("cyc_2880")
    po = synth.gaussian_eddy(cfg, noise=1e-2)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("QGCM_HIP_NO_FUSED_AVG", flag)
        m = OceanModel(cfg)
        try:
            m.set_p(po, 0.99 * po)
            m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            m.set_cyc_forcing(*synth.tau_line_integrals(cfg, tx))
            snaps = []
            for n, s0 in ((1, 1), (25, 2), (34, 27)):
                m.steps(n, s0=s0)
                snaps.append((m.get_state(), np.asarray(m.get_scalars())))
            out[flag] = snaps
        finally:
            m.close()
    for (sa, ca), (sb, cb) in zip(out["1"], out["0"]):
        for f, x, y in zip(FIELDS, sa, sb):
            assert np.array_equal(x, y), f
        assert np.array_equal(ca, cb)


@pytest.mark.gpu
def test_fused_leapfrog_average_with_mixed_layer_is_bitwise(monkeypatch):
    """... and with the ocean mixed layer on the device: po / qo are averaged by the step's kernels, sst keeps its own
    one-field pass (k_oml_average), the mixed layer's final reduction rides in k_tend<.., AVG> as in the plain kernel."""
    from qgcm_hip import OceanModel, oml_preset, synth
    from qgcm_hip.config import OceanConfig
    cfg = OceanConfig("nl3_box_avg_oml", 16, 10, 12, 6, 16, 3, dxo=2.5e4, dta=240.0, fnot=9.37456e-05, beta=1.7536e-11,
                      cyclic=False, hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3)
    om = oml_preset(cfg)
    sst, sstm, fnet, txo, tyo = synth.mixed_layer_fields(cfg, om)
    wekto, _ = synth.wekpo_from_tau(cfg, txo, tyo)
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=5)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("QGCM_HIP_NO_FUSED_AVG", flag)
        m = OceanModel(cfg)
        try:
            m.oml_init(om)
            m.oml_set_state(sst, sstm)
            m.oml_set_forcing(fnet, wekto, txo, tyo)
            m.set_p(po, np.asfortranarray(0.99 * po))
            m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            snaps = []
            for n, s0 in ((1, 1), (25, 2), (34, 27)):
                m.steps(n, s0=s0)
                snaps.append((m.get_state(), np.asarray(m.get_scalars()), m.oml_get_state()))
            out[flag] = snaps
        finally:
            m.close()
    for (sa, ca, ta), (sb, cb, tb) in zip(out["1"], out["0"]):
        for f, x, y in zip(FIELDS, sa, sb):
            assert np.array_equal(x, y), f
        assert np.array_equal(ca, cb)
        for x, y in zip(ta, tb):
            assert np.array_equal(np.asarray(x), np.asarray(y))
