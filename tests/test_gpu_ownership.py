"""Who owns the device memory: a handle gives back every allocation it took, set-up calls that are repeated replace
their buffers instead of piling new ones up, and none of it changes a result.  The figures are the library's own count
of the allocations it holds in this process (qgcm_hip_debug_live_allocs: blocks, bytes) - exact and process-local,
where the device's free memory moves with whatever else runs on the GPU.  Every test compares against the count at
its own start: other handles of the process may be alive."""
import numpy as np
import pytest

from common import load_golden, oml_config, oml_load, preset, same_bits

pytestmark = pytest.mark.gpu


def live():
    from qgcm_hip.lib import live_allocs
    return live_allocs()


def set_grid_again(m):
    """qgcm_hip_set_grid once more with the arguments the constructor gave it (QGCM_HIP_THOMAS_SEG_ROWS is read there)."""
    from qgcm_hip.lib import check
    from qgcm_hip.model import _dp
    check(m.L.qgcm_hip_set_grid(m.h, _dp(m.yporel), _dp(m.bd2oc), _dp(m.ddynoc)))


def ramp(cfg):
    """A sponge ramp that any ocean accepts (periodic in x)."""
    return np.asfortranarray(np.broadcast_to(np.linspace(0.0, 0.2, cfg.nypo), (cfg.nxpo, cfg.nypo)))


# 1. a handle gives back everything ------------------------------------------------------------------------------------
def test_coupled_pair_gives_back_everything():
    """cpl_tiny with its atmosphere, both mixed layers, both halves of xforc and every diagnostic switched on and read
    once after a few coupled steps, so that every first-use allocation has happened: closing the two handles brings
    blocks and bytes back to where they were."""
    from qgcm_hip import coupled_steps, oml_preset
    from test_gpu_heat import _cpl_tiny
    base = live()
    o, a = _cpl_tiny(False, True)
    try:
        oc, at = o.cfg, a.cfg
        o.set_sponge(ramp(oc), 1.0e-7)
        o.set_dtopoc(np.zeros((oc.nxpo, oc.nypo), order="F"))
        o.set_monitor_params(oml_preset(oc))
        a.set_atm_monitor_params(ocean=oc)
        o.enable_po_mean()
        o.enable_covariance(12)
        a.enable_covariance(2)
        o.schedule_vorticity_budget(2, 1, capacity=4)
        o.set_areas([0.0, 0.2 * oc.xlo], [oc.xlo, 0.7 * oc.xlo], [0.0, 0.1 * oc.ylo], [oc.ylo, 0.6 * oc.ylo])
        a.set_areas([0.0], [at.xla], [0.0], [at.yla])
        o.helmholtz(np.ones((oc.nxpo, oc.nypo), order="F"), o.bd2oc - o.rdm2oc[1])  # (the tables of tt_tmp)
        coupled_steps(o, a, 1, 6, 3, xforc=True)
        o.sync()
        a.sync()
        # the ocean's diagnostics, once each
        o.monitors()
        o.valids()
        o.prsamp()
        o.tavocn()
        o.time_means()
        o.po_mean()
        o.covocn()
        o.covariance()
        o.read_vorticity_budgets()
        o.vorticity_budget(1)
        o.ocean_dump()
        o.area_averages()
        o.cfl()
        # ... and the atmosphere's
        a.monitors()
        a.atm_valids()
        a.tavatm()
        a.time_means()
        a.covatm()
        a.covariance()
        a.atmos_dump()
        a.area_averages()
        a.cfl()
        held = live()
        assert held[0] > base[0] + 50 and held[1] > base[1]  # (the two handles hold far more buffers than that)
    finally:
        o.close()
        a.close()
    assert live() == base


def test_slab_with_communicator_and_cyclic_ocean_give_back_everything():
    """A box_small y-slab handle that spans the basin, with the mixed layer and a communicator (its exchange buffers
    and all ranks' slab constants), and a cyclic ocean (ybnd, the device copy of the cyclic constraint parameters)."""
    from qgcm_hip import OceanModel, oml_preset
    from qgcm_hip.slab import HipSlab, global_consts, rccl_unique_id
    base = live()
    cfg = preset("box_small")
    consts = global_consts(cfg, lambda rhs, boc: np.zeros_like(rhs))  # any homogeneous solutions will do here
    sl = HipSlab(cfg, consts, 1, cfg.nypo, 0, 1)
    try:
        sl.oml_init(oml_preset(cfg))
        sl.comm_init(rccl_unique_id())
        assert live()[0] > base[0]
    finally:
        sl.close()
    assert live() == base
    g = load_golden("cyc_tiny")
    m = OceanModel(preset("cyc_tiny"))
    try:
        m.set_p(g["in_po"], g["in_pom"])
        m.set_forcing(g["in_wekpo"], g["in_entoc"], g["in_xon"])
        m.set_cyc_forcing(float(g["in_txis"]), float(g["in_txin"]), g["in_enis"], g["in_enin"])
        m.steps(3)
        m.sync()
        assert live()[0] > base[0]
    finally:
        m.close()
    assert live() == base


# 2. set-up calls repeated replace, they do not pile up ----------------------------------------------------------------
SEG_ROWS = 20  # box_tiny has 35 interior rows: two segments of 18 and 17


def box_tiny_model():
    """box_tiny with the mixed layer's fixture loaded (mixed layer not yet on)."""
    from qgcm_hip import OceanModel
    cfg = preset("box_tiny")
    g = load_golden("oml_box_tiny")
    m = OceanModel(cfg)
    return m, g, cfg


@pytest.fixture(scope="module")
def repeated(request):
    """One box_tiny handle taken through every repeated set-up call, with the count after each call: (model, counts).
    The environment variable is set and restored by hand (a module's fixture cannot use monkeypatch)."""
    import os
    m, g, cfg = box_tiny_model()
    request.addfinalizer(m.close)
    om = oml_config(g)
    n = {"start": live()}
    for k in (1, 2):
        m.oml_init(om)
        n["oml_init %d" % k] = live()
    for k, r in enumerate((ramp(cfg), None, ramp(cfg))):
        m.set_sponge(r, 1.0e-7)
        n["sponge %d" % k] = live()
    for k in (1, 2):
        m.set_dtopoc(np.full((cfg.nxpo, cfg.nypo), 10.0, order="F"))
        n["dtopoc %d" % k] = live()
    for k, cap in enumerate((1, 3, 1)):
        m.schedule_vorticity_budget(2, 1, capacity=cap)
        n["ring %d" % k] = live()
    m.schedule_vorticity_budget(2, 0)
    n["ring off"] = live()
    old = os.environ.get("QGCM_HIP_THOMAS_SEG_ROWS")
    try:
        for k, seg in enumerate((None, SEG_ROWS, None, SEG_ROWS, None)):
            if seg is None:
                os.environ.pop("QGCM_HIP_THOMAS_SEG_ROWS", None)
            else:
                os.environ["QGCM_HIP_THOMAS_SEG_ROWS"] = str(seg)
            set_grid_again(m)
            if seg is not None:  # (the segments' second set of tables: the last qgcm_hip_helmholtz's)
                m.helmholtz(np.ones((cfg.nxpo, cfg.nypo), order="F"), m.bd2oc - m.rdm2oc[1])
            n["grid %d" % k] = live()
    finally:
        if old is None:
            os.environ.pop("QGCM_HIP_THOMAS_SEG_ROWS", None)
        else:
            os.environ["QGCM_HIP_THOMAS_SEG_ROWS"] = old
    return m, g, cfg, om, n


def test_repeated_setup_replaces(repeated):
    """oml_init, set_sponge, set_dtopoc, the scheduled dump's ring and set_grid (also under another segment plan and
    back) called again leave the count where the first call left it."""
    n = repeated[4]
    assert n["oml_init 1"][0] == n["start"][0] + 11  # (the mixed layer's eleven buffers)
    assert n["oml_init 2"] == n["oml_init 1"]
    assert n["sponge 0"][0] == n["oml_init 2"][0] + 1 and n["sponge 1"] == n["oml_init 2"] and n["sponge 2"] == n["sponge 0"]
    assert n["dtopoc 1"][0] == n["sponge 2"][0] + 1 and n["dtopoc 2"] == n["dtopoc 1"]
    # the ring is one buffer whatever its capacity; it grows and is not given back before the schedule goes
    assert n["ring 0"][0] == n["ring 1"][0] == n["ring 2"][0] == n["dtopoc 2"][0] + 1
    assert n["ring 0"][1] < n["ring 1"][1] == n["ring 2"][1]
    assert n["ring off"] == n["dtopoc 2"]
    # set_grid again: nothing new.  Under a plan of two segments: the segments' buffers on top, the same ones the second
    # time; back to one segment they are gone (the pivot tables keep the larger size they have grown to)
    assert n["grid 0"] == n["ring off"]
    assert n["grid 1"][0] > n["grid 0"][0]
    assert n["grid 2"][0] == n["grid 0"][0] and n["grid 2"][1] >= n["grid 0"][1]
    assert n["grid 3"] == n["grid 1"]
    assert n["grid 4"] == n["grid 2"]


def test_repeated_setup_of_a_coupled_pair_replaces():
    """aml_init, xforc_setup and xforc_heat_setup, each called twice the same way."""
    from qgcm_hip import xforc_heat_setup, xforc_setup
    import numpy_heat as nh
    from test_gpu_heat import _cpl_tiny, _heat_cfg
    h = nh.load("heat_cpl_tiny")
    P = nh.params(h)
    o, a = _cpl_tiny(False, True)
    try:
        first = live()
        a.aml_init(a.aml_cfg, xc1ast=h["in_xc1ast"], dtopat=h["in_dtopat"])
        assert live() == first
        xforc_setup(o, a, tau_udiff=True)  # (switches the heat half off: set up again below)
        assert live() == first
        xforc_heat_setup(o, a, _heat_cfg(P))
        assert live() == first
    finally:
        o.close()
        a.close()


def test_covariance_off_and_dump_buffer_growth():
    """enable_covariance then qgcm_hip_cov_init(nsi = 0): the count is back where it was.  vorticity_budget at nsko = 2,
    then at nsko = 1 (a longer result): still exactly one dump buffer, grown."""
    from qgcm_hip.lib import check
    m, g, cfg = box_tiny_model()
    try:
        m.set_p(g["in_po"], g["in_pom"])
        before = live()
        m.enable_covariance(12)
        assert live()[0] == before[0] + 8  # two matrices, two means, two deviation vectors, the row sums, the status word
        check(m.L.qgcm_hip_cov_init(m.h, 0, 0, 1))
        assert live() == before
        m.vorticity_budget(nsko=2)
        one = live()
        assert one[0] == before[0] + 1
        m.vorticity_budget(nsko=1)
        two = live()
        assert two[0] == one[0] and two[1] > one[1]
    finally:
        m.close()


# 3. results do not depend on any of it --------------------------------------------------------------------------------
def test_steps_after_repeated_setup_are_those_of_a_fresh_handle(repeated):
    """Three steps of the handle that went through the repeated set-up are bitwise the three steps of a fresh handle
    given the same state and the same settings, each once."""
    m, g, cfg, om, _ = repeated
    fresh, _, _ = box_tiny_model()
    try:
        fresh.oml_init(om)
        fresh.set_sponge(ramp(cfg), 1.0e-7)
        out = []
        for x in (m, fresh):
            oml_load(x, g, cfg, False)
            x.steps(3, s0=1)
            x.sync()
            out.append(list(x.get_state()) + list(x.oml_get_state()))
        assert all(np.isfinite(f).all() for f in out[1])
        assert not np.array_equal(out[1][0], g["in_po"])
        for k, (p, q) in enumerate(zip(*out)):
            same_bits(p, q, "field %d" % k)
    finally:
        fresh.close()
