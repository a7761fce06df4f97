"""The ocean's time averages on the device: the fork's running mean of po (avg_ocn_k247 /
ocnc_avgout_k247) and tavocn / tavout, against the golden values of the reference (tests/golden/tav_*.npz) and the
numpy restatement tests/numpy_tavg.py of pulled states.  Every comparison is bitwise.

The running mean sees each step's po after ocqbdy and before the leapfrog averaging.  With one step per call,
po_mean(reset=True) returns that po exactly (1/1 = 1); the test checks it against the state after the step: equal on
ordinary steps, and po == 0.5*(that po + pom) on averaging steps (k_lf_average's expression)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import numpy_tavg as nt
from common import load_golden
from qgcm_hip import OceanModel, oml_preset, preset, synth
from qgcm_hip.slab import partition
from test_gpu_slab_diagnostics import close, gathered_model, make_slabs, slabs_like, stepped_slabs
from test_tavg_cpu import CASES, LAYER_CASES, calls, golden_consts, load_tav

pytestmark = pytest.mark.gpu
NAMES = nt.SUM_NAMES + ("uptpoc", "vptpoc")


def same(got, want):
    for n in NAMES:
        assert got[n].shape == want[n].shape, n
        assert np.array_equal(got[n], want[n]), n


# 1. golden values of the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + LAYER_CASES)
@pytest.mark.parametrize("mixed_layer", [False, True])
def test_golden_time_means(case, mixed_layer):
    g = load_tav(case)
    cfg = preset(case[:-3] if case.endswith("_sb") else case)  # the fixture's grid and layers
    assert bool(cfg.cyclic) == bool(g["c_cyclic"]) and (cfg.nxpo, cfg.nypo, cfg.nlo) == g["in0_po"].shape
    om = oml_preset(cfg, sb_hflux=bool(g["c_sb_hflux"]), nb_hflux=bool(g["c_nb_hflux"]))
    m = OceanModel(cfg)
    try:
        if mixed_layer:
            m.oml_init(om)  # tavocn then takes hmoc, ycexp, tsbdy, tnbdy and the flags from the mixed layer
        else:
            m.set_time_mean_params(om)
        assert m.time_means()["nsumoc"] == 0
        for f in calls(g):
            m.set_state(f["po"], f["po"], f["qo"], f["qo"])
            m.set_forcing(f["wekpo"], np.zeros_like(f["wekpo"]), np.zeros(cfg.nlo - 1))
            if mixed_layer:
                m.oml_set_state(f["sst"], f["sst"])
                m.oml_set_forcing(f["fnetoc"], f["wekto"], f["tauxo"], f["tauyo"])
            else:
                m.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
                m.set_time_mean_fields(f["fnetoc"])
            m.tavocn()
        got = m.time_means()
        assert got["nsumoc"] == 3
        same(got, {n: g["out_" + n] for n in NAMES})
        same(m.time_means(), got)  # reading does not consume the sums
        part = m.time_means(["uptpoc", "sstav"])
        assert sorted(part) == ["nsumoc", "sstav", "uptpoc"] and np.array_equal(part["uptpoc"], got["uptpoc"])
        m.reset_time_means()
        z = m.time_means()
        assert z["nsumoc"] == 0 and not any(np.any(z[n]) for n in NAMES)  # rnsoc = 0 when nsumoc = 0
    finally:
        m.close()


# 2. the running mean of po across steps ------------------------------------------------------------------------------
def ocean(cfgname, mixed_layer):
    cfg = preset(cfgname) if isinstance(cfgname, str) else cfgname  # a preset's name or a configuration
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    m = OceanModel(cfg)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    m.set_p(po, np.asfortranarray(0.999 * po))
    m.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(cfg.nlo - 1))
    if cfg.cyclic:
        txis, txin = synth.tau_line_integrals(cfg, tx)
        m.set_cyc_forcing(txis, txin, np.zeros(cfg.nlo - 1), np.zeros(cfg.nlo - 1))
    if mixed_layer:
        m.oml_init(om)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
    else:
        m.set_time_mean_params(om)
        m.set_monitor_fields(tx, ty, wekto, sst)
        m.set_time_mean_fields(fnet)
    return m


def per_step_po(m, s, n):
    """n single steps from s: the po each step adds, checked against the state after it; their numpy sum."""
    tot = None
    for k in range(s, s + n):
        m.steps(1, s0=k)
        pre, cnt = m.po_mean(reset=True, count=True)
        assert cnt == 1
        po, pom, _, _ = m.get_state()
        if (k - 1) % 25 == 0:
            assert np.array_equal(po, 0.5 * (pre + pom)) and not np.array_equal(po, pre), k
        else:
            assert np.array_equal(po, pre), k
        tot = pre if tot is None else tot + pre
    return tot


@pytest.mark.parametrize("cfgname,mixed_layer,fused", [("natl5", False, True), ("natl5", False, False),
                                                        ("socn5", False, True), ("natl5", True, True)])
def test_po_mean_over_60_steps(cfgname, mixed_layer, fused, monkeypatch):
    if not fused:
        monkeypatch.setenv("QGCM_HIP_NO_FUSED_AVG", "1")  # read when a handle is created
    a, b, c = ocean(cfgname, mixed_layer), ocean(cfgname, mixed_layer), ocean(cfgname, mixed_layer)
    try:
        a.enable_po_mean()
        a.steps(60, s0=1)  # steps 1, 26, 51 average
        mean, n = a.po_mean(count=True)
        assert n == 60
        b.enable_po_mean()
        tot = per_step_po(b, 1, 60)
        assert np.array_equal(mean, nt.po_mean(tot, 60))
        assert np.array_equal(mean, a.po_mean())  # reading without reset keeps the sum
        c.steps(60, s0=1)  # never enabled: the same state, bitwise
        for x, y in zip(a.get_state(), c.get_state()):
            assert np.array_equal(x, y)
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        # reset: the mean after a reset counts only the later steps
        a.po_mean(reset=True)
        a.steps(30, s0=61)
        c.enable_po_mean()
        tot = per_step_po(c, 61, 30)
        got, n = a.po_mean(count=True)
        assert n == 30 and np.array_equal(got, nt.po_mean(tot, 30))
        # switched off: the sum stays, nothing is added
        a.enable_po_mean(False)
        a.steps(4, s0=91)
        assert np.array_equal(a.po_mean(), got)
    finally:
        for m in (a, b, c):
            m.close()


def test_launch_sequence_unchanged_when_never_enabled():
    m = ocean("natl5", False)
    try:
        off = m.profile_steps(30, s0=1)
        assert off["k_poavg_add"][1] == 0
        m2 = ocean("natl5", False)
        try:
            m2.enable_po_mean()
            on = m2.profile_steps(30, s0=1)
        finally:
            m2.close()
        assert on["k_poavg_add"][1] == 30
        for k in off:  # the averaging step of an accumulating run is the unfused one: one k_lf_average either way
            if k not in ("k_poavg_add", "k_noop_train"):
                assert on[k][1] == off[k][1], k
    finally:
        m.close()


# 3. tavocn at full size, interleaved with steps --------------------------------------------------------------------
def host_fields(m, cfgname, mixed_layer, f):
    po, _, qo, _ = m.get_state()
    out = dict(f, po=po, qo=qo)
    if mixed_layer:
        out["sst"] = m.oml_get_state()[0]
    return out


@pytest.mark.parametrize("cfgname,mixed_layer", [("natl5", False), ("socn5", False), ("natl5", True)])
def test_full_size_tavocn(cfgname, mixed_layer):
    cfg = preset(cfgname)
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, fnetoc=fnet)
    c = nt.consts(cfg.dxo, cfg.fnot, om.ycexp, om.hmoc, om.tsbdy, om.tnbdy, cfg.cyclic, om.sb_hflux, om.nb_hflux)
    m = ocean(cfgname, mixed_layer)
    try:
        S = nt.tavini(cfg.nxpo, cfg.nypo, cfg.nlo)
        for n in (3, 23, 1, 9):  # the second call follows the averaging step 26
            m.steps(n)
            m.tavocn()
            nt.tavocn(S, host_fields(m, cfgname, mixed_layer, f), c)
        got = m.time_means()
        assert got["nsumoc"] == 4
        same(got, nt.tavout(S))
    finally:
        m.close()


# 4. y-slabs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,mixed_layer", [("natl5", False), ("natl5", True), ("socn5", False)])
def test_slab_time_means_equal_whole_domain(cfgname, mixed_layer):
    m = ocean(cfgname, mixed_layer)
    cfg = m.cfg
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, entoc=np.zeros_like(wekpo))
    try:
        m.steps(26, s0=1)  # ends with an averaging step
        m.tavocn()
        whole = m.time_means()
        for nranks in (2, 3, 8):
            so = slabs_like(m, om, f, mixed_layer, partition(cfg.nypo, nranks))
            try:
                if mixed_layer:
                    for x in so.slabs:  # slabs_like gives the slabs a zero fnetoc
                        x.oml_set_forcing(fnet, wekto, tx, ty)
                else:
                    so.set_time_mean_params(om)
                    so.set_time_mean_fields(fnet)
                so.tavocn()
                got = so.time_means()
                assert got["nsumoc"] == 1
                same(got, whole)
            finally:
                close(so)
    finally:
        m.close()


@pytest.mark.parametrize("early", [False, True])
def test_slab_steps_po_mean_and_halo_rows(early):
    """Slab steps across the averaging step 26: the per-step po of the slabs against the gathered state, and tavocn on the slabs against a whole-domain handle holding the
    gathered state (the flux terms at the slab edges read the halo rows)."""
    so, om, f = stepped_slabs("box_med", 3, early)
    f = dict(f, fnetoc=np.zeros_like(f["sst"]))
    so.set_time_mean_params(om)
    try:
        so.steps(20)
        so.enable_po_mean()
        for k in range(21, 31):
            so.steps(1, s0=k)
            pre = so.po_mean(reset=True)
            m = gathered_model(so, om, f)
            try:
                po, pom, _, _ = m.get_state()
                if (k - 1) % 25 == 0:
                    assert np.array_equal(po, 0.5 * (pre + pom)), k
                else:
                    assert np.array_equal(po, pre), k
                if k in (26, 28):
                    so.reset_time_means()
                    so.tavocn()
                    m.set_time_mean_params(om)
                    m.tavocn()
                    same(so.time_means(), m.time_means())
            finally:
                m.close()
    finally:
        close(so)
