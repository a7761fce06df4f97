"""MI355X parity of the ocean monitors through the C ABI: qgcm_hip_monitors (the ocean half of
monnc_comp and couroc, src/monitor_diag.F) against the numpy restatement tests/numpy_monitors.py of the pulled state.

First against the golden values of the TRUE reference (tests/golden/mon_*.npz, make_golden_monnc.py: the
reference's own monnc_comp on the tiny fixtures' states), then at full size against the restatement, which reproduces
those golden values (tests/test_monitors_cpu.py).

Bars: the extrema (po, sst, couroc's velocities, Courant numbers), everything derived from them pointwise (osfmin,
osfmax, occirc, occtot) and the jet position and value (ocjpos, ocjval: serial zonal sums as in the reference) bit
exact; every area integral within 1e-12 of the integral of the modulus of its integrand (the restatement's `scales`:
wetmoc, utauoc, ddtkeoc ... are near zero by construction)."""
import ctypes

import numpy as np
import pytest

from common import load_golden
from numpy_monitors import monitors as np_monitors
from qgcm_hip import OceanModel, QgcmHipError, check, oml_preset, preset, synth
from qgcm_hip.model import unpack_monitors

pytestmark = pytest.mark.gpu

EXACT = ("sstmin", "sstmax", "umminoc", "ummaxoc", "vmminoc", "vmmaxoc", "cnmloc", "ugminoc", "ugmaxoc", "vgminoc",
         "vgmaxoc", "cnqgoc", "osfmin", "osfmax", "occirc", "occtot", "ocjpos", "ocjval")
TOL = 1e-12
GOLDEN_CASES = ["box_tiny", "cyc_tiny", "box_tiny5", "box_tiny2", "cyc_tiny6"]


def entoc_field(cfg):
    x = np.arange(cfg.nxpo)[:, None] / (cfg.nxpo - 1.0)
    y = np.arange(cfg.nypo)[None, :] / (cfg.nypo - 1.0)
    e = 2.0e-6 * np.sin(np.pi * y) * np.cos(2.0 * np.pi * x) + 5.0e-7 * y
    if cfg.cyclic:
        e[-1, :] = e[0, :]
    return np.asfortranarray(e)


def setup(cfgname, mixed_layer):
    """A model with an eddy state, wind, a non-zero entrainment and (with or without the mixed layer) the fields the
    monitors read; returns (model, fields the state does not carry).  cfgname: a preset's name or a configuration."""
    cfg = preset(cfgname) if isinstance(cfgname, str) else cfgname
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    m = OceanModel(cfg)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    entoc = entoc_field(cfg)
    m.set_p(po, po)
    m.set_forcing(wekpo, entoc, np.zeros(cfg.nlo - 1))
    if cfg.cyclic:
        txis, txin = synth.tau_line_integrals(cfg, tx)
        m.set_cyc_forcing(txis, txin, np.zeros(cfg.nlo - 1), np.zeros(cfg.nlo - 1))
    m.set_monitor_params(om)
    if mixed_layer:
        m.oml_init(om)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
    else:
        m.set_monitor_fields(tx, ty, wekto, sst)
    return m, om, dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, entoc=entoc)


def reference(m, om, f, mixed_layer):
    """The restatement on what the device holds now."""
    cfg = m.cfg
    po, pom, qo, _ = m.get_state()
    f = dict(f, po=po, pom=pom, qo=qo)
    if mixed_layer:
        f["sst"] = m.oml_get_state()[0]
        f["entoc"] = m.oml_get_diag()[0]
    c = dict(cyclic=cfg.cyclic, fnot=cfg.fnot, dxo=cfg.dxo, dto=cfg.dto, gpoc=cfg.gpoc[:cfg.nlo - 1], hoc=cfg.hoc,
             ah2oc=cfg.ah2oc, ah4oc=cfg.ah4oc, delek=cfg.delek, rhooc=om.rhooc, cpoc=om.cpoc, hmoc=om.hmoc,
             ycexp=om.ycexp, sb_hflux=om.sb_hflux, nb_hflux=om.nb_hflux)
    return np_monitors(f, c)


def compare(got, want, scales):
    bad = []
    for name, ref in want.items():
        g, r, s = np.atleast_1d(got[name]), np.atleast_1d(ref), np.atleast_1d(scales[name])
        if name in EXACT:
            if not np.array_equal(g, r):
                bad.append((name, g, r))
        elif np.any(np.abs(g - r) > TOL * s + 1e-300):
            bad.append((name, g, r, s))
    assert not bad, bad


def run(cfgname, nsteps, mixed_layer):
    m, om, f = setup(cfgname, mixed_layer)
    try:
        if nsteps:
            m.steps(nsteps, s0=1)
        got = m.monitors()
        want, scales = reference(m, om, f, mixed_layer)
        assert set(got) == set(want)
        compare(got, want, scales)
        return got, want
    finally:
        m.close()


def golden_case(name):
    """Inputs, constants and the reference's packed result of tests/golden/mon_<name>.npz."""
    g = load_golden("mon_" + name)
    cfg = preset(name)
    f = {k[3:]: g[k] for k in g if k.startswith("in_")}
    c = {k[2:]: float(g[k]) for k in g if k.startswith("c_")}
    c.update(cyclic=cfg.cyclic, fnot=cfg.fnot, gpoc=cfg.gpoc[:cfg.nlo - 1], hoc=cfg.hoc[:cfg.nlo],
             ah2oc=cfg.ah2oc[:cfg.nlo], ah4oc=cfg.ah4oc[:cfg.nlo])
    return cfg, f, c, unpack_monitors(g["monitors"], cfg.nlo)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_against_the_reference(name):
    cfg, f, c, want = golden_case(name)
    _, scales = np_monitors(f, c)
    m = OceanModel(cfg)
    try:
        m.set_state(f["po"], f["pom"], f["qo"], f["qom"])
        m.set_forcing(f["wekpo"], f["entoc"], np.zeros(cfg.nlo - 1))
        m.set_monitor_params(rhooc=c["rhooc"], cpoc=c["cpoc"], hmoc=c["hmoc"], ycexp=c["ycexp"],
                             sb_hflux=bool(c["sb_hflux"]), nb_hflux=bool(c["nb_hflux"]))
        m.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
        compare(m.monitors(), want, scales)
    finally:
        m.close()


@pytest.mark.parametrize("cfgname", ["box_tiny", "cyc_tiny", "box_tiny5"])
@pytest.mark.parametrize("mixed_layer", [False, True])
def test_small_cases(cfgname, mixed_layer):
    got, want = run(cfgname, 10, mixed_layer)
    # the rate terms see po != pom and the entrainment terms a non-zero entoc
    assert np.all(want["ddtkeoc"] != 0.0) and want["pkenoc"] != 0.0 and want["entmoc"] != 0.0


@pytest.mark.parametrize("cfgname", ["box_small", "cyc_small", "natl5", "socn5"])
@pytest.mark.parametrize("mixed_layer", [False, True])
def test_full_size_after_60_steps(cfgname, mixed_layer):
    run(cfgname, 60, mixed_layer)


def test_averaging_step_reads_the_averaged_levels():
    """Step 26 ends with the fused leapfrog averaging ((s-1) mod 25 == 0): the monitors read the averaged levels,
    the ones qgcm_hip_get_state hands out."""
    run("box_small", 26, True)


def test_no_side_effects_and_reproducible():
    m, om, f = setup("cyc_small", True)
    m2, _, _ = setup("cyc_small", True)
    try:
        m.steps(50, s0=1)
        before = m.get_state() + list(m.oml_get_state())
        a = m.monitor_vector()
        b = m.monitor_vector()
        assert np.array_equal(a, b)
        after = m.get_state() + list(m.oml_get_state())
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        m.steps(50, s0=51)
        m2.steps(100, s0=1)
        assert all(np.array_equal(x, y) for x, y in zip(m.get_state(), m2.get_state()))
        assert all(np.array_equal(x, y) for x, y in zip(m.oml_get_state(), m2.oml_get_state()))
    finally:
        m.close()
        m2.close()


def test_refusals():
    cfg = preset("box_tiny")
    m = OceanModel(cfg)
    try:
        with pytest.raises(QgcmHipError, match="qgcm_hip_set_mon_params"):
            m.monitors()
        m.set_monitor_params()
        with pytest.raises(QgcmHipError, match="tauxo was never given"):
            m.monitors()
        tx, ty = synth.wind_stress(cfg)
        wekto, _ = synth.wekpo_from_tau(cfg, tx, ty)
        m.set_monitor_fields(tx, ty, wekto)
        with pytest.raises(QgcmHipError, match="sst was never given"):
            m.monitors()
        m.set_monitor_fields(sst=np.zeros((cfg.nxto, cfg.nyto)))
        assert len(m.monitor_vector()) == 19 * cfg.nlo + 16
    finally:
        m.close()


def test_slab_handle_refuses():
    from common import make_oracle
    from qgcm_hip.slab import HipSlab, global_consts, partition
    cfg = preset("box_small")
    o = make_oracle(cfg)
    try:
        consts = global_consts(cfg, o.helmholtz)
    finally:
        o.close()
    (g0, g1), _ = partition(cfg.nypo, 2)
    sl = HipSlab(cfg, consts, g0, g1, 0, 2)
    try:
        out = np.zeros(19 * cfg.nlo + 16)
        with pytest.raises(QgcmHipError, match="whole domain"):
            check(sl.L.qgcm_hip_monitors(sl.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    finally:
        sl.close()
