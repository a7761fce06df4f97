"""MI355X parity of the atmosphere monitors and valids through the C ABI: qgcm_hip_atm_monitors (the
atmosphere half of monnc_comp and courat) and qgcm_hip_atm_valids against the reference's own values
(tests/golden/atmon_*.npz) and, at full size, against the numpy restatement tests/numpy_atm_monitors.py of the pulled
state, which reproduces those values (tests/test_atm_monitors_cpu.py).

Bars: extrema, Courant numbers, atstpos / atstval and tmaooc bit exact; every area integral within 1e-12 of the
integral of the modulus of its integrand (the restatement's `scales`)."""
import numpy as np
import pytest

import numpy_atm_monitors as na
from numpy_atm_monitors import synthetic_fields
from common import atm_apply
from qgcm_hip import AtmosModel, QgcmHipError, atmos_preset, coupled_steps, preset, share_gpu, synth
from test_atm_monitors_cpu import EXACT, golden_case

pytestmark = pytest.mark.gpu

TOL = 1e-12
FIELDS = ("wekta", "tauxa", "tauya", "ast", "hmixa", "uekat", "vekat")


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


def consts(acfg, p):
    """The restatement's constants for the atmosphere acfg and the params struct p."""
    nl = acfg.nla
    return dict(dxa=acfg.dxa, dta=acfg.dta, fnot=acfg.fnot, gpat=np.asarray(acfg.gpat[:nl - 1]),
                hat=np.asarray(acfg.hat[:nl]), ah4at=np.asarray(acfg.ah4at[:nl]), rhoat=p.rhoat, cpat=p.cpat,
                hmat=p.hmat, davgat=p.davgat, aup=np.array(p.aup[:nl - 1]), bup=p.bup, cup=p.cup, dup=p.dup,
                nx1=p.nx1, ny1=p.ny1, nxaooc=p.nxaooc, nyaooc=p.nyaooc)


MONKW = dict(davgat=37.5, aup=[0.05, 0.1], bup=0.31, cup=-4.0e-3, dup=1.7)


def full_size_atmos(name="cpl_natl5"):
    """An AtmosModel at the coupled preset `name` with synthetic state, forcing and monitor inputs."""
    from qgcm_hip.model import atm_mon_params
    acfg, ocfg = atmos_preset(name), preset(name)
    s = synth.atmos_fields(acfg)
    m = AtmosModel(acfg, ddynat=s["ddynat"])
    atm_apply(m, s)
    fl = synthetic_fields(acfg, 3)
    m.set_atm_monitor_params(ocfg, **MONKW)
    m.set_atm_monitor_fields(**fl)
    return m, dict(fl, wekpa=s["wekpa"], entat=s["entat"]), consts(acfg, atm_mon_params(acfg, ocfg, **MONKW))


def restated(m, fl, c):
    pa, pam, qa, _ = m.get_state()
    return na.monitors(dict(fl, pa=pa, pam=pam, qa=qa), c)


@pytest.mark.parametrize("name", ["cpl_tiny", "cpl_small", "cpl_tiny_a4"])
def test_against_the_reference(name):
    f, c, want, val, ok = golden_case(name)
    _, scales = na.monitors(f, c)
    acfg = atmos_preset(name)
    m = AtmosModel(acfg)
    try:
        m.set_state(f["pa"], f["pam"], f["qa"], f["qa"])
        m.set_forcing(f["wekpa"], f["entat"], np.zeros(acfg.nla - 1))
        m.set_atm_monitor_params(nx1=int(c["nx1"]), ny1=int(c["ny1"]), nxaooc=int(c["nxaooc"]),
                                 nyaooc=int(c["nyaooc"]), rhoat=c["rhoat"], cpat=c["cpat"], hmat=c["hmat"],
                                 davgat=c["davgat"], aup=c["aup"], bup=c["bup"], cup=c["cup"], dup=c["dup"])
        m.set_atm_monitor_fields(**{k: f[k] for k in FIELDS})
        compare(m.monitors(), want, scales)
        good, out = m.atm_valids()
        assert np.array_equal(out, val) and good == bool(ok[0])
    finally:
        m.close()


def test_full_size_across_the_averaging_step():
    """cpl_natl5's atmosphere, 130 steps (the averaging at step 101 included): the device against the restatement
    of the pulled state."""
    m, fl, c = full_size_atmos()
    try:
        m.steps(130, s0=1)
        want, scales = restated(m, fl, c)
        got = m.monitors()
        compare(got, want, scales)
        assert np.all(got["atstpos"] > 0) and np.all(got["ddtkeat"] != 0.0)
    finally:
        m.close()


def test_coupled_window_both_halves():
    """qgcm_hip_coupled_steps on the cpl_natl5 pair with the CU split of share_gpu: the ocean's and the atmosphere's
    monitors against their restatements."""
    import test_gpu_monitors as om
    o, oml, ofl = om.setup("cpl_natl5", False)
    a, fl, c = full_size_atmos()
    try:
        assert share_gpu(o, a) > 0
        coupled_steps(o, a, 1, 48, 3)
        want, scales = om.reference(o, oml, ofl, False)
        om.compare(o.monitors(), want, scales)
        want, scales = restated(a, fl, c)
        compare(a.monitors(), want, scales)
    finally:
        o.close()
        a.close()


def test_no_side_effects_and_reproducible():
    """Two calls give bitwise-equal vectors and leave the state bitwise unchanged; a twin stepped without calls
    ends bitwise equal; the step's launches are the same with and without calls."""
    m, _, _ = full_size_atmos()
    t, _, _ = full_size_atmos()
    try:
        m.steps(20, s0=1)
        t.steps(20, s0=1)
        s0 = m.get_state()
        v1, v2 = m.monitor_vector(), m.monitor_vector()
        m.atm_valids()
        assert np.array_equal(v1, v2)
        for x, y in zip(s0, m.get_state()):
            assert np.array_equal(x, y)
        m.steps(30)
        t.steps(30)
        for x, y in zip(m.get_state(), t.get_state()):
            assert np.array_equal(x, y)
        pm = m.profile_steps(5)
        m.monitors()
        pt = t.profile_steps(5)
        assert {k: n for k, (_, n) in pm.items()} == {k: n for k, (_, n) in pt.items()}
        for x, y in zip(m.get_state(), t.get_state()):
            assert np.array_equal(x, y)
    finally:
        m.close()
        t.close()


def test_refusals():
    from qgcm_hip import OceanModel
    acfg, ocfg = atmos_preset("cpl_tiny"), preset("cpl_tiny")
    s = synth.atmos_fields(acfg)
    fl = synthetic_fields(acfg, 3)
    m = AtmosModel(acfg, ddynat=s["ddynat"])
    o = OceanModel(preset("box_tiny"))
    try:
        atm_apply(m, s)
        with pytest.raises(QgcmHipError, match="set_atm_mon_params has not been called"):
            m.monitors()
        m.set_atm_monitor_params(ocfg)
        with pytest.raises(QgcmHipError, match="wekta was never given"):
            m.monitors()
        with pytest.raises(QgcmHipError, match="wekta was never given"):
            m.atm_valids()
        m.set_atm_monitor_fields(**{k: fl[k] for k in FIELDS if k != "vekat"})
        m.atm_valids()   # valids reads no vekat
        with pytest.raises(QgcmHipError, match="vekat was never given"):
            m.monitors()
        with pytest.raises(QgcmHipError, match="do not lie on"):
            m.set_atm_monitor_params(nxaooc=acfg.nxta + 1, nyaooc=1)
        # qgcm_hip_monitors on the atmosphere still refuses with its own message
        import ctypes
        with pytest.raises(QgcmHipError, match="only the ocean half of monnc_comp is implemented"):
            from qgcm_hip.model import OceanModel as OM
            OM.monitor_vector(m)
        # an ocean handle
        for call in (lambda: o.L.qgcm_hip_atm_monitors(o.h, np.zeros(100).ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                     lambda: o.L.qgcm_hip_atm_valids(o.h, np.zeros(12).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                      ctypes.byref(ctypes.c_int()))):
            assert call() != 0
            assert "the handle is an ocean" in o.L.qgcm_hip_last_error().decode()
        assert o.L.qgcm_hip_atm_monitor_len(o.h) == -1
    finally:
        m.close()
        o.close()


def test_refuses_a_y_slab_handle():
    """An atmosphere cannot be split into y-slabs: qgcm_hip_create refuses the handle, so the entry points' own y-slab
    refusal is never reached from a handle that exists."""
    import ctypes
    from qgcm_hip.lib import Params, load_library
    acfg = atmos_preset("cpl_tiny")
    base = AtmosModel(acfg)
    p = Params.from_buffer_copy(base.params)
    base.close()
    p.slab_g0, p.slab_g1 = 1, acfg.nypa // 2
    L = load_library()
    h = ctypes.c_void_p()
    assert L.qgcm_hip_create(ctypes.byref(h), ctypes.byref(p), -1) != 0
    assert "y-slabs are implemented for the oceans only" in L.qgcm_hip_last_error().decode()
    assert not h.value


def test_atm_valids_flags_bad_ast():
    """Bitwise extrema, and solnok false with the right extremum when ast = 95 at one point (bad data handed in)."""
    m, fl, _ = full_size_atmos()
    try:
        m.steps(10, s0=1)
        pa, _, qa, _ = m.get_state()
        good, out = m.atm_valids()
        assert good and np.array_equal(out, na.valids(dict(fl, pa=pa, qa=qa)))
        ast = fl["ast"].copy(order="F")
        ast[17, 23] = 95.0
        m.set_atm_monitor_fields(ast=ast)
        good, out = m.atm_valids()
        assert not good and out[5] == 95.0 and np.array_equal(out, na.valids(dict(fl, ast=ast, pa=pa, qa=qa)))
    finally:
        m.close()
