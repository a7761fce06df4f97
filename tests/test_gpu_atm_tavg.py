"""MI355X parity of the atmosphere's time averages and periodic dump through the C ABI: qgcm_hip_tavatm /
_atm_tav_out / _atm_tav_reset / _tavatm_schedule and qgcm_hip_atnc_sample against the reference's own values
(tests/golden/atav_*.npz) and, at full size, against the numpy restatement tests/numpy_atm_tavg.py of the pulled state,
which reproduces those values (tests/test_atm_tavg_cpu.py).  Every comparison is bitwise."""
import ctypes

import numpy as np
import pytest

import numpy_atm_tavg as na
from numpy_atm_monitors import synthetic_fields
from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, atmos_preset, coupled_steps, preset, share_gpu
from qgcm_hip.model import ATM_TAV_LAYOUT
from test_atm_tavg_cpu import golden_case
from test_gpu_atm_monitors import full_size_atmos

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in ATM_TAV_LAYOUT]
FIELDS = ("tauxa", "tauya", "wekta", "ast", "hmixa")


def fnetat(acfg, seed=5):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(-40.0 + 60.0 * rng.standard_normal((acfg.nxpa - 1, acfg.nypa - 1)))


def same(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    bad = [k for k in a if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    assert not bad, bad


def atmos(name="cpl_natl5"):
    """full_size_atmos (synthetic state, forcing, monitor fields, hmat = 1000) plus fnetat: (model, inputs, consts)."""
    m, fl, _ = full_size_atmos(name)
    acfg = atmos_preset(name)
    fl = dict(fl, fnetat=fnetat(acfg))
    m.set_time_mean_fields(fl["fnetat"])
    return m, fl, na.consts(acfg.dxa, acfg.fnot, 1000.0)


def restated_sum(S, m, fl, c):
    pa, _, qa, _ = m.get_state()
    return na.tavatm(S, dict(fl, pa=pa, qa=qa), c)


@pytest.mark.parametrize("name", ["cpl_tiny", "cpl_small", "cpl_tiny_a4"])
def test_against_the_reference(name):
    g, c, calls, last = golden_case(name)
    acfg = atmos_preset(name)
    m = AtmosModel(acfg)
    try:
        m.set_atm_monitor_params(preset(name), hmat=float(g["c_hmat"]))
        for f in calls:
            m.set_state(f["pa"], f["pa"], f["qa"], f["qa"])
            m.set_atm_monitor_fields(**{k: f[k] for k in FIELDS})
            m.set_time_mean_fields(f["fnetat"])
            m.tavatm()
        got = m.time_means()
        assert got.pop("nsumat") == 3
        same(got, {k: g["out_" + k] for k in NAMES})
        # readout repeats; a subset computes and returns only what was asked
        same(m.time_means(), dict(got, nsumat=3))
        sub = m.time_means(["uptpat", "vptpat", "patav"])
        assert sorted(sub) == ["nsumat", "patav", "uptpat", "vptpat"]
        same({k: sub[k] for k in ("patav", "uptpat", "vptpat")}, {k: got[k] for k in ("patav", "uptpat", "vptpat")})
        # atnc_out of the last state, every flag on and a partial outflat
        for nska in (1, 2, 5):
            d = m.atmos_dump(nska)
            want = {k: (g["n%d_%s" % (nska, k)] if k in ("pa", "qa", "ha") else g["n%d_%s" % (nska, k)][0])
                    for k in na.ATNC_NAMES}
            same(d, want)
            part = m.atmos_dump(nska, outflat=(0, 1, 0, 1, 1, 0, 1))
            same(part, {k: want[k] for k in ("pa", "wekta", "ha", "hmixa")})
        m.reset_time_means()
        z = m.time_means()
        assert z.pop("nsumat") == 0 and all(not np.any(v) for v in z.values())
    finally:
        m.close()


def test_full_size_across_the_averaging_step():
    """cpl_natl5's atmosphere, 130 steps with tavatm() every 10 (the averaging at step 101 included), against the
    restatement of the pulled states."""
    m, fl, c = atmos()
    try:
        S = na.tavini(m.cfg.nxpa, m.cfg.nypa, m.cfg.nla)
        m.steps(0, s0=1)
        for _ in range(13):
            m.steps(10)
            m.tavatm()
            restated_sum(S, m, fl, c)
        got = m.time_means()
        assert got.pop("nsumat") == 13
        same(got, na.tavout(S))
        assert np.any(got["uptpat"]) and np.any(got["vptpat"])
        pa, _, qa, _ = m.get_state()
        d = m.atmos_dump(2)
        want = na.atnc_out(dict(fl, pa=pa, qa=qa), np.asarray(m.cfg.gpat[:m.cfg.nla - 1]), 2)
        same(d, {k: (v if k in ("pa", "qa", "ha") else v[0]) for k, v in want.items()})
    finally:
        m.close()


def test_schedule_equals_explicit_calls():
    """steps(240) with schedule_time_means(every=50, phase=1) against tavatm() after windows that end at 1, 51, 101,
    151 and 201 (the averaging step 101 is one of them)."""
    a, _, _ = atmos()
    b, _, _ = atmos()
    try:
        a.schedule_time_means(50, 1)
        a.steps(240, s0=1)
        b.steps(0, s0=1)
        for n in (1, 50, 50, 50, 50):
            b.steps(n)
            b.tavatm()
        b.steps(39)
        ta, tb = a.time_means(), b.time_means()
        assert ta["nsumat"] == tb["nsumat"] == 5
        same(ta, tb)
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
    finally:
        a.close()
        b.close()


def test_schedule_inside_coupled_steps():
    """The cpl_natl5 pair under share_gpu's CU split: coupled_steps(1, 240, 3) with every=120, phase=60 against
    explicit tavatm() after coupled windows that end at 60 and 180."""
    import test_gpu_monitors as om
    o1, _, _ = om.setup("cpl_natl5", False)
    o2, _, _ = om.setup("cpl_natl5", False)
    a1, _, _ = atmos()
    a2, _, _ = atmos()
    try:
        assert share_gpu(o1, a1) > 0
        a1.schedule_time_means(120, 60)
        coupled_steps(o1, a1, 1, 240, 3)
        assert share_gpu(o2, a2) > 0
        coupled_steps(o2, a2, 1, 60, 3)
        a2.tavatm()
        coupled_steps(o2, a2, 61, 120, 3)
        a2.tavatm()
        coupled_steps(o2, a2, 181, 60, 3)
        t1, t2 = a1.time_means(), a2.time_means()
        assert t1["nsumat"] == t2["nsumat"] == 2
        same(t1, t2)
        for x, y in zip(a1.get_state(), a2.get_state()):
            assert np.array_equal(x, y)
    finally:
        for h in (o1, o2, a1, a2):
            h.close()


def test_no_side_effects():
    """No schedule: the launches of profile_steps are those of a handle that never used the feature.  A schedule: the
    state after the steps is that of a twin without one, and the only extra launches are one k_tavat_accum per
    scheduled step."""
    m, _, _ = atmos()
    t, _, _ = atmos()
    try:
        m.tavatm()
        m.time_means()
        m.atmos_dump(2)
        m.schedule_time_means(7, 3)
        m.schedule_time_means(0)
        pm, pt = m.profile_steps(12, s0=1), t.profile_steps(12, s0=1)
        assert {k: n for k, (_, n) in pm.items()} == {k: n for k, (_, n) in pt.items()}
        assert pm["k_tavat_accum"][1] == 0
        m.schedule_time_means(10, 3)
        on, off = m.profile_steps(30), t.profile_steps(30)  # steps 13..42: scheduled 13, 23, 33
        for k in on:
            if k not in ("k_tavat_accum", "k_noop_train"):
                assert on[k][1] == off[k][1], k
        assert on["k_tavat_accum"][1] == 3 and off["k_tavat_accum"][1] == 0
        m.steps(160)   # graphs cut at the scheduled steps, the averaging at step 101 included
        t.steps(160)
        for x, y in zip(m.get_state(), t.get_state()):
            assert np.array_equal(x, y)
        assert m.time_means(["txatav"])["nsumat"] == 1 + 3 + 16
    finally:
        m.close()
        t.close()


def test_refusals():
    acfg = atmos_preset("cpl_tiny")
    fl = synthetic_fields(acfg, 3)
    m = AtmosModel(acfg)
    o = OceanModel(preset("box_tiny"))
    try:
        with pytest.raises(QgcmHipError, match="hmat is missing"):
            m.tavatm()
        m.set_atm_monitor_params(preset("cpl_tiny"))
        with pytest.raises(QgcmHipError, match="tauxa was never given"):
            m.tavatm()
        # a selected field that was never given; unselected ones need not be set
        with pytest.raises(QgcmHipError, match="ast was never given"):
            m.atmos_dump()
        d = m.atmos_dump(3, outflat=(0, 1, 1, 0, 1, 0, 0))
        assert sorted(d) == ["ha", "pa", "qa"]
        m.set_atm_monitor_fields(**{k: fl[k] for k in FIELDS})
        with pytest.raises(QgcmHipError, match="fnetat was never given"):
            m.tavatm()
        # a scheduled contribution with a missing input fails before anything is launched
        m.schedule_time_means(2, 1)
        s0 = m.get_state()
        with pytest.raises(QgcmHipError, match="fnetat was never given"):
            m.steps(4, s0=1)
        for x, y in zip(s0, m.get_state()):
            assert np.array_equal(x, y)
        m.schedule_time_means(0)
        m.set_time_mean_fields(fnetat(acfg))
        m.tavatm()
        for nska in (0, -2):
            with pytest.raises(QgcmHipError, match="nska = %d" % nska):
                m.atmos_dump(nska)
        for every, phase in ((-1, 0), (10, 10), (10, -1)):
            with pytest.raises(QgcmHipError, match="every|phase"):
                m.schedule_time_means(every, phase)
        # the ocean's entry points still refuse the atmosphere with their current message
        msg = "the handle is an atmosphere \\(only the ocean's time averages are implemented\\)"
        with pytest.raises(QgcmHipError, match=msg):
            m.tavocn()
        with pytest.raises(QgcmHipError, match=msg):
            OceanModel.time_means(m)
        with pytest.raises(QgcmHipError, match=msg):
            OceanModel.reset_time_means(m)
        with pytest.raises(QgcmHipError, match=msg):
            OceanModel.set_time_mean_fields(m, np.zeros((acfg.nxta, acfg.nyta)))
        # an ocean handle
        dp = ctypes.POINTER(ctypes.c_double)
        fl7 = (ctypes.c_int * 7)(*([1] * 7))
        L = o.L
        calls = [lambda: L.qgcm_hip_set_atm_tav_fields(o.h, None), lambda: L.qgcm_hip_tavatm(o.h),
                 lambda: L.qgcm_hip_atm_tav_reset(o.h), lambda: L.qgcm_hip_atm_tav_out(o.h, None, None),
                 lambda: L.qgcm_hip_tavatm_schedule(o.h, 10, 1),
                 lambda: L.qgcm_hip_atnc_sample(o.h, 1, fl7, np.zeros(10).ctypes.data_as(dp))]
        for call in calls:
            assert call() != 0
            assert "the handle is an ocean" in L.qgcm_hip_last_error().decode()
        assert L.qgcm_hip_atnc_sample_len(o.h, 1, fl7) == -1
        assert "the handle is an ocean" in L.qgcm_hip_last_error().decode()
    finally:
        m.close()
        o.close()
