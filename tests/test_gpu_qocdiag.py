"""The ocean's periodic dumps on the device: qocdiag_out's vorticity budget and ocnc_out's subsample
against the golden values of the reference (tests/golden/qod_*.npz) and the numpy restatement
tests/numpy_qocdiag.py of pulled states; the schedule inside steps(); y-slabs against the whole-domain handle.  Every
comparison is bitwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import numpy_qocdiag as nq
from common import load_golden
from qgcm_hip import OceanModel, QgcmHipError, preset
from qgcm_hip.slab import partition
from test_gpu_monitors import setup
from test_gpu_slab_diagnostics import close, load, make_slabs
from test_qocdiag_cpu import CASES, NC_NAMES, NSKO, golden_inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLAT = ("sst", "wekto", "tauxo", "tauyo")  # one plane: OceanModel.ocean_dump returns them as 2-d arrays


def same(got, want, names=nq.TERMS):
    for n in names:
        assert got[n].shape == want[n].shape, n
        assert np.array_equal(got[n], want[n]), n


def golden_model(case):
    g = load_golden("qod_" + case)
    cfg = preset(case)
    f = golden_inputs(g)
    m = OceanModel(cfg)
    m.set_state(f["po"], f["pom"], f["qo"], f["qom"])
    m.set_forcing(f["wekpo"], f["entoc"], np.zeros(cfg.nlo - 1))
    m.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
    return g, cfg, f, m


# 1. golden values of the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_golden(case):
    g, cfg, f, m = golden_model(case)
    try:
        for nsko in NSKO:
            got = m.vorticity_budget(nsko)
            for t in nq.TERMS:
                key = "n%d_qd_%s" % (nsko, t)
                want = g[key] if key in g else np.zeros_like(got["dqdt"])  # qt2dif: zero when every ah2oc is 0
                assert np.array_equal(got[t], want), (nsko, t)
            d = m.ocean_dump(nsko)
            assert sorted(d) == sorted(NC_NAMES) and "sst" in d
            for name, v in d.items():
                w = g["n%d_nc_%s" % (nsko, NC_NAMES[name])]
                assert np.array_equal(v, w[0] if name in ("sst", "wekto", "tauxo", "tauyo") else w), (nsko, name)
            part = m.ocean_dump(nsko, (0, 1, 0, 0, 1, 0, 1))
            assert sorted(part) == ["h", "po"]
        # the state is not changed
        for x, y in zip(m.get_state(), (f["po"], f["pom"], f["qo"], f["qom"])):
            assert np.array_equal(x, y)
    finally:
        m.close()


def test_ocean_dump_names_a_missing_field():
    cfg = preset("box_tiny")
    m = OceanModel(cfg)
    try:
        with pytest.raises(QgcmHipError, match="sst"):
            m.ocean_dump(1)
        assert sorted(m.ocean_dump(2, (0, 1, 1, 0, 1, 0, 0))) == ["h", "po", "qo"]  # no forcing field asked for
    finally:
        m.close()


# 2. full size against the restatement --------------------------------------------------------------------------------
def restated(m, f, mixed_layer, nsko):
    po, pom, qo, qom = m.get_state()
    entoc = m.oml_get_diag()[0] if mixed_layer else f["entoc"]
    return nq.budget(po, pom, qo, qom, f["wekpo"], entoc, nq.consts(m.cfg), nsko)


@pytest.mark.parametrize("cfgname", ["natl5", "socn5"])
@pytest.mark.parametrize("mixed_layer", [False, True])
def test_full_size(cfgname, mixed_layer):
    m, om, f = setup(cfgname, mixed_layer)
    try:
        m.steps(26, s0=1)  # steps 1 and 26 average
        for nsko in (1, 2):
            same(m.vorticity_budget(nsko), restated(m, f, mixed_layer, nsko))
        po, _, qo, _ = m.get_state()
        sst = m.oml_get_state()[0] if mixed_layer else f["sst"]
        want = nq.ocnc(sst, po, qo, f["wekto"], f["tauxo"], f["tauyo"], m.cfg.gpoc, 2)
        got = m.ocean_dump(2)  # (with the mixed layer: sst, wekto, tauxo, tauyo from its arrays, T pitch ldt)
        assert sorted(got) == sorted(want)
        for n in want:
            assert np.array_equal(got[n], want[n][0] if n in FLAT else want[n]), n
    finally:
        m.close()


# 3. the schedule inside steps() ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["natl5", "socn5"])
def test_scheduled_dump_is_taken_after_oml(cfgname):
    """Mixed layer on: the snapshot of step 26 equals a twin stepped to 25 that calls oml() then vorticity_budget(),
    and differs from the budget between steps (entoc of the step just taken)."""
    a, _, f = setup(cfgname, True)
    b, _, _ = setup(cfgname, True)
    try:
        a.schedule_vorticity_budget(2, 25, capacity=2)
        a.steps(26, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 26]
        assert a.read_vorticity_budgets() == []
        b.steps(25, s0=1)
        between = b.vorticity_budget(2)
        b.oml()
        twin = b.vorticity_budget(2)
        same(snaps[1][1], twin)
        assert not np.array_equal(snaps[1][1]["qotent"], between["qotent"])
    finally:
        a.close()
        b.close()


def test_scheduled_dump_without_mixed_layer_equals_between_steps():
    a, _, _ = setup("natl5", False)
    b, _, _ = setup("natl5", False)
    try:
        a.schedule_vorticity_budget(1, 10, capacity=3)
        a.steps(21, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 11, 21]
        for s0, n in ((1, 0), (1, 10), (11, 10)):
            b.steps(n, s0=s0)
            same(snaps[(s0 + n - 1) // 10][1], b.vorticity_budget(1))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mixed_layer", [False, True])
def test_schedule_leaves_the_state_bitwise(mixed_layer):
    a, _, _ = setup("natl5", mixed_layer)
    b, _, _ = setup("natl5", mixed_layer)
    try:
        a.schedule_vorticity_budget(2, 25, capacity=5)
        a.prepare_steps(120, s0=1)
        a.steps(120, s0=1)
        b.steps(120, s0=1)
        assert [s for s, _ in a.read_vorticity_budgets()] == [1, 26, 51, 76, 101]
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        if mixed_layer:
            for x, y in zip(a.oml_get_state(), b.oml_get_state()):
                assert np.array_equal(x, y)
    finally:
        a.close()
        b.close()


def test_profile_shows_the_same_launches_on_non_dump_steps():
    a, _, _ = setup("natl5", True)
    b, _, _ = setup("natl5", True)
    try:
        a.schedule_vorticity_budget(1, 100, capacity=1)  # dumps at 1, 101: none in steps 2..31
        a.steps(1, s0=1)
        b.steps(1, s0=1)
        on, off = a.profile_steps(30, s0=2), b.profile_steps(30, s0=2)
        for k in off:
            if k != "k_noop_train":
                assert on[k][1] == off[k][1], k
    finally:
        a.close()
        b.close()


def test_ring_overflow_fails_before_stepping():
    a, _, _ = setup("natl5", False)
    try:
        a.schedule_vorticity_budget(2, 5, capacity=2)
        before = a.get_state()
        with pytest.raises(QgcmHipError, match="ring"):
            a.steps(11, s0=1)  # dumps at 1, 6, 11
        for x, y in zip(a.get_state(), before):
            assert np.array_equal(x, y)
        a.steps(10, s0=1)
        assert [s for s, _ in a.read_vorticity_budgets()] == [1, 6]
        a.schedule_vorticity_budget(0, 0)
        a.steps(10, s0=11)  # no schedule: nothing recorded, nothing refused
        assert a.read_vorticity_budgets() == []
    finally:
        a.close()


# 4. y-slabs -----------------------------------------------------------------------------------------------------------
def slab_check(m, so, nsko, f=None):
    whole = m.vorticity_budget(nsko)
    wd = m.ocean_dump(nsko) if f is not None else None
    for x in so.slabs:
        mp0, mp1, mt0, mt1 = x.subsample_rows(nsko)
        same(x.vorticity_budget(nsko), {t: v[:, mp0:mp1] for t, v in whole.items()})
        if wd is not None:
            d = x.ocean_dump(nsko)
            for n, v in d.items():
                r0, r1 = (mt0, mt1) if n in ("sst", "wekto") else (mp0, mp1)
                assert np.array_equal(v, wd[n][..., r0:r1, :]), n
    # SlabOcean: the basin from one all-gather of the owned subsample rows
    same(so.vorticity_budget(nsko), whole)
    if wd is not None:
        got = so.ocean_dump(nsko)
        assert sorted(got) == sorted(wd)
        for n in wd:
            assert np.array_equal(got[n], wd[n]), n
    x = so.slabs[0]
    assert x.L.qgcm_hip_qocdiag_schedule(x.h, 1, 5, 1) == 1  # the schedule is whole-domain only
    assert "y-slab" in x.L.qgcm_hip_last_error().decode()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs_tiny(case, nranks):
    g, cfg, f, m = golden_model(case)
    so = make_slabs(cfg, partition(cfg.nypo, nranks))
    try:
        load(so, f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"])
        for x in so.slabs:
            x.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])  # (global arrays; cut per slab)
        for nsko in NSKO:
            slab_check(m, so, nsko, f)
    finally:
        close(so)
        m.close()


@pytest.mark.parametrize("nranks", [2, 8])
def test_slabs_natl5(nranks):
    m, om, f = setup("natl5", False)
    try:
        m.steps(26, s0=1)
        po, pom, qo, qom = m.get_state()
        so = make_slabs(m.cfg, partition(m.cfg.nypo, nranks))
        try:
            load(so, po, pom, qo, qom, f["wekpo"], f["entoc"])
            for nsko in (1, 2):
                slab_check(m, so, nsko)
        finally:
            close(so)
    finally:
        m.close()


# 5. one process per slab ---------------------------------------------------------------------------------------------
def test_three_processes_over_gloo():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr",
           "127.0.0.1", "--master-port", "29747", os.path.join(HERE, "mp_qocdiag_worker.py"), "box_small"]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "MP_QOCDIAG_RESULT OK" in r.stdout, r.stdout[-3000:]
