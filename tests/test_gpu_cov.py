"""MI355X parity of the covariance matrices through the C ABI: qgcm_hip_cov_init / _add / _out / _reset /
_schedule and the slab part / combine, against the reference's own values (tests/golden/cov_*.npz, acov_*.npz) and, at
full size, against the numpy restatement tests/numpy_cov.py of the pulled state, which reproduces those values
(tests/test_cov_cpu.py).  Every comparison is bitwise."""
import glob
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import numpy_cov as nc
from qgcm_hip import AtmosModel, OceanModel, QgcmHipError, atmos_preset, coupled_steps, oml_preset, preset, share_gpu
from qgcm_hip.model import cov_row_split
from qgcm_hip.slab import partition
from test_gpu_slab_diagnostics import close, slabs_like
from test_gpu_tavg import ocean
from qgcm_hip import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
OCN = ("covpo", "avgpo", "swtpo", "nupo", "covto", "avgto", "swtto", "nuto")
ATM = ("covpa", "avgpa", "swtpa", "nupa", "covta", "avgta", "swtta", "nuta")


def same(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    bad = [k for k in a if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    assert not bad, bad


def restated(acc_p, acc_t, names):
    return dict(zip(names, (acc_p.cov, acc_p.mean, acc_p.swt, acc_p.nu, acc_t.cov, acc_t.mean, acc_t.swt, acc_t.nu)))


def pulled(m, mixed_layer, sst):
    """Layer 1 of p and the T field the device reads, from the host copies."""
    p = m.get_state()[0][:, :, 0]
    return p, (m.oml_get_state()[0] if mixed_layer else sst)


# 1. the reference's numbers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "cov_*.npz")) + glob.glob(os.path.join(GOLD, "acov_*.npz"))),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_against_the_reference(path):
    g = np.load(path)
    nsi, atm = int(g["c_nsi"]), bool(g["c_atm"])
    fixture = str(g["c_fixture"])
    cfg = atmos_preset({"atm_tiny": "cpl_tiny", "atm_small": "cpl_small"}[fixture]) if atm else preset(fixture)
    m = AtmosModel(cfg) if atm else OceanModel(cfg)
    names = ATM if atm else OCN
    try:
        m.enable_covariance(nsi)
        n = 0
        while "in%d_p1" % n in g.files:
            p1, t = g["in%d_p1" % n], g["in%d_t" % n]
            nl = cfg.nla if atm else cfg.nlo
            p = np.asfortranarray(np.repeat(p1[:, :, None], nl, axis=2))
            m.set_state(p, p, p, p)
            if atm:
                m.set_atm_monitor_fields(ast=t)
                m.covatm()
            else:
                m.set_monitor_fields(sst=t)
                m.covocn()
            n += 1
        got = m.covariance()
        want = dict(zip(names, (g["out_cov_p"], g["out_avg_p"], float(g["out_swt_p"]), int(g["out_nu_p"]),
                                g["out_cov_t"], g["out_avg_t"], float(g["out_swt_t"]), int(g["out_nu_t"]))))
        same(got, want)
        # a range read is a slice of the whole
        sz = m.covariance_size()
        k0, cnt = sz["nmat"] // 3, sz["nmat"] // 4
        part = m.covariance(k0, cnt)
        assert np.array_equal(part[names[0]], want[names[0]][k0:k0 + cnt])
        assert np.array_equal(part[names[4]], want[names[4]][k0:k0 + cnt])
        m.reset_covariance()
        z = m.covariance()
        assert z[names[3]] == 0 and not np.any(z[names[0]]) and not np.any(z[names[1]])
    finally:
        m.close()


# 2. full size against the numpy restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,mixed_layer", [("natl5", False), ("natl5", True), ("socn5", False), ("socn5", True)])
def test_full_size_ocean(cfgname, mixed_layer):
    m = ocean(cfgname, mixed_layer)
    cfg = m.cfg
    sst = synth.mixed_layer_fields(cfg, oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer), seed=5)[0]
    try:
        m.enable_covariance(16)
        nvar = (cfg.nxto // 16) * (cfg.nyto // 16)
        assert m.covariance_size()["nvar"] == nvar
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        before = None
        for n in (3, 22, 1, 9):  # the third contribution follows the averaging step 26
            m.steps(n)
            before = [a.copy() for a in m.get_state()]
            m.covocn()
            nc.covocn(*pulled(m, mixed_layer, sst), 16, ap, at)
        for x, y in zip(before, m.get_state()):  # accumulating leaves the state alone
            assert np.array_equal(x, y)
        same(m.covariance(), restated(ap, at, OCN))
    finally:
        m.close()


def test_full_size_atmosphere():
    from test_gpu_atm_tavg import atmos
    m, fl, _ = atmos("cpl_natl5")
    try:
        m.enable_covariance(2)
        nvar = (m.cfg.nxpa - 1) // 2 * ((m.cfg.nypa - 1) // 2)
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        for n in (5, 95, 1, 30):  # the third follows the atmosphere's averaging step 101
            m.steps(n)
            m.covatm()
            nc.covocn(m.get_state()[0][:, :, 0], fl["ast"], 2, ap, at)
        same(m.covariance(), restated(ap, at, ATM))
    finally:
        m.close()


def test_non_temporal_variant_is_bitwise_the_same(monkeypatch):
    ms = []
    try:
        for nt in ("0", "1"):
            monkeypatch.setenv("QGCM_HIP_COV_NT", nt)
            m = ocean("natl5", False)
            ms.append(m)
            m.enable_covariance(16)
            for n in (2, 2, 2):
                m.steps(n)
                m.covocn()
        same(ms[0].covariance(), ms[1].covariance())
    finally:
        for m in ms:
            m.close()


# 3. the schedule ------------------------------------------------------------------------------------------------------
def test_schedule_equals_explicit_calls():
    """steps(120) with schedule_covariance(every=25, phase=1) against covocn() after windows that end at 1, 26, 51, 76,
    101 (averaging steps among them)."""
    a = ocean("natl5", True)
    b = ocean("natl5", True)
    try:
        for m in (a, b):
            m.enable_covariance(16)
        a.schedule_covariance(25, 1)
        a.steps(120, s0=1)
        b.steps(0, s0=1)
        for n in (1, 25, 25, 25, 25):
            b.steps(n)
            b.covocn()
        b.steps(19)
        ca, cb = a.covariance(), b.covariance()
        assert ca["nupo"] == cb["nupo"] == 5
        same(ca, cb)
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(a.oml_get_state()[0], b.oml_get_state()[0])
    finally:
        a.close()
        b.close()


def test_schedule_inside_coupled_steps():
    """The cpl_natl5 pair under share_gpu: coupled_steps(1, 240, 3) with an ocean schedule every 20 ocean steps,
    phase 0 (ntcovoc = 60, nstr = 3, nsteps0 = 0) and an atmosphere schedule every 60 steps, phase 0, beside a tavatm
    schedule on the same steps, against explicit calls after coupled windows that end at 60, 120, 180 and 240."""
    import test_gpu_monitors as om
    from test_gpu_atm_tavg import atmos
    o1, _, _ = om.setup("cpl_natl5", False)
    o2, _, _ = om.setup("cpl_natl5", False)
    a1, _, _ = atmos()
    a2, _, _ = atmos()
    try:
        for h in (o1, o2):
            h.enable_covariance(16)
        for h in (a1, a2):
            h.enable_covariance(2)
        assert share_gpu(o1, a1) > 0
        o1.schedule_covariance(20, 0)
        a1.schedule_covariance(60, 0)
        a1.schedule_time_means(60, 0)
        coupled_steps(o1, a1, 1, 240, 3)
        assert share_gpu(o2, a2) > 0
        for nt0 in (1, 61, 121, 181):
            coupled_steps(o2, a2, nt0, 60, 3)
            a2.tavatm()
            o2.covocn()
            a2.covatm()
        co1, co2 = o1.covariance(), o2.covariance()
        ca1, ca2 = a1.covariance(), a2.covariance()
        assert co1["nupo"] == co2["nupo"] == 4 and ca1["nupa"] == ca2["nupa"] == 4
        same(co1, co2)
        same(ca1, ca2)
        for x, y in zip(a1.get_state() + o1.get_state(), a2.get_state() + o2.get_state()):
            assert np.array_equal(x, y)
    finally:
        for h in (o1, o2, a1, a2):
            h.close()


def test_no_side_effects():
    """No schedule: the launches of profile_steps are those of a handle that never used the feature.  A schedule: the
    only extra launches are one k_cov per scheduled step."""
    m = ocean("natl5", False)
    t = ocean("natl5", False)
    try:
        m.enable_covariance(16)
        m.covocn()
        m.schedule_covariance(7, 3)
        m.schedule_covariance(0)
        pm, pt = m.profile_steps(12, s0=1), t.profile_steps(12, s0=1)
        assert {k: n for k, (_, n) in pm.items() if k != "k_noop_train"} == \
            {k: n for k, (_, n) in pt.items() if k != "k_noop_train"}
        assert pm["k_cov"][1] == 0
        m.schedule_covariance(10, 3)
        on, off = m.profile_steps(30), t.profile_steps(30)  # steps 13..42: scheduled 13, 23, 33
        for k in on:
            if k not in ("k_cov", "k_noop_train"):
                assert on[k][1] == off[k][1], k
        assert on["k_cov"][1] == 3
    finally:
        m.close()
        t.close()


# 4. y-slabs -----------------------------------------------------------------------------------------------------------
def test_slabs_equal_whole_domain():
    m = ocean("natl5", False)
    cfg = m.cfg
    om = oml_preset(cfg)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, entoc=np.zeros_like(wekpo))
    try:
        m.enable_covariance(16)
        m.steps(3, s0=1)
        for _ in range(3):  # three contributions of one state: the first sets the mean, the others update
            m.covocn()
        whole = m.covariance()
        for nranks in (2, 3, 8):
            so = slabs_like(m, om, f, False, partition(cfg.nypo, nranks))
            try:
                so.enable_covariance(16)
                for _ in range(3):
                    so.covocn()
                got = so.covariance()
                same(got, whole)
                # every rank holds its own rows only, and the shares tile the matrix
                nvar = whole["avgpo"].size
                for r, x in enumerate(so.slabs):
                    sz = x.covariance_size()
                    i0, i1 = cov_row_split(nvar, r, nranks), cov_row_split(nvar, r + 1, nranks)
                    assert (sz["k0"], sz["k1"]) == (i0 * (i0 + 1) // 2, i1 * (i1 + 1) // 2)
                parts = so.covariance_parts()
                assert sum(len(d["covpo"]) for d in parts) == len(whole["covpo"])
            finally:
                close(so)
    finally:
        m.close()


def test_three_processes_over_gloo(tmp_path):
    """Three processes, one slab each, exchanging over torch.distributed (gloo): the assembled matrices equal the
    whole-domain handle's."""
    import subprocess
    import sys
    m = ocean("natl5", False)
    try:
        m.enable_covariance(16)
        m.steps(3, s0=1)
        po, pom, qo, qom = m.get_state()
        for _ in range(3):
            m.covocn()
        whole = m.covariance()
    finally:
        m.close()
    cfg = preset("natl5")
    sst = synth.mixed_layer_fields(cfg, oml_preset(cfg), seed=5)[0]
    np.savez(tmp_path / "state.npz", po=po, pom=pom, qo=qo, qom=qom, sst=sst)
    worker = os.path.join(os.path.dirname(__file__), "mp_cov_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + os.getpid() % 1000), WORLD_SIZE="3")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(tmp_path)], env=dict(env, RANK=str(r)))
             for r in range(3)]
    rcs = [p.wait(timeout=600) for p in procs]
    assert rcs == [0, 0, 0], rcs
    for r in range(3):
        got = dict(np.load(tmp_path / ("out%d.npz" % r)))
        same({k: (got[k] if got[k].ndim else got[k].item()) for k in got}, whole)


# 5. the 64-bit path ---------------------------------------------------------------------------------------------------
def test_64bit_packed_index():
    """SOcn 5 km with nsi = 6: nvar = 73 728, 2 717 945 856 entries per matrix (43.5 GB for the two).  Entries read
    around k = 2^31 - 1 and at the end of the triangle equal numpy's from the pulled po / sst."""
    cfg = preset("socn5")
    nvar = (cfg.nxto // 6) * (cfg.nyto // 6)
    nmat = nvar * (nvar + 1) // 2
    need = 2 * nmat * 8
    free, _ = torch.cuda.mem_get_info()
    if free < need + (4 << 30):
        pytest.skip("needs %d bytes of device memory for the two matrices, %d free" % (need, free))
    m = ocean("socn5", False)
    sst = synth.mixed_layer_fields(cfg, oml_preset(cfg), seed=5)[0]
    try:
        m.enable_covariance(6)
        assert m.covariance_size() == dict(nvar=nvar, nmat=nmat, k0=0, k1=nmat)
        ranges = [(2 ** 31 - 1 - 5000, 10000), (2 ** 32 - 5000, 10000) if nmat > 2 ** 32 else (nmat // 2, 1000),
                  (nmat - 10000, 10000)]
        accs = [(nc.Dssp(nvar, k, k + n), nc.Dssp(nvar, k, k + n)) for k, n in ranges]
        for n in (2, 2, 2):
            m.steps(n)
            m.covocn()
            p1 = m.get_state()[0][:, :, 0]
            u, v = nc.psampl(p1, 6), nc.tsampl(sst, 6)
            for ap, at in accs:
                ap.add(u)
                at.add(v)
        for (k, n), (ap, at) in zip(ranges, accs):
            got = m.covariance(k, n)
            assert np.array_equal(got["covpo"], ap.cov) and np.array_equal(got["covto"], at.cov), k
            assert np.count_nonzero(got["covpo"]) > n // 2
        got = m.covariance(0, 0)
        assert np.array_equal(got["avgpo"], accs[0][0].mean) and got["nupo"] == 3
    finally:
        m.close()


# 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    m = OceanModel(preset("box_tiny"))
    try:
        for nsi in (1, 5, -2):  # 5 divides neither nxto = 48 nor nyto = 36; 1: psampl's count is not tsampl's
            with pytest.raises(QgcmHipError, match="nsi"):
                m.enable_covariance(nsi)
        with pytest.raises(QgcmHipError, match="off"):
            m.covocn()
        m.enable_covariance(4)
        with pytest.raises(QgcmHipError, match="sst"):
            m.covocn()
        m.schedule_covariance(3, 1)
        with pytest.raises(QgcmHipError, match="sst"):
            m.steps(5, s0=1)
        with pytest.raises(QgcmHipError, match="phase"):
            m.schedule_covariance(3, 3)
        with pytest.raises(QgcmHipError, match="outside"):
            m.covariance(0, m.covariance_size()["nmat"] + 1)
        m.enable_covariance(0)
        with pytest.raises(QgcmHipError, match="off"):
            m.covariance()
    finally:
        m.close()
    a = AtmosModel(atmos_preset("cpl_tiny"))
    try:
        a.enable_covariance(2)
        with pytest.raises(QgcmHipError, match="ast"):
            a.covatm()
        with pytest.raises(QgcmHipError, match="covatm"):
            a.covocn()
    finally:
        a.close()


def test_slab_refuses_schedule_and_bad_tiling():
    m = ocean("natl5", False)
    cfg = m.cfg
    om = oml_preset(cfg)
    sst, _, _, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, entoc=np.zeros_like(wekpo))
    so = slabs_like(m, om, f, False, partition(cfg.nypo, 2))
    try:
        so.enable_covariance(16)
        x = so.slabs[0]
        with pytest.raises(QgcmHipError, match="y-slab"):
            check_schedule(x)
        send, gath = so._cov_bufs
        for i, s in enumerate(so.slabs):
            s.cov_part(send[i])
        for s in so.slabs:
            s.sync()
        # the gathered parts in the wrong rank order do not tile the rows
        n = x.cov_part_len()
        gath[0][:n].copy_(send[1])
        gath[0][n:].copy_(send[0])
        with pytest.raises(QgcmHipError, match="tile"):
            x.cov_combine(gath[0])
        assert x.covariance(0, 0)["nupo"] == 0
    finally:
        close(so)
        m.close()


def check_schedule(slab):
    from qgcm_hip.lib import check
    check(slab.L.qgcm_hip_cov_schedule(slab.h, 5, 0))


# 7. resources ---------------------------------------------------------------------------------------------------------
def test_cov_kernels_do_not_spill():
    path = os.path.join(os.path.dirname(__file__), "..", "q-gcm_amd", "lib", "kernel_resources.txt")
    res, cur = {}, None
    for line in open(path):
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if mm and cur:
            res[cur] = int(mm.group(1))
    cov = {k: v for k, v in res.items() if "k_cov_" in k}
    assert any("k_cov_rank1ILb0" in k for k in cov) and any("k_cov_rank1ILb1" in k for k in cov)
    assert any("k_cov_rowsums" in k for k in cov) and any("k_cov_combine" in k for k in cov)
    assert all(v == 0 for v in cov.values()), cov
