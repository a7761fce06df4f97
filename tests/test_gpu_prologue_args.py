"""The leading scalar kernel arguments of k_dst64, k_dst64_unpack, k_thomas and k_tend (qgcm_dev.h: QG_ROW_ARGS,
QG_TH_ARGS, QG_TEND_ARGS) duplicate fields of the structs behind them, so that the compiler preloads them into SGPRs.  What can go wrong is a
scalar that disagrees with its struct on a path the big basin never takes: an odd last row, a wave that leaves early,
layer0 != 0, other layer counts, y-slabs.  The smallest grid that reaches them: 193 x 67 (nxto = 192 = 64*3, 65 interior
rows).  The CPU test reads the build's prologue report for the instantiations of the 5 km step."""
import os
import re

import numpy as np
import pytest

from common import FIELDS, relerr

LAYERS = {2: dict(hoc=(500.0, 3500.0), gpoc=(0.02,), ah2oc=(0.0, 0.0), ah4oc=(1.2e10,) * 2),
          3: dict(hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3),
          4: dict(hoc=(300.0, 500.0, 1200.0, 2000.0), gpoc=(0.02, 0.01, 0.005), ah2oc=(0.0,) * 4, ah4oc=(1.2e10,) * 4)}


def tiny_box(nlo):
    from qgcm_hip.config import OceanConfig
    cfg = OceanConfig("pro_nl%d" % nlo, 40, 16, 32, 11, 6, nlo, dxo=2.5e4, dta=240.0, fnot=9.37456e-05, beta=1.7536e-11,
                      cyclic=False, **LAYERS[nlo])
    # M = 3; 65 interior rows: the last row pair has no second row (has_b false), and the 33 pairs leave the second
    # wave of k_dst64's last two-wave workgroup without a pair (the early exit ja > jr1)
    nr = cfg.nypo - 2
    assert cfg.nxto == 192 and nr % 2 == 1 and ((nr + 1) // 2) % 2 == 1
    return cfg


def inputs(cfg):
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=11)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxpo) / 5.0)[:, None] * np.ones(cfg.nypo)[None, :])
    xon = np.zeros(cfg.nlo - 1)
    xon[0] = 3e2
    return po, pom, wek, ent, xon


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [None, "QGCM_HIP_NO_FUSED_CONSTR", "QGCM_HIP_NO_FUSED_UNPACK"])
@pytest.mark.parametrize("nlo", [2, 3, 4])
def test_graph_and_eager_launch_sites_agree_bitwise(nlo, switch, monkeypatch):
    """Three steps through steps() (a captured two-step block and one more step) against the same three steps as
    qgostep / ocinvq / ocqbdy calls, bit for bit: the two paths fill the scalars at different launch sites.  With the
    fused kernels switched off the row transforms run as launches of their own, layer by layer (layer0 != 0)."""
    from qgcm_hip import OceanModel
    if switch:
        monkeypatch.setenv(switch, "1")  # read when a handle is created
    cfg = tiny_box(nlo)
    po, pom, wek, ent, xon = inputs(cfg)
    m = OceanModel(cfg)
    try:
        m.set_p(po, pom)
        m.set_forcing(wek, ent, xon)
        m.steps(3, s0=1)
        a, sa = m.get_state(), m.get_scalars()
        m.set_p(po, pom)
        m.set_forcing(wek, ent, xon)
        for s in range(1, 4):
            m.qgostep()
            m.ocinvq()
            m.ocqbdy()
            if (s - 1) % 25 == 0:
                m.lf_average()
        b, sb = m.get_state(), m.get_scalars()
    finally:
        m.close()
    for f, x, y in zip(FIELDS, a, b):
        assert np.isfinite(x).all(), f
        assert np.array_equal(x, y), (f, nlo, switch, float(np.abs(x - y).max()))
    assert np.array_equal(sa, sb)
    assert not np.array_equal(a[0], po)  # (the steps did something)


@pytest.mark.gpu
def test_two_y_slabs_of_the_tiny_box():
    """The same box as two y-slabs (jr0, joff and the row windows of the tendency are no longer trivial) against the
    one-piece run.  The slab solve composes the Thomas sweeps differently, so this is not a bitwise comparison: the
    bound is the one of the existing slab tests (test_gpu_parity.py: 1e-10 of the field's maximum)."""
    import torch
    from qgcm_hip import OceanModel
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = tiny_box(3)
    po, pom, wek, ent, xon = inputs(cfg)
    m = OceanModel(cfg)
    slabs = []
    try:
        m.set_p(po, pom)
        m.set_forcing(wek, ent, xon)
        st0, scal0 = m.get_state(), m.get_scalars()
        m.steps(3, s0=1)
        whole = m.get_state()
        consts = global_consts(cfg)
        parts = partition(cfg.nypo, 2)
        slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
        so.homsol()
        so.scatter_state(st0[0], st0[1], st0[2], st0[3], wek, ent, xon, scal0)
        so.steps(3, s0=1)
        got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
        for g0, g1, fields in so.gather_local():
            for dst, src in zip(got, fields):
                dst[:, g0 - 1:g1, :] = src
        for f, x, y in zip(FIELDS, got, whole):
            e = relerr(x, y)
            print("two slabs vs one piece, %s: %.3e" % (f, e))
            assert e < 1e-10, (f, e)
        assert np.array_equal(slabs[0].get_scalars(), slabs[1].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        m.close()


# symbol prefix -> (SGPRs preloaded, waits for scalar loads before the first vector load)
HOT = {"_Z7k_dst64ILi15ELb0EEv": (12, 0),
       "_Z8k_thomasILi16ELi0ELb0ELi8EEv": (14, 0),
       "_Z14k_dst64_unpackILi15ELi3ELb1ELb0ELb1ELb0EEv": (12, 0)}


def test_hot_kernels_preload_their_first_arguments(repo_root):
    """The build's prologue report (q-gcm_amd/csrc/prologue_report.py, written by the Makefile): the three solver
    kernels of the 5 km step get their leading arguments in SGPRs, issue their first vector load without waiting for a
    scalar load, use no scratch, and k_dst64_unpack keeps two waves per SIMD.  k_tend gets its tile mapping in SGPRs; the
    first vector load in its program text belongs to the side job of workgroup 0 (the mixed layer's last reduction),
    which reads its own struct: one wait, where the parent had two.  It must stay at or below 78 VGPRs."""
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_prologue.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_prologue.txt missing - rebuild with `make -C q-gcm_amd/csrc`")
    rep = {}
    for line in open(path):
        name, rest = line.split(None, 1)
        rep[name] = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", rest)}
    for prefix, (pre, waits) in HOT.items():
        hits = [k for k in rep if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, hits)
        r = rep[hits[0]]
        assert r["preload"] == pre, (hits[0], r)
        assert r["scalar_waits"] == waits and r["scalar_loads"] <= 12, (hits[0], r)
        assert r["scratch"] == 0, (hits[0], r)
    r = rep[[k for k in rep if k.startswith("_Z14k_dst64_unpackILi15ELi3ELb1ELb0ELb1ELb0EEv")][0]]
    assert r["occupancy"] == 2, r
    tend = [k for k in rep if k.startswith("_Z6k_tendILi3ELb0ELb1ELb0EEv")]
    assert len(tend) == 1
    r = rep[tend[0]]
    assert r["scratch"] == 0 and r["vgpr"] <= 78, r
    assert r["preload"] == 14 and r["scalar_waits"] == 1, r
