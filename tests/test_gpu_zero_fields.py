"""The zero-field variants of the tendency kernel (k_tend.h: k_tend_z<NL, CYC, WTQ, AVG, ZM>) against the kernel that
reads entoc and ddynoc, bit for bit.  A handle knows on the host which of the two fields hold +0.0 everywhere
(qgcm_hip_tend_zero_mask: bit 0 entoc, bit 1 ddynoc) and launches the instantiation that leaves them out;
QGCM_HIP_READ_ZERO_FIELDS=1, read when a handle is created, keeps the reading kernel.  What can go wrong: a variant whose
arithmetic on the literal 0.0 rounds or signs differently, a launch site that does not go through the one choice, a
captured graph replayed after the fields changed, a -0.0 taken for a zero, a device-side writer of entoc the host does not
know of.  The CPU test reads the build's reports for the new kernels."""
import dataclasses
import os
import re

import numpy as np
import pytest

from common import FIELDS, preset
from test_gpu_prologue_args import LAYERS, tiny_box

SWITCH = "QGCM_HIP_READ_ZERO_FIELDS"
NSTEPS = 27  # step 26 stores the averaged time level itself (the AVG instantiations)


def grid(name):
    """pro<n>: the 193 x 67 box of test_gpu_prologue_args.py with n layers; cyc<n>: cyc_tiny with n layers; else a preset."""
    if name.startswith("pro"):
        return tiny_box(int(name[3:]))
    if name.startswith("cyc") and name[3:].isdigit():
        n = int(name[3:])
        lay = dict(LAYERS[n], ah4oc=(3.2e12,) * n)
        return dataclasses.replace(preset("cyc_tiny"), name=name, nlo=n, **lay)
    return preset(name)


def fields(cfg):
    """State and forcing; entoc and ddynoc both non-zero everywhere (periodic in x where the grid is)."""
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=11)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ph = 2.0 * np.pi * np.arange(cfg.nxpo) / cfg.nxto
    y = np.arange(cfg.nypo) / cfg.nyto
    ent = np.asfortranarray(1e-7 * (1.5 + np.cos(3.0 * ph))[:, None] * (1.0 + y)[None, :])
    ddy = np.asfortranarray(2e-7 * (1.5 + np.sin(2.0 * ph))[:, None] * (2.0 - y)[None, :])
    xon = np.zeros(cfg.nlo - 1)
    xon[0] = 3e2
    return po, pom, wek, ent, ddy, xon


def zeroed(mask, ent, ddy):
    """The two fields with those of `mask` (bit 0 entoc, bit 1 ddynoc) replaced by +0.0."""
    return (np.zeros_like(ent) if mask & 1 else ent), (np.zeros_like(ddy) if mask & 2 else ddy)


def one_point(a, value):
    """Zeros but for one interior point of the last tile (a load left out there cannot hide)."""
    z = np.zeros_like(a)
    z[-2, -2] = value
    return z


def snapshot(m):
    return [x.copy() for x in m.get_state()] + [m.get_scalars().copy()]


def assert_same(a, b, what):
    for f, x, y in zip(FIELDS + ("scalars",), a, b):
        assert np.isfinite(x).all(), (what, f)
        assert np.array_equal(x, y), (what, f, float(np.abs(x - y).max()))
        # (array_equal takes -0.0 for +0.0: the sign bits too)
        assert np.array_equal(np.signbit(x), np.signbit(y)), (what, f, "signs")


def make(cfg, ddy, forced, monkeypatch, cls=None):
    """A fresh handle; forced: created under QGCM_HIP_READ_ZERO_FIELDS=1."""
    from qgcm_hip import OceanModel
    if forced:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    try:
        return (cls or OceanModel)(cfg, ddy)
    finally:
        monkeypatch.delenv(SWITCH, raising=False)


def eager_steps(m, n):
    for s in range(1, n + 1):
        m.qgostep()
        m.ocinvq()
        m.ocqbdy()
        if (s - 1) % 25 == 0:
            m.lf_average()


def run_both_paths(cfg, mask, monkeypatch, what):
    """27 steps through steps() and through the three eager calls, in a handle that picks the variant and in one that
    reads both fields; returns nothing, asserts bitwise equality and the masks."""
    po, pom, wek, ent, ddy, xon = fields(cfg)
    ent, ddy = zeroed(mask, ent, ddy)
    models = [make(cfg, ddy, forced, monkeypatch) for forced in (False, True)]
    try:
        got = {}
        for path in ("graph", "eager"):
            for m, forced in zip(models, (False, True)):
                m.set_p(po, pom)
                m.set_forcing(wek, ent, xon)
                assert m.tend_zero_mask() == (0 if forced else mask), (what, forced, m.tend_zero_mask())
                if path == "graph":
                    m.steps(NSTEPS, s0=1)
                else:
                    eager_steps(m, NSTEPS)
                got[path, forced] = snapshot(m)
            assert_same(got[path, False], got[path, True], "%s %s mask %d" % (what, path, mask))
        assert not np.array_equal(got["graph", False][0], po)  # (the steps did something)
    finally:
        for m in models:
            m.close()


FULL = ["pro2", "pro3", "pro4", "cyc2", "cyc3", "cyc4"]


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [3, 2, 1])
@pytest.mark.parametrize("name", FULL)
def test_variant_is_bitwise_the_reading_kernel(name, mask, monkeypatch):
    """Both fields zero, only ddynoc zero, only entoc zero; NL = 2, 3, 4; box and cyclic."""
    run_both_paths(grid(name), mask, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box_tiny", "box_med", "cyc_med"])
def test_variant_is_bitwise_on_the_preset_grids(name, monkeypatch):
    run_both_paths(grid(name), 3, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mask", [("pro3", 3), ("cyc3", 2), ("pro4", 1)])
def test_variant_is_bitwise_in_the_wide_tile(name, mask, monkeypatch):
    """QGCM_HIP_TEND_WIDE=1: the instantiations of the HBM-bound sizes (32-wide tiles, plain stores)."""
    monkeypatch.setenv("QGCM_HIP_TEND_WIDE", "1")
    run_both_paths(grid(name), mask, monkeypatch, name + " wide")


@pytest.mark.gpu
def test_variant_is_bitwise_on_two_y_slabs(monkeypatch):
    """The 193 x 67 box as two y-slabs: every slab scans its own rows - the lower one finds both fields zero, the upper
    one holds the only non-zero entoc point."""
    import torch
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = tiny_box(3)
    po, pom, wek, ent, ddy, xon = fields(cfg)
    ent = one_point(ent, 1e-7)
    m = make(cfg, None, True, monkeypatch)
    try:
        m.set_p(po, pom)
        st0, scal0 = m.get_state(), m.get_scalars()
    finally:
        m.close()
    consts = global_consts(cfg)
    parts = partition(cfg.nypo, 2)
    got = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv(SWITCH, "1")
        slabs = []
        try:
            slabs = [HipSlab(cfg, consts, g0, g1, r, 2, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
            so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
            so.homsol()
            so.scatter_state(st0[0], st0[1], st0[2], st0[3], wek, ent, xon, scal0)
            masks = [int(sl.L.qgcm_hip_tend_zero_mask(sl.h)) for sl in slabs]
            assert masks == ([0, 0] if forced else [3, 2]), (forced, masks)
            so.steps(NSTEPS, s0=1)
            out = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
            for g0, g1, fl in so.gather_local():
                for dst, src in zip(out, fl):
                    dst[:, g0 - 1:g1, :] = src
            got[forced] = out + [slabs[0].get_scalars().copy()]
        finally:
            for sl in slabs:
                sl.close()
            monkeypatch.delenv(SWITCH, raising=False)
    assert_same(got[False], got[True], "two slabs")
    assert not np.array_equal(got[False][0], st0[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [3, 1])
def test_variant_is_bitwise_on_the_atmosphere(mask, monkeypatch):
    """The atmosphere handle of cpl_tiny (entat and the topography act on layer 1 with the other sign): 27 steps through
    steps() and three through qgastep / atinvq / atqzbd."""
    from qgcm_hip import AtmosModel, config, synth
    from common import atm_apply
    acfg = config.atmos_preset("cpl_tiny")
    f = dict(synth.atmos_fields(acfg))
    f["entat"], f["ddynat"] = zeroed(mask, np.asfortranarray(f["entat"]), np.asfortranarray(f["ddynat"]))
    assert np.abs(f["entat"]).max() > 0 or mask & 1
    models = [make(acfg, f["ddynat"], forced, monkeypatch, cls=AtmosModel) for forced in (False, True)]
    try:
        got = {}
        for path in ("graph", "eager"):
            for m, forced in zip(models, (False, True)):
                atm_apply(m, f)
                assert m.tend_zero_mask() == (0 if forced else mask)
                if path == "graph":
                    m.steps(NSTEPS, s0=1)
                else:
                    for s in range(1, 4):
                        m.qgastep()
                        m.atinvq()
                        m.atqzbd()
                        if (s - 1) % 100 == 0:
                            m.lf_average()
                got[path, forced] = snapshot(m)
            assert_same(got[path, False], got[path, True], "atmosphere %s mask %d" % (path, mask))
    finally:
        for m in models:
            m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["entoc", "ddynoc"])
def test_no_stale_choice(which, monkeypatch):
    """One handle through three legs of 50 steps (one captured block each): the field zero, then non-zero in one point of
    the last tile, then zero again.  After every leg the state is that of a handle with the same history that reads
    both fields, and the mask follows the field."""
    from qgcm_hip.model import _dp
    cfg = tiny_box(3)
    po, pom, wek, ent, ddy, xon = fields(cfg)
    zero = np.zeros_like(ent)
    spike = one_point(ent, 1e-7)
    models = [make(cfg, None, forced, monkeypatch) for forced in (False, True)]
    try:
        for m in models:
            m.set_p(po, pom)
            m.set_forcing(wek, zero, xon)
        for leg, (fld, want) in enumerate([(zero, 3), (spike, 2 if which == "entoc" else 1), (zero, 3)]):
            snaps = []
            for m, forced in zip(models, (False, True)):
                if which == "entoc":
                    m.set_forcing(None, fld, None)
                else:
                    assert m.L.qgcm_hip_set_geometry(m.h, _dp(m.yporel), _dp(fld)) == 0
                assert m.tend_zero_mask() == (0 if forced else want), (leg, forced, m.tend_zero_mask())
                m.steps(50, s0=1 + 50 * leg)
                snaps.append(snapshot(m))
            assert_same(snaps[0], snaps[1], "%s leg %d" % (which, leg))
            if leg == 0:
                first = snaps[0]
        # the non-zero leg changed the result (the spike was read) ...
        fresh = make(cfg, None, True, monkeypatch)
        try:
            fresh.set_p(po, pom)
            fresh.set_forcing(wek, zero, xon)
            fresh.steps(150, s0=1)
            assert not np.array_equal(fresh.get_state()[2], snaps[0][2])
        finally:
            fresh.close()
        assert not np.array_equal(first[0], po)
        # ... and a NULL entoc leaves what is known about the buffer as it was
        models[0].set_forcing(wek, None, xon)
        assert models[0].tend_zero_mask() == 3
    finally:
        for m in models:
            m.close()


@pytest.mark.gpu
def test_minus_zero_is_not_zero(monkeypatch):
    """Fields of -0.0 are read: qdot(2) = dq + fohfac * (-0.0) and ql - (-0.0) are not the +0.0 expressions' bits in
    every case, so the handle must not pick a variant for them."""
    cfg = tiny_box(3)
    po, pom, wek, ent, ddy, xon = fields(cfg)
    mz = np.asfortranarray(np.full_like(ent, -0.0))
    assert np.signbit(mz).all()
    for e, d, want in ((mz, mz, 0), (mz, None, 2), (np.zeros_like(ent), mz, 1)):
        models = [make(cfg, d, forced, monkeypatch) for forced in (False, True)]
        try:
            snaps = []
            for m, forced in zip(models, (False, True)):
                m.set_p(po, pom)
                m.set_forcing(wek, e, xon)
                assert m.tend_zero_mask() == (0 if forced else want), (want, forced, m.tend_zero_mask())
                m.steps(NSTEPS, s0=1)
                snaps.append(snapshot(m))
            assert_same(snaps[0], snaps[1], "-0.0, mask %d" % want)
        finally:
            for m in models:
                m.close()


@pytest.mark.gpu
def test_mixed_layer_keeps_entoc_read(monkeypatch):
    """Mixed layer on: k_oml_entoc writes entoc every step, so bit 0 is never set - not after a set_forcing of zeros
    either; ddynoc's bit may be.  State and sst are bitwise those of the handle that reads both."""
    from qgcm_hip import synth
    from qgcm_hip.config import oml_preset
    cfg = preset("box_med")
    om = oml_preset(cfg)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    models = [make(cfg, None, forced, monkeypatch) for forced in (False, True)]
    try:
        snaps = []
        for m, forced in zip(models, (False, True)):
            assert m.tend_zero_mask() == (0 if forced else 3)  # (a fresh handle: both buffers zero-filled)
            m.oml_init(om)
            assert m.tend_zero_mask() == (0 if forced else 2)
            m.set_p(po, po)
            m.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(cfg.nlo - 1))
            assert m.tend_zero_mask() == (0 if forced else 2)
            m.oml_set_state(sst, sstm)
            m.oml_set_forcing(fnet, wekto, tx, ty)
            m.steps(NSTEPS, s0=1)
            assert m.tend_zero_mask() == (0 if forced else 2)
            ent, _ = m.oml_get_diag()
            assert np.abs(ent).max() > 0.0
            snaps.append(snapshot(m) + [x.copy() for x in m.oml_get_state()] + [ent])
        for i, (x, y) in enumerate(zip(snaps[0], snaps[1])):
            assert np.array_equal(x, y), i
    finally:
        for m in models:
            m.close()


def _reports(repo_root):
    lib = os.path.join(repo_root, "q-gcm_amd", "lib")
    pro, res = os.path.join(lib, "kernel_prologue.txt"), os.path.join(lib, "kernel_resources.txt")
    if not (os.path.exists(pro) and os.path.exists(res)):
        pytest.fail("kernel_prologue.txt / kernel_resources.txt missing - rebuild with `make -C q-gcm_amd/csrc`")
    rep = {}
    for line in open(pro):
        name, rest = line.split(None, 1)
        rep[name] = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", rest)}
    return rep, open(res).read()


# NL, CYC, WTQ, AVG of every k_tend instantiation that has variants (NL = 2, 3, 4; AVG where it exists)
TWINS = [(nl, cyc, wtq, False) for nl in (2, 3, 4) for cyc in (False, True) for wtq in (False, True)] + \
        [(2, False, True, True), (3, False, True, True), (4, False, True, True), (3, True, True, True), (3, True, False, True)]


def test_variants_in_the_build_reports(repo_root):
    """The build's reports list k_tend_z<NL, CYC, WTQ, AVG, ZM> for ZM = 1, 2, 3 next to every k_tend twin, with no
    scratch, no more VGPRs than the twin, the twin's occupancy, and the same 14 preloaded SGPRs and one scalar wait
    before the first vector load; layer counts above 4 have no variants.

    (k_tend_z<2, true, false, false, 3> took 84 against 82 until the wide-tile variants got a compiler barrier in their
    Jacobian: DESIGN 3.1.)"""
    rep, res = _reports(repo_root)
    b = lambda x: "Lb%dE" % int(x)
    more = []  # variants with more VGPRs than their twins: all of them are looked at before the assertion
    for nl, cyc, wtq, avg in TWINS:
        targs = "Li%dE%s%s%s" % (nl, b(cyc), b(wtq), b(avg))
        twin = [k for k in rep if k.startswith("_Z6k_tendI%sEv" % targs)]
        assert len(twin) == 1, (targs, twin)
        t = rep[twin[0]]
        for zm in (1, 2, 3):
            hits = [k for k in rep if k.startswith("_Z8k_tend_zI%sLi%dEEv" % (targs, zm))]
            assert len(hits) == 1, (targs, zm, hits)
            r = rep[hits[0]]
            print(hits[0][:40], r, "twin", t)
            assert r["scratch"] == 0, (hits[0], r)
            if r["vgpr"] > t["vgpr"]:
                more.append((hits[0].split("EvPKd")[0], r["vgpr"], t["vgpr"]))
            assert r["occupancy"] >= t["occupancy"], (hits[0], r, t)
            assert r["preload"] == t["preload"] == 14 and r["scalar_waits"] <= t["scalar_waits"], (hits[0], r, t)
            assert hits[0] in res, hits[0]  # (the compiler's own resource report names it too)
    assert len([k for k in rep if k.startswith("_Z8k_tend_zI")]) == 3 * len(TWINS)
    assert not more, more
