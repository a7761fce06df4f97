"""The row-band kernel of the 5 km box ocean (k_tend_rows.h): tendency, leapfrog and projection by bands of interior rows
whose epilogue runs the forward row transform - in place of k_tend + k_dst64 on the plain steps of qgcm_hip_steps.  The
modal right-hand side reaches the transform as the very doubles k_tend would have stored and the transform is
dst64_front / dst64_back unchanged, so the fused path is compared BITWISE against the two launches
(QGCM_HIP_NO_BAND_ROWS=1).  What can go wrong: bands against a wall row, a partial last band, an odd last row pair, the
strips' halo lanes at the W / E wall columns.  The grids are the flattest that reach them, all 961 wide (the kernel
exists for nxto = 960): 961 x 9 (seven interior rows: every band within reach of a wall row), 961 x 17 (fifteen rows:
odd), 961 x 33 (bands with no wall in reach, a partial last band)."""
import os
import re

import numpy as np
import pytest

from common import FIELDS

LAY = dict(hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3)
GRIDS = {"961x9": (8, 120, 1), "961x17": (16, 60, 1), "961x33": (16, 60, 2)}  # ndxr, nxaooc, nyaooc
SWITCH = "QGCM_HIP_NO_BAND_ROWS"


def wide_box(grid):
    from qgcm_hip.config import OceanConfig
    ndxr, nxa, nya = GRIDS[grid]
    cfg = OceanConfig("band_" + grid, nxa + 8, nya + 5, nxa, nya, ndxr, 3, dxo=5.0e3, dta=240.0, fnot=9.37456e-05,
                      beta=1.7536e-11, cyclic=False, **LAY)
    assert cfg.nxto == 960 and cfg.nypo == int(grid.split("x")[1])
    return cfg


def inputs(cfg, zero_ent):
    """zero_ent: entoc all zero AND a flat bottom (zero mask 3); else both fields non-zero everywhere (mask 0)."""
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=11)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxpo) / 5.0)[:, None] * np.ones(cfg.nypo)[None, :])
    if zero_ent:
        ent = np.zeros_like(ent)
    ph = 2.0 * np.pi * np.arange(cfg.nxpo) / cfg.nxto
    y = np.arange(cfg.nypo) / cfg.nyto
    ddy = None if zero_ent else np.asfortranarray(2e-7 * (1.5 + np.sin(2.0 * ph))[:, None] * (2.0 - y)[None, :])
    xon = np.zeros(cfg.nlo - 1)
    xon[0] = 3e2
    return po, pom, wek, ent, ddy, xon


def stepped(cfg, zero_ent, nsteps, eager=False):
    from qgcm_hip import OceanModel
    po, pom, wek, ent, ddy, xon = inputs(cfg, zero_ent)
    m = OceanModel(cfg, ddynoc=ddy)
    try:
        m.set_p(po, pom)
        m.set_forcing(wek, ent, xon)
        if eager:
            for s in range(1, nsteps + 1):
                m.qgostep()
                m.ocinvq()
                m.ocqbdy()
                if (s - 1) % 25 == 0:
                    m.lf_average()
        else:
            m.steps(nsteps, s0=1)
        return m.get_state(), m.get_scalars(), m.tend_zero_mask(), po
    finally:
        m.close()


def assert_same(a, b, what):
    (fa, sa, _, po), (fb, sb, _, _) = a, b
    for f, x, y in zip(FIELDS, fa, fb):
        assert np.isfinite(x).all(), (f, what)
        assert np.array_equal(x, y), (f, what, float(np.abs(x - y).max()))
    assert np.array_equal(sa, sb), what
    assert not np.array_equal(fa[0], po)  # (the steps did something)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_rows_are_bitwise_the_two_launches(grid, zero_ent, monkeypatch):
    """27 steps through steps(): a graph block, the averaging steps 1 and 26 (they keep the two launches), the tail -
    fused against QGCM_HIP_NO_BAND_ROWS=1, once with entoc all zero over a flat bottom (ZM = 3) and once with entoc and
    ddynoc both non-zero everywhere (ZM = 0: the loads of both fields and the topography term see real values)."""
    cfg = wide_box(grid)
    a = stepped(cfg, zero_ent, 27)
    assert a[2] == (3 if zero_ent else 0)
    monkeypatch.setenv(SWITCH, "1")
    b = stepped(cfg, zero_ent, 27)
    assert_same(a, b, (grid, zero_ent))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_graph_replay_is_the_eager_calls(grid):
    """Three steps through steps() (fused rows on steps 2 and 3) against the same steps as qgostep / ocinvq / ocqbdy
    calls (always k_tend + k_dst64), bit for bit."""
    cfg = wide_box(grid)
    assert_same(stepped(cfg, True, 3), stepped(cfg, True, 3, eager=True), grid)


def launches(cfg, zero_ent=True, flat=True, sponge=False, oml=False, cu_range=False):
    from qgcm_hip import OceanModel, oml_preset, synth
    po, pom, wek, ent, ddy, xon = inputs(cfg, zero_ent)
    m = OceanModel(cfg, ddynoc=None if flat else ddy)
    try:
        m.set_p(po, pom)
        m.set_forcing(wek, ent, xon)
        if cu_range:  # (as share_gpu gives the ocean of a coupled run: the kernel wants every CU, one workgroup each)
            assert m.L.qgcm_hip_set_cu_range(m.h, 64, 128) == 0
        if sponge:
            m.set_sponge(np.asfortranarray(np.full((cfg.nxpo, cfg.nypo), 0.5)), 1e-7)
        if oml:
            om = oml_preset(cfg, sb_hflux=True, nb_hflux=True)
            sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
            wekto, _ = synth.wekpo_from_tau(cfg, tx, ty)
            m.oml_init(om)
            m.oml_set_state(sst, sstm)
            m.oml_set_forcing(fnet, wekto, tx, ty)
        prof = m.profile_steps(30, s0=1)
    finally:
        m.close()
    return {k: n for k, (_, n) in prof.items() if n}


@pytest.mark.gpu
def test_launch_plan_fused():
    """The forward rows launch on the two averaging steps only; the fused launch counts as k_tend."""
    got = launches(wide_box("961x17"))
    assert got["k_tend"] == 30 and got["k_dst_fwd"] == 2, got


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["switch", "sponge", "oml", "mask2", "cu_range"])
def test_launch_plan_falls_back(why, monkeypatch):
    if why == "switch":
        monkeypatch.setenv(SWITCH, "1")
    # (mask2: non-zero entoc over a flat bottom - an instantiation the kernel does not have)
    got = launches(wide_box("961x17"), zero_ent=(why != "mask2"), sponge=(why == "sponge"), oml=(why == "oml"),
                   cu_range=(why == "cu_range"))
    assert got["k_tend"] == 30 and got["k_dst_fwd"] == 30, (why, got)


@pytest.mark.gpu
def test_launch_plan_of_box_med_is_unchanged():
    from test_gpu_launch_plan import EXPECTED, launches as plan_launches
    assert plan_launches("box_med") == EXPECTED["box_med"]


def _report(repo_root, name):
    path = os.path.join(repo_root, "q-gcm_amd", "lib", name)
    if not os.path.exists(path):
        pytest.fail("%s missing - rebuild with `make -C q-gcm_amd/csrc`" % name)
    return open(path).read()


def test_band_kernel_resources(repo_root):
    """From the build's resource report: both instantiations (ZM = 0, 3) use no scratch and keep at least two waves per
    SIMD (the transform waves' registers: three)."""
    txt = _report(repo_root, "kernel_resources.txt")
    blocks = re.split(r"Function Name: ", txt)[1:]
    mine = [b for b in blocks if b.startswith("_Z11k_tend_rowsILi3E")]
    assert len(mine) == 2, [b.split()[0] for b in mine]
    for b in mine:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 2, b.split()[0]
    assert "k_tend_rows" in _report(repo_root, "kernel_prologue.txt")
