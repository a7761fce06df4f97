"""The row-band kernel of the 5 km box ocean (k_tend_rows.h): tendency, leapfrog and projection by bands of interior rows
whose epilogue runs the forward row transform - in place of k_tend + k_dst64 on the plain steps of qgcm_hip_steps.  The
modal right-hand side reaches the transform as the very doubles k_tend would have stored and the transform is
dst64_front / dst64_back unchanged, so the fused path is compared BITWISE against the two launches
(QGCM_HIP_NO_BAND_ROWS=1), and both against the CPU oracle.

What can go wrong depends on the BAND SHAPE of the grid, not only on how far a band is from a wall.  With rows = ny - 2
interior rows, B = TR_BAND = 4 rows per band, nbands = ceil(rows / B) and per_xcd = ceil(nbands / 8) (the kernel's own
formulas; band = (blockIdx & 7) * per_xcd + (blockIdx >> 3), workgroups with band >= nbands leave at once) the grids
are, all 961 wide (the kernel exists for nxto = 960):

  grid     rows  rows mod 4  nbands  per_xcd  what it reaches
  961x6       4      0          1       1     ONE band that is first and last: both wall-row copies and both wall rules in
                                              one workgroup; no partial band, the clamped loads start at the wall row
  961x7       5      1          2       1     a last band of one row (its pair 0 has no second row, pair 1 leaves) that
                                              lies against the N wall row
  961x9       7      3          2       1     every band within reach of a wall row
  961x16     14      2          4       1     a last band of two rows (pair 0 whole, pair 1 absent)
  961x17     15      3          4       1     an odd number of rows
  961x33     31      3          8       1     bands with no wall in reach, one band per XCD
  961x36     34      2          9       2     per_xcd = 2 with seven idle workgroups
  961x66     64      0         16       2     per_xcd = 2, no idle workgroup, no partial band
  961x67     65      1         17       3     per_xcd = 3 with seven idle workgroups, a last band of one row

(NAtl 5 km itself: 959 rows, mod 3, 240 bands, per_xcd 30, none idle.)  Odd refinement ratios (ndxr = 3, 5) give the
remainders 0, 1, 2; with ndxr a multiple of 4 the remainder is always 3.  test_band_shapes_are_covered recomputes the
table from TR_BAND and says which shapes are missing after a retuning.

The inputs vary from row to row AND from column to column in every field the kernel loads (test_inputs_vary_...): a load
of the wrong row or column cannot return the right bits.

test_plan_changes_keep_the_bits moves ONE handle between the fused and the two-launch plan while it holds captured
graphs: set_forcing flips the zero mask (the graphs stay, only graph_key separates them), qgcm_hip_set_cu_range switches
the plan off and on."""
import functools
import os
import re

import numpy as np
import pytest

from common import FIELDS, bits, make_oracle, relerr

LAY = dict(hoc=(350.0, 750.0, 2900.0), gpoc=(0.025, 0.0125), ah2oc=(0.0,) * 3, ah4oc=(1.2e10,) * 3)
GRIDS = {"961x9": (8, 120, 1), "961x17": (16, 60, 1), "961x33": (16, 60, 2),  # ndxr, nxaooc, nyaooc
         "961x6": (5, 192, 1), "961x7": (3, 320, 2), "961x16": (5, 192, 3), "961x36": (5, 192, 7),
         "961x66": (5, 192, 13), "961x67": (3, 320, 22)}
SWITCH = "QGCM_HIP_NO_BAND_ROWS"
TOL_60 = 1e-10    # test_gpu_parity.TOL_60: whole steps against the reference, runs of this length
TOL_SCAL = 1e-11  # test_gpu_parity.test_whole_steps_vs_reference: the constraint scalars (common.scal_err's scale)


def wide_box(grid):
    from qgcm_hip.config import OceanConfig
    ndxr, nxa, nya = GRIDS[grid]
    cfg = OceanConfig("band_" + grid, nxa + 8, nya + 5, nxa, nya, ndxr, 3, dxo=5.0e3, dta=240.0, fnot=9.37456e-05,
                      beta=1.7536e-11, cyclic=False, **LAY)
    assert cfg.nxto == 960 and cfg.nypo == int(grid.split("x")[1])
    return cfg


def band_shape(nypo, B):
    """(rows, rows mod B, nbands, per_xcd) by the formulas of k_tend_rows.h."""
    rows = nypo - 2
    nbands = (rows + B - 1) // B
    return rows, rows % B, nbands, (nbands + 7) // 8


def inputs(cfg, zero_ent):
    """zero_ent: entoc all zero AND a flat bottom (zero mask 3); else both fields non-zero everywhere (mask 0).  Every
    field varies in x and in y (synth's Ekman pumping is a function of y alone: it gets an x-dependent part here)."""
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg, noise=2e-2, seed=11)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    ph = 2.0 * np.pi * np.arange(cfg.nxpo) / cfg.nxto
    y = np.arange(cfg.nypo) / cfg.nyto
    # (synth's pumping also repeats from row to row where ny - 1 is a multiple of 6: the added part vanishes nowhere)
    wek = np.asfortranarray(wek + 0.1 * np.abs(wek).max() * (1.5 + np.sin(3.0 * ph))[:, None] * (1.0 + y)[None, :])
    ent = np.asfortranarray(1e-7 * np.cos(np.arange(cfg.nxpo) / 5.0)[:, None] * (1.0 + y)[None, :])
    if zero_ent:
        ent = np.zeros_like(ent)
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
        # (array_equal takes -0.0 for +0.0: the sign bits too, as test_gpu_zero_fields.assert_same)
        assert np.array_equal(np.signbit(x), np.signbit(y)), (f, what, "signs")
    assert np.isfinite(sa).all(), what
    assert np.array_equal(sa, sb), what
    assert np.array_equal(np.signbit(sa), np.signbit(sb)), (what, "signs of the scalars")
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


# ---- against the CPU oracle -----------------------------------------------------------------------------------------
ORACLE_STEPS = 27


@functools.lru_cache(maxsize=None)
def oracle_run(grid, zero_ent):
    """The oracle's side of test_fused_rows_vs_oracle, computed once per case and never modified: the start state (from
    po, pom as the oracle derives q and the constraint scalars), the state after the single step 2 from it, and state
    and scalars after steps 1 .. 27 from it."""
    import oracle_binding as ob
    cfg = wide_box(grid)
    po, pom, wek, ent, ddy, xon = inputs(cfg, zero_ent)
    out = {}
    for s0, n, tag in ((2, 1, "one"), (1, ORACLE_STEPS, "end")):  # (a fresh oracle for either run)
        o = make_oracle(cfg) if ddy is None else ob.Oracle(
            cfg.nxpo, cfg.nypo, cfg.nlo, cfg.cyclic, cfg.fnot, cfg.beta, cfg.dxo, cfg.dto, cfg.delek, cfg.bccooc,
            cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc, cfg.yporel(), ddy)
        try:
            o.set_forcing(wek, ent, xon)
            o.set_p(po, pom)
            out["init"], out["init_scal"] = o.get_state(), o.get_scalars()
            o.steps(s0, n)
            out[tag], out[tag + "_scal"] = o.get_state(), o.get_scalars()
        finally:
            o.close()
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            assert np.isfinite(a).all()
            a.setflags(write=False)
    return out


def oracle_figures(grid, zero_ent):
    """A fresh handle (fused or, under QGCM_HIP_NO_BAND_ROWS=1, the two launches) against oracle_run: the number of
    interior qo points that differ in their bits after the one step 2, and after 27 steps relerr of every field and the
    error of the constraint scalars relative to xlo * ylo * max|po| (common.scal_err)."""
    from qgcm_hip import OceanModel
    cfg = wide_box(grid)
    _, _, wek, ent, ddy, xon = inputs(cfg, zero_ent)
    ref = oracle_run(grid, zero_ent)
    m = OceanModel(cfg, ddynoc=ddy)
    try:
        m.set_forcing(wek, ent, xon)
        assert m.tend_zero_mask() == (3 if zero_ent else 0)
        m.set_state(*ref["init"])
        m.set_scalars(ref["init_scal"])
        m.steps(1, s0=2)  # a plain step: fused
        st = m.get_state()
        qo, qr = st[2][1:-1, 1:-1, :], ref["one"][2][1:-1, 1:-1, :]
        fig = dict(qo_points=int((bits(qo) != bits(qr)).sum()), qo_maxdiff=float(np.abs(qo - qr).max()),
                   qo_moved=not np.array_equal(qo, ref["init"][2][1:-1, 1:-1, :]))
        fig["one"] = {f: relerr(x, y) for f, x, y in zip(FIELDS, st, ref["one"])}
        m.set_state(*ref["init"])
        m.set_scalars(ref["init_scal"])
        m.steps(ORACLE_STEPS, s0=1)
        end = m.get_state()
        assert all(np.isfinite(x).all() for x in end)
        fig["end"] = {f: relerr(x, y) for f, x, y in zip(FIELDS, end, ref["end"])}
        nl = cfg.nlo
        scale = cfg.xlo * cfg.ylo * np.abs(ref["end"][0]).max()
        fig["scal"] = float(np.abs(m.get_scalars()[:2 * (nl - 1)] - ref["end_scal"][:2 * (nl - 1)]).max() / scale)
        fig["moved"] = relerr(ref["end"][0], ref["init"][0])
    finally:
        m.close()
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_rows_vs_oracle(grid, zero_ent):
    """The reference that is not the sibling kernel: the CPU oracle on the same grid and inputs.

    ONE fused step (step 2, a plain one) from the oracle's start state: qo on the interior points (rows 2 .. ny-1,
    columns 2 .. nx-1) has the oracle's bits - the exactness the suite asserts of qgostep on other grids.

    27 steps (a graph block, the averaging steps 1 and 26, the tail): relerr of every field below TOL_60 and the
    constraint scalars below TOL_SCAL.  The tolerances are the suite's standing ones; what they rest on here is the
    TWO-LAUNCH path (QGCM_HIP_NO_BAND_ROWS=1, the code from before the fused kernel) against the oracle on these grids,
    measured on an MI355X - the largest relerr of po, pom, qo, qom after 27 steps, with entoc = 0 over a flat bottom /
    with entoc and ddynoc non-zero:

      961x6   2.2e-14 / 2.0e-14     961x16  1.9e-13 / 2.2e-13     961x36  3.2e-13 / 3.1e-13
      961x7   4.0e-14 / 4.3e-14     961x17  2.0e-13 / 1.9e-13     961x66  3.8e-13 / 3.7e-13
      961x9   7.8e-14 / 6.5e-14     961x33  3.7e-13 / 3.6e-13     961x67  4.3e-13 / 4.1e-13

    (always qo or qom; po and pom stay below 6e-15; the largest after ANY of the steps 1 .. 27 is 4.7e-13), the scalars
    0.0 in all eighteen runs: a factor of 200 inside TOL_60 although the state changes by up to 96 % of its own size, so
    all 27 steps are kept on every grid.  Interior qo after the one step had the oracle's bits on the two-launch path
    too, on all nine grids: the inversion and ocqbdy leave those points alone, no point is exempt."""
    fig = oracle_figures(grid, zero_ent)
    print(grid, zero_ent, fig)
    assert fig["qo_moved"]
    assert fig["qo_points"] == 0, (grid, zero_ent, fig["qo_points"], fig["qo_maxdiff"])
    assert all(v < TOL_60 for v in fig["end"].values()), (grid, zero_ent, fig["end"])
    assert fig["scal"] < TOL_SCAL, (grid, zero_ent, fig["scal"])


# ---- plan changes inside one handle ---------------------------------------------------------------------------------
def _snap(m, po):
    return m.get_state(), m.get_scalars(), m.tend_zero_mask(), po


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["961x16", "961x36"])
def test_plan_changes_keep_the_bits(grid, monkeypatch):
    """Two handles on one grid with a non-zero ddynoc, one of them created under QGCM_HIP_NO_BAND_ROWS=1, through the same
    five stages with the step number running on:

      1 entoc non-zero (mask 0): fused            2 entoc zero (mask 1): the two launches - the graph cache is hit under
      3 entoc non-zero again: fused                 another key, the fused blocks of stage 1 stay and stage 3 replays them
      4 qgcm_hip_set_cu_range(h, 64, 128): the two launches        5 qgcm_hip_set_cu_range(h, 0, 0): fused again

    A stage is 50 steps: 23 through profile_steps (eager, counted launch by launch; the first is an averaging step), then
    27 through steps() (a captured block of 26 with the averaging step in it, and the tail).  50 steps are two averaging
    cycles and an even number of buffer rotations, so the captured block of every stage has the same key but for the
    zero mask.  After either part the two handles agree in every bit of state and scalars; the counts of the normal
    handle show the forward rows on the averaging step alone in stages 1, 3, 5 and on every step in stages 2, 4 - the
    test cannot pass by never fusing."""
    from qgcm_hip import OceanModel
    cfg = wide_box(grid)
    po, pom, wek, ent, ddy, xon = inputs(cfg, False)
    zero = np.zeros_like(ent)
    ms = []
    try:
        for forced in (False, True):
            if forced:
                monkeypatch.setenv(SWITCH, "1")
            ms.append(OceanModel(cfg, ddynoc=ddy))
        monkeypatch.delenv(SWITCH)  # (read when a handle is created)
        for m in ms:
            m.set_p(po, pom)

        def cu_range(first, count):
            for m in ms:
                assert m.L.qgcm_hip_set_cu_range(m.h, first, count) == 0

        stages = [(lambda: None, ent, 0, True), (lambda: None, zero, 1, False), (lambda: None, ent, 0, True),
                  (lambda: cu_range(64, 128), ent, 0, False), (lambda: cu_range(0, 0), ent, 0, True)]
        s0 = 1
        for k, (change, e, mask, fused) in enumerate(stages, 1):
            change()
            counts = []
            for m in ms:
                m.set_forcing(wek, e, xon)
                assert m.tend_zero_mask() == mask, (k, m.tend_zero_mask())
                counts.append({name: n for name, (_, n) in m.profile_steps(23, s0=s0).items()})
            assert (s0 - 1) % 25 == 0  # (the one averaging step of the 23)
            assert counts[0]["k_tend"] == 23 and counts[0].get("k_dst_fwd", 0) == (1 if fused else 23), (k, counts[0])
            assert counts[1]["k_tend"] == 23 and counts[1].get("k_dst_fwd", 0) == 23, (k, counts[1])
            assert_same(_snap(ms[0], po), _snap(ms[1], po), (grid, "stage", k, "profiled"))
            for m in ms:
                m.steps(27, s0=s0 + 23)
            assert_same(_snap(ms[0], po), _snap(ms[1], po), (grid, "stage", k))
            s0 += 50
    finally:
        for m in ms:
            m.close()


def launches(cfg, zero_ent=True, flat=True, sponge=False, oml=False, cu_range=False):
    from qgcm_hip import OceanModel, oml_preset, synth
    po, pom, wek, ent, ddy, xon = inputs(cfg, zero_ent)
    if ddy is None and not flat:
        ddy = inputs(cfg, False)[4]
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
        mask = m.tend_zero_mask()
        prof = m.profile_steps(30, s0=1)
    finally:
        m.close()
    got = {k: n for k, (_, n) in prof.items() if n}
    got["mask"] = mask
    return got


@pytest.mark.gpu
def test_launch_plan_fused():
    """The forward rows launch on the two averaging steps only; the fused launch counts as k_tend."""
    got = launches(wide_box("961x17"))
    assert got["k_tend"] == 30 and got["k_dst_fwd"] == 2, got


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["switch", "sponge", "oml", "mask2", "cu_range", "mask1"])
def test_launch_plan_falls_back(why, monkeypatch):
    if why == "switch":
        monkeypatch.setenv(SWITCH, "1")
    # (mask2: non-zero entoc over a flat bottom, mask1: entoc zero over a non-flat bottom - instantiations the kernel
    #  does not have)
    got = launches(wide_box("961x17"), zero_ent=(why != "mask2"), flat=(why != "mask1"), sponge=(why == "sponge"),
                   oml=(why == "oml"), cu_range=(why == "cu_range"))
    if why in ("mask1", "mask2"):
        assert got["mask"] == int(why[4]), got
    assert got["k_tend"] == 30 and got["k_dst_fwd"] == 30, (why, got)


@pytest.mark.gpu
def test_launch_plan_of_box_med_is_unchanged():
    from test_gpu_launch_plan import EXPECTED, launches as plan_launches
    assert plan_launches("box_med") == EXPECTED["box_med"]


# ---- no GPU ---------------------------------------------------------------------------------------------------------
def test_band_shapes_are_covered(repo_root):
    """TR_BAND as k_tend_rows.h has it, the band shape of every grid of GRIDS recomputed from it: the table reaches
    every remainder of rows / B, one band that is first and last, one band per XCD at the most, several bands per XCD
    with idle workgroups and several with none.  After a retuning of TR_BAND the message names the shapes that want a
    grid."""
    src = open(os.path.join(repo_root, "q-gcm_amd", "csrc", "k_tend_rows.h")).read()
    hit = re.findall(r"constexpr\s+int\s+TR_BAND\s*=\s*(\d+)\s*;", src)
    assert len(hit) == 1, hit
    B = int(hit[0])
    shapes = {g: band_shape(wide_box(g).nypo, B) for g in GRIDS}
    print(B, shapes)
    if B == 4:  # (the table of the module docstring)
        assert shapes == {"961x9": (7, 3, 2, 1), "961x17": (15, 3, 4, 1), "961x33": (31, 3, 8, 1), "961x6": (4, 0, 1, 1),
                          "961x7": (5, 1, 2, 1), "961x16": (14, 2, 4, 1), "961x36": (34, 2, 9, 2),
                          "961x66": (64, 0, 16, 2), "961x67": (65, 1, 17, 3)}
    want = {"rows mod B == %d" % r: (lambda s, r=r: s[1] == r) for r in range(B)}
    want["nbands == 1"] = lambda s: s[2] == 1
    want["per_xcd == 1"] = lambda s: s[3] == 1
    want["per_xcd > 1 with idle workgroups (8 * per_xcd > nbands)"] = lambda s: s[3] > 1 and 8 * s[3] > s[2]
    want["per_xcd > 1 with no idle workgroup (8 * per_xcd == nbands)"] = lambda s: s[3] > 1 and 8 * s[3] == s[2]
    missing = [name for name, has in want.items() if not any(has(s) for s in shapes.values())]
    assert not missing, ("TR_BAND = %d: add grids to GRIDS that reach" % B, missing, shapes)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_inputs_vary_from_row_to_row_and_column_to_column(grid):
    """Every non-zero input field of inputs() differs between any two adjacent interior rows and any two adjacent
    interior columns, layer by layer: no load of a neighbouring row or column returns the right bits."""
    cfg = wide_box(grid)
    po, pom, wek, ent, ddy, xon = inputs(cfg, False)
    assert inputs(cfg, True)[4] is None and not inputs(cfg, True)[3].any()
    for name, a in (("po", po), ("pom", pom), ("wekpo", wek), ("entoc", ent), ("ddynoc", ddy)):
        a = a.reshape(cfg.nxpo, cfg.nypo, -1)[1:-1, 1:-1, :]
        assert a.shape[0] == cfg.nxpo - 2 and a.shape[1] == cfg.nypo - 2
        assert np.isfinite(a).all() and (a != 0.0).any(axis=(0, 1)).all(), name
        assert (np.diff(a, axis=0) != 0.0).all(), (grid, name, "adjacent columns")
        assert (np.diff(a, axis=1) != 0.0).all(), (grid, name, "adjacent rows")


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
