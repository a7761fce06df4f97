"""The two strip bodies of the row-band kernel (k_tend_rows.h, k_tend_rows_strip.inc): a strip steps without the wall
rule, without row or column clamps and without the partial-band break when its band is out of reach of the wall ROWS and
the strip itself out of reach of the wall COLUMNS; every other strip takes the body with the rule.  Where no wall is in
reach the wall body's selects return the interior values, so the choice cannot change a bit - unless a predicate is
wrong.

Band predicate, restated here from the cascade (not from the kernel's text): with B = TR_BAND = 4 rows per band and
j0 = 2 + B b the first row of band b, the widest level, Del^2, is formed on rows j0 - 2 .. j0 + B + 1; the band is
wall-free iff all of them are interior rows 2 .. ny - 1, that is b >= 1 and ny >= 4 b + 8.  It is NOT "neither first nor
last": the band before a short last band can reach row ny, and so can the middle band of three.  A partial band is never
wall-free.  Path of every band (W: wall body, F: wall-free), and ny - (4 b + 8) of the bands b >= 1 - the predicate
flips between -1 and 0, and the grids together reach every value from -1 to 3:

  grid     bands  path                 ny - (4 b + 8), b = 1 ..
  961x6      1    W
  961x7      2    WW                   -5
  961x9      2    WW                   -3
  961x11     3    WWW                  -1 -5          the middle band's top Del^2 row is the N wall row
  961x13     3    WFW                   1 -3          one wall-free band between two wall bands, a last band of 3 rows
  961x16     4    WFFW                  4  0 -4
  961x17     4    WFFW                  5  1 -3
  961x33     8    WFFFFFFW             21 17 13  9  5  1 -3
  961x36     9    WFFFFFFFW            24 20 16 12  8  4  0 -4
  961x66    16    WFFFFFFFFFFFFFFW     54 50 .. 6  2 -2
  961x67    17    WFFFFFFFFFFFFFFWW    55 51 .. 7  3 -1 -5

All but 961x11 and 961x13 are the grids of test_gpu_band_rows.py, which therefore pins the wall-free body bitwise
against the two launches and the oracle already; the two new grids run here through the same helpers and bars.

Strip predicate: no lane of the strip (56 owned columns and 4 halo lanes on either side) is column 1 or nx; at nx = 961
strips 1 .. 16 of 18."""
import os
import re

import numpy as np
import pytest

import test_gpu_band_rows as tbr

PATH_GRIDS = {"961x11": (5, 192, 2), "961x13": (3, 320, 4)}  # ndxr, nxaooc, nyaooc
PATHS = {"961x6": "W", "961x7": "WW", "961x9": "WW", "961x11": "WWW", "961x13": "WFW", "961x16": "WFFW",
         "961x17": "WFFW", "961x33": "WFFFFFFW", "961x36": "WFFFFFFFW", "961x66": "W" + 14 * "F" + "W",
         "961x67": "W" + 14 * "F" + "WW"}


def box(grid):
    """wide_box of test_gpu_band_rows for its grids and for the two of this module."""
    if grid in tbr.GRIDS:
        return _wide_box(grid)
    from qgcm_hip.config import OceanConfig
    ndxr, nxa, nya = PATH_GRIDS[grid]
    cfg = OceanConfig("band_" + grid, nxa + 8, nya + 5, nxa, nya, ndxr, 3, dxo=5.0e3, dta=240.0, fnot=9.37456e-05,
                      beta=1.7536e-11, cyclic=False, **tbr.LAY)
    assert cfg.nxto == 960 and cfg.nypo == int(grid.split("x")[1])
    return cfg


_wide_box = tbr.wide_box


@pytest.fixture
def both_grid_sets(monkeypatch):
    """The helpers of test_gpu_band_rows look their grid up by name: let them find the grids of this module too."""
    monkeypatch.setattr(tbr, "wide_box", box)


def band_is_wall_free(b, ny, B):
    return b >= 1 and ny >= B * b + B + 4  # (B = 4: ny >= 4 b + 8)


# ---- no GPU ---------------------------------------------------------------------------------------------------------
def test_band_paths_match_the_table(repo_root):
    src = open(os.path.join(repo_root, "q-gcm_amd", "csrc", "k_tend_rows.h")).read()
    hit = re.findall(r"constexpr\s+int\s+TR_BAND\s*=\s*(\d+)\s*;", src)
    assert len(hit) == 1, hit
    B = int(hit[0])
    assert B == 4, ("TR_BAND = %d: the table of band paths in this module's docstring, PATHS and the grids chosen to "
                    "reach ny - (4 b + 8) = -1 .. 3 are those of four-row bands; recompute them for the new height" % B)
    reached = set()
    for grid, want in PATHS.items():
        ny = box(grid).nypo
        rows, _, nbands, _ = tbr.band_shape(ny, B)
        got = ""
        for b in range(nbands):
            free = band_is_wall_free(b, ny, B)
            # the definition: every row on which the cascade forms Del^2 is an interior row - and the band is whole
            j0 = 2 + B * b
            by_rows = all(2 <= j <= ny - 1 for j in range(j0 - 2, j0 + B + 2))
            assert free == by_rows, (grid, b)
            if free:
                assert j0 + B - 1 <= ny - 1 and j0 - 3 >= 1 and j0 + B + 2 <= ny, (grid, b, "a partial band or a clamped row")
            if b >= 1:
                reached.add(ny - (4 * b + 8))
            got += "F" if free else "W"
        assert got == want, (grid, got, want)
        assert got[0] == "W" and got[-1] == "W"
    assert set(PATHS) == set(tbr.GRIDS) | set(PATH_GRIDS)
    assert {-1, 0, 1, 2, 3} <= reached, sorted(reached)
    # what the two new grids are for
    assert "F" not in PATHS["961x11"] and len(PATHS["961x11"]) == 3
    assert PATHS["961x13"] == "WFW" and tbr.band_shape(13, B)[1] == 3


def test_strip_paths_at_961():
    """Lanes of strip s are columns 56 s - 3 .. 56 s + 60: wall-free iff none is column 1 or nx and all lie inside."""
    nx, free = 961, []
    for s in range((nx + 55) // 56):
        cols = range(56 * s + 1 - 4, 56 * s + 1 - 4 + 64)
        free.append(all(2 <= c <= nx - 1 for c in cols))
    assert free == [False] + 16 * [True] + [False]


# ---- GPU: the two new grids through the helpers of test_gpu_band_rows -------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("nsteps", [3, 27])
@pytest.mark.parametrize("grid", list(PATH_GRIDS))
def test_fused_rows_are_bitwise_the_two_launches(grid, nsteps, zero_ent, monkeypatch):
    cfg = box(grid)
    a = tbr.stepped(cfg, zero_ent, nsteps)
    assert a[2] == (3 if zero_ent else 0)
    monkeypatch.setenv(tbr.SWITCH, "1")
    b = tbr.stepped(cfg, zero_ent, nsteps)
    tbr.assert_same(a, b, (grid, nsteps, zero_ent))


@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("grid", list(PATH_GRIDS))
def test_graph_replay_is_the_eager_calls(grid, zero_ent):
    cfg = box(grid)
    tbr.assert_same(tbr.stepped(cfg, zero_ent, 3), tbr.stepped(cfg, zero_ent, 3, eager=True), (grid, zero_ent))


@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("grid", list(PATH_GRIDS))
def test_fused_rows_vs_oracle(grid, zero_ent, both_grid_sets):
    """Interior qo after ONE fused step has the oracle's bits; 27 steps stay inside the standing tolerances
    (test_gpu_band_rows.test_fused_rows_vs_oracle, whose figures bound these shorter grids too)."""
    fig = tbr.oracle_figures(grid, zero_ent)
    print(grid, zero_ent, fig)
    assert fig["qo_moved"]
    assert fig["qo_points"] == 0, (grid, zero_ent, fig["qo_points"], fig["qo_maxdiff"])
    assert all(v < tbr.TOL_60 for v in fig["end"].values()), (grid, zero_ent, fig["end"])
    assert fig["scal"] < tbr.TOL_SCAL, (grid, zero_ent, fig["scal"])
