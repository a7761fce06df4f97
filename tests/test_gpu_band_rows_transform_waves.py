"""The transform waves of the row-band kernel (k_tend_rows.h): the forward row transforms of a band run on the LAST
B/2 x NL waves of the workgroup (waves 6 .. 11 of 12), which take their LDS region and their (row pair, mode) from the
transform index tx = wave - 6, request the transform's tables and write their W64 row in front of the workgroup barrier,
and must reach that barrier exactly once whether their row pair exists or not.

Grids, all 961 wide, with B = TR_BAND = 4 rows per band (band_shape of test_gpu_band_rows):

  grid     rows  bands  what it reaches
  961x8       6    2    the last band holds ONE row pair: the three transform waves of the absent pair have requested
                        their tables like the others, pass the barrier and leave
  961x10      8    2    two whole bands, each of them first or last (both wall-row copies, no band out of reach of a wall)
  961x12     10    3    whole, whole, one pair

On each grid, through the helpers and bars of test_gpu_band_rows.py: fused == the two launches (QGCM_HIP_NO_BAND_ROWS=1)
bit for bit after 3 and after 27 steps, graph replay == the eager calls, both with entoc zero over a flat bottom (ZM = 3)
and with entoc and ddynoc non-zero everywhere (ZM = 0).  A region taken from the wave number instead of tx transforms
rows nobody wrote; yporel of a neighbouring row changes the modal right-hand side of every row: neither keeps the bits."""
import pytest

import test_gpu_band_rows as tbr

WAVE_GRIDS = {"961x8": (1, 960, 7), "961x10": (3, 320, 3), "961x12": (1, 960, 11)}  # ndxr, nxaooc, nyaooc
SHAPES = {"961x8": (6, 2, 2, 1), "961x10": (8, 0, 2, 1), "961x12": (10, 2, 3, 1)}   # rows, rows mod 4, nbands, per_xcd


def box(grid):
    from qgcm_hip.config import OceanConfig
    ndxr, nxa, nya = WAVE_GRIDS[grid]
    cfg = OceanConfig("band_" + grid, nxa + 8, nya + 5, nxa, nya, ndxr, 3, dxo=5.0e3, dta=240.0, fnot=9.37456e-05,
                      beta=1.7536e-11, cyclic=False, **tbr.LAY)
    assert cfg.nxto == 960 and cfg.nypo == int(grid.split("x")[1])
    return cfg


# ---- no GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(WAVE_GRIDS))
def test_grids_have_the_band_shapes_of_the_table(grid):
    cfg = box(grid)
    assert tbr.band_shape(cfg.nypo, 4) == SHAPES[grid]
    rows, _, nbands, _ = SHAPES[grid]
    pairs_in_last_band = (rows - 4 * (nbands - 1) + 1) // 2
    assert pairs_in_last_band == {"961x8": 1, "961x10": 2, "961x12": 1}[grid]
    # (the inputs vary from row to row and column to column on these grids too)
    for a in tbr.inputs(cfg, False)[:3]:
        a = a.reshape(cfg.nxpo, cfg.nypo, -1)[1:-1, 1:-1, :]
        assert (a[1:] != a[:-1]).all() and (a[:, 1:] != a[:, :-1]).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("nsteps", [3, 27])
@pytest.mark.parametrize("grid", list(WAVE_GRIDS))
def test_fused_rows_are_bitwise_the_two_launches(grid, nsteps, zero_ent, monkeypatch):
    cfg = box(grid)
    a = tbr.stepped(cfg, zero_ent, nsteps)
    assert a[2] == (3 if zero_ent else 0)
    monkeypatch.setenv(tbr.SWITCH, "1")
    b = tbr.stepped(cfg, zero_ent, nsteps)
    tbr.assert_same(a, b, (grid, nsteps, zero_ent))


@pytest.mark.gpu
@pytest.mark.parametrize("zero_ent", [True, False])
@pytest.mark.parametrize("grid", list(WAVE_GRIDS))
def test_graph_replay_is_the_eager_calls(grid, zero_ent):
    cfg = box(grid)
    tbr.assert_same(tbr.stepped(cfg, zero_ent, 3), tbr.stepped(cfg, zero_ent, 3, eager=True), (grid, zero_ent))
