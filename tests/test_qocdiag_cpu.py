"""The ocean's periodic dumps without a GPU: the numpy restatement tests/numpy_qocdiag.py reproduces the
golden values of the TRUE reference (tests/golden/make_golden_qocdiag.py: qocdiag.F's qocdiag_out and nc_subs.F's
ocnc_out, compiled unmodified) bitwise, and the new entry points are in header, binding and library."""
import ctypes
import os

import numpy as np
import pytest

import numpy_qocdiag as nq
from common import load_golden
from qgcm_hip import lib, model, preset
from qgcm_hip.slab import HipSlab, SlabOcean

CASES = ["box_tiny", "cyc_tiny", "box_tiny_ah2", "box_tiny5", "cyc_tiny6"]
NSKO = (1, 2, 7)
NEW = ["qgcm_hip_qocdiag_len", "qgcm_hip_qocdiag", "qgcm_hip_qocdiag_schedule", "qgcm_hip_qocdiag_read",
       "qgcm_hip_ocnc_sample_len", "qgcm_hip_ocnc_sample", "qgcm_hip_subsample_rows"]
# ocnc_out's netCDF variable names (src/nc_subs.F:ocnc_init) -> the keys of OceanModel.ocean_dump
NC_NAMES = dict(sst="sst", po="p", qo="q", wekto="wekt", h="h", tauxo="taux", tauyo="tauy")


def golden_inputs(g):
    return {k[3:]: g[k] for k in g if k.startswith("in_")}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nsko", NSKO)
def test_restatement_reproduces_the_reference_bitwise(case, nsko):
    g = load_golden("qod_" + case)
    cfg = preset(case)
    f = golden_inputs(g)
    got = nq.budget(f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"], nq.consts(cfg), nsko)
    for t in nq.TERMS:
        key = "n%d_qd_%s" % (nsko, t)
        if t == "qt2dif" and key not in g:  # the reference writes qt2dif only when some ah2oc is nonzero
            assert not any(cfg.ah2oc[:cfg.nlo]) and not got[t].any()
            continue
        assert got[t].shape == g[key].shape, t
        assert np.array_equal(got[t], g[key]), t
    nc = nq.ocnc(f["sst"], f["po"], f["qo"], f["wekto"], f["tauxo"], f["tauyo"], cfg.gpoc, nsko)
    for name, v in nc.items():
        assert np.array_equal(v, g["n%d_nc_%s" % (nsko, NC_NAMES[name])]), name


def test_golden_cases_exercise_the_branches():
    assert "n1_qd_qt2dif" in load_golden("qod_box_tiny_ah2")
    assert "n1_qd_qt2dif" not in load_golden("qod_box_tiny")
    g5 = load_golden("qod_box_tiny5")
    ent = g5["n1_qd_qotent"]
    assert ent.shape[0] == 5 and ent[0].any() and ent[1].any() and not ent[2:4].any() and ent[4].any()
    # nsko = 7 on 49 x 37: mod = 0 in x (7 columns), mod = 2 in y (6 rows)
    assert g5["n7_qd_dqdt"].shape[1:] == (6, 7)


def test_subsample_counts():
    assert [model.subsample_count(49, s) for s in NSKO] == [49, 25, 7]
    assert [model.subsample_count(37, s) for s in NSKO] == [37, 19, 6]
    assert model.subsample_count(48, 7) == nq.count(48, 7) == 7


def test_library_and_binding_have_the_entry_points(repo_root):
    path = lib.library_path()
    if not os.path.exists(path):
        pytest.fail("libqgcm_hip.so not built")
    L = ctypes.CDLL(path)
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in lib.SYMBOLS
        assert " %s(" % s in hdr, s
    for name in ("vorticity_budget", "schedule_vorticity_budget", "read_vorticity_budgets", "ocean_dump"):
        assert callable(getattr(model.OceanModel, name))
    for name in ("vorticity_budget", "ocean_dump", "subsample_rows"):
        assert callable(getattr(HipSlab, name))
    for name in ("vorticity_budget", "ocean_dump"):
        assert callable(getattr(SlabOcean, name))


def test_new_kernels_do_not_spill(repo_root):
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.txt missing")
    seen, cur = 0, None
    for line in open(path):
        if "Function Name:" in line:
            cur = line.split("Function Name:")[1].split()[0]
        if cur and ("k_qocdiag" in cur or "k_ocnc_sample" in cur) and "ScratchSize" in line:
            assert line.split("ScratchSize [bytes/lane]:")[1].split()[0] == "0", cur
            seen += 1
    assert seen >= 3  # k_qocdiag (box, cyclic), k_ocnc_sample
