"""The ocean's time averages without a GPU: the numpy restatement tests/numpy_tavg.py reproduces the
golden values of the TRUE reference (tests/golden/make_golden_tavg.py: timavge.F's tavini / tavocn / tavout and
avg_ocn_k247) bitwise, and the new entry points are in header, binding and library."""
import ctypes
import os

import numpy as np
import pytest

import numpy_tavg as nt
from common import load_golden
from qgcm_hip import lib, model
from qgcm_hip.slab import HipSlab, SlabOcean

CASES = ["box_tiny", "box_tiny_sb", "cyc_tiny"]
# two, five and six layers (TAV_UU(nl) of the advection sums; fixtures box_tiny2, box_tiny5, cyc_tiny6)
LAYER_CASES = ["box_tiny2", "box_tiny5", "box_tiny5_sb", "cyc_tiny6"]
NEW = ["qgcm_hip_poavg_enable", "qgcm_hip_poavg_out", "qgcm_hip_set_tav_params", "qgcm_hip_set_tav_fields",
       "qgcm_hip_tavocn", "qgcm_hip_tav_reset", "qgcm_hip_tav_out"]


def golden_consts(g):
    return nt.consts(float(g["c_dxo"]), float(g["c_fnot"]), float(g["c_ycexp"]), float(g["c_hmoc"]),
                     float(g["c_tsbdy"]), float(g["c_tnbdy"]), int(g["c_cyclic"]), int(g["c_sb_hflux"]),
                     int(g["c_nb_hflux"]))


def load_tav(case):
    """tests/golden/tav_<case>.npz; the cases at other than three layers name the snapshots of their fixture that were
    the reference's po and qo (in<n>_state, avg_states) instead of holding a second copy: filled in here."""
    g = load_golden("tav_" + case)
    if "c_fixture" in g:
        fx = load_golden(str(g["c_fixture"]))
        n = 0
        while "in%d_state" % n in g:
            st = str(g["in%d_state" % n])
            g["in%d_po" % n], g["in%d_qo" % n] = fx[st + "_po"], fx[st + "_qo"]
            n += 1
        g["avg_po"] = np.stack([fx[str(s) + "_po"] for s in g["avg_states"]])
    return g


def calls(g):
    n = 0
    while "in%d_po" % n in g:
        yield {k[len("in%d_" % n):]: v for k, v in g.items() if k.startswith("in%d_" % n)}
        n += 1


@pytest.mark.parametrize("case", CASES + LAYER_CASES)
def test_restatement_reproduces_the_reference_bitwise(case):
    g = load_tav(case)
    c = golden_consts(g)
    nxpo, nypo, nlo = g["in0_po"].shape
    assert nlo == {"box_tiny2": 2, "box_tiny5": 5, "box_tiny5_sb": 5, "cyc_tiny6": 6}.get(case, 3)
    assert g["out_pocav"].shape == g["out_qocav"].shape == (nxpo, nypo, nlo)
    S = nt.tavini(nxpo, nypo, nlo)
    for f in calls(g):
        nt.tavocn(S, f, c)
    assert S["nsumoc"] == int(g["out_nsumoc"]) == 3
    M = nt.tavout(S)
    for name in nt.SUM_NAMES + ("uptpoc", "vptpoc"):
        assert M[name].shape == g["out_" + name].shape, name
        assert np.array_equal(M[name], g["out_" + name]), name
    po_sum = np.zeros_like(g["avg_po"][0])
    for p in g["avg_po"]:
        po_sum = po_sum + p
    assert np.array_equal(po_sum, g["out_po_sum"])
    assert np.array_equal(nt.po_mean(po_sum, len(g["avg_po"])), g["out_po_mean"])
    assert int(g["out_nsum_ocavg"]) == len(g["avg_po"])


def test_boundary_options_change_the_boundary_rows_only():
    for a, b in (("tav_box_tiny", "tav_box_tiny_sb"), ("tav_box_tiny5", "tav_box_tiny5_sb")):
        box, sb = load_golden(a), load_golden(b)  # (outputs only: no need for load_tav)
        d = box["out_vvfo"] != sb["out_vvfo"]
        assert d[:, 0].any() and not d[:, 1:].any()


def test_empty_sums_give_zero_means():
    M = nt.tavout(nt.tavini(5, 4, 2))
    assert all(not np.any(v) for v in M.values())


def test_library_and_binding_have_the_entry_points():
    path = lib.library_path()
    if not os.path.exists(path):
        pytest.fail("libqgcm_hip.so not built")
    L = ctypes.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in lib.SYMBOLS
    assert lib.TAV_NOUT == len(model.TAV_LAYOUT) == 16
    for name in ("enable_po_mean", "po_mean", "tavocn", "time_means", "reset_time_means", "set_time_mean_params",
                 "set_time_mean_fields"):
        assert callable(getattr(model.OceanModel, name))
        assert callable(getattr(HipSlab, name))
        assert callable(getattr(SlabOcean, name))


def test_tav_params_struct_layout(repo_root):
    assert ctypes.sizeof(lib.TavParams) == 4 * 8 + 2 * 4
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    body = hdr[hdr.index("typedef struct qgcm_hip_tav_params {"):hdr.index("} qgcm_hip_tav_params;")]
    pos = [body.index(" %s" % f[0]) for f in lib.TavParams._fields_]
    assert pos == sorted(pos)
    assert "#define QGCM_HIP_TAV_NOUT 16" in hdr
    # the output order of the header comment is TAV_LAYOUT's
    doc = hdr[hdr.index("qgcm_hip_tav_out(h, fields, nsumoc)"):hdr.index("typedef struct qgcm_hip_tav_params")]
    pos = [doc.index(" %s" % n) for n, _ in model.TAV_LAYOUT]
    assert pos == sorted(pos)


def test_new_kernels_do_not_spill(repo_root):
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.txt missing")
    seen, cur = 0, None
    for line in open(path):
        if "Function Name:" in line:
            cur = line.split("Function Name:")[1].split()[0]
        if cur and ("k_tav_" in cur or "k_poavg" in cur) and "ScratchSize" in line:
            assert line.split("ScratchSize [bytes/lane]:")[1].split()[0] == "0", cur
            seen += 1
    assert seen >= 2 * 7 + 7 + 1  # k_tav_accum (8 per nlo), k_tav_mean (7), k_poavg_add
