"""The atmosphere's time averages and periodic dump (qgcm_hip_tavatm / _atm_tav_out / _atnc_sample) without a
GPU: the numpy restatement tests/numpy_atm_tavg.py reproduces the TRUE reference's tavatm / tavout / atnc_out
(tests/golden/atav_*.npz, make_golden_atm_tavg.py) bitwise, the library and the binding have the new entry points, the
Python methods exist, the Fortran interface declares them, and the new kernels do not spill."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import numpy_atm_tavg as na
from common import load_golden
from qgcm_hip import lib, model

NEW = ["qgcm_hip_set_atm_tav_fields", "qgcm_hip_tavatm", "qgcm_hip_atm_tav_reset", "qgcm_hip_atm_tav_out",
       "qgcm_hip_tavatm_schedule", "qgcm_hip_atnc_sample_len", "qgcm_hip_atnc_sample"]
GOLDEN = ["cpl_tiny", "cpl_small", "cpl_tiny_a4"]  # (the last: four layers, ah4at different in each)
NSKA = (1, 2, 5)


def golden_case(name):
    """(golden arrays, constants, the tavatm inputs in call order, the atnc_out inputs) of atav_<name>.npz."""
    g = load_golden("atav_" + name)
    c = na.consts(float(g["c_dxa"]), float(g["c_fnot"]), float(g["c_hmat"]))
    calls, n = [], 0
    while "in%d_pa" % n in g:
        calls.append({k[len("in%d_" % n):]: g[k] for k in g if k.startswith("in%d_" % n)})
        n += 1
    return g, c, calls, calls[-1]


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_the_reference_bitwise(name):
    g, c, calls, last = golden_case(name)
    nxpa, nypa, nla = calls[0]["pa"].shape
    S = na.tavini(nxpa, nypa, nla)
    for f in calls:
        na.tavatm(S, f, c)
    assert S["nsumat"] == int(g["out_nsumat"]) == 3
    M = na.tavout(S)
    for n, _ in model.ATM_TAV_LAYOUT:
        assert M[n].shape == g["out_" + n].shape, n
        assert np.array_equal(M[n], g["out_" + n]), n
    for nska in NSKA:
        d = na.atnc_out(last, g["c_gpat"], nska)
        assert list(d) == list(na.ATNC_NAMES)
        for k, v in d.items():
            want = g["n%d_%s" % (nska, k)]
            assert v.shape == want.shape and np.array_equal(v, want), (nska, k)
            rows, cols = v.shape[1:]
            nx = nxpa - (k in ("ast", "wekta", "hmixa"))
            ny = nypa - (k in ("ast", "wekta", "hmixa"))
            assert (cols, rows) == (model.subsample_count(nx, nska), model.subsample_count(ny, nska))


def test_the_goldens_tell_column_nxpa_from_column_1():
    """The forcing's column nxpa differs from column 1, so a zonal flux copied from column 1 (the cyclic ocean's rule)
    fails the comparison; tuf(nxpa) is tuf(1) by the reference's own rule."""
    for name in GOLDEN:
        g, _, calls, _ = golden_case(name)
        assert not np.array_equal(calls[0]["tauya"][-1], calls[0]["tauya"][0])
        assert not np.array_equal(g["out_uufa"][-1], g["out_uufa"][0])
        assert np.array_equal(g["out_tufa"][-1], g["out_tufa"][0])
        # the zonal boundaries: no meridional flux
        assert not np.any(g["out_vvfa"][:, [0, -1]]) and not np.any(g["out_vtvfa"][:, [0, -1]])


def test_empty_sums_give_zero_means():
    M = na.tavout(na.tavini(6, 5, 3))
    assert all(not np.any(v) for v in M.values())


def test_library_binding_and_methods():
    path = lib.library_path()
    if not os.path.exists(path):
        pytest.fail("libqgcm_hip.so not built")
    L = ctypes.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in lib.SYMBOLS
    assert lib.ATM_TAV_NOUT == len(model.ATM_TAV_LAYOUT) == 15
    assert [n for n, *_ in model.ATNC_FIELDS] == list(na.ATNC_NAMES)
    for name in ("set_time_mean_fields", "tavatm", "time_means", "reset_time_means", "schedule_time_means",
                 "atmos_dump"):
        assert callable(getattr(model.AtmosModel, name))
    for name in ("set_time_mean_fields", "time_means", "reset_time_means"):
        assert getattr(model.AtmosModel, name) is not getattr(model.OceanModel, name)
    # tavocn() stays the ocean's (the library refuses an atmosphere handle)
    assert model.AtmosModel.tavocn is model.OceanModel.tavocn


def test_header_order_and_constant(repo_root):
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    assert "#define QGCM_HIP_ATM_TAV_NOUT 15" in hdr
    doc = hdr[hdr.index("qgcm_hip_atm_tav_out(h, fields, nsumat)"):hdr.index("qgcm_hip_tavatm_schedule(h, every, phase)")]
    pos = [doc.index(" %s" % n) for n, _ in model.ATM_TAV_LAYOUT]
    assert pos == sorted(pos)
    doc = hdr[hdr.index("qgcm_hip_atnc_sample(h, nska, outflat, out)"):hdr.index("#define QGCM_HIP_ATM_TAV_NOUT")]
    pos = [re.search(r"\b%s\b" % n, doc).start() for n in na.ATNC_NAMES]
    assert pos == sorted(pos)


def test_fortran_interface_declares_the_entry_points(repo_root, tmp_path):
    fc = "/opt/rocm/bin/amdflang"
    if not os.path.exists(fc):
        pytest.fail("amdflang not found")
    src = os.path.join(repo_root, "q-gcm_amd", "fortran", "qgcm_hip_iface.F90")
    subprocess.check_call([fc, "-c", src, "-o", str(tmp_path / "iface.o"), "-J", str(tmp_path)], cwd=str(tmp_path))
    text = open(src).read()
    for s in NEW:
        assert "name='%s'" % s in text, s


def test_new_kernels_do_not_spill(repo_root):
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.txt missing - rebuild with `make -C q-gcm_amd/csrc`")
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            res[cur] = int(m.group(1))
    new = [k for k in res if "k_tavat_accum" in k or "k_atnc_sample" in k]
    assert sum(1 for k in new if "k_tavat_accum" in k) == 7 and sum(1 for k in new if "k_atnc_sample" in k) == 1
    for k in new:
        assert res[k] == 0, "%s spills %d B per lane" % (k, res[k])
