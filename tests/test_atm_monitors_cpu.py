"""The atmosphere monitors and valids (qgcm_hip_atm_monitors / _atm_valids) without a GPU: the library
exports the new entry points, the Python wrappers, the struct and the packed layout agree with include/qgcm_hip.h, the
new kernels do not spill, the Fortran interface declares them, and the numpy restatement tests/numpy_atm_monitors.py
reproduces the reference's own monnc_comp / courat / valids (tests/golden/atmon_*.npz, make_golden_atm_monnc.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import numpy_atm_monitors as na
from common import load_golden
from qgcm_hip import lib, model

NEW = ["qgcm_hip_set_atm_mon_params", "qgcm_hip_set_atm_monitor_fields", "qgcm_hip_atm_monitor_len",
       "qgcm_hip_atm_monitors", "qgcm_hip_atm_valids"]
# bitwise against the reference: extrema, Courant numbers, jet position and value, tmaooc
EXACT = ("astmin", "astmax", "tmaooc", "umminat", "ummaxat", "vmminat", "vmmaxat", "cnmlat", "ugminat", "ugmaxat",
         "vgminat", "vgmaxat", "cnqgat", "atstpos", "atstval")
GOLDEN = ["cpl_tiny", "cpl_small", "cpl_tiny_a4"]  # (the last: four layers, ah4at different in each)


def golden_case(name):
    """Inputs f, constants c, the reference's monitors (dict), valids extrema and solnok of atmon_<name>.npz."""
    g = load_golden("atmon_" + name)
    f = {k[3:]: g[k] for k in g if k.startswith("in_")}
    c = {k[2:]: (g[k] if g[k].ndim else g[k][()]) for k in g if k.startswith("c_")}
    return f, c, model.unpack_atm_monitors(g["monitors"], f["pa"].shape[2]), g["valids"], g["solnok"]


def test_library_exports_the_atm_monitor_entry_points():
    path = lib.library_path()
    if not os.path.exists(path):
        pytest.fail("libqgcm_hip.so not built")
    L = ctypes.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in lib.SYMBOLS
    for name in ("set_atm_monitor_params", "set_atm_monitor_fields", "atm_valids"):
        assert callable(getattr(model.AtmosModel, name))
    # monitors() / monitor_vector() are the atmosphere's own on AtmosModel
    assert model.AtmosModel.monitors is not model.OceanModel.monitors
    assert model.AtmosModel.monitor_vector is not model.OceanModel.monitor_vector
    assert model.AtmosModel.valids is model.OceanModel.valids


def test_atm_mon_params_struct_layout(repo_root):
    assert ctypes.sizeof(lib.AtmMonParams) == 4 * 8 + 7 * 8 + 3 * 8 + 4 * 4
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    body = hdr[hdr.index("typedef struct qgcm_hip_atm_mon_params {"):hdr.index("} qgcm_hip_atm_mon_params;")]
    pos = [body.index(" %s" % f[0]) for f in lib.AtmMonParams._fields_]
    assert pos == sorted(pos)


@pytest.mark.parametrize("nl", [2, 3, 5, 8])
def test_atm_layout_length_and_order(repo_root, nl):
    n = sum({0: 1, -1: nl - 1, 1: nl}[k] for _, k in model.ATM_MONITOR_LAYOUT)
    assert n == 18 * nl + 11
    d = model.unpack_atm_monitors(np.arange(n, dtype=np.float64), nl)
    assert d["wetmat"] == 0.0 and d["cnqgat"][-1] == n - 1
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    blk = hdr[hdr.index("qgcm_hip_atm_monitors(h, out) fails"):hdr.index("As the reference writes them")]
    names = [w for w in re.findall(r"\b([a-z][a-z0-9]+)\b", blk) if w in d]
    assert names == [nme for nme, _ in model.ATM_MONITOR_LAYOUT]


def test_atm_mon_params_defaults():
    from qgcm_hip import atmos_preset, preset
    a, o = atmos_preset("cpl_natl5"), preset("cpl_natl5")
    p = model.atm_mon_params(a, o)
    assert (p.rhoat, p.cpat, p.hmat, p.davgat) == (1.0, 1.0e3, 1000.0, 0.0)
    assert (p.nxaooc, p.nyaooc) == (60, 60) and (p.nx1, p.ny1) == (1 + (384 - 60) // 2, 1 + (96 - 60) // 2)
    with pytest.raises(lib.QgcmHipError):
        model.atm_mon_params(a)


def test_atm_kernels_do_not_spill(repo_root):
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
    new = [k for k in res if "k_atmon_" in k or "k_atval" in k]
    assert sum(1 for k in new if "k_atmon_scan" in k) == 7 and sum(1 for k in new if "k_atmon_final" in k) == 7
    assert any("k_atmon_chain" in k for k in new) and any("k_atval" in k for k in new)
    for k in new:
        assert res[k] == 0, "%s spills %d B per lane" % (k, res[k])


def test_fortran_interface_declares_the_atm_entry_points(repo_root, tmp_path):
    fc = "/opt/rocm/bin/amdflang"
    if not os.path.exists(fc):
        pytest.fail("amdflang not found")
    src = os.path.join(repo_root, "q-gcm_amd", "fortran", "qgcm_hip_iface.F90")
    subprocess.check_call([fc, "-c", src, "-o", str(tmp_path / "iface.o"), "-J", str(tmp_path)], cwd=str(tmp_path))
    text = open(src).read()
    for s in NEW:
        assert "name='%s'" % s in text, s
    assert "type, bind(C) :: qgcm_hip_atm_mon_params" in text


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_the_reference(name):
    f, c, want, val, ok = golden_case(name)
    v, s = na.monitors(f, c)
    assert set(v) == set(want) == set(dict(model.ATM_MONITOR_LAYOUT))
    # a non-trivial case: rates, the entrainment term and the stress work are non-zero, every layer has a jet
    assert np.all(want["ddtkeat"] != 0.0) and want["pkenat"][0] != 0.0 and want["utauat"] != 0.0
    assert np.all(want["atstpos"] > 0) and want["tmaooc"] != 0.0 and want["olrtop"] != 0.0
    for n in want:
        got, ref, sc = np.atleast_1d(v[n]), np.atleast_1d(want[n]), np.atleast_1d(s[n])
        if n in EXACT:
            assert np.array_equal(got, ref), n
        else:
            assert np.all(np.abs(got - ref) <= 1e-13 * sc), (n, got, ref)
    assert np.array_equal(na.valids(f), val)
    assert na.solnok(val) == bool(ok[0]) and ok[0] == 1.0 and ok[1] == 0.0
