"""CPU checks of the y-slab diagnostics (qgcm_hip_*_part / _combine): the library exports them, the binding declares
them, and the compiler's resource report of the build shows that their kernels use no scratch."""
import ctypes
import os
import re

import pytest

from qgcm_hip import lib

NEW_SYMBOLS = ["qgcm_hip_monitor_part_len", "qgcm_hip_monitors_part", "qgcm_hip_monitors_combine",
               "qgcm_hip_valids_part_len", "qgcm_hip_valids_part", "qgcm_hip_valids_combine",
               "qgcm_hip_prsamp_part_len", "qgcm_hip_prsamp_part", "qgcm_hip_prsamp_combine"]


def test_symbols_declared_bound_and_exported(repo_root):
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    L = ctypes.CDLL(lib.library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in lib.SYMBOLS, s
        assert hasattr(L, s), s


def test_binding_sets_argtypes():
    L = lib.load_library()
    for s in NEW_SYMBOLS:
        assert getattr(L, s).argtypes is not None, s


def resources(repo_root):
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.txt missing - rebuild with `make -C q-gcm_amd/csrc`")
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split()[0]] = int(m.group(2))
    return res


def test_slab_diagnostic_kernels_use_no_scratch(repo_root):
    res = resources(repo_root)
    # the slab scan, the summary and combine kernels, all layer counts
    new = ["_Z14k_monslab_scanILi%dELb%dE" % (nl, cyc) for nl in range(2, 9) for cyc in (0, 1)]
    new += ["_Z14k_monslab_partILi", "_Z17k_monslab_combineILi", "_Z13k_valids_partILi", "_Z16k_valids_combineILi",
            "_Z13k_prsamp_partILi", "_Z16k_prsamp_combineILi", "_Z9k_mon_jet"]
    for h in new:
        hits = [k for k in res if k.startswith(h)]
        assert hits, "kernel %s not in the report" % h
        for k in hits:
            assert res[k]["ScratchSize"] == 0, "%s uses %d B of scratch per lane" % (k, res[k]["ScratchSize"])


def test_mon_scan_lds_unchanged(repo_root):
    res = resources(repo_root)
    hits = [k for k in res if k.startswith("_Z10k_mon_scanI") or k.startswith("_Z14k_monslab_scanI")]
    assert hits
    for k in hits:
        assert res[k]["LDS"] <= 47040, (k, res[k]["LDS"])
