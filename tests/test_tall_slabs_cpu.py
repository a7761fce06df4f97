"""CPU checks of the y-slabs cut into segments (k_thomas_slab.h): the library exports qgcm_hip_thomas_plan, the header and
the binding declare it, and the compiler's resource report of the build shows that the new kernels exist and use no
scratch."""
import ctypes
import re

import os

from qgcm_hip import lib
from test_slab_diagnostics_cpu import resources


def test_plan_entry_declared_bound_and_exported(repo_root):
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    L = ctypes.CDLL(lib.library_path())
    s = "qgcm_hip_thomas_plan"
    assert re.search(r"\b%s\(" % s, hdr)
    assert s in lib.SYMBOLS
    assert hasattr(L, s)
    assert getattr(lib.load_library(), s).argtypes is not None
    assert "QGCM_HIP_THOMAS_SLAB_SEG_ROWS" in hdr
    assert lib.load_library().qgcm_hip_abi_version() == 3


def test_segmented_slab_kernels_use_no_scratch(repo_root):
    res = resources(repo_root)
    # the fold of the segments' summaries, set-up and per-solve half, and the correction pass over a slab's segments
    for h in ("_Z13k_thomas_foldILb1EE", "_Z13k_thomas_foldILb0EE", "_Z18k_thomas_corr_slab"):
        hits = [k for k in res if k.startswith(h)]
        assert hits, "kernel %s not in the report" % h
        for k in hits:
            assert res[k]["ScratchSize"] == 0, "%s uses %d B of scratch per lane" % (k, res[k]["ScratchSize"])
