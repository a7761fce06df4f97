#!/usr/bin/env python3
"""Golden values of xforc at refinements above 64 from the TRUE reference: the momentum half at ndxr = 75,
80 and 128 and the heat half with the mixed layer's chain at ndxr = 80.

The builds, the drivers, the inputs and the branch check are make_golden_xforc.py's and make_golden_heat.py's own,
imported from there and unchanged; this script only names the cases and packs the files.  What differs from those
generators' files: the five weight tables (3.7 to 10.6 MB per case) are not stored.  The reference's tables are
asserted bitwise hostinit.bcuini(ndxr, bccoat, dya) here, and per table the sum of the int64 views modulo 2^64 is
recorded (tabsum_<name>), which tests/test_wide_ndxr_cpu.py recomputes from bcuini.  A case keeps two states where the
packed file stays below 1 MiB and one where it would not.

The cases and what each is for (XFW_G = 32 atmosphere p points per workgroup of k_xf_wekpa_stage, k_xf_wekpa_stage.h):
  xf_r80_ud     the natl1 preset's refinement on a box ocean.  nxpa = 37: two workgroups of the staged box average on a
                row, the second with 5 of its 32 points, the cyclic wrap reached from the first and from the last;
                nxta % 8 = 4: a tail workgroup of k_xf_fine
  xf_r75_ud     odd ndxr above 64: half weights, nijwid = 76, the paired jsou / jnor rows (nxto = 150 = 2 * 3 * 5^2)
  xf_cyc80_ud   cyclic ocean as wide as the atmosphere, nxpo = 321: the ocean's own line integrals
  xf_r128_ud    the limit of the range on the smallest grid the reference takes, nypa = 3 (CPU tests: a device handle
                needs four p rows)
  xf_r128n3_ud  the same with nypa = 4, the smallest atmosphere a device handle takes
  heat_r80      make_golden_heat.py's chain of K = 3 cycles of [xforc; 3 x aml] at ndxr = 80: k_xf_heat_oc's loop over
                the 6400 ocean points of a cell takes a hundred rounds of 64

  python tests/golden/make_golden_wide_ndxr.py           # writes tests/golden/{xf_r80_ud,...,heat_r80}.npz
  python tests/golden/make_golden_wide_ndxr.py NAME ...  # writes only the named cases
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "q-gcm_amd", "python"))
import make_golden_heat as mh  # noqa: E402
import make_golden_xforc as mx  # noqa: E402
from qgcm_hip import hostinit  # noqa: E402

LIMIT = 1 << 20
# (file, (nxta, nyta, nxaooc, nyaooc, ndxr), cyclic ocean, states wanted); all with tau_udiff
XF_CASES = [("xf_r80_ud", (36, 4, 2, 1, 80), False, 2),
            ("xf_r75_ud", (8, 4, 2, 1, 75), False, 2),
            ("xf_cyc80_ud", (4, 4, 4, 1, 80), True, 1),
            ("xf_r128_ud", (4, 2, 1, 1, 128), False, 1),
            ("xf_r128n3_ud", (4, 3, 1, 1, 128), False, 1)]
# (file, dims, cyclic ocean, plain)
HEAT_CASES = [("heat_r80", (12, 4, 2, 1, 80), False, False)]


def table_sum(t):
    """The sum of a table's int64 views modulo 2^64 (as an int64, in Fortran order: the order does not matter)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(t, dtype=np.float64)).view(np.int64).sum(dtype=np.int64)


def xf_case(name, dims, cyc, nstates):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    pairs = [mx.smooth_pair(dims, cyc, 100 + s) for s in range(nstates)]
    wrk = tempfile.mkdtemp(prefix="xf_")
    try:
        mx.build(wrk, dims, cyc, True)
        res = mx.run(wrk, dims, pairs)
    finally:
        shutil.rmtree(wrk, ignore_errors=True)
    T = hostinit.bcuini(ndxr, mx.CONST["bccoat"], ndxr * mx.CONST["dxo"])
    out = dict(c_dims=np.array(dims, dtype=np.int64), c_cyclic=np.int64(cyc), c_tau_udiff=np.int64(1),
               c_nx1=np.int64(1 + (nxta - nxaooc) // 2), c_ny1=np.int64(1 + (nyta - nyaooc) // 2),
               c_fnot=np.float64(float(mx.FNOT.replace("D", "e"))))
    out.update({"c_" + k: np.float64(v) for k, v in mx.CONST.items()})
    for t in mx.TABLES:
        ref = res.pop("tab_" + t)
        assert np.array_equal(np.asfortranarray(T[t]).ravel(order="F").view(np.int64), ref.ravel(order="F").view(np.int64)), (name, t)
        out["tabsum_" + t] = table_sum(ref)
    names = [n for n, _ in mx.shapes(dims)]
    for keep in range(nstates, 0, -1):  # as many states as fit
        d = dict(out)
        for s in range(keep):
            d["in%d_pam1" % s], d["in%d_pom1" % s] = pairs[s]
            d.update({"out%d_%s" % (s, n): res["out%d_%s" % (s, n)] for n in names})
        d["c_nstates"] = np.int64(keep)
        if mh.packed_size(d) < LIMIT:
            break
    return {name: d}


def heat_case(name, dims, cyc, plain, seed):
    C = mh.constants(dims, plain)
    F = mh.inputs(dims, cyc, plain, C, seed)
    wrk = tempfile.mkdtemp(prefix="heat_")
    try:
        mh.build(wrk, dims, cyc)
        res = mh.run(wrk, dims, C, F)
    finally:
        shutil.rmtree(wrk, ignore_errors=True)
    mh.check_branches(name, dims, cyc, C, F, res)
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    out = dict(c_dims=np.array(dims, dtype=np.int64), c_cyclic=np.int64(cyc), c_K=np.int64(mh.K), c_nstr=np.int64(mh.NSTR),
               c_nx1=np.int64(1 + (nxta - nxaooc) // 2), c_ny1=np.int64(1 + (nyta - nyaooc) // 2),
               c_fnot=np.float64(float(mh.FNOT.replace("D", "e"))))
    out.update({"c_" + k: np.float64(v) for k, v in C.items()})
    out.update({"in_" + k: np.asfortranarray(v) for k, v in F.items()})
    out.update(res)
    assert mh.packed_size(out) < LIMIT, (name, mh.packed_size(out))
    return {name: out}


if __name__ == "__main__":
    only = sys.argv[1:]
    assert all(n in [c[0] for c in XF_CASES + HEAT_CASES] for n in only), only
    files = {}
    for name, dims, cyc, nstates in XF_CASES:
        if not only or name in only:
            files.update(xf_case(name, dims, cyc, nstates))
    for ic, (name, dims, cyc, plain) in enumerate(HEAT_CASES):
        if not only or name in only:
            files.update(heat_case(name, dims, cyc, plain, 400 + ic))
    for fn, d in files.items():
        path = os.path.join(HERE, "%s.npz" % fn)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < LIMIT, (fn, size)
        sys.stderr.write("wrote %s.npz (%d bytes, %s states)\n" % (fn, size, d.get("c_nstates", "-")))
