"""The numpy restatement of xforc's momentum half (tests/numpy_xforc.py) against the reference's own results
(tests/golden/xf_*.npz, written by tests/golden/make_golden_xforc.py): IEEE operations in the reference's order
reproduce every field and every line integral bit for bit, and hostinit.bcuini reproduces the weight tables."""
import numpy as np
import pytest

import numpy_xforc as nx
from qgcm_hip import hostinit


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("case", nx.CASES)
def test_restatement_is_bitwise(case):
    g = nx.load(case)
    for s in range(2):
        R = nx.restated(case, s)
        for f in nx.POINTWISE + nx.INTEGRALS:
            ref = g["out%d_%s" % (s, f)]
            assert np.shape(R[f]) == ref.shape, (f, np.shape(R[f]), ref.shape)
            assert np.all(np.isfinite(ref)), f
            assert np.array_equal(_bits(R[f]), _bits(ref)), "%s state %d %s: max |diff| %.3e" % (
                case, s, f, np.max(np.abs(np.asarray(R[f]) - ref)))


def test_fixtures_exercise_their_branches():
    tiny, ud = nx.load("xf_cpl_tiny"), nx.load("xf_cpl_tiny_ud")
    assert not np.array_equal(tiny["out0_tauxo"], ud["out0_tauxo"])  # the shear term
    assert np.array_equal(tiny["in0_pam1"], ud["in0_pam1"])
    cyc = nx.load("xf_cyc4_ud")
    assert int(cyc["c_cyclic"]) == 1 and int(cyc["c_nx1"]) == 1 and float(cyc["out0_txisoc"]) != 0.0
    assert int(nx.load("xf_odd5_ud")["c_dims"][4]) % 2 == 1
    for case in nx.CASES:
        g = nx.load(case)
        for s in range(2):
            assert np.abs(g["out%d_wekpa" % s]).max() > 0 and np.abs(g["out%d_wekpo" % s]).max() > 0
    # The launch geometry of qgcm_hip_xforc (k_xforc.h), from the fixtures' dimensions alone: 256 threads along a row
    # of nxpa, nxta, nxpo or nxto points, 64 along nxpa in k_xf_wekpa, XF_CX = 8 cells per workgroup of k_xf_fine, one
    # workgroup striding by 256 in k_xf_lines.  Each line is one path that some fixture must reach.
    P = [nx.params(nx.load(c)) for c in nx.CASES]
    for p in P:
        p.update(nxpa=p["nxta"] + 1, nxto=p["nxaooc"] * p["ndxr"], nxpo=p["nxaooc"] * p["ndxr"] + 1)
    blocks = lambda n, w: -(-n // w)
    # k_xf_coarse, k_xf_atm: a second block along nxpa; k_xf_wekta: along nxta
    assert any(blocks(p["nxpa"], 256) >= 2 for p in P) and any(blocks(p["nxta"], 256) >= 2 for p in P)
    # ... and a second block that holds the copy column ia = nxpa alone
    assert any(p["nxpa"] % 256 == 1 and p["nxpo"] % 256 == 1 for p in P)
    # k_xf_wekpa: more than two blocks of 64, the cyclic wrap of `it` reached from the first and from the last
    assert any(blocks(p["nxpa"], 64) >= 3 for p in P)
    # k_xf_fine: a tail workgroup of fewer than 8 cells (it holds column nxta, whose icp2 wraps), with a full one before
    assert any(p["nxta"] % 8 != 0 and p["nxta"] > 8 for p in P)
    # k_xf_tauo, k_wekto, k_wekpo: a second block along the ocean's rows, for a box and for a cyclic ocean
    assert any(blocks(p["nxpo"], 256) >= 2 and blocks(p["nxto"], 256) >= 2 and not p["cyclic"] for p in P)
    assert any(blocks(p["nxpo"], 256) >= 2 and blocks(p["nxto"], 256) >= 2 and p["cyclic"] for p in P)
    # k_xf_lines: a second round of the cyclic ocean's loop (the atmosphere's loop over nxpaor takes several in every case)
    assert any(p["cyclic"] and p["nxpo"] > 256 for p in P)
    assert all(float(nx.load(c)["out0_txisoc"]) != 0.0 and float(nx.load(c)["out0_txinoc"]) != 0.0
               for c, p in zip(nx.CASES, P) if p["cyclic"])


# hostinit.bcuini against the tables the reference built.  Bitwise for ndxr = 4, 12 and 16.  At ndxr = 5 the reference
# binary differs from its own run-time arithmetic: the compiler unrolls the short loops of bcuini and folds ss**i at
# compile time with one rounding, where the running code multiplies.  Measured: at most 2**-52 (2.2e-16) absolute on
# entries of magnitude <= 1; the bound is twice that.
@pytest.mark.parametrize("case", nx.CASES)
def test_bcuini(case):
    g = nx.load(case)
    P = nx.params(g)
    T = hostinit.bcuini(P["ndxr"], P["bccoat"], P["ndxr"] * P["dxo"])
    for t in nx.TABLES:
        ref = g["tab_" + t]
        assert T[t].shape == ref.shape
        if P["ndxr"] == 5:
            d = np.max(np.abs(T[t] - ref))
            print("%s %s: max |diff| %.3e" % (case, t, d))
            assert d <= 2.0 * 2.0 ** -52
        else:
            assert np.array_equal(_bits(np.asfortranarray(T[t]).ravel(order="F")), _bits(ref.ravel(order="F"))), t
        # auvbcu's northern cells read row jj = ndxr, which bcuini never fills
        assert not T[t][:, :, P["ndxr"]].any() and not T[t][:, P["ndxr"], :].any()
