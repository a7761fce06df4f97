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
