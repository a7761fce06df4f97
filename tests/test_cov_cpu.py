"""CPU checks of the covariance diagnostics: the numpy restatement against the reference's goldens, the
row-sum form against psampl / tsampl for many slab splits, the split of the matrix rows across ranks, and the
triangular-number inversion of k_cov_rank1."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "q-gcm_amd", "python"))
sys.path.insert(0, os.path.dirname(__file__))

import numpy_cov as nc  # noqa: E402
from qgcm_hip.model import cov_row_split  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "cov_*.npz")) + glob.glob(os.path.join(GOLD, "acov_*.npz")))


def test_golden_files_present():
    names = {os.path.basename(f) for f in FILES}
    for n in ("cov_box_tiny_3", "cov_box_tiny_4", "cov_cyc_tiny_4", "cov_box_small_16", "cov_box_small_8",
              "acov_cpl_tiny_2", "acov_cpl_small_2"):
        assert n + ".npz" in names
    for f in FILES:
        assert os.path.getsize(f) < 1 << 20


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_numpy_reproduces_golden(path):
    g = np.load(path)
    nsi = int(g["c_nsi"])
    nxt, nyt = g["in0_t"].shape
    nvar = (nxt // nsi) * (nyt // nsi)
    ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
    n = 0
    while "in%d_p1" % n in g.files:
        nc.covocn(g["in%d_p1" % n], g["in%d_t" % n], nsi, ap, at)
        n += 1
    assert n >= 4
    assert ap.nu == int(g["out_nu_p"]) == n and at.nu == int(g["out_nu_t"]) == n
    assert ap.swt == g["out_swt_p"] and at.swt == g["out_swt_t"]
    np.testing.assert_array_equal(ap.mean, g["out_avg_p"])
    np.testing.assert_array_equal(at.mean, g["out_avg_t"])
    np.testing.assert_array_equal(ap.cov, g["out_cov_p"])
    np.testing.assert_array_equal(at.cov, g["out_cov_t"])
    assert np.count_nonzero(ap.cov) > ap.nmat // 2  # (the update did something)


def _fields(nx, ny, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nx + 1, ny + 1)), rng.standard_normal((nx, ny))


def _split(nyp, cuts):
    """1-based p rows of each rank and its T rows (the last rank has one T row fewer than p rows)."""
    b = [0] + list(cuts) + [nyp]
    out = []
    for r in range(len(b) - 1):
        p0, p1 = b[r] + 1, b[r + 1]
        out.append((p0, p1, p0, p1 - 1 if p1 == nyp else p1))
    return out


@pytest.mark.parametrize("nx,ny,nsi", [(48, 36, 4), (48, 36, 3), (96, 80, 16), (64, 32, 2)])
@pytest.mark.parametrize("cuts", ["1", "2", "3", "8", "inside"])
def test_rowsum_form_reproduces_psampl_tsampl(nx, ny, nsi, cuts):
    p, t = _fields(nx, ny, nx + ny + nsi)
    nyp = ny + 1
    if cuts == "inside":  # cuts that fall inside blocks, next to block edges and one row from the ends
        c = sorted({1, nsi - 1, nsi + 1, 2 * nsi + nsi // 2, nyp - 2})
    else:
        P = int(cuts)
        c = [round(nyp * r / P) for r in range(1, P)]
    parts = [nc.part(p, t, nsi, *s, part_len=4 + (nyp + ny) * (nx // nsi)) for s in _split(nyp, c)]
    up, ut = nc.combine(parts, nsi, nx // nsi, nyp, ny)
    np.testing.assert_array_equal(up, nc.psampl(p, nsi))
    np.testing.assert_array_equal(ut, nc.tsampl(t, nsi))


def test_combine_refuses_parts_that_do_not_tile():
    p, t = _fields(16, 12, 1)
    good = [nc.part(p, t, 2, *s) for s in _split(13, [6])]
    nc.combine(good, 2, 8, 13, 12)
    with pytest.raises(ValueError):
        nc.combine(good[::-1], 2, 8, 13, 12)
    with pytest.raises(ValueError):
        nc.combine(good[:1], 2, 8, 13, 12)


@pytest.mark.parametrize("nvar", [1, 2, 3, 30, 3600, 10368, 73728, 90000])
@pytest.mark.parametrize("nranks", [1, 2, 3, 7, 8])
def test_matrix_row_split_tiles_and_balances(nvar, nranks):
    nmat = nvar * (nvar + 1) // 2
    rows = [cov_row_split(nvar, r, nranks) for r in range(nranks + 1)]
    assert rows[0] == 0 and rows[-1] == nvar
    assert all(a <= b for a, b in zip(rows, rows[1:]))
    ks = [i * (i + 1) // 2 for i in rows]
    assert ks[0] == 0 and ks[-1] == nmat
    # each share is its 1/nranks of the elements to within one matrix row
    for r in range(nranks):
        assert abs((ks[r + 1] - ks[r]) - nmat / nranks) <= 2 * nvar


def test_ranged_update_equals_whole():
    rng = np.random.default_rng(7)
    nvar = 50
    whole = nc.Dssp(nvar)
    shares = [nc.Dssp(nvar, *(i * (i + 1) // 2 for i in (cov_row_split(nvar, r, 3), cov_row_split(nvar, r + 1, 3))))
              for r in range(3)]
    for _ in range(4):
        x = rng.standard_normal(nvar)
        whole.add(x)
        for s in shares:
            s.add(x)
    np.testing.assert_array_equal(np.concatenate([s.cov for s in shares]), whole.cov)


def test_triangular_inversion_exact_near_2_31_and_2_32():
    import math
    for base in (2 ** 31, 2 ** 32, 4050045000, 2717945856):
        for k in list(range(base - 3000, base + 3000)) + [base * 3 - 1]:
            i, j = nc.rowcol(k)
            assert 0 <= j <= i and i * (i + 1) // 2 + j == k
            assert i == (math.isqrt(8 * k + 1) - 1) // 2
    # the first and last entries of every row around the 32-bit boundary
    i0 = (math.isqrt(8 * 2 ** 32 + 1) - 1) // 2
    for i in range(i0 - 20, i0 + 20):
        k = i * (i + 1) // 2
        assert nc.rowcol(k) == (i, 0) and nc.rowcol(k + i) == (i, i)
