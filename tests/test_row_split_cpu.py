"""CPU checks of the split of cyclic rows longer than one row transform (k_row_split.h): the plan function
qgcm_hip_row_split (pure host code of the library, no device), and the algebra of the split - a numpy restatement of the
two formulas the kernels implement, wrapped around the oracle's FFTPACK-equivalent sub-transforms and compared against
the oracle's direct transform."""
import os

import numpy as np
import pytest

import oracle_binding as ob
from qgcm_hip import QgcmHipError, config, lib

# nxto = nxaooc * ndxr of the ten parameter files the reference ships under src/ (parameters_data.F and
# parameters_data.F.{NAtl.{5,4,2,1}km, SOcn.{5,4,3,2,1}km.wideatm}) and the plan DESIGN 3.5c documents for each
REFERENCE_ROWS = {"default": (960, 1, 960), "NAtl.5km": (960, 1, 960), "NAtl.4km": (1200, 1, 1200), "NAtl.2km": (2400, 1, 2400),
                  "NAtl.1km": (4800, 1, 4800), "SOcn.5km": (4608, 1, 4608), "SOcn.4km": (5760, 2, 2880),
                  "SOcn.3km": (7680, 2, 3840), "SOcn.2km": (11520, 3, 3840), "SOcn.1km": (23040, 5, 4608)}


def test_plan_of_every_reference_row_length():
    for name, (nxto, P, L) in REFERENCE_ROWS.items():
        assert lib.row_split(nxto) == (P, L), name
        assert P * L == nxto and L <= lib.ROW_MAX and (P == 1 or L % 2 == 0)


def test_plan_boundaries_and_forced_values():
    assert lib.row_split(5104) == (1, 5104)      # the longest row one transform holds
    assert lib.row_split(5106) == (3, 1702)      # 5106 / 2 = 2553 is odd: the next P
    assert lib.row_split(48, 2) == (2, 24) and lib.row_split(48, 3) == (3, 16) and lib.row_split(48, 4) == (4, 12)
    assert lib.row_split(96, 2) == (2, 48) and lib.row_split(96, 4) == (4, 24)
    assert lib.row_split(160, 5) == (5, 32)
    assert lib.row_split(48) == (1, 48) and lib.row_split(96, 0) == (1, 96)
    for nxto in range(5106, 5 * 5104 + 1, 1234):  # whatever the rule gives holds its conditions
        try:
            P, L = lib.row_split(nxto)
        except QgcmHipError:
            continue
        assert 2 <= P <= lib.ROW_SPLIT_MAX_P and P * L == nxto and L % 2 == 0 and L <= lib.ROW_MAX, nxto
        assert not any(nxto % p == 0 and (nxto // p) % 2 == 0 and nxto // p <= 2560 for p in range(2, P)), nxto  # (<= 2560: two buffers fit)


def test_plan_refusals_name_the_limit():
    with pytest.raises(QgcmHipError, match="nxto=5105 is longer than one row transform.*no P in 2 .. 5"):
        lib.row_split(5105)                      # odd: no P leaves an even L
    with pytest.raises(QgcmHipError, match="no P in 2 .. 5"):
        lib.row_split(5 * 5104 + 10)             # even the largest P leaves more than 5104 points
    with pytest.raises(QgcmHipError, match="QGCM_HIP_ROW_SPLIT=5 does not divide nxto=48"):
        lib.row_split(48, 5)
    with pytest.raises(QgcmHipError, match="QGCM_HIP_ROW_SPLIT=2 leaves sub-rows of an odd length 27"):
        lib.row_split(54, 2)
    with pytest.raises(QgcmHipError, match="QGCM_HIP_ROW_SPLIT=2 leaves sub-rows of 11520 points"):
        lib.row_split(23040, 2)
    for bad in (1, 6, 7):
        with pytest.raises(QgcmHipError, match="outside 2 .. 5"):
            lib.row_split(48, bad)
    with pytest.raises(QgcmHipError, match="nxto = 1"):
        lib.row_split(1)


# ---- the algebra: FFTPACK's half-complex order r(1) = X_0, r(2k) = Re X_k, r(2k+1) = Im X_k, r(n) = X_{n/2} ----------
def hc_to_complex(r):
    n = len(r)
    X = np.zeros(n // 2 + 1, dtype=complex)
    X[0], X[n // 2] = r[0], r[n - 1]
    X[1:n // 2] = r[1:n - 1:2] + 1j * r[2:n - 1:2]
    return X


def complex_to_hc(X, n):
    r = np.zeros(n)
    r[0], r[n - 1] = X[0].real, X[n // 2].real
    r[1:n - 1:2], r[2:n - 1:2] = X[1:n // 2].real, X[1:n // 2].imag
    return r


def split_forward(x, P):
    """X[k] = sum_p W_N^{p k} Y_p[k mod L], Y_p = rfft_L(x[p::P]); Y_p[j] = conj(Y_p[L - j]) beyond L/2."""
    N = len(x)
    L = N // P
    k = np.arange(N // 2 + 1)
    k0 = k % L
    X = np.zeros(N // 2 + 1, dtype=complex)
    for p in range(P):
        Y = hc_to_complex(ob.rfftf(x[p::P]))
        Yk = np.where(k0 > L // 2, np.conj(Y[np.where(k0 > L // 2, L - k0, k0)]), Y[np.minimum(k0, L // 2)])
        X += np.exp(-2j * np.pi * ((p * k) % N) / N) * Yk
    return complex_to_hc(X, N)


def split_inverse(r, P):
    """Y_p[k] = sum_q W_N^{-p (k + L q)} X[k + L q], X beyond N/2 by Hermitian symmetry; x[p::P] = rfftb_L(Y_p)."""
    N = len(r)
    L = N // P
    X = hc_to_complex(r)
    k = np.arange(L // 2 + 1)
    x = np.zeros(N)
    for p in range(P):
        Y = np.zeros(L // 2 + 1, dtype=complex)
        for q in range(P):
            j = k + L * q
            Xj = np.where(j > N // 2, np.conj(X[np.where(j > N // 2, N - j, j)]), X[np.minimum(j, N // 2)])
            Y += np.exp(2j * np.pi * ((p * j) % N) / N) * Xj
        x[p::P] = ob.rfftb(complex_to_hc(Y, L))
    return x


@pytest.mark.parametrize("N,P", [(5760, 2), (7680, 2), (11520, 3), (23040, 5), (48, 2), (48, 3), (96, 4), (160, 5)])
def test_split_algebra_against_the_direct_transform(N, P):
    """Both formulas against the oracle's direct drfftf / drfftb, relative to the largest coefficient.  The bar is the
    device test's TOLF = 5e-14 (test_row_transforms_against_fftpack_vectors); measured here: at most 2.2e-15."""
    x = np.random.default_rng(N + P).standard_normal(N)
    f = ob.rfftf(x)
    ef = np.abs(split_forward(x, P) - f).max() / np.abs(f).max()
    b = ob.rfftb(f)
    eb = np.abs(split_inverse(f, P) - b).max() / np.abs(b).max()
    print("N = %d = %d x %d: forward %.2e inverse %.2e" % (N, P, N // P, ef, eb))
    assert ef < 5e-14 and eb < 5e-14
    assert np.abs(b / N - x).max() < 1e-13  # (drfftb is the unnormalised inverse)


def test_presets_and_declarations():
    """The four presets carry the grid lines of the reference's parameter files; the header, the ctypes binding and the
    ISO_C_BINDING interface declare the two functions."""
    for name, key, nypo in (("socn4", "SOcn.4km", 721), ("socn3", "SOcn.3km", 961), ("socn2", "SOcn.2km", 1441), ("socn1", "SOcn.1km", 2881)):
        cfg = config.preset(name)
        assert (cfg.nxto, cfg.nypo, cfg.nlo, cfg.cyclic) == (REFERENCE_ROWS[key][0], nypo, 3, True), name
        assert cfg.nxaooc == cfg.nxta and cfg.fnot == config.preset("socn5").fnot
        assert lib.row_split(cfg.nxto)[1:] == REFERENCE_ROWS[key][2:]
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    hdr = open(os.path.join(root, "include", "qgcm_hip.h")).read()
    f90 = open(os.path.join(root, "q-gcm_amd", "fortran", "qgcm_hip_iface.F90")).read()
    for s in ("qgcm_hip_row_split", "qgcm_hip_row_plan"):
        assert s in lib.SYMBOLS and s + "(" in hdr and "name='%s'" % s in f90, s
        assert hasattr(lib.load_library(), s)
