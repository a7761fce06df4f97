"""The ocean monitors (qgcm_hip_monitors) without a GPU: the library exports the new entry points,
the Python wrappers and the packed layout agree with include/qgcm_hip.h, the kernels do not spill, and the numpy
restatement tests/numpy_monitors.py holds the properties the Fortran guarantees."""
import ctypes
import os
import re

import numpy as np
import pytest

import numpy_monitors as nm
from qgcm_hip import lib, model, oml_preset, preset, synth

NEW = ["qgcm_hip_monitor_len", "qgcm_hip_set_mon_params", "qgcm_hip_set_monitor_fields", "qgcm_hip_monitors"]


def test_library_exports_the_monitor_entry_points():
    path = lib.library_path()
    if not os.path.exists(path):
        pytest.fail("libqgcm_hip.so not built")
    L = ctypes.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in lib.SYMBOLS
    for name in ("set_monitor_params", "set_monitor_fields", "monitors", "monitor_vector"):
        assert callable(getattr(model.OceanModel, name))


def test_mon_params_struct_layout(repo_root):
    assert ctypes.sizeof(lib.MonParams) == 4 * 8 + 2 * 4
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    body = hdr[hdr.index("typedef struct qgcm_hip_mon_params {"):hdr.index("} qgcm_hip_mon_params;")]
    pos = [body.index(" %s" % f[0]) for f in lib.MonParams._fields_]
    assert pos == sorted(pos)


@pytest.mark.parametrize("nl", [2, 3, 5, 8])
def test_layout_length_and_order(repo_root, nl):
    n = sum({0: 1, -1: nl - 1, 1: nl}[k] for _, k in model.MONITOR_LAYOUT)
    assert n == 19 * nl + 16
    d = model.unpack_monitors(np.arange(n, dtype=np.float64), nl)
    assert d["wetmoc"] == 0.0 and d["cnqgoc"][-1] == n - 1
    # the header lists the names in the same order
    hdr = open(os.path.join(repo_root, "include", "qgcm_hip.h")).read()
    blk = hdr[hdr.index("qgcm_hip_monitors: out, in this order"):hdr.index("typedef struct qgcm_hip_mon_params")]
    names = [w for w in re.findall(r"\b([a-z][a-z0-9]+)\b", blk) if w in d]
    assert names == [nme for nme, _ in model.MONITOR_LAYOUT]


def test_monitor_kernels_do_not_spill(repo_root):
    """As tests/test_abi.py reads the build's resource report: every instantiation of k_mon_scan / k_mon_final (the
    nlo = 3 ones are those of NAtl and SOcn 5 km) uses no scratch."""
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
    for h in ("_Z10k_mon_scanILi3ELb0EE", "_Z10k_mon_scanILi3ELb1EE", "_Z11k_mon_finalILi3EE", "_Z9k_mon_jet"):
        hits = [k for k in res if k.startswith(h)]
        assert hits, "kernel %s not in the report" % h
        for k in hits:
            assert res[k] == 0, "%s spills %d B per lane" % (k, res[k])
    assert sum(1 for k in res if "k_mon_" in k) == 3 * 7 + 1   # nlo = 2 .. 8: box + cyclic scan, final; k_mon_jet


def _jet_chunk(repo_root):
    src = open(os.path.join(repo_root, "q-gcm_amd", "csrc", "k_monitors.h")).read()
    return int(re.search(r"#define MON_JET_CHUNK (\d+)", src).group(1))


def _chunked_jet_sum(u, chunk):
    """k_mon_jet's arithmetic on one row of ugeos: the row passes through a buffer of `chunk` values; one lane keeps
    its running sum across the passes, adding the values of each in order, and remembers the last value of the last
    pass, which it subtracts at the end."""
    ujet, last = np.float64(0.0), np.float64(0.0)
    for c0 in range(0, len(u), chunk):
        buf = u[c0:c0 + chunk].copy()
        for x in buf:
            ujet = ujet + x
        last = buf[-1]
    return ujet - last


@pytest.mark.parametrize("nxpo", [8191, 8192, 8193, 11521, 23041])
def test_chunked_jet_sum_is_the_row_sum(repo_root, nxpo):
    """Rows longer than MON_JET_CHUNK pass through k_mon_jet's LDS in chunks.  The running sum carried across the
    chunk boundaries is bitwise numpy_monitors' row sum (np.cumsum: serial over i, then - u(nxpo)), because the order of
    the additions is the same; sums per chunk added afterwards are not - the fix rests on the order."""
    chunk = _jet_chunk(repo_root)
    assert chunk == 8192 and chunk * 8 <= 65536 and chunk >= 5105  # every row the 5 km basins have is one pass
    rng = np.random.default_rng(nxpo)
    po = rng.uniform(-1.0, 1.0, (nxpo, 2, 1)) * 10.0 ** rng.uniform(-3.0, 3.0, (nxpo, 1, 1))
    rdxof0 = 1.0 / (5.0e3 * -1.19467e-04)
    ugeos = -rdxof0 * (po[:, 1:, 0] - po[:, :-1, 0])
    want = np.cumsum(ugeos, axis=0)[-1, :] - ugeos[-1, :]  # numpy_monitors.monitors, ujeto before abs and / nxt
    got = _chunked_jet_sum(ugeos[:, 0], chunk)
    assert got.tobytes() == want[0].tobytes()
    npass = -(-nxpo // chunk)
    assert npass == {8191: 1, 8192: 1, 8193: 2, 11521: 2, 23041: 3}[nxpo]
    if nxpo > chunk + 1:  # (8193: the second chunk is one value, both orders are the same additions)
        parts = [np.cumsum(ugeos[c0:c0 + chunk, 0])[-1] for c0 in range(0, nxpo, chunk)]
        tree = parts[0]
        for p in parts[1:]:
            tree = tree + p
        assert (tree - ugeos[-1, 0]) != want[0]  # another order of the same terms: not the reference's bits
        # ... and the columns past the first chunk matter
        assert (np.cumsum(ugeos[:chunk, 0])[-1] - ugeos[chunk - 1, 0]) != want[0]


def _loop_lap(a, dxm2, cyc):
    """Del-sqd of del4bx / del4ch point by point, as the Fortran writes it (1-based indices shifted by one)."""
    nx, ny = a.shape
    d = np.zeros_like(a)
    for j in range(ny):
        for i in range(nx):
            if 0 < j < ny - 1 and (cyc or 0 < i < nx - 1):
                im, ip = (i - 1) % nx, (i + 1) % nx
                d[i, j] = dxm2 * (a[i, j - 1] + a[im, j] + a[ip, j] + a[i, j + 1] - 4.0 * a[i, j])
                continue
            if not cyc and i == 0:
                s = a[2, j] - 2.0 * a[1, j] + a[0, j]
            elif not cyc and i == nx - 1:
                s = a[i, j] - 2.0 * a[i - 1, j] + a[i - 2, j]
            else:
                s = a[(i - 1) % nx, j] - 2.0 * a[i, j] + a[(i + 1) % nx, j]
            if j == 0:
                s = s + a[i, 2] - 2.0 * a[i, 1] + a[i, 0]
            elif j == ny - 1:
                s = s + a[i, j] - 2.0 * a[i, j - 1] + a[i, j - 2]
            else:
                s = s + a[i, j - 1] - 2.0 * a[i, j] + a[i, j + 1]
            d[i, j] = dxm2 * s
    return d


@pytest.mark.parametrize("cyc", [False, True])
def test_restated_del4_is_the_fortran_loops(cyc):
    a = np.random.default_rng(3).uniform(-1.0, 1.0, (9, 7))
    d2, d4 = nm.del4(a, 0.25, cyc)
    assert np.array_equal(d2, _loop_lap(a, 0.25, cyc))
    assert np.array_equal(d4, _loop_lap(_loop_lap(a, 0.25, cyc), 0.25, cyc))


def test_restated_del4_of_quadratics():
    """One-sided and centred second differences are exact for quadratics: Del-sqd of x^2 + y^2 is 4 everywhere, so
    Del-4th vanishes, on every edge and corner of the box form."""
    x, y = np.meshgrid(np.arange(8.0), np.arange(6.0), indexing="ij")
    d2, d4 = nm.del4(x * x + y * y, 1.0, False)
    assert np.array_equal(d2, np.full_like(d2, 4.0)) and not d4.any()


def test_restated_genint_weights():
    v = np.ones((5, 4))
    assert nm.genint(v, 0.5, 0.5) == 3 * 2 + 0.5 * (2 * 2 + 2 * 3) + 0.25 * 4
    assert nm.genint(v, 1.0, 1.0) == 20.0


def _case(cfgname):
    cfg = preset(cfgname)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    pom = 0.999 * po
    om = synth.mixed_layer_fields(cfg, oml_preset(cfg), seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, om[3], om[4])
    f = dict(po=po, pom=pom, qo=1e-6 * po, wekpo=wekpo, entoc=1e-6 * po[:, :, 0], tauxo=om[3], tauyo=om[4],
             wekto=wekto, sst=om[0])
    c = dict(cyclic=cfg.cyclic, fnot=cfg.fnot, dxo=cfg.dxo, dto=cfg.dto, gpoc=cfg.gpoc[:cfg.nlo - 1], hoc=cfg.hoc,
             ah2oc=cfg.ah2oc, ah4oc=cfg.ah4oc, delek=cfg.delek, rhooc=1.0e3, cpoc=4.0e3, hmoc=100.0, ycexp=1.0,
             sb_hflux=False, nb_hflux=False)
    return cfg, f, c


@pytest.mark.parametrize("cfgname", ["box_tiny", "cyc_tiny"])
def test_restatement_properties(cfgname):
    cfg, f, c = _case(cfgname)
    v, s = nm.monitors(f, c)
    assert set(v) == set(dict(model.MONITOR_LAYOUT))
    assert v["sstmin"] == f["sst"].min() and v["sstmax"] == f["sst"].max()
    assert np.all(v["kealoc"] > 0.0) and v["btdgoc"] > 0.0 and np.all(v["et2moc"] > 0.0)
    assert v["watmoc"] >= abs(v["wetmoc"]) and v["occtot"] == pytest.approx(v["occirc"].sum())
    for n in v:
        assert np.all(np.asarray(s[n]) >= np.abs(v[n]) * (1 - 1e-12)), n


@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny", "box_tiny5", "box_tiny2", "cyc_tiny6"])
def test_restatement_reproduces_the_reference(name):
    """tests/golden/mon_<name>.npz holds the reference's own monnc_comp / couroc (make_golden_monnc.py): the restatement
    gives its extrema, jet position and value, transports and Courant numbers bitwise, and every integral to 1e-13 of
    the integral of the modulus of its integrand."""
    from test_gpu_monitors import EXACT, golden_case
    cfg, f, c, want = golden_case(name)
    v, s = nm.monitors(f, c)
    assert set(v) == set(want)
    assert want["pkenoc"] != 0.0 and np.all(want["ddtkeoc"] != 0.0) and np.all(want["ocjpos"] > 0)
    for n in want:
        got, ref, sc = np.atleast_1d(v[n]), np.atleast_1d(want[n]), np.atleast_1d(s[n])
        if n in EXACT:
            assert np.array_equal(got, ref), n
        else:
            assert np.all(np.abs(got - ref) <= 1e-13 * sc), (n, got, ref)
