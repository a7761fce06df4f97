"""xforc at refinements above 64 without a GPU: the fixtures of tests/golden/make_golden_wide_ndxr.py (ndxr =
75, 80, 128; the reference's own results) against the numpy restatements with hostinit.bcuini's tables, the table
checksums the generator recorded in place of the tables, the slab plans (lib.xforc_bands, lib.xforc_sums: host code of
the library) at ndxr = 75 and 80 against the brute-force restatements of the kernels' index expressions, and the launch
paths the GPU cases of tests/test_gpu_wide_ndxr.py must keep reaching."""
import dataclasses

import numpy as np
import pytest

import numpy_heat as nh
import numpy_xforc as nx
import numpy_xforc_sums as ns
from numpy_xforc_bands import FIELDS, HDR, LINES, needed_rows
from qgcm_hip import QgcmHipError, config, hostinit, lib
from qgcm_hip.slab import partition
from test_xforc_bands_cpu import _cell_rows, _seas, _slab_rows
from test_xforc_sums_cpu import _cuts

XF_CASES = ("xf_r80_ud", "xf_r75_ud", "xf_cyc80_ud", "xf_r128_ud", "xf_r128n3_ud")
# the cases a device handle can be made for: qgcm_hip_create takes no grid of fewer than four p rows (xf_r128_ud: nypa = 3)
GPU_CASES = tuple(c for c in XF_CASES if c != "xf_r128_ud")
HEAT_CASE = "heat_r80"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.all(np.isfinite(b)), what
    assert np.array_equal(_bits(a), _bits(b)), "%s: max |diff| %.3e, %d differ" % (
        what, np.max(np.abs(np.asarray(a) - b)), int((_bits(a) != _bits(b)).sum()))


_tables, _restated = {}, {}


def tables(case):
    """hostinit.bcuini's tables for a fixture (computed once, shared): the fixtures store none."""
    if case not in _tables:
        P = nx.params(nx.load(case))
        _tables[case] = hostinit.bcuini(P["ndxr"], P["bccoat"], P["ndxr"] * P["dxo"])
    return _tables[case]


def restated(case, s):
    """numpy_xforc.xforc of state s of a fixture with bcuini's tables (computed once, shared)."""
    if (case, s) not in _restated:
        g = nx.load(case)
        _restated[(case, s)] = nx.xforc(g["in%d_pam1" % s], g["in%d_pom1" % s], tables(case), nx.params(g))
    return _restated[(case, s)]


def nstates(case):
    return int(nx.load(case)["c_nstates"])


@pytest.mark.parametrize("case", XF_CASES)
def test_table_checksums(case):
    """The generator asserted the reference's five tables bitwise bcuini's and recorded per table the sum of the int64
    views modulo 2^64: bcuini here gives the same sums, and fills neither row nor column ndxr."""
    g = nx.load(case)
    n = nx.params(g)["ndxr"]
    for t in nx.TABLES:
        T = tables(case)[t]
        assert T.shape == (16, n + 1, n + 1) and np.all(np.isfinite(T))
        with np.errstate(over="ignore"):
            assert _bits(T).sum(dtype=np.int64) == np.int64(g["tabsum_" + t]), (case, t)
        assert not T[:, :, n].any() and not T[:, n, :].any()
        assert "tab_" + t not in g


@pytest.mark.parametrize("case", XF_CASES)
def test_restatement_is_bitwise(case):
    g = nx.load(case)
    for s in range(nstates(case)):
        R = restated(case, s)
        for f in nx.POINTWISE + nx.INTEGRALS:
            _same(R[f], g["out%d_%s" % (s, f)], "%s state %d %s" % (case, s, f))
        assert np.abs(g["out%d_wekpa" % s]).max() > 0 and np.abs(g["out%d_wekpo" % s]).max() > 0


def test_heat_restatement_is_bitwise():
    """heat_r80 at the bars of tests/test_heat_cpu.py: every field and every serially summed scalar of the K cycles of
    [xforc; 3 x aml] bit for bit, asto from the package's own coordinates, fsprim to 1 ulp."""
    g = nh.load(HEAT_CASE)
    P = nh.params(g)
    R = nh.restated(HEAT_CASE)
    for c in range(P["K"]):
        H = R[("x", c)]
        for f in ("fnetoc", "fnetat") + nh.HEAT_SCALARS:
            _same(H[f], g["x%d_%s" % (c, f)], "xforc %d %s" % (c, f))
        for s in range(P["nstr"]):
            A = R[("a", c, s)]
            for f in nh.AML_FIELDS + nh.AML_SUMS + ("cfraat",):
                _same(A[f], g["a%d%d_%s" % (c, s, f)], "aml %d.%d %s" % (c, s, f))
    _same(R[("x", 0)]["asto"], g["t_asto"], "asto")
    oc = dataclasses.replace(config.preset("cpl_tiny"), nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"],
                             nyaooc=P["nyaooc"], ndxr=P["ndxr"], dxo=P["dxo"])
    G = hostinit.grid_coordinates(config.atmos_of(oc), oc)
    for k in ("xta", "yta", "xto", "yto"):
        _same(G[k], g["t_" + k], k)
    T = hostinit.bilint_tables(G["xta"], G["yta"], G["xto"], G["yto"], P["dxa"], P["dya"])
    _same(nh.bilint(T, g["in_astm"]), g["t_asto"], "asto from the package's coordinates")
    for tab, yrel in (("fsa", G["ytarel"]), ("fso", G["ytorel"])):
        mine, ref = hostinit.fsprim(yrel, P["fspco"], G["yla"]), g["t_" + tab]
        assert np.all(np.abs(mine - ref) <= np.spacing(np.abs(ref))), tab


def test_band_plan_against_brute_force():
    """tests/test_xforc_bands_cpu.py's loop at ndxr = 75 and 80 on 1 to 5 ranks: the windows cover every fine p row and
    T row the kernels' index expressions touch, are no wider than whole cell rows, the bands tile 1 .. nypa, every line
    sum has one owner."""
    NXPA, count = 17, 0
    for nyta in (2, 3, 6):
        nypa = nyta + 1
        for ndxr in (75, 80):
            for nranks in range(1, 6):
                for ny1, nyaooc in _seas(nyta):
                    nyg = nyaooc * ndxr + 1
                    tag = "nyta %d ndxr %d nranks %d ny1 %d nyaooc %d" % (nyta, ndxr, nranks, ny1, nyaooc)
                    if nranks > nypa:
                        with pytest.raises(QgcmHipError, match="every rank needs a band"):
                            lib.xforc_bands(NXPA, nyta, ndxr, ny1, nyaooc, [(1, nyg)] * nranks)
                        continue
                    slabs = _slab_rows(nyg, nranks)
                    plan = lib.xforc_bands(NXPA, nyta, ndxr, ny1, nyaooc, partition(nyg, nranks))
                    assert len(plan) == nranks and plan[0]["band"][0] == 1 and plan[-1]["band"][1] == nypa, tag
                    for p, q in zip(plan, plan[1:]):
                        assert q["band"][0] == p["band"][1] + 1, tag
                    nrow = max(p["band"][1] - p["band"][0] + 1 for p in plan)
                    for f in LINES:
                        assert sum(f in p["own"] for p in plan) == 1, (tag, f)
                    for r, p in enumerate(plan):
                        need_p, need_t = needed_rows(nyta, ndxr, ny1, nyg, p["band"], slabs[r], p["own"])
                        win = set()
                        for (c0, c1), (f0, f1) in zip(p["cells"], p["fine"]):
                            rows = set().union(*[_cell_rows(c, ndxr, nyta) for c in range(c0, c1 + 1)])
                            assert rows == set(range(f0, f1 + 1)), (tag, r)
                            for c in range(c0, c1 + 1):
                                assert _cell_rows(c, ndxr, nyta) & need_p, (tag, r, c)
                            assert not (win & rows), (tag, r)
                            win |= rows
                        assert 1 <= len(p["cells"]) <= 2 and 1 <= min(win) and max(win) <= nyta * ndxr + 1, (tag, r)
                        assert need_p <= win, (tag, r, sorted(need_p - win))
                        assert set(range(p["trows"][0], p["trows"][1] + 1)) == need_t, (tag, r, p["trows"])
                        assert p["nrow"] == nrow and p["mom_len"] == HDR + len(FIELDS) * nrow * NXPA, (tag, r)
                        count += 1
    assert count > 100


def test_sums_plan_against_brute_force():
    """tests/test_xforc_sums_cpu.py's loop at ndxr = 75 and 80 on 1 to 5 ranks, even and uneven cuts: the ownership tiles
    1 .. nypaor, every row a kernel of the rank reads lies in its window / its owned T rows, [a0, a1] is exactly the
    coarse rows it contributes to, the line sums have one owner each; a refusal is a shared pair of line rows."""
    NXPA, seen = 9, 0
    for ndxr in (75, 80):
        for nyta, ny1, nyaooc in ((8, 1, 3), (8, 3, 3), (8, 6, 3), (6, 1, 6), (9, 2, 5)):
            D = ns.dims(nyta, ndxr, ny1, nyaooc)
            cell = lambda f: min((f - 1) // ndxr + 1, nyta)  # noqa: E731
            for nranks in range(1, 6):
                for rows in _cuts(D["nyg"], nranks):
                    Pown, Town = ns.owner_rows(D, rows)
                    try:
                        plan = lib.xforc_sums(NXPA, nyta, ndxr, ny1, nyaooc, rows)
                    except QgcmHipError as e:
                        assert "would share" in str(e) and D["odd"]
                        assert Pown[D["jsou"]] != Pown[D["jsou"] + 1] or Pown[D["jnor"]] != Pown[D["jnor"] - 1], (rows, str(e))
                        continue
                    if D["odd"]:
                        assert Pown[D["jsou"]] == Pown[D["jsou"] + 1] and Pown[D["jnor"]] == Pown[D["jnor"] - 1]
                    seen += 1
                    tag = (ndxr, nyta, ny1, nyaooc, rows)
                    assert plan[0]["fine"][0] == 1 and plan[-1]["fine"][1] == D["nypaor"], tag
                    owners = []
                    for r, p in enumerate(plan):
                        f0, f1 = p["fine"]
                        assert list(np.nonzero(Pown[1:] == r)[0] + 1) == list(range(f0, f1 + 1)), tag
                        assert list(np.nonzero(Town[1:] == r)[0] + 1) == list(range(p["trows"][0], p["trows"][1] + 1)), tag
                        R = ns.reads(D, rows, r)
                        w0, w1 = p["window"]
                        assert (min(R["P"]), max(R["P"])) == (w0, w1) == (max(1, f0 - 3), min(D["nypaor"], f1 + 3)), (tag, r)
                        assert R["T"] == set(range(p["trows"][0], p["trows"][1] + 1)), tag
                        c0, c1 = p["cells"]
                        assert (c0, c1) == (cell(min(R["P"])), cell(max(R["P"]))), (tag, r)
                        assert p["coarse"] == (max(1, c0 - 1), min(D["nypa"], c1 + 2)), tag
                        assert R["A"] == set(range(p["arows"][0], p["arows"][1] + 1)), (tag, r)
                        assert sorted(p["own"]) == R["own"], (tag, r)
                        owners += list(p["own"])
                        assert p["nrow"] == max(q["arows"][1] - q["arows"][0] + 1 for q in plan)
                        assert p["mom_len"] == 8 + 5 * p["nrow"] * NXPA
                    assert sorted(owners) == sorted(ns.LINES), (tag, owners)
    assert seen > 50


def test_fixtures_reach_their_paths():
    """From the fixtures' c_dims, one expression per path of the launch geometry (k_xf_wekpa_stage.h, k_xforc.h)."""
    G = lib.xforc_wekpa_stage_points()
    P = {c: nx.params(nx.load(c)) for c in XF_CASES}
    assert all(p["tau_udiff"] for p in P.values())
    assert all(p["ndxr"] > lib.XFORC_WEKPA_STAGE_ABOVE for p in P.values())  # the staged box average by default
    p = P["xf_r80_ud"]
    assert p["ndxr"] == config.preset("natl1").ndxr == config.preset("cpl_natl1").ndxr == 80
    # k_xf_wekpa_stage: two workgroups on a row, the last one not full; the wrap reached from the first and the last
    assert p["nxta"] + 1 > G and (p["nxta"] + 1) % G != 0
    # k_xf_fine: a tail workgroup of fewer than 8 cells with a full one before it
    assert p["nxta"] % 8 != 0 and p["nxta"] > 8
    assert (p["nxaooc"], p["nyaooc"]) == (2, 1) and nstates("xf_r80_ud") == 2
    # odd ndxr above 64: half weights, nijwid = ndxr + 1, the paired jsou / jnor rows; a row length the row kernels take
    p = P["xf_r75_ud"]
    assert p["ndxr"] % 2 == 1 and p["ndxr"] + p["ndxr"] % 2 == 76 and p["nxaooc"] * p["ndxr"] == 150
    # the cyclic ocean's own line integrals, over two blocks of 256
    p = P["xf_cyc80_ud"]
    assert p["cyclic"] and p["nxaooc"] == p["nxta"] and p["nx1"] == 1 and p["nxaooc"] * p["ndxr"] + 1 == 321
    assert float(nx.load("xf_cyc80_ud")["out0_txisoc"]) != 0.0 and float(nx.load("xf_cyc80_ud")["out0_txinoc"]) != 0.0
    # the limit of the range
    assert P["xf_r128_ud"]["ndxr"] == P["xf_r128n3_ud"]["ndxr"] == lib.XFORC_NDXR_MAX == 128
    assert all((P[c]["nyta"] + 1 >= 4) == (c in GPU_CASES) for c in XF_CASES)
    # k_xf_heat_oc: a hundred rounds of 64 over a cell's ocean points
    h = nh.params(nh.load(HEAT_CASE))
    assert h["ndxr"] == 80 and h["ndxr"] ** 2 // 64 == 100 and h["xcexp"] != 1.0
    # every committed fixture stays below the limit of a committed file
    import os
    for c in XF_CASES + (HEAT_CASE,):
        assert os.path.getsize(os.path.join(nx.GOLDEN, c + ".npz")) < (1 << 20), c


def test_preset():
    """cpl_natl1: the natl1 ocean as a coupled preset under the 385 x 97 atmosphere at 80 km; natl1 itself untouched."""
    oc, at = config.preset("cpl_natl1"), config.atmos_preset("cpl_natl1")
    assert dataclasses.replace(oc, name="natl1") == config.preset("natl1")
    assert (oc.nxpo, oc.nypo, oc.ndxr) == (4801, 4801, 80) and (at.nxpa, at.nypa, at.dxa) == (385, 97, 8.0e4)
    assert at.nla == 3 and at.ah4at == config.atmos_preset("cpl_natl5").ah4at  # (both atmospheres are the 80 km one)
