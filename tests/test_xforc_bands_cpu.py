"""The banded slab xforc without a GPU: the band plan (lib.xforc_bands: host code of the library) against a
brute-force restatement of the kernels' index expressions (tests/numpy_xforc_bands.py), and SlabOcean's choreography
with bands = True on numpy stand-ins."""
import numpy as np
import pytest

from numpy_xforc_bands import FIELDS, HDR, LINE_TRUTH, LINES, BandAtmos, BandRowSlab, needed_rows, truth
from qgcm_hip import QgcmHipError, lib
from qgcm_hip.slab import HALO, SlabOcean, partition
from test_slab_coupled_cpu import CountingComm, _configs, _heat_cfg, _same

NXPA = 17


def _slab_rows(nyg, nranks):
    """The rows the slabs of slab.partition hold: owned and up to HALO halo rows inside the basin."""
    return [(max(1, g0 - HALO), min(nyg, g1 + HALO)) for g0, g1 in partition(nyg, nranks)]


def _seas(nyta):
    """(ny1, nyaooc): a sea in the middle, at the southern edge and at the northern edge of the atmosphere."""
    nyaooc = max(1, nyta // 2)
    return sorted({(1 + (nyta - nyaooc) // 2, nyaooc), (1, nyaooc), (nyta - nyaooc + 1, nyaooc)})


def _cell_rows(c, n, nyta):
    """The fine p rows k_xf_fine writes for the cell row c: jj = 0 .. ndxr - 1, and the extra row of the northernmost."""
    return set(range(1 + (c - 1) * n, c * n + 1)) | ({nyta * n + 1} if c == nyta else set())


def test_plan_against_brute_force():
    """For every geometry of the issue's loop - nyta in {2, 3, 12, 20}, ndxr in {1, 4, 5, 12, 16}, nranks in {1, 2, 3, 5,
    nypa}, the sea in the middle and at either edge; slabs as slab.partition cuts them, with their halo rows - the
    plan's windows cover every fine p row and fine T row the kernels' index expressions touch for the rank's band, slab
    and line sums; they are no wider than whole cell rows (every cell row of the window holds a needed row; the T rows
    are exactly the needed ones); the bands tile 1 .. nypa; every line sum has one owner; the message length is the
    layout's.  More ranks than atmosphere rows are refused: a rank without a band has no place in the message."""
    count = 0
    for nyta in (2, 3, 12, 20):
        nypa = nyta + 1
        for ndxr in (1, 4, 5, 12, 16):
            for nranks in sorted({1, 2, 3, 5, nypa}):
                for ny1, nyaooc in _seas(nyta):
                    if nyaooc * ndxr + 1 < nranks:  # (the slabs need a row each: let the sea fill the atmosphere)
                        ny1, nyaooc = 1, nyta
                    nyg = nyaooc * ndxr + 1
                    tag = "nyta %d ndxr %d nranks %d ny1 %d nyaooc %d" % (nyta, ndxr, nranks, ny1, nyaooc)
                    if nranks > nypa:
                        with pytest.raises(QgcmHipError, match="every rank needs a band"):
                            lib.xforc_bands(NXPA, nyta, ndxr, ny1, nyaooc, [(1, nyg)] * nranks)
                        continue
                    slabs = _slab_rows(nyg, nranks)
                    plan = lib.xforc_bands(NXPA, nyta, ndxr, ny1, nyaooc, partition(nyg, nranks))
                    assert len(plan) == nranks
                    # the bands tile 1 .. nypa
                    assert plan[0]["band"][0] == 1 and plan[-1]["band"][1] == nypa, tag
                    for p, q in zip(plan, plan[1:]):
                        assert q["band"][0] == p["band"][1] + 1, tag
                    assert all(p["band"][1] >= p["band"][0] for p in plan), tag
                    nrow = max(p["band"][1] - p["band"][0] + 1 for p in plan)
                    for f in LINES:
                        assert sum(f in p["own"] for p in plan) == 1, (tag, f)
                    for r, p in enumerate(plan):
                        need_p, need_t = needed_rows(nyta, ndxr, ny1, nyg, p["band"], slabs[r], p["own"])
                        win = set()
                        for (c0, c1), (f0, f1) in zip(p["cells"], p["fine"]):
                            rows = set().union(*[_cell_rows(c, ndxr, nyta) for c in range(c0, c1 + 1)])
                            assert rows == set(range(f0, f1 + 1)), (tag, r, "the fine rows of the cell rows")
                            for c in range(c0, c1 + 1):
                                assert _cell_rows(c, ndxr, nyta) & need_p, (tag, r, "cell row %d holds no needed row" % c)
                            assert not (win & rows), (tag, r, "the intervals overlap")
                            win |= rows
                        assert 1 <= len(p["cells"]) <= 2 and 1 <= min(win) and max(win) <= nyta * ndxr + 1, (tag, r)
                        if len(p["cells"]) == 2:  # (they would have been merged had they touched)
                            assert p["cells"][1][0] > p["cells"][0][1] + 1, (tag, r)
                        assert need_p <= win, (tag, r, sorted(need_p - win))
                        assert set(range(p["trows"][0], p["trows"][1] + 1)) == need_t, (tag, r, p["trows"])
                        assert p["nrow"] == nrow and p["mom_len"] == HDR + len(FIELDS) * nrow * NXPA, (tag, r)
                        count += 1
    assert count > 500


def test_plan_refusals():
    with pytest.raises(QgcmHipError, match="outside 1..13"):
        lib.xforc_bands(NXPA, 12, 4, 2, 3, [(1, 9), (7, 14)])
    with pytest.raises(QgcmHipError, match="bad geometry"):
        lib.xforc_bands(NXPA, 12, 4, 11, 3, [(1, 13)])


def _setup(case, nranks, heat):
    g, P, oc, at = _configs(case)
    log = []
    slabs = [BandRowSlab(oc, g0, g1, r, nranks) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.log = log
        x.oml_set_sstm(g["in_sstm"])
    so = SlabOcean(oc, slabs, CountingComm(nranks, log))
    reps = [BandAtmos(at, g, P, r, log) for r in range(nranks)]
    tabs = {k: np.zeros((16, P["ndxr"] + 1, P["ndxr"] + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}
    so.xforc_setup(reps, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tables=tabs,
                   nx1=P["nx1"], ny1=P["ny1"], bands=True)
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], fsa=g["t_fsa"], fso=g["t_fso"],
                            coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    del log[:]
    return g, P, oc, at, so, reps, log


@pytest.mark.parametrize("case,nranks", [("heat_cpl_tiny", 1), ("heat_cpl_tiny", 3), ("heat_cpl_small", 5), ("heat_cyc72", 2),
                                         ("heat_cyc72", 3)])
@pytest.mark.parametrize("heat", [False, True])
def test_banded_choreography(case, nranks, heat):
    """xforc() with bands = True on virtual ranks of numpy stand-ins: every rank's part, ONE all-gather of the whole
    message - the momentum block, and behind it the heat block if the heat half is on - then the combine on every rank,
    with and without the heat half.  Before the scatter a replica holds its own band only; after it every replica holds
    every row of the six fields and the line sums, bit-equal across ranks; the heat half behind the momentum block gives
    the bits of the unbanded run."""
    g, P, oc, at, so, reps, log = _setup(case, nranks, heat)
    plan = so.xforc_plan
    mom = HDR + len(FIELDS) * plan[0]["nrow"] * at.nxpa
    assert all(p["mom_len"] == mom for p in plan)
    msg = mom + (4 * P["nxaooc"] * P["nyaooc"] if heat else 0)
    assert [x.xforc_msg_len(a) for x, a in zip(so.slabs, reps)] == [msg] * nranks
    so.xforc()
    assert [e[0] for e in log] == ["xforc_part"] * nranks + ["all_gather"] + ["xforc_combine"] * nranks, log
    assert log[nranks] == ("all_gather", msg)
    lines = [f for f in LINES if oc.cyclic or f.endswith("at")]
    for a in reps:
        for f in FIELDS:
            _same(a.mom[f], truth(f, at), f)
            _same(a.mom[f], reps[0].mom[f], f + " across replicas")
        for f in lines:
            assert a.lines[f] == LINE_TRUTH[f], f
    if heat:
        from test_slab_coupled_cpu import _setup as plain
        g2, P2, oc2, so2, reps2, log2 = plain(case, nranks)
        so2.xforc()
        for h, h2 in zip(so.xforc_heat_get(), so2.xforc_heat_get()):
            _same(h["fnetat"], h2["fnetat"], "fnetat against the unbanded run")
            _same(h["fnetoc"], h2["fnetoc"], "fnetoc against the unbanded run")
    # a second call and a coupled window keep the rule: one all-gather of this message per xforc
    del log[:]
    if heat:
        so.coupled_steps(1, 4, 3, xforc=True)
        assert sum(1 for e in log if e == ("all_gather", msg)) == 2
        assert [e[0] for e in log if e[0].startswith("xforc")] == (["xforc_part"] * nranks + ["xforc_combine"] * nranks) * 2


def test_default_is_unbanded():
    """bands = False (the default): no plan, and without the heat half no message."""
    g, P, oc, at = _configs("heat_cpl_tiny")
    slabs = [BandRowSlab(oc, g0, g1, r, 2) for r, (g0, g1) in enumerate(partition(oc.nypo, 2))]
    so = SlabOcean(oc, slabs, CountingComm(2, []))
    reps = [BandAtmos(at, g, P, r) for r in range(2)]
    tabs = {k: np.zeros((16, P["ndxr"] + 1, P["ndxr"] + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}
    so.xforc_setup(reps, tables=tabs, nx1=P["nx1"], ny1=P["ny1"])
    assert so.xforc_plan is None and so._xf_bufs is None
    assert [x.xforc_msg_len(a) for x, a in zip(slabs, reps)] == [0, 0]
