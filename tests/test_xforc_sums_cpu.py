"""The owner-computed sums of the slab xforc without a GPU: the ownership plan against a brute-force
restatement of the kernels' index expressions, the refusals, the message lengths, SlabOcean's choreography on numpy
stand-ins (tests/numpy_xforc_sums.py), the partial sums and the rank-ordered combine against the sequential loops of the
reference, and the paths the GPU cases must keep reaching."""
import numpy as np
import pytest

import numpy_xforc as nx
import numpy_xforc_sums as ns
from numpy_slab_udiff import configs
from numpy_xforc_bands import BandAtmos
from qgcm_hip import QgcmHipError, config, lib
from qgcm_hip.slab import SlabOcean, owned_rows_tile, partition
from test_slab_coupled_cpu import CountingComm, _configs, _heat_cfg, _same

NXPA = 9


def _cuts(nyg, nranks):
    """The even cut and, where the rows allow, two uneven ones (every rank owns at least 4 rows)."""
    out = [partition(nyg, nranks)]
    if nranks > 1 and nyg >= 4 * nranks + 3:
        spare = nyg - 4 * nranks
        for first in (True, False):  # all the spare rows on the first / on the last rank
            n = [4 + (spare if (k == 0) == first and k in (0, nranks - 1) else 0) for k in range(nranks)]
            lo, rows = 1, []
            for k in n:
                rows.append((lo, lo + k - 1))
                lo += k
            out.append(rows)
    return [r for r in out if all(g1 - g0 + 1 >= 4 for g0, g1 in r)]


def test_plan_against_brute_force():
    """Even and odd ndxr, the sea touching row 1 or not (and the last row or not), 1 - 5 ranks, even and uneven cuts: the
    ownership tiles 1 .. nypaor; every fine row a kernel of the rank reads lies in its window, every T row in its owned
    T rows; the pressure rows under the window's sea rows the rank reads lie within g0 - 4 .. g1 + 4; the cell rows are
    exactly those that hold a read row; [a0, a1] is exactly the coarse rows the rank contributes to; the line sums have
    one owner each; nrow and the lengths follow.  A plan refused for a shared pair of line rows is one where the brute
    force finds the pair under two owners."""
    seen = refused = 0
    for ndxr in (4, 5, 7, 12):
        for nyta, ny1, nyaooc in ((8, 1, 3), (8, 3, 3), (8, 6, 3), (6, 1, 6), (9, 2, 5)):
            D = ns.dims(nyta, ndxr, ny1, nyaooc)
            cell = lambda f: min((f - 1) // ndxr + 1, nyta)
            for nranks in range(1, 6):
                for rows in _cuts(D["nyg"], nranks):
                    Pown, Town = ns.owner_rows(D, rows)
                    try:
                        plan = lib.xforc_sums(NXPA, nyta, ndxr, ny1, nyaooc, rows)
                    except QgcmHipError as e:
                        assert "would share" in str(e) and D["odd"]
                        assert Pown[D["jsou"]] != Pown[D["jsou"] + 1] or Pown[D["jnor"]] != Pown[D["jnor"] - 1], (rows, str(e))
                        refused += 1
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
                        if r:
                            assert f0 == plan[r - 1]["fine"][1] + 1, tag
                        R = ns.reads(D, rows, r)
                        w0, w1 = p["window"]
                        assert min(R["P"]) == w0 and max(R["P"]) == w1, (tag, r, sorted(R["P"]), p)
                        assert (w0, w1) == (max(1, f0 - 3), min(D["nypaor"], f1 + 3)), tag
                        assert R["T"] == set(range(p["trows"][0], p["trows"][1] + 1)), tag
                        g0, g1 = rows[r]
                        for f in R["P"]:  # xf_point reads pom rows jo - 1 .. jo + 1 (clipped at the basin's walls)
                            jo = f - D["jocoff"]
                            if 1 <= jo <= D["nyg"]:
                                assert g0 - 4 <= max(1, jo - 1) and min(D["nyg"], jo + 1) <= g1 + 4, (tag, r, f)
                        c0, c1 = p["cells"]
                        assert (c0, c1) == (cell(min(R["P"])), cell(max(R["P"]))), (tag, r)  # no wider than whole cell rows
                        fine_lo, fine_hi = 1 + (c0 - 1) * ndxr, D["nypaor"] if c1 == nyta else c1 * ndxr
                        assert fine_lo <= w0 and w1 <= fine_hi
                        assert p["coarse"] == (max(1, c0 - 1), min(D["nypa"], c1 + 2)), tag
                        assert R["A"] == set(range(p["arows"][0], p["arows"][1] + 1)), (tag, r, sorted(R["A"]), p["arows"])
                        assert sorted(p["own"]) == R["own"], (tag, r, p["own"], R["own"])
                        owners += list(p["own"])
                        assert p["nrow"] == max(q["arows"][1] - q["arows"][0] + 1 for q in plan)
                        assert p["mom_len"] == 8 + 5 * p["nrow"] * NXPA
                    assert sorted(owners) == sorted(ns.LINES), (tag, owners)
    assert seen > 100 and refused > 0, (seen, refused)


def test_plan_refusals():
    """Fewer than 4 owned rows, no rank, ranges that do not tile 1 .. nypo (a gap, an overlap, a short end, a late
    start), a bad geometry - each refused with its reason; SlabOcean.xforc_setup refuses the flag beside bands,
    udiff_gather or tau_udiff."""
    ok = (NXPA, 8, 4, 3, 3)  # nyg = 13
    assert len(lib.xforc_sums(*ok, [(1, 6), (7, 13)])) == 2
    with pytest.raises(QgcmHipError, match="rank 1 owns 3 ocean rows, fewer than 4"):
        lib.xforc_sums(*ok, [(1, 6), (7, 9), (10, 13)])
    with pytest.raises(QgcmHipError, match="nranks = 0, need at least one rank"):
        lib.xforc_sums(*ok, [])
    for rows in ([(1, 6), (8, 13)], [(1, 7), (7, 13)], [(2, 6), (7, 13)]):
        with pytest.raises(QgcmHipError, match="do not tile 1..13: rank . owns"):
            lib.xforc_sums(*ok, rows)
    with pytest.raises(QgcmHipError, match="do not tile 1..13: the last rank's end at 12"):
        lib.xforc_sums(*ok, [(1, 6), (7, 12)])
    with pytest.raises(QgcmHipError, match="bad geometry"):
        lib.xforc_sums(NXPA, 8, 4, 7, 3, [(1, 13)])
    # odd ndxr, a sea from row 1 to the last row: ndxr 5 pairs the fine rows 3, 4 and 28, 29, which a rank of 4 rows holds;
    # ndxr 7 pairs 4, 5 and 39, 40, which the seams 4 | 5 and 39 | 40 cut
    assert lib.xforc_sums(NXPA, 6, 5, 1, 6, [(1, 4), (5, 27), (28, 31)])[0]["own"] == ("txisat", "txisoc")
    with pytest.raises(QgcmHipError, match="txinat reads the fine rows 39 and 40, which rank 1 .* would share"):
        lib.xforc_sums(NXPA, 6, 7, 1, 6, [(1, 39), (40, 43)])
    with pytest.raises(QgcmHipError, match="txisat reads the fine rows 4 and 5, which rank 0 .* would share"):
        lib.xforc_sums(NXPA, 6, 7, 1, 6, [(1, 4), (5, 43)])
    g, P, oc, so, reps, log = _setup("heat_cpl_tiny", 2, False)
    kw = dict(tables=_tabs(P["ndxr"]), nx1=P["nx1"], ny1=P["ny1"])
    for bad in (dict(bands=True), dict(udiff_gather=True), dict(tau_udiff=True)):
        with pytest.raises(ValueError, match="udiff_sums = True excludes"):
            so.xforc_setup(reps, udiff_sums=True, **dict(kw, **bad))
    so.slabs[1].g0 += 1  # a row nobody owns
    with pytest.raises(ValueError, match="do not tile"):
        so.xforc_setup(reps, udiff_sums=True, **kw)


def test_lengths():
    """The edge message is 8 + 8 nxpo doubles: cpl_natl5 on 4 ranks 8 + 8 * 961 = 7696 against the gather's 231 609; NAtl
    1 km on eight ranks 38 416 against 2.9 M.  The momentum block is 8 + 5 nrow nxpa."""
    oc = config.preset("cpl_natl5")
    at = config.atmos_of(oc)
    assert oc.nxpo == 961 and ns.HDR + 2 * ns.EDGE * oc.nxpo == 7696
    assert 8 + owned_rows_tile(partition(oc.nypo, 4), oc.nypo) * oc.nxpo == 231609
    assert 8 + 8 * 4801 == 38416 and 8 + 601 * 4801 == 2885409
    plan = lib.xforc_sums(at.nxpa, at.nyta, oc.ndxr, 1 + (at.nyta - oc.nyaooc) // 2, oc.nyaooc, partition(oc.nypo, 4))
    assert all(p["mom_len"] == 8 + 5 * p["nrow"] * at.nxpa for p in plan)
    assert plan[0]["nrow"] < at.nypa  # (the land rows weigh on the outer ranks: DESIGN 6r)
    assert lib.XFORC_SUM_HEADER == lib.XFORC_EDGE_HEADER == ns.HDR and lib.XFORC_EDGE_ROWS == ns.EDGE
    assert lib.XFORC_SUM_FIELDS == ns.FIELDS


def _tabs(n):
    return {k: np.zeros((16, n + 1, n + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}


def _setup(case, nranks, heat, sums=False):
    g, P, oc, at = _configs(case)
    log = []
    slabs = [ns.SumsRowSlab(oc, g0, g1, r, nranks) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.log = log
        x.oml_set_sstm(g["in_sstm"])
        x.set_pom(g["in_pom"])
    so = SlabOcean(oc, slabs, CountingComm(nranks, log))
    reps = [BandAtmos(at, g, P, r, log) for r in range(nranks)]
    so.xforc_setup(reps, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tables=_tabs(P["ndxr"]),
                   nx1=P["nx1"], ny1=P["ny1"], udiff_sums=sums)
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], fsa=g["t_fsa"], fso=g["t_fso"],
                            coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    del log[:]
    return g, P, oc, so, reps, log


@pytest.mark.parametrize("case,nranks", [("heat_cpl_tiny", 1), ("heat_cpl_tiny", 3), ("heat_cyc72", 2)])
@pytest.mark.parametrize("heat", [False, True])
def test_choreography(case, nranks, heat):
    """One xforc(): edge pack on every rank, the small all-gather, edge assemble on every rank, part on every rank, the
    main all-gather, combine on every rank - exactly two all-gathers, with or without the heat half, on one rank too.
    Every rank's array holds the basin's rows g0 - 4 .. g1 + 4 and nothing else, each written once; the replicas end
    equal, with every entry written, and equal to the sequential sums within the bounds (bit-equal where uncut); the
    heat half is the plain slab run's bits.  A second call, a coupled window and the way back keep the counts."""
    g, P, oc, so, reps, log = _setup(case, nranks, heat, sums=True)
    n = nranks
    assert so.xforc_plan == lib.xforc_sums(reps[0].cfg.nxpa, reps[0].cfg.nyta, P["ndxr"], P["ny1"], P["nyaooc"], partition(oc.nypo, n))
    so.xforc()
    want = ["edge_pack"] * n + ["all_gather"] + ["edge_assemble"] * n + ["xforc_part"] * n + ["all_gather"] + ["xforc_combine"] * n
    assert [e[0] for e in log] == want, log
    assert log[n] == ("all_gather", 8 + 8 * oc.nxpo)
    assert log[3 * n + 1] == ("all_gather", so.slabs[0].xforc_msg_len(reps[0]))
    assert so.slabs[0].xforc_msg_len(reps[0]) == so.xforc_plan[0]["mom_len"] + (4 * P["nxaooc"] * P["nyaooc"] if heat else 0)
    for x in so.slabs:
        lo, hi = max(1, x.g0 - 4), min(oc.nypo, x.g1 + 4)
        _same(x.assembled[:, lo - 1:hi], g["in_pom"][:, lo - 1:hi], "rows g0 - 4 .. g1 + 4 on rank %d" % x.rank)
        assert np.isnan(x.assembled[:, :lo - 1]).all() and np.isnan(x.assembled[:, hi:]).all()
        assert list(x.written) == [0] * (lo - 1) + [1] * (hi - lo + 1) + [0] * (oc.nypo - hi)
    D = so.slabs[0].D
    txf, tyf, wf, uvekfc = ns.synthetic(reps[0].cfg, D["n"])
    seq = dict(ns.nx_coarse(D, reps[0].cfg.nxta, txf, tyf, uvekfc), wekpa=ns.wekpa_seq(D, reps[0].cfg.nxta, wf))
    B = ns.bounds(D, reps[0].cfg.nxta, txf, tyf, wf, uvekfc, 1.0, ns.owner_rows(D, partition(oc.nypo, n))[0])
    for a in reps:
        for f in ns.FIELDS:
            assert not np.isnan(a.sums[f]).any(), f
            _same(a.sums[f], reps[0].sums[f], f + " on the replicas")
        _same(a.sums["vekat"], seq["vekat"], "vekat")
        _same(a.sums["tauxa"], txf[::D["n"], ::D["n"]], "tauxa")
        for f in ("uekat", "wekpa"):
            cut, bound = B[f]
            _same(a.sums[f][~cut], seq[f][~cut], f + " where no seam cuts")
            assert np.all(np.abs(a.sums[f] - seq[f])[cut] <= bound[cut]), f
            assert cut.any() == (n > 1)
        assert a.sum_lines == {f: 1.0 + k for k, f in enumerate(ns.LINES)}
    if heat:
        from test_slab_coupled_cpu import _setup as plain
        g2, P2, oc2, so2, reps2, log2 = plain(case, nranks)
        so2.xforc()
        for h, h2 in zip(so.xforc_heat_get(), so2.xforc_heat_get()):
            _same(h["fnetat"], h2["fnetat"], "fnetat")
            _same(h["fnetoc"], h2["fnetoc"], "fnetoc")
        del log[:]
        so.coupled_steps(1, 4, 3, xforc=True)  # two ocean steps
        assert sum(1 for e in log if e[0] == "all_gather" and e[1] != 1) == 4, log
    x, a = so.slabs[0], reps[0]
    with pytest.raises(ValueError, match="the edge rows have not been assembled for this call"):
        x.xforc_part(a, so._xf_bufs[0][0])
    if heat:  # (the stand-ins keep their heat set-up, the library drops it with the momentum half's)
        return
    # the way back
    so.xforc_setup(reps, tables=_tabs(P["ndxr"]), nx1=P["nx1"], ny1=P["ny1"])
    assert so._xf_edge_bufs is None and so.xforc_plan is None
    del log[:]
    so.xforc()
    assert [e[0] for e in log] == ["xforc_part"] * n


def _rank_sums(case, s, rows):
    """The partial sums of every rank of a cut and their combine, from the fixture's fine stress."""
    g = nx.load(case)
    P = nx.params(g)
    D = ns.dims(P["nyta"], P["ndxr"], P["ny1"], P["nyaooc"])
    txf, tyf, wf, uvekfc = ns.fine(case, s)
    plan = lib.xforc_sums(P["nxta"] + 1, P["nyta"], P["ndxr"], P["ny1"], P["nyaooc"], rows)
    msgs = [(p["fine"][0], p["fine"][1], p["arows"][0],
             ns.part(D, P["nxta"], txf, tyf, wf, uvekfc, p["fine"][0], p["fine"][1], p["arows"][0], p["arows"][1], p["nrow"]))
            for p in plan]
    return D, P, plan, msgs, ns.combine(D, P["nxta"], uvekfc, msgs)


@pytest.mark.parametrize("case,nranks", [("xf_cpl_tiny_ud", 1), ("xf_cpl_tiny_ud", 2), ("xf_cpl_tiny_ud", 3), ("xf_odd5_ud", 3),
                                         ("xf_cyc4_ud", 3)])
def test_arithmetic(case, nranks):
    """The partial sums and the rank-ordered combine, restated, against the sequential loops of the reference
    (numpy_xforc.xforc on the fixture's second state): tauxa, tauya, vekat bit-equal; uekat, wekpa bit-equal where no
    seam cuts the line / the box - everywhere on one rank - and inside DESIGN 6r's bounds where one does; no entry is left
    unwritten."""
    g = nx.load(case)
    D, P, plan, msgs, R = _rank_sums(case, 1, partition(nx.params(g)["nyaooc"] * nx.params(g)["ndxr"] + 1, nranks))
    ref = nx.restated(case, 1)
    txf, tyf, wf, uvekfc = ns.fine(case, 1)
    Pown = ns.owner_rows(D, [p["rows"] for p in plan])[0]
    B = ns.bounds(D, P["nxta"], txf, tyf, wf, uvekfc, 1.0, Pown)
    for f in ("tauxa", "tauya", "vekat"):
        _same(R[f], ref[f], f)
    for f in ("uekat", "wekpa"):
        cut, bound = B[f]
        assert not np.isnan(R[f]).any()
        assert cut.any() == (nranks > 1) and not cut.all()
        _same(R[f][~cut], ref[f][~cut], f + " where no seam cuts")
        d = np.abs(R[f] - ref[f])
        assert np.all(d[cut] <= bound[cut]), (f, (d[cut] / bound[cut]).max())
        print("%s on %d ranks: %s differs at %d of %d cut entries, largest |diff| / bound %.3f"
              % (case, nranks, f, (d[cut] > 0).sum(), cut.sum(), (d[cut] / bound[cut]).max() if cut.any() else 0.0))


def test_minus_zero():
    """A line whose terms on one rank sum to -0.0 and which no other rank holds terms of: the combine starts from the
    first CONTRIBUTING rank's value, so the result is -uvekfc * -0.0 = +0.0 as the sequential loop gives; starting from a
    +0.0 placeholder of a rank that does not contribute would give -uvekfc * (+0.0 + -0.0) = -0.0."""
    D = ns.dims(8, 4, 3, 3)
    nxta = 4
    rows = [(1, 6), (7, 13)]
    plan = lib.xforc_sums(nxta + 1, 8, 4, 3, 3, rows)
    nxf = nxta * 4 + 1
    txf, tyf = np.ones((nxf, D["nypaor"])), np.full((nxf, D["nypaor"]), -0.0)
    wf = np.full((nxf - 1, D["nytaor"]), -0.0)
    msgs = [(p["fine"][0], p["fine"][1], p["arows"][0],
             ns.part(D, nxta, txf, tyf, wf, 0.125, p["fine"][0], p["fine"][1], p["arows"][0], p["arows"][1], p["nrow"])) for p in plan]
    R = ns.combine(D, nxta, 0.125, msgs)
    seq = ns.nx_coarse(D, nxta, txf, tyf, 0.125)
    uncut = ~ns.bounds(D, nxta, txf, tyf, wf, 0.125, 1.0, ns.owner_rows(D, rows)[0])["uekat"][0]
    assert uncut.any() and not np.signbit(seq["uekat"]).any()
    _same(R["uekat"][uncut], seq["uekat"][uncut], "uekat of -0.0 terms")
    ja = D["nyta"]  # a line only the last rank holds: rank 0 sends a +0.0 placeholder row or none
    assert plan[1]["fine"][0] <= 1 + (ja - 1) * 4
    naive = -0.125 * (0.0 + msgs[1][3][3, ja - msgs[1][2]])
    assert np.signbit(naive).all() and not np.signbit(R["uekat"][:, ja - 1]).any()


def test_edge_copies():
    """The two copies restated on a cut by hand: headers, the 4 + 4 owned rows, a neighbour's header that does not fit
    writes nothing."""
    nxpo, nypo = 5, 14
    pom = np.arange(1.0, nxpo * nypo + 1).reshape(nxpo, nypo)
    rows = [(1, 4), (5, 10), (11, 14)]
    msgs = [ns.edge_pack(pom[:, g0 - 1:g1], g0, g1, 1) for g0, g1 in rows]
    for (g0, g1), m in zip(rows, msgs):
        assert list(m[:8]) == [g0, g1, nxpo, 0, 0, 0, 0, 0]
        body = m[8:].reshape(8, nxpo)
        assert np.array_equal(body[:4], pom[:, g0 - 1:g0 + 3].T) and np.array_equal(body[4:], pom[:, g1 - 4:g1].T)
    out, written = ns.edge_assemble(np.concatenate(msgs), 1, 3, pom[:, 4:10], 5, 10, 1, nypo)
    assert np.array_equal(out, pom) and list(written) == [1] * 14
    out, written = ns.edge_assemble(np.concatenate(msgs), 0, 3, pom[:, :4], 1, 4, 1, nypo)
    assert np.array_equal(out[:, :8], pom[:, :8]) and np.isnan(out[:, 8:]).all()
    for h in ([5, 9, nxpo], [6, 10, nxpo], [5, 10, nxpo + 1], [0, 3, nxpo], [np.nan] * 3):
        bad = [m.copy() for m in msgs]
        bad[1][:3] = h
        out, written = ns.edge_assemble(np.concatenate(bad), 0, 3, pom[:, :4], 1, 4, 1, nypo)
        if h[0] == 5 and h[2] == nxpo:
            continue  # (rank 0 reads rank 1's FIRST rows: a header that still begins at the seam fits)
        assert np.isnan(out[:, 4:]).all() and list(written) == [1] * 4 + [0] * 10, h


def test_covered_paths():
    """From the fixtures' dimensions: every GPU case on more than one rank has, above the sea, at least one cut and one
    uncut uekat line and wekpa box; xf_cpl_tiny_ud (49 x 37, ndxr 12) on 3 ranks leaves the line over ocean rows 1 - 13
    whole and cuts the one over 13 - 25, on 2 ranks the seam 19 | 20 cuts the middle cell; one case has a seam directly
    beside a cell-boundary row; both kinds of basin, an odd ndxr and second blocks of the copy kernels are among them."""
    beside = False
    for case, nranks in ns.CASES:
        g, P, oc, at = configs(case)
        D = ns.dims(P["nyta"], P["ndxr"], P["ny1"], P["nyaooc"])
        rows = partition(oc.nypo, nranks)
        lib.xforc_sums(at.nxpa, at.nyta, P["ndxr"], P["ny1"], P["nyaooc"], rows)  # (not refused)
        Pown = ns.owner_rows(D, rows)[0]
        sea = [ja for ja in range(P["ny1"], P["ny1"] + P["nyaooc"])]  # the lines over sea rows only
        lines = [len({Pown[1 + (ja - 1) * D["n"] + k] for k in range(D["n"] + 1)}) > 1 for ja in sea]
        boxes = [len({Pown[j] for j in range(ns.box_rows(D, ja)[0], ns.box_rows(D, ja)[1] + 1)}) > 1 for ja in sea + [sea[-1] + 1]]
        if nranks > 1:
            assert any(lines) and not all(lines), (case, nranks, lines)
            assert any(boxes) and not all(boxes), (case, nranks, boxes)
            beside = beside or any((g1 - 1) % D["n"] == 0 or g1 % D["n"] == 0 for g0, g1 in rows[:-1])
        else:
            assert not any(lines) and not any(boxes)
    assert beside
    assert partition(37, 3) == [(1, 13), (14, 25), (26, 37)] and partition(37, 2)[0] == (1, 19)
    g, P, oc, at = configs("xf_cpl_tiny_ud")
    assert (oc.nxpo, oc.nypo, P["ndxr"]) == (49, 37, 12)
    D = ns.dims(P["nyta"], 12, P["ny1"], P["nyaooc"])
    Pown = ns.owner_rows(D, partition(37, 3))[0]
    j = D["jocoff"]
    assert len(set(Pown[j + 1:j + 14])) == 1 and len(set(Pown[j + 13:j + 26])) == 2
    Pown = ns.owner_rows(D, partition(37, 2))[0]
    assert len(set(Pown[j + 13:j + 26])) == 2
    assert {nx.params(nx.load(c))["cyclic"] for c, k in ns.CASES} == {0, 1}
    assert any(nx.params(nx.load(c))["ndxr"] % 2 for c, k in ns.CASES)
    assert any(configs(c)[2].nxpo > 256 for c, k in ns.CASES)  # second blocks of the edge copies
