"""tau_udiff on a y-slab ocean without a GPU: SlabOcean's choreography with udiff_gather = True on numpy
stand-ins (tests/numpy_slab_udiff.py), the message and the assembled array of the two copies restated, the lengths, and
the paths the GPU cases must keep reaching."""
import numpy as np
import pytest

import numpy_heat as nh
import numpy_xforc as nx
from numpy_slab_udiff import (BOX, CASES, CUTS, HDR, WIDE, BareAtmos, UdiffRowSlab, clipped_rows, configs, dims, pom_assemble, pom_pack)
from numpy_xforc_bands import BandAtmos
from qgcm_hip import config
from qgcm_hip.slab import SlabOcean, local_rows, owned_rows_tile, partition
from test_slab_coupled_cpu import CountingComm, _configs, _heat_cfg, _same


def _tabs(n):
    # a dummy set of weight tables: the momentum half is not restated here
    return {k: np.zeros((16, n + 1, n + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}


def _heat_setup(case, nranks, heat, bands, udiff):
    """A heat fixture's geometry on row views, its in_pom as the surface pressure."""
    g, P, oc, at = _configs(case)
    log = []
    slabs = [UdiffRowSlab(oc, g0, g1, r, nranks) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.log = log
        x.oml_set_sstm(g["in_sstm"])
        x.set_pom(g["in_pom"])
    so = SlabOcean(oc, slabs, CountingComm(nranks, log))
    reps = [BandAtmos(at, g, P, r, log) for r in range(nranks)]
    so.xforc_setup(reps, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tables=_tabs(P["ndxr"]),
                   nx1=P["nx1"], ny1=P["ny1"], bands=bands, udiff_gather=udiff)
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], fsa=g["t_fsa"], fso=g["t_fso"],
                            coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    del log[:]
    return g, P, oc, so, reps, log


@pytest.mark.parametrize("case,nranks", [("heat_cpl_tiny", 3), ("heat_cyc72", 2)])
@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("bands", [False, True])
@pytest.mark.parametrize("udiff", [False, True])
def test_choreography(case, nranks, heat, bands, udiff):
    """One xforc(): pack on every rank, the all-gather of the pressure rows, assemble on every rank, then the sequence
    as it was - part, and with the heat half or bands the all-gather of the message and the combine.  Two all-gathers
    with the heat half or bands, one without either; with the shear term off one and none, as before.  A second call and
    a coupled window keep the count."""
    g, P, oc, so, reps, log = _heat_setup(case, nranks, heat, bands, udiff)
    so.xforc()
    n = nranks
    pre = ["pom_pack"] * n + ["all_gather"] + ["pom_assemble"] * n if udiff else []
    post = ["all_gather"] + ["xforc_combine"] * n if (heat or bands) else []
    assert [e[0] for e in log] == pre + ["xforc_part"] * n + post, log
    assert sum(1 for e in log if e[0] == "all_gather") == int(udiff) + int(heat or bands)
    if udiff:
        nrow = max(g1 - g0 + 1 for g0, g1 in partition(oc.nypo, nranks))
        assert log[n] == ("all_gather", HDR + nrow * oc.nxpo)
        for x in so.slabs:
            _same(x.assembled, g["in_pom"], "the assembled array on rank %d" % x.rank)
            assert np.all(x.written == 1)
    if heat or bands:
        assert log[-n - 1] == ("all_gather", so.slabs[0].xforc_msg_len(reps[0]))
    if heat:  # the heat half does not see the shear term: the bits of the run without it
        from test_slab_coupled_cpu import _setup as plain
        g2, P2, oc2, so2, reps2, log2 = plain(case, nranks)
        so2.xforc()
        for h, h2 in zip(so.xforc_heat_get(), so2.xforc_heat_get()):
            _same(h["fnetat"], h2["fnetat"], "fnetat")
            _same(h["fnetoc"], h2["fnetoc"], "fnetoc")
        del log[:]
        so.coupled_steps(1, 4, 3, xforc=True)  # two ocean steps
        assert sum(1 for e in log if e[0] == "all_gather" and e[1] != 1) == 2 * (int(udiff) + 1), log
        assert [e[0] for e in log if e[0] in ("pom_pack", "pom_assemble")] == (["pom_pack"] * n + ["pom_assemble"] * n) * (2 if udiff else 0)


def test_part_needs_a_fresh_assemble():
    """With the shear term on a part without an assemble since the last part is refused; after the refusal a whole
    xforc() goes through; the shear-free set-up on the same objects needs none."""
    g, P, oc, so, reps, log = _heat_setup("heat_cpl_tiny", 2, False, False, True)
    x, a = so.slabs[0], reps[0]
    with pytest.raises(ValueError, match="the surface pressure has not been assembled for this call"):
        x.xforc_part(a, None)
    so.xforc()
    with pytest.raises(ValueError, match="the surface pressure has not been assembled for this call"):
        x.xforc_part(a, None)
    so.xforc()
    _same(x.assembled, g["in_pom"], "after the refusals")
    so.xforc_setup(reps, tables=_tabs(P["ndxr"]), nx1=P["nx1"], ny1=P["ny1"])
    assert so._xf_pom_bufs is None
    del log[:]
    so.xforc()
    assert [e[0] for e in log] == ["xforc_part"] * 2


def test_keywords():
    """udiff_gather with tau_udiff is a ValueError that says to pass only the former; tau_udiff alone reaches the
    set-up call, which refuses it as before; owned rows that do not tile the basin are refused on the host."""
    g, P, oc, so, reps, log = _heat_setup("heat_cpl_tiny", 2, False, False, False)
    kw = dict(tables=_tabs(P["ndxr"]), nx1=P["nx1"], ny1=P["ny1"])
    with pytest.raises(ValueError, match="pass only udiff_gather"):
        so.xforc_setup(reps, tau_udiff=True, udiff_gather=True, **kw)
    with pytest.raises(ValueError, match="tau_udiff is not available with a y-slab ocean"):
        so.xforc_setup(reps, tau_udiff=True, **kw)
    so.slabs[1].g0 += 1  # a row nobody owns
    with pytest.raises(ValueError, match="do not tile"):
        so.xforc_setup(reps, udiff_gather=True, **kw)
    with pytest.raises(ValueError, match="end at 36"):
        owned_rows_tile([(1, 19), (20, 36)], 37)
    assert owned_rows_tile(partition(37, 3), 37) == 13 and owned_rows_tile(partition(81, 5), 81) == 17


def _rows_of(case, cut):
    nxpo, nypo, n = dims(case)
    return cut(nypo) if callable(cut) else partition(nypo, cut)


ALL = [(c, k) for c, k in CASES] + CUTS


@pytest.mark.parametrize("case,cut", ALL, ids=["%s-%s" % (c, k if isinstance(k, int) else "cut") for c, k in ALL])
def test_assembled_array_and_length(case, cut):
    """Through SlabOcean.xforc_setup / xforc() on row views: every rank's assembled array is the basin's pom(:,:,1) by
    integer view, every point written once, from owned rows only (the stand-ins' halo rows hold NaN); the message is
    8 + nrow * nxpo doubles, its header g0, g1, nxpo and zeros, its padding rows +0.0."""
    g, P, oc, at = configs(case)
    rows = _rows_of(case, cut)
    nranks, nxpo, nypo = len(rows), oc.nxpo, oc.nypo
    assert g["in1_pom1"].shape == (nxpo, nypo)
    log = []
    slabs = [UdiffRowSlab(oc, g0, g1, r, nranks) for r, (g0, g1) in enumerate(rows)]
    for x in slabs:
        x.log = log
        x.set_pom(g["in1_pom1"])
    so = SlabOcean(oc, slabs, CountingComm(nranks, log))
    so.xforc_setup([BareAtmos(at, r) for r in range(nranks)], tables=_tabs(P["ndxr"]), nx1=P["nx1"], ny1=P["ny1"], udiff_gather=True)
    nrow = max(g1 - g0 + 1 for g0, g1 in rows)
    assert [x.xforc_pom_len(None) for x in slabs] == [HDR + nrow * nxpo] * nranks
    del log[:]
    so.xforc()
    assert [e for e in log if e[0] == "all_gather"] == [("all_gather", HDR + nrow * nxpo)]
    send, gath = so._xf_pom_bufs
    for x, s in zip(slabs, send):
        m = s.numpy()
        assert list(m[:HDR]) == [x.g0, x.g1, nxpo, 0, 0, 0, 0, 0]
        body = m[HDR:].reshape(nrow, nxpo)
        own = x.g1 - x.g0 + 1
        _same(body[:own], g["in1_pom1"][:, x.g0 - 1:x.g1].T, "the owned rows of rank %d" % x.rank)
        assert not body[own:].any() and not np.signbit(body[own:]).any()
        _same(x.assembled, g["in1_pom1"], "the assembled array on rank %d" % x.rank)
        assert np.all(x.written == 1)
    if nranks > 1 and nypo % nranks:
        assert any(x.g1 - x.g0 + 1 < nrow for x in slabs)  # padding rows present
    if callable(cut):
        assert slabs[0].g0 == slabs[0].g1 == 1 and slabs[-1].g0 == slabs[-1].g1 == nypo  # a rank that owns one row


def test_headers_that_write_nothing():
    """A header that does not describe rows inside 1 .. nypo, more rows than the message holds, or another row length:
    its rank writes nothing, the others' rows land."""
    nxpo, nypo, nrow = 5, 9, 5
    pom = np.arange(1.0, nxpo * nypo + 1).reshape(nxpo, nypo)
    rows = [(1, 5), (6, 9)]
    good = [pom_pack(pom[:, g0 - 1:g1], g0, g1, 1, nrow) for g0, g1 in rows]
    for h in ([0, 3, nxpo], [6, 10, nxpo], [7, 6, nxpo], [1, 9, nxpo], [6, 9, nxpo + 1], [np.nan, np.nan, np.nan]):
        bad = good[1].copy()
        bad[:3] = h
        out, written = pom_assemble(np.concatenate([good[0], bad]), 2, nrow, nxpo, nypo)
        assert np.array_equal(out[:, :5], pom[:, :5]) and np.isnan(out[:, 5:]).all(), h
        assert list(written) == [1] * 5 + [0] * 4
    out, written = pom_assemble(np.concatenate(good), 2, nrow, nxpo, nypo)
    assert np.array_equal(out, pom)


def test_lengths():
    """8 + nrow * nxpo for the cases, and for cpl_natl5 on 4 ranks: 231 609 doubles per rank."""
    for case, nranks in CASES:
        nxpo, nypo, n = dims(case)
        assert HDR + owned_rows_tile(partition(nypo, nranks), nypo) * nxpo == HDR + -(-nypo // nranks) * nxpo
    oc = config.preset("cpl_natl5")
    assert HDR + owned_rows_tile(partition(oc.nypo, 4), oc.nypo) * oc.nxpo == 231609
    # NAtl 1 km on eight ranks (DESIGN 6q's prediction): 8 + 601 * 4801 doubles per rank
    assert -(-4801 // 8) == 601 and 8 * (HDR + 601 * 4801) == 23_083_272 and 8 * 23_083_272 == 184_666_176


def test_covered_paths():
    """From the fixtures' dimensions: every case on more than one rank keeps a seam inside an atmosphere cell
    (g1 mod ndxr != 0); the copy kernels' second block is reached (nxpo > 256) by the wide cases; both kinds of basin
    and an odd ndxr are among the cases; one cut puts a seam between ocean rows 1 | 2 and nypo - 1 | nypo, the one-sided
    zbfcoc rows beside their neighbours; some case has an interior slab (halos on both sides) and uneven slabs."""
    for case, nranks in CASES:
        nxpo, nypo, n = dims(case)
        assert nx.params(nx.load(case))["tau_udiff"] == 1, case
        if nranks > 1:
            seams = [g1 for g0, g1 in partition(nypo, nranks)[:-1]]
            assert any(g1 % n != 0 for g1 in seams), (case, nranks, seams)
    assert sorted(dims(c)[0] for c, k in WIDE if c in ("xf_wide_ud", "xf_edge_ud")) == [257, 321]
    assert dims("xf_cycwide_ud")[0] > 256 and dims("xf_cyc4_ud")[0] <= 256
    assert {nx.params(nx.load(c))["cyclic"] for c, k in CASES} == {0, 1}
    assert any(dims(c)[2] % 2 for c, k in BOX)
    assert ("xf_cpl_tiny_ud", 1) in CASES
    assert any(k >= 3 for c, k in CASES) and any(dims(c)[1] % k for c, k in CASES if k > 1)
    hit = False
    for case, cut in CUTS:
        nypo = dims(case)[1]
        rows = cut(nypo)
        assert owned_rows_tile(rows, nypo) >= 1
        hit = hit or (rows[0] == (1, 1) and rows[1][0] == 2 and rows[-1] == (nypo, nypo) and rows[-2][1] == nypo - 1)
        for g0, g1 in rows:  # the row views the cut gives: owned rows inside the local rows, those inside the basin
            nyl, joff, jlo, jhi = clipped_rows(nypo, g0, g1)
            assert joff + jlo == g0 and joff + jhi == g1 and 1 <= jlo <= jhi <= nyl and joff >= 0 and joff + nyl <= nypo
    assert hit
    for case, nranks in CASES:  # the cuts of slab.partition: the clipped view is slab.local_rows
        nypo = dims(case)[1]
        for g0, g1 in partition(nypo, nranks):
            assert clipped_rows(nypo, g0, g1) == local_rows(nypo, g0, g1)


def test_heat_fixtures_have_a_surface_pressure():
    """The heat fixtures the GPU test drives with the shear term carry a non-zero pom."""
    for case in ("heat_cpl_tiny", "heat_cyc72"):
        assert np.abs(nh.load(case)["in_pom"]).max() > 1.0
