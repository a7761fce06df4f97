"""Ocean mixed layer: the CPU restatement of oml / omladf (oracle/qgcm_oracle.c) against the
golden vectors of the TRUE reference (tests/golden/make_golden_oml.py; twelve reference builds, three of them the tiny grids with two, five and six layers).  Three on the 48 x 36 T
grid of the tiny presets (box with no-flux walls, box with -Dsb_hflux, cyclic with -Dnb_hflux), run for 40 steps; six on
grids that cross the seams of the device kernels' tiles (65 x 25, 128 x 16, channels of 128 and 72 columns) with the wall
options the tiny ones lack (-Dnb_hflux on a box, both options on a box, -Dsb_hflux on a channel), one call and two steps
each.  The restatement is pinned at those sizes and options here, without a GPU; the fixtures themselves are checked for
the branches they are meant to reach, and the bounds the GPU tests hold the reordered sums to (common.oml_bounds) are
checked against a numpy re-summation of the reference's own terms."""
import numpy as np
import pytest

from common import (OML_CASES, OML_SEAM_CASES, OML_SEAM_SNAPS, FIELDS, load_golden, make_oracle, oml_bounds,
                    oml_check_sums, oml_config, oml_convecting, oml_init_oracle, oml_load, oml_numpy_sums,
                    oml_seam_columns, oml_snaps, relerr, same_bits)
from qgcm_hip import preset


@pytest.mark.parametrize("case,cfgname", OML_CASES + OML_SEAM_CASES)
def test_one_call_is_bitwise_the_reference(case, cfgname):
    g, cfg = load_golden(case), preset(cfgname)
    om = oml_config(g)
    o = make_oracle(cfg)
    try:
        o.oml_init(om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc, om.sb_hflux, om.tsbdy,
                   om.nb_hflux, om.tnbdy)
        oml_load(o, g, cfg, True)
        o.oml()
        sst, sstm, ent, scal = o.oml_get()
        # the reference's omlsubs.F is compiled without OpenMP (flang rejects its REDUCTION(-:)), so even the
        # global sums run in the order restated here
        assert np.array_equal(sst, g["call_sst"])
        assert np.array_equal(sstm, g["call_sstm"])
        assert np.array_equal(ent, g["call_entoc"])
        assert scal[1] == g["call_scal"][1]                       # convecting fraction
        assert abs(scal[2] - g["call_scal"][2]) <= 1e-14 * abs(g["call_scal"][2])
        # xon(1) is the area integral of a field whose mean was removed: compare to area * max|entoc|
        area = cfg.xlo * cfg.ylo * np.abs(ent).max()
        assert abs(scal[0] - g["call_scal"][0]) <= 1e-14 * area
        if cfg.cyclic:
            assert np.allclose(scal[3:], g["call_scal"][3:], rtol=1e-13, atol=0.0)
    finally:
        o.close()


@pytest.mark.parametrize("case,cfgname", OML_CASES)
def test_coupled_steps(case, cfgname):
    """oml, qgostep, ocinvq, ocqbdy (+ averaging incl. sst), src/q-gcm.F:1232-1249,1328-1366."""
    g, cfg = load_golden(case), preset(cfgname)
    om = oml_config(g)
    o = make_oracle(cfg)
    try:
        o.oml_init(om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc, om.sb_hflux, om.tsbdy,
                   om.nb_hflux, om.tnbdy)
        oml_load(o, g, cfg, True)
        done = 0
        for n in oml_snaps(case):
            o.steps_oml(done + 1, n - done)
            done = n
            sst, sstm, ent, _ = o.oml_get()
            assert relerr(sst, g["steps%d_sst" % n]) < 1e-14
            assert relerr(ent, g["steps%d_entoc" % n]) < 1e-11
            for f, x in zip(FIELDS, o.get_state()):
                assert relerr(x, g["steps%d_%s" % (n, f)]) < 1e-12, (f, n)
    finally:
        o.close()


@pytest.mark.parametrize("case,cfgname", OML_SEAM_CASES)
def test_seam_fixture_steps(case, cfgname):
    """The coupled steps of the seam fixtures: the first step begins with oml from the inputs and its averaging of sst is
    exact, so sst / sstm are bitwise after it; after the second the bars of test_coupled_steps hold."""
    g, cfg = load_golden(case), preset(cfgname)
    o = make_oracle(cfg)
    try:
        oml_init_oracle(o, oml_config(g))
        oml_load(o, g, cfg, True)
        done = 0
        for n in OML_SEAM_SNAPS:
            o.steps_oml(done + 1, n - done)
            done = n
            sst, sstm, ent, _ = o.oml_get()
            if n == 1:
                same_bits(sst, g["steps1_sst"], case + " sst after step 1")
                same_bits(sstm, g["steps1_sstm"], case + " sstm after step 1")
            assert relerr(sst, g["steps%d_sst" % n]) < 1e-14
            assert relerr(sstm, g["steps%d_sstm" % n]) < 1e-14
            assert relerr(ent, g["steps%d_entoc" % n]) < 1e-11
        assert relerr(o.get_state()[0], g["steps2_po"]) < 1e-12
    finally:
        o.close()


def _call_terms(case, cfgname):
    """(g, cfg, xfo, coneno) of the one call of a fixture, the terms from the restatement (bitwise the reference's:
    test_one_call_is_bitwise_the_reference)."""
    g, cfg = load_golden(case), preset(cfgname)
    o = make_oracle(cfg)
    try:
        oml_init_oracle(o, oml_config(g))
        oml_load(o, g, cfg, True)
        o.oml()
        xfo, coneno = o.oml_get_xfo()
    finally:
        o.close()
    return g, cfg, xfo, coneno


@pytest.mark.parametrize("case,cfgname", OML_SEAM_CASES)
def test_bounds_hold_a_pairwise_resummation(case, cfgname):
    """common.oml_bounds before the GPU tests rely on it: the reference's own terms summed again in numpy's pairwise
    order (another reordering, as the device's tree is) stay inside the bounds.  The bounds are not vacuous: the
    pointwise one is below 1e-12 of max|entoc|, and a mean shifted by three bounds is caught."""
    g, cfg, xfo, coneno = _call_terms(case, cfgname)
    b = oml_bounds(cfg, xfo, coneno, g["call_entoc"])
    ent, scal = oml_numpy_sums(cfg, xfo, coneno)
    scal[1] = g["call_scal"][1]
    r = oml_check_sums(case + " numpy", cfg, b, ent, scal, g["call_entoc"], g["call_scal"])
    print(case, "largest |diff| / bound of the pairwise re-summation:", r)
    assert b["entoc"] < 1e-12 * np.abs(g["call_entoc"]).max()
    ocnorm = 1.0 / (float(cfg.nxto) * float(cfg.nyto))
    shifted = xfo.copy()
    shifted[0, 0] += 3.0 * b["entoc"] / ocnorm  # moves the mean by three bounds
    ent2, _ = oml_numpy_sums(cfg, shifted, coneno)
    assert np.abs(ent2[2:-2, 2:-2] - g["call_entoc"][2:-2, 2:-2]).max() > b["entoc"]


def test_fixtures_exercise_their_branches():
    """Conditions on the seam fixtures, met by the reference alone (the generator asserts them when it writes the
    files): the dimensions the tile situations need; convecting and non-convecting points in each of the T columns next
    to every x seam (two on either side) and in both wall rows; the wall options change what they should and nothing
    else: -Dnb_hflux the two northernmost T rows of the one call's sst (Del^4 = Del^2 of Del^2 reaches one row beyond
    the wall row), -Dsb_hflux the two southernmost, and those rows do differ."""
    dims = {"oml_box_seam": (65, 25), "oml_box_seam_nb": (65, 25), "oml_box_seam_sbnb": (65, 25),
            "oml_box_128_sbnb": (128, 16), "oml_cyc_128": (128, 20), "oml_cyc_72_sbnb": (72, 20)}
    flags = {"oml_box_seam": (0, 0), "oml_box_seam_nb": (0, 1), "oml_box_seam_sbnb": (1, 1), "oml_box_128_sbnb": (1, 1),
             "oml_cyc_128": (0, 1), "oml_cyc_72_sbnb": (1, 1)}
    G = {}
    for case, cfgname in OML_SEAM_CASES:
        g, cfg = load_golden(case), preset(cfgname)
        G[case] = g
        assert (cfg.nxto, cfg.nyto) == dims[case] == g["call_sst"].shape, case
        assert g["call_entoc"].shape == (cfg.nxpo, cfg.nypo) and cfg.nxpo > 64 and cfg.nypo > 16, case
        assert (int(g["oml_params"][7]), int(g["oml_params"][9])) == flags[case], case
        assert cfg.cyclic == case.startswith("oml_cyc"), case
        conv = oml_convecting(g["call_sst"], g["oml_params"][1])
        n = cfg.nxto * cfg.nyto
        assert abs(conv.sum() - g["call_scal"][1] * n) < 1e-9, case  # the mask is the reference's own count
        assert 0.0 < g["call_scal"][1] < 1.0, case
        cols = oml_seam_columns(cfg.nxto, cfg.cyclic)
        assert cols, case
        for c in cols:
            assert conv[c, :].any() and not conv[c, :].all(), (case, "column", c)
        for r in (0, -1):
            assert conv[:, r].any() and not conv[:, r].all(), (case, "row", r)
    # 65 x 25: a last tile of one column and one row; 128 x 16: exact multiples; 128 / 72 columns round a channel
    assert 65 % 64 == 1 and 25 % 8 == 1 and 128 % 64 == 0 and 16 % 8 == 0 and 72 % 64 == 8
    assert oml_seam_columns(65, False) == [62, 63, 64] and oml_seam_columns(128, True) == [0, 1, 62, 63, 64, 65, 126, 127]
    assert oml_seam_columns(72, True) == [0, 1, 62, 63, 64, 65, 70, 71]
    base, nb, sbnb = G["oml_box_seam"], G["oml_box_seam_nb"], G["oml_box_seam_sbnb"]
    for k in ("in_sst", "in_sstm", "in_fnetoc", "in_wekto", "in_tauxo", "in_tauyo", "in_po", "in_pom", "in_wekpo"):
        assert np.array_equal(base[k], nb[k]) and np.array_equal(base[k], sbnb[k]), k  # the wall option alone differs
    for g in (nb, sbnb):
        assert np.array_equal(g["call_sstm"], base["call_sstm"])  # the old sst
    d_nb = base["call_sst"] != nb["call_sst"]
    assert not d_nb[:, :-2].any() and d_nb[:, -2].any() and d_nb[:, -1].any()
    d_sb = base["call_sst"] != sbnb["call_sst"]
    assert not d_sb[:, 2:-2].any() and all(d_sb[:, r].any() for r in (0, 1, -2, -1))
    assert np.array_equal(nb["call_sst"][:, 2:], sbnb["call_sst"][:, 2:])  # north of the two southern rows: nb alone
    # every point of those rows that did not convect (and so kept its own value) differs
    keep = ~oml_convecting(base["call_sst"], base["oml_params"][1]) & ~oml_convecting(sbnb["call_sst"], base["oml_params"][1])
    for r in (0, 1, -2, -1):
        assert keep[:, r].any() and d_sb[keep[:, r], r].all(), r
