"""The numpy restatement of aml / amladf and of the heat half of xforc (tests/numpy_heat.py) against the reference's own
results (tests/golden/heat_*.npz, written by tests/golden/make_golden_heat.py): IEEE operations in the reference's
order reproduce every field and every serially summed scalar bit for bit, hostinit.bilint_tables reproduces asto and
hostinit.fsprim the forcing tables.  The restatement is what the device kernels are debugged against."""
import numpy as np
import pytest

import numpy_heat as nh
from qgcm_hip import hostinit


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.all(np.isfinite(b)), what
    assert np.array_equal(_bits(a), _bits(b)), "%s: max |diff| %.3e, %d differ" % (
        what, np.max(np.abs(np.asarray(a) - b)), int((_bits(a) != _bits(b)).sum()))


@pytest.mark.parametrize("case", nh.CASES)
def test_aml_restatement_is_bitwise(case):
    g = nh.load(case)
    P = nh.params(g)
    R = nh.restated(case)
    for c in range(P["K"]):
        for s in range(P["nstr"]):
            A = R[("a", c, s)]
            for f in nh.AML_FIELDS + nh.AML_SUMS + ("cfraat",):
                _same(A[f], g["a%d%d_%s" % (c, s, f)], "%s aml %d.%d %s" % (case, c, s, f))


@pytest.mark.parametrize("case", nh.CASES)
def test_heat_restatement_is_bitwise(case):
    g = nh.load(case)
    P = nh.params(g)
    R = nh.restated(case)
    for c in range(P["K"]):
        H = R[("x", c)]
        for f in ("fnetoc", "fnetat") + nh.HEAT_SCALARS:
            _same(H[f], g["x%d_%s" % (c, f)], "%s xforc %d %s" % (case, c, f))
    _same(R[("x", 0)]["asto"], g["t_asto"], case + " asto")


@pytest.mark.parametrize("case", nh.CASES)
def test_hostinit_tables(case):
    """bilint_tables (from the coordinates the package derives itself) gives asto bitwise; fsprim agrees with the
    reference's libm to 1 ulp."""
    from qgcm_hip import config
    import dataclasses
    g = nh.load(case)
    P = nh.params(g)
    oc = dataclasses.replace(config.preset("cpl_tiny"), nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"],
                             nyaooc=P["nyaooc"], ndxr=P["ndxr"], dxo=P["dxo"])
    G = hostinit.grid_coordinates(config.atmos_of(oc), oc)
    for k in ("xta", "yta", "xto", "yto"):
        _same(G[k], g["t_" + k], case + " " + k)
    T = hostinit.bilint_tables(G["xta"], G["yta"], G["xto"], G["yto"], P["dxa"], P["dya"])
    _same(nh.bilint(T, g["in_astm"]), g["t_asto"], case + " asto")
    assert T["iam"].min() >= 1 and T["iap"].max() <= P["nxta"] and T["jam"].min() >= 1 and T["jap"].max() <= P["nyta"]
    if P["cyclic"]:  # the mended indices: the first ocean columns lie west of the first atmospheric T point
        assert T["iam"][0] == P["nxta"] and T["iap"][0] == 1 and T["iap"][-1] == 1
    for tab, yrel in (("fsa", G["ytarel"]), ("fso", G["ytorel"])):
        mine, ref = hostinit.fsprim(yrel, P["fspco"], G["yla"]), g["t_" + tab]
        ulp = np.spacing(np.abs(ref))
        print("%s %s: max |diff| / ulp = %.2f" % (case, tab, np.max(np.abs(mine - ref) / ulp)))
        assert np.all(np.abs(mine - ref) <= ulp), tab


def test_fixtures_exercise_their_branches():
    """The conditions the generator asserts, seen again from the restatement: every case takes every branch of the
    step in some call and none of them somewhere in the interior; fnetat above the ocean is neither zero nor the land
    formula; xcexp != 1 with non-zero xc1ast / dtopat occurs, and so do odd ndxr, the cyclic ocean and a grid wider and
    taller than one 64 x 8 tile."""
    for case in nh.CASES:
        g = nh.load(case)
        P = nh.params(g)
        R = nh.restated(case)
        got = dict(diab=False, floor=False, conv=False, none=False)
        for c in range(P["K"]):
            H = R[("x", c)]
            oc = H["ocean"]
            assert oc.sum() == P["nxaooc"] * P["nyaooc"]
            assert np.all(H["fnetat"][oc] != 0.0) and np.all(H["fnetat"][oc] != H["fnetat_land"][oc]), case
            _same(H["fnetat"][~oc], H["fnetat_land"][~oc], case + " land")
            for s in range(P["nstr"]):
                b = R[("a", c, s)]["branches"]
                for k in ("diab", "floor", "conv"):
                    got[k] |= bool(b[k].any())
                got["none"] |= bool((~b["diab"] & ~b["floor"] & ~b["conv"])[1:-1, 1:-1].any())
                cf = float(g["a%d%d_cfraat" % (c, s)])
                assert abs(cf * P["nxta"] * P["nyta"] - float(b["conv"].sum())) < 1.0e-9
        assert all(got.values()), (case, got)
        assert any(0.0 < float(g["a%d%d_cfraat" % (c, s)]) < 1.0 for c in range(P["K"]) for s in range(P["nstr"]))
    P = [nh.params(nh.load(c)) for c in nh.CASES]
    assert any(p["xcexp"] != 1.0 for p in P) and any(p["xcexp"] == 1.0 for p in P)
    assert any(np.abs(nh.load(c)["in_xc1ast"]).max() > 0 and np.abs(nh.load(c)["in_dtopat"]).max() > 0 for c in nh.CASES)
    assert any(p["ndxr"] % 2 == 1 for p in P) and any(p["cyclic"] and p["nxaooc"] == p["nxta"] for p in P)
    assert any(p["nxta"] > 64 and p["nyta"] > 8 for p in P)
    # The launch geometry (k_xforc.h, k_aml.h), from the fixtures' dimensions alone; each line is one path that some
    # fixture must reach.
    blocks = lambda n, w: -(-n // w)
    # k_xf_heat_oc: a wave strides by 64 over the ndxr^2 ocean points of a cell; the production refinement takes four rounds
    assert any(p["ndxr"] == 16 for p in P)
    # k_xf_heat_final: one workgroup strides by 256 over the cells above the ocean; a second round, box and cyclic
    assert any(p["nxaooc"] * p["nyaooc"] > 256 and not p["cyclic"] for p in P)
    assert any(p["nxaooc"] * p["nyaooc"] > 256 and p["cyclic"] for p in P)
    # k_aml_step, k_aml_entat: 64-wide tiles; more than two tile columns and a last one that is neither full nor half
    assert any(blocks(p["nxta"], 64) >= 3 and p["nxta"] % 64 not in (0, 32) for p in P)
    # ... and a last tile of at most 8 columns (most of its threads idle, the zonal wrap right behind its few columns)
    assert any(0 < p["nxta"] % 64 <= 8 for p in P)
    # aml fed by uekat, vekat, wekta of multi-block momentum kernels: 256 threads along nxpa = nxta + 1
    assert any(blocks(p["nxta"] + 1, 256) >= 2 for p in P)
    # a<c><s>_* records cut into more than one extra part are all merged back
    g = nh.load("heat_300")
    assert all("a%d%d_%s" % (c, s, f) in g for c in range(3) for s in range(3) for f in nh.AML_FIELDS + nh.AML_SUMS)
