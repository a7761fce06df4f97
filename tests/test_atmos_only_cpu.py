"""Atmosphere-only runs without a GPU: the numpy restatement of the heat half as a -Datmos_only build of
the reference runs it (tests/numpy_atmos_only.py) against the reference's own results (tests/golden/ato_*.npz), the
index paths the six fixtures are there for, and the restart dump of an atmos_only build."""
import struct

import numpy as np
import pytest

import numpy_atmos_only as na
from qgcm_hip import preset, restart


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("case", na.CASES)
def test_restatement(case):
    """heat_sst from the reference's state before every cycle: asto, fnetat over land (its pointwise tail included)
    bitwise; above the sea within the worst case of reordering a cell's ndxr^2 terms, 2 ndxr^2 2^-53 sum|terms|, plus
    one spacing of the value itself (the tail is added to the sum afterwards); the monitors within 2 n 2^-53
    sum|terms|; arocav = 0 exactly, in the reference and in the restatement."""
    g = na.load(case)
    P = na.params(g)
    R = na.restated(case)
    assert np.array_equal(_bits(R[0]["asto"]), _bits(g["t_asto"]))
    blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
    for c in range(P["K"]):
        H, ref = R[c], g["x%d_fnetat" % c]
        sea = H["ocean"]
        assert sea[blk].all() and sea.sum() == H["cell_abs"].size
        assert np.array_equal(_bits(H["fnetat"][~sea]), _bits(ref[~sea])), (case, c)
        assert np.array_equal(_bits(H["fnetat_land"][~sea]), _bits(ref[~sea])), (case, c)
        bound = 2.0 * P["ndxr"] ** 2 * 2.0 ** -53 * H["cell_abs"] + np.spacing(np.abs(ref[blk]))
        diff = np.abs(H["fnetat"][blk] - ref[blk])
        assert np.all(diff <= bound), (case, c, diff.max(), (diff / bound).max())
        assert np.all(ref[sea] != 0.0) and np.all(ref[sea] != H["fnetat_land"][sea])
        for f in na.SST_SCALARS:
            r = float(g["x%d_%s" % (c, f)])
            b = 2.0 * H["n_" + f] * 2.0 ** -53 * H["abs_" + f]
            assert abs(H[f] - r) <= b, (case, c, f, H[f], r, b)
        assert float(g["x%d_arocav" % c]) == 0.0 and H["arocav"] == 0.0
        assert "x%d_fnetoc" % c not in g


def test_fixture_paths():
    """From the fixtures' own dimensions: the index paths of the table in make_golden_atmos_only.py stay covered."""
    dims = {case: tuple(int(v) for v in na.load(case)["c_dims"]) for case in na.CASES}
    rounds = set()
    for nxta, nyta, nxaooc, nyaooc, ndxr in dims.values():
        full, part = divmod(ndxr * ndxr, 64)
        rounds.add("partial only" if full == 0 else "full only" if part == 0 else "full + partial")
    assert rounds == {"partial only", "full + partial", "full only"}
    assert any(nxta * nyta == nxaooc * nyaooc for nxta, nyta, nxaooc, nyaooc, _ in dims.values())      # natlan == 0
    assert any(nxaooc == nxta and nyaooc < nyta for nxta, nyta, nxaooc, nyaooc, _ in dims.values())    # wrapped, with land
    assert any(nxaooc * nyaooc > 256 for _, _, nxaooc, nyaooc, _ in dims.values())                     # ncell > 256
    assert any(ndxr % 2 == 1 for *_, ndxr in dims.values()) and any(ndxr == 16 for *_, ndxr in dims.values())
    for case, (nxta, nyta, nxaooc, nyaooc, ndxr) in dims.items():
        P = na.params(na.load(case))
        assert P["dxa"] / float(ndxr) == P["dxo"], case  # (the dxo the library derives without an ocean handle)


def _fields(cfg, nla, seed):
    rng = np.random.default_rng(seed)
    f = lambda *sh: np.asfortranarray(rng.standard_normal(sh))
    sha, shT, shA = (cfg.nxta + 1, cfg.nyta + 1, nla), (cfg.nxto, cfg.nyto), (cfg.nxta, cfg.nyta)
    return dict(tyrs=3.25, pa=f(*sha), pam=f(*sha), sst=f(*shT), sstm=f(*shT), ast=f(*shA), astm=f(*shA),
                hmixa=f(*shA), hmixam=f(*shA))


@pytest.mark.parametrize("nla", [3, 4])
def test_restart_atmos_only(tmp_path, nla):
    """tyrs | pa, pam | sst, sstm | ast, astm | hmixa, hmixam (src/q-gcm.F:3076-3086 with atmos_only): the length, the
    round trip, and the refusal to read it as a coupled dump."""
    cfg = preset("cpl_tiny")
    x = _fields(cfg, nla, 7)
    path = str(tmp_path / "lastday")
    restart.write_restart(path, cfg, atmos_only=True, **x)
    nP, nT, nA = (cfg.nxta + 1) * (cfg.nyta + 1) * nla, cfg.nxto * cfg.nyto, cfg.nxta * cfg.nyta
    sizes = [8, 16 * nP, 16 * nT, 16 * nA, 16 * nA]
    raw = open(path, "rb").read()
    assert len(raw) == sum(sizes) + 8 * len(sizes)
    o = 0
    for n in sizes:  # every record between its two markers
        assert struct.unpack("<i", raw[o:o + 4])[0] == n == struct.unpack("<i", raw[o + 4 + n:o + 8 + n])[0]
        o += n + 8
    y = restart.read_restart(path, cfg, atmos_only=True)
    assert set(y) == set(x) and y["tyrs"] == x["tyrs"]
    for k in x:
        if k != "tyrs":
            assert y[k].shape == x[k].shape and np.array_equal(_bits(y[k]), _bits(x[k])), k
    with pytest.raises(ValueError):
        restart.read_restart(path, cfg, coupled=True)
    with pytest.raises(ValueError):
        restart.read_restart(path, cfg)
    with pytest.raises(ValueError, match="no po / pom"):
        restart.write_restart(path, cfg, 0.0, np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)), atmos_only=True, pa=x["pa"], pam=x["pam"])
    with pytest.raises(ValueError, match="pa / pam must be"):
        restart.write_restart(path, cfg, 0.0, atmos_only=True, pa=x["pa"][:-1], pam=x["pam"][:-1])


@pytest.mark.parametrize("coupled", [False, True])
def test_restart_default_unchanged(tmp_path, coupled):
    """Without atmos_only the writer's bytes are the record sequence it always wrote - tyrs | po, pom | [pa, pam] |
    sst, sstm | ast, astm | hmixa, hmixam, laid out here by hand - and the reader returns the same dict."""
    cfg = preset("cpl_tiny")
    rng = np.random.default_rng(11)
    f = lambda *sh: np.asfortranarray(rng.standard_normal(sh))
    sh3, shT, shA, sha = (cfg.nxpo, cfg.nypo, cfg.nlo), (cfg.nxto, cfg.nyto), (cfg.nxta, cfg.nyta), (cfg.nxta + 1, cfg.nyta + 1, 3)
    x = dict(po=f(*sh3), pom=f(*sh3), sst=f(*shT), sstm=f(*shT), ast=f(*shA), astm=f(*shA), hmixa=f(*shA), hmixam=f(*shA))
    if coupled:
        x.update(pa=f(*sha), pam=f(*sha))
    path = str(tmp_path / "lastday")
    restart.write_restart(path, cfg, 1.5, x["po"], x["pom"], x["sst"], x["sstm"], x["ast"], x["astm"], x["hmixa"], x["hmixam"],
                          pa=x.get("pa"), pam=x.get("pam"))
    groups = [("po", "pom")] + ([("pa", "pam")] if coupled else []) + [("sst", "sstm"), ("ast", "astm"), ("hmixa", "hmixam")]
    want = struct.pack("<i", 8) + struct.pack("<d", 1.5) + struct.pack("<i", 8)
    for grp in groups:
        body = b"".join(x[k].tobytes(order="F") for k in grp)
        want += struct.pack("<i", len(body)) + body + struct.pack("<i", len(body))
    n3, nT, nA, na3 = int(np.prod(sh3)), int(np.prod(shT)), int(np.prod(shA)), int(np.prod(sha))
    assert len(want) == 8 + 16 * n3 + (16 * na3 if coupled else 0) + 16 * nT + 32 * nA + 8 * (5 + coupled)
    assert open(path, "rb").read() == want
    y = restart.read_restart(path, cfg, coupled=coupled)
    assert set(y) == set(x) | {"tyrs"} and y["tyrs"] == 1.5
    for k in x:
        assert np.array_equal(_bits(y[k]), _bits(x[k])), k
