"""Shared helpers for the parity tests (tests may use oracle/, the product may not)."""
import os

import numpy as np

import oracle_binding as ob
from qgcm_hip import config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("po", "pom", "qo", "qom")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a).max())


def make_oracle(cfg, yporel=None):
    o = ob.Oracle(cfg.nxpo, cfg.nypo, cfg.nlo, cfg.cyclic, cfg.fnot, cfg.beta, cfg.dxo, cfg.dto,
                  cfg.delek, cfg.bccooc, cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc,
                  cfg.yporel() if yporel is None else yporel)
    if getattr(cfg, "l_spl", 0.0) > 0.0:  # a -Dsponge_layer_k247 configuration: as OceanModel does by itself
        from qgcm_hip import hostinit
        o.set_sponge(hostinit.sponge_ramp(cfg), cfg.c1_spl)
    return o


def apply_inputs(model, g, cfg):
    """Load the fixture's inputs into an Oracle or an OceanModel (same method names)."""
    model.set_p(g["in_po"], g["in_pom"])
    model.set_forcing(g["in_wekpo"], g["in_entoc"], g["in_xon"])
    if cfg.cyclic:
        model.set_cyc_forcing(float(g["in_txis"]), float(g["in_txin"]), g["in_enis"], g["in_enin"])
    if "in_rspl" in g:  # the reference build's own ramp (its exp() need not round like numpy's)
        model.set_sponge(g["in_rspl"], float(g["in_c1spl"]))


def load_snapshot(model, g, tag):
    model.set_state(*[g["%s_%s" % (tag, f)] for f in FIELDS])
    model.set_scalars(g[tag + "_scal"])


def state_errs(model, g, tag):
    st = model.get_state()
    return {f: relerr(st[i], g["%s_%s" % (tag, f)]) for i, f in enumerate(FIELDS)}


def scal_err(model, g, tag, cfg):
    """Constraint scalars are cancelling area integrals: compare relative to
    xlo*ylo*max|po|, not to their own magnitude."""
    s, r = model.get_scalars(), g[tag + "_scal"]
    scale = cfg.xlo * cfg.ylo * np.abs(g[tag + "_po"]).max()
    nl = cfg.nlo
    e = np.abs(s[:2 * (nl - 1)] - r[:2 * (nl - 1)]).max() / scale
    if cfg.cyclic:
        den = np.abs(r[2 * (nl - 1):]).max()
        e = max(e, np.abs(s[2 * (nl - 1):] - r[2 * (nl - 1):]).max() / den)
    return float(e)


# *_ah2: the tiny grids with ah2oc != 0 (the Del-4th-of-p viscosity term of src/qgosubs.F:375-377 and, cyclic, the
# ap3soc / ap3noc boundary sums) - tests/golden/make_golden.py
# *_spl: the tiny grids of reference builds with -Dsponge_layer_k247 (src/qgosubs.F:203-205)
CONFIG_NAMES = ("box_tiny", "box_tiny2", "box_small", "cyc_tiny", "cyc_small", "box_tiny_ah2", "cyc_tiny_ah2",
                "box_tiny_spl", "cyc_tiny_spl", "box_tiny5", "cyc_tiny6")
BOX_NAMES = ("box_tiny", "box_tiny2", "box_small", "box_tiny_ah2", "box_tiny_spl", "box_tiny5")
SNAPS = {"box_tiny": (1, 2, 25, 26, 60), "box_tiny2": (1, 26), "box_tiny5": (1, 2, 26), "cyc_tiny6": (1, 2, 26), "box_small": (1, 30),
         "cyc_tiny": (1, 2, 25, 26, 60), "cyc_small": (1, 30), "box_tiny_ah2": (1, 2, 26), "cyc_tiny_ah2": (1, 2, 26),
         "box_tiny_spl": (1, 2, 26), "cyc_tiny_spl": (1, 2, 26)}


def preset(name):
    return config.preset(name)


# layer tables of the oceans that no preset carries: nlo -> hoc, gpoc, ah2oc, ah4oc (test_gpu_parity's
# test_fast_kernels_with_two_and_four_layers, tests/test_gpu_ocean_layers.py)
OCEAN_LAYERS = {
    2: dict(hoc=(500.0, 3500.0), gpoc=(0.02,), ah2oc=(0.0, 0.0), ah4oc=(1.2e10,) * 2),
    4: dict(hoc=(300.0, 500.0, 1200.0, 2000.0), gpoc=(0.02, 0.01, 0.005), ah2oc=(0.0,) * 4, ah4oc=(1.2e10,) * 4),
    5: dict(hoc=(300.0, 400.0, 600.0, 1000.0, 1700.0), gpoc=(0.02, 0.012, 0.008, 0.005), ah2oc=(0.0,) * 5, ah4oc=(1.2e10,) * 5),
    6: dict(hoc=(250.0, 350.0, 500.0, 700.0, 1000.0, 1200.0), gpoc=(0.02, 0.015, 0.01, 0.007, 0.004), ah2oc=(0.0,) * 6,
            ah4oc=(1.2e10,) * 6),
    8: dict(hoc=(200.0, 250.0, 300.0, 400.0, 500.0, 650.0, 800.0, 900.0), gpoc=(0.02, 0.016, 0.013, 0.01, 0.008, 0.006, 0.004),
            ah2oc=(0.0,) * 8, ah4oc=(1.2e10,) * 8)}


def layer_cfg(nlo, cyclic):
    """The 193-column grids of test_fast_kernels_with_two_and_four_layers: nl<nlo>_box 193 x 97, nl<nlo>_cyc 193 x 65,
    nxto = 192 = 64 * 3 (the wave-per-row-pair kernels; two to four layers take their fused forms)."""
    base = dict(fnot=-1.19467e-04, beta=1.31301e-11, cyclic=True) if cyclic else dict(fnot=9.37456e-05, beta=1.7536e-11, cyclic=False)
    cfg = config.OceanConfig("nl%d_%s" % (nlo, "cyc" if cyclic else "box"), 12 if cyclic else 16, 10, 12, 4 if cyclic else 6, 16, nlo,
                             dxo=2.5e4, dta=240.0, **OCEAN_LAYERS[nlo], **base)
    assert cfg.nxto == 192
    return cfg


# ---- ocean mixed layer fixtures (tests/golden/make_golden_oml.py) -----------------------------
OML_CASES = (("oml_box_tiny", "box_tiny"), ("oml_box_tiny_sb", "box_tiny"), ("oml_cyc_tiny", "cyc_tiny"),
             # two, five and six layers: entoc enters layers 1 and 2; at two layers layer 2 is the bottom layer
             ("oml_box_tiny2", "box_tiny2"), ("oml_box_tiny5", "box_tiny5"), ("oml_cyc_tiny6", "cyc_tiny6"))
OML_SNAPS = (1, 2, 26, 40)
# ... of which the five- and six-layer fixtures hold the first two (step 1 averages; each further snapshot is four
# fields of five or six layers, and a committed file stays under 1 MiB)
OML_CASE_SNAPS = {"oml_box_tiny5": (1, 2), "oml_cyc_tiny6": (1, 2)}


def oml_snaps(case):
    return OML_CASE_SNAPS.get(case, OML_SNAPS)


# ... and the short fixtures on grids that cross the seams of the device kernels' tiles (k_oml_step: 64 x 8 T points,
# k_oml_entoc: 64 x 16 p points): one call and two coupled steps each
OML_SEAM_CASES = (("oml_box_seam", "box_seam"), ("oml_box_seam_nb", "box_seam"), ("oml_box_seam_sbnb", "box_seam"),
                  ("oml_box_128_sbnb", "box_128"), ("oml_cyc_128", "cyc_128"), ("oml_cyc_72_sbnb", "cyc_72"))
OML_SEAM_SNAPS = (1, 2)


def oml_config(g):
    """OmlConfig of a mixed-layer fixture."""
    p = g["oml_params"]
    return config.OmlConfig(hmoc=p[0], toc=(p[1], p[2]), st2d=p[3], st4d=p[4], ycexp=p[5], rhooc=1.0, cpoc=1.0 / p[6],
                            sb_hflux=bool(p[7]), tsbdy=p[8], nb_hflux=bool(p[9]), tnbdy=p[10])


def oml_load(model, g, cfg, is_oracle):
    """Inputs of a mixed-layer fixture into an Oracle or an OceanModel."""
    nl = cfg.nlo
    model.set_p(g["in_po"], g["in_pom"])
    model.set_forcing(g["in_wekpo"], np.zeros((cfg.nxpo, cfg.nypo), order="F"), np.zeros(nl - 1))
    if cfg.cyclic:
        model.set_cyc_forcing(float(g["in_txis"]), float(g["in_txin"]), np.zeros(nl - 1), np.zeros(nl - 1))
    if is_oracle:
        model.oml_set(g["in_sst"], g["in_sstm"], g["in_fnetoc"], g["in_wekto"], g["in_tauxo"], g["in_tauyo"])
    else:
        model.oml_set_state(g["in_sst"], g["in_sstm"])
        model.oml_set_forcing(g["in_fnetoc"], g["in_wekto"], g["in_tauxo"], g["in_tauyo"])


def oml_init_oracle(o, om):
    o.oml_init(om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc, om.sb_hflux, om.tsbdy,
               om.nb_hflux, om.tnbdy)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b, what):
    """Equality by integer view; the message counts and locates the points that differ (0-based indices)."""
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    ne = np.asarray(bits(a) != bits(b))
    if ne.any():
        where = np.argwhere(ne)
        raise AssertionError("%s: %d points differ, max |diff| %.3e, first at %s, columns %d..%d, rows %s" % (
            what, int(ne.sum()), np.abs(np.asarray(a) - np.asarray(b)).max(), where[:8].tolist(),
            where[:, 0].min(), where[:, 0].max(), sorted(set(where[:, -1].tolist()))[:12]))


def oml_weights(cfg):
    """Trapezoidal weights of xintp on the p grid (src/intsubs.f:78-133) and of the boundary line sums."""
    wx, wy = np.ones(cfg.nxpo), np.ones(cfg.nypo)
    wx[0] = wx[-1] = wy[0] = wy[-1] = 0.5
    return wx, wy


def oml_bounds(cfg, xfo, coneno, entoc):
    """How far the mixed layer's reordered sums may lie from the reference's.  Everything pointwise in oml is bitwise;
    only the ORDER of four kinds of sums differs on the device.  With u = 2^-53, a sum of n terms formed with r
    roundings in any order lies within r u sum|terms| of the exact sum (to first order in u), so two orders differ by at
    most 2 r u sum|terms|; a scaling of the sum is one more rounding of the chain.

      mean   xmean = (sum of the N = nxto nyto values of xfo) * ocnorm: N - 1 additions and the scaling, r = N:
             B_mean = 2 N u sum|xfo| ocnorm
      entoc  0.25 ((x0 - m) + (x1 - m) + (x2 - m) + (x3 - m)) of identical x with means that differ by d <= B_mean: each
             difference carries d and is rounded (u X each side, X = max|xfo| + |mean| bounds every |x - m|), the three
             additions round partial sums of at most 4 X: 4 d + 2 u (4 X + 3 * 4 X) = 4 d + 32 u X before the exact
             factor 0.25 (the two-cell and one-cell forms on the walls come out smaller):
             B_entoc = B_mean + 8 u X
      xon(1) dxo dyo sum(w entoc) over the n = nxpo nypo points of the p grid: n - 1 additions and two scalings
             (r = n + 1) of terms that themselves differ by at most w B_entoc (sum(w) = N < n):
             B_xon = dxo dyo (2 (n + 1) u sum|w entoc| + n B_entoc)
      line sums  dxo sum(wx entoc(:, row)), nxpo terms, one scaling (r = nxpo), terms within wx B_entoc:
             B_line = dxo (2 nxpo u sum|wx entoc| + nxpo B_entoc)
      centoc dxo dyo sum(-coneno): N identical terms, two scalings (r = N + 1): B_centoc = 2 (N + 1) u sum|coneno| dxo dyo
    xfo, coneno: the reference algorithm's terms (oracle.oml_get_xfo()); entoc: the reference's result."""
    u = 2.0 ** -53
    N, n = cfg.nxto * cfg.nyto, cfg.nxpo * cfg.nypo
    ocnorm = 1.0 / (float(cfg.nxto) * float(cfg.nyto))
    wx, wy = oml_weights(cfg)
    mean = float(xfo.sum()) * ocnorm
    b = dict(mean=2.0 * N * u * float(np.abs(xfo).sum()) * ocnorm)
    b["entoc"] = b["mean"] + 8.0 * u * (float(np.abs(xfo).max()) + abs(mean))
    b["xon"] = cfg.dxo * cfg.dyo * (2.0 * (n + 1) * u * float(np.abs(wx[:, None] * wy[None, :] * entoc).sum()) + n * b["entoc"])
    b["centoc"] = 2.0 * (N + 1) * u * float(np.abs(coneno).sum()) * cfg.dxo * cfg.dyo
    for k, row in (("enis", 0), ("enin", -1)):
        b[k] = cfg.dxo * (2.0 * cfg.nxpo * u * float(np.abs(wx * entoc[:, row]).sum()) + cfg.nxpo * b["entoc"])
    return b


def oml_check_sums(tag, cfg, bound, ent, scal, ref_ent, ref_scal):
    """entoc and the scalars (xon(1), cfraoc, centoc, enisoc(1), eninoc(1)) of one call against the reference's within
    oml_bounds; every figure is printed before it is asserted.  Returns the largest |diff| / bound per quantity."""
    ratios = {}
    d = np.abs(np.asarray(ent) - ref_ent)
    ij = np.unravel_index(int(d.argmax()), d.shape)
    print("%s entoc: max |diff| %.3e at %s, bound %.3e" % (tag, d.max(), ij, bound["entoc"]))
    assert d.max() <= bound["entoc"], (tag, "entoc", float(d.max()), ij, bound["entoc"])
    ratios["entoc"] = float(d.max() / bound["entoc"])
    assert scal[1] == ref_scal[1], (tag, "cfraoc", scal[1], ref_scal[1])  # the convecting fraction: an exact count
    names = (("xon", 0), ("centoc", 2)) + ((("enis", 3), ("enin", 4)) if cfg.cyclic else ())
    for f, k in names:
        diff = abs(float(scal[k]) - float(ref_scal[k]))
        print("%s %s: got %.17e reference %.17e |diff| %.3e bound %.3e" % (tag, f, scal[k], ref_scal[k], diff, bound[f]))
        assert diff <= bound[f], (tag, f, float(scal[k]), float(ref_scal[k]), bound[f])
        ratios[f] = diff / bound[f]
    return ratios


def oml_numpy_sums(cfg, xfo, coneno):
    """The reordered part of oml (src/omlsubs.F:131-233) again with numpy's pairwise sums: mean removal, averaging onto
    the p grid in the reference's operand order, xon(1), centoc and the line sums.  Returns entoc and the five scalars
    (cfraoc left 0: it is a count)."""
    nx, ny = cfg.nxpo, cfg.nypo
    ocnorm = 1.0 / (float(cfg.nxto) * float(cfg.nyto))
    x = xfo - float(np.sum(xfo)) * ocnorm
    e = np.zeros((nx, ny), order="F")
    e[1:-1, 1:-1] = 0.25 * (x[:-1, :-1] + x[1:, :-1] + x[:-1, 1:] + x[1:, 1:])
    e[1:-1, 0] = 0.5 * (x[:-1, 0] + x[1:, 0])
    e[1:-1, -1] = 0.5 * (x[:-1, -1] + x[1:, -1])
    if cfg.cyclic:
        e[0, 1:-1] = 0.25 * (x[-1, :-1] + x[0, :-1] + x[-1, 1:] + x[0, 1:])
        e[0, 0] = 0.5 * (x[-1, 0] + x[0, 0])
        e[0, -1] = 0.5 * (x[-1, -1] + x[0, -1])
        e[-1, :] = e[0, :]
    else:
        e[0, 1:-1] = 0.5 * (x[0, :-1] + x[0, 1:])
        e[-1, 1:-1] = 0.5 * (x[-1, :-1] + x[-1, 1:])
        e[0, 0], e[-1, 0], e[0, -1], e[-1, -1] = x[0, 0], x[-1, 0], x[0, -1], x[-1, -1]
    wx, wy = oml_weights(cfg)
    scal = np.zeros(5)
    scal[0] = float(np.sum(wx[:, None] * wy[None, :] * e)) * cfg.dxo * cfg.dyo
    scal[2] = float(np.sum(-coneno)) * cfg.dxo * cfg.dyo
    if cfg.cyclic:
        scal[3] = cfg.dxo * float(np.sum(wx * e[:, 0]))
        scal[4] = cfg.dxo * float(np.sum(wx * e[:, -1]))
    return e, scal


def oml_convecting(call_sst, toc1):
    """Points that convected in a call: the adjustment (7.13, src/omlsubs.F:116-119) leaves them at toc(1), to the
    rounding of one addition; every other point ends above it."""
    return call_sst <= toc1 * (1.0 + 4.0 * np.finfo(float).eps)


def oml_seam_columns(nxto, cyclic):
    """0-based T columns next to an x seam of the 64-wide tiles, two on either side where the grid has them; a
    channel's wrap is a seam between its last and its first tile."""
    cols = set()
    for s in range(64, nxto, 64):
        cols.update(c for c in (s - 2, s - 1, s, s + 1) if c < nxto)
    if cyclic and nxto > 64:
        cols.update((nxto - 2, nxto - 1, 0, 1))
    return sorted(cols)


# ---- atmosphere fixtures (tests/golden/make_golden_atmos.py), SURVEY 8 row f3 ------------------------------
# atm_tiny_a<n>: cpl_tiny's atmosphere with n = 2, 4, 5 layers and a different ah4at in every layer (reference builds
# cpl_tiny_a<n>; config.atmos_preset reads the layer count from the name)
ATM_CASES = (("atm_tiny", "cpl_tiny"), ("atm_small", "cpl_small"), ("atm_natl5", "cpl_natl5"),
             ("atm_tiny_a2", "cpl_tiny_a2"), ("atm_tiny_a4", "cpl_tiny_a4"), ("atm_tiny_a5", "cpl_tiny_a5"))
ATM_SNAPS = {"atm_tiny": (1, 2, 100, 101, 130), "atm_small": (1, 40), "atm_natl5": (1, 6, 101),
             "atm_tiny_a2": (1, 2, 100, 101, 130), "atm_tiny_a4": (1, 2, 100, 101, 130),
             "atm_tiny_a5": (1, 2, 100, 101, 130)}
ATM_LAYER_CASES = ("atm_tiny_a2", "atm_tiny_a4", "atm_tiny_a5")
CPL_CASES = ("cpl_tiny", "cpl_tiny_a4")  # coupled main loop fixtures (make_golden_atmos.py coupled)
ATM_FIELDS = ("pa", "pam", "qa", "qam")


def atm_inputs(g, acfg):
    """Inputs of an atmosphere fixture. atm_natl5 stores every 4th row / column: the full fields are re-generated
    from qgcm_hip.synth.atmos_fields and must reproduce the stored sample bit for bit."""
    st = int(g["stride"]) if "stride" in g else 1
    if st == 1:
        return {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    from qgcm_hip import synth
    f = synth.atmos_fields(acfg)
    for k in ("pa", "pam", "wekpa", "entat", "ddynat"):
        assert np.array_equal(f[k][::st, ::st], g["in_" + k]), "synthetic atmosphere input %s drifted from the fixture" % k
    for k in ("xan", "txis", "txin", "enis", "enin"):
        assert np.array_equal(np.asarray(f[k]), g["in_" + k]), k
    return f


def make_atm_oracle(acfg, g, f):
    return ob.AtmosOracle(acfg.nxpa, acfg.nypa, acfg.nla, acfg.fnot, acfg.beta, acfg.dxa, acfg.dta, acfg.bccoat,
                          acfg.ah4at, acfg.hat, acfg.gpat, g["c_yparel"], f["ddynat"])


def atm_wide(nxta, nla):
    """cpl_tiny's atmosphere (dxa, dta, nyta = 12) with nla layers on rows of nxta points: 192 and 384 take the
    wave-per-row-pair kernels.  No reference build exists at these shapes: the CPU oracle is the yardstick."""
    import dataclasses
    at = config.atmos_preset("cpl_tiny", nla)
    return dataclasses.replace(at, nxta=nxta, name="%s_w%d" % (at.name, nxta + 1))


def make_atm_oracle_of(acfg, f):
    """AtmosOracle with the configuration's own yparel (no fixture)."""
    return ob.AtmosOracle(acfg.nxpa, acfg.nypa, acfg.nla, acfg.fnot, acfg.beta, acfg.dxa, acfg.dta, acfg.bccoat,
                          acfg.ah4at, acfg.hat, acfg.gpat, acfg.yporel(), f["ddynat"])


def atm_mode_errs(name, ctl2m, ctm2l, g):
    """relerr of the mode matrices ctl2m[k, m], ctm2l[m, k] against the reference's.  The reference's atmospheric
    eigenvectors keep the sign LAPACK's Schur vectors happen to have (eigmode.f:283-296; no rule restates it), and no
    result depends on it as long as both matrices carry the same one (cm2l * cl2m = 1).  For the three-layer fixtures
    "positive in layer 1" reproduces it and the comparison is as it always was; with four and five layers some modes
    come out negated, so for ATM_LAYER_CASES each mode is compared under the sign that its layer-1 component has in
    the reference's ctl2m - one sign per mode, applied to its column of ctl2m and its row of ctm2l alike."""
    rl, rm = g["c_ctl2mat"], g["c_ctm2lat"]
    if name in ATM_LAYER_CASES:
        sg = np.sign(rl[0, :]) * np.sign(np.asarray(ctl2m)[0, :])
        assert np.all(np.abs(sg) == 1.0)
        ctl2m, ctm2l = np.asarray(ctl2m) * sg[None, :], np.asarray(ctm2l) * sg[:, None]
    return relerr(ctl2m, rl), relerr(ctm2l, rm)


def atm_apply(model, f):
    """Start-up sequence + forcing into an AtmosOracle or an AtmosModel (same method names)."""
    model.set_p(f["pa"], f["pam"])
    model.set_forcing(f["wekpa"], f["entat"], f["xan"], float(f["txis"]), float(f["txin"]), f["enis"], f["enin"])


def atm_state_errs(model, g, tag):
    st = int(g["stride"]) if "stride" in g else 1
    s = model.get_state()
    return {n: relerr(s[i][::st, ::st], g["%s_%s" % (tag, n)]) for i, n in enumerate(ATM_FIELDS)}


def atm_load_snapshot(model, g, tag):
    model.set_state(*[g["%s_%s" % (tag, n)] for n in ATM_FIELDS])
    model.set_scalars(g[tag + "_scal"])


def atm_scal_err(model, g, tag, acfg):
    """dpiat relative to xla*yla*max|pa| (cancelling area integrals); atmc* relative to their maximum."""
    s, r = model.get_scalars(), g[tag + "_scal"]
    nl = acfg.nla
    scale = acfg.xla * acfg.yla * np.abs(g[tag + "_pa"]).max()
    e = np.abs(s[:2 * (nl - 1)] - r[:2 * (nl - 1)]).max() / scale
    den = np.abs(r[2 * (nl - 1):]).max()
    return float(max(e, np.abs(s[2 * (nl - 1):] - r[2 * (nl - 1):]).max() / den))


def cpl_fullsize_inputs(g, oc, at):
    """Inputs of tests/golden/cpl_natl5_sample.npz (make_golden_atmos.py coupled_fullsize): re-generated from
    qgcm_hip.synth; the stored strided samples must be reproduced bit for bit."""
    from qgcm_hip import synth
    so, sa = int(g["stride_oc"]), int(g["stride"])
    po = synth.gaussian_eddy(oc, noise=1.0e-3)
    pom = np.asfortranarray(0.98 * po)
    tx, ty = synth.wind_stress(oc)
    _, wekpo = synth.wekpo_from_tau(oc, tx, ty)
    for k, v in (("po", po), ("pom", pom), ("wekpo", wekpo)):
        assert np.array_equal(v[::so, ::so], g["in_" + k]), "synthetic ocean input %s drifted from the fixture" % k
    f = synth.atmos_fields(at)
    for k in ("pa", "pam", "wekpa", "entat", "ddynat"):
        assert np.array_equal(f[k][::sa, ::sa], g["in_" + k]), "synthetic atmosphere input %s drifted from the fixture" % k
    for k in ("xan", "txis", "txin", "enis", "enin"):
        assert np.array_equal(np.asarray(f[k]), g["in_" + k]), k
    return po, pom, wekpo, f


def cpl_fullsize_errs(ocean, atmos, g, nt):
    so = int(g["stride_oc"])
    e = {n: float(np.abs(ocean.get_state()[i][::so, ::so] - g["nt%d_%s" % (nt, n)]).max() / float(g["nt%d_%s_max" % (nt, n)]))
         for i, n in enumerate(FIELDS)}
    e.update(atm_state_errs(atmos, g, "nt%d" % nt))
    return e
