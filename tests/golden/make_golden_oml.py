#!/usr/bin/env python3
"""Golden vectors of the ocean mixed layer (oml / omladf, src/omlsubs.F) from the TRUE
reference compiled by oracle/build_ref.sh.  Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_oml.py

One reference build per fixture (grid and boundary variant are compile-time options there), twelve in all.
On the 48 x 36 T grid of the tiny presets:
  oml_box_tiny      box ocean, no-flux walls                      (-Docean_only)
  oml_box_tiny_sb   box ocean, specified southern temperature     (-Docean_only -Dsb_hflux)
  oml_cyc_tiny      zonally cyclic ocean, specified northern T    (-Docean_only -Dcyclic_ocean -Dnb_hflux)
and on the tiny grids with two, five and six layers (entoc enters layers 1 and 2: at two layers layer 2 is the bottom;
the five- and six-layer files hold the coupled runs after 1 and 2 steps only):
  oml_box_tiny2     box_tiny2, 30 x 24 T cells, two layers;  oml_box_tiny5  box_tiny5, five layers
  oml_cyc_tiny6     cyc_tiny6, six layers, -Dnb_hflux
Each of these holds the inputs, the result of ONE `call oml` from them, and coupled runs
(oml, qgostep, ocinvq, ocqbdy + averaging, src/q-gcm.F:1232-1249,1328-1366) after 1, 2, 26 and 40 steps.

On grids that cross the seams of the device kernels' tiles (k_oml_step: 64 x 8 T points, k_oml_entoc: 64 x 16 p points):
  oml_box_seam       box, T grid 65 x 25, no-flux walls: one seam, a last tile of one column / one row, p grid 66 x 26
  oml_box_seam_nb    the same inputs, -Dnb_hflux
  oml_box_seam_sbnb  the same inputs, -Dsb_hflux -Dnb_hflux
  oml_box_128_sbnb   box, 128 x 16, both: exact multiples of the tile, wall rows on tile edges, p grid 129 x 17
  oml_cyc_128        channel, 128 x 20, -Dnb_hflux (every cyclic build carries it): the wrap from tile 0 into tile 1 and back
  oml_cyc_72_sbnb    channel, 72 x 20, -Dsb_hflux -Dnb_hflux: the wrap with a last tile of 8 columns, southern wall on a channel
(the reference's FFT set-up accepts both channel widths as they stand: 128 = 2^7, 72 = 2^3 3^2.)
These hold the inputs, one `call oml`, and sst, sstm, entoc and the mixed-layer scalars after 1 and 2 coupled steps (po
after step 2 only).  Their sst adds tilted stripes of 2.5 K to synth.mixed_layer_fields, so that convecting and
non-convecting points lie on both sides of every seam and in both wall rows (synth's own field convects in the northern
half only); the generator asserts this, tests/test_oml_oracle.py::test_fixtures_exercise_their_branches checks it again.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))

# fixture -> (reference configuration of oracle/ref_binding.CONFIGS, preset of qgcm_hip.config)
VARIANTS = {"oml_box_tiny": ("box_tiny", "box_tiny"), "oml_box_tiny_sb": ("box_tiny_sb", "box_tiny"),
            "oml_cyc_tiny": ("cyc_tiny", "cyc_tiny"),
            # two, five and six layers: entoc enters layers 1 and 2, and at two layers layer 2 is the bottom layer
            "oml_box_tiny2": ("box_tiny2", "box_tiny2"), "oml_box_tiny5": ("box_tiny5", "box_tiny5"),
            "oml_cyc_tiny6": ("cyc_tiny6", "cyc_tiny6"),
            "oml_box_seam": ("box_seam", "box_seam"), "oml_box_seam_nb": ("box_seam_nb", "box_seam"),
            "oml_box_seam_sbnb": ("box_seam_sbnb", "box_seam"), "oml_box_128_sbnb": ("box_128_sbnb", "box_128"),
            "oml_cyc_128": ("cyc_128", "cyc_128"), "oml_cyc_72_sbnb": ("cyc_72_sbnb", "cyc_72")}
SNAPS = (1, 2, 26, 40)
SHORT = {"oml_box_tiny5": (1, 2), "oml_cyc_tiny6": (1, 2)}  # the prefix of SNAPS that keeps the file under 1 MiB
SEAM = tuple(v for v in VARIANTS if "tiny" not in v)  # the short fixtures of the tile-seam grids
SEAM_SNAPS = (1, 2)
SEAM_SEED = 11  # one seed: the three oml_box_seam* fixtures differ by the wall option alone


def seam_fields(cfg, om, seed):
    """synth.mixed_layer_fields + stripes of 2.5 K across sst and sstm, tilted (two periods in x, one in y) so that every
    column and both wall rows cross toc(1); periodic in x."""
    from qgcm_hip import synth
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=seed)
    x = (np.arange(cfg.nxto)[:, None] + 0.5) / cfg.nxto
    y = (np.arange(cfg.nyto)[None, :] + 0.5) / cfg.nyto
    stripes = 2.5 * np.sin(2.0 * np.pi * (2.0 * x + y))
    return np.asfortranarray(sst + stripes), np.asfortranarray(sstm + stripes), fnet, tx, ty


def check_branches(name, g, cfg):
    """What a seam fixture has to reach (asserted here on the reference's own result)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from common import oml_convecting as convecting, oml_seam_columns as seam_columns
    toc1 = g["oml_params"][1]
    conv = convecting(g["call_sst"], toc1)
    n = cfg.nxto * cfg.nyto
    assert abs(conv.sum() - g["call_scal"][1] * n) < 1.0e-9, (name, conv.sum(), g["call_scal"][1] * n)
    assert 0 < conv.sum() < n, name
    for c in seam_columns(cfg.nxto, cfg.cyclic):
        assert conv[c, :].any() and not conv[c, :].all(), (name, "column", c)
    for r in (0, -1):
        assert conv[:, r].any() and not conv[:, r].all(), (name, "row", r)


def make(name):
    import ref_binding
    from qgcm_hip import config, synth
    refcfg, preset = VARIANTS[name]
    cfg = config.preset(preset)
    ref_binding.build(refcfg)
    r = ref_binding.RefLib(refcfg)
    sb, nb = r.oml_flags()
    om = config.oml_preset(cfg, sb_hflux=bool(sb), nb_hflux=bool(nb))
    r.init(cfg.dxo, cfg.dto, cfg.delek, cfg.bccooc, cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc)
    r.oml_init(om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc, om.tsbdy, om.tnbdy)
    nl = cfg.nlo
    po = synth.gaussian_eddy(cfg, noise=1.0e-3)
    pom = np.asfortranarray(0.98 * po)
    seam = name in SEAM
    if seam:
        sst, sstm, fnet, tx, ty = seam_fields(cfg, om, SEAM_SEED)
    else:
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=11)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    out = dict(in_po=po, in_pom=pom, in_sst=sst, in_sstm=sstm, in_fnetoc=fnet, in_tauxo=tx, in_tauyo=ty,
               in_wekto=wekto, in_wekpo=wekpo,
               oml_params=np.array([om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc,
                                    float(sb), om.tsbdy, float(nb), om.tnbdy]))

    def load():
        r.set_p(po, pom)
        r.set_forcing(wekpo, None, np.zeros(nl - 1))
        if cfg.cyclic:
            txis, txin = synth.tau_line_integrals(cfg, tx)
            r.set_cyc_forcing(txis, txin, np.zeros(nl - 1), np.zeros(nl - 1))
            out.update(in_txis=txis, in_txin=txin)
        r.oml_set(sst, sstm, fnet, wekto, tx, ty)

    load()
    r.oml()
    a, b, e, s = r.oml_get()
    out.update(call_sst=a, call_sstm=b, call_entoc=e, call_scal=s)
    load()
    done = 0
    for n in (SEAM_SNAPS if seam else SHORT.get(name, SNAPS)):
        r.steps_oml(done + 1, n - done)
        done = n
        st = r.get_state()
        a, b, e, s = r.oml_get()
        for f, x in zip(("po", "pom", "qo", "qom"), st):
            if not seam or (f == "po" and n == SEAM_SNAPS[-1]):
                out["steps%d_%s" % (n, f)] = x
        out["steps%d_sst" % n], out["steps%d_sstm" % n], out["steps%d_entoc" % n] = a, b, e
        out["steps%d_omlscal" % n] = s
        if not seam:
            out["steps%d_scal" % n] = r.get_scalars()
    if seam:
        check_branches(name, out, cfg)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "written; convecting fraction after one call:", out["call_scal"][1])


if __name__ == "__main__":
    if len(sys.argv) > 1:
        make(sys.argv[1])
    else:
        for v in VARIANTS:  # one reference configuration per process (oracle/ref_binding.py)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), v])
