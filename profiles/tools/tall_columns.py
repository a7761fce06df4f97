"""NAtl 1 km (4801 x 4801 x 3, dto = 180 s) as ONE whole-domain handle, its column of 4799 interior rows solved in segments
(DESIGN 3.3b); printed as a log (profiles/tall_columns.log).
  python3 profiles/tools/tall_columns.py check          OceanModel(preset("natl1")) - hostinit and homsol through the
                                                        segmented solver - and two steps against the TRUE reference's
                                                        sample tests/golden/natl1_sample.npz (every 64th row / column),
                                                        compared as test_full_size_natl1_eight_slabs_vs_reference_sample
                                                        does: 1e-11 of each field's maximum, 1e-12 on the constraint scalars
  python3 profiles/tools/tall_columns.py time [N ...]   time per step, HIP events over graph-replayed steps as bench.py
                                                        brackets them (5 windows of 20 steps each, no averaging step), and
                                                        the per-kernel times of 20 eager steps, for every maximum segment
                                                        length N (QGCM_HIP_THOMAS_SEG_ROWS; default 2048 1024 640)
  python3 profiles/tools/tall_columns.py slabs          the same basin as eight y-slabs: bench.py's figure of one middle
                                                        slab stepping alone; x 8 is an EXTRAPOLATION to the eight slabs one
                                                        after the other on one GPU, without the two exchanges (the basin
                                                        stepped as eight virtual slabs is not timed here)"""
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401


def inputs(cfg):
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    return po, wek


def model(cfg, seg_rows=None, consts=None):
    from qgcm_hip import OceanModel, lib
    if seg_rows:
        os.environ["QGCM_HIP_THOMAS_SEG_ROWS"] = str(seg_rows)  # read by qgcm_hip_set_grid
    else:
        os.environ.pop("QGCM_HIP_THOMAS_SEG_ROWS", None)
    t0 = time.perf_counter()
    m = OceanModel(cfg, consts=consts)
    plan = [n for _, n in lib.thomas_segments(cfg.nypo - 2, seg_rows or 0)]
    print("handle: max segment %s -> %d segments of %d..%d rows, set-up %.1f s%s" % (
        seg_rows or "default", len(plan), min(plan), max(plan), time.perf_counter() - t0,
        " (constants reused)" if consts else " (hostinit + homsol on the device solver)"), flush=True)
    return m


def all_consts(m):
    c = dict(amatoc=m.amatoc, rdm2oc=m.rdm2oc, ctl2moc=m.ctl2moc, ctm2loc=m.ctm2loc)
    c.update(m.homog)
    return c


def check():
    from common import FIELDS, load_golden
    from qgcm_hip import preset
    cfg = preset("natl1")
    g = load_golden("natl1_sample")
    st = int(g["stride"])
    po, wek = inputs(cfg)
    assert np.array_equal(po[::st, ::st], g["in_po"]) and np.array_equal(wek[::st, ::st], g["in_wekpo"])
    m = model(cfg)
    ok = True
    try:
        m.set_p(po, po)
        m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        for s in (1, 2):
            m.steps(1, s0=s)
            worst = {f: float(np.abs(x[::st, ::st, :] - g["steps%d_%s" % (s, f)]).max() / float(g["steps%d_%s_max" % (s, f)]))
                     for f, x in zip(FIELDS, m.get_state())}
            sm, sr = m.get_scalars(), g["steps%d_scal" % s]
            n1 = 2 * (cfg.nlo - 1)
            se = float(np.abs(sm[:n1] - sr[:n1]).max() / (cfg.xlo * cfg.ylo * float(g["steps%d_po_max" % s])))
            good = all(v < 1e-11 for v in worst.values()) and se < 1e-12
            ok = ok and good
            print("step %d vs the reference sample: %s constraint scalars %.3e -> %s" % (
                s, {f: "%.3e" % v for f, v in worst.items()}, se, "within 1e-11 / 1e-12" if good else "OUTSIDE the bounds"), flush=True)
    finally:
        m.close()
    return 0 if ok else 1


def timing(lengths):
    from qgcm_hip import preset
    cfg = preset("natl1")
    po, wek = inputs(cfg)
    consts = None
    for n in lengths:
        m = model(cfg, n, consts)
        try:
            consts = consts or all_consts(m)
            m.set_p(po, po)
            m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
            m.steps(45, s0=1)          # steps 1 and 26 average; windows below: steps 2 .. 25 + k 25 never do
            s0, wins = 52, []
            for _ in range(5):         # 20-step windows between averaging steps (52..71, 77..96, ...)
                m.steps(20, s0=s0)     # rehearsal: the graphs of this phase exist
                wins.append(1e3 * m.time_steps(20, s0=s0) / 20)
                s0 += 25
            pr = m.profile_steps(20, s0=s0)
            fin = bool(np.isfinite(m.get_state()[0]).all())
            print("max segment %d: us per step, 5 windows of 20 graph-replayed steps: %s  median %.1f  state finite: %s" % (
                n, " ".join("%.1f" % w for w in wins), float(np.median(wins)), fin), flush=True)
            print("   eager per-kernel us per launch (HIP-event brackets, bracket cost included): " + ", ".join(
                "%s %.1f (x%d)" % (k, 1e3 * ms / max(c, 1), c) for k, (ms, c) in sorted(pr.items()) if c and not k.startswith("k_noop")), flush=True)
        finally:
            m.close()
    return 0


def slabs():
    import bench
    r = bench.natl1_one_slab_figure(0)
    print("eight y-slabs, one middle slab alone: " + json.dumps(r), flush=True)
    print("   x 8 slabs = %.1f us per step of the whole basin (extrapolated from the one slab; exchanges not included)" % (8 * r["us_per_step_one_slab_alone"]), flush=True)
    return 0


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "check"
    if what == "check":
        sys.exit(check())
    if what == "time":
        sys.exit(timing([int(a) for a in sys.argv[2:]] or [2048, 1024, 640]))
    if what == "slabs":
        sys.exit(slabs())
    sys.exit("usage: tall_columns.py check | time [N ...] | slabs")
