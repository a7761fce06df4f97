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
                                                        stepped as eight virtual slabs is not timed here)
  python3 profiles/tools/tall_columns.py slab [P:N,.. ...] the same basin as P y-slabs (2: 2400-row slabs, in segments; 3 / 4:
                                                        1600 / 1200 rows), ONE middle slab stepping alone as run_workload.py
                                                        natl1_one_slab sets it up (the other ranks' summaries and halo rows
                                                        held at the last real step), for every QGCM_HIP_THOMAS_SLAB_SEG_ROWS
                                                        = N (0: unset): 20-step windows replayed from a graph, HIP events,
                                                        the state restored before every replay; then HIP-event brackets
                                                        around the launches of each Thomas phase, eager (profiles/tall_slabs.log).
                                                        One GPU: what one rank computes per step, no exchange - not a scaling
                                                        measurement"""
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


def one_slab(groups):
    from qgcm_hip import hostinit, preset, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("natl1")
    consts = global_consts(cfg)
    po = synth.gaussian_eddy(cfg)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    scal = hostinit.constr(cfg, consts["amatoc"], po, po)
    z2 = np.zeros_like(wek)
    for nranks, n in ((p, n) for p, lengths in groups for n in lengths):
        r = nranks // 2
        if n:
            os.environ["QGCM_HIP_THOMAS_SLAB_SEG_ROWS"] = str(n)  # read by qgcm_hip_set_grid
        else:
            os.environ.pop("QGCM_HIP_THOMAS_SLAB_SEG_ROWS", None)
        slabs = [HipSlab(cfg, consts, g0, g1, k, nranks, sync_each_call=True) for k, (g0, g1) in enumerate(partition(cfg.nypo, nranks))]
        try:
            x = slabs[r]
            plan = [c for _, c in x.thomas_plan()]
            so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
            so.homsol()
            so.scatter_state(po, po, qo, qo, wek, z2, np.zeros(cfg.nlo - 1), scal)
            so.steps(4, s0=1)          # real steps of all slabs: the exchange buffers hold consistent values
            torch.cuda.synchronize()
            x.sync_each_call = False
            st = torch.cuda.ExternalStream(x.stream_ptr)
            mine = so.th_gath[r][r * x.th_len:(r + 1) * x.th_len]
            state0, scal0 = x.get_state(), x.get_scalars()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                for _ in range(20):    # the stages of SlabOcean.step for this slab alone (steps without an averaging)
                    x.stage(1, so.th_send[r])
                    mine.copy_(so.th_send[r])   # its own summary is current, the other ranks' stay at the last real step
                    x.stage(2, so.th_gath[r], so.h_to_lo[r], so.h_to_hi[r])
                    x.stage(3, so.h_from_lo[r], so.h_from_hi[r], None, 0)
            e0, e1, wins = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), []
            for rep in range(6):       # the first replay is a rehearsal
                x.set_state(*state0)
                x.set_scalars(scal0)
                with torch.cuda.stream(st):
                    e0.record()
                    gr.replay()
                    e1.record()
                e1.synchronize()
                if rep:
                    wins.append(1e3 * e0.elapsed_time(e1) / 20)
            # the solve alone, eager: HIP events around the launches of each phase (what the work array holds does not
            # change what the launches do)
            x.set_state(*state0)
            x.set_scalars(scal0)
            ph = {1: [], 2: []}
            with torch.cuda.stream(st):
                for rep in range(21):
                    for phase in (1, 2):
                        e0.record()
                        x.thomas_phase(phase, so.th_gath[r] if phase == 2 else None, so.th_send[r] if phase == 1 else None)
                        e1.record()
                        e1.synchronize()
                        if rep:
                            ph[phase].append(1e3 * e0.elapsed_time(e1))
            print("%d slabs, slab %d (rows %d..%d) alone, max segment %s -> %d segment(s) of %d..%d rows: us per step, 5 windows "
                  "of 20 graph-replayed steps: %s  median %.1f" % (nranks, r, x.g0, x.g1, n or "unset", len(plan), min(plan), max(plan),
                                                                  " ".join("%.1f" % w for w in wins), float(np.median(wins))), flush=True)
            print("   eager HIP-event brackets (bracket cost included), median of 20: phase 1 (%s) %.1f us, phase 2 (%s) %.1f us" % (
                "k_thomas_seg + k_thomas_fold" if len(plan) > 1 else "k_thomas<R, 1>", float(np.median(ph[1])),
                "k_thomas_corr_slab" if len(plan) > 1 else "k_thomas_corr", float(np.median(ph[2]))), flush=True)
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_stream(torch.cuda.default_stream())
            for sl in slabs:
                sl.close()
    return 0


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "check"
    if what == "check":
        sys.exit(check())
    if what == "time":
        sys.exit(timing([int(a) for a in sys.argv[2:]] or [2048, 1024, 640]))
    if what == "slabs":
        sys.exit(slabs())
    if what == "slab":
        groups = [(int(a.split(":")[0]), [int(n) for n in a.split(":")[1].split(",")]) for a in sys.argv[2:]]
        sys.exit(one_slab(groups or [(2, [2048, 1024, 640])]))
    sys.exit("usage: tall_columns.py check | time [N ...] | slabs | slab [P:N,N,... ...]")
