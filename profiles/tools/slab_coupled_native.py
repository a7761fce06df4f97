"""The coupled window on a y-slab ocean, driven from Python and by the library, at cpl_natl5 (atmosphere
385 x 97, ocean 961 x 961, ndxr 16; replicated xforc, both mixed layers and the heat half on) on ONE rank of cuda:0,
printed as a log (profiles/slab_coupled_native.log).  Three set-ups live side by side in one session and take turns,
eight timed windows each after one warm-up window each:
  python   SlabOcean.coupled_steps as the parent commit has it: stage calls from Python, a synchronise after each, the
           all-gathers host-staged (LocalComm)
  library  the same rank on a one-rank RCCL communicator after use_library_coupling(): qgcm_hip_slab_coupled_steps
  whole    the whole-domain coupled_steps on the same GPU: the floor
A window is 20 ocean steps (60 atmospheric steps, nstr 3), timed with HIP events: one recorded on the ocean's stream
and one on the atmosphere's in front of the window (after a device synchronise), one on each behind it; the time is the
longest of the four differences.  Medians and spreads (max - min); a gain counts when it clears three spreads.
With QGCM_HIP_LIB pointing at a build of the parent commit the script gives the parent's figures for `python` and
`whole` (its library has no library-driven window)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import slab_coupled as sc  # noqa: E402  (the inputs and set-ups of profiles/tools/slab_coupled.py; it extends sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

NOCEAN, RUNS = 20, 8


def stream_of(m):
    return torch.cuda.ExternalStream(m.L.qgcm_hip_stream(m.h), device=torch.device("cuda", torch.cuda.current_device()))


def timed(run, oc, at):
    """us per ocean step of run() between events on the two handles' streams."""
    so, sa = stream_of(oc), stream_of(at)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    ev[0].record(so)
    ev[1].record(sa)
    run()
    ev[2].record(so)
    ev[3].record(sa)
    torch.cuda.synchronize()
    return 1e3 * max(a.elapsed_time(b) for a in ev[:2] for b in ev[2:]) / NOCEAN


def main():
    from qgcm_hip import config, coupled_steps, xforc_heat_setup, xforc_setup
    from qgcm_hip.slab import global_consts, rccl_unique_id
    native_lib = not os.environ.get("QGCM_HIP_LIB")
    print("device: %s; library: %s" % (torch.cuda.get_device_name(0), "in-tree" if native_lib else "the build QGCM_HIP_LIB names"), flush=True)
    I = sc.inputs()
    nstr = I["nstr"]
    nwin = NOCEAN * nstr
    o, a = sc.ocean(I), sc.atmosphere(I)
    xforc_setup(o, a, tau_udiff=False)
    xforc_heat_setup(o, a, config.HeatConfig(**sc.HT))
    consts = global_consts(I["oc"], o.helmholtz)
    sets = {"whole": (o, a, lambda nt0: coupled_steps(o, a, nt0, nwin, nstr, xforc=True))}
    py, _, pyr = sc.slab_setup(I, consts, 1)
    sets["python"] = (py.slabs[0], pyr[0], lambda nt0: py.coupled_steps(nt0, nwin, nstr, xforc=True))
    has = hasattr(o.L, "qgcm_hip_slab_coupled_steps")
    if has:
        nat, _, natr = sc.slab_setup(I, consts, 1)
        nat.use_library_exchanges(rccl_unique_id())
        nat.slabs[0].sync_each_call = False
        nat.use_library_coupling()
        sets["library"] = (nat.slabs[0], natr[0], lambda nt0: nat.coupled_steps(nt0, nwin, nstr, xforc=True))
        sw = dict(oml=True, heat=True, xforc_len=nat.slabs[0].xforc_msg_len(natr[0]), oml_len=nat.slabs[0].oml_len,
                  summary_len=nat.slabs[0].th_len, halo_len=nat.slabs[0].halo_len)
        from qgcm_hip.lib import slab_coupled_plan
        plan = slab_coupled_plan(1, 1, nwin, nstr, True, **sw)
        print("the library's plan of one window: %d operations, %d of them all-gathers (%s doubles per rank)"
              % (len(plan), sum(1 for n, _ in plan if n.startswith("gather_")),
                 ", ".join("%s %d" % (n, ln) for n, ln in sorted(set(e for e in plan if e[0].startswith("gather_"))))), flush=True)
    order = [k for k in ("python", "library", "whole") if k in sets]
    t = {k: [] for k in order}
    nt0 = 1
    for rnd in range(RUNS + 1):  # (round 0: the warm-up windows - graph capture, first launches)
        for k in order:
            oc, at, run = sets[k]
            us = timed(lambda: run(nt0), oc, at)
            if rnd:
                t[k].append(us)
        nt0 += nwin
    for k in order:
        v = t[k]
        print("%-7s window of %d ocean steps (%d atmospheric, nstr %d), us per ocean step: median %.1f, spread %.1f (%s)"
              % (k, NOCEAN, nwin, nstr, float(np.median(v)), max(v) - min(v), " ".join("%.1f" % x for x in v)), flush=True)
    if has:
        st = [np.array(x) for x in sets["library"][0].get_state()]
        ref = [np.array(x) for x in sets["python"][0].get_state()]
        whole = [np.array(x) for x in o.get_state()]
        eq = lambda p, q: all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(p, q))
        print("after %d windows: the library's ocean state finite: %s; bitwise the Python-driven one: %s; bitwise the whole domain's: %s"
              % (RUNS + 1, all(np.isfinite(x).all() for x in st), eq(st, ref), eq(st, whole)), flush=True)
        mp, ml, mw = (float(np.median(t[k])) for k in ("python", "library", "whole"))
        sp = max(max(t[k]) - min(t[k]) for k in ("python", "library"))
        print("library against python: %.1f us per ocean step less (%.1f %%), the larger spread of the two %.1f: %s three spreads; "
              "left to the whole-domain window: %.1f us" % (mp - ml, 100.0 * (mp - ml) / mp, sp,
                                                            "clears" if mp - ml > 3.0 * sp else "does NOT clear", ml - mw), flush=True)
    for k in order:
        for m in sets[k][:2]:
            m.close()


if __name__ == "__main__":
    main()
