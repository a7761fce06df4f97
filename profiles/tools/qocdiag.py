"""Timings of the ocean's periodic dumps on cuda:0, printed as a log (profiles/qocdiag.log):
  python3 profiles/tools/qocdiag.py          call wall times of vorticity_budget / ocean_dump and the get_state pull at
                                             NAtl 5 km and SOcn 5 km; the step with a schedule whose dumps fall outside
                                             the window against none (alternated); the extra cost of a dump step
  python3 profiles/tools/qocdiag.py trace    a short run for rocprofv3 --kernel-trace --stats (k_qocdiag, k_ocnc_sample)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from qgcm_hip import OceanModel, oml_preset, preset, synth  # noqa: E402


def ocean(name, mixed_layer=True):
    cfg = preset(name)
    om = oml_preset(cfg)
    m = OceanModel(cfg)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    m.set_p(po, np.asfortranarray(0.999 * po))
    m.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(cfg.nlo - 1))
    if cfg.cyclic:
        txis, txin = synth.tau_line_integrals(cfg, tx)
        m.set_cyc_forcing(txis, txin, np.zeros(cfg.nlo - 1), np.zeros(cfg.nlo - 1))
    if mixed_layer:
        m.oml_init(om)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
    else:
        m.set_monitor_fields(tx, ty, wekto, sst)
    return m


def wall(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * np.median(t)


def calls(name):
    m = ocean(name)
    m.steps(26, s0=1)
    cfg = m.cfg
    for nsko in (1, 2):
        print("%s %dx%dx%d vorticity_budget(nsko=%d): %.3f ms per call (kernel + D2H + unpack)"
              % (name, cfg.nxpo, cfg.nypo, cfg.nlo, nsko, wall(lambda: m.vorticity_budget(nsko), 10), ))
    print("%s ocean_dump(nsko=1, all fields): %.3f ms per call" % (name, wall(lambda: m.ocean_dump(1), 10)))
    print("%s get_state() (po, pom, qo, qom pulled): %.3f ms per call" % (name, wall(m.get_state, 5)))
    m.close()


def paired(a, b, n, s0, reps, after=None):
    """HIP-event ms of n steps on handles a and b, alternated (each first in turn); the first pair warms up.
    Returns the median of a, of b, and the 10 / 50 / 90 % points of the paired differences a - b."""
    ta, tb, s = [], [], s0
    for r in range(2 * reps + 1):
        if r % 2:
            tb.append(b.time_steps(n, s0=s))
        ta.append(a.time_steps(n, s0=s))
        if after:
            after()
        if not r % 2:
            tb.append(b.time_steps(n, s0=s))
        s += n
    d = np.array(ta[1:]) - np.array(tb[1:])
    return np.median(ta[1:]), np.median(tb[1:]), np.percentile(d, [10, 50, 90])


def steps(name, reps=12):
    a, b = ocean(name), ocean(name)
    # a: schedule with dumps at 1, 10001, ..: none inside the windows that start at step 2
    a.schedule_vorticity_budget(1, 10000, capacity=1)
    a.steps(1, s0=1)
    a.read_vorticity_budgets()
    b.steps(1, s0=1)
    n = 200
    ta, tb, d = paired(a, b, n, 2, reps)
    print("%s step time, schedule set (no dump in window) %.2f us vs none %.2f us: %+.2f us per step"
          " (paired differences 10/50/90 %%: %+.2f / %+.2f / %+.2f us)"
          % (name, 1e3 * ta / n, 1e3 * tb / n, 1e3 * (ta - tb) / n, *(1e3 * d / n)))
    a.close()
    b.close()
    # the extra cost of dump steps against no schedule: every = 25 in 100-step windows (4 dumps, even gaps of 24 steps:
    # graphs only between them) and every = 26 in 104-step windows (4 dumps, odd gaps of 25: each gap also runs one
    # non-dump step eagerly)
    for nsko, every, n in ((1, 25, 100), (2, 25, 100), (2, 26, 104)):
        a, b = ocean(name), ocean(name)
        a.schedule_vorticity_budget(nsko, every, capacity=4)
        ta, tb, d = paired(a, b, n, 1, reps, after=a.read_vorticity_budgets)
        print("%s %d steps with 4 dump steps (nsko=%d, every=%d) %.3f ms vs none %.3f ms: %+.1f us per dump step"
              " (paired differences 10/50/90 %%: %+.1f / %+.1f / %+.1f us per dump step)"
              % (name, n, nsko, every, ta, tb, 1e3 * (ta - tb) / 4, *(1e3 * d / 4)))
        a.close()
        b.close()


def trace():
    for name in ("natl5", "socn5"):
        m = ocean(name)
        m.steps(3, s0=1)
        for nsko in (1, 2):
            for _ in range(5):
                m.vorticity_budget(nsko)
        for _ in range(5):
            m.ocean_dump(1)
        m.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        for name in ("natl5", "socn5"):
            calls(name)
            steps(name)
