"""Timings of the atmosphere's time averages and periodic dump at cpl_natl5 (385 x 97 x 3) on cuda:0,
printed as a log (profiles/atm_tavg.log):
  python3 profiles/tools/atm_tavg.py          tavatm(), time_means(), atmos_dump(), get_state() (host clock, each call
                                              synchronised; medians) and a 2400-step coupled window with and without
                                              the coupled examples' schedule (every 120, phase 60), alternated
  python3 profiles/tools/atm_tavg.py trace    a short run for rocprofv3 --kernel-trace --stats (named kernels)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from qgcm_hip import coupled_steps, share_gpu  # noqa: E402


def atmos():
    from test_gpu_atm_tavg import atmos as a
    return a()[0]


def timed(fn, n, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t = 1e6 * np.array(t)
    return np.median(t), np.percentile(t, 10), np.percentile(t, 90), n


def calls():
    m = atmos()
    m.steps(20, s0=1)

    def tav():
        m.tavatm()
        m.sync()
    r = [("tavatm() + sync", timed(tav, 400, 20)),
         ("time_means() all 15 outputs", timed(lambda: m.time_means(), 50)),
         ("time_means(['uptpat', 'vptpat'])", timed(lambda: m.time_means(["uptpat", "vptpat"]), 100)),
         ("atmos_dump(nska=1)", timed(lambda: m.atmos_dump(1), 100)),
         ("atmos_dump(nska=2)", timed(lambda: m.atmos_dump(2), 100)),
         ("get_state() for comparison", timed(lambda: m.get_state(), 100))]
    for name, (med, p10, p90, n) in r:
        print("cpl_natl5 atmosphere  %-34s %8.1f us per call (median of %d; p10 %.1f, p90 %.1f)" % (name, med, n, p10, p90))
    m.close()


def coupled(reps=4, n=2400, nstr=3):
    import test_gpu_monitors as om
    o, _, _ = om.setup("cpl_natl5", False)
    a = atmos()
    share_gpu(o, a)
    nt = 1
    res = {False: [], True: []}

    def window(on):
        nonlocal nt
        a.schedule_time_means(120 if on else 0, 60)
        o.sync()
        a.sync()
        t0 = time.perf_counter()
        coupled_steps(o, a, nt, n, nstr)
        o.sync()
        a.sync()
        nt += n
        return 1e6 * (time.perf_counter() - t0) / (n // nstr)
    for on in (False, True):  # graphs of both cut patterns built outside the timed windows
        window(on)
    for _ in range(reps):
        for on in (False, True):
            res[on].append(window(on))
    off, on = np.median(res[False]), np.median(res[True])
    print("cpl_natl5 coupled window of %d atmosphere steps (CU split %d), us per ocean step: no schedule %.2f, "
          "schedule every 120 phase 60 (%d contributions) %.2f, difference %+.2f; off %s, on %s"
          % (n, share_gpu(o, a), off, n // 120, on, on - off, " ".join("%.2f" % x for x in res[False]),
             " ".join("%.2f" % x for x in res[True])))
    print("  nsumat after the runs: %d" % a.time_means(["txatav"])["nsumat"])
    o.close()
    a.close()


def trace():
    m = atmos()
    m.steps(20, s0=1)
    for _ in range(200):
        m.tavatm()
    m.sync()
    m.time_means()
    m.time_means(["uptpat", "vptpat"])
    m.atmos_dump(1)
    m.atmos_dump(2)
    m.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        print("device: %s" % torch.cuda.get_device_name(0))
        calls()
        coupled()
