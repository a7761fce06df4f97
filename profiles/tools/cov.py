"""Timings of the covariance matrices on cuda:0, printed as a log (profiles/cov.log):
  python3 profiles/tools/cov.py          one covocn at NAtl 5 km (nsi 16) and SOcn 5 km (nsi 16), one covatm at 385 x 97
                                         (nsi 2): HIP-event time of back-to-back contributions, the rank-1 update's
                                         GB/s (4 x 8 x nmat bytes: both matrices read and written) next to
                                         stream_mix_bandwidth(1, 1, one matrix's bytes), default and non-temporal
                                         loads / stores (QGCM_HIP_COV_NT=1) alternated; NAtl 5 km windows of 1000
                                         steps with and without a schedule every 25 steps, alternated
  python3 profiles/tools/cov.py trace    a short run for rocprofv3 --kernel-trace --stats (named kernels)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def ocean(name, nt):
    os.environ["QGCM_HIP_COV_NT"] = "1" if nt else "0"
    from test_gpu_tavg import ocean as mk
    m = mk(name, False)
    m.enable_covariance(16)
    return m


def atmos(nt):
    os.environ["QGCM_HIP_COV_NT"] = "1" if nt else "0"
    from test_gpu_atm_tavg import atmos as mk
    m = mk()[0]
    m.enable_covariance(2)
    return m


def per_call_us(m, add, n):
    """Host clock around n back-to-back contributions ending in a synchronise (the launches pipeline)."""
    for _ in range(3):
        add()
    m.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        add()
    m.sync()
    return 1e6 * (time.perf_counter() - t0) / n


def contributions():
    out = []
    for label, mk, add, n in (("NAtl 5 km covocn nsi 16", lambda nt: ocean("natl5", nt), "covocn", 200),
                              ("SOcn 5 km covocn nsi 16", lambda nt: ocean("socn5", nt), "covocn", 50),
                              ("385x97 covatm nsi 2", atmos, "covatm", 50)):
        ms = [mk(False), mk(True)]
        sz = ms[0].covariance_size()
        mat = 8 * sz["nmat"]
        bw = ms[0].stream_mix_bandwidth(1, 1, mat)
        res = {False: [], True: []}
        for _ in range(3):
            for nt, m in zip((False, True), ms):
                res[nt].append(per_call_us(m, getattr(m, add), n))
        for nt in (False, True):
            us = float(np.median(res[nt]))
            print("%-26s nvar %6d  %7.1f MB per matrix  %s  %8.1f us per call (median of 3 x %d; %s)  = %6.0f GB/s "
                  "for 4 x matrix bytes; stream_mix(1,1) %6.0f GB/s" %
                  (label, sz["nvar"], mat / 1e6, "nt     " if nt else "default", us, n,
                   " ".join("%.1f" % x for x in res[nt]), 4 * mat / (us * 1e-6) / 1e9, bw), flush=True)
        for m in ms:
            m.close()


def schedule_cost():
    os.environ["QGCM_HIP_COV_NT"] = "0"
    from test_gpu_tavg import ocean as mk
    a, b = mk("natl5", False), mk("natl5", False)
    a.enable_covariance(16)
    a.schedule_covariance(25, 0)
    for m in (a, b):
        m.prepare_steps(1000, s0=1)
        m.steps(1000, s0=1)
        m.sync()
    res = {"off": [], "on": []}
    s0 = 1001
    for _ in range(4):
        for key, m in (("off", b), ("on", a)):
            m.prepare_steps(1000, s0=s0)
            t0 = time.perf_counter()
            m.steps(1000, s0=s0)
            m.sync()
            res[key].append(1e6 * (time.perf_counter() - t0) / 1000)
        s0 += 1000
    off, on = np.median(res["off"]), np.median(res["on"])
    print("NAtl 5 km window of 1000 steps, us per step: no schedule %.2f, schedule every 25 (40 contributions) %.2f, "
          "difference %+.2f; off %s, on %s" % (off, on, on - off, " ".join("%.2f" % x for x in res["off"]),
                                               " ".join("%.2f" % x for x in res["on"])))
    print("  nupo after the runs: %d" % a.covariance(0, 0)["nupo"])
    a.close()
    b.close()


def trace():
    for mk, add in ((lambda: ocean("natl5", False), "covocn"), (lambda: ocean("socn5", False), "covocn"),
                    (lambda: atmos(False), "covatm")):
        m = mk()
        for _ in range(20):
            getattr(m, add)()
        m.sync()
        m.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        print("device: %s" % torch.cuda.get_device_name(0), flush=True)
        contributions()
        schedule_cost()
