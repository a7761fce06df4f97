"""Timings of the area averages and the CFL check on cuda:0, printed as a log (profiles/areacfl.log):
  python3 profiles/tools/areacfl.py
area_averages() with the reference's five sample areas (src/areas.limits) and cfl(), each as a synchronised call from
Python, next to monitors() and to the pulls they replace - get_state() plus oml_get_state() - alternated in one process;
medians with the 10th and 90th percentile.  natl5 with the mixed layer on, then the atmosphere of cpl_natl5."""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
for p in (os.path.join(ROOT, "q-gcm_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_gpu_monitors as tm  # noqa: E402
import test_gpu_atm_monitors as ta  # noqa: E402

REPS = 40
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def med(fns):
    t = {k: [] for k in fns}
    for k, f in fns.items():  # warm up
        f(); f()
    for _ in range(REPS):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    return {k: (1e6 * np.median(v), 1e6 * np.percentile(v, 10), 1e6 * np.percentile(v, 90)) for k, v in t.items()}


# the reference's five sample areas (src/areas.limits)
OC = ([0.0, 400.0e3, 0.0, 400.0e3, 200.0e3], [400.0e3, 800.0e3, 400.0e3, 800.0e3, 600.0e3],
      [0.0, 0.0, 400.0e3, 400.0e3, 200.0e3], [400.0e3, 400.0e3, 800.0e3, 800.0e3, 600.0e3])
AT = ([0.0, 7680.0e3, 15360.0e3, 23040.0e3, 12960.0e3], [7680.0e3, 15360.0e3, 23040.0e3, 30720.0e3, 17760.0e3],
      [1440.0e3] * 5, [6240.0e3] * 5)

m, om, f = tm.setup("natl5", True)
m.set_areas(*OC)
m.steps(30, s0=1)
m.sync()
# (the pulls first and a bare synchronise after them: whatever the runtime still does on the host after a large copy
#  to pageable memory falls into the spacer, not into the next variant)
r = med({"pull sst (oml_get_state)": m.oml_get_state, "pull po.. (get_state)": m.get_state, "sync (spacer)": m.sync,
         "monitors": m.monitors, "area_averages": m.area_averages, "cfl": m.cfl})
r2 = med({"area_averages": m.area_averages, "cfl": m.cfl})
say("natl5, mixed layer on, 961 x 961 x 3 (synchronised calls from Python, median [p10, p90] of %d, alternated):" % REPS)
for k, v in r.items():
    say("  %-28s %10.1f us  [%9.1f, %9.1f]" % (k, *v))
say("the two calls alone, alternated:")
for k, v in r2.items():
    say("  %-28s %10.1f us  [%9.1f, %9.1f]" % (k, *v))
say("  area averages: %s" % np.array2string(m.area_averages(), precision=6))
c = m.cfl()
say("  cfl courant: %s nbad %s" % (np.array2string(c["courant"], precision=4), c["nbad"]))
m.close()

a, fl, cc = ta.full_size_atmos()
a.set_areas(*AT)
a.steps(10, s0=1)
a.sync()


r = med({"pull pa.. (get_state)": a.get_state, "sync (spacer)": a.sync, "monitors": a.monitors,
         "area_averages": a.area_averages, "cfl": a.cfl})
say("cpl_natl5 atmosphere, 385 x 97 x 3 (ast from the setter: without aml a host holds it already; the pull that\n"
    "cfl() replaces is get_state()):")
for k, v in r.items():
    say("  %-28s %10.1f us  [%9.1f, %9.1f]" % (k, *v))
a.close()
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
