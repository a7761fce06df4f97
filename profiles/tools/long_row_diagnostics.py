"""The cost of monitors() (qgcm_hip_monitors: k_mon_scan, k_mon_jet, k_mon_final, one copy back) on cuda:0, printed as
log lines (profiles/long_row_diagnostics.log):
  python3 profiles/tools/long_row_diagnostics.py LABEL CASE [CASE ...]
CASE: a preset's name (natl5, socn5) or long<nxto> (the thin channel of tests/test_gpu_long_rows.long_cfg: nxto + 1
columns, 33 rows, 3 layers).  Per case: the state of tests/test_gpu_monitors.setup without the mixed layer, 10 steps,
then REPS synchronised calls of monitors() from Python after a warm-up; the median with the 10th and 90th percentile.
One process per library: QGCM_HIP_LIB selects a parent build under this commit's binding, LABEL names it in the line."""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
for p in (os.path.join(ROOT, "q-gcm_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_gpu_monitors as tm  # noqa: E402
from test_gpu_long_rows import long_cfg  # noqa: E402

REPS = 300


def run(label, case):
    cfg = long_cfg(int(case[4:])) if case.startswith("long") else case
    m, om, f = tm.setup(cfg, False)
    try:
        m.steps(10, s0=1)
        m.sync()
        for _ in range(20):
            m.monitor_vector()
        t = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            m.monitor_vector()
            t.append(time.perf_counter() - t0)
        v = m.monitors()
        print("%-7s %-10s %6d x %4d x %d  rows %d x %d  monitors() %8.1f us  [%8.1f, %8.1f]  (median [p10, p90] of %d)  ocjpos %s ocjval %s" % (
            label, case, m.cfg.nxpo, m.cfg.nypo, m.cfg.nlo, *m.row_plan(), 1e6 * np.median(t), 1e6 * np.percentile(t, 10),
            1e6 * np.percentile(t, 90), REPS, v["ocjpos"].astype(int).tolist(), np.array2string(v["ocjval"], precision=6)), flush=True)
    finally:
        m.close()


if __name__ == "__main__":
    for c in sys.argv[2:]:
        run(sys.argv[1], c)
