"""Phase timeline of the row-band kernel k_tend_rows from in-kernel stamps (TR_STAMP, k_tend_rows.h).
build: the library with -DQG_STAMPS on k_tend_rows.hip ALONE (every translation unit would define its own stamp table):
       compile the five units to objects with the Makefile's flags, k_tend_rows.hip with -DQG_STAMPS added, link -shared.
run:   QGCM_HIP_LIB=/path/lib_stamps.so python profiles/tools/stamps_band.py [preset]   (from the repo root, on the GPU box)
Stamps (100 MHz clock, per workgroup): thread 0 = wave 0, which steps two strips at NAtl 5 km - 0 entry, 1 first strip
done, 2 last strip done (in front of the barrier); lane 0 of the first transform wave - 3 its strips done, 4 tables in
(in front of the barrier; a build of the parent commit stamps it behind the front half, where its tables are in), 5 past
the barrier, 9 front half done, 6 transform done, 7 stores issued, 8 stores drained."""
import ctypes as C, sys
sys.path.insert(0, "q-gcm_amd/python"); sys.path.insert(0, ".")
import numpy as np
from qgcm_hip import preset
from qgcm_hip.model import OceanModel
import bench
cfg = preset(sys.argv[1] if len(sys.argv) > 1 else "natl5")
po, wek = bench.synthetic_inputs(cfg)
m = OceanModel(cfg, device=0)
m.set_p(po, po); m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
m.steps(60, s0=1)
m.sync()
NK, NB, NS = 4, 4096, 12
labels = ["entry", "wave 0: first strip done", "wave 0: last strip done", "transform wave: strips done",
          "transform wave: tables in", "transform wave: past the barrier", "transform done", "stores issued", "stores drained", "front half done"]
buf = np.zeros((NK, NB, NS), dtype=np.int64)
get = m.L.qgcm_hip_debug_stamps_rows
get.argtypes = [C.c_void_p, C.c_size_t]
for rep in range(3):
    m.steps(20)  # one captured 20-step block: the stamps of its last step remain
    m.sync()
    assert get(buf.ctypes.data, buf.nbytes) == 0
    b = buf[3]
    live = (b[:, 0] > 0) & (b[:, 8] > 0)
    t0 = b[live, 0].min()
    print("== k_tend_rows, rep %d: %d workgroups stamped" % (rep, live.sum()))
    for i, lab in enumerate(labels):
        us = (b[live, i] - t0) / 100.0
        print("  %-34s min %6.2f  p10 %6.2f  med %6.2f  p90 %6.2f  max %6.2f us" % (lab, us.min(), np.percentile(us, 10), np.median(us), np.percentile(us, 90), us.max()))
    # per workgroup intervals
    def iv(a, c):
        return (b[live, c] - b[live, a]) / 100.0
    for name, a, c in (("first strip (entry -> 1)", 0, 1), ("second strip (1 -> 2)", 1, 2), ("transform wave's strip (entry -> 3)", 0, 3),
                       ("table loads, waited for (3 -> 4)", 3, 4), ("transform wave waits at the barrier (4 -> 5)", 4, 5),
                       ("last strip done -> transform wave past the barrier (2 -> 5)", 2, 5),
                       ("front half (5 -> 9)", 5, 9), ("back half (9 -> 6)", 9, 6), ("stores issued (6 -> 7)", 6, 7), ("stores drained (7 -> 8)", 7, 8),
                       ("workgroup (entry -> 8)", 0, 8)):
        d = iv(a, c)
        print("  interval %-60s min %6.2f  med %6.2f  p90 %6.2f  max %6.2f us" % (name, d.min(), np.median(d), np.percentile(d, 90), d.max()))
    if (buf[0][live] > 0).any():  # per wave (lane 0 of each): first strip done, all strips done, after the workgroup's entry
        for k, lab in ((1, "first strip done"), (0, "all strips done, at the barrier")):
            w = (buf[k][live][:, :12] - b[live, 0][:, None]) / 100.0
            print("  wave 0..11, %-32s med %s" % (lab, " ".join("%5.2f" % x for x in np.median(w, axis=0))))
        w = buf[0][live][:, :12]
        print("  last wave at the barrier: counts per wave %s" % np.bincount(w.argmax(axis=1), minlength=12).tolist())
        print("  the barrier opens (5) after the last wave's arrival: med %.2f us" % np.median((b[live, 5] - w.max(axis=1)) / 100.0))
    print("  kernel span (first entry -> last drain): %.2f us" % ((b[live, 8].max() - t0) / 100.0))
