"""Timings of the ocean's time averages on cuda:0, printed as a log (profiles/time_means.log):
  python3 profiles/tools/time_means.py          step with the po sum off / on (alternated) at NAtl 5 km, SOcn 5 km and
                                                NAtl 1 km as eight y-slabs; tavocn and the readouts at NAtl 5 km
  python3 profiles/tools/time_means.py trace    a short eager run for rocprofv3 --kernel-trace --stats (named kernels)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from qgcm_hip import OceanModel, oml_preset, preset, synth  # noqa: E402


def ocean(name):
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
    m.set_time_mean_params(om)
    m.set_monitor_fields(tx, ty, wekto, sst)
    m.set_time_mean_fields(fnet)
    return m


def whole(name, n=500, reps=4):
    m = ocean(name)
    s = 1
    for on in (False, True):  # warm both graph sets
        m.enable_po_mean(on)
        m.time_steps(n, s0=s)
        s += n
    t = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            m.enable_po_mean(on)
            t[on].append(1e3 * m.time_steps(n, s0=s) / n)
            s += n
    off, on = np.median(t[False]), np.median(t[True])
    print("%-8s step, po sum off: %7.2f us  on: %7.2f us  (+%.2f us; medians of %d x %d steps, alternated; "
          "off %s, on %s)" % (name, off, on, on - off, reps, n, " ".join("%.2f" % x for x in t[False]),
                              " ".join("%.2f" % x for x in t[True])))
    return m


def slabs_natl1(n=20, reps=3):
    from qgcm_hip import hostinit
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("natl1")
    consts = global_consts(cfg)
    S = [HipSlab(cfg, consts, g0, g1, r, 8) for r, (g0, g1) in enumerate(partition(cfg.nypo, 8))]
    so = SlabOcean(cfg, S, LocalComm(8, after=torch.cuda.synchronize))
    so.homsol()
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    pom = np.asfortranarray(0.999 * po)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    so.scatter_state(po, pom, qo, qom, wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1),
                     hostinit.constr(cfg, consts["amatoc"], po, pom))
    so.steps(5)
    t = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            so.enable_po_mean(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            so.steps(n)
            for x in S:
                x.sync()
            t[on].append(1e6 * (time.perf_counter() - t0) / n)
    off, on = np.median(t[False]), np.median(t[True])
    print("natl1 as 8 virtual slabs on one GPU (Python-driven stages): basin step, po sum off: %.0f us  on: %.0f us  "
          "(+%.0f us = 8 slabs' k_poavg_add; medians of %d x %d steps)" % (off, on, on - off, reps, n))
    for x in S:
        x.close()


def calls_natl5(m, reps=20):
    m.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.tavocn()
    m.sync()
    print("natl5    tavocn: %.1f us per call (host clock, %d calls, synchronised)" % (1e6 * (time.perf_counter() - t0) / reps, reps))
    for what, fn in (("time_means() all 16 outputs", lambda: m.time_means()),
                     ("time_means(['uptpoc', 'vptpoc'])", lambda: m.time_means(["uptpoc", "vptpoc"])),
                     ("po_mean()", lambda: m.po_mean()),
                     ("get_state() for comparison", lambda: m.get_state())):
        fn()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        print("natl5    %-34s %.1f ms per call" % (what + ":", 1e3 * (time.perf_counter() - t0) / 3))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        m = ocean("natl5")
        m.enable_po_mean()
        m.profile_steps(50, s0=1)
        for _ in range(10):
            m.tavocn()
        m.time_means()
        m.po_mean()
        m.sync()
        sys.exit(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    m = whole("natl5")
    calls_natl5(m)
    m.close()
    whole("socn5").close()
    slabs_natl1()
