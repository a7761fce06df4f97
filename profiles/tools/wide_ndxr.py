"""xforc at cpl_natl1 (atmosphere 385 x 97, ocean 4801 x 4801, ndxr 80) as one handle pair on cuda:0, with
tau_udiff and the heat half on, printed as a log (profiles/wide_ndxr.log).  Host clock around work that ends in a
synchronise.
  python3 profiles/tools/wide_ndxr.py          one synchronised xforc(), median of 50, with the box average in its plain
                                               and in its staged form (QGCM_HIP_XF_WEKPA_STAGE = 0 / 1 at the set-up of two
                                               atmospheres above the one ocean), alternated, eight rounds; the device
                                               memory of the handles; a coupled window per ocean step with xforc=True
  python3 profiles/tools/wide_ndxr.py trace    a short run for rocprofv3 --kernel-trace --stats (named kernels), the
                                               form of the box average taken from the environment
The radiation coefficients are those of profiles/tools/heat.py; the pressures are qgcm_hip.synth's."""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

VAR = "QGCM_HIP_XF_WEKPA_STAGE"
NSTR = 3


def ocean():
    from qgcm_hip import OceanModel, config, oml_preset, synth
    oc = config.preset("cpl_natl1")
    po = synth.gaussian_eddy(oc, noise=1.0e-3)
    o = OceanModel(oc)
    o.set_p(po, np.asfortranarray(0.98 * po))
    del po
    zp = np.zeros((oc.nxpo, oc.nypo), order="F")
    o.set_forcing(zp, zp.copy(order="F"), np.zeros(oc.nlo - 1))
    o.oml_init(oml_preset(oc))
    yo = (np.arange(oc.nyto) + 0.5) / oc.nyto
    sst = np.asfortranarray(np.broadcast_to(4.0 * np.cos(np.pi * yo)[None, :], (oc.nxto, oc.nyto)))
    o.oml_set_state(sst=sst, sstm=sst)
    return o


def atmosphere(o, stage):
    """An atmosphere above `o` with both halves of xforc set up; stage: the variable's value at the set-up (None: unset)."""
    from qgcm_hip import AtmosModel, config, synth, xforc_heat_setup, xforc_setup
    at = config.atmos_preset("cpl_natl1")
    f = synth.atmos_fields(at)
    a = AtmosModel(at, ddynat=f["ddynat"])
    a.set_p(f["pa"], f["pam"])
    a.set_forcing(f["wekpa"], f["entat"], f["xan"], float(f["txis"]), float(f["txin"]), f["enis"], f["enin"])
    old = os.environ.get(VAR)
    if stage is not None:
        os.environ[VAR] = stage
    try:
        xforc_setup(o, a, tau_udiff=True)
    finally:
        if stage is not None:
            if old is None:
                del os.environ[VAR]
            else:
                os.environ[VAR] = old
    am = config.AmlConfig(tat=(30.0, 40.0), aface=(1.1e-6, -0.4e-6), bface=0.7e-6, cface=-0.3e-6, dface=2.3e-4)
    ht = config.HeatConfig(D0up=6.5, Dmup=5.1, Dmdown=-5.6, Adown11=-4.7e-3, Bmup=8.9e-3, B1down=-3.1e-3, Cmup=-2.2e-3, C1down=1.3e-3)
    a.aml_init(am)
    x, y = (np.arange(at.nxta) + 0.5) / at.nxta, (np.arange(at.nyta) + 0.5) / at.nyta
    ast = np.asfortranarray(-5.0 + 6.0 * np.cos(np.pi * y)[None, :] + 1.5 * np.cos(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    hm = np.asfortranarray(1000.0 + 40.0 * np.sin(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    a.aml_set_state(ast, ast, hm, hm)
    xforc_heat_setup(o, a, ht)
    return a


def mem(tag):
    from qgcm_hip import lib
    blocks, nbytes = lib.live_allocs()
    free, total = torch.cuda.mem_get_info()
    print("device memory %s: the library holds %.2f GB in %d blocks; the device reports %.2f of %.2f GB in use"
          % (tag, nbytes / 1e9, blocks, (total - free) / 1e9, total / 1e9), flush=True)
    return nbytes


def ab():
    from qgcm_hip import coupled_steps, share_gpu, xforc, xforc_get
    t0 = time.perf_counter()
    m0 = mem("before the handles")
    o = ocean()
    m1 = mem("with the ocean handle (mixed layer on)")
    A = {"0": atmosphere(o, "0")}
    m2 = mem("with one atmosphere handle (xforc's two halves set up)")
    A["1"] = atmosphere(o, "1")
    oc, at = o.cfg, A["0"].cfg
    print("the ocean handle %.2f GB; an atmosphere handle with xforc %.2f GB, of which the three fine arrays %.2f GB; set-up took %.0f s of host time"
          % ((m1 - m0) / 1e9, (m2 - m1) / 1e9, 3 * (at.nxta * oc.ndxr + 1) * (at.nyta * oc.ndxr + 1) * 8 / 1e9, time.perf_counter() - t0), flush=True)
    out = {}
    for k, a in A.items():
        for _ in range(5):
            xforc(o, a)
        a.sync()
        o.sync()
        out[k] = xforc_get(o, a, names=("wekpa", "wekpo", "tauxa"))
    same = all(np.array_equal(out["0"][f].view(np.int64), out["1"][f].view(np.int64)) for f in out["0"])
    print("wekpa, wekpo, tauxa of the two forms bit-equal: %s; wekpa finite %s, max |wekpa| %.3e" % (
        same, bool(np.isfinite(out["1"]["wekpa"]).all()), np.abs(out["1"]["wekpa"]).max()), flush=True)
    med = {"0": [], "1": []}
    for r in range(8):
        for k in ("0", "1"):
            a = A[k]
            us = []
            for _ in range(50):
                t0 = time.perf_counter()
                xforc(o, a)
                a.sync()
                us.append(1e6 * (time.perf_counter() - t0))
            med[k].append(float(np.median(us)))
    for k in ("0", "1"):
        print("one synchronised xforc(), %s=%s, median of 50 per round, us: %s; median of the rounds %.1f, spread (max - min) %.1f"
              % (VAR, k, " ".join("%.1f" % v for v in med[k]), np.median(med[k]), max(med[k]) - min(med[k])), flush=True)
    d = float(np.median(med["0"]) - np.median(med["1"]))
    sp = max(max(med[k]) - min(med[k]) for k in med)
    print("plain - staged = %+.1f us per call = %.1f spreads of %.1f us (the larger of the two)" % (d, d / sp if sp else float("inf"), sp), flush=True)
    # the coupled window on the default dispatch (a third atmosphere would cost another 5.7 GB: the staged one is the default's)
    a = atmosphere(o, None)
    A["default"] = a
    share_gpu(o, a)
    n, nt0 = 10 * NSTR, 1
    coupled_steps(o, a, nt0, n, NSTR, xforc=True)  # warm-up: the graphs of the window's blocks
    o.sync()
    a.sync()
    res = {True: [], False: []}
    for _ in range(3):
        for xf in (False, True):
            nt0 += n
            t0 = time.perf_counter()
            coupled_steps(o, a, nt0, n, NSTR, xforc=xf)
            o.sync()
            a.sync()
            res[xf].append(1e3 * (time.perf_counter() - t0) / (n // NSTR))
    print("coupled window of %d atmospheric steps (nstr %d, CU ranges of share_gpu), ms per ocean step: forcing held %s, xforc=True %s; "
          "medians %.2f and %.2f" % (n, NSTR, " ".join("%.2f" % v for v in res[False]), " ".join("%.2f" % v for v in res[True]),
                                     np.median(res[False]), np.median(res[True])), flush=True)
    print("  state finite after %d atmospheric steps: %s" % (nt0 + n - 1, bool(np.isfinite(o.get_state()[0]).all() and np.isfinite(a.get_state()[0]).all())),
          flush=True)
    mem("with the ocean and three atmosphere handles")
    for m in list(A.values()) + [o]:
        m.close()


def trace():
    from qgcm_hip import xforc
    o = ocean()
    a = atmosphere(o, None)
    for _ in range(10):
        xforc(o, a)
    a.sync()
    a.close()
    o.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        print("device: %s" % torch.cuda.get_device_name(0), flush=True)
        ab()
