"""Timings of an atmosphere-only run with the atmosphere of cpl_natl5 (385 x 97, ndxr 16, the sea 60 x 60
cells = an SST of 960 x 960 points, no ocean handle) on cuda:0, printed as a log (profiles/atmos_only.log).  Host clock
around work that ends in a synchronise; the two variants of a comparison alternate in one process; medians.
  python3 profiles/tools/atmos_only.py    one synchronised xforc(None, a) without and with the heat half from the SST;
                                          atmos_only windows coupled_steps(None, a, ..., xforc=True) of 300 steps
                                          (nstr 3), per nstr = 3 steps
The radiation coefficients and the mixed-layer state are those of profiles/tools/heat.py."""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def model(sst_half):
    """The atmosphere of cpl_natl5 with xforc's momentum half set up without an ocean and the mixed layer on;
    sst_half: the heat half from a prescribed SST as well."""
    from common import atm_apply, cpl_fullsize_inputs, load_golden
    from qgcm_hip import AtmosModel, config, xforc_setup, xforc_sst_setup
    g = load_golden("cpl_natl5_sample")
    oc, at = config.preset("cpl_natl5"), config.atmos_preset("cpl_natl5")
    _, _, _, f = cpl_fullsize_inputs(g, oc, at)
    a = AtmosModel(at, ddynat=f["ddynat"])
    atm_apply(a, f)
    xforc_setup(None, a, ndxr=oc.ndxr, nxaooc=oc.nxaooc, nyaooc=oc.nyaooc)
    am = config.AmlConfig(tat=(30.0, 40.0), aface=(1.1e-6, -0.4e-6), bface=0.7e-6, cface=-0.3e-6, dface=2.3e-4)
    a.aml_init(am)
    x, y = (np.arange(at.nxta) + 0.5) / at.nxta, (np.arange(at.nyta) + 0.5) / at.nyta
    ast = np.asfortranarray(-5.0 + 6.0 * np.cos(np.pi * y)[None, :] + 1.5 * np.cos(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    hm = np.asfortranarray(1000.0 + 40.0 * np.sin(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    a.aml_set_state(ast, ast, hm, hm)
    if sst_half:
        ht = config.HeatConfig(D0up=6.5, Dmup=5.1, Dmdown=-5.6, Adown11=-4.7e-3, Bmup=8.9e-3, B1down=-3.1e-3, Cmup=-2.2e-3,
                               C1down=1.3e-3)
        yo = (np.arange(oc.nyto) + 0.5) / oc.nyto
        sst = np.asfortranarray(np.broadcast_to(4.0 * np.cos(np.pi * yo)[None, :], (oc.nxto, oc.nyto)))
        xforc_sst_setup(a, oc, ht, sst)
    return a, int(g["nstr"]), oc


def xforc_call():
    from qgcm_hip import xforc
    pairs = {"momentum": model(False), "sst": model(True)}

    def run(k):
        a = pairs[k][0]
        t0 = time.perf_counter()
        xforc(None, a)
        a.sync()
        return 1e6 * (time.perf_counter() - t0)

    for k in pairs:
        for _ in range(5):
            run(k)
    res = {k: [] for k in pairs}
    for _ in range(50):
        for k in pairs:
            res[k].append(run(k))
    p, m = np.median(res["momentum"]), np.median(res["sst"])
    oc = pairs["sst"][2]
    print("one synchronised xforc(None, a), us (median of 50, alternated): momentum half %.1f, with the heat half from the "
          "SST %.1f, difference %+.1f (3 launches added); the heat half's own bytes: the SST read = %.1f MB"
          % (p, m, m - p, oc.nxto * oc.nyto * 8 / 1e6), flush=True)
    for a, _, _ in pairs.values():
        a.close()


def windows():
    from qgcm_hip import coupled_steps, xforc_sst_get
    n = 300
    pairs = {"held": model(True), "atmos_only": model(True)}
    nstr = pairs["held"][1]
    nt0 = [1]

    def run(k):
        a = pairs[k][0]
        t0 = time.perf_counter()
        coupled_steps(None, a, nt0[0], n, nstr, xforc=(k == "atmos_only"))
        a.sync()
        return 1e6 * (time.perf_counter() - t0) / (n // nstr)

    for k in pairs:
        run(k)
    res = {k: [] for k in pairs}
    for _ in range(4):
        nt0[0] += n
        for k in pairs:
            res[k].append(run(k))
    p, m = np.median(res["held"]), np.median(res["atmos_only"])
    print("window of %d atmospheric steps (nstr %d, whole chip, aml on in both), us per nstr = %d steps: forcing held %.1f, "
          "atmos_only sequence xforc; (aml; qgastep; atinvq; atqzbd) x nstr %.1f, difference %+.1f; held %s, atmos_only %s" % (
              n, nstr, nstr, p, m, m - p, " ".join("%.1f" % v for v in res["held"]),
              " ".join("%.1f" % v for v in res["atmos_only"])), flush=True)
    for k, (a, _, _) in pairs.items():
        H = xforc_sst_get(a)
        print("  %s: state finite: %s; arlaav %.4f slhfav %.4f oradav %.4f arocav %.1f" % (
            k, bool(np.isfinite(a.get_state()[0]).all() and np.isfinite(a.aml_get_state()[0]).all()), H["arlaav"],
            H["slhfav"], H["oradav"], H["arocav"]))
        a.close()


if __name__ == "__main__":
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    xforc_call()
    windows()
