"""Timings of the momentum half of xforc at cpl_natl5 (atmosphere 385 x 97, ocean 961 x 961, ndxr 16) on
cuda:0, printed as a log (profiles/xforc.log):
  python3 profiles/tools/xforc.py          one synchronised xforc() call and back-to-back calls (host clock around work
                                           that ends in a synchronise); the bytes the design moves; coupled windows of
                                           300 atmospheric steps (100 ocean steps) with xforc on and with the forcing
                                           held (the path without this feature), alternated, CU ranges as bench.py
  python3 profiles/tools/xforc.py trace    a short run for rocprofv3 --kernel-trace --stats (named kernels)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def models(setup=True, share=False):
    from common import atm_apply, cpl_fullsize_inputs, load_golden
    from qgcm_hip import AtmosModel, OceanModel, config, share_gpu, xforc_setup
    g = load_golden("cpl_natl5_sample")
    oc, at = config.preset("cpl_natl5"), config.atmos_preset("cpl_natl5")
    po, pom, wekpo, f = cpl_fullsize_inputs(g, oc, at)
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(po, pom)
    o.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(oc.nlo - 1))
    atm_apply(a, f)
    if setup:
        xforc_setup(o, a, tau_udiff=True)
    if share:
        share_gpu(o, a)
    return o, a, int(g["nstr"])


def one_call():
    from qgcm_hip import xforc
    o, a, _ = models()
    oc, at = o.cfg, a.cfg
    for _ in range(5):
        xforc(o, a)
    a.sync()
    o.sync()
    sync_us = []
    for _ in range(50):
        t0 = time.perf_counter()
        xforc(o, a)
        a.sync()
        sync_us.append(1e6 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    for _ in range(50):
        xforc(o, a)
    a.sync()
    b2b = 1e6 * (time.perf_counter() - t0) / 50
    print("one synchronised xforc(): median %.1f us, min %.1f, max %.1f (50 calls); back to back %.1f us per call"
          % (np.median(sync_us), min(sync_us), max(sync_us), b2b), flush=True)
    nfine = (at.nxta * oc.ndxr + 1) * (at.nyta * oc.ndxr + 1) * 8
    nocn = oc.nxpo * oc.nypo * 8
    print("bytes: one ocean p field %.2f MB (pom(:,:,1) read; tauxo, tauyo, wekto, wekpo written: 5 fields = %.1f MB "
          "unavoidable); one fine field %.1f MB; materialised: tauxaor, tauyaor (written by k_xf_fine, read by "
          "k_xf_wektaor, k_xf_atm, k_xf_tauo, k_xf_lines) and wektaor (written once, read by k_xf_wekpa)"
          % (nocn / 1e6, 5 * nocn / 1e6, nfine / 1e6))
    print("k_xf_fine's own bytes: 2 fine fields written + pom read = %.1f MB (the weight tables, 5 x %d KB, stay in L2)"
          % ((2 * nfine + nocn) / 1e6, 16 * (oc.ndxr + 1) * oc.ndxr * 8 // 1024), flush=True)
    o.close()
    a.close()


def windows():
    from qgcm_hip import coupled_steps
    n = 300
    pairs = {"held": models(setup=True, share=True), "xforc": models(setup=True, share=True)}
    nstr = pairs["held"][2]
    nt0 = 1
    for key, (o, a, _) in pairs.items():  # warm-up: the graphs of the window's blocks
        coupled_steps(o, a, nt0, n, nstr, xforc=(key == "xforc"))
        o.sync()
        a.sync()
    res = {"held": [], "xforc": []}
    for _ in range(4):
        nt0 += n
        for key, (o, a, _) in pairs.items():
            t0 = time.perf_counter()
            coupled_steps(o, a, nt0, n, nstr, xforc=(key == "xforc"))
            o.sync()
            a.sync()
            res[key].append(1e6 * (time.perf_counter() - t0) / (n // nstr))
    h, x = np.median(res["held"]), np.median(res["xforc"])
    print("coupled window of %d atmospheric steps (nstr %d, CU ranges of share_gpu), us per ocean step: forcing held "
          "%.1f, xforc on %.1f, difference %+.1f; held %s, xforc %s" % (
              n, nstr, h, x, x - h, " ".join("%.1f" % v for v in res["held"]), " ".join("%.1f" % v for v in res["xforc"])),
          flush=True)
    for key, (o, a, _) in pairs.items():
        print("  %s: state finite: %s" % (key, bool(np.isfinite(o.get_state()[0]).all() and np.isfinite(a.get_state()[0]).all())))
        o.close()
        a.close()


def trace():
    from qgcm_hip import xforc
    o, a, _ = models()
    for _ in range(20):
        xforc(o, a)
    a.sync()
    o.close()
    a.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        print("device: %s" % torch.cuda.get_device_name(0), flush=True)
        one_call()
        windows()
