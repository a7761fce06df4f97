"""Timings of the atmospheric mixed layer and of the heat half of xforc at cpl_natl5 (atmosphere 385 x 97,
ocean 961 x 961, ndxr 16) on cuda:0, printed as a log (profiles/heat.log).  Host clock around work that ends in a
synchronise; every comparison alternates the two variants in one process and reports medians.
  python3 profiles/tools/heat.py          one atmospheric step with aml set up against the same step without it; one
                                          synchronised xforc() with the heat half against the same call without it;
                                          coupled windows of 300 atmospheric steps (100 ocean steps, CU ranges as
                                          bench.py, the ocean's mixed layer on in both) with and without aml + heat
  python3 profiles/tools/heat.py trace    a short run for rocprofv3 --kernel-trace --stats (named kernels)
The radiation coefficients are those of the test fixtures (tests/golden/make_golden_heat.py: double-gyre magnitude);
the mixed-layer state is smooth and stays away from the convective branch, as a spun-up run does almost everywhere."""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def models(mixed, share=False):
    """cpl_natl5 with xforc's momentum half and the ocean's mixed layer; mixed: aml and the heat half as well."""
    from common import atm_apply, cpl_fullsize_inputs, load_golden
    from qgcm_hip import AtmosModel, OceanModel, config, oml_preset, share_gpu, xforc_heat_setup, xforc_setup
    g = load_golden("cpl_natl5_sample")
    oc, at = config.preset("cpl_natl5"), config.atmos_preset("cpl_natl5")
    po, pom, wekpo, f = cpl_fullsize_inputs(g, oc, at)
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(po, pom)
    o.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(oc.nlo - 1))
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    o.oml_init(oml_preset(oc))
    yo = (np.arange(oc.nyto) + 0.5) / oc.nyto
    sst = np.asfortranarray(np.broadcast_to(4.0 * np.cos(np.pi * yo)[None, :], (oc.nxto, oc.nyto)))
    o.oml_set_state(sst=sst, sstm=sst)
    if mixed:
        am = config.AmlConfig(tat=(30.0, 40.0), aface=(1.1e-6, -0.4e-6), bface=0.7e-6, cface=-0.3e-6, dface=2.3e-4)
        ht = config.HeatConfig(D0up=6.5, Dmup=5.1, Dmdown=-5.6, Adown11=-4.7e-3, Bmup=8.9e-3, B1down=-3.1e-3, Cmup=-2.2e-3,
                               C1down=1.3e-3)
        a.aml_init(am)
        x, y = (np.arange(at.nxta) + 0.5) / at.nxta, (np.arange(at.nyta) + 0.5) / at.nyta
        ast = np.asfortranarray(-5.0 + 6.0 * np.cos(np.pi * y)[None, :] + 1.5 * np.cos(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
        hm = np.asfortranarray(1000.0 + 40.0 * np.sin(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
        a.aml_set_state(ast, ast, hm, hm)
        xforc_heat_setup(o, a, ht)
    if share:
        share_gpu(o, a)
    return o, a, int(g["nstr"])


def _alternate(run, keys, reps):
    res = {k: [] for k in keys}
    for _ in range(reps):
        for k in keys:
            res[k].append(run(k))
    return res


def atmos_step():
    pairs = {"plain": models(False), "aml": models(True)}
    n, nt = 600, {"plain": 1, "aml": 1}

    def run(k):
        a = pairs[k][1]
        t0 = time.perf_counter()
        a.steps(n, s0=nt[k])
        a.sync()
        nt[k] += n
        return 1e6 * (time.perf_counter() - t0) / n

    for k in pairs:  # warm-up: the graphs of every rotation the timed calls replay
        for _ in range(3):
            run(k)
    res = _alternate(run, ("plain", "aml"), 7)
    p, m = np.median(res["plain"]), np.median(res["aml"])
    print("one atmospheric step (%d steps per call, graphs, whole chip), us: without aml %.2f, with aml %.2f, "
          "difference %+.2f (2 launches added per step: k_aml_step, k_aml_entat; the final reduction rides in k_tend); "
          "plain %s, aml %s" % (n, p, m, m - p, " ".join("%.2f" % v for v in res["plain"]), " ".join("%.2f" % v for v in res["aml"])),
          flush=True)
    ast = pairs["aml"][1].aml_get_state()[0]
    print("  aml: ast finite %s, range %.2f .. %.2f; cfraat %.4f" % (bool(np.isfinite(ast).all()), ast.min(), ast.max(),
                                                                   pairs["aml"][1].aml_get_diag()[1]["cfraat"]), flush=True)
    for o, a, _ in pairs.values():
        o.close()
        a.close()


def xforc_call():
    from qgcm_hip import xforc
    pairs = {"momentum": models(False), "heat": models(True)}

    def run(k):
        o, a, _ = pairs[k]
        t0 = time.perf_counter()
        xforc(o, a)
        a.sync()
        return 1e6 * (time.perf_counter() - t0)

    for k in pairs:
        for _ in range(5):
            run(k)
    res = _alternate(run, ("momentum", "heat"), 50)
    p, m = np.median(res["momentum"]), np.median(res["heat"])
    oc = pairs["heat"][0].cfg
    print("one synchronised xforc(), us (median of 50, alternated): momentum half %.1f, with the heat half %.1f, "
          "difference %+.1f (3 launches added); the heat half's own bytes: sstm read + fnetoc written = %.1f MB"
          % (p, m, m - p, 2 * oc.nxto * oc.nyto * 8 / 1e6), flush=True)
    for o, a, _ in pairs.values():
        o.close()
        a.close()


def windows():
    from qgcm_hip import coupled_steps
    n = 300
    pairs = {"plain": models(False, share=True), "mixed": models(True, share=True)}
    nstr = pairs["plain"][2]
    nt0 = [1]

    def run(k):
        o, a, _ = pairs[k]
        t0 = time.perf_counter()
        coupled_steps(o, a, nt0[0], n, nstr, xforc=True)
        o.sync()
        a.sync()
        return 1e6 * (time.perf_counter() - t0) / (n // nstr)

    for k in pairs:
        run(k)
    res = {"plain": [], "mixed": []}
    for _ in range(4):
        nt0[0] += n
        for k in pairs:
            res[k].append(run(k))
    p, m = np.median(res["plain"]), np.median(res["mixed"])
    print("coupled window of %d atmospheric steps (nstr %d, CU ranges of share_gpu, xforc and oml on in both), us per "
          "ocean step: without aml / heat %.1f, with %.1f, difference %+.1f; plain %s, mixed %s" % (
              n, nstr, p, m, m - p, " ".join("%.1f" % v for v in res["plain"]), " ".join("%.1f" % v for v in res["mixed"])),
          flush=True)
    for k, (o, a, _) in pairs.items():
        print("  %s: state finite: %s" % (k, bool(np.isfinite(o.get_state()[0]).all() and np.isfinite(a.get_state()[0]).all())))
        o.close()
        a.close()


def trace():
    from qgcm_hip import xforc
    o, a, _ = models(True)
    for _ in range(20):
        xforc(o, a)
        a.aml()
    a.sync()
    o.close()
    a.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace()
    else:
        print("device: %s" % torch.cuda.get_device_name(0), flush=True)
        atmos_step()
        xforc_call()
        windows()
