"""The Southern Ocean presets whose rows are split (socn4, socn3, socn2, socn1 - 5760 x 721, 7680 x 961,
11520 x 1441, 23040 x 2881 points, three layers) at full size; printed as a log (profiles/long_rows.log).
  python3 profiles/tools/long_rows.py [preset ...]   per preset: OceanModel(preset) - hostinit and homsol through the
                                                     device solver - then the time per step by HIP events over
                                                     graph-replayed steps as bench.py brackets them (5 windows of 20
                                                     steps, none with an averaging step) and the per-class kernel times
                                                     of 20 eager steps (qgcm_hip_profile_steps)"""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401


def run(name):
    from qgcm_hip import OceanModel, lib, preset, synth
    cfg = preset(name)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    t0 = time.perf_counter()
    m = OceanModel(cfg)
    try:
        blocks, nbytes = lib.live_allocs()
        print("%s: %d x %d x %d, dxo %.0f m, dto %.0f s; rows %d x %d, column in %d segment(s); set-up %.1f s; device memory %.2f GB" % (
            name, cfg.nxpo, cfg.nypo, cfg.nlo, cfg.dxo, cfg.dto, *m.row_plan(), len(m.thomas_plan()), time.perf_counter() - t0, nbytes / 1e9), flush=True)
        m.set_p(po, po)
        m.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
        m.set_cyc_forcing(*(synth.tau_line_integrals(cfg, tx) + (np.zeros(cfg.nlo - 1), np.zeros(cfg.nlo - 1))))
        m.steps(45, s0=1)          # steps 1 and 26 average; the windows below never do
        s0, wins = 52, []
        for _ in range(5):         # 20-step windows between averaging steps (52..71, 77..96, ...)
            m.steps(20, s0=s0)     # rehearsal: the graphs of this phase exist
            wins.append(1e3 * m.time_steps(20, s0=s0) / 20)
            s0 += 25
        pr = m.profile_steps(20, s0=s0)
        fin = bool(np.isfinite(m.get_state()[0]).all())
        print("   us per step, 5 windows of 20 graph-replayed steps: %s  median %.1f  state finite: %s" % (
            " ".join("%.1f" % w for w in wins), float(np.median(wins)), fin), flush=True)
        tot = sum(ms for k, (ms, c) in pr.items() if c and not k.startswith("k_noop"))
        print("   eager per-class us per step (HIP-event brackets around every launch, bracket cost included; launches per step): " + ", ".join(
            "%s %.1f (x%d)" % (k, 1e3 * ms / 20, c // 20) for k, (ms, c) in sorted(pr.items()) if c and not k.startswith("k_noop"))
            + "; sum %.1f" % (1e3 * tot / 20), flush=True)
    finally:
        m.close()


if __name__ == "__main__":
    for n in (sys.argv[1:] or ["socn4", "socn3", "socn2", "socn1"]):
        run(n)
