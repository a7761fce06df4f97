"""Cases of the drop-in test (tests/test_dropin.py, tests/golden/make_golden_dropin.py): the reference main
program src/q-gcm.F over the shim, one executable per compile-time grid."""
import os
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DROP = os.path.join(ROOT, "q-gcm_amd", "fortran", "dropin")
BUILD = os.path.join(ROOT, "oracle", "build_dropin.sh")  # products under oracle/_ref/dropin/<cfg>/ (exe_path)
NSTEPS = 120
# (ocean steps, tolerance on max|difference| / max|reference| of every restart field).  The coupled model carries
# switches (convective adjustment of both mixed layers, src/amlsubs.F / src/omlsubs.F) that amplify rounding: the
# UNMODIFIED reference run with 1 vs 5 OpenMP threads (different summation order in xintp) differs by 1.8e-3 in po
# after 30 ocean steps and 5e-4 after 120, while 2 vs 1 threads stay identical for 30 steps - hence one tight
# single-step comparison and one loose long one for that case.
# Measured on the MI355X in round 3 (one OpenMP thread for the coupled case, gpurun_out/dropin_errors.log): box 7.6e-15,
# cyclic 8e-16, coupled from rest 2.7e-11 after 120 ocean steps (round 2 allowed 2e-2 on the strength of the
# reference's own 1-vs-5-thread spread; on ONE thread both executables are reproducible and agree this closely).
# box_tiny_spl (round 4): the box case compiled with -Dsponge_layer_k247 - the shim sends r_spl / c1_spl to the device
RUNS = {"box_tiny": ((120, 1e-9),), "cyc_tiny": ((120, 1e-9),), "cpl_tiny": ((1, 1e-12), (120, 1e-8)),
        "box_tiny_spl": ((120, 1e-9),)}
# Round 3 pins the coupled OCEAN half: after one ocean step from radiative balance the ocean is still at rest (po = pom
# = 0 on both sides), so (1, 1e-12) above checks the atmosphere and the mixed layers only - and for dozens of steps
# after that po stays below 1e-8 m2/s2 and is driven by rounding noise (xon(1), "zero by construction of entoc in
# oml", src/ocisubs.F:334-336, enters dpioc with an O(1) gain: HIP vs reference 1.9e-7 of max|po| = 1.2e-11 after 4
# steps).  So these runs start from a RESTART dump with an energetic ocean: the reference's own 120-step dump
# (tests/golden/dropin_cpl_tiny_lastday.bin: atmosphere, both mixed layers) with the ocean replaced by the
# Gaussian-eddy state of qgcm_hip.synth (max|po| = 1.5 m2/s2), time stamp 0 - read back by the main program through
# src/q-gcm.F:612-640.  (ocean steps, tolerance); one OpenMP thread, where both executables are bitwise reproducible.
# Measured: every restart field within 1e-15 of the reference's after 4 AND after 30 ocean steps.
RUNS_RESTART = {"cpl_tiny": ((4, 1e-12), (30, 1e-11))}
# OpenMP threads of the host code (golden generation and test alike).  The coupled reference is NOT run-to-run
# reproducible with two threads: two runs of the unmodified q-gcm_ref on the same case differ in pa / ast after ONE
# ocean step (thread-order dependent sums in xforc / aml, amplified by the nearly singular barotropic zonal-mean mode
# of the channel to ~1e-12) - observed as a flaky 1e-12 comparison.  One thread is reproducible, for both executables.
THREADS = {"box_tiny": 2, "cyc_tiny": 2, "cpl_tiny": 1, "box_tiny_spl": 2}

# cfg -> ((nxta, nyta, nxaooc, nyaooc, ndxr, nlo, fnot, beta), mode); dims as oracle/ref_binding.CONFIGS
CASES = {
    "box_tiny": ((8, 8, 4, 3, 12, 3, "9.37456D-05", "1.75360D-11"), "box"),
    "cyc_tiny": ((4, 8, "nxta", 3, 12, 3, "-1.19467D-04", "1.31301D-11"), "cyclic"),
    "cpl_tiny": ((16, 12, 4, 3, 12, 3, "9.37456D-05", "1.75360D-11"), "coupled"),
    "box_tiny_spl": ((8, 8, 4, 3, 12, 3, "9.37456D-05", "1.75360D-11"), "box_spl"),
}


def exe_path(cfg, which):
    return os.path.join(ROOT, "oracle", "_ref", "dropin", cfg, "q-gcm_" + which)


def golden_name(cfg, nsteps, restart=False):
    return "dropin_%s_%slastday%s.bin" % (cfg, "eddy_" if restart else "", "" if nsteps == NSTEPS and not restart else "_%d" % nsteps)


def write_eddy_restart(cfg, path):
    """The restart dump of RUNS_RESTART (see there) for a coupled case."""
    sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
    from qgcm_hip import config, restart, synth
    oc = config.preset(cfg)
    r = restart.read_restart(os.path.join(ROOT, "tests", "golden", golden_name(cfg, NSTEPS)), oc, coupled=True)
    po = synth.gaussian_eddy(oc)
    restart.write_restart(path, oc, 0.0, po, po, r["sst"], r["sstm"], r["ast"], r["astm"], r["hmixa"], r["hmixam"],
                          pa=r["pa"], pam=r["pam"])


def prepare_case(cfg, rundir, nsteps=NSTEPS, restart=False):
    subprocess.check_call([sys.executable, os.path.join(DROP, "make_case.py"), cfg, rundir, str(nsteps)],
                          stdout=subprocess.DEVNULL)
    if CASES[cfg][1] == "coupled":  # initial state of examples/double_gyre_coupled: radiative balance
        p = os.path.join(rundir, "input.params")
        txt = open(p).read()
        assert "\nzero\n" in txt
        if restart:
            write_eddy_restart(cfg, os.path.join(rundir, "restart.bin"))
        open(p, "w").write(txt.replace("\nzero\n", "\nrestart.bin\n" if restart else "\nrbal\n"))
