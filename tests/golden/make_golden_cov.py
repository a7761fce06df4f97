#!/usr/bin/env python3
"""Golden values of the covariance matrices (covini / covocn / covatm, src/covaria_diag.F) from the TRUE reference.

Compiles the reference's covaria_diag.F unmodified, with -Dget_covar and the modules it USEs, plus a small driver of
this script's own, in a temporary directory (one build per case: the subsampling interval nscvoc / nscvat is a
compile-time PARAMETER, substituted into parameters_data.F).  covaria_diag.F is preprocessed with -DPRIVATE=PUBLIC so
that the driver can read the matrices, means, sums of weights and counts of MODULE covaria (besides the access
attributes the word occurs only in OpenMP directives, which are comments in this build without -fopenmp).  The ocean
cases build with -Docean_only, the atmosphere cases as a coupled model (covocn USEs ocstate unconditionally).  The driver calls covini, then covocn (covatm)
on four stepped states of the fixtures, each with a seeded synthetic sst (ast) of its own, and writes covout's
arrays.  All reference sources, objects and .mod files stay in the temporary directory, which is deleted.

  python tests/golden/make_golden_cov.py           # writes tests/golden/cov_*.npz, acov_*.npz
  python tests/golden/make_golden_cov.py time [N]  # the reference's covatm at 384 x 96 (nscvat 2) on N (16) threads
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("QGCM_REFERENCE", "/root/reference")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
MODS = ["atconst_data.F", "occonst_data.F", "atstate_data.F", "ocstate_data.F", "intrfac_data.F", "timinfo_data.F",
        "nc_subs.F"]

DRIVER = r"""
program cov_driver
#ifdef ATM
  use atstate, only : p => pa
  use intrfac, only : t => ast
#else
  use ocstate, only : p => po
  use intrfac, only : t => sst
#endif
  use covaria
  implicit none
  integer :: n, s, nrep
  integer(8) :: c0, c1, cr
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) n, nrep
  call covini
  do s = 1, n
    read (10) p, t
    call COVCALL
  end do
  close (10)
  call system_clock(c0, cr)
  do s = 1, nrep
    call COVCALL
  end do
  call system_clock(c1)
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
  write (11) dble(c1 - c0)/dble(cr)/dble(max(nrep, 1))
#ifndef TIMING
#  ifdef ATM
  write (11) dble(nupa), dble(nuta), swtpa, swtta
  write (11) avgpa, avgta, covpa, covta
#  else
  write (11) dble(nupo), dble(nuto), swtpo, swtto
  write (11) avgpo, avgto, covpo, covto
#  endif
#endif
  close (11)
end program cov_driver
"""


def build(wrk, dims, nsi, atm, timing=False):
    nxta, nyta, nxaooc, nyaooc, ndxr, nlo, fnot, beta = dims
    src = os.path.join(REF, "src")
    with open(os.path.join(REF, "examples", "double_gyre_ocean_only", "parameters_data.F.dg_oo")) as f:
        lines = f.read().split("\n")
    for i, ln in enumerate(lines):
        if ln.startswith("      PARAMETER ( nxta = "):
            lines[i] = "      PARAMETER ( nxta = %s, nyta = %s, nla = 3 )" % (nxta, nyta)
        elif ln.startswith("      PARAMETER ( nxaooc = "):
            lines[i] = "      PARAMETER ( nxaooc = %s, nyaooc = %s, ndxr = %s, nlo = %s )" % (nxaooc, nyaooc, ndxr, nlo)
        elif ln.startswith("      PARAMETER ( fnot = "):
            lines[i] = "      PARAMETER ( fnot = %s, beta = %s )" % (fnot, beta)
        elif ln.startswith("      PARAMETER ( nscvat = "):
            lines[i] = ln.replace("nscvat =  2", "nscvat = %d" % (nsi if atm else 2))
        elif ln.startswith("     &            nscvoc = 16"):
            lines[i] = ln.replace("nscvoc = 16", "nscvoc = %d" % (16 if atm else nsi))
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(wrk, "cov_driver.F90"), "w") as f:
        f.write(DRIVER)
    omp = ["-fopenmp"] if timing else []
    # (covocn USEs ocstate outside its ocean_only guard: the atmosphere cases build the coupled variant)
    q = ([] if atm else ["-Docean_only"]) + ["-Dget_covar"]
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2"] + q + omp
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    # (timing: OpenMP on and no -DPRIVATE=PUBLIC - the word also names the OpenMP clauses - so nothing is read back)
    subprocess.check_call(fc + ([] if timing else ["-DPRIVATE=PUBLIC"]) + ["-c", "-I" + src,
                                                                           os.path.join(src, "covaria_diag.F")], cwd=wrk)
    objs.append("covaria_diag.o")
    d = ["-DATM", "-DCOVCALL=covatm"] if atm else ["-DCOVCALL=covocn"]
    subprocess.check_call([FC, "-cpp", "-O2"] + d + (["-DTIMING"] if timing else []) + omp + ["-c", "cov_driver.F90"],
                          cwd=wrk)
    subprocess.check_call([FC, "-o", "cov_driver", "cov_driver.o"] + objs + omp, cwd=wrk)


def run(wrk, calls, nvar, nrep=0, env=None):
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([len(calls), nrep], dtype=np.int32).tobytes())
        for p, t in calls:
            fh.write(np.asfortranarray(p, dtype=np.float64).tobytes(order="F"))
            fh.write(np.asfortranarray(t, dtype=np.float64).tobytes(order="F"))
    subprocess.check_call([os.path.join(wrk, "cov_driver")], cwd=wrk, env=env)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
    if nvar is None:
        return dict(seconds=out[0])
    nmat = nvar * (nvar + 1) // 2
    res = dict(seconds=out[0], nu_p=int(out[1]), nu_t=int(out[2]), swt_p=out[3], swt_t=out[4])
    o = 5
    for k, n in (("avg_p", nvar), ("avg_t", nvar), ("cov_p", nmat), ("cov_t", nmat)):
        res[k] = out[o:o + n].copy()
        o += n
    assert o == len(out)
    return res


def ocean_calls(fixture, states, refcfg=None):
    """(po, sst) per covocn call: the fixture's stepped po (all layers, as MODULE ocstate holds it) and a seeded sst."""
    from qgcm_hip import oml_preset, preset, synth
    cfg = preset(fixture)
    om = oml_preset(cfg)
    g = np.load(os.path.join(HERE, fixture + ".npz"))
    return cfg, [(g[s + "_po"], synth.mixed_layer_fields(cfg, om, seed=11 + n)[0]) for n, s in enumerate(states)]


def atmos_calls(fixture, states, refcfg):
    """(pa, ast) per covatm call: the fixture's stepped pa and a seeded ast (numpy_atm_monitors.synthetic_fields)."""
    from numpy_atm_monitors import synthetic_fields
    from qgcm_hip import atmos_preset
    acfg = atmos_preset(refcfg)
    g = np.load(os.path.join(HERE, fixture + ".npz"))
    return acfg, [(g[s + "_pa"], synthetic_fields(acfg, 21 + n)["ast"]) for n, s in enumerate(states)]


# (golden file, fixture, reference configuration, nsi, the stepped states covocn / covatm read, atmosphere?)
CASES = [("cov_box_tiny_3", "box_tiny", "box_tiny", 3, ("ocqbdy", "steps1", "steps25", "steps26"), False),
         ("cov_box_tiny_4", "box_tiny", "box_tiny", 4, ("ocqbdy", "steps1", "steps25", "steps26"), False),
         ("cov_cyc_tiny_4", "cyc_tiny", "cyc_tiny", 4, ("ocqbdy", "steps1", "steps25", "steps26"), False),
         ("cov_box_small_16", "box_small", "box_small", 16, ("init", "ocqbdy", "steps1", "steps30"), False),
         ("cov_box_small_8", "box_small", "box_small", 8, ("init", "ocqbdy", "steps1", "steps30"), False),
         ("acov_cpl_tiny_2", "atm_tiny", "cpl_tiny", 2, ("atqzbd", "steps100", "steps101", "steps130"), True),
         ("acov_cpl_small_2", "atm_small", "cpl_small", 2, ("init", "atqzbd", "steps1", "steps40"), True)]


def time_covatm(nthreads):
    """Seconds per covatm of the reference at 384 x 96 (cpl_natl5's atmosphere, nscvat = 2) on nthreads threads."""
    import ref_binding
    dims = ref_binding.CONFIGS["cpl_natl5"][:8]
    nxt, nyt = dims[0], dims[1]
    rng = np.random.default_rng(3)
    calls = [(rng.standard_normal((nxt + 1, nyt + 1, 3)), rng.standard_normal((nxt, nyt))) for _ in range(3)]
    wrk = tempfile.mkdtemp(prefix="cov_")
    try:
        build(wrk, dims, 2, True, timing=True)
        env = dict(os.environ, OMP_NUM_THREADS=str(nthreads))
        return run(wrk, calls, None, nrep=10, env=env)["seconds"]
    finally:
        shutil.rmtree(wrk, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
        print("reference covatm 384x96 nscvat=2 (nvcvat 9216): %.1f ms per call on %d threads" % (1e3 * time_covatm(n), n))
        sys.exit(0)
    import ref_binding
    for out_name, fixture, refcfg, nsi, states, atm in CASES:
        cfg, calls = (atmos_calls if atm else ocean_calls)(fixture, states, refcfg)
        nxt, nyt = calls[0][1].shape
        nvar = (nxt // nsi) * (nyt // nsi)
        wrk = tempfile.mkdtemp(prefix="cov_")
        try:
            build(wrk, ref_binding.CONFIGS[refcfg][:8], nsi, atm)
            res = run(wrk, calls, nvar)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        out = dict(c_nsi=np.int64(nsi), c_atm=np.int64(atm), c_fixture=np.array(fixture))
        for n, (p, t) in enumerate(calls):
            out["in%d_p1" % n] = np.asarray(p[:, :, 0])  # (only layer 1 is sampled)
            out["in%d_t" % n] = np.asarray(t)
        out.update({"out_" + k: np.asarray(v) for k, v in res.items() if k != "seconds"})
        path = os.path.join(HERE, "%s.npz" % out_name)
        np.savez_compressed(path, **out)
        sys.stderr.write("wrote %s.npz (nvar %d, %d bytes)\n" % (out_name, nvar, os.path.getsize(path)))
