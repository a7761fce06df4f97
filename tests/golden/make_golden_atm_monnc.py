#!/usr/bin/env python3
"""Golden values of the atmosphere half of monnc_comp and courat (src/monitor_diag.F) and of the atmospheric valids
(src/valsubs.F) from the TRUE reference.

Compiles the reference's monitor_diag.F and valsubs.F unmodified, with the modules they USE and a small driver of this
script's own, in a temporary directory (one build per grid: the dimensions are compile-time PARAMETERs of a coupled
configuration, -Datmos_only -Dsb_hflux, so that the ocean half is left out and the driver needs no ocean inputs).  It
fills MODULE atstate / atconst / intrfac / radiate with the stepped states of the atmosphere fixtures (atm_tiny step 130,
29 steps after the averaging at step 101, so pa != pam; atm_small step 40), their wekpa / entat, seeded synthetic
wekta, tauxa, tauya, ast, hmixa, uekat, vekat and non-zero Aup .. Dup, davgat; calls monnc_comp and valids, and stores
inputs and the MODULE monitor variables (layout of qgcm_hip_atm_monitors) as tests/golden/atmon_<case>.npz.  valids
prints its extrema only when they fail, so the driver takes the twelve extrema with minval / maxval and stores the
reference's solnok with them, for the inputs and for the inputs with ast = 95 at one point.  All reference sources,
objects and .mod files stay in the temporary directory, which is deleted.

  python tests/golden/make_golden_atm_monnc.py [case ...] # the golden files, or the named ones (build machine only)
  python tests/golden/make_golden_atm_monnc.py time [N]  # time the host atmosphere half at 385 x 97 x 3 on N threads
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
MODS = ["atconst_data.F", "occonst_data.F", "atstate_data.F", "intrfac_data.F", "monitor_data.F", "radiate_data.F",
        "timinfo_data.F", "nc_subs.F", "monitor_diag.F", "valsubs.F"]
FLAGS = ["-Datmos_only", "-Dsb_hflux"]

DRIVER = r"""
program atmon_driver
  use parameters, only : nxpa, nypa, nxta, nyta, nla, fnot
  use atconst
  use atstate, only : pa, pam, qa, wekta, wekpa, entat
  use intrfac, only : ast, tauxa, tauya, hmixa, hmat, uekat, vekat
  use radiate, only : Aup, Bup, Cup, Dup
  use monitor
  use mondiag, only : monnc_comp
  use valsubs, only : valids
  implicit none
  integer :: nrep, r, ibad, jbad
  integer(8) :: c0, c1, cr
  double precision :: sc(9), aupr(nla-1), sv
  logical :: ok1, ok2
  character(len=16) :: arg
  nrep = 1
  if (command_argument_count() > 0) then
    call get_command_argument(1, arg)
    read (arg, *) nrep
  end if
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) sc, aupr, gpat(1:nla-1), hat, ah4at, ibad, jbad
  read (10) pa, pam, qa, wekpa, entat, wekta, tauxa, tauya, ast, hmixa, uekat, vekat
  close (10)
  dxa = sc(1); dta = sc(2); rhoat = sc(3); cpat = sc(4); hmat = sc(5); davgat = sc(6)
  Aup(nla,1:nla-1) = aupr; Bup(nla) = sc(7); Cup(nla) = sc(8); Dup(nla) = sc(9)
  hdxam1 = 0.5d0/dxa
  dxam2 = 1.0d0/(dxa*dxa)
  rdxaf0 = 1.0d0/(dxa*fnot)
  call system_clock(c0, cr)
  do r = 1, nrep
    call monnc_comp
  end do
  call system_clock(c1)
  ok1 = .true.
  call valids (ok1)
  sv = ast(ibad, jbad)
  ast(ibad, jbad) = 95.0d0
  ok2 = .true.
  call valids (ok2)
  ast(ibad, jbad) = sv
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
  write (11) wetmat, watmat, wepmat, wapmat
  write (11) entmat, enamat, etamat, et2mat, ddtpeat, pkenat
  write (11) utauat
  write (11) pavgat, qavgat, ah4dat, kealat, ddtkeat, dble(atstpos), atstval
  write (11) tmlmat, hmlmat, astmin, astmax, hcmlat, tmaooc, olrtop
  write (11) umminat, ummaxat, vmminat, vmmaxat, cnmlat
  write (11) ugminat, ugmaxat, vgminat, vgmaxat, cnqgat
  write (11) minval(pa), maxval(pa), minval(qa), maxval(qa), minval(ast), maxval(ast)
  write (11) minval(wekta), maxval(wekta), minval(tauxa), maxval(tauxa), minval(tauya), maxval(tauya)
  write (11) merge(1.0d0, 0.0d0, ok1), merge(1.0d0, 0.0d0, ok2)
  write (11) dble(c1 - c0)/dble(cr)/dble(nrep)
  close (11)
end program atmon_driver
"""


def build(wrk, dims, nla=3):
    nxta, nyta, nxaooc, nyaooc, ndxr, nlo, fnot, beta = dims
    src = os.path.join(REF, "src")
    with open(os.path.join(REF, "examples", "double_gyre_ocean_only", "parameters_data.F.dg_oo")) as f:
        lines = f.read().split("\n")
    for i, ln in enumerate(lines):
        if ln.startswith("      PARAMETER ( nxta = "):
            lines[i] = "      PARAMETER ( nxta = %s, nyta = %s, nla = %d )" % (nxta, nyta, nla)
        elif ln.startswith("      PARAMETER ( nxaooc = "):
            lines[i] = "      PARAMETER ( nxaooc = %s, nyaooc = %s, ndxr = %s, nlo = %s )" % (nxaooc, nyaooc, ndxr, nlo)
        elif ln.startswith("      PARAMETER ( fnot = "):
            lines[i] = "      PARAMETER ( fnot = %s, beta = %s )" % (fnot, beta)
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(wrk, "atmon_driver.F90"), "w") as f:
        f.write(DRIVER)
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2", "-fopenmp"] + FLAGS
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call([FC, "-cpp", "-O2", "-fopenmp", "-c", "atmon_driver.F90"], cwd=wrk)
    subprocess.check_call([FC, "-fopenmp", "-o", "atmon_driver", "atmon_driver.o"] + objs, cwd=wrk)


def inputs(acfg, ocfg, g, step, seed):
    f = dict(pa=g[step + "_pa"], pam=g[step + "_pam"], qa=g[step + "_qa"], wekpa=g["in_wekpa"], entat=g["in_entat"])
    from numpy_atm_monitors import synthetic_fields
    f.update(synthetic_fields(acfg, seed))
    nl = acfg.nla
    c = dict(dxa=acfg.dxa, dta=acfg.dta, fnot=acfg.fnot, rhoat=1.0, cpat=1.0e3, hmat=1000.0, davgat=37.5,
             bup=0.31, cup=-4.0e-3, dup=1.7, aup=np.array([0.05 * (k + 1) for k in range(nl - 1)]),
             gpat=np.asarray(acfg.gpat[:nl - 1]), hat=np.asarray(acfg.hat[:nl]), ah4at=np.asarray(acfg.ah4at[:nl]),
             nxaooc=ocfg.nxaooc, nyaooc=ocfg.nyaooc, nx1=1 + (acfg.nxta - ocfg.nxaooc) // 2,
             ny1=1 + (acfg.nyta - ocfg.nyaooc) // 2, ibad=acfg.nxta // 3 + 1, jbad=acfg.nyta // 2 + 1)
    return f, c


def run(wrk, f, c, nrep=1, threads=None):
    sc = np.array([c[k] for k in ("dxa", "dta", "rhoat", "cpat", "hmat", "davgat", "bup", "cup", "dup")])
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        for a in (sc, c["aup"], c["gpat"], c["hat"], c["ah4at"]):
            fh.write(np.asarray(a, dtype=np.float64).tobytes())
        fh.write(np.array([c["ibad"], c["jbad"]], dtype=np.int32).tobytes())
        for k in ("pa", "pam", "qa", "wekpa", "entat", "wekta", "tauxa", "tauya", "ast", "hmixa", "uekat", "vekat"):
            fh.write(np.asfortranarray(f[k], dtype=np.float64).tobytes(order="F"))
    env = dict(os.environ, OMP_NUM_THREADS=str(threads or 1))
    env.setdefault("OMP_STACKSIZE", "64M")
    res = subprocess.run([os.path.join(wrk, "atmon_driver"), str(nrep)], cwd=wrk, env=env, capture_output=True,
                         text=True, check=True)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
    nl = len(c["hat"])
    n = 18 * nl + 11
    return out[:n], out[n:n + 12], out[n + 12:n + 14], out[-1], res.stdout


if __name__ == "__main__":
    import ref_binding
    from qgcm_hip import atmos_preset, preset, synth
    timing = len(sys.argv) > 1 and sys.argv[1] == "time"
    # (cpl_tiny_a4: four layers, so that the layer loops run over more than two interfaces)
    cases = [("cpl_natl5", None, None)] if timing else [("cpl_tiny", "atm_tiny", "steps130"),
                                                       ("cpl_small", "atm_small", "steps40"),
                                                       ("cpl_tiny_a4", "atm_tiny_a4", "steps130")]
    if not timing and len(sys.argv) > 1:  # only the named cases
        cases = [c for c in cases if c[0] in sys.argv[1:]]
    for name, fixture, step in cases:
        a = ref_binding.CONFIGS[name]
        acfg, ocfg = atmos_preset(name), preset(name)
        wrk = tempfile.mkdtemp(prefix="atmonnc_")
        try:
            build(wrk, a[:8], acfg.nla)
            if timing:
                s = synth.atmos_fields(acfg)
                g = dict(x_pa=s["pa"], x_pam=s["pam"], x_qa=1e-6 * s["pa"], in_wekpa=s["wekpa"], in_entat=s["entat"])
                f, c = inputs(acfg, ocfg, g, "x", 11)
                nth = int(sys.argv[2]) if len(sys.argv) > 2 else 16
                run(wrk, f, c, 1, nth)
                t = run(wrk, f, c, 20, nth)[3]
                sys.stderr.write("host monnc_comp (atmosphere only, courat included) at %dx%dx%d, %d threads: "
                                 "%.3f ms per call\n" % (acfg.nxpa, acfg.nypa, acfg.nla, nth, 1e3 * t))
                continue
            g = np.load(os.path.join(HERE, fixture + ".npz"))
            f, c = inputs(acfg, ocfg, g, step, {"atm_tiny": 7, "atm_small": 8, "atm_tiny_a4": 9}[fixture])
            vec, val, ok, _, _ = run(wrk, f, c)
            out = {"in_" + k: np.asarray(v) for k, v in f.items()}
            out.update({"c_" + k: np.asarray(v) for k, v in c.items()})
            out["monitors"] = vec
            out["valids"] = val
            out["solnok"] = ok
            np.savez_compressed(os.path.join(HERE, "atmon_%s.npz" % name), **out)
            sys.stderr.write("wrote atmon_%s.npz (%d values, solnok %s)\n" % (name, len(vec), ok))
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
