#!/usr/bin/env python3
"""Golden values of the atmosphere's time averages (tavini / tavatm / tavout, src/timavge.F) and of its periodic dump
(atnc_out, src/nc_subs.F:1077-1326) from the TRUE reference.

Compiles the reference's timavge.F and nc_subs.F unmodified, with the modules they USE and a small driver of this
script's own, in a temporary directory (one build per grid: the dimensions are compile-time PARAMETERs of a coupled
configuration; -Datmos_only leaves the ocean halves out).  timavge.F is preprocessed with -DPRIVATE=PUBLIC so that the
driver can read the atmosphere sums of MODULE timavge (as make_golden_tavg.py does), nc_subs.F with -Duse_netcdf
against the netCDF stand-in of make_golden_qocdiag.py (the project's own text: nf_put_vara_double records what
atnc_out writes).  The driver fills MODULE atconst / atstate / intrfac, calls tavini, tavatm on three stepped states of
the atmosphere fixtures (each with seeded synthetic forcing of its own, whose column nxpa differs from column 1), then
tavout, and writes the scaled sums; tavout's eddy fluxes uptpat / vptpat are locals written only to netCDF, derived
here from the reference's scaled arrays with tavout's own expression.  Then atnc_init / atnc_out for nska = 1, 2, 5 on
the last state.  All reference sources, objects and .mod files stay in the temporary directory, which is deleted.

  python tests/golden/make_golden_atm_tavg.py           # writes tests/golden/atav_cpl_{tiny,small,tiny_a4}.npz
  python tests/golden/make_golden_atm_tavg.py cpl_tiny_a4  # only the named cases
  python tests/golden/make_golden_atm_tavg.py time [N]  # the reference's tavatm at 385 x 97 x 3 on N (16) threads
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
sys.path.insert(0, HERE)
REF = os.environ.get("QGCM_REFERENCE", "/root/reference")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
MODS = ["atconst_data.F", "occonst_data.F", "atstate_data.F", "ocstate_data.F", "intrfac_data.F", "timinfo_data.F"]
NSKA = (1, 2, 5)
SUMS = ("txatav", "tyatav", "wtatav", "fmatav", "astav", "patav", "qatav", "uufa", "tufa", "utufa", "vvfa", "tvfa",
        "vtvfa")
# (golden file, fixture, the three stepped states tavatm reads)
CASES = [("cpl_tiny", "atm_tiny", ("steps100", "steps101", "steps130")),
         ("cpl_small", "atm_small", ("steps1", "atqzbd", "steps40")),
         ("cpl_tiny_a4", "atm_tiny_a4", ("steps100", "steps101", "steps130"))]

DRIVER = r"""
program atav_driver
  use parameters, only : nxpa, nypa, nxta, nyta, nla, fnot
  use atconst, only : dxa, rdxaf0, gpat
  use atstate, only : pa, qa, wekta
  use intrfac, only : ast, tauxa, tauya, fnetat, hmat, hmixa
  use timinfo, only : ntdone, noutat, tyrs, noutstepat
  use timavge
#ifndef TIMING
  use nc_subs, only : atnc_init, atnc_out, atpid, attid
#endif
  implicit none
  integer :: ntav, nrep, nnska, s, r, nska(8), outflat(7)
  integer(8) :: c0, c1, cr
  double precision :: sc(2)
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) sc
  dxa = sc(1); hmat = sc(2)
  rdxaf0 = 1.0d0/(dxa*fnot)
  read (10) gpat(1:nla-1)
  read (10) ntav, nrep, nnska
  read (10) nska(1:nnska)
  call tavini
  do s = 1, ntav
    read (10) pa, qa, tauxa, tauya, wekta, fnetat, ast, hmixa
    call tavatm
  end do
  close (10)
  call system_clock(c0, cr)
  do r = 1, nrep
    call tavatm
  end do
  call system_clock(c1)
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
#ifndef TIMING
  call tavout
  write (11) dble(nsumat)
  write (11) txatav, tyatav, wtatav, fmatav, astav, patav, qatav, uufa, tufa, utufa, vvfa, tvfa, vtvfa
#endif
  write (11) dble(c1 - c0)/dble(cr)/dble(max(nrep, 1))
  close (11)
#ifndef TIMING
  ntdone = 0; noutat = 1; tyrs = 0.0d0; noutstepat = 1
  outflat = 1
  open (21, file='rec.bin', access='sequential', form='unformatted', status='replace')
  do r = 1, nnska
    atpid = 1; attid = 2
    call atnc_init (nska(r), outflat)
    call atnc_out (nska(r), outflat)
  end do
  close (21)
#endif
end program atav_driver
"""


def build(wrk, dims, timing=False, nla=3):
    from make_golden_qocdiag import NETCDF_INC, NETCDF_STUBS
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
    with open(os.path.join(wrk, "netcdf.inc"), "w") as f:
        f.write(NETCDF_INC)
    with open(os.path.join(wrk, "nfstub.f90"), "w") as f:
        f.write(NETCDF_STUBS)
    with open(os.path.join(wrk, "atav_driver.F90"), "w") as f:
        f.write(DRIVER)
    # timing: OpenMP on, and no -DPRIVATE=PUBLIC (the word also names the OpenMP clauses), so no sums are read
    omp = ["-fopenmp"] if timing else []
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2", "-Datmos_only"] + omp
    inc = ["-I" + wrk, "-I" + src]
    objs = []
    subprocess.check_call([FC, "-O2", "-c", "nfstub.f90"], cwd=wrk)
    objs.append("nfstub.o")
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c"] + inc + [f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call(fc + ["-Duse_netcdf", "-c"] + inc + [os.path.join(src, "nc_subs.F")], cwd=wrk)
    objs.append("nc_subs.o")
    subprocess.check_call(fc + ([] if timing else ["-DPRIVATE=PUBLIC"]) + ["-c"] + inc + [os.path.join(src, "timavge.F")],
                          cwd=wrk)
    objs.append("timavge.o")
    subprocess.check_call([FC, "-cpp", "-O2"] + (["-DTIMING"] if timing else []) + omp + ["-c", "atav_driver.F90"], cwd=wrk)
    subprocess.check_call([FC, "-o", "atav_driver", "atav_driver.o"] + objs + omp, cwd=wrk)


def forcing(acfg, seed):
    """tauxa, tauya, wekta, ast, hmixa (numpy_atm_monitors.synthetic_fields: seeded noise on smooth fields, so that
    column nxpa differs from column 1) and a seeded fnetat (nxta, nyta)."""
    from numpy_atm_monitors import synthetic_fields
    s = synthetic_fields(acfg, seed)
    rng = np.random.default_rng(1000 + seed)
    fnetat = np.asfortranarray(-40.0 + 60.0 * rng.standard_normal((acfg.nxpa - 1, acfg.nypa - 1)))
    return dict(tauxa=s["tauxa"], tauya=s["tauya"], wekta=s["wekta"], fnetat=fnetat, ast=s["ast"], hmixa=s["hmixa"])


def run(wrk, acfg, hmat, calls, nrep=0, nska=NSKA, threads=None):
    F = lambda a: np.asfortranarray(a, dtype=np.float64).tobytes(order="F")
    nl = acfg.nla
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([acfg.dxa, hmat], dtype=np.float64).tobytes())
        fh.write(np.array(acfg.gpat[:nl - 1], dtype=np.float64).tobytes())
        fh.write(np.array([len(calls), nrep, len(nska)] + list(nska), dtype=np.int32).tobytes())
        for f in calls:
            for k in ("pa", "qa", "tauxa", "tauya", "wekta", "fnetat", "ast", "hmixa"):
                fh.write(F(f[k]))
    env = dict(os.environ, OMP_NUM_THREADS=str(threads or 1))
    subprocess.check_call([os.path.join(wrk, "atav_driver")], cwd=wrk, env=env)
    return np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)


def unpack(out, acfg):
    nxp, nyp, nl = acfg.nxpa, acfg.nypa, acfg.nla
    nxt, nyt = nxp - 1, nyp - 1
    shapes = dict(txatav=(nxp, nyp), tyatav=(nxp, nyp), wtatav=(nxt, nyt), fmatav=(nxt, nyt), astav=(nxt, nyt),
                  patav=(nxp, nyp, nl), qatav=(nxp, nyp, nl), uufa=(nxp, nyt), tufa=(nxp, nyt), utufa=(nxp, nyt),
                  vvfa=(nxt, nyp), tvfa=(nxt, nyp), vtvfa=(nxt, nyp))
    res = dict(nsumat=int(out[0]))
    o = 1
    for k in SUMS:
        n = int(np.prod(shapes[k]))
        res[k] = out[o:o + n].reshape(shapes[k], order="F")
        o += n
    assert o == len(out) - 1  # (the time per call)
    res["uptpat"] = res["utufa"] - res["uufa"] * res["tufa"]   # tavout, src/timavge.F:785
    res["vptpat"] = res["vtvfa"] - res["vvfa"] * res["tvfa"]   # tavout, src/timavge.F:795
    return res


def dumps(wrk, nl):
    """atnc_out's records per nska (in NSKA order, one atnc_init + atnc_out each): dict 'n<nska>_<field>' ->
    (planes, rows, columns)."""
    from make_golden_qocdiag import read_records
    names = {"ast": "ast", "p": "pa", "q": "qa", "wekt": "wekta", "h": "ha", "taux": "tauxa", "tauy": "tauya",
             "hmixa": "hmixa"}
    recs = [r for r in read_records(os.path.join(wrk, "rec.bin")) if len(r[2]) >= 3]  # (not the time axes)
    assert len(recs) == len(names) * len(NSKA)  # every flag on: eight fields per atnc_out call
    out = {}
    for n, (name, start, cnt, data) in enumerate(recs):
        planes = cnt[2] if len(cnt) == 4 else 1
        out["n%d_%s" % (NSKA[n // len(names)], names[name])] = data.reshape(planes, cnt[1], cnt[0])
    return out


def time_mode():
    """tavatm of the reference, -fopenmp, N threads, at cpl_natl5's atmosphere (385 x 97 x 3): a host CPU figure."""
    import ref_binding
    from qgcm_hip import atmos_preset, synth
    acfg = atmos_preset("cpl_natl5")
    s = synth.atmos_fields(acfg)
    f = dict(forcing(acfg, 3), pa=s["pa"], qa=1e-6 * s["pa"])
    nth = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    wrk = tempfile.mkdtemp(prefix="atav_")
    try:
        build(wrk, ref_binding.CONFIGS["cpl_natl5"][:8], timing=True)
        run(wrk, acfg, 1000.0, [f], nrep=20, threads=nth)
        t = run(wrk, acfg, 1000.0, [f], nrep=400, threads=nth)[-1]
        print("reference tavatm (host CPU, -O2 -fopenmp) %dx%dx%d, %d threads: %.1f us per call"
              % (acfg.nxpa, acfg.nypa, acfg.nla, nth, 1e6 * t))
    finally:
        shutil.rmtree(wrk, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        time_mode()
        sys.exit(0)
    import ref_binding
    from qgcm_hip import atmos_preset
    hmat = 1000.0  # examples/double_gyre_coupled's input.params
    for name, fixture, states in [c for c in CASES if len(sys.argv) == 1 or c[0] in sys.argv[1:]]:
        acfg = atmos_preset(name)
        g = np.load(os.path.join(HERE, fixture + ".npz"))
        calls = [dict(forcing(acfg, 21 + n), pa=g[st + "_pa"], qa=g[st + "_qa"]) for n, st in enumerate(states)]
        wrk = tempfile.mkdtemp(prefix="atav_")
        try:
            build(wrk, ref_binding.CONFIGS[name][:8], nla=acfg.nla)
            res = unpack(run(wrk, acfg, hmat, calls), acfg)
            rec = dumps(wrk, acfg.nla)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        out = {"c_" + k: np.float64(v) for k, v in dict(dxa=acfg.dxa, fnot=acfg.fnot, hmat=hmat).items()}
        out["c_gpat"] = np.asarray(acfg.gpat[:acfg.nla - 1], dtype=np.float64)
        for n, f in enumerate(calls):
            out.update({"in%d_%s" % (n, k): np.asarray(v) for k, v in f.items()})
        out.update({"out_" + k: np.asarray(v) for k, v in res.items()})
        out.update(rec)
        np.savez_compressed(os.path.join(HERE, "atav_%s.npz" % name), **out)
        sys.stderr.write("wrote atav_%s.npz (nsumat %d, %d dump fields)\n" % (name, res["nsumat"], len(rec)))
