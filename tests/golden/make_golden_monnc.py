#!/usr/bin/env python3
"""Golden values of the ocean half of monnc_comp and couroc (src/monitor_diag.F) from the TRUE reference.

Compiles the reference's monitor_diag.F unmodified, with the modules it USEs and a small driver of this script's own,
in a temporary directory (one build per grid: the dimensions are compile-time PARAMETERs), fills MODULE ocstate /
occonst / intrfac with the stepped states of the existing tiny fixtures (step 26, just after a leapfrog averaging, so
po != pom), a non-zero entoc, a wind stress with both components, wekto and sst, calls monnc_comp and stores inputs and
the MODULE monitor variables (layout of qgcm_hip_monitors) as tests/golden/mon_<case>.npz.  All reference sources,
objects and .mod files stay in the temporary directory, which is deleted.

  python tests/golden/make_golden_monnc.py           # the golden files (build machine only)
  python tests/golden/make_golden_monnc.py time [N]  # time the host monnc_comp at 961 x 961 x 3 on N threads (16)
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
REF = os.environ.get("QGCM_REFERENCE", "/root/reference")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
MODS = ["atconst_data.F", "occonst_data.F", "ocstate_data.F", "intrfac_data.F", "monitor_data.F", "radiate_data.F",
        "timinfo_data.F", "nc_subs.F", "monitor_diag.F"]
RHOOC, CPOC = 1.0e3, 4.0e3

DRIVER = r"""
program mon_driver
  use parameters, only : nxpo, nypo, nxto, nyto, nlo, fnot
  use occonst
  use ocstate, only : po, pom, qo, wekto, wekpo, entoc
  use intrfac, only : sst, tauxo, tauyo, hmoc
  use monitor
  use mondiag, only : monnc_comp
  implicit none
  integer :: nrep, r, k
  integer(8) :: c0, c1, cr
  double precision :: sc(7)
  character(len=16) :: arg
  nrep = 1
  if (command_argument_count() > 0) then
    call get_command_argument(1, arg)
    read (arg, *) nrep
  end if
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) sc, gpoc(1:nlo-1), hoc, ah2oc, ah4oc
  read (10) po, pom, qo, wekpo, entoc, tauxo, tauyo, wekto, sst
  close (10)
  dxo = sc(1); dto = sc(2); delek = sc(3); rhooc = sc(4); cpoc = sc(5); ycexp = sc(6); hmoc = sc(7)
  hdxom1 = 0.5d0/dxo
  dxom2 = 1.0d0/(dxo*dxo)
  rdxof0 = 1.0d0/(dxo*fnot)
  call system_clock(c0, cr)
  do r = 1, nrep
    call monnc_comp
  end do
  call system_clock(c1)
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
  write (11) wetmoc, watmoc, wepmoc, wapmoc, entmoc, enamoc
  write (11) etamoc, et2moc, ddtpeoc, pkenoc, utauoc
  write (11) pavgoc, qavgoc, ah2doc, ah4doc, kealoc, ddtkeoc, osfmin, osfmax, occirc, dble(ocjpos), ocjval
  write (11) btdgoc, sstmin, sstmax, tmlmoc, hfmloc, occtot
  write (11) umminoc, ummaxoc, vmminoc, vmmaxoc, cnmloc
  write (11) ugminoc, ugmaxoc, vgminoc, vgmaxoc, cnqgoc
  write (11) dble(c1 - c0)/dble(cr)/dble(nrep)
  close (11)
end program mon_driver
"""


def build(wrk, dims, cyclic):
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
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(wrk, "mon_driver.F90"), "w") as f:
        f.write(DRIVER)
    q = ["-Docean_only"] + (["-Dcyclic_ocean", "-Dnb_hflux"] if cyclic else [])
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2", "-fopenmp"] + q
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call([FC, "-cpp", "-O2", "-fopenmp", "-c", "mon_driver.F90"], cwd=wrk)
    subprocess.check_call([FC, "-fopenmp", "-o", "mon_driver", "mon_driver.o"] + objs, cwd=wrk)


def inputs(cfg, g):
    """The fixture's state after step 26 and synthetic forcing fields (all stored in the golden file)."""
    from qgcm_hip import oml_preset, synth
    om = oml_preset(cfg)
    sst, _, _, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    x = np.arange(cfg.nxpo)[:, None] / (cfg.nxpo - 1.0)
    y = np.arange(cfg.nypo)[None, :] / (cfg.nypo - 1.0)
    entoc = 2.0e-6 * np.sin(np.pi * y) * np.cos(2.0 * np.pi * x) + 5.0e-7 * y
    if cfg.cyclic:
        entoc[-1, :] = entoc[0, :]
    f = dict(po=g["steps26_po"], pom=g["steps26_pom"], qo=g["steps26_qo"], qom=g["steps26_qom"], wekpo=wekpo,
             entoc=np.asfortranarray(entoc), tauxo=tx, tauyo=ty, wekto=wekto, sst=sst)
    c = dict(dxo=cfg.dxo, dto=cfg.dto, delek=cfg.delek, rhooc=RHOOC, cpoc=CPOC, ycexp=om.ycexp, hmoc=om.hmoc,
             sb_hflux=0, nb_hflux=int(cfg.cyclic))
    return f, c


def run(wrk, cfg, f, c, nrep=1, threads=None):
    nl = cfg.nlo
    sc = np.array([c[k] for k in ("dxo", "dto", "delek", "rhooc", "cpoc", "ycexp", "hmoc")])
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        for a in (sc, np.asarray(cfg.gpoc[:nl - 1]), np.asarray(cfg.hoc[:nl]), np.asarray(cfg.ah2oc[:nl]),
                  np.asarray(cfg.ah4oc[:nl])):
            fh.write(np.asarray(a, dtype=np.float64).tobytes())
        for k in ("po", "pom", "qo", "wekpo", "entoc", "tauxo", "tauyo", "wekto", "sst"):
            fh.write(np.asfortranarray(f[k], dtype=np.float64).tobytes(order="F"))
    env = dict(os.environ, OMP_NUM_THREADS=str(threads or 1))
    env.setdefault("OMP_STACKSIZE", "64M")

    def big_stack():   # monnc_comp's work arrays are automatic (on the stack): 7 MB each at 961 x 961
        import resource
        resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    subprocess.check_call([os.path.join(wrk, "mon_driver"), str(nrep)], cwd=wrk, env=env, preexec_fn=big_stack)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
    return out[:-1], out[-1]


if __name__ == "__main__":
    import ref_binding
    from qgcm_hip import preset
    timing = len(sys.argv) > 1 and sys.argv[1] == "time"
    cases = [("box_natl5", "natl5")] if timing else [("box_tiny", "box_tiny"), ("cyc_tiny", "cyc_tiny"),
                                                       ("box_tiny5", "box_tiny5"), ("box_tiny2", "box_tiny2"),
                                                       ("cyc_tiny6", "cyc_tiny6")]
    for refcfg, name in cases:
        a = ref_binding.CONFIGS[refcfg]
        cfg = preset(name)
        wrk = tempfile.mkdtemp(prefix="monnc_")
        try:
            build(wrk, a[:8], cfg.cyclic)
            if timing:
                from qgcm_hip import synth
                po = synth.gaussian_eddy(cfg, noise=1e-3)
                g = dict(steps26_po=po, steps26_pom=0.999 * po, steps26_qo=1e-6 * po, steps26_qom=1e-6 * po)
                f, c = inputs(cfg, g)
                nth = int(sys.argv[2]) if len(sys.argv) > 2 else 16
                run(wrk, cfg, f, c, 1, nth)
                _, t = run(wrk, cfg, f, c, 10, nth)
                sys.stderr.write("host monnc_comp (ocean only) at %dx%dx%d, %d threads: %.2f ms per call\n"
                                 % (cfg.nxpo, cfg.nypo, cfg.nlo, nth, 1e3 * t))
                continue
            g = np.load(os.path.join(HERE, name + ".npz"))
            f, c = inputs(cfg, g)
            vec, _ = run(wrk, cfg, f, c)
            out = {"in_" + k: v for k, v in f.items()}
            out.update({"c_" + k: np.float64(v) for k, v in c.items()})
            out["monitors"] = vec
            np.savez_compressed(os.path.join(HERE, "mon_%s.npz" % name), **out)
            sys.stderr.write("wrote mon_%s.npz (%d values)\n" % (name, len(vec)))
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
