#!/usr/bin/env python3
"""Golden values of the momentum half of xforc (src/xfosubs.F:137-709) from the TRUE reference.

Compiles the reference's xfosubs.F unmodified, as a coupled model (ocean_only is never defined), with the modules it
USEs and a small driver of this script's own, in a temporary directory (one build per case: the dimensions are
compile-time PARAMETERs, substituted into the coupled example's parameters_data.F; -Dtau_udiff and -Dcyclic_ocean are
build options).  xfosubs.F is preprocessed with -DPRIVATE=PUBLIC so that the driver can read the bicubic weight tables
of MODULE xfosubs (besides the access attributes the word occurs only in OpenMP directives, which are comments in a
build without -fopenmp).  The driver sets the constants to the values below, reads two seeded, smooth pam / pom pairs
of spun-up magnitude, calls xforc on each and writes the twelve momentum fields, the four line integrals and, once,
the five weight tables.  Every thermodynamic input is zero (fnetoc / fnetat are not recorded).  All reference sources,
objects and .mod files stay in the temporary directory, which is deleted.

The cases and what each is for (the launch geometry is that of qgcm_hip_xforc: 256 threads along a row for the
pointwise kernels, 64 for k_xf_wekpa, XF_CX = 8 atmosphere cells per workgroup in k_xf_fine, one workgroup striding by
256 in k_xf_lines):
  xf_cpl_tiny / _ud   the smallest coupled grid, without and with the shear term (tau_udiff)
  xf_cpl_small_ud     ndxr = 16, the production refinement
  xf_odd5_ud          odd ndxr (half weights on both edges of a cell)
  xf_cyc4_ud          cyclic ocean as wide as the atmosphere (the ocean's own line integrals)
  xf_wide_ud          nxpa = 301: two blocks of 256 and five of 64 along the atmosphere's rows; nxta % 8 = 4: a tail
                      workgroup of k_xf_fine that holds column nxta and its wrap; nxpo = 321: two blocks along the
                      ocean's rows (k_xf_tauo, k_wekto, k_wekpo)
  xf_edge_ud          nxpa = nxpo = 257: the second block holds exactly one live thread, on the atmosphere the copy
                      column ia = nxpa
  xf_cycwide_ud       cyclic ocean with nxpo = 361: two rounds of k_xf_lines' loop over the ocean; nxta % 8 = 2

  python tests/golden/make_golden_xforc.py           # writes tests/golden/xf_*.npz
  python tests/golden/make_golden_xforc.py NAME ...  # writes only the named cases
  python tests/golden/make_golden_xforc.py time [N]  # the reference's xforc at cpl_natl5 on N (16) threads
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("QGCM_REFERENCE", "/root/reference")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
MODS = ["atconst_data.F", "occonst_data.F", "athomog_data.F", "ochomog_data.F", "atstate_data.F", "ocstate_data.F",
        "intrfac_data.F", "radiate_data.F", "monitor_data.F"]
FNOT, BETA = "9.37456D-05", "1.75360D-11"
# the constants the driver sets (SI units; dxa = ndxr*dxo, dya = dxa, dyo = dxo as src/q-gcm.F:380-413)
CONST = dict(dxo=5.0e3, cdat=1.3e-3, raoro=1.0e-3, hmat=1.0e3, hmoc=1.0e2, bccoat=1.0, bccooc=0.2)

DRIVER = r"""
program xf_driver
  use parameters
  use atconst
  use occonst
  use athomog, only : txisat, txinat
  use atstate, only : pam, wekpa, wekta
  use ochomog
  use ocstate, only : pom, wekpo, wekto
  use intrfac
  use radiate
  use xfosubs
  implicit none
  integer :: n, s, nrep, r
  integer(8) :: c0, c1, cr
  double precision :: cst(7), sec, txo(2)
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) n, nrep
  read (10) cst
  dxo = cst(1); cdat = cst(2); raoro = cst(3); hmat = cst(4); hmoc = cst(5); bccoat = cst(6); bccooc = cst(7)
  dyo = dxo; dxa = ndxr*dxo; dya = dxa
  rdxaf0 = 1.0d0/(dxa*fnot)
  rdxof0 = 1.0d0/(dxo*fnot)
  ! the thermodynamic half runs on zeros (gpat and yla are divisors)
  pam = 0.0d0; pom = 0.0d0; sstm = 0.0d0; astm = 0.0d0; hmixam = 0.0d0; hmadmp = 0.0d0; dtopat = 0.0d0
  xta = 0.0d0; yta = 0.0d0; xto = 0.0d0; yto = 0.0d0; ytarel = 0.0d0; ytorel = 0.0d0; yla = 1.0d0; gpat = 1.0d0
  fspco = 0.0d0; xlamda = 0.0d0; Adown = 0.0d0; Bmup = 0.0d0; B1down = 0.0d0; Cmup = 0.0d0; C1down = 0.0d0
  D0up = 0.0d0; Dmup = 0.0d0; Dmdown = 0.0d0
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
  sec = 0.0d0
  do s = 1, n
    read (10) pam(:,:,1), pom(:,:,1)
    call xforc
    if (s == n .and. nrep > 0) then
      call system_clock(c0, cr)
      do r = 1, nrep
        call xforc
      end do
      call system_clock(c1)
      sec = dble(c1 - c0)/dble(cr)/dble(nrep)
    end if
    txo = 0.0d0
#ifdef cyclic_ocean
    txo(1) = txisoc; txo(2) = txinoc
#endif
#ifndef TIMING
    write (11) tauxa, tauya, uekat, vekat, wekta, wekpa, tauxo, tauyo, wekto, wekpo, txisat, txinat, txo
#endif
  end do
  close (10)
#ifndef TIMING
  write (11) stbbb, stbus, stbvs, stbun, stbvn
#endif
  write (11) sec
  close (11)
end program xf_driver
"""

# (file, (nxta, nyta, nxaooc, nyaooc, ndxr), cyclic ocean, tau_udiff)
CASES = [("xf_cpl_tiny", (16, 12, 4, 3, 12), False, False),
         ("xf_cpl_tiny_ud", (16, 12, 4, 3, 12), False, True),
         ("xf_cpl_small_ud", (32, 20, 6, 5, 16), False, True),
         ("xf_odd5_ud", (16, 12, 6, 4, 5), False, True),
         ("xf_cyc4_ud", (16, 12, 16, 4, 4), True, True),
         ("xf_wide_ud", (300, 12, 80, 4, 4), False, True),
         ("xf_edge_ud", (256, 12, 64, 4, 4), False, True),
         ("xf_cycwide_ud", (90, 12, 90, 4, 4), True, True)]
NATL5 = (384, 96, 60, 60, 16)


def build(wrk, dims, cyc, udiff, timing=False):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    src = os.path.join(REF, "src")
    with open(os.path.join(REF, "examples", "double_gyre_coupled", "parameters_data.F.dg_oo")) as f:
        lines = f.read().split("\n")
    hits = 0
    for i, ln in enumerate(lines):
        if ln.startswith("      PARAMETER ( nxta = "):
            lines[i] = "      PARAMETER ( nxta = %d, nyta = %d, nla = 3 )" % (nxta, nyta)
            hits += 1
        elif ln.startswith("      PARAMETER ( nxaooc = "):
            lines[i] = "      PARAMETER ( nxaooc = %d, nyaooc = %d, ndxr = %d, nlo = 3 )" % (nxaooc, nyaooc, ndxr)
            hits += 1
        elif ln.startswith("      PARAMETER ( fnot = "):
            lines[i] = "      PARAMETER ( fnot = %s, beta = %s )" % (FNOT, BETA)
            hits += 1
        elif ln.startswith("      PARAMETER ( nscvat = ") and not timing:
            lines[i] = ln.replace("nscvat =  2", "nscvat =  1")  # (any nxta, nyta; the covariances are not built)
        elif ln.startswith("     &            nscvoc = 16") and not timing:
            lines[i] = ln.replace("nscvoc = 16", "nscvoc = 1")
    assert hits == 3
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(wrk, "xf_driver.F90"), "w") as f:
        f.write(DRIVER)
    omp = ["-fopenmp"] if timing else []
    q = (["-Dcyclic_ocean"] if cyc else []) + (["-Dtau_udiff"] if udiff else [])
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2"] + q + omp
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    # (timing: OpenMP on and no -DPRIVATE=PUBLIC - the word also names the OpenMP clauses - so no table is read back)
    subprocess.check_call(fc + ([] if timing else ["-DPRIVATE=PUBLIC"]) + ["-c", "-I" + src,
                                                                           os.path.join(src, "xfosubs.F")], cwd=wrk)
    objs.append("xfosubs.o")
    subprocess.check_call([FC, "-cpp", "-O2"] + q + (["-DTIMING"] if timing else []) + omp + ["-c", "xf_driver.F90"],
                          cwd=wrk)
    subprocess.check_call([FC, "-o", "xf_driver", "xf_driver.o"] + objs + omp, cwd=wrk)


def smooth_pair(dims, cyc, seed):
    """A smooth (pam(:,:,1), pom(:,:,1)) of spun-up magnitude: a few seeded Fourier modes, zonally periodic where the
    domain is (column nx repeats column 1); jets of ~20 m/s in the atmosphere and ~0.5 m/s in the ocean."""
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    rng = np.random.default_rng(seed)

    def field(nx, ny, amp, periodic, nmodes):
        x = np.arange(nx)[:, None] / (nx - 1.0)
        y = np.arange(ny)[None, :] / (ny - 1.0)
        f = amp * np.cos(np.pi * y) * (1.0 + 0.0 * x)
        for _ in range(nmodes):
            kx, ky = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            a, ph, ph2 = rng.standard_normal() * amp * 0.3, rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            fx = np.cos(2 * np.pi * kx * x + ph) if periodic else np.sin(np.pi * kx * x + 0.3 * ph)
            f = f + a * fx * np.cos(np.pi * ky * y + ph2)
        if periodic:
            f[-1, :] = f[0, :]
        return np.asfortranarray(f)

    pam = field(nxta + 1, nyta + 1, 2.0e3, True, 5)
    pom = field(nxaooc * ndxr + 1, nyaooc * ndxr + 1, 5.0, cyc, 6)
    return pam, pom


def shapes(dims):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    nxpa, nypa, nxto, nyto = nxta + 1, nyta + 1, nxaooc * ndxr, nyaooc * ndxr
    nxpo, nypo = nxto + 1, nyto + 1
    return [("tauxa", (nxpa, nypa)), ("tauya", (nxpa, nypa)), ("uekat", (nxpa, nyta)), ("vekat", (nxta, nypa)),
            ("wekta", (nxta, nyta)), ("wekpa", (nxpa, nypa)), ("tauxo", (nxpo, nypo)), ("tauyo", (nxpo, nypo)),
            ("wekto", (nxto, nyto)), ("wekpo", (nxpo, nypo)), ("txisat", ()), ("txinat", ()), ("txisoc", ()),
            ("txinoc", ())]


TABLES = ("stbbb", "stbus", "stbvs", "stbun", "stbvn")


def _big_stack():
    import resource
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def run(wrk, dims, pairs, nrep=0, env=None, timing=False):
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([len(pairs), nrep], dtype=np.int32).tobytes())
        fh.write(np.array([CONST[k] for k in ("dxo", "cdat", "raoro", "hmat", "hmoc", "bccoat", "bccooc")]).tobytes())
        for pam, pom in pairs:
            fh.write(np.asfortranarray(pam, dtype=np.float64).tobytes(order="F"))
            fh.write(np.asfortranarray(pom, dtype=np.float64).tobytes(order="F"))
    # (xforc's automatic arrays at ocean resolution, 75 MB each at cpl_natl5, need more than the default stack)
    subprocess.check_call([os.path.join(wrk, "xf_driver")], cwd=wrk, env=env, preexec_fn=_big_stack)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
    if timing:
        return dict(seconds=out[-1])
    res, o = {}, 0
    for s in range(len(pairs)):
        for name, shp in shapes(dims):
            n = int(np.prod(shp)) if shp else 1
            v = out[o:o + n]
            res["out%d_%s" % (s, name)] = v.reshape(shp, order="F").copy() if shp else np.float64(v[0])
            o += n
    ndxr = dims[4]
    for t in TABLES:
        n = 16 * (ndxr + 1) * (ndxr + 1)
        res["tab_" + t] = out[o:o + n].reshape((16, ndxr + 1, ndxr + 1), order="F").copy()
        o += n
    assert o + 1 == len(out)
    return res


def time_xforc(nthreads):
    """Seconds per xforc of the reference (both halves; the thermodynamic one on zeros) at cpl_natl5 with -Dtau_udiff."""
    wrk = tempfile.mkdtemp(prefix="xf_")
    try:
        build(wrk, NATL5, False, True, timing=True)
        env = dict(os.environ, OMP_NUM_THREADS=str(nthreads), OMP_STACKSIZE="2G")
        return run(wrk, NATL5, [smooth_pair(NATL5, False, 5)], nrep=5, env=env, timing=True)["seconds"]
    finally:
        shutil.rmtree(wrk, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
        print("reference xforc at cpl_natl5 (385x97 / 961x961, ndxr 16, tau_udiff): %.1f ms per call on %d threads"
              % (1e3 * time_xforc(n), n))
        sys.exit(0)
    only = sys.argv[1:]
    assert all(n in [c[0] for c in CASES] for n in only), only
    done = {}
    for name, dims, cyc, udiff in CASES:
        if only and name not in only:
            continue
        pairs = [smooth_pair(dims, cyc, 100 + s) for s in range(2)]
        wrk = tempfile.mkdtemp(prefix="xf_")
        try:
            build(wrk, dims, cyc, udiff)
            res = run(wrk, dims, pairs)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        nxta, nyta, nxaooc, nyaooc, ndxr = dims
        out = dict(c_dims=np.array(dims, dtype=np.int64), c_cyclic=np.int64(cyc), c_tau_udiff=np.int64(udiff),
                   c_nx1=np.int64(1 + (nxta - nxaooc) // 2), c_ny1=np.int64(1 + (nyta - nyaooc) // 2),
                   c_fnot=np.float64(float(FNOT.replace("D", "e"))))
        out.update({"c_" + k: np.float64(v) for k, v in CONST.items()})
        for s, (pam, pom) in enumerate(pairs):
            out["in%d_pam1" % s] = pam
            out["in%d_pom1" % s] = pom
        out.update(res)
        path = os.path.join(HERE, "%s.npz" % name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < (1 << 20), (name, size)
        sys.stderr.write("wrote %s.npz (%d bytes)\n" % (name, size))
        done[name] = out
    # the shear term must be visible in the fixtures, else tau_udiff would not be tested
    if "xf_cpl_tiny" in done and "xf_cpl_tiny_ud" in done:
        assert not np.array_equal(done["xf_cpl_tiny"]["out0_tauxo"], done["xf_cpl_tiny_ud"]["out0_tauxo"])
