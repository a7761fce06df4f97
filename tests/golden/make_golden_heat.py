#!/usr/bin/env python3
"""Golden values of the atmospheric mixed layer (aml / amladf, src/amlsubs.F) and of the heat half of xforc
(src/xfosubs.F:711-853 with bilint and fsprim) from the TRUE reference.

Compiles the reference's xfosubs.F, amlsubs.F, intsubs.f and the data modules unmodified, as a coupled model, with a
small driver of this script's own, in a temporary directory (one build per case: the dimensions are compile-time
PARAMETERs, substituted into the coupled example's parameters_data.F; -Dcyclic_ocean is a build option; no -fopenmp,
so every sum of the reference runs serially in its written order).  xfosubs.F is preprocessed with -DPRIVATE=PUBLIC, as
make_golden_xforc.py does, so that the driver can call bilint and fsprim.  The radiation set-up (radiat) is not run:
the driver sets every constant by hand to the distinct non-zero values of double-gyre magnitude recorded in the
fixture (c_*); the grid spacings, derived constants and coordinate vectors are computed by this script and read in.  It reads seeded smooth pa, pam (3 layers), pom, sstm, ast, astm, hmixa, hmixam, xc1ast, dtopat and runs

    K = 3 cycles of [ call xforc ; nstr = 3 x call aml ]        with pa / pam / pom / sstm held

writing after every call what the call produced:
    x<c>_*   after xforc of cycle c:  fnetoc, fnetat, wekta, uekat, vekat, arlaav, slhfav, oradav, arocav
    a<c><s>_* after aml s of cycle c: ast, astm, hmixa, hmixam, entat, xan, enisat, eninat, cfraat, centat
and once asto (bilint of the initial astm), the two fsprim tables and the coordinate vectors xta, yta, xto, yto.
All reference sources, objects and .mod files stay in the temporary directory, which is deleted.

The step kernel's workgroup tile is 64 x 8 T points (k_aml.h), so the (96, 24, ..) case crosses a tile boundary in x
and in y.  The temperature fields carry a warm patch on the zonal seam next to the northern wall (away from the cells
above the ocean), where astm passes tat(1): every branch of the step is taken there, at the wall, at the seam and in
the interior, and the assertions at the end of this script check that on the reference's own outputs.

The cases and what each is for:
  heat_cpl_tiny    the smallest coupled grid, plain (xcexp = 1, xc1ast = dtopat = 0), ndxr = 12
  heat_odd5        odd ndxr
  heat_cyc4        cyclic ocean as wide as the atmosphere (bilint's wrapped columns)
  heat_wide        (96, 24): two aml tile columns and three tile rows
  heat_cpl_small   ndxr = 16, the production refinement: k_xf_heat_oc's loop over the ndxr^2 ocean points of a cell
                   takes four rounds of 64
  heat_cyc72       cyclic, 288 cells above the ocean: a second round of k_xf_heat_final's loops of stride 256; the
                   last aml tile is 8 columns wide
  heat_300         320 cells above the ocean; five aml tile columns with a tail of 44; nxpa = 301, so aml reads uekat,
                   vekat and wekta that the momentum kernels produced in more than one block

  python tests/golden/make_golden_heat.py           # writes tests/golden/heat_*.npz
  python tests/golden/make_golden_heat.py NAME ...  # writes only the named cases
  python tests/golden/make_golden_heat.py time [N]  # the reference's xforc (N = 16 threads) and aml (one) at cpl_natl5
"""
import io
import os
import re
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
K, NSTR = 3, 3
# the constants the driver sets, in the order it reads them (SI units).  The diffusivities are the double-gyre
# input.params values scaled from its 80 km atmosphere to the case's dxa (same grid-scale damping rate).
CNAMES = ("dxo", "cdat", "raoro", "hmat", "hmoc", "bccoat", "bccooc", "dta", "hmamin", "hmadmp", "rrcpat", "tat1",
          "tat2", "xcexp", "at2d", "at4d", "ahmd", "aface1", "aface2", "bface", "cface", "dface", "gpat1", "gpat2",
          "fspco", "xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup", "C1down")


def constants(dims, plain):
    ndxr = dims[4]
    dxo = 5.0e3
    r = ndxr * dxo / 8.0e4
    return dict(dxo=dxo, cdat=1.3e-3, raoro=1.0e-3, hmat=1.0e3, hmoc=1.0e2, bccoat=1.0, bccooc=0.2, dta=180.0,
                hmamin=100.0, hmadmp=0.15, rrcpat=1.0e-3, tat1=30.0, tat2=40.0, xcexp=1.0 if plain else 0.9,
                at2d=2.5e4 * r * r, at4d=2.0e14 * r ** 4, ahmd=2.0e5 * r * r, aface1=1.1e-6, aface2=-0.4e-6,
                bface=0.7e-6, cface=-0.3e-6, dface=2.3e-4, gpat1=1.2, gpat2=0.4, fspco=80.0, xlamda=35.0, D0up=6.5,
                Dmup=5.1, Dmdown=-5.6, Adown11=-4.7e-3, Bmup=8.9e-3, B1down=-3.1e-3, Cmup=-2.2e-3, C1down=1.3e-3)


GNAMES = ("dxa", "dya", "dyo", "hdxam1", "dxam2", "xla", "yla", "rdxaf0", "rdxof0", "tdta")


def geometry(dims, C):
    """The grid spacings, the derived constants and the T-point coordinates of both grids (the ocean centred in the
    atmosphere, as MODULE parameters places it), computed here and handed to the driver."""
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    fnot = float(FNOT.replace("D", "e"))
    dxo = C["dxo"]
    dxa = ndxr * dxo
    nx1, ny1 = 1 + (nxta - nxaooc) // 2, 1 + (nyta - nyaooc) // 2
    yla = nyta * dxa
    G = dict(dxa=dxa, dya=dxa, dyo=dxo, hdxam1=0.5 / dxa, dxam2=1.0 / (dxa * dxa), xla=nxta * dxa, yla=yla,
             rdxaf0=1.0 / (dxa * fnot), rdxof0=1.0 / (dxo * fnot), tdta=2.0 * C["dta"])
    G["xta"] = np.arange(nxta) * dxa + 0.5 * dxa
    G["yta"] = np.arange(nyta) * dxa + 0.5 * dxa
    G["xto"] = (np.arange(nxaooc * ndxr) * dxo + (nx1 - 1) * dxa) + 0.5 * dxo
    G["yto"] = ((ny1 - 1) * dxa + np.arange(nyaooc * ndxr) * dxo) + 0.5 * dxo
    G["ytarel"] = G["yta"] - 0.5 * yla
    G["ytorel"] = G["yto"] - 0.5 * yla
    return G


DRIVER = r"""
program heat_driver
  use parameters
  use atconst
  use occonst
  use athomog, only : xan, enisat, eninat
  use atstate, only : pa, pam, entat, wekta
  use ochomog
  use ocstate, only : pom
  use intrfac
  use radiate
  use monitor, only : arlaav, slhfav, oradav, arocav, cfraat, centat
  use xfosubs
  use amlsubs
  implicit none
  integer, parameter :: ncst = 34
  integer :: ncyc, ns, nrep, c, s, r, j
  integer(8) :: c0, c1, cr
  double precision :: cst(ncst), geo(10), secx, seca
#ifndef TIMING
  double precision :: asto(nxto,nyto), fsa(nyta), fso(nyto)
#endif
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) ncyc, ns, nrep
  read (10) cst
  dxo = cst(1); cdat = cst(2); raoro = cst(3); hmat = cst(4); hmoc = cst(5); bccoat = cst(6); bccooc = cst(7)
  dta = cst(8); hmamin = cst(9); hmadmp = cst(10); rrcpat = cst(11); tat = 0.0d0; tat(1) = cst(12); tat(2) = cst(13)
  xcexp = cst(14); at2d = cst(15); at4d = cst(16); ahmd = cst(17); aface(1) = cst(18); aface(2) = cst(19)
  bface = cst(20); cface = cst(21); dface = cst(22); gpat(1) = cst(23); gpat(2) = cst(24); fspco = cst(25)
  xlamda = cst(26); D0up = cst(27); Dmup = cst(28); Dmdown = cst(29); Adown = 0.0d0; Adown(1,1) = cst(30)
  Bmup = cst(31); B1down = cst(32); Cmup = cst(33); C1down = cst(34)
  ! the grids and the derived constants come from the script (in.bin), which computes them on its own side
  read (10) geo
  dxa = geo(1); dya = geo(2); dyo = geo(3); hdxam1 = geo(4); dxam2 = geo(5); xla = geo(6); yla = geo(7)
  rdxaf0 = geo(8); rdxof0 = geo(9); tdta = geo(10)
  read (10) xta, yta, ytarel, xto, yto, ytorel
  pom = 0.0d0
  read (10) pa, pam, pom(:,:,1), sstm, ast, astm, hmixa, hmixam, xc1ast, dtopat
  close (10)
  xan = 0.0d0; enisat = 0.0d0; eninat = 0.0d0
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
#ifndef TIMING
  call bilint (xta, yta, nxta, nyta, astm, xto, yto, nxto, nyto, asto, 1.0d0)
  do j=1,nyta
    fsa(j) = fsprim( ytarel(j) )
  enddo
  do j=1,nyto
    fso(j) = fsprim( ytorel(j) )
  enddo
  write (11) asto, fsa, fso, xta, yta, xto, yto
#endif
  secx = 0.0d0; seca = 0.0d0
  do c = 1, ncyc
    call xforc
#ifndef TIMING
    write (11) fnetoc, fnetat, wekta, uekat, vekat, arlaav, slhfav, oradav, arocav
#endif
    do s = 1, ns
      call aml
#ifndef TIMING
      write (11) ast, astm, hmixa, hmixam, entat, xan(1), enisat(1), eninat(1), cfraat, centat
#endif
    end do
  end do
  if (nrep > 0) then
    call system_clock(c0, cr)
    do r = 1, nrep
      call xforc
    end do
    call system_clock(c1)
    secx = dble(c1 - c0)/dble(cr)/dble(nrep)
    call system_clock(c0, cr)
    do r = 1, nrep
      call aml
    end do
    call system_clock(c1)
    seca = dble(c1 - c0)/dble(cr)/dble(nrep)
  end if
  write (11) secx, seca
  close (11)
end program heat_driver
"""

# (file, (nxta, nyta, nxaooc, nyaooc, ndxr), cyclic ocean, plain: xcexp = 1 and xc1ast = dtopat = 0)
CASES = [("heat_cpl_tiny", (16, 12, 4, 3, 12), False, True),
         ("heat_odd5", (16, 12, 6, 4, 5), False, False),
         ("heat_cyc4", (16, 12, 16, 4, 4), True, False),
         ("heat_wide", (96, 24, 6, 5, 4), False, False),
         ("heat_cpl_small", (32, 20, 6, 5, 16), False, False),
         ("heat_cyc72", (72, 12, 72, 4, 4), True, False),
         ("heat_300", (300, 12, 80, 4, 4), False, False)]
NATL5 = (384, 96, 60, 60, 16)


def build(wrk, dims, cyc, timing=False):
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
    with open(os.path.join(wrk, "heat_driver.F90"), "w") as f:
        f.write(DRIVER)
    omp = ["-fopenmp"] if timing else []
    q = ["-Dcyclic_ocean"] if cyc else []
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2"] + q + omp
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS] + [os.path.join(src, "intsubs.f")]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    # (timing: OpenMP on and no -DPRIVATE=PUBLIC - the word also names the OpenMP clauses - so bilint / fsprim are not called)
    subprocess.check_call(fc + ([] if timing else ["-DPRIVATE=PUBLIC"]) + ["-c", "-I" + src,
                                                                           os.path.join(src, "xfosubs.F")], cwd=wrk)
    # (amlsubs.F always without -fopenmp: flang refuses its REDUCTION(-:centsm) clause, deprecated since OpenMP 5.2, and
    #  the source stays unmodified - so the timing mode runs aml on ONE thread and xforc on all of them)
    subprocess.check_call([a for a in fc if a != "-fopenmp"] + ["-c", "-I" + src, os.path.join(src, "amlsubs.F")], cwd=wrk)
    objs += ["xfosubs.o", "amlsubs.o"]
    subprocess.check_call([FC, "-cpp", "-O2"] + q + (["-DTIMING"] if timing else []) + omp + ["-c", "heat_driver.F90"],
                          cwd=wrk)
    subprocess.check_call([FC, "-o", "heat_driver", "heat_driver.o"] + objs + omp, cwd=wrk)


def inputs(dims, cyc, plain, C, seed):
    """Seeded smooth inputs of spun-up magnitude.  p-grid fields repeat column 1 in column nx; T-grid fields are
    periodic over nxta cells.  ast / astm: a few K around -5 with a warm patch (peak above tat(1)) centred on the zonal
    seam one row below the northern wall; hmixa / hmixam: hmat +- 100 m with a thin spot near the southern wall."""
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    rng = np.random.default_rng(seed)

    def modes(x, y, amp, periodic, nmodes):
        f = np.zeros((x.size, y.size))
        for _ in range(nmodes):
            kx, ky = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            a, ph, ph2 = rng.standard_normal() * amp, rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            fx = np.cos(2 * np.pi * kx * x + ph) if periodic else np.sin(np.pi * kx * x + 0.3 * ph)
            f = f + a * fx[:, None] * np.cos(np.pi * ky * y + ph2)[None, :]
        return f

    xp, yp = np.arange(nxta + 1) / float(nxta), np.arange(nyta + 1) / float(nyta)
    xt, yt = (np.arange(nxta) + 0.5) / nxta, (np.arange(nyta) + 0.5) / nyta
    nxto, nyto = nxaooc * ndxr, nyaooc * ndxr
    xo, yo = np.arange(nxto + 1) / float(nxto), np.arange(nyto + 1) / float(nyto)
    xot, yot = (np.arange(nxto) + 0.5) / nxto, (np.arange(nyto) + 0.5) / nyto

    def pfield(amp, jet):
        f = jet * np.cos(np.pi * yp)[None, :] + modes(xp, yp, amp, True, 5)
        f[-1, :] = f[0, :]
        return f

    # layer-1 pressure: a jet of ~8 m/s (u = -dp/dy / f0) with eddies of a third of that; weaker aloft
    jet = 8.0 * nyta * (ndxr * C["dxo"]) * float(FNOT.replace("D", "e")) / np.pi
    pam = np.stack([pfield(0.3 * a, a) for a in (jet, 0.4 * jet, 0.15 * jet)], axis=2)
    pa = pam + np.stack([pfield(0.01 * a, 0.0) for a in (jet, 0.4 * jet, 0.15 * jet)], axis=2)
    pom = 5.0 * np.cos(np.pi * yo)[None, :] + modes(xo, yo, 1.5, cyc, 6)
    if cyc:
        pom[-1, :] = pom[0, :]
    sstm = 4.0 * np.cos(np.pi * yot)[None, :] + modes(xot, yot, 1.0, cyc, 5)
    # the warm patch: distance in cells from (the seam, T row nyta-1), periodic in x
    ci = np.minimum(np.arange(nxta) + 0.5, nxta - (np.arange(nxta) + 0.5))
    cj = np.arange(nyta) + 0.5 - (nyta - 1.5)
    patch = np.exp(-(ci[:, None] ** 2 + cj[None, :] ** 2) / (2.0 * 2.2 ** 2))
    astm = -5.0 + modes(xt, yt, 2.5, True, 5) + 41.0 * patch
    ast = astm + modes(xt, yt, 0.3, True, 4) + 1.5 * patch
    # ... and a thin spot (a few metres below hmamin) in the south-west quarter, so that the hmamin floor is taken
    di = np.arange(nxta) - float(nxta // 4)
    dj = np.arange(nyta) - 2.0
    thin = np.exp(-(di[:, None] ** 2 + dj[None, :] ** 2) / (2.0 * 2.5 ** 2))
    hmixam = C["hmat"] + modes(xt, yt, 40.0, True, 5)
    hmixam = hmixam + (C["hmamin"] - 12.0 - hmixam) * thin
    hmixa = hmixam + modes(xt, yt, 3.0, True, 4) * (1.0 - thin)
    if plain:
        xc1ast, dtopat = np.zeros((nxta, nyta)), np.zeros((nxta + 1, nyta + 1))
    else:
        xc1ast = modes(xt, yt, 0.5, True, 4)
        dtopat = modes(xp, yp, 60.0, True, 4)
        dtopat[-1, :] = dtopat[0, :]
    return dict(pa=pa, pam=pam, pom=pom, sstm=sstm, ast=ast, astm=astm, hmixa=hmixa, hmixam=hmixam, xc1ast=xc1ast,
                dtopat=dtopat)


INPUT_ORDER = ("pa", "pam", "pom", "sstm", "ast", "astm", "hmixa", "hmixam", "xc1ast", "dtopat")


def shapes(dims):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    nxpa, nypa, nxto, nyto = nxta + 1, nyta + 1, nxaooc * ndxr, nyaooc * ndxr
    once = [("asto", (nxto, nyto)), ("fsa", (nyta,)), ("fso", (nyto,)), ("xta", (nxta,)), ("yta", (nyta,)),
            ("xto", (nxto,)), ("yto", (nyto,))]
    xf = [("fnetoc", (nxto, nyto)), ("fnetat", (nxta, nyta)), ("wekta", (nxta, nyta)), ("uekat", (nxpa, nyta)),
          ("vekat", (nxta, nypa)), ("arlaav", ()), ("slhfav", ()), ("oradav", ()), ("arocav", ())]
    am = [("ast", (nxta, nyta)), ("astm", (nxta, nyta)), ("hmixa", (nxta, nyta)), ("hmixam", (nxta, nyta)),
          ("entat", (nxpa, nypa)), ("xan", ()), ("enisat", ()), ("eninat", ()), ("cfraat", ()), ("centat", ())]
    return once, xf, am


def _big_stack():
    import resource
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def run(wrk, dims, C, F, ncyc=K, ns=NSTR, nrep=0, env=None, timing=False):
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([ncyc, ns, nrep], dtype=np.int32).tobytes())
        fh.write(np.array([C[k] for k in CNAMES]).tobytes())
        G = geometry(dims, C)
        fh.write(np.array([G[k] for k in GNAMES]).tobytes())
        for k in ("xta", "yta", "ytarel", "xto", "yto", "ytorel"):
            fh.write(np.ascontiguousarray(G[k], dtype=np.float64).tobytes())
        for k in INPUT_ORDER:
            fh.write(np.asfortranarray(F[k], dtype=np.float64).tobytes(order="F"))
    subprocess.check_call([os.path.join(wrk, "heat_driver")], cwd=wrk, env=env, preexec_fn=_big_stack)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
    if timing:
        return dict(xforc=out[-2], aml=out[-1])
    res, o = {}, 0

    def take(prefix, lst):
        nonlocal o
        for name, shp in lst:
            n = int(np.prod(shp)) if shp else 1
            v = out[o:o + n]
            res[prefix + name] = v.reshape(shp, order="F").copy() if shp else np.float64(v[0])
            o += n

    once, xf, am = shapes(dims)
    take("t_", once)
    for c in range(ncyc):
        take("x%d_" % c, xf)
        for s in range(ns):
            take("a%d%d_" % (c, s), am)
    assert o + 2 == len(out)
    return res


def time_reference(nthreads):
    """Seconds per call of the reference's xforc (both halves) and of its aml at cpl_natl5."""
    wrk = tempfile.mkdtemp(prefix="heat_")
    try:
        build(wrk, NATL5, False, timing=True)
        C = constants(NATL5, False)
        env = dict(os.environ, OMP_NUM_THREADS=str(nthreads), OMP_STACKSIZE="2G")
        return run(wrk, NATL5, C, inputs(NATL5, False, False, C, 5), ncyc=1, ns=1, nrep=5, env=env, timing=True)
    finally:
        shutil.rmtree(wrk, ignore_errors=True)


def check_branches(name, dims, cyc, C, F, res):
    """Every branch of the step must be taken by the reference itself, else a test could pass by skipping it.  The
    branch masks come from the numpy restatement (tests/numpy_heat.py) fed with the reference's own inputs of every
    call, and the restatement must give the reference's fields bit for bit while it is at it."""
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy_heat as nh
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    g = dict(c_dims=np.array(dims), c_nx1=1 + (nxta - nxaooc) // 2, c_ny1=1 + (nyta - nyaooc) // 2, c_cyclic=int(cyc),
             c_fnot=float(FNOT.replace("D", "e")), c_K=K, c_nstr=NSTR)
    g.update({"c_" + k: v for k, v in C.items()})
    P = nh.params(g)
    T = nh.bilint_tables(res["t_xta"], res["t_yta"], res["t_xto"], res["t_yto"], P["dxa"], P["dya"])
    got = dict(diab=False, floor=False, conv=False, none=False)
    S = {k: F[k] for k in ("ast", "astm", "hmixa", "hmixam")}
    for c in range(K):
        H = nh.heat(S["astm"], S["hmixam"], F["sstm"], F["pam"], F["dtopat"], res["t_fsa"], res["t_fso"], T, P)
        fa = res["x%d_fnetat" % c]
        assert np.array_equal(H["fnetat"], fa) and np.array_equal(H["fnetoc"], res["x%d_fnetoc" % c]), (name, c)
        assert np.all(fa[H["ocean"]] != 0.0) and np.all(fa[H["ocean"]] != H["fnetat_land"][H["ocean"]]), (name, c)
        for s in range(NSTR):
            A = nh.aml(S, fa, res["x%d_wekta" % c], res["x%d_uekat" % c], res["x%d_vekat" % c], F["pa"], F["pam"],
                       F["xc1ast"], F["dtopat"], P)
            S = {k: res["a%d%d_%s" % (c, s, k)] for k in ("ast", "astm", "hmixa", "hmixam")}
            for k in S:
                assert np.all(np.isfinite(S[k])) and np.array_equal(A[k], S[k]), (name, c, s, k)
            b = A["branches"]
            for k in ("diab", "floor", "conv"):
                got[k] |= bool(b[k].any())
            got["none"] |= bool((~b["diab"] & ~b["floor"] & ~b["conv"])[1:-1, 1:-1].any())
    cf = [float(res["a%d%d_cfraat" % (c, s)]) for c in range(K) for s in range(NSTR)]
    assert all(got.values()) and any(0.0 < v < 1.0 for v in cf), (name, got, cf)


def packed_size(d):
    """The size of the compressed file that np.savez_compressed would write for d."""
    buf = io.BytesIO()
    np.savez_compressed(buf, **d)
    return buf.getbuffer().nbytes


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
        t = time_reference(n)
        print("reference at cpl_natl5 (385x97 / 961x961, ndxr 16): xforc (both halves) %.2f ms per call on %d threads, "
              "aml %.3f ms per call on one thread (built without OpenMP)" % (1e3 * t["xforc"], n, 1e3 * t["aml"]))
        sys.exit(0)
    only = sys.argv[1:]
    assert all(n in [c[0] for c in CASES] for n in only), only
    for ic, (name, dims, cyc, plain) in enumerate(CASES):
        if only and name not in only:
            continue
        C = constants(dims, plain)
        F = inputs(dims, cyc, plain, C, 300 + ic)
        wrk = tempfile.mkdtemp(prefix="heat_")
        try:
            build(wrk, dims, cyc)
            res = run(wrk, dims, C, F)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        check_branches(name, dims, cyc, C, F, res)
        sys.stderr.write("%s: cfraat %s\n" % (name, " ".join("%.4f" % res["a%d%d_cfraat" % (c, s)] for c in range(K) for s in range(NSTR))))
        sys.stderr.write("%s: max|ast| %s\n" % (name, " ".join("%.2f" % np.abs(res["a%d%d_ast" % (c, s)]).max() for c in range(K) for s in range(NSTR))))
        sys.stderr.write("%s: hmixa range %s\n" % (name, " ".join("%.0f-%.0f" % (res["a%d%d_hmixa" % (c, s)].min(), res["a%d%d_hmixa" % (c, s)].max()) for c in range(K) for s in range(NSTR))))
        nxta, nyta, nxaooc, nyaooc, ndxr = dims
        out = dict(c_dims=np.array(dims, dtype=np.int64), c_cyclic=np.int64(cyc), c_K=np.int64(K), c_nstr=np.int64(NSTR),
                   c_nx1=np.int64(1 + (nxta - nxaooc) // 2), c_ny1=np.int64(1 + (nyta - nyaooc) // 2),
                   c_fnot=np.float64(float(FNOT.replace("D", "e"))))
        out.update({"c_" + k: np.float64(v) for k, v in C.items()})
        out.update({"in_" + k: np.asfortranarray(v) for k, v in F.items()})
        out.update(res)
        # (one file per case, or several where the nine aml records would push it past the size limit of a committed
        #  file: <case>.npz with everything else and <case>_aml.npz, <case>_aml2.npz, ... with the a<c><s>_* records,
        #  cut call by call into as few parts as stay under the limit)
        parts = {name: out}
        if sum(np.asarray(v).nbytes for v in out.values()) > 900000:
            parts = {name: {k: v for k, v in out.items() if not re.match(r"a\d\d_", k)}}
            calls = ["a%d%d_" % (c, s) for c in range(K) for s in range(NSTR)]
            for n in range(1, len(calls) + 1):
                cut = [calls[len(calls) * i // n:len(calls) * (i + 1) // n] for i in range(n)]
                aml = {name + "_aml" + (str(i + 1) if i else ""): {k: v for k, v in out.items() if k[:4] in grp}
                       for i, grp in enumerate(cut)}
                if all(packed_size(d) < (1 << 20) for d in aml.values()):
                    break
            parts.update(aml)
            assert sum(len(d) for d in parts.values()) == len(out)
        for fn, d in parts.items():
            path = os.path.join(HERE, "%s.npz" % fn)
            np.savez_compressed(path, **d)
            size = os.path.getsize(path)
            assert size < (1 << 20), (fn, size)
            sys.stderr.write("wrote %s.npz (%d bytes)\n" % (fn, size))
