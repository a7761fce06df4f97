#!/usr/bin/env python3
"""Golden values of xforc (both halves) and of the atmospheric mixed layer from the TRUE reference built as an
ATMOSPHERE-ONLY model (-Datmos_only): the sea below the atmosphere is an SST that is read once and held
(src/q-gcm.F:753-786, sstm = sst), fnetoc and arocsm are skipped (src/xfosubs.F:805-812), no ocean array exists.

Compiles the reference's xfosubs.F, amlsubs.F, intsubs.f and the data modules unmodified with -Datmos_only, and a small
driver of this script's own, in a temporary directory (one build per case: the dimensions are compile-time PARAMETERs,
substituted into the coupled example's parameters_data.F; no -fopenmp, so every sum of the reference runs serially in
its written order).  xfosubs.F is preprocessed with -DPRIVATE=PUBLIC, as make_golden_heat.py does, so that the driver
can call bilint and fsprim.  The constants are make_golden_heat.constants (dxo = 5 km, so that dxa/ndxr == dxo in
floating point: without an ocean handle the library derives dxo that way, and this script asserts the equality per
case); the inputs are make_golden_heat.inputs without pom.  The driver runs

    K = 3 cycles of [ call xforc ; nstr = 3 x call aml ]        with pa / pam / sstm held

writing after every call what the call produced:
    x<c>_*    after xforc of cycle c: fnetat, wekta, uekat, vekat, tauxa, tauya, wekpa, txisat, txinat, arlaav, slhfav,
              oradav, arocav
    a<c><s>_* after aml s of cycle c: ast, astm, hmixa, hmixam, entat, xan, enisat, eninat, cfraat, centat
and once asto (bilint of the initial astm), the table fsprim(ytarel), the coordinate vectors xta, yta, xto, yto and,
as make_golden_xforc.py does, the five bicubic weight tables of MODULE xfosubs (tab_*: at odd ndxr the reference binary's
tables differ in the last bit from its own run-time arithmetic, tests/test_xforc_cpu.py, so a bitwise comparison of
the momentum half needs the tables the reference used).
All reference sources, objects and .mod files stay in the temporary directory, which is deleted.

The cases (nxta, nyta, nxaooc, nyaooc, ndxr) and what each reaches in k_xf_heat_sst / k_xf_heat_atm / k_xf_heat_final:
  ato_tiny    16, 12,  4,  3, 12  plain (xcexp = 1, xc1ast = dtopat = 0); 144 points per cell: two full rounds of 64 lanes
                                  and a partial one
  ato_odd5    16, 12,  6,  4,  5  odd ndxr; 25 points: one partial round
  ato_full4   16, 12, 16,  4,  4  sea as wide as the atmosphere: bilint's wrapped columns, natlan != 0
  ato_allsea  16, 12, 16, 12,  2  nxaooc = nxta, nyaooc = nyta (the default of src/parameters_data.F): natlan = 0, the
                                  arlaav = 0 branch, no land cell
  ato_r16     32, 20,  6,  5, 16  the production refinement: four full rounds
  ato_cyc72   72, 12, 72,  4,  4  288 cells: a second round of k_xf_heat_final's stride-256 loops; a last aml tile 8
                                  columns wide

  python tests/golden/make_golden_atmos_only.py           # writes tests/golden/ato_*.npz
  python tests/golden/make_golden_atmos_only.py NAME ...  # writes only the named cases
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_heat as mh  # noqa: E402

K, NSTR = 3, 3

DRIVER = r"""
program ato_driver
  use parameters
  use atconst
  use occonst
  use athomog, only : xan, enisat, eninat, txisat, txinat
  use atstate, only : pa, pam, entat, wekta, wekpa
  use intrfac
  use radiate
  use monitor, only : arlaav, slhfav, oradav, arocav, cfraat, centat
  use xfosubs
  use amlsubs
  implicit none
  integer, parameter :: ncst = 34
  integer :: ncyc, ns, c, s, j
  double precision :: cst(ncst), geo(10)
  double precision :: asto(nxto,nyto), fsa(nyta)
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) ncyc, ns
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
  ! the SST is read once and held: sstm = sst (src/q-gcm.F:753-786)
  read (10) pa, pam, sst, ast, astm, hmixa, hmixam, xc1ast, dtopat
  sstm = sst
  close (10)
  xan = 0.0d0; enisat = 0.0d0; eninat = 0.0d0
  open (11, file='out.bin', access='stream', form='unformatted', status='replace')
  call bilint (xta, yta, nxta, nyta, astm, xto, yto, nxto, nyto, asto, 1.0d0)
  do j=1,nyta
    fsa(j) = fsprim( ytarel(j) )
  enddo
  write (11) asto, fsa, xta, yta, xto, yto
  do c = 1, ncyc
    call xforc
    write (11) fnetat, wekta, uekat, vekat, tauxa, tauya, wekpa, txisat, txinat, arlaav, slhfav, oradav, arocav
    do s = 1, ns
      call aml
      write (11) ast, astm, hmixa, hmixam, entat, xan(1), enisat(1), eninat(1), cfraat, centat
    end do
  end do
  write (11) stbbb, stbus, stbvs, stbun, stbvn
  close (11)
end program ato_driver
"""

# (file, (nxta, nyta, nxaooc, nyaooc, ndxr), sstm zonally periodic, plain: xcexp = 1 and xc1ast = dtopat = 0)
CASES = [("ato_tiny", (16, 12, 4, 3, 12), False, True),
         ("ato_odd5", (16, 12, 6, 4, 5), False, False),
         ("ato_full4", (16, 12, 16, 4, 4), True, False),
         ("ato_allsea", (16, 12, 16, 12, 2), True, False),
         ("ato_r16", (32, 20, 6, 5, 16), False, False),
         ("ato_cyc72", (72, 12, 72, 4, 4), True, False)]
TABLES = ("stbbb", "stbus", "stbvs", "stbun", "stbvn")
INPUT_ORDER = ("pa", "pam", "sstm", "ast", "astm", "hmixa", "hmixam", "xc1ast", "dtopat")


def build(wrk, dims):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    src = os.path.join(mh.REF, "src")
    with open(os.path.join(mh.REF, "examples", "double_gyre_coupled", "parameters_data.F.dg_oo")) as f:
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
            lines[i] = "      PARAMETER ( fnot = %s, beta = %s )" % (mh.FNOT, mh.BETA)
            hits += 1
        elif ln.startswith("      PARAMETER ( nscvat = "):
            lines[i] = ln.replace("nscvat =  2", "nscvat =  1")  # (any nxta, nyta; the covariances are not built)
        elif ln.startswith("     &            nscvoc = 16"):
            lines[i] = ln.replace("nscvoc = 16", "nscvoc = 1")
    assert hits == 3
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    with open(os.path.join(wrk, "ato_driver.F90"), "w") as f:
        f.write(DRIVER)
    fc = [mh.FC, "-cpp", "-ffixed-line-length-132", "-O2", "-Datmos_only"]
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in mh.MODS] + [os.path.join(src, "intsubs.f")]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call(fc + ["-DPRIVATE=PUBLIC", "-c", "-I" + src, os.path.join(src, "xfosubs.F")], cwd=wrk)
    subprocess.check_call(fc + ["-c", "-I" + src, os.path.join(src, "amlsubs.F")], cwd=wrk)
    objs += ["xfosubs.o", "amlsubs.o"]
    subprocess.check_call([mh.FC, "-cpp", "-O2", "-Datmos_only", "-c", "ato_driver.F90"], cwd=wrk)
    subprocess.check_call([mh.FC, "-o", "ato_driver", "ato_driver.o"] + objs, cwd=wrk)


def shapes(dims):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    nxpa, nypa, nxto, nyto = nxta + 1, nyta + 1, nxaooc * ndxr, nyaooc * ndxr
    once = [("asto", (nxto, nyto)), ("fsa", (nyta,)), ("xta", (nxta,)), ("yta", (nyta,)), ("xto", (nxto,)), ("yto", (nyto,))]
    xf = [("fnetat", (nxta, nyta)), ("wekta", (nxta, nyta)), ("uekat", (nxpa, nyta)), ("vekat", (nxta, nypa)),
          ("tauxa", (nxpa, nypa)), ("tauya", (nxpa, nypa)), ("wekpa", (nxpa, nypa)), ("txisat", ()), ("txinat", ()),
          ("arlaav", ()), ("slhfav", ()), ("oradav", ()), ("arocav", ())]
    return once, xf, mh.shapes(dims)[2]


def run(wrk, dims, C, F):
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([K, NSTR], dtype=np.int32).tobytes())
        fh.write(np.array([C[k] for k in mh.CNAMES]).tobytes())
        G = mh.geometry(dims, C)
        fh.write(np.array([G[k] for k in mh.GNAMES]).tobytes())
        for k in ("xta", "yta", "ytarel", "xto", "yto", "ytorel"):
            fh.write(np.ascontiguousarray(G[k], dtype=np.float64).tobytes())
        for k in INPUT_ORDER:
            fh.write(np.asfortranarray(F[k], dtype=np.float64).tobytes(order="F"))
    subprocess.check_call([os.path.join(wrk, "ato_driver")], cwd=wrk, preexec_fn=mh._big_stack)
    out = np.fromfile(os.path.join(wrk, "out.bin"), dtype=np.float64)
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
    for c in range(K):
        take("x%d_" % c, xf)
        for s in range(NSTR):
            take("a%d%d_" % (c, s), am)
    ndxr = dims[4]
    for t in TABLES:
        n = 16 * (ndxr + 1) * (ndxr + 1)
        res["tab_" + t] = out[o:o + n].reshape((16, ndxr + 1, ndxr + 1), order="F").copy()
        o += n
    assert o == len(out)
    return res


def check(name, dims, C, F, res):
    """On the reference's own outputs: the numpy restatement (tests/numpy_atmos_only.py, numpy_heat.aml) gives the
    pointwise fields bit for bit, arocav is the 0 * ocnorm of an arocsm nothing was added to, every cell above the sea differs from its land value, and
    every branch of the mixed layer's step is taken - else a test could pass by skipping it.  Returns the branches
    taken; the caller asserts all of them for every case (ato_allsea, without a land cell, needs no exemption)."""
    import numpy_atmos_only as na
    import numpy_heat as nh
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    g = dict(c_dims=np.array(dims), c_nx1=1 + (nxta - nxaooc) // 2, c_ny1=1 + (nyta - nyaooc) // 2, c_cyclic=0,
             c_fnot=float(mh.FNOT.replace("D", "e")), c_K=K, c_nstr=NSTR)
    g.update({"c_" + k: v for k, v in C.items()})
    P = nh.params(g)
    assert P["dxa"] / float(ndxr) == P["dxo"], (name, P["dxa"], P["dxo"])  # (what the library derives without an ocean)
    T = nh.bilint_tables(res["t_xta"], res["t_yta"], res["t_xto"], res["t_yto"], P["dxa"], P["dya"])
    assert np.array_equal(nh.bilint(T, F["astm"]), res["t_asto"]), name
    got = dict(diab=False, floor=False, conv=False, none=False)
    S = {k: F[k] for k in na.STATE}
    for c in range(K):
        H = na.heat_sst(S["astm"], S["hmixam"], F["sstm"], F["pam"], F["dtopat"], res["t_fsa"], T, P)
        fa = res["x%d_fnetat" % c]
        land = ~H["ocean"]
        assert np.array_equal(H["fnetat"][land], fa[land]), (name, c)
        # above the sea the reference's serial sum is the restatement's: same order, same bits
        assert np.array_equal(H["fnetat"], fa), (name, c)
        assert np.all(fa[H["ocean"]] != 0.0) and np.all(fa[H["ocean"]] != H["fnetat_land"][H["ocean"]]), (name, c)
        assert float(res["x%d_arocav" % c]) == 0.0, (name, c)
        for k in na.SST_SCALARS:
            assert float(res["x%d_%s" % (c, k)]) == H[k], (name, c, k)
        assert (float(res["x%d_arlaav" % c]) == 0.0) == (nxaooc * nyaooc == nxta * nyta), (name, c)
        for s in range(NSTR):
            A = nh.aml(S, fa, res["x%d_wekta" % c], res["x%d_uekat" % c], res["x%d_vekat" % c], F["pa"], F["pam"],
                       F["xc1ast"], F["dtopat"], P)
            S = {k: res["a%d%d_%s" % (c, s, k)] for k in na.STATE}
            for k in S:
                assert np.all(np.isfinite(S[k])) and np.array_equal(A[k], S[k]), (name, c, s, k)
            assert np.array_equal(A["entat"], res["a%d%d_entat" % (c, s)]), (name, c, s)
            b = A["branches"]
            for k in ("diab", "floor", "conv"):
                got[k] |= bool(b[k].any())
            got["none"] |= bool((~b["diab"] & ~b["floor"] & ~b["conv"])[1:-1, 1:-1].any())
    cf = [float(res["a%d%d_cfraat" % (c, s)]) for c in range(K) for s in range(NSTR)]
    got["cfraat"] = any(0.0 < v < 1.0 for v in cf)
    return got


if __name__ == "__main__":
    only = sys.argv[1:]
    assert all(n in [c[0] for c in CASES] for n in only), only
    for ic, (name, dims, cyc, plain) in enumerate(CASES):
        if only and name not in only:
            continue
        C = mh.constants(dims, plain)
        F = mh.inputs(dims, cyc, plain, C, 400 + ic)
        del F["pom"]
        wrk = tempfile.mkdtemp(prefix="ato_")
        try:
            build(wrk, dims)
            res = run(wrk, dims, C, F)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        got = check(name, dims, C, F, res)
        sys.stderr.write("%s: branches %s\n" % (name, got))
        assert all(got.values()), (name, got)  # (ato_allsea too: its warm patch and thin spot lie above the sea, and count)
        nxta, nyta, nxaooc, nyaooc, ndxr = dims
        out = dict(c_dims=np.array(dims, dtype=np.int64), c_cyclic=np.int64(0), c_K=np.int64(K), c_nstr=np.int64(NSTR),
                   c_nx1=np.int64(1 + (nxta - nxaooc) // 2), c_ny1=np.int64(1 + (nyta - nyaooc) // 2),
                   c_fnot=np.float64(float(mh.FNOT.replace("D", "e"))))
        out.update({"c_" + k: np.float64(v) for k, v in C.items()})
        out.update({"in_" + k: np.asfortranarray(v) for k, v in F.items()})
        out.update(res)
        # (one file per case, or <case>.npz and <case>_aml.npz, <case>_aml2.npz, ... with the a<c><s>_* records where
        #  one file would pass the size limit of a committed file, as make_golden_heat.py cuts them)
        parts = {name: out}
        if sum(np.asarray(v).nbytes for v in out.values()) > 900000:
            parts = {name: {k: v for k, v in out.items() if not re.match(r"a\d\d_", k)}}
            calls = ["a%d%d_" % (c, s) for c in range(K) for s in range(NSTR)]
            for n in range(1, len(calls) + 1):
                cut = [calls[len(calls) * i // n:len(calls) * (i + 1) // n] for i in range(n)]
                aml = {name + "_aml" + (str(i + 1) if i else ""): {k: v for k, v in out.items() if k[:4] in grp}
                       for i, grp in enumerate(cut)}
                if all(mh.packed_size(d) < (1 << 20) for d in aml.values()):
                    break
            parts.update(aml)
            assert sum(len(d) for d in parts.values()) == len(out)
        for fn, d in parts.items():
            path = os.path.join(HERE, "%s.npz" % fn)
            np.savez_compressed(path, **d)
            size = os.path.getsize(path)
            assert size < (1 << 20), (fn, size)
            sys.stderr.write("wrote %s.npz (%d bytes)\n" % (fn, size))
