#!/usr/bin/env python3
"""Golden values of the ocean's periodic dumps - qocdiag_out (src/qocdiag.F:303-687) and ocnc_out
(src/nc_subs.F:837-1072) - from the TRUE reference.

Both routines do their arithmetic only inside `#ifdef use_netcdf`, and no netCDF library is needed to run them: this
script compiles the reference's qocdiag.F and nc_subs.F UNMODIFIED with -Dqoc_diag -Duse_netcdf against a netCDF
stand-in that is this script's own text (NETCDF_INC, NETCDF_STUBS): a netcdf.inc with the constants and the nf_*
declarations the two files use, and stub nf_* functions.  nf_def_var numbers the variables and remembers their names
and ranks; nf_put_vara_double appends (name, start, count, data) to a record file.  Everything is built in a temporary
directory (one build per case: the dimensions and the cyclic option are compile-time) with the flags of
make_golden_tavg.py, and deleted.  The driver fills MODULE occonst / ocstate / intrfac, then calls, as the main program
does, qocdiag_init (nsko) and qocdiag_out (nsko) (src/q-gcm.F:1052, 1234-1239), and ocnc_init / ocnc_out
(src/q-gcm.F:1050, 1459-1461).

  python tests/golden/make_golden_qocdiag.py          # writes tests/golden/qod_{box_tiny,cyc_tiny,box_tiny_ah2,box_tiny5,cyc_tiny6}.npz
  python tests/golden/make_golden_qocdiag.py time     # the reference's qocdiag_out time at 961 x 961 x 3, 16 threads
"""
import os
import resource
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
MODS = ["atconst_data.F", "occonst_data.F", "atstate_data.F", "ocstate_data.F", "intrfac_data.F", "timinfo_data.F"]
NSKO = (1, 2, 7)
OUTFLOC = (1, 1, 1, 1, 1, 1, 0)

NETCDF_INC = """
      integer NF_NOERR, NF_FLOAT, NF_DOUBLE, NF_CLOBBER
      parameter ( NF_NOERR = 0, NF_FLOAT = 5, NF_DOUBLE = 6 )
      parameter ( NF_CLOBBER = 0 )
      integer nf_def_dim, nf_def_var, nf_enddef, nf_put_att_text
      integer nf_put_var_double, nf_put_vara_double, nf_create
      integer nf_close, nf_inq_dimid, nf_inq_dimlen, nf_inq_varid
      integer nf_get_var_double
      character*80 nf_strerror
      external nf_def_dim, nf_def_var, nf_enddef, nf_put_att_text
      external nf_put_var_double, nf_put_vara_double, nf_create
      external nf_close, nf_inq_dimid, nf_inq_dimlen, nf_inq_varid
      external nf_get_var_double, nf_strerror
"""

NETCDF_STUBS = r"""
module nfstub
  implicit none
  integer, save :: nvar = 0, ndim = 0
  character(len=32), save :: vname(1000)
  integer, save :: vnd(1000), vfile(1000)
end module nfstub

integer function nf_create(path, mode, ncid)
  character(len=*) :: path
  integer :: mode, ncid
  integer, save :: nfile = 0
  nfile = nfile + 1
  ncid = nfile
  nf_create = 0
end function
integer function nf_def_dim(ncid, name, len, dimid)
  use nfstub
  character(len=*) :: name
  integer :: ncid, len, dimid
  ndim = ndim + 1
  dimid = ndim
  nf_def_dim = 0
end function
integer function nf_def_var(ncid, name, xtype, nd, dimids, varid)
  use nfstub
  character(len=*) :: name
  integer :: ncid, xtype, nd, dimids(*), varid
  nvar = nvar + 1
  vname(nvar) = name
  vnd(nvar) = nd
  vfile(nvar) = ncid
  varid = nvar
  nf_def_var = 0
end function
integer function nf_put_vara_double(ncid, varid, start, cnt, dat)
  use nfstub
  integer :: ncid, varid, start(*), cnt(*)
  double precision :: dat(*)
  integer :: n, i
  n = 1
  do i = 1, vnd(varid)
    n = n * cnt(i)
  end do
  write (21) vname(varid), vnd(varid)
  write (21) (start(i), i = 1, vnd(varid)), (cnt(i), i = 1, vnd(varid))
  write (21) dat(1:n)
  nf_put_vara_double = 0
end function
integer function nf_enddef(ncid)
  integer :: ncid
  nf_enddef = 0
end function
integer function nf_close(ncid)
  integer :: ncid
  nf_close = 0
end function
integer function nf_put_att_text(ncid, varid, name, len, text)
  character(len=*) :: name, text
  integer :: ncid, varid, len
  nf_put_att_text = 0
end function
integer function nf_put_var_double(ncid, varid, dat)
  integer :: ncid, varid
  double precision :: dat(*)
  nf_put_var_double = 0
end function
integer function nf_inq_dimid(ncid, name, dimid)
  character(len=*) :: name
  integer :: ncid, dimid
  dimid = 1
  nf_inq_dimid = 0
end function
integer function nf_inq_dimlen(ncid, dimid, len)
  integer :: ncid, dimid, len
  len = 1
  nf_inq_dimlen = 0
end function
integer function nf_inq_varid(ncid, name, varid)
  character(len=*) :: name
  integer :: ncid, varid
  varid = 1
  nf_inq_varid = 0
end function
integer function nf_get_var_double(ncid, varid, dat)
  integer :: ncid, varid
  double precision :: dat(*)
  nf_get_var_double = 0
end function
character(len=80) function nf_strerror(ncstat)
  integer :: ncstat
  nf_strerror = 'stub'
end function
"""

DRIVER = r"""
program qod_driver
  use parameters, only : nxpo, nypo, nlo
  use occonst
  use ocstate, only : po, pom, qo, qom, wekpo, entoc
  use intrfac, only : sst, tauxo, tauyo
  use ocstate, only : wekto
  use timinfo, only : ntdone, noutoc, tyrs, noutstepoc
  use qocdiag
  use nc_subs, only : ocnc_init, ocnc_out
  implicit none
  integer :: nsko, nrep, r, outfloc(7)
  double precision :: sc(4), t0, t1
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) sc
  dxo = sc(1); dyo = sc(1); bccooc = sc(2); delek = sc(3); dto = sc(4)
  dxom2 = 1.0d0/(dxo*dxo)
  tdto = 2.0d0*dto
  read (10) hoc, ah2oc, ah4oc, gpoc
  read (10) po, pom, qo, qom, wekpo, entoc
  read (10) sst, wekto, tauxo, tauyo
  read (10) nsko, nrep, outfloc
  close (10)
  ntdone = 0; noutoc = 1; tyrs = 0.0d0; noutstepoc = 1
  open (21, file='rec.bin', access='sequential', form='unformatted', status='replace')
  qocncid = 1
  call qocdiag_init (nsko)
  t0 = omp_wall()
  do r = 1, nrep
    call qocdiag_out (nsko)
  end do
  t1 = omp_wall()
  if ( nrep.eq.1 ) then
    call ocnc_init (nsko, outfloc)
    call ocnc_out (nsko, outfloc)
  end if
  close (21)
  open (11, file='time.txt', status='replace')
  write (11, *) (t1 - t0) / nrep
  close (11)
contains
  double precision function omp_wall()
    integer(8) :: c, rate
    call system_clock (c, rate)
    omp_wall = dble(c) / dble(rate)
  end function
end program qod_driver
"""


def build(wrk, dims, cyclic, openmp=False):
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
    with open(os.path.join(wrk, "netcdf.inc"), "w") as f:
        f.write(NETCDF_INC)
    with open(os.path.join(wrk, "nfstub.f90"), "w") as f:
        f.write(NETCDF_STUBS)
    with open(os.path.join(wrk, "qod_driver.F90"), "w") as f:
        f.write(DRIVER)
    q = ["-Docean_only", "-Dqoc_diag", "-Duse_netcdf"] + (["-Dcyclic_ocean"] if cyclic else [])
    omp = ["-fopenmp"] if openmp else []
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2"] + omp + q
    inc = ["-I" + wrk, "-I" + src]
    objs = []
    subprocess.check_call([FC, "-O2", "-c", "nfstub.f90"], cwd=wrk)
    objs.append("nfstub.o")
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS + ["nc_subs.F", "qocdiag.F"]]:
        subprocess.check_call(fc + ["-c"] + inc + [f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call([FC, "-cpp", "-O2", "-c", "qod_driver.F90"], cwd=wrk)
    subprocess.check_call([FC, "-o", "qod_driver", "qod_driver.o"] + objs + omp, cwd=wrk)


def read_records(path):
    """(name, start, count, data) of every nf_put_vara_double call (Fortran sequential records)."""
    raw = open(path, "rb").read()
    recs, o = [], 0

    def rec():
        nonlocal o
        n = int(np.frombuffer(raw, np.int32, 1, o)[0])
        b = raw[o + 4:o + 4 + n]
        o += n + 8
        return b
    while o < len(raw):
        h = rec()
        name, nd = h[:32].decode().strip(), int(np.frombuffer(h, np.int32, 1, 32)[0])
        sc = np.frombuffer(rec(), np.int32)
        recs.append((name, sc[:nd].copy(), sc[nd:].copy(), np.frombuffer(rec(), np.float64).copy()))
    return recs


def run(wrk, cfg, f, nsko, nrep=1, env=None):
    F = lambda a: np.asfortranarray(a, dtype=np.float64).tobytes(order="F")
    nl = cfg.nlo
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([cfg.dxo, cfg.bccooc, cfg.delek, cfg.dto], dtype=np.float64).tobytes())
        for v in (cfg.hoc, cfg.ah2oc, cfg.ah4oc, cfg.gpoc):
            fh.write(np.array(v[:nl] if len(v) >= nl else v, dtype=np.float64).tobytes())
        for k in ("po", "pom", "qo", "qom", "wekpo", "entoc", "sst", "wekto", "tauxo", "tauyo"):
            fh.write(F(f[k]))
        fh.write(np.array([nsko, nrep] + list(OUTFLOC), dtype=np.int32).tobytes())
    # qocdiag_out keeps eight (nxpo, nypo) automatic arrays (src/qocdiag.F:344-348): 60 MB of stack at 961 x 961
    big_stack = lambda: resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    subprocess.check_call([os.path.join(wrk, "qod_driver")], cwd=wrk, env=env, preexec_fn=big_stack)
    return read_records(os.path.join(wrk, "rec.bin")), float(open(os.path.join(wrk, "time.txt")).read())


def assemble(recs, nl):
    """qocdiag_out's per-layer records -> (nlo, jpwk, ipwk) per term; ocnc_out's -> (planes, rows, columns)."""
    out = {}
    for name, start, cnt, data in recs:
        if len(cnt) < 3:  # the time axes
            continue
        if name in ("dqdt", "qotjac", "qt2dif", "qt4dif", "qotent"):
            a = out.setdefault("qd_" + name, np.zeros((nl, cnt[1], cnt[0])))
            a[start[2] - 1] = data.reshape(cnt[1], cnt[0])
        else:
            planes = cnt[2] if len(cnt) == 4 else 1
            out["nc_" + name] = data.reshape(planes, cnt[1], cnt[0])
    return out


def inputs(cfg, g, om, state, seed):
    from qgcm_hip import synth
    sst, _, _, tx, ty = synth.mixed_layer_fields(cfg, om, seed=seed)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    rng = np.random.default_rng(seed)
    entoc = 1e-6 * rng.standard_normal((cfg.nxpo, cfg.nypo))
    if cfg.cyclic:
        entoc[-1] = entoc[0]
    return dict(po=g[state + "_po"], pom=g[state + "_pom"], qo=g[state + "_qo"], qom=g[state + "_qom"], wekpo=wekpo,
                entoc=np.asfortranarray(entoc), sst=sst, wekto=wekto, tauxo=tx, tauyo=ty)


# (golden file, fixture, reference configuration, state)
CASES = [("box_tiny", "box_tiny", "box_tiny", "steps26"), ("cyc_tiny", "cyc_tiny", "cyc_tiny", "steps26"),
         ("box_tiny_ah2", "box_tiny_ah2", "box_tiny", "steps26"), ("box_tiny5", "box_tiny5", "box_tiny5", "steps26"),
         ("cyc_tiny6", "cyc_tiny6", "cyc_tiny6", "steps26")]


def time_mode():
    """qocdiag_out of the reference, -fopenmp, 16 threads, on a 961 x 961 x 3 box (nxaooc = nyaooc = 60, ndxr = 16)."""
    import ref_binding
    from qgcm_hip import oml_preset, preset
    cfg = preset("natl5")
    om = oml_preset(cfg)
    rng = np.random.default_rng(1)
    shp = (cfg.nxpo, cfg.nypo, cfg.nlo)
    po = np.asfortranarray(rng.standard_normal(shp))
    f = dict(po=po, pom=po * 0.999, qo=po * 1e-9, qom=po * 1.1e-9)
    from qgcm_hip import synth
    sst, _, _, tx, ty = synth.mixed_layer_fields(cfg, om, seed=3)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f.update(wekpo=wekpo, entoc=np.zeros((cfg.nxpo, cfg.nypo)), sst=sst, wekto=wekto, tauxo=tx, tauyo=ty)
    wrk = tempfile.mkdtemp(prefix="qod_")
    try:
        build(wrk, ref_binding.CONFIGS["box_natl5"][:8], False, openmp=True)
        env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "16"), OMP_STACKSIZE="512M")
        for nsko in (1, 2):
            _, t = run(wrk, cfg, f, nsko, nrep=5, env=env)
            print("reference qocdiag_out %dx%dx%d nsko=%d threads=%s: %.2f ms per call"
                  % (cfg.nxpo, cfg.nypo, cfg.nlo, nsko, env["OMP_NUM_THREADS"], 1e3 * t))
    finally:
        shutil.rmtree(wrk, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "time":
        time_mode()
        sys.exit(0)
    import ref_binding
    from qgcm_hip import oml_preset, preset
    for out_name, fixture, refcfg, state in CASES:
        cfg = preset(fixture)
        om = oml_preset(cfg)
        g = np.load(os.path.join(HERE, fixture + ".npz"))
        f = inputs(cfg, g, om, state, seed=11)
        out = {"in_" + k: v for k, v in f.items()}
        wrk = tempfile.mkdtemp(prefix="qod_")
        try:
            build(wrk, ref_binding.CONFIGS[refcfg][:8], cfg.cyclic)
            for nsko in NSKO:
                recs, _ = run(wrk, cfg, f, nsko)
                out.update({"n%d_%s" % (nsko, k): v for k, v in assemble(recs, cfg.nlo).items()})
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        np.savez_compressed(os.path.join(HERE, "qod_%s.npz" % out_name), **out)
        sys.stderr.write("wrote qod_%s.npz (%s)\n" % (out_name, ", ".join(sorted(k for k in out if k.startswith("n1_")))))
