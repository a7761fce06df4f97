#!/usr/bin/env python3
"""Golden values of the area averages (areavg / areint, src/areasubs_diag.F, cpp option get_areav) and of the CFL
check (cfltry, src/q-gcm.F:2121-2440) from the TRUE reference.

Compiles the reference's areasubs_diag.F and the data modules unmodified, as a coupled model, in a temporary directory
(one build per case: the dimensions are compile-time PARAMETERs, substituted into the coupled example's
parameters_data.F; no -fopenmp, so every sum and every scan runs serially in its written order; -ffp-contract=off, so
areint's `facs*asums + facn*asumn + arsum` is not contracted and the numpy restatement can give it bit for bit).

  areavg  writes its results only through netCDF calls (tavoc / tavat are locals).  The build gets this script's own
          stand-in `netcdf.inc`, its own nf_* functions and a MODULE nc_subs with handle_err: nf_put_vara_double hands
          the doubles over bitwise (variable id, count, values on a stream file).  areasubs_diag.F itself is compiled
          as it is, with -Dget_areav -Duse_netcdf.  The subscripts and weights it prints are parsed and recorded.
  cfltry  is an external subroutine inside q-gcm.F: its lines (SUBROUTINE cfltry .. END SUBROUTINE cfltry) are copied
          into the temporary directory, as patch_main.py does with the main program, and its print-out is parsed:
          the maxima and Courant numbers at the 8 significant digits of `1p,9d15.7`, and every
          `Bad ...; CFL, i, j[, k]` line exactly.

The driver sets the grid constants both routines read (dxo, dyo, xlo, ylo, dto, rdxof0 and the atmosphere's; hmoc),
reads sst, ast, po, pa, tauxo, tauyo, uekat, vekat and calls areavg and cfltry once.  Every case records both fluids
(oc_* / at_*); the case's name says which one it was shaped for.  All reference sources, objects and .mod files stay in
the temporary directory, which is deleted.

The device kernels' tiles: one wave (64 lanes) strides an area's row segment; the CFL scan uses 64 x 16 tiles.
  area_box   ocean 300 x 40 T cells, nine areas: the whole domain (weights 1 at subscripts 1 and nxto / nyto), limits
             exactly on cell edges (the >= / > asymmetry), mid-cell limits with four different fractional weights, a
             single row (j1 == j2), a single column (i1 == i2), one wider than 256 columns, one of three columns, two
             overlapping ones
  area_atm   atmosphere 72 x 24, five areas; its ocean block is a second record with n = 1
  cfl_box    ocean 97 x 41 p points, three layers: two tile columns (the second 33 wide), three tile rows (the last 9
             high); offenders across the tile seam in layer 1 and the mixed layer, the maximum of layer 2's |v| on
             the last scanned row, none in layer 3
  cfl_cyc    a cyclic ocean of 129 x 25: a third tile column one point wide, offenders next to the seam
  cfl_atm    atmosphere 33 x 13 with uekat / vekat
  cfl_box2, cfl_box5, cfl_cyc6
             the grids of cfl_box and cfl_cyc with nlo = 2, 5, 6 (NLO) and a po that differs in every layer.  The
             largest |v| of the LAST layer lies at two points with bit-equal values (TIES): the later one in scan order
             (j outer) has the smaller i, so the reference's order - its Bad lines - decides between them

  python tests/golden/make_golden_areacfl.py           # writes tests/golden/areacfl_*.npz and areas_limits_*.txt
  python tests/golden/make_golden_areacfl.py NAME ...  # only the named cases
"""
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
MODS = ["atconst_data.F", "occonst_data.F", "atstate_data.F", "ocstate_data.F", "intrfac_data.F", "timinfo_data.F"]
FNOT, BETA = "9.37456D-05", "1.75360D-11"
F0 = float(FNOT.replace("D", "e"))
DXO, DTO, DTA, HMOC, CFLCRIT = 5.0e3, 540.0, 180.0, 100.0, 0.8

NETCDF_INC = """\
*     stand-in for netcdf.inc: the constants and functions areasubs_diag.F names
      integer NF_NOERR, NF_INT, NF_FLOAT
      parameter ( NF_NOERR = 0, NF_INT = 4, NF_FLOAT = 5 )
      integer nf_def_dim, nf_def_var, nf_put_att_text, nf_enddef
      integer nf_put_var_int, nf_put_vara_double
      external nf_def_dim, nf_def_var, nf_put_att_text, nf_enddef
      external nf_put_var_int, nf_put_vara_double
"""

NC_STUB = r"""
module nc_subs
  implicit none
contains
  subroutine handle_err (ncstat, fromst)
    integer, intent(in) :: ncstat
    character (len=*), intent(in), optional :: fromst
    print *, ' netCDF stand-in: error ', ncstat
    stop 1
  end subroutine handle_err
end module nc_subs

module nc_stub_state
  implicit none
  integer :: nvars = 0, ndims = 0, dimlen(16), varnd(16), vardim(4,16)
end module nc_stub_state

integer function nf_def_dim (ncid, name, length, dimid)
  use nc_stub_state
  integer :: ncid, length, dimid
  character (len=*) :: name
  ndims = ndims + 1
  dimlen(ndims) = length
  dimid = ndims
  nf_def_dim = 0
end function

integer function nf_def_var (ncid, name, xtype, nd, dimids, varid)
  use nc_stub_state
  integer :: ncid, xtype, nd, dimids(*), varid
  character (len=*) :: name
  nvars = nvars + 1
  varnd(nvars) = nd
  vardim(1:nd,nvars) = dimids(1:nd)
  varid = nvars
  write (48) -nvars, len(name)
  write (48) name
  nf_def_var = 0
end function

integer function nf_put_att_text (ncid, varid, name, length, text)
  integer :: ncid, varid, length
  character (len=*) :: name, text
  nf_put_att_text = 0
end function

integer function nf_enddef (ncid)
  integer :: ncid
  nf_enddef = 0
end function

integer function nf_put_var_int (ncid, varid, ivals)
  integer :: ncid, varid, ivals(*)
  nf_put_var_int = 0
end function

! the doubles, bitwise: variable id, how many, the values
integer function nf_put_vara_double (ncid, varid, start, count, dvals)
  use nc_stub_state
  integer :: ncid, varid, start(*), count(*), n, d
  double precision :: dvals(*)
  n = 1
  do d = 1, varnd(varid)
    n = n*count(d)
  end do
  write (48) varid, n
  write (48) dvals(1:n)
  nf_put_vara_double = 0
end function
"""

DRIVER = r"""
program areacfl_driver
  use parameters
  use atconst
  use occonst
  use atstate, only : pa
  use ocstate, only : po
  use intrfac
  use timinfo
  use areasubs
  implicit none
  double precision :: cst(5)
  open (10, file='in.bin', access='stream', form='unformatted', status='old')
  read (10) cst
  dxo = cst(1); dto = cst(2); dxa = cst(3); dta = cst(4); hmoc = cst(5)
  dyo = dxo; dya = dxa
  xlo = nxto*dxo; ylo = nyto*dyo; xla = nxta*dxa; yla = nyta*dya
  rdxof0 = 1.0d0/(dxo*fnot); rdxaf0 = 1.0d0/(dxa*fnot)
  read (10) sst, ast, po, pa, tauxo, tauyo, uekat, vekat
  close (10)
  ntdone = 0; nocmon = 1; numoutsteps = 1; tyrs = 0.0d0; tday = 0.0d0
  arencid = 1
  open (48, file='out.bin', access='stream', form='unformatted', status='replace')
  call areavg
  close (48)
  call cfltry (0)
end program areacfl_driver
"""

# (name, (nxta, nyta, nxaooc, nyaooc, ndxr), ocean areas (xlo, xhi, ylo, yhi) in km, atmosphere areas)
CASES = [
    ("area_box", (80, 12, 75, 10, 4),
     [(0.0, 1500.0, 0.0, 200.0), (100.0, 400.0, 50.0, 150.0), (101.2, 397.1, 51.9, 148.3), (200.0, 700.0, 61.0, 63.0),
      (751.0, 753.0, 20.0, 180.0), (50.0, 1450.0, 12.0, 188.0), (500.0, 515.0, 0.0, 200.0), (600.0, 1000.0, 40.0, 160.0),
      (800.0, 1200.0, 80.0, 200.0)],
     [(0.0, 1600.0, 0.0, 240.0)]),
    ("area_atm", (72, 24, 4, 3, 4),
     [(11.0, 63.5, 7.25, 51.0)],
     [(0.0, 1440.0, 0.0, 480.0), (200.0, 1000.0, 100.0, 400.0), (213.0, 1011.0, 96.0, 389.0), (705.0, 712.0, 243.0, 255.0),
      (600.0, 1400.0, 200.0, 480.0)]),
    ("cfl_box", (32, 12, 24, 10, 4), [(0.0, 480.0, 0.0, 200.0)], [(0.0, 640.0, 0.0, 240.0)]),
    ("cfl_cyc", (32, 8, 32, 6, 4), [(0.0, 640.0, 0.0, 120.0)], [(0.0, 640.0, 0.0, 160.0)]),
    ("cfl_atm", (32, 12, 4, 3, 4), [(0.0, 80.0, 0.0, 60.0)], [(0.0, 640.0, 0.0, 240.0)]),
    ("cfl_box2", (32, 12, 24, 10, 4), [(0.0, 480.0, 0.0, 200.0)], [(0.0, 640.0, 0.0, 240.0)]),
    ("cfl_box5", (32, 12, 24, 10, 4), [(0.0, 480.0, 0.0, 200.0)], [(0.0, 640.0, 0.0, 240.0)]),
    ("cfl_cyc6", (32, 8, 32, 6, 4), [(0.0, 640.0, 0.0, 120.0)], [(0.0, 640.0, 0.0, 160.0)]),
]
NLO = {"cfl_box2": 2, "cfl_box5": 5, "cfl_cyc6": 6}  # ocean layers (every other case: 3)
# the tied pair of the last layer's |v| (1-based i, j of the difference p(i+1,j) - p(i,j)): first and second in scan order
TIES = {"cfl_box2": ((80, 7), (10, 30)), "cfl_box5": ((80, 7), (10, 30)), "cfl_cyc6": ((100, 5), (20, 18))}
TIE_COURANT = 1.6
NAMES = ("oc1", "oc2", "oc3", "oc4", "oc5", "oc6", "oc7", "oc8", "oc9")


def limits_text(oc, at):
    """areas.limits in the reference's layout: list-directed records with D exponents, names in (9(8x,a3))."""
    def block(areas, prefix):
        rows = ["%4d" % len(areas)]
        for c in range(4):
            rows.append("".join("%11s" % ("%.2fd3" % a[c]) for a in areas))
        rows.append("".join("%8s%s" % ("", "%s%d" % (prefix, m + 1)) for m in range(len(areas))))
        return rows
    return "\n".join(block(oc, "oc") + block(at, "at")) + "\n"


def metres(areas):
    """The limits as the reference reads them from limits_text's decimal strings."""
    return np.array([[float("%.2fe3" % v) for v in a] for a in areas])


def build(wrk, dims, nlo=3):
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
            lines[i] = "      PARAMETER ( nxaooc = %d, nyaooc = %d, ndxr = %d, nlo = %d )" % (nxaooc, nyaooc, ndxr, nlo)
            hits += 1
        elif ln.startswith("      PARAMETER ( fnot = "):
            lines[i] = "      PARAMETER ( fnot = %s, beta = %s )" % (FNOT, BETA)
            hits += 1
        elif ln.startswith("      PARAMETER ( nscvat = "):
            lines[i] = ln.replace("nscvat =  2", "nscvat =  1")
        elif ln.startswith("     &            nscvoc = 16"):
            lines[i] = ln.replace("nscvoc = 16", "nscvoc = 1")
    assert hits == 3
    with open(os.path.join(wrk, "parameters_data.F"), "w") as f:
        f.write("\n".join(lines))
    # cfltry: the lines of the external subroutine, copied out of the main program's file
    with open(os.path.join(src, "q-gcm.F")) as f:
        main = f.read().split("\n")
    a = [i for i, ln in enumerate(main) if ln.startswith("      SUBROUTINE cfltry")]
    b = [i for i, ln in enumerate(main) if ln.startswith("      END SUBROUTINE cfltry")]
    assert len(a) == 1 and len(b) == 1 and a[0] < b[0]
    with open(os.path.join(wrk, "cfltry.F"), "w") as f:
        f.write("\n".join(main[a[0]:b[0] + 1]) + "\n")
    for fn, txt in (("netcdf.inc", NETCDF_INC), ("nc_stub.F90", NC_STUB), ("areacfl_driver.F90", DRIVER)):
        with open(os.path.join(wrk, fn), "w") as f:
            f.write(txt)
    fc = [FC, "-cpp", "-ffixed-line-length-132", "-O2", "-ffp-contract=off"]
    objs = []
    for f in ["parameters_data.F"] + [os.path.join(src, m) for m in MODS]:
        subprocess.check_call(fc + ["-c", "-I" + src, f], cwd=wrk)
        objs.append(os.path.splitext(os.path.basename(f))[0] + ".o")
    subprocess.check_call([FC, "-O2", "-c", "nc_stub.F90"], cwd=wrk)
    subprocess.check_call(fc + ["-Dget_areav", "-Duse_netcdf", "-c", "-I" + wrk, "-I" + src,
                                os.path.join(src, "areasubs_diag.F")], cwd=wrk)
    subprocess.check_call(fc + ["-c", "cfltry.F"], cwd=wrk)
    subprocess.check_call([FC, "-O2", "-c", "areacfl_driver.F90"], cwd=wrk)
    subprocess.check_call([FC, "-o", "areacfl_driver", "areacfl_driver.o", "nc_stub.o", "areasubs_diag.o", "cfltry.o"] + objs,
                          cwd=wrk)


def smooth(rng, nx, ny, periodic, nmodes=5):
    x, y = np.arange(nx) / float(nx - 1 if not periodic else nx), np.arange(ny) / float(max(ny - 1, 1))
    f = np.zeros((nx, ny))
    for _ in range(nmodes):
        kx, ky = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        a, ph, ph2 = rng.standard_normal(), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        fx = np.cos(2 * np.pi * kx * x + ph) if periodic else np.sin(np.pi * kx * x + 0.3 * ph)
        f += a * fx[:, None] * np.cos(np.pi * ky * y + ph2)[None, :]
    return f / max(np.abs(f).max(), 1e-30)


def pressure(rng, nx, ny, dx, dt, cyc, spikes, nl=3):
    """nl layers of pressure whose geostrophic Courant numbers stay near 0.3, 0.2, 0.1 (three layers; otherwise 0.32
    falling by 0.03 per layer), plus `spikes`: (layer, i, j, Courant number) of single points raised so that the four
    differences around them exceed that number."""
    unit = dx / dt * dx * F0  # the pressure difference of Courant number 1
    p = np.zeros((nx, ny, nl))
    for k, c in enumerate((0.3, 0.2, 0.1) if nl == 3 else [0.32 - 0.03 * k for k in range(nl)]):
        f = smooth(rng, nx - 1 if cyc else nx, ny, cyc)
        if cyc:
            f = np.concatenate([f, f[:1]], axis=0)
        g = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
        p[:, :, k] = f * (c * unit / g)
    for k, i, j, c in spikes:
        p[i - 1, j - 1, k] += c * unit
        if cyc and i in (1, nx):
            p[nx - i, j - 1, k] = p[i - 1, j - 1, k]
    return p


def tie(p, pair, dx, dt):
    """Gives the last layer's |v| the same value, bit for bit, at the two differences of `pair`, above every other one.
    Both differences get the same operands up to a shift that is exact: p(i,j) is rounded to a multiple of 2^-30 and
    p(i+1,j) = p(i,j) +- D with D a multiple of 2^-30, so that p(i+1,j) - p(i,j) = +-D without rounding.  The sign is
    that of the background's p(i+2,j) - p(i,j), which keeps the next difference, p(i+2,j) - p(i+1,j), below D."""
    q = 2.0 ** -30
    D = np.round(TIE_COURANT * (dx / dt * dx * F0) / q) * q
    for i, j in pair:
        a = np.round(p[i - 1, j - 1, -1] / q) * q
        sg = 1.0 if p[i + 1, j - 1, -1] >= a else -1.0
        p[i - 1, j - 1, -1], p[i, j - 1, -1] = a, a + sg * D
        assert (a + sg * D) - a == sg * D


def inputs(name, dims, seed):
    nxta, nyta, nxaooc, nyaooc, ndxr = dims
    nxto, nyto = nxaooc * ndxr, nyaooc * ndxr
    nxpo, nypo, nxpa, nypa = nxto + 1, nyto + 1, nxta + 1, nyta + 1
    dxa = ndxr * DXO
    rng = np.random.default_rng(seed)
    cyc = name in ("cfl_cyc", "cfl_cyc6")
    F = {}
    # temperatures of both signs, a few K, with grid-scale noise (so that sum|terms| is well above |sum|)
    F["sst"] = 6.0 * smooth(rng, nxto, nyto, False) + 1.5 * rng.standard_normal((nxto, nyto)) + 0.7
    F["ast"] = 9.0 * smooth(rng, nxta, nyta, True) + 2.0 * rng.standard_normal((nxta, nyta)) - 1.3
    # offenders: layer 1 across the seam of the first two tile columns / rows; layer 2 on the last scanned row
    if cyc:
        oc_sp = [(0, nxpo, 17, 1.3), (1, 64, nypo, 1.2)]
    elif name.startswith("cfl_box"):
        oc_sp = [(0, 65, 17, 1.3), (1, 40, nypo, 1.2)]
    else:
        oc_sp = [(0, max(2, nxpo // 2), max(2, nypo // 2), 1.3), (1, 3, nypo, 1.2)]
    F["po"] = pressure(rng, nxpo, nypo, DXO, DTO, cyc, oc_sp, NLO.get(name, 3))
    if name in TIES:
        tie(F["po"], TIES[name], DXO, DTO)
    F["pa"] = pressure(rng, nxpa, nypa, dxa, DTA, True, [(0, nxpa, 9, 1.3), (1, 20, nypa, 1.2)])
    # stresses of 1e-4 m^2 s^-2 with one strong spot each, so that the mixed layer has offenders of its own
    vo = DXO / DTO
    tau1 = vo * F0 * HMOC  # rhf0hm*(2*tau1) = the velocity of Courant number 1
    F["tauxo"] = 1.0e-4 * smooth(rng, nxpo, nypo, False)
    F["tauyo"] = 1.0e-4 * smooth(rng, nxpo, nypo, False)
    F["tauxo"][min(20, nxpo - 2), min(30, nypo - 2)] += 2.4 * tau1
    va = dxa / DTA
    F["uekat"] = 0.05 * va * smooth(rng, nxpa, nyta, True)
    F["vekat"] = 0.05 * va * smooth(rng, nxta, nypa, True)
    F["uekat"][5, 3] += 1.3 * va
    return F


ORDER = ("sst", "ast", "po", "pa", "tauxo", "tauyo", "uekat", "vekat")


def run(wrk, dims, F, oc, at):
    with open(os.path.join(wrk, "areas.limits"), "w") as f:
        f.write(limits_text(oc, at))
    with open(os.path.join(wrk, "in.bin"), "wb") as fh:
        fh.write(np.array([DXO, DTO, dims[4] * DXO, DTA, HMOC]).tobytes())
        for k in ORDER:
            fh.write(np.asfortranarray(F[k], dtype=np.float64).tobytes(order="F"))
    txt = subprocess.run([os.path.join(wrk, "areacfl_driver")], cwd=wrk, check=True, stdout=subprocess.PIPE,
                         text=True).stdout
    return txt, open(os.path.join(wrk, "out.bin"), "rb").read()


def parse_nc(raw):
    """The stand-in's stream: (-id, len(name)), name for every nf_def_var; (id, n), n doubles for every put."""
    names, vals, o = {}, {}, 0
    while o < len(raw):
        vid, n = np.frombuffer(raw, dtype=np.int32, count=2, offset=o)
        o += 8
        if vid < 0:
            names[-vid] = raw[o:o + n].decode()
            o += n
        else:
            vals[names[int(vid)]] = np.frombuffer(raw, dtype=np.float64, count=n, offset=o).copy()
            o += 8 * n
    assert o == len(raw)
    return vals


def fnum(s):
    return float(s.replace("D", "E"))


def parse_areas(txt):
    """The subscripts and weights areavg prints, per fluid: dict of (n, 4) arrays it, wt, ip, wp."""
    out = {}
    oc = txt.index("Oceanic subareas:")
    at = txt.index("Atmospheric subareas:")
    end = txt.index("CFL testing")
    for key, part in (("oc", txt[oc:at]), ("at", txt[at:end])):
        it = re.findall(r"i1t, i2t, j1t, j2t =\s*(-?\d+)\s+(-?\d+)\s+(-?\d+)\s+(-?\d+)", part)
        ip = re.findall(r"i1p, i2p, j1p, j2p =\s*(-?\d+)\s+(-?\d+)\s+(-?\d+)\s+(-?\d+)", part)
        w = re.findall(r"weights =\s*(\S+)\s+(\S+)\s+(\S+)\s+(\S+)", part)
        assert len(it) == len(ip) and len(w) == 2 * len(it)
        out[key + "_it"] = np.array(it, dtype=np.int64).reshape(-1, 4)
        out[key + "_ip"] = np.array(ip, dtype=np.int64).reshape(-1, 4)
        out[key + "_wt"] = np.array(w[0::2], dtype=np.float64).reshape(-1, 4)
        out[key + "_wp"] = np.array(w[1::2], dtype=np.float64).reshape(-1, 4)
    return out


def parse_cfl(txt, nlo=3, nla=3):
    """cfltry's print-out per fluid (nlo ocean layers, nla atmospheric ones): printed maxima and Courant numbers in the order ml |u|, ml |v|, |u|(k), |v|(k),
    and the Bad lines as rows (quantity, i, j, printed Courant number) in print order."""
    out = {}
    body = txt[txt.index("CFL testing"):]
    cut = body.index("Atm. m.l.")
    for key, tag, part, nl in (("oc", "Ocn.", body[:cut], nlo), ("at", "Atm.", body[cut:], nla)):
        num = r"([-+0-9.DE]+)"
        mu = re.search(re.escape(tag) + r" m\.l\. \|u\| max, CFL =\s*" + num + r"\s+" + num, part)
        mv = re.search(re.escape(tag) + r" m\.l\. \|v\| max, CFL =\s*" + num + r"\s+" + num, part)
        mx, cf = [fnum(mu.group(1)), fnum(mv.group(1))], [fnum(mu.group(2)), fnum(mv.group(2))]
        for c in ("u", "v"):
            a = re.search(re.escape(tag) + r" max geos \|%s\|\(k\) =((?:\s*[-+0-9.DE]+){%d})" % (c, nl), part)
            b = re.search(re.escape(tag) + r" CFL geos \|%s\|\(k\) =((?:\s*[-+0-9.DE]+){%d})" % (c, nl), part)
            mx += [fnum(s) for s in a.group(1).split()]
            cf += [fnum(s) for s in b.group(1).split()]
        bad = []
        for ln in part.split("\n"):
            m = re.match(r"\s*Bad (m\.l\. )?\|([uv])\|; CFL, i, j(, k)? =\s*([-+0-9.DE]+)\s+(\d+)\s+(\d+)(?:\s+(\d+))?\s*$", ln)
            if m:
                c = 0 if m.group(2) == "u" else 1
                q = c if m.group(1) else 2 + c * nl + int(m.group(7)) - 1
                bad.append((q, int(m.group(5)), int(m.group(6)), fnum(m.group(4))))
        out[key + "_max"] = np.array(mx)
        out[key + "_cfl"] = np.array(cf)
        out[key + "_bad"] = np.array(bad, dtype=np.float64).reshape(-1, 4)
    return out


def check(name, res):
    """What the cases are for, asserted on the reference's own output."""
    if name == "cfl_box":
        bad, mx, cf = res["oc_bad"], res["oc_max"], res["oc_cfl"]
        cnt = np.array([(bad[:, 0] == q).sum() for q in range(len(mx))])
        assert all(1 <= c <= 50 for c in cnt[cnt > 0]), cnt
        assert cnt[0] > 0 or cnt[1] > 0, cnt
        assert (cnt[2:] > 0).any() and (cnt == 0).any(), cnt
        assert np.all(np.abs(bad[:, 3] / CFLCRIT - 1.0) > 1e-6) and np.all(np.abs(cf / CFLCRIT - 1.0) > 1e-6)
        nxpo, nypo = res["in_po"].shape[:2]
        # the maximum of some quantity on the last scanned row or column: among the Bad lines of a quantity the one
        # with the largest printed value
        last = False
        for q in np.nonzero(cnt)[0]:
            rows = bad[bad[:, 0] == q]
            i, j = rows[np.argmax(rows[:, 3]), 1:3]
            isu = q == 0 or 2 <= q < 5
            last |= (j == (nypo - 1 if isu else nypo)) or (i == (nxpo if isu else nxpo - 1))
        assert last, bad
    if name in TIES:  # the tie exists in the input, and the reference reports the first of the pair in scan order
        p, nl = res["in_po"], res["in_po"].shape[2]
        v = np.abs((1.0 / (DXO * F0)) * (p[1:, :, -1] - p[:-1, :, -1]))
        at = np.argwhere(v == v.max()) + 1
        (ia, ja), (ib, jb) = TIES[name]
        assert sorted(map(tuple, at.tolist())) == sorted([(ia, ja), (ib, jb)]), at
        assert v[ia - 1, ja - 1].tobytes() == v[ib - 1, jb - 1].tobytes()
        assert ja < jb and ia > ib  # j outer: the first in scan order is not the one with the smaller i
        assert res["oc_max"][2 + 2 * nl - 1] == float("%.7e" % v.max())
        rows = res["oc_bad"][res["oc_bad"][:, 0] == 2 + 2 * nl - 1]
        top = rows[rows[:, 3] == rows[:, 3].max()]
        assert [tuple(r) for r in top[:, 1:3].astype(int).tolist()] == [(ia, ja), (ib, jb)], rows
        assert len({po.tobytes() for po in np.moveaxis(p, 2, 0)}) == nl
    if name == "area_box":
        it, wt = res["oc_it"], res["oc_wt"]
        nxto, nyto = res["in_sst"].shape
        assert tuple(it[0]) == (1, nxto, 1, nyto) and np.all(wt[0] == 1.0)
        assert np.all(wt[1] == 1.0) and len(set(wt[2])) == 4 and np.all((wt[2] > 0) & (wt[2] < 1))
        assert it[3][2] == it[3][3] and it[4][0] == it[4][1]
        assert it[5][1] - it[5][0] + 1 > 256 and it[6][1] - it[6][0] + 1 == 3
        assert it[7][0] < it[8][0] <= it[7][1] and it[7][2] < it[8][2] <= it[7][3]


if __name__ == "__main__":
    only = sys.argv[1:]
    assert all(n in [c[0] for c in CASES] for n in only), only
    for ic, (name, dims, oc, at) in enumerate(CASES):
        if only and name not in only:
            continue
        F = inputs(name, dims, 700 + ic)
        wrk = tempfile.mkdtemp(prefix="areacfl_")
        try:
            build(wrk, dims, NLO.get(name, 3))
            txt, raw = run(wrk, dims, F, oc, at)
        finally:
            shutil.rmtree(wrk, ignore_errors=True)
        nc = parse_nc(raw)
        res = dict(c_dims=np.array(dims, dtype=np.int64), c_fnot=np.float64(F0), c_dxo=np.float64(DXO),
                   c_dto=np.float64(DTO), c_dxa=np.float64(dims[4] * DXO), c_dta=np.float64(DTA), c_hmoc=np.float64(HMOC),
                   c_cflcrit=np.float64(CFLCRIT), c_cyclic=np.int64(name in ("cfl_cyc", "cfl_cyc6")),
                   oc_lim=metres(oc), at_lim=metres(at), oc_tav=nc["ocdata"], at_tav=nc["atdata"])
        res.update({"in_" + k: np.asfortranarray(v) for k, v in F.items()})
        res.update(parse_areas(txt))
        res.update(parse_cfl(txt, NLO.get(name, 3)))
        assert len(res["oc_tav"]) == len(oc) and len(res["at_tav"]) == len(at)
        check(name, res)
        path = os.path.join(HERE, "areacfl_%s.npz" % name)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        assert size < (1 << 20), (name, size)
        sys.stderr.write("wrote areacfl_%s.npz (%d bytes): oc Bad %d, at Bad %d\n"
                         % (name, size, len(res["oc_bad"]), len(res["at_bad"])))
        if name == "area_atm":  # a small limits file in the reference's format, for hostinit.read_areas_limits
            with open(os.path.join(HERE, "areas_limits_area_atm.txt"), "w") as f:
                f.write(limits_text(oc, at))
