"""areavg / areint (src/areasubs_diag.F) and cfltry (src/q-gcm.F:2121-2440) restated with IEEE operations in the
reference's order: serial sums, its operand order, no contraction.  The CPU suite holds this against the reference's own
results (tests/golden/areacfl_*.npz); the GPU suite holds the device against it."""
import os

import numpy as np

from qgcm_hip import hostinit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("area_box", "area_atm", "cfl_box", "cfl_cyc", "cfl_atm")
# the ocean's CFL check at other layer counts: case -> ocean layers (their areas and atmosphere repeat cfl_box / cfl_cyc
# and are not run again)
CFL_LAYER_CASES = {"cfl_box2": 2, "cfl_box5": 5, "cfl_cyc6": 6}
EXTREM = 1.0e30


def load(case):
    with np.load(os.path.join(GOLDEN, "areacfl_%s.npz" % case)) as z:
        return {k: z[k] for k in z.files}


def grid(g, fluid):
    """dx, dt, T cells (nx, ny) of a fixture's ocean ("oc") or atmosphere ("at")."""
    nxta, nyta, nxaooc, nyaooc, ndxr = (int(v) for v in g["c_dims"])
    if fluid == "oc":
        return float(g["c_dxo"]), float(g["c_dto"]), nxaooc * ndxr, nyaooc * ndxr
    return float(g["c_dxa"]), float(g["c_dta"]), nxta, nyta


def tables(g, fluid):
    dx, _, nx, ny = grid(g, fluid)
    lim = g[fluid + "_lim"]
    return hostinit.area_limits(lim[:, 0], lim[:, 1], lim[:, 2], lim[:, 3], dx, dx, nx, ny)


def areint(a, ilo, ihi, jlo, jhi, facw, face, facs, facn):
    """areint (:603-677) on array(nx, ny), 1-based subscripts: (answer, numerator, denominator, sum of |terms|, points).
    The last two are not the reference's: they size the bound of a sum in another order."""
    A = np.asarray(a, dtype=np.float64)
    col = lambda j: [float(v) for v in A[ilo - 1:ihi, j - 1]]
    arsum = wtsum = 0.0
    s, n = col(jlo), col(jhi)
    asums, wsums, asumn, wsumn = facw * s[0], facw, facw * n[0], facw
    absum = 0.0
    for j in range(jlo + 1, jhi):
        r = col(j)
        asumi, wsumi = facw * r[0], facw
        for v in r[1:-1] if ihi > ilo else []:
            asumi = asumi + v
            wsumi = wsumi + 1.0
        asumi = asumi + face * r[-1]
        wsumi = wsumi + face
        arsum = arsum + asumi
        wtsum = wtsum + wsumi
        absum += abs(facw * r[0]) + sum(abs(v) for v in r[1:-1]) + abs(face * r[-1])
    for v, w in zip(s[1:-1], n[1:-1]) if ihi > ilo else []:
        asums = asums + v
        wsums = wsums + 1.0
        asumn = asumn + w
        wsumn = wsumn + 1.0
    asums = asums + face * s[-1]
    wsums = wsums + face
    asumn = asumn + face * n[-1]
    wsumn = wsumn + face
    num = facs * asums + facn * asumn + arsum
    den = facs * wsums + facn * wsumn + wtsum
    for row, f in ((s, facs), (n, facn)):
        absum += abs(f) * (abs(facw * row[0]) + sum(abs(v) for v in row[1:-1]) + abs(face * row[-1]))
    return num / den, num, den, absum, (ihi - ilo + 1) * (jhi - jlo + 1)


def areavg(field, T):
    """Every area of the tables T (hostinit.area_limits): arrays avg, num, den, absum, npts."""
    out = [areint(field, int(T["i1"][m]), int(T["i2"][m]), int(T["j1"][m]), int(T["j2"][m]), float(T["facw"][m]),
                  float(T["face"][m]), float(T["facs"][m]), float(T["facn"][m])) for m in range(len(T["i1"]))]
    return tuple(np.array(c) for c in zip(*out))


def reorder_bound(absum, npts):
    """2 n 2^-53 sum|terms|: the project's bound on a sum of n terms taken in another order (both orders within
    n 2^-53 sum|terms| of the exact sum to first order)."""
    return 2.0 * npts * 2.0 ** -53 * absum


def cfl_names(nl):
    return ["ml_u", "ml_v"] + ["u%d" % (k + 1) for k in range(nl)] + ["v%d" % (k + 1) for k in range(nl)]


def cfltry(p, sx, sy, rdxf0, dt, dx, cflcrit=0.8, atm=False, rhf0hm=None):
    """cfltry for one fluid.  p (nx, ny, nl); ocean: sx, sy = tauxo, tauyo and rhf0hm = 0.5/(fnot*hmoc); atmosphere
    (atm): sx, sy = uekat (nx, ny-1), vekat (nx-1, ny).  Returns dict: maxima, courant (max*dt/dx as printed), nbad,
    loc (1-based i, j of the first maximum in scan order, j outer) over cfl_names(nl), and bad: the rows (quantity, i,
    j, Courant number) of the reference's Bad lines in its print order."""
    p = np.asarray(p, dtype=np.float64)
    nx, ny, nl = p.shape
    du = lambda k: -rdxf0 * (p[:, 1:, k] - p[:, :-1, k])   # (nx, ny-1): j = 1..ny-1, i = 1..nx
    dv = lambda k: rdxf0 * (p[1:, :, k] - p[:-1, :, k])    # (nx-1, ny)
    if atm:
        q = [np.abs(du(0) + sx), np.abs(dv(0) + sy)]
    else:
        q = [np.abs(du(0) + rhf0hm * (sy[:, 1:] + sy[:, :-1])), np.abs(dv(0) - rhf0hm * (sx[1:, :] + sx[:-1, :]))]
    q += [np.abs(du(k)) for k in range(nl)] + [np.abs(dv(k)) for k in range(nl)]
    order = [0, 1] + [x for k in range(nl) for x in (2 + k, 2 + nl + k)]  # the Bad lines: m.l. u, v, then u(k), v(k) per k
    mx, loc, nbad, bad = np.zeros(len(q)), np.zeros((len(q), 2), dtype=np.int64), np.zeros(len(q), dtype=np.int64), {}
    for n, a in enumerate(q):
        flat = a.ravel(order="F")  # i fastest: the scan order
        m = max(-EXTREM, float(flat.max()))
        at = int(np.argmax(flat))  # first occurrence
        mx[n] = m
        loc[n] = (at % a.shape[0] + 1, at // a.shape[0] + 1)
        rows = []
        if m * dt / dx >= cflcrit:
            c = (dt / dx) * flat
            for at in np.nonzero(c >= cflcrit)[0]:
                rows.append((n, at % a.shape[0] + 1, at // a.shape[0] + 1, c[at]))
        nbad[n] = len(rows)
        bad[n] = rows
    lines = [r for n in order for r in bad[n]]
    return {"names": cfl_names(nl), "maxima": mx, "courant": mx * dt / dx, "nbad": nbad, "loc": loc,
            "bad": np.array(lines, dtype=np.float64).reshape(-1, 4)}


def cfl_of_fixture(g, fluid):
    dx, dt, _, _ = grid(g, fluid)
    fnot = float(g["c_fnot"])
    rd = 1.0 / (dx * fnot)
    if fluid == "oc":
        return cfltry(g["in_po"], g["in_tauxo"], g["in_tauyo"], rd, dt, dx, float(g["c_cflcrit"]),
                      rhf0hm=0.5 / (fnot * float(g["c_hmoc"])))
    return cfltry(g["in_pa"], g["in_uekat"], g["in_vekat"], rd, dt, dx, float(g["c_cflcrit"]), atm=True)


def printed(x):
    """x as `1p,d15.7` prints it: 8 significant digits."""
    return np.array([float("%.7e" % v) for v in np.atleast_1d(x)])
