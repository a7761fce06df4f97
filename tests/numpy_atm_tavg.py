"""numpy restatement of the atmosphere's time averages and periodic dump: tavatm / tavout's atmosphere half
(src/timavge.F:278-421, 715-801) and atnc_out (src/nc_subs.F:1077-1326).

Elementwise, with the reference's expressions in the reference's order: it reproduces the golden files of
tests/golden/make_golden_atm_tavg.py bitwise (tests/test_atm_tavg_cpu.py) and is the oracle of the full-size GPU tests.
Arrays are (x, y[, k]) in Fortran index order, 0-based."""
import numpy as np

SUM_NAMES = ("txatav", "tyatav", "wtatav", "fmatav", "astav", "patav", "qatav", "uufa", "tufa", "utufa", "vvfa", "tvfa",
             "vtvfa")
ATNC_NAMES = ("ast", "pa", "qa", "wekta", "ha", "tauxa", "tauya", "hmixa")  # atnc_out's order
ATNC_FLAG = dict(ast=0, pa=1, qa=2, wekta=3, ha=4, tauxa=5, tauya=5, hmixa=6)  # index into outflat


def consts(dxa, fnot, hmat):
    """rdxaf0 of MODULE atconst (src/q-gcm.F) and tavatm's rhf0hm (src/timavge.F:301)."""
    return dict(rdxaf0=1.0 / (dxa * fnot), rhf0hm=0.5 / (fnot * hmat))


def tavini(nxpa, nypa, nla):
    nxta, nyta = nxpa - 1, nypa - 1
    z = lambda *s: np.zeros(s, order="F")
    return dict(nsumat=0, txatav=z(nxpa, nypa), tyatav=z(nxpa, nypa), wtatav=z(nxta, nyta), fmatav=z(nxta, nyta),
                astav=z(nxta, nyta), patav=z(nxpa, nypa, nla), qatav=z(nxpa, nypa, nla), uufa=z(nxpa, nyta),
                tufa=z(nxpa, nyta), utufa=z(nxpa, nyta), vvfa=z(nxta, nypa), tvfa=z(nxta, nypa), vtvfa=z(nxta, nypa))


def fluxes(f, c):
    """uuf, tuf, utuf (nxpa, nyta) and vvf, tvf, vtvf (nxta, nypa) of one tavatm call."""
    p1, ast, tx, ty = f["pa"][:, :, 0], f["ast"], f["tauxa"], f["tauya"]
    rdx, rh = c["rdxaf0"], c["rhf0hm"]
    nxpa, nypa = p1.shape
    nxta, nyta = nxpa - 1, nypa - 1
    # zonal advection: tuf(1) = tuf(nxpa) = 0.5*(ast(1,j) + ast(nxta,j)); uuf at every column 1..nxpa, no wrap
    tuf = np.zeros((nxpa, nyta), order="F")
    tuf[0] = 0.5 * (ast[0] + ast[nxta - 1])
    tuf[1:nxpa - 1] = 0.5 * (ast[1:nxta] + ast[0:nxta - 1])
    tuf[nxpa - 1] = 0.5 * (ast[0] + ast[nxta - 1])
    uuf = -(rdx * (p1[:, 1:] - p1[:, :-1])) - rh * (ty[:, 1:] + ty[:, :-1])
    utuf = uuf * tuf
    # meridional advection: inner rows, then the zonal boundaries
    vvf, tvf, vtvf = (np.zeros((nxta, nypa), order="F") for _ in range(3))
    j = slice(1, nypa - 1)
    vvf[:, j] = rdx * (p1[1:, j] - p1[:-1, j]) + rh * (tx[1:, j] + tx[:-1, j])
    tvf[:, j] = 0.5 * (ast[:, 1:] + ast[:, :-1])
    vtvf[:, j] = vvf[:, j] * tvf[:, j]
    vvf[:, 0], tvf[:, 0], vtvf[:, 0] = 0.0, ast[:, 0], 0.0
    vvf[:, -1], tvf[:, -1], vtvf[:, -1] = 0.0, ast[:, nypa - 2], 0.0
    return uuf, tuf, utuf, vvf, tvf, vtvf


def tavatm(S, f, c):
    """One contribution: f = pa, qa (nxpa,nypa,nla), tauxa, tauya (nxpa,nypa), wekta, fnetat, ast (nxta,nyta)."""
    S["txatav"] = S["txatav"] + f["tauxa"]
    S["tyatav"] = S["tyatav"] + f["tauya"]
    S["wtatav"] = S["wtatav"] + f["wekta"]
    S["fmatav"] = S["fmatav"] + f["fnetat"]
    S["astav"] = S["astav"] + f["ast"]
    for name, v in zip(("uufa", "tufa", "utufa", "vvfa", "tvfa", "vtvfa"), fluxes(f, c)):
        S[name] = S[name] + v
    S["patav"] = S["patav"] + f["pa"]
    S["qatav"] = S["qatav"] + f["qa"]
    S["nsumat"] += 1
    return S


def tavout(S):
    """tavout's atmosphere means and eddy fluxes (the sums are left alone)."""
    r = 0.0 if S["nsumat"] == 0 else 1.0 / float(S["nsumat"])
    M = {n: r * S[n] for n in SUM_NAMES}
    M["uptpat"] = M["utufa"] - M["uufa"] * M["tufa"]
    M["vptpat"] = M["vtvfa"] - M["vvfa"] * M["tvfa"]
    return M


def atnc_out(f, gpat, nska, outflat=(1,) * 7):
    """atnc_out's selected fields at the points (1+i*nska, 1+j*nska): dict name -> (planes, rows, columns), each plane
    as the reference fills wrk (i fastest).  f: pa, qa, ast, wekta, tauxa, tauya, hmixa."""
    s = lambda a: np.ascontiguousarray(a[::nska, ::nska].T)
    pa, nla = f["pa"], f["pa"].shape[2]
    out = {}
    for name in ATNC_NAMES:
        if int(outflat[ATNC_FLAG[name]]) != 1:
            continue
        if name in ("pa", "qa"):
            out[name] = np.stack([s(f[name][:, :, k]) for k in range(nla)])
        elif name == "ha":
            out[name] = np.stack([s((pa[:, :, k] - pa[:, :, k + 1]) / gpat[k]) for k in range(nla - 1)])
        else:
            out[name] = s(f[name])[None]
    return out
