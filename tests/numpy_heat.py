"""numpy restatement of the atmospheric mixed layer (aml / amladf, src/amlsubs.F) and of the heat half of xforc
(src/xfosubs.F:711-853 with bilint, :891-993): every expression in the reference's operand order, every sum in its
serial order, so that IEEE arithmetic reproduces the reference bit for bit.  Arrays are indexed [i-1, j-1] (Fortran
order).  The fixtures are tests/golden/heat_*.npz (tests/golden/make_golden_heat.py)."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("heat_cpl_tiny", "heat_odd5", "heat_cyc4", "heat_wide", "heat_cpl_small", "heat_cyc72", "heat_300")
AML_FIELDS = ("ast", "astm", "hmixa", "hmixam", "entat")
AML_SUMS = ("xan", "enisat", "eninat", "centat")  # (cfraat is an exact count)
HEAT_SCALARS = ("arlaav", "slhfav", "oradav", "arocav")
CNAMES = ("dxo", "cdat", "raoro", "hmat", "hmoc", "bccoat", "bccooc", "dta", "hmamin", "hmadmp", "rrcpat", "tat1",
          "tat2", "xcexp", "at2d", "at4d", "ahmd", "aface1", "aface2", "bface", "cface", "dface", "gpat1", "gpat2",
          "fspco", "xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup", "C1down")

_cache = {}


def load(case):
    """The fixture as a dict (loaded once, shared, never modified by the tests); every part <case>_aml*.npz, where the
    generator had to split a case, is merged in."""
    if case not in _cache:
        d = {}
        for path in [os.path.join(GOLDEN, case + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, case + "_aml*.npz"))):
            with np.load(path) as g:
                assert not set(g.files) & set(d), path
                d.update({k: g[k] for k in g.files})
        _cache[case] = d
    return _cache[case]


def params(g):
    """Dimensions and constants of a fixture, with the derived constants of src/q-gcm.F:380-441."""
    nxta, nyta, nxaooc, nyaooc, ndxr = (int(v) for v in g["c_dims"])
    P = dict(nxta=nxta, nyta=nyta, nxaooc=nxaooc, nyaooc=nyaooc, ndxr=ndxr, nx1=int(g["c_nx1"]), ny1=int(g["c_ny1"]),
             cyclic=int(g["c_cyclic"]), fnot=float(g["c_fnot"]), K=int(g["c_K"]), nstr=int(g["c_nstr"]))
    for k in CNAMES:
        P[k] = float(g["c_" + k])
    dxa = ndxr * P["dxo"]
    P.update(dxa=dxa, dya=dxa, hdxam1=0.5 / dxa, dxam2=1.0 / (dxa * dxa), rdxaf0=1.0 / (dxa * P["fnot"]),
             tdta=2.0 * P["dta"], yla=nyta * dxa)
    return P


def _serial(values, start=0.0):
    """Left-to-right sum, and the sum of the magnitudes."""
    s, a = start, abs(start)
    for v in values:
        s = s + v
        a = a + abs(v)
    return s, a


def amladf(ast, astm, hmixa, hmixam, uekat, vekat, pa1, P):
    """tmrhs, hmrhs of src/amlsubs.F:246-563."""
    nxta, nyta = P["nxta"], P["nyta"]
    rdxaf0, hdxam1, hmat = P["rdxaf0"], P["hdxam1"], P["hmat"]
    d2tfac = P["at2d"] * P["dxam2"]
    d4tfac = P["at4d"] * P["dxam2"] ** 2
    hmdfac = P["ahmd"] * P["dxam2"]
    W = lambda f: np.roll(f, 1, axis=0)   # value at i-1 (cyclic)
    E = lambda f: np.roll(f, -1, axis=0)  # value at i+1
    # face velocities: U(i, j) on the west face of T cell (i, j), i = 1..nxpa; V(i, j) on its south face, j = 1..nypa
    U = -rdxaf0 * (pa1[:, 1:] - pa1[:, :-1]) + uekat
    V = vekat.copy()
    V[:, 1:-1] = rdxaf0 * (pa1[1:, 1:-1] - pa1[:-1, 1:-1]) + vekat[:, 1:-1]
    um, up = U[:-1, :], U[1:, :]
    vm, vp = V[:, :-1], V[:, 1:]
    xadvt = hdxam1 * (up * (ast + E(ast)) - um * (W(ast) + ast))
    xadvh = hdxam1 * (up * (hmixa + E(hmixa)) - um * (W(hmixa) + hmixa))
    yadvt, yadvh = np.zeros((nxta, nyta)), np.zeros((nxta, nyta))
    j = slice(1, nyta - 1)
    yadvt[:, j] = hdxam1 * (vp[:, j] * (ast[:, 2:] + ast[:, j]) - vm[:, j] * (ast[:, j] + ast[:, :-2]))
    yadvh[:, j] = hdxam1 * (vp[:, j] * (hmixa[:, 2:] + hmixa[:, j]) - vm[:, j] * (hmixa[:, j] + hmixa[:, :-2]))
    yadvt[:, 0] = hdxam1 * vp[:, 0] * (ast[:, 1] + ast[:, 0])
    yadvh[:, 0] = hdxam1 * (vp[:, 0] * (hmixa[:, 1] + hmixa[:, 0]) - vm[:, 0] * (hmixa[:, 0] + hmat))
    yadvt[:, -1] = hdxam1 * (-vm[:, -1] * (ast[:, -1] + ast[:, -2]))
    yadvh[:, -1] = hdxam1 * (vp[:, -1] * (hmat + hmixa[:, -1]) - vm[:, -1] * (hmixa[:, -1] + hmixa[:, -2]))
    tmrhs = -(xadvt + yadvt)
    del2t, lap = np.zeros((nxta, nyta)), np.zeros((nxta, nyta))
    del2t[:, j] = astm[:, :-2] + W(astm)[:, j] + E(astm)[:, j] + astm[:, 2:] - 4.0 * astm[:, j]
    del2t[:, 0] = W(astm)[:, 0] + E(astm)[:, 0] + astm[:, 1] - 3.0 * astm[:, 0]
    del2t[:, -1] = astm[:, -2] + W(astm)[:, -1] + E(astm)[:, -1] - 3.0 * astm[:, -1]
    lap[:, j] = hmixam[:, :-2] + W(hmixam)[:, j] + E(hmixam)[:, j] + hmixam[:, 2:] - 4.0 * hmixam[:, j]
    lap[:, 0] = hmat + W(hmixam)[:, 0] + E(hmixam)[:, 0] + hmixam[:, 1] - 4.0 * hmixam[:, 0]
    lap[:, -1] = hmixam[:, -2] + W(hmixam)[:, -1] + E(hmixam)[:, -1] + hmat - 4.0 * hmixam[:, -1]
    hmrhs = -(xadvh + yadvh) + hmdfac * lap
    d = del2t
    d4 = np.zeros((nxta, nyta))
    d4[:, j] = d[:, :-2] + W(d)[:, j] + E(d)[:, j] + d[:, 2:] - 4.0 * d[:, j]
    d4[:, 0] = W(d)[:, 0] + E(d)[:, 0] + d[:, 1] - 3.0 * d[:, 0]
    d4[:, -1] = d[:, -2] + W(d)[:, -1] + E(d)[:, -1] - 3.0 * d[:, -1]
    tmrhs = tmrhs + d2tfac * d - d4tfac * d4
    return tmrhs, hmrhs


def xintp(v):
    """src/intsubs.f:78-133, and the sum of |terms|."""
    nx, ny = v.shape
    sump, a = 0.0, 0.0
    for j in range(1, ny - 1):
        sumi, ai = _serial(list(v[1:-1, j]) + [0.5 * v[-1, j]], 0.5 * v[0, j])
        sump += sumi
        a += ai
    xxs, as_ = _serial(list(v[1:-1, 0]), 0.5 * v[0, 0])
    xxn, an = _serial(list(v[1:-1, -1]), 0.5 * v[0, -1])
    xxs = xxs + 0.5 * v[-1, 0]
    xxn = xxn + 0.5 * v[-1, -1]
    return sump + 0.5 * (xxs + xxn), a + 0.5 * (as_ + an + 0.5 * abs(v[-1, 0]) + 0.5 * abs(v[-1, -1]))


def aml(S, fnetat, wekta, uekat, vekat, pa, pam, xc1ast, dtopat, P):
    """One `call aml` (src/amlsubs.F:47-238) from the state S = dict(ast, astm, hmixa, hmixam).  Returns the new state
    with entat, the scalars xan, enisat, eninat, cfraat, centat and, per parallel sum, n_<name> / abs_<name>: the
    number of terms and the sum of their magnitudes (before the dxa, dya scaling); `branches`: the masks of the three
    branches of the step."""
    nxta, nyta = P["nxta"], P["nyta"]
    ast, astm, hmixa, hmixam = S["ast"], S["astm"], S["hmixa"], S["hmixam"]
    hmat, tdta, tat1, rrcpat, xcexp = P["hmat"], P["tdta"], P["tat1"], P["rrcpat"], P["xcexp"]
    hmainv = 1.0 / hmat
    hdrcdt = P["hmadmp"] * rrcpat * tdta
    diabcr = tat1 - 2.0 * hdrcdt
    entfac = 1.0 / (tdta * (P["tat2"] - tat1))
    xbfac = xcexp * P["bface"]
    # aface(l) / gpat(l) over the nla - 1 interfaces (src/amlsubs.F:88-90); the fixtures carry the two of three layers
    aface, gpat = P.get("aface", (P["aface1"], P["aface2"])), P.get("gpat", (P["gpat1"], P["gpat2"]))
    nla = pam.shape[2]
    assert len(aface) >= nla - 1 and len(gpat) >= nla - 1
    afacdp = [aface[l] / gpat[l] for l in range(nla - 1)]
    tmrhs, hmrhs = amladf(ast, astm, hmixa, hmixam, uekat, vekat, pa[:, :, 0], P)
    cold = astm <= diabcr
    with np.errstate(divide="ignore", invalid="ignore"):
        dhdiab = hdrcdt * (hmixam - hmat) / (tat1 - astm)
        hn = hmixam + tdta * hmrhs - dhdiab
        dhfix = np.maximum(P["hmamin"] - hn, 0.0)
        hn = hn + dhfix
        dtfix = dhfix * (tat1 - astm) / hmixam
    hnew = np.where(cold, hn, hmat)
    dtfix = np.where(cold, dtfix, 0.0)
    trhtot = tmrhs + rrcpat * fnetat / hmixam - hmainv * wekta * astm
    astnew = astm + tdta * trhtot + dtfix
    xfaent = xbfac * (hmixam - hmat) + P["dface"] * (xcexp * astm + xc1ast)
    dtanew = tat1 - astnew
    conena = entfac * hmixa * np.minimum(0.0, dtanew)
    xfa = xfaent - xcexp * conena
    astnew = astnew + np.minimum(0.0, dtanew)
    cterm = 0.5 - np.copysign(0.5, dtanew)
    cfrasm, _ = _serial(cterm.ravel(order="F"))
    centsm, acent = _serial((-conena).ravel(order="F"))
    # entrainment on the p grid
    Wx = np.roll(xfa, 1, axis=0)
    ent = np.zeros((nxta + 1, nyta + 1))
    ent[:-1, 1:-1] = 0.25 * (Wx[:, :-1] + xfa[:, :-1] + Wx[:, 1:] + xfa[:, 1:])
    ent[:-1, 0] = 0.5 * (Wx[:, 0] + xfa[:, 0])
    ent[:-1, -1] = 0.5 * (Wx[:, -1] + xfa[:, -1])
    ent[-1, :] = ent[0, :]
    adpsum = 0.0
    for l in range(nla - 1):  # src/amlsubs.F:203-209
        adpsum = adpsum + afacdp[l] * (pam[:, :, l] - pam[:, :, l + 1])
    ent = ent + adpsum + P["cface"] * dtopat
    xi, axi = xintp(ent)
    ens, aens = _serial(list(ent[1:-1, 0]), 0.5 * ent[0, 0])
    enn, aenn = _serial(list(ent[1:-1, -1]), 0.5 * ent[0, -1])
    ens = ens + 0.5 * ent[-1, 0]
    enn = enn + 0.5 * ent[-1, -1]
    atnorm = 1.0 / (nxta * nyta)
    return dict(ast=astnew, astm=ast.copy(), hmixa=hnew, hmixam=hmixa.copy(), entat=ent, xfa=xfa,
                xan=xi * P["dxa"] * P["dya"], enisat=P["dxa"] * ens, eninat=P["dxa"] * enn, cfraat=cfrasm * atnorm,
                centat=centsm * P["dxa"] * P["dya"],
                n_xan=(nxta + 1) * (nyta + 1), abs_xan=axi, n_enisat=nxta + 1, abs_enisat=aens + 0.5 * abs(ent[-1, 0]),
                n_eninat=nxta + 1, abs_eninat=aenn + 0.5 * abs(ent[-1, -1]), n_centat=nxta * nyta, abs_centat=acent,
                branches=dict(diab=~cold, floor=cold & (dhfix > 0.0), conv=dtanew < 0.0))


def bilint_tables(xta, yta, xto, yto, dxa, dya):
    """The index and weight vectors of bilint (src/xfosubs.F:916-980): iam, iap, jam, jap 1-based."""
    nxat, nyat = len(xta), len(yta)
    dxainv, dyainv = 1.0 / dxa, 1.0 / dya
    iam = np.trunc(1.0 + dxainv * (xto - xta[0])).astype(np.int64)
    iap = iam + 1
    xam = np.where(iam >= 1, xta[np.clip(iam, 1, nxat) - 1], xta[0] - dxa)
    wpx = dxainv * (xto - xam)
    wmx = 1.0 - wpx
    iam = 1 + np.mod(iam + nxat - 1, nxat)
    iap = 1 + np.mod(iap + nxat - 1, nxat)
    jam = np.trunc(1.0 + dyainv * (yto - yta[0])).astype(np.int64)
    jap = jam + 1
    jam = np.maximum(jam, 1)
    jap = np.minimum(jap, nyat)
    wpy = dyainv * (yto - yta[jam - 1])
    wmy = 1.0 - wpy
    return dict(iam=iam, iap=iap, wmx=wmx, wpx=wpx, jam=jam, jap=jap, wmy=wmy, wpy=wpy)


def bilint(T, atmos):
    """The interpolant of src/xfosubs.F:984-989 with fmult = 1 from the tables T."""
    im, ip, jm, jp = T["iam"] - 1, T["iap"] - 1, T["jam"] - 1, T["jap"] - 1
    wmx, wpx = T["wmx"][:, None], T["wpx"][:, None]
    wmy, wpy = T["wmy"][None, :], T["wpy"][None, :]
    return 1.0 * (wmx * wmy * atmos[np.ix_(im, jm)] + wpx * wmy * atmos[np.ix_(ip, jm)]
                  + wmx * wpy * atmos[np.ix_(im, jp)] + wpx * wpy * atmos[np.ix_(ip, jp)])


def heat(astm, hmixam, sstm, pam, dtopat, fsa, fso, T, P):
    """The heat half of one `call xforc` (src/xfosubs.F:711-853): fnetoc, fnetat, the four monitors and, for the
    parallel sums, n_<name> / abs_<name>; `cell_abs` (nxaooc, nyaooc): the sum of |terms| of every cell above the
    ocean; `fnetat_land`: what fnetat would be with every cell treated as land."""
    nxta, nyta, nxaooc, nyaooc, ndxr = P["nxta"], P["nyta"], P["nxaooc"], P["nyaooc"], P["ndxr"]
    nx1, ny1 = P["nx1"], P["ny1"]
    nxto, nyto = nxaooc * ndxr, nyaooc * ndxr
    Dmup, Dmdown, D0up, xlamda = P["Dmup"], P["Dmdown"], P["D0up"], P["xlamda"]
    asto = bilint(T, astm)
    fnetat = -fsa[None, :] - Dmup * astm
    land = fnetat.copy()
    arlasm, aarl = _serial(astm.ravel(order="F"))
    io, jo = slice(nx1 - 1, nx1 - 1 + nxaooc), slice(ny1 - 1, ny1 - 1 + nyaooc)
    fnetat[io, jo] = 0.0
    for v in astm[io, jo].ravel(order="F"):
        arlasm = arlasm - v
        aarl = aarl + abs(v)
    natlan = nxta * nyta - nxaooc * nyaooc
    arlaav = 0.0 if natlan == 0 else Dmup * arlasm / float(natlan)
    ocfrac = P["dxo"] * P["dxo"] / (P["dxa"] * P["dya"])
    fmafac = P["Adown11"] * 0.25 / P["gpat1"]
    fmatop = 0.25 * (P["Cmup"] + P["C1down"])
    hmafac = -P["hmadmp"] - P["Bmup"] - P["B1down"]
    ocnrad = D0up * sstm
    slhf = xlamda * (sstm - asto)
    atmrad = Dmdown * asto
    fnetoc = -fso[None, :] - atmrad - ocnrad - slhf
    atmrad2 = (Dmdown - Dmup) * asto
    term = ocfrac * (ocnrad + atmrad2 + slhf)
    cell = np.zeros((nxaooc, nyaooc))
    cabs = np.zeros((nxaooc, nyaooc))
    for jj in range(ndxr):  # (the serial order of every cell's own terms: jo outer, io inner)
        for ii in range(ndxr):
            cell = cell + term[ii::ndxr, jj::ndxr]
            cabs = cabs + np.abs(term[ii::ndxr, jj::ndxr])
    fnetat[io, jo] = cell
    arocsm, aaro = _serial(atmrad.ravel(order="F"))
    slhfsm, aslh = _serial(slhf.ravel(order="F"))
    oradsm, aora = _serial(ocnrad.ravel(order="F"))

    def tail(f):
        return (f - fmafac * (pam[:-1, :-1, 0] - pam[:-1, :-1, 1] + pam[1:, :-1, 0] - pam[1:, :-1, 1]
                              + pam[:-1, 1:, 0] - pam[:-1, 1:, 1] + pam[1:, 1:, 0] - pam[1:, 1:, 1])
                - fmatop * (dtopat[:-1, :-1] + dtopat[1:, :-1] + dtopat[:-1, 1:] + dtopat[1:, 1:])
                + hmafac * (hmixam - P["hmat"]))

    ocnorm = 1.0 / (nxto * nyto)
    ocean = np.zeros((nxta, nyta), dtype=bool)
    ocean[io, jo] = True
    return dict(fnetoc=fnetoc, fnetat=tail(fnetat), fnetat_land=tail(land), asto=asto, ocean=ocean, cell_abs=cabs,
                arlaav=arlaav, slhfav=slhfsm * ocnorm, oradav=oradsm * ocnorm, arocav=arocsm * ocnorm,
                n_arlaav=nxta * nyta + nxaooc * nyaooc, abs_arlaav=aarl * (abs(Dmup) / float(natlan) if natlan else 0.0),
                n_slhfav=nxto * nyto, abs_slhfav=aslh * ocnorm, n_oradav=nxto * nyto, abs_oradav=aora * ocnorm,
                n_arocav=nxto * nyto, abs_arocav=aaro * ocnorm)


def tables_of(g, P):
    return bilint_tables(g["t_xta"], g["t_yta"], g["t_xto"], g["t_yto"], P["dxa"], P["dya"])


_restated = {}


def restated(case):
    """The fixture's K cycles re-fed call by call: the restatement of every call from the reference's own inputs to
    that call.  dict: ("x", c) -> heat(...), ("a", c, s) -> aml(...).  Computed once per case and shared."""
    if case in _restated:
        return _restated[case]
    g = load(case)
    P = params(g)
    T = tables_of(g, P)
    R = {}
    S = {k: g["in_" + k] for k in ("ast", "astm", "hmixa", "hmixam")}
    for c in range(P["K"]):
        R[("x", c)] = heat(S["astm"], S["hmixam"], g["in_sstm"], g["in_pam"], g["in_dtopat"], g["t_fsa"], g["t_fso"], T, P)
        for s in range(P["nstr"]):
            R[("a", c, s)] = aml(S, g["x%d_fnetat" % c], g["x%d_wekta" % c], g["x%d_uekat" % c], g["x%d_vekat" % c],
                                 g["in_pa"], g["in_pam"], g["in_xc1ast"], g["in_dtopat"], P)
            S = {k: g["a%d%d_%s" % (c, s, k)] for k in ("ast", "astm", "hmixa", "hmixam")}
    _restated[case] = R
    return R
