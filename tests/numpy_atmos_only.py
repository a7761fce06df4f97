"""numpy restatement of the heat half of xforc as a -Datmos_only build of the reference runs it (src/xfosubs.F:711-853
without the lines :805-812): the sea is a prescribed SST that is read once and held (src/q-gcm.F:753-786), fnetoc is
not computed and arocsm stays at the 0 it was set to.  It is numpy_heat.heat with those lines removed; bilint, the
serial sums, aml and the constants are numpy_heat's own.  The fixtures are tests/golden/ato_*.npz
(tests/golden/make_golden_atmos_only.py)."""
import numpy as np

from numpy_heat import _serial, aml, bilint, bilint_tables, load, params  # noqa: F401

CASES = ("ato_tiny", "ato_odd5", "ato_full4", "ato_allsea", "ato_r16", "ato_cyc72")
STATE = ("ast", "astm", "hmixa", "hmixam")
MOM_FIELDS = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa")
MOM_INTEGRALS = ("txisat", "txinat")
SST_SCALARS = ("arlaav", "slhfav", "oradav")  # (arocav is 0 exactly)


def heat_sst(astm, hmixam, sst, pam, dtopat, fsa, T, P):
    """The heat half of one `call xforc` of an atmos_only build: fnetat, the monitors (arocav = 0) and, for the
    parallel sums, n_<name> / abs_<name>; `cell_abs` (nxaooc, nyaooc): the sum of |terms| of every cell above the sea;
    `fnetat_land`: what fnetat would be with every cell treated as land."""
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
    ocnrad = D0up * sst
    slhf = xlamda * (sst - asto)
    atmrad = (Dmdown - Dmup) * asto
    term = ocfrac * (ocnrad + atmrad + slhf)
    cell = np.zeros((nxaooc, nyaooc))
    cabs = np.zeros((nxaooc, nyaooc))
    for jj in range(ndxr):  # (the serial order of every cell's own terms: jo outer, io inner)
        for ii in range(ndxr):
            cell = cell + term[ii::ndxr, jj::ndxr]
            cabs = cabs + np.abs(term[ii::ndxr, jj::ndxr])
    fnetat[io, jo] = cell
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
    return dict(fnetat=tail(fnetat), fnetat_land=tail(land), asto=asto, ocean=ocean, cell_abs=cabs,
                arlaav=arlaav, slhfav=slhfsm * ocnorm, oradav=oradsm * ocnorm, arocav=0.0,
                n_arlaav=nxta * nyta + nxaooc * nyaooc, abs_arlaav=aarl * (abs(Dmup) / float(natlan) if natlan else 0.0),
                n_slhfav=nxto * nyto, abs_slhfav=aslh * ocnorm, n_oradav=nxto * nyto, abs_oradav=aora * ocnorm,
                n_arocav=0, abs_arocav=0.0)


def tables_of(g, P):
    return bilint_tables(g["t_xta"], g["t_yta"], g["t_xto"], g["t_yto"], P["dxa"], P["dya"])


def state_before(g, P, c, s):
    """The reference's mixed-layer state before aml s of cycle c (s = 0: before the cycle's xforc too)."""
    k = c * P["nstr"] + s
    if k == 0:
        return {f: g["in_" + f] for f in STATE}
    c0, s0 = divmod(k - 1, P["nstr"])
    return {f: g["a%d%d_%s" % (c0, s0, f)] for f in STATE}


_restated = {}


def restated(case):
    """The heat half of every cycle's xforc restated from the reference's own inputs to it: c -> heat_sst(...).
    Computed once per case and shared."""
    if case not in _restated:
        g = load(case)
        P = params(g)
        T = tables_of(g, P)
        R = {}
        for c in range(P["K"]):
            S = state_before(g, P, c, 0)
            R[c] = heat_sst(S["astm"], S["hmixam"], g["in_sstm"], g["in_pam"], g["in_dtopat"], g["t_fsa"], T, P)
        _restated[case] = R
    return _restated[case]
