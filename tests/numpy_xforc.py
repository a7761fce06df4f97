"""numpy restatement of the momentum half of xforc (src/xfosubs.F:137-709, with auvbcu :997-1234): every expression
in the reference's operand order, every sum in its order, so that IEEE arithmetic reproduces the reference bit for bit.
Arrays are indexed [i-1, j-1] (Fortran order); `tabs` holds the five weight tables (16, 0:ndxr, 0:ndxr)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("xf_cpl_tiny", "xf_cpl_tiny_ud", "xf_cpl_small_ud", "xf_odd5_ud", "xf_cyc4_ud", "xf_wide_ud", "xf_edge_ud",
         "xf_cycwide_ud")
POINTWISE = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa", "tauxo", "tauyo", "wekto", "wekpo")
INTEGRALS = ("txisat", "txinat", "txisoc", "txinoc")
TABLES = ("stbbb", "stbus", "stbvs", "stbun", "stbvn")

_cache = {}


def load(case):
    """The fixture as a dict (loaded once, shared, never modified by the tests)."""
    if case not in _cache:
        with np.load(os.path.join(GOLDEN, case + ".npz")) as g:
            _cache[case] = {k: g[k] for k in g.files}
    return _cache[case]


def params(g):
    """Dimensions and constants of a fixture."""
    nxta, nyta, nxaooc, nyaooc, ndxr = (int(v) for v in g["c_dims"])
    P = dict(nxta=nxta, nyta=nyta, nxaooc=nxaooc, nyaooc=nyaooc, ndxr=ndxr, nx1=int(g["c_nx1"]), ny1=int(g["c_ny1"]),
             cyclic=int(g["c_cyclic"]), tau_udiff=int(g["c_tau_udiff"]), fnot=float(g["c_fnot"]))
    for k in ("dxo", "cdat", "raoro", "hmat", "hmoc", "bccoat", "bccooc"):
        P[k] = float(g["c_" + k])
    return P


def tables(g):
    return {t: g["tab_" + t] for t in TABLES}


def _serial(terms):
    """Left-to-right sum of a list of scalars, and the sum of their magnitudes."""
    s, a = terms[0], abs(terms[0])
    for t in terms[1:]:
        s = s + t
        a = a + abs(t)
    return s, a


def xforc(pam1, pom1, tabs, P):
    """One call of xforc (momentum half).  Returns the twelve fields, the four integrals (txisoc / txinoc 0 for a box
    ocean) and, per integral, `n_<name>` (number of terms) and `abs_<name>` (sum of |terms|, before the dxo scaling)."""
    ndxr, nxta, nyta = P["ndxr"], P["nxta"], P["nyta"]
    nxpa, nypa = nxta + 1, nyta + 1
    nxtaor, nytaor = nxta * ndxr, nyta * ndxr
    nxpaor, nypaor = nxtaor + 1, nytaor + 1
    nxto, nyto = ndxr * P["nxaooc"], ndxr * P["nyaooc"]
    nxpo, nypo = nxto + 1, nyto + 1
    iocoff, jocoff = (P["nx1"] - 1) * ndxr, (P["ny1"] - 1) * ndxr
    fnot, dxo = P["fnot"], P["dxo"]
    dxa = ndxr * dxo
    rdxaf0, rdxof0 = 1.0 / (dxa * fnot), 1.0 / (dxo * fnot)
    hxafac, hxofac = 0.5 * rdxaf0, 0.5 * rdxof0
    cdat, hmat, hmoc, raoro = P["cdat"], P["hmat"], P["hmoc"], P["raoro"]
    uvekfc = 1.0 / (hmat * fnot * float(ndxr))
    hmrdxa = hmat / dxa
    cdhfaa = (cdat / fnot) / hmat
    cdhfab = (cdat / fnot) * (1.0 / hmat + raoro / hmoc)
    cdrfaa, cdrfab = cdat / abs(cdhfaa), cdat / abs(cdhfab)
    qu2faa, qu2fab = 4.0 * cdhfaa * cdhfaa, 4.0 * cdhfab * cdhfab
    ndxodd = ndxr % 2 == 1
    nijwid = ndxr + ndxr % 2
    wt = np.ones(ndxr + 1)
    if ndxodd:
        wt[0] = wt[ndxr] = 0.5
    else:
        wt[ndxr] = 0.0
    pam = np.asarray(pam1, dtype=np.float64)
    # coarse geostrophic velocity (:182-213)
    zbfcat = rdxaf0 / (0.5 * P["bccoat"] + 1.0)
    u1at, v1at = np.zeros((nxpa, nypa)), np.zeros((nxpa, nypa))
    u1at[:, 0] = -zbfcat * (pam[:, 1] - pam[:, 0])
    u1at[:, -1] = -zbfcat * (pam[:, -1] - pam[:, -2])
    u1at[:, 1:-1] = -hxafac * (pam[:, 2:] - pam[:, :-2])
    v1at[1:-1, 1:-1] = hxafac * (pam[2:, 1:-1] - pam[:-2, 1:-1])
    v1at[0, 1:-1] = hxafac * (pam[1, 1:-1] - pam[nxpa - 2, 1:-1])
    u1at[-1, 1:-1] = u1at[0, 1:-1]
    v1at[-1, 1:-1] = v1at[0, 1:-1]
    # bicubic interpolation (auvbcu)
    ic = np.arange(nxta)
    cols = [(ic - 1 + nxta) % nxta, ic, ic + 1, (ic + 2) % nxta]
    u1f, v1f = np.zeros((nxpaor, nypaor)), np.zeros((nxpaor, nypaor))
    for jc in range(1, nyta + 1):
        ud, vd = np.zeros((16, nxta)), np.zeros((16, nxta))
        for r, jd in enumerate((-1, 0, 1, 2)):
            j = jc + jd  # 1-based coarse row
            for q in range(4):
                if 1 <= j <= nypa and not (jc == nyta and jd == 2):
                    ud[4 * r + q] = u1at[cols[q], j - 1]
                    vd[4 * r + q] = v1at[cols[q], j - 1]
                elif jc == 1:  # jd = -1: zeros for u, the boundary row of u for v
                    vd[4 * r + q] = u1at[cols[q], 0]
                else:          # jc = nyta, jd = 2
                    vd[4 * r + q] = u1at[cols[q], nypa - 1]
        if jc == 1:
            tu, tv, njj = tabs["stbus"], tabs["stbvs"], ndxr
        elif jc == nyta:
            tu, tv, njj = tabs["stbun"], tabs["stbvn"], ndxr + 1
        else:
            tu, tv, njj = tabs["stbbb"], tabs["stbbb"], ndxr
        us, vs = np.zeros((nxta, ndxr, njj)), np.zeros((nxta, ndxr, njj))
        for k in range(16):
            us = us + ud[k][:, None, None] * tu[k, :ndxr, :njj][None]
            vs = vs + vd[k][:, None, None] * tv[k, :ndxr, :njj][None]
        j0 = (jc - 1) * ndxr
        u1f[:nxtaor, j0:j0 + njj] = us.reshape(nxtaor, njj)
        v1f[:nxtaor, j0:j0 + njj] = vs.reshape(nxtaor, njj)
    u1f[-1, :] = u1f[0, :]
    v1f[-1, :] = v1f[0, :]
    cdrfac, qu2fac = np.full((nxpaor, nypaor), cdrfaa), np.full((nxpaor, nypaor), qu2faa)
    pom = None if pom1 is None else np.asarray(pom1, dtype=np.float64)
    if P["tau_udiff"]:
        zbfcoc = rdxof0 / (0.5 * P["bccooc"] + 1.0)
        u1oc, v1oc = np.zeros((nxpo, nypo)), np.zeros((nxpo, nypo))
        u1oc[:, 0] = -zbfcoc * (pom[:, 1] - pom[:, 0])
        u1oc[:, -1] = -zbfcoc * (pom[:, -1] - pom[:, -2])
        u1oc[1:-1, 1:-1] = -hxofac * (pom[1:-1, 2:] - pom[1:-1, :-2])
        v1oc[1:-1, 1:-1] = hxofac * (pom[2:, 1:-1] - pom[:-2, 1:-1])
        if P["cyclic"]:
            u1oc[0, 1:-1] = -hxofac * (pom[0, 2:] - pom[0, :-2])
            v1oc[0, 1:-1] = hxofac * (pom[1, 1:-1] - pom[nxpo - 2, 1:-1])
            u1oc[-1, 1:-1] = -hxofac * (pom[-1, 2:] - pom[-1, :-2])
            v1oc[-1, 1:-1] = hxofac * (pom[1, 1:-1] - pom[nxpo - 2, 1:-1])
        else:
            v1oc[0, 1:-1] = zbfcoc * (pom[1, 1:-1] - pom[0, 1:-1])
            v1oc[-1, 1:-1] = zbfcoc * (pom[-1, 1:-1] - pom[-2, 1:-1])
        u1f[iocoff:iocoff + nxpo, jocoff:jocoff + nypo] -= u1oc
        v1f[iocoff:iocoff + nxpo, jocoff:jocoff + nypo] -= v1oc
        cdrfac[iocoff:iocoff + nxpo, jocoff:jocoff + nypo] = cdrfab
        qu2fac[iocoff:iocoff + nxpo, jocoff:jocoff + nypo] = qu2fab
    # drag law (:319-353)
    scasqd = -0.5 + 0.5 * np.sqrt(1.0 + qu2fac * (u1f * u1f + v1f * v1f))
    scashr = np.sqrt(scasqd)
    cdochi = cdrfac * scashr / (1.0 + scasqd)
    txf = cdochi * (u1f - scashr * v1f)
    tyf = cdochi * (v1f + scashr * u1f)
    R = {}
    R["tauxa"] = txf[::ndxr, ::ndxr].copy()
    R["tauya"] = tyf[::ndxr, ::ndxr].copy()
    # Ekman velocities on the coarse grid (:377-416)
    io = np.arange(nxta) * ndxr
    jo = np.arange(nypa) * ndxr
    ts = 0.5 * txf[io][:, jo]
    for i in range(1, ndxr):
        ts = ts + txf[io + i][:, jo]
    ts = ts + 0.5 * txf[io + ndxr][:, jo]
    vekat = uvekfc * ts
    jo = np.arange(nyta) * ndxr
    ts = 0.5 * tyf[io][:, jo]
    for j in range(1, ndxr):
        ts = ts + tyf[io][:, jo + j]
    ts = ts + 0.5 * tyf[io][:, jo + ndxr]
    uekat = np.zeros((nxpa, nyta))
    uekat[:nxta] = -uvekfc * ts
    uekat[nxta] = uekat[0]
    R["uekat"], R["vekat"] = uekat, vekat
    R["wekta"] = -hmrdxa * (uekat[1:, :] - uekat[:-1, :] + vekat[:, 1:] - vekat[:, :-1])
    # fine Ekman velocity at T points (:425-432) and its box average at p points (:446-471)
    wf = hxofac * (tyf[1:, :-1] + tyf[1:, 1:] - (tyf[:-1, :-1] + tyf[:-1, 1:]) + txf[:-1, :-1] + txf[1:, :-1]
                   - (txf[:-1, 1:] + txf[1:, 1:]))
    wekpa = np.zeros((nxpa, nypa))
    ibeg = np.arange(nxpa) * ndxr - (ndxr - 1) // 2  # 1-based first column of the box, per ia
    for ja in range(1, nypa + 1):
        jbeg = (ja - 1) * ndxr - (ndxr - 1) // 2
        jlo, jhi = max(1, jbeg), min(jbeg + nijwid - 1, nytaor)
        wsum, wtasum = np.zeros(nxpa), np.zeros(nxpa)
        for j in range(jlo, jhi + 1):
            wtj = wt[j - jbeg]
            for di in range(nijwid):
                it = (ibeg + di - 1 + nxtaor) % nxtaor  # 0-based
                wsum = wsum + wt[di] * wtj
                wtasum = wtasum + wt[di] * wtj * wf[it, j - 1]
        wekpa[:, ja - 1] = wtasum / wsum
    R["wekpa"] = wekpa
    # stress line integrals of the atmosphere's momentum constraints (:493-517)
    jsou, jnor = 1 + ndxr // 2, nypaor - ndxr // 2
    if ndxodd:
        rs = txf[:, jsou - 1] + txf[:, jsou]
        rn = txf[:, jnor - 1] + txf[:, jnor - 2]
        fac = 0.5 * dxo
    else:
        rs, rn, fac = txf[:, jsou - 1], txf[:, jnor - 1], dxo
    for name, r in (("txisat", rs), ("txinat", rn)):
        terms = [0.5 * r[0]] + [r[i] for i in range(1, nxpaor - 1)] + [0.5 * r[-1]]
        s, a = _serial(terms)
        R[name], R["n_" + name], R["abs_" + name] = fac * s, len(terms), a
    # ocean (:554-683)
    tauxo = raoro * txf[iocoff:iocoff + nxpo, jocoff:jocoff + nypo]
    tauyo = raoro * tyf[iocoff:iocoff + nxpo, jocoff:jocoff + nypo]
    R["tauxo"], R["tauyo"] = tauxo, tauyo
    wekto = hxofac * (tauyo[1:, 1:] + tauyo[1:, :-1] - (tauyo[:-1, 1:] + tauyo[:-1, :-1]) + tauxo[1:, :-1]
                      + tauxo[:-1, :-1] - (tauxo[1:, 1:] + tauxo[:-1, 1:]))
    R["wekto"] = wekto
    wekpo = np.zeros((nxpo, nypo))
    wekpo[1:-1, 1:-1] = 0.25 * (wekto[:-1, :-1] + wekto[:-1, 1:] + wekto[1:, :-1] + wekto[1:, 1:])
    wekpo[1:-1, 0] = 0.5 * (wekto[:-1, 0] + wekto[1:, 0])
    wekpo[1:-1, -1] = 0.5 * (wekto[:-1, -1] + wekto[1:, -1])
    if P["cyclic"]:
        wekpo[0, 1:-1] = 0.25 * (wekto[-1, :-1] + wekto[-1, 1:] + wekto[0, :-1] + wekto[0, 1:])
        wekpo[0, 0] = 0.5 * (wekto[-1, 0] + wekto[0, 0])
        wekpo[0, -1] = 0.5 * (wekto[-1, -1] + wekto[0, -1])
        wekpo[-1, :] = wekpo[0, :]
    else:
        wekpo[0, 1:-1] = 0.5 * (wekto[0, :-1] + wekto[0, 1:])
        wekpo[-1, 1:-1] = 0.5 * (wekto[-1, :-1] + wekto[-1, 1:])
        wekpo[0, 0], wekpo[0, -1] = wekto[0, 0], wekto[0, -1]
        wekpo[-1, 0], wekpo[-1, -1] = wekto[-1, 0], wekto[-1, -1]
    R["wekpo"] = wekpo
    for name, r in (("txisoc", tauxo[:, 0] + tauxo[:, 1]), ("txinoc", tauxo[:, -2] + tauxo[:, -1])):
        if P["cyclic"]:
            terms = [0.5 * r[0]] + [r[i] for i in range(1, nxpo - 1)] + [0.5 * r[-1]]
            s, a = _serial(terms)
            R[name], R["n_" + name], R["abs_" + name] = 0.5 * dxo * s, len(terms), a
        else:
            R[name], R["n_" + name], R["abs_" + name] = 0.0, 0, 0.0
    return R


_results = {}


def restated(case, s):
    """xforc of state s of a fixture, from the fixture's own tables (computed once, shared)."""
    if (case, s) not in _results:
        g = load(case)
        _results[(case, s)] = xforc(g["in%d_pam1" % s], g["in%d_pom1" % s], tables(g), params(g))
    return _results[(case, s)]
