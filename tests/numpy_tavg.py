"""numpy restatement of the ocean's time averages: tavocn / tavout (src/timavge.F:425-619, 667-880) and the fork's
running mean of po (avg_ocn_k247, src/timavge.F:624-662; the scaling of ocnc_avgout_k247, src/nc_subs.F:1944-2052).

Elementwise, with the reference's expressions in the reference's order: it reproduces the golden files of
tests/golden/make_golden_tavg.py bitwise (tests/test_tavg_cpu.py) and is the oracle of the full-size GPU tests.
Arrays are (x, y[, k]) in Fortran index order, 0-based."""
import numpy as np

SUM_NAMES = ("txocav", "tyocav", "wpocav", "wtocav", "fmocav", "sstav", "pocav", "qocav", "uufo", "tufo", "utufo",
             "vvfo", "tvfo", "vtvfo")


def consts(dxo, fnot, ycexp, hmoc, tsbdy, tnbdy, cyclic, sb_hflux, nb_hflux):
    """The constants tavocn derives (src/q-gcm.F:436, src/timavge.F:447-448) and its boundary options."""
    rdxof0 = 1.0 / (dxo * fnot)
    return dict(uvgfac=ycexp * rdxof0, rhf0hm=0.5 / (fnot * hmoc), tsbdy=tsbdy, tnbdy=tnbdy, cyclic=bool(cyclic),
                sb=bool(sb_hflux), nb=bool(nb_hflux))


def tavini(nxpo, nypo, nlo):
    nxto, nyto = nxpo - 1, nypo - 1
    z = lambda *s: np.zeros(s, order="F")
    return dict(nsumoc=0, txocav=z(nxpo, nypo), tyocav=z(nxpo, nypo), wpocav=z(nxpo, nypo), wtocav=z(nxto, nyto),
                fmocav=z(nxto, nyto), sstav=z(nxto, nyto), pocav=z(nxpo, nypo, nlo), qocav=z(nxpo, nypo, nlo),
                uufo=z(nxpo, nyto), tufo=z(nxpo, nyto), utufo=z(nxpo, nyto), vvfo=z(nxto, nypo), tvfo=z(nxto, nypo),
                vtvfo=z(nxto, nypo))


def fluxes(f, c):
    """uuf, tuf, utuf (nxpo, nyto) and vvf, tvf, vtvf (nxto, nypo) of one tavocn call."""
    p1, sst, tx, ty = f["po"][:, :, 0], f["sst"], f["tauxo"], f["tauyo"]
    uvg, rh = c["uvgfac"], c["rhf0hm"]
    nxpo, nypo = p1.shape
    nxto, nyto = nxpo - 1, nypo - 1
    uuf, tuf, utuf = (np.zeros((nxpo, nyto), order="F") for _ in range(3))
    i = slice(1, nxpo - 1)
    uuf[i] = -(uvg * (p1[i, 1:] - p1[i, :-1])) + rh * (ty[i, 1:] + ty[i, :-1])
    tuf[i] = 0.5 * (sst[1:nxto] + sst[0:nxto - 1])
    utuf[i] = uuf[i] * tuf[i]
    if c["cyclic"]:
        uuf[0] = -(uvg * (p1[0, 1:] - p1[0, :-1])) + rh * (ty[0, 1:] + ty[0, :-1])
        tuf[0] = 0.5 * (sst[0] + sst[nxto - 1])
        utuf[0] = uuf[0] * tuf[0]
        uuf[-1], tuf[-1], utuf[-1] = uuf[0], tuf[0], utuf[0]
    else:
        uuf[0], tuf[0], utuf[0] = 0.0, sst[0], 0.0
        uuf[-1], tuf[-1], utuf[-1] = 0.0, sst[nxto - 1], 0.0
    vvf, tvf, vtvf = (np.zeros((nxto, nypo), order="F") for _ in range(3))
    j = slice(1, nypo - 1)
    vvf[:, j] = uvg * (p1[1:, j] - p1[:-1, j]) - rh * (tx[1:, j] + tx[:-1, j])
    tvf[:, j] = 0.5 * (sst[:, 1:] + sst[:, :-1])
    vtvf[:, j] = vvf[:, j] * tvf[:, j]
    if c["sb"]:
        vvf[:, 0] = -(rh * (tx[1:, 0] + tx[:-1, 0]))
        tvf[:, 0] = 0.5 * (sst[:, 0] + c["tsbdy"])
        vtvf[:, 0] = vvf[:, 0] * tvf[:, 0]
    else:
        vvf[:, 0], tvf[:, 0], vtvf[:, 0] = 0.0, sst[:, 0], 0.0
    if c["nb"]:
        vvf[:, -1] = -(rh * (tx[1:, -1] + tx[:-1, -1]))
        tvf[:, -1] = 0.5 * (sst[:, -1] + c["tnbdy"])
        vtvf[:, -1] = vvf[:, -1] * tvf[:, -1]
    else:
        vvf[:, -1], tvf[:, -1], vtvf[:, -1] = 0.0, sst[:, -1], 0.0
    return uuf, tuf, utuf, vvf, tvf, vtvf


def tavocn(S, f, c):
    """One contribution: f = po, qo (nxpo,nypo,nlo), wekpo, tauxo, tauyo (nxpo,nypo), wekto, sst, fnetoc (nxto,nyto)."""
    S["txocav"] = S["txocav"] + f["tauxo"]
    S["tyocav"] = S["tyocav"] + f["tauyo"]
    S["wpocav"] = S["wpocav"] + f["wekpo"]
    S["wtocav"] = S["wtocav"] + f["wekto"]
    S["fmocav"] = S["fmocav"] + f["fnetoc"]
    S["sstav"] = S["sstav"] + f["sst"]
    for name, v in zip(("uufo", "tufo", "utufo", "vvfo", "tvfo", "vtvfo"), fluxes(f, c)):
        S[name] = S[name] + v
    S["pocav"] = S["pocav"] + f["po"]
    S["qocav"] = S["qocav"] + f["qo"]
    S["nsumoc"] += 1
    return S


def tavout(S):
    """tavout's means and eddy fluxes (the sums are left alone)."""
    r = 0.0 if S["nsumoc"] == 0 else 1.0 / float(S["nsumoc"])
    M = {n: r * S[n] for n in SUM_NAMES}
    M["uptpoc"] = M["utufo"] - M["uufo"] * M["tufo"]
    M["vptpoc"] = M["vtvfo"] - M["vvfo"] * M["tvfo"]
    return M


def po_mean(po_sum, nsum):
    """ocnc_avgout_k247: rnsum = 1/nsum, then rnsum * po_avg."""
    rnsum = 1.0 / float(nsum)
    return rnsum * po_sum
