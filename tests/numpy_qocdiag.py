"""numpy restatement of the reference's periodic ocean dumps: qocdiag_out (src/qocdiag.F:303-687) and the subsample
of ocnc_out (src/nc_subs.F:837-1072).  Every expression keeps the reference's operand order (numpy does not contract),
so this is the oracle at full size, bitwise.  Arrays are (nxpo, nypo[, nlo]) as in the reference; results are
(nlo, jpwk, ipwk) - the order the device returns."""
import numpy as np

TERMS = ("dqdt", "qotjac", "qt2dif", "qt4dif", "qotent")


def count(n, nsko):
    m = n % nsko
    return min(m, 1) + (n - m) // nsko


def consts(cfg):
    """The scalar prologue of qocdiag_out (src/qocdiag.F:369-376) from an OceanConfig."""
    nl = cfg.nlo
    dxom2 = 1.0 / (cfg.dxo * cfg.dxo)
    return dict(adfaco=1.0 / (12.0 * cfg.dxo * cfg.dyo * cfg.fnot), dxom2=dxom2,
                bcfaco=cfg.bccooc * dxom2 / (0.5 * cfg.bccooc + 1.0),
                fohfac=[cfg.fnot / cfg.hoc[k] for k in range(nl)],
                bdrfac=0.5 * np.sign(cfg.fnot) * cfg.delek / cfg.hoc[nl - 1], rdto=1.0 / cfg.dto,
                ah2fac=[cfg.ah2oc[k] / cfg.fnot for k in range(nl)], ah4fac=[cfg.ah4oc[k] / cfg.fnot for k in range(nl)],
                cyclic=bool(cfg.cyclic))


def _lap(a, bcfaco, dxom2, cyclic):
    """del2p / del4p of src/qocdiag.F:405-477 (a: (nx, ny))."""
    nx, ny = a.shape
    d = np.zeros_like(a)
    d[:, 0] = bcfaco * (a[:, 1] - a[:, 0])
    d[:, ny - 1] = bcfaco * (a[:, ny - 2] - a[:, ny - 1])
    J = slice(1, ny - 1)
    Jm, Jp = slice(0, ny - 2), slice(2, ny)
    if cyclic:
        d[0, J] = (a[0, Jm] + a[nx - 2, J] + a[1, J] + a[0, Jp] - 4.0 * a[0, J]) * dxom2
    else:
        d[0, J] = bcfaco * (a[1, J] - a[0, J])
    d[1:nx - 1, J] = (a[1:nx - 1, Jm] + a[0:nx - 2, J] + a[2:nx, J] + a[1:nx - 1, Jp] - 4.0 * a[1:nx - 1, J]) * dxom2
    if cyclic:
        d[nx - 1, J] = d[0, J]
    else:
        d[nx - 1, J] = bcfaco * (a[nx - 2, J] - a[nx - 1, J])
    return d


def budget(po, pom, qo, qom, wekpo, entoc, c, nsko=1):
    """dict term -> (nlo, jpwk, ipwk): qocdiag_out's dqdt, qotjac, qt2dif, qt4dif, qotent at the subsampled points."""
    nx, ny, nl = po.shape
    cyc = c["cyclic"]
    ip, jp = count(nx, nsko), count(ny, nsko)
    res = {t: np.zeros((nl, jp, ip)) for t in TERMS}
    J, Jm, Jp = slice(1, ny - 1), slice(0, ny - 2), slice(2, ny)
    for k in range(nl):
        d2 = _lap(pom[:, :, k], c["bcfaco"], c["dxom2"], cyc)
        d4 = _lap(d2, c["bcfaco"], c["dxom2"], cyc)
        T = {t: np.zeros((nx, ny)) for t in TERMS}
        # interior columns 2..nxpo-1, and column 1 of the cyclic ocean (i-1 -> nxpo-1)
        I = np.arange(0 if cyc else 1, nx - 1)
        Il = np.where(I == 0, nx - 2, I - 1)
        Ir = I + 1
        p, q = po[:, :, k], qo[:, :, k]
        d6p = c["dxom2"] * (d4[I][:, Jm] + d4[Il][:, J] + d4[Ir][:, J] + d4[I][:, Jp] - 4.0 * d4[I][:, J])
        qt2 = c["ah2fac"][k] * d4[I][:, J]
        qt4 = -(c["ah4fac"][k] * d6p)
        jac = c["adfaco"] * ((q[Ir][:, J] - q[Il][:, J]) * (p[I][:, Jp] - p[I][:, Jm])
                             + (q[I][:, Jm] - q[I][:, Jp]) * (p[Ir][:, J] - p[Il][:, J])
                             + q[Ir][:, J] * (p[Ir][:, Jp] - p[Ir][:, Jm])
                             - q[Il][:, J] * (p[Il][:, Jp] - p[Il][:, Jm])
                             - q[I][:, Jp] * (p[Ir][:, Jp] - p[Il][:, Jp])
                             + q[I][:, Jm] * (p[Ir][:, Jm] - p[Il][:, Jm])
                             + p[I][:, Jp] * (q[Ir][:, Jp] - q[Il][:, Jp])
                             - p[I][:, Jm] * (q[Ir][:, Jm] - q[Il][:, Jm])
                             - p[Ir][:, J] * (q[Ir][:, Jp] - q[Ir][:, Jm])
                             + p[Il][:, J] * (q[Il][:, Jp] - q[Il][:, Jm]))
        if k == 0:
            ent = c["fohfac"][0] * (wekpo[I][:, J] - entoc[I][:, J])
        elif k == 1:
            ent = c["fohfac"][1] * entoc[I][:, J]
        else:
            ent = np.zeros_like(jac)
        if k == nl - 1:
            ent = ent - c["bdrfac"] * d2[I][:, J]
        dq = jac + qt2 + qt4 + ent
        for t, v in zip(TERMS, (dq, jac, qt2, qt4, ent)):
            T[t][I[0]:I[-1] + 1, J] = v
        dqb = c["rdto"] * (qo[:, :, k] - qom[:, :, k])
        if cyc:
            for t in TERMS:
                T[t][nx - 1, J] = T[t][0, J]
        else:
            T["dqdt"][0, J] = dqb[0, J]
            T["dqdt"][nx - 1, J] = dqb[nx - 1, J]
        T["dqdt"][:, 0] = dqb[:, 0]
        T["dqdt"][:, ny - 1] = dqb[:, ny - 1]
        for t in TERMS:
            res[t][k] = T[t][0:1 + (ip - 1) * nsko:nsko, 0:1 + (jp - 1) * nsko:nsko].T
    return res


def ocnc(sst, po, qo, wekto, tauxo, tauyo, gpoc, nsko=1, outfloc=(1, 1, 1, 1, 1, 1, 0)):
    """ocnc_out's subsample (src/nc_subs.F:898-1064): dict of the selected fields, (planes, rows, columns) each."""
    nx, ny, nl = po.shape

    def sub(a, n1, n2):
        i, j = count(n1, nsko), count(n2, nsko)
        return a[0:1 + (i - 1) * nsko:nsko, 0:1 + (j - 1) * nsko:nsko].T

    out = {}
    if outfloc[0] == 1:
        out["sst"] = sub(sst, nx - 1, ny - 1)[None]
    if outfloc[1] == 1:
        out["po"] = np.stack([sub(po[:, :, k], nx, ny) for k in range(nl)])
    if outfloc[2] == 1:
        out["qo"] = np.stack([sub(qo[:, :, k], nx, ny) for k in range(nl)])
    if outfloc[3] == 1:
        out["wekto"] = sub(wekto, nx - 1, ny - 1)[None]
    if outfloc[4] == 1:
        out["h"] = np.stack([(1.0 / gpoc[k]) * (sub(po[:, :, k + 1], nx, ny) - sub(po[:, :, k], nx, ny))
                             for k in range(nl - 1)])
    if outfloc[5] == 1:
        out["tauxo"] = sub(tauxo, nx, ny)[None]
        out["tauyo"] = sub(tauyo, nx, ny)[None]
    return out
