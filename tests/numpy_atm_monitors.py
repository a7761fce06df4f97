"""numpy restatement of the atmosphere half of monnc_comp, of courat and of the atmospheric valids
(src/monitor_diag.F:160-172, 185-475, 1213-1444; src/valsubs.F:120-269), written from the Fortran.  The oracle of
qgcm_hip_atm_monitors for the sizes the reference fixtures do not cover.

monitors(f, c) -> (values, scales):
  f: pa, pam, qa (nxpa,nypa,nla), wekpa, entat, tauxa, tauya (nxpa,nypa), wekta, ast, hmixa (nxta,nyta),
     uekat (nxpa,nyta), vekat (nxta,nypa)
  c: dxa, dta, fnot, gpat, hat, ah4at, rhoat, cpat, hmat, davgat, aup, bup, cup, dup, nx1, ny1, nxaooc, nyaooc
  values: the MODULE monitor names of qgcm_hip.model.ATM_MONITOR_LAYOUT
  scales: for every quantity that is an area integral (or built from them: olrtop), the same expression with every
          integrand and factor replaced by its modulus; for the other quantities their own modulus.
valids(f) -> the twelve extrema of qgcm_hip_atm_valids.
"""
import numpy as np

from numpy_monitors import del4, genint


def synthetic_fields(acfg, seed):
    """Seeded wekta, ast, hmixa (T grid), tauxa, tauya (p grid), uekat (nxpa,nyta), vekat (nxta,nypa): smooth fields
    with both components non-zero plus noise; hmixa positive."""
    rng = np.random.default_rng(seed)
    nxp, nyp = acfg.nxpa, acfg.nypa

    def smooth(nx, ny, amp, off=0.0):
        x = np.arange(nx)[:, None] / max(nx - 1.0, 1.0)
        y = np.arange(ny)[None, :] / max(ny - 1.0, 1.0)
        base = np.sin(2 * np.pi * x + 0.3) * np.cos(np.pi * y) + 0.4 * y
        return np.asfortranarray(off + amp * (base + 0.1 * rng.uniform(-1.0, 1.0, (nx, ny))))
    return dict(wekta=smooth(nxp - 1, nyp - 1, 2.0e-3), tauxa=smooth(nxp, nyp, 0.15), tauya=smooth(nxp, nyp, 0.05),
                ast=smooth(nxp - 1, nyp - 1, 8.0, 2.0), hmixa=smooth(nxp - 1, nyp - 1, 150.0, 1000.0),
                uekat=smooth(nxp, nyp - 1, 0.8), vekat=smooth(nxp - 1, nyp, 0.6))


def _serial(a):
    """Left-to-right sum, as a Fortran DO loop adds (np.cumsum is sequential)."""
    return float(np.cumsum(a)[-1])


def _courat_layer(p, rdx, cfac, uek=None, vek=None):
    """courat's face velocities of every T cell (:1247-1434): u on (nxpa, nyta), v on (nxta, nypa) with vekat (mixed
    layer) or 0 (Q-G layers) on the zonal boundaries; returns umin, umax, vmin, vmax, Courant number."""
    u = -rdx * (p[:, 1:] - p[:, :-1])
    if uek is not None:
        u = u + uek
    v = rdx * (p[1:, :] - p[:-1, :])
    if vek is not None:
        v = v + vek
        v[:, 0], v[:, -1] = vek[:, 0], vek[:, -1]
    else:
        v[:, 0], v[:, -1] = 0.0, 0.0
    um, up, vm, vp = u[:-1, :], u[1:, :], v[:, :-1], v[:, 1:]
    vsq = (um + up) * (um + up) + (vm + vp) * (vm + vp)
    return u.min(), u.max(), v.min(), v.max(), cfac * np.sqrt(vsq.max())


def monitors(f, c):
    pa, pam, qa = f["pa"], f["pam"], f["qa"]
    nx, ny, nl = pa.shape
    nxt, nyt = nx - 1, ny - 1
    dta = c["dta"]
    rdx = 1.0 / (c["dxa"] * c["fnot"])
    dxm2 = 1.0 / (c["dxa"] * c["dxa"])
    cfac = 0.5 / c["dxa"] * dta
    on = 1.0 / (nxt * nyt)
    rho = c["rhoat"]
    v, s = {}, {}

    def put(name, val, sc):
        v[name], s[name] = val, sc

    def gi(a, fw, fs):
        return genint(a, fw, fs), genint(np.abs(a), fw, fs)

    wekta, wekpa, entat = f["wekta"], f["wekpa"], f["entat"]
    for name, a, fw in (("wetmat", wekta, 1.0), ("watmat", np.abs(wekta), 1.0), ("wepmat", wekpa, 0.5),
                        ("wapmat", np.abs(wekpa), 0.5)):
        x, xs = gi(a, fw, fw)
        put(name, x * on, xs * on)
    ent, ena, sent, sena = (np.zeros(nl - 1) for _ in range(4))
    x, xs = gi(entat, 0.5, 0.5)
    ent[0], sent[0] = x * on, xs * on
    x, xs = gi(np.abs(entat), 0.5, 0.5)
    ena[0], sena[0] = x * on, xs * on
    put("entmat", ent, sent)
    put("enamat", ena, sena)
    eta_m, et2_m, ddtpe, pken = (np.zeros(nl - 1) for _ in range(4))
    s_eta, s_et2, s_ddtpe, s_pken = (np.zeros(nl - 1) for _ in range(4))
    for k in range(nl - 1):
        rg = 1.0 / c["gpat"][k]
        eta = rg * (pa[:, :, k] - pa[:, :, k + 1])
        etadot = (rg / dta) * (pa[:, :, k] - pa[:, :, k + 1] - pam[:, :, k] + pam[:, :, k + 1])
        x, xs = gi(eta, 0.5, 0.5)
        eta_m[k], s_eta[k] = x * on, xs * on
        x, xs = gi(eta * eta, 0.5, 0.5)
        et2_m[k], s_et2[k] = x * on, xs * on
        x, xs = gi(eta * etadot, 0.5, 0.5)
        ddtpe[k], s_ddtpe[k] = rho * c["gpat"][k] * x, abs(rho * c["gpat"][k]) * xs     # no atnorm (:282)
        if k == 0:
            x, xs = gi(eta * entat, 0.5, 0.5)
            pken[0], s_pken[0] = rho * c["gpat"][0] * x * on, abs(rho * c["gpat"][0]) * xs * on
    put("etamat", eta_m, s_eta)
    put("et2mat", et2_m, s_et2)
    put("ddtpeat", ddtpe, s_ddtpe)
    put("pkenat", pken, s_pken)
    ug1 = -rdx * (pa[:, 1:, 0] - pa[:, :-1, 0])
    ux, uxs = gi(ug1 * (0.5 * (f["tauxa"][:, 1:] + f["tauxa"][:, :-1])), 0.5, 1.0)
    vg1 = rdx * (pa[1:, :, 0] - pa[:-1, :, 0])
    vy, vys = gi(vg1 * (0.5 * (f["tauya"][1:, :] + f["tauya"][:-1, :])), 1.0, 0.5)
    put("utauat", rho * (vy + ux) * on, abs(rho) * (vys + uxs) * on)

    names = ("pavgat", "qavgat", "ah4dat", "kealat", "ddtkeat", "atstpos", "atstval")
    L = {n: np.zeros(nl) for n in names}
    S = {n: np.zeros(nl) for n in names}
    for k in range(nl):
        ugat = -rdx * (pam[:, 1:, k] - pam[:, :-1, k])
        _, d4u = del4(ugat, dxm2, True)
        vgat = rdx * (pam[1:, :, k] - pam[:-1, :, k])
        d2v, d4v = del4(vgat, dxm2, True)
        ug = -rdx * (pa[:, 1:, k] - pa[:, :-1, k])
        ugdot = -(rdx / dta) * (pa[:, 1:, k] - pa[:, :-1, k] - pam[:, 1:, k] + pam[:, :-1, k])
        ujeta = np.array([abs(_serial(ug[:, j]) - ug[-1, j]) / float(nxt) for j in range(nyt)])
        pos, val = 0, 0.0
        for j in range(nyt):
            if ujeta[j] > val:
                pos, val = j + 1, ujeta[j]
        u4, u4s = gi(ug * d4u, 0.5, 1.0)
        uke, ukes = gi(ug * ug, 0.5, 1.0)
        ukd, ukds = gi(ug * ugdot, 0.5, 1.0)
        vg = rdx * (pa[1:, :, k] - pa[:-1, :, k])
        v4, v4s = gi(vg * d4v, 1.0, 0.5)
        vke, vkes = gi(vg * vg, 1.0, 0.5)
        vkd, vkds = gi(d2v, 1.0, 0.5)   # attwk3 = Del-sqd(lagged v): vgdot is never stored (:399-409)
        pint, pints = gi(pa[:, :, k], 0.5, 0.5)
        qint, qints = gi(qa[:, :, k], 0.5, 0.5)
        h = c["hat"][k]
        L["pavgat"][k], S["pavgat"][k] = pint * on, pints * on
        L["qavgat"][k], S["qavgat"][k] = qint * on, qints * on
        L["ah4dat"][k] = rho * c["ah4at"][k] * h * (u4 + v4) * on
        S["ah4dat"][k] = abs(rho * c["ah4at"][k] * h) * (u4s + v4s) * on
        L["kealat"][k], S["kealat"][k] = 0.5 * rho * h * (uke + vke) * on, abs(0.5 * rho * h) * (ukes + vkes) * on
        L["ddtkeat"][k], S["ddtkeat"][k] = rho * h * (ukd + vkd) * on, abs(rho * h) * (ukds + vkds) * on
        L["atstpos"][k], L["atstval"][k] = pos, val
        S["atstpos"][k], S["atstval"][k] = pos, val
    for n in names:
        put(n, L[n].astype(np.int64) if n == "atstpos" else L[n], S[n])

    ast, hmixa = f["ast"], f["hmixa"]
    tml, tmls = gi(ast, 1.0, 1.0)
    hml, hmls = gi(hmixa, 1.0, 1.0)
    put("tmlmat", tml * on, tmls * on)
    put("hmlmat", hml * on, hmls * on)
    put("astmin", ast.min(), abs(ast.min()))
    put("astmax", ast.max(), abs(ast.max()))
    hc, hcs = gi(ast * hmixa, 1.0, 1.0)
    put("hcmlat", rho * c["cpat"] * hc * on, abs(rho * c["cpat"]) * hcs * on)
    i0, j0 = int(c["nx1"]) - 1, int(c["ny1"]) - 1
    blk = ast[i0:i0 + int(c["nxaooc"]), j0:j0 + int(c["nyaooc"])]
    tma = _serial(blk.ravel(order="F")) / float(int(c["nxaooc"]) * int(c["nyaooc"]))
    put("tmaooc", tma, abs(tma))
    olr = c["bup"] * (v["hmlmat"] - c["hmat"]) + c["cup"] * c["davgat"] + c["dup"] * v["tmlmat"]
    olrs = abs(c["bup"]) * (s["hmlmat"] + abs(c["hmat"])) + abs(c["cup"] * c["davgat"]) + abs(c["dup"]) * s["tmlmat"]
    for i in range(nl - 1):
        olr = olr + c["aup"][i] * v["etamat"][i]
        olrs = olrs + abs(c["aup"][i]) * s["etamat"][i]
    put("olrtop", olr, olrs)

    x = _courat_layer(pa[:, :, 0], rdx, cfac, f["uekat"], f["vekat"])
    for n, val in zip(("umminat", "ummaxat", "vmminat", "vmmaxat", "cnmlat"), x):
        put(n, val, abs(val))
    q = np.array([_courat_layer(pa[:, :, k], rdx, cfac) for k in range(nl)])
    for i, n in enumerate(("ugminat", "ugmaxat", "vgminat", "vgmaxat", "cnqgat")):
        put(n, q[:, i], np.abs(q[:, i]))
    return v, s


def valids(f):
    """min, max of pa, qa, ast, wekta, tauxa, tauya (src/valsubs.F:120-180)."""
    out = []
    for n in ("pa", "qa", "ast", "wekta", "tauxa", "tauya"):
        out += [f[n].min(), f[n].max()]
    return np.array(out)


EXT = (1.0e7, 0.05, 90.0, 1.0, 10.0, 10.0)  # patext, qatext, astext, wtaext, tauext (tauxa, tauya)


def solnok(out):
    return all(abs(out[2 * i]) < e and abs(out[2 * i + 1]) < e for i, e in enumerate(EXT))
