"""numpy restatement of the ocean half of monnc_comp and of couroc (src/monitor_diag.F:479-832, poref :173-182,
del4bx :899-1020, del4ch :1026-1151, genint :1155-1209, couroc :1450-1928), written from the Fortran.  The oracle of
qgcm_hip_monitors for the sizes the reference fixtures do not cover.

monitors(f, c) -> (values, scales):
  f: po, pom, qo (nxpo,nypo,nlo), wekpo, entoc, tauxo, tauyo (nxpo,nypo), wekto, sst (nxto,nyto)
  c: cyclic, fnot, dxo, dto, gpoc, hoc, ah2oc, ah4oc, delek, rhooc, cpoc, hmoc, ycexp, sb_hflux, nb_hflux
  values: the MODULE monitor names of qgcm_hip.model.MONITOR_LAYOUT
  scales: for every quantity that is an area integral, the same expression with every integrand and factor replaced
          by its modulus (the scale of its rounding error: wetmoc, utauoc, ddtkeoc ... are near zero by construction);
          for the other quantities their own modulus.
"""
import numpy as np


def genint(val, facwe, facsn):
    """Area integral with weight facwe on the W / E edges and facsn on the S / N edges (:1155-1209)."""
    nx, ny = val.shape
    wx = np.ones(nx)
    wx[0] = wx[-1] = facwe
    wy = np.ones(ny)
    wy[0] = wy[-1] = facsn
    return float(np.einsum("i,ij,j->", wx, val, wy))


def _lap(arr, dxm2, cyc):
    """Del-sqd of del4bx (one-sided differences on all edges) or del4ch (periodic in x) (:925-986, :1053-1098)."""
    nx, ny = arr.shape
    a = arr
    d = np.zeros_like(a)
    if cyc:
        am, ap = np.roll(a, 1, axis=0), np.roll(a, -1, axis=0)
        d[:, 1:-1] = dxm2 * (a[:, :-2] + am[:, 1:-1] + ap[:, 1:-1] + a[:, 2:] - 4.0 * a[:, 1:-1])
        xs = am - 2.0 * a + ap
    else:
        d[1:-1, 1:-1] = dxm2 * (a[1:-1, :-2] + a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, 2:] - 4.0 * a[1:-1, 1:-1])
        xs = np.zeros_like(a)
        xs[1:-1] = a[:-2] - 2.0 * a[1:-1] + a[2:]
        xs[0] = a[2] - 2.0 * a[1] + a[0]
        xs[-1] = a[-1] - 2.0 * a[-2] + a[-3]
        # W / E edges of the interior rows
        for i in (0, nx - 1):
            d[i, 1:-1] = dxm2 * (xs[i, 1:-1] + a[i, :-2] - 2.0 * a[i, 1:-1] + a[i, 2:])
    d[:, 0] = dxm2 * (xs[:, 0] + a[:, 2] - 2.0 * a[:, 1] + a[:, 0])
    d[:, -1] = dxm2 * (xs[:, -1] + a[:, -1] - 2.0 * a[:, -2] + a[:, -3])
    return d


def del4(arr, dxm2, cyc):
    """(Del-sqd, Del-4th) of arr: del4bx / del4ch."""
    d2 = _lap(arr, dxm2, cyc)
    return d2, _lap(d2, dxm2, cyc)


def _couroc_layer(po, cyc, uvg, rh, tx, ty, sb, nb):
    """Velocities on the faces of every T cell (couroc, :1492-1925); returns umin, umax, vmin, vmax, vsqmax.
    rh = 0: a Q-G layer; else the mixed layer with its Ekman part (rhf0hm) and the boundary options sb / nb."""
    nx, ny = po.shape
    nxt, nyt = nx - 1, ny - 1
    uf = -uvg * (po[:, 1:] - po[:, :-1]) + rh * (ty[:, 1:] + ty[:, :-1])        # (nx, nyt): u on the W / E faces
    if not cyc:
        uf[0, :] = 0.0
        uf[-1, :] = 0.0
    vf = uvg * (po[1:, :] - po[:-1, :]) - rh * (tx[1:, :] + tx[:-1, :])         # (nxt, ny): v on the S / N faces
    vs = -rh * (tx[1:, 0] + tx[:-1, 0]) if sb else np.zeros(nxt)
    vn = -rh * (tx[1:, -1] + tx[:-1, -1]) if nb else np.zeros(nxt)
    vf = vf.copy()
    vf[:, 0], vf[:, -1] = vs, vn
    um, up = uf[:-1, :], uf[1:, :]
    vm, vp = vf[:, :-1], vf[:, 1:]
    ucount = uf[1:, :]
    if rh != 0.0:   # the mixed layer's corner rows start the recurrence at i = 2: u(1) of rows 1 and nyto is not scanned
        ucount = np.concatenate([uf[1:, :].ravel(), uf[0, 1:-1]])
    else:
        ucount = uf.ravel()
    vsq = (um + up) ** 2 + (vm + vp) ** 2
    return ucount.min(), ucount.max(), min(vm.min(), vp.min()), max(vm.max(), vp.max()), vsq.max()


def monitors(f, c):
    po, pom, qo = f["po"], f["pom"], f["qo"]
    wekpo, entoc, tauxo, tauyo, wekto, sst = (f[k] for k in ("wekpo", "entoc", "tauxo", "tauyo", "wekto", "sst"))
    nx, ny, nl = po.shape
    nxt, nyt = nx - 1, ny - 1
    cyc = bool(c["cyclic"])
    fnot, dxo, dto = c["fnot"], c["dxo"], c["dto"]
    rhooc, cpoc = c["rhooc"], c["cpoc"]
    gpoc, hoc, ah2oc, ah4oc = (np.asarray(c[k], dtype=np.float64) for k in ("gpoc", "hoc", "ah2oc", "ah4oc"))
    ocnorm = 1.0 / (nxt * nyt)
    rdxof0 = 1.0 / (dxo * fnot)
    dxom2 = 1.0 / (dxo * dxo)
    hdxom1 = 0.5 / dxo
    v, s = {}, {}
    P, U, V, T = (0.5, 0.5), (0.5, 1.0), (1.0, 0.5), (1.0, 1.0)

    def gi(x, g):
        return genint(x, *g), genint(np.abs(x), *g)

    # Ekman velocity and entrainment (:516-552)
    for name, x, g in (("wetmoc", wekto, T), ("wepmoc", wekpo, P), ("entmoc", entoc, P)):
        a, b = gi(x, g)
        v[name], s[name] = a * ocnorm, b * ocnorm
    for name, x, g in (("watmoc", wekto, T), ("wapmoc", wekpo, P), ("enamoc", entoc, P)):
        a, b = gi(np.abs(x), g)
        v[name], s[name] = a * ocnorm, b * ocnorm
    # interface displacements (:556-590)
    for k in ("etamoc", "et2moc", "ddtpeoc"):
        v[k], s[k] = np.zeros(nl - 1), np.zeros(nl - 1)
    for k in range(nl - 1):
        rg = 1.0 / gpoc[k]
        eta = rg * (po[:, :, k + 1] - po[:, :, k])
        etadot = (rg / dto) * (po[:, :, k] - po[:, :, k + 1] - pom[:, :, k] + pom[:, :, k + 1])
        a, b = gi(eta, P)
        v["etamoc"][k], s["etamoc"][k] = a * ocnorm, b * ocnorm
        a, b = gi(eta * eta, P)
        v["et2moc"][k], s["et2moc"][k] = a * ocnorm, b * ocnorm
        a, b = gi(eta * etadot, P)
        v["ddtpeoc"][k], s["ddtpeoc"][k] = rhooc * gpoc[k] * a, abs(rhooc * gpoc[k]) * b
        if k == 0:
            a, b = gi(eta * entoc, P)
            v["pkenoc"], s["pkenoc"] = rhooc * gpoc[0] * a * ocnorm, abs(rhooc * gpoc[0]) * b * ocnorm
    # KE exchange with the wind (:596-615)
    ug1 = -rdxof0 * (po[:, 1:, 0] - po[:, :-1, 0])
    vg1 = rdxof0 * (po[1:, :, 0] - po[:-1, :, 0])
    a1, b1 = gi(ug1 * 0.5 * (tauxo[:, 1:] + tauxo[:, :-1]), U)
    a2, b2 = gi(vg1 * 0.5 * (tauyo[1:, :] + tauyo[:-1, :]), V)
    v["utauoc"], s["utauoc"] = rhooc * (a2 + a1) * ocnorm, abs(rhooc) * (b2 + b1) * ocnorm
    # layers (:619-751)
    names = ("pavgoc", "qavgoc", "ah2doc", "ah4doc", "kealoc", "ddtkeoc", "osfmin", "osfmax", "occirc", "ocjpos", "ocjval")
    for n in names:
        v[n], s[n] = np.zeros(nl), np.zeros(nl)
    for n in ("ugminoc", "ugmaxoc", "vgminoc", "vgmaxoc", "cnqgoc"):
        v[n] = np.zeros(nl)
    if fnot > 0.0:
        poref = po[0, 0, :].copy()
    elif fnot < 0.0:
        poref = po[0, -1, :].copy()
    else:
        poref = np.zeros(nl)
    for k in range(nl):
        ugoc = -rdxof0 * (pom[:, 1:, k] - pom[:, :-1, k])
        vgoc = rdxof0 * (pom[1:, :, k] - pom[:-1, :, k])
        u2, u4 = del4(ugoc, dxom2, cyc)
        v2, v4 = del4(vgoc, dxom2, cyc)
        ugeos = -rdxof0 * (po[:, 1:, k] - po[:, :-1, k])
        ugdot = -(rdxof0 / dto) * (po[:, 1:, k] - pom[:, :-1, k] - pom[:, 1:, k] + pom[:, :-1, k])  # (sic, :679-680)
        vgeos = rdxof0 * (po[1:, :, k] - po[:-1, :, k])
        vgdot = (rdxof0 / dto) * (po[1:, :, k] - po[:-1, :, k] - pom[1:, :, k] + pom[:-1, :, k])
        ujeto = np.abs(np.cumsum(ugeos, axis=0)[-1, :] - ugeos[-1, :]) / nxt   # serial over i, then - u(nxpo) (:671-688)
        pos, val = 0, 0.0
        for j in range(nyt):
            if ujeto[j] > val:
                pos, val = j + 1, ujeto[j]
        v["ocjpos"][k], v["ocjval"][k] = pos, val
        s["ocjpos"][k], s["ocjval"][k] = pos, val
        I = {n: gi(x, g) for n, x, g in (("u2", ugeos * u2, U), ("u4", ugeos * u4, U), ("uke", ugeos * ugeos, U),
                                         ("ukd", ugeos * ugdot, U), ("v2", vgeos * v2, V), ("v4", vgeos * v4, V),
                                         ("vke", vgeos * vgeos, V), ("vkd", vgeos * vgdot, V),
                                         ("p", po[:, :, k], P), ("q", qo[:, :, k], P))}

        def put(name, fac, *terms):
            v[name][k] = fac * sum(I[t][0] for t in terms) * ocnorm
            s[name][k] = abs(fac) * sum(I[t][1] for t in terms) * ocnorm
        put("pavgoc", 1.0, "p")
        put("qavgoc", 1.0, "q")
        put("ah2doc", -rhooc * ah2oc[k] * hoc[k], "u2", "v2")
        put("ah4doc", rhooc * ah4oc[k] * hoc[k], "u4", "v4")
        put("kealoc", 0.5 * rhooc * hoc[k], "uke", "vke")
        put("ddtkeoc", rhooc * hoc[k], "ukd", "vkd")
        pomin, pomax = po[:, :, k].min(), po[:, :, k].max()
        v["osfmin"][k] = 1.0e-6 * hoc[k] * (min(pomin / fnot, pomax / fnot) - poref[k] / fnot)
        v["osfmax"][k] = 1.0e-6 * hoc[k] * (max(pomin / fnot, pomax / fnot) - poref[k] / fnot)
        v["occirc"][k] = 1.0e-6 * hoc[k] * (po[0, 0, k] - po[0, -1, k]) / fnot
        for n in ("osfmin", "osfmax", "occirc"):
            s[n][k] = abs(v[n][k])
        umin, umax, vmin, vmax, vsq = _couroc_layer(po[:, :, k], cyc, rdxof0, 0.0, tauxo, tauyo, False, False)
        v["ugminoc"][k], v["ugmaxoc"][k], v["vgminoc"][k], v["vgmaxoc"][k] = umin, umax, vmin, vmax
        v["cnqgoc"][k] = hdxom1 * dto * np.sqrt(vsq)
    # bottom drag (:757-780)
    ub = -rdxof0 * (pom[:, 1:, -1] - pom[:, :-1, -1])
    vb = rdxof0 * (pom[1:, :, -1] - pom[:-1, :, -1])
    a1, b1 = gi(ub * ub, U)
    a2, b2 = gi(vb * vb, V)
    fac = 0.5 * rhooc * c["delek"] * abs(fnot)
    v["btdgoc"], s["btdgoc"] = fac * (a1 + a2) * ocnorm, abs(fac) * (b1 + b2) * ocnorm
    # mixed layer temperature (:786-807)
    v["sstmin"], v["sstmax"] = float(sst.min()), float(sst.max())
    a, b = gi(sst * wekto, T)
    v["hfmloc"], s["hfmloc"] = rhooc * cpoc * a * ocnorm, abs(rhooc * cpoc) * b * ocnorm
    a, b = gi(sst, T)
    v["tmlmoc"], s["tmlmoc"] = a * ocnorm, b * ocnorm
    v["occtot"] = float(v["occirc"].sum())
    s["occtot"] = float(np.abs(v["occirc"]).sum())
    # couroc's mixed layer (:1492-1744)
    uvg = c["ycexp"] * rdxof0
    rh = 0.5 / (fnot * c["hmoc"])
    umin, umax, vmin, vmax, vsq = _couroc_layer(po[:, :, 0], cyc, uvg, rh, tauxo, tauyo, c["sb_hflux"], c["nb_hflux"])
    v["umminoc"], v["ummaxoc"], v["vmminoc"], v["vmmaxoc"] = umin, umax, vmin, vmax
    v["cnmloc"] = hdxom1 * dto * np.sqrt(vsq)
    for n in v:
        if n not in s:
            s[n] = np.abs(v[n])
    return v, s
