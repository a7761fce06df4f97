"""numpy restatement of covaria_diag.F (psampl, tsampl, dssp with wt = 1) and of its row-sum form.

Every sum is formed in the reference's operand order, so the results are bitwise the reference's (and the device's).
Fields are (nx, ny) arrays indexed [i, j] as the reference's datap(i, j); sample vectors are ordered as its
ivs = (js-1)*(nx/nsi) + is; the packed matrix index is k = i(i+1)/2 + j (0-based, j <= i).
"""
import math

import numpy as np


def psampl(p, nsi):
    """psampl (src/covaria_diag.F:431-488) as written: inner rows, then the S and N boundary rows of each block."""
    nx, ny = p.shape
    nbx, nby = nx // nsi, ny // nsi
    i1 = (np.arange(nbx) * nsi)[:, None]  # 0-based id1
    j1 = (np.arange(nby) * nsi)[None, :]  # 0-based jd1

    def rowsum(jd):
        s = 0.5 * p[i1, jd]
        for o in range(1, nsi):
            s = s + p[i1 + o, jd]
        return s + 0.5 * p[i1 + nsi, jd]

    sumd = np.zeros((nbx, nby))
    for o in range(1, nsi):
        sumd = sumd + rowsum(j1 + o)
    sums, sumn = rowsum(j1), rowsum(j1 + nsi)
    return (sumd + 0.5 * (sums + sumn)).ravel(order="F")


def tsampl(t, nsi):
    """tsampl (src/covaria_diag.F:359-423), nsi > 1."""
    nx, ny = t.shape
    nbx, nby = nx // nsi, ny // nsi
    i1 = (np.arange(nbx) * nsi)[:, None]
    j1 = (np.arange(nby) * nsi)[None, :]
    sumd = np.zeros((nbx, nby))
    for q in range(nsi):
        sumi = np.zeros((nbx, nby))
        for o in range(nsi):
            sumi = sumi + t[i1 + o, j1 + q]
        sumd = sumd + sumi
    return sumd.ravel(order="F")


# -- row-sum form (k_cov_rowsums / k_cov_combine) ---------------------------------------------------------------------
def p_rowsums(p, nsi, rows):
    """r(is, j) of the p grid for the given 0-based rows: (nbx, len(rows))."""
    nbx = (p.shape[0] - 1) // nsi
    i1 = (np.arange(nbx) * nsi)[:, None]
    rows = np.asarray(rows)[None, :]
    s = 0.5 * p[i1, rows]
    for o in range(1, nsi):
        s = s + p[i1 + o, rows]
    return s + 0.5 * p[i1 + nsi, rows]


def t_rowsums(t, nsi, rows):
    nbx = t.shape[0] // nsi
    i1 = (np.arange(nbx) * nsi)[:, None]
    rows = np.asarray(rows)[None, :]
    s = np.zeros((nbx, rows.shape[1]))
    for o in range(nsi):
        s = s + t[i1 + o, rows]
    return s


def part(p, t, nsi, jp0, jp1, jt0, jt1, part_len=None):
    """One rank's part (1-based global rows jp0..jp1 of p, jt0..jt1 of T): the header and the row sums, as
    qgcm_hip_cov_part writes it."""
    rp = p_rowsums(p, nsi, np.arange(jp0 - 1, jp1))
    rt = t_rowsums(t, nsi, np.arange(jt0 - 1, jt1))
    v = np.concatenate([[jp0, jp1, jt0, jt1], rp.ravel(order="F"), rt.ravel(order="F")]).astype(np.float64)
    if part_len is not None:
        v = np.concatenate([v, np.zeros(part_len - len(v))])
    return v


def combine(parts, nsi, nbx, nyp, nyt):
    """k_cov_combine's sample vectors (u_p, u_t) from the parts in rank order; raises when they do not tile the rows."""
    rp, rt, np_, nt = {}, {}, 0, 0
    for k, v in enumerate(parts):
        p0, p1, t0, t1 = (int(x) for x in v[:4])
        if p0 != np_ + 1 or p1 < p0 or t0 != nt + 1 or t1 < t0 - 1:
            raise ValueError("rank %d does not continue the rows" % k)
        a = v[4:4 + (p1 - p0 + 1) * nbx].reshape(nbx, -1, order="F")
        b = v[4 + (p1 - p0 + 1) * nbx:4 + (p1 - p0 + 1 + t1 - t0 + 1) * nbx].reshape(nbx, -1, order="F")
        for j in range(p0, p1 + 1):
            rp[j] = a[:, j - p0]
        for j in range(t0, t1 + 1):
            rt[j] = b[:, j - t0]
        np_, nt = p1, t1
    if np_ != nyp or nt != nyt:
        raise ValueError("the parts end at rows %d, %d" % (np_, nt))
    nby = nyt // nsi
    up, ut = np.zeros((nbx, nby)), np.zeros((nbx, nby))
    for js in range(nby):
        jd1 = 1 + js * nsi
        sumd = np.zeros(nbx)
        for jd in range(jd1 + 1, jd1 + nsi):
            sumd = sumd + rp[jd]
        up[:, js] = sumd + 0.5 * (rp[jd1] + rp[jd1 + nsi])
        sumd = np.zeros(nbx)
        for jd in range(jd1, jd1 + nsi):
            sumd = sumd + rt[jd]
        ut[:, js] = sumd
    return up.ravel(order="F"), ut.ravel(order="F")


# -- dssp (Algorithm AS 41, src/covaria_diag.F:496-595) with wt = 1 ---------------------------------------------------
class Dssp:
    def __init__(self, nvar, k0=0, k1=None):
        self.nvar = nvar
        self.nmat = nvar * (nvar + 1) // 2
        self.k0, self.k1 = k0, self.nmat if k1 is None else k1
        self.mean = np.zeros(nvar)
        self.cov = np.zeros(self.k1 - self.k0)
        self.nu, self.swt = 0, 0.0

    def add(self, x):
        wt = 1.0
        self.nu += 1
        self.swt = self.swt + wt
        b = wt / self.swt
        if self.nu == 1:
            self.mean = np.array(x, dtype=np.float64)
            self.cov[:] = 0.0
            return
        c = wt - b * wt
        d = x - self.mean
        self.mean = self.mean + b * d
        i0, _ = rowcol(self.k0)
        for i in range(i0, self.nvar):
            k = i * (i + 1) // 2
            if k >= self.k1:
                break
            a, e = max(k, self.k0), min(k + i + 1, self.k1)
            seg = slice(a - self.k0, e - self.k0)
            self.cov[seg] = self.cov[seg] + (c * d[i]) * d[a - k:e - k]


def rowcol(k):
    """Row i and column j of packed entry k, as k_cov.h's cov_rowcol: the triangular root in double, then an exact
    integer correction."""
    r = int((math.sqrt(8.0 * float(k) + 1.0) - 1.0) * 0.5)
    while r > 0 and r * (r + 1) // 2 > k:
        r -= 1
    while (r + 1) * (r + 2) // 2 <= k:
        r += 1
    return r, k - r * (r + 1) // 2


def covocn(p1, t, nsi, acc_p, acc_t):
    """One covocn / covatm: psampl of layer 1 of p, tsampl of the T field, dssp on each."""
    acc_p.add(psampl(p1, nsi))
    acc_t.add(tsampl(t, nsi))
