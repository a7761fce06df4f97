"""TEST INFRASTRUCTURE: the owner-computed sums of the slab xforc restated in numpy.

  owner_rows      who owns which fine p row / fine T row, from the ranks' owned ocean rows alone
  reads           the fine p rows, fine T rows and coarse rows one rank's kernels touch, listed one index expression at a
                  time from k_xforc_rows.inc / k_xforc_slab.h - the brute-force side of tests/test_xforc_sums_cpu.py
  fine            txf, tyf (the fine stress) and wf (wektaor) of a fixture's state: numpy_xforc.xforc up to its drag law
  part / combine  k_xf_sums_atm + k_xf_sums_wekpa and k_xf_sums_combine: the message's five fields, the rank-ordered sums
  bounds          per entry: is the uekat line / wekpa box cut, and the bounds of DESIGN 6r for the cut ones
  edge_pack / edge_assemble   the two copy kernels
  SumsRowSlab     numpy_slab_udiff.UdiffRowSlab with the calls of this mode, on a synthetic fine stress

Arrays are indexed [i-1, j-1]."""
import inspect

import numpy as np
import torch

import numpy_xforc as nx
from numpy_slab_udiff import UdiffRowSlab

HDR = 8     # lib.XFORC_SUM_HEADER, lib.XFORC_EDGE_HEADER
EDGE = 4    # lib.XFORC_EDGE_ROWS
FIELDS = ("tauxa", "tauya", "vekat", "uekat", "wekpa")
LINES = ("txisat", "txinat", "txisoc", "txinoc")

# (fixture, ranks): the cases of tests/test_gpu_xforc_sums.py
BOX = [("xf_cpl_tiny_ud", 1), ("xf_cpl_tiny_ud", 2), ("xf_cpl_tiny_ud", 3), ("xf_cpl_small_ud", 5), ("xf_odd5_ud", 3)]
WIDE = [("xf_cyc4_ud", 2), ("xf_cyc4_ud", 3), ("xf_cycwide_ud", 2), ("xf_cycwide_ud", 3), ("xf_wide_ud", 2), ("xf_edge_ud", 2)]
CASES = BOX + WIDE


def dims(nyta, ndxr, ny1, nyaooc):
    n = ndxr
    return dict(n=n, nyta=nyta, nypa=nyta + 1, nytaor=nyta * n, nypaor=nyta * n + 1, odd=n % 2, nijwid=n + n % 2,
                nyg=nyaooc * n + 1, jocoff=(ny1 - 1) * n, jsou=1 + n // 2, jnor=nyta * n + 1 - n // 2)


def owner_rows(D, rows):
    """(P, T): P[f] / T[j] = the rank that owns fine p row f / fine T row j (1-based; entry 0 unused).  The fine row above
    ocean row g belongs to g's owner, the land south of the sea to rank 0, the land north of it to the last rank; T row
    j to the owner of p row j."""
    P = np.zeros(D["nypaor"] + 1, dtype=int)
    for f in range(1, D["nypaor"] + 1):
        g = f - D["jocoff"]
        if g < 1:
            P[f] = 0
        elif g > D["nyg"]:
            P[f] = len(rows) - 1
        else:
            P[f] = [r for r, (g0, g1) in enumerate(rows) if g0 <= g <= g1][0]
    return P, P[:D["nytaor"] + 1]


def box_rows(D, ja):
    """The fine T rows of wekpa's box at coarse row ja (k_xf_wekpa: jlo .. jhi) and jbeg."""
    jbeg = (ja - 1) * D["n"] - (D["n"] - 1) // 2
    return max(jbeg, 1), min(jbeg + D["nijwid"] - 1, D["nytaor"]), jbeg


def reads(D, rows, r, cyclic=True):
    """What rank r's kernels touch: dict(P = fine p rows whose stress is read, T = fine T rows of wektaor read or written,
    A = coarse rows the rank contributes anything to, own = the line sums it forms)."""
    n, nyg, jocoff = D["n"], D["nyg"], D["jocoff"]
    Pown, Town = owner_rows(D, rows)
    g0, g1 = rows[r]
    P, T, A, own = set(), set(), set(), []
    for j in range(1, D["nytaor"] + 1):      # k_xf_wektaor_win on the owned T rows: p rows j, j + 1
        if Town[j] == r:
            T.add(j)
            P.update((j, j + 1))
    for g in range(max(1, g0 - 3), min(nyg, g1 + 3) + 1):  # k_xf_tauo on the slab's local rows (three halo rows)
        P.add(jocoff + g)
    if g0 == 1:                              # k_xf_lines_oc_slab
        own.append("txisoc")
        if cyclic:
            P.update((jocoff + 1, jocoff + 2))
    if g1 == nyg:
        own.append("txinoc")
        if cyclic:
            P.update((jocoff + nyg - 1, jocoff + nyg))
    if Pown[D["jsou"]] == r:                 # k_xf_lines_win
        own.append("txisat")
        P.update((D["jsou"], D["jsou"] + 1) if D["odd"] else (D["jsou"],))
    if Pown[D["jnor"]] == r:
        own.append("txinat")
        P.update((D["jnor"], D["jnor"] - 1) if D["odd"] else (D["jnor"],))
    for ja in range(1, D["nypa"] + 1):
        joff = 1 + (ja - 1) * n
        if Pown[joff] == r:                  # k_xf_sums_atm: tauxa, tauya, vekat from row joff
            P.add(joff)
            A.add(ja)
        if ja <= D["nyta"]:                  # ... and the terms of uekat's line in the owned rows
            mine = [joff + k for k in range(n + 1) if Pown[joff + k] == r]
            P.update(mine)
            if mine:
                A.add(ja)
        jlo, jhi, jbeg = box_rows(D, ja)     # k_xf_sums_wekpa: the box's rows in the owned T rows
        mine = [j for j in range(jlo, jhi + 1) if Town[j] == r]
        T.update(mine)
        if mine:
            A.add(ja)
    return dict(P=P, T=T, A=A, own=sorted(own))


# numpy_xforc.xforc up to and including its drag law: the same text, so the same bits (the fixtures pin it to the
# reference); what follows `R = {}` there is replaced by the return of the fine stress.
_src = inspect.getsource(nx.xforc)
assert _src.count("    R = {}\n") == 1
_ns = dict(np=np)
exec(_src.split("    R = {}\n")[0].replace("def xforc(", "def _fine_stress(") + "    return txf, tyf, hxofac, uvekfc\n", _ns)
_fine = {}


def wektaor(txf, tyf, hxofac):
    """k_xf_wektaor's expression on every fine T point."""
    return hxofac * (tyf[1:, :-1] + tyf[1:, 1:] - (tyf[:-1, :-1] + tyf[:-1, 1:]) + txf[:-1, :-1] + txf[1:, :-1]
                     - (txf[:-1, 1:] + txf[1:, 1:]))


def fine(case, s):
    """(txf, tyf, wf, uvekfc) of state s of a fixture (computed once, shared)."""
    if (case, s) not in _fine:
        g = nx.load(case)
        txf, tyf, hxofac, uvekfc = _ns["_fine_stress"](g["in%d_pam1" % s], g["in%d_pom1" % s], nx.tables(g), nx.params(g))
        _fine[(case, s)] = (txf, tyf, wektaor(txf, tyf, hxofac), uvekfc)
    return _fine[(case, s)]


def _wt(D):
    wt = np.ones(D["n"] + 1)
    if D["odd"]:
        wt[0] = wt[D["n"]] = 0.5
    else:
        wt[D["n"]] = 0.0
    return wt


def part(D, nxta, txf, tyf, wf, uvekfc, f0, f1, a0, a1, nrow):
    """The five fields (5, nrow, nxpa) of rank's message: k_xf_sums_atm's and k_xf_sums_wekpa's expressions and order on the
    owned fine p rows f0 .. f1 and the owned fine T rows f0 .. min(f1, nytaor)."""
    n, nxpa, nxtaor = D["n"], nxta + 1, nxta * D["n"]
    t1 = min(f1, D["nytaor"])
    M = np.zeros((5, nrow, nxpa))
    io = np.arange(nxpa) * n
    ic = np.where(np.arange(nxpa) == nxta, 0, np.arange(nxpa)) * n  # uekat(nxpa, ja) = uekat(1, ja)
    wt = _wt(D)
    ibeg = np.arange(nxpa) * n - (n - 1) // 2
    for jr in range(nrow):
        ja = a0 + jr
        if ja > a1 or ja > D["nypa"]:
            continue
        joff = 1 + (ja - 1) * n
        if f0 <= joff <= f1:
            M[0, jr] = txf[io, joff - 1]
            M[1, jr] = tyf[io, joff - 1]
            t = txf[:, joff - 1]
            s = 0.5 * t[io[:nxta]]
            for i in range(1, n):
                s = s + t[io[:nxta] + i]
            s = s + 0.5 * t[io[:nxta] + n]
            M[2, jr, :nxta] = uvekfc * s
        if ja <= D["nyta"]:
            k0, k1 = max(0, f0 - joff), min(n, f1 - joff)
            s = None
            for k in range(k0, k1 + 1):
                v = tyf[ic, joff - 1 + k]
                v = 0.5 * v if k in (0, n) else v
                s = v if s is None else s + v
            if s is not None:
                M[3, jr] = s
        jlo, jhi, jbeg = box_rows(D, ja)
        acc = np.zeros(nxpa)
        for j in range(max(jlo, f0), min(jhi, t1) + 1):
            wtj = wt[j - jbeg]
            for d in range(D["nijwid"]):
                it = (ibeg + d - 1 + nxtaor) % nxtaor
                acc = acc + wt[d] * wtj * wf[it, j - 1]
        M[4, jr] = acc
    return M


def combine(D, nxta, uvekfc, msgs):
    """k_xf_sums_combine on a list of (f0, f1, a0, fields (5, nrow, nxpa)) in rank order: dict of tauxa, tauya, vekat,
    uekat, wekpa, NaN where no rank wrote."""
    n, nxpa = D["n"], nxta + 1
    R = dict(tauxa=np.full((nxpa, D["nypa"]), np.nan), tauya=np.full((nxpa, D["nypa"]), np.nan),
             vekat=np.full((nxta, D["nypa"]), np.nan), uekat=np.full((nxpa, D["nyta"]), np.nan),
             wekpa=np.full((nxpa, D["nypa"]), np.nan))
    wt = _wt(D)
    for ja in range(1, D["nypa"] + 1):
        joff = 1 + (ja - 1) * n
        jlo, jhi, jbeg = box_rows(D, ja)
        us = wp = None
        for f0, f1, a0, M in msgs:
            jr = ja - a0
            if jr < 0 or jr >= M.shape[1]:
                continue
            if f0 <= joff <= f1:
                R["tauxa"][:, ja - 1], R["tauya"][:, ja - 1], R["vekat"][:, ja - 1] = M[0, jr], M[1, jr], M[2, jr, :nxta]
            if ja <= D["nyta"] and joff <= f1 and joff + n >= f0:
                us = M[3, jr] if us is None else us + M[3, jr]
            if jlo <= min(f1, D["nytaor"]) and jhi >= f0:
                wp = M[4, jr] if wp is None else wp + M[4, jr]
        if us is not None:
            R["uekat"][:, ja - 1] = -uvekfc * us
        if wp is not None:
            wsum = 0.0
            for j in range(jlo, jhi + 1):
                for d in range(D["nijwid"]):
                    wsum = wsum + wt[d] * wt[j - jbeg]
            R["wekpa"][:, ja - 1] = wp / wsum
    return R


def bounds(D, nxta, txf, tyf, wf, uvekfc, hmrdxa, Pown):
    """Per entry of uekat (nxpa, nyta), wekpa (nxpa, nypa) and wekta (nxta, nyta): `cut` (more than one rank owns terms of
    it) and the bound of DESIGN 6r on |slabs - whole domain|:

      uekat   2 (ndxr + 1) 2^-53 uvekfc sum |w_k tyf_k|          (a sum of ndxr + 1 terms in another order)
      wekpa   2 N 2^-53 sum |w wf| / wsum, N the terms of the clipped box
      wekta = -hmrdxa (ue[i+1] - ue[i] + ve[j+1] - ve[j]): vekat is bitwise, so in exact arithmetic the two results differ
              by hmrdxa (d[i+1] - d[i]) with |d| <= the uekat bounds, B = B[i+1] + B[i] in all.  Each result carries the
              rounding of the expression's three additions and one product, each at most 2^-53 (1 + 3 2^-53) of a partial
              result no larger than S = |ue[i+1]| + |ue[i]| + |ve[j+1]| + |ve[j]| + B (the whole-domain operands; + B covers
              the slabs'): 4 roundings in each of the two results, 8 in all, taken as 9 to cover the second-order terms:
              hmrdxa B + 9 2^-53 hmrdxa S.  It is cut where either uekat it reads is."""
    n, nxpa, nxtaor = D["n"], nxta + 1, nxta * D["n"]
    eps = 2.0 ** -53
    ic = np.where(np.arange(nxpa) == nxta, 0, np.arange(nxpa)) * n
    wt = _wt(D)
    ibeg = np.arange(nxpa) * n - (n - 1) // 2
    ucut, ub = np.zeros((nxpa, D["nyta"]), bool), np.zeros((nxpa, D["nyta"]))
    for ja in range(1, D["nyta"] + 1):
        joff = 1 + (ja - 1) * n
        ucut[:, ja - 1] = len({Pown[joff + k] for k in range(n + 1)}) > 1
        a = np.zeros(nxpa)
        for k in range(n + 1):
            a = a + (0.5 if k in (0, n) else 1.0) * np.abs(tyf[ic, joff - 1 + k])
        ub[:, ja - 1] = 2.0 * (n + 1) * eps * uvekfc * a
    pcut, pb = np.zeros((nxpa, D["nypa"]), bool), np.zeros((nxpa, D["nypa"]))
    for ja in range(1, D["nypa"] + 1):
        jlo, jhi, jbeg = box_rows(D, ja)
        pcut[:, ja - 1] = len({Pown[j] for j in range(jlo, jhi + 1)}) > 1
        a, wsum, N = np.zeros(nxpa), 0.0, 0
        for j in range(jlo, jhi + 1):
            for d in range(D["nijwid"]):
                it = (ibeg + d - 1 + nxtaor) % nxtaor
                a = a + wt[d] * wt[j - jbeg] * np.abs(wf[it, j - 1])
                wsum += wt[d] * wt[j - jbeg]
                N += 1
        pb[:, ja - 1] = 2.0 * N * eps * a / wsum
    R = nx_coarse(D, nxta, txf, tyf, uvekfc)
    ue, ve = R["uekat"], R["vekat"]
    B = ub[1:] + ub[:-1]
    S = np.abs(ue[1:]) + np.abs(ue[:-1]) + np.abs(ve[:, 1:]) + np.abs(ve[:, :-1]) + B
    tb = hmrdxa * B + 9.0 * eps * hmrdxa * S
    tcut = ucut[1:] | ucut[:-1]
    return dict(uekat=(ucut, ub), wekpa=(pcut, pb), wekta=(tcut, np.where(tcut, tb, 0.0)))


def nx_coarse(D, nxta, txf, tyf, uvekfc):
    """uekat and vekat by the sequential loops of the reference (numpy_xforc.xforc's, from the fine stress)."""
    n, nxpa = D["n"], nxta + 1
    io = np.arange(nxta) * n
    jo = np.arange(D["nypa"]) * n
    ts = 0.5 * txf[io][:, jo]
    for i in range(1, n):
        ts = ts + txf[io + i][:, jo]
    ts = ts + 0.5 * txf[io + n][:, jo]
    vekat = uvekfc * ts
    jo = np.arange(D["nyta"]) * n
    ts = 0.5 * tyf[io][:, jo]
    for j in range(1, n):
        ts = ts + tyf[io][:, jo + j]
    ts = ts + 0.5 * tyf[io][:, jo + n]
    uekat = np.zeros((nxpa, D["nyta"]))
    uekat[:nxta] = -uvekfc * ts
    uekat[nxta] = uekat[0]
    return dict(uekat=uekat, vekat=vekat)


def wekpa_seq(D, nxta, wf):
    """wekpa by the sequential loops of the reference (numpy_xforc.xforc's, from wektaor)."""
    n, nxpa, nxtaor = D["n"], nxta + 1, nxta * D["n"]
    wt = _wt(D)
    ibeg = np.arange(nxpa) * n - (n - 1) // 2
    out = np.zeros((nxpa, D["nypa"]))
    for ja in range(1, D["nypa"] + 1):
        jlo, jhi, jbeg = box_rows(D, ja)
        wsum, wtasum = np.zeros(nxpa), np.zeros(nxpa)
        for j in range(jlo, jhi + 1):
            for d in range(D["nijwid"]):
                it = (ibeg + d - 1 + nxtaor) % nxtaor
                wsum = wsum + wt[d] * wt[j - jbeg]
                wtasum = wtasum + wt[d] * wt[j - jbeg] * wf[it, j - 1]
        out[:, ja - 1] = wtasum / wsum
    return out


# ---- the edge rows ---------------------------------------------------------------------------------------------------
def edge_pack(pom_local, g0, g1, jlo):
    """k_xf_edge_pack: pom_local (nxpo, nyl) holds the slab's local rows, the owned ones from local row jlo (1-based)."""
    nxpo = pom_local.shape[0]
    m = np.zeros(HDR + 2 * EDGE * nxpo)
    m[0], m[1], m[2] = g0, g1, nxpo
    own = pom_local[:, jlo - 1:jlo + g1 - g0]
    body = m[HDR:].reshape(2 * EDGE, nxpo)
    body[:EDGE] = own[:, :EDGE].T
    body[EDGE:] = own[:, -EDGE:].T
    return m


def edge_assemble(gath, rank, nranks, pom_local, g0, g1, jlo, nypo):
    """k_xf_edge_assemble: (array (nxpo, nypo) from NaN, times written per row)."""
    nxpo = pom_local.shape[0]
    out, written = np.full((nxpo, nypo), np.nan), np.zeros(nypo, dtype=int)
    out[:, g0 - 1:g1] = pom_local[:, jlo - 1:jlo + g1 - g0]
    written[g0 - 1:g1] += 1
    g = np.asarray(gath).reshape(nranks, HDR + 2 * EDGE * nxpo)
    for r, south in ((rank - 1, True), (rank + 1, False)):
        if r < 0 or r >= nranks:
            continue
        h0, h1, nxm = (int(v) if np.isfinite(v) else 0 for v in g[r, :3])
        if h0 < 1 or h1 > nypo or h1 - h0 + 1 < EDGE or nxm != nxpo or (h1 != g0 - 1 if south else h0 != g1 + 1):
            continue
        body = g[r, HDR:].reshape(2 * EDGE, nxpo)
        if south:
            out[:, g0 - 1 - EDGE:g0 - 1] = body[EDGE:].T
            written[g0 - 1 - EDGE:g0 - 1] += 1
        else:
            out[:, g1:g1 + EDGE] = body[:EDGE].T
            written[g1:g1 + EDGE] += 1
    return out, written


# ---- the stand-in -------------------------------------------------------------------------------------------------------
def synthetic(cfg_at, ndxr):
    """A fixed synthetic fine stress (txf, tyf, wf, uvekfc) on the atmosphere's fine grid."""
    nxf, nyf = cfg_at.nxta * ndxr + 1, cfg_at.nyta * ndxr + 1
    i, j = np.meshgrid(np.arange(nxf), np.arange(nyf), indexing="ij")
    txf = np.sin(0.37 * i + 0.5) * np.cos(0.11 * j) + 1e-3 * j
    tyf = np.cos(0.23 * i) * np.sin(0.19 * j + 0.3) - 1e-3 * i
    txf[-1], tyf[-1] = txf[0], tyf[0]
    return txf, tyf, wektaor(txf, tyf, 0.5), 0.125


class SumsRowSlab(UdiffRowSlab):
    """The calls of the mode on a row view: the edge copies restated, the part and the combine on the synthetic fine stress
    (NaN outside the rank's window, so a read of a row the plan does not compute shows), the heat block behind."""
    sm = None

    def xforc_init(self, atm, p):
        UdiffRowSlab.xforc_init(self, atm, p)
        self.sm = None

    def xforc_sums_init(self, atm, rows):
        from qgcm_hip import lib
        X = self.xp
        if self.bands or self.ud:
            raise ValueError("the modes exclude each other")
        self.D = dims(atm.cfg.nyta, X["ndxr"], X["ny1"], X["nyaooc"])
        plan = lib.xforc_sums(atm.cfg.nxpa, atm.cfg.nyta, X["ndxr"], X["ny1"], X["nyaooc"], rows)
        assert plan[self.rank]["rows"] == (self.g0, self.g1)
        self.sm = dict(plan=plan[self.rank], fresh=False, nranks=len(rows))
        self._note("xforc_sums_init")

    def xforc_edge_len(self, atm):
        return HDR + 2 * EDGE * self.cfg.nxpo

    def xforc_edge_pack(self, atm, send):
        self._note("edge_pack")
        send.copy_(torch.from_numpy(edge_pack(self.pom, self.g0, self.g1, self.jlo)))

    def xforc_edge_assemble(self, atm, gath):
        self._note("edge_assemble")
        self.assembled, self.written = edge_assemble(gath.numpy(), self.rank, self.sm["nranks"], self.pom, self.g0, self.g1,
                                                     self.jlo, self.cfg.nypo)
        self.sm["fresh"] = True

    def _mom_len(self, atm):
        if self.sm:
            return HDR + len(FIELDS) * self.sm["plan"]["nrow"] * atm.cfg.nxpa
        return UdiffRowSlab._mom_len(self, atm)

    def xforc_msg_len(self, atm):
        if not self.sm:
            return UdiffRowSlab.xforc_msg_len(self, atm)
        return self._mom_len(atm) + (4 * self.xp["nxaooc"] * self.xp["nyaooc"] if hasattr(self, "hp") else 0)

    def xforc_part(self, atm, send):
        if not self.sm:
            return UdiffRowSlab.xforc_part(self, atm, send)
        if not self.sm["fresh"]:
            raise ValueError("the edge rows have not been assembled for this call")
        self.sm["fresh"] = False
        p, D = self.sm["plan"], self.D
        txf, tyf, wf, uvekfc = synthetic(atm.cfg, D["n"])
        (w0, w1), (t0, t1) = p["window"], p["trows"]
        for a in (txf, tyf):  # what the rank does not compute
            a[:, :w0 - 1] = np.nan
            a[:, w1:] = np.nan
        wf[:, :t0 - 1] = np.nan
        wf[:, t1:] = np.nan
        M = part(D, atm.cfg.nxta, txf, tyf, wf, uvekfc, p["fine"][0], p["fine"][1], p["arows"][0], p["arows"][1], p["nrow"])
        m = np.zeros(self._mom_len(atm))
        m[0], m[1], m[2] = p["fine"][0], p["fine"][1], p["arows"][0]
        m[3] = sum(1 << LINES.index(f) for f in p["own"])
        for f in p["own"]:
            m[4 + LINES.index(f)] = 1.0 + LINES.index(f)
        m[HDR:] = M.ravel()
        send[:m.size].copy_(torch.from_numpy(m))
        if hasattr(self, "hp"):
            UdiffRowSlab.xforc_part(self, atm, send[m.size:])
        else:
            self._note("xforc_part")

    def xforc_combine(self, atm, gath):
        if not self.sm:
            return UdiffRowSlab.xforc_combine(self, atm, gath)
        ml, nrow, nxpa = self._mom_len(atm), self.sm["plan"]["nrow"], atm.cfg.nxpa
        g = gath.numpy().reshape(self.nranks, -1)
        msgs = [(int(g[r, 0]), int(g[r, 1]), int(g[r, 2]), g[r, HDR:ml].reshape(5, nrow, nxpa)) for r in range(self.nranks)]
        atm.sums = combine(self.D, atm.cfg.nxta, 0.125, msgs)
        atm.sum_lines = {}
        for r in range(self.nranks):
            for k, f in enumerate(LINES):
                if int(g[r, 3]) >> k & 1:
                    assert f not in atm.sum_lines
                    atm.sum_lines[f] = g[r, 4 + k]
        if hasattr(self, "hp"):
            UdiffRowSlab.xforc_combine(self, atm, torch.from_numpy(np.ascontiguousarray(g[:, ml:]).ravel()))
        else:
            self._note("xforc_combine")
