"""TEST INFRASTRUCTURE: numpy stand-ins for what SlabOcean's coupled calls drive on a GPU, so that the
orchestration - xforc_setup / xforc_heat_setup / xforc / coupled_steps - runs on CPU with virtual ranks:

  CoupledSlabMixin   the heat half of xforc on a slab, restated from tests/numpy_heat.py: fnetoc pointwise on every local T
                     row, the partial cell sums over the OWNED rows in the device's order (k_xforc_slab.h: a wave of 64
                     lanes strides over the cell's ndxr^2 points in point order, then the xor butterfly), the message
                     (4, ncell), the rank-ordered combine and the pointwise tail.  The momentum half's ocean side is
                     pointwise in the replicated fine stress (rows of the whole-domain result by construction): the GPU tests
                     hold it; here xforc_part only records that it ran.
  NumpyCoupledSlab   the mixin on numpy_slab.NumpySlab: a box slab that really steps
  RowSlab            the mixin on a bare row view, for fixtures NumpySlab does not step (channels): its stages only record
  NumpyAtmos         a replica of the atmosphere: the lagged mixed-layer state, aml restated (numpy_heat.aml) per step

Every object appends (name, rank) to a shared `log`, which pins the order of calls."""
import numpy as np
import torch

import numpy_heat as nh
from numpy_slab import NumpySlab
from qgcm_hip.slab import local_rows


def butterfly(v):
    """The xor butterfly of a 64-lane wave (offsets 32 .. 1): every lane ends with the same sum; lane 0's is returned."""
    v = np.array(v, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ off]
    return v[0]


def cell_partial(term, rows):
    """The device's sum of one cell's terms (ndxr, ndxr; [ii, jj]) over the T rows jj with rows[jj]: lane = point % 64 in
    point order p = jj * ndxr + ii, each lane adding its points in turn from +0.0, then the butterfly."""
    n = term.shape[0]
    lanes = np.zeros(64)
    for p in range(n * n):
        ii, jj = p % n, p // n
        if rows[jj]:
            lanes[p % 64] = lanes[p % 64] + term[ii, jj]
    return butterfly(lanes)


class CoupledSlabMixin:
    log = None  # shared list, set by the test

    def _note(self, what):
        if self.log is not None:
            self.log.append((what, self.rank))

    def own_t(self):
        """Owned T rows, 0-based global, half-open: T row j lies between p rows j and j+1; the rank that owns row nypo
        stops one short."""
        return self.g0 - 1, min(self.g1, self.cfg.nypo - 1)

    def xforc_init(self, atm, p):
        self.xp = dict(ndxr=p.ndxr, nx1=p.nx1, ny1=p.ny1, nxaooc=p.nxaooc, nyaooc=p.nyaooc, tau_udiff=p.tau_udiff)
        if p.tau_udiff:
            raise ValueError("tau_udiff is not available with a y-slab ocean")
        if self.cfg.nyto != p.nyaooc * p.ndxr or self.cfg.nxto != p.nxaooc * p.ndxr:
            raise ValueError("mismatched geometry")
        self._note("xforc_init")

    def xforc_heat_init(self, atm, p, arrays=None):
        fsa, fso, xta, yta, xto, yto = arrays
        self.fsa, self.fso = np.array(fsa), np.array(fso)
        dxa = self.cfg.ndxr * self.cfg.dxo
        self.T = nh.bilint_tables(np.array(xta), np.array(yta), np.array(xto), np.array(yto), dxa, dxa)
        self.hp = {k: getattr(p, k) for k in ("xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup",
                                                "C1down", "hmadmp", "hmat")}
        self._note("xforc_heat_init")

    def xforc_msg_len(self, atm):
        return 4 * self.xp["nxaooc"] * self.xp["nyaooc"] if hasattr(self, "hp") else 0

    def oml_set_sstm(self, sstm):
        """The lagged sst on the local T rows, from the GLOBAL field."""
        self.sstm = np.array(sstm[:, self.joff:self.joff + self.nyl - 1])

    def xforc_part(self, atm, send):
        self._note("xforc_part")
        if not hasattr(self, "hp"):
            return
        X, H, n = self.xp, self.hp, self.xp["ndxr"]
        tr = slice(self.joff, self.joff + self.nyl - 1)  # the local T rows, global 0-based
        T = dict(self.T, jam=self.T["jam"][tr], jap=self.T["jap"][tr], wmy=self.T["wmy"][tr], wpy=self.T["wpy"][tr])
        asto = nh.bilint(T, atm.S["astm"])
        sst = self.sstm
        ocnrad, slhf, atmrad = H["D0up"] * sst, H["xlamda"] * (sst - asto), H["Dmdown"] * asto
        self.fnetoc = -self.fso[None, tr] - atmrad - ocnrad - slhf
        dxa = n * self.cfg.dxo
        ocfrac = self.cfg.dxo * self.cfg.dxo / (dxa * dxa)
        terms = [ocfrac * (ocnrad + (H["Dmdown"] - H["Dmup"]) * asto + slhf), atmrad, slhf, ocnrad]
        t0, t1 = self.own_t()
        ncx, ncy = X["nxaooc"], X["nyaooc"]
        msg = np.zeros((4, ncy, ncx))
        for cb in range(ncy):
            gj = np.arange(cb * n, (cb + 1) * n)
            rows = (gj >= t0) & (gj < t1)
            if not rows.any():
                continue
            lj = np.clip(gj - self.joff, 0, self.nyl - 2)  # (rows outside the slab are masked out by `rows`)
            for ca in range(ncx):
                for q in range(4):
                    msg[q, cb, ca] = cell_partial(terms[q][ca * n:(ca + 1) * n, :][:, lj], rows)
        send.copy_(torch.from_numpy(msg.ravel()))

    def xforc_combine(self, atm, gath):
        self._note("xforc_combine")
        X = self.xp
        ncell = X["nxaooc"] * X["nyaooc"]
        g = gath.numpy().reshape(self.nranks, 4, ncell)
        tot = g[0].copy()
        for r in range(1, self.nranks):  # rank order, from the first rank's value (k_xf_heat_combine)
            tot = tot + g[r]
        atm.heat_tail(tot.reshape(4, X["nyaooc"], X["nxaooc"]), X, self.hp, self.fsa, self.cfg)

    def xforc_fetch(self, atm, heat):
        return dict(fnetoc=self.fnetoc, fnetat=atm.fnetat, **atm.scal)


class NumpyCoupledSlab(CoupledSlabMixin, NumpySlab):
    def stage(self, n, a=None, b=None, c=None, flags=0):
        if n == 1:
            self._note("ocean_step")
        return NumpySlab.stage(self, n, a, b, c, flags)


class RowSlab(CoupledSlabMixin):
    """The row view of a slab and nothing else: its stages record and move no data."""

    def __init__(self, cfg, g0, g1, rank, nranks):
        self.cfg, self.g0, self.g1, self.rank, self.nranks = cfg, g0, g1, rank, nranks
        self.nyl, self.joff, self.jlo, self.jhi = local_rows(cfg.nypo, g0, g1)
        self.th_len = self.halo_len = self.cst_len = 1

    def new_buffer(self, n):
        return torch.zeros(int(n), dtype=torch.float64)

    def sync(self):
        pass

    def thomas_consts(self, dst):
        pass

    def set_thomas_consts(self, gath):
        pass

    def stage(self, n, a=None, b=None, c=None, flags=0):
        if n == 1:
            self._note("ocean_step")


class NumpyAtmos:
    """One replica: cfg, the mixed-layer state S (ast, astm, hmixa, hmixam), the held pressures; steps() = aml per step."""

    def __init__(self, cfg, g, P, rank, log=None):
        self.cfg, self.g, self.P, self.rank, self.log = cfg, g, P, rank, log
        self.S = {k: np.array(g["in_" + k]) for k in ("ast", "astm", "hmixa", "hmixam")}
        self.fnetat, self.scal, self.entat = None, {}, None
        self.step_index = 1

    def sync(self):
        pass

    def heat_tail(self, tot, X, H, fsa, ocfg):
        """fnetat and the monitors from the combined sums (k_xf_heat_atm, k_xf_heat_final): the land value or the cell's
        sum, then the pointwise tail of numpy_heat.heat."""
        g, P = self.g, self.P
        astm, hmixam, pam, dtop = self.S["astm"], self.S["hmixam"], g["in_pam"], g["in_dtopat"]
        f = -fsa[None, :] - H["Dmup"] * astm
        io = slice(X["nx1"] - 1, X["nx1"] - 1 + X["nxaooc"])
        jo = slice(X["ny1"] - 1, X["ny1"] - 1 + X["nyaooc"])
        f[io, jo] = tot[0].T
        fmafac = H["Adown11"] * 0.25 / P["gpat1"]
        fmatop = 0.25 * (H["Cmup"] + H["C1down"])
        hmafac = -H["hmadmp"] - H["Bmup"] - H["B1down"]
        self.fnetat = (f - fmafac * (pam[:-1, :-1, 0] - pam[:-1, :-1, 1] + pam[1:, :-1, 0] - pam[1:, :-1, 1]
                                     + pam[:-1, 1:, 0] - pam[:-1, 1:, 1] + pam[1:, 1:, 0] - pam[1:, 1:, 1])
                       - fmatop * (dtop[:-1, :-1] + dtop[1:, :-1] + dtop[:-1, 1:] + dtop[1:, 1:])
                       + hmafac * (hmixam - H["hmat"]))
        ocnorm = 1.0 / (ocfg.nxto * ocfg.nyto)
        sums = [float(np.sum(tot[q])) for q in (1, 2, 3)]  # (the device: a fixed tree; any order is within the bound)
        self.scal = dict(arocav=sums[0] * ocnorm, slhfav=sums[1] * ocnorm, oradav=sums[2] * ocnorm)

    def steps(self, n, s0=None):
        g, P = self.g, self.P
        for _ in range(int(n)):
            if self.log is not None:
                self.log.append(("atmos_step", self.rank))
            A = nh.aml(self.S, self.fnetat, g["x0_wekta"], g["x0_uekat"], g["x0_vekat"], g["in_pa"], g["in_pam"],
                       g["in_xc1ast"], g["in_dtopat"], P)
            self.S = {k: A[k] for k in ("ast", "astm", "hmixa", "hmixam")}
            self.entat = A["entat"]
