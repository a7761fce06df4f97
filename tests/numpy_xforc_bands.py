"""TEST INFRASTRUCTURE: the banded slab xforc restated in numpy.

  needed_rows     the fine p rows and fine T rows one rank's kernels touch, listed one index expression at a time from
                  k_xforc_rows.inc / k_xforc.h / k_xforc_slab.h - the brute-force side of tests/test_xforc_bands_cpu.py
  BandRowSlab     numpy_slab_coupled.RowSlab with the banded calls: the momentum block of the message (header, six fields
                  of nrow rows) packed from the band's rows of the replica and scattered from every rank's message
  BandAtmos       numpy_slab_coupled.NumpyAtmos with the six coarse fields and the four line sums of the momentum half

The momentum half itself is not restated (the GPU tests hold it): a replica's `truth` is a fixed synthetic field per
name; a banded rank writes only its band's rows (and the vekat row past it) into its replica, NaN elsewhere, so that
the scatter is what completes a replica."""
import numpy as np
import torch

from numpy_slab_coupled import NumpyAtmos, RowSlab

FIELDS = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa")
LINES = ("txisat", "txinat", "txisoc", "txinoc")
HDR = 8


def needed_rows(nyta, ndxr, ny1, nyg, band, slab, own):
    """(set of fine p rows, set of fine T rows), 1-based, that the kernels of a rank read or write for: its band's rows of
    the six fields, its slab's rows lo..hi of tauxo / tauyo, and the line sums named in `own`."""
    n, nypa, nytaor = ndxr, nyta + 1, nyta * ndxr
    nypaor, odd, nijwid = nytaor + 1, ndxr % 2, ndxr + ndxr % 2
    a0, a1 = band
    P, T = set(), set()
    for ja in range(a0, a1 + 1):
        P.add(1 + (ja - 1) * n)                      # tauxa, tauya: txf / tyf at row joff; vekat: txf along row joff
        if ja <= nyta:
            P.update(1 + (ja - 1) * n + j for j in range(n + 1))  # uekat: tyf at rows joff .. joff + ndxr
            P.add(1 + ja * n)                        # wekta(ja) reads vekat(ja + 1): row joff of ja + 1
        jbeg = (ja - 1) * n - (n - 1) // 2           # wekpa: fine T rows jbeg .. jbeg + nijwid - 1, clipped
        for j in range(max(jbeg, 1), min(jbeg + nijwid - 1, nytaor) + 1):
            T.add(j)
            P.update((j, j + 1))                     # wektaor(j) reads p rows j, j + 1
    jocoff = (ny1 - 1) * n
    P.update(jocoff + g for g in range(slab[0], slab[1] + 1))  # k_xf_tauo: fine row jocoff + joff + j
    jsou, jnor = 1 + n // 2, nypaor - n // 2
    if "txisat" in own:
        P.update((jsou, jsou + 1) if odd else (jsou,))
    if "txinat" in own:
        P.update((jnor, jnor - 1) if odd else (jnor,))
    if "txisoc" in own:
        P.update((jocoff + 1, jocoff + 2))
    if "txinoc" in own:
        P.update((jocoff + nyg - 1, jocoff + nyg))
    return P, T


def truth(name, cfg):
    """The synthetic whole-domain value of a coarse field, (nx, ny) with the field's own shape."""
    shp = dict(tauxa=(cfg.nxpa, cfg.nypa), tauya=(cfg.nxpa, cfg.nypa), uekat=(cfg.nxpa, cfg.nyta), vekat=(cfg.nxta, cfg.nypa),
               wekta=(cfg.nxta, cfg.nyta), wekpa=(cfg.nxpa, cfg.nypa))[name]
    i, j = np.meshgrid(np.arange(shp[0]), np.arange(shp[1]), indexing="ij")
    return np.sin(0.37 * i + 1.0 + FIELDS.index(name)) * np.cos(0.11 * j) + 1e-3 * j


LINE_TRUTH = dict(txisat=1.25, txinat=-2.5, txisoc=3.75, txinoc=-4.125)


class BandAtmos(NumpyAtmos):
    def __init__(self, *a, **k):
        NumpyAtmos.__init__(self, *a, **k)
        self.mom = {f: np.full_like(truth(f, self.cfg), np.nan) for f in FIELDS}
        self.lines = {f: np.nan for f in LINES}


class BandRowSlab(RowSlab):
    bands = None

    def xforc_bands_init(self, atm, band, nrow):
        self.bands = dict(band=(int(band[0]), int(band[1])), nrow=int(nrow))
        self._note("xforc_bands_init")

    def _mom_len(self, atm):
        return HDR + len(FIELDS) * self.bands["nrow"] * atm.cfg.nxpa

    def xforc_msg_len(self, atm):
        heat = RowSlab.xforc_msg_len(self, atm)
        return heat + (self._mom_len(atm) if self.bands else 0)

    def _own(self, atm):
        a0, a1 = self.bands["band"]
        own = [a0 == 1, a1 == atm.cfg.nypa, self.cfg.cyclic and self.joff == 0,
               self.cfg.cyclic and self.joff + self.nyl == self.cfg.nypo]
        return [f for f, o in zip(LINES, own) if o]

    def xforc_part(self, atm, send):
        if not self.bands:
            return RowSlab.xforc_part(self, atm, send)
        (a0, a1), nrow, nxpa = self.bands["band"], self.bands["nrow"], atm.cfg.nxpa
        for f in FIELDS:  # the band's rows, and the row past it where the windowed k_xf_atm writes it
            t = truth(f, atm.cfg)
            hi = min(a1 + (1 if f in ("tauxa", "tauya", "vekat") else 0), t.shape[1])
            atm.mom[f][:, a0 - 1:hi] = t[:, a0 - 1:hi]
        own = self._own(atm)
        for f in own:
            atm.lines[f] = LINE_TRUTH[f]
        m = np.zeros(self._mom_len(atm))
        m[0], m[1], m[2] = a0, a1, sum(1 << LINES.index(f) for f in own)
        for f in own:
            m[4 + LINES.index(f)] = atm.lines[f]
        blk = m[HDR:].reshape(len(FIELDS), nrow, nxpa)
        for k, f in enumerate(FIELDS):
            a = atm.mom[f]
            rows = max(0, min(a1, a.shape[1]) - a0 + 1)
            blk[k, :rows, :a.shape[0]] = a[:, a0 - 1:a0 - 1 + rows].T
        send[:m.size].copy_(torch.from_numpy(m))
        if hasattr(self, "hp"):
            RowSlab.xforc_part(self, atm, send[m.size:])
        else:
            self._note("xforc_part")

    def xforc_combine(self, atm, gath):
        if not self.bands:
            return RowSlab.xforc_combine(self, atm, gath)
        nrow, nxpa, ml = self.bands["nrow"], atm.cfg.nxpa, self._mom_len(atm)
        g = gath.numpy().reshape(self.nranks, -1)
        for r in range(self.nranks):
            a0, a1, own = int(g[r, 0]), int(g[r, 1]), int(g[r, 2])
            blk = g[r, HDR:ml].reshape(len(FIELDS), nrow, nxpa)
            for k, f in enumerate(FIELDS):
                a = atm.mom[f]
                rows = max(0, min(a1, a.shape[1]) - a0 + 1)
                a[:, a0 - 1:a0 - 1 + rows] = blk[k, :rows, :a.shape[0]].T
            for k, f in enumerate(LINES):
                if own >> k & 1:
                    atm.lines[f] = g[r, 4 + k]
        if hasattr(self, "hp"):
            RowSlab.xforc_combine(self, atm, torch.from_numpy(np.ascontiguousarray(g[:, ml:]).ravel()))
        else:
            self._note("xforc_combine")
