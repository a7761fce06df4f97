"""TEST INFRASTRUCTURE: numpy stand-ins for the gather of the surface pressure ahead of the slab xforc, so that
SlabOcean's choreography with udiff_gather = True runs on CPU with virtual ranks:

  pom_pack / pom_assemble   the two copy kernels of k_xforc_slab.h restated: the message (8 + nrow * nxpo doubles: g0, g1,
                            nxpo, zeros, then the OWNED rows, +0.0 past them) and the assembled array (nxpo, nypo)
  UdiffRowSlab              numpy_xforc_bands.BandRowSlab (a row view: banded or not, with or without the heat half) with
                            the four calls of the shear term and the part's refusal; its halo rows of pom hold NaN, so
                            a packed halo row would show

CASES are the grids and rank counts the GPU tests cut with slab.partition; CUTS are cuts by hand (CPU only).  The
fixtures are the whole-domain path's tau_udiff fixtures (tests/numpy_xforc.py)."""
import numpy as np
import torch

import numpy_xforc as nx
from numpy_xforc_bands import BandRowSlab
from qgcm_hip.slab import HALO

HDR = 8  # lib.XFORC_POM_HEADER

# (fixture, ranks): the cases of tests/test_gpu_slab_udiff.py
BOX = [("xf_cpl_tiny_ud", 1), ("xf_cpl_tiny_ud", 2), ("xf_cpl_tiny_ud", 3), ("xf_cpl_small_ud", 5), ("xf_odd5_ud", 3)]
WIDE = [("xf_cyc4_ud", 2), ("xf_cyc4_ud", 3), ("xf_cycwide_ud", 2), ("xf_cycwide_ud", 3), ("xf_wide_ud", 2), ("xf_edge_ud", 2)]
CASES = BOX + WIDE
# cuts by hand: a seam between ocean rows 1 | 2 and nypo - 1 | nypo (the one-sided zbfcoc rows beside their neighbours;
# the first and the last rank own one row each)
CUTS = [("xf_cyc4_ud", lambda nypo: [(1, 1), (2, nypo - 1), (nypo, nypo)]),
        ("xf_cpl_tiny_ud", lambda nypo: [(1, 1), (2, 20), (21, nypo - 1), (nypo, nypo)])]


def configs(case):
    """(fixture, its parameters, ocean configuration, atmosphere configuration) as tests/test_gpu_xforc.py:_models has them."""
    import dataclasses
    from qgcm_hip import config
    g = nx.load(case)
    P = nx.params(g)
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"])
    return g, P, oc, config.atmos_of(oc, bccoat=P["bccoat"])


class BareAtmos:
    """A replica that only names its configuration (the momentum half is not restated on CPU)."""

    def __init__(self, cfg, rank):
        self.cfg, self.rank = cfg, rank

    def sync(self):
        pass


def dims(case):
    """(nxpo, nypo, ndxr) of a fixture."""
    P = nx.params(nx.load(case))
    return P["nxaooc"] * P["ndxr"] + 1, P["nyaooc"] * P["ndxr"] + 1, P["ndxr"]


def pom_pack(pom_local, g0, g1, jlo, nrow):
    """k_xf_pom_pack: pom_local (nxpo, nyl) holds the slab's local rows, the owned ones from local row jlo (1-based)."""
    nxpo = pom_local.shape[0]
    m = np.zeros(HDR + nrow * nxpo)
    m[0], m[1], m[2] = g0, g1, nxpo
    n = g1 - g0 + 1
    m[HDR:].reshape(nrow, nxpo)[:n] = pom_local[:, jlo - 1:jlo - 1 + n].T
    return m


def pom_assemble(gath, nranks, nrow, nxpo, nypo, out=None):
    """k_xf_pom_assemble: rank r's rows -> rows g0(r) .. g1(r) of (nxpo, nypo); starts from NaN (the poisoned array)
    unless `out` is given.  A header that does not describe rows inside 1 .. nypo writes nothing."""
    if out is None:
        out = np.full((nxpo, nypo), np.nan)
    g = np.asarray(gath).reshape(nranks, HDR + nrow * nxpo)
    written = np.zeros(nypo, dtype=int)
    for r in range(nranks):
        g0, g1, nxm = (int(v) if np.isfinite(v) else 0 for v in g[r, :3])  # (the device's conversion gives 0 for a NaN)
        if g0 < 1 or g1 > nypo or g1 < g0 or g1 - g0 + 1 > nrow or nxm != nxpo:
            continue
        out[:, g0 - 1:g1] = g[r, HDR:].reshape(nrow, nxpo)[:g1 - g0 + 1].T
        written[g0 - 1:g1] += 1
    return out, written


def clipped_rows(nyg, g0, g1):
    """slab.local_rows with the halo rows clipped to the basin: (nyl, joff, jlo, jhi).  The same as local_rows wherever a
    slab's neighbours hold its three halo rows; a cut by hand (CUTS) may leave fewer."""
    lo, hi = max(1, g0 - HALO), min(nyg, g1 + HALO)
    return hi - lo + 1, lo - 1, g0 - lo + 1, g1 - lo + 1


class UdiffRowSlab(BandRowSlab):
    ud = None

    def __init__(self, cfg, g0, g1, rank, nranks):
        BandRowSlab.__init__(self, cfg, g0, g1, rank, nranks)
        self.nyl, self.joff, self.jlo, self.jhi = clipped_rows(cfg.nypo, g0, g1)

    def set_pom(self, pom):
        """The slab's local rows of the GLOBAL pom(:,:,1); the halo rows are replaced by NaN (they are never packed)."""
        self.pom = np.array(pom[:, self.joff:self.joff + self.nyl])
        self.pom[:, :self.jlo - 1] = np.nan
        self.pom[:, self.jhi:] = np.nan

    def xforc_init(self, atm, p):
        BandRowSlab.xforc_init(self, atm, p)
        self.ud = None  # (a later set-up returns the pair to the shear-free path)
        self.bands = None

    def xforc_udiff_init(self, atm, nrow, nranks):
        if nrow < self.g1 - self.g0 + 1 or nranks < 1:
            raise ValueError("the common row count does not hold this slab's owned rows")
        self.ud = dict(nrow=int(nrow), nranks=int(nranks), fresh=False)
        self.assembled = None
        self._note("xforc_udiff_init")

    def xforc_pom_len(self, atm):
        return HDR + self.ud["nrow"] * self.cfg.nxpo

    def xforc_pom_pack(self, atm, send):
        self._note("pom_pack")
        send.copy_(torch.from_numpy(pom_pack(self.pom, self.g0, self.g1, self.jlo, self.ud["nrow"])))

    def xforc_pom_assemble(self, atm, gath):
        self._note("pom_assemble")
        self.assembled, self.written = pom_assemble(gath.numpy(), self.ud["nranks"], self.ud["nrow"], self.cfg.nxpo, self.cfg.nypo)
        self.ud["fresh"] = True

    def xforc_part(self, atm, send):
        if self.ud:
            if not self.ud["fresh"]:
                raise ValueError("the surface pressure has not been assembled for this call")
            self.ud["fresh"] = False
        BandRowSlab.xforc_part(self, atm, send)
