"""The plan of the library-driven coupled window (qgcm_hip_slab_coupled_plan) against the order the Python
driver issues: SlabOcean.coupled_steps runs on virtual ranks of recording stand-ins - the row views of
tests/numpy_slab_coupled.py with every call logged and no data moved - and lib.slab_coupled_plan must name the same
operations, with the same message lengths, in the same order, on every rank.  No GPU: the plan is host code."""
import numpy as np
import pytest

from numpy_slab_coupled import NumpyAtmos, RowSlab
from qgcm_hip import lib
from qgcm_hip.slab import SlabOcean, partition
from test_slab_coupled_cpu import CountingComm, _configs, _heat_cfg

CASE = "heat_cpl_tiny"  # ocean 49 x 37: three ranks own 13, 12 and 12 rows
MODES = ("replicated", "bands", "udiff_gather", "udiff_sums")
NT0, N = 73, 30  # ten ocean steps at nstr = 3: steps 25 .. 34, across the averaging after step 26
OML_LEN, SUMMARY_LEN, HALO_LEN = 3, 11, 5  # (the stand-ins' lengths: distinct, so that a swapped exchange shows)


class RecordingComm(CountingComm):
    def halo_exchange(self, to_lo, to_hi, from_lo, from_hi):
        ref = next(t for t in list(to_lo) + list(to_hi) if t is not None)
        self.log.append(("halo_exchange", ref.numel()))
        CountingComm.halo_exchange(self, to_lo, to_hi, from_lo, from_hi)


class RecordingSlab(RowSlab):
    """A row view whose every call of the window is logged as (name, rank); the lengths are what the real calls would
    report, up to their values."""

    def __init__(self, cfg, g0, g1, rank, nranks, oml):
        RowSlab.__init__(self, cfg, g0, g1, rank, nranks)
        self.th_len, self.halo_len = SUMMARY_LEN, HALO_LEN
        self.oml_on, self.oml_len = oml, OML_LEN
        self.heat, self.mom_len, self.pom_len, self.edge_len = False, 0, 0, 0

    # set-up: remembered, not logged
    def xforc_init(self, atm, p):
        self.ncell = p.nxaooc * p.nyaooc
        self.heat, self.mom_len, self.pom_len, self.edge_len = False, 0, 0, 0

    def xforc_heat_init(self, atm, p, arrays=None):
        self.heat = True

    def xforc_bands_init(self, atm, band, nrow):
        self.mom_len = lib.XFORC_BAND_HEADER + len(lib.XFORC_BAND_FIELDS) * nrow * atm.cfg.nxpa

    def xforc_udiff_init(self, atm, nrow, nranks):
        self.pom_len = lib.XFORC_POM_HEADER + nrow * self.cfg.nxpo

    def xforc_sums_init(self, atm, rows):
        self.mom_len = lib.XFORC_SUM_HEADER + len(lib.XFORC_SUM_FIELDS) * 7 * atm.cfg.nxpa
        self.edge_len = lib.XFORC_EDGE_HEADER + 2 * lib.XFORC_EDGE_ROWS * self.cfg.nxpo

    def xforc_msg_len(self, atm):
        return self.mom_len + (4 * self.ncell if self.heat else 0)

    def xforc_pom_len(self, atm):
        return self.pom_len

    def xforc_edge_len(self, atm):
        return self.edge_len

    # the window's calls
    def stage(self, n, a=None, b=None, c=None, flags=0):
        self._note({10: "oml_a", 11: "oml_b", 1: "stage1", 2: "stage2", 3: "stage3_avg" if flags & 1 else "stage3"}[n])


for _name in ("xforc_edge_pack", "xforc_edge_assemble", "xforc_pom_pack", "xforc_pom_assemble", "xforc_part", "xforc_combine"):
    setattr(RecordingSlab, _name, (lambda nm: lambda self, atm, buf: self._note(nm))(_name))


class RecordingAtmos(NumpyAtmos):
    def steps(self, n, s0=None):
        for _ in range(int(n)):
            self.log.append(("atm_step", self.rank))


def _setup(nranks, mode, heat, oml):
    g, P, oc, at = _configs(CASE)
    log = []
    slabs = [RecordingSlab(oc, g0, g1, r, nranks, oml) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.log = log
    so = SlabOcean(oc, slabs, RecordingComm(nranks, log))
    reps = [RecordingAtmos(at, g, P, r, log) for r in range(nranks)]
    tabs = {k: np.zeros((16, P["ndxr"] + 1, P["ndxr"] + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}
    so.xforc_setup(reps, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tables=tabs,
                   nx1=P["nx1"], ny1=P["ny1"], **({} if mode == "replicated" else {mode: True}))
    if heat:
        so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], fsa=g["t_fsa"], fso=g["t_fso"],
                            coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    del log[:]
    return so, reps, log


def _plan(x, a, nranks, nstr, xforc, mode, heat, oml, halo_p2p=True, nt0=NT0, n=N):
    """The plan from what rank x's own calls report."""
    return lib.slab_coupled_plan(nranks, nt0, n, nstr, xforc, oml=oml, heat=heat, bands=mode == "bands",
                                 udiff_gather=mode == "udiff_gather", udiff_sums=mode == "udiff_sums", halo_p2p=halo_p2p,
                                 xforc_len=x.xforc_msg_len(a), pom_len=x.xforc_pom_len(a), edge_len=x.xforc_edge_len(a),
                                 oml_len=x.oml_len, summary_len=x.th_len, halo_len=x.halo_len)


def _as_issued(plan):
    """A plan in the vocabulary of the log: an all-gather and a halo exchange by their lengths, a call by its name."""
    out = []
    for name, ln in plan:
        if name.startswith("gather_"):
            out.append(("all_gather", ln))
        elif name == "halo_p2p":
            out.append(("halo_exchange", ln))
        else:
            assert ln == 0, (name, ln)
            out.append((name,))
    return out


def _issued(log, rank):
    """What rank `rank` took part in: its own calls and every exchange (the virtual ranks interleave in the log)."""
    return [e if e[0] in ("all_gather", "halo_exchange") else (e[0],) for e in log
            if e[0] in ("all_gather", "halo_exchange") or e[1] == rank]


COLLECTIVES = ("gather_edge", "gather_pom", "gather_xforc", "gather_oml", "gather_summary", "halo_gather", "halo_p2p")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_plan_is_the_python_drivers_order(nranks, mode):
    """The window nt0 = 73, n = 30 with the heat half and the ocean mixed layer on and off, xforc = 0 and 1, nstr = 3 and
    nstr = 1 (no ocean step): on every rank the plan is, entry by entry, what SlabOcean.coupled_steps issued there; and
    all ranks' plans hold the same collectives with the same lengths in the same order (no rank waits in one collective
    while another has entered a different one: what one GPU cannot show by running)."""
    for heat in (False, True):
        for oml in (False, True):
            so, reps, log = _setup(nranks, mode, heat, oml)
            for xforc in (False, True):
                for nstr in (3, 1):
                    del log[:]
                    so.coupled_steps(NT0, N, nstr, xforc=xforc)
                    tag = (nranks, mode, heat, oml, xforc, nstr)
                    plans = [_plan(x, a, nranks, nstr, xforc, mode, heat, oml) for x, a in zip(so.slabs, reps)]
                    for x, plan in zip(so.slabs, plans):
                        assert _as_issued(plan) == _issued(log, x.rank), (tag, x.rank)
                    coll = [[e for e in p if e[0] in COLLECTIVES] for p in plans]
                    assert all(c == coll[0] for c in coll), tag
                    names = [e[0] for e in plans[0]]
                    assert names.count("atm_step") == N, tag
                    assert names.count("stage1") == (10 if nstr == 3 else 0), tag
                    assert names.count("stage3_avg") == (1 if nstr == 3 else 0), tag  # ocean step 26
                    assert ("gather_summary", SUMMARY_LEN) in plans[0] or nstr == 1, tag
                    assert (names.count("xforc_part") > 0) == (xforc and nstr == 3), tag


def test_plan_by_hand():
    """Two short windows written out: replicated with the heat half and the mixed layer on two ranks from nt = 1 (the
    ocean's first step ends with the averaging), and udiff_sums on one rank from the middle of an ocean step's span."""
    xf = [("xforc_part", 0), ("gather_xforc", 40), ("xforc_combine", 0)]
    oc = [("oml_a", 0), ("gather_oml", 3), ("oml_b", 0), ("stage1", 0), ("gather_summary", 7), ("stage2", 0), ("halo_p2p", 5)]
    at = [("atm_step", 0)]
    kw = dict(oml=True, heat=True, xforc_len=40, oml_len=3, summary_len=7, halo_len=5)
    got = lib.slab_coupled_plan(2, 1, 5, 3, True, **kw)
    assert got == xf + oc + [("stage3_avg", 0)] + at * 3 + xf + oc + [("stage3", 0)] + at * 2
    # the halo rows as one all-gather: both edge messages
    gat = lib.slab_coupled_plan(2, 1, 5, 3, True, halo_p2p=False, **kw)
    assert gat == [("halo_gather", 10) if e == ("halo_p2p", 5) else e for e in got] and gat != got
    # held forcing: the same window without xforc's entries
    assert lib.slab_coupled_plan(2, 1, 5, 3, False, **kw) == [e for e in got if e not in xf]
    # one rank: no halo exchange, stage 3 only where the step ends with the averaging (ocean step 26 = nt 76)
    edge = [("xforc_edge_pack", 0), ("gather_edge", 9), ("xforc_edge_assemble", 0)]
    step = [("stage1", 0), ("gather_summary", 7), ("stage2", 0)]
    got = lib.slab_coupled_plan(1, 72, 6, 3, True, udiff_sums=True, xforc_len=50, edge_len=9, summary_len=7)
    xs = edge + [("xforc_part", 0), ("gather_xforc", 50), ("xforc_combine", 0)]
    assert got == at + xs + step + at * 3 + xs + step + [("stage3_avg", 0)] + at * 2
    # the shear term's gather in front, the momentum half alone exchanges nothing else
    got = lib.slab_coupled_plan(1, 4, 1, 3, True, udiff_gather=True, pom_len=21, summary_len=7)
    assert got == [("xforc_pom_pack", 0), ("gather_pom", 21), ("xforc_pom_assemble", 0), ("xforc_part", 0)] + step + at
    assert lib.slab_coupled_plan(3, 5, 0, 3, True, summary_len=7, halo_len=5) == []


def test_plan_refusals():
    """A bad step range, no ranks, a message of the chosen mode without a length, modes that exclude each other."""
    ok = dict(summary_len=7, halo_len=5)
    for args, kw, msg in [((2, 0, 5, 3, True), ok, "bad step range"), ((2, 1, -1, 3, True), ok, "bad step range"),
                          ((2, 1, 5, 0, True), ok, "bad step range"), ((0, 1, 5, 3, True), ok, "nranks = 0"),
                          ((2, 1, 5, 3, True), dict(ok, heat=True), "xforc_len = 0"),
                          ((2, 1, 5, 3, True), dict(ok, udiff_gather=True), "pom_len = 0"),
                          ((2, 1, 5, 3, True), dict(ok, udiff_sums=True, xforc_len=9), "edge_len = 0"),
                          ((2, 1, 5, 3, False), dict(ok, oml=True), "oml_len = 0"),
                          ((2, 1, 5, 3, False), dict(halo_len=5), "summary_len = 0"),
                          ((2, 1, 5, 3, False), dict(summary_len=7), "halo_len = 0"),
                          ((2, 1, 5, 3, True), dict(ok, udiff_sums=True, bands=True, xforc_len=9, edge_len=9), "udiff_sums excludes")]:
        with pytest.raises(lib.QgcmHipError, match="qgcm_hip_slab_coupled_plan: .*" + msg):
            lib.slab_coupled_plan(*args, **kw)
    # held forcing needs none of xforc's lengths
    assert lib.slab_coupled_plan(1, 1, 1, 3, False, heat=True, udiff_gather=True, summary_len=7)
