"""SlabOcean's coupled calls on CPU: virtual ranks of numpy stand-ins (tests/numpy_slab_coupled.py) run the
choreography of xforc() and coupled_steps() and are held to the whole-domain restatement (tests/numpy_heat.py) and the
reference's own results (tests/golden/heat_cpl_tiny, heat_cpl_small, heat_cyc72).  What this pins without a GPU: the
order of calls, one all-gather per xforc, bit-equal replicas, the ownership of T rows and the summation order of a
cell a seam cuts."""
import dataclasses

import numpy as np
import pytest

import numpy_heat as nh
from numpy_slab_coupled import NumpyAtmos, NumpyCoupledSlab, RowSlab, butterfly, cell_partial
from qgcm_hip import config
from qgcm_hip.slab import LocalComm, SlabOcean, partition

CASES = [("heat_cpl_tiny", 1), ("heat_cpl_tiny", 2), ("heat_cpl_tiny", 3), ("heat_cpl_small", 5), ("heat_cyc72", 2),
         ("heat_cyc72", 3)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    assert np.array_equal(_bits(a), _bits(b)), "%s: max |diff| %.3e" % (what, np.max(np.abs(np.asarray(a) - b)))


class CountingComm(LocalComm):
    def __init__(self, nranks, log):
        LocalComm.__init__(self, nranks)
        self.log = log

    def all_gather(self, gath, send):
        self.log.append(("all_gather", send[0].numel()))
        LocalComm.all_gather(self, gath, send)


def _configs(case):
    g = nh.load(case)
    P = nh.params(g)
    base = config.preset("cyc_tiny" if P["cyclic"] else "cpl_tiny")
    oc = dataclasses.replace(base, name=case, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"], nyaooc=P["nyaooc"],
                             ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    return g, P, oc, config.atmos_of(oc, bccoat=P["bccoat"], gpat=(P["gpat1"], P["gpat2"]))


def _heat_cfg(P):
    return config.HeatConfig(**{k: P[k] for k in ("D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup", "C1down",
                                                  "xlamda", "fspco")})


def _setup(case, nranks, slab=None):
    g, P, oc, at = _configs(case)
    log = []
    make = slab or (lambda g0, g1, r: RowSlab(oc, g0, g1, r, nranks))
    slabs = [make(g0, g1, r) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.log = log
        x.oml_set_sstm(g["in_sstm"])
    so = SlabOcean(oc, slabs, CountingComm(nranks, log))
    reps = [NumpyAtmos(at, g, P, r, log) for r in range(nranks)]
    # a dummy set of weight tables: the momentum half is not restated here (numpy_slab_coupled.py)
    tabs = {k: np.zeros((16, P["ndxr"] + 1, P["ndxr"] + 1), order="F") for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")}
    so.xforc_setup(reps, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tables=tabs,
                   nx1=P["nx1"], ny1=P["ny1"])
    so.xforc_heat_setup(_heat_cfg(P), hmadmp=P["hmadmp"], hmat=P["hmat"], fsa=g["t_fsa"], fso=g["t_fso"],
                        coords={k: g["t_" + k] for k in ("xta", "yta", "xto", "yto")})
    del log[:]
    return g, P, oc, so, reps, log


def test_cell_partial_is_the_device_order():
    """The restated order on a full cell: lane l of the wave adds points l, l + 64, ... in turn, then the butterfly pairs
    lanes at distance 32, 16, ... 1; a cell cut into two row ranges gives partials whose sum is the full sum to rounding
    and exactly when one range is empty."""
    rng = np.random.default_rng(5)
    for n in (4, 12, 16):
        t = rng.standard_normal((n, n)) * 10.0 ** rng.integers(-3, 4, (n, n))
        lanes = np.zeros(64)
        flat = t.ravel(order="F")  # point p = jj * n + ii
        for p, v in enumerate(flat):
            lanes[p % 64] += v
        full = cell_partial(t, np.ones(n, dtype=bool))
        assert full == butterfly(lanes)
        assert cell_partial(t, np.zeros(n, dtype=bool)) == 0.0 and not np.signbit(cell_partial(t, np.zeros(n, dtype=bool)))
        lo = np.arange(n) < n // 3
        a, b = cell_partial(t, lo), cell_partial(t, ~lo)
        assert abs((a + b) - full) <= 2.0 * n * n * 2.0 ** -53 * np.abs(t).sum()
        assert full + 0.0 == full and _bits(0.0 + full) == _bits(full)


@pytest.mark.parametrize("case,nranks", CASES)
def test_xforc_heat_on_virtual_ranks(case, nranks):
    """One xforc(): exactly one all-gather, of 4 * nxaooc * nyaooc doubles per rank, between every rank's part and every
    rank's combine; fnetoc on every local T row bitwise the restatement's and the fixture's rows; fnetat bitwise over
    land; above the ocean within 2 n 2^-53 sum|terms| (n = ndxr^2) plus one ulp of the value of the fixture (the serial
    sum; the tail is added afterwards, tests/test_gpu_heat.py:test_heat_golden); the cells no seam cuts bitwise the
    one-rank run's; the monitors within their bound; all replicas bit-equal; every owned T row belongs to one rank."""
    g, P, oc, so, reps, log = _setup(case, nranks)
    N = nh.restated(case)[("x", 0)]
    so.xforc()
    names = [e[0] for e in log]
    assert names == ["xforc_part"] * nranks + ["all_gather"] + ["xforc_combine"] * nranks, names
    assert log[nranks] == ("all_gather", 4 * P["nxaooc"] * P["nyaooc"])
    H = so.xforc_heat_get()
    owner = np.full(oc.nyto, -1)
    for x in so.slabs:
        t0, t1 = x.own_t()
        assert np.all(owner[t0:t1] == -1)
        owner[t0:t1] = x.rank
    assert np.all(owner >= 0)
    n = P["ndxr"]
    cut = np.array([len(set(owner[cb * n:(cb + 1) * n])) > 1 for cb in range(P["nyaooc"])])
    assert (cut.any() and not cut.all()) if nranks > 1 else not cut.any()
    blk = (slice(P["nx1"] - 1, P["nx1"] - 1 + P["nxaooc"]), slice(P["ny1"] - 1, P["ny1"] - 1 + P["nyaooc"]))
    ref = g["x0_fnetat"]
    bound = 2.0 * n * n * 2.0 ** -53 * N["cell_abs"] + np.spacing(np.abs(ref[blk]))
    if nranks > 1:
        one = _one_rank(case)
    for x, h in zip(so.slabs, H):
        tr = slice(x.joff, x.joff + x.nyl - 1)
        _same(h["fnetoc"], N["fnetoc"][:, tr], "fnetoc")
        _same(h["fnetoc"], g["x0_fnetoc"][:, tr], "fnetoc against the fixture")
        _same(h["fnetat"], H[0]["fnetat"], "replicas")
        _same(h["fnetat"][~N["ocean"]], ref[~N["ocean"]], "fnetat over land")
        assert np.all(np.abs(h["fnetat"][blk] - ref[blk]) <= bound)
        if nranks > 1:
            _same(h["fnetat"][blk][:, ~cut], one["fnetat"][blk][:, ~cut], "cells no seam cuts")
        for f in ("slhfav", "oradav", "arocav"):
            assert abs(h[f] - float(g["x0_" + f])) <= 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f], f
            assert h[f] == H[0][f]


_one = {}


def _one_rank(case):
    if case not in _one:
        g, P, oc, so, reps, log = _setup(case, 1)
        so.xforc()
        _one[case] = so.xforc_heat_get()[0]
    return _one[case]


def test_coupled_steps_order_and_replicas():
    """coupled_steps(1, 7, 3, xforc=True) on three ranks of the channel's row views: per ocean step xforc (parts, ONE
    all-gather of the message, combines), then the ocean step on every slab, then the atmospheric steps on every
    replica - the reference's order (src/q-gcm.F:1220-1268); after the window the replicas are bit-equal and equal to a
    whole-domain (one-rank) run within the chain's bar of tests/test_gpu_heat.py:test_chained, 1e-13.  xforc = False:
    no part, no combine, no message."""
    case, nranks = "heat_cyc72", 3
    g, P, oc, so, reps, log = _setup(case, nranks)
    so.coupled_steps(1, 7, 3, xforc=True)
    msg = 4 * P["nxaooc"] * P["nyaooc"]
    ev = [e[0] for e in log if e[0] != "all_gather" or e[1] == msg]
    cyc = lambda k: (["xforc_part"] * nranks + ["all_gather"] + ["xforc_combine"] * nranks + ["ocean_step"] * nranks
                     + ["atmos_step"] * k * nranks)
    # (the replicas step one after the other: rank 0's k steps, then rank 1's, ...)
    assert ev == cyc(3) + cyc(3) + cyc(1), ev
    assert sum(1 for e in log if e == ("all_gather", msg)) == 3
    for a in reps[1:]:
        for k in a.S:
            _same(a.S[k], reps[0].S[k], "replica " + k)
        _same(a.entat, reps[0].entat, "replica entat")
    g1, P1, oc1, so1, reps1, log1 = _setup(case, 1)
    so1.coupled_steps(1, 7, 3, xforc=True)
    for k in ("ast", "hmixa"):
        e = np.abs(reps[0].S[k] - reps1[0].S[k]).max() / np.abs(reps1[0].S[k]).max()
        assert e < 1e-13, (k, e)
    del log[:]
    so.coupled_steps(8, 6, 3, xforc=False)
    ev = [e[0] for e in log if e[0] != "all_gather" or e[1] == msg]
    assert ev == ["atmos_step"] * 2 * nranks + ["ocean_step"] * nranks + ["atmos_step"] * 3 * nranks + ["ocean_step"] * nranks \
        + ["atmos_step"] * nranks, ev


def test_box_slabs_step_inside_the_window():
    """NumpySlab slabs (a box that really steps) inside coupled_steps: the ocean state after the window is bitwise the
    state after the same number of plain SlabOcean.steps - the window adds calls around the step and changes none."""
    from common import make_oracle
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import global_consts
    case, nranks = "heat_cpl_tiny", 3
    g, P, oc, at = _configs(case)
    o = make_oracle(oc)
    try:
        consts = global_consts(oc, o.helmholtz)
    finally:
        o.close()
    po = synth.gaussian_eddy(oc, noise=1e-2)
    qo = hostinit.q_from_p(oc, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    scal = hostinit.constr(oc, consts["amatoc"], po, po)
    _, wek = synth.wekpo_from_tau(oc, *synth.wind_stress(oc))
    out = []
    for coupled in (True, False):
        gg, PP, occ, so, reps, log = _setup(case, nranks, slab=lambda g0, g1, r: NumpyCoupledSlab(oc, consts, g0, g1, r, nranks))
        so.scatter_state(po, po, qo, qo, wek, np.zeros_like(wek), np.zeros(oc.nlo - 1), scal)
        if coupled:
            so.coupled_steps(1, 6, 3, xforc=True)
        else:
            so.steps(2, s0=1)
        out.append(so.gather_local())
    for (g0, g1, fa), (_, _, fb) in zip(*out):
        for x, y in zip(fa, fb):
            _same(x, y, "rows %d..%d" % (g0, g1))
