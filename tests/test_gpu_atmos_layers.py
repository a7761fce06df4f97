"""The wave-per-row-pair atmosphere at layer counts other than three, against the CPU oracle.  Needs an MI355X.

Every atmosphere fixture of the reference has 17, 33 or 385 x 97 columns, and only 17 x 13 exists with nla != 3
(tests/golden/atm_tiny_a<n>.npz): rows of 16 points take the generic row kernels.  Rows of 192 (m64 = 3) and 384
(m64 = 6, the production family) take k_rfft64.h, whose layer handling differs by count: nla = 2 .. 4 ride the
constraint on the inverse rows (k_rfft64_unpack<NL> with its extra wave, constraint parts A / B), nla = 5 .. 8 run plain
inverse rows + k_constr_cyc + k_unpack_cyc; 8 is the ABI's limit and fills every QG_MAXL-sized array.  No reference
build exists at these shapes.  The yardstick is oracle/qgcm_oracle.c, which tests/test_atmos_oracle.py pins to the
reference at nla = 2, 4, 5 on 17 x 13 (bitwise after qgastep and atqzbd, 1.5e-15 after atinvq, 1.2e-14 after 130
steps); its layer loops carry no shape dependence.  nla = 8 has neither a reference build nor a fixture: there the
oracle's generic layer loops are the only yardstick.

Bars are those of tests/test_gpu_atmos.py: bit equality after qgastep, and of pam, qa, qam after atinvq and of all four
fields after atqzbd from the oracle's state; pa within TOL_CALL after atinvq; TOL_RUN after 130 free-running steps (the
averaging after step 101 included)."""
import numpy as np
import pytest

from common import ATM_FIELDS, atm_apply, atm_load_snapshot, atm_scal_err, atm_state_errs, atm_wide, make_atm_oracle_of
from qgcm_hip import synth

pytestmark = pytest.mark.gpu

TOL_CALL = 1e-12   # as tests/test_gpu_atmos.py
TOL_RUN = 1e-10
SHAPES = (192, 384)
COUNTS = (2, 4, 5, 8)
_refs = {}


def snapshot(o, tag, out):
    for n, v in zip(ATM_FIELDS, o.get_state()):
        out["%s_%s" % (tag, n)] = v
    out[tag + "_scal"] = o.get_scalars()


def reference(nxta, nla):
    """(configuration, inputs, the oracle's snapshots in a fixture's layout), computed once per shape and count and
    never modified."""
    if (nxta, nla) not in _refs:
        acfg = atm_wide(nxta, nla)
        f = synth.atmos_fields(acfg)
        o = make_atm_oracle_of(acfg, f)
        g = {}
        atm_apply(o, f)
        snapshot(o, "init", g)
        o.qgastep()
        snapshot(o, "qgastep", g)
        o.atinvq()
        snapshot(o, "atinvq", g)
        o.atqzbd()
        snapshot(o, "atqzbd", g)
        atm_apply(o, f)
        o.steps(1, 130)
        snapshot(o, "steps130", g)
        o.close()
        assert all(np.isfinite(v).all() for v in g.values())
        _refs[(nxta, nla)] = acfg, f, g
    return _refs[(nxta, nla)]


def against_the_oracle(nxta, nla, what):
    from qgcm_hip import AtmosModel
    acfg, f, g = reference(nxta, nla)
    m = AtmosModel(acfg, ddynat=f["ddynat"])
    try:
        atm_apply(m, f)
        e = atm_state_errs(m, g, "init")
        print(what, "init", e)
        assert all(v < 1e-14 for v in e.values()), e
        atm_load_snapshot(m, g, "init")
        m.qgastep()
        e = atm_state_errs(m, g, "qgastep")
        assert all(v == 0.0 for v in e.values()), ("qgastep", e)
        m.atinvq()
        e = atm_state_errs(m, g, "atinvq")
        print(what, "atinvq", e, "scalars", atm_scal_err(m, g, "atinvq", acfg))
        assert e["pam"] == 0.0 and e["qa"] == 0.0 and e["qam"] == 0.0 and e["pa"] < TOL_CALL, ("atinvq", e)
        assert atm_scal_err(m, g, "atinvq", acfg) < 1e-13
        m.atqzbd()
        e = atm_state_errs(m, g, "atqzbd")
        print(what, "atqzbd", e)
        assert all(v < TOL_CALL for v in e.values()), ("atqzbd", e)
        atm_load_snapshot(m, g, "atinvq")   # ... and from the oracle's own pa: the boundary rule alone, bit for bit
        m.atqzbd()
        e = atm_state_errs(m, g, "atqzbd")
        assert all(v == 0.0 for v in e.values()), ("atqzbd from the oracle's state", e)
        atm_apply(m, f)
        m.steps(130, s0=1)
        e = atm_state_errs(m, g, "steps130")
        print(what, "steps130", e, "scalars", atm_scal_err(m, g, "steps130", acfg))
        assert all(v < TOL_RUN for v in e.values()), ("steps130", e)
        assert atm_scal_err(m, g, "steps130", acfg) < 1e-11
    finally:
        m.close()


@pytest.mark.parametrize("nla", COUNTS)
@pytest.mark.parametrize("nxta", SHAPES)
def test_calls_and_130_steps_vs_oracle(nxta, nla):
    against_the_oracle(nxta, nla, "%dx13x%d" % (nxta + 1, nla))


@pytest.mark.parametrize("switch", ["QGCM_HIP_NO_FUSED_UNPACK", "QGCM_HIP_NO_FUSED_CONSTR"])
@pytest.mark.parametrize("nla", (4, 5))
def test_unfused_paths_vs_oracle(nla, switch, monkeypatch):
    """385 x 13 with the riding unpack, resp. the riding constraint, switched off (read when a handle is created): the
    same oracle at the same bars."""
    monkeypatch.setenv(switch, "1")
    against_the_oracle(384, nla, "385x13x%d %s" % (nla, switch))


@pytest.mark.parametrize("nla", (4, 5))
def test_graph_replay_equals_eager(nla):
    """steps(230) replays captured graphs (two averagings): bitwise the eager call sequence."""
    from qgcm_hip import AtmosModel
    acfg, f, _ = reference(384, nla)
    m = AtmosModel(acfg, ddynat=f["ddynat"])
    try:
        atm_apply(m, f)
        m.steps(230, s0=1)
        a, sa = m.get_state(), m.get_scalars()
        atm_apply(m, f)
        for s in range(1, 231):
            m.qgastep()
            m.atinvq()
            m.atqzbd()
            if (s - 1) % 100 == 0:
                m.lf_average()
        b, sb = m.get_state(), m.get_scalars()
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert np.array_equal(sa, sb)
        assert all(np.isfinite(x).all() for x in a)
    finally:
        m.close()
