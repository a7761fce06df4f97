"""MI355X parity of the ocean mixed layer through the C ABI: qgcm_hip_oml against the golden
vectors of the TRUE reference and against the CPU oracle.

Bars: everything point-wise is bit exact (same expressions, contraction off); the only reordered arithmetic is
the global sums (reference: sequential over i then j; here a fixed tree): the mean entrainment, and through it entoc,
xon(1) and the line sums, and centoc.  sst itself is bitwise after one call and after the first step.

Pinned by the reference (twelve builds, tests/golden/make_golden_oml.py; three of them the tiny grids with two, five and
six layers, under the same fixed bars): the three tiny fixtures on one 48 x 36 tile
column for 40 steps at fixed bars; six fixtures on grids that cross the tiles of k_oml_step (64 x 8) and k_oml_entoc
(64 x 16) - one seam with a last tile of one column and one row, exact multiples of the tile with the wall rows on tile
edges, the zonal wrap between tiles with a full and with a short last tile - under no-flux walls, -Dnb_hflux and both
options on a box, -Dnb_hflux and both on a channel: sst / sstm by integer view, the reordered sums within the bounds
derived in common.oml_bounds.  Pinned by the oracle only (itself bitwise the reference at all twelve): grids of two and
three tile columns and eight to twelve tile rows under all four option pairs, among them the channel without -Dnb_hflux,
which no reference build carries, and -Dsb_hflux alone on a channel."""
import numpy as np
import pytest

from common import (OML_CASES, OML_SEAM_CASES, FIELDS, load_golden, make_oracle, oml_bounds, oml_check_sums,
                    oml_config, oml_init_oracle, oml_load, oml_snaps, relerr, same_bits)
from qgcm_hip import OceanModel, oml_preset, preset, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,cfgname", OML_CASES)
def test_one_call_vs_reference(case, cfgname):
    g, cfg = load_golden(case), preset(cfgname)
    om = oml_config(g)
    m = OceanModel(cfg)
    try:
        m.oml_init(om)
        oml_load(m, g, cfg, False)
        m.oml()
        sst, sstm = m.oml_get_state()
        ent, d = m.oml_get_diag()
        assert np.array_equal(sst, g["call_sst"])      # bit exact
        assert np.array_equal(sstm, g["call_sstm"])
        assert relerr(ent, g["call_entoc"]) < 1e-13
        assert d[1] == g["call_scal"][1]               # convecting fraction: an exact count
        assert abs(d[2] - g["call_scal"][2]) <= 1e-13 * abs(g["call_scal"][2])
        area = cfg.xlo * cfg.ylo * np.abs(ent).max()
        assert abs(d[0] - g["call_scal"][0]) <= 1e-13 * area
        if cfg.cyclic:
            assert np.allclose(d[3:], g["call_scal"][3:], rtol=1e-11, atol=0.0)
    finally:
        m.close()


@pytest.mark.parametrize("case,cfgname", OML_CASES)
def test_coupled_steps_vs_reference(case, cfgname):
    """qgcm_hip_steps with the mixed layer on = oml, qgostep, ocinvq, ocqbdy + averaging incl. sst
    (src/q-gcm.F:1232-1249, 1328-1366); 40 steps cross the averaging twice and the three sst buffers rotate (the
    five- and six-layer fixtures hold steps 1 and 2 only: common.oml_snaps)."""
    g, cfg = load_golden(case), preset(cfgname)
    om = oml_config(g)
    m = OceanModel(cfg)
    try:
        m.oml_init(om)
        oml_load(m, g, cfg, False)
        done = 0
        for n in oml_snaps(case):
            m.steps(n - done, s0=done + 1)
            done = n
            sst, sstm = m.oml_get_state()
            ent, _ = m.oml_get_diag()
            assert relerr(sst, g["steps%d_sst" % n]) < 1e-13, n
            assert relerr(sstm, g["steps%d_sstm" % n]) < 1e-13, n
            assert relerr(ent, g["steps%d_entoc" % n]) < 1e-10, n
            for f, x in zip(FIELDS, m.get_state()):
                assert relerr(x, g["steps%d_%s" % (n, f)]) < 1e-10, (f, n)
    finally:
        m.close()


_TERMS = {}


def _reference_terms(case, cfgname):
    """(xfo, coneno) of the one call of a fixture from the restatement (bitwise the reference's there:
    tests/test_oml_oracle.py), computed once per fixture."""
    if case not in _TERMS:
        g, cfg = load_golden(case), preset(cfgname)
        o = make_oracle(cfg)
        try:
            oml_init_oracle(o, oml_config(g))
            oml_load(o, g, cfg, True)
            o.oml()
            _TERMS[case] = o.oml_get_xfo()
        finally:
            o.close()
    return _TERMS[case]


@pytest.mark.parametrize("case,cfgname", OML_SEAM_CASES)
def test_one_call_bitwise_at_tile_seams(case, cfgname):
    """One oml() on the grids that cross the tiles' seams, against the reference: sst and sstm by integer view (count
    and place of differing points in the message), the convecting fraction exact, entoc, xon(1), centoc and a channel's
    line sums within common.oml_bounds (derived there; figures printed); a second call from the same state gives
    identical bits."""
    g, cfg = load_golden(case), preset(cfgname)
    xfo, coneno = _reference_terms(case, cfgname)
    bound = oml_bounds(cfg, xfo, coneno, g["call_entoc"])
    m = OceanModel(cfg)
    try:
        m.oml_init(oml_config(g))
        runs = []
        for rep in range(2):
            oml_load(m, g, cfg, False)
            m.oml()
            runs.append(tuple(m.oml_get_state()) + tuple(m.oml_get_diag()))
        (sst, sstm, ent, d), (sst2, sstm2, ent2, d2) = runs
        same_bits(sst, g["call_sst"], case + " sst")
        same_bits(sstm, g["call_sstm"], case + " sstm")
        r = oml_check_sums(case, cfg, bound, ent, d, g["call_entoc"], g["call_scal"])
        print(case, "largest |diff| / bound:", {k: round(v, 4) for k, v in r.items()})
        same_bits(sst2, sst, case + " sst (repeat)")
        same_bits(sstm2, sstm, case + " sstm (repeat)")
        same_bits(ent2, ent, case + " entoc (repeat)")
        same_bits(d2, d, case + " scalars (repeat)")
    finally:
        m.close()


@pytest.mark.parametrize("case,cfgname", OML_SEAM_CASES)
def test_first_step_is_bitwise(case, cfgname):
    """qgcm_hip_steps on the seam grids: the first step begins with oml from the inputs and its averaging of sst is
    exact, so sst and sstm are bitwise the reference's after it; after the second the bars of
    test_coupled_steps_vs_reference hold for sst, sstm, entoc and po."""
    g, cfg = load_golden(case), preset(cfgname)
    m = OceanModel(cfg)
    try:
        m.oml_init(oml_config(g))
        oml_load(m, g, cfg, False)
        m.steps(1, s0=1)
        sst, sstm = m.oml_get_state()
        same_bits(sst, g["steps1_sst"], case + " sst after step 1")
        same_bits(sstm, g["steps1_sstm"], case + " sstm after step 1")
        m.steps(1, s0=2)
        sst, sstm = m.oml_get_state()
        ent, _ = m.oml_get_diag()
        errs = dict(sst=relerr(sst, g["steps2_sst"]), sstm=relerr(sstm, g["steps2_sstm"]),
                    entoc=relerr(ent, g["steps2_entoc"]), po=relerr(m.get_state()[0], g["steps2_po"]))
        print(case, "after step 2:", errs)
        assert errs["sst"] < 1e-13 and errs["sstm"] < 1e-13, errs
        assert errs["entoc"] < 1e-10 and errs["po"] < 1e-10, errs
    finally:
        m.close()


@pytest.mark.parametrize("sb,nb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("cfgname", ["box_med", "cyc_small", "cyc_med"])
def test_one_call_bitwise_vs_oracle_all_wall_options(cfgname, sb, nb):
    """One oml() on grids of two and three tile columns under every pair of wall options (inputs of
    test_graph_replay_and_oracle), among them the channel without nb_hflux, which no reference build carries: sst and
    sstm bitwise the oracle's, entoc and the scalars within common.oml_bounds."""
    cfg = preset(cfgname)
    om = oml_preset(cfg, sb_hflux=sb, nb_hflux=nb)
    tag = "%s sb=%d nb=%d" % (cfgname, sb, nb)
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
        wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
        nl = cfg.nlo
        oml_init_oracle(o, om)
        m.oml_init(om)
        for mod in (o, m):
            mod.set_p(po, po)
            mod.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(nl - 1))
            if cfg.cyclic:
                txis, txin = synth.tau_line_integrals(cfg, tx)
                mod.set_cyc_forcing(txis, txin, np.zeros(nl - 1), np.zeros(nl - 1))
        o.oml_set(sst, sstm, fnet, wekto, tx, ty)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
        o.oml()
        m.oml()
        a, b, e, s = o.oml_get()
        xfo, coneno = o.oml_get_xfo()
        sa, sb_ = m.oml_get_state()
        ent, d = m.oml_get_diag()
        same_bits(sa, a, tag + " sst")
        same_bits(sb_, b, tag + " sstm")
        r = oml_check_sums(tag, cfg, oml_bounds(cfg, xfo, coneno, e), ent, d, e, s)
        print(tag, "largest |diff| / bound:", {k: round(v, 4) for k, v in r.items()})
    finally:
        m.close()
        o.close()


@pytest.mark.parametrize("cfgname,sb,nb", [("box_med", False, False), ("box_med", True, True), ("cyc_small", True, True)])
def test_graph_replay_and_oracle(cfgname, sb, nb):
    """120 steps (two 50-step HIP graphs with different sst-buffer rotations + eager remainder) against the CPU
    oracle, on grids that run the fused kernels; every boundary-option combination incl. those the reference
    example builds do not carry (the oracle restates them from src/omlsubs.F)."""
    cfg = preset(cfgname)
    om = oml_preset(cfg, sb_hflux=sb, nb_hflux=nb)
    o = make_oracle(cfg)
    m = OceanModel(cfg)
    try:
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
        wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
        nl = cfg.nlo
        o.oml_init(om.hmoc, om.toc[0], om.toc[1], om.st2d, om.st4d, om.ycexp, om.rrcpoc, om.sb_hflux, om.tsbdy,
                   om.nb_hflux, om.tnbdy)
        m.oml_init(om)
        for mod in (o, m):
            mod.set_p(po, po)
            mod.set_forcing(wekpo, np.zeros_like(wekpo), np.zeros(nl - 1))
            if cfg.cyclic:
                txis, txin = synth.tau_line_integrals(cfg, tx)
                mod.set_cyc_forcing(txis, txin, np.zeros(nl - 1), np.zeros(nl - 1))
        o.oml_set(sst, sstm, fnet, wekto, tx, ty)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
        o.steps_oml(1, 120)
        m.steps(120, s0=1)
        a, b, e, _ = o.oml_get()
        sa, sb_ = m.oml_get_state()
        ent, _ = m.oml_get_diag()
        assert relerr(sa, a) < 1e-12 and relerr(sb_, b) < 1e-12
        assert relerr(ent, e) < 1e-9
        for f, x, y in zip(FIELDS, m.get_state(), o.get_state()):
            assert relerr(x, y) < 1e-9, f
    finally:
        m.close()
        o.close()


def test_one_for_one_calls_equal_steps():
    """The call sequence of the reference main program issued call by call (oml, qgostep, ocinvq, ocqbdy and the
    averaging block when mod(s-1,25) == 0 - as the Fortran shim does) is bitwise qgcm_hip_steps."""
    g, cfg = load_golden("oml_box_tiny"), preset("box_tiny")
    om = oml_config(g)
    ma, mb = OceanModel(cfg), OceanModel(cfg)
    try:
        for m in (ma, mb):
            m.oml_init(om)
            oml_load(m, g, cfg, False)
        ma.steps(30, s0=1)
        for s in range(1, 31):
            mb.oml(); mb.qgostep(); mb.ocinvq(); mb.ocqbdy()
            if (s - 1) % 25 == 0:
                mb.lf_average()
        for x, y in zip(ma.get_state() + ma.oml_get_state(), mb.get_state() + mb.oml_get_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(ma.get_scalars(), mb.get_scalars())
    finally:
        ma.close()
        mb.close()


def test_oml_needs_init_and_whole_domain():
    cfg = preset("box_small")
    m = OceanModel(cfg)
    try:
        with pytest.raises(Exception, match="qgcm_hip_oml_init has not been called"):
            m.oml()
    finally:
        m.close()


@pytest.mark.parametrize("cfgname,nranks,sb,nb", [("box_small", 1, False, False), ("box_small", 2, True, True), ("box_med", 3, False, True),
                                                  ("cyc_small", 2, True, True), ("cyc_med", 3, False, False)])
def test_mixed_layer_on_y_slabs(cfgname, nranks, sb, nb):
    """The mixed layer on y-slabs (virtual ranks on this one GPU): `oml` in two halves around one all-gather of three
    numbers per rank (the mean entrainment), the T row below every slab recomputed locally (entoc averages two T rows
    onto a p row), xon(1) and the line integrals in the step message, edge rows of sst in the halo messages.  60 steps
    (two averagings, every sst buffer rotation) against the whole-domain handle: fields <= 1e-10, sst within 1e-12; after
    the first step, whose sst depends on the inputs alone (the recomputed T row below every slab and the j < jT0 skip
    included), every slab's owned rows of sst and sstm are the whole-domain handle's bit for bit."""
    import torch
    from qgcm_hip import hostinit
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset(cfgname)
    om = oml_preset(cfg, sb_hflux=sb, nb_hflux=nb)
    m = OceanModel(cfg)
    slabs = []
    try:
        consts = global_consts(cfg, None if cfg.cyclic else m.helmholtz)
        po = synth.gaussian_eddy(cfg, noise=1e-3)
        pom = np.asfortranarray(0.995 * po)
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=7)
        wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
        nl = cfg.nlo
        zero2, xon = np.zeros_like(wekpo), np.zeros(nl - 1)
        m.oml_init(om)
        m.set_p(po, pom)
        m.set_forcing(wekpo, zero2, xon)
        cyc = (synth.tau_line_integrals(cfg, tx) + (np.zeros(nl - 1), np.zeros(nl - 1))) if cfg.cyclic else None
        if cyc:
            m.set_cyc_forcing(*cyc)
        m.oml_set_state(sst, sstm)
        m.oml_set_forcing(fnet, wekto, tx, ty)
        st = m.get_state()
        scal = m.get_scalars()
        parts = partition(cfg.nypo, nranks)
        slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
        for sl in slabs:
            sl.oml_init(om)
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.scatter_state(st[0], st[1], st[2], st[3], wekpo, zero2, xon, scal)
        for sl in slabs:
            if cyc:
                sl.set_cyc_forcing(*cyc)
            sl.oml_set_state(sst, sstm)
            sl.oml_set_forcing(fnet, wekto, tx, ty)
        for nst in (1, 59):
            so.steps(nst)
            m.steps(nst)
            got = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo)) for _ in range(4)]
            for g0, g1, fields in so.gather_local():
                for dst, src in zip(got, fields):
                    dst[:, g0 - 1:g1, :] = src
            for f, x, y in zip(FIELDS, got, m.get_state()):
                assert relerr(x, y) < 1e-10, (f, nst)
            ga, gb = m.oml_get_state()
            for sl in slabs:
                la, lb = sl.oml_get_state()
                t1 = min(sl.g1, cfg.nypo - 1)  # owned T rows g0..t1 (global, 1-based)
                loc = slice(sl.g0 - 1 - sl.joff, t1 - sl.joff)
                if nst == 1:
                    assert np.array_equal(la[:, loc], ga[:, sl.g0 - 1:t1]), (sl.rank, "sst after the first step")
                    assert np.array_equal(lb[:, loc], gb[:, sl.g0 - 1:t1]), (sl.rank, "sstm after the first step")
                assert relerr(la[:, loc], ga[:, sl.g0 - 1:t1]) < 1e-12, (sl.rank, nst)
                assert relerr(lb[:, loc], gb[:, sl.g0 - 1:t1]) < 1e-12, (sl.rank, nst)
        for sl in slabs:
            assert np.array_equal(sl.get_scalars(), slabs[0].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        m.close()
