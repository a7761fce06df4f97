"""The ocean outside the step path at layer counts other than three.  Needs an MI355X.

Every ocean kernel that depends on the number of layers is compiled for nlo = 2 .. 8; the step path is pinned at 2, 4,
5, 6 and 8 layers (test_gpu_parity.py, test_gpu_tall_slabs.py), what was built on top of it ran with three.  Here:

  A  by the reference, at 2, 5 and 6 layers (box_tiny2 31 x 25 x 2, box_tiny5 49 x 37 x 5, cyc_tiny6 49 x 37 x 6): the
     goldens tav_*, areacfl_cfl_{box2,box5,cyc6}, mon_*, qod_cyc_tiny6 and oml_* of these fixtures run through the
     parametrised tests of test_gpu_tavg.py, test_gpu_areacfl.py, test_gpu_monitors.py, test_gpu_qocdiag.py and
     test_gpu_oml.py (their case lists carry the new names); this file adds the first mixed-layer step, the running
     mean of po and the y-slab forms of the diagnostics.
  B  by the oracle and the numpy restatements, at 2, 4 and 8 layers on the 193-column grids of
     test_gpu_parity.test_fast_kernels_with_two_and_four_layers (common.layer_cfg): the mixed layer inside 30 steps,
     every diagnostic of the state after them, ties of the CFL maxima across workgroups and slabs, the single-name
     masks of time_means at eight layers, the schedules inside steps() at two and five layers.  The restatements
     reproduce the reference at 2, 5 and 6 layers on the CPU (test_tavg_cpu.py, test_areacfl_cpu.py,
     test_monitors_cpu.py, test_qocdiag_cpu.py, test_oml_oracle.py); that is what stands behind them at 4 and 8.
  C  a column cut into segments and rows split in ONE handle, against the true reference's snapshots.
  D  a coupled window over an ocean of two and of five layers.

No bar is new: each test names the three-layer test whose recipe and bar it repeats."""
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import numpy_areacfl as na
import numpy_cov as nc
import numpy_qocdiag as nq
import numpy_tavg as nt
import test_gpu_areacfl as t_areacfl
import test_gpu_cov as t_cov
import test_gpu_monitors as t_mon
import test_gpu_qocdiag as t_qod
import test_gpu_slab_diagnostics as t_slab
import test_gpu_tavg as t_tav
from common import (FIELDS, OCEAN_LAYERS, SNAPS, apply_inputs, atm_apply, bits, layer_cfg, load_golden, load_snapshot,
                    make_oracle, oml_bounds, oml_check_sums, oml_config, oml_init_oracle, oml_load, preset, relerr,
                    same_bits, scal_err, state_errs)
from numpy_monitors import monitors as np_monitors
from qgcm_hip import (AtmosModel, OceanModel, config, coupled_steps, lib, oml_preset, share_gpu, synth, xforc,
                      xforc_setup)
from qgcm_hip.model import TAV_LAYOUT
from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition, slab_slice
from test_gpu_long_rows import SPLIT_LAUNCHES

pytestmark = pytest.mark.gpu

TOL_CALL = 1e-12  # one Helmholtz solve (test_gpu_parity)
LAYER_FIXTURES = ("box_tiny2", "box_tiny5", "cyc_tiny6")
BSUM_LEN = 5 * 16 * 2  # per layer: the boundary line sums in a cyclic slab's message (5 quantities, BSUM_NB = 16, 2 sides)


# =====================================================================================================================
# A. by the reference, at 2, 5 and 6 layers
# =====================================================================================================================
@pytest.mark.parametrize("case,cfgname", [("oml_" + n, n) for n in LAYER_FIXTURES])
def test_first_step_is_bitwise(case, cfgname):
    """test_gpu_oml.test_first_step_is_bitwise on the fixtures of two, five and six layers: sst and sstm after the first
    step by integer view; after the second the bars of test_coupled_steps_vs_reference (sst, sstm 1e-13; entoc, po
    1e-10).  entoc enters layers 1 and 2: at two layers layer 2 is the bottom layer."""
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


@pytest.mark.parametrize("cfgname", LAYER_FIXTURES)
@pytest.mark.parametrize("mixed_layer", [False, True], ids=["no_oml", "oml"])
def test_po_mean_over_30_steps(cfgname, mixed_layer):
    """test_gpu_tavg.test_po_mean_over_60_steps, 30 steps (steps 1 and 26 average), on the tiny fixtures' grids: the
    sum accumulated inside steps(30) against the per-step po of a second handle (each checked against the state after
    its step), scaled by numpy_tavg.po_mean - the reference's scaling at 2, 5 and 6 layers (test_tavg_cpu.py) - bitwise;
    the state bitwise that of a handle that never enabled the sum."""
    a, b, c = (t_tav.ocean(cfgname, mixed_layer) for _ in range(3))
    try:
        a.enable_po_mean()
        a.steps(30, s0=1)
        mean, n = a.po_mean(count=True)
        assert n == 30 and mean.shape[2] == a.cfg.nlo
        b.enable_po_mean()
        tot = t_tav.per_step_po(b, 1, 30)
        assert np.array_equal(mean, nt.po_mean(tot, 30))
        assert np.array_equal(mean, a.po_mean())  # reading without reset keeps the sum
        c.steps(30, s0=1)
        for h in (b, c):
            for name, x, y in zip(FIELDS, a.get_state(), h.get_state()):
                same_bits(x, y, name)
    finally:
        for m in (a, b, c):
            m.close()


@pytest.mark.parametrize("cfgname", ["box_tiny5", "cyc_tiny6"])
@pytest.mark.parametrize("mixed_layer", [False, True], ids=["no_oml", "oml"])
def test_slab_time_means_equal_whole_domain(cfgname, mixed_layer):
    """test_gpu_tavg.test_slab_time_means_equal_whole_domain on two and three y-slabs of the five- and six-layer
    fixtures' grids: after 26 steps (the last one averages) tavocn on the slabs gives the whole handle's means,
    bitwise.  gridDim.y of k_tav_accum / k_tav_mean is the owned rows; the field index TAV_UU(nl)."""
    m = t_tav.ocean(cfgname, mixed_layer)
    cfg = m.cfg
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, entoc=np.zeros_like(wekpo))
    try:
        m.steps(26, s0=1)
        m.tavocn()
        whole = m.time_means()
        assert whole["pocav"].shape[2] == cfg.nlo and np.any(whole["uufo"]) and np.any(whole["vtvfo"])
        for nranks in (2, 3):
            so = t_slab.slabs_like(m, om, f, mixed_layer, partition(cfg.nypo, nranks))
            try:
                if mixed_layer:
                    for x in so.slabs:  # slabs_like gives the slabs a zero fnetoc
                        x.oml_set_forcing(fnet, wekto, tx, ty)
                else:
                    so.set_time_mean_params(om)
                    so.set_time_mean_fields(fnet)
                so.tavocn()
                got = so.time_means()
                assert got["nsumoc"] == 1
                t_tav.same(got, whole)
            finally:
                t_slab.close(so)
    finally:
        m.close()


@pytest.mark.parametrize("name", ["box_tiny5", "cyc_tiny6"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_slab_monitors_valids_and_prsamp(name, nranks):
    """test_gpu_slab_diagnostics.test_golden, test_valids_bitwise and test_prsamp on the five- and six-layer fixtures:
    the monitors of the slabs against the reference's own (mon_<name>.npz; EXACT names bitwise, integrals within 1e-12
    of their scale), valids bitwise the whole handle's, prsamp's spot values and sst range bitwise, its averages within
    1e-12 of the average of the modulus."""
    cfg, f, c, want = t_mon.golden_case(name)
    _, scales = np_monitors(f, c)
    m = OceanModel(cfg)
    so = t_slab.make_slabs(cfg, partition(cfg.nypo, nranks))
    try:
        m.set_state(f["po"], f["pom"], f["qo"], f["qom"])
        m.set_forcing(f["wekpo"], f["entoc"], np.zeros(cfg.nlo - 1))
        t_slab.load(so, f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"])
        for x in so.slabs:
            x.set_monitor_params(rhooc=c["rhooc"], cpoc=c["cpoc"], hmoc=c["hmoc"], ycexp=c["ycexp"],
                                 sb_hflux=bool(c["sb_hflux"]), nb_hflux=bool(c["nb_hflux"]))
            x.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
        t_slab.same_on_every_rank(so, "monitors")
        t_mon.compare(so.monitors(), want, scales)
        got = t_slab.same_on_every_rank(so, "valids")
        ok, out = m.valids()
        assert got[0] == ok and ok and np.array_equal(got[1], out) and len(out) == 14 + cfg.nlo
        t_slab.same_on_every_rank(so, "prsamp")
        got, whole = so.prsamp(), m.prsamp()
        for k in ("po_centre", "qo_centre", "sstmin", "sstmax"):
            assert np.array_equal(got[k], whole[k]), k
        assert len(got["po_centre"]) == cfg.nlo
        on = 1.0 / (cfg.nxto * cfg.nyto)
        for k, fld in (("pavgoc", "po"), ("qavgoc", "qo")):
            assert np.all(np.abs(got[k] - whole[k]) <= 1e-12 * t_slab.xintp_abs(f[fld]) * on), k
    finally:
        t_slab.close(so)
        m.close()


# =====================================================================================================================
# B. by the oracle and the restatements, at 2, 4 and 8 layers on 193 x 97 / 193 x 65
# =====================================================================================================================
ALL_WALLS = [(False, False), (True, False), (False, True), (True, True)]
ML_CASES = [(2, cyc, sb, nb) for cyc in (False, True) for sb, nb in ALL_WALLS] + \
           [(nlo, cyc, True, True) for nlo in (4, 8) for cyc in (False, True)]


def ml_fields(cfg, om):
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(po=po, pom=np.asfortranarray(0.995 * po), sst=sst, sstm=sstm, fnetoc=fnet, tauxo=tx, tauyo=ty, wekto=wekto,
             wekpo=wekpo, entoc=np.zeros_like(wekpo))
    if cfg.cyclic:
        f["txis"], f["txin"] = synth.tau_line_integrals(cfg, tx)
    return f


def ml_load(mod, cfg, f, is_oracle):
    """The inputs into an Oracle or a handle whose mixed layer is on (common.oml_load's sequence)."""
    nl = cfg.nlo
    mod.set_p(f["po"], f["pom"])
    mod.set_forcing(f["wekpo"], f["entoc"], np.zeros(nl - 1))
    if cfg.cyclic:
        mod.set_cyc_forcing(f["txis"], f["txin"], np.zeros(nl - 1), np.zeros(nl - 1))
    if is_oracle:
        mod.oml_set(f["sst"], f["sstm"], f["fnetoc"], f["wekto"], f["tauxo"], f["tauyo"])
    else:
        mod.oml_set_state(f["sst"], f["sstm"])
        mod.oml_set_forcing(f["fnetoc"], f["wekto"], f["tauxo"], f["tauyo"])


def ml_handle(cfg, om, f):
    m = OceanModel(cfg)
    m.oml_init(om)
    ml_load(m, cfg, f, False)
    return m


@pytest.mark.parametrize("nlo,cyclic,sb,nb", ML_CASES)
def test_mixed_layer_inside_30_steps(nlo, cyclic, sb, nb):
    """The mixed layer inside a step at two, four and eight layers (k_tend<NL> with the QgOmlFinal riders; two and four
    take the fused forms, eight the separate launches), all four wall options at two layers.
      one call   test_gpu_oml.test_one_call_bitwise_vs_oracle_all_wall_options: sst, sstm bitwise the oracle's, entoc and
                 the scalars within common.oml_bounds;
      30 steps   (three 10-step graph blocks, steps 1 and 26 average) at the bars of test_graph_replay_and_oracle: sst,
                 sstm 1e-12, entoc and the fields 1e-9; graph replay bitwise the eager calls oml, qgostep, ocinvq, ocqbdy
                 (+ lf_average), as test_gpu_oml.test_one_for_one_calls_equal_steps;
      two slabs  (sb = nb = 1) the same run at the bars of test_mixed_layer_on_y_slabs: the owned rows of sst, sstm
                 bitwise after the first step, 1e-12 after 30, fields 1e-10, the scalars equal on both ranks; the slab
                 message is 3 nlo ldw + 3 doubles (+ the boundary line sums of a channel)."""
    cfg = layer_cfg(nlo, cyclic)
    om = oml_preset(cfg, sb_hflux=sb, nb_hflux=nb)
    tag = "%s sb=%d nb=%d" % (cfg.name, sb, nb)
    f = ml_fields(cfg, om)
    o = make_oracle(cfg)
    a, b = ml_handle(cfg, om, f), ml_handle(cfg, om, f)
    slabs = []
    try:
        oml_init_oracle(o, om)
        ml_load(o, cfg, f, True)
        # one call
        o.oml()
        b.oml()
        ra, rb, re, rs = o.oml_get()
        xfo, coneno = o.oml_get_xfo()
        sa, sb_ = b.oml_get_state()
        ent, d = b.oml_get_diag()
        same_bits(sa, ra, tag + " sst")
        same_bits(sb_, rb, tag + " sstm")
        r = oml_check_sums(tag, cfg, oml_bounds(cfg, xfo, coneno, re), ent, d, re, rs)
        print(tag, "largest |diff| / bound:", {k: round(v, 4) for k, v in r.items()})
        # 30 steps: oracle, graph replay, eager calls
        ml_load(o, cfg, f, True)
        ml_load(b, cfg, f, False)
        st0, scal0 = a.get_state(), a.get_scalars()
        o.steps_oml(1, 30)
        a.steps(30, s0=1)
        first = None
        for s in range(1, 31):
            b.oml(); b.qgostep(); b.ocinvq(); b.ocqbdy()
            if (s - 1) % 25 == 0:
                b.lf_average()
            if s == 1:
                first = [np.array(x) for x in b.get_state() + list(b.oml_get_state())]
        ra, rb, re, _ = o.oml_get()
        sa, sb_ = a.oml_get_state()
        ent, _ = a.oml_get_diag()
        errs = dict(sst=relerr(sa, ra), sstm=relerr(sb_, rb), entoc=relerr(ent, re))
        errs.update({n: relerr(x, y) for n, x, y in zip(FIELDS, a.get_state(), o.get_state())})
        print(tag, "30 steps vs oracle:", errs)
        assert errs["sst"] < 1e-12 and errs["sstm"] < 1e-12, errs
        assert all(errs[k] < 1e-9 for k in ("entoc",) + FIELDS), errs
        for name, x, y in zip(FIELDS + ("sst", "sstm"), a.get_state() + list(a.oml_get_state()),
                              b.get_state() + list(b.oml_get_state())):
            same_bits(x, y, tag + " graph vs eager " + name)
        same_bits(a.get_scalars(), b.get_scalars(), tag + " scalars")
        if not (sb and nb):
            return
        # two y-slabs
        consts = global_consts(cfg, None if cfg.cyclic else a.helmholtz)
        parts = partition(cfg.nypo, 2)
        slabs = [HipSlab(cfg, consts, g0, g1, rk, 2, sync_each_call=True) for rk, (g0, g1) in enumerate(parts)]
        for sl in slabs:
            sl.oml_init(om)
            ldw = -(-(cfg.nxto + 1) // 16) * 16
            assert sl.th_len == 3 * nlo * ldw + 3 + (BSUM_LEN * nlo if cyclic else 0)
        so = SlabOcean(cfg, slabs, LocalComm(2, after=torch.cuda.synchronize))
        so.scatter_state(st0[0], st0[1], st0[2], st0[3], f["wekpo"], f["entoc"], np.zeros(nlo - 1), scal0)
        for sl in slabs:
            if cyclic:
                sl.set_cyc_forcing(f["txis"], f["txin"], np.zeros(nlo - 1), np.zeros(nlo - 1))
            sl.oml_set_state(f["sst"], f["sstm"])
            sl.oml_set_forcing(f["fnetoc"], f["wekto"], f["tauxo"], f["tauyo"])
        for nst in (1, 29):
            so.steps(nst)
            whole = first if nst == 1 else a.get_state() + list(a.oml_get_state())
            got = [np.zeros((cfg.nxpo, cfg.nypo, nlo)) for _ in range(4)]
            for g0, g1, fields in so.gather_local():
                for dst, src in zip(got, fields):
                    dst[:, g0 - 1:g1, :] = src
            for name, x, y in zip(FIELDS, got, whole[:4]):
                assert relerr(x, y) < 1e-10, (tag, name, nst)
            for sl in slabs:
                la, lb = sl.oml_get_state()
                t1 = min(sl.g1, cfg.nypo - 1)  # owned T rows g0..t1 (global, 1-based)
                loc = slice(sl.g0 - 1 - sl.joff, t1 - sl.joff)
                if nst == 1:
                    same_bits(la[:, loc], whole[4][:, sl.g0 - 1:t1], tag + " slab sst after the first step")
                    same_bits(lb[:, loc], whole[5][:, sl.g0 - 1:t1], tag + " slab sstm after the first step")
                assert relerr(la[:, loc], whole[4][:, sl.g0 - 1:t1]) < 1e-12, (tag, sl.rank, nst)
                assert relerr(lb[:, loc], whole[5][:, sl.g0 - 1:t1]) < 1e-12, (tag, sl.rank, nst)
        assert np.array_equal(slabs[0].get_scalars(), slabs[1].get_scalars())
    finally:
        for sl in slabs:
            sl.close()
        a.close()
        b.close()
        o.close()


@pytest.mark.parametrize("nlo", [2, 4, 8])
@pytest.mark.parametrize("cyclic", [False, True], ids=["box", "cyclic"])
def test_diagnostics_after_30_steps(nlo, cyclic):
    """Every diagnostic of the state after 30 mixed-layer steps (sb = nb = 1) against its numpy restatement of the pulled
    state, each at the rule of its three-layer file:
      running mean of po   test_gpu_tavg.test_po_mean_over_60_steps: bitwise the per-step sums of a twin, states bitwise
      monitors()           test_gpu_monitors.run: EXACT names bitwise, integrals within 1e-12 of their scale
      valids(), prsamp()   test_gpu_long_row_diagnostics.test_valids_and_prsamp_at_23040: numpy's own extrema bitwise;
                           the layer averages within 1e-12 of the average of the modulus
      qocdiag / ocnc       test_gpu_qocdiag.test_full_size: bitwise
      covocn()             test_gpu_cov.test_full_size_ocean: bitwise (nsi = 16: 12 x 6 / 12 x 4 variables)
      area_averages()      test_gpu_areacfl.test_area_averages_follow_the_sst_rotation: denominators bitwise, numerators
                           within 2 n 2^-53 sum|terms|
      cfl()                test_gpu_areacfl.test_cfl_of_a_stepped_handle: maxima, counts, locations exact; at eight
                           layers the 18 maxima are distinct and non-zero on the numpy side, so that a dropped second
                           pass of k_cfl_final (16 waves, one quantity each) cannot pass
      tavocn() x 3         test_gpu_tavg.test_full_size_tavocn: time_means() bitwise numpy_tavg's."""
    cfg = layer_cfg(nlo, cyclic)
    om = oml_preset(cfg, sb_hflux=True, nb_hflux=True)
    f = ml_fields(cfg, om)
    m, twin = ml_handle(cfg, om, f), ml_handle(cfg, om, f)
    tag = cfg.name
    try:
        m.set_monitor_params(om)
        m.enable_po_mean()
        m.enable_covariance(16)
        nvar = (cfg.nxto // 16) * (cfg.nyto // 16)
        assert m.covariance_size()["nvar"] == nvar
        x, y = cfg.xlo, cfg.ylo
        T = m.set_areas([0.0, 0.13 * x, 0.4 * x], [x, 0.71 * x, 0.9 * x], [0.0, 0.22 * y, 0.5 * y], [y, 0.83 * y, y])
        m.steps(30, s0=1)
        # the running mean of po
        mean, n = m.po_mean(count=True)
        twin.enable_po_mean()
        tot = t_tav.per_step_po(twin, 1, 30)
        assert n == 30 and mean.shape == (cfg.nxpo, cfg.nypo, nlo) and np.array_equal(mean, nt.po_mean(tot, 30))
        for name, a, b in zip(FIELDS, m.get_state(), twin.get_state()):
            same_bits(a, b, tag + " " + name)
        p, pom, q, qom = m.get_state()
        s = m.oml_get_state()[0]
        # monitors
        got = m.monitors()
        want, scales = t_mon.reference(m, om, f, True)
        assert set(got) == set(want) and len(want["ddtkeoc"]) == nlo
        assert np.all(want["ddtkeoc"] != 0.0) and want["pkenoc"] != 0.0 and want["entmoc"] != 0.0
        t_mon.compare(got, want, scales)
        # valids
        ok, out = m.valids()
        assert ok and len(out) == 14 + nlo
        assert out[0] == p.min() and out[1] == p.max() and out[2] == q.min() and out[3] == q.max()
        assert out[4] == s.min() and out[5] == s.max()
        assert out[6] == f["wekto"].min() and out[7] == f["wekto"].max()
        rg = 1.0 / np.asarray(cfg.gpoc)
        eta = [rg[k] * (p[:, :, k + 1] - p[:, :, k]) for k in range(nlo - 1)]
        h = [cfg.hoc[0] - eta[0]] + [cfg.hoc[k] - eta[k] + eta[k - 1] for k in range(1, nlo - 1)] + \
            [cfg.hoc[nlo - 1] + eta[nlo - 2] - 0.0]
        assert (out[8], out[9]) == (h[0].min(), h[0].max())
        if nlo > 2:  # all inner layers together (test_gpu_valids.test_more_than_four_layers)
            assert (out[10], out[11]) == (min(v.min() for v in h[1:-1]), max(v.max() for v in h[1:-1]))
        assert (out[12], out[13]) == (h[-1].min(), h[-1].max())
        assert np.all(out[14:] == 0.0)
        # prsamp
        got = m.prsamp()
        ic, jc = (cfg.nxpo + 1) // 2 - 1, (cfg.nypo + 1) // 2 - 1  # src/q-gcm.F:1974-1975, 0-based
        assert np.array_equal(got["po_centre"], p[ic, jc, :]) and np.array_equal(got["qo_centre"], q[ic, jc, :])
        assert got["sstmin"] == s.min() and got["sstmax"] == s.max()
        w = np.ones(p.shape[:2])
        w[0, :] *= 0.5
        w[-1, :] *= 0.5
        w[:, 0] *= 0.5
        w[:, -1] *= 0.5
        on = 1.0 / (cfg.nxto * cfg.nyto)
        for k, a in (("pavgoc", p), ("qavgoc", q)):
            ref = np.einsum("ij,ijk->k", w, a) * on
            assert len(got[k]) == nlo and np.all(np.abs(got[k] - ref) <= 1e-12 * t_slab.xintp_abs(a) * on), k
        # qocdiag / ocnc_sample
        for nsko in (1, 2):
            t_qod.same(m.vorticity_budget(nsko), t_qod.restated(m, f, True, nsko))
        want = nq.ocnc(s, p, q, f["wekto"], f["tauxo"], f["tauyo"], cfg.gpoc, 2)
        got = m.ocean_dump(2)
        assert sorted(got) == sorted(want) and got["h"].shape[0] == nlo - 1
        for n in want:
            assert np.array_equal(got[n], want[n][0] if n in t_qod.FLAT else want[n]), n
        # covariance
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        m.covocn()
        nc.covocn(p[:, :, 0], s, 16, ap, at)
        t_cov.same(m.covariance(), t_cov.restated(ap, at, t_cov.OCN))
        # area averages and CFL
        t_areacfl.check_areas(tag + " stepped", m.area_averages(parts=True), s, T)
        kw = dict(rdxf0=1.0 / (cfg.dxo * cfg.fnot), dt=cfg.dto, dx=cfg.dxo, rhf0hm=0.5 / (cfg.fnot * om.hmoc))
        crit = 0.5 * na.cfltry(p, f["tauxo"], f["tauyo"], cflcrit=0.8, **kw)["courant"].max()
        want = na.cfltry(p, f["tauxo"], f["tauyo"], cflcrit=crit, **kw)
        assert want["nbad"].sum() > 0 and len(want["maxima"]) == 2 * (nlo + 1)
        assert len(set(want["maxima"])) == 2 * (nlo + 1) and np.all(want["maxima"] > 0.0)
        t_areacfl.check_cfl(tag + " stepped", m.cfl(crit), want)
        # time means: three contributions, one step apart
        c = nt.consts(cfg.dxo, cfg.fnot, om.ycexp, om.hmoc, om.tsbdy, om.tnbdy, cfg.cyclic, om.sb_hflux, om.nb_hflux)
        S = nt.tavini(cfg.nxpo, cfg.nypo, nlo)
        for k in range(3):
            m.steps(1 if k else 0)
            m.tavocn()
            nt.tavocn(S, t_tav.host_fields(m, cfg.name, True, f), c)
        got = m.time_means()
        assert got["nsumoc"] == 3 and got["qocav"].shape[2] == nlo
        t_tav.same(got, nt.tavout(S))
    finally:
        m.close()
        twin.close()


def test_time_mean_masks_at_eight_layers():
    """k_tav_mean<8>'s 32-bit mask carries 30 fields (bits 0 .. 29: six surface sums, pocav and qocav of eight layers, the
    six flux sums, uptpoc, vptpoc).  The ABI selects by output name - 16 of them, pocav / qocav set eight bits each, uptpoc
    / vptpoc bits 28 and 29 - so the unit tested is a name: a per-bit sentinel in the device's buffer of means cannot be
    observed through it.  That buffer lives as long as the handle, so a read that follows a full read of the same sums
    would find correct stale values whatever its mask did.  Hence every name is read ALONE right after a contribution
    that changed every sum (the forcing is scaled from one contribution to the next, so that the means of the forcing
    fields move too; asserted on the numpy side), before any other read of those sums, and is bitwise numpy_tavg's mean
    (test_gpu_tavg.test_golden_time_means' partial read and bar).  A name whose bits were dropped, misplaced or skipped
    returns the means of the earlier sums or memory never written, and fails."""
    cfg = layer_cfg(8, False)
    om = oml_preset(cfg, sb_hflux=True, nb_hflux=False)
    f = ml_fields(cfg, om)
    m = ml_handle(cfg, om, f)
    try:
        c = nt.consts(cfg.dxo, cfg.fnot, om.ycexp, om.hmoc, om.tsbdy, om.tnbdy, cfg.cyclic, om.sb_hflux, om.nb_hflux)
        S = nt.tavini(cfg.nxpo, cfg.nypo, 8)
        names = [n for n, _ in TAV_LAYOUT]
        assert len(names) == 16 and 6 + 2 * 8 + 6 + 2 == 30
        prev = nt.tavout(S)
        for k, name in enumerate(names):
            g = dict(f)
            for fld in ("fnetoc", "wekto", "tauxo", "tauyo", "wekpo"):
                g[fld] = np.asfortranarray((1.0 + 0.125 * k) * f[fld])
            m.set_forcing(g["wekpo"], g["entoc"], np.zeros(7))
            m.oml_set_forcing(g["fnetoc"], g["wekto"], g["tauxo"], g["tauyo"])
            m.steps(1)
            m.tavocn()
            nt.tavocn(S, t_tav.host_fields(m, cfg.name, True, g), c)
            want = nt.tavout(S)
            part = m.time_means([name])  # the first read of these sums
            assert sorted(part) == sorted([name, "nsumoc"]) and part["nsumoc"] == k + 1
            assert k == 0 or not np.array_equal(want[name], prev[name]), name  # stale means would not pass
            assert np.any(want[name]) or name in ("uptpoc", "vptpoc") and k == 0, name
            same_bits(part[name], want[name], name)
            prev = want
        t_tav.same(m.time_means(), prev)  # the partial reads left the sums alone
    finally:
        m.close()


def tie_last_layer(p, pair):
    """Gives the last layer's |v| the same value, bit for bit, at the differences p(i+1,j) - p(i,j) of the two (i, j) of
    `pair` (1-based), above every other one: p(i,j) is rounded to a multiple of a power of two and p(i+1,j) = p(i,j) +- D
    with D a multiple of it twice the largest difference of the layer, so that the difference is +-D without rounding;
    the sign is that of the background's p(i+2,j) - p(i,j), which keeps the next difference below D (the recipe of
    tests/golden/make_golden_areacfl.py's tie)."""
    dmax = np.abs(np.diff(p[:, :, -1], axis=0)).max()
    q = 2.0 ** (np.floor(np.log2(dmax)) - 20)
    D = np.round(2.0 * dmax / q) * q
    for i, j in pair:
        a = np.round(p[i - 1, j - 1, -1] / q) * q
        sg = 1.0 if p[i + 1, j - 1, -1] >= a else -1.0
        p[i - 1, j - 1, -1], p[i, j - 1, -1] = a, a + sg * D
        assert (a + sg * D) - a == sg * D


TIED_PAIRS = {"far": ((150, 20), (30, 70)), "near": ((40, 20), (35, 70))}


@pytest.mark.parametrize("nlo", [2, 4, 8])
@pytest.mark.parametrize("which", ["far", "near"])
def test_cfl_tie_across_workgroups_and_slabs(nlo, which):
    """test_gpu_areacfl.test_cfl_against_the_reference's rule (maxima, counts, locations exactly the restatement's) and
    test_slab_cfl's on the 193 x 97 box with the last layer's largest |v| tied, bit for bit, between two points.
      far   (150, 20) and (30, 70): 120 columns apart, so on the whole handle the tie crosses the 64-column workgroups
            of k_cfl_scan and is settled in k_cfl_final;
      near  a second pair, (40, 20) and (35, 70): one tile column, so that on two y-slabs (rows 1 - 49, 50 - 97), where
            it lies in the first and in the last slab, nothing but k_cfl_combine settles it.
    Both pairs run both ways (either one lies in the first and in the last slab).  First in scan order (j outer) is the
    point in row 20, the one with the larger i; the reference decides the same rule at 2, 5 and 6 layers
    (areacfl_cfl_{box2,box5,cyc6}.npz)."""
    cfg = layer_cfg(nlo, False)
    om = oml_preset(cfg)
    pair = TIED_PAIRS[which]
    assert (abs(pair[0][0] - pair[1][0]) > 64) == (which == "far") and ((pair[0][0] - 1) // 64 == (pair[1][0] - 1) // 64) == (which == "near")
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    for k in range(nlo):  # a po that differs in every layer
        po[:, :, k] *= 1.0 + 0.07 * k
    tie_last_layer(po, pair)
    po = np.asfortranarray(po)
    sst, _, _, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    kw = dict(rdxf0=1.0 / (cfg.dxo * cfg.fnot), dt=cfg.dto, dx=cfg.dxo, rhf0hm=0.5 / (cfg.fnot * om.hmoc))
    q = na.cfl_names(nlo).index("v%d" % nlo)
    crit = 0.5 * na.cfltry(po, tx, ty, cflcrit=0.8, **kw)["courant"][q]  # half the tied value: both points are offenders
    want = na.cfltry(po, tx, ty, cflcrit=crit, **kw)
    v = np.abs(kw["rdxf0"] * (po[1:, :, -1] - po[:-1, :, -1]))
    at = sorted(map(tuple, (np.argwhere(bits(v) == bits(v.max())) + 1).tolist()))
    assert at == sorted(pair) and tuple(want["loc"][q]) == pair[0] and want["nbad"][q] >= 2
    assert len(set(want["maxima"])) == 2 * (nlo + 1) and np.all(want["maxima"] > 0.0)
    parts = partition(cfg.nypo, 2)
    assert parts[0][0] <= pair[0][1] <= parts[0][1] and parts[1][0] <= pair[1][1] <= parts[1][1]
    m = OceanModel(cfg)
    so = t_slab.make_slabs(cfg, parts)
    try:
        m.set_state(po, po, po, po)
        m.set_monitor_params(hmoc=om.hmoc)
        m.set_monitor_fields(tx, ty, np.zeros_like(sst), sst)
        t_areacfl.check_cfl("%s %s tie" % (cfg.name, which), m.cfl(crit), want)
        for x in so.slabs:
            sl = slab_slice(cfg.nypo, x.g0, x.g1)
            x.set_state(po[:, sl], po[:, sl], po[:, sl], po[:, sl])
            x.set_monitor_params(hmoc=om.hmoc)
            x.set_monitor_fields(tx, ty, np.zeros_like(sst), sst)
        for r in so.diagnostic("cfl", cflcrit=crit):
            t_areacfl.check_cfl("%s %s tie, two slabs" % (cfg.name, which), r, want)
    finally:
        t_slab.close(so)
        m.close()


@pytest.mark.parametrize("cfgname", ["box_tiny2", "box_tiny5"])
@pytest.mark.parametrize("mixed_layer", [False, True], ids=["no_oml", "oml"])
def test_schedules_inside_steps(cfgname, mixed_layer):
    """The scheduled vorticity budget (every 9 steps: 1, 10, 19, 28), the scheduled covariance (after steps 1 and 26)
    and the running mean of po inside steps(30) at two and five layers are bitwise the same calls made between single
    steps, and the state is that of a handle with nothing scheduled.  With the mixed layer on a scheduled budget is
    taken after its step's oml: each of the four snapshots is compared with a fresh handle stepped to the step before,
    which calls oml() and then vorticity_budget(), and the last differs from the budget between steps
    (test_gpu_qocdiag.test_scheduled_dump_without_mixed_layer_equals_between_steps, test_scheduled_dump_is_taken_after_oml,
    test_schedule_leaves_the_state_bitwise; test_gpu_cov.test_schedule_equals_explicit_calls;
    test_gpu_tavg.test_po_mean_over_60_steps)."""
    a, _, _ = t_mon.setup(cfgname, mixed_layer)
    b, _, _ = t_mon.setup(cfgname, mixed_layer)
    c, _, _ = t_mon.setup(cfgname, mixed_layer)
    try:
        for m in (a, b):
            m.enable_covariance(6)  # 5 x 4 variables on box_tiny2's 30 x 24 T cells, 8 x 6 on box_tiny5's 48 x 36
            m.enable_po_mean()
        a.schedule_vorticity_budget(2, 9, capacity=4)
        a.schedule_covariance(25, 1)
        a.prepare_steps(30, s0=1)
        a.steps(30, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 10, 19, 28] and snaps[0][1]["dqdt"].shape[0] == a.cfg.nlo
        tot, twin = None, {}
        for s in range(1, 31):
            if (s - 1) % 9 == 0 and not mixed_layer:
                twin[s] = b.vorticity_budget(2)
            b.steps(1, s0=s)
            pre = b.po_mean(reset=True)
            tot = pre if tot is None else tot + pre
            if s % 25 == 1:
                b.covocn()
        if mixed_layer:  # a snapshot is taken after its step's oml: a fresh handle per snapshot (oml() changes sst)
            for s in (1, 10, 19, 28):
                h, _, _ = t_mon.setup(cfgname, True)
                try:
                    h.steps(s - 1, s0=1)
                    between = h.vorticity_budget(2)
                    h.oml()
                    twin[s] = h.vorticity_budget(2)
                finally:
                    h.close()
            assert not np.array_equal(snaps[3][1]["qotent"], between["qotent"])
        assert sorted(twin) == [1, 10, 19, 28]
        for s, snap in snaps:
            t_qod.same(snap, twin[s])
        ca, cb = a.covariance(), b.covariance()
        assert ca["nupo"] == cb["nupo"] == 2
        t_cov.same(ca, cb)
        mean, n = a.po_mean(count=True)
        assert n == 30 and np.array_equal(mean, nt.po_mean(tot, 30))
        if not mixed_layer:
            c.steps(30, s0=1)
        for h in ((b,) if mixed_layer else (b, c)):
            for name, x, y in zip(FIELDS, a.get_state(), h.get_state()):
                same_bits(x, y, name)
        if mixed_layer:
            for x, y in zip(a.oml_get_state(), b.oml_get_state()):
                same_bits(x, y, "sst")
    finally:
        for m in (a, b, c):
            m.close()


# =====================================================================================================================
# C. segments and split rows in ONE handle, against the true reference's snapshots
# =====================================================================================================================
def whole_steps_vs_reference(m, name, tag):
    """test_gpu_parity.test_whole_steps_vs_reference on the handle m: the committed snapshots of the true reference, the
    first two steps within 1e-12, the later ones within 1e-10, the scalars within 1e-11.  Returns the largest errors."""
    cfg, g = m.cfg, load_golden(name)
    apply_inputs(m, g, cfg)
    done, worst = 0, dict(first=0.0, later=0.0, scal=0.0)
    for s in SNAPS[name]:
        m.steps(s - done, s0=done + 1)
        done = s
        e = state_errs(m, g, "steps%d" % s)
        se = scal_err(m, g, "steps%d" % s, cfg)
        print(tag, "step", s, e, "scalars %.3e" % se)
        assert all(v < (TOL_CALL if s <= 2 else 1e-10) for v in e.values()), (s, e)
        assert se < 1e-11
        k = "first" if s <= 2 else "later"
        worst[k], worst["scal"] = max(worst[k], max(e.values())), max(worst["scal"], se)
    print(tag, "largest:", worst)
    return done


def ocinvq_vs_reference(m, name, tag):
    """test_gpu_parity.test_helmholtz_vs_reference and test_ocinvq on the handle m: both Helmholtz vectors and po after
    ocinvq within 1e-12, pom, qo, qom untouched, the scalars within 1e-13; qo, po after ocqbdy within 1e-12."""
    cfg, g = m.cfg, load_golden(name)
    assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc"]), g["helm_sol"]) < TOL_CALL
    assert relerr(m.helmholtz(g["helm_rhs"], g["helm_boc0"]), g["helm_sol0"]) < TOL_CALL
    apply_inputs(m, g, cfg)
    load_snapshot(m, g, "init")
    m.qgostep()
    m.ocinvq()
    e = state_errs(m, g, "ocinvq")
    se = scal_err(m, g, "ocinvq", cfg)
    print(tag, e, "scalars %.3e" % se)
    assert e["pom"] == 0.0 and e["qo"] == 0.0 and e["qom"] == 0.0, e
    assert e["po"] < TOL_CALL, e
    assert se < 1e-13
    m.ocqbdy()
    e = state_errs(m, g, "ocqbdy")
    assert e["qo"] < TOL_CALL and e["po"] < TOL_CALL, e


@pytest.mark.parametrize("name", LAYER_FIXTURES)
@pytest.mark.parametrize("seg_rows", [16, 7])
def test_forced_segments_vs_reference(name, seg_rows, monkeypatch):
    """test_gpu_tall_columns.test_forced_segments_whole_steps_vs_reference and test_forced_segments_ocinvq_vs_reference
    (same bars) at two, five and six layers: 35 interior rows (box_tiny5, cyc_tiny6) as 12, 12, 11 or five of 7,
    23 (box_tiny2) as 12, 11 or 6, 6, 6, 5.  The tables of k_thomas_seg / k_thomas_corr_seg are offset by
    ceil(nk / TH_KW) nl S; the plan is asserted on the handle, so that a silently unforced plan fails."""
    cfg = preset(name)
    plan = lib.thomas_segments(cfg.nypo - 2, seg_rows)
    assert len(plan) >= 2 and max(n for _, n in plan) <= seg_rows and min(n for _, n in plan) >= lib.THOMAS_SEG_MIN
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", str(seg_rows))  # read by qgcm_hip_set_grid
    for check in (ocinvq_vs_reference, whole_steps_vs_reference):
        m = OceanModel(cfg)
        try:
            assert m.thomas_plan() == plan and m.row_plan() == (1, cfg.nxto)
            done = check(m, name, "%s seg %d" % (name, seg_rows))
            if done:  # the launch plan of the segmented solve: two Thomas launches per step
                prof = m.profile_steps(2, s0=done + 1)
                assert prof["k_thomas"][1] == 4 and prof["k_tend"][1] == 2
        finally:
            m.close()


@pytest.mark.parametrize("P", [2, 3, 4])
def test_forced_split_vs_reference(P, monkeypatch):
    """test_gpu_long_rows.test_forced_split_whole_steps_vs_reference and test_forced_split_ocinvq_vs_reference (same
    bars) on cyc_tiny6: rows of 48 points as P interleaved sub-rows, six modes in blockIdx.z + layer0 and six scratch
    strides; then the launch counts of the split row family."""
    name = "cyc_tiny6"
    cfg = preset(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", str(P))  # read by qgcm_hip_set_grid
    for check in (ocinvq_vs_reference, whole_steps_vs_reference):
        m = OceanModel(cfg)
        try:
            assert m.row_plan() == (P, cfg.nxto // P) == lib.row_split(cfg.nxto, P) and len(m.thomas_plan()) == 1
            done = check(m, name, "%s split %d" % (name, P))
            if done:
                prof = {k: n for k, (_, n) in m.profile_steps(2, s0=done + 1).items() if n}
                for k, n in SPLIT_LAUNCHES.items():
                    assert prof[k] == 2 * n, (k, prof)
        finally:
            m.close()


def test_split_rows_on_a_column_in_segments(monkeypatch):
    """test_gpu_long_rows.test_split_rows_on_a_column_in_segments on cyc_tiny6: rows as 2 x 24, the column as three
    segments of 12, 12, 11 rows; the true reference's snapshots and per-call vectors at the bars of
    test_whole_steps_vs_reference and test_ocinvq; two Thomas launches per step beside the split's."""
    name = "cyc_tiny6"
    cfg = preset(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", "2")
    monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", "16")
    for check in (ocinvq_vs_reference, whole_steps_vs_reference):
        m = OceanModel(cfg)
        try:
            assert m.row_plan() == (2, 24) and [n for _, n in m.thomas_plan()] == [12, 12, 11]
            done = check(m, name, name + " split 2, seg 16")
            if done:
                prof = {k: n for k, (_, n) in m.profile_steps(2, s0=done + 1).items() if n}
                assert prof["k_thomas"] == 4 and prof["k_dst_fwd"] == 6 and prof["k_dst_inv"] == 6 and prof["k_constr"] == 2, prof
        finally:
            m.close()


# =====================================================================================================================
# D. a coupled window over an ocean of two and of five layers
# =====================================================================================================================
def coupled_ocean(nlo):
    """cpl_tiny's ocean (49 x 37, its constants and ah4oc) with the layers of common.OCEAN_LAYERS."""
    base = config.preset("cpl_tiny")
    lay = OCEAN_LAYERS[nlo]
    return dataclasses.replace(base, name="cpl_tiny_o%d" % nlo, nlo=nlo, hoc=lay["hoc"], gpoc=lay["gpoc"], ah2oc=(0.0,) * nlo,
                               ah4oc=(base.ah4oc[0],) * nlo)


def coupled_inputs(oc):
    g = load_golden("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    po = synth.gaussian_eddy(oc, noise=1e-3)
    return f, po, np.asfortranarray(0.98 * po), g["in_wekpo"]


def coupled_pair(nlo, share):
    oc, at = coupled_ocean(nlo), config.atmos_preset("cpl_tiny")
    f, po, pom, wek = coupled_inputs(oc)
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(po, pom)
    o.set_forcing(wek, np.zeros_like(wek), np.zeros(nlo - 1))
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("nlo", [2, 5])
@pytest.mark.parametrize("share", [False, True], ids=["one_stream", "share_gpu"])
def test_coupled_window(nlo, share):
    """test_gpu_xforc.test_coupled_window with the ocean at two and at five layers under cpl_tiny's three-layer
    atmosphere, nstr = 3, seven atmospheric steps: the window with xforc=True is bitwise the explicit sequence xforc();
    ocean.steps(1); atmos.steps(k), differs from the window with the forcing held, and every field is finite; the same
    with a CU range on both handles."""
    nstr, n = 3, 7
    res = {}
    for mode in ("window", "explicit", "held"):
        o, a = coupled_pair(nlo, share)
        try:
            if mode == "explicit":
                nt0 = 1
                while nt0 <= n:
                    xforc(o, a)
                    o.steps(1, s0=(nt0 - 1) // nstr + 1)
                    k = min(nstr, n - nt0 + 1)
                    a.steps(k, s0=nt0)
                    nt0 += k
            else:
                coupled_steps(o, a, 1, n, nstr, xforc=(mode == "window"))
            o.sync()
            a.sync()
            res[mode] = [np.array(x) for x in o.get_state()] + [np.array(x) for x in a.get_state()]
            assert all(np.isfinite(x).all() for x in res[mode]) and res[mode][0].shape[2] == nlo
        finally:
            o.close()
            a.close()
    for name, x, y in zip(FIELDS + ("pa", "pam", "qa", "qam"), res["window"], res["explicit"]):
        same_bits(x, y, name)
    assert not np.array_equal(res["window"][0], res["held"][0])  # po: the atmosphere drives the ocean
    assert not np.array_equal(res["window"][4], res["held"][4])  # pa: and is driven by its own stress


@pytest.mark.parametrize("nlo", [2, 5])
def test_coupled_steps_with_held_forcing_vs_oracle(nlo):
    """test_gpu_tall_diagnostics.test_coupled_steps_with_held_forcing_vs_oracle: with the forcing held the two halves
    are independent, so the ocean after the 12 ocean steps of coupled_steps(o, a, 1, 36, 3) is the oracle's after 12
    steps: fields within 1e-10, scalars within 1e-11."""
    oc = coupled_ocean(nlo)
    f, po, pom, wek = coupled_inputs(oc)
    r = make_oracle(oc)
    o = OceanModel(oc)
    a = AtmosModel(config.atmos_preset("cpl_tiny"), ddynat=f["ddynat"])
    try:
        for mod in (r, o):
            mod.set_p(po, pom)
            mod.set_forcing(wek, np.zeros_like(wek), np.zeros(nlo - 1))
        atm_apply(a, f)
        r.steps(1, 12)
        coupled_steps(o, a, 1, 36, 3)
        o.sync()
        a.sync()
        ref = r.get_state()
        errs = {n: relerr(x, y) for n, x, y in zip(FIELDS, o.get_state(), ref)}
        se = scal_err(o, {"s12_scal": r.get_scalars(), "s12_po": ref[0]}, "s12", oc)
        print("nlo %d: 12 ocean steps in a coupled window:" % nlo, errs, "scalars %.3e" % se)
        assert all(v < 1e-10 for v in errs.values()), errs
        assert se < 1e-11
        assert all(np.isfinite(x).all() for x in a.get_state())
    finally:
        o.close()
        a.close()
        r.close()
