"""The diagnostics, xforc and a coupled window on zonally cyclic ocean handles whose rows are split: the
thin channels of test_gpu_long_rows.py, long_cfg(nxto) = (nxto + 1) x 33 x 3 with nxto = 5760 (2 x 2880), 11520
(3 x 3840: the first length whose jet row passes 64 KiB) and 23040 (5 x 4608: an odd P, a jet row past a CU's LDS), and
the split forced on the small basins the true reference pins.  The diagnostic kernels do not read the row plan; what
differs on such a handle is the length of their rows (columns in loops, LDS rows, keys and results past column 8192) and
the launch sequence of steps() they are scheduled into: ten launches per step, unfused inverse rows + k_unpack_cyc, a
stand-alone k_constr_cyc, the averaging step never fused.

Every test is the recipe of an existing test of the 5 km basins with its bars unchanged (named in each docstring); the
other side is the numpy restatement of the pulled state, the device against itself, the C oracle's runs shared in
test_gpu_long_rows.reference(), or the committed goldens of the true reference.  Where a result carries a column number
or depends on columns far along the row the inputs are shaped so that it lies past column 8192 (5104 at nxto = 5760),
and that is asserted on the reference side."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

import numpy_areacfl as na
import numpy_cov as nc
import numpy_qocdiag as nq
import numpy_tavg as nt
import numpy_xforc as nx
import test_gpu_areacfl as t_areacfl
import test_gpu_cov as t_cov
import test_gpu_monitors as t_mon
import test_gpu_qocdiag as t_qod
import test_gpu_slab_diagnostics as t_slab
import test_gpu_tavg as t_tav
from common import FIELDS, atm_apply, bits, load_golden, preset, relerr, same_bits, scal_err
from qgcm_hip import (AtmosModel, OceanModel, config, coupled_steps, hostinit, oml_preset, share_gpu, synth, xforc,
                      xforc_get, xforc_setup)
from qgcm_hip.slab import partition
from test_gpu_long_rows import PLANS, SPLIT_LAUNCHES, TOL_RUN, load, long_cfg, reference

pytestmark = pytest.mark.gpu

CHUNK = 8192   # columns one LDS pass of k_mon_jet holds: the results below depend on columns past it
SINGLE = 5104  # columns one row transform holds (DST_SINGLE_MAXN): every row here is longer
NSKO = 16      # 16 divides nxto and 32: the subsample holds p columns 1, 17, ..., nxto + 1 and p rows 1, 17, 33
LAYER = pytest.mark.parametrize("mixed_layer", [False, True], ids=["no_oml", "oml"])
SPLITS = pytest.mark.parametrize("P", [2, 3, 4])


def past(cfg):
    """The column the asserted locations lie beyond: 8192 where the row has it, else 5104."""
    return CHUNK if cfg.nxpo > CHUNK else SINGLE


def far_eddy(cfg, amp=4.0, dipole=False):
    """The eddy state of the 5 km recipes plus a second, stronger eddy in layer 1 centred on column 0.9 nxto, skewed in
    y: centred on p row 10 (1-based) it falls off over 4 rows to the south and over 1.5 rows to the north, so its largest
    gradient is one T row, and over 6 columns in x, so it has vanished long before the seam.  It is the largest |u| and
    |v| of layer 1, the maximum of po and both extrema of qo, and it moves the zonal sums of its rows.  dipole: a
    negative twin centred on column 0.8 nxto, p row 22 - the minimum of po."""
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    i = np.arange(cfg.nxpo, dtype=np.float64)[:, None]
    j = np.arange(cfg.nypo, dtype=np.float64)[None, :]
    for sign, xc, jc in ((1.0, 0.9, 9.0), (-1.0, 0.8, 21.0))[:2 if dipole else 1]:
        d = j - jc
        po[:, :, 0] += sign * amp * np.exp(-((i - xc * cfg.nxto) / 6.0) ** 2) * np.exp(-(d / np.where(d < 0.0, 4.0, 1.5)) ** 2)
    po[-1, :, :] = po[0, :, :]
    return np.asfortranarray(po)


def jet_of_columns(cfg, po, ncol):
    """ocjpos, ocjval of layer 1 as numpy_monitors forms them (the serial zonal sum, minus its last term), from the
    columns 1 .. ncol of po alone: what a kernel would report that dropped the rest of the row."""
    ug = -(1.0 / (cfg.dxo * cfg.fnot)) * (po[:ncol, 1:, 0] - po[:ncol, :-1, 0])
    uj = np.abs(np.cumsum(ug, axis=0)[-1, :] - ug[-1, :]) / cfg.nxto
    pos, val = 0, 0.0
    for r in range(cfg.nyto):
        if uj[r] > val:
            pos, val = r + 1, uj[r]
    return pos, val


def worst_ratio(got, want, scales):
    """The largest |device - restatement| of the integrals in units of their bar, 1e-12 of the scale (printed, not a bar
    of its own: t_mon.compare asserts)."""
    r = [np.max(np.abs(np.atleast_1d(got[n]) - np.atleast_1d(want[n])) / (t_mon.TOL * np.atleast_1d(scales[n]) + 1e-300))
         for n in want if n not in t_mon.EXACT]
    return float(max(r))


def split_model(name, P, monkeypatch, seg_rows=None):
    """The variables qgcm_hip_set_grid reads, and the plan a handle of preset `name` then has."""
    cfg = preset(name)
    monkeypatch.setenv("QGCM_HIP_ROW_SPLIT", str(P))
    if seg_rows:
        monkeypatch.setenv("QGCM_HIP_THOMAS_SEG_ROWS", str(seg_rows))
    m = OceanModel(cfg)
    try:
        assert m.row_plan() == (P, cfg.nxto // P)
        return len(m.thomas_plan())
    finally:
        m.close()


# 1. ocean monitors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nxto", [5760, 11520, 23040])
@LAYER
@pytest.mark.parametrize("nsteps", [10, 26])
def test_monitors(nxto, mixed_layer, nsteps):
    """test_gpu_monitors.run (test_small_cases' 10 steps, test_averaging_step_reads_the_averaged_levels' 26: the
    unfused k_lf_average here) with the far eddy: the EXACT names bitwise, every integral within 1e-12 of its scale.
    k_mon_jet takes the rows of 11521 and 23041 points in two and three LDS passes; the jet of layer 1 computed from
    the first 8192 (5104) columns alone is another, so a pass dropped or taken out of order fails the bitwise bar."""
    cfg = long_cfg(nxto)
    m, om, f = t_mon.setup(cfg, mixed_layer)
    try:
        assert m.row_plan() == PLANS[nxto]
        po = far_eddy(cfg)
        m.set_p(po, po)
        m.steps(nsteps, s0=1)
        got = m.monitors()
        want, scales = t_mon.reference(m, om, f, mixed_layer)
        cut = jet_of_columns(cfg, m.get_state()[0], past(cfg))
        full = jet_of_columns(cfg, m.get_state()[0], cfg.nxpo)
        print("ocjpos", want["ocjpos"], "device", got["ocjpos"], "ocjval", want["ocjval"], "columns 1..%d alone:" % past(cfg), cut)
        assert set(got) == set(want)
        # the rate terms see po != pom and the entrainment terms a non-zero entoc
        assert np.all(want["ddtkeoc"] != 0.0) and want["pkenoc"] != 0.0 and want["entmoc"] != 0.0
        assert full == (want["ocjpos"][0], want["ocjval"][0]) and want["ocjpos"][0] > 0
        assert cut != full and cut[1] != full[1]
        print("integrals: worst |diff| / bar %.3e" % worst_ratio(got, want, scales))
        t_mon.compare(got, want, scales)
    finally:
        m.close()


@SPLITS
def test_monitors_against_the_reference_with_forced_split(P, monkeypatch):
    """test_gpu_monitors.test_against_the_reference on cyc_tiny (the true reference's own monnc_comp / couroc) with its
    rows split in 2, 3 and 4, at its bars."""
    split_model("cyc_tiny", P, monkeypatch)
    t_mon.test_against_the_reference("cyc_tiny")


# 2. valids / prsamp -----------------------------------------------------------------------------------------------------
def test_valids_and_prsamp_at_23040():
    """test_gpu_valids.test_full_size_after_steps_and_without_mixed_layer with the mixed layer on, so that the sst and
    wekto entries are scanned too: the numbers equal numpy's own min / max of the pulled state, bitwise; the extrema of
    po, qo and sst all lie at columns past 8192.  prsamp (test_gpu_slab_diagnostics.test_prsamp's bars): the centre
    values and the sst extrema bitwise, the layer averages within 1e-12 of the average of the modulus; the centre
    column is 11521."""
    cfg = long_cfg(23040)
    m, om, f = t_mon.setup(cfg, True)
    try:
        po = far_eddy(cfg, amp=2.0, dipole=True)  # (half the amplitude: no layer gets as thin as valids' thkmin)
        m.set_p(po, po)
        sst, sstm = (np.array(x, order="F") for x in m.oml_get_state())
        # (10 K warmer: the convective adjustment (7.13) floors sst at toc(1), and a floor has its minimum everywhere)
        for c, r, v in ((20000, 7, 5.0), (12345, 25, -5.0)):
            sst[c, r] += v
            sstm[c, r] += v
        sst += 10.0
        sstm += 10.0
        m.oml_set_state(sst, sstm)
        m.steps(10, s0=1)
        ok, out = m.valids()
        p, _, q, _ = m.get_state()
        s = m.oml_get_state()[0]
        assert ok
        where = {}
        for n, a in (("po", p), ("qo", q), ("sst", s)):
            where[n] = (np.unravel_index(a.argmin(), a.shape)[0] + 1, np.unravel_index(a.argmax(), a.shape)[0] + 1)
        print("columns of (min, max):", where)
        assert all(c > CHUNK for cc in where.values() for c in cc), where
        assert out[0] == p.min() and out[1] == p.max() and out[2] == q.min() and out[3] == q.max()
        assert out[4] == s.min() and out[5] == s.max()
        assert out[6] == f["wekto"].min() and out[7] == f["wekto"].max()
        rg = 1.0 / np.asarray(cfg.gpoc)
        eta = [rg[k] * (p[:, :, k + 1] - p[:, :, k]) for k in range(cfg.nlo - 1)]
        ht = cfg.hoc[0] - eta[0]
        hi = cfg.hoc[1] - eta[1] + eta[0]
        hb = cfg.hoc[2] + eta[1] - 0.0
        assert (out[8], out[9]) == (ht.min(), ht.max())
        assert (out[10], out[11]) == (hi.min(), hi.max())
        assert (out[12], out[13]) == (hb.min(), hb.max())
        assert np.all(out[14:] == 0.0)
        got = m.prsamp()
        ic, jc = (cfg.nxpo + 1) // 2 - 1, (cfg.nypo + 1) // 2 - 1  # src/q-gcm.F:1974-1975, 0-based
        assert ic + 1 == 11521 > CHUNK
        assert np.array_equal(got["po_centre"], p[ic, jc, :]) and np.array_equal(got["qo_centre"], q[ic, jc, :])
        assert got["sstmin"] == s.min() and got["sstmax"] == s.max()
        w = np.ones(p.shape[:2])
        w[0, :] *= 0.5
        w[-1, :] *= 0.5
        w[:, 0] *= 0.5
        w[:, -1] *= 0.5
        on = 1.0 / (cfg.nxto * cfg.nyto)
        for k, a in (("pavgoc", p), ("qavgoc", q)):
            want = np.einsum("ij,ijk->k", w, a) * on
            print(k, got[k], want, "bound", 1e-12 * t_slab.xintp_abs(a) * on)
            assert np.all(np.abs(got[k] - want) <= 1e-12 * t_slab.xintp_abs(a) * on), k
    finally:
        m.close()


# 3. time averages -------------------------------------------------------------------------------------------------------
@LAYER
def test_tavocn(mixed_layer):
    """test_gpu_tavg.test_full_size_tavocn at nxto = 11520: contributions after 3, 23, 1 and 9 steps (the second
    follows the averaging step 26) against numpy_tavg of the pulled states, bitwise.  The means vary along the columns
    past 8192."""
    cfg = long_cfg(11520)
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, fnetoc=fnet)
    c = nt.consts(cfg.dxo, cfg.fnot, om.ycexp, om.hmoc, om.tsbdy, om.tnbdy, cfg.cyclic, om.sb_hflux, om.nb_hflux)
    m = t_tav.ocean(cfg, mixed_layer)
    try:
        assert m.row_plan() == PLANS[11520]
        S = nt.tavini(cfg.nxpo, cfg.nypo, cfg.nlo)
        for n in (3, 23, 1, 9):
            m.steps(n)
            m.tavocn()
            nt.tavocn(S, t_tav.host_fields(m, cfg.name, mixed_layer, f), c)
        got = m.time_means()
        want = nt.tavout(S)
        assert got["nsumoc"] == 4
        for n in ("sstav", "pocav", "qocav", "uptpoc", "vptpoc"):
            assert want[n].shape[0] > CHUNK and np.ptp(want[n][CHUNK:]) > 0.0, n
        t_tav.same(got, want)
    finally:
        m.close()


def test_po_mean_over_30_steps():
    """test_gpu_tavg.test_po_mean_over_60_steps, 30 steps (steps 1 and 26 average) at nxto = 5760: the sum accumulated
    inside steps(30) against the per-step po of a second handle stepped one at a time (each checked against the state
    after its step: po before the averaging on steps 1 and 26), bitwise; the state bitwise that of a third handle that
    never enabled the sum."""
    cfg = long_cfg(5760)
    a, b, c = (t_tav.ocean(cfg, False) for _ in range(3))
    try:
        assert a.row_plan() == PLANS[5760]
        a.enable_po_mean()
        a.steps(30, s0=1)
        mean, n = a.po_mean(count=True)
        assert n == 30
        b.enable_po_mean()
        tot = t_tav.per_step_po(b, 1, 30)
        assert np.ptp(tot[SINGLE:]) > 0.0
        assert np.array_equal(mean, nt.po_mean(tot, 30))
        assert np.array_equal(mean, a.po_mean())  # reading without reset keeps the sum
        c.steps(30, s0=1)
        for h in (b, c):
            for name, x, y in zip(FIELDS, a.get_state(), h.get_state()):
                same_bits(x, y, name)
    finally:
        for m in (a, b, c):
            m.close()


def test_po_mean_launches():
    """test_gpu_tavg.test_launch_sequence_unchanged_when_never_enabled on the split step: k_poavg_add once per step, the
    launches of the split row family (SPLIT_LAUNCHES) per step, and the sum changes no other count (k_lf_average is a
    launch of its own on a split handle with or without it)."""
    cfg = long_cfg(5760)
    off_m, on_m = t_tav.ocean(cfg, False), t_tav.ocean(cfg, False)
    try:
        off = off_m.profile_steps(30, s0=1)
        on_m.enable_po_mean()
        on = on_m.profile_steps(30, s0=1)
        print({k: (off[k][1], on[k][1]) for k in off if off[k][1] or on[k][1]})
        assert off["k_poavg_add"][1] == 0 and on["k_poavg_add"][1] == 30
        for k, n in SPLIT_LAUNCHES.items():
            assert on[k][1] == off[k][1] == 30 * n, k
        assert on["k_lf_average"][1] == off["k_lf_average"][1] == 2
        for k in off:
            if k not in ("k_poavg_add", "k_noop_train"):
                assert on[k][1] == off[k][1], k
    finally:
        off_m.close()
        on_m.close()


# 4. periodic dumps ------------------------------------------------------------------------------------------------------
@LAYER
def test_dumps(mixed_layer):
    """test_gpu_qocdiag.test_full_size at nxto = 11520: vorticity_budget() at nsko = 1 (every column) and 16 (columns 1,
    17, ..., 11521: 209 of the 721 lie past 8192) and ocean_dump(16) after 26 steps against numpy_qocdiag of the pulled
    state, bitwise."""
    cfg = long_cfg(11520)
    cols = np.arange(1, cfg.nxpo + 1, NSKO)  # 1-based p columns of the subsample
    assert len(cols) == 721 and cols[-1] == cfg.nxpo and (cols > CHUNK).sum() == 209
    m, om, f = t_mon.setup(cfg, mixed_layer)
    try:
        po = far_eddy(cfg)
        m.set_p(po, po)
        m.steps(26, s0=1)  # steps 1 and 26 average
        for nsko in (1, NSKO):
            got = m.vorticity_budget(nsko)
            assert got["dqdt"].shape == ((cfg.nlo, 3, 721) if nsko == NSKO else (cfg.nlo, cfg.nypo, cfg.nxpo))
            want = t_qod.restated(m, f, mixed_layer, nsko)
            assert np.ptp(want["dqdt"][..., (CHUNK // nsko) + 1:]) > 0.0
            t_qod.same(got, want)
        po, _, qo, _ = m.get_state()
        sst = m.oml_get_state()[0] if mixed_layer else f["sst"]
        want = nq.ocnc(sst, po, qo, f["wekto"], f["tauxo"], f["tauyo"], cfg.gpoc, NSKO)
        got = m.ocean_dump(NSKO)
        assert sorted(got) == sorted(want)
        for n in want:
            w = want[n][0] if n in t_qod.FLAT else want[n]
            assert got[n].shape == w.shape and np.array_equal(got[n], w), n
        assert got["po"].shape == (cfg.nlo, 3, 721) and np.array_equal(got["po"][:, :, -1], po[-1, ::NSKO, :].T)
    finally:
        m.close()


def test_scheduled_dump_without_mixed_layer_equals_between_steps():
    """The test of that name in test_gpu_qocdiag, inside steps(30) at nxto = 5760: snapshots at steps 1, 10, 19 and 28
    (the last after the averaging step 26) equal the budgets a twin takes between single calls of steps()."""
    cfg = long_cfg(5760)
    a, _, _ = t_mon.setup(cfg, False)
    b, _, _ = t_mon.setup(cfg, False)
    try:
        a.schedule_vorticity_budget(NSKO, 9, capacity=4)
        a.steps(30, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 10, 19, 28]
        assert a.read_vorticity_budgets() == []
        assert snaps[0][1]["dqdt"].shape == (cfg.nlo, 3, 361) and np.ptp(snaps[3][1]["dqdt"][..., SINGLE // NSKO + 1:]) > 0.0
        for k, (s0, n) in enumerate(((1, 0), (1, 9), (10, 9), (19, 9))):
            b.steps(n, s0=s0)
            t_qod.same(snaps[k][1], b.vorticity_budget(NSKO))
    finally:
        a.close()
        b.close()


def test_scheduled_dump_is_taken_after_oml():
    """The test of that name in test_gpu_qocdiag at nxto = 5760: the snapshot of step 26 equals a twin stepped to 25 that
    calls oml() then vorticity_budget(), and differs from the budget between steps."""
    cfg = long_cfg(5760)
    a, _, _ = t_mon.setup(cfg, True)
    b, _, _ = t_mon.setup(cfg, True)
    try:
        a.schedule_vorticity_budget(NSKO, 25, capacity=2)
        a.steps(30, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 26]
        b.steps(25, s0=1)
        between = b.vorticity_budget(NSKO)
        b.oml()
        t_qod.same(snaps[1][1], b.vorticity_budget(NSKO))
        assert not np.array_equal(snaps[1][1]["qotent"], between["qotent"])
    finally:
        a.close()
        b.close()


@LAYER
def test_schedule_leaves_the_state_bitwise(mixed_layer):
    """The test of that name in test_gpu_qocdiag over 30 steps at nxto = 5760: the graph blocks with the dump's launches
    among the ten of a split step leave the bits of a handle that has no schedule."""
    cfg = long_cfg(5760)
    a, _, _ = t_mon.setup(cfg, mixed_layer)
    b, _, _ = t_mon.setup(cfg, mixed_layer)
    try:
        a.schedule_vorticity_budget(NSKO, 25, capacity=2)
        a.prepare_steps(30, s0=1)
        a.steps(30, s0=1)
        b.steps(30, s0=1)
        assert [s for s, _ in a.read_vorticity_budgets()] == [1, 26]
        for name, x, y in zip(FIELDS, a.get_state(), b.get_state()):
            same_bits(x, y, name)
        if mixed_layer:
            for x, y in zip(a.oml_get_state(), b.oml_get_state()):
                same_bits(x, y, "sst")
    finally:
        a.close()
        b.close()


# 5. covariances -----------------------------------------------------------------------------------------------------------
@LAYER
def test_covariance(mixed_layer):
    """test_gpu_cov.test_full_size_ocean at nxto = 5760 with nsi = 16 (nvar = 360 x 2 = 720: the boxes of a subsampled
    row span the whole length, 41 of them past column 5104): contributions after 3, 22, 1 and 9 steps (the third follows
    the averaging step 26) against numpy_cov of the pulled po and sst, bitwise; the state untouched."""
    cfg = long_cfg(5760)
    m = t_tav.ocean(cfg, mixed_layer)
    sst = synth.mixed_layer_fields(cfg, oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer), seed=5)[0]
    try:
        assert m.row_plan() == PLANS[5760]
        m.enable_covariance(NSKO)
        nvar = 360 * 2
        assert m.covariance_size()["nvar"] == nvar == (cfg.nxto // NSKO) * (cfg.nyto // NSKO)
        assert (np.arange(360) * NSKO + 1 > SINGLE).sum() == 41
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        before = None
        for n in (3, 22, 1, 9):
            m.steps(n)
            before = [a.copy() for a in m.get_state()]
            m.covocn()
            nc.covocn(*t_cov.pulled(m, mixed_layer, sst), NSKO, ap, at)
        for x, y in zip(before, m.get_state()):
            assert np.array_equal(x, y)
        want = t_cov.restated(ap, at, t_cov.OCN)
        assert np.ptp(want["avgpo"][320:360]) > 0.0  # the first row's boxes past column 5104 (ivs = (js-1) 360 + is)
        t_cov.same(m.covariance(), want)
    finally:
        m.close()


def test_covariance_schedule_equals_explicit_calls():
    """test_gpu_cov.test_schedule_equals_explicit_calls inside steps(30) at nxto = 5760: schedule_covariance(25, 1) adds
    after steps 1 and 26, both averaging steps."""
    cfg = long_cfg(5760)
    a, b = t_tav.ocean(cfg, True), t_tav.ocean(cfg, True)
    try:
        for m in (a, b):
            m.enable_covariance(NSKO)
        a.schedule_covariance(25, 1)
        a.steps(30, s0=1)
        b.steps(0, s0=1)
        for n in (1, 25):
            b.steps(n)
            b.covocn()
        b.steps(4)
        ca, cb = a.covariance(), b.covariance()
        assert ca["nupo"] == cb["nupo"] == 2
        t_cov.same(ca, cb)
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(a.oml_get_state()[0], b.oml_get_state()[0])
    finally:
        a.close()
        b.close()


@SPLITS
def test_covariance_against_the_reference_with_forced_split(P, monkeypatch):
    """test_gpu_cov.test_against_the_reference on cyc_tiny (tests/golden/cov_cyc_tiny_4.npz, the true reference's
    covocn) with its rows split, bitwise."""
    split_model("cyc_tiny", P, monkeypatch)
    t_cov.test_against_the_reference(os.path.join(t_cov.GOLD, "cov_cyc_tiny_4.npz"))


# 6. area averages and CFL -----------------------------------------------------------------------------------------------
def test_area_averages_follow_the_sst_rotation():
    """The test of that name in test_gpu_areacfl at nxto = 23040, with areas placed by the columns: the basin, one whose
    western and eastern edges lie either side of column 8192 and one wholly past it."""
    cfg = long_cfg(23040)
    m, om, f = t_mon.setup(cfg, True)
    try:
        x, y = cfg.xlo, cfg.ylo
        T = m.set_areas([0.0, 0.3 * x, 0.4 * x], [x, 0.5 * x, 0.9 * x], [0.0, 0.22 * y, 0.5 * y], [y, 0.83 * y, y])
        print("T columns of the areas:", list(zip(T["i1"], T["i2"])))
        assert T["i1"][1] < CHUNK < T["i2"][1]
        assert T["i1"][2] > CHUNK and T["i2"][2] > 2 * CHUNK
        before = m.area_averages()
        m.steps(30, s0=1)
        got = m.area_averages(parts=True)
        assert not np.array_equal(before, got[0])
        t_areacfl.check_areas(cfg.name + " stepped", got, m.oml_get_state()[0], T)
        assert np.array_equal(bits(m.area_averages()), bits(got[0]))
    finally:
        m.close()


def test_cfl_of_a_stepped_handle():
    """The test of that name in test_gpu_areacfl at nxto = 23040 with the far eddy: the criterion at half the largest
    Courant number, so offenders exist; maxima, counts and locations exactly the restatement's.  The keys of the maxima
    are (j-1) nx + (i-1): those of layer 1 carry columns past 16384."""
    cfg = long_cfg(23040)
    m, om, f = t_mon.setup(cfg, True)
    try:
        po = far_eddy(cfg)
        m.set_p(po, po)
        m.steps(30, s0=1)
        po = m.get_state()[0]
        kw = dict(rdxf0=1.0 / (cfg.dxo * cfg.fnot), dt=cfg.dto, dx=cfg.dxo, rhf0hm=0.5 / (cfg.fnot * om.hmoc))
        crit = 0.5 * na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=0.8, **kw)["courant"].max()
        want = na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=crit, **kw)
        assert want["nbad"].sum() > 0
        cols = dict(zip(want["names"], want["loc"][:, 0]))
        assert cols["u1"] > 2 * CHUNK and cols["v1"] > 2 * CHUNK, cols
        assert want["bad"][:, 1].max() > 2 * CHUNK  # offenders too
        t_areacfl.check_cfl(cfg.name + " stepped", m.cfl(crit), want)
    finally:
        m.close()


# 7. xforc and a coupled window ------------------------------------------------------------------------------------------
def coupled_cfgs():
    """The 5761 x 33 x 3 channel under its own 361 x 9 x 3 atmosphere (ndxr = 16: inside xforc_init's ndxr <= 64); the
    ocean spans the atmosphere's length and sits at ny1 = 4."""
    oc = long_cfg(5760)
    r = oc.ndxr * oc.dxo / 8.0e4
    at = config.atmos_of(oc, ah4at=(1.5e14 * r ** 4,) * 3)  # as config.atmos_preset scales it
    assert (oc.nxpo, oc.nypo, at.nxpa, at.nypa) == (5761, 33, 361, 9)
    return oc, at


def test_xforc_pointwise():
    """test_gpu_xforc.test_golden against numpy_xforc itself (the CPU suite holds it to the reference bit for bit):
    every pointwise field by integer view, the four line integrals within 2 n 2^-53 sum|terms| dxo, a second call
    identical.  The ocean's fields have 5761 columns; tau_udiff reads the ocean's pressure, the far eddy past column
    5104, under the atmosphere's."""
    oc, at = coupled_cfgs()
    P = dict(nxta=oc.nxta, nyta=oc.nyta, nxaooc=oc.nxaooc, nyaooc=oc.nyaooc, ndxr=oc.ndxr, nx1=1, ny1=4, cyclic=1,
             tau_udiff=1, fnot=oc.fnot, dxo=oc.dxo, cdat=1.3e-3, raoro=1.0e-3, hmat=1000.0, hmoc=100.0,
             bccoat=at.bccoat, bccooc=oc.bccooc)
    pam1 = synth.atmos_fields(at)["pam"][:, :, 0]
    pom1 = far_eddy(oc)[:, :, 0]
    tabs = hostinit.bcuini(oc.ndxr, at.bccoat, at.dya)
    N = nx.xforc(pam1, pom1, tabs, P)
    quiet = nx.xforc(pam1, synth.gaussian_eddy(oc, noise=1e-3)[:, :, 0], tabs, P)
    where = np.argwhere(N["tauxo"] != quiet["tauxo"])[:, 0]
    assert where.size and where.min() + 1 > SINGLE  # what the far eddy changes lies past column 5104
    o, a = OceanModel(oc), AtmosModel(at)
    try:
        assert o.row_plan() == PLANS[5760]
        xforc_setup(o, a, cdat=P["cdat"], rhoat=P["raoro"], rhooc=1.0, hmat=P["hmat"], hmoc=P["hmoc"], tau_udiff=True)
        assert a.xforc_origin == (P["nx1"], P["ny1"])
        for mod, fld in ((a, pam1), (o, pom1)):  # both time levels, the other layers zero (test_gpu_xforc._load_state)
            p = np.zeros(fld.shape + (3,), order="F")
            p[:, :, 0] = fld
            mod.set_state(po=p, pom=p)
        xforc(o, a)
        R = xforc_get(o, a)
        xforc(o, a)
        R2 = xforc_get(o, a)
        for f in nx.POINTWISE:
            assert R[f].shape == N[f].shape, f
            same_bits(R[f], N[f], f)
            same_bits(R[f], R2[f], f + ", second call")
            assert np.any(N[f] != 0.0), f
        for f in nx.INTEGRALS:
            bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * P["dxo"]
            print("%s: device %.17e restatement %.17e |diff| %.3e bound %.3e" % (f, R[f], N[f], abs(R[f] - N[f]), bound))
            assert abs(R[f] - N[f]) <= bound, (f, R[f], N[f], bound)
            assert R[f] == R2[f], f
            assert N[f] != 0.0
    finally:
        o.close()
        a.close()


def coupled_pair(share):
    oc, at = coupled_cfgs()
    f = synth.atmos_fields(at)
    po = synth.gaussian_eddy(oc, noise=1e-3)
    tx, ty = synth.wind_stress(oc)
    _, wek = synth.wekpo_from_tau(oc, tx, ty)
    o = OceanModel(oc)
    a = AtmosModel(at, ddynat=f["ddynat"])
    o.set_p(po, np.asfortranarray(0.98 * po))
    o.set_forcing(wek, np.zeros_like(wek), np.zeros(oc.nlo - 1))
    o.set_cyc_forcing(*synth.tau_line_integrals(oc, tx))
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("share", [False, True])
def test_coupled_window(share):
    """test_gpu_xforc.test_coupled_window with the split ocean, nstr = 3, seven atmospheric steps: the window with
    xforc=True is bitwise the explicit sequence xforc(); ocean.steps(1); atmos.steps(k), differs from the window with
    the forcing held, and every field is finite; the same with a CU range on both handles."""
    nstr, n = 3, 7
    res = {}
    for mode in ("window", "explicit", "held"):
        o, a = coupled_pair(share)
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
            assert all(np.isfinite(x).all() for x in res[mode])
        finally:
            o.close()
            a.close()
    for name, x, y in zip(FIELDS + ("pa", "pam", "qa", "qam"), res["window"], res["explicit"]):
        same_bits(x, y, name)
    assert not np.array_equal(res["window"][0], res["held"][0])  # po: the atmosphere drives the ocean
    assert not np.array_equal(res["window"][4], res["held"][4])  # pa: and is driven by its own stress
    assert not np.array_equal(res["window"][0][SINGLE:], res["held"][0][SINGLE:])  # ... past column 5104 too


def test_coupled_steps_with_held_forcing_vs_oracle():
    """The split step inside the coupled capture against the oracle: with the forcing held the two halves are
    independent, so the channel of reference(long_cfg(5760)) under the cpl_tiny atmosphere is, after the 12 ocean steps
    of coupled_steps(o, a, 1, 36, 3), the oracle's state after 12 steps - the bars of
    test_gpu_long_rows.test_long_rows_twelve_steps_vs_oracle."""
    r = reference(long_cfg(5760))
    cfg = r["cfg"]
    g = load_golden("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    o = OceanModel(cfg)
    a = AtmosModel(config.atmos_preset("cpl_tiny"), ddynat=f["ddynat"])
    try:
        assert o.row_plan() == PLANS[5760]
        load(o, r)
        atm_apply(a, f)
        coupled_steps(o, a, 1, 36, 3)
        o.sync()
        a.sync()
        errs = {n: relerr(x, y) for n, x, y in zip(FIELDS, o.get_state(), r["end"])}
        se = scal_err(o, {"s12_scal": r["end_scal"], "s12_po": r["end"][0]}, "s12", cfg)
        print("12 ocean steps in a coupled window:", errs, "scalars %.3e" % se)
        assert np.ptp(r["end"][0][SINGLE:]) > 0.0
        assert all(v < TOL_RUN for v in errs.values()), errs
        assert se < 1e-11
        assert all(np.isfinite(x).all() for x in a.get_state())
    finally:
        o.close()
        a.close()


# 8. split rows and a column in segments together ------------------------------------------------------------------------
@LAYER
def test_monitors_on_split_rows_and_a_column_in_segments(mixed_layer, monkeypatch):
    """test_gpu_monitors.test_small_cases on cyc_small with its rows as 2 x 48 and its column in four segments (SOcn
    1 km needs both), at its bars."""
    assert split_model("cyc_small", 2, monkeypatch, seg_rows=20) == 4
    got, want = t_mon.run("cyc_small", 10, mixed_layer)
    assert np.all(want["ddtkeoc"] != 0.0) and want["pkenoc"] != 0.0 and want["entmoc"] != 0.0


def test_scheduled_dump_on_split_rows_and_a_column_in_segments(monkeypatch):
    """test_gpu_qocdiag.test_scheduled_dump_is_taken_after_oml on cyc_small with split rows and a segmented column."""
    assert split_model("cyc_small", 2, monkeypatch, seg_rows=20) == 4
    a, _, _ = t_mon.setup("cyc_small", True)
    b, _, _ = t_mon.setup("cyc_small", True)
    try:
        assert a.row_plan() == (2, 48) and len(a.thomas_plan()) == 4
        a.schedule_vorticity_budget(2, 25, capacity=2)
        a.steps(26, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 26]
        assert a.read_vorticity_budgets() == []
        b.steps(25, s0=1)
        between = b.vorticity_budget(2)
        b.oml()
        t_qod.same(snaps[1][1], b.vorticity_budget(2))
        assert not np.array_equal(snaps[1][1]["qotent"], between["qotent"])
    finally:
        a.close()
        b.close()


# 9. y-slabs -------------------------------------------------------------------------------------------------------------
def test_monitors_whole_handle_vs_three_y_slabs():
    """test_gpu_slab_diagnostics.test_full_size at nxto = 11520 on three virtual y-slabs of 11 rows (monitors_part on
    each, one gather, monitors_combine; k_mon_jet is shared with the whole handle): against the whole handle and the
    restatement, the EXACT names bitwise, every integral within 1e-12 of its scale."""
    cfg = long_cfg(11520)
    m, om, f = t_mon.setup(cfg, False)
    try:
        po = far_eddy(cfg)
        m.set_p(po, po)
        m.steps(10, s0=1)
        whole = m.monitors()
        want, scales = t_mon.reference(m, om, f, False)
        full = (want["ocjpos"][0], want["ocjval"][0])
        assert jet_of_columns(cfg, m.get_state()[0], CHUNK) != full and full[0] > 0
        t_mon.compare(whole, want, scales)
        parts = partition(cfg.nypo, 3)
        assert [g1 - g0 + 1 for g0, g1 in parts] == [11, 11, 11]
        so = t_slab.slabs_like(m, om, f, False, parts)
        try:
            assert all(x.row_plan() == PLANS[11520] for x in so.slabs)
            got = so.monitors()
            print("integrals: worst |diff| / bar, slabs vs whole %.3e, slabs vs restatement %.3e" % (
                worst_ratio(got, whole, scales), worst_ratio(got, want, scales)))
            t_mon.compare(got, whole, scales)
            t_mon.compare(got, want, scales)
        finally:
            t_slab.close(so)
    finally:
        m.close()
