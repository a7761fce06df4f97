"""The diagnostics, xforc and a coupled window on whole-domain ocean handles whose column is cut into segments
(DESIGN 3.3b): the 2053-row basins of test_gpu_tall_columns.py, tall_cfg(171) (49 x 2053 x 3, three segments of 684 /
684 / 683 rows) and its cyclic twin.  The diagnostic kernels do not read the segment plan; what differs on such a handle
is their launch geometry (rows in a grid dimension, row loops, row numbers in keys and results past 2048) and the launch
sequence of steps() they are scheduled into: five launches per step with two Thomas launches, part A of the cyclic
constraint algebra as a launch of its own, the averaging step never fused.

Every test is the recipe of an existing test of the 5 km basins with its bars unchanged (named in each docstring); the
other side is the numpy restatement of the pulled state, the device against itself, or the C oracle's runs shared in
test_gpu_tall_columns.reference().  Where a result carries a row number the inputs are shaped so that it lies above row
2048, and that is asserted on the reference side."""
import dataclasses

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
import test_gpu_tavg as t_tav
from common import FIELDS, atm_apply, bits, load_golden, relerr, same_bits, scal_err
from qgcm_hip import (AtmosModel, OceanModel, config, coupled_steps, hostinit, lib, oml_preset, share_gpu, synth, xforc,
                      xforc_get, xforc_setup)
from test_gpu_tall_columns import TOL_RUN, load_box, reference, tall_cfg

pytestmark = pytest.mark.gpu

LIMIT = 2048  # rows one Thomas segment holds: the columns below are the first past it
NSKO = 12     # 12 divides 48 and 2052: the subsample holds p rows 1, 13, ..., 2053 and T rows 1, 13, ..., 2041
BASINS = pytest.mark.parametrize("cyclic", [False, True], ids=["box", "cyclic"])
LAYER = pytest.mark.parametrize("mixed_layer", [False, True], ids=["no_oml", "oml"])


def seams(cfg):
    """1-based p rows at which a segment of the handle's column ends (interior row r is p row r + 1)."""
    plan = lib.thomas_segments(cfg.nypo - 2)
    assert cfg.nypo == 2053 and [n for _, n in plan] == [684, 684, 683]
    return [first + n + 1 for first, n in plan[:-1]]


def northern_eddy(cfg):
    """The eddy state of the 5 km recipes plus a second, stronger eddy in layer 1 next to the northern wall, skewed:
    centred on p row 2049 (1-based) it falls off over 8 rows to the south and over 1.5 rows to the north, so the largest
    gradient of the basin is its northern flank, between p rows 2050 and 2051 = T row 2050, and the eddy has vanished
    (8 e^-7) at the wall, where a box holds p constant.  Its zonal-mean flank is twice the jet that the mixed layer's
    boundary fluxes raise along that wall in 30 steps (T row 2052: the oracle's mixed layer gives 0.047 m/s against
    0.089).  The jet position and the CFL locations of layer 1 are then row numbers above 2048 and below the last row."""
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    i = np.arange(cfg.nxpo, dtype=np.float64)[:, None]
    d = np.arange(cfg.nypo, dtype=np.float64)[None, :] - 2048.0
    po[:, :, 0] += 8.0 * np.exp(-((i - 0.4 * cfg.nxto) / 6.0) ** 2) * np.exp(-(d / np.where(d < 0.0, 8.0, 1.5)) ** 2)
    if cfg.cyclic:
        po[-1, :, :] = po[0, :, :]
    return np.asfortranarray(po)


# 1. ocean monitors ------------------------------------------------------------------------------------------------------
@BASINS
@LAYER
@pytest.mark.parametrize("nsteps", [10, 26])
def test_monitors(cyclic, mixed_layer, nsteps):
    """test_gpu_monitors.run (test_small_cases' 10 steps, test_averaging_step_reads_the_averaged_levels' 26: the
    unfused k_lf_average here) with the northern eddy: the EXACT names bitwise, every integral within 1e-12 of its
    scale.  k_mon_jet's grid is (owned T rows, nl): 2052 rows; ocjpos of layer 1 is a row above 2048."""
    cfg = tall_cfg(171, cyclic)
    m, om, f = t_mon.setup(cfg, mixed_layer)
    try:
        po = northern_eddy(cfg)
        m.set_p(po, po)
        m.steps(nsteps, s0=1)
        got = m.monitors()
        want, scales = t_mon.reference(m, om, f, mixed_layer)
        print("ocjpos", want["ocjpos"], "device", got["ocjpos"], "ocjval", want["ocjval"])
        assert set(got) == set(want)
        # the rate terms see po != pom and the entrainment terms a non-zero entoc
        assert np.all(want["ddtkeoc"] != 0.0) and want["pkenoc"] != 0.0 and want["entmoc"] != 0.0
        assert LIMIT < want["ocjpos"][0] < cfg.nyto
        t_mon.compare(got, want, scales)
    finally:
        m.close()


# 2. time averages -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cyclic,mixed_layer", [(False, False), (False, True), (True, False)],
                         ids=["box", "box_oml", "cyclic"])
def test_tavocn(cyclic, mixed_layer):
    """test_gpu_tavg.test_full_size_tavocn: contributions after 3, 23, 1 and 9 steps (the second follows the averaging
    step 26) against numpy_tavg of the pulled states, bitwise.  k_tav_accum and k_tav_mean have the rows in grid.y."""
    cfg = tall_cfg(171, cyclic)
    om = oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer)
    sst, _, fnet, tx, ty = synth.mixed_layer_fields(cfg, om, seed=5)
    wekto, wekpo = synth.wekpo_from_tau(cfg, tx, ty)
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wekpo, fnetoc=fnet)
    c = nt.consts(cfg.dxo, cfg.fnot, om.ycexp, om.hmoc, om.tsbdy, om.tnbdy, cfg.cyclic, om.sb_hflux, om.nb_hflux)
    m = t_tav.ocean(cfg, mixed_layer)
    try:
        S = nt.tavini(cfg.nxpo, cfg.nypo, cfg.nlo)
        for n in (3, 23, 1, 9):
            m.steps(n)
            m.tavocn()
            nt.tavocn(S, t_tav.host_fields(m, cfg.name, mixed_layer, f), c)
        got = m.time_means()
        assert got["nsumoc"] == 4
        t_tav.same(got, nt.tavout(S))
    finally:
        m.close()


@BASINS
def test_po_mean_over_30_steps(cyclic):
    """test_gpu_tavg.test_po_mean_over_60_steps, 30 steps (steps 1 and 26 average): the sum accumulated inside
    steps(30) against the per-step po of a second handle stepped one at a time (each checked against the state after
    its step: po before the averaging on steps 1 and 26), bitwise; the state bitwise that of a third handle that never
    enabled the sum."""
    cfg = tall_cfg(171, cyclic)
    a, b, c = (t_tav.ocean(cfg, False) for _ in range(3))
    try:
        a.enable_po_mean()
        a.steps(30, s0=1)
        mean, n = a.po_mean(count=True)
        assert n == 30
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


@BASINS
def test_po_mean_launches(cyclic):
    """test_gpu_tavg.test_launch_sequence_unchanged_when_never_enabled on the segmented step: k_poavg_add once per
    step, two Thomas launches per step, and the sum changes no other count (k_lf_average is a launch of its own on a
    tall handle with or without it)."""
    cfg = tall_cfg(171, cyclic)
    off_m, on_m = t_tav.ocean(cfg, False), t_tav.ocean(cfg, False)
    try:
        off = off_m.profile_steps(30, s0=1)
        on_m.enable_po_mean()
        on = on_m.profile_steps(30, s0=1)
        print({k: (off[k][1], on[k][1]) for k in off if off[k][1] or on[k][1]})
        assert off["k_poavg_add"][1] == 0 and on["k_poavg_add"][1] == 30
        assert on["k_thomas"][1] == 60 and off["k_thomas"][1] == 60
        assert on["k_lf_average"][1] == off["k_lf_average"][1] == 2
        for k in off:
            if k not in ("k_poavg_add", "k_noop_train"):
                assert on[k][1] == off[k][1], k
    finally:
        off_m.close()
        on_m.close()


# 3. periodic dumps ------------------------------------------------------------------------------------------------------
@BASINS
@LAYER
def test_dumps(cyclic, mixed_layer):
    """test_gpu_qocdiag.test_full_size: vorticity_budget() at nsko = 1 (every row) and 12 (rows 1, 13, ..., 2053) and
    ocean_dump(12) after 26 steps against numpy_qocdiag of the pulled state, bitwise."""
    cfg = tall_cfg(171, cyclic)
    rows = np.arange(1, cfg.nypo + 1, NSKO)  # 1-based p rows of the subsample
    assert len(rows) == 172 and rows[-1] == cfg.nypo == 2053 and rows[-1] > LIMIT
    m, om, f = t_mon.setup(cfg, mixed_layer)
    try:
        m.steps(26, s0=1)  # steps 1 and 26 average
        for nsko in (1, NSKO):
            got = m.vorticity_budget(nsko)
            assert got["dqdt"].shape == ((cfg.nlo, 172, 5) if nsko == NSKO else (cfg.nlo, cfg.nypo, cfg.nxpo))
            t_qod.same(got, t_qod.restated(m, f, mixed_layer, nsko))
        po, _, qo, _ = m.get_state()
        sst = m.oml_get_state()[0] if mixed_layer else f["sst"]
        want = nq.ocnc(sst, po, qo, f["wekto"], f["tauxo"], f["tauyo"], cfg.gpoc, NSKO)
        got = m.ocean_dump(NSKO)
        assert sorted(got) == sorted(want)
        for n in want:
            w = want[n][0] if n in t_qod.FLAT else want[n]
            assert got[n].shape == w.shape and np.array_equal(got[n], w), n
        assert got["po"].shape == (cfg.nlo, 172, 5) and np.array_equal(got["po"][:, -1, :], po[::NSKO, -1, :].T)
    finally:
        m.close()


@BASINS
def test_scheduled_dump_without_mixed_layer_equals_between_steps(cyclic):
    """The test of that name in test_gpu_qocdiag, inside steps(30): snapshots at steps 1, 10, 19 and 28 (the last after
    the averaging step 26) equal the budgets a twin takes between single calls of steps()."""
    cfg = tall_cfg(171, cyclic)
    a, _, _ = t_mon.setup(cfg, False)
    b, _, _ = t_mon.setup(cfg, False)
    try:
        a.schedule_vorticity_budget(NSKO, 9, capacity=4)
        a.steps(30, s0=1)
        snaps = a.read_vorticity_budgets()
        assert [s for s, _ in snaps] == [1, 10, 19, 28]
        assert a.read_vorticity_budgets() == []
        for k, (s0, n) in enumerate(((1, 0), (1, 9), (10, 9), (19, 9))):
            b.steps(n, s0=s0)
            t_qod.same(snaps[k][1], b.vorticity_budget(NSKO))
    finally:
        a.close()
        b.close()


@BASINS
def test_scheduled_dump_is_taken_after_oml(cyclic):
    """The test of that name in test_gpu_qocdiag: the snapshot of step 26 equals a twin stepped to 25 that calls oml()
    then vorticity_budget(), and differs from the budget between steps."""
    cfg = tall_cfg(171, cyclic)
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


@BASINS
@LAYER
def test_schedule_leaves_the_state_bitwise(cyclic, mixed_layer):
    """The test of that name in test_gpu_qocdiag over 30 steps: the graph blocks with the dump's launches among the
    five of a segmented step leave the bits of a handle that has no schedule."""
    cfg = tall_cfg(171, cyclic)
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


# 4. covariances -----------------------------------------------------------------------------------------------------------
@BASINS
@LAYER
def test_covariance(cyclic, mixed_layer):
    """test_gpu_cov.test_full_size_ocean with nsi = 12 (nvar = 4 x 171 = 684): contributions after 3, 22, 1 and 9 steps
    (the third follows the averaging step 26) against numpy_cov of the pulled po and sst, bitwise; the state untouched."""
    cfg = tall_cfg(171, cyclic)
    m = t_tav.ocean(cfg, mixed_layer)
    sst = synth.mixed_layer_fields(cfg, oml_preset(cfg, sb_hflux=mixed_layer, nb_hflux=mixed_layer), seed=5)[0]
    try:
        m.enable_covariance(NSKO)
        nvar = 4 * 171
        assert m.covariance_size()["nvar"] == nvar == (cfg.nxto // NSKO) * (cfg.nyto // NSKO)
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        before = None
        for n in (3, 22, 1, 9):
            m.steps(n)
            before = [a.copy() for a in m.get_state()]
            m.covocn()
            nc.covocn(*t_cov.pulled(m, mixed_layer, sst), NSKO, ap, at)
        for x, y in zip(before, m.get_state()):
            assert np.array_equal(x, y)
        t_cov.same(m.covariance(), t_cov.restated(ap, at, t_cov.OCN))
    finally:
        m.close()


@BASINS
def test_covariance_schedule_equals_explicit_calls(cyclic):
    """test_gpu_cov.test_schedule_equals_explicit_calls inside steps(30): schedule_covariance(25, 1) adds after steps 1
    and 26, both averaging steps."""
    cfg = tall_cfg(171, cyclic)
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


# 5. area averages and CFL -----------------------------------------------------------------------------------------------
@BASINS
def test_area_averages_follow_the_sst_rotation(cyclic):
    """The test of that name in test_gpu_areacfl, with areas placed by the segments: the basin, one whose southern and
    northern edges lie in different segments (it spans the middle one) and one wholly above row 2048."""
    cfg = tall_cfg(171, cyclic)
    m, om, f = t_mon.setup(cfg, True)
    try:
        x, y, d = cfg.xlo, cfg.ylo, cfg.dyo
        T = m.set_areas([0.0, 0.13 * x, 0.4 * x], [x, 0.71 * x, 0.9 * x], [0.0, 0.22 * y, 2049.5 * d],
                        [y, 0.83 * y, y])
        s1, s2 = seams(cfg)
        print("T rows of the areas:", list(zip(T["j1"], T["j2"])), "segments end at p rows", s1, s2)
        assert T["j1"][1] < s1 and s2 < T["j2"][1]
        assert T["j1"][2] > LIMIT and T["j2"][2] == cfg.nyto
        before = m.area_averages()
        m.steps(30, s0=1)
        got = m.area_averages(parts=True)
        assert not np.array_equal(before, got[0])
        t_areacfl.check_areas(cfg.name + " stepped", got, m.oml_get_state()[0], T)
        assert np.array_equal(bits(m.area_averages()), bits(got[0]))
    finally:
        m.close()


@BASINS
def test_cfl_of_a_stepped_handle(cyclic):
    """The test of that name in test_gpu_areacfl with the northern eddy: the criterion at half the largest Courant
    number, so offenders exist; maxima, counts and locations exactly the restatement's.  The keys of the maxima are
    (j-1) nx + (i-1) and the locations global rows: those of layer 1 lie above row 2048."""
    cfg = tall_cfg(171, cyclic)
    m, om, f = t_mon.setup(cfg, True)
    try:
        po = northern_eddy(cfg)
        m.set_p(po, po)
        m.steps(30, s0=1)
        po = m.get_state()[0]
        kw = dict(rdxf0=1.0 / (cfg.dxo * cfg.fnot), dt=cfg.dto, dx=cfg.dxo, rhf0hm=0.5 / (cfg.fnot * om.hmoc))
        crit = 0.5 * na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=0.8, **kw)["courant"].max()
        want = na.cfltry(po, f["tauxo"], f["tauyo"], cflcrit=crit, **kw)
        assert want["nbad"].sum() > 0
        rows = dict(zip(want["names"], want["loc"][:, 1]))
        assert rows["u1"] > LIMIT and rows["v1"] > LIMIT, rows
        assert want["bad"][:, 2].max() > LIMIT  # offenders too
        t_areacfl.check_cfl(cfg.name + " stepped", m.cfl(crit), want)
    finally:
        m.close()


# 6. xforc and a coupled window ------------------------------------------------------------------------------------------
def coupled_cfgs():
    """A 49 x 2053 x 3 ocean with the constants of cpl_tiny under its own 17 x 176 x 3 atmosphere (not tall: the
    atmosphere's column stays below the limit); the ocean sits at nx1 = 7, ny1 = 3."""
    oc = dataclasses.replace(config.preset("cpl_tiny"), name="cpl_tall", nxta=16, nyta=175, nxaooc=4, nyaooc=171, ndxr=12)
    r = oc.ndxr * oc.dxo / 8.0e4
    at = config.atmos_of(oc, ah4at=(1.5e14 * r ** 4,) * 3)  # as config.atmos_preset scales it
    assert (oc.nxpo, oc.nypo, at.nxpa, at.nypa) == (49, 2053, 17, 176)
    assert len(lib.thomas_segments(oc.nypo - 2)) == 3
    return oc, at


def test_xforc_pointwise():
    """test_gpu_xforc.test_golden against numpy_xforc itself (the CPU suite holds it to the reference bit for bit):
    every pointwise field by integer view, the four line integrals within 2 n 2^-53 sum|terms| dxo, a second call
    identical.  The ocean's fields have 2053 rows; tau_udiff reads the ocean's pressure under the atmosphere's."""
    oc, at = coupled_cfgs()
    P = dict(nxta=oc.nxta, nyta=oc.nyta, nxaooc=oc.nxaooc, nyaooc=oc.nyaooc, ndxr=oc.ndxr, nx1=7, ny1=3, cyclic=0,
             tau_udiff=1, fnot=oc.fnot, dxo=oc.dxo, cdat=1.3e-3, raoro=1.0e-3, hmat=1000.0, hmoc=100.0,
             bccoat=at.bccoat, bccooc=oc.bccooc)
    pam1 = synth.atmos_fields(at)["pam"][:, :, 0]
    pom1 = northern_eddy(oc)[:, :, 0]
    tabs = hostinit.bcuini(oc.ndxr, at.bccoat, at.dya)
    N = nx.xforc(pam1, pom1, tabs, P)
    o, a = OceanModel(oc), AtmosModel(at)
    try:
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
            if f.endswith("at"):
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
    atm_apply(a, f)
    xforc_setup(o, a, tau_udiff=True)
    if share:
        assert share_gpu(o, a) > 0
    return o, a


@pytest.mark.parametrize("share", [False, True])
def test_coupled_window(share):
    """test_gpu_xforc.test_coupled_window with the segmented ocean, nstr = 3, seven atmospheric steps: the window with
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


def test_coupled_steps_with_held_forcing_vs_oracle():
    """The segmented step inside the coupled capture against the oracle: with the forcing held the two halves are
    independent, so the 2053-row box of reference(171) under the cpl_tiny atmosphere is, after the 12 ocean steps of
    coupled_steps(o, a, 1, 36, 3), the oracle's state after 12 steps - the bars of
    test_gpu_tall_columns.test_columns_past_2048_rows_vs_oracle."""
    r = reference(171)
    cfg = r["cfg"]
    g = load_golden("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    o = OceanModel(cfg)
    a = AtmosModel(config.atmos_preset("cpl_tiny"), ddynat=f["ddynat"])
    try:
        load_box(o, r)
        atm_apply(a, f)
        coupled_steps(o, a, 1, 36, 3)
        o.sync()
        a.sync()
        errs = {n: relerr(x, y) for n, x, y in zip(FIELDS, o.get_state(), r["s12"])}
        se = scal_err(o, {"s12_scal": r["s12_scal"], "s12_po": r["s12"][0]}, "s12", cfg)
        print("12 ocean steps in a coupled window:", errs, "scalars %.3e" % se)
        assert all(v < TOL_RUN for v in errs.values()), errs
        assert se < 1e-11
        assert all(np.isfinite(x).all() for x in a.get_state())
    finally:
        o.close()
        a.close()
