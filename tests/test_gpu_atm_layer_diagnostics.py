"""The atmosphere's diagnostics and mixed layer on the device at layer counts other than three.  Needs an MI355X.

cpl_tiny's atmosphere (17 x 13) with nla = 2 and 4 layers (the monitors also with 5), ah4at different in every layer
(qgcm_hip.config.ATMOS_LAYERS): freshly set and again after 130 steps (the averaging after step 101 included),
monitors() / atm_valids(), tavatm() / time_means(), atmos_dump(), covatm(), area_averages() and cfl() against the
numpy restatements of the pulled state, by the rules of test_gpu_atm_monitors.py, test_gpu_atm_tavg.py,
test_gpu_cov.py and test_gpu_areacfl.py: exact where those are exact, the `scales`-based bar and the reordering bound
elsewhere.  The device against the reference's own four-layer values is test_against_the_reference[cpl_tiny_a4] of
test_gpu_atm_monitors.py and test_gpu_atm_tavg.py.

What pins the restatements at these counts: the monitors and the time averages / dump reproduce the reference at four
layers (tests/golden/atmon_cpl_tiny_a4.npz, atav_cpl_tiny_a4.npz; test_atm_monitors_cpu.py, test_atm_tavg_cpu.py).
The covariance, area-average / CFL restatements are NOT pinned by the reference at any count but three: covatm and
areavg read layer 1 and ast only, cfltry's layer handling is a plain loop over the layers of one expression.  The
mixed layer's (numpy_heat.aml) only layer dependence is the sum over the nla - 1 interfaces of src/amlsubs.F:203-209,
restated as that loop; its fixtures all have three layers, so aml() at 2 and 4 layers is restatement-only by design."""
import dataclasses

import numpy as np
import pytest

import numpy_areacfl as nar
import numpy_atm_monitors as nm
import numpy_atm_tavg as nt
import numpy_cov as nc
import numpy_heat as nh
from common import atm_apply, relerr, same_bits
from qgcm_hip import AtmosModel, atmos_preset, config, preset, synth
from qgcm_hip.model import atm_mon_params
from test_gpu_atm_monitors import compare, consts
from test_gpu_atm_tavg import fnetat, same
from test_gpu_areacfl import check_areas, check_cfl
from test_gpu_cov import ATM, restated

pytestmark = pytest.mark.gpu


def setup(nla):
    """A stepped-able AtmosModel of cpl_tiny's atmosphere with nla layers and every diagnostic input set: (model, inputs,
    monitor constants, time-average constants)."""
    acfg, ocfg = atmos_preset("cpl_tiny", nla), preset("cpl_tiny")
    s = synth.atmos_fields(acfg)
    m = AtmosModel(acfg, ddynat=s["ddynat"])
    atm_apply(m, s)
    fl = dict(nm.synthetic_fields(acfg, 3), fnetat=fnetat(acfg), wekpa=s["wekpa"], entat=s["entat"])
    kw = dict(davgat=37.5, aup=[0.05 * (k + 1) for k in range(nla - 1)], bup=0.31, cup=-4.0e-3, dup=1.7)
    m.set_atm_monitor_params(ocfg, **kw)
    m.set_atm_monitor_fields(**{k: fl[k] for k in ("wekta", "tauxa", "tauya", "ast", "hmixa", "uekat", "vekat")})
    m.set_time_mean_fields(fl["fnetat"])
    return m, fl, consts(acfg, atm_mon_params(acfg, ocfg, **kw)), nt.consts(acfg.dxa, acfg.fnot, 1000.0)


@pytest.mark.parametrize("nla", [2, 4, 5])
def test_monitors_and_valids(nla):
    m, fl, c, _ = setup(nla)
    try:
        for n in (0, 130):
            m.steps(n, s0=1)
            pa, pam, qa, _ = m.get_state()
            want, scales = nm.monitors(dict(fl, pa=pa, pam=pam, qa=qa), c)
            got = m.monitors()
            compare(got, want, scales)
            assert np.all(got["atstpos"] > 0) and (n == 0 or np.all(got["ddtkeat"] != 0.0))
            good, out = m.atm_valids()
            val = nm.valids(dict(fl, pa=pa, qa=qa))
            assert np.array_equal(out, val) and good == nm.solnok(val)
    finally:
        m.close()


@pytest.mark.parametrize("nla", [2, 4])
def test_time_means_dump_covariance_areas_and_cfl(nla):
    m, fl, _, c = setup(nla)
    acfg = m.cfg
    try:
        m.enable_covariance(2)
        nvar = (acfg.nxpa - 1) // 2 * ((acfg.nypa - 1) // 2)
        ap, at = nc.Dssp(nvar), nc.Dssp(nvar)
        x, y = acfg.xla, acfg.yla
        T = m.set_areas([0.0, 0.13 * x, 0.4 * x], [x, 0.71 * x, 0.9 * x], [0.0, 0.22 * y, 0.5 * y], [y, 0.83 * y, y])
        S = nt.tavini(acfg.nxpa, acfg.nypa, nla)
        kw = dict(rdxf0=1.0 / (acfg.dxa * acfg.fnot), dt=acfg.dta, dx=acfg.dxa, atm=True)
        for n in (0, 130):
            m.steps(n, s0=1)
            pa, _, qa, _ = m.get_state()
            tag = "nla %d after %d steps" % (nla, n)
            # time averages and the dump: bitwise (test_gpu_atm_tavg.py)
            m.tavatm()
            nt.tavatm(S, dict(fl, pa=pa, qa=qa), c)
            for nska in (1, 2, 5):
                want = nt.atnc_out(dict(fl, pa=pa, qa=qa), np.asarray(acfg.gpat[:nla - 1]), nska)
                same(m.atmos_dump(nska), {k: (v if k in ("pa", "qa", "ha") else v[0]) for k, v in want.items()})
            # covariance: bitwise (test_gpu_cov.py)
            m.covatm()
            nc.covocn(pa[:, :, 0], fl["ast"], 2, ap, at)
            # area averages: the reordering bound; CFL: bitwise (test_gpu_areacfl.py)
            check_areas(tag, m.area_averages(parts=True), fl["ast"], T)
            crit = 0.5 * nar.cfltry(pa, fl["uekat"], fl["vekat"], cflcrit=0.8, **kw)["courant"].max()
            want = nar.cfltry(pa, fl["uekat"], fl["vekat"], cflcrit=crit, **kw)
            assert want["nbad"].sum() > 0 and len(want["names"]) == 2 + 2 * nla
            check_cfl(tag, m.cfl(crit), want)
        got = m.time_means()
        assert got.pop("nsumat") == 2
        same(got, nt.tavout(S))
        assert np.any(got["uptpat"]) and np.any(got["vptpat"])
        same(m.covariance(), restated(ap, at, ATM))
    finally:
        m.close()


# ---- aml() ------------------------------------------------------------------------------------------------------------
# entrainment factors of the nla - 1 interfaces: the three-layer fixture's two values continued, no two alike
AFACE = (1.1e-06, -4.0e-07, 2.5e-07)


def aml_setup(nla):
    """heat_cpl_tiny's grid, constants and mixed-layer inputs over an atmosphere of nla layers (ATMOS_LAYERS), its
    pressures from synth.atmos_fields: (model, fixture, the restatement's constants, pa, pam)."""
    from test_gpu_heat import _aml_cfg
    g = nh.load("heat_cpl_tiny")
    P = dict(nh.params(g))
    hat, gpat, _ = config.ATMOS_LAYERS[nla]
    base = config.preset("cpl_tiny")
    oc = dataclasses.replace(base, name="aml_a%d" % nla, nxta=P["nxta"], nyta=P["nyta"], nxaooc=P["nxaooc"],
                             nyaooc=P["nyaooc"], ndxr=P["ndxr"], dxo=P["dxo"], fnot=P["fnot"], bccooc=P["bccooc"], dta=P["dta"])
    at = config.atmos_of(oc, bccoat=P["bccoat"], nla=nla, hat=hat, gpat=gpat, ah4at=(1.5e14,) * nla)
    P.update(aface=AFACE[:nla - 1], gpat=gpat)
    s = synth.atmos_fields(at)
    a = AtmosModel(at)
    a.aml_init(dataclasses.replace(_aml_cfg(P), aface=P["aface"]), xc1ast=g["in_xc1ast"], dtopat=g["in_dtopat"])
    a.set_state(po=s["pa"], pom=s["pam"])
    a.set_time_mean_fields(fnetat=g["x0_fnetat"])
    a.set_atm_monitor_fields(wekta=g["x0_wekta"], uekat=g["x0_uekat"], vekat=g["x0_vekat"])
    return a, g, P, s["pa"], s["pam"]


@pytest.mark.parametrize("nla", [2, 4])
def test_aml_one_call_and_nine_chained(nla):
    """One call: ast, astm, hmixa, hmixam, entat bitwise, cfraat exact, the sums within 2 n 2^-53 sum|terms| (bars of
    test_gpu_heat.py test_aml_golden).  Nine chained calls with nothing re-fed: ast, hmixa, entat within 1e-13 of their
    maximum (test_chained)."""
    a, g, P, pa, pam = aml_setup(nla)
    scale = dict(xan=P["dxa"] * P["dya"], centat=P["dxa"] * P["dya"], enisat=P["dxa"], eninat=P["dxa"])
    STATE = ("ast", "astm", "hmixa", "hmixam")
    try:
        S = {f: g["in_" + f] for f in STATE}
        a.aml_set_state(**S)
        for call in range(9):
            a.aml()
            N = nh.aml(S, g["x0_fnetat"], g["x0_wekta"], g["x0_uekat"], g["x0_vekat"], pa, pam, g["in_xc1ast"],
                       g["in_dtopat"], P)
            st, (entat, d) = a.aml_get_state(), a.aml_get_diag()
            S = {f: N[f] for f in STATE}
            if call == 0:
                for f, v in zip(STATE, st):
                    same_bits(v, N[f], "nla %d aml %s" % (nla, f))
                same_bits(entat, N["entat"], "nla %d aml entat" % nla)
                assert d["cfraat"] == N["cfraat"]
                for f in nh.AML_SUMS:
                    bound = 2.0 * N["n_" + f] * 2.0 ** -53 * N["abs_" + f] * scale[f]
                    print("nla %d aml %s: device %.17e restated %.17e |diff| %.3e bound %.3e" % (nla, f, d[f], N[f], abs(d[f] - N[f]), bound))
                    assert abs(d[f] - N[f]) <= bound, (f, d[f], N[f], bound)
                # every interface's term is there to be missed: each is far above the rounding of entat
                for l in range(nla - 1):
                    term = (P["aface"][l] / P["gpat"][l]) * (pam[:, :, l] - pam[:, :, l + 1])
                    assert np.abs(term).max() > 1e-6 * np.abs(N["entat"]).max(), l
        errs = dict(ast=relerr(st[0], N["ast"]), hmixa=relerr(st[2], N["hmixa"]), entat=relerr(entat, N["entat"]))
        print("nla %d after nine calls" % nla, errs)
        for k, e in errs.items():
            assert e < 1e-13, (k, e)
    finally:
        a.close()
