"""The ocean monitors, valids and prsamp on y-slabs (qgcm_hip_*_part / _combine through SlabOcean.monitors / valids /
prsamp): slabs as LocalComm virtual ranks on one GPU, against the golden values of the reference, against a
whole-domain OceanModel holding the same state and against the numpy restatement tests/numpy_monitors.py.

Bars as in tests/test_gpu_monitors.py: extrema, Courant numbers, osfmin / osfmax, occirc / occtot, ocjpos / ocjval
bitwise; every integral within 1e-12 of the integral of the modulus of its integrand.  valids: bitwise.  prsamp: the
spot values and the sst range bitwise, the averages to rounding."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

from numpy_monitors import monitors as np_monitors
from qgcm_hip import OceanModel, QgcmHipError, check, hostinit, oml_preset, preset, synth
from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition, slab_slice
from test_gpu_monitors import compare, golden_case, reference, setup

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def make_slabs(cfg, parts, consts=None, om=None):
    consts = global_consts(cfg) if consts is None else consts
    P = len(parts)
    S = [HipSlab(cfg, consts, g0, g1, r, P, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
    if om is not None:
        for x in S:
            x.oml_init(om)
    return SlabOcean(cfg, S, LocalComm(P, after=torch.cuda.synchronize))


def close(so):
    for x in so.slabs:
        x.close()


def load(so, po, pom, qo, qom, wekpo, entoc):
    nl = so.cfg.nlo
    for x in so.slabs:
        sl = slab_slice(so.cfg.nypo, x.g0, x.g1)
        x.set_state(po[:, sl], pom[:, sl], qo[:, sl], qom[:, sl])
        x.set_forcing(wekpo[:, sl], entoc[:, sl], np.zeros(nl - 1))


def same_on_every_rank(so, kind):
    res = so.diagnostic(kind)
    for r in res[1:]:
        if kind == "valids":
            assert r[0] == res[0][0] and np.array_equal(r[1], res[0][1])
        else:
            assert np.array_equal(r, res[0])
    return res[0]


# 1. golden values of the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny", "box_tiny5"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_golden(name, nranks):
    cfg, f, c, want = golden_case(name)
    _, scales = np_monitors(f, c)
    so = make_slabs(cfg, partition(cfg.nypo, nranks))
    try:
        load(so, f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"])
        for x in so.slabs:
            x.set_monitor_params(rhooc=c["rhooc"], cpoc=c["cpoc"], hmoc=c["hmoc"], ycexp=c["ycexp"],
                                 sb_hflux=bool(c["sb_hflux"]), nb_hflux=bool(c["nb_hflux"]))
            x.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
        same_on_every_rank(so, "monitors")
        compare(so.monitors(), want, scales)
    finally:
        close(so)


# 2. full size: the whole-domain model's state on slabs -----------------------------------------------------------
def slabs_like(m, om, f, mixed_layer, parts):
    """Slabs holding what the whole-domain model m holds now."""
    cfg = m.cfg
    po, pom, qo, qom = m.get_state()
    entoc = m.oml_get_diag()[0] if mixed_layer else f["entoc"]
    so = make_slabs(cfg, parts, om=om if mixed_layer else None)
    load(so, po, pom, qo, qom, f["wekpo"], entoc)
    for x in so.slabs:
        x.set_monitor_params(om)
        if mixed_layer:
            sst, sstm = m.oml_get_state()
            x.oml_set_state(sst, sstm)
            x.oml_set_forcing(np.zeros_like(sst), f["wekto"], f["tauxo"], f["tauyo"])
        else:
            x.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
    return so


@pytest.mark.parametrize("cfgname", ["natl5", "socn5"])
@pytest.mark.parametrize("mixed_layer", [False, True])
def test_full_size(cfgname, mixed_layer):
    m, om, f = setup(cfgname, mixed_layer)
    try:
        m.steps(10, s0=1)
        whole = m.monitors()
        want, scales = reference(m, om, f, mixed_layer)
        compare(whole, want, scales)
        for nranks in (2, 3, 8):
            so = slabs_like(m, om, f, mixed_layer, partition(m.cfg.nypo, nranks))
            try:
                got = so.monitors()
                compare(got, whole, scales)
                compare(got, want, scales)
            finally:
                close(so)
    finally:
        m.close()


# 3. halo currency: slab steps, then monitors against the gathered state ---------------------------------------------
def stepped_slabs(cfgname, nranks, early):
    cfg = preset(cfgname)
    om = oml_preset(cfg)
    po = synth.gaussian_eddy(cfg, noise=1e-2)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    wekto, wek = synth.wekpo_from_tau(cfg, tx, ty)
    consts = global_consts(cfg)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
    ent = np.zeros_like(wek)
    so = make_slabs(cfg, partition(cfg.nypo, nranks), consts)
    so.early_tend = early
    so.homsol()
    so.scatter_state(po, pom, qo, qom, wek, ent, np.zeros(cfg.nlo - 1), scal)
    sst = np.asfortranarray(np.full((cfg.nxto, cfg.nyto), 15.0) + 0.1 * np.arange(cfg.nyto)[None, :])
    f = dict(tauxo=tx, tauyo=ty, wekto=wekto, sst=sst, wekpo=wek, entoc=ent)
    for x in so.slabs:
        x.set_monitor_params(om)
        x.set_monitor_fields(tx, ty, wekto, sst)
    return so, om, f


def gathered_model(so, om, f):
    cfg = so.cfg
    st = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo), order="F") for _ in range(4)]
    for g0, g1, arrs in so.gather_local():
        for a, b in zip(st, arrs):
            a[:, g0 - 1:g1, :] = b
    m = OceanModel(cfg)
    m.set_state(*st)
    m.set_forcing(f["wekpo"], f["entoc"], np.zeros(cfg.nlo - 1))
    m.set_monitor_params(om)
    m.set_monitor_fields(f["tauxo"], f["tauyo"], f["wekto"], f["sst"])
    return m


@pytest.mark.parametrize("early", [False, True])
def test_halo_rows_are_current_after_steps_and_averaging(early):
    so, om, f = stepped_slabs("box_med", 2, early)
    try:
        for n in (1, 25, 3):  # step 26 is an averaging step
            so.steps(n)
            m = gathered_model(so, om, f)
            try:
                want, scales = reference(m, om, f, False)
                whole = m.monitors()
                got = so.monitors()
                compare(got, whole, scales)
                compare(got, want, scales)
            finally:
                m.close()
    finally:
        close(so)


# 4. valids ---------------------------------------------------------------------------------------------------------
def golden_state(name):
    cfg, f, c, _ = golden_case(name)
    m = OceanModel(cfg)
    m.set_state(f["po"], f["pom"], f["qo"], f["qom"])
    m.set_forcing(f["wekpo"], f["entoc"], np.zeros(cfg.nlo - 1))
    return cfg, f, m


def valids_both(cfg, f, m, parts, dtopoc=None):
    so = make_slabs(cfg, parts)
    try:
        load(so, f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"])
        if dtopoc is not None:
            m.set_dtopoc(dtopoc)
            for x in so.slabs:
                x.set_dtopoc(dtopoc)
        got = same_on_every_rank(so, "valids")
        want = m.valids()
        assert got[0] == want[0]
        assert np.array_equal(got[1], want[1])
        return got
    finally:
        close(so)


@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny", "box_tiny5"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_valids_bitwise(name, nranks):
    cfg, f, m = golden_state(name)
    try:
        ok, _ = valids_both(cfg, f, m, partition(cfg.nypo, nranks))
        assert ok
    finally:
        m.close()


def test_valids_failing_po_on_the_last_rank():
    cfg, f, m = golden_state("box_tiny")
    try:
        parts = partition(cfg.nypo, 3)
        f = dict(f, po=np.array(f["po"], order="F"))
        f["po"][7, parts[-1][0] + 1, 1] = 2.0e4  # |po| >= 1e4 in a row rank 2 owns
        m.set_state(f["po"], f["pom"], f["qo"], f["qom"])
        ok, out = valids_both(cfg, f, m, parts)
        assert not ok and out[1] == 2.0e4
    finally:
        m.close()


def test_valids_thin_layers_with_topography():
    cfg, f, m = golden_state("box_tiny")
    try:
        x = np.arange(cfg.nxpo)[:, None] / (cfg.nxpo - 1.0)
        y = np.arange(cfg.nypo)[None, :] / (cfg.nypo - 1.0)
        hb = cfg.hoc[cfg.nlo - 1]
        dtopoc = np.asfortranarray(np.broadcast_to(hb * 1.05 * np.exp(-((x - 0.5) ** 2 + (y - 0.6) ** 2) / 0.05),
                                                   (cfg.nxpo, cfg.nypo)))
        ok, out = valids_both(cfg, f, m, partition(cfg.nypo, 3), dtopoc)
        assert out[14 + cfg.nlo - 1] > 0.0  # hfbad of the bottom layer
    finally:
        m.close()


# 5. prsamp ---------------------------------------------------------------------------------------------------------
def xintp_abs(a):
    w = np.ones(a.shape[:2])
    w[0, :] *= 0.5
    w[-1, :] *= 0.5
    w[:, 0] *= 0.5
    w[:, -1] *= 0.5
    return np.einsum("ij,ijk->k", w, np.abs(a))


@pytest.mark.parametrize("where", ["last", "first", "even"])
def test_prsamp(where):
    cfg, f, m = golden_state("box_tiny")
    try:
        nyc = (cfg.nypo + 1) // 2
        parts = {"last": [(1, nyc), (nyc + 1, cfg.nypo)], "first": [(1, nyc - 1), (nyc, cfg.nypo)],
                 "even": partition(cfg.nypo, 3)}[where]
        so = make_slabs(cfg, parts)
        try:
            load(so, f["po"], f["pom"], f["qo"], f["qom"], f["wekpo"], f["entoc"])
            same_on_every_rank(so, "prsamp")
            got, want = so.prsamp(), m.prsamp()
        finally:
            close(so)
        for k in ("po_centre", "qo_centre", "sstmin", "sstmax"):
            assert np.array_equal(got[k], want[k]), k
        on = 1.0 / (cfg.nxto * cfg.nyto)
        for k, fld in (("pavgoc", "po"), ("qavgoc", "qo")):
            assert np.all(np.abs(got[k] - want[k]) <= 1e-12 * xintp_abs(f[fld]) * on), k
    finally:
        m.close()


def test_prsamp_sst_with_the_mixed_layer():
    m, om, f = setup("box_small", True)
    try:
        m.steps(3, s0=1)
        so = slabs_like(m, om, f, True, partition(m.cfg.nypo, 3))
        try:
            got, want = so.prsamp(), m.prsamp()
            okv, outv = so.valids()
            wokv, woutv = m.valids()
        finally:
            close(so)
        for k in ("po_centre", "qo_centre", "sstmin", "sstmax"):
            assert np.array_equal(got[k], want[k]), k
        assert got["sstmin"] < 1e30 and okv == wokv and np.array_equal(outv, woutv)
    finally:
        m.close()


# 6. consistency ----------------------------------------------------------------------------------------------------
def test_no_side_effects_repeatable_and_refusals():
    so, om, f = stepped_slabs("box_small", 3, False)
    try:
        so.steps(4)
        before = [x.get_state() + [x.get_scalars()] for x in so.slabs]
        for kind in ("monitors", "valids", "prsamp"):
            a = same_on_every_rank(so, kind)
            b = same_on_every_rank(so, kind)
            if kind == "valids":
                assert a[0] == b[0] and np.array_equal(a[1], b[1])
            else:
                assert np.array_equal(a, b)
        after = [x.get_state() + [x.get_scalars()] for x in so.slabs]
        assert all(np.array_equal(p, q) for u, v in zip(before, after) for p, q in zip(u, v))
        # a gather that does not tile the rows: rank order swapped, one rank missing
        x = so.slabs[0]
        for kind in ("monitors", "valids", "prsamp"):
            send, gath = so._diag_bufs[kind]
            n = send[0].numel()
            swapped = torch.cat([gath[0][n:2 * n], gath[0][:n], gath[0][2 * n:]])
            with pytest.raises(QgcmHipError, match="do not tile"):
                x.diag_combine(kind, swapped)
            x.nranks = 2
            try:
                with pytest.raises(QgcmHipError, match="do not tile"):
                    x.diag_combine(kind, gath[0][:2 * n])
            finally:
                x.nranks = 3
        # the whole-domain entry points still refuse a slab handle
        out = np.zeros(19 * so.cfg.nlo + 16)
        with pytest.raises(QgcmHipError, match="whole domain"):
            check(x.L.qgcm_hip_monitors(x.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    finally:
        close(so)


def test_whole_domain_part_and_combine():
    """_part + _combine with nranks = 1 on a whole-domain handle: the one-call results (integrals to rounding)."""
    m, om, f = setup("box_small", False)
    try:
        m.steps(5, s0=1)
        so = slabs_like(m, om, f, False, [(1, m.cfg.nypo)])
        try:
            assert so.slabs[0].nranks == 1
            _, scales = reference(m, om, f, False)
            compare(so.monitors(), m.monitors(), scales)
            ok, out = so.valids()
            wok, wout = m.valids()
            assert ok == wok and np.array_equal(out, wout)
        finally:
            close(so)
    finally:
        m.close()


# 7. one process per slab -------------------------------------------------------------------------------------------
def test_three_processes_over_gloo():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr",
           "127.0.0.1", "--master-port", "29743", os.path.join(HERE, "mp_slab_diag_worker.py"), "box_small"]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "MP_SLAB_DIAG_RESULT OK" in r.stdout, r.stdout[-3000:]
