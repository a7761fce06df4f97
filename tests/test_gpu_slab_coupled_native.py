"""The coupled window on a y-slab ocean driven by the library (qgcm_hip_slab_coupled_steps): one rank on a
real RCCL communicator - all a one-GPU box can hold - created as tests/test_gpu_parity.py creates its rank for
qgcm_hip_slab_steps.  The window nt0 = 73, n = 30, nstr = 3 is ten ocean steps, across ocean step 26 (leapfrog
averaging) and nt = 101 (the atmosphere's averaging), with both mixed layers and the heat half on.  Every state field
and scalar after it is held BITWISE (0 ulp) to the same window driven from Python (SlabOcean.coupled_steps on one
LocalComm rank) and to the whole-domain coupled_steps (one rank is bitwise the whole domain in every
mode).  Shapes: cpl_tiny (ocean 49 x 37, ndxr = 12, atmosphere 17 x 13) and the channel heat_cyc72 (289 x 17)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import numpy_heat as nh
import test_gpu_slab_coupled as tsc
from test_gpu_slab_coupled import _same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

NT0, N, NSTR = 73, 30, 3
MODES = ("replicated", "bands", "udiff_gather", "udiff_sums")
FIELDS = ("po", "pom", "qo", "qom", "sst", "pa", "pam", "qa", "ast", "hmixa", "fnetoc", "fnetat", "wekpo", "wekpa", "tauxo",
          "tauyo")


def _snapshot(o, a, xf, heat):
    """Every state field and scalar of an ocean handle (a whole-domain model, or the one slab that holds every row) and
    an atmosphere after a window; xf, heat: the outputs of the last xforc (dicts)."""
    o.sync()
    a.sync()
    d = dict(zip(("po", "pom", "qo", "qom"), o.get_state()))
    d.update(zip(("sst", "sstm"), o.oml_get_state()))
    d.update(zip(("pa", "pam", "qa", "qam"), a.get_state()))
    d.update(zip(("ast", "astm", "hmixa", "hmixam"), a.aml_get_state()))
    d["entat"] = a.aml_get_diag()[0]
    d["ocean scalars"], d["atmosphere scalars"] = o.get_scalars(), a.get_scalars()
    d.update({"xforc " + k: v for k, v in xf.items()})
    d.update({"heat " + k: v for k, v in heat.items()})
    for k in FIELDS:  # (what the window is held to, under the names it is stated in)
        assert any(n in (k, "xforc " + k, "heat " + k) for n in d), k
    out = {k: np.array(v, dtype=np.float64) for k, v in d.items()}
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def _all_same(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k in sorted(ref):
        _same(got[k], ref[k], "%s: %s" % (what, k))


def _go_native(so):
    """The rank onto a real communicator and the library's window; the calls return with the work queued."""
    from qgcm_hip.slab import rccl_unique_id
    so.use_library_exchanges(rccl_unique_id())
    so.slabs[0].sync_each_call = False
    so.use_library_coupling()


def _slab_cpl_tiny(mode):
    """tests/test_gpu_slab_coupled.py:_cpl_tiny on one rank, xforc set up again in `mode` before anything has run."""
    P = nh.params(nh.load("heat_cpl_tiny"))
    so, reps = tsc._cpl_tiny(1)
    so.xforc_setup(reps, **({} if mode == "replicated" else {mode: True}))
    so.xforc_heat_setup(tsc._heat_cfg(P))
    return so, reps


_res = {}


def _window(kind, mode, xforc=True):
    """The window on cpl_tiny; kind: "whole" (the whole-domain models, tau_udiff on for the two udiff modes), "python"
    (SlabOcean.coupled_steps, one LocalComm rank) or "native".  Computed once per key, shared, unchanged."""
    udiff = mode in ("udiff_gather", "udiff_sums")
    key = (kind, udiff if kind == "whole" else mode)
    if key in _res:
        return _res[key]
    if kind == "whole":
        from qgcm_hip import coupled_steps, xforc_get, xforc_heat_get, xforc_heat_setup, xforc_setup
        o, a = tsc._cpl_tiny(0)
        try:
            if udiff:
                xforc_setup(o, a, tau_udiff=True)
                xforc_heat_setup(o, a, tsc._heat_cfg(nh.params(nh.load("heat_cpl_tiny"))))
            coupled_steps(o, a, NT0, N, NSTR, xforc=True)
            _res[key] = _snapshot(o, a, xforc_get(o, a), xforc_heat_get(o, a))
        finally:
            o.close()
            a.close()
    else:
        so, reps = _slab_cpl_tiny(mode)
        try:
            if kind == "native":
                _go_native(so)
            so.coupled_steps(NT0, N, NSTR, xforc=True)
            _res[key] = _snapshot(so.slabs[0], reps[0], so.xforc_get()[0], so.xforc_heat_get()[0])
        finally:
            tsc._close(so, reps)
    return _res[key]


@pytest.mark.parametrize("mode", MODES)
def test_window_is_the_python_drivers_and_the_whole_domains(mode):
    """Ten ocean steps in each of the four xforc modes: po, pom, qo, qom, sst, pa, pam, qa, ast, hmixa, fnetoc, fnetat,
    wekpo, wekpa, tauxo, tauyo - and the lagged levels, entat, the other outputs of xforc and the scalars of both
    handles - by integer view equal to the Python-driven window and to the whole-domain window."""
    got = _window("native", mode)
    _all_same(got, _window("python", mode), "%s: library window against the Python-driven one" % mode)
    _all_same(got, _window("whole", mode), "%s: library window against the whole-domain one" % mode)
    # the window moved what it should: the shear term changes the ocean, ten steps change everything
    if mode == "udiff_gather":
        assert not np.array_equal(got["po"], _window("native", "replicated")["po"])


def test_held_forcing_is_the_explicit_sequence():
    """xforc = 0: the window with the forcing held is bitwise the explicit sequence of step() and the replica's steps
    on a Python-driven rank."""
    res = []
    for kind in ("native", "explicit"):
        so, reps = _slab_cpl_tiny("replicated")
        try:
            so.xforc()  # (a forcing to hold)
            if kind == "native":
                _go_native(so)
                so.coupled_steps(NT0, N, NSTR, xforc=False)
            else:
                for nt in range(NT0, NT0 + N, NSTR):
                    so.step((nt - 1) // NSTR + 1)
                    reps[0].steps(NSTR, s0=nt)
            res.append(_snapshot(so.slabs[0], reps[0], so.xforc_get()[0], so.xforc_heat_get()[0]))
        finally:
            tsc._close(so, reps)
    _all_same(res[0], res[1], "held forcing")
    assert not np.array_equal(res[0]["ast"], _window("native", "replicated")["ast"])


def test_channel():
    """The channel heat_cyc72 (289 x 17, ndxr = 4: the cyclic ocean's line integrals, the wrap) in replicated mode with
    the heat half: bitwise the Python-driven window.  Against the whole-domain window: everything xforc leaves and the
    whole atmosphere bitwise (one rank's xforc is the whole-domain call's bits), the stepped ocean and its
    mixed layer at the bars the slab tests hold a stepped channel to (tests/test_gpu_slab_coupled.py:_window_close: 1e-10
    and 1e-12 of the maximum) - a cyclic slab forms its constraint sums in another order than the whole-domain handle,
    with or without this driver (measured on one Python-driven rank: po 1.9e-15, qo 4.6e-15, sst 5.9e-16 of the
    maximum).  The window is nt0 = 73, n = 9: ocean steps
    25, 26 (with its leapfrog averaging) and 27.  The fixture was recorded for single xforc calls and its state is not a
    balanced one: stepped, it grows about tenfold per ocean step from the third on under either driver (measured:
    max |pa| 9.0, 23.9, 254.5 after steps one to three, not finite after the seventh), so the ten steps of the cpl_tiny
    window would compare NaNs."""
    from qgcm_hip import coupled_steps, xforc_get, xforc_heat_get
    case, res, N = "heat_cyc72", {}, 9
    for kind in ("native", "python"):
        g, P, so, reps = tsc._slabbed(case, 1)
        try:
            if kind == "native":
                _go_native(so)
            so.coupled_steps(NT0, N, NSTR, xforc=True)
            res[kind] = _snapshot(so.slabs[0], reps[0], so.xforc_get()[0], so.xforc_heat_get()[0])
        finally:
            tsc._close(so, reps)
    g, P, o, a = tsc._whole(case)
    try:
        coupled_steps(o, a, NT0, N, NSTR, xforc=True)
        res["whole"] = _snapshot(o, a, xforc_get(o, a), xforc_heat_get(o, a))
    finally:
        o.close()
        a.close()
    assert res["native"]["xforc txisoc"] != 0.0 and res["native"]["xforc txinoc"] != 0.0
    _all_same(res["native"], res["python"], "channel: library window against the Python-driven one")
    got, ref = res["native"], res["whole"]
    for k in sorted(ref):
        if k.startswith(("xforc ", "heat ")) or k in ("pa", "pam", "qa", "qam", "ast", "astm", "hmixa", "hmixam", "entat",
                                                      "atmosphere scalars"):
            _same(got[k], ref[k], "channel: library window against the whole-domain one: " + k)
    form = lambda d: dict(ocean=[d[k] for k in ("po", "pom", "qo", "qom")], sst=[d["sst"], d["sstm"]],
                          atmos=[d[k] for k in ("pa", "pam", "qa", "qam")],
                          aml=[d[k] for k in ("ast", "astm", "hmixa", "hmixam")], entat=d["entat"])
    tsc._window_close(form(got), form(ref), "channel: library window against the whole-domain one")


def test_refusals():
    """Every refusal names its reason and changes nothing: the window that follows them gives the bits of a run that met
    none."""
    from qgcm_hip import AtmosModel, QgcmHipError
    from qgcm_hip.slab import rccl_unique_id
    so, reps = _slab_cpl_tiny("replicated")
    so2, reps2 = tsc._cpl_tiny(1)
    extra = []
    try:
        x, a = so.slabs[0], reps[0]
        with pytest.raises(ValueError, match="use_library_exchanges first"):
            so.use_library_coupling()
        with pytest.raises(QgcmHipError, match=r"qgcm_hip_slab_coupled_init: no communicator \(qgcm_hip_comm_init\)"):
            x.coupled_init(a)
        so.use_library_exchanges(rccl_unique_id())
        x.sync_each_call = False
        b = AtmosModel(a.cfg)  # init before the xforc set-up
        extra.append(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_slab_coupled_init: qgcm_hip_xforc_slab_init has not been called for this atmosphere"):
            x.coupled_init(b)
        with pytest.raises(QgcmHipError, match="qgcm_hip_slab_coupled_init: the ocean handle is not the one qgcm_hip_xforc_slab_init was called with"):
            x.coupled_init(reps2[0])  # an atmosphere set up for another slab
        with pytest.raises(QgcmHipError, match="qgcm_hip_slab_coupled_steps: qgcm_hip_slab_coupled_init has not been called"):
            x.coupled_steps(a, NT0, N, NSTR, True)
        x.set_overlap(1)
        with pytest.raises(QgcmHipError, match=r"qgcm_hip_slab_coupled_init: the overlapped halo exchange is switched on \(qgcm_hip_comm_set_overlap\)"):
            so.use_library_coupling()
        x.set_overlap(0)
        so.use_library_coupling()
        x.set_overlap(1)  # ... switched on after the init
        with pytest.raises(QgcmHipError, match="qgcm_hip_slab_coupled_steps: the overlapped halo exchange is switched on"):
            so.coupled_steps(NT0, N, NSTR, xforc=True)
        x.set_overlap(0)
        with pytest.raises(QgcmHipError, match="qgcm_hip_slab_coupled_steps: bad step range"):
            so.slabs[0].coupled_steps(a, 0, N, NSTR, True)
        so.xforc_setup(reps, bands=True)  # the mode changed after the init: other message sizes
        with pytest.raises(QgcmHipError, match="xforc's set-up changed after qgcm_hip_slab_coupled_init"):
            x.coupled_steps(a, NT0, N, NSTR, True)
        so.xforc_setup(reps)
        so.xforc_heat_setup(tsc._heat_cfg(nh.params(nh.load("heat_cpl_tiny"))))
        so.use_library_coupling()
        so.coupled_steps(NT0, N, NSTR, xforc=True)
        got = _snapshot(x, a, so.xforc_get()[0], so.xforc_heat_get()[0])
        _all_same(got, _window("python", "replicated"), "after the refusals")
        assert so.step_index == (NT0 + N - 2) // NSTR + 2 and a.step_index == NT0 + N
    finally:
        for m in extra:
            m.close()
        tsc._close(so, reps)
        tsc._close(so2, reps2)


def test_two_ranks_two_processes():
    """Two processes, one GPU each, RCCL between them: the library's window against the Python-driven DistComm path at
    the slab tests' bars (tests/test_gpu_slab_coupled.py:_window_close), the replicas bit-equal across the ranks.  Needs
    two GPUs: a one-GPU machine skips it, and RCCL with more than one rank stays unexecuted there for this path."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29791", os.path.join(HERE, "mp_slab_coupled_worker.py")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "MP_SLAB_COUPLED_RESULT OK" in r.stdout, r.stdout[-3000:]
