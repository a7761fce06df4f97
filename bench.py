#!/usr/bin/env python3
"""bench.py - ocean timesteps/s of the MI355X-native Q-GCM PV-advance/inversion path.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A "step" is one ocean timestep of the hot path: qgostep -> ocinvq -> ocqbdy (+ the
leapfrog averaging every 25th step), src/q-gcm.F:1243-1249,1328-1366, on the
synthetic NAtl-5km-shaped 3-layer grid (961 x 961 x 3, fp64; BASELINE.json
configs[1]) with all inputs resident in HBM.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times exactly K steps and prints the headline line
(`value`, `ms_per_step`).  --dump-outputs DIR writes the state the timed steps
left behind as DIR/*.npy (one GPU; see dump_outputs).  --full adds everything
else: the objects below and the secondary figures (the reference's call sequence,
the mixed layer, SOcn 5 km, coupled, NAtl 1 km; N > 1: weak scaling and the other
basins), each measured in runs of its own after the headline window.

Extra objects in the --full line:
  roofline      dominant kernel: algorithmic bytes per launch / HIP-event average
                launch duration measured live on the library's stream, against the
                nominal 8 TB/s HBM peak (MI355X_MICROARCH.md).
  cpu_baseline  the true reference Fortran+FFTPACK path (oracle/_ref, kind
                "reference") or, if that library is absent, the C restatement
                (kind "port"), timed on this box's host cores on a bounded sample.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # nominal MI355X HBM3E peak (MI355X_MICROARCH.md)
WORKLOAD = "natl5"

# Algorithmic bytes per launch in units of N*8 B (N = nxpo*nypo), SURVEY.md 8(d):
# P1 tendency+leapfrog+projection 24, P2/P4 row transforms 6 each, P3 Thomas 6,
# P5 unpack 14 (box).  "own" = what this implementation's kernel has to move
# (rotating time-level buffers: no qom/pom rewrite, no po re-read) - DESIGN.md.
ALGO_FIELDS = {"k_tend": (24, 21), "k_dst_fwd": (6, 6), "k_thomas": (6, 6), "k_dst_inv": (6, 6),
               "k_unpack": (14, 8), "k_constr": (0, 0), "k_cyc_bsums": (0, 0), "k_noop": (0, 0), "k_ocqbdy": (0, 0), "k_lf_average": (0, 0),
               "k_oml": (0, 0), "k_oml_entoc": (0, 0)}


def divert_stdout():
    """The reference Fortran prints its start-up report on fd 1 (and its runtime
    flushes at exit): point fd 1 at stderr for good and return a private handle to
    the real stdout for our ONE JSON line."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)
    return os.fdopen(real, "w")


def synthetic_inputs(cfg):
    from qgcm_hip import synth
    po = synth.gaussian_eddy(cfg)              # IC B of SURVEY 8d
    tx, ty = synth.wind_stress(cfg)            # double-gyre wind
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    return po, wek


DUMP_SAMPLE_POINTS = 1_000_000  # pom / qom sample size: with po and qo whole, 60.3 MB in all at NAtl 5 km
DUMP_SAMPLE_SEED = 20241015


def dump_outputs(outdir, state, scalars):
    """--dump-outputs: what a caller of the timed path receives after its last step (OceanModel.get_state,
    get_scalars), float64.  po.npy and qo.npy hold the whole (nxpo, nypo, nlo) fields; pom and qom, which would take
    the total past 64 MB, go out as the values at one fixed sample of flat Fortran-order indices (the same for both,
    drawn from DUMP_SAMPLE_SEED), pom_sample.npy and qom_sample.npy; scalars.npy holds the constraint scalars."""
    po, pom, qo, qom = state
    n = po.size
    idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, size=min(DUMP_SAMPLE_POINTS, n), replace=False))
    os.makedirs(outdir, exist_ok=True)
    arrays = {"po": po, "qo": qo, "pom_sample": pom.ravel(order="F")[idx], "qom_sample": qom.ravel(order="F")[idx],
              "scalars": scalars}
    for name, a in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), np.asarray(a, dtype=np.float64))


def host_cores():
    """CPUs this process may really use: affinity mask capped by the cgroup CPU quota
    (a GPU box hands each job a share of the host, e.g. 16 of 256 hardware threads)."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except Exception:
            continue
    env = os.environ.get("QGCM_CPU_BASELINE_THREADS")
    if env:
        n = int(env)
    return min(n, 64)  # the reference parallelises over j only; more threads than that do not help it


def cpu_model():
    """`Model name` of lscpu (SURVEY 8d asks for it beside the core count)."""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return None


def cpu_baseline(cfg, po, wek, budget_s=15.0):
    """Reference (or port) ocean steps/s on the host cores; bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    cores = host_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    os.environ.setdefault("OMP_STACKSIZE", "1G")
    zeros2 = np.zeros_like(wek)
    kind, model = None, None
    try:
        import ref_binding
        if os.path.exists(ref_binding.lib_path("box_natl5")):
            r = ref_binding.RefLib("box_natl5")
            assert (r.nx, r.ny, r.nl) == (cfg.nxpo, cfg.nypo, cfg.nlo)
            r.init(cfg.dxo, cfg.dto, cfg.delek, cfg.bccooc, cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc)
            r.set_p(po, po)
            r.set_forcing(wek, zeros2, np.zeros(cfg.nlo - 1))
            kind, model = "reference", r
            ref_binding.set_threads(cores)
    except Exception as e:  # fall back to the port, say why
        print("cpu_baseline: reference library unusable (%s); timing the C port" % e, file=sys.stderr)
    if model is None:
        import oracle_binding as ob
        ob.set_threads(cores)
        o = ob.Oracle(cfg.nxpo, cfg.nypo, cfg.nlo, cfg.cyclic, cfg.fnot, cfg.beta, cfg.dxo, cfg.dto, cfg.delek,
                      cfg.bccooc, cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc, cfg.yporel())
        o.set_p(po, po)
        o.set_forcing(wek, zeros2, np.zeros(cfg.nlo - 1))
        kind, model = "port", o
    model.steps(1, 5)  # warm-up
    t0 = time.perf_counter()
    model.steps(6, 10)
    per = (time.perf_counter() - t0) / 10
    n = int(max(10, min(2000, budget_s / per)))
    t0 = time.perf_counter()
    model.steps(16, n)
    dt = time.perf_counter() - t0
    sps = n / dt
    # the same on ONE thread (SURVEY 8d asks for both): the OpenMP runtime is already in the process
    one = None
    try:
        def set_threads(k):
            if kind == "port":
                ob.set_threads(k)
            else:
                ref_binding.set_threads(k)  # applied on the thread that runs the reference (oracle/ref_binding.py)
        set_threads(1)
        model.steps(16 + n, 2)
        t0 = time.perf_counter()
        n1 = int(max(5, min(40, 4.0 / (per * min(cores, 8)))))
        model.steps(18 + n, n1)
        one = round(n1 / (time.perf_counter() - t0), 3)
        set_threads(cores)
    except Exception as e:  # noqa: BLE001
        print("cpu_baseline: single-thread timing skipped (%r)" % (e,), file=sys.stderr)
    return {"value": round(sps, 3), "unit": "steps/s", "cores": cores, "kind": kind, "cpu_model": cpu_model(), "value_1_thread": one,
            "ms_per_step": round(1e3 / sps, 4), "model_years_per_day": round(cfg.model_years_per_day(sps), 2),
            "sample": "%d ocean steps of the same %s workload (Gaussian-eddy IC, double-gyre wind), "
                      "%d OpenMP threads, %.1f s" % (n, WORKLOAD, cores, dt)}


def coupled_figure(cfg, po, wek, device, nocean=400):
    """double_gyre_coupled (BASELINE configs[3]): ocean steps/s of the coupled main loop (1 ocean + nstr atmospheric
    steps per ocean step, src/q-gcm.F:1220-1268) and the atmosphere's own step time."""
    import torch
    from qgcm_hip import AtmosModel, OceanModel, atmos_of, coupled_steps, share_gpu, synth
    at = atmos_of(cfg)
    f = synth.atmos_fields(at)
    a = AtmosModel(at, ddynat=f["ddynat"], device=device)
    a.set_p(f["pa"], f["pam"])
    a.set_forcing(f["wekpa"], f["entat"], f["xan"], f["txis"], f["txin"], f["enis"], f["enin"])
    o = OceanModel(cfg, device=device)
    o.set_p(po, po)
    o.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
    nstr = cfg.nstr
    a.steps(200, s0=1)                      # atmosphere alone: graphs of both averaging phases instantiated
    ms_a = a.time_steps(1200, s0=201)
    nt = 1401

    def timed(nt):
        coupled_steps(o, a, nt, 100 * nstr, nstr)   # warm-up of the coupled loop (instantiates the graphs of both halves)
        nt += 100 * nstr
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        coupled_steps(o, a, nt, nocean * nstr, nstr)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, nt + nocean * nstr
    dt_u, nt = timed(nt)                    # both halves on unrestricted streams: they queue for the same wave slots
    acu = share_gpu(o, a)                   # disjoint CU ranges (qgcm_hip_set_cu_range): each half keeps its own pace
    dt, nt = timed(nt)
    ok = bool(np.isfinite(a.get_state()[0]).all() and np.isfinite(o.get_state()[0]).all())
    a.close()
    o.close()
    return {"ocean_steps_per_s": round(nocean / dt, 2), "ms_per_ocean_step": round(1e3 * dt / nocean, 5),
            "atmos_steps_per_ocean_step": nstr, "atmos_alone_us_per_step": round(1e3 * ms_a / 1200, 3),
            "atmos_grid": [at.nxpa, at.nypa, at.nla], "model_years_per_day": round(cfg.model_years_per_day(nocean / dt), 1),
            "cu_partition": {"atmosphere_cus": acu, "ocean_steps_per_s_without_it": round(nocean / dt_u, 2)},
            "state_finite": ok, "note": "forcing held; ocean and atmosphere on their own HIP streams of one GPU, each on its own "
                                        "range of compute units (qgcm_hip_set_cu_range)"}


def natl1_one_slab_figure(device, nranks=8, nrep=12):
    """BASELINE configs[4] on ONE GPU: NAtl 1 km (4801 x 4801 x 3, dto = 180 s) cut into the eight y-slabs of the 8-GPU
    run; after real steps of all eight (virtual ranks on this GPU, the exchange buffers then hold consistent values) ONE
    middle slab steps alone - what one GPU of the eight computes per step, the two exchanges not included.  Four steps as
    one captured graph, HIP events, the state restored before every replay (a slab whose neighbours stand still leaves
    the real solution after 5-6 steps).  The 8-GPU figure derived from it is a PREDICTION and labelled so."""
    import torch
    from qgcm_hip import hostinit, preset, synth
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, global_consts, partition
    cfg = preset("natl1")
    consts = global_consts(cfg)
    po = synth.gaussian_eddy(cfg)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    scal = hostinit.constr(cfg, consts["amatoc"], po, po)
    slabs = [HipSlab(cfg, consts, g0, g1, r, nranks, device=device, sync_each_call=True) for r, (g0, g1) in enumerate(partition(cfg.nypo, nranks))]
    try:
        so = SlabOcean(cfg, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
        so.homsol()
        so.scatter_state(po, po, qo, qo, wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1), scal)
        del po, qo, wek
        so.steps(4, s0=1)
        torch.cuda.synchronize()
        r = nranks // 2
        x = slabs[r]
        x.sync_each_call = False
        st = torch.cuda.ExternalStream(x.stream_ptr)
        mine = so.th_gath[r][r * x.th_len:(r + 1) * x.th_len]
        state0, scal0 = x.get_state(), x.get_scalars()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            for _ in range(4):     # the stages of SlabOcean.step for this slab alone (steps without an averaging)
                x.stage(1, so.th_send[r])
                mine.copy_(so.th_send[r])   # its own summary is current, the other ranks' stay at the last real step
                x.stage(2, so.th_gath[r], so.h_to_lo[r], so.h_to_hi[r])
                x.stage(3, so.h_from_lo[r], so.h_from_hi[r], None, 0)
        e0, e1, tg = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), 0.0
        for _ in range(nrep):
            x.set_state(*state0)
            x.set_scalars(scal0)
            with torch.cuda.stream(st):
                e0.record()
                gr.replay()
                e1.record()
            e1.synchronize()
            tg += e0.elapsed_time(e1)
        us = 1e3 * tg / (4 * nrep)
        fin = bool(all(np.isfinite(f).all() for f in x.get_state()))
        npts = cfg.nxpo * (x.g1 - x.g0 + 1)
        return {"us_per_step_one_slab_alone": round(us, 2), "slab_rows": x.g1 - x.g0 + 1, "grid": [cfg.nxpo, cfg.nypo, cfg.nlo],
                "n_slabs": nranks, "state_finite": fin,
                "step_hbm_frac_of_8TBps": round(56 * npts * 8.0 / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                "measured": "one middle slab of the eight stepping alone on this GPU, four steps as one captured graph, "
                            "%d replays, HIP events; no collective in the window" % nrep,
                "PREDICTED_8_gpu_steps_per_s": round(1e6 / (us + 37.0), 1),
                "prediction_assumes": "two exchanges per step on the critical path, not measured here: all-gather of the slab "
                                      "summaries 25 us + halo send/recv 12 us (DESIGN 6b')"}
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())
        for sl in slabs:
            sl.close()


def pmc_traffic(kernel, name="pmc_traffic.json"):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc summary, if any."""
    path = os.path.join(ROOT, "profiles", name)
    try:
        return json.load(open(path)).get(kernel)
    except Exception:
        return None


def call_sequence_figure(model, s0, nsteps=400, nvalid=40):
    """What a drop-in executable gets: the reference main program's own call sequence through the C ABI - three
    eager calls per ocean step (call qgostep / call ocinvq / call ocqbdy, src/q-gcm.F:1243-1249), the leapfrog
    averaging of src/q-gcm.F:1328-1366 every 25th step and `valids` every nvalid = valday*86400/dto = 40 steps
    (src/q-gcm.F:657,1278) - no captured graphs, the host in the loop (here: Python over ctypes; the Fortran shim
    makes the same calls)."""
    def run(n, s):
        for _ in range(n):
            model.qgostep()
            model.ocinvq()
            model.ocqbdy()
            if (s - 1) % 25 == 0:
                model.lf_average()
            if s % nvalid == 0:
                model.valids()
            s += 1
        return s
    s = run(80, s0)
    model.sync()
    t0 = time.perf_counter()
    s = run(nsteps, s)
    model.sync()
    dt = time.perf_counter() - t0
    model.step_index = s
    return {"steps_per_s": round(nsteps / dt, 2), "ms_per_step": round(1e3 * dt / nsteps, 5), "steps": nsteps,
            "calls_per_step": "qgcm_hip_qgostep + qgcm_hip_ocinvq + qgcm_hip_ocqbdy, eager launches; "
                              "qgcm_hip_lf_average every 25th, qgcm_hip_valids every %d steps" % nvalid}


def calibrated_kernel_us(prof, nprof, step_ms):
    """Per-kernel microseconds from qgcm_hip_profile_steps' raw brackets: the bracket overhead is whatever makes the
    bracketed launches of the profiled steps add up to the graph-replayed step time (see main)."""
    prof = {k: v for k, v in prof.items() if not k.startswith("k_noop")}
    raw_ms = sum(v[0] for v in prof.values())
    nlaunch = sum(v[1] for v in prof.values())
    bracket_us = max(1e3 * (raw_ms - nprof * step_ms) / max(nlaunch, 1), 0.0)
    return {k: 1e3 * max(v[0] - 1e-3 * bracket_us * v[1], 0.0) / max(v[1], 1) for k, v in prof.items() if v[1]}, bracket_us


def slab_secondary(cfg, world, rank, local_rank, barrier, use_library, halo_p2p, nsteps, nwarm, bid, with_oml=False, overlap=False):
    """A secondary multi-GPU figure: the basin `cfg` cut into `world` y-slabs, one per rank, stepped by the driver
    the headline measurement settled on (library-issued RCCL exchanges if they were verified there, else
    torch.distributed).  Returns basin steps/s etc. (max over ranks); every rank must call it (collective)."""
    import torch
    import torch.distributed as dist
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import DistComm, HipSlab, SlabOcean, broadcast_unique_id, global_consts, partition
    t_setup = time.perf_counter()
    consts = global_consts(cfg)  # eigmod, bd2oc, yporel (host, init only); homsol runs on the slabs below
    po = synth.gaussian_eddy(cfg)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    scal = hostinit.constr(cfg, consts["amatoc"], po, po)
    g0, g1 = partition(cfg.nypo, world)[rank]
    slab = HipSlab(cfg, consts, g0, g1, rank, world, device=local_rank)
    if with_oml:  # ocean mixed layer on the slabs: one more (three numbers per rank) all-gather per step
        from qgcm_hip import oml_preset
        om = oml_preset(cfg)
        sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om)
        wekto, wek = synth.wekpo_from_tau(cfg, tx, ty)
        slab.oml_init(om)
    torch.cuda.set_stream(torch.cuda.ExternalStream(slab.stream_ptr, device=slab.device))
    so = SlabOcean(cfg, [slab], DistComm(halo_via_all_gather=not halo_p2p))
    if not cfg.cyclic:
        so.homsol()  # homogeneous solutions by the distributed Helmholtz solve itself (no host-side solver)
    # (channel: they are functions of y and came with global_consts - a tridiagonal solve per mode)
    driver = "torch.distributed (RCCL) between qgcm_hip_slab_stage calls"
    if use_library:
        so.use_library_exchanges(broadcast_unique_id(dist, slab.device))
        slab.set_halo_p2p(halo_p2p)
        slab.set_overlap(overlap)  # (the choice of the headline measurement; never applies with the mixed layer on)
        driver = "library-issued RCCL (qgcm_hip_slab_steps)"
    driver += ", halo rows by %s" % ("send/recv" if halo_p2p else "all-gather")
    so.scatter_state(po, po, qo, qo, wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1), scal)
    if cfg.cyclic:
        slab.set_cyc_forcing(*synth.tau_line_integrals(cfg, tx))
    if with_oml:
        slab.oml_set_state(sst, sstm)
        slab.oml_set_forcing(fnet, wekto, tx, ty)
    del po, qo, wek, consts
    t_setup = time.perf_counter() - t_setup
    so.steps(nwarm, s0=1)
    barrier()
    t0 = time.perf_counter()
    so.steps(nsteps, s0=nwarm + 1)
    barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    (_, _, fields), = so.gather_local()
    fin = torch.tensor([1.0 if all(np.isfinite(x).all() for x in fields) else 0.0], dtype=torch.float64, device="cuda")
    dist.all_reduce(fin, op=dist.ReduceOp.MIN)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())  # the slab's stream dies with the handle
    slab.close()
    wall = float(t.item())
    sps = nsteps / wall
    npts = cfg.nxpo * cfg.nypo
    return {"basin_steps_per_s": round(sps, 2), "ms_per_step": round(1e3 * wall / nsteps, 5), "steps": nsteps, "warmup": nwarm,
            "grid": [cfg.nxpo, cfg.nypo, cfg.nlo], "slab_rows": g1 - g0 + 1, "n_gpus": world, "dto_s": cfg.dto,
            "model_years_per_day": round(cfg.model_years_per_day(sps), 1), "state_finite": bool(fin.item() > 0.5),
            "step_hbm_frac_per_gpu": round(56 * npts * 8.0 * sps / world / 1e9 / HBM_PEAK_GBS, 4),
            "exchange_driver": driver, "host_setup_s": round(t_setup, 1), "config": bid}


def run_slabs(args, world, rank, local_rank, cfg5, real_stdout, barrier):
    """N > 1: y-slab decomposition, one rank per GPU over RCCL.

    `value` is BASELINE.json's metric: ocean timesteps/s of the FIXED NAtl 5 km basin (961 x 961 x 3) cut into `world`
    y-slabs ("scaling": "strong" - total work fixed; round 2 reported the weak-scaling figure here).  The ranks
    exchange slab summaries (tridiagonal sweeps + area integrals) and halo rows every step (qgcm_hip_slab_steps /
    qgcm_hip.slab.SlabOcean).  Secondary keys (--full): `weak_scaling_natl5_slab_per_gpu` (a NAtl-5km-shaped slab per
    GPU of a basin `world` times taller), NAtl 1 km, SOcn 5 km, the mixed layer."""
    import dataclasses

    import torch
    import torch.distributed as dist
    from qgcm_hip import hostinit, synth
    from qgcm_hip.slab import (DistComm, HipSlab, SlabOcean, broadcast_unique_id, global_consts, partition,
                               slab_slice)

    cfg_tall = dataclasses.replace(cfg5, name="natl5_x%d" % world, nyaooc=cfg5.nyaooc * world, nyta=cfg5.nyta * world)
    cfg = cfg5
    consts = global_consts(cfg)  # eigmod, bd2oc, yporel (host, init only); homsol runs on the slabs below
    po = synth.gaussian_eddy(cfg)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    scal = hostinit.constr(cfg, consts["amatoc"], po, po)
    g0, g1 = partition(cfg.nypo, world)[rank]
    slab = HipSlab(cfg, consts, g0, g1, rank, world, device=local_rank)
    # torch.distributed collectives are ordered on the library's own stream
    torch.cuda.set_stream(torch.cuda.ExternalStream(slab.stream_ptr, device=slab.device))
    so = SlabOcean(cfg, [slab], DistComm(halo_via_all_gather=False))  # halo rows: the two neighbours only
    so.homsol()  # homogeneous solutions by the distributed Helmholtz solve itself (no host-side solver)
    zero2, xon0 = np.zeros_like(wek), np.zeros(cfg.nlo - 1)

    def local_state():
        (_, _, fields), = so.gather_local()
        return fields + [slab.get_scalars()]

    def measure():
        """warm-up + exactly args.steps timed steps with the current driver; max over ranks; state check"""
        so.scatter_state(po, po, qo, qo, wek, zero2, xon0, scal)
        so.steps(args.warmup, s0=1)
        barrier()
        t0 = time.perf_counter()
        so.steps(args.steps, s0=args.warmup + 1)
        barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        (_, _, fields), = so.gather_local()
        fin = torch.tensor([1.0 if all(np.isfinite(x).all() for x in fields) else 0.0], dtype=torch.float64, device="cuda")
        dist.all_reduce(fin, op=dist.ReduceOp.MIN)
        return float(t.item()), bool(fin.item() > 0.5)

    extra = {}   # secondary figures (filled after the headline measurement)

    def line(wall, finite, driver, library_exchanges="ok"):
        basin_sps = args.steps / wall
        npts = cfg5.nxpo * cfg5.nypo
        return json.dumps({
            "metric": "ocean timesteps/sec (NAtl 5km 3-layer qgostep+ocinvq+ocqbdy)",
            "value": round(basin_sps, 2), "unit": "steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * wall / args.steps, 5),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "double_gyre_ocean_only NAtl 5km, 961x961x3 p-grid (the FIXED basin of BASELINE.json's "
                                   "metric) over %d y-slabs of ~%d rows, dto=540s, Gaussian-eddy IC + double-gyre wind, "
                                   "oml off" % (world, cfg.nypo // world),
                       "grid": [cfg.nxpo, cfg.nypo, cfg.nlo],
                       "parallelism": "y-slabs over %d GPUs: two exchanges per step - one all-gather of the slab summaries "
                                      "(tridiagonal sweeps + area integrals) and the halo rows with the two neighbours (RCCL)" % world,
                       "exchange_driver": driver,
                       "value_counts": "timesteps of the one fixed basin (not multiplied by n_gpus)"},
            "basin_steps_per_s": round(basin_sps, 2),
            "model_years_per_day": round(cfg5.model_years_per_day(basin_sps), 1),
            "state_finite": finite,
            "library_exchanges": library_exchanges,   # "ok" | "not tried" | "stalled" (watchdog) | "failed"
            "rccl_ranks": world if dist.get_backend() == "nccl" else 0,
            "step_hbm_frac_per_gpu": round(56 * npts * 8.0 * basin_sps / 1e9 / HBM_PEAK_GBS, 4),
            "roofline": None, "cpu_baseline": None, **extra,
        }) + "\n"

    # 1. The exchanges issued by Python (torch.distributed between the three stage calls): the plain, safe driver.
    #    Its measurement is kept as the line to print should anything below fail or stall.
    drv_torch = "torch.distributed (RCCL) between qgcm_hip_slab_stage calls"
    wall_t, fin_t = measure()
    best = (wall_t, fin_t, drv_torch)
    lib_status = "not tried"
    use_library = os.environ.get("QGCM_BENCH_EXCHANGES", "library") == "library" and dist.get_backend() == "nccl"
    if use_library:
        # 2. The exchanges issued by the library itself (qgcm_hip_slab_steps: RCCL from C++ on the same stream, the
        #    host out of the step loop). This path cannot be exercised on the one-GPU development box beyond a
        #    one-rank communicator, so it runs under a watchdog: if it stalls, every rank leaves and rank 0 prints
        #    the torch.distributed line measured above.
        import threading

        def bail():
            # The stall goes INTO the record (a SCALE file must not hide it) and the run fails: the value printed is
            # the torch.distributed measurement taken before, the exit code is non-zero. Nothing is restarted.
            if extra.get("halo_overlap", {}).get("status") == "trying":
                extra["halo_overlap"] = {"status": "STALLED (watchdog fired); the line is the measurement taken before the trial"}
            if rank == 0:
                real_stdout.write(line(best[0], best[1], best[2] + "; LIBRARY-ISSUED EXCHANGES STALLED (watchdog fired)",
                                       library_exchanges="stalled"))
                real_stdout.flush()
            print("bench.py: library-issued exchanges stalled; reported the torch.distributed measurement, exit 3", file=sys.stderr)
            os._exit(3)
        dog = threading.Timer(float(os.environ.get("QGCM_BENCH_WATCHDOG_S", "240")), bail)
        dog.daemon = True
        dog.start()
        nver = 27  # covers a pending exchange, its join and an averaging step (step 26) on real ranks
        so.scatter_state(po, po, qo, qo, wek, zero2, xon0, scal)
        so.steps(nver, s0=1)
        ref = local_state()
        so.scatter_state(po, po, qo, qo, wek, zero2, xon0, scal)
        ok = 1.0
        try:
            so.use_library_exchanges(broadcast_unique_id(dist, slab.device))
            so.steps(nver, s0=1)
            ok = 1.0 if all(np.array_equal(a, b) for a, b in zip(ref, local_state())) else 0.0
        except Exception as e:  # noqa: BLE001 - any failure means: stay with the torch.distributed driver
            print("library-issued exchanges unavailable: %r" % (e,), file=sys.stderr)
            ok = 0.0
        t = torch.tensor([ok], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        lib_status = "ok" if t.item() > 0.5 else "failed (see stderr); torch.distributed driver reported"
        if t.item() > 0.5:
            driver = "library-issued RCCL (qgcm_hip_slab_steps), verified bitwise against the torch.distributed driver"

            # transport of the halo rows: one all-gather of everybody's edge rows, or grouped send/recv with the
            # two neighbours - measured on this node (max over ranks), the faster one is used if it is also bitwise
            def timed(p2p, overlap=False):
                slab.set_halo_p2p(p2p)
                slab.set_overlap(overlap)
                so.scatter_state(po, po, qo, qo, wek, zero2, xon0, scal)
                so.steps(nver, s0=1)
                same = all(np.array_equal(a, b) for a, b in zip(ref, local_state()))
                so.steps(50, s0=nver + 1)
                barrier()
                t0 = time.perf_counter()
                so.steps(100, s0=nver + 51)
                barrier()
                tt = torch.tensor([time.perf_counter() - t0, 0.0 if same else 1.0], dtype=torch.float64, device="cuda")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                return float(tt[0].item()), tt[1].item() < 0.5
            try:
                t_ag, ok_ag = timed(False)
                t_pp, ok_pp = timed(True)
                # neighbour send/recv is the default transport (it moves 2 edge messages per rank, the all-gather
                # nranks of them); the all-gather is taken only if it is measurably (> 2 %) faster on this node
                use_p2p = ok_pp and (t_pp <= 1.02 * t_ag or not ok_ag)
                slab.set_halo_p2p(use_p2p)
                driver += "; halo rows by %s (all-gather %.1f us/step, send/recv %.1f us/step%s)" % (
                    "send/recv" if use_p2p else "all-gather", 1e4 * t_ag, 1e4 * t_pp, "" if ok_pp else ", send/recv NOT bitwise")
            except Exception as e:  # noqa: BLE001
                print("halo transport tuning failed: %r" % (e,), file=sys.stderr)
                slab.set_halo_p2p(False)
            slab.set_overlap(False)
            wall_l, fin_l = measure()
            driver += "; torch.distributed driver: %.1f us/step" % (1e6 * wall_t / args.steps)
            try:  # what the exchanges cost by themselves on this node (for the record)
                pr = slab.comm_probe(200)
                driver += "; exchanges alone: summaries all-gather %.1f us, halo all-gather %.1f us, halo send/recv %.1f us" % tuple(pr)
            except Exception as e:  # noqa: BLE001
                print("exchange probe failed: %r" % (e,), file=sys.stderr)
            if fin_l and wall_l <= wall_t:
                best = (wall_l, fin_l, driver)
            else:
                best = (wall_t, fin_t, drv_torch + "; library-issued driver: %.1f us/step" % (1e6 * wall_l / args.steps))
            # Last, with the line above already in hand (a stall from here on prints THAT line, marked): the halo exchange
            # on a second stream under the inner tile rows of the next step's tendency launch (qgcm_hip_comm_set_overlap).
            # Never run between different GPUs before this node; kept only if bitwise and faster.
            if best[2].startswith("library") and os.environ.get("QGCM_BENCH_NO_OVERLAP_TRIAL") != "1":
                extra["halo_overlap"] = {"status": "trying"}
                try:
                    use_p2p = "halo rows by send/recv" in driver
                    t_base, _ = timed(use_p2p, False)
                    t_ov, ok_ov = timed(use_p2p, True)
                    use_ov = ok_ov and t_ov < t_base
                    slab.set_overlap(use_ov)
                    extra["halo_overlap"] = {"status": "ok", "used": bool(use_ov), "bitwise": bool(ok_ov),
                                             "us_per_step_plain": round(1e4 * t_base, 2), "us_per_step_overlapped": round(1e4 * t_ov, 2)}
                    if use_ov:
                        wall_o, fin_o = measure()
                        if fin_o and wall_o < best[0]:
                            best = (wall_o, fin_o, driver + "; halo exchange overlapped with the next step's inner tendency tiles "
                                    "(%.1f vs %.1f us/step)" % (1e6 * wall_o / args.steps, 1e6 * wall_l / args.steps))
                        else:
                            slab.set_overlap(False)
                            extra["halo_overlap"]["used"] = False
                except Exception as e:  # noqa: BLE001
                    print("overlap trial failed: %r" % (e,), file=sys.stderr)
                    extra["halo_overlap"] = {"status": "failed: %r" % (e,)}
                    slab.set_overlap(False)
        dog.cancel()
    dist.barrier()
    # ---- secondary figures: NOT `value`; same driver as the headline chose ------------------------------------------
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())  # the slab's stream dies with the handle
    slab.close()
    lib_ok = lib_status == "ok" and best[2].startswith("library")
    p2p = "halo rows by send/recv" in best[2]
    ovl = bool(lib_ok and extra.get("halo_overlap", {}).get("used", False))
    if args.full and os.environ.get("QGCM_BENCH_NO_SECONDARY") != "1":
        import threading
        from qgcm_hip import preset

        def bail2():  # a stall in a secondary figure: the headline line goes out with the stall recorded, exit 3
            extra["secondary_figures"] = "STALLED (watchdog fired)"
            if rank == 0:
                real_stdout.write(line(*best, library_exchanges=lib_status))
                real_stdout.flush()
            os._exit(3)
        dog2 = threading.Timer(float(os.environ.get("QGCM_BENCH_WATCHDOG2_S", "420")), bail2)
        dog2.daemon = True
        dog2.start()
        # (1) weak scaling: a NAtl-5km-shaped slab (961 x ~960 rows) per GPU of a basin `world` times taller
        try:
            w = slab_secondary(cfg_tall, world, rank, local_rank, barrier, lib_ok, p2p, 400, 100,
                               "NAtl 5km-shaped slab per GPU: 961 x %d x 3 basin (%d x taller)" % (cfg_tall.nypo, world), overlap=ovl)
            w["natl5_equivalent_steps_per_s"] = round(world * w["basin_steps_per_s"], 2)  # = n_gpus x basin timesteps
            extra["weak_scaling_natl5_slab_per_gpu"] = w
        except Exception as e:  # noqa: BLE001 - secondary figure only
            extra["weak_scaling_natl5_slab_per_gpu"] = {"error": repr(e)}
        # (2) BASELINE configs[4]: NAtl 1 km (4801 x 4801 x 3, dto = 180 s) over the GPUs of the node; one slab may hold
        #     at most 2048 interior rows (single-segment Thomas kernel), i.e. at least 3 GPUs
        if world >= 3:
            try:
                extra["natl1km"] = slab_secondary(preset("natl1"), world, rank, local_rank, barrier, lib_ok, p2p, 100, 20,
                                                  "NAtl 1km ocean-only, 3 layers, y-slabs over %d GPUs" % world, overlap=ovl)
            except Exception as e:  # noqa: BLE001
                extra["natl1km"] = {"error": repr(e)}
        # (2b) the fixed NAtl 5 km basin with the ocean mixed layer on the slabs (three exchanges per step)
        try:
            extra["strong_scaling_natl5_mixed_layer"] = slab_secondary(cfg5, world, rank, local_rank, barrier, lib_ok, p2p, 200, 60,
                                                                       "NAtl 5km + ocean mixed layer, fixed basin over %d GPUs" % world, with_oml=True)
        except Exception as e:  # noqa: BLE001
            extra["strong_scaling_natl5_mixed_layer"] = {"error": repr(e)}
        # (3) BASELINE configs[2]: Southern Ocean 5 km periodic channel (4609 x 577 x 3) cut into `world` slabs
        try:
            extra["socn5_cyclic_slabs"] = slab_secondary(preset("socn5"), world, rank, local_rank, barrier, lib_ok, p2p, 200, 40,
                                                         "SOcn 5km cyclic channel, fixed basin over %d GPUs" % world, overlap=ovl)
        except Exception as e:  # noqa: BLE001
            extra["socn5_cyclic_slabs"] = {"error": repr(e)}
        dog2.cancel()
    if rank == 0:
        real_stdout.write(line(*best, library_exchanges=lib_status))
        real_stdout.flush()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--warmup", type=int, default=160)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline, per-kernel times, secondary figures and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the state after the last timed step to DIR/<name>.npy (one GPU)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    real_stdout = divert_stdout()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus %d must be launched with torch.distributed.run (WORLD_SIZE=%d)"
                             % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
    if os.environ.get("QGCM_BENCH_SAME_GPU") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    # QGCM_BENCH_FORCE_SLABS=1 routes a 1-rank run through the y-slab code path (rehearsal of
    # the multi-GPU plumbing on a one-GPU box; needs the torch.distributed.run environment)
    force_slabs = os.environ.get("QGCM_BENCH_FORCE_SLABS") == "1"
    if world > 1 or force_slabs:
        if args.dump_outputs:
            raise SystemExit("bench.py --dump-outputs is implemented for the one-GPU path only")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # QGCM_BENCH_BACKEND=gloo + QGCM_BENCH_SAME_GPU=1: rehearsal of the multi-rank code path with
        # all ranks on one card (RCCL refuses duplicate devices); production is nccl = RCCL over xGMI
        backend = os.environ.get("QGCM_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from qgcm_hip import OceanModel, preset
    cfg = preset(WORKLOAD)

    def barrier():
        if world > 1 or force_slabs:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1 or force_slabs:
        run_slabs(args, world, rank, local_rank, cfg, real_stdout, barrier)
        return

    po, wek = synthetic_inputs(cfg)
    model = OceanModel(cfg, device=local_rank)
    model.set_p(po, po)
    model.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))

    model.steps(args.warmup, s0=1)
    # Untimed rehearsal of the timed call: the same number of steps, then filler steps up to a multiple of 50, so that
    # the timed region starts at the same position of the 25-step averaging cycle with the same buffer rotation and
    # replays exactly the HIP graphs the rehearsal built and has already run once (graphs are keyed by block length,
    # (s0-1) mod 25 and the rotation state).  Round 2 captured and instantiated the tail graphs INSIDE the window
    # (BENCH_r02: 97.1 us/step by wall against 79.2 us/step by HIP events).
    # The rehearsal is repeated until at least 200 untimed steps (~15 ms) have run: a 20-step window right after 5
    # warm-up steps otherwise measures the GPU's clock ramp (76 us/step by HIP events against 69.7 in steady state).
    s_timed = args.warmup + 1
    done = 0
    while True:
        model.steps(args.steps, s0=s_timed)
        fill = (-args.steps) % 50
        model.steps(fill, s0=s_timed + args.steps)
        s_timed += args.steps + fill
        done += args.steps + fill
        if done >= 200:
            break
    model.prepare_steps(args.steps, s0=s_timed)  # (a no-op after the rehearsal; kept as the explicit guarantee)
    barrier()
    t0 = time.perf_counter()
    ev_ms = model.time_steps(args.steps, s0=s_timed)  # HIP events on the library's stream
    barrier()
    wall = time.perf_counter() - t0
    state = model.get_state()
    finite = bool(all(np.isfinite(x).all() for x in state))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, state, model.get_scalars())

    npts = cfg.nxpo * cfg.nypo
    steps_per_s = world * args.steps / wall
    out = {
        "metric": "ocean timesteps/sec (NAtl 5km 3-layer qgostep+ocinvq+ocqbdy)",
        "value": round(steps_per_s, 2), "unit": "steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(1e3 * wall / args.steps, 5),
        # (the basin is fixed as N grows - BASELINE.json's metric: the N > 1 lines say "strong" too)
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "double_gyre_ocean_only NAtl 5km, 961x961x3 p-grid, dto=540s, "
                               "Gaussian-eddy IC + double-gyre wind, oml off",
                   "grid": [cfg.nxpo, cfg.nypo, cfg.nlo],
                   "parallelism": "single GPU"},
        "model_years_per_day": round(cfg.model_years_per_day(steps_per_s), 1),
        "hip_event_ms_per_step": round(ev_ms / args.steps, 5),
        # steps run before the timed window opens: --warmup + the untimed rehearsal of the timed call (graph
        # capture / instantiation and the GPU's clock ramp stay outside the window, see above)
        "untimed_steps_before_window": args.warmup + done,
        "launch_mode": "HIP graphs: %d x 50-step block(s) + %s, %d eager step(s); built and replayed once before the window" % (
            args.steps // 50, ("one %d-step block" % ((args.steps % 50) & ~1)) if (args.steps % 50) >= 2 else "no tail block",
            (args.steps % 50) % 2),
        "state_finite": finite,
        "step_hbm_frac": round(56 * npts * 8.0 * (args.steps / (ev_ms * 1e-3)) / 1e9 / HBM_PEAK_GBS, 4),
    }
    # ---- --full: per-kernel HIP-event timing for the roofline entry, then the secondary figures ---------
    if args.full:
        nprof = 100
        prof = model.profile_steps(nprof, s0=s_timed + args.steps)
        # Every launch is bracketed by two HIP events on the library's stream. An event record is a packet of its
        # own, so a raw bracket reads kernel + record overhead. The overhead per bracket is calibrated on the timed
        # region itself: the same steps replayed from HIP graphs (no brackets, no gaps) take ev_ms/steps each, so
        #     overhead = (sum of all raw brackets of the profiled steps - profiled steps x graph step time) / launches.
        # With it the per-kernel times add up to the measured step time; they land within ~2 % of rocprofv3's
        # kernel durations (profiles/). An empty launch bracketed the same way (k_noop) and a train of empty
        # launches in one bracket are reported beside it for reference.
        noop_us = 1e3 * prof["k_noop"][0] / max(prof["k_noop"][1], 1)
        train_us = 1e3 * prof["k_noop_train"][0] / max(prof["k_noop_train"][1], 1)
        prof = {k: v for k, v in prof.items() if not k.startswith("k_noop")}
        raw_ms = sum(v[0] for v in prof.values())
        nlaunch = sum(v[1] for v in prof.values())
        bracket_us = max(1e3 * (raw_ms - nprof * ev_ms / args.steps) / max(nlaunch, 1), 0.0)
        prof = {k: (max(v[0] - 1e-3 * bracket_us * v[1], 0.0), v[1]) for k, v in prof.items()}
        dom = max(prof, key=lambda k: prof[k][0])
        tot_ms, nl = prof[dom]
        avg_us = 1e3 * tot_ms / max(nl, 1)
        # `achieved` divides the bytes this kernel HAS to move (its compulsory traffic, "own": the time levels rotate
        # instead of being copied, so k_tend moves 21 fields, not the 24 of SURVEY 8d's reference-algorithm count) by
        # the launch time; rocprofv3 --pmc confirms that figure (`traffic`). The SURVEY count is kept as a labelled
        # secondary: it credits bytes the kernel never touches and once exceeded the measured copy bandwidth.
        f_survey, f_own = ALGO_FIELDS[dom]
        abytes = f_own * npts * 8.0
        achieved = abytes / (avg_us * 1e-6) / 1e9
        copy_gbs = model.copy_bandwidth(1 << 30, 10)
        # what a PURE streaming kernel with this kernel's read : write mix (15 fields read, 6 written, nothing else)
        # reaches on buffers of this workload's field size: the practical ceiling beside the nominal 8 TB/s
        mix = {"k_tend": (15, 6), "k_dst_fwd": (3, 3), "k_thomas": (3, 3), "k_dst_inv": (5, 3)}.get(dom)
        stream_gbs = model.stream_mix_bandwidth(mix[0], mix[1], npts * 8, 20) if mix else None
        out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(dom),
                           "traffic_source": "committed rocprofv3 --pmc collection of this command (profiles/pmc_traffic.json, "
                                             "profiles/collect.sh), not measured in this run",
                           "avg_launch_us": round(avg_us, 3), "algorithmic_bytes_per_launch": abytes,
                           "reference_algorithm_bytes_per_launch": f_survey * npts * 8.0,
                           "frac_reference_algorithm_bytes": round(f_survey * npts * 8.0 / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                           "measured_copy_GBps": round(copy_gbs, 1),
                           "measured_stream_same_mix_GBps": round(stream_gbs, 1) if stream_gbs else None,
                           "frac_of_measured_stream": round(achieved / stream_gbs, 4) if stream_gbs else None,
                           "event_bracket_us": {"subtracted_per_launch": round(bracket_us, 3),
                                                "calibration": "bracketed kernel times sum to the graph-replayed step time",
                                                "empty_launch_bracketed": round(noop_us, 3),
                                                "empty_launch_in_train": round(train_us, 3)},
                           "kernel_us": {k: round(1e3 * v[0] / max(v[1], 1), 3) for k, v in prof.items()}}
        secondary = os.environ.get("QGCM_BENCH_NO_SECONDARY") != "1"  # profiles/collect.sh profiles the main workload only
        # Secondary figure: the rate of the reference's own call sequence (what a drop-in q-gcm executable sees)
        try:
            if not secondary:
                raise RuntimeError("skipped (QGCM_BENCH_NO_SECONDARY=1)")
            out["call_sequence"] = call_sequence_figure(model, model.step_index)
        except Exception as e:  # noqa: BLE001 - secondary figure only
            out["call_sequence"] = {"error": repr(e)}
        # Secondary figure (not `value`): the same workload with the ocean mixed layer on the device
        # (`call oml`) - the end-to-end ocean-only step without any per-step PCIe traffic.
        try:
            if not secondary:
                raise RuntimeError("skipped (QGCM_BENCH_NO_SECONDARY=1)")
            from qgcm_hip import oml_preset, synth
            om = oml_preset(cfg)
            sst, sstm, fnet, tx, ty = synth.mixed_layer_fields(cfg, om)
            wekto, _ = synth.wekpo_from_tau(cfg, tx, ty)
            model.oml_init(om)
            model.oml_set_state(sst, sstm)
            model.oml_set_forcing(fnet, wekto, tx, ty)
            model.set_p(po, po)
            model.steps(300, s0=1)  # warm-up: the three 50-step graphs of the sst buffer rotation get instantiated
            ms = model.time_steps(args.steps, s0=301)
            pr2 = model.profile_steps(50, s0=301 + args.steps)
            st_ok = bool(np.isfinite(model.oml_get_state()[0]).all())
            # `call oml` on the device: k_oml_step (reads sstm, sst, po(1), tauxo, tauyo, fnetoc, wekto; writes sst, the raw
            # entrainment: 9 fields) and k_oml_entoc (reads the entrainment, writes entoc: 2 fields) - own bytes, live
            # HIP-event brackets minus the calibrated bracket cost (src/omlsubs.F:47-763)
            us_a = 1e3 * pr2["k_oml"][0] / max(pr2["k_oml"][1], 1) - bracket_us
            us_b = 1e3 * pr2["k_oml_entoc"][0] / max(pr2["k_oml_entoc"][1], 1) - bracket_us
            nT = cfg.nxto * cfg.nyto * 8.0
            out["with_mixed_layer"] = {"steps_per_s": round(args.steps / (ms * 1e-3), 2),
                                       "ms_per_step": round(ms / args.steps, 5), "state_finite": st_ok,
                                       "mixed_layer_us_per_step": round(1e3 * (ms / args.steps - ev_ms / args.steps), 3),
                                       "oml_kernels_us_bracketed": round(us_a + us_b, 3),
                                       "roofline": [{"bound": "hbm", "kernel": k, "achieved": round(f * nT / (u * 1e-6) / 1e9, 1),
                                                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(f * nT / (u * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                                     "avg_launch_us": round(u, 3), "algorithmic_bytes_per_launch": f * nT,
                                                     "traffic": pmc_traffic(k, "pmc_traffic_oml.json"),
                                                     "traffic_source": "committed rocprofv3 --pmc collection (profiles/pmc_traffic_oml.json), if any"}
                                                    for k, f, u in (("k_oml_step", 9, us_a), ("k_oml_entoc", 2, us_b))]}
        except Exception as e:  # noqa: BLE001 - secondary figure only
            out["with_mixed_layer"] = {"error": repr(e)}
        # Secondary figure: BASELINE configs[2], the zonally cyclic Southern Ocean channel at 5 km (4609 x 577 x 3)
        try:
            if not secondary:
                raise RuntimeError("skipped (QGCM_BENCH_NO_SECONDARY=1)")
            from qgcm_hip import synth as _synth
            cfg_s = preset("socn5")
            ms_ = OceanModel(cfg_s, device=local_rank)
            po_s = _synth.gaussian_eddy(cfg_s)
            tx_s, ty_s = _synth.wind_stress(cfg_s)
            _, wek_s = _synth.wekpo_from_tau(cfg_s, tx_s, ty_s)
            ms_.set_p(po_s, po_s)
            ms_.set_forcing(wek_s, np.zeros_like(wek_s), np.zeros(cfg_s.nlo - 1))
            ms_.set_cyc_forcing(*_synth.tau_line_integrals(cfg_s, tx_s))
            ms_.steps(100, s0=1)
            t_s = ms_.time_steps(400, s0=101)
            pr_s, _ = calibrated_kernel_us(ms_.profile_steps(50, s0=501), 50, t_s / 400)
            stream_s = ms_.stream_mix_bandwidth(15, 6, cfg_s.nxpo * cfg_s.nypo * 8, 10)
            ok_s = bool(np.isfinite(ms_.get_state()[0]).all())
            ms_.close()
            out["socn5_cyclic"] = {"steps_per_s": round(400 / (t_s * 1e-3), 2), "ms_per_step": round(t_s / 400, 5),
                                   "grid": [cfg_s.nxpo, cfg_s.nypo, cfg_s.nlo], "state_finite": ok_s,
                                   "kernel_us": {k: round(v, 2) for k, v in pr_s.items()}}
            # The NAtl 5 km working set (172 MB) sits in the 256 MiB Infinity Cache, so the headline `roofline` is not an
            # HBM measurement; at SOcn 5 km (4609 x 577 x 3: 21 fields = 447 MB for the same kernel) it is.
            nb_s = ALGO_FIELDS["k_tend"][1] * cfg_s.nxpo * cfg_s.nypo * 8.0
            ach_s = nb_s / (pr_s["k_tend"] * 1e-6) / 1e9
            out["roofline_hbm_bound"] = {"bound": "hbm", "kernel": "k_tend", "workload": "SOcn 5km cyclic channel 4609x577x3 (BASELINE configs[2])",
                                         "achieved": round(ach_s, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": round(ach_s / HBM_PEAK_GBS, 4), "avg_launch_us": round(pr_s["k_tend"], 3),
                                         "algorithmic_bytes_per_launch": nb_s,
                                         "measured_stream_same_mix_GBps": round(stream_s, 1),
                                         "frac_of_measured_stream": round(ach_s / stream_s, 4),
                                         "traffic": pmc_traffic("k_tend", "pmc_traffic_socn5.json"),
                                         "traffic_source": "committed rocprofv3 --pmc collection (profiles/pmc_traffic_socn5.json), "
                                                           "not measured in this run"}
        except Exception as e:  # noqa: BLE001 - secondary figure only
            out["socn5_cyclic"] = {"error": repr(e)}
        # Secondary figure: BASELINE configs[3] double_gyre_coupled - the NAtl 5 km ocean under the 385 x 97 x 3
        # atmosphere, three atmospheric steps (qgastep, atinvq, atqzbd) per ocean step, both on this
        # GPU on their own streams, forcing held (xforc / aml / oml belong to the host side of a coupled run).
        try:
            if not secondary:
                raise RuntimeError("skipped (QGCM_BENCH_NO_SECONDARY=1)")
            out["coupled"] = coupled_figure(cfg, po, wek, local_rank)
        except Exception as e:  # noqa: BLE001 - secondary figure only
            out["coupled"] = {"error": repr(e)}
        # Secondary figure: BASELINE configs[4] (NAtl 1 km over 8 GPUs) as far as ONE GPU can measure it
        try:
            if not secondary:
                raise RuntimeError("skipped (QGCM_BENCH_NO_SECONDARY=1)")
            out["natl1km_one_slab_of_8"] = natl1_one_slab_figure(local_rank)
        except Exception as e:  # noqa: BLE001 - secondary figure only
            out["natl1km_one_slab_of_8"] = {"error": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            model.close()
            out["cpu_baseline"] = cpu_baseline(cfg, po, wek)
    real_stdout.write(json.dumps(out) + "\n")
    real_stdout.flush()


if __name__ == "__main__":
    main()
