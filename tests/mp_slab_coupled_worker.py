"""Worker of tests/test_gpu_slab_coupled_native.py:test_two_ranks_two_processes: one process per slab, ONE GPU PER
PROCESS, RCCL between them.  Each process runs the coupled window of cpl_tiny on its slab twice - driven from Python
over DistComm ("nccl"), and by the library (use_library_exchanges + use_library_coupling) - and compares the two at the
slab tests' bars; the replicas of the atmosphere must be bit-equal across the ranks.
usage (under torch.distributed.run, two processes): mp_slab_coupled_worker.py"""
import dataclasses
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (os.path.join(ROOT, "q-gcm_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import numpy_heat as nh  # noqa: E402
import test_gpu_slab_coupled as tsc  # noqa: E402
from common import atm_apply, load_golden  # noqa: E402
from qgcm_hip import AtmosModel, OceanModel, config, oml_preset  # noqa: E402
from qgcm_hip.slab import DistComm, HipSlab, SlabOcean, broadcast_unique_id, global_consts, partition  # noqa: E402

NT0, N, NSTR = 73, 30, 3


def build(rank, P, dev):
    """tests/test_gpu_slab_coupled.py:_cpl_tiny for this process's slab on device `dev`."""
    g, h = load_golden("cpl_tiny"), nh.load("heat_cpl_tiny")
    Q = nh.params(h)
    oc, at = config.preset("cpl_tiny"), config.atmos_preset("cpl_tiny")
    f = {k: g["in_" + k] for k in ("pa", "pam", "wekpa", "entat", "ddynat", "xan", "txis", "txin", "enis", "enin")}
    sst = 22.0 + 0.5 * h["in_sstm"]
    zero, xon = np.zeros_like(g["in_wekpo"]), np.zeros(oc.nlo - 1)
    o = OceanModel(oc, device=dev)
    try:
        o.set_p(g["in_po"], g["in_pom"])
        o.set_forcing(g["in_wekpo"], zero, xon)
        consts, st, scal = global_consts(oc, o.helmholtz), o.get_state(), o.get_scalars()
    finally:
        o.close()
    g0, g1 = partition(oc.nypo, P)[rank]
    slab = HipSlab(oc, consts, g0, g1, rank, P, device=dev)
    slab.oml_init(oml_preset(oc))
    torch.cuda.set_stream(torch.cuda.ExternalStream(slab.stream_ptr, device=slab.device))
    so = SlabOcean(oc, [slab], DistComm())
    so.scatter_state(st[0], st[1], st[2], st[3], g["in_wekpo"], zero, xon, scal)
    slab.oml_set_state(sst=sst, sstm=sst)
    a = AtmosModel(at, ddynat=f["ddynat"], device=dev)
    atm_apply(a, f)
    r = at.dxa / (Q["ndxr"] * Q["dxo"])
    am = dataclasses.replace(tsc._aml_cfg(Q), at2d=Q["at2d"] * r * r, at4d=Q["at4d"] * r ** 4, ahmd=Q["ahmd"] * r * r)
    a.aml_init(am, xc1ast=h["in_xc1ast"], dtopat=h["in_dtopat"])
    a.aml_set_state(**{k: h["in_" + k] for k in tsc.STATE})
    so.xforc_setup([a])
    so.xforc_heat_setup(tsc._heat_cfg(Q))
    return so, a


def main():
    rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", rank))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=P)
    res = []
    for native in (False, True):
        so, a = build(rank, P, dev)
        slab = so.slabs[0]
        if native:
            so.use_library_exchanges(broadcast_unique_id(dist, slab.device))
            so.use_library_coupling()
        so.coupled_steps(NT0, N, NSTR, xforc=True)
        slab.sync()
        res.append(tsc._collect(slab.get_state(), slab.oml_get_state(), a))
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())
        slab.close()
        a.close()
    ok = True
    try:
        tsc._window_close(res[1], res[0], "rank %d: library window against the Python-driven one" % rank)
    except AssertionError as e:
        print("rank", rank, e, flush=True)
        ok = False
    # the replicas: rank 0's ast of the library window on every rank
    t = torch.from_numpy(np.ascontiguousarray(res[1]["aml"][0])).to("cuda:%d" % dev)
    ref = t.clone()
    dist.broadcast(ref, src=0)
    ok = ok and bool(torch.equal(t.view(torch.int64), ref.view(torch.int64)))
    ok = ok and all(np.isfinite(v).all() for v in res[1]["ocean"])
    flag = torch.tensor([1.0 if ok else 0.0], device="cuda:%d" % dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("MP_SLAB_COUPLED_RESULT", "OK" if flag.item() > 0.5 else "MISMATCH", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
