"""Worker of tests/test_gpu_qocdiag.py: ONE PROCESS PER SLAB on the same GPU (torch.distributed, gloo).  Each rank
steps its slab through SlabOcean over DistComm, then SlabOcean.vorticity_budget / ocean_dump assemble the basin.  The
same decomposition also runs as virtual ranks inside this process, and a whole-domain OceanModel holds their gathered
state; the assembled results must equal the whole-domain handle's bitwise on every rank.
usage (under torch.distributed.run): mp_qocdiag_worker.py <preset>"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from qgcm_hip import OceanModel, hostinit, preset, synth  # noqa: E402
from qgcm_hip.slab import DistComm, HipSlab, LocalComm, SlabOcean, global_consts, partition  # noqa: E402


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)


def main():
    rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    cfg = preset(sys.argv[1])
    po = synth.gaussian_eddy(cfg, noise=1e-2)
    pom = np.asfortranarray(0.99 * po)
    tx, ty = synth.wind_stress(cfg)
    wekto, wek = synth.wekpo_from_tau(cfg, tx, ty)
    sst = np.asfortranarray(np.full((cfg.nxto, cfg.nyto), 15.0) + 0.1 * np.arange(cfg.nyto)[None, :])
    consts = global_consts(cfg)
    qo = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], po)
    qom = hostinit.q_from_p(cfg, consts["amatoc"], consts["yporel"], consts["ddynoc"], pom)
    scal = hostinit.constr(cfg, consts["amatoc"], po, pom)
    ent = np.asfortranarray(1e-7 * np.sin(np.arange(cfg.nxpo * cfg.nypo)).reshape(cfg.nxpo, cfg.nypo))
    xon = np.zeros(cfg.nlo - 1)
    parts = partition(cfg.nypo, P)

    def prepare(so):
        so.homsol()
        so.scatter_state(po, pom, qo, qom, wek, ent, xon, scal)
        for x in so.slabs:
            x.set_monitor_fields(tx, ty, wekto, sst)

    vs = [HipSlab(cfg, consts, g0, g1, r, P, sync_each_call=True) for r, (g0, g1) in enumerate(parts)]
    vo = SlabOcean(cfg, vs, LocalComm(P, after=torch.cuda.synchronize))
    prepare(vo)
    g0, g1 = parts[rank]
    slab = HipSlab(cfg, consts, g0, g1, rank, P, device=0)
    torch.cuda.set_stream(torch.cuda.ExternalStream(slab.stream_ptr, device=slab.device))
    so = SlabOcean(cfg, [slab], DistComm(halo_via_all_gather=True))
    prepare(so)
    ok = True
    for nst in (1, 27):  # crosses the averaging after step 26
        so.steps(nst)
        vo.steps(nst)
        st = [np.zeros((cfg.nxpo, cfg.nypo, cfg.nlo), order="F") for _ in range(4)]
        for a0, a1, arrs in vo.gather_local():
            for a, b in zip(st, arrs):
                a[:, a0 - 1:a1, :] = b
        m = OceanModel(cfg)
        m.set_state(*st)
        m.set_forcing(wek, ent, xon)
        m.set_monitor_fields(tx, ty, wekto, sst)
        for nsko in (1, 2, 5):
            ok = ok and same(so.vorticity_budget(nsko), m.vorticity_budget(nsko))
            ok = ok and same(so.ocean_dump(nsko), m.ocean_dump(nsko))
            ok = ok and same(vo.vorticity_budget(nsko), m.vorticity_budget(nsko))
        m.close()
    t = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("MP_QOCDIAG_RESULT", "OK" if t.item() > 0.5 else "MISMATCH", flush=True)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())
    slab.close()
    for v in vs:
        v.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
