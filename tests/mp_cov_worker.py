"""Worker of tests/test_gpu_cov.py: ONE PROCESS PER SLAB on the same GPU (torch.distributed, gloo).  Each rank loads
its rows of the state in <dir>/state.npz (po, pom, qo, qom of NAtl 5 km and an sst), accumulates three covocn
contributions through SlabOcean over DistComm (row sums, one all-gather, the combine on every rank, the update of the
matrix rows the rank holds), then assembles the matrices and writes covariance() to <dir>/out<rank>.npz.
usage: mp_cov_worker.py <rank> <dir>   (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT in the environment)"""
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from qgcm_hip import preset  # noqa: E402
from qgcm_hip.slab import DistComm, HipSlab, SlabOcean, global_consts, partition, slab_slice  # noqa: E402


def main():
    rank, P = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    out_dir = sys.argv[2]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    cfg = preset("natl5")
    st = np.load(os.path.join(out_dir, "state.npz"))
    g0, g1 = partition(cfg.nypo, P)[rank]
    slab = HipSlab(cfg, global_consts(cfg), g0, g1, rank, P, device=0)
    torch.cuda.set_stream(torch.cuda.ExternalStream(slab.stream_ptr, device=slab.device))
    so = SlabOcean(cfg, [slab], DistComm(halo_via_all_gather=True))
    sl = slab_slice(cfg.nypo, g0, g1)
    slab.set_state(*[np.asfortranarray(st[k][:, sl]) for k in ("po", "pom", "qo", "qom")])
    slab.set_monitor_fields(sst=st["sst"])
    so.enable_covariance(16)
    for _ in range(3):
        so.covocn()
    got = so.covariance()
    np.savez(os.path.join(out_dir, "out%d.npz" % rank), **{k: np.asarray(v) for k, v in got.items()})
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())
    slab.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
