"""y-slab decomposition of the ocean hot path across GPUs (one process per GPU).

The reference is a single-process OpenMP code; this decomposition is new design
(SURVEY 8e).  Rank r owns a contiguous range of rows j for all i and layers - x is
never split, so the tendency kernel, the row transforms and the unpack stay local.
Per ocean step the ranks exchange

  * the slab summaries of the tridiagonal sweeps along y and of the area integrals (ONE
    all-gather of 7*nlo*nk doubles: both sweeps and the column sums are linear in the
    values entering a slab, see k_thomas.h, instead of two all-to-all transposes of the
    whole work array and an all-reduce); every rank derives bit-identical constraint
    coefficients from it,
  * halo rows of the new po (3 rows: del-6 of the lagged field) and qo (1 row).

The exchanges are issued either from here (torch.distributed between the stage calls) or
by the library itself (`use_library_exchanges`: RCCL from C++, qgcm_hip_slab_steps).

`SlabOcean` is the orchestration; it is independent of where the slab kernels
run (`HipSlab`: the C ABI on a GPU) and of the transport (`LocalComm`: several
slabs in one process, used to test the decomposition on one GPU; `DistComm`:
torch.distributed, "nccl" = RCCL over xGMI on the GPU node, "gloo" in CPU tests).
All message buffers are torch tensors.

Import order: torch bundles its own HIP runtime; a process that uses torch (these transports do) must import it
before the first OceanModel / HipSlab loads libqgcm_hip.so, otherwise torch reports "No HIP GPUs are available".
"""
import ctypes as C

import numpy as np

from . import hostinit
from .handle import TAV_LAYOUT, Handle, _dp, subsample_count
from .lib import check, load_library
from .model import cfl_dict, cov_row_split, prsamp_dict, unpack_monitors

HALO = 3


def partition(nyg, nranks):
    """Global row ranges (1-based, inclusive) of the y-slabs: near-equal, contiguous."""
    base, rem = divmod(nyg, nranks)
    out, g = [], 1
    for r in range(nranks):
        n = base + (1 if r < rem else 0)
        out.append((g, g + n - 1))
        g += n
    return out


def owned_rows_tile(rows, nyg):
    """rows[r] = (g0, g1), the global p rows rank r owns: raises unless they tile 1 .. nyg in rank order; returns the
    longest range (the common row count of a message that carries every rank's owned rows)."""
    nxt = 1
    for r, (g0, g1) in enumerate(rows):
        if g0 != nxt or g1 < g0:
            raise ValueError("rank %d owns rows %d..%d: the slabs' owned rows do not tile 1..%d" % (r, g0, g1, nyg))
        nxt = g1 + 1
    if nxt != nyg + 1:
        raise ValueError("the slabs' owned rows end at %d, the basin has %d" % (nxt - 1, nyg))
    return max(g1 - g0 + 1 for g0, g1 in rows)


def local_rows(nyg, g0, g1):
    """(nyl, joff, jlo, jhi): local array rows, global = local + joff, owned local range."""
    hlo = HALO if g0 > 1 else 0
    hhi = HALO if g1 < nyg else 0
    return (g1 - g0 + 1) + hlo + hhi, g0 - hlo - 1, hlo + 1, hlo + (g1 - g0 + 1)


def slab_slice(nyg, g0, g1):
    """numpy slice (0-based) of the global rows held locally (owned + halos)."""
    nyl, joff, _, _ = local_rows(nyg, g0, g1)
    return slice(joff, joff + nyl)


# --------------------------------------------------------------------------
# transports
# --------------------------------------------------------------------------
class LocalComm:
    """All slabs live in this process (virtual ranks)."""

    def __init__(self, nranks, after=None):
        self.nranks = nranks
        self.local_ranks = list(range(nranks))
        self.after = after  # e.g. torch.cuda.synchronize when the buffers are device tensors

    def all_gather(self, gath, send):
        n = send[0].numel()
        for g in gath:
            for r, s in enumerate(send):
                g[r * n:(r + 1) * n].copy_(s)
        if self.after:
            self.after()

    def halo_exchange(self, to_lo, to_hi, from_lo, from_hi):
        for r in range(self.nranks):
            if r > 0:
                from_lo[r].copy_(to_hi[r - 1])
            if r < self.nranks - 1:
                from_hi[r].copy_(to_lo[r + 1])
        if self.after:
            self.after()


class DistComm:
    """One slab per process over torch.distributed (backend nccl = RCCL, or gloo)."""

    def __init__(self, group=None, halo_via_all_gather=False):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.nranks = dist.get_world_size(group)
        self.local_ranks = [self.rank]
        # halo rows either as point-to-point send/recv with the two neighbours or as ONE
        # all-gather of everybody's edge rows (2 x 92 KB per rank at 5 km: cheaper than two
        # latency-bound p2p launches on xGMI, and it uses a single collective type)
        self.halo_via_all_gather = halo_via_all_gather
        self._hsend = self._hgath = None
        # gloo moves device tensors through the host and is not ordered on the slab's HIP stream (rehearsals of the
        # multi-rank path on one GPU, CPU tests): bracket its collectives with device synchronisations. nccl = RCCL
        # is stream-ordered and needs none.
        self.host_staged = dist.get_backend(group) != "nccl"

    def _fence(self):
        if self.host_staged:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize()

    def _all_gather(self, gath, send):
        if self.host_staged and send.is_cuda:  # gloo: explicit host staging (its device-tensor path is not reliable)
            import torch
            h = torch.empty(gath.numel(), dtype=gath.dtype)
            self.dist.all_gather_into_tensor(h, send.cpu(), group=self.group)
            gath.copy_(h)
        else:
            self.dist.all_gather_into_tensor(gath, send, group=self.group)

    def all_gather(self, gath, send):
        self._fence()
        self._all_gather(gath[0], send[0])
        self._fence()

    def halo_exchange(self, to_lo, to_hi, from_lo, from_hi):
        self._fence()
        try:
            return self._halo_exchange(to_lo, to_hi, from_lo, from_hi)
        finally:
            self._fence()

    def _halo_exchange(self, to_lo, to_hi, from_lo, from_hi):
        if self.halo_via_all_gather:
            return self._halo_all_gather(to_lo, to_hi, from_lo, from_hi)
        d, r = self.dist, self.rank
        stage = self.host_staged and (to_lo[0] if to_lo[0] is not None else to_hi[0]).is_cuda
        sl = (to_lo[0].cpu() if stage else to_lo[0]) if r > 0 else None
        sh = (to_hi[0].cpu() if stage else to_hi[0]) if r < self.nranks - 1 else None
        rl = (from_lo[0].cpu() if stage else from_lo[0]) if r > 0 else None
        rh = (from_hi[0].cpu() if stage else from_hi[0]) if r < self.nranks - 1 else None
        ops = []
        if r > 0:
            ops += [d.P2POp(d.isend, sl, r - 1, self.group), d.P2POp(d.irecv, rl, r - 1, self.group)]
        if r < self.nranks - 1:
            ops += [d.P2POp(d.isend, sh, r + 1, self.group), d.P2POp(d.irecv, rh, r + 1, self.group)]
        if ops:
            for w in d.batch_isend_irecv(ops):
                w.wait()
        if stage:
            if r > 0:
                from_lo[0].copy_(rl)
            if r < self.nranks - 1:
                from_hi[0].copy_(rh)

    def _halo_all_gather(self, to_lo, to_hi, from_lo, from_hi):
        r, P = self.rank, self.nranks
        ref = to_lo[0] if to_lo[0] is not None else to_hi[0]
        n = ref.numel()
        if self._hsend is None:
            self._hsend = ref.new_zeros(2 * n)
            self._hgath = ref.new_zeros(2 * n * P)
            if ref.is_cuda:  # fills run on torch's current stream: settle before the slab's stream writes (SlabOcean._settle)
                import torch
                torch.cuda.synchronize()
        if to_lo[0] is not None:
            self._hsend[:n].copy_(to_lo[0])
        if to_hi[0] is not None:
            self._hsend[n:].copy_(to_hi[0])
        self._all_gather(self._hgath, self._hsend)
        if r > 0:  # what the lower neighbour sent upwards
            from_lo[0].copy_(self._hgath[(2 * (r - 1) + 1) * n:(2 * (r - 1) + 2) * n])
        if r < P - 1:  # what the upper neighbour sent downwards
            from_hi[0].copy_(self._hgath[(2 * (r + 1)) * n:(2 * (r + 1) + 1) * n])


def rccl_unique_id():
    """The rendezvous id of qgcm_hip_comm_unique_id (call on rank 0, hand to every rank)."""
    buf = C.create_string_buffer(128)
    check(load_library().qgcm_hip_comm_unique_id(buf, 128))
    return buf.raw


def broadcast_unique_id(dist, device, group=None):
    """rank 0 creates the id, torch.distributed carries it to the others."""
    import torch
    t = torch.zeros(128, dtype=torch.uint8, device=device)
    if dist.get_rank(group) == 0:
        t.copy_(torch.frombuffer(bytearray(rccl_unique_id()), dtype=torch.uint8))
    dist.broadcast(t, src=0, group=group)
    return bytes(t.cpu().numpy().tobytes())


# --------------------------------------------------------------------------
# one slab on one GPU through the C ABI
# --------------------------------------------------------------------------
class HipSlab(Handle):
    """The slab kernels of include/qgcm_hip.h ("y-slab building blocks") on the handle that owns the global rows
    g0..g1; what it shares with the whole-domain OceanModel is Handle's."""

    def __init__(self, cfg, consts, g0, g1, rank, nranks, device=-1, sync_each_call=False):
        import torch
        self.torch = torch
        self.g0, self.g1, self.consts = g0, g1, consts
        self.sync_each_call = sync_each_call
        _, self.joff, self.jlo, self.jhi = local_rows(cfg.nypo, g0, g1)
        Handle.__init__(self, cfg, consts, device, g=(g0, g1), p_rows=slab_slice(cfg.nypo, g0, g1), rank=rank, nranks=nranks)
        if cfg.cyclic:
            self.set_homog_cyc(consts)
        elif "ochom" in consts:  # global homogeneous solutions given; else SlabOcean.homsol() computes them on the slabs
            self.set_homog_box(consts)
        self.device = torch.device("cuda", torch.cuda.current_device() if device < 0 else device)
        self.cst_len = self.L.qgcm_hip_thomas_const_len(self.h)
        self.stream_ptr = self.L.qgcm_hip_stream(self.h)
        self.oml_on = False
        self._msg_lens()

    def _msg_lens(self):
        self.th_len = self.L.qgcm_hip_thomas_msg_len(self.h)
        self.halo_len = self.L.qgcm_hip_halo_msg_len(self.h)

    def wrk_fill(self, v):
        check(self.L.qgcm_hip_wrk_fill(self.h, float(v))); self._done()

    def area_integrals(self):
        x = np.zeros(self.cfg.nlo)
        check(self.L.qgcm_hip_area_integrals(self.h, _dp(x)))
        return x

    # buffers -------------------------------------------------------------
    def new_buffer(self, n):
        return self.torch.zeros(int(n), dtype=self.torch.float64, device=self.device)

    @staticmethod
    def _ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _done(self):
        if self.sync_each_call:
            check(self.L.qgcm_hip_sync(self.h))

    def oml_init(self, om):
        """Switch the mixed layer on for this slab (before SlabOcean sizes its message buffers)."""
        Handle.oml_init(self, om)
        self.oml_on = True
        self._msg_lens()
        self.oml_len = self.L.qgcm_hip_oml_msg_len(self.h)

    # covariance matrices: this rank's row sums and the combine (Handle: the matrix rows this rank holds)
    def cov_part_len(self):
        n = self.L.qgcm_hip_cov_part_len(self.h)
        if n < 0:
            check(1)
        return n

    def cov_part(self, send):
        """This rank's row sums -> send (device buffer of cov_part_len() doubles); asynchronous."""
        check(self.L.qgcm_hip_cov_part(self.h, self._ptr(send)))
        self._done()

    def cov_combine(self, gath):
        """All ranks' row sums (rank-major) -> the means everywhere and the update of the rows this rank holds."""
        check(self.L.qgcm_hip_cov_combine(self.h, self._ptr(gath), int(self.nranks)))
        self._done()

    # diagnostics: the ocean monitors, valids, prsamp, areavg and cfl as per-rank summaries (SlabOcean.diagnostic)
    def diag_part_len(self, kind):
        return {"monitors": self.L.qgcm_hip_monitor_part_len, "valids": self.L.qgcm_hip_valids_part_len,
                "prsamp": self.L.qgcm_hip_prsamp_part_len, "areavg": self.L.qgcm_hip_areavg_part_len,
                "cfl": self.L.qgcm_hip_cfl_part_len}[kind](self.h)

    def diag_part(self, kind, send, cflcrit=0.8):
        """This rank's summary of `kind` -> send (device buffer of diag_part_len(kind) doubles); asynchronous."""
        if kind == "cfl":
            check(self.L.qgcm_hip_cfl_part(self.h, float(cflcrit), self._ptr(send)))
            self._done()
            return
        fn = {"monitors": self.L.qgcm_hip_monitors_part, "valids": self.L.qgcm_hip_valids_part,
              "prsamp": self.L.qgcm_hip_prsamp_part, "areavg": self.L.qgcm_hip_areavg_part}[kind]
        check(fn(self.h, self._ptr(send)))
        self._done()

    def diag_combine(self, kind, gath, cflcrit=0.8):
        """All ranks' summaries (rank-major) -> the whole-domain call's packed result (valids: (solnok, out); areavg:
        (averages, numerators, denominators); cfl: the dict of OceanModel.cfl)."""
        nl, P = self.cfg.nlo, self.nranks
        if kind == "areavg":
            n = self.L.qgcm_hip_areavg_count(self.h)
            avg, num, den = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
            check(self.L.qgcm_hip_areavg_combine(self.h, self._ptr(gath), P, _dp(avg), _dp(num), _dp(den)))
            return avg[:n], num[:n], den[:n]
        if kind == "cfl":
            nq = self.L.qgcm_hip_cfl_len(self.h)
            mx, nb, loc = np.zeros(nq), np.zeros(nq, dtype=np.int32), np.zeros(2 * nq, dtype=np.int32)
            ip = C.POINTER(C.c_int)
            check(self.L.qgcm_hip_cfl_combine(self.h, self._ptr(gath), P, float(cflcrit), _dp(mx), nb.ctypes.data_as(ip),
                                              loc.ctypes.data_as(ip)))
            return cfl_dict(self.cfg, mx, nb, loc)
        if kind == "monitors":
            out = np.zeros(self.L.qgcm_hip_monitor_len(self.h))
            check(self.L.qgcm_hip_monitors_combine(self.h, self._ptr(gath), P, _dp(out)))
            return out
        if kind == "valids":
            out, ok = np.zeros(14 + nl), C.c_int()
            check(self.L.qgcm_hip_valids_combine(self.h, self._ptr(gath), P, _dp(out), C.byref(ok)))
            return bool(ok.value), out
        out = np.zeros(4 * nl + 2)
        check(self.L.qgcm_hip_prsamp_combine(self.h, self._ptr(gath), P, _dp(out)))
        return out

    # xforc under a replicated atmosphere (SlabOcean.xforc): `atm` is this rank's AtmosModel --------------
    def xforc_init(self, atm, p):
        check(self.L.qgcm_hip_xforc_slab_init(self.h, atm.h, C.byref(p)))

    def xforc_heat_init(self, atm, p, arrays=None):
        """p: lib.XforcHeatParams; arrays: what it points to (fsa, fso, xta, yta, xto, yto), unused here."""
        check(self.L.qgcm_hip_xforc_heat_slab_init(self.h, atm.h, C.byref(p)))

    def xforc_bands_init(self, atm, band, nrow):
        """Switch this pair to the banded atmosphere side (qgcm_hip_xforc_slab_bands): band = (a0, a1) and
        nrow from lib.xforc_bands."""
        check(self.L.qgcm_hip_xforc_slab_bands(self.h, atm.h, int(band[0]), int(band[1]), int(nrow), int(self.nranks)))

    # tau_udiff on slabs: the basin's pom(:,:,1) assembled on every rank ahead of the part
    def xforc_udiff_init(self, atm, nrow, nranks):
        """Switch the shear term on for this pair (qgcm_hip_xforc_slab_udiff), after xforc_init with tau_udiff = 0: nrow =
        the longest owned p-row range of any rank."""
        check(self.L.qgcm_hip_xforc_slab_udiff(self.h, atm.h, int(nrow), int(nranks)))

    def xforc_pom_len(self, atm):
        n = C.c_long()
        check(self.L.qgcm_hip_xforc_slab_pom_len(self.h, atm.h, C.byref(n)))
        return int(n.value)

    def xforc_pom_pack(self, atm, send):
        """This slab's owned rows of pom(:,:,1) behind their header -> send (device buffer of xforc_pom_len doubles);
        asynchronous, on the atmosphere's stream."""
        check(self.L.qgcm_hip_xforc_slab_pom_pack(self.h, atm.h, self._ptr(send)))

    def xforc_pom_assemble(self, atm, gath):
        """All ranks' rows (rank-major) -> the assembled pom(:,:,1) the next xforc_part reads."""
        check(self.L.qgcm_hip_xforc_slab_pom_assemble(self.h, atm.h, self._ptr(gath), int(self.nranks)))

    # tau_udiff without that gather: the stress above the owned rows, rank-ordered partial sums
    def xforc_sums_init(self, atm, rows):
        """Switch this pair to the owner-computed sums (qgcm_hip_xforc_slab_sums), after xforc_init with tau_udiff = 0:
        rows[r] = (g0, g1), the global ocean p rows rank r owns; the library keeps this rank's part of lib.xforc_sums."""
        n = len(rows)
        lo, hi = (C.c_int * n)(*[int(a) for a, _ in rows]), (C.c_int * n)(*[int(b) for _, b in rows])
        check(self.L.qgcm_hip_xforc_slab_sums(self.h, atm.h, int(self.rank), n, lo, hi))

    def xforc_edge_len(self, atm):
        n = C.c_long(0)
        check(self.L.qgcm_hip_xforc_slab_edge_len(self.h, atm.h, C.byref(n)))
        return int(n.value)

    def xforc_edge_pack(self, atm, send):
        """The first 4 and the last 4 owned rows of pom(:,:,1) behind their header -> send (device buffer of
        xforc_edge_len doubles); asynchronous, on the atmosphere's stream."""
        check(self.L.qgcm_hip_xforc_slab_edge_pack(self.h, atm.h, self._ptr(send)))

    def xforc_edge_assemble(self, atm, gath):
        """The slab's owned rows and the neighbours' edge rows (gath: all ranks' messages, rank-major) -> rows
        g0 - 4 .. g1 + 4 of the array the next xforc_part reads."""
        check(self.L.qgcm_hip_xforc_slab_edge_assemble(self.h, atm.h, self._ptr(gath), int(self.nranks)))

    def xforc_msg_len(self, atm):
        return self.L.qgcm_hip_xforc_slab_msg_len(atm.h)

    def xforc_part(self, atm, send):
        """The momentum half, fnetoc and this rank's partial cell sums -> send (device buffer of xforc_msg_len doubles,
        None without the heat half); asynchronous, on the atmosphere's stream.  Banded (xforc_bands_init): the atmosphere
        side on this rank's windows only, and its band of the coarse fields in front of the cell sums in `send`."""
        check(self.L.qgcm_hip_xforc_slab_part(self.h, atm.h, self._ptr(send)))

    def xforc_combine(self, atm, gath):
        """All ranks' partial cell sums (rank-major) -> fnetat and the monitors on this rank's replica.  Banded: first every
        rank's band of the coarse fields and the line sums into the replica; required without the heat half too."""
        check(self.L.qgcm_hip_xforc_slab_combine(self.h, atm.h, self._ptr(gath), int(self.nranks)))

    def xforc_fetch(self, atm, heat):
        """dict of the last xforc's outputs (qgcm_hip_xforc_slab_get): the momentum half's, or (heat) the heat half's."""
        from .model import HEAT_SCALARS, XFORC_FIELDS, XFORC_INTEGRALS
        c, o, nyl = atm.cfg, self.cfg, self.nyl
        shapes = dict(tauxa=(c.nxpa, c.nypa), tauya=(c.nxpa, c.nypa), uekat=(c.nxpa, c.nyta), vekat=(c.nxta, c.nypa),
                      wekta=(c.nxta, c.nyta), wekpa=(c.nxpa, c.nypa), tauxo=(o.nxpo, nyl), tauyo=(o.nxpo, nyl),
                      wekto=(o.nxto, nyl - 1), wekpo=(o.nxpo, nyl))
        if heat:
            fo, fa, sc = np.zeros((o.nxto, nyl - 1), order="F"), np.zeros((c.nxta, c.nyta), order="F"), np.zeros(4)
            check(self.L.qgcm_hip_xforc_slab_get(self.h, atm.h, *([None] * 11 + [_dp(fo), _dp(fa), _dp(sc)])))
            return dict(fnetoc=fo, fnetat=fa, **{k: float(v) for k, v in zip(HEAT_SCALARS, sc)})
        d = {n: np.zeros(shapes[n], order="F") for n in XFORC_FIELDS}
        txi = np.zeros(4)
        check(self.L.qgcm_hip_xforc_slab_get(self.h, atm.h, *([_dp(d[n]) for n in XFORC_FIELDS] + [_dp(txi), None, None, None])))
        d.update({n: float(txi[k]) for k, n in enumerate(XFORC_INTEGRALS)})
        return d

    # slab kernels -------------------------------------------------------------
    def thomas_phase(self, phase, gath, send):
        check(self.L.qgcm_hip_thomas_phase(self.h, int(phase), self._ptr(gath), self._ptr(send), self.rank, self.nranks))
        self._done()

    def thomas_consts(self, dst):
        """This slab's right-hand-side independent summary constants -> dst (device buffer of cst_len doubles)."""
        check(self.L.qgcm_hip_thomas_consts(self.h, self._ptr(dst))); self._done()

    def set_thomas_consts(self, gath):
        """All ranks' constants (rank-major); once after set-up."""
        check(self.L.qgcm_hip_set_thomas_consts(self.h, self._ptr(gath), self.nranks)); self._done()

    def constr(self):
        check(self.L.qgcm_hip_constr(self.h)); self._done()

    def unpack(self, fuse_ocqbdy=True):
        check(self.L.qgcm_hip_unpack(self.h, int(fuse_ocqbdy))); self._done()

    def halo_pack(self, to_lo, to_hi):
        check(self.L.qgcm_hip_halo_pack(self.h, self._ptr(to_lo), self._ptr(to_hi))); self._done()

    def halo_unpack(self, from_lo, from_hi):
        check(self.L.qgcm_hip_halo_unpack(self.h, self._ptr(from_lo), self._ptr(from_hi))); self._done()

    # exchanges issued by the library itself (RCCL on its own stream) ---------------
    def comm_init(self, comm_id):
        """Collective over all ranks' handles; comm_id = rccl_unique_id() of rank 0."""
        check(self.L.qgcm_hip_comm_init(self.h, comm_id, len(comm_id), self.rank, self.nranks))
        self.has_comm = True

    def comm_probe(self, reps=200):
        """The step's exchanges back to back (collective): us per summaries all-gather, halo all-gather, halo send/recv."""
        us = (C.c_double * 3)()
        check(self.L.qgcm_hip_comm_probe(self.h, int(reps), us))
        return [us[0], us[1], us[2]]

    def set_halo_p2p(self, on):
        check(self.L.qgcm_hip_comm_set_halo_p2p(self.h, int(on)))

    def set_overlap(self, on):
        """Library-issued exchanges: halo exchange on a second stream under the next step's inner tendency tiles."""
        check(self.L.qgcm_hip_comm_set_overlap(self.h, int(on)))

    def slab_steps(self, s0, n):
        check(self.L.qgcm_hip_slab_steps(self.h, int(s0), int(n)))
        self._done()

    # the coupled window driven by the library ---------------------------
    def coupled_init(self, atm):
        """Size the window's exchange buffers for this slab and its replica (qgcm_hip_slab_coupled_init): after comm_init
        and every xforc set-up call."""
        check(self.L.qgcm_hip_slab_coupled_init(self.h, atm.h))

    def coupled_steps(self, atm, nt0, n, nstr, xforc):
        """One window (qgcm_hip_slab_coupled_steps): collective, asynchronous."""
        check(self.L.qgcm_hip_slab_coupled_steps(self.h, atm.h, int(nt0), int(n), int(nstr), int(bool(xforc))))
        self._done()

    def stage(self, n, a=None, b=None, c=None, flags=0):
        """One C call per communication-free stage (qgcm_hip_slab_stage)."""
        check(self.L.qgcm_hip_slab_stage(self.h, int(n), self._ptr(a), self._ptr(b), self._ptr(c), self.rank, self.nranks, int(flags)))
        self._done()


# --------------------------------------------------------------------------
# orchestration
# --------------------------------------------------------------------------
def tend_tile_rows(cfg, g0, g1):
    """Tile rows of the tendency launch on the slab of global rows g0..g1 (k_tend.h tend_tiling: 16-row tiles; the
    northern wall row of a box basin is peeled off when it would open a tile row of its own)."""
    rows = g1 - g0 + 1
    peel = (not cfg.cyclic) and rows % 16 == 1 and rows > 1 and g1 == cfg.nypo
    return rows // 16 if peel else -(-rows // 16)


class SlabOcean:
    """The distributed ocean step.  `slabs` are the slab objects this process owns
    (one per local rank of `comm`); a slab object provides the methods of HipSlab."""

    def __init__(self, cfg, slabs, comm, stream_ctx=None):
        self.cfg, self.slabs, self.comm = cfg, slabs, comm
        self.P = comm.nranks
        nl = cfg.nlo
        self.stream_ctx = stream_ctx  # context manager factory that makes torch's current stream the slab's stream
        self.th_send = [s.new_buffer(s.th_len) for s in slabs]
        self.th_gath = [s.new_buffer(s.th_len * self.P) for s in slabs]
        self.h_to_lo = [s.new_buffer(s.halo_len) if s.rank > 0 else None for s in slabs]
        self.h_to_hi = [s.new_buffer(s.halo_len) if s.rank < self.P - 1 else None for s in slabs]
        self.h_from_lo = [s.new_buffer(s.halo_len) if s.rank > 0 else None for s in slabs]
        self.h_from_hi = [s.new_buffer(s.halo_len) if s.rank < self.P - 1 else None for s in slabs]
        # mixed layer (HipSlab.oml_init on every slab BEFORE this constructor): one more small all-gather per step
        self.oml_on = all(getattr(s, "oml_on", False) for s in slabs)
        if self.oml_on:
            self.om_send = [s.new_buffer(s.oml_len) for s in slabs]
            self.om_gath = [s.new_buffer(s.oml_len * self.P) for s in slabs]
        self._settle()
        self.step_index = 1
        # the right-hand-side independent part of the slab summaries is exchanged once
        if self.P > 1:
            cs_send = [s.new_buffer(s.cst_len) for s in slabs]
            cs_gath = [s.new_buffer(s.cst_len * self.P) for s in slabs]
            self._settle()
            for i, x in enumerate(slabs):
                x.thomas_consts(cs_send[i])
            self._comm(comm.all_gather, cs_gath, cs_send)
            for i, x in enumerate(slabs):
                x.set_thomas_consts(cs_gath[i])
            for x in slabs:
                x.sync()

    @staticmethod
    def _settle():
        """torch zero-fills a new buffer on ITS current stream - the null stream unless the caller made the slab's
        stream current - and the slabs' streams are non-blocking: not ordered against it.  A kernel that writes into a
        fresh buffer could be overtaken by the fill.  Wait for the fills before the buffers are used."""
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        except ImportError:  # numpy-backed slabs of the CPU tests
            pass

    def _comm(self, fn, *a):
        if self.stream_ctx is None:
            fn(*a)
        else:
            with self.stream_ctx():
                fn(*a)

    def step(self, s):
        S, cm = self.slabs, self.comm
        if self.oml_on:  # `call oml` precedes qgostep (src/q-gcm.F:1232): its mean entrainment is a basin-wide number
            for i, x in enumerate(S):
                x.stage(10, self.om_send[i])
            self._comm(cm.all_gather, self.om_gath, self.om_send)
            for i, x in enumerate(S):
                x.stage(11, self.om_gath[i])
        if getattr(self, "_halo_pending", False):
            # early_tend: the halo rows of the previous step have not been unpacked yet - the inner tile rows of the
            # tendency launch do not read them (stage 4); then halo rows in (stage 3) and the rest of stage 1 (stage 5)
            for x in S:
                x.stage(4)
            for i, x in enumerate(S):
                x.stage(3, self.h_from_lo[i], self.h_from_hi[i], None, 0)
            self._halo_pending = False
            for i, x in enumerate(S):
                x.stage(5, self.th_send[i])
        else:
            for i, x in enumerate(S):  # tendency, forward row transform, slab summary of the y sweeps
                x.stage(1, self.th_send[i])
        self._comm(cm.all_gather, self.th_gath, self.th_send)
        # both sweeps + basin-wide area integrals, constraints, inverse row transform,
        # modes -> layers (+ boundary PV), halo rows out
        for i, x in enumerate(S):
            x.stage(2, self.th_gath[i], self.h_to_lo[i], self.h_to_hi[i])
        if self.P > 1:
            self._comm(cm.halo_exchange, self.h_to_lo, self.h_to_hi, self.h_from_lo, self.h_from_hi)
        avg = 1 if (s - 1) % 25 == 0 else 0
        if (getattr(self, "early_tend", False) and self.P > 1 and not avg and not self.oml_on
                and all(tend_tile_rows(self.cfg, x.g0, x.g1) >= 3 for x in S)):
            self._halo_pending = True  # stage 3 of this step follows stage 4 of the next one (the order the library's
            return                     # overlapped exchange produces, qgcm_hip_comm_set_overlap)
        if self.P > 1 or avg:
            for i, x in enumerate(S):  # halo rows in, leapfrog averaging every 25th step
                x.stage(3, self.h_from_lo[i], self.h_from_hi[i], None, avg)

    def _join(self):
        if getattr(self, "_halo_pending", False):
            for i, x in enumerate(self.slabs):
                x.stage(3, self.h_from_lo[i], self.h_from_hi[i], None, 0)
            self._halo_pending = False

    # diagnostics, collective: every rank calls them between steps() calls and gets the same result --------------
    def diagnostic(self, kind, **kw):
        """kind = "monitors", "valids", "prsamp", "areavg" or "cfl" (kw: cflcrit): every local slab writes its summary,
        one all-gather, every local slab combines the gathered buffer.  Returns the list of the local slabs' results
        (bitwise the same)."""
        S = self.slabs
        bufs = getattr(self, "_diag_bufs", None)
        if bufs is None:
            bufs = self._diag_bufs = {}
        if kind not in bufs:
            n = [x.diag_part_len(kind) for x in S]
            bufs[kind] = ([x.new_buffer(m) for x, m in zip(S, n)], [x.new_buffer(m * self.P) for x, m in zip(S, n)])
            self._settle()
        send, gath = bufs[kind]
        self._join()  # the halo rows the scans read must be current
        for i, x in enumerate(S):
            x.diag_part(kind, send[i], **kw)
        for x in S:  # the summaries are complete before a transport reads them (LocalComm copies on torch's stream)
            x.sync()
        self._comm(self.comm.all_gather, gath, send)
        return [x.diag_combine(kind, gath[i], **kw) for i, x in enumerate(S)]

    def monitors(self):
        """As OceanModel.monitors(): the ocean half of monnc_comp and couroc over the whole basin."""
        return unpack_monitors(self.diagnostic("monitors")[0], self.cfg.nlo)

    def valids(self):
        """As OceanModel.valids(): (solnok, out)."""
        return self.diagnostic("valids")[0]

    def prsamp(self):
        """As OceanModel.prsamp()."""
        return prsamp_dict(self.diagnostic("prsamp")[0], self.cfg.nlo)

    def set_areas(self, xlo=None, xhi=None, ylo=None, yhi=None, tables=None):
        """As OceanModel.set_areas, on every local slab."""
        return [x.set_areas(xlo, xhi, ylo, yhi, tables) for x in self.slabs][0]

    def area_averages(self, parts=False):
        """As OceanModel.area_averages(): one all-gather of 29 doubles per rank."""
        r = self.diagnostic("areavg")[0]
        return r if parts else r[0]

    def cfl(self, cflcrit=0.8):
        """As OceanModel.cfl(): bitwise the whole-domain result."""
        return self.diagnostic("cfl", cflcrit=cflcrit)[0]

    # time averages: every rank sums its owned rows; a readout assembles the basin with one all-gather
    def _assemble(self, parts):
        """parts[i]: dict name -> owned-row array (rows on axis 1) of local slab i.  One all-gather of the packed arrays
        (g0, g1, then every field padded to the largest slab's rows); returns dict name -> whole-basin array."""
        S, cfg = self.slabs, self.cfg
        grids = dict(TAV_LAYOUT)
        names = sorted(parts[0])
        rmax = max(g1 - g0 + 1 for g0, g1 in partition(cfg.nypo, self.P))
        rmax = max([rmax] + [x.g1 - x.g0 + 1 for x in S])
        tail = lambda a: a.shape[2] if a.ndim == 3 else 1
        sizes = [(n, parts[0][n].shape[0], tail(parts[0][n])) for n in names]
        ln = 2 + sum(nx * rmax * k for _, nx, k in sizes)
        send, gath = [], []
        for x, d in zip(S, parts):
            v = np.zeros(ln)
            v[0], v[1] = x.g0, x.g1
            o = 2
            for n, nx, k in sizes:
                buf = np.zeros((nx, rmax, k), order="F")
                a = d[n].reshape(nx, -1, k, order="F")
                buf[:, :a.shape[1], :] = a
                v[o:o + nx * rmax * k] = buf.ravel(order="F")
                o += nx * rmax * k
            t = x.new_buffer(ln)
            t.copy_(x.torch.from_numpy(v))
            send.append(t)
            gath.append(x.new_buffer(ln * self.P))
        self._settle()
        self._comm(self.comm.all_gather, gath, send)
        g = gath[0].cpu().numpy().reshape(self.P, ln)
        out = {}
        o = 2
        for n, nx, k in sizes:
            tgrid = grids.get(n) in ("t", "u")  # T-row fields: one row fewer on the rank that owns row nypo
            full = np.zeros((nx, cfg.nyto if tgrid else cfg.nypo, k), order="F")
            for r in range(self.P):
                g0, g1 = int(g[r, 0]), int(g[r, 1])
                rows = g1 - g0 + 1 - (1 if tgrid and g1 == cfg.nypo else 0)
                blk = g[r, o:o + nx * rmax * k].reshape(nx, rmax, k, order="F")
                full[:, g0 - 1:g0 - 1 + rows, :] = blk[:, :rows, :]
            out[n] = full if parts[0][n].ndim == 3 else full[:, :, 0]
            o += nx * rmax * k
        return out

    def enable_po_mean(self, on=True):
        for x in self.slabs:
            x.enable_po_mean(on)

    def po_mean(self, reset=False, count=False):
        """As OceanModel.po_mean: the whole basin's running mean of po, assembled from the owned rows (collective)."""
        self._join()
        res = [x.po_mean(reset) for x in self.slabs]
        a = self._assemble([{"po": m} for m, _ in res])["po"]
        return (a, res[0][1]) if count else a

    def set_time_mean_params(self, oml=None, **kw):
        for x in self.slabs:
            x.set_time_mean_params(oml, **kw)

    def set_time_mean_fields(self, fnetoc=None):
        for x in self.slabs:
            x.set_time_mean_fields(fnetoc)

    def tavocn(self):
        """One tavocn contribution on every slab (no exchange: the halo rows the fluxes read are current)."""
        self._join()
        for x in self.slabs:
            x.tavocn()

    def time_means(self, names=None):
        """As OceanModel.time_means: the whole basin's means, assembled from the owned rows (collective)."""
        self._join()
        res = [x.time_means(names) for x in self.slabs]
        out = self._assemble([d for d, _ in res])
        out["nsumoc"] = res[0][1]
        return out

    def reset_time_means(self):
        for x in self.slabs:
            x.reset_time_means()

    # covariance matrices, collective: row sums of every rank, one all-gather, the combine on every rank ----
    def enable_covariance(self, nsi=16):
        S = self.slabs
        for x in S:
            x.enable_covariance(nsi)
        n = S[0].cov_part_len()
        self._cov_bufs = ([x.new_buffer(n) for x in S], [x.new_buffer(n * self.P) for x in S])
        self._settle()

    def covocn(self):
        """One covocn contribution: every rank's row sums, one all-gather, every rank forms the same vectors and means
        and updates the matrix rows it holds."""
        S = self.slabs
        send, gath = self._cov_bufs
        self._join()  # (the row sums read owned rows only; the pending halo stage belongs to the step)
        for i, x in enumerate(S):
            x.cov_part(send[i])
        for x in S:
            x.sync()
        self._comm(self.comm.all_gather, gath, send)
        for i, x in enumerate(S):
            x.cov_combine(gath[i])

    def covariance_parts(self, k0=None, count=None):
        """The local slabs' shares (HipSlab.covariance), for matrices too large to assemble."""
        return [x.covariance(k0, count) for x in self.slabs]

    def covariance(self):
        """As OceanModel.covariance(): the whole matrices, assembled from every rank's rows with one all-gather."""
        S = self.slabs
        parts = self.covariance_parts()
        sz = S[0].covariance_size()
        nvar, P = sz["nvar"], self.P
        ks = [cov_row_split(nvar, r, P) * (cov_row_split(nvar, r, P) + 1) // 2 for r in range(P + 1)]
        m = max(ks[r + 1] - ks[r] for r in range(P))
        send, gath = [], []
        for x, d in zip(S, parts):
            v = np.zeros(2 * m)
            v[:len(d["covpo"])] = d["covpo"]
            v[m:m + len(d["covto"])] = d["covto"]
            t = x.new_buffer(2 * m)
            t.copy_(x.torch.from_numpy(v))
            send.append(t)
            gath.append(x.new_buffer(2 * m * P))
        self._settle()
        self._comm(self.comm.all_gather, gath, send)
        g = gath[0].cpu().numpy().reshape(P, 2 * m)
        out = dict(parts[0])
        out["covpo"] = np.concatenate([g[r, :ks[r + 1] - ks[r]] for r in range(P)])
        out["covto"] = np.concatenate([g[r, m:m + ks[r + 1] - ks[r]] for r in range(P)])
        assert len(out["covpo"]) == sz["nmat"]
        return out

    def reset_covariance(self):
        for x in self.slabs:
            x.reset_covariance()

    # periodic ocean dumps, collective: the owned subsample rows of every rank, one all-gather -----------
    def _gather_subsample(self, parts, rows, nsko, tnames=()):
        """parts[i]: dict name -> (planes, rows, columns) owned subsample rows of local slab i; rows[i] its
        (mp0, mp1, mt0, mt1) (HipSlab.subsample_rows), T-grid rows for the names in `tnames`.  One all-gather of the
        packed blocks (row ranges, then every field padded to the largest rank's rows); dict name -> basin array."""
        S, cfg = self.slabs, self.cfg
        names = sorted(parts[0])
        first = lambda g0: (g0 - 1 + nsko - 1) // nsko
        rmax = max([max(first(g0), (g1 - 1) // nsko + 1) - first(g0) for g0, g1 in partition(cfg.nypo, self.P)]
                   + [r[1] - r[0] for r in rows] + [1])
        sizes = [(n, parts[0][n].shape[0], parts[0][n].shape[2]) for n in names]
        ln = 4 + sum(k * rmax * nc for _, k, nc in sizes)
        send, gath = [], []
        for x, d, r in zip(S, parts, rows):
            v = np.zeros(ln)
            v[:4] = r
            o = 4
            for n, k, nc in sizes:
                buf = np.zeros((k, rmax, nc))
                buf[:, :d[n].shape[1], :] = d[n]
                v[o:o + buf.size] = buf.ravel()
                o += buf.size
            t = x.new_buffer(ln)
            t.copy_(x.torch.from_numpy(v))
            send.append(t)
            gath.append(x.new_buffer(ln * self.P))
        self._settle()
        self._comm(self.comm.all_gather, gath, send)
        g = gath[0].cpu().numpy().reshape(self.P, ln)
        out, o = {}, 4
        for n, k, nc in sizes:
            tg = n in tnames
            full = np.zeros((k, subsample_count(cfg.nyto if tg else cfg.nypo, nsko), nc))
            for r in range(self.P):
                m0, m1 = (int(g[r, 2]), int(g[r, 3])) if tg else (int(g[r, 0]), int(g[r, 1]))
                blk = g[r, o:o + k * rmax * nc].reshape(k, rmax, nc)
                full[:, m0:m1, :] = blk[:, :m1 - m0, :]
            out[n] = full
            o += k * rmax * nc
        return out

    def vorticity_budget(self, nsko=1):
        """As OceanModel.vorticity_budget: the whole basin's (nlo, jpwk, ipwk) arrays, assembled from the owned
        subsample rows of every rank (collective)."""
        self._join()
        return self._gather_subsample([x.vorticity_budget(nsko) for x in self.slabs],
                                      [x.subsample_rows(nsko) for x in self.slabs], nsko)

    def ocean_dump(self, nsko=1, outfloc=(1, 1, 1, 1, 1, 1, 0)):
        """As OceanModel.ocean_dump: the whole basin's subsampled fields (collective)."""
        self._join()
        flat = ("sst", "wekto", "tauxo", "tauyo")
        parts = [{n: (v[None] if n in flat else v) for n, v in x.ocean_dump(nsko, outfloc).items()}
                 for x in self.slabs]
        out = self._gather_subsample(parts, [x.subsample_rows(nsko) for x in self.slabs], nsko, ("sst", "wekto"))
        return {n: (v[0] if n in flat else v) for n, v in out.items()}

    def homsol(self):
        """homsol of the box ocean (src/conhoms.F:549-641) ON the slabs: the modal Helmholtz problems of a step are
        homsol's, so one distributed solve with right-hand side 1 gives every ochom(:,:,m); no host-side solver.
        Sets the homogeneous solutions on every local slab and returns the global products aipohs, cdiffo, cdhoc."""
        cfg, S = self.cfg, self.slabs
        nl = cfg.nlo
        rdm2, cm2l = S[0].consts["rdm2oc"], S[0].consts["ctm2loc"]
        for i, x in enumerate(S):
            x.wrk_fill(1.0)
            x.row_transform(0)
            x.thomas_phase(1, None, self.th_send[i])
        self._comm(self.comm.all_gather, self.th_gath, self.th_send)
        sols, xin = [], None
        for i, x in enumerate(S):
            x.thomas_phase(2, self.th_gath[i], None)
            xin = x.area_integrals()          # dxo*dyo*xintp(solution of mode m), basin-wide, the same on every rank
            x.row_transform(1)
            sols.append(x.wrk_get())
        dA = cfg.dxo * cfg.dyo
        aipohs = np.array([dA * cfg.nxto * cfg.nyto + rdm2[m + 1] * xin[m + 1] for m in range(nl - 1)])  # xintp(1) = nxto*nyto
        cdiffo = np.zeros((nl, nl - 1), order="F")
        cdhoc = np.zeros((nl - 1, nl - 1), order="F")
        for k in range(nl - 1):
            for m in range(nl):
                cdiffo[m, k] = cm2l[m, k + 1] - cm2l[m, k]
            for m in range(nl - 1):
                cdhoc[k, m] = (cm2l[m + 1, k + 1] - cm2l[m + 1, k]) * aipohs[m]
        for x, w in zip(S, sols):
            oh = np.zeros((cfg.nxpo, x.nyl, nl - 1), order="F")
            for m in range(nl - 1):
                oh[:, :, m] = 1.0 + rdm2[m + 1] * w[:, :, m + 1]
            # halo rows belong to the neighbours' solves; unpack only reads ochom on owned rows
            x.set_homog(oh, cdiffo, cdhoc)
            x.ochom_local = oh
        return dict(aipohs=aipohs, cdiffo=cdiffo, cdhoc=cdhoc)

    def use_library_exchanges(self, comm_id):
        """From now on steps() runs qgcm_hip_slab_steps: the library issues the RCCL exchanges
        itself, Python is out of the step loop.  One slab per process; collective."""
        assert len(self.slabs) == 1
        self.slabs[0].comm_init(comm_id)
        self.native = True

    def steps(self, n, s0=None):
        s0 = self.step_index if s0 is None else int(s0)
        if getattr(self, "native", False):
            self.slabs[0].slab_steps(s0, n)
        else:
            for s in range(s0, s0 + int(n)):
                self.step(s)
            self._join()
        self.step_index = s0 + int(n)

    # coupled runs: xforc under a replicated atmosphere, collective ---------------------------------------
    def xforc_setup(self, atmospheres, cdat=1.3e-3, rhoat=1.0, rhooc=1.0e3, hmat=1000.0, hmoc=100.0, tau_udiff=False,
                    tables=None, ndxr=None, nxaooc=None, nyaooc=None, nx1=None, ny1=None, bands=False, udiff_gather=False,
                    udiff_sums=False):
        """As model.xforc_setup (ndxr, nxaooc, nyaooc default to the ocean configuration's), for the slabs: `atmospheres` holds one whole-domain AtmosModel per local slab, on that
        slab's device - replicas of one atmosphere, which every rank steps redundantly and which stay bitwise identical.
        tau_udiff = True is refused by the library (the fine stress above the sea needs every slab's pom on every rank);
        udiff_gather = True is that physics on slabs: every xforc() first all-gathers the slabs' owned rows of
        pom(:,:,1) and assembles the basin's layer on every rank, and the stress kernels run on it unchanged - every
        momentum output is bitwise the whole-domain xforc's with tau_udiff = True.  Pass only udiff_gather.
        bands = True: every rank runs the atmosphere side only on the fine rows its band of atmosphere rows
        (lib.xforc_bands, kept as self.xforc_plan) and its slab need; the bands travel in front of the heat block in the
        one all-gather, so xforc() then always gathers and combines.  The results are bitwise the default's.
        udiff_sums = True is the shear term without that gather: every rank forms the fine stress above the
        ocean rows it owns, from its own pressure and the 4 rows beyond each seam (a small all-gather of 8 + 8 * nxpo
        doubles per rank), and the ranks exchange rank-ordered partial sums of uekat and wekpa; xforc() then always runs
        two all-gathers.  A line or box of the sums that no seam cuts keeps the whole-domain bits, a cut one differs by
        rounding.  It excludes bands, udiff_gather and tau_udiff; the plan (lib.xforc_sums) is kept as self.xforc_plan."""
        from .lib import XforcParams, xforc_bands, xforc_sums
        S, oc = self.slabs, self.cfg
        if udiff_sums and (bands or udiff_gather or tau_udiff):
            raise ValueError("xforc_setup: udiff_sums = True excludes bands, udiff_gather and tau_udiff (it implies the shear "
                             "term and splits the atmosphere side by the slabs' own rows)")
        if udiff_gather and tau_udiff:
            raise ValueError("xforc_setup: pass only udiff_gather = True (tau_udiff = True alone asks the library for the "
                             "shear term without the gather, which it refuses)")
        if len(atmospheres) != len(S):
            raise ValueError("xforc_setup: %d atmospheres for %d local slabs" % (len(atmospheres), len(S)))
        acfg = atmospheres[0].cfg
        ndxr = int(oc.ndxr if ndxr is None else ndxr)
        if tables is None:
            tables = hostinit.bcuini(ndxr, acfg.bccoat, acfg.dya)
        keep = [np.asfortranarray(tables[k], dtype=np.float64) for k in ("stbbb", "stbus", "stbvs", "stbun", "stbvn")]
        for t in keep:
            if t.shape != (16, ndxr + 1, ndxr + 1):
                raise ValueError("xforc_setup: a weight table has shape %s, need (16, %d, %d)" % (t.shape, ndxr + 1, ndxr + 1))
        p = XforcParams()
        p.ndxr = ndxr
        p.nxaooc, p.nyaooc = int(oc.nxaooc if nxaooc is None else nxaooc), int(oc.nyaooc if nyaooc is None else nyaooc)
        p.nx1 = 1 + (acfg.nxta - p.nxaooc) // 2 if nx1 is None else int(nx1)
        p.ny1 = 1 + (acfg.nyta - p.nyaooc) // 2 if ny1 is None else int(ny1)
        p.cdat, p.raoro, p.hmat, p.hmoc = float(cdat), float(rhoat) / float(rhooc), float(hmat), float(hmoc)
        p.bccoat, p.bccooc = float(acfg.bccoat), float(oc.bccooc)
        p.tau_udiff = int(bool(tau_udiff))
        p.stbbb, p.stbus, p.stbvs, p.stbun, p.stbvn = [_dp(t) for t in keep]
        for x, a in zip(S, atmospheres):
            x.xforc_init(a, p)
            a.xforc_origin = (int(p.nx1), int(p.ny1))  # (where xforc_heat_setup finds the ocean)
        self.atmos = list(atmospheres)
        self.native_coupling = False  # (use_library_coupling sized its buffers for the set-up this call replaces)
        self._xf_bufs = None
        self._xf_pom_bufs = None
        self._xf_edge_bufs = None
        self.xforc_plan = None
        if bands or udiff_gather or udiff_sums:
            rows = partition(oc.nypo, self.P)
            for x in S:  # (slabs cut otherwise than partition(): their own rows)
                rows[x.rank] = (x.g0, x.g1)
        if udiff_gather:
            nrow = owned_rows_tile(rows, oc.nypo)
            for x, a in zip(S, atmospheres):
                x.xforc_udiff_init(a, nrow, self.P)
            n = [x.xforc_pom_len(a) for x, a in zip(S, atmospheres)]
            self._xf_pom_bufs = ([x.new_buffer(m) for x, m in zip(S, n)], [x.new_buffer(m * self.P) for x, m in zip(S, n)])
            self._settle()
        if udiff_sums:
            owned_rows_tile(rows, oc.nypo)
            self.xforc_plan = xforc_sums(acfg.nxpa, acfg.nyta, ndxr, p.ny1, p.nyaooc, rows)
            for x, a in zip(S, atmospheres):
                x.xforc_sums_init(a, rows)
            n = [x.xforc_edge_len(a) for x, a in zip(S, atmospheres)]
            self._xf_edge_bufs = ([x.new_buffer(m) for x, m in zip(S, n)], [x.new_buffer(m * self.P) for x, m in zip(S, n)])
            self._xf_size_bufs()
        if bands:
            self.xforc_plan = xforc_bands(acfg.nxpa, acfg.nyta, ndxr, p.ny1, p.nyaooc, rows)
            for x, a in zip(S, atmospheres):
                b = self.xforc_plan[x.rank]
                x.xforc_bands_init(a, b["band"], b["nrow"])
            self._xf_size_bufs()

    def _xf_size_bufs(self):
        n = [x.xforc_msg_len(a) for x, a in zip(self.slabs, self.atmos)]
        self._xf_bufs = ([x.new_buffer(m) for x, m in zip(self.slabs, n)], [x.new_buffer(m * self.P) for x, m in zip(self.slabs, n)])
        self._settle()

    def xforc_heat_setup(self, heat, hmadmp=None, hmat=None, fsa=None, fso=None, coords=None):
        """As model.xforc_heat_setup, after xforc_setup, oml_init on every slab and aml_init on every replica; the tables
        and coordinates are the whole basin's."""
        from .lib import XforcHeatParams
        from .model import _heat_params
        for x, a in zip(self.slabs, self.atmos):
            p = XforcHeatParams()
            keep = _heat_params("SlabOcean.xforc_heat_setup", p, a, self.cfg, heat, hmadmp, hmat, coords, fsa=fsa, fso=fso)
            x.xforc_heat_init(a, p, keep)
            del keep  # (copied by now)
        self._xf_size_bufs()

    def xforc(self):
        """One `call xforc`: every local rank runs the momentum half on its replica and its slab's rows; with the heat
        half, one all-gather of the partial cell sums (4*nxaooc*nyaooc doubles per rank) and the rank-ordered combine.
        Banded (xforc_setup(bands=True)): always one all-gather - the ranks' bands, then the heat block - and the combine.
        With the shear term (xforc_setup(udiff_gather=True)) one more all-gather in front: pack, the gather of the pressure
        rows (8 + nrow * nxpo doubles per rank), assemble on every local rank; then the sequence above, unchanged.
        With the owner-computed sums (xforc_setup(udiff_sums=True)) always two all-gathers: edge pack, the gather of the
        edge rows (8 + 8 * nxpo doubles per rank), edge assemble, part, the gather of the messages, combine."""
        S, A = self.slabs, self.atmos
        self._join()
        if getattr(self, "_xf_edge_bufs", None):  # the 4 rows beyond each seam onto the neighbours first
            esend, egath = self._xf_edge_bufs
            for i, (x, a) in enumerate(zip(S, A)):
                x.xforc_edge_pack(a, esend[i])
            for a in A:
                a.sync()
            self._comm(self.comm.all_gather, egath, esend)
            for x in S:
                x.sync()
            for i, (x, a) in enumerate(zip(S, A)):
                x.xforc_edge_assemble(a, egath[i])
        if getattr(self, "_xf_pom_bufs", None):  # the shear term: the basin's pom(:,:,1) onto every rank first
            psend, pgath = self._xf_pom_bufs
            for i, (x, a) in enumerate(zip(S, A)):
                x.xforc_pom_pack(a, psend[i])
            for a in A:
                a.sync()
            self._comm(self.comm.all_gather, pgath, psend)
            for x in S:
                x.sync()
            for i, (x, a) in enumerate(zip(S, A)):
                x.xforc_pom_assemble(a, pgath[i])
        send, gath = self._xf_bufs if self._xf_bufs else ([None] * len(S), None)
        for i, (x, a) in enumerate(zip(S, A)):
            x.xforc_part(a, send[i])
        if gath is None:
            return
        for a in A:  # the messages are complete before a transport reads them (they are written on the replicas' streams)
            a.sync()
        self._comm(self.comm.all_gather, gath, send)
        for x in S:  # ... and gathered before the replicas' streams read them (a transport may run on the slab's stream)
            x.sync()
        for i, (x, a) in enumerate(zip(S, A)):
            x.xforc_combine(a, gath[i])

    def xforc_get(self):
        """The momentum half's outputs of the last xforc(), one dict per local slab: model.xforc_get's names, the
        ocean's fields with the slab's local rows (owned + halo; global row = local + slab.joff)."""
        return [x.xforc_fetch(a, False) for x, a in zip(self.slabs, self.atmos)]

    def xforc_heat_get(self):
        """The heat half's outputs of the last xforc(), one dict per local slab: model.xforc_heat_get's names, fnetoc
        with the slab's local T rows."""
        return [x.xforc_fetch(a, True) for x, a in zip(self.slabs, self.atmos)]

    def use_library_coupling(self):
        """From now on coupled_steps() runs qgcm_hip_slab_coupled_steps: the library issues the whole window -
        xforc with its all-gathers over RCCL, the mixed layers, the slab step, the replica's steps - with events between
        the slab's stream and the replica's and no host wait; Python is out of the window.  Opt-in, one slab per process,
        after use_library_exchanges() and the xforc set-ups (call it again after a set-up call changed the mode).  xforc()
        on its own and the virtual ranks keep the Python-driven path."""
        if len(self.slabs) != 1:
            raise ValueError("use_library_coupling: one slab per process (virtual ranks keep the Python-driven window)")
        if not getattr(self, "native", False):
            raise ValueError("use_library_coupling: call use_library_exchanges first (it creates the communicator)")
        if not hasattr(self, "atmos"):
            raise ValueError("use_library_coupling: call xforc_setup first (it names the replica of the atmosphere)")
        self._join()
        self.slabs[0].coupled_init(self.atmos[0])
        self.native_coupling = True

    def coupled_steps(self, nt0, n, nstr, xforc=False):
        """As model.coupled_steps (src/q-gcm.F:1220-1268): n atmospheric steps nt = nt0.. on every replica with one slab
        ocean step before every one with mod(nt,nstr) == 1; xforc = True: xforc() before each ocean step, False: the
        forcing is held.  With the mixed layers on the window is xforc; oml; qgostep ...; (aml; qgastep ...) x nstr."""
        nt0, n, nstr = int(nt0), int(n), int(nstr)
        if nt0 < 1 or n < 0 or nstr < 1:
            raise ValueError("coupled_steps: bad step range")
        if not hasattr(self, "atmos"):
            raise ValueError("coupled_steps: call xforc_setup first (it names the replicas of the atmosphere)")
        if getattr(self, "native_coupling", False):  # use_library_coupling: the library runs the whole window
            self.slabs[0].coupled_steps(self.atmos[0], nt0, n, nstr, xforc)
            self.atmos[0].step_index = nt0 + n
            if nstr > 1 and n > 0:  # ocean steps s with nt = 1 + (s - 1) * nstr inside the window
                sfirst, slast = (nt0 + nstr - 2) // nstr + 1, (nt0 + n - 2) // nstr + 1
                if slast >= sfirst:
                    self.step_index = slast + 1
            return
        nt, end = nt0, nt0 + n
        while nt < end:
            nxt = end
            if nstr > 1:  # (nstr = 1 never steps the ocean in the reference)
                if nt % nstr == 1:
                    if xforc:
                        self.xforc()
                    self.steps(1, s0=(nt - 1) // nstr + 1)
                nn = nt + (nstr - (nt - 1) % nstr)  # the next nt with mod(nt,nstr) == 1
                nxt = min(nn, end)
            for a in self.atmos:
                a.steps(nxt - nt, s0=nt)
            nt = nxt

    # helpers to scatter / gather global arrays (host side, for tests and set-up) --
    def scatter_state(self, po, pom, qo, qom, wekpo, entoc, xon, scal):
        nyg = self.cfg.nypo
        for x in self.slabs:
            sl = slab_slice(nyg, x.g0, x.g1)
            x.set_state(po[:, sl, :], pom[:, sl, :], qo[:, sl, :], qom[:, sl, :])
            x.set_forcing(wekpo[:, sl], entoc[:, sl], xon)
            x.set_scalars(scal)

    def gather_local(self):
        """Owned rows of the local slabs: list of (g0, g1, [po, pom, qo, qom])."""
        out = []
        for x in self.slabs:
            st = x.get_state()
            out.append((x.g0, x.g1, [a[:, x.jlo - 1:x.jhi, :] for a in st]))
        return out


def global_consts(cfg, helmholtz=None):
    """Start-up constants on the GLOBAL grid (numpy, init-only), as in OceanModel.  helmholtz = None: without the
    homogeneous solutions - SlabOcean.homsol() then computes them on the slabs (no host-side solver)."""
    A, rdm2, cl2m, cm2l = hostinit.eigmod(cfg.gpoc, cfg.hoc, cfg.fnot)
    aoc, bd2 = hostinit.bd2oc(cfg)
    c = dict(amatoc=A, rdm2oc=rdm2, ctl2moc=cl2m, ctm2loc=cm2l, aoc=aoc, bd2oc=bd2, yporel=cfg.yporel(),
             ddynoc=np.zeros((cfg.nxpo, cfg.nypo), order="F"))
    if cfg.cyclic:
        # channel: the homogeneous solutions depend on y only - a tridiagonal solve per mode, no 2-D solver needed
        solve = helmholtz if helmholtz is not None else (lambda rhs, boc: hostinit.helmholtz_cyc_column(cfg, rhs, boc))
        c.update(hostinit.homsol_cyc(cfg, rdm2, bd2, c["yporel"], solve))
    elif helmholtz is not None:
        c.update(hostinit.homsol_box(cfg, rdm2, cm2l, bd2, helmholtz))
    return c
