"""Timings of xforc and of the coupled window on a y-slab ocean under a replicated atmosphere at cpl_natl5
(atmosphere 385 x 97, ocean 961 x 961, ndxr 16) on cuda:0, printed as a log (profiles/slab_coupled.log).  Virtual ranks
on one GPU: every rank's replica and slab share the device, so the figures say what the calls cost, not how they
scale.  Host clock around work that ends in a synchronise; medians.
  python3 profiles/tools/slab_coupled.py   the whole-domain xforc() and coupled window (tau_udiff off, both mixed layers
                                           and the heat half on), then - where the library has the slab entry points -
                                           1, 2 and 4 virtual ranks: every rank's xforc_slab_part, every rank's combine,
                                           and the window per ocean step
  python3 profiles/tools/slab_coupled.py bands   the banded atmosphere side (profiles/slab_bands.log): on 1, 2
                                           and 4 virtual ranks two set-ups side by side, replicated and banded, timed in
                                           alternating blocks in one session: xforc_slab_part and the combine per rank
  python3 profiles/tools/slab_coupled.py udiff   the shear term on slabs (profiles/slab_udiff.log): on 1, 2 and
                                           4 virtual ranks two set-ups side by side, shear-free and udiff_gather, timed
                                           in alternating blocks in one session: pom_pack, pom_assemble, xforc_slab_part
                                           and the combine per rank
  python3 profiles/tools/slab_coupled.py sums    the shear term by owner-computed sums (DESIGN 6r;
                                           profiles/slab_udiff_sums.log): on 1, 2 and 4 virtual ranks three set-ups side by
                                           side - udiff_gather replicated, udiff_gather banded, udiff_sums - timed in
                                           alternating blocks in one session: the pack and the assemble ahead of the part,
                                           xforc_slab_part and the combine per rank, SlabOcean.xforc() for all ranks
With QGCM_HIP_LIB pointing at a build of the parent commit the same script gives the parent's whole-domain figures."""
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

NWIN = 60  # atmospheric steps per timed window


def inputs():
    from common import cpl_fullsize_inputs, load_golden
    from qgcm_hip import config
    g = load_golden("cpl_natl5_sample")
    oc, at = config.preset("cpl_natl5"), config.atmos_preset("cpl_natl5")
    po, pom, wekpo, f = cpl_fullsize_inputs(g, oc, at)
    yo = (np.arange(oc.nyto) + 0.5) / oc.nyto
    sst = np.asfortranarray(np.broadcast_to(4.0 * np.cos(np.pi * yo)[None, :], (oc.nxto, oc.nyto)))
    return dict(oc=oc, at=at, po=po, pom=pom, wekpo=wekpo, f=f, sst=sst, nstr=int(g["nstr"]))


AM = dict(tat=(30.0, 40.0), aface=(1.1e-6, -0.4e-6), bface=0.7e-6, cface=-0.3e-6, dface=2.3e-4)
HT = dict(D0up=6.5, Dmup=5.1, Dmdown=-5.6, Adown11=-4.7e-3, Bmup=8.9e-3, B1down=-3.1e-3, Cmup=-2.2e-3, C1down=1.3e-3)


def atmosphere(I):
    from common import atm_apply
    from qgcm_hip import AtmosModel, config
    at = I["at"]
    a = AtmosModel(at, ddynat=I["f"]["ddynat"])
    atm_apply(a, I["f"])
    a.aml_init(config.AmlConfig(**AM))
    x, y = (np.arange(at.nxta) + 0.5) / at.nxta, (np.arange(at.nyta) + 0.5) / at.nyta
    ast = np.asfortranarray(-5.0 + 6.0 * np.cos(np.pi * y)[None, :] + 1.5 * np.cos(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    hm = np.asfortranarray(1000.0 + 40.0 * np.sin(2 * np.pi * x)[:, None] * np.sin(np.pi * y)[None, :])
    a.aml_set_state(ast, ast, hm, hm)
    return a


def ocean(I):
    from qgcm_hip import OceanModel, oml_preset
    oc = I["oc"]
    o = OceanModel(oc)
    o.set_p(I["po"], I["pom"])
    o.set_forcing(I["wekpo"], np.zeros_like(I["wekpo"]), np.zeros(oc.nlo - 1))
    o.oml_init(oml_preset(oc))
    o.oml_set_state(sst=I["sst"], sstm=I["sst"])
    return o


def med(v):
    return float(np.median(v))


def whole(I):
    from qgcm_hip import config, coupled_steps, xforc, xforc_heat_setup, xforc_setup
    o, a = ocean(I), atmosphere(I)
    xforc_setup(o, a, tau_udiff=False)
    xforc_heat_setup(o, a, config.HeatConfig(**HT))
    t = []
    for k in range(35):
        t0 = time.perf_counter()
        xforc(o, a)
        a.sync()
        t.append(1e6 * (time.perf_counter() - t0))
    print("whole domain: one synchronised xforc() (both halves, tau_udiff off), us, median of 30: %.1f" % med(t[5:]), flush=True)
    nstr, nt0, w = I["nstr"], 1, []
    for k in range(5):
        t0 = time.perf_counter()
        coupled_steps(o, a, nt0, NWIN, nstr, xforc=True)
        o.sync()
        a.sync()
        w.append(1e6 * (time.perf_counter() - t0) / (NWIN // nstr))
        nt0 += NWIN
    print("whole domain: coupled window of %d atmospheric steps (nstr %d, no CU ranges), us per ocean step: median of 4 "
          "after one warm-up %.1f (%s)" % (NWIN, nstr, med(w[1:]), " ".join("%.1f" % v for v in w)), flush=True)
    consts = None
    if hasattr(o.L, "qgcm_hip_xforc_slab_init"):
        from qgcm_hip.slab import global_consts
        consts = (global_consts(I["oc"], o.helmholtz),)
    o.close()
    a.close()
    return consts


def time_xforc(so, slabs, reps, n):
    """n synchronised xforc calls in their parts: us of (every rank's part, every rank's combine, SlabOcean.xforc())."""
    send, gath = so._xf_bufs
    tp, tc, tx = [], [], []
    for k in range(n):
        t0 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_part(a, send[i])
        for a in reps:
            a.sync()
        t1 = time.perf_counter()
        so.comm.all_gather(gath, send)
        t2 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_combine(a, gath[i])
        for a in reps:
            a.sync()
        t3 = time.perf_counter()
        tp.append(1e6 * (t1 - t0))
        tc.append(1e6 * (t3 - t2))
        t0 = time.perf_counter()
        so.xforc()
        for a in reps:
            a.sync()
        tx.append(1e6 * (time.perf_counter() - t0))
    return tp, tc, tx


def slab_setup(I, consts, nranks, bands=False, udiff=False, sums=False):
    from qgcm_hip import config, oml_preset
    from qgcm_hip.slab import HipSlab, LocalComm, SlabOcean, partition
    oc = I["oc"]
    o = ocean(I)
    st, scal = o.get_state(), o.get_scalars()
    o.close()
    slabs = [HipSlab(oc, consts, g0, g1, r, nranks, sync_each_call=True) for r, (g0, g1) in enumerate(partition(oc.nypo, nranks))]
    for x in slabs:
        x.oml_init(oml_preset(oc))
    so = SlabOcean(oc, slabs, LocalComm(nranks, after=torch.cuda.synchronize))
    so.scatter_state(st[0], st[1], st[2], st[3], I["wekpo"], np.zeros_like(I["wekpo"]), np.zeros(oc.nlo - 1), scal)
    for x in slabs:
        x.oml_set_state(sst=I["sst"], sstm=I["sst"])
    reps = [atmosphere(I) for _ in slabs]
    kw = dict(dict(bands=True) if bands else {}, **(dict(udiff_gather=True) if udiff else {}))
    so.xforc_setup(reps, tau_udiff=False, **dict(kw, **(dict(udiff_sums=True) if sums else {})))
    so.xforc_heat_setup(config.HeatConfig(**HT))
    return so, slabs, reps


def slabbed(I, consts, nranks):
    so, slabs, reps = slab_setup(I, consts, nranks)
    send, gath = so._xf_bufs
    tp, tc, tx = time_xforc(so, slabs, reps, 35)
    print("%d virtual rank(s): synchronised, us, median of 30: xforc_slab_part on every rank %.1f (%.1f per rank), combine "
          "on every rank %.1f (%.1f per rank), SlabOcean.xforc() with its host-staged all-gather %.1f; message %d doubles per rank"
          % (nranks, med(tp[5:]), med(tp[5:]) / nranks, med(tc[5:]), med(tc[5:]) / nranks, med(tx[5:]), send[0].numel()), flush=True)
    nstr, nt0, w = I["nstr"], 1, []
    for k in range(5):
        t0 = time.perf_counter()
        so.coupled_steps(nt0, NWIN, nstr, xforc=True)
        for m in slabs + reps:
            m.sync()
        w.append(1e6 * (time.perf_counter() - t0) / (NWIN // nstr))
        nt0 += NWIN
    ok = all(np.isfinite(x.get_state()[0]).all() for x in slabs) and all(np.isfinite(a.get_state()[0]).all() for a in reps)
    print("%d virtual rank(s): coupled window of %d atmospheric steps (stage calls from Python, a synchronise after each, "
          "every replica stepped), us per ocean step: median of 4 after one warm-up %.1f (%s); state finite: %s"
          % (nranks, NWIN, med(w[1:]), " ".join("%.1f" % v for v in w), ok), flush=True)
    for m in slabs + reps:
        m.close()


def banded(I, consts, nranks, rounds=4):
    """Replicated and banded set-ups of `nranks` virtual ranks side by side, timed in alternating blocks of 25 calls (the
    first 5 of a block dropped): per mode the median of each block, then the median and the spread (max - min) of the
    block medians.  The two agree bitwise (tests/test_gpu_xforc_bands.py); checked here on wekpa and fnetat."""
    sets = [slab_setup(I, consts, nranks, bands=b) for b in (False, True)]
    blocks = {False: [], True: []}
    for rnd in range(rounds):
        for b, (so, slabs, reps) in zip((False, True), sets):
            tp, tc, tx = time_xforc(so, slabs, reps, 25)
            blocks[b].append((med(tp[5:]) / nranks, med(tc[5:]) / nranks, med(tx[5:])))
    out = [[dict(m, **h) for m, h in zip(so.xforc_get(), so.xforc_heat_get())] for so, _, _ in sets]
    same = all(np.array_equal(x[f].view(np.int64), y[f].view(np.int64)) for x, y in zip(*out) for f in ("wekpa", "fnetat", "tauxo", "vekat"))
    plan = sets[1][0].xforc_plan
    nfine = I["at"].nyta * I["oc"].ndxr + 1
    print("%d virtual rank(s): message %d (replicated) / %d (banded) doubles per rank; fine rows computed per rank, of %d: %s; "
          "outputs bit-equal: %s" % (nranks, sets[0][0]._xf_bufs[0][0].numel(), sets[1][0]._xf_bufs[0][0].numel(), nfine,
                                     " ".join(str(sum(f1 - f0 + 1 for f0, f1 in p["fine"])) for p in plan), same), flush=True)
    for b, name in ((False, "replicated"), (True, "banded    ")):
        for k, what in enumerate(("xforc_slab_part per rank", "combine per rank", "SlabOcean.xforc() with its host-staged all-gather")):
            v = [blk[k] for blk in blocks[b]]
            print("%d virtual rank(s), %s: %s, us: median of the block medians %.1f, spread %.1f (%s)"
                  % (nranks, name, what, med(v), max(v) - min(v), " ".join("%.1f" % t for t in v)), flush=True)
    for so, slabs, reps in sets:
        for m in slabs + reps:
            m.close()


def time_pom(so, slabs, reps, n):
    """n synchronised gathers of the surface pressure in their parts: us of (every rank's pack, every rank's assemble).
    Every assemble is followed by nothing: the next part of time_xforc's loop finds the flag set."""
    send, gath = so._xf_pom_bufs
    tk, ta = [], []
    for k in range(n):
        t0 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_pom_pack(a, send[i])
        for a in reps:
            a.sync()
        t1 = time.perf_counter()
        so.comm.all_gather(gath, send)
        t2 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_pom_assemble(a, gath[i])
        for a in reps:
            a.sync()
        t3 = time.perf_counter()
        tk.append(1e6 * (t1 - t0))
        ta.append(1e6 * (t3 - t2))
    return tk, ta


def time_xforc_udiff(so, slabs, reps, n):
    """time_xforc for a set-up with the shear term: an (untimed) gather of the pressure ahead of every timed part."""
    send, gath = so._xf_bufs
    psend, pgath = so._xf_pom_bufs
    tp, tc, tx = [], [], []
    for k in range(n):
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_pom_pack(a, psend[i])
        for a in reps:
            a.sync()
        so.comm.all_gather(pgath, psend)
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_pom_assemble(a, pgath[i])
        for a in reps:
            a.sync()
        t0 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_part(a, send[i])
        for a in reps:
            a.sync()
        t1 = time.perf_counter()
        so.comm.all_gather(gath, send)
        t2 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_combine(a, gath[i])
        for a in reps:
            a.sync()
        t3 = time.perf_counter()
        tp.append(1e6 * (t1 - t0))
        tc.append(1e6 * (t3 - t2))
        t0 = time.perf_counter()
        so.xforc()
        for a in reps:
            a.sync()
        tx.append(1e6 * (time.perf_counter() - t0))
    return tp, tc, tx


def sheared(I, consts, nranks, rounds=4):
    """Shear-free and udiff_gather set-ups of `nranks` virtual ranks side by side (replicated atmosphere side, the heat
    half on), timed in alternating blocks of 25 calls (the first 5 of a block dropped): per mode the median of each
    block, then the median and the spread (max - min) of the block medians.  With the shear term the outputs are the
    whole-domain call's with tau_udiff (tests/test_gpu_slab_udiff.py); checked here: finite, and tauxo moved."""
    sets = [slab_setup(I, consts, nranks, udiff=u) for u in (False, True)]
    blocks = {False: [], True: []}
    pom = []
    for rnd in range(rounds):
        for u, (so, slabs, reps) in zip((False, True), sets):
            if u:
                tk, ta = time_pom(so, slabs, reps, 25)
                pom.append((med(tk[5:]) / nranks, med(ta[5:]) / nranks))
                tp, tc, tx = time_xforc_udiff(so, slabs, reps, 25)
            else:
                tp, tc, tx = time_xforc(so, slabs, reps, 25)
            blocks[u].append((med(tp[5:]) / nranks, med(tc[5:]) / nranks, med(tx[5:])))
    out = [so.xforc_get() for so, _, _ in sets]
    finite = all(np.isfinite(m[f]).all() for m in out[1] for f in ("wekpa", "tauxo", "wekto"))
    moved = float(np.mean([np.mean(x["tauxo"] != y["tauxo"]) for x, y in zip(*out)]))
    print("%d virtual rank(s): pressure message %d doubles per rank (%d gathered per rank); heat message %d; outputs finite: %s; "
          "tauxo differs from the shear-free run at %.3f of the slabs' points" % (
              nranks, sets[1][0]._xf_pom_bufs[0][0].numel(), sets[1][0]._xf_pom_bufs[1][0].numel(),
              sets[1][0]._xf_bufs[0][0].numel(), finite, moved), flush=True)
    for k, what in enumerate(("pom_pack per rank", "pom_assemble per rank")):
        v = [blk[k] for blk in pom]
        print("%d virtual rank(s), shear term on : %s, us: median of the block medians %.1f, spread %.1f (%s)"
              % (nranks, what, med(v), max(v) - min(v), " ".join("%.1f" % t for t in v)), flush=True)
    for u, name in ((False, "shear term off"), (True, "shear term on ")):
        for k, what in enumerate(("xforc_slab_part per rank", "combine per rank", "SlabOcean.xforc() with its host-staged all-gather(s)")):
            v = [blk[k] for blk in blocks[u]]
            print("%d virtual rank(s), %s: %s, us: median of the block medians %.1f, spread %.1f (%s)"
                  % (nranks, name, what, med(v), max(v) - min(v), " ".join("%.1f" % t for t in v)), flush=True)
    for so, slabs, reps in sets:
        for m in slabs + reps:
            m.close()


def time_shear(so, slabs, reps, n):
    """n synchronised xforc calls of a set-up with the shear term, in their parts: us of (every rank's pack ahead of the
    part, every rank's assemble, every rank's part, every rank's combine, SlabOcean.xforc()).  The pack and the assemble are
    the gather's (pom rows) or the sums' (edge rows), whichever the set-up has."""
    send, gath = so._xf_bufs
    edge = getattr(so, "_xf_edge_bufs", None)
    psend, pgath = edge if edge else so._xf_pom_bufs
    T = [[] for _ in range(5)]
    for k in range(n):
        t0 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            (x.xforc_edge_pack if edge else x.xforc_pom_pack)(a, psend[i])
        for a in reps:
            a.sync()
        t1 = time.perf_counter()
        so.comm.all_gather(pgath, psend)
        t2 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            (x.xforc_edge_assemble if edge else x.xforc_pom_assemble)(a, pgath[i])
        for a in reps:
            a.sync()
        t3 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_part(a, send[i])
        for a in reps:
            a.sync()
        t4 = time.perf_counter()
        so.comm.all_gather(gath, send)
        t5 = time.perf_counter()
        for i, (x, a) in enumerate(zip(slabs, reps)):
            x.xforc_combine(a, gath[i])
        for a in reps:
            a.sync()
        t6 = time.perf_counter()
        so.xforc()
        for a in reps:
            a.sync()
        t7 = time.perf_counter()
        for v, d in zip(T, (t1 - t0, t3 - t2, t4 - t3, t6 - t5, t7 - t6)):
            v.append(1e6 * d)
    return T


def summed(I, consts, nranks, rounds=4):
    """udiff_gather replicated, udiff_gather banded and udiff_sums set-ups of `nranks` virtual ranks side by side (the heat
    half on), timed in alternating blocks of 25 calls (the first 5 of a block dropped): per mode the median of each block,
    then the median and the spread (max - min) of the block medians.  The gather's two forms are the whole-domain call's
    bits; the sums differ from them at the cut entries of uekat, wekpa, wekta only (tests/test_gpu_xforc_sums.py); checked
    here: tauxo and vekat bit-equal across the three, the largest relative difference of wekpa."""
    modes = (("gather, replicated", dict(udiff=True)), ("gather, banded    ", dict(udiff=True, bands=True)), ("sums              ", dict(sums=True)))
    sets = [slab_setup(I, consts, nranks, **kw) for _, kw in modes]
    blocks = [[] for _ in modes]
    for rnd in range(rounds):
        for k, (so, slabs, reps) in enumerate(sets):
            T = time_shear(so, slabs, reps, 25)
            blocks[k].append([med(v[5:]) / (1 if j == 4 else nranks) for j, v in enumerate(T)])
    out = [so.xforc_get() for so, _, _ in sets]
    same = all(np.array_equal(x[f].view(np.int64), y[f].view(np.int64)) for o in out[1:] for x, y in zip(out[0], o) for f in ("tauxo", "vekat", "tauxa"))
    rel = max(float(np.abs(x["wekpa"] - y["wekpa"]).max() / np.abs(x["wekpa"]).max()) for x, y in zip(out[0], out[2]))
    so = sets[2][0]
    nfine = I["at"].nyta * I["oc"].ndxr + 1
    print("%d virtual rank(s): pressure message %d (gather) / %d (sums: edges) doubles per rank; main message %d (gather, replicated) / "
          "%d (gather, banded) / %d (sums) doubles per rank; fine rows computed per rank in the sums' windows, of %d: %s; coarse "
          "rows per rank: %s; tauxa, vekat, tauxo bit-equal across the three: %s; wekpa, sums against gather: largest |diff| / max %.2e"
          % (nranks, sets[0][0]._xf_pom_bufs[0][0].numel(), so._xf_edge_bufs[0][0].numel(), sets[0][0]._xf_bufs[0][0].numel(),
             sets[1][0]._xf_bufs[0][0].numel(), so._xf_bufs[0][0].numel(), nfine,
             " ".join(str((p["cells"][1] - p["cells"][0] + 1) * I["oc"].ndxr) for p in so.xforc_plan),
             " ".join("%d-%d" % p["arows"] for p in so.xforc_plan), same, rel), flush=True)
    names = ("pack per rank", "assemble per rank", "xforc_slab_part per rank", "combine per rank",
             "SlabOcean.xforc() for all ranks with its host-staged all-gathers")
    for k, (name, _) in enumerate(modes):
        for j, what in enumerate(names):
            v = [blk[j] for blk in blocks[k]]
            print("%d virtual rank(s), %s: %s, us: median of the block medians %.1f, spread %.1f (%s)"
                  % (nranks, name, what, med(v), max(v) - min(v), " ".join("%.1f" % t for t in v)), flush=True)
    for so, slabs, reps in sets:
        for m in slabs + reps:
            m.close()


if __name__ == "__main__":
    print("device: %s; library: %s" % (torch.cuda.get_device_name(0), "the build QGCM_HIP_LIB names" if os.environ.get("QGCM_HIP_LIB") else "in-tree"), flush=True)
    I = inputs()
    if sys.argv[1:] in (["bands"], ["udiff"], ["sums"]):
        from qgcm_hip.slab import global_consts
        o = ocean(I)
        consts = global_consts(I["oc"], o.helmholtz)
        o.close()
        for n in (1, 2, 4):
            dict(bands=banded, udiff=sheared, sums=summed)[sys.argv[1]](I, consts, n)
        sys.exit(0)
    c = whole(I)
    if c is not None:
        for n in (1, 2, 4):
            slabbed(I, c[0], n)
