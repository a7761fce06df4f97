"""qgcm_hip.handle.Handle on the GPU: the accessors OceanModel (the whole domain) and HipSlab (three y-slabs on one
card) share are pure copies to and from the device, so every round trip is bitwise - no kernel's result is compared
and no tolerance is needed.  What the library is handed is pinned without a GPU in test_handle_cpu.py; here the real
library receives it: the local blocks of set_state, the scalars, and the stored T rows cut out of GLOBAL mixed-layer
arrays.  Every handle closes twice and gives back what it took."""
import numpy as np
import pytest

from common import preset, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["box_tiny", "cyc_tiny"])
def test_round_trips_are_bitwise_on_slabs_and_whole_domain(name):
    from qgcm_hip import OceanModel, oml_preset
    from qgcm_hip.lib import live_allocs
    from qgcm_hip.slab import HipSlab, global_consts, local_rows, partition
    base = live_allocs()
    cfg = preset(name)
    consts = global_consts(cfg, lambda rhs, boc: np.zeros_like(rhs))  # any homogeneous solutions will do here
    parts = partition(cfg.nypo, 3)
    handles = [HipSlab(cfg, consts, g0, g1, r, 3) for r, (g0, g1) in enumerate(parts)] + [OceanModel(cfg)]
    # the T rows each handle stores: a slab's local T array holds rows joff .. joff + nyl - 2 of the global one
    t_rows = []
    for g0, g1 in parts:
        nyl, joff, _, _ = local_rows(cfg.nypo, g0, g1)
        t_rows.append(slice(joff, joff + nyl - 1))
    t_rows.append(slice(0, cfg.nyto))
    rng = np.random.default_rng(20)
    sst, sstm = (np.asfortranarray(rng.standard_normal((cfg.nxto, cfg.nyto))) for _ in range(2))
    try:
        assert live_allocs()[0] > base[0]
        for x, rows in zip(handles, t_rows):
            assert x.nyl == rows.stop - rows.start + 1
            state = [np.asfortranarray(rng.standard_normal((cfg.nxpo, x.nyl, cfg.nlo))) for _ in range(4)]
            x.set_state(*state)
            for a, b, f in zip(x.get_state(), state, ("po", "pom", "qo", "qom")):
                same_bits(a, b, "%s of rank %d of %d" % (f, x.rank, x.nranks))
            s = rng.standard_normal(2 * (cfg.nlo - 1) + 4 * cfg.nlo)
            x.set_scalars(s)
            if not cfg.cyclic:  # (qgcm_hip_get_scalars returns the channel's constraint constants of a box as zeros)
                s[2 * (cfg.nlo - 1):] = 0.0
            same_bits(x.get_scalars(), s, "scalars of rank %d of %d" % (x.rank, x.nranks))
            x.oml_init(oml_preset(cfg))
            x.oml_set_state(sst, sstm)
            for a, b, f in zip(x.oml_get_state(), (sst, sstm), ("sst", "sstm")):
                assert a.shape == (cfg.nxto, x.nyl - 1)
                same_bits(a, b[:, rows], "%s of rank %d of %d" % (f, x.rank, x.nranks))
            x.oml_set_state(None, sst)  # None leaves sst as it is
            for a in x.oml_get_state():
                same_bits(a, sst[:, rows], "sst, sstm of rank %d of %d after (None, sst)" % (x.rank, x.nranks))
    finally:
        for x in handles:
            x.close()
            x.close()
            assert not x.h
    assert live_allocs() == base
