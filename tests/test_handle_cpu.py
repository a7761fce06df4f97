"""qgcm_hip.handle.Handle without a GPU and without the library: OceanModel (the whole domain) and HipSlab (a y-slab)
are driven against a stand-in for the loaded library that records what it is handed.  What the two classes share is
written once in Handle; these tests pin what differs between a whole-domain handle and a slab - the rows cut out of
GLOBAL arrays, the slab fields of qgcm_hip_params, the sync after launches, the owned-row counts of the readers - and
that None reaches the library as NULL on both."""
import ctypes as C

import numpy as np
import pytest

import qgcm_hip
from qgcm_hip import AtmosModel, OceanModel, atmos_preset, hostinit, preset
from qgcm_hip.lib import Params
from qgcm_hip.slab import HipSlab, local_rows, partition, slab_slice

PRESETS = ["box_tiny", "cyc_tiny"]
KINDS = ["south", "middle", "north", "whole"]


class FakeLib:
    """Every qgcm_hip_* attribute records (name, args) and returns 0; the *_len calls and qgcm_hip_stream return a
    small integer.  grab: entry point -> shapes of its arguments after the handle (None: not a double array); the
    arrays behind those pointers are copied into `got` during the call, while their owner is alive."""

    def __init__(self):
        self.calls, self.grab, self.got = [], {}, {}

    def __getattr__(self, name):
        if not name.startswith("qgcm_hip_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name == "qgcm_hip_create":
                args[0]._obj.value = 1  # a non-null handle, so that close() has something to destroy
            if name in self.grab:
                self.got[name] = [None if p is None or shp is None else
                                  np.ctypeslib.as_array(p, shape=(int(np.prod(shp)),)).copy().reshape(shp, order="F")
                                  for p, shp in zip(args[1:], self.grab[name])]
            return 7 if name.endswith("_len") or name == "qgcm_hip_stream" else 0
        return entry

    def args(self, name):
        """The arguments of the last call of `name`."""
        return [a for n, a in self.calls if n == name][-1]

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


@pytest.fixture
def fake(monkeypatch):
    L = FakeLib()
    for mod in (qgcm_hip, qgcm_hip.lib, qgcm_hip.handle, qgcm_hip.slab):
        monkeypatch.setattr(mod, "load_library", lambda: L)
    return L


def coded(shape, k=0):
    """Fortran-ordered float64 array whose entries encode their own (i, j[, l]) and the argument number k."""
    idx = np.indices(shape)
    a = 1.0e6 * k + idx[0] + 1.0e3 * idx[1] + (0.25 * idx[2] if len(shape) == 3 else 0.0)
    return np.asfortranarray(a, dtype=np.float64)


def consts_of(cfg, atmos=False):
    """Start-up constants on the global grid; the homogeneous solutions are coded arrays of the right shapes (no
    Helmholtz solve is available without the library)."""
    A, rdm2, cl2m, cm2l = hostinit.eigmod(cfg.gpoc, cfg.hoc, cfg.fnot, atmos=atmos)
    aoc, bd2 = hostinit.bd2oc(cfg)
    nx, ny, nl = cfg.nxpo, cfg.nypo, cfg.nlo
    c = dict(amatoc=A, rdm2oc=rdm2, ctl2moc=cl2m, ctm2loc=cm2l, aoc=aoc, bd2oc=bd2, yporel=cfg.yporel(),
             ddynoc=coded((nx, ny), 9))
    if cfg.cyclic:
        c.update(pch1oc=coded((ny, nl - 1), 1), pch2oc=coded((ny, nl - 1), 2), pbhoc=np.arange(ny) + 0.5, hbsioc=1.5,
                 aipbho=2.5, **{k: np.arange(nl - 1) + 1.0 for k in ("aipcho", "hc1soc", "hc2soc", "hc1noc", "hc2noc")})
    else:
        c.update(ochom=coded((nx, ny, nl - 1), 3), cdiffo=np.zeros((nl, nl - 1)), cdhoc=np.zeros((nl - 1, nl - 1)))
    return c


def rows_of(cfg, kind):
    """(g, p rows, T rows) a handle of `kind` stores: the slab's rows as slab_slice / HipSlab's T-grid rule give
    them (T row j lies between p rows j and j+1: one fewer than the p rows stored), or every row."""
    if kind == "whole":
        return None, slice(0, cfg.nypo), slice(0, cfg.nyto)
    g0, g1 = partition(cfg.nypo, 3)[KINDS.index(kind)]
    nyl, joff, _, _ = local_rows(cfg.nypo, g0, g1)
    return (g0, g1), slab_slice(cfg.nypo, g0, g1), slice(joff, joff + nyl - 1)


def make(cfg, consts, kind, **kw):
    if kind == "whole":
        return (AtmosModel if getattr(cfg, "atmos", False) else OceanModel)(cfg, consts["ddynoc"], 0, consts)
    g0, g1 = partition(cfg.nypo, 3)[KINDS.index(kind)]
    return HipSlab(cfg, consts, g0, g1, KINDS.index(kind), 3, device=0, **kw)


def fields(p):
    return {n: (list(getattr(p, n)) if hasattr(getattr(p, n), "__len__") else getattr(p, n)) for n, _ in Params._fields_}


# (a) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRESETS + ["atmos"])
def test_both_classes_fill_params_alike(fake, name):
    atmos = name == "atmos"
    cfg = atmos_preset("cpl_tiny") if atmos else preset(name)
    consts = consts_of(cfg, atmos)
    made = {}
    for kind in KINDS:
        x = make(cfg, consts, kind)
        made[kind] = fields(fake.args("qgcm_hip_create")[1]._obj)
        assert made[kind] == fields(x.params)
    whole = made["whole"]
    assert (whole["slab_g0"], whole["slab_g1"], whole["atmos"]) == (0, 0, int(atmos))
    assert whole["nlo"] == cfg.nlo and whole["nypo"] == cfg.nypo and whole["rdm2oc"][:cfg.nlo] == list(consts["rdm2oc"])
    for kind, (g0, g1) in zip(KINDS, partition(cfg.nypo, 3)):
        assert (made[kind]["slab_g0"], made[kind]["slab_g1"], made[kind]["atmos"]) == (g0, g1, 0)
        differ = {n for n in whole if whole[n] != made[kind][n]}
        assert differ == ({"slab_g0", "slab_g1", "atmos"} if atmos else {"slab_g0", "slab_g1"})


# (b) -------------------------------------------------------------------------------------------------------------
# setter -> (entry point, grids of its array arguments, trailing arguments)
GLOBAL_SETTERS = {"oml_set_state": ("qgcm_hip_oml_set_state", "tt", ()),
                  "oml_set_forcing": ("qgcm_hip_oml_set_forcing", "ttpp", ()),
                  "set_monitor_fields": ("qgcm_hip_set_monitor_fields", "pptt", ()),
                  "set_time_mean_fields": ("qgcm_hip_set_tav_fields", "t", ()),
                  "set_dtopoc": ("qgcm_hip_set_dtopoc", "p", ()),
                  "set_sponge": ("qgcm_hip_set_sponge", "p", (-2.5e-5,))}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", PRESETS)
def test_global_arrays_are_cut_to_the_stored_rows(fake, name, kind):
    cfg = preset(name)
    consts = consts_of(cfg)
    g, prow, trow = rows_of(cfg, kind)
    npr, ntr, nx, n1 = prow.stop - prow.start, trow.stop - trow.start, cfg.nxpo, cfg.nlo - 1
    assert ntr == npr - 1
    fake.grab = {"qgcm_hip_set_grid": [(npr,), None, (nx, npr)], "qgcm_hip_set_homog_box": [(nx, npr, n1), None, None],
                 "qgcm_hip_set_homog_cyc": [(npr, n1), (npr, n1), (npr,)] + [None] * 7}
    x = make(cfg, consts, kind)
    assert (x.nyl, x.rank, x.nranks) == (npr, 0 if g is None else KINDS.index(kind), 1 if g is None else 3)
    yp, _, dd = fake.got["qgcm_hip_set_grid"]
    assert np.array_equal(yp, consts["yporel"][prow]) and np.array_equal(dd, consts["ddynoc"][:, prow])
    if cfg.cyclic:
        p1, p2, pb = fake.got["qgcm_hip_set_homog_cyc"][:3]
        assert np.array_equal(p1, consts["pch1oc"][prow]) and np.array_equal(p2, consts["pch2oc"][prow])
        assert np.array_equal(pb, consts["pbhoc"][prow])
        assert fake.args("qgcm_hip_set_homog_cyc")[-2:] == (1.5, 2.5)
    else:
        assert np.array_equal(fake.got["qgcm_hip_set_homog_box"][0], consts["ochom"][:, prow, :])
    glob = dict(p=(cfg.nxpo, cfg.nypo), t=(cfg.nxto, cfg.nyto))
    rows, local = dict(p=prow, t=trow), dict(p=(cfg.nxpo, npr), t=(cfg.nxto, ntr))
    for setter, (entry, grids, tail) in GLOBAL_SETTERS.items():
        arrays = [coded(glob[gr], k + 1) for k, gr in enumerate(grids)]
        fake.grab = {entry: [local[gr] for gr in grids]}
        getattr(x, setter)(*arrays, *tail)
        args = fake.args(entry)
        assert len(args) == 1 + len(grids) + len(tail) and args[0] is x.h and args[1 + len(grids):] == tail, setter
        for k, gr in enumerate(grids):
            assert np.array_equal(fake.got[entry][k], arrays[k][:, rows[gr]]), (setter, k)
            if kind == "whole":  # the identity cut hands the caller's own array on
                assert C.cast(args[1 + k], C.c_void_p).value == arrays[k].ctypes.data, (setter, k)
    # the local-block accessors are sized by the stored rows
    assert all(a.shape == (cfg.nxpo, npr, cfg.nlo) for a in x.get_state() + [x.wrk_get()])
    assert all(a.shape == (cfg.nxto, ntr) for a in x.oml_get_state())
    x.close()
    x.close()
    assert not x.h and fake.count("qgcm_hip_destroy") == 1


def test_a_global_array_of_the_wrong_shape_is_refused(fake):
    cfg = preset("box_tiny")
    for kind in ("middle", "whole"):
        x = make(cfg, consts_of(cfg), kind)
        with pytest.raises(AssertionError):
            x.oml_set_state(coded((cfg.nxto, cfg.nyto - 1)), None)
        with pytest.raises(AssertionError):
            x.set_sponge(coded((cfg.nxpo, cfg.nypo + 1)), 1.0)
        with pytest.raises(AssertionError):
            x.set_scalars(np.zeros(x.nscal + 1))


# (c) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["middle", "whole"])
@pytest.mark.parametrize("name", PRESETS)
def test_none_stays_null(fake, name, kind):
    cfg = preset(name)
    x = make(cfg, consts_of(cfg), kind)
    for setter, (entry, grids, tail) in GLOBAL_SETTERS.items():
        getattr(x, setter)(*[None] * len(grids), *tail)
        assert fake.args(entry)[1:1 + len(grids)] == (None,) * len(grids), setter
    assert fake.args("qgcm_hip_set_sponge")[2] == 0.0
    x.set_state(None, None, None, None)
    assert fake.args("qgcm_hip_set_state")[1:] == (None,) * 4
    x.set_forcing(None, None, None)
    assert fake.args("qgcm_hip_set_forcing")[1:] == (None,) * 3
    # one field given, the others left alone
    x.set_monitor_fields(sst=coded((cfg.nxto, cfg.nyto)))
    a = fake.args("qgcm_hip_set_monitor_fields")
    assert a[1:4] == (None,) * 3 and a[4] is not None


# (d) -------------------------------------------------------------------------------------------------------------
def launches(x):
    x.tavocn()
    x.qgostep()
    x.lf_average()
    x.row_transform(0)


@pytest.mark.parametrize("name", PRESETS)
def test_sync_hook(fake, name):
    cfg = preset(name)
    consts = consts_of(cfg)
    for x in (make(cfg, consts, "whole"), make(cfg, consts, "middle")):
        launches(x)
        assert fake.count("qgcm_hip_sync") == 0
    x = make(cfg, consts, "middle", sync_each_call=True)
    n0 = fake.count("qgcm_hip_sync")
    launches(x)
    names = [n for n, _ in fake.calls]
    for entry in ("qgcm_hip_tavocn", "qgcm_hip_qgostep", "qgcm_hip_lf_average", "qgcm_hip_row_transform"):
        assert names[len(names) - 1 - names[::-1].index(entry) + 1] == "qgcm_hip_sync", entry
    assert fake.count("qgcm_hip_sync") == n0 + 4
    x.sync()
    assert fake.count("qgcm_hip_sync") == n0 + 5


# (e) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", PRESETS)
def test_readers_are_sized_by_the_owned_rows(fake, name, kind):
    cfg = preset(name)
    x = make(cfg, consts_of(cfg), kind)
    g0, g1 = (1, cfg.nypo) if kind == "whole" else (x.g0, x.g1)
    own_p = g1 - g0 + 1
    own_t = own_p - 1 if kind in ("north", "whole") else own_p  # the handle that owns row nypo owns one T row fewer
    assert (x.own_p, x.own_t) == (own_p, own_t)
    nxp, nxt, nl = cfg.nxpo, cfg.nxto, cfg.nlo
    shapes = dict(txocav=(nxp, own_p), sstav=(nxt, own_t), pocav=(nxp, own_p, nl), uufo=(nxp, own_t), vvfo=(nxt, own_p))
    if kind == "whole":
        assert x.po_mean().shape == (nxp, cfg.nypo, nl) and (own_p, own_t) == (cfg.nypo, cfg.nyto)
        mean, n = x.po_mean(reset=True, count=True)
        means = x.time_means()
        assert means.pop("nsumoc") == 0
    else:
        mean, n = x.po_mean(reset=True)
        means, nsum = x.time_means()
        assert nsum == 0
    assert mean.shape == (nxp, own_p, nl) and n == 0 and fake.args("qgcm_hip_poavg_out")[3] == 1
    assert len(means) == 16 and all(means[k].shape == s for k, s in shapes.items())
    sub = x.time_means(["sstav"])
    assert list(sub if kind == "whole" else sub[0])[:1] == ["sstav"]


def test_hipslab_oml_init_refreshes_the_message_lengths(fake):
    cfg = preset("box_tiny")
    x = make(cfg, consts_of(cfg), "middle")
    assert not x.oml_on and (x.th_len, x.cst_len, x.halo_len, x.stream_ptr) == (7, 7, 7, 7)
    n = fake.count("qgcm_hip_thomas_msg_len"), fake.count("qgcm_hip_halo_msg_len")
    x.oml_init(qgcm_hip.OmlConfig())
    assert x.oml_on and x.oml_len == 7
    assert (fake.count("qgcm_hip_thomas_msg_len"), fake.count("qgcm_hip_halo_msg_len")) == (n[0] + 1, n[1] + 1)
    p = fake.args("qgcm_hip_oml_init")[1]._obj
    m = make(cfg, consts_of(cfg), "whole")
    m.oml_init(qgcm_hip.OmlConfig())
    q = fake.args("qgcm_hip_oml_init")[1]._obj
    assert bytes(p) == bytes(q) and not hasattr(m, "oml_on")
