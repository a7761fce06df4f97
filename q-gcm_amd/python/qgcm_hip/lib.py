"""ctypes binding of the C ABI declared in include/qgcm_hip.h."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
MAXL = 8
ABI_VERSION = 3  # QGCM_HIP_ABI_VERSION of include/qgcm_hip.h


class QgcmHipError(RuntimeError):
    pass


def library_path():
    """In-tree build; QGCM_HIP_LIB overrides it (kernel experiments / ablation builds)."""
    return os.environ.get("QGCM_HIP_LIB") or os.path.normpath(os.path.join(HERE, "..", "..", "lib", "libqgcm_hip.so"))


class Params(C.Structure):
    """struct qgcm_hip_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("nxpo", C.c_int), ("nypo", C.c_int), ("nlo", C.c_int), ("cyclic", C.c_int),
        ("fnot", C.c_double), ("beta", C.c_double), ("dxo", C.c_double), ("dyo", C.c_double),
        ("tdto", C.c_double), ("delek", C.c_double), ("bccooc", C.c_double),
        ("ah2oc", C.c_double * MAXL), ("ah4oc", C.c_double * MAXL),
        ("hoc", C.c_double * MAXL), ("gpoc", C.c_double * MAXL),
        ("amatoc", C.c_double * (MAXL * MAXL)), ("ctl2moc", C.c_double * (MAXL * MAXL)),
        ("ctm2loc", C.c_double * (MAXL * MAXL)), ("rdm2oc", C.c_double * MAXL),
        ("aoc", C.c_double),
        ("slab_g0", C.c_int), ("slab_g1", C.c_int),
        ("atmos", C.c_int),
    ]


class OmlParams(C.Structure):
    """struct qgcm_hip_oml_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("hmoc", C.c_double), ("toc1", C.c_double), ("toc2", C.c_double), ("st2d", C.c_double), ("st4d", C.c_double),
        ("ycexp", C.c_double), ("rrcpoc", C.c_double), ("tsbdy", C.c_double), ("tnbdy", C.c_double),
        ("sb_hflux", C.c_int), ("nb_hflux", C.c_int),
    ]


class MonParams(C.Structure):
    """struct qgcm_hip_mon_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("rhooc", C.c_double), ("cpoc", C.c_double), ("hmoc", C.c_double), ("ycexp", C.c_double),
        ("sb_hflux", C.c_int), ("nb_hflux", C.c_int),
    ]


class AtmMonParams(C.Structure):
    """struct qgcm_hip_atm_mon_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("rhoat", C.c_double), ("cpat", C.c_double), ("hmat", C.c_double), ("davgat", C.c_double),
        ("aup", C.c_double * (MAXL - 1)), ("bup", C.c_double), ("cup", C.c_double), ("dup", C.c_double),
        ("nx1", C.c_int), ("ny1", C.c_int), ("nxaooc", C.c_int), ("nyaooc", C.c_int),
    ]


class TavParams(C.Structure):
    """struct qgcm_hip_tav_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("hmoc", C.c_double), ("ycexp", C.c_double), ("tsbdy", C.c_double), ("tnbdy", C.c_double),
        ("sb_hflux", C.c_int), ("nb_hflux", C.c_int),
    ]


class XforcParams(C.Structure):
    """struct qgcm_hip_xforc_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("ndxr", C.c_int), ("nx1", C.c_int), ("ny1", C.c_int), ("nxaooc", C.c_int), ("nyaooc", C.c_int),
        ("cdat", C.c_double), ("raoro", C.c_double), ("hmat", C.c_double), ("hmoc", C.c_double),
        ("bccoat", C.c_double), ("bccooc", C.c_double), ("tau_udiff", C.c_int),
        ("stbbb", C.POINTER(C.c_double)), ("stbus", C.POINTER(C.c_double)), ("stbvs", C.POINTER(C.c_double)),
        ("stbun", C.POINTER(C.c_double)), ("stbvn", C.POINTER(C.c_double)),
    ]


class AmlParams(C.Structure):
    """struct qgcm_hip_aml_params (include/qgcm_hip.h)."""
    _fields_ = [
        ("hmat", C.c_double), ("hmamin", C.c_double), ("hmadmp", C.c_double), ("rrcpat", C.c_double),
        ("tat1", C.c_double), ("tat2", C.c_double), ("xcexp", C.c_double),
        ("at2d", C.c_double), ("at4d", C.c_double), ("ahmd", C.c_double),
        ("aface", C.c_double * (MAXL - 1)), ("bface", C.c_double), ("cface", C.c_double), ("dface", C.c_double),
        ("xc1ast", C.POINTER(C.c_double)), ("dtopat", C.POINTER(C.c_double)),
    ]


class XforcHeatParams(C.Structure):
    """struct qgcm_hip_xforc_heat_params (include/qgcm_hip.h)."""
    _fields_ = [(n, C.c_double) for n in ("xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup",
                                          "C1down", "hmadmp", "hmat")] + [
        (n, C.POINTER(C.c_double)) for n in ("fsa", "fso", "xta", "yta", "xto", "yto")]


class XforcBand(C.Structure):
    """struct qgcm_hip_xforc_band (include/qgcm_hip.h): one rank's part of the band plan."""
    _fields_ = [("a0", C.c_int), ("a1", C.c_int), ("own", C.c_int), ("nseg", C.c_int),
                ("c0", C.c_int * 2), ("c1", C.c_int * 2), ("f0", C.c_int * 2), ("f1", C.c_int * 2),
                ("t0", C.c_int), ("t1", C.c_int), ("nrow", C.c_int), ("mom_len", C.c_int)]


class XforcSum(C.Structure):
    """struct qgcm_hip_xforc_sum (include/qgcm_hip.h): one rank's part of the ownership plan of the owner-computed sums."""
    _fields_ = [(n, C.c_int) for n in ("g0", "g1", "f0", "f1", "t0", "t1", "w0", "w1", "c0", "c1", "u0", "u1", "a0", "a1", "own",
                                       "nrow", "mom_len", "pad")]


class XforcSstParams(C.Structure):
    """struct qgcm_hip_xforc_sst_params (include/qgcm_hip.h)."""
    _fields_ = [(n, C.c_double) for n in ("xlamda", "D0up", "Dmup", "Dmdown", "Adown11", "Bmup", "B1down", "Cmup",
                                          "C1down", "hmadmp", "hmat")] + [
        (n, C.POINTER(C.c_double)) for n in ("fsa", "xta", "yta", "xto", "yto")] + [
        ("dxo", C.c_double), ("dyo", C.c_double), ("sst", C.POINTER(C.c_double))]


class SlabCoupledSwitches(C.Structure):
    """struct qgcm_hip_slab_coupled_switches (include/qgcm_hip.h): the switches and message lengths of a coupled window."""
    _fields_ = [(n, C.c_int) for n in ("oml", "heat", "bands", "udiff_gather", "udiff_sums", "halo_p2p")] + [
        (n, C.c_long) for n in ("xforc_len", "pom_len", "edge_len", "oml_len", "summary_len", "halo_len")]


TAV_NOUT = 16  # QGCM_HIP_TAV_NOUT
ATM_TAV_NOUT = 15  # QGCM_HIP_ATM_TAV_NOUT


# every symbol include/qgcm_hip.h declares
SYMBOLS = [
    "qgcm_hip_create", "qgcm_hip_destroy", "qgcm_hip_last_error", "qgcm_hip_abi_version",
    "qgcm_hip_set_grid", "qgcm_hip_set_geometry", "qgcm_hip_set_homog_box", "qgcm_hip_set_homog_cyc",
    "qgcm_hip_set_state", "qgcm_hip_get_state", "qgcm_hip_set_forcing", "qgcm_hip_tend_zero_mask", "qgcm_hip_set_cyc_forcing", "qgcm_hip_set_sponge",
    "qgcm_hip_set_scalars", "qgcm_hip_get_scalars", "qgcm_hip_get_inv_diag", "qgcm_hip_get_monitors",
    "qgcm_hip_qgostep", "qgcm_hip_ocinvq", "qgcm_hip_ocqbdy", "qgcm_hip_lf_average", "qgcm_hip_ocqbdy_host",
    "qgcm_hip_steps", "qgcm_hip_sync", "qgcm_hip_helmholtz",
    "qgcm_hip_qgastep", "qgcm_hip_atinvq", "qgcm_hip_atqzbd", "qgcm_hip_get_bsums", "qgcm_hip_coupled_steps", "qgcm_hip_set_cu_range",
    "qgcm_hip_wrk_fill", "qgcm_hip_wrk_get", "qgcm_hip_wrk_set", "qgcm_hip_area_integrals",
    "qgcm_hip_local_rows", "qgcm_hip_row_transform", "qgcm_hip_thomas_msg_len", "qgcm_hip_thomas_phase",
    "qgcm_hip_thomas_const_len", "qgcm_hip_thomas_consts", "qgcm_hip_set_thomas_consts", "qgcm_hip_thomas_segments", "qgcm_hip_thomas_plan",
    "qgcm_hip_row_split", "qgcm_hip_row_plan",
    "qgcm_hip_constr", "qgcm_hip_unpack",
    "qgcm_hip_halo_msg_len", "qgcm_hip_halo_pack", "qgcm_hip_halo_unpack", "qgcm_hip_slab_stage", "qgcm_hip_oml_msg_len",
    "qgcm_hip_comm_unique_id", "qgcm_hip_comm_init", "qgcm_hip_slab_steps", "qgcm_hip_comm_set_halo_p2p", "qgcm_hip_comm_set_overlap", "qgcm_hip_comm_probe",
    "qgcm_hip_oml_init", "qgcm_hip_oml_set_state", "qgcm_hip_oml_get_state", "qgcm_hip_oml_set_forcing",
    "qgcm_hip_oml", "qgcm_hip_oml_get_diag", "qgcm_hip_set_dtopoc", "qgcm_hip_valids",
    "qgcm_hip_init_from_p", "qgcm_hip_wekpo_from_tau", "qgcm_hip_prsamp",
    "qgcm_hip_monitor_len", "qgcm_hip_set_mon_params", "qgcm_hip_set_monitor_fields", "qgcm_hip_monitors",
    "qgcm_hip_monitor_part_len", "qgcm_hip_monitors_part", "qgcm_hip_monitors_combine",
    "qgcm_hip_valids_part_len", "qgcm_hip_valids_part", "qgcm_hip_valids_combine",
    "qgcm_hip_prsamp_part_len", "qgcm_hip_prsamp_part", "qgcm_hip_prsamp_combine",
    "qgcm_hip_set_atm_mon_params", "qgcm_hip_set_atm_monitor_fields", "qgcm_hip_atm_monitor_len",
    "qgcm_hip_atm_monitors", "qgcm_hip_atm_valids",
    "qgcm_hip_poavg_enable", "qgcm_hip_poavg_out", "qgcm_hip_set_tav_params", "qgcm_hip_set_tav_fields",
    "qgcm_hip_tavocn", "qgcm_hip_tav_reset", "qgcm_hip_tav_out",
    "qgcm_hip_qocdiag_len", "qgcm_hip_qocdiag", "qgcm_hip_qocdiag_schedule", "qgcm_hip_qocdiag_read",
    "qgcm_hip_ocnc_sample_len", "qgcm_hip_ocnc_sample", "qgcm_hip_subsample_rows",
    "qgcm_hip_set_atm_tav_fields", "qgcm_hip_tavatm", "qgcm_hip_atm_tav_reset", "qgcm_hip_atm_tav_out",
    "qgcm_hip_tavatm_schedule", "qgcm_hip_atnc_sample_len", "qgcm_hip_atnc_sample",
    "qgcm_hip_cov_init", "qgcm_hip_cov_size", "qgcm_hip_cov_add", "qgcm_hip_cov_reset", "qgcm_hip_cov_out",
    "qgcm_hip_cov_schedule", "qgcm_hip_cov_part_len", "qgcm_hip_cov_part", "qgcm_hip_cov_combine",
    "qgcm_hip_areavg_init", "qgcm_hip_areavg_count", "qgcm_hip_areavg", "qgcm_hip_areavg_part_len", "qgcm_hip_areavg_part",
    "qgcm_hip_areavg_combine", "qgcm_hip_cfl_len", "qgcm_hip_cfl", "qgcm_hip_cfl_part_len", "qgcm_hip_cfl_part",
    "qgcm_hip_cfl_combine",
    "qgcm_hip_xforc_init", "qgcm_hip_xforc", "qgcm_hip_xforc_get", "qgcm_hip_coupled_set_xforc",
    "qgcm_hip_aml_init", "qgcm_hip_aml_set_state", "qgcm_hip_aml_get_state", "qgcm_hip_aml", "qgcm_hip_aml_get_diag",
    "qgcm_hip_xforc_heat_init", "qgcm_hip_xforc_heat_get",
    "qgcm_hip_xforc_sst_init", "qgcm_hip_xforc_sst_set", "qgcm_hip_xforc_sst_get",
    "qgcm_hip_xforc_slab_init", "qgcm_hip_xforc_heat_slab_init", "qgcm_hip_xforc_slab_msg_len", "qgcm_hip_xforc_slab_part",
    "qgcm_hip_xforc_slab_combine", "qgcm_hip_xforc_slab_get", "qgcm_hip_xforc_bands", "qgcm_hip_xforc_slab_bands",
    "qgcm_hip_xforc_slab_udiff", "qgcm_hip_xforc_slab_pom_len", "qgcm_hip_xforc_slab_pom_pack", "qgcm_hip_xforc_slab_pom_assemble",
    "qgcm_hip_xforc_sums", "qgcm_hip_xforc_slab_sums", "qgcm_hip_xforc_slab_edge_len", "qgcm_hip_xforc_slab_edge_pack",
    "qgcm_hip_xforc_slab_edge_assemble",
    "qgcm_hip_slab_coupled_code_name", "qgcm_hip_slab_coupled_plan", "qgcm_hip_slab_coupled_init", "qgcm_hip_slab_coupled_steps",
    "qgcm_hip_time_steps", "qgcm_hip_prepare_steps", "qgcm_hip_profile_steps", "qgcm_hip_copy_bandwidth", "qgcm_hip_stream_mix_bandwidth", "qgcm_hip_stream",
    "qgcm_hip_debug_live_allocs",
]

_lib = None


def load_library():
    """Load libqgcm_hip.so; raises QgcmHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise QgcmHipError("HIP library %s is missing - run __graft_entry__.build() "
                           "(make -C q-gcm_amd/csrc); there is no CPU fallback" % path)
    L = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    L.qgcm_hip_last_error.restype = C.c_char_p
    if L.qgcm_hip_abi_version() != ABI_VERSION:
        raise QgcmHipError("%s has ABI version %d, this package binds version %d (include/qgcm_hip.h) - rebuild it"
                           % (path, L.qgcm_hip_abi_version(), ABI_VERSION))
    L.qgcm_hip_create.argtypes = [C.POINTER(vp), C.POINTER(Params), C.c_int]
    L.qgcm_hip_destroy.argtypes = [vp]
    L.qgcm_hip_set_grid.argtypes = [vp, dp, dp, dp]
    L.qgcm_hip_set_geometry.argtypes = [vp, dp, dp]
    L.qgcm_hip_set_homog_box.argtypes = [vp, dp, dp, dp]
    L.qgcm_hip_set_homog_cyc.argtypes = [vp] + [dp] * 8 + [C.c_double, C.c_double]
    L.qgcm_hip_set_state.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_get_state.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_set_forcing.argtypes = [vp, dp, dp, dp]
    if hasattr(L, "qgcm_hip_tend_zero_mask"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_tend_zero_mask.argtypes = [vp]
    L.qgcm_hip_set_cyc_forcing.argtypes = [vp, C.c_double, C.c_double, dp, dp]
    L.qgcm_hip_set_sponge.argtypes = [vp, dp, C.c_double]
    L.qgcm_hip_set_scalars.argtypes = [vp, dp]
    L.qgcm_hip_get_scalars.argtypes = [vp, dp]
    L.qgcm_hip_get_inv_diag.argtypes = [vp, dp, dp]
    L.qgcm_hip_get_monitors.argtypes = [vp, dp, dp]
    for n in ("qgcm_hip_qgostep", "qgcm_hip_ocinvq", "qgcm_hip_ocqbdy", "qgcm_hip_lf_average", "qgcm_hip_sync"):
        getattr(L, n).argtypes = [vp]
    for n in ("qgcm_hip_qgastep", "qgcm_hip_atinvq", "qgcm_hip_atqzbd"):
        getattr(L, n).argtypes = [vp]
    L.qgcm_hip_get_bsums.argtypes = [vp, dp]
    L.qgcm_hip_coupled_steps.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.qgcm_hip_set_cu_range.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_ocqbdy_host.argtypes = [vp, dp, dp]
    L.qgcm_hip_steps.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_helmholtz.argtypes = [vp, dp, dp]
    ip = C.POINTER(C.c_int)
    L.qgcm_hip_local_rows.argtypes = [vp, ip, ip, ip, ip]
    L.qgcm_hip_row_transform.argtypes = [vp, C.c_int]
    L.qgcm_hip_wrk_fill.argtypes = [vp, C.c_double]
    L.qgcm_hip_wrk_get.argtypes = [vp, dp]
    L.qgcm_hip_wrk_set.argtypes = [vp, dp]
    L.qgcm_hip_area_integrals.argtypes = [vp, dp]
    L.qgcm_hip_thomas_msg_len.argtypes = [vp]
    L.qgcm_hip_thomas_const_len.argtypes = [vp]
    L.qgcm_hip_thomas_consts.argtypes = [vp, vp]
    L.qgcm_hip_set_thomas_consts.argtypes = [vp, vp, C.c_int]
    L.qgcm_hip_thomas_phase.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
    L.qgcm_hip_thomas_segments.argtypes = [C.c_int, C.c_int, ip, ip, ip]
    L.qgcm_hip_thomas_plan.argtypes = [vp, ip, ip, ip]
    if hasattr(L, "qgcm_hip_row_split"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_row_split.argtypes = [C.c_int, C.c_int, ip, ip]
        L.qgcm_hip_row_plan.argtypes = [vp, ip, ip]
    L.qgcm_hip_constr.argtypes = [vp]
    L.qgcm_hip_unpack.argtypes = [vp, C.c_int]
    L.qgcm_hip_halo_msg_len.argtypes = [vp]
    L.qgcm_hip_oml_msg_len.argtypes = [vp]
    L.qgcm_hip_halo_pack.argtypes = [vp, vp, vp]
    L.qgcm_hip_halo_unpack.argtypes = [vp, vp, vp]
    L.qgcm_hip_slab_stage.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int]
    L.qgcm_hip_comm_unique_id.argtypes = [C.c_char_p, C.c_int]
    L.qgcm_hip_comm_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.qgcm_hip_slab_steps.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_comm_set_halo_p2p.argtypes = [vp, C.c_int]
    L.qgcm_hip_comm_set_overlap.argtypes = [vp, C.c_int]
    L.qgcm_hip_comm_probe.argtypes = [vp, C.c_int, dp]
    L.qgcm_hip_oml_init.argtypes = [vp, C.POINTER(OmlParams)]
    L.qgcm_hip_oml_set_state.argtypes = [vp, dp, dp]
    L.qgcm_hip_oml_get_state.argtypes = [vp, dp, dp]
    L.qgcm_hip_oml_set_forcing.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_oml.argtypes = [vp]
    L.qgcm_hip_oml_get_diag.argtypes = [vp, dp, dp]
    L.qgcm_hip_set_dtopoc.argtypes = [vp, dp]
    L.qgcm_hip_valids.argtypes = [vp, dp, C.POINTER(C.c_int)]
    L.qgcm_hip_init_from_p.argtypes = [vp]
    L.qgcm_hip_wekpo_from_tau.argtypes = [vp, dp, dp]
    L.qgcm_hip_prsamp.argtypes = [vp, dp]
    L.qgcm_hip_monitor_len.argtypes = [vp]
    L.qgcm_hip_set_mon_params.argtypes = [vp, C.POINTER(MonParams)]
    L.qgcm_hip_set_monitor_fields.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_monitors.argtypes = [vp, dp]
    for n in ("qgcm_hip_monitor_part_len", "qgcm_hip_valids_part_len", "qgcm_hip_prsamp_part_len"):
        getattr(L, n).argtypes = [vp]
    for n in ("qgcm_hip_monitors_part", "qgcm_hip_valids_part", "qgcm_hip_prsamp_part"):
        getattr(L, n).argtypes = [vp, vp]
    L.qgcm_hip_monitors_combine.argtypes = [vp, vp, C.c_int, dp]
    L.qgcm_hip_valids_combine.argtypes = [vp, vp, C.c_int, dp, C.POINTER(C.c_int)]
    L.qgcm_hip_prsamp_combine.argtypes = [vp, vp, C.c_int, dp]
    L.qgcm_hip_set_atm_mon_params.argtypes = [vp, C.POINTER(AtmMonParams)]
    L.qgcm_hip_set_atm_monitor_fields.argtypes = [vp] + [dp] * 7
    L.qgcm_hip_atm_monitor_len.argtypes = [vp]
    L.qgcm_hip_atm_monitors.argtypes = [vp, dp]
    L.qgcm_hip_atm_valids.argtypes = [vp, dp, C.POINTER(C.c_int)]
    L.qgcm_hip_poavg_enable.argtypes = [vp, C.c_int]
    L.qgcm_hip_poavg_out.argtypes = [vp, dp, C.POINTER(C.c_int), C.c_int]
    L.qgcm_hip_set_tav_params.argtypes = [vp, C.POINTER(TavParams)]
    L.qgcm_hip_set_tav_fields.argtypes = [vp, dp]
    L.qgcm_hip_tavocn.argtypes = [vp]
    L.qgcm_hip_tav_reset.argtypes = [vp]
    L.qgcm_hip_tav_out.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_int)]
    ip = C.POINTER(C.c_int)
    L.qgcm_hip_qocdiag_len.argtypes = [vp, C.c_int]
    L.qgcm_hip_qocdiag_len.restype = C.c_long
    L.qgcm_hip_qocdiag.argtypes = [vp, C.c_int, dp]
    L.qgcm_hip_qocdiag_schedule.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.qgcm_hip_qocdiag_read.argtypes = [vp, dp, ip, C.c_int, ip]
    L.qgcm_hip_ocnc_sample_len.argtypes = [vp, C.c_int, ip]
    L.qgcm_hip_ocnc_sample_len.restype = C.c_long
    L.qgcm_hip_ocnc_sample.argtypes = [vp, C.c_int, ip, dp]
    L.qgcm_hip_subsample_rows.argtypes = [vp, C.c_int, ip, ip, ip, ip]
    L.qgcm_hip_set_atm_tav_fields.argtypes = [vp, dp]
    L.qgcm_hip_tavatm.argtypes = [vp]
    L.qgcm_hip_atm_tav_reset.argtypes = [vp]
    L.qgcm_hip_atm_tav_out.argtypes = [vp, C.POINTER(dp), ip]
    L.qgcm_hip_tavatm_schedule.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_atnc_sample_len.argtypes = [vp, C.c_int, ip]
    L.qgcm_hip_atnc_sample_len.restype = C.c_long
    L.qgcm_hip_atnc_sample.argtypes = [vp, C.c_int, ip, dp]
    lp = C.POINTER(C.c_long)
    L.qgcm_hip_cov_init.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.qgcm_hip_cov_size.argtypes = [vp, lp, lp, lp, lp]
    L.qgcm_hip_cov_add.argtypes = [vp]
    L.qgcm_hip_cov_reset.argtypes = [vp]
    L.qgcm_hip_cov_out.argtypes = [vp, C.c_int, dp, dp, lp, C.c_long, C.c_long, dp]
    L.qgcm_hip_cov_schedule.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_cov_part_len.argtypes = [vp]
    L.qgcm_hip_cov_part_len.restype = C.c_long
    L.qgcm_hip_cov_part.argtypes = [vp, vp]
    L.qgcm_hip_cov_combine.argtypes = [vp, vp, C.c_int]
    L.qgcm_hip_areavg_init.argtypes = [vp, C.c_int] + [ip] * 4 + [dp] * 4
    L.qgcm_hip_areavg.argtypes = [vp, dp, dp, dp]
    for n in ("qgcm_hip_areavg_count", "qgcm_hip_areavg_part_len", "qgcm_hip_cfl_len", "qgcm_hip_cfl_part_len"):
        getattr(L, n).argtypes = [vp]
    L.qgcm_hip_areavg_part.argtypes = [vp, vp]
    L.qgcm_hip_areavg_combine.argtypes = [vp, vp, C.c_int, dp, dp, dp]
    L.qgcm_hip_cfl.argtypes = [vp, C.c_double, dp, ip, ip]
    L.qgcm_hip_cfl_part.argtypes = [vp, C.c_double, vp]
    L.qgcm_hip_cfl_combine.argtypes = [vp, vp, C.c_int, C.c_double, dp, ip, ip]
    L.qgcm_hip_xforc_init.argtypes = [vp, vp, C.POINTER(XforcParams)]
    L.qgcm_hip_xforc.argtypes = [vp, vp]
    L.qgcm_hip_xforc_get.argtypes = [vp, vp] + [dp] * 11
    L.qgcm_hip_coupled_set_xforc.argtypes = [vp, vp, C.c_int]
    L.qgcm_hip_aml_init.argtypes = [vp, C.POINTER(AmlParams)]
    L.qgcm_hip_aml_set_state.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_aml_get_state.argtypes = [vp, dp, dp, dp, dp]
    L.qgcm_hip_aml.argtypes = [vp]
    L.qgcm_hip_aml_get_diag.argtypes = [vp, dp, dp]
    L.qgcm_hip_xforc_heat_init.argtypes = [vp, vp, C.POINTER(XforcHeatParams)]
    L.qgcm_hip_xforc_heat_get.argtypes = [vp, vp, dp, dp, dp]
    if hasattr(L, "qgcm_hip_xforc_sst_init"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_xforc_sst_init.argtypes = [vp, C.POINTER(XforcSstParams)]
        L.qgcm_hip_xforc_sst_set.argtypes = [vp, dp]
        L.qgcm_hip_xforc_sst_get.argtypes = [vp, dp, dp]
    if hasattr(L, "qgcm_hip_xforc_slab_init"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_xforc_slab_init.argtypes = [vp, vp, C.POINTER(XforcParams)]
        L.qgcm_hip_xforc_heat_slab_init.argtypes = [vp, vp, C.POINTER(XforcHeatParams)]
        L.qgcm_hip_xforc_slab_msg_len.argtypes = [vp]
        L.qgcm_hip_xforc_slab_part.argtypes = [vp, vp, vp]
        L.qgcm_hip_xforc_slab_combine.argtypes = [vp, vp, vp, C.c_int]
        L.qgcm_hip_xforc_slab_get.argtypes = [vp, vp] + [dp] * 14
    if hasattr(L, "qgcm_hip_xforc_bands"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_xforc_bands.argtypes = [C.c_int] * 6 + [ip, ip, C.POINTER(XforcBand)]
        L.qgcm_hip_xforc_slab_bands.argtypes = [vp, vp] + [C.c_int] * 4
    if hasattr(L, "qgcm_hip_xforc_slab_udiff"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_xforc_slab_udiff.argtypes = [vp, vp, C.c_int, C.c_int]
        L.qgcm_hip_xforc_slab_pom_len.argtypes = [vp, vp, C.POINTER(C.c_long)]
        L.qgcm_hip_xforc_slab_pom_pack.argtypes = [vp, vp, vp]
        L.qgcm_hip_xforc_slab_pom_assemble.argtypes = [vp, vp, vp, C.c_int]
    if hasattr(L, "qgcm_hip_xforc_sums"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_xforc_sums.argtypes = [C.c_int] * 6 + [ip, ip, C.POINTER(XforcSum)]
        L.qgcm_hip_xforc_slab_sums.argtypes = [vp, vp, C.c_int, C.c_int, ip, ip]
        L.qgcm_hip_xforc_slab_edge_len.argtypes = [vp, vp, C.POINTER(C.c_long)]
        L.qgcm_hip_xforc_slab_edge_pack.argtypes = [vp, vp, vp]
        L.qgcm_hip_xforc_slab_edge_assemble.argtypes = [vp, vp, vp, C.c_int]
    if hasattr(L, "qgcm_hip_slab_coupled_plan"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_slab_coupled_code_name.argtypes = [C.c_int]
        L.qgcm_hip_slab_coupled_code_name.restype = C.c_char_p
        L.qgcm_hip_slab_coupled_plan.argtypes = [C.POINTER(SlabCoupledSwitches)] + [C.c_int] * 5 + [C.c_long, ip, C.POINTER(C.c_long),
                                                                                                  C.POINTER(C.c_long)]
        L.qgcm_hip_slab_coupled_init.argtypes = [vp, vp]
        L.qgcm_hip_slab_coupled_steps.argtypes = [vp, vp] + [C.c_int] * 4
    L.qgcm_hip_time_steps.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.qgcm_hip_prepare_steps.argtypes = [vp, C.c_int, C.c_int]
    L.qgcm_hip_profile_steps.argtypes = [vp, C.c_int, C.c_int, dp, C.POINTER(C.c_int),
                                         C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    L.qgcm_hip_copy_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, dp]
    L.qgcm_hip_stream_mix_bandwidth.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_int, dp]
    L.qgcm_hip_stream.argtypes = [vp]
    L.qgcm_hip_stream.restype = vp
    if hasattr(L, "qgcm_hip_debug_live_allocs"):  # (added within ABI version 3: a QGCM_HIP_LIB build may predate it)
        L.qgcm_hip_debug_live_allocs.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_size_t)]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise QgcmHipError(load_library().qgcm_hip_last_error().decode())


def live_allocs():
    """(blocks, bytes) of device memory the library holds in this process right now, over all handles
    (qgcm_hip_debug_live_allocs): exact and process-local, for tests of what a handle gives back."""
    blocks, nbytes = C.c_long(0), C.c_size_t(0)
    check(load_library().qgcm_hip_debug_live_allocs(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


THOMAS_MAX_ROWS = 2048  # QGCM_HIP_THOMAS_MAX_ROWS
THOMAS_SEG_MIN = 4      # QGCM_HIP_THOMAS_SEG_MIN
THOMAS_MAX_SEG = 64     # QGCM_HIP_THOMAS_MAX_SEG
THOMAS_SEG_DEFAULT = 1024  # QGCM_HIP_THOMAS_SEG_DEFAULT


def thomas_segments(nrows, max_rows=0):
    """The segment plan of a column of `nrows` interior rows (qgcm_hip_thomas_segments; host code, no device):
    [(first, count)] per segment.  max_rows = 0: no maximum given (QGCM_HIP_THOMAS_SEG_ROWS unset)."""
    n = C.c_int(0)
    first, count = (C.c_int * THOMAS_MAX_SEG)(), (C.c_int * THOMAS_MAX_SEG)()
    check(load_library().qgcm_hip_thomas_segments(nrows, max_rows, C.byref(n), first, count))
    return [(first[s], count[s]) for s in range(n.value)]


def thomas_plan(handle):
    """The segment plan a handle uses (qgcm_hip_thomas_plan): [(first, count)] per segment, rows counted from the
    handle's first interior row; one entry for a handle on the single-segment kernel."""
    n = C.c_int(0)
    first, count = (C.c_int * THOMAS_MAX_SEG)(), (C.c_int * THOMAS_MAX_SEG)()
    check(load_library().qgcm_hip_thomas_plan(handle, C.byref(n), first, count))
    return [(first[s], count[s]) for s in range(n.value)]


ROW_MAX = 5104          # DST_SINGLE_MAXN (k_dst.h): the longest row (or sub-row) one row transform holds
ROW_SPLIT_MAX_P = 5     # QGCM_HIP_ROW_SPLIT_MAX_P


def row_split(nxto, forced=0):
    """The row plan (P, L) of a zonally cyclic ocean with rows of `nxto` points (qgcm_hip_row_split; host code, no
    device): each row is transformed as P interleaved sub-rows of length L = nxto / P; (1, nxto) up to 5104 points.
    forced > 0: that P (QGCM_HIP_ROW_SPLIT); forced = 0: the default rule."""
    p, l = C.c_int(0), C.c_int(0)
    check(load_library().qgcm_hip_row_split(nxto, forced, C.byref(p), C.byref(l)))
    return p.value, l.value


XFORC_BAND_LINES = ("txisat", "txinat", "txisoc", "txinoc")  # the bits of `own`
XFORC_BAND_HEADER = 8   # XFB_HDR (k_xforc_slab.h): a0, a1, own, 0 and the four line sums in front of the fields
XFORC_POM_HEADER = 8    # XFP_HDR (k_xforc_slab.h): g0, g1, nxpo and zeros in front of the surface pressure's rows
XFORC_BAND_FIELDS = ("tauxa", "tauya", "uekat", "vekat", "wekta", "wekpa")  # the message's fields, (nrow, nxpa) each


def xforc_bands(nxpa, nyta, ndxr, ny1, nyaooc, slab_rows):
    """The band plan of the banded slab xforc (qgcm_hip_xforc_bands; host code, no device) for
    len(slab_rows) ranks; slab_rows[r] = (g0, g1): the global ocean p rows rank r's slab owns.  One
    dict per rank: band (a0, a1) - atmosphere p rows; cells [(c0, c1)] - the one or two intervals of cell rows the fine
    stress is computed on; fine [(f0, f1)] - the fine p rows they cover; trows (t0, t1) - the fine T rows of wektaor;
    own - the names of the line sums the rank forms; nrow - rows per field in the message (the longest band);
    mom_len - doubles of the message's momentum block."""
    n = len(slab_rows)
    lo, hi = (C.c_int * n)(*[int(a) for a, _ in slab_rows]), (C.c_int * n)(*[int(b) for _, b in slab_rows])
    out = (XforcBand * n)()
    check(load_library().qgcm_hip_xforc_bands(int(nxpa), int(nyta), int(ndxr), int(ny1), int(nyaooc), n, lo, hi, out))
    return [dict(band=(b.a0, b.a1), cells=[(b.c0[s], b.c1[s]) for s in range(b.nseg)],
                 fine=[(b.f0[s], b.f1[s]) for s in range(b.nseg)], trows=(b.t0, b.t1),
                 own=tuple(nm for k, nm in enumerate(XFORC_BAND_LINES) if b.own >> k & 1), nrow=b.nrow, mom_len=b.mom_len)
            for b in out]


XFORC_NDXR_MAX = 128    # the widest refinement xforc's set-ups accept
XFORC_WEKPA_STAGE_ABOVE = 64  # XF_WEKPA_STAGE_ABOVE (k_xforc_rows.h): above it the box average is k_xf_wekpa_stage's


def xforc_wekpa_stage_points():
    """XFW_G (k_xf_wekpa_stage.h): the zonally adjacent atmosphere p points a workgroup of the staged box
    average owns (qgcm_hip_xf_wekpa_stage_points; host code, no device)."""
    return int(load_library().qgcm_hip_xf_wekpa_stage_points())


XFORC_SUM_HEADER = 8    # XFS_HDR (k_xforc_slab.h): f0, f1, a0, own and the four line sums in front of the fields
XFORC_EDGE_HEADER = 8   # XFE_HDR: g0, g1, nxpo and zeros in front of the 4 + 4 edge rows
XFORC_EDGE_ROWS = 4     # XFE_ROWS: the owned rows sent from each end of a slab
XFORC_SUM_FIELDS = ("tauxa", "tauya", "vekat", "uekat", "wekpa")  # (uekat, wekpa: partial sums), (nrow, nxpa) each


def xforc_sums(nxpa, nyta, ndxr, ny1, nyaooc, slab_rows):
    """The ownership plan of the owner-computed sums (qgcm_hip_xforc_sums; host code, no device) for
    len(slab_rows) ranks; slab_rows[r] = (g0, g1): the global ocean p rows rank r's slab owns.  One dict per rank: rows
    (g0, g1); fine (f0, f1) - the owned fine p rows; trows (t0, t1) - the owned fine T rows; window (w0, w1) - the fine
    rows whose stress the rank holds correct; cells (c0, c1) - the cell rows k_xf_fine runs on; coarse (u0, u1) - the
    rows of u1at / v1at; arows (a0, a1) - the coarse rows whose sample, uekat line or wekpa box meets the owned rows; own -
    the names of the line sums the rank forms; nrow - rows per field in the message; mom_len - doubles of its momentum
    block."""
    n = len(slab_rows)
    lo, hi = (C.c_int * max(n, 1))(*[int(a) for a, _ in slab_rows]), (C.c_int * max(n, 1))(*[int(b) for _, b in slab_rows])
    out = (XforcSum * max(n, 1))()
    check(load_library().qgcm_hip_xforc_sums(int(nxpa), int(nyta), int(ndxr), int(ny1), int(nyaooc), n, lo, hi, out))
    return [dict(rows=(b.g0, b.g1), fine=(b.f0, b.f1), trows=(b.t0, b.t1), window=(b.w0, b.w1), cells=(b.c0, b.c1),
                 coarse=(b.u0, b.u1), arows=(b.a0, b.a1),
                 own=tuple(nm for k, nm in enumerate(XFORC_BAND_LINES) if b.own >> k & 1), nrow=b.nrow, mom_len=b.mom_len)
            for b in out]


def slab_coupled_plan(nranks, nt0, n, nstr, xforc, oml=False, heat=False, bands=False, udiff_gather=False, udiff_sums=False,
                      halo_p2p=True, xforc_len=0, pom_len=0, edge_len=0, oml_len=0, summary_len=0, halo_len=0):
    """The operations of one coupled window on a y-slab ocean, in the order qgcm_hip_slab_coupled_steps issues them
    (qgcm_hip_slab_coupled_plan; host code, no device): a list of (name, length) - the names of
    qgcm_hip_slab_coupled_code_name, length = doubles per rank of an exchange (gather_*, halo_*) and 0 otherwise.  The
    switches say what the run has set up, the lengths are those of xforc_msg_len, xforc_pom_len, xforc_edge_len,
    oml_len, th_len and halo_len.  The plan is the same on every rank."""
    L = load_library()
    sw = SlabCoupledSwitches(int(bool(oml)), int(bool(heat)), int(bool(bands)), int(bool(udiff_gather)), int(bool(udiff_sums)),
                             int(bool(halo_p2p)), int(xforc_len), int(pom_len), int(edge_len), int(oml_len), int(summary_len),
                             int(halo_len))
    args = (C.byref(sw), int(nranks), int(nt0), int(n), int(nstr), int(bool(xforc)))
    count = C.c_long(0)
    check(L.qgcm_hip_slab_coupled_plan(*args, 0, None, None, C.byref(count)))
    m = max(count.value, 1)
    codes, lens = (C.c_int * m)(), (C.c_long * m)()
    check(L.qgcm_hip_slab_coupled_plan(*args, m, codes, lens, C.byref(count)))
    return [(L.qgcm_hip_slab_coupled_code_name(codes[k]).decode(), int(lens[k])) for k in range(count.value)]


def row_plan(handle):
    """The row plan (P, L) a handle uses (qgcm_hip_row_plan); (1, nxto) for a handle that transforms its rows whole."""
    p, l = C.c_int(0), C.c_int(0)
    check(load_library().qgcm_hip_row_plan(handle, C.byref(p), C.byref(l)))
    return p.value, l.value
