"""Which launches one step makes, per configuration (the step plan).  Every case creates a model, sets a
synthetic state and counts the launches of profile_steps(30, s0=1) per kernel class - steps 1 and 26 are the ocean's
leapfrog-averaging steps (the atmosphere averages every 100 steps: step 1 only).  The bitwise A/B tests pin the RESULTS
of every path; this file pins which path a configuration TAKES, so that a change of the host code that silently routes
a configuration through another (equally correct, slower) sequence fails here.

The table is measured, not derived: the dictionaries were recorded with this file at commit c6e6950 ("Step the
atmospheric mixed layer and the heat half of xforc on device"), before the step plan existed, and pasted in.  Only
kernel classes with at least one launch are listed; every other class must count zero.  k_noop is the empty launch
that closes each profiled step, k_noop_train the 512 empty launches of the calibration."""
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, see qgcm_hip/slab.py)

from common import atm_apply, atm_wide
from qgcm_hip import AtmosModel, config, synth
from test_gpu_tavg import ocean

pytestmark = pytest.mark.gpu

# id: (preset, variant, switch set before the handle is created)
CASES = {
    "box_tiny": ("box_tiny", None, None),            # generic box rows, 3 layers
    "box_tiny5": ("box_tiny5", None, None),          # ... 5 layers
    "box_med": ("box_med", None, None),              # k_dst64_unpack
    "cyc_tiny": ("cyc_tiny", None, None),            # generic cyclic rows
    "cyc_tiny6": ("cyc_tiny6", None, None),          # ... 6 layers
    "cyc_med": ("cyc_med", None, None),              # k_rfft64_unpack
    "cyc_2880": ("cyc_2880", None, None),            # k_rfft3_unpack
    "atm_cpl_tiny": ("cpl_tiny", "atmos", None),     # the smallest atmosphere the tests step
    "atm_385_a4": ((384, 4), "atmos_wide", None),    # 385 x 13, four layers: k_rfft64_unpack with the constraint riding
    "atm_385_a5": ((384, 5), "atmos_wide", None),    # ... five: plain inverse rows + k_constr_cyc + k_unpack_cyc
    "box_med_oml": ("box_med", "oml", None),
    "box_med_po_mean": ("box_med", "po_mean", None),
    "box_med_no_fused_constr": ("box_med", None, "QGCM_HIP_NO_FUSED_CONSTR"),
    "box_med_no_fused_unpack": ("box_med", None, "QGCM_HIP_NO_FUSED_UNPACK"),
    "box_med_no_fused_avg": ("box_med", None, "QGCM_HIP_NO_FUSED_AVG"),
    "box_med_generic_dst": ("box_med", None, "QGCM_HIP_GENERIC_DST"),
    "cyc_2880_no_fused_constr": ("cyc_2880", None, "QGCM_HIP_NO_FUSED_CONSTR"),
    "cyc_2880_no_fused_avg": ("cyc_2880", None, "QGCM_HIP_NO_FUSED_AVG"),
}

EXPECTED = {
    "box_tiny": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_unpack": 30,
                 "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "box_tiny5": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30, "k_unpack": 30,
                  "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "box_med": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2, "k_noop": 30,
                "k_noop_train": 512},
    "cyc_tiny": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_unpack": 30,
                 "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "cyc_tiny6": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30, "k_unpack": 30,
                  "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "cyc_med": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2, "k_noop": 30,
                "k_noop_train": 512},
    "cyc_2880": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2, "k_noop": 30,
                 "k_noop_train": 512},
    "atm_cpl_tiny": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_unpack": 30,
                     "k_lf_average": 1, "k_noop": 30, "k_noop_train": 512},
    # (not recorded but required: the atmosphere's layer count must pick the launches the cyclic ocean's does - four
    #  layers as cyc_med, five as cyc_tiny6 - with the atmosphere's single averaging at step 1)
    "atm_385_a4": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 1, "k_noop": 30,
                   "k_noop_train": 512},
    "atm_385_a5": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30, "k_unpack": 30,
                   "k_lf_average": 1, "k_noop": 30, "k_noop_train": 512},
    "box_med_oml": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2,
                    "k_oml": 30, "k_oml_entoc": 30, "k_noop": 30, "k_noop_train": 512},
    "box_med_po_mean": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2,
                        "k_noop": 30, "k_noop_train": 512, "k_poavg_add": 30},
    "box_med_no_fused_constr": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30,
                                "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "box_med_no_fused_unpack": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30,
                                "k_unpack": 30, "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "box_med_no_fused_avg": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2,
                             "k_noop": 30, "k_noop_train": 512},
    "box_med_generic_dst": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_unpack": 30,
                            "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "cyc_2880_no_fused_constr": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_constr": 30,
                                 "k_unpack": 30, "k_lf_average": 2, "k_noop": 30, "k_noop_train": 512},
    "cyc_2880_no_fused_avg": {"k_tend": 30, "k_dst_fwd": 30, "k_thomas": 30, "k_dst_inv": 30, "k_lf_average": 2,
                              "k_noop": 30, "k_noop_train": 512},
}


def launches(case):
    """{kernel class: launches} of steps 1 .. 30 of a fresh model of `case` (classes that never launch left out)."""
    name, variant, _ = CASES[case]
    if variant in ("atmos", "atmos_wide"):
        acfg = config.atmos_preset(name) if variant == "atmos" else atm_wide(*name)
        f = synth.atmos_fields(acfg)
        m = AtmosModel(acfg, ddynat=f["ddynat"])
        atm_apply(m, f)
    else:
        m = ocean(name, variant == "oml")
        if variant == "po_mean":
            m.enable_po_mean()
    try:
        prof = m.profile_steps(30, s0=1)
    finally:
        m.close()
    return {k: n for k, (_, n) in prof.items() if n}


@pytest.mark.parametrize("case", list(CASES))
def test_launches_of_30_steps(case, monkeypatch):
    switch = CASES[case][2]
    if switch:
        monkeypatch.setenv(switch, "1")  # read when a handle is created
    got = launches(case)
    print(case, got)
    assert got == EXPECTED[case]
