#!/usr/bin/env python3
"""Pins the split rows to the reference itself, in the manner of make_golden_fullsize.py: two steps of the
TRUE reference on a thin zonally cyclic channel of 33 rows at a real row length, nxto = 5760 (SOcn 4 km) and 23040
(SOcn 1 km), from the deterministic synthetic inputs of qgcm_hip.synth.  Stored: every 96th (23040: 384th) column, all
rows, of po, pom, qo, qom + the constraint scalars after steps 1 and 2 (tests/golden/longrows_<nxto>_sample.npz, under
half a megabyte each).  The tests re-generate the inputs from the same synth code; a strided sample of the inputs is
stored too and must match bit for bit.  The reference builds of the two channels are registered here, at run time
(oracle/ref_binding.CONFIGS has no entry for them).  Build container only:

    python tests/golden/make_golden_long_rows_sample.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "q-gcm_amd", "python"))

import ref_binding  # noqa: E402
from qgcm_hip import synth  # noqa: E402
from qgcm_hip.config import _SOCN, OceanConfig  # noqa: E402

STRIDE = {5760: 96, 23040: 384}


def channel(nxto):
    """tests/test_gpu_long_rows.long_cfg: nxto columns, 33 rows, the constants of the Southern Ocean presets at 5 km."""
    return OceanConfig("longrows_%d" % nxto, nxto // 16, 8, nxto // 16, 2, 16, 3, dxo=5.0e3, **_SOCN)


def make(nxto):
    cfg = channel(nxto)
    ST = STRIDE[nxto]
    ref = "cyc_rows%d" % nxto
    ref_binding.CONFIGS[ref] = (cfg.nxta, cfg.nyta, "nxta", cfg.nyaooc, cfg.ndxr, cfg.nlo, "-1.19467D-04", "1.31301D-11", 1)
    ref_binding.build(ref)
    r = ref_binding.RefLib(ref)
    assert (r.nx, r.ny, r.nl, bool(r.cyclic)) == (cfg.nxpo, cfg.nypo, cfg.nlo, cfg.cyclic)
    assert r.fnot == cfg.fnot and r.beta == cfg.beta
    r.init(cfg.dxo, cfg.dto, cfg.delek, cfg.bccooc, cfg.ah2oc, cfg.ah4oc, cfg.hoc, cfg.gpoc)
    po = synth.gaussian_eddy(cfg, noise=1e-3)
    tx, ty = synth.wind_stress(cfg)
    _, wek = synth.wekpo_from_tau(cfg, tx, ty)
    r.set_p(po, po)
    r.set_forcing(wek, np.zeros_like(wek), np.zeros(cfg.nlo - 1))
    txis, txin = synth.tau_line_integrals(cfg, tx)
    r.set_cyc_forcing(txis, txin)
    out = {"stride": np.array(ST), "in_po": po[::ST].copy(), "in_wekpo": wek[::ST].copy(), "in_txis": np.array(txis),
           "in_txin": np.array(txin)}
    for s in (1, 2):
        r.steps(s, 1)
        for n, v in zip(("po", "pom", "qo", "qom"), r.get_state()):
            out["steps%d_%s" % (s, n)] = v[::ST].copy()
            out["steps%d_%s_max" % (s, n)] = np.array(np.abs(v).max())
        out["steps%d_scal" % s] = r.get_scalars()
    np.savez_compressed(os.path.join(HERE, "longrows_%d_sample.npz" % nxto), **out)
    print("wrote longrows_%d_sample.npz" % nxto)


if __name__ == "__main__":
    if len(sys.argv) == 2:
        make(int(sys.argv[1]))
    else:  # one process per channel: the reference libraries export identical symbols
        for n in sorted(STRIDE):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), str(n)])
