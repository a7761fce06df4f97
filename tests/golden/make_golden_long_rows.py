#!/usr/bin/env python3
"""FFTPACK known-answer vectors at the row lengths of the Southern Ocean presets beyond one row transform (SOcn 4 km,
3 km, 2 km, 1 km: nxto = 5760, 7680, 11520, 23040): drfftf / drfftb of the TRUE reference's FFTPACK, made the way
make_golden.py makes fftpack_long.  One file per length, tests/golden/fftpack_rows_<n>.npz (23040 x 3 doubles are
553 KB); any reference build serves (FFTPACK does not depend on the grid).

Run in the build container only (needs the reference's sources):

    python tests/golden/make_golden_long_rows.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_binding  # noqa: E402

LENGTHS = (5760, 7680, 11520, 23040)


def make(r, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    f = r.drfft(x, +1)
    out = {"drfft_in_%d" % n: x, "drfftf_out_%d" % n: f, "drfftb_out_%d" % n: r.drfft(f, -1)}
    np.savez_compressed(os.path.join(HERE, "fftpack_rows_%d.npz" % n), **out)
    print("wrote fftpack_rows_%d" % n)


if __name__ == "__main__":
    ref_binding.build("box_tiny")
    ref = ref_binding.RefLib("box_tiny")
    for n in LENGTHS:
        make(ref, n)
