#!/usr/bin/env python3
"""Generates tests/golden/g24_emd.npz: seeded cloud pairs and their exact Earth Mover's optimum for the two sizes at which the numpy
Hungarian of tests/emd_ref.py is too slow for a test: N = 1024 (B = 2) and N = 2048 (B = 1).

Clouds: normalised Gaussian draws, i.e. uniform on the unit sphere; the second cloud of a pair is scaled by 0.9.  Costs: tests/emd_ref.sqdist
(float32, the kernel's rounding order) taken to float64; optimum: scipy.optimize.linear_sum_assignment on that matrix, the matched costs summed
in float64.  Stored: x1_<N>, x2_<N> float32 [B, N, 3], opt_<N> float64 [B], assign_<N> int32 [B, N] (one optimal matching).

    python tests/golden/make_golden_emd.py        (needs scipy)
"""
import os
import sys
import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from emd_ref import sqdist                                            # noqa: E402

CASES = ((1024, 2), (2048, 1))
SEED = 24


def sphere(rs, B, N, scale=1.0):
    x = rs.standard_normal((B, N, 3))
    return (scale * x / np.linalg.norm(x, axis=2, keepdims=True)).astype(np.float32)


def main():
    rs = np.random.RandomState(SEED)
    out = {}
    for N, B in CASES:
        x1, x2 = sphere(rs, B, N), sphere(rs, B, N, 0.9)
        opt, assign = np.empty(B), np.empty((B, N), dtype=np.int32)
        for b in range(B):
            c = sqdist(x1[b], x2[b]).astype(np.float64)
            rows, cols = linear_sum_assignment(c)
            assert np.array_equal(rows, np.arange(N))
            assign[b], opt[b] = cols, c[rows, cols].sum()
        out.update({f"x1_{N}": x1, f"x2_{N}": x2, f"opt_{N}": opt, f"assign_{N}": assign})
        print(N, B, opt)
    path = os.path.join(HERE, "g24_emd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
