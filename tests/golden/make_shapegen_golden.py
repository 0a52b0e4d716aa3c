#!/usr/bin/env python3
"""Generate tests/golden/fcoef_*.npz by running the REAL reference's fourier_coeffs and flatten_coeffs (data.py:42-49, :30-33) on
the CPU: the part of the shape generators that can be pinned to the reference, because it touches neither the polygon library
nor scipy.

Runs at development time only, on a machine that has a checkout of the reference:

    python tests/golden/make_shapegen_golden.py <directory of the reference checkout>

The reference is imported under the stand-in modules make_curve_golden.py uses.  Nothing of the reference is copied: a fixture
holds data only - points [rows, P_max, 2] float64 (zero-padded), counts [rows], and the reference's OUTPUT
flatten_coeffs(fourier_coeffs(points[i, :counts[i]], n_coeffs)[None]) for n_coeffs = 5 and 25 as ref5 [rows, 20], ref25 [rows, 100].
    fcoef_rings     lens rings of tests/shapegen_oracle.py (seed 11): eight with 31 points and eight with 32
    fcoef_outlines  closed outlines of 100 .. 300 points, rounded to float32 so that a GPU test feeds the very same numbers
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import shapegen_oracle as so  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402

OUTLINE_COUNTS = (100, 101, 128, 173, 256, 299, 300)


def ring_cases():
    d = so.draws(11, 0, 400).astype(np.float32)
    d = d[~so.ambiguous(d)]
    ring, cnt = so.rings(d)
    rows = np.concatenate([np.nonzero(cnt == 31)[0][:8], np.nonzero(cnt == 32)[0][:8]])
    return ring[rows].astype(np.float32).astype(np.float64), cnt[rows], d[rows]


def outline_cases():
    rng = np.random.RandomState(5)
    pts = np.zeros((len(OUTLINE_COUNTS), max(OUTLINE_COUNTS), 2))
    for i, c in enumerate(OUTLINE_COUNTS):
        t = 2 * np.pi * np.arange(c) / c
        rad = 1.0 + 0.3 * np.cos(3 * t + rng.rand()) + 0.1 * np.sin(7 * t) + 0.02 * rng.randn(c)
        pts[i, :c, 0] = (1.5 + rng.rand()) * rad * np.cos(t) + rng.randn()
        pts[i, :c, 1] = rad * np.sin(t) + rng.randn()
    return pts.astype(np.float32).astype(np.float64), np.array(OUTLINE_COUNTS, dtype=np.int32)


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "data.py")):
        sys.exit(__doc__)
    data, _ = import_reference(sys.argv[1])
    model = data.LensShapeModel()

    def ref(points, counts, k):
        return np.concatenate([model.flatten_coeffs(model.fourier_coeffs(points[i, :counts[i]], k)[None]) for i in range(len(points))])

    ring, cnt, d = ring_cases()
    np.savez(os.path.join(HERE, "fcoef_rings.npz"), points=ring, counts=cnt, draws=d, ref5=ref(ring, cnt, 5), ref25=ref(ring, cnt, 25))
    pts, pc = outline_cases()
    np.savez(os.path.join(HERE, "fcoef_outlines.npz"), points=pts, counts=pc, ref5=ref(pts, pc, 5), ref25=ref(pts, pc, 25))
    for name, p, c in (("fcoef_rings", ring, cnt), ("fcoef_outlines", pts, pc)):
        f = np.load(os.path.join(HERE, name + ".npz"))
        worst = max(float(np.abs(so.coeffs(p, c, k) - f[f"ref{k}"]).max()) for k in (5, 25))
        print(f"{name}: {len(p)} rows, counts {sorted(set(c.tolist()))}, the oracle's DFT differs from the reference by at most {worst:.3g}")


if __name__ == "__main__":
    main()
