#!/usr/bin/env python3
"""Generate tests/golden/plusgen_rings.npz by running the REAL reference's PlusShapeModel.densify_polyline, fourier_coeffs and
flatten_coeffs (data.py:176-186, :42-49, :30-33) on the CPU: everything of generate_plus_shape after the union, the part that can
be pinned to the reference, because the union itself needs the polygon library.

Runs at development time only, on a machine that has a checkout of the reference:

    python tests/golden/make_plusgen_golden.py <directory of the reference checkout>

The reference is imported under the stand-in modules make_curve_golden.py uses.  Nothing of the reference is copied: the fixture
holds data only - for corner rings of tests/plusgen_oracle.py covering all nine patterns (tests/plusgen_cases.py pattern_draws, two
rows of each, and the exact half-integer row of corner_case_draws):
    draws [rows, 9] float32, arms [rows], corners [rows], rings [rows, 12, 2] float64 (NaN behind a ring's corners)
    dense [rows, 128, 2] float64, zero-padded, and counts [rows]: the reference's OUTPUT densify_polyline(ring)
    ref25 [rows, 100]: its OUTPUT flatten_coeffs(fourier_coeffs(dense, 25)[None])
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import plusgen_oracle as po  # noqa: E402
from plusgen_cases import corner_case_draws, pattern_draws  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402


def ring_cases():
    d, masks = pattern_draws(per=2)
    d = np.concatenate([d, corner_case_draws()[-1:]])
    c = po.local_coords(d)
    V, nc = po.ring_sorted(c)
    return d, po.arms(c), nc, V


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "data.py")):
        sys.exit(__doc__)
    data, _ = import_reference(sys.argv[1])
    model = data.PlusShapeModel()
    d, arms, nc, V = ring_cases()
    dense = np.zeros((len(d), po.POINTS, 2))
    counts = np.zeros(len(d), dtype=np.int32)
    ref25 = np.zeros((len(d), 100))
    for i in range(len(d)):
        pts = model.densify_polyline(V[i, :nc[i]])
        counts[i] = len(pts)
        dense[i, :len(pts)] = pts
        ref25[i] = model.flatten_coeffs(model.fourier_coeffs(pts, 25)[None])[0]
    np.savez(os.path.join(HERE, "plusgen_rings.npz"), draws=d, arms=arms.astype(np.int32), corners=nc.astype(np.int32), rings=V,
             dense=dense, counts=counts, ref25=ref25)
    mine, N = po.densify(V, nc)
    print(f"plusgen_rings: {len(d)} rows, arms {sorted(set(arms.tolist()))}, counts {counts.min()}..{counts.max()}; the oracle's "
          f"densify differs from the reference by at most {np.abs(mine - dense).max():.3g} (counts equal: {(N == counts).all()}), its "
          f"DFT by at most {np.abs(po.coeffs(dense, counts) - ref25).max():.3g}")


if __name__ == "__main__":
    main()
