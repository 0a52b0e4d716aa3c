#!/usr/bin/env python3
"""Generate tests/golden/plus_*.npz by running the REAL reference functions - trace_fourier_curves (data.py:51-57) at 1000 and at
100 points, plus_segments_from_params (best_shape_fit.py:26-50), points_to_plus_loss (best_shape_fit.py:54-65),
max_and_avg_hausdorff_distance_plus_shape (best_shape_fit.py:153-156) and densify_polyline (data.py:176-186) - on the CPU, the way
eval_shapes.py:82-95 strings them together.

Runs at development time only, on a machine that has a checkout of the reference, scipy and torch:

    python tests/golden/make_plus_golden.py <directory of the reference checkout>

The reference's modules import dataset, geometry, plotting and progress packages at the top; the functions above touch none of
them, so whichever is not installed (shapely, for one) is an empty stand-in in sys.modules (make_curve_golden.import_reference).
The params go in as float64 one-element tensors of their float32 values, so that what is recorded is the functions' arithmetic and
not one more rounding.  Nothing of the reference is copied: a fixture holds data only - x (curve_oracle.gauss(seed, rows, K)),
params (plus_oracle.golden_params), and per row the reference's kept segments (padded to 12 with NaN, and their number), its loss
(one column per weight of GOLDEN_WEIGHTS) on the 100-point trace, max_h and avg_h on the 1000-point trace, and the length of the
densified outline.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import plus_oracle as po  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "best_shape_fit.py")):
        sys.exit(__doc__)
    import torch
    data, _ = import_reference(sys.argv[1])
    import best_shape_fit as bsf
    model = data.PlusShapeModel()
    for case in po.GOLDEN_CASES:
        n = case["rows"]
        x, params = po.golden_x(case), po.golden_params(case)
        coeffs = model.unflatten_coeffs(x)
        dense = model.trace_fourier_curves(coeffs, n_points=po.GOLDEN_P)
        coarse = model.trace_fourier_curves(coeffs)
        assert dense.shape == (n, po.GOLDEN_P, 2) and coarse.shape == (n, po.GOLDEN_FIT_P, 2) and dense.dtype == np.float64
        segs, n_seg = np.full((n, 12, 2, 2), np.nan), np.empty(n, np.int64)
        max_h, avg_h, loss, M = np.empty(n), np.empty(n), np.empty((n, len(po.GOLDEN_WEIGHTS))), np.empty(n, np.int64)
        for j in range(n):
            pr = [torch.tensor([float(v)], dtype=torch.float64) for v in params[j]]
            s = bsf.plus_segments_from_params(pr).numpy()
            n_seg[j] = len(s)
            segs[j, :len(s)] = s
            max_h[j], avg_h[j] = bsf.max_and_avg_hausdorff_distance_plus_shape(pr, dense[j])
            M[j] = len(model.densify_polyline(s[:, 0, :], max_dist=po.GOLDEN_MAX_DIST))
            for w, weight in enumerate(po.GOLDEN_WEIGHTS):
                loss[j, w] = bsf.points_to_plus_loss(torch.from_numpy(coarse[j]), pr, weight).item()
        ref = po.plus64(params, x, po.GOLDEN_P, po.GOLDEN_MAX_DIST)
        path = os.path.join(HERE, f"plus_{case['name']}.npz")
        np.savez(path, x=x, params=params, ref_segments=segs, ref_n_segments=n_seg, ref_max_h=max_h, ref_avg_h=avg_h, ref_loss=loss,
                 ref_outline_points=M)
        print(f"{case['name']}: {os.path.getsize(path)} bytes; against the float64 oracle: max_h {np.abs(max_h - ref['max_h']).max():.3g}, "
              f"avg_h {np.abs(avg_h - ref['avg_h']).max():.3g}, M {np.abs(M - ref['M']).max()}, kept segments {n_seg.tolist()}")


if __name__ == "__main__":
    main()
