#!/usr/bin/env python3
"""Generate tests/golden/hausdorff_*.npz by running the REAL reference functions - trace_fourier_curves (data.py:51-57) at 1000 and
at 100 points, lens_points_from_params (best_shape_fit.py:195-199), max_and_avg_hausdorff_distance (best_shape_fit.py:143-149) and
points_to_lens_loss (best_shape_fit.py:203-209) - on the CPU, the way run_experiments.py:147-159 strings them together.

Runs at development time only, on a machine that has a checkout of the reference, scipy and torch:

    python tests/golden/make_hausdorff_golden.py <directory of the reference checkout>

data.py and best_shape_fit.py import dataset, geometry, plotting and progress packages at the top; the functions above touch none
of them, so whichever is not installed (shapely, for one) is an empty stand-in in sys.modules.  The reference's own lens prototype
needs shapely, so the template is the analytic two-arc lens of tests/hausdorff_oracle.py lens_template.  The reference's tensors
are float32 where the fit made them; here prototype and params go in as float64 copies of their float32 values, so that what is
recorded is the functions' arithmetic and not one more rounding.  Nothing of the reference is copied: a fixture holds data only -
x (curve_oracle.gauss(seed, rows, 5)), the template, params (hausdorff_oracle.golden_params), the reference's max_h, avg_h and
loss (one column per weight of GOLDEN_WEIGHTS) per row, and the dense points the reference traced for the first and the last row.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import curve_oracle as co  # noqa: E402
import hausdorff_oracle as ho  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "best_shape_fit.py")):
        sys.exit(__doc__)
    import torch
    data, _ = import_reference(sys.argv[1])
    import best_shape_fit as bsf
    model = data.LensShapeModel()
    for case in ho.GOLDEN_CASES:
        n = case["rows"]
        x = co.gauss(case["seed"], n, 5)
        template = ho.lens_template(case["points"])
        params = ho.golden_params(case["seed"], n)
        coeffs = model.unflatten_coeffs(x)
        dense = model.trace_fourier_curves(coeffs, n_points=ho.GOLDEN_P)
        coarse = model.trace_fourier_curves(coeffs)
        assert dense.shape == (n, ho.GOLDEN_P, 2) and coarse.shape == (n, ho.GOLDEN_FIT_P, 2) and dense.dtype == np.float64
        proto = torch.from_numpy(template.astype(np.float64))
        max_h, avg_h, loss = np.empty(n), np.empty(n), np.empty((n, len(ho.GOLDEN_WEIGHTS)))
        for j in range(n):
            pr = [torch.tensor([float(v)], dtype=torch.float64) for v in params[j]]
            lens = bsf.lens_points_from_params(proto, pr).numpy()
            max_h[j], avg_h[j] = bsf.max_and_avg_hausdorff_distance(lens, dense[j])
            for w, weight in enumerate(ho.GOLDEN_WEIGHTS):
                loss[j, w] = bsf.points_to_lens_loss(proto, torch.from_numpy(coarse[j]), pr, weight).item()
        ref = ho.distances64(x, template, params, P=ho.GOLDEN_P)
        path = os.path.join(HERE, f"hausdorff_{case['name']}.npz")
        np.savez(path, x=x, template=template, params=params, ref_max_h=max_h, ref_avg_h=avg_h, ref_loss=loss,
                 ref_points_first=dense[0], ref_points_last=dense[-1])
        print(f"{case['name']}: {os.path.getsize(path)} bytes; against the float64 oracle: max_h {np.abs(max_h - ref['max_h']).max():.3g}, "
              f"avg_h {np.abs(avg_h - ref['avg_h']).max():.3g}, points {np.abs(dense - co.points64(x, ho.GOLDEN_P)).max():.3g}")


if __name__ == "__main__":
    main()
