#!/usr/bin/env python3
"""Generate tests/golden/lensfit_*.npz by running the REAL reference functions on the CPU:

  grad_n16  points_to_lens_loss(prototype, points, params, w).backward() (best_shape_fit.py:203-209 over :195-199): the loss and
            the four gradients for lensfit_oracle.GOLDEN_GRAD's rows and weights, on the 100 points the reference traces
            (data.py:51-57); prototype and params go in as float64 copies of their float32 values, so that what is recorded is the
            functions' arithmetic and not one more rounding;
  fit_n8, fit_edge_n8
            fit_lens_shape_to_points(points) (best_shape_fit.py:230-261), called as run_experiments.py:150-152 calls it - on the
            float32 tensor of a row's 100 traced points - for the rows of lensfit_oracle.GOLDEN_FIT and GOLDEN_FIT_EDGE: the
            returned parameters.

Runs at development time only, on a machine that has a checkout of the reference, scipy and torch:

    python tests/golden/make_lensfit_golden.py <directory of the reference checkout>

The reference's own lens prototype needs shapely (a stand-in here, see make_curve_golden.import_reference), so
best_shape_fit.get_lens_prototype is replaced, in this script, by the analytic lens of tests/lensfit_oracle.py lens_prototype(130).
Nothing of the reference is copied: a fixture holds data only - x (lensfit_oracle.lens_rows), the prototype, the parameters and
what the reference returned.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import curve_oracle as co  # noqa: E402
import lensfit_oracle as lo  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "best_shape_fit.py")):
        sys.exit(__doc__)
    import torch
    data, _ = import_reference(sys.argv[1])
    import best_shape_fit as bsf
    model = data.LensShapeModel()

    case = lo.GOLDEN_GRAD
    n, weights = case["rows"], case["weights"]
    x = lo.lens_rows(case["seed"], n)
    proto32 = lo.lens_prototype(case["points"])
    params = lo.golden_grad_params(case["seed"], n)
    coarse = model.trace_fourier_curves(model.unflatten_coeffs(x))
    assert coarse.shape == (n, lo.FIT_P, 2) and coarse.dtype == np.float64
    proto = torch.from_numpy(proto32.astype(np.float64))
    loss, grad = np.empty((n, len(weights))), np.empty((n, len(weights), 4))
    worst = 0.0
    for j in range(n):
        for w, weight in enumerate(weights):
            pr = [torch.tensor([float(v)], dtype=torch.float64, requires_grad=True) for v in params[j]]
            L = bsf.points_to_lens_loss(proto, torch.from_numpy(coarse[j]), pr, weight)
            L.backward()
            loss[j, w], grad[j, w] = L.item(), [v.grad.item() for v in pr]
            L64, g64, _ = lo.evaluate64(proto32, co.points64(x, lo.FIT_P)[j], params[j], weight)
            worst = max(worst, abs(L64 - loss[j, w]), np.abs(g64 - grad[j, w]).max())
    path = os.path.join(HERE, f"lensfit_{case['name']}.npz")
    np.savez(path, x=x, prototype=proto32, params=params, ref_loss=loss, ref_grad=grad)
    print(f"{case['name']}: {os.path.getsize(path)} bytes; against the float64 oracle: {worst:.3g}")

    for case in (lo.GOLDEN_FIT, lo.GOLDEN_FIT_EDGE):
        n = case["rows"]
        x = lo.lens_rows(case["seed"], n)
        proto32 = lo.lens_prototype(case["points"])
        bsf.get_lens_prototype = lambda: torch.from_numpy(proto32.copy())
        coarse = model.trace_fourier_curves(model.unflatten_coeffs(x))
        fitted = np.empty((n, 4), np.float32)
        diffs = []
        for j in range(n):
            points = torch.tensor(coarse[j]).float()
            fitted[j] = [float(v) for v in bsf.fit_lens_shape_to_points(points)]
            b = points.numpy().astype(np.float64)
            diffs.append(lo.param_diff(lo.fit64(proto32, b, lo.starts64(b))["params"], fitted[j]))
        path = os.path.join(HERE, f"lensfit_{case['name']}.npz")
        np.savez(path, x=x, prototype=proto32, ref_params=fitted)
        print(f"{case['name']}: {os.path.getsize(path)} bytes; against the float64 restatement of the fit: " +
              ", ".join(f"{d:.2g}" for d in diffs))

if __name__ == "__main__":
    main()
