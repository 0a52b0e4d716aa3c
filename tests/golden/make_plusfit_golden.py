#!/usr/bin/env python3
"""Generate tests/golden/plusfit_*.npz by running the REAL reference functions on the CPU:

  grad_n16  points_to_plus_loss(points, params, w).backward() (best_shape_fit.py:54-65 over :26-50 and :15-22) in float64: the
            loss and the nine gradients for plusfit_oracle.GOLDEN_GRAD's rows and weights, on the 100 points the reference traces
            (data.py:51-57); the parameters go in as float64 copies of their float32 values.  Rows 3 and 7 have xlength = 1
            (both clamps of the x arm act), rows 5 and 11 ylength = 0.5;
  fit_n6    fit_plus_shape_to_points(points) (best_shape_fit.py:93-129), called as eval_shapes.py:85-87 calls it - on the float32
            tensor of a row's 100 traced points - under np.random.seed(plusfit_oracle.GOLDEN_FIT["np_seed"]), with fit_line
            (:83-89, RANSAC) wrapped to record the angle it gave and points_to_plus_loss wrapped to count the starts that ran:
            the coefficients, the RANSAC angle, the returned parameters, the number of starts.

Runs at development time only, on a machine that has a checkout of the reference, scipy, scikit-learn and torch:

    python tests/golden/make_plusfit_golden.py <directory of the reference checkout>

Nothing of the reference is copied: a fixture holds data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import curve_oracle as co  # noqa: E402
import plusfit_oracle as pfo  # noqa: E402
from make_curve_golden import import_reference  # noqa: E402


def golden_grad_params(case):
    _, base = pfo.plus_rows(case["seed"], case["rows"])
    p = pfo.eval_params(base, case["seed"] + 1)
    p[[3, 7], 0] = 1.0
    p[[5, 11], 1] = 0.5
    return p


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "best_shape_fit.py")):
        sys.exit(__doc__)
    import torch
    data, _ = import_reference(sys.argv[1])
    import best_shape_fit as bsf
    model = data.LensShapeModel()

    case = pfo.GOLDEN_GRAD
    n, weights = case["rows"], case["weights"]
    x, _ = pfo.plus_rows(case["seed"], n)
    params = golden_grad_params(case)
    coarse = model.trace_fourier_curves(model.unflatten_coeffs(x))
    assert coarse.shape == (n, pfo.FIT_P, 2) and coarse.dtype == np.float64
    loss, grad = np.empty((n, len(weights))), np.empty((n, len(weights), 9))
    worst = 0.0
    b64 = co.points64(x, pfo.FIT_P)
    for j in range(n):
        for w, weight in enumerate(weights):
            pr = [torch.tensor([float(v)], dtype=torch.float64, requires_grad=True) for v in params[j]]
            L = bsf.points_to_plus_loss(torch.from_numpy(coarse[j]), pr, weight)
            L.backward()
            loss[j, w], grad[j, w] = L.item(), [v.grad.item() for v in pr]
            L64, g64, _ = pfo.evaluate64(b64[j], params[j], weight)
            worst = max(worst, abs(L64 - loss[j, w]), np.abs(g64 - grad[j, w]).max())
    path = os.path.join(HERE, f"plusfit_{case['name']}.npz")
    np.savez(path, x=x, params=params, ref_loss=loss, ref_grad=grad)
    print(f"{case['name']}: {os.path.getsize(path)} bytes; against the float64 oracle: {worst:.3g}")

    case = pfo.GOLDEN_FIT
    n = case["rows"]
    x, _ = pfo.plus_rows(case["seed"], n)
    coarse = model.trace_fourier_curves(model.unflatten_coeffs(x))
    angles, calls = [], [0]
    fit_line, loss_fn = bsf.fit_line, bsf.points_to_plus_loss

    def recording_fit_line(points):
        line = fit_line(points)
        angles.append(float(np.arctan2(line[1, 1] - line[0, 1], 1)))
        return line

    def counting_loss(*a, **k):
        calls[0] += 1
        return loss_fn(*a, **k)

    bsf.fit_line, bsf.points_to_plus_loss = recording_fit_line, counting_loss
    fitted, n_run = np.empty((n, 9), np.float32), np.empty(n, np.int32)
    diffs = []
    np.random.seed(case["np_seed"])
    for j in range(n):
        calls[0] = 0
        points = torch.tensor(coarse[j]).float()
        fitted[j] = [float(v) for v in bsf.fit_plus_shape_to_points(points)]
        assert calls[0] % 400 == 0
        n_run[j] = calls[0] // 400
        b = points.numpy().astype(np.float64)
        ref = pfo.fit64(b, pfo.starts64(b, angles[j]))
        diffs.append((pfo.param_diff(ref["params"], fitted[j]), ref["n_run"]))
    path = os.path.join(HERE, f"plusfit_{case['name']}.npz")
    np.savez(path, x=x, ref_angle=np.array(angles), ref_params=fitted, ref_n_run=n_run)
    print(f"{case['name']}: {os.path.getsize(path)} bytes; starts run {n_run.tolist()}; against the float64 restatement of the "
          "fit (deviation, its starts): " + ", ".join(f"{d:.2g} ({k})" for d, k in diffs))


if __name__ == "__main__":
    main()
