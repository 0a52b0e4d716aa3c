#!/usr/bin/env python3
"""Generate tests/golden/abc_*.npz by running the REAL reference quantile_ABC (rejection_sampling.py:88-96) on the CPU.

Runs at development time only, on a machine that has a checkout of the reference and scipy (distance_matrix):

    python tests/golden/make_abc_golden.py <directory of the reference checkout>

rejection_sampling.py imports the reference's `data` module (datasets, a simulator) and plotting / progress packages at the
top; none of them is touched by quantile_ABC, so `data` and whichever of the others is not installed are empty stand-ins in
sys.modules.  Nothing of the reference is copied: a fixture holds the case's seed and shape, the checksum of the inputs
regenerated from it (tests/abc_oracle.py golden_inputs; the last column of x is the row number), and the reference's OUTPUT -
the row numbers of its sample, in its order, and its threshold.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from abc_oracle import GOLDEN_CASES, band_count, checksum, golden_inputs, order64  # noqa: E402


def import_reference(ref_dir):
    sys.modules["data"] = types.ModuleType("data")
    for name in ("matplotlib", "matplotlib.pyplot", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].__dict__.setdefault("tqdm", lambda it, *a, **k: it)
    from scipy.spatial import distance_matrix  # noqa: F401  (the reference's distances: a stand-in would record nothing)
    sys.path.insert(0, ref_dir)
    import rejection_sampling
    return rejection_sampling


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "rejection_sampling.py")):
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    for case in GOLDEN_CASES:
        x, y, t = golden_inputs(case)
        n = case["n"]
        with contextlib.redirect_stdout(io.StringIO()):
            sample, threshold = ref.quantile_ABC(x, y, t, n=n)
        rows = sample[:, -1].astype(np.int64)
        assert sample.shape == (n, x.shape[1]) and np.array_equal(x[rows], sample)
        D, order = order64(y, t)
        same = np.array_equal(order[1:n + 1], rows)
        diff = float(threshold) - float(np.sqrt(D[order[n + 1]]))
        np.savez(os.path.join(HERE, f"abc_{case['name']}.npz"), seed=np.int64(case["seed"]), N=np.int64(case["N"]),
                 ny=np.int64(case["ny"]), n=np.int64(n), in_checksum=np.float64(checksum([x, y, t])),
                 ref_rows=rows.astype(np.int32), ref_threshold=np.float64(threshold))
        print(f"{case['name']}: threshold {float(threshold):.9g}, rows equal the float64 order: {same}, threshold difference {diff:.3g}, "
              f"rows in the band at rank n + 1: {band_count(D, order, n + 2, case['ny'])}")


if __name__ == "__main__":
    main()
