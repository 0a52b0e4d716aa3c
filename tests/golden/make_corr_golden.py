#!/usr/bin/env python3
"""Generate tests/golden/corr_*.npz: the reference's correlation MSE (run_experiments.py:212-221) on seeded inputs.

    python tests/golden/make_corr_golden.py

What the reference computes there is three numpy calls, so no checkout of it is needed: a fixture holds the case's seed, the
checksum of the inputs regenerated from it (tests/corr_oracle.py golden_inputs: a sample x and a second, ground-truth sample),
and numpy's OUTPUTS on them - corr = np.corrcoef(x.T), corr_true = np.corrcoef(second sample.T) (correlation_conditional,
rejection_sampling.py:130) and mse = np.nanmean(np.square(corr - corr_true)).  n4000_d20 is the conditional lens model's shape.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from corr_oracle import GOLDEN_CASES, checksum, golden_inputs  # noqa: E402


def main():
    for case in GOLDEN_CASES:
        x, y = golden_inputs(case)
        corr = np.corrcoef(x.astype(np.float64).T)
        corr_true = np.corrcoef(y.astype(np.float64).T)
        mse = np.nanmean(np.square(corr - corr_true))
        np.savez(os.path.join(HERE, f"corr_{case['name']}.npz"), seed=np.int64(case["seed"]), n=np.int64(case["n"]),
                 d=np.int64(case["d"]), in_checksum=np.float64(checksum([x, y])), corr=corr, corr_true=corr_true,
                 mse=np.float64(mse))
        print(f"{case['name']}: mse {mse:.9g}, max |corr - corr_true| {np.abs(corr - corr_true).max():.3g}")


if __name__ == "__main__":
    main()
