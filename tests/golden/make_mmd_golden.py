#!/usr/bin/env python3
"""Generate tests/golden/mmd_*.npz by running the REAL reference multi_mmd (rejection_sampling.py:56-73) on the CPU.

Runs at development time only, on a machine that has a checkout of the reference:

    python tests/golden/make_mmd_golden.py <directory of the reference checkout>

rejection_sampling.py imports the reference's `data` module (datasets, a simulator) and plotting / progress packages at the
top; none of them is touched by multi_mmd, so `data` and whichever of the others is not installed are empty stand-ins in
sys.modules.  multi_mmd calls `.cuda()` on its accumulators: torch.Tensor.cuda is the identity while it runs.  Nothing of
the reference is copied: a fixture holds the case's seed, the checksum of the inputs regenerated from it (tests/mmd_oracle.py
golden_inputs) and the reference's OUTPUT.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mmd_oracle import GOLDEN_CASES, checksum, golden_inputs, mmd_terms64  # noqa: E402


def import_reference(ref_dir):
    sys.modules["data"] = types.ModuleType("data")
    for name in ("matplotlib", "matplotlib.pyplot", "tqdm", "scipy", "scipy.spatial"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].__dict__.setdefault("tqdm", lambda it, *a, **k: it)
    sys.modules["scipy.spatial"].__dict__.setdefault("distance_matrix", None)
    sys.path.insert(0, ref_dir)
    import rejection_sampling
    return rejection_sampling


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "rejection_sampling.py")):
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for case in GOLDEN_CASES:
            x, y = golden_inputs(case)
            with torch.no_grad():
                got = float(ref.multi_mmd(torch.from_numpy(x), torch.from_numpy(y), widths_exponents=list(case["kernels"])))
            want = mmd_terms64(x, y, case["kernels"])[0]
            np.savez(os.path.join(HERE, f"mmd_{case['name']}.npz"), seed=np.int64(case["seed"]), n=np.int64(case["n"]),
                     d=np.int64(case["d"]), kernels=np.asarray(case["kernels"], dtype=np.float64),
                     in_checksum=np.float64(checksum([x, y])), ref_mmd=np.float32(got))
            print(f"{case['name']}: reference {got:.9g}, float64 {want:.9g}, difference {got - want:.3g}")
    finally:
        torch.Tensor.cuda = real_cuda


if __name__ == "__main__":
    main()
