#!/usr/bin/env python3
"""Generate tests/golden/curve_*.npz by running the REAL reference simulator - LensShapeModel.forward_process (data.py:127-139)
and mean_target_distance (rejection_sampling.py:99-102) - on the CPU.

Runs at development time only, on a machine that has a checkout of the reference, scipy (pdist / squareform) and torch:

    python tests/golden/make_curve_golden.py <directory of the reference checkout>

data.py and rejection_sampling.py import dataset, geometry, plotting and progress packages at the top; the simulator touches
none of them, so whichever is not installed (shapely, for one) is an empty stand-in in sys.modules.  Nothing of the reference is
copied: a fixture holds data only - x (the unambiguous rows of tests/curve_oracle.py gauss(seed, draw, 5), cut to `rows`), the
reference's forward_process(x, noise=0.0) OUTPUT and, for the distance cases, the seed, y_target and the reference's
mean_target_distance value with numpy's global generator seeded by `seed` (so that the noise forward_process draws is
RandomState(seed).randn(rows, 2), which the tests regenerate).
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from curve_oracle import GOLDEN_CASES, features64, golden_draw  # noqa: E402


class _Anything(types.ModuleType):
    """a stand-in module: any attribute is another stand-in (enough for `from shapely import geometry as geo`)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything(self.__name__ + "." + name)


def import_reference(ref_dir):
    for name in ("pandas", "matplotlib", "matplotlib.pyplot", "shapely", "shapely.geometry", "shapely.ops", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Anything(name)
    if isinstance(sys.modules["tqdm"], _Anything):
        sys.modules["tqdm"].__dict__["tqdm"] = lambda it, *a, **k: it
    from scipy.spatial.distance import pdist, squareform  # noqa: F401  (the reference's distances: a stand-in would record nothing)
    sys.path.insert(0, ref_dir)
    import data
    import rejection_sampling
    return data, rejection_sampling


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "data.py")):
        sys.exit(__doc__)
    import torch
    data, ref = import_reference(sys.argv[1])
    model = data.LensShapeModel()
    for case in GOLDEN_CASES:
        draw, keep = golden_draw(case)
        x = draw[keep][:case["rows"]]
        assert x.shape == (case["rows"], 20), (case["name"], x.shape, int(keep.sum()))
        used = int(np.nonzero(keep)[0][case["rows"] - 1]) + 1
        y0 = model.forward_process(x, noise=0.0)
        out = dict(x=x, ref_y=y0.astype(np.float64))
        diff = float(np.abs(y0 - features64(x, 100)[0]).max())
        msg = f"{case['name']}: {used - case['rows']} ambiguous rows dropped among the first {used} of {case['draw']} drawn " \
              f"({int(keep.sum())} of {case['draw']} unambiguous), features differ from the float64 oracle by at most {diff:.3g}"
        if case["distance"]:
            y_target = (y0[case["rows"] // 2] + np.array([0.3, -0.2])).astype(np.float32)
            tt = torch.tensor(y_target[None, :]).expand(case["rows"], 2)           # as rejection_sampling.py:195 passes it
            np.random.seed(case["seed"])
            mean = ref.mean_target_distance(model, tt, torch.from_numpy(x))
            assert mean.dtype == torch.float32
            out.update(seed=np.int64(case["seed"]), y_target=y_target, ref_mean=np.float32(mean.item()))
            msg += f", mean_target_distance {mean.item():.9g}"
        np.savez(os.path.join(HERE, f"curve_{case['name']}.npz"), **out)
        print(msg)


if __name__ == "__main__":
    main()
