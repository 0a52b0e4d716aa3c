#!/usr/bin/env python3
"""Generate tests/golden/pointset_bits.npz: the output bits of hint_hausdorff_run and hint_plus_run on the cases of
tests/pointset_cases.py, as the library that is built in the tree computes them on an MI355X.

Runs at development time only, on a machine with the GPU, at a commit whose bits are the ones to keep:

    python tests/golden/make_pointset_bits.py [output file]

The fixture was recorded at the last commit at which hint_hausdorff.hip and hint_plus.hip each held their own copy of the walk,
the trace, the tile loop and the reductions; tests/test_gpu_pointset_bits.py holds every later build to it.  Re-record only for a
change that is meant to move bits (a change of the contract in include/hint_amd.h), never to make that test pass.  A fixture holds
data only: per case a sha256 of each input array, max_dist, and the outputs (`points` and `segments` as a sha256).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import pointset_cases as pc  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pointset_bits.npz")
    from hint_amd import _lib
    rec = {"build": np.array(_lib.load().hint_build_info().decode())}
    for name in list(pc.HAUSDORFF) + list(pc.PLUS):
        inp = pc.inputs(name)
        if name in pc.PLUS:
            pc.check_plus_rows(name, inp)                    # before anything is recorded
        out = pc.run(name, inp)
        rec.update(pc.record(name, inp, out))
        print(name, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, "max_dist", inp.get("max_dist"))
    np.savez_compressed(path, **rec)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(rec)} arrays; {rec['build']}")


if __name__ == "__main__":
    main()
