#!/usr/bin/env python3
"""Extend tests/golden/pointset_bits.npz and tests/golden/plusfit_bits.npz: the output bits of hint_hausdorff_run, hint_plus_run,
hint_lensfit_run and hint_plusfit_run on the cases of tests/pointset_cases.py, as the library that is built in the tree (or the
one HINT_AMD_LIB names) computes them on an MI355X.

Runs at development time only, on a machine with the GPU, with a library whose bits are the ones to keep:

    python tests/golden/make_pointset_bits.py [output directory]

A case goes to the file of its name's prefix: hd_*, pl_* and lf_* to pointset_bits.npz, pf_* to plusfit_bits.npz (the first file
is near the 64 KiB its test allows).  Per file, only the cases it does not hold yet are run and recorded; every array it holds is
carried over as it is, and the script refuses to write a file in which one of them differs.  The hd_* and pl_* cases were recorded
at the last commit at which hint_hausdorff.hip and hint_plus.hip each held their own copy of the walk, the trace, the tile loop
and the reductions (`build`); the lf_* cases at the last commit at which hint_lensfit.hip held its own placement and arg-min walk
(`build/lensfit`); the pf_* cases at the last commit at which hint_lensfit.hip and hint_plusfit.hip each held their own fit
driver - the state, the trace record, the update rule, the selection - before hint_fit.hpp (`build/plusfit`).
tests/test_gpu_pointset_bits.py holds every later build to them.  Re-record only for a change that is meant to move bits (a change
of the contract in include/hint_amd.h), never to make that test pass.  A fixture holds data only: per case a sha256 of each input
array, max_dist, and the outputs (`points` and `segments` as a sha256).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import pointset_cases as pc  # noqa: E402

# by a case name's prefix: the fixture's file, and the key its build string is kept under
FIXTURE = {"hd": "pointset_bits.npz", "pl": "pointset_bits.npz", "lf": "pointset_bits.npz", "pf": "plusfit_bits.npz"}
BUILD_KEY = {"hd": "build", "pl": "build", "lf": "build/lensfit", "pf": "build/plusfit"}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_plusfit_output(name, inp, out, n_run):
    """every word of a start that ran is finite (a NaN would pin nothing about the arithmetic), and the starts ran that the CPU
    says run"""
    assert "n_run" not in out or np.array_equal(out["n_run"], n_run), (name, out["n_run"], n_run)
    ran = np.arange(inp["starts"].shape[1])[None, :] < n_run[:, None]
    for k, v in out.items():
        fin = np.isfinite(v)
        assert fin[ran].all() if k in ("all_params", "all_loss", "grad", "trace") else fin.all(), (name, k)


def extend(fixture, names, out_dir, build):
    src = os.path.join(HERE, fixture)
    old = {}
    if os.path.exists(src):
        with np.load(src) as f:
            old = {k: f[k] for k in f.files}
    held = {k.split("/")[0] for k in old}
    rec = dict(old)
    for name in names:
        if name in held:
            continue
        inp = pc.inputs(name)
        if name in pc.PLUS:
            pc.check_plus_rows(name, inp)                    # before anything is recorded
        n_run = pc.check_plusfit_rows(name, inp) if name in pc.PLUSFIT else None
        out = pc.run(name, inp)
        if name in pc.LENSFIT:                               # a NaN would pin nothing about the arithmetic
            assert all(np.isfinite(v).all() for v in out.values()), (name, {k: int((~np.isfinite(v)).sum()) for k, v in out.items()})
        if name in pc.PLUSFIT:
            check_plusfit_output(name, inp, out, n_run)
        new = pc.record(name, inp, out)
        new[BUILD_KEY[name[:2]]] = build
        for k, v in new.items():
            assert k not in old or same(old[k], v), f"{k} is in the fixture already and would change"
        rec.update(new)
        print(name, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, "max_dist", inp.get("max_dist"))
    if len(rec) == len(old):
        return print(f"{fixture}: holds every case")
    path = os.path.join(out_dir, fixture)
    np.savez_compressed(path, **rec)
    with np.load(path) as f:
        assert set(old) <= set(f.files) and all(same(f[k], v) for k, v in old.items()), "an array of the fixture changed"
        print(f"{path}: {os.path.getsize(path)} bytes, {len(f.files)} arrays ({len(old)} carried over)")


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    from hint_amd import _lib
    build = np.array(_lib.load().hint_build_info().decode())
    names = list(pc.HAUSDORFF) + list(pc.PLUS) + list(pc.LENSFIT) + list(pc.PLUSFIT)
    for fixture in sorted(set(FIXTURE.values())):
        extend(fixture, [n for n in names if FIXTURE[n[:2]] == fixture], out_dir, build)


if __name__ == "__main__":
    main()
