"""Host cost of a call of the evaluation wrappers at a batch where the call is host-bound (64 rows): the wall time per call over
`--calls` back-to-back calls with one synchronise at the end (us_per_call) and the part of it the host needed to issue them
(enqueue_us_per_call: where it is well below the former, the call is bound by its kernels, not by the host), for
sample_lens_prior, sample_plus_prior, curve_features, hausdorff_distances (the curve given as points, a 16-point template),
multi_mmd (64 x 64, d = 4) and corrcoef (64 x 4).  Prints one JSON line.  For an A/B of two checkouts, run this file of each of
them in turn, several times (NOTES.md has such a table)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rows", type=int, default=64)
    args = ap.parse_args()
    import torch
    import hint_amd
    from hint_amd import _lib
    dev = torch.device("cuda:0")
    n = args.rows
    g = torch.Generator(device=dev).manual_seed(1)
    x = hint_amd.sample_lens_prior(n, 3, device=dev)
    pts = torch.randn(n, 100, 2, device=dev, generator=g)
    template = torch.randn(16, 2, device=dev, generator=g)
    a, b, c = (torch.randn(n, 4, device=dev, generator=g) for _ in range(3))
    ops = {
        "sample_lens_prior": lambda: hint_amd.sample_lens_prior(n, 3, device=dev),
        "sample_plus_prior": lambda: hint_amd.sample_plus_prior(n, 3, device=dev),
        "curve_features": lambda: hint_amd.curve_features(x),
        "hausdorff_distances": lambda: hint_amd.hausdorff_distances(pts, template),
        "multi_mmd": lambda: hint_amd.multi_mmd(a, b),
        "corrcoef": lambda: hint_amd.corrcoef(c),
    }
    row = {"rows": n, "calls": args.calls, "tree": ROOT, "build": _lib.load().hint_build_info().decode(), "us_per_call": {},
           "enqueue_us_per_call": {}}
    for name, fn in ops.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        row["us_per_call"][name] = round((time.perf_counter() - t0) / args.calls * 1e6, 3)
        row["enqueue_us_per_call"][name] = round((t1 - t0) / args.calls * 1e6, 3)
    print(json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
