#!/usr/bin/env python3
"""Time hint_amd.target_distances (one launch of hint_curve_run) against the formulation a user would otherwise write on the
same device,

    points = einsum(re, cos) - einsum(im, sin);  d = torch.cdist(points, points);  argmax over [chunk, P, P];  two gathers

chunked over rows so that the [chunk, P, P] matrix fits, alternating the two in one process.

    python tools/curve_time.py [--out profiles/curve_time.json] [--commit <hash>]

Shapes: K = 5, P = 100 at N = 4000 (the evaluation loop's call), 2^20 and 2^24 rows.  Every size runs in a child process of its
own under a time limit, and a size that fails ends the run: nothing more is started on the device after it.  Both routes are
warmed up, every repetition is bracketed by HIP events on the current stream, and the medians, quartiles and extremes are
printed and written, with the library's build string and the commit.
"""
import math
import os
import sys

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((4000, 30), (1 << 20, 10), (1 << 24, 3))          # (rows, repetitions)
K, P = 5, 100
CHUNK = 1 << 16         # rows of the torch formulation's [chunk, P, P] matrix: 2.6 GB in fp32
LIMIT_S = 300           # per size


def one_size(n, reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "curve_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    w = torch.tensor([.1, .3, 1, .6, .2], device=dev).repeat(4)
    x = torch.randn(n, 4 * K, generator=g, device=dev) * w
    t = torch.tensor([0.5, -1.0], device=dev)
    m = torch.arange(K, device=dev) - K // 2
    ang = 2 * math.pi * (m[None, :] * torch.arange(P, device=dev)[:, None]).double() / (P - 1)
    cos, sin = ang.cos().float(), ang.sin().float()

    def torch_route():
        out = torch.empty(n, device=dev)
        for a in range(0, n, CHUNK):
            xc = x[a:a + CHUNK]
            c = xc.shape[0]
            re, im = xc[:, :2 * K].reshape(c, 2, K), xc[:, 2 * K:].reshape(c, 2, K)
            pts = torch.einsum("nak,tk->nta", re, cos) - torch.einsum("nak,tk->nta", im, sin)
            best = torch.cdist(pts, pts).reshape(c, P * P).argmax(1)
            i, j = best // P, best % P
            rows = torch.arange(c, device=dev)
            diff = pts[rows, j] - pts[rows, i]
            out[a:a + c] = ((diff.flip(1) - t) ** 2).sum(1).sqrt()
        return out

    routes = {"fused": lambda: hint_amd.target_distances(x, t, 0.0), "torch": torch_route}

    us, outs = alternate(routes, reps, warmup)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    # the two choose the same pair except where the maximum is nearly tied (cdist's rounding is its own)
    row["rows_within_1e-4_of_torch"] = int(((outs["fused"] - outs["torch"]).abs() <= 1e-4).sum())
    row["workgroups"], row["rows_per_tile"], row["rows_per_wavefront"] = (int(lib.hint_curve_geometry(n, K, P, f)) for f in range(3))
    row["fused_rows_per_second"] = n / (row["fused"]["median_us"] * 1e-6)
    row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused", "torch"))
    print(f"N={n} torch / fused = {row['torch_over_fused']:.2f}; fused {row['fused_rows_per_second'] / 1e9:.3f} G rows/s on "
          f"{row['workgroups']} workgroups; {row['rows_within_1e-4_of_torch']} of {n} distances within 1e-4 of torch's")


def main():
    args = parser("curve_time.json", 3).parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.warmup)
    res = {"n_coeffs": K, "n_points": P, "torch_chunk_rows": CHUNK, "commit": args.commit or commit_of_tree(), "shapes": {}}
    return drive(__file__, LIMIT_S, [(n, ("--reps", reps, "--warmup", args.warmup)) for n, reps in SIZES], res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
