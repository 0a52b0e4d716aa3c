#!/usr/bin/env python3
"""Time hint_amd.hausdorff_distances on coefficients (one launch of hint_hausdorff_run) against the formulation a user would
otherwise write on the same device,

    points = einsum(re, cos) - einsum(im, sin);  lens = (prototype @ R) * scale + (x, y);  d = torch.cdist(lens, points)
    minima = cat(d.min(2), d.min(1));  max_h = minima.max(1);  avg_h = minima.mean(1)

chunked over rows so that the [chunk, M, P] matrix stays under 1 GiB, alternating the two in one process.

    python tools/hausdorff_time.py [--out profiles/hausdorff_time.json] [--commit <hash>]

Shapes: K = 5, P = 1000, M = 1000 at N = 1000 (the evaluation loop's call) and 2^16 rows.  Every size runs in a child process of
its own under a time limit, and a size that fails ends the run: nothing more is started on the device after it.  Both routes are
warmed up, every repetition is bracketed by HIP events on the current stream, and the medians, quartiles and extremes are
printed and written, with the library's build string and the commit.
"""
import math
import os
import sys

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1000, 20), (1 << 16, 5))          # (rows, repetitions)
K, P, M = 5, 1000, 1000
CHUNK = 256             # rows of the torch formulation's [chunk, M, P] matrix: 1.02 GB in fp32, just under 1 GiB
LIMIT_S = 300           # per size


def one_size(n, reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "hausdorff_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    w = torch.tensor([.1, .3, 1, .6, .2], device=dev).repeat(4)
    x = torch.randn(n, 4 * K, generator=g, device=dev) * w
    # a two-arc lens of M points, and params around the identity
    th = torch.linspace(0.0, 2 * math.pi, M + 1, device=dev)[:M]
    proto = torch.stack([torch.cos(th), 0.4 * torch.sin(th) * torch.sin(th).abs()], 1).contiguous()
    params = torch.cat([0.3 * torch.randn(n, 2, generator=g, device=dev), 0.5 + 2 * torch.rand(n, 1, generator=g, device=dev),
                        math.pi * (2 * torch.rand(n, 1, generator=g, device=dev) - 1)], 1).contiguous()
    m = torch.arange(K, device=dev) - K // 2
    ang = 2 * math.pi * (m[None, :] * torch.arange(P, device=dev)[:, None]).double() / (P - 1)
    cos, sin = ang.cos().float(), ang.sin().float()

    def torch_route():
        max_h, avg_h = torch.empty(n, device=dev), torch.empty(n, device=dev)
        for a in range(0, n, CHUNK):
            xc, pc = x[a:a + CHUNK], params[a:a + CHUNK]
            c = xc.shape[0]
            re, im = xc[:, :2 * K].reshape(c, 2, K), xc[:, 2 * K:].reshape(c, 2, K)
            pts = torch.einsum("nak,tk->nta", re, cos) - torch.einsum("nak,tk->nta", im, sin)
            cs, sn = pc[:, 3].cos(), pc[:, 3].sin()
            R = torch.stack([torch.stack([cs, sn], 1), torch.stack([-sn, cs], 1)], 1)             # [c, 2, 2]
            lens = torch.matmul(proto[None], R) * pc[:, 2, None, None] + pc[:, None, :2]
            d = torch.cdist(lens, pts)                                                            # [c, M, P]
            minima = torch.cat([d.min(2).values, d.min(1).values], 1)
            max_h[a:a + c], avg_h[a:a + c] = minima.max(1).values, minima.mean(1)
        return max_h, avg_h

    routes = {"fused": lambda: hint_amd.hausdorff_distances(x, proto, params, n_points=P), "torch": torch_route}

    us, outs = alternate(routes, reps, warmup)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    row["max_abs_difference_max_h"] = float((outs["fused"][0] - outs["torch"][0]).abs().max())
    row["max_abs_difference_avg_h"] = float((outs["fused"][1] - outs["torch"][1]).abs().max())
    row["workgroups"] = int(lib.hint_hausdorff_geometry(n, P, M, 0))
    row["fused_pairs_per_second"] = 2.0 * n * P * M / (row["fused"]["median_us"] * 1e-6)      # each pair is met in both passes
    row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
    row["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused", "torch"))
    print(f"N={n} torch / fused = {row['torch_over_fused']:.2f}; fused {row['fused_pairs_per_second'] / 1e12:.3f} T pair visits/s on "
          f"{row['workgroups']} workgroups; max_h differs from torch's by at most {row['max_abs_difference_max_h']:.3g}, avg_h by "
          f"{row['max_abs_difference_avg_h']:.3g}")


def main():
    args = parser("hausdorff_time.json", 3).parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.warmup)
    res = {"n_coeffs": K, "n_points": P, "template_points": M, "torch_chunk_rows": CHUNK, "commit": args.commit or commit_of_tree(), "shapes": {}}
    return drive(__file__, LIMIT_S, [(n, ("--reps", reps, "--warmup", args.warmup)) for n, reps in SIZES], res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
