#!/usr/bin/env python3
"""Time hint_amd.fit_lens_shapes on coefficients (lens_fit_starts and one launch of hint_lensfit_run) against the formulation a
user would otherwise write on the same device: the same schedule as batched torch autograd,

    lens = (prototype @ R) * scale + (x, y)                               [c, 2, M, 2], from params [c, 2, 4] that require grad
    d = ((lens[:, :, None] - points[:, None, :, None]) ** 2).sum(-1)      [c, 2, P, M]
    loss = d.min(3).values.mean(2) + d.min(2).values.mean(2);  loss.sum().backward()
    buf = g (first step) or momentum * buf + g;  params -= lr_i * buf;  lr_i *= gamma

100 steps from the same two starts, chunked over rows so that the [chunk, 2, P, M] tensor stays near 200 MB, alternating the two
in one process.

    python tools/lensfit_time.py [--out profiles/lensfit_time.json] [--commit <hash>]

Shapes: K = 5, P = 100, M = 130, 2 starts x 100 steps at N = 1000 (the evaluation loop's call) and 2^16 rows.  Every size runs in
a child process of its own under a time limit, and a size that fails ends the run: nothing more is started on the device after
it.  Both routes are warmed up, every repetition is bracketed by HIP events on the current stream, and the medians, quartiles and
extremes are printed and written, with the library's build string and the commit.  The reference's own host loop is not timed
here (DESIGN section 16 quotes it from a CPU run).
"""
import math
import os
import sys

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1000, 10), (1 << 16, 3))          # (rows, repetitions)
K, P, M, STARTS, STEPS = 5, 100, 130, 2, 100
LR, ANGLE_LR, MOMENTUM, GAMMA = 0.1, 0.01, 0.2, 0.1 ** (1 / 100)
CHUNK = 2048            # rows of the torch formulation's [chunk, 2, P, M] tensor: 213 MB in fp32
LIMIT_S = 420           # per size


def lens_rim(r0, r1, d, n0, n1, dev):
    """the rim of the intersection of the discs (0, 0), r0 and (d, 0), r1: n0 + n1 points, centred"""
    import torch
    xs = (d * d + r0 * r0 - r1 * r1) / (2 * d)
    ys = math.sqrt(r0 * r0 - xs * xs)
    t0, t1 = math.atan2(ys, xs), math.atan2(ys, d - xs)
    f0 = torch.linspace(-t0, t0, n0 + 1, device=dev)[:n0]
    f1 = torch.linspace(math.pi - t1, math.pi + t1, n1 + 1, device=dev)[:n1]
    pts = torch.cat([torch.stack([r0 * f0.cos(), r0 * f0.sin()], 1), torch.stack([d + r1 * f1.cos(), r1 * f1.sin()], 1)])
    return pts - pts.mean(0)


def one_size(n, reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "lensfit_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    proto = lens_rim(1.5, 3.0, 3.6, 47, M - 47, dev).contiguous()
    # lens-like rows: the prototype's own shape at a random size, angle and place, as Fourier coefficients of 128 rim points
    rim = lens_rim(1.5, 3.0, 3.6, 46, 82, dev)                                                    # [128, 2]
    size = (1.0 + torch.rand(n, 1, 1, generator=g, device=dev)) / 1.5
    ang = math.pi * (2 * torch.rand(n, generator=g, device=dev) - 1)
    R = torch.stack([torch.stack([ang.cos(), ang.sin()], 1), torch.stack([-ang.sin(), ang.cos()], 1)], 1)
    pts = torch.matmul(rim[None] * size, R) + 0.5 * torch.randn(n, 1, 2, generator=g, device=dev)
    m = torch.arange(K, device=dev) - K // 2
    ph = -2 * math.pi * (m[None, :] * torch.arange(128, device=dev)[:, None]).double() / 128      # [128, K]
    re = torch.einsum("nta,tk->nak", pts.double(), ph.cos()) / 128
    im = torch.einsum("nta,tk->nak", pts.double(), ph.sin()) / 128
    x = torch.cat([re.reshape(n, -1), im.reshape(n, -1)], 1).float().contiguous()
    rates = torch.tensor([LR, LR, LR, ANGLE_LR], device=dev)

    def torch_route():
        curves = hint_amd.trace_fourier_curves(x, P)
        starts = hint_amd.lens_fit_starts(x)
        params, loss = torch.empty(n, 4, device=dev), torch.empty(n, device=dev)
        for a in range(0, n, CHUNK):
            b = curves[a:a + CHUNK]
            p = starts[a:a + CHUNK].clone().requires_grad_(True)
            buf, decay, last = None, 1.0, None
            for i in range(STEPS):
                cs, sn = p[..., 3].cos(), p[..., 3].sin()
                Rm = torch.stack([torch.stack([cs, sn], -1), torch.stack([-sn, cs], -1)], -2)     # [c, 2, 2, 2]
                lens = torch.matmul(proto, Rm) * p[..., 2, None, None] + p[..., None, :2]         # [c, 2, M, 2]
                d = ((lens[:, :, None] - b[:, None, :, None]) ** 2).sum(-1)                       # [c, 2, P, M]
                last = d.min(3).values.mean(2) + d.min(2).values.mean(2)                          # [c, 2]
                (grad,) = torch.autograd.grad(last.sum(), p)
                with torch.no_grad():
                    buf = grad if buf is None else MOMENTUM * buf + grad
                    p -= rates * decay * buf
                decay *= GAMMA
            with torch.no_grad():
                best = last.argmin(1)
                rows = torch.arange(p.shape[0], device=dev)
                params[a:a + CHUNK], loss[a:a + CHUNK] = p[rows, best], last[rows, best]
        return params, loss

    routes = {"fused": lambda: hint_amd.fit_lens_shapes(x, proto), "torch": torch_route}

    peak = {}

    def fused_peak():
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        routes["fused"]()
        torch.cuda.synchronize()
        peak["fused"] = int(torch.cuda.max_memory_allocated() - base)

    us, outs = alternate(routes, reps, warmup, fused_peak)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    row["max_abs_difference_loss"] = float((outs["fused"][1] - outs["torch"][1]).abs().max())
    row["median_abs_difference_params"] = float((outs["fused"][0] - outs["torch"][0]).abs().median())
    row["median_loss"] = float(outs["fused"][1].median())
    row["workgroups"] = int(lib.hint_lensfit_geometry(n, P, 0))
    row["fused_pairs_per_second"] = 2.0 * n * STARTS * STEPS * P * M / (row["fused"]["median_us"] * 1e-6)
    row["fused_us_per_row"] = row["fused"]["median_us"] / n
    row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
    row["fused_peak_bytes_above_inputs"] = peak["fused"]
    row["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused", "torch"))
    print(f"N={n} torch / fused = {row['torch_over_fused']:.2f}; fused {row['fused_us_per_row']:.2f} us a row, "
          f"{row['fused_pairs_per_second'] / 1e12:.3f} T pair visits/s on {row['workgroups']} workgroups, "
          f"{row['fused_peak_bytes_above_inputs']} bytes allocated above its inputs (torch route: peak {row['torch_peak_bytes']}); "
          f"the loss differs from torch's by at most {row['max_abs_difference_loss']:.3g} (median loss {row['median_loss']:.3g})")


def main():
    args = parser("lensfit_time.json", 1).parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.warmup)
    res = {"n_coeffs": K, "n_points": P, "prototype_points": M, "starts": STARTS, "steps": STEPS, "torch_chunk_rows": CHUNK,
           "commit": args.commit or commit_of_tree(), "shapes": {}}
    return drive(__file__, LIMIT_S, [(n, ("--reps", reps, "--warmup", args.warmup)) for n, reps in SIZES], res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
