#!/usr/bin/env python3
"""Time hint_amd.fit_plus_shapes on coefficients (plus_fit_starts from a given angle and one launch of hint_plusfit_run) against
the formulation a user would otherwise write on the same device: the same schedule as batched torch autograd,

    W = vertices(params) @ R + offsets                                    [c, 12, 2], from params [c, 9] that require grad
    d = squared distance of every point to every kept segment             [c, 12, P]
    loss = d.min(1).values.mean(1) + w_i * (corner distances).min(2).values.mean(1);  loss.sum().backward()
    buf = g (first step) or momentum * buf + g;  params -= lr_i * buf;  lr_i *= gamma;  w_i = 1 - i / 400

400 steps from each of the nine starts in turn, a start run for the rows that have not stopped yet (loss < stop_loss ends a row),
alternating the two routes in one process.  (No width is zero on these rows, so all twelve segments are kept throughout.)

    python tools/plusfit_time.py [--out profiles/plusfit_time.json] [--commit <hash>]

Shapes: K = 25, P = 100, 9 starts x 400 steps at N = 1000 and 2^16 rows, each with stop_loss = 0.005 (the reference's) and with
stop_loss = 0 (every start runs).  The angle is given (0 for every row: the rows are drawn axis-parallel, so that the tool times the
fit and not the angle search).  Every size runs in a child process of its own under a time limit, and a size that fails ends the
run: nothing more is started on the device after it.  Both routes are warmed up, every repetition is bracketed by HIP events on the
current stream, and the medians, quartiles and extremes are printed and written, with the library's build string and the commit.
The reference's own host loop is not timed here (DESIGN section 17 quotes it from a CPU run).
"""
import math
import os
import sys

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1000, 3), (1 << 16, 2))           # (rows, repetitions)
K, P, STARTS, STEPS = 25, 100, 9, 400
LR, ANGLE_LR, MOMENTUM, GAMMA, STOP = 0.1, 0.01, 0.2, 0.1 ** (1 / 400), 0.005
LIMIT_S = 420           # per size
VX = (0, 1, 1, 2, 2, 3, 3, 2, 2, 1, 1, 0)   # of (xleft, yleft, yright, xright)
VY = (0, 0, 1, 1, 0, 0, 2, 2, 3, 3, 2, 2)   # of (xtop, ytop, xbottom, ybottom)


def vertices(p):
    """local vertices [c, 12, 2] of params p [c, 9], as plus_segments_from_params forms them"""
    import torch
    xl, yl, xw, yw, xs, ys = (p[:, i] for i in range(6))
    xtop, xbottom, yright, yleft = xw / 2, -xw / 2, yw / 2, -yw / 2
    xleft, xright = torch.minimum(xs - xl / 2, yleft - 0.01), torch.maximum(xs + xl / 2, yright + 0.01)
    ytop, ybottom = torch.maximum(ys + yl / 2, xtop + 0.01), torch.minimum(ys - yl / 2, xbottom - 0.01)
    cx, cy = torch.stack([xleft, yleft, yright, xright], 1), torch.stack([xtop, ytop, xbottom, ybottom], 1)
    return torch.stack([cx[:, list(VX)], cy[:, list(VY)]], 2)


def plus_loss(p, b, w):
    """points_to_plus_loss for every row: p [c, 9], b [c, P, 2] -> [c]"""
    import torch
    V = vertices(p)
    cs, sn = p[:, 8].cos(), p[:, 8].sin()
    R = torch.stack([torch.stack([cs, sn], 1), torch.stack([-sn, cs], 1)], 1)              # [c, 2, 2]
    W = torch.matmul(V, R) + p[:, None, 6:8]
    n = torch.roll(W, -1, 1) - W
    L = (n * n).sum(2).sqrt()
    n = n / L[:, :, None]
    ap = W[:, :, None, :] - b[:, None, :, :]                                                # [c, 12, P, 2]
    ln = torch.maximum(torch.zeros_like(L)[:, :, None], torch.minimum(L[:, :, None], -(ap * n[:, :, None, :]).sum(3)))
    v = ap + ln[..., None] * n[:, :, None, :]
    seg = (v * v).sum(3).min(1).values.mean(1)
    corner = (ap * ap).sum(3).min(2).values.mean(1)
    return seg + w * corner


def torch_fit(b, starts, stop_loss, steps=STEPS):
    """the reference's fit, batched: b [n, P, 2], starts [n, S, 9] -> (params [n, 9], loss [n])"""
    import torch
    n, dev = b.shape[0], b.device
    rates = torch.tensor([LR] * 8 + [ANGLE_LR], device=dev)
    params, loss = starts[:, 0].clone(), torch.full((n,), float("inf"), device=dev)
    active = torch.arange(n, device=dev)
    for s in range(starts.shape[1]):
        if active.numel() == 0:
            break
        bb = b[active]
        p = starts[active, s].clone().requires_grad_(True)
        buf, decay, last = None, 1.0, None
        for i in range(steps):
            last = plus_loss(p, bb, 1.0 - i / steps)
            (grad,) = torch.autograd.grad(last.sum(), p)
            with torch.no_grad():
                buf = grad if buf is None else MOMENTUM * buf + grad
                p -= rates * decay * buf
            decay *= GAMMA
        with torch.no_grad():
            last = last.detach()
            better = last < loss[active]
            rows = active[better]
            params[rows], loss[rows] = p.detach()[better], last[better]
            if stop_loss > 0:
                active = active[~(last < stop_loss)]
    return params, loss


def plus_rows(n, dev, g):
    """plus-like coefficient rows [n, 4 K]: axis-parallel pluses of random arms, 60 points an edge, as Fourier coefficients"""
    import torch
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, device=dev)        # noqa: E731
    p = torch.stack([u(3, 6), u(3, 6), u(0.4, 2.2), u(0.4, 2.2), u(-1.0, 1.0), u(-1.0, 1.0),
                     0.5 * torch.randn(n, generator=g, device=dev), 0.5 * torch.randn(n, generator=g, device=dev),
                     torch.zeros(n, device=dev)], 1)
    W = vertices(p) + p[:, None, 6:8]
    t = torch.arange(60, device=dev) / 60.0
    pts = (W[:, :, None, :] + t[None, None, :, None] * (torch.roll(W, -1, 1) - W)[:, :, None, :]).reshape(n, 720, 2)
    m = torch.arange(K, device=dev) - K // 2
    ph = -2 * math.pi * (m[None, :] * torch.arange(720, device=dev)[:, None]).double() / 720
    re = torch.einsum("nta,tk->nak", pts.double(), ph.cos()) / 720
    im = torch.einsum("nta,tk->nak", pts.double(), ph.sin()) / 720
    return torch.cat([re.reshape(n, -1), im.reshape(n, -1)], 1).float().contiguous()


def one_size(n, reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "plusfit_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    x = plus_rows(n, dev, g)
    angle = torch.zeros(n, device=dev)

    def fused(stop):
        return lambda: hint_amd.fit_plus_shapes(x, angle=angle, stop_loss=stop)

    def torch_route(stop):
        return lambda: torch_fit(hint_amd.trace_fourier_curves(x, P), hint_amd.plus_fit_starts(x, angle), stop)

    routes = {"fused": fused(STOP), "torch": torch_route(STOP), "fused_all": fused(0.0), "torch_all": torch_route(0.0)}
    us, outs = alternate(routes, reps, warmup)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    _, _, extra = hint_amd.fit_plus_shapes(x, angle=angle, stop_loss=STOP, return_all=True)
    row["mean_starts_run"] = float(extra["n_run"].float().mean())
    for tag in ("", "_all"):
        f, t = outs["fused" + tag], outs["torch" + tag]
        row["median_abs_difference_loss" + tag] = float((f[1] - t[1]).abs().median())
        row["max_abs_difference_loss" + tag] = float((f[1] - t[1]).abs().max())
        row["torch_over_fused" + tag] = row["torch" + tag]["median_us"] / row["fused" + tag]["median_us"]
        row["fused_us_per_row" + tag] = row["fused" + tag]["median_us"] / n
    row["median_loss"] = float(outs["fused"][1].median())
    row["workgroups"] = int(lib.hint_plusfit_geometry(n, P, 0))
    row["fused_all_us_per_step"] = row["fused_all"]["median_us"] * row["workgroups"] / (n * STARTS * STEPS)
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused", "torch", "fused_all", "torch_all"), width=9)
    print(f"N={n} torch / fused = {row['torch_over_fused']:.2f} with stop_loss {STOP} ({row['mean_starts_run']:.2f} starts a row), "
          f"{row['torch_over_fused_all']:.2f} with every start run; fused {row['fused_us_per_row']:.2f} / "
          f"{row['fused_us_per_row_all']:.2f} us a row on {row['workgroups']} workgroups, {row['fused_all_us_per_step']:.2f} us a "
          f"step of a workgroup; the loss differs from torch's by {row['median_abs_difference_loss']:.3g} in the median, "
          f"{row['max_abs_difference_loss']:.3g} at most (median loss {row['median_loss']:.3g})")


def main():
    args = parser("plusfit_time.json", 1).parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.warmup)
    res = {"n_coeffs": K, "n_points": P, "starts": STARTS, "steps": STEPS, "stop_loss": STOP,
           "commit": args.commit or commit_of_tree(), "shapes": {}}
    return drive(__file__, LIMIT_S, [(n, ("--reps", reps, "--warmup", args.warmup)) for n, reps in SIZES], res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
