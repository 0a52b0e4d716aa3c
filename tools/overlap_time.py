#!/usr/bin/env python3
"""Time hint_amd.lens_iou_dice and hint_amd.plus_iou_dice (one launch of hint_overlap_run each) against the route a user would
write without the kernel,

  "torch": the same pair formula as batched torch on the same device - every curve edge against every template edge in
           [chunk, P, M] tensors (the common x-interval, the four heights, the split at the crossing, the signed sum), in chunks
           of rows that keep one such tensor under 256 MiB; the plus's vertices by broadcasting

alternating the routes in one process, and hint_amd.lens_shape_scores / hint_amd.plus_shape_scores end to end (the fit, IoU /
DICE, the dense trace and the Hausdorff distances: the body of the reference's evaluation loop).

    python tools/overlap_time.py [--out profiles/overlap_time.json] [--commit <hash>]

Shapes: P = 100 curve points (K = 5 for the lens rows, K = 25 for the plus rows), a prototype of M = 130 points, the plus's 12
vertices, at N = 1000 and 2^16 rows.  Every size runs in a child process of its own under a time limit, and a size that fails
ends the run: nothing more is started on the device after it.  The routes are warmed up, every repetition is bracketed by HIP
events on the current stream, and the medians, quartiles and extremes are printed and written, with the library's build string
and the commit.
"""
import math
import os
import sys

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1000, 20, 5), (1 << 16, 5, 2))          # (rows, repetitions of the overlap routes, of the end-to-end scores)
K_LENS, K_PLUS, P, M = 5, 25, 100, 130
CHUNK_BYTES = 256 << 20
LIMIT_S = 420           # per size


def one_size(n, reps, score_reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "overlap_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                                      # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=g, device=dev)                                   # noqa: E731

    # a prototype: the rim of the intersection of two unit-ish discs, M points, centred
    th = torch.linspace(-1.0, 1.0, M // 2 + 1, device=dev)[:-1]
    proto = torch.cat([torch.stack([1.5 * torch.cos(th) - 0.8, 1.5 * torch.sin(th)], 1),
                       torch.stack([0.8 - 1.5 * torch.cos(th), -1.5 * torch.sin(th)], 1)]).contiguous()
    proto = proto - proto.mean(0)

    def coeffs(points, k):
        """flat [n, 4 k] coefficients of closed polygons points [n, q, 2]: the discrete Fourier sums over m = -k/2 .. k/2"""
        q = points.shape[1]
        ms = torch.arange(-(k // 2), k // 2 + 1, device=dev)
        ang = -2 * math.pi * (ms[None, :] * torch.arange(q, device=dev)[:, None]).double() / q    # [q, k]
        re = torch.einsum("nqa,qk->nak", points.double(), ang.cos()) / q
        im = torch.einsum("nqa,qk->nak", points.double(), ang.sin()) / q
        return torch.cat([re.reshape(len(points), -1), im.reshape(len(points), -1)], 1).float().contiguous()

    def place(a, pr):
        cs, sn = pr[:, 3].cos()[:, None], pr[:, 3].sin()[:, None]
        qx, qy = a[None, :, 0] * cs - a[None, :, 1] * sn, a[None, :, 0] * sn + a[None, :, 1] * cs
        return torch.stack([qx * pr[:, 2:3] + pr[:, 0:1], qy * pr[:, 2:3] + pr[:, 1:2]], 2)

    # lens rows: the prototype placed at random and a little deformed, as coefficients; the parameters to score: near them
    true = torch.cat([0.3 * randn(n, 2), 0.8 + 1.2 * rnd(n, 1), math.pi * (2 * rnd(n, 1) - 1)], 1)
    x_lens = coeffs(place(proto, true), K_LENS)
    lens_params = (true + 0.05 * randn(n, 4)).contiguous()

    VX, VY = [0, 1, 1, 2, 2, 3, 3, 2, 2, 1, 1, 0], [0, 0, 1, 1, 0, 0, 2, 2, 3, 3, 2, 2]

    def plus_vertices(pc):
        xl, yl, xw, yw, xs, ys, xo, yo, ang = pc.unbind(1)
        xleft, xright, xtop, xbottom = xs - xl / 2, xs + xl / 2, xw / 2, -xw / 2
        yleft, yright, ybottom, ytop = -yw / 2, yw / 2, ys - yl / 2, ys + yl / 2
        xleft, xright = torch.minimum(xleft, yleft - 0.01), torch.maximum(xright, yright + 0.01)
        ytop, ybottom = torch.maximum(ytop, xtop + 0.01), torch.minimum(ybottom, xbottom - 0.01)
        cx, cy = torch.stack([xleft, yleft, yright, xright], 1), torch.stack([xtop, ytop, xbottom, ybottom], 1)
        V = torch.stack([cx[:, VX], cy[:, VY]], 2)                                                # [c, 12, 2]
        cs, sn = ang.cos()[:, None], ang.sin()[:, None]
        return torch.stack([V[..., 0] * cs - V[..., 1] * sn + xo[:, None], V[..., 0] * sn + V[..., 1] * cs + yo[:, None]], 2)

    # plus rows: plausible shapes, 20 points an edge, as coefficients; the parameters to score: near them
    shape = torch.cat([3 + 3 * rnd(n, 2), 0.4 + 1.8 * rnd(n, 2), 3 * rnd(n, 2) - 1.5, 0.5 * randn(n, 2), math.pi * (2 * rnd(n, 1) - 1)], 1)
    W = plus_vertices(shape)
    t = (torch.arange(20, device=dev) / 20.0)[None, None, :, None]
    outline = (W[:, :, None, :] + t * (W.roll(-1, 1) - W)[:, :, None, :]).reshape(n, 240, 2)
    x_plus = coeffs(outline, K_PLUS)
    plus_params = (shape + 0.05 * randn(n, 9)).contiguous()

    m = {k: torch.arange(k, device=dev) - k // 2 for k in (K_LENS, K_PLUS)}

    def torch_points(xc, k):
        c = xc.shape[0]
        ang = 2 * math.pi * (m[k][None, :] * torch.arange(P, device=dev)[:, None]).double() / (P - 1)
        re, im = xc[:, :2 * k].reshape(c, 2, k), xc[:, 2 * k:].reshape(c, 2, k)
        return torch.einsum("nak,tk->nta", re, ang.cos().float()) - torch.einsum("nak,tk->nta", im, ang.sin().float())

    def height(x0, h0, x1, h1, q):
        return h0 + ((q - x0) / (x1 - x0)).clamp(0, 1) * (h1 - h0)

    def torch_overlap(C, T):
        """(iou, dice) of curves C [c, P, 2] and templates T [c, M, 2] by the pair formula, [c, P, M] tensors"""
        y0 = torch.minimum(C[..., 1].amin(1), T[..., 1].amin(1))[:, None]
        C1, T1 = C.roll(-1, 1), T.roll(-1, 1)
        ex0, eh0, ex1, eh1 = (v[:, :, None] for v in (C[..., 0], C[..., 1] - y0, C1[..., 0], C1[..., 1] - y0))
        fx0, fh0, fx1, fh1 = (v[:, None, :] for v in (T[..., 0], T[..., 1] - y0, T1[..., 0], T1[..., 1] - y0))
        a = torch.maximum(torch.minimum(ex0, ex1), torch.minimum(fx0, fx1))
        b = torch.minimum(torch.maximum(ex0, ex1), torch.maximum(fx0, fx1))
        live = a < b
        ea, eb = height(ex0, eh0, ex1, eh1, a), height(ex0, eh0, ex1, eh1, b)
        fa, fb = height(fx0, fh0, fx1, fh1, a), height(fx0, fh0, fx1, fh1, b)
        da, db = ea - fa, eb - fb
        ma, mb = torch.minimum(ea, fa), torch.minimum(eb, fb)
        tau = (da / (da - db)).nan_to_num(0.0)
        split = ea + tau * (eb - ea) + tau * ma + (1 - tau) * mb
        total = torch.where(da * db < 0, split, ma + mb)
        sign = torch.where((ex1 < ex0) != (fx1 < fx0), -1.0, 1.0)
        inter = torch.where(live, sign * 0.5 * (b - a) * total, 0.0).double().sum((1, 2)).abs()
        ac = (0.5 * (C1[..., 0] - C[..., 0]) * (C[..., 1] + C1[..., 1] - 2 * y0)).double().sum(1).abs()
        at = (0.5 * (T1[..., 0] - T[..., 0]) * (T[..., 1] + T1[..., 1] - 2 * y0)).double().sum(1).abs()
        inter = torch.minimum(inter, torch.minimum(ac, at))
        return (inter / (ac + at - inter)).float(), (2 * inter / (ac + at)).float()

    def chunked(xc, k, template_of, m_pts):
        chunk = max(1, CHUNK_BYTES // (4 * P * m_pts))
        iou, dice = torch.empty(n, device=dev), torch.empty(n, device=dev)
        for a in range(0, n, chunk):
            iou[a:a + chunk], dice[a:a + chunk] = torch_overlap(torch_points(xc[a:a + chunk], k), template_of(slice(a, a + chunk)))
        return iou, dice

    routes = {"fused_lens": lambda: hint_amd.lens_iou_dice(x_lens, proto, lens_params),
              "torch_lens": lambda: chunked(x_lens, K_LENS, lambda s: place(proto, lens_params[s]), M),
              "fused_plus": lambda: hint_amd.plus_iou_dice(x_plus, plus_params),
              "torch_plus": lambda: chunked(x_plus, K_PLUS, lambda s: plus_vertices(plus_params[s]), 12)}
    us, outs = alternate(routes, reps, warmup)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    for name in ("lens", "plus"):
        f, t_ = outs[f"fused_{name}"], outs[f"torch_{name}"]
        simple = f[2] == 0
        row[f"rows_simple_{name}"] = int(simple.sum())
        row[f"mean_iou_{name}"] = float(f[0][simple].double().mean())
        row[f"max_abs_difference_iou_{name}"] = float((f[0] - t_[0])[simple].abs().max())
        row[f"torch_over_fused_{name}"] = row[f"torch_{name}"]["median_us"] / row[f"fused_{name}"]["median_us"]
    row["fused_pairs_per_second_lens"] = float(n) * P * M / (row["fused_lens"]["median_us"] * 1e-6)
    row["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    # the evaluation loop's body, end to end
    hint_amd.lens_shape_scores(x_lens[:64], proto), hint_amd.plus_shape_scores(x_plus[:64])       # (loads the kernels)
    torch.cuda.synchronize()
    sc = {"scores_lens": [], "scores_plus": []}
    for _ in range(score_reps):
        dt, s_l = timed(lambda: hint_amd.lens_shape_scores(x_lens, proto))
        sc["scores_lens"].append(dt)
        dt, s_p = timed(lambda: hint_amd.plus_shape_scores(x_plus))
        sc["scores_plus"].append(dt)
    for name, s in (("lens", s_l), ("plus", s_p)):
        row[f"scores_{name}"] = stats(sc[f"scores_{name}"])
        row[f"scores_{name}_mean_iou"] = float(s.iou.double().nanmean())
        row[f"scores_{name}_mean_max_h"] = float(s.max_h.double().nanmean())
        row[f"scores_{name}_rows_crossing"] = int((s.crossings > 0).sum())
    row["workgroups"] = int(lib.hint_overlap_geometry(n, P, M, 0))
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused_lens", "torch_lens", "fused_plus", "torch_plus", "scores_lens", "scores_plus"), 12, 14)
    print(f"N={n} torch / fused: lens {row['torch_over_fused_lens']:.2f}, plus {row['torch_over_fused_plus']:.2f}; IoU differs from "
          f"torch's by at most {row['max_abs_difference_iou_lens']:.3g} (lens) and {row['max_abs_difference_iou_plus']:.3g} (plus) "
          f"on the {row['rows_simple_lens']} and {row['rows_simple_plus']} rows whose curve is simple; scores: mean IoU "
          f"{row['scores_lens_mean_iou']:.3f} (lens), {row['scores_plus_mean_iou']:.3f} (plus)")


def main():
    ap = parser("overlap_time.json", 3)
    ap.add_argument("--score-reps", type=int, default=1, help="(internal) repetitions of the end-to-end scores of --one")
    args = ap.parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.score_reps, args.warmup)
    res = {"n_points": P, "n_coeffs_lens": K_LENS, "n_coeffs_plus": K_PLUS, "prototype_points": M, "torch_chunk_bytes": CHUNK_BYTES,
           "commit": args.commit or commit_of_tree(), "shapes": {}}
    sizes = [(n, ("--reps", reps, "--score-reps", score_reps, "--warmup", args.warmup)) for n, reps, score_reps in SIZES]
    return drive(__file__, LIMIT_S, sizes, res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
