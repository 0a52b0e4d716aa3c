#!/usr/bin/env python3
"""Time hint_amd.plus_hausdorff_distances and hint_amd.plus_fit_loss on coefficients (one launch of hint_plus_run each) against
the two routes a user had before,

  (a) "ragged": the outline of every row densified on the host - data.py:176-186 restated, a Python loop over rows and edges with
      an np.linspace each - concatenated, uploaded and handed to hint_amd.hausdorff_distances as a ragged template; host time
      (the loop and the concatenation) and device time (upload and launch) are reported separately
  (b) "torch": a plain torch formulation on the same device - the segments by broadcasting, the outline padded to the longest
      edge of the chunk, torch.cdist in chunks of rows that keep the distance matrix under 1 GiB, masked minima and means; the
      loss as a broadcast point-to-segment distance

alternating the routes in one process.

    python tools/plus_time.py [--out profiles/plus_time.json] [--commit <hash>]

Shapes: K = 25, max_dist = 0.02, P = 1000 for the distances and P = 100 for the loss, at N = 1000 and 2^16 rows.  Every size runs
in a child process of its own under a time limit, and a size that fails ends the run: nothing more is started on the device after
it.  The device routes are warmed up, every repetition is bracketed by HIP events on the current stream, and the medians,
quartiles and extremes are printed and written, with the library's build string and the commit.
"""
import math
import os
import sys
import time

from _timing import alternate, commit_of_tree, drive, emit_row, parser, print_stats, stats, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1000, 20, 3), (1 << 16, 5, 1))          # (rows, repetitions of the device routes, of the host route)
K, P, P_FIT, MAX_DIST = 25, 1000, 100, 0.02
CHUNK = 64              # rows of the torch formulation's [chunk, 12 * longest edge, P] matrix: under 1 GiB in fp32
LIMIT_S = 420           # per size


def one_size(n, reps, host_reps, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "plus_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                                      # noqa: E731
    x = torch.randn(n, 4 * K, generator=g, device=dev) * 0.6
    # plausible fits: lengths 3..6, widths 0.4..2.2, shifts +-1.5, offsets N(0, 0.5), every angle
    params = torch.cat([3 + 3 * rnd(n, 2), 0.4 + 1.8 * rnd(n, 2), 3 * rnd(n, 2) - 1.5, 0.5 * torch.randn(n, 2, generator=g, device=dev),
                        math.pi * (2 * rnd(n, 1) - 1)], 1).contiguous()
    m = torch.arange(K, device=dev) - K // 2

    def twiddles(p):
        ang = 2 * math.pi * (m[None, :] * torch.arange(p, device=dev)[:, None]).double() / (p - 1)
        return ang.cos().float(), ang.sin().float()

    tw = {P: twiddles(P), P_FIT: twiddles(P_FIT)}
    VX, VY = [0, 1, 1, 2, 2, 3, 3, 2, 2, 1, 1, 0], [0, 0, 1, 1, 0, 0, 2, 2, 3, 3, 2, 2]

    def torch_points(xc, p):
        c = xc.shape[0]
        re, im = xc[:, :2 * K].reshape(c, 2, K), xc[:, 2 * K:].reshape(c, 2, K)
        return torch.einsum("nak,tk->nta", re, tw[p][0]) - torch.einsum("nak,tk->nta", im, tw[p][1])

    def torch_vertices(pc):
        xl, yl, xw, yw, xs, ys, xo, yo, ang = pc.unbind(1)
        xleft, xright, xtop, xbottom = xs - xl / 2, xs + xl / 2, xw / 2, -xw / 2
        yleft, yright, ybottom, ytop = -yw / 2, yw / 2, ys - yl / 2, ys + yl / 2
        xleft, xright = torch.minimum(xleft, yleft - 0.01), torch.maximum(xright, yright + 0.01)
        ytop, ybottom = torch.maximum(ytop, xtop + 0.01), torch.minimum(ybottom, xbottom - 0.01)
        cx, cy = torch.stack([xleft, yleft, yright, xright], 1), torch.stack([xtop, ytop, xbottom, ybottom], 1)
        V = torch.stack([cx[:, VX], cy[:, VY]], 2)                                                # [c, 12, 2]
        cs, sn = ang.cos()[:, None], ang.sin()[:, None]
        W = torch.stack([V[..., 0] * cs - V[..., 1] * sn + xo[:, None], V[..., 0] * sn + V[..., 1] * cs + yo[:, None]], 2)
        return W, (V != V.roll(-1, 1)).any(2)

    def torch_hausdorff():
        max_h, avg_h = torch.empty(n, device=dev), torch.empty(n, device=dev)
        for a in range(0, n, CHUNK):
            pts = torch_points(x[a:a + CHUNK], P)
            W, kept = torch_vertices(params[a:a + CHUNK])
            c = W.shape[0]
            W1 = W.roll(-1, 1)
            cnt = torch.where(kept, ((W1 - W).abs().amax(2).double() / MAX_DIST).round().clamp(min=1), 0.0)      # [c, 12]
            longest = int(cnt.max())
            i = torch.arange(longest, device=dev)[None, None, :]
            t = (i / (cnt[..., None] - 1).clamp(min=1)).float().clamp(max=1)
            valid = (i < cnt[..., None]).reshape(c, -1)
            out = (t[..., None] * W1[:, :, None, :] + (1 - t[..., None]) * W[:, :, None, :]).reshape(c, -1, 2)
            d = torch.cdist(out, pts)                                                             # [c, 12 longest, P]
            ma = d.min(2).values
            mb = torch.where(valid[..., None], d, torch.inf).min(1).values
            max_h[a:a + c] = torch.maximum(torch.where(valid, ma, 0.0).max(1).values, mb.max(1).values)
            avg_h[a:a + c] = (torch.where(valid, ma, 0.0).sum(1) + mb.sum(1)) / (valid.sum(1) + P)
        return max_h, avg_h

    def torch_loss():
        pts = torch_points(x, P_FIT)                                                              # [n, P, 2]
        W, kept = torch_vertices(params)
        nv = W.roll(-1, 1) - W
        L = nv.norm(dim=2)
        nv = nv / L[..., None]
        ap = W[:, :, None, :] - pts[:, None, :, :]                                                # [n, 12, P, 2]
        ln = torch.minimum(L[..., None], -(ap * nv[:, :, None, :]).sum(3)).clamp(min=0)
        d2 = ((ap + ln[..., None] * nv[:, :, None, :]) ** 2).sum(3)
        seg = torch.where(kept[..., None], d2, torch.inf).min(1).values.mean(1)
        cd = (ap ** 2).sum(3).min(2).values
        return seg + (cd * kept).sum(1) / kept.sum(1)

    def host_densify():
        """data.py:176-186 on the kept vertices of every row: (template [T, 2], offsets [n + 1])"""
        seg, keep = hint_amd.plus_segments(params)
        seg, keep = seg.cpu().numpy().astype(np.float64), keep.cpu().numpy()
        t0 = time.perf_counter()
        rows, offsets = [], np.zeros(n + 1, np.int64)
        for r in range(n):
            coords = seg[r, [s for s in range(12) if (keep[r] >> s) & 1], 0, :]
            dense = []
            for i in range(len(coords)):
                start, end = coords[(i + 1) % len(coords)], coords[i]
                cnt = max(1, int(round(np.max(np.abs(end - start)) / MAX_DIST)))
                dense.append(np.array([t * start + (1 - t) * end for t in np.linspace(0, 1, cnt)]))
            rows.append(np.concatenate(dense))
            offsets[r + 1] = offsets[r] + len(rows[-1])
        tpl = np.concatenate(rows).astype(np.float32)
        return tpl, offsets, (time.perf_counter() - t0) * 1e6

    routes = {"fused_hausdorff": lambda: hint_amd.plus_hausdorff_distances(x, params, max_dist=MAX_DIST, n_points=P),
              "torch_hausdorff": torch_hausdorff,
              "fused_loss": lambda: hint_amd.plus_fit_loss(x, params), "torch_loss": torch_loss}
    us, outs = alternate(routes, reps, warmup)
    # the ragged route: the host loop, then upload and launch
    host_us, dev_us = [], []
    for _ in range(host_reps):
        tpl, offsets, dt = host_densify()
        host_us.append(dt)
        for _ in range(3):
            ddt, ragged = timed(lambda: hint_amd.hausdorff_distances(x, torch.from_numpy(tpl).to(dev), offsets=torch.from_numpy(offsets).to(dev),
                                                                      n_points=P))
            dev_us.append(ddt)
    lib = _lib.load()
    row = {name: stats(v) for name, v in us.items()}
    row["ragged_host"], row["ragged_device"] = stats(host_us), stats(dev_us)
    row["outline_points_mean"] = float(len(tpl) / n)
    served = torch.isfinite(outs["fused_hausdorff"][0])
    row["rows_served"] = int(served.sum())
    row["max_abs_difference_max_h_torch"] = float((outs["fused_hausdorff"][0] - outs["torch_hausdorff"][0])[served].abs().max())
    row["max_abs_difference_avg_h_torch"] = float((outs["fused_hausdorff"][1] - outs["torch_hausdorff"][1])[served].abs().max())
    row["max_abs_difference_max_h_ragged"] = float((outs["fused_hausdorff"][0] - ragged[0])[served].abs().max())
    row["max_abs_difference_loss_torch"] = float((outs["fused_loss"] - outs["torch_loss"]).abs().max())
    row["workgroups"] = int(lib.hint_plus_geometry(n, P, 0))
    row["fused_pairs_per_second"] = 2.0 * len(tpl) * P / (row["fused_hausdorff"]["median_us"] * 1e-6)
    for name in ("hausdorff", "loss"):
        row[f"torch_over_fused_{name}"] = row[f"torch_{name}"]["median_us"] / row[f"fused_{name}"]["median_us"]
    row["ragged_device_over_fused"] = row["ragged_device"]["median_us"] / row["fused_hausdorff"]["median_us"]
    row["ragged_host_over_fused"] = row["ragged_host"]["median_us"] / row["fused_hausdorff"]["median_us"]
    row["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    return emit_row(row, lib)


def summary(n, row):
    print_stats(n, row, ("fused_hausdorff", "torch_hausdorff", "ragged_host", "ragged_device", "fused_loss", "torch_loss"), 16, 14)
    print(f"N={n} torch / fused: distances {row['torch_over_fused_hausdorff']:.2f}, loss {row['torch_over_fused_loss']:.2f}; ragged "
          f"route / fused: device {row['ragged_device_over_fused']:.2f}, host {row['ragged_host_over_fused']:.1f}; "
          f"{row['outline_points_mean']:.0f} outline points a row, {row['rows_served']} of {n} rows served; max_h differs from "
          f"torch's by at most {row['max_abs_difference_max_h_torch']:.3g}, from the ragged route's by "
          f"{row['max_abs_difference_max_h_ragged']:.3g}; the loss from torch's by {row['max_abs_difference_loss_torch']:.3g}")


def main():
    ap = parser("plus_time.json", 3)
    ap.add_argument("--host-reps", type=int, default=1, help="(internal) repetitions of the host route of --one")
    args = ap.parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.host_reps, args.warmup)
    res = {"n_coeffs": K, "n_points": P, "n_points_loss": P_FIT, "max_dist": MAX_DIST, "torch_chunk_rows": CHUNK,
           "commit": args.commit or commit_of_tree(), "shapes": {}}
    sizes = [(n, ("--reps", reps, "--host-reps", host_reps, "--warmup", args.warmup)) for n, reps, host_reps in SIZES]
    return drive(__file__, LIMIT_S, sizes, res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
