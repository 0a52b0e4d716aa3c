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
import argparse
import json
import math
import os
import subprocess
import sys
import time

from _timing import commit_of_tree, stats

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

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3, out          # microseconds

    routes = {"fused_hausdorff": lambda: hint_amd.plus_hausdorff_distances(x, params, max_dist=MAX_DIST, n_points=P),
              "torch_hausdorff": torch_hausdorff,
              "fused_loss": lambda: hint_amd.plus_fit_loss(x, params), "torch_loss": torch_loss}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in routes}
    outs = {}
    for _ in range(reps):                            # alternate: clocks and caches drift for all routes alike
        for name, fn in routes.items():
            dt, out = timed(fn)
            us[name].append(dt)
            outs[name] = out
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
    row["device"] = torch.cuda.get_device_name(0)
    row["build"] = lib.hint_build_info().decode()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plus_time.json"))
    ap.add_argument("--commit", default=None, help="the commit the tree was built from (default: git rev-parse HEAD)")
    ap.add_argument("--one", type=int, default=0, help="(internal) time this N and print its JSON row")
    ap.add_argument("--reps", type=int, default=0, help="(internal) repetitions of --one")
    ap.add_argument("--host-reps", type=int, default=1, help="(internal) repetitions of the host route of --one")
    args = ap.parse_args()
    if args.one:
        print("ROW " + json.dumps(one_size(args.one, args.reps, args.host_reps, args.warmup)))
        return 0
    res = {"n_coeffs": K, "n_points": P, "n_points_loss": P_FIT, "max_dist": MAX_DIST, "torch_chunk_rows": CHUNK,
           "commit": args.commit or commit_of_tree(), "shapes": {}}
    for n, reps, host_reps in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(reps), "--host-reps",
                                str(host_reps), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"N={n}: no result within {LIMIT_S} s; stopping")
            return 1
        rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not rows:
            print(f"N={n}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            return 1
        row = json.loads(rows[-1])
        res["device"], res["build"] = row.pop("device"), row.pop("build")
        res["shapes"][str(n)] = row
        for name in ("fused_hausdorff", "torch_hausdorff", "ragged_host", "ragged_device", "fused_loss", "torch_loss"):
            s = row[name]
            print(f"N={n} {name:16s} median {s['median_us']:14.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
                  f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  ({s['reps']} repetitions)")
        print(f"N={n} torch / fused: distances {row['torch_over_fused_hausdorff']:.2f}, loss {row['torch_over_fused_loss']:.2f}; ragged "
              f"route / fused: device {row['ragged_device_over_fused']:.2f}, host {row['ragged_host_over_fused']:.1f}; "
              f"{row['outline_points_mean']:.0f} outline points a row, {row['rows_served']} of {n} rows served; max_h differs from "
              f"torch's by at most {row['max_abs_difference_max_h_torch']:.3g}, from the ragged route's by "
              f"{row['max_abs_difference_max_h_ragged']:.3g}; the loss from torch's by {row['max_abs_difference_loss_torch']:.3g}")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
