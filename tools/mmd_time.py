#!/usr/bin/env python3
"""Time hint_amd.multi_mmd against the torch formulation it replaces (three N x N GEMMs, norms from the Gram diagonals, clamp,
one pass per kernel and term, one mean), alternating the two in one process.

    python tools/mmd_time.py [--reps 200] [--out profiles/mmd_time.json]

Shapes: N = M = 4000 at d = 20 and d = 100 (what compare_unconditional / compare_conditional score).  Both are warmed up, every
repetition is bracketed by HIP events on the current stream, and the medians, quartiles and extremes are printed and written.
"""
import argparse
import json
import os
import sys

import torch

from _timing import alternate, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hint_amd  # noqa: E402
from hint_amd import _lib  # noqa: E402

KERNELS = ((0.5, 1), (0.2, 1), (0.2, 0.5))


def torch_formulation(x, y, kernels=KERNELS):
    gxx, gyy, gxy = x @ x.t(), y @ y.t(), x @ y.t()
    rx, ry = gxx.diag(), gyy.diag()
    dxx = (rx[:, None] + rx[None, :] - 2. * gxx).clamp(min=0)
    dyy = (ry[:, None] + ry[None, :] - 2. * gyy).clamp(min=0)
    dxy = (rx[:, None] + ry[None, :] - 2. * gxy).clamp(min=0)
    kxx, kyy, kxy = torch.zeros_like(gxx), torch.zeros_like(gyy), torch.zeros_like(gxy)
    for C, a in kernels:
        kxx += C ** a * ((C + dxx) / a) ** -a
        kyy += C ** a * ((C + dyy) / a) ** -a
        kxy += C ** a * ((C + dxy) / a) ** -a
    return torch.mean(kxx + kyy - 2. * kxy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mmd_time.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().hint_build_info().decode(), "kernels": KERNELS, "shapes": {}}
    for n, d in ((4000, 20), (4000, 100)):
        g = torch.Generator(device=dev).manual_seed(n + d)
        x = torch.randn(n, d, generator=g, device=dev)
        y = 0.05 + 1.05 * torch.randn(n, d, generator=g, device=dev)
        gt = hint_amd.MultiMMD(y)
        routes = {"fused": lambda: hint_amd.multi_mmd(x, y), "fused_yy_kept": lambda: gt.mmd(x),
                  "torch": lambda: torch_formulation(x, y)}
        us, outs = alternate(routes, args.reps, args.warmup)
        vals = {k: float(v) for k, v in outs.items()}
        row = {k: stats(v) for k, v in us.items()}
        row["values"] = vals
        row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
        row["torch_over_fused_yy_kept"] = row["torch"]["median_us"] / row["fused_yy_kept"]["median_us"]
        res["shapes"][f"{n}x{d}"] = row
        for k in routes:
            s = row[k]
            print(f"N={n} d={d} {k:14s} median {s['median_us']:9.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
                  f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  value {vals[k]:.9g}")
        print(f"N={n} d={d} torch / fused = {row['torch_over_fused']:.2f}, with mean YY kept {row['torch_over_fused_yy_kept']:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
