#!/usr/bin/env python3
"""Time the correlation MSE of a device sample (the second number of the reference's test_likelihood, run_experiments.py:212-221)
on three routes, alternating them in one process:

  "host":  what the reference does - x.cpu().numpy(), np.corrcoef(x.T), np.nanmean(np.square(corr - corr_true))
  "torch": torch.corrcoef(x.T.double()) and a nanmean on the device, the result brought back as a float
  "fused": hint_amd.corr_mse(x, corr_true) (hint_corr_run: four launches), the result brought back as a float

    python tools/corr_timing.py [--reps 200] [--warmup 10] [--out profiles/corr_timing.json] [--commit <hash>]

Shapes: 10000 x 100 and 4000 x 100 (the unconditional and conditional samples of the widest models) and 4000 x 20 (the
conditional lens model).  Every repetition of every route starts on an idle device and ends when its float is on the host, and
is timed with the host's clock: each route pays for its own synchronisation, as a caller who wants the number does.  The
"fused_device" figure is the same call bracketed by HIP events instead, without the read-back.  One process, no children; it
arms its own time limit (--limit seconds, SIGALRM: the process ends there) and fails without a GPU.
"""
import json
import os
import signal
import sys
import time

import numpy as np

from _timing import commit_of_tree, parser, stats, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((10000, 100), (4000, 100), (4000, 20))


def main():
    ap = parser("corr_timing.json", 10)
    ap.set_defaults(reps=200)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "corr_timing.py needs a GPU"
    assert args.reps >= 1
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"commit": args.commit or commit_of_tree(), "device": torch.cuda.get_device_name(0), "build": lib.hint_build_info().decode(),
           "reps": args.reps, "warmup": args.warmup, "clock": "host, idle device to float on the host", "shapes": {}}
    for n, d in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + d)
        A = torch.randn(d, d, generator=g, device=dev) / d ** 0.5 + 0.5 * torch.eye(d, device=dev)
        x = (torch.randn(n, d, generator=g, device=dev) @ A).contiguous()
        y = torch.randn(n, d, generator=g, device=dev) @ (A + 0.1 * torch.randn(d, d, generator=g, device=dev) / d ** 0.5)
        corr_true = np.corrcoef(y.cpu().numpy().T)
        t_dev = torch.from_numpy(corr_true).to(dev)

        def host():
            c = np.corrcoef(x.cpu().numpy().T)
            return float(np.nanmean(np.square(c - corr_true)))

        def torch_route():
            c = torch.corrcoef(x.t().double())
            return float(torch.nanmean(torch.square(c - t_dev)))

        def fused():
            return float(hint_amd.corr_mse(x, t_dev))

        routes = {"host": host, "torch": torch_route, "fused": fused}
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        us = {name: [] for name in routes}
        us["fused_device"] = []
        val = {}
        for _ in range(args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                val[name] = fn()
                us[name].append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            us["fused_device"].append(timed(lambda: hint_amd.corr_mse(x, t_dev))[0])
        row = {name: stats(v) for name, v in us.items()}
        row["mse"] = val
        row["fused_minus_host"] = val["fused"] - val["host"]
        row["torch_minus_host"] = val["torch"] - val["host"]
        row["host_over_fused"] = row["host"]["median_us"] / row["fused"]["median_us"]
        row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
        row["workspace_bytes"] = int(lib.hint_corr_workspace_bytes(n, d))
        row["jobs"], row["rows_per_slab"] = int(lib.hint_corr_job(n, d, -1, 0)), int(lib.hint_corr_job(n, d, -1, 2))
        res["shapes"][f"{n}x{d}"] = row
        for name in ("host", "torch", "fused", "fused_device"):
            s = row[name]
            print(f"{n}x{d} {name:12s} median {s['median_us']:9.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
                  f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  ({s['reps']} repetitions)")
        print(f"{n}x{d} host / fused {row['host_over_fused']:.2f}, torch / fused {row['torch_over_fused']:.2f}; mse {val['fused']:.12g}, "
              f"fused - host {row['fused_minus_host']:.3g}, torch - host {row['torch_minus_host']:.3g}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
