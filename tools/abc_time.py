#!/usr/bin/env python3
"""Time hint_amd.nearest_rows against the formulation a user would otherwise write,

    torch.topk(((y - t) ** 2).sum(1), k, largest=False)

alternating the two in one process, and record the device bytes each allocates.

    python tools/abc_time.py [--reps 30] [--out profiles/abc_time.json]

Shapes: ny = 2, k = 4002 (quantile_abc with n = 4000) at N = 2^20, 2^24 and 1e8 (what compare_conditional selects from).  Every
size runs in a child process of its own under a time limit, and a size that fails ends the run: nothing more is started on the
device after it.  Both routes are warmed up, every repetition is bracketed by HIP events on the current stream, and the medians,
quartiles and extremes are printed and written.
"""
import argparse
import json
import os
import subprocess
import sys

from _timing import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1 << 20, 1 << 24, 10 ** 8)
NY, K = 2, 4002
LIMIT_S = 240           # per size


def one_size(n, reps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import hint_amd
    from hint_amd import _lib

    assert torch.cuda.is_available(), "abc_time.py needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(n % 1000003)
    y = torch.randn(n, NY, generator=g, device=dev)
    t = torch.randn(NY, generator=g, device=dev)
    routes = {"fused": lambda: hint_amd.nearest_rows(y, t, K),
              "torch": lambda: torch.topk(((y - t) ** 2).sum(1), K, largest=False)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3, out          # microseconds

    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    peak = {}
    for name, fn in routes.items():                  # device bytes a call allocates on top of y and the target
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated(dev) - base)
        del out
    us = {name: [] for name in routes}
    outs = {}
    for _ in range(reps):                            # alternate: clocks and caches drift for both routes alike
        for name, fn in routes.items():
            dt, out = timed(fn)
            us[name].append(dt)
            outs[name] = out
    fi, fd = outs["fused"]
    tv, ti = outs["torch"]
    # topk's order among its results is its own: compare as sets
    agree = len(set(fi.tolist()) & set(ti.tolist()))
    lib = _lib.load()
    passes = lib.hint_abc_geometry(n, NY, 2)
    row = {name: stats(v) for name, v in us.items()}
    row["allocated_bytes"] = peak
    row["workspace_bytes"] = int(lib.hint_abc_workspace_bytes(n, NY, K))
    row["workgroups"], row["rows_per_workgroup"], row["passes_over_y"] = (int(lib.hint_abc_geometry(n, NY, f)) for f in range(3))
    row["fused_y_bytes_per_second"] = passes * n * NY * 4 / (row["fused"]["median_us"] * 1e-6)
    row["torch_over_fused"] = row["torch"]["median_us"] / row["fused"]["median_us"]
    row["indices_shared_with_topk"] = agree
    row["threshold"] = float(fd[-1])
    row["device"] = torch.cuda.get_device_name(0)
    row["build"] = lib.hint_build_info().decode()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abc_time.json"))
    ap.add_argument("--one", type=int, default=0, help="(internal) time this N and print its JSON row")
    args = ap.parse_args()
    if args.one:
        print("ROW " + json.dumps(one_size(args.one, args.reps, args.warmup)))
        return 0
    res = {"ny": NY, "k": K, "shapes": {}}
    for n in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(args.reps), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=LIMIT_S)
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
        for name in ("fused", "torch"):
            s = row[name]
            print(f"N={n} {name:6s} median {s['median_us']:10.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
                  f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  allocates {row['allocated_bytes'][name]} bytes")
        print(f"N={n} torch / fused = {row['torch_over_fused']:.2f}; fused reads y at {row['fused_y_bytes_per_second'] / 1e12:.2f} TB/s "
              f"over {row['passes_over_y']} passes; {row['indices_shared_with_topk']} of {K} indices shared with topk")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
