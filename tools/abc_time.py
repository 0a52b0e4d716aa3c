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
import os
import sys

from _timing import alternate, drive, emit_row, parser, stats

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

    peak = {}

    def peaks():
        for name, fn in routes.items():              # device bytes a call allocates on top of y and the target
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out = fn()
            torch.cuda.synchronize()
            peak[name] = int(torch.cuda.max_memory_allocated(dev) - base)
            del out

    us, outs = alternate(routes, reps, warmup, peaks)
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
    return emit_row(row, lib)


def summary(n, row):
    for name in ("fused", "torch"):
        s = row[name]
        print(f"N={n} {name:6s} median {s['median_us']:10.1f} us  quartiles {s['q1_us']:.1f} .. {s['q3_us']:.1f}  "
              f"range {s['min_us']:.1f} .. {s['max_us']:.1f}  allocates {row['allocated_bytes'][name]} bytes")
    print(f"N={n} torch / fused = {row['torch_over_fused']:.2f}; fused reads y at {row['fused_y_bytes_per_second'] / 1e12:.2f} TB/s "
          f"over {row['passes_over_y']} passes; {row['indices_shared_with_topk']} of {K} indices shared with topk")


def main():
    ap = parser("abc_time.json", 5, commit=False)
    ap.set_defaults(reps=30)
    args = ap.parse_args()
    if args.one:
        return one_size(args.one, args.reps, args.warmup)
    res = {"ny": NY, "k": K, "shapes": {}}
    return drive(__file__, LIMIT_S, [(n, ("--reps", args.reps, "--warmup", args.warmup)) for n in SIZES], res, args.out, summary)


if __name__ == "__main__":
    sys.exit(main())
