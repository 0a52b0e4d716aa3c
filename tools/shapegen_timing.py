#!/usr/bin/env python3
"""Time the lens-shape prior sampler (hint_amd.sample_lens_prior: one launch of hint_lensgen_run a call; the reference's
LensShapeModel.sample_prior, data.py:102-111, a polygon-library intersection and a DFT per row on the host):

    python tools/shapegen_timing.py [--reps 20] [--warmup 3] [--rows 10000000] [--out profiles/shapegen_timing.json] [--commit <hash>]

  "prior"   sample_lens_prior(rows, seed) into a fresh tensor, HIP events around the call: rows per second, and the share of the
            write bound this is (80 bytes a row against --peak-gbs, 8000 GB/s of HBM by default)
  "joint"   sample_lens_joint(rows, seed): the sampler, the observation noise and the simulator (two launches)
  "chunks"  1e8 rows (ten times --rows) as ten calls with offset = 0, rows, 2 rows, ..: the prior of prepare_samples
            (rejection_sampling.py:76-85), each chunk dropped before the next is made, host clock around all ten
  "oracle"  tests/shapegen_oracle.py on the host (numpy float64, Sutherland-Hodgman clipping) on --oracle-rows rows, for scale:
            it stands where the reference's loop stood, whose polygon library is not a dependency of this project
One process, no children; it arms its own time limit (--limit seconds, SIGALRM: the process ends there) and fails without a GPU.
"""
import json
import os
import signal
import sys
import time

from _timing import commit_of_tree, parser, stats, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = parser("shapegen_timing.json", 3)
    ap.set_defaults(reps=20)
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--oracle-rows", type=int, default=2000)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM bandwidth the write bound is taken from")
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hint_amd
    from hint_amd import _lib
    import shapegen_oracle as so

    assert torch.cuda.is_available(), "shapegen_timing.py needs a GPU"
    assert args.reps >= 1 and args.rows >= 1
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n, seed = args.rows, 20261020
    res = {"commit": args.commit or commit_of_tree(), "device": torch.cuda.get_device_name(0), "build": lib.hint_build_info().decode(),
           "reps": args.reps, "warmup": args.warmup, "rows": n, "peak_gbs": args.peak_gbs}
    routes = {"prior": lambda: hint_amd.sample_lens_prior(n, seed, device=dev),
              "joint": lambda: hint_amd.sample_lens_joint(n, seed, device=dev)}
    for fn in routes.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():
            us[name].append(timed(fn)[0])
    for name in routes:
        row = stats(us[name])
        row["rows_per_s"] = n / (row["median_us"] * 1e-6)
        res[name] = row
        print(f"{name:6s} {n} rows: median {row['median_us']:.1f} us  quartiles {row['q1_us']:.1f} .. {row['q3_us']:.1f}  "
              f"range {row['min_us']:.1f} .. {row['max_us']:.1f}  ({row['reps']} repetitions): {row['rows_per_s']:.4g} rows / s")
    bound_us = 80.0 * n / (args.peak_gbs * 1e9) * 1e6
    res["prior"]["write_bound_us"] = bound_us
    res["prior"]["fraction_of_write_bound"] = bound_us / res["prior"]["median_us"]
    print(f"write bound (80 B / row at {args.peak_gbs:.0f} GB/s): {bound_us:.1f} us: the sampler reaches "
          f"{100 * res['prior']['fraction_of_write_bound']:.1f} % of it")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in range(10):
        x = hint_amd.sample_lens_prior(n, seed, offset=c * n, device=dev)
        del x
    torch.cuda.synchronize()
    res["chunks"] = {"rows": 10 * n, "chunk_rows": n, "seconds": time.perf_counter() - t0}
    print(f"chunks {10 * n} rows in 10 calls: {res['chunks']['seconds']:.4f} s")
    d = so.draws(seed, 0, args.oracle_rows)
    t0 = time.perf_counter()
    so.sample(d)
    dt = time.perf_counter() - t0
    res["oracle"] = {"rows": args.oracle_rows, "seconds": dt, "rows_per_s": args.oracle_rows / dt}
    print(f"oracle {args.oracle_rows} rows on the host: {dt:.3f} s, {res['oracle']['rows_per_s']:.0f} rows / s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
