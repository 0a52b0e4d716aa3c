#!/usr/bin/env python3
"""Time the plus-shape sampler (hint_amd.sample_plus_prior and its siblings: one launch of hint_plusgen_run a call; the reference's
PlusShapeModel.sample_prior / sample_joint, data.py:229-252, a polygon-library union, a densify_polyline and a 25-coefficient DFT
per row on the host):

    python tools/plusgen_timing.py [--reps 20] [--warmup 3] [--rows 10000000] [--out profiles/plusgen_timing.json] [--commit <hash>]

  "prior"        sample_plus_prior(rows, seed) into a fresh tensor, HIP events around the call: rows per second, the share of the
                 write bound this is (400 bytes a row against --peak-gbs, 8000 GB/s of HBM by default), and the share of the lens
                 sampler's measured rate (--lens-rows-per-s, profiles/shapegen_timing.json) scaled by the transform's operation
                 count: 32 points x 3 frequencies there, the mean point count x 13 frequencies here
  "joint"        sample_plus_joint(rows, seed): x and y in the same launch
  "labels"       a labels-only run (y alone): the candidates of the rejection loop
  "conditional"  sample_plus_conditional(target, 4000, seed, radius=0.05), the reference's radius (rejection_sampling.py:113-127),
                 host clock around the call (it reads one number back per chunk), with `tried` recorded
  "oracle"       tests/plusgen_oracle.py on the host (numpy float64) on --oracle-rows rows, for scale: it stands where the
                 reference's loop stood, whose polygon library is not a dependency of this project
One process, no children; it arms its own time limit (--limit seconds, SIGALRM: the process ends there) and fails without a GPU.
"""
import json
import os
import signal
import sys
import time

from _timing import commit_of_tree, parser, stats, timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = (0.2, -0.1, 0.6, 1.5)


def main():
    ap = parser("plusgen_timing.json", 3)
    ap.set_defaults(reps=20)
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--oracle-rows", type=int, default=2000)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM bandwidth the write bound is taken from")
    ap.add_argument("--lens-rows-per-s", type=float, default=2.2e10, help="the lens sampler's measured rate (DESIGN section 21)")
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends itself")
    args = ap.parse_args()
    signal.alarm(args.limit)
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hint_amd
    from hint_amd import _lib, plusgen
    import plusgen_oracle as po

    assert torch.cuda.is_available(), "plusgen_timing.py needs a GPU"
    assert args.reps >= 1 and args.rows >= 1
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n, seed = args.rows, 20261020
    res = {"commit": args.commit or commit_of_tree(), "device": torch.cuda.get_device_name(0), "build": lib.hint_build_info().decode(),
           "reps": args.reps, "warmup": args.warmup, "rows": n, "peak_gbs": args.peak_gbs}
    routes = {"prior": lambda: hint_amd.sample_plus_prior(n, seed, device=dev),
              "joint": lambda: hint_amd.sample_plus_joint(n, seed, device=dev),
              "labels": lambda: plusgen._plus_run(n, seed, 0, dev, None, ["y"])}
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
    bound_us = 400.0 * n / (args.peak_gbs * 1e9) * 1e6
    counts = plusgen._plus_run(min(n, 10 ** 6), seed, 0, dev, None, ["y", "counts"])["counts"]
    mean_count = float(counts.double().mean())
    scaled = args.lens_rows_per_s * (32 * 3) / (mean_count * 13)
    res["prior"].update(write_bound_us=bound_us, fraction_of_write_bound=bound_us / res["prior"]["median_us"], mean_count=mean_count,
                        lens_rate_scaled_rows_per_s=scaled, fraction_of_lens_rate_scaled=res["prior"]["rows_per_s"] / scaled)
    print(f"write bound (400 B / row at {args.peak_gbs:.0f} GB/s): {bound_us:.1f} us: the sampler reaches "
          f"{100 * res['prior']['fraction_of_write_bound']:.1f} % of it; the lens sampler's rate scaled by the operation count "
          f"(mean count {mean_count:.1f}): {scaled:.3g} rows / s, of which this is {100 * res['prior']['fraction_of_lens_rate_scaled']:.0f} %")
    for _ in range(2):                                       # the second call is the one timed: the first warms the chunk's allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, y, tried = hint_amd.sample_plus_conditional(TARGET, 4000, seed, 0.05, device=dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    res["conditional"] = {"n": 4000, "radius": 0.05, "target": list(TARGET), "tried": tried, "seconds": dt, "accepted_one_in": tried / 4000.0}
    print(f"conditional: 4000 rows within 0.05 of {TARGET}: {tried} candidates tried (one in {tried / 4000.0:.0f} kept), {dt:.4f} s")
    d = po.draws(seed, 0, args.oracle_rows)
    t0 = time.perf_counter()
    po.sample(d)
    dt = time.perf_counter() - t0
    res["oracle"] = {"rows": args.oracle_rows, "seconds": dt, "rows_per_s": args.oracle_rows / dt}
    print(f"oracle {args.oracle_rows} rows on the host: {dt:.3f} s, {res['oracle']['rows_per_s']:.0f} rows / s")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
