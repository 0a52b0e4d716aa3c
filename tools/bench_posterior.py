"""Posterior sampling of the conditional model at cfg 4 full size (conditional_hint_4_full.py:58-94: x d = 100, y d = 4, 4 blocks,
hidden 224; weights 0.03 * randn as tests/test_gpu_conditional.py): HIP-event times per call of
  module_inverse         the reference's model_inverse (conditional_hint_4_full.py:99-102) on the module route: a forward of both
                         lanes on random x, then the inverse of both lanes - one observation expanded to B rows, as
                         rejection_sampling.py:168-213 (compare_conditional) calls it
  sample_one_y           ConditionalHintFlow.sample_conditional(y [ny], z_x [B, nx]): one observation, B draws
  sample_per_row_y       sample_conditional with B distinct observations
  x_lane_forward         ConditionalHintFlow.x_lane_forward at B rows, B distinct observations (evaluate(only_x=True))
and the agreement of sample_one_y with module_inverse.  Prints one JSON line (and writes it to --out).
   python tools/bench_posterior.py [--batch 4096] [--reps 50] [--warmup 5] [--out file.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hint_amd  # noqa: E402


def timed(fn, reps, warmup):
    """median and minimum of `reps` calls, each between two HIP events on the current stream, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    nx, ny, B = 100, 4, a.batch
    model = hint_amd.ConditionalHintFlow(nx, ny, 4, 224).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            p.data = 0.03 * torch.randn_like(p)
    y1 = torch.randn(ny, device=dev)
    yB = torch.randn(B, ny, device=dev)
    z = torch.randn(B, nx, device=dev)

    def model_inverse(y, zx):          # conditional_hint_4_full.py:99-102
        z_y, _ = model([y, torch.randn(y.shape[0], nx, device=dev)])
        _, x = model([z_y, zx], rev=True)
        return x

    y_exp = y1.expand(B, ny)
    res = {"config": f"cfg 4: nx {nx}, ny {ny}, 4 blocks, hidden 224, B {B}", "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        res["module_inverse"] = timed(lambda: model_inverse(y_exp, z), a.reps, a.warmup)
        res["sample_one_y"] = timed(lambda: model.sample_conditional(y1, z), a.reps, a.warmup)
        res["sample_per_row_y"] = timed(lambda: model.sample_conditional(yB, z), a.reps, a.warmup)
        res["x_lane_forward"] = timed(lambda: model.x_lane_forward(z, yB), a.reps, a.warmup)
        xm = model_inverse(y_exp, z)
        xs, _ = model.sample_conditional(y1, z)
    res["speedup_one_y_vs_module"] = round(res["module_inverse"]["median_us"] / res["sample_one_y"]["median_us"], 2)
    res["max_abs_diff_one_y_vs_module"] = float((xs - xm).abs().max())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
