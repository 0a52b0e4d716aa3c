"""What feeds the training step, measured on the MI355X: one epoch of 390 batches of 4096 rows of synthetic
POWER-shaped data (1 600 000 x 6, 8 blocks [140, 70, 35, 17]) through

    (a) fit          FlowTrainer.fit_epoch on a DeviceDataset: one keyed gather and one step_many per 16 batches
    (b) resident     step_many on random batches that already sit in its input buffers: the floor (no data path at all)
    (c) loader       the reference's DataLoader(TensorDataset(x, zeros), batch_size, shuffle=True, drop_last=True) on the host
                     (data.py:503-506), each batch copied into input_buffers() and stepped

Wall time of a whole epoch by the host's clock, the device synchronised before the first and after the last batch; every route is
warmed (graphs captured, kernels loaded) by a short run first; (a) and (b) alternate over --reps epochs, (c) runs --loader-reps.
Prints one JSON line.  There is no CPU path: without a GPU the script fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hint_amd  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_600_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loader-reps", type=int, default=1)
    ap.add_argument("--loader-batches", type=int, default=0, help="batches of the loader's epoch (0: all)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "epoch_path.py measures on a GPU"
    dev = torch.device("cuda:0")
    d, B, K = 6, args.batch, args.chunk
    g = torch.Generator().manual_seed(1)
    host_x = torch.randn(args.rows, d, generator=g)
    ds = hint_amd.DeviceDataset(host_x.to(dev), seed=1)
    ds.standardize()
    n_batches = ds.n_batches(B)
    torch.manual_seed(0)
    flow = hint_amd.HintFlow(d, 8, [140, 70, 35, 17]).to(dev)
    tr = hint_amd.FlowTrainer(flow, seed=3)

    def fit():
        return tr.fit_epoch(ds, fit.epoch, B, chunk=K)
    fit.epoch = 0

    resident = torch.randn(K, B, d, device=dev)

    def floor():
        xs, _ = tr.input_buffers_many(resident)
        for _ in range(n_batches // K):
            tr.step_many(xs)
        for j in range(n_batches % K):
            tr.step(xs[j])

    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(host_x, torch.zeros(len(host_x), 1)), batch_size=B,
                                         shuffle=True, drop_last=True)
    n_loader = n_batches if args.loader_batches == 0 else min(n_batches, args.loader_batches)

    def loaded():
        buf, _ = tr.input_buffers(torch.zeros(B, d, device=dev))
        for i, (x, _) in enumerate(loader):
            if i >= n_loader:
                break
            buf.copy_(x, non_blocking=True)
            tr.step(buf)

    tr.fit_epoch(ds, 0, B, max_batches=2 * K + 1, chunk=K)      # warm-up: both graphs, every kernel
    floor()
    torch.cuda.synchronize()
    t = {"fit": [], "resident": []}
    for rep in range(args.reps):
        fit.epoch = rep + 1
        t["fit"].append(wall(fit))
        t["resident"].append(wall(floor))
    t["loader"] = [wall(loaded) for _ in range(args.loader_reps)]
    gather_us = []
    out = tr._static_many["x"]
    for rep in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ds.gather(rep, 0, K, B, out=out)
        b.record()
        b.synchronize()
        gather_us.append(a.elapsed_time(b) * 1e3)
    res = dict(rows=args.rows, d=d, batch=B, chunk=K, batches=n_batches, loader_batches=n_loader, reps=args.reps,
               device=torch.cuda.get_device_name(0), gather_us_median=statistics.median(gather_us))
    for name, v in t.items():
        nb = n_loader if name == "loader" else n_batches
        res[name] = dict(epoch_s_median=statistics.median(v), epoch_s_min=min(v), epoch_s_max=max(v),
                         ms_per_step=1e3 * statistics.median(v) / nb)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
