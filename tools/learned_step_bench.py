"""Step times of FlowTrainer(learned_perms=True) against the module route with ClampAdam and against the fixed twin on the
block-by-block route, and the batched finish launch against single grad runs (DESIGN section 25 quotes its output).  HIP events
around 10 calls, 25 such samples per variant after 5 warm-up calls, the variants taking turns; prints one JSON object with the
median, minimum and maximum of every variant's samples in ms per call.  Needs an MI355X:
    python tools/learned_step_bench.py"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import hint_amd
from hint_amd import _lib, householder as hh
from hint_amd._ops import _run_desc

DEV = "cuda:0"
ADAM = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)
SAMPLES, INNER = 25, 10


def fixed_twin(flow, make):
    twin = make().to(DEV)
    twin.load_state_dict(flow.state_dict(), strict=False)
    for i, p in enumerate(flow.perms):
        if isinstance(p, hint_amd.HouseholderPerm):
            twin.perms[i] = hint_amd.FixedOrthogonal([(p.d,)], W=p.matrix().clone()).to(DEV)
    return twin


def alternate(variants):
    """{name: fn} -> {name: [ms per call]}: every sample times INNER calls of one variant, the variants taking turns"""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(SAMPLES):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / INNER)
    return out


def summary(ts):
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for k, v in ts.items()}


def steps(name, d, blocks, widths, B):
    torch.manual_seed(0)
    flow = hint_amd.HintFlow(d, blocks, widths, learned_perms=True).to(DEV)
    module = copy.deepcopy(flow)
    twin = fixed_twin(flow, lambda: hint_amd.HintFlow(d, blocks, widths))
    twin2 = copy.deepcopy(twin)
    flow2 = copy.deepcopy(flow)
    x = torch.randn(B, d, device=DEV)
    params = [p for p in module.parameters() if p.requires_grad]
    optim = hint_amd.ClampAdam(params, grad_clamp=5.0, **ADAM)

    def module_step():
        optim.zero_grad()
        xn = x + 0.01 * torch.randn_like(x)
        z = module(xn)
        J = module.log_jacobian(run_forward=False)
        (0.5 * torch.sum(z ** 2, dim=1).mean() - J.mean()).backward()
        optim.step()
    kw = dict(grad_clamp=5.0, seed=1, **ADAM)
    tg = hint_amd.FlowTrainer(flow, learned_perms=True, **kw)
    te = hint_amd.FlowTrainer(flow2, learned_perms=True, use_graph=False, **kw)
    fg = hint_amd.FlowTrainer(twin, use_chain=False, **kw)
    fe = hint_amd.FlowTrainer(twin2, use_chain=False, use_graph=False, **kw)
    ts = alternate({"a_module_route_clamp_adam": module_step, "b_learned_captured": lambda: tg.step(x),
                    "b_learned_eager": lambda: te.step(x), "c_fixed_twin_unchained_captured": lambda: fg.step(x),
                    "c_fixed_twin_unchained_eager": lambda: fe.step(x)})
    rec = summary(ts)
    rec["b_minus_c_captured_ms"] = rec["b_learned_captured"]["median_ms"] - rec["c_fixed_twin_unchained_captured"]["median_ms"]
    rec["b_minus_c_eager_ms"] = rec["b_learned_eager"]["median_ms"] - rec["c_fixed_twin_unchained_eager"]["median_ms"]
    rec["shape"] = dict(d=d, blocks=blocks, widths=widths, B=B, permutations=len(tg.perm_mods))
    return rec


def finish(m=3, d=100, n=100, B=4096):
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    Vs = (0.2 * torch.randn(m, n, d, generator=g) + torch.eye(n, d)).to(DEV).contiguous()
    xs = (torch.randn(m, B, d, generator=g) + 2).to(DEV)
    gys = (torch.randn(m, B, d, generator=g) + 2).to(DEV)
    W = torch.empty(m, d, d, device=DEV)
    gV, gV1 = torch.empty(m, n, d, device=DEV), torch.empty(m, n, d, device=DEV)
    nbytes = lib.hint_householder_many_workspace_bytes(1, m, B, d, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws1 = torch.empty(nbytes // m, dtype=torch.uint8, device=DEV)

    def many(op, **f):
        job = _lib.HouseholderMany()
        job.op, job.m, job.B, job.d, job.n = op, m, B, d, n
        job.Vs, job.vs_stride, job.W, job.w_stride = Vs.data_ptr(), n * d, W.data_ptr(), d * d
        job.g_V, job.gv_stride = gV.data_ptr(), n * d
        job.workspace, job.workspace_bytes, job.ws_stride = ws.data_ptr(), nbytes, nbytes // (4 * m)
        for k, v in f.items():
            setattr(job, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        _run_desc("hint_householder_many_run", job, DEV)
    many(0)

    def rows():
        for j in range(m):
            many(1, j=j, x=xs[j], g_y=gys[j])

    def singles():
        for j in range(m):
            hh._run(2, DEV, B=B, d=d, n=n, Vs=Vs[j], W=W[j], x=xs[j], g_y=gys[j], g_V=gV1[j], workspace=ws1)
    rows()
    ts = alternate({"finish_many_one_launch": lambda: many(2), "rows_x3_plus_finish_many": lambda: (rows(), many(2)),
                    "three_single_grad_runs_gram_plus_finish": singles})
    torch.cuda.synchronize()
    assert torch.equal(gV.view(torch.int32), gV1.view(torch.int32))
    rec = summary(ts)
    rec["shape"] = dict(m=m, d=d, n=n, B=B)
    return rec


if __name__ == "__main__":
    out = {"finish": finish(), "flagship": steps("flagship", 100, 4, [224, 112, 56], 4096),
           "lens": steps("lens", 20, 2, [95, 47, 23], 10000)}
    print(json.dumps(out, indent=1))
