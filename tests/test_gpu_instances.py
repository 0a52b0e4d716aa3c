"""Every kernel instance the planner can launch against the float64 oracle (oracle/hint_oracle.py), one ledger case at a time
(tests/instance_cases.py; tests/test_dispatch_cpu.py checks the ledger without a GPU).

Per case: the batch size follows the device's CU count, and hint_plan_dispatch must show the declared instances (and, for the
multi-pass cases, two or more passes of the tile loop with a ragged last one) before anything is compared - a partitioned device
fails here instead of testing something else.  Then forward z and J, inverse x and J, and d/dx, d/dc and every weight-gradient
tensor under random per-row cotangents g_z, g_J (the NLL's d/dJ is the same constant for every row and would hide a per-row
error).  Rows with a hidden pre-activation within KINK (relative to the row's largest) of a ReLU kink in the float64 oracle get
zero cotangents: either subgradient is right there, and a zero cotangent keeps the batch size - and so the dispatch - unchanged.
Their forward and inverse are compared like every other row's."""
import pytest
import torch

import hint_amd
from hint_amd import _lib
from instance_cases import CASES, knob_env, mismatch, plan_dispatch
from oracle import hint_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINK = 1e-5
TOL_FWD = 1e-5          # z, J, inverse x, inverse J: of the largest magnitude (at least 1)
TOL_GX = 1e-4           # d/dx, d/dc: of the largest entry
TOL_GW = 2e-4           # each weight-gradient tensor: of its largest entry


class Spy:
    """records, per row, how close the oracle's hidden pre-activations come to a ReLU kink and the largest |s| fed to atan"""

    def __init__(self, B):
        self.kink = torch.full((B,), float("inf"), dtype=torch.float64)
        self.s_max = torch.zeros(B, dtype=torch.float64)

    def __enter__(self):
        self.relu, self.atan = torch.relu, torch.atan

        def relu(t):
            if t.numel() > 0:
                a = t.detach().abs().reshape(t.shape[0], -1)
                self.kink = torch.minimum(self.kink, a.min(dim=1).values / a.max(dim=1).values.clamp(min=1e-3))
            return self.relu(t)

        def atan(t):
            if t.numel() > 0:
                self.s_max = torch.maximum(self.s_max, t.detach().abs().reshape(t.shape[0], -1).max(dim=1).values)
            return self.atan(t)
        torch.relu, torch.atan = relu, atan
        return self

    def __exit__(self, *exc):
        torch.relu, torch.atan = self.relu, self.atan


def big_s(P, f):
    """the root's s subnet's last layer x f: atan saturates (|s| >= 10) - the root is the forward's last level and the inverse's
    first, so no other level sees the large values and z stays bounded"""
    return {k: (v * f if k in ("tree.s.4.weight", "tree.s.4.bias") else v) for k, v in P.items()}


def inputs(case, B, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, case.d, generator=g)
    c = torch.randn(B, case.dc, generator=g) if case.dc else None
    zi = torch.randn(B, case.d, generator=g)
    gz = torch.randn(B, case.d, generator=g)
    gJ = torch.randn(B, generator=g)
    return x, c, zi, gz, gJ


def block_params(case):
    """(the tree's node table, its float32 parameters) of a block case"""
    nodes = orc.build_nodes(case.d, [(case.dc,)] if case.dc else [], list(case.widths))
    P = orc.init_params(nodes, seed=5, scale=case.scale)
    if case.big_s:
        P = big_s(P, case.big_s)
    return nodes, P


def oracle_block_rows(case, nodes, P, rows):
    """float64 oracle of one block on explicit rows = (x, c, zi, gz, gJ) (float32, on the host): the kept-row mask, the largest |s|,
    the cotangents as used (zero on rows next to a kink) and every reference quantity"""
    x, c, zi, gz, gJ = rows
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    x64 = x.double().requires_grad_(True)
    c64 = [c.double().requires_grad_(True)] if case.dc else []
    with Spy(x.shape[0]) as spy:
        z64, J64 = orc.block_apply(nodes, P64, x64, c64, rev=False)
    keep = spy.kink > KINK
    gz, gJ = gz * keep[:, None], gJ * keep
    ((z64 * gz.double()).sum() + (J64 * gJ.double()).sum()).backward()
    with torch.no_grad():
        xi64, Ji64 = orc.block_apply(nodes, {k: v.detach() for k, v in P64.items()}, zi.double(),
                                     [t.detach() for t in c64], rev=True)
    ref = dict(z=z64.detach(), J=J64.detach(), xi=xi64, Ji=Ji64, gx=x64.grad, gc=c64[0].grad if case.dc else None,
               gw={k: v.grad for k, v in P64.items()})
    return (x, c, zi, gz, gJ), keep, spy.s_max, ref


def oracle_block(case, B):
    """float64 oracle of one block: parameters (float32), inputs, kept-row mask, and every reference quantity"""
    nodes, P = block_params(case)
    rows, keep, s_max, ref = oracle_block_rows(case, nodes, P, inputs(case, B))
    return P, rows, keep, s_max, ref


def make_chain_pair(case):
    """OracleFlow in float64 and the same flow (the same float32 weights) on the GPU"""
    dims_c = [(case.dc,)] if case.dc else ()
    ref = orc.OracleFlow(case.d, case.n_blocks, list(case.widths), dims_c=dims_c, seed=3, init_scale=case.scale,
                         dtype=torch.float64)
    ref.params = [{k: v.float().double() for k, v in P.items()} for P in ref.params]
    if case.big_s:
        ref.params = [big_s(P, case.big_s) for P in ref.params]
    ref.perms = [None if p is None else p.float().double() for p in ref.perms]
    flow = hint_amd.HintFlow(case.d, case.n_blocks, list(case.widths), ndim_c=case.dc)
    for i, blk in enumerate(flow.blocks):
        blk.load_state_dict({k: v.float() for k, v in ref.params[i].items()})
        if ref.perms[i] is not None:
            flow.perms[i].W.copy_(ref.perms[i].float())
    return ref, flow.to(DEV)


def oracle_chain(case, B, ref):
    x, c, zi, gz, gJ = inputs(case, B)
    for P in ref.params:
        for p in P.values():
            p.requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    cr = (c.double().requires_grad_(True),) if case.dc else ()
    with Spy(B) as spy:
        z64, J64 = ref.forward(x64, cr)
    keep = spy.kink > KINK
    gz, gJ = gz * keep[:, None], gJ * keep
    ((z64 * gz.double()).sum() + (J64 * gJ.double()).sum()).backward()
    with torch.no_grad():
        xi64, Ji64 = ref.inverse(zi.double(), tuple(t.detach() for t in cr))
    out = dict(z=z64.detach(), J=J64.detach(), xi=xi64, Ji=Ji64, gx=x64.grad, gc=cr[0].grad if case.dc else None,
               gw={(i, k): v.grad for i, P in enumerate(ref.params) for k, v in P.items()})
    return (x, c, zi, gz, gJ), keep, spy.s_max, out


def err(a, b):
    """max |a - b| over max |b| (at least 1e-30)"""
    a = a.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def check_fwd(what, got, ref):
    d = float((got.detach().double().cpu() - ref).abs().max())
    assert d <= TOL_FWD * max(1.0, float(ref.abs().max())), (what, d, float(ref.abs().max()))


def check_grads(name, gx, gc, gw, ref):
    assert err(gx, ref["gx"]) <= TOL_GX, (name, "d/dx", err(gx, ref["gx"]))
    if gc is not None:
        assert err(gc, ref["gc"]) <= TOL_GX, (name, "d/dc", err(gc, ref["gc"]))
    gmax = max(float(v.abs().max()) for v in ref["gw"].values())
    for k, r in ref["gw"].items():
        e = float((gw[k].detach().double().cpu() - r).abs().max())
        assert e <= TOL_GW * float(r.abs().max()) + 1e-7 * gmax, (name, k, e, float(r.abs().max()))


def assert_dispatch(case, lib, plan, B):
    disp = plan_dispatch(lib, plan, B)
    print(f"{case.name}: B={B} on {disp['num_cu']} CUs: nw={disp['nw']} nr={disp['nr']} grid={disp['grid']} passes={disp['passes']} "
          f"groups={disp['groups']}")
    m = mismatch(case, disp)
    assert m is None, m
    return disp


def run_block(case, lib, cu):
    B = case.B(cu)
    P, (x, c, zi, gz, gJ), keep, s_max, ref = oracle_block(case, B)
    blk = hint_amd.HierarchicalAffineCouplingBlock([(case.d,)], dims_c=[(case.dc,)] if case.dc else [],
                                                   c_internal=list(case.widths))
    blk.load_state_dict(P)
    blk = blk.to(DEV)
    eng = blk.tree.engine(torch.device(DEV))
    assert_dispatch(case, lib, eng.plan, B)
    xd = x.to(DEV).requires_grad_(True)
    cd = [c.to(DEV).requires_grad_(True)] if case.dc else []
    (z,) = blk([xd], c=cd)
    J = blk.jacobian(None)
    check_fwd("z", z, ref["z"])
    check_fwd("J", J, ref["J"])
    ((z * gz.to(DEV)).sum() + (J * gJ.to(DEV)).sum()).backward()
    named = dict(blk.named_parameters())
    check_grads(case.name, xd.grad, cd[0].grad if case.dc else None, {k: named[k].grad for k in ref["gw"]}, ref)
    with torch.no_grad():
        (xi,) = blk([zi.to(DEV)], c=[t.detach() for t in cd], rev=True)
        Ji = blk.jacobian(None)
    check_fwd("inverse x", xi, ref["xi"])
    check_fwd("inverse J", Ji, ref["Ji"])
    return keep, s_max


def run_chain(case, lib, cu):
    B = case.B(cu)
    ref, flow = make_chain_pair(case)
    (x, c, zi, gz, gJ), keep, s_max, out = oracle_chain(case, B, ref)
    tr = hint_amd.FlowTrainer(flow, noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    chain = tr._chain_for(B)
    assert_dispatch(case, lib, tr.engines[0].plan, B)
    st = torch.cuda.current_stream().cuda_stream
    xd = x.to(DEV)
    cd = c.to(DEV) if case.dc else None
    cp = cd.data_ptr() if case.dc else None
    z, J = torch.empty_like(xd), torch.empty(B, device=DEV)
    _lib.check(lib.hint_chain_forward(chain, xd.data_ptr(), cp, z.data_ptr(), J.data_ptr(), None, None, st), "hint_chain_forward")
    gx = torch.empty_like(xd)
    gc = torch.zeros_like(cd) if case.dc else None
    gzd, gJd = gz.to(DEV).contiguous(), gJ.to(DEV).contiguous()
    _lib.check(lib.hint_chain_backward(chain, xd.data_ptr(), cp, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(),
                                       gc.data_ptr() if case.dc else None, 1.0, 0.0, 0, st), "hint_chain_backward")
    torch.cuda.synchronize()
    check_fwd("z", z, out["z"])
    check_fwd("J", J, out["J"])
    gw = {}
    for bi, ((a, b), eng) in enumerate(zip(tr.slices, tr.engines)):
        for p, g in zip(eng.params, eng.split_flat(tr.G[a:b])):
            name = [n for n, q in flow.blocks[bi].named_parameters() if q is p][0]
            gw[(bi, name)] = g
    check_grads(case.name, gx, gc, gw, out)
    with torch.no_grad():
        xi, Ji = tr.sample(zi.to(DEV), cd)
    check_fwd("inverse x", xi, out["xi"])
    check_fwd("inverse J", Ji, out["Ji"])
    return keep, s_max


BIG = {c.name for c in CASES if c.B(256) > 20000}


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.timeout(600)) if c.name in BIG else c for c in CASES],
                         ids=[c.name for c in CASES])
def test_instance_vs_oracle(case, monkeypatch):
    torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 oracle: a GPU box has many host cores)
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    knob_env(monkeypatch, lib, case.knobs)           # (before the plan is made: some knobs are read by the planner)
    try:
        keep, s_max = (run_chain if case.entry == "chain" else run_block)(case, lib, cu)
    finally:
        monkeypatch.undo()
        lib.hint_debug_reload_knobs()
    B = keep.numel()
    dropped = B - int(keep.sum())
    print(f"{case.name}: {dropped} of {B} rows next to a ReLU kink (zero cotangents); max |s| {float(s_max.max()):.1f}")
    assert dropped <= case.kink_cap * B, f"{dropped} of {B} rows next to a ReLU kink (cap {case.kink_cap:.0%})"
    if case.big_s:
        assert float((s_max >= 10).double().mean()) >= 0.01, "big_s case: too few rows with |s| >= 10"
