"""ConditionalFlowTrainer's fast path at the lane pairings the other conditional tests do not run: a wave-local x lane (its
hint_block_backward_rows, its own x_in in the gathered part B, the lean part B that rebuilds a1 from x_in), a y lane on the general
kernels (ndim_y >= 9: the conditions' gradients enter through `g_add` in hint_bwd.hip instead of hint_wl_bwd.hip), and both lanes
wave-local - each at 37 rows and at a batch past 16 rows per CU, eager and as one graph replay.

hint_plan_dispatch on the three plans (hac_x, ac_y_to_x, ac_y) must show the declared families before anything is compared.  Then
one step against OracleComposition in float64 with the method, the kink-free pool and the tolerances of
test_conditional_trainer_gradient_at_4096_rows (assert_step_matches_oracle): the loss pair, x_jac, and every parameter tensor's
gradient read out of Adam's first moment (beta1 = 0, lr = 0, no clamp, no decay)."""
import functools

import pytest
import torch

import hint_amd
from hint_amd import _lib
from instance_cases import plan_dispatch
from test_gpu_chain_workloads import KINK
from test_gpu_conditional import OracleComposition, assert_step_matches_oracle
from test_gpu_instances import Spy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (nx, ny, blocks, hidden) -> per batch kind the dispatch fields each plan must show
SHAPES = {
    (6, 10, 2, 24): dict(       # x lane wave-local, y lane general with g_add
        small=dict(hac_x=dict(wl=1, nr=1), ac_y_to_x=dict(wl=0), ac_y=dict(wl=0, fwd=1, bwd=2, dw_small=1, dw_wide=1)),
        large=dict(hac_x=dict(wl=1, nr=2), ac_y_to_x=dict(wl=0), ac_y=dict(wl=0, fwd=1, bwd=2, dw_small=1, dw_wide=1, alt4=1))),
    (12, 10, 3, 32): dict(      # x lane FLY (n3 on the 4-wavefront variant at the larger B), y lane general
        small=dict(hac_x=dict(wl=0, fwd=2, bwd=3, alt4=0), ac_y_to_x=dict(wl=0), ac_y=dict(wl=0, bwd=2)),
        large=dict(hac_x=dict(wl=0, fwd=1, bwd=2, alt4=1), ac_y_to_x=dict(wl=0), ac_y=dict(wl=0, bwd=2, alt4=1))),
    (8, 2, 2, 32): dict(        # both lanes wave-local
        small=dict(hac_x=dict(wl=1, nr=1), ac_y_to_x=dict(wl=0), ac_y=dict(wl=1, nr=1)),
        large=dict(hac_x=dict(wl=1, nr=2), ac_y_to_x=dict(wl=0), ac_y=dict(wl=1, nr=2))),
}


def batch(kind, cu):
    return 37 if kind == "small" else 16 * cu + 37


def make_model(shape):
    nx, ny, nb, hidden = shape
    torch.manual_seed(2)
    m = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            p.data = 0.07 * torch.randn(p.shape, generator=g)
    return m.to(DEV)


@functools.lru_cache(maxsize=2)
def reference(shape, B):
    """the float64 composition's step on B kink-free rows (shared by the eager and the graph case): x, y, the loss pair, x_jac and the
    parameters with their gradients"""
    nx, ny, nb, hidden = shape
    comp = OracleComposition(make_model(shape), dtype=torch.float64)
    POOL = B + B // 8 + 64
    g = torch.Generator().manual_seed(6)
    xp, yp = torch.randn(POOL, nx, generator=g), torch.randn(POOL, ny, generator=g)
    with torch.no_grad(), Spy(POOL) as spy:
        comp.forward(xp, yp)
    keep = torch.nonzero(spy.kink > KINK).flatten()
    assert keep.numel() >= B, f"only {keep.numel()} of {POOL} rows off the kinks"
    print(f"conditional lanes {shape} B={B}: {POOL - keep.numel()} of {POOL} pool rows next to a ReLU kink")
    x, y = xp[keep[:B]].contiguous(), yp[keep[:B]].contiguous()
    xo, yo, jx, jy, _ = comp.forward(x, y)
    z = torch.cat([xo, yo], dim=-1)
    l0, l1 = 0.5 * torch.sum(z ** 2, dim=1).mean(), -(jx + jy).mean()      # train_conditional.py:132-143
    (l0 + l1).backward()
    return x, y, l0.detach(), l1.detach(), jx.detach(), comp.P


CASES = [(s, k, g) for s in SHAPES for k in ("small", "large") for g in (False, True)]


@pytest.mark.parametrize("shape,kind,use_graph", CASES,
                         ids=[f"x{s[0]}-y{s[1]}-{k}-{'graph' if g else 'eager'}" for s, k, g in CASES])
def test_conditional_step_on_lane_pairing(shape, kind, use_graph):
    torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 oracle: a GPU box has many host cores)
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = batch(kind, cu)
    m = make_model(shape)
    for name, mod in (("hac_x", m.hac_x[0]), ("ac_y_to_x", m.ac_y_to_x[0]), ("ac_y", m.ac_y[0])):
        disp = plan_dispatch(lib, mod.tree.engine(torch.device(DEV)).plan, B)
        want = SHAPES[shape][kind][name]
        got = {k: disp[k] for k in want}
        print(f"{shape} B={B} on {disp['num_cu']} CUs: {name} wl={disp['wl']} nr={disp['nr']} alt4={disp['alt4']} fwd={disp['fwd']} bwd={disp['bwd']} "
              f"dw=<{disp['dw_small']},{disp['dw_wide']}>")
        assert got == want, (shape, B, name, got, want)
    x, y, l0, l1, jx, Po = reference(shape, B)
    mods = []
    for i in range(shape[2]):
        mods += [(f"hac_x.{i}", m.hac_x[i], 0), (f"ac_y_to_x.{i}", m.ac_y_to_x[i], shape[1]), (f"ac_y.{i}", m.ac_y[i], 0)]
    tr = hint_amd.ConditionalFlowTrainer(m, noise=0.0, use_graph=use_graph, lr=0.0, betas=(0.0, 0.95), weight_decay=0.0, grad_clamp=0.0)
    w0 = tr.P.clone()
    g0, g1 = tr.step(x.to(DEV), y.to(DEV))
    assert (tr._graph is not None) == use_graph
    total = assert_step_matches_oracle(tr, mods, Po, (g0, g1), l0, l1, jx)
    print(f"{shape} B={B} {'graph' if use_graph else 'eager'}: all gradients together {total:.2e} of their norm (bound 1e-4)")
    assert torch.equal(tr.P, w0)                          # lr = 0: the weights did not move
