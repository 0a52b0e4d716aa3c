"""The shape-specialised wave-local instances (hint_amd/csrc/hint_wl_shape.hpp) against the dynamic ones, bit for bit: the same
launches with HINT_WL_STATIC on and off (knobs re-read in between) on cfg 2's tree - chains of 2 and 3 blocks with a fixed
permutation in front of every block - and on GAS's tree with row pairs forced (HINT_WL_NR=2, batches whose last pair has its
second tile behind the batch).  Compared: z, J, the loss sums, g_x, the whole tape, the whole backward workspace (coupling
gradients, part B's slabs and the backward kernel's dW1 | db1 slabs as the reduction leaves them) and the flat gradient; then
three FlowTrainer steps, eager and as graph replays: parameters and loss pairs.  No tolerance: the dynamic instances are checked
against the float64 oracle by the rest of the suite, these tests tie the static ones to them.  hint_debug_last_wl_shape says
which instance a launch took."""
import pytest
import torch

import hint_amd
from hint_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREES = {"cfg2": dict(d=6, widths=[140, 70, 35, 17], shape=0, nr=None),
         "gas": dict(d=8, widths=[128, 64, 32, 16], shape=1, nr="2")}
CHAIN_CASES = [("cfg2", n, B) for n in (2, 3) for B in (1, 16, 17, 33, 272)] + [("gas", 2, B) for B in (17, 33, 48)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def set_knobs(mp, lib, tree, static):
    mp.setenv("HINT_WL_STATIC", "1" if static else "0")
    if TREES[tree]["nr"]:
        mp.setenv("HINT_WL_NR", TREES[tree]["nr"])
    else:
        mp.delenv("HINT_WL_NR", raising=False)
    lib.hint_debug_reload_knobs()


@pytest.fixture()
def knobs(monkeypatch):
    lib = _lib.load()
    yield lambda tree, static: set_knobs(monkeypatch, lib, tree, static)
    monkeypatch.undo()
    lib.hint_debug_reload_knobs()


def make_flow(tree, n_blocks, seed=5):
    t = TREES[tree]
    flow = hint_amd.HintFlow(t["d"], n_blocks, list(t["widths"]), perm_first=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in flow.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return flow.to(DEV)


def run_chain(tr, lib, x):
    """one chained training forward + backward through the C entry points on zeroed buffers; everything they wrote"""
    B = x.shape[0]
    chain = tr._chain_for(B)
    tapes, wsb, _ = tr._chains[B][2]
    for t in (tapes, wsb, tr.G, tr.loss_acc):
        t.zero_()
    z, J, gx = torch.empty_like(x), torch.empty(B, dtype=torch.float32, device=DEV), torch.empty_like(x)
    _lib.check(lib.hint_chain_forward_noisy(chain, x.data_ptr(), None, z.data_ptr(), J.data_ptr(), None, tr.loss_acc.data_ptr(),
                                            0.0, None, None, stream()), "hint_chain_forward_noisy")
    fwd = lib.hint_debug_last_wl_shape(0)
    _lib.check(lib.hint_chain_backward(chain, x.data_ptr(), None, z.data_ptr(), None, gx.data_ptr(), None, 1.0 / B, -1.0 / B, 1,
                                       stream()), "hint_chain_backward")
    bwd = lib.hint_debug_last_wl_shape(1)
    torch.cuda.synchronize()
    out = dict(z=z, J=J, loss=tr.loss_acc.clone(), g_x=gx, tape=tapes.clone(), workspace=wsb.clone(), grad=tr.G.clone())
    return out, (fwd, bwd)


@pytest.mark.parametrize("tree,n_blocks,B", CHAIN_CASES, ids=[f"{t}-{n}blocks-B{B}" for t, n, B in CHAIN_CASES])
def test_static_and_dynamic_instances_agree_bit_for_bit(tree, n_blocks, B, knobs):
    lib = _lib.load()
    knobs(tree, True)
    tr = hint_amd.FlowTrainer(make_flow(tree, n_blocks), noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    x = torch.randn(B, TREES[tree]["d"], generator=torch.Generator().manual_seed(11 + B)).to(DEV)
    got, took = run_chain(tr, lib, x)
    assert took == (TREES[tree]["shape"],) * 2, f"the static instances did not run: {took}"
    knobs(tree, False)
    ref, took = run_chain(tr, lib, x)
    assert took == (-1, -1), f"HINT_WL_STATIC=0 still ran a static instance: {took}"
    assert torch.isfinite(ref["z"]).all() and torch.isfinite(ref["grad"]).all() and float(ref["grad"].abs().max()) > 0
    for k in ref:
        assert torch.equal(got[k].view(torch.uint8).reshape(-1), ref[k].view(torch.uint8).reshape(-1)), f"{k} differs"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("tree", list(TREES))
def test_trainer_steps_agree_bit_for_bit(tree, use_graph, knobs):
    lib = _lib.load()
    d = TREES[tree]["d"]
    xs = [torch.randn(33, d, generator=torch.Generator().manual_seed(70 + i)).to(DEV) for i in range(3)]
    runs = []
    for static in (True, False):
        knobs(tree, static)
        tr = hint_amd.FlowTrainer(make_flow(tree, 2), noise=0.01, use_graph=use_graph, seed=2 ** 40 + 3)
        losses = []
        for x in xs:
            l0, l1 = tr.step(x)
            losses.append(torch.stack([l0, l1]).clone())
        torch.cuda.synchronize()
        took = (lib.hint_debug_last_wl_shape(0), lib.hint_debug_last_wl_shape(1))
        want = TREES[tree]["shape"] if static else -1
        assert took == (want, want), (static, took)
        runs.append((tr.P.clone(), torch.stack(losses)))
    assert torch.isfinite(runs[1][0]).all() and torch.isfinite(runs[1][1]).all()
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "parameters differ"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), "loss pairs differ"
