"""The level schedule folded into the shape-specialised wave-local instances (hint_amd/csrc/hint_wl_shape.hpp WlSched: the group
loop unrolled over the shape's group list, a group's k-blocks, tile counts, entry and slot counts and slabs per net as constants)
against the dynamic instances, bit for bit, on the shapes tests/test_gpu_wl_static.py does not run - the smallest at which those
constants can be wrong:
  * a ONE-block chain on cfg 2's tree (no next block: the hand-over record behind the block's last group, `wrap` / `has_next`),
    at B = 1 and B = 17;
  * an 8-block chain at B = 16 and B = 17 (the slab-set phase and the parameter double buffer across many blocks);
  * GAS's tree (three groups per block: the slab set alternates across blocks) with row pairs at B = 17 and B = 33, one and three
    blocks.
Every block has its fixed permutation.  Compared with HINT_WL_STATIC on and off (knobs re-read in between): z, J, the loss sums,
g_x, the whole tape, the whole backward workspace after the reduction and the flat gradient.  No tolerance.  Each case asserts
through hint_debug_last_wl_shape that the static instances ran."""
import pytest
import torch

import hint_amd
from hint_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREES = {"cfg2": dict(d=6, widths=[140, 70, 35, 17], shape=0, nr=None),
         "gas": dict(d=8, widths=[128, 64, 32, 16], shape=1, nr="2")}
CASES = [("cfg2", 1, 1), ("cfg2", 1, 17), ("cfg2", 8, 16), ("cfg2", 8, 17),
         ("gas", 1, 17), ("gas", 1, 33), ("gas", 3, 17), ("gas", 3, 33)]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture()
def knobs(monkeypatch):
    lib = _lib.load()

    def set_knobs(tree, static):
        monkeypatch.setenv("HINT_WL_STATIC", "1" if static else "0")
        if TREES[tree]["nr"]:
            monkeypatch.setenv("HINT_WL_NR", TREES[tree]["nr"])
        else:
            monkeypatch.delenv("HINT_WL_NR", raising=False)
        lib.hint_debug_reload_knobs()

    yield set_knobs
    monkeypatch.undo()
    lib.hint_debug_reload_knobs()


def make_flow(tree, n_blocks, seed=9):
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


@pytest.mark.parametrize("tree,n_blocks,B", CASES, ids=[f"{t}-{n}blocks-B{B}" for t, n, B in CASES])
def test_folded_schedule_agrees_with_the_dynamic_instances_bit_for_bit(tree, n_blocks, B, knobs):
    lib = _lib.load()
    knobs(tree, True)
    tr = hint_amd.FlowTrainer(make_flow(tree, n_blocks), noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    x = torch.randn(B, TREES[tree]["d"], generator=torch.Generator().manual_seed(23 + B)).to(DEV)
    got, took = run_chain(tr, lib, x)
    assert took == (TREES[tree]["shape"],) * 2, f"the static instances did not run: {took}"
    knobs(tree, False)
    ref, took = run_chain(tr, lib, x)
    assert took == (-1, -1), f"HINT_WL_STATIC=0 still ran a static instance: {took}"
    assert torch.isfinite(ref["z"]).all() and torch.isfinite(ref["grad"]).all() and float(ref["grad"].abs().max()) > 0
    for k in ref:
        assert torch.equal(got[k].view(torch.uint8).reshape(-1), ref[k].view(torch.uint8).reshape(-1)), f"{k} differs"
