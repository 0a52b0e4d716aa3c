"""The thin widths folded into the per-tile epilogues of the shape-specialised wave-local instances (hint_amd/csrc/hint_wl.hpp
wl_row: the forward's thin product and fold only for the unit's r outputs, the backward's pre-activation, product and fold only
for its cin inputs) against the dynamic instances, bit for bit:
  * cfg 2's tree [140, 70, 35, 17], d = 6 (leaves cin 1 / r 2, root 3 / 3), one block at B = 1 and B = 17;
  * the same tree, 8 blocks with a permutation per block, at B = 16;
  * GAS's tree [128, 64, 32, 16], d = 8 (4 / 4, 2 / 2, 1 / 1; two tiles in every row), 3 blocks with row pairs at B = 17 and 33;
  * cfg 2's one-block chain at B = 17 with one input row holding inf and one holding NaN: what the static instances no longer
    compute is `0-vector * 0.f` added to a pre-activation and results in slab components no coupling entry addresses, so
    non-finite rows must come out identically too - NaN positions and payloads included.
Compared with HINT_WL_STATIC on and off (knobs re-read in between): z, J, the loss sums, g_x, the whole tape, the whole backward
workspace after the reduction and the flat gradient, as bytes.  Every case asserts through hint_debug_last_wl_shape that the
static instances ran."""
import pytest
import torch

import hint_amd
from hint_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREES = {"cfg2": dict(d=6, widths=[140, 70, 35, 17], shape=0, nr=None),
         "gas": dict(d=8, widths=[128, 64, 32, 16], shape=1, nr="2")}
CASES = [("cfg2", 1, 1), ("cfg2", 1, 17), ("cfg2", 8, 16), ("gas", 3, 17), ("gas", 3, 33)]


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


def make_flow(tree, n_blocks, seed=11):
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


def static_and_dynamic(tree, n_blocks, x, knobs):
    lib = _lib.load()
    knobs(tree, True)
    tr = hint_amd.FlowTrainer(make_flow(tree, n_blocks), noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    got, took = run_chain(tr, lib, x)
    assert took == (TREES[tree]["shape"],) * 2, f"the static instances did not run: {took}"
    knobs(tree, False)
    ref, took = run_chain(tr, lib, x)
    assert took == (-1, -1), f"HINT_WL_STATIC=0 still ran a static instance: {took}"
    return got, ref


def assert_same_bytes(got, ref):
    for k in ref:
        assert torch.equal(got[k].view(torch.uint8).reshape(-1), ref[k].view(torch.uint8).reshape(-1)), f"{k} differs"


@pytest.mark.parametrize("tree,n_blocks,B", CASES, ids=[f"{t}-{n}blocks-B{B}" for t, n, B in CASES])
def test_folded_thin_widths_agree_with_the_dynamic_instances_bit_for_bit(tree, n_blocks, B, knobs):
    x = torch.randn(B, TREES[tree]["d"], generator=torch.Generator().manual_seed(41 + B)).to(DEV)
    got, ref = static_and_dynamic(tree, n_blocks, x, knobs)
    assert torch.isfinite(ref["z"]).all() and torch.isfinite(ref["grad"]).all() and float(ref["grad"].abs().max()) > 0
    assert_same_bytes(got, ref)


def test_non_finite_rows_agree_bit_for_bit(knobs):
    B, d = 17, TREES["cfg2"]["d"]
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(41 + B))
    x[3, 1] = float("inf")          # a lane that feeds the root's subnets (upper half) ...
    x[16, 4] = float("nan")         # ... and, in the second row tile, one of the transformed half
    got, ref = static_and_dynamic("cfg2", 1, x.to(DEV), knobs)
    # the case is what it says: the poisoned rows are non-finite in the reference, the others are not
    zf = torch.isfinite(ref["z"]).all(dim=1).cpu()
    assert not zf[3] and not zf[16] and zf[[i for i in range(B) if i not in (3, 16)]].all()
    assert not torch.isfinite(ref["grad"]).all()
    assert_same_bytes(got, ref)
