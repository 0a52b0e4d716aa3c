"""GPU tests of FlowTrainer(learned_perms=True): the block-by-block route that trains a HintFlow's HouseholderPerms.

What is compared with what, and why the tolerance:
  block gradients   the block slices of G and the loss pair against FlowTrainer(use_chain=False) on the fixed twin
                    (FixedOrthogonal(W=perm.matrix())): the same block kernels on the same inputs, so bit for bit
  Vs gradients      against Vs.grad of the module route (loss.backward() on the same flow and batch) and against the float64
                    statement (householder_oracle.g_V_from_g_W) on the float64 Gram of the GPU's own h_(j-1) and g(x_j):
                    rel_err < 1e-4, the project's gradient tolerance
  ten steps         against the module route with ClampAdam from the same start and batches: loss pairs within 1e-3 relative,
                    final Vs and weights rel_err < 1e-3, |W W^T - I|_max < 1e-5 - the tolerances of test_gpu_householder.py's
                    ten-step test and of the conditional session test
Shapes: HintFlow(20, 2, [32, 16]), HintFlow(6, 3, [32, 16]) (wave-local kernels), HintFlow(20, 3, [32, 16], ndim_c=2) and one
with perm_first=True; B = 64 (one row tile group) and 272 (a ragged second slab of the Gram); noise = 0 unless stated."""
import copy

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd._lib import HintAmdError
import householder_oracle as ho
from guarded import bits_equal
from test_gpu_householder import DEV, fixed_twin
from util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = {
    "d20": ((20, 2, [32, 16]), {}),
    "wave_local": ((6, 3, [32, 16]), {}),
    "conditional": ((20, 3, [32, 16]), {"ndim_c": 2}),
    "perm_first": ((20, 2, [32, 16]), {"perm_first": True}),
}
BATCHES = (64, 272)
ADAM = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)


def make(shape, learned=True, seed=0):
    args, kw = SHAPES[shape]
    torch.manual_seed(seed)
    return hint_amd.HintFlow(*args, learned_perms=learned, **kw).to(DEV)


def batch(shape, B, seed=0, K=None):
    args, kw = SHAPES[shape]
    g = torch.Generator().manual_seed(100 + seed)
    lead = (B,) if K is None else (K, B)
    x = torch.randn(*lead, args[0], generator=g).to(DEV)
    c = torch.randn(*lead, kw["ndim_c"], generator=g).to(DEV) if kw.get("ndim_c") else None
    return x, c


def trainer(flow, **kw):
    kw = dict(dict(noise=0.0, seed=11, learned_perms=True, **ADAM), **kw)
    return hint_amd.FlowTrainer(flow, grad_clamp=5.0, **kw)


def grab_gradients(t, x, c):
    """one un-captured step -> (G before the optimizer, the loss pair, what the backward pass saw at the trainable boundaries)"""
    got = {}

    def hook(tr):
        got["G"] = tr.G.clone()
        got["seen"] = [(j, h.clone(), g.clone()) for j, h, g in (tr._lp_seen or [])]
    t._grad_hook = hook
    l0, l1 = t.step(x, c)
    t._grad_hook = None
    return got["G"], (l0.clone(), l1.clone()), got["seen"]


def module_loss(flow, x, c):
    z = flow(x, c=c)
    J = flow.log_jacobian(run_forward=False)
    return 0.5 * torch.sum(z ** 2, dim=1).mean(), -J.mean()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradients_of_blocks_and_permutations(shape, B):
    flow = make(shape)
    args, kw = SHAPES[shape]
    module = copy.deepcopy(flow)
    twin = fixed_twin(flow, lambda: hint_amd.HintFlow(*args, **kw))
    x, c = batch(shape, B)
    t = trainer(flow, use_graph=False)
    n_blocks_floats = t.perm_base
    assert t.n_floats == n_blocks_floats + len(t.perm_mods) * t.perm_stride and len(t.perm_mods) == len(t._lp) > 0
    G, loss, seen = grab_gradients(t, x, c)
    # the blocks: the fixed route's kernels on the same inputs
    tw = hint_amd.FlowTrainer(twin, grad_clamp=5.0, noise=0.0, seed=11, use_graph=False, use_chain=False, **ADAM)
    assert tw.n_floats == n_blocks_floats and tw.slices == t.slices       # block offsets do not move
    Gf, lossf, _ = grab_gradients(tw, x, c)
    assert bits_equal(G[:n_blocks_floats], Gf) and bool(G[:n_blocks_floats].abs().sum() > 0)
    assert bits_equal(loss[0], lossf[0]) and bits_equal(loss[1], lossf[1])
    # the permutations, against the module route ...
    sum(module_loss(module, x, c)).backward()
    trainable = [p for p in module.perms if isinstance(p, hint_amd.HouseholderPerm)]
    assert len(trainable) == len(t.perm_mods) == len(seen)
    for j, p in enumerate(trainable):
        got = t.perm_slice(j, G)
        e = rel_err(got.cpu().numpy(), p.Vs.grad.cpu().numpy())
        print(f"{shape} B {B} permutation {j}: Vs gradient rel_err to the module route {e:.3g}")
        assert e < 1e-4, (j, e)
    # ... and against the float64 statement on the Gram of what the GPU saw at the boundary
    for j, h, gx in seen:
        G64 = h.double().cpu().t() @ gx.double().cpu()
        want = ho.g_V_from_g_W(trainable[j].Vs.detach().cpu(), G64)
        e = rel_err(t.perm_slice(j, G).cpu().numpy(), want.numpy())
        print(f"{shape} B {B} permutation {j}: Vs gradient rel_err to float64 {e:.3g}")
        assert e < 1e-4, (j, e)
    # the floats between two Vs slices carry no gradient
    for j in range(len(trainable)):
        a = t.perm_base + j * t.perm_stride
        assert not bool(G[a + trainable[j].Vs.numel():a + t.perm_stride].any())


@pytest.mark.parametrize("shape,B", [("d20", 64), ("wave_local", 272), ("conditional", 64), ("perm_first", 272)])
def test_ten_steps_against_the_module_route_with_clamp_adam(shape, B):
    flow = make(shape, seed=4)
    module = copy.deepcopy(flow)
    batches = [batch(shape, B, seed=s) for s in range(10)]
    t = trainer(flow)
    params = [p for p in module.parameters() if p.requires_grad]
    optim = hint_amd.ClampAdam(params, grad_clamp=5.0, **ADAM)
    hist = [[], []]
    for x, c in batches:
        hist[0].append([float(v) for v in t.step(x, c)])
        optim.zero_grad()
        pair = module_loss(module, x, c)
        hist[1].append([float(v.detach()) for v in pair])
        sum(pair).backward()
        optim.step()
    np.testing.assert_allclose(np.array(hist[0]), np.array(hist[1]), rtol=1e-3, atol=0)
    a, b = dict(flow.named_parameters()), dict(module.named_parameters())
    assert a.keys() == b.keys() and any("Vs" in k for k in a)
    for k in a:
        e = rel_err(a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy())
        assert e < 1e-3, (k, e)
    d = flow.ndim_x
    for i, p in enumerate(flow.perms):
        if isinstance(p, hint_amd.HouseholderPerm):
            assert not torch.equal(p.Vs.detach(), make(shape, seed=4).perms[i].Vs.detach())      # it was trained
            W = p.matrix().double()
            assert float((W @ W.t() - torch.eye(d, dtype=torch.float64, device=DEV)).abs().max()) < 1e-5


@pytest.mark.parametrize("shape", ["d20", "wave_local", "conditional"])
def test_graph_eager_step_many_and_fit_epoch_give_the_same_bits(shape):
    """noise = 0.01 from one seed: the captured iteration, the un-captured one, step_many(K = 3) and fit_epoch over the same
    batches leave the same bits in P"""
    B = 64
    start = make(shape, seed=7)
    xs, cs = batch(shape, B, seed=3, K=3)
    ends = {}
    for name in ("graph", "eager", "many", "again"):
        flow = copy.deepcopy(start)
        t = trainer(flow, noise=0.01, seed=5, use_graph=name != "eager")
        if name == "many":
            t.step_many(xs, cs)
            assert t.step_losses().shape == (3, 2) and bool(torch.isfinite(t.step_losses()).all())
        else:
            for k in range(3):
                t.step(xs[k], cs[k] if cs is not None else None)
        assert t.step_count == 3
        ends[name] = t.P.clone()
        if name == "graph":
            assert t._graph is not None and t._adam_in_graph       # the optimizer is inside the one replay
    for name in ("eager", "many", "again"):
        assert bits_equal(ends[name], ends["graph"]), name
    assert not bits_equal(ends["graph"], trainer(copy.deepcopy(start)).P)
    # fit_epoch on five batches against the same batches stepped by hand
    args, kw = SHAPES[shape]
    g = torch.Generator().manual_seed(9)
    rows = torch.randn(5 * B, args[0], generator=g).to(DEV)
    ys = torch.randn(5 * B, kw["ndim_c"], generator=g).to(DEV) if kw.get("ndim_c") else None
    data = hint_amd.DeviceDataset(rows, ys, seed=3)
    a, b = trainer(copy.deepcopy(start), noise=0.01, seed=5), trainer(copy.deepcopy(start), noise=0.01, seed=5)
    losses = a.fit_epoch(data, 0, B, chunk=2)
    assert losses.shape == (5, 2)
    by_hand = []
    for k in range(5):
        got = data.gather(0, k, 1, B)
        x, c = (got[0][0], got[1][0]) if isinstance(got, tuple) else (got[0], None)
        by_hand.append(torch.stack(tuple(b.step(x, c))))
    assert bits_equal(a.P, b.P) and bits_equal(losses, torch.stack(by_hand))


def test_views_state_dict_sample_and_evaluate():
    flow = make("conditional", seed=2)
    v0 = [p.Vs.detach().clone() for p in flow.perms if isinstance(p, hint_amd.HouseholderPerm)]
    t = trainer(flow)
    for j, m in enumerate(t.perm_mods):
        a = t.perm_base + j * t.perm_stride
        assert m.Vs.data_ptr() == t.P.data_ptr() + 4 * a and bits_equal(m.Vs.detach(), v0[j])      # a view of its P slice
        assert a >= t.slices[-1][1]                                                               # behind every block slice
    for s in range(3):
        t.step(*batch("conditional", 64, seed=s))
    sd = flow.state_dict()
    assert bits_equal(sd["perms.1.Vs"], t.perm_slice(0)) and not bits_equal(sd["perms.1.Vs"], v0[0])
    assert bits_equal(sd["perms.2.Vs"], t.perm_slice(1)) and not bits_equal(sd["perms.2.Vs"], v0[1])
    z, c = batch("conditional", 64, seed=20)
    x, J = t.sample(z, c)
    with torch.no_grad():
        want = flow(z, c=c, rev=True)
        assert bits_equal(x, want) and bits_equal(J, flow.log_jacobian(rev=True, run_forward=False))
        rows, ys = batch("conditional", 128, seed=21)
        got = t.evaluate(hint_amd.DeviceDataset(rows, ys, shuffle=False), batch_size=64, noise=0.0)
        pairs = [torch.stack(module_loss(flow, rows[a:a + 64], ys[a:a + 64])) for a in (0, 64)]
    assert rel_err(got.cpu().numpy(), torch.stack(pairs).mean(dim=0).cpu().numpy()) < 1e-5
    # the lr setter reaches the captured optimizer: a zero rate leaves P (without weight decay's share: lr scales both) as it is
    t.lr = 0.0
    before = t.P.clone()
    t.step(*batch("conditional", 64, seed=4))
    assert bits_equal(t.P, before) and t.lr == 0.0
    bufs = t.input_buffers(*batch("conditional", 64, seed=5))
    assert bufs[0].data_ptr() == t._static["x"].data_ptr() and bufs[1].data_ptr() == t._static["c"].data_ptr()
    assert t.input_buffers_many(*batch("conditional", 64, seed=5, K=2))[0].shape == (2, 64, 20)


@pytest.mark.parametrize("use_graph", [False, True])
def test_rebinding_and_load_state_dict_are_picked_up_by_the_next_step(use_graph):
    start = make("d20", seed=3)
    new = ho.init_Vs(20, 20, seed=99).to(DEV)
    x, c = batch("d20", 64)
    # the reference: a trainer whose flow held the new Vs from the start, stepped once behind one step on the old values'
    # weights - built by replaying the same two steps with the new values written in place between them
    ends = []
    for how in ("in_place", "rebind", "load_state_dict"):
        flow = copy.deepcopy(start)
        t = trainer(flow, use_graph=use_graph)
        t.step(x, c)
        if how == "in_place":
            with torch.no_grad():
                flow.perms[1].Vs.copy_(new)
        elif how == "rebind":
            flow.perms[1].Vs.data = new.clone()
            assert flow.perms[1].Vs.data_ptr() != t.perm_slice(0).data_ptr()
        else:
            sd = {k: v.clone() for k, v in flow.state_dict().items()}
            sd["perms.1.Vs"] = new.clone()
            flow.load_state_dict(sd)
        t.step(x, c)
        assert flow.perms[1].Vs.data_ptr() == t.perm_slice(0).data_ptr()          # pulled back into the arena
        ends.append(t.P.clone())
    assert bits_equal(ends[1], ends[0]) and bits_equal(ends[2], ends[0])
    plain = trainer(copy.deepcopy(start), use_graph=use_graph)
    plain.step(x, c)
    plain.step(x, c)
    assert not bits_equal(plain.P, ends[0])                                       # (the new values made a difference)


def pointers(flow):
    return [p.data_ptr() for p in flow.parameters()]


def test_refusals_come_before_any_launch_and_the_switch_changes_nothing_on_a_fixed_flow():
    flow = make("d20")
    before = pointers(flow)
    with pytest.raises(HintAmdError, match="ClampAdam"):
        hint_amd.FlowTrainer(flow)                                                # the default: as it was
    with pytest.raises(HintAmdError, match="learned_perms"):
        hint_amd.FlowTrainer(flow, learned_perms=False)
    with pytest.raises(HintAmdError, match="reshuffle"):
        torch.manual_seed(0)
        shuffled = hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True, reshuffle=True).to(DEV)
        ptrs = pointers(shuffled)
        try:
            hint_amd.FlowTrainer(shuffled, learned_perms=True)
        finally:
            assert pointers(shuffled) == ptrs                                     # no arena was built: nothing was launched
    ragged = make("wave_local")
    ragged.perms[2] = hint_amd.HouseholderPerm([(6,)], n_reflections=3, seed=8).to(DEV)
    ptrs = pointers(ragged)
    with pytest.raises(HintAmdError, match="n_reflections"):
        hint_amd.FlowTrainer(ragged, learned_perms=True)
    assert pointers(ragged) == ptrs and pointers(flow) == before
    with pytest.raises(HintAmdError, match="ClampAdam"):
        hint_amd.ConditionalFlowTrainer(hint_amd.ConditionalHintFlow(20, 2, 2, 32, learned_perms=True).to(DEV))
    # learned_perms=True on a flow without trainable permutations is the default trainer, bit for bit
    start = make("conditional", learned=False, seed=6)
    ends = []
    for switch in (False, True):
        t = hint_amd.FlowTrainer(copy.deepcopy(start), noise=0.01, seed=5, learned_perms=switch)
        assert t._chainable and not t._lp and t.n_floats == t.slices[-1][1]
        for s in range(3):
            t.step(*batch("conditional", 64, seed=s))
        ends.append(t.P.clone())
    assert bits_equal(ends[0], ends[1])
    # ... and so is one whose permutations are all fixed=True HouseholderPerms
    frozen = make("d20", seed=6)
    frozen.perms[1].Vs.requires_grad_(False)
    t = hint_amd.FlowTrainer(frozen, noise=0.0, seed=5, learned_perms=True)
    assert t._chainable and not t._lp
    t.step(*batch("d20", 64))
