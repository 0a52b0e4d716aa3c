"""GPU tests of hint_amd.ClampAdam and hint_adam_multi_step: bit identity with the flat-arena kernel, segments of every
alignment between guard bands, the reference loop's golden trajectory with the optimizer swapped in, and the optimizer
contract (schedulers, skipped parameters, state exchange with torch.optim.Adam, rebound storage, the pack cache)."""
import copy
import ctypes as C
import io

import numpy as np
import pytest
import torch

import hint_amd
from guarded import NAN_BITS, bits_equal
from hint_amd import _lib
from hint_amd import hint as H
from test_gpu_flow import build_flow, check_update
from util import CHAIN_CASES, load_chain_case, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.01 * 3e-2, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)         # train_unconditional.py:174-176

# ClampAdam against clamp loop + torch.optim.Adam on a whole model (tests 7, 8, 9, 11): per-tensor rel_err of the weights.
# Noise floor of that comparison without the code under test - the same loop under torch.optim.Adam(foreach=True) against
# torch.optim.Adam(foreach=False), 12 steps of test_matches_torch_adam_with_scheduler_and_skipped_block, which prints it:
# FLOOR_MEASURED below.  The bound is 4x that floor (ClampAdam differs from torch in fused-multiply-add contraction on top of
# what torch's two paths differ in) or 1e-5, whichever is larger.
FLOOR_MEASURED = 7.3e-8         # measured on an MI355X (ClampAdam against torch in the same run: 7.3e-8; tests 8 and 11: 1.1e-7)
MODEL_TOL = max(4 * FLOOR_MEASURED, 1e-5)


def multi_create(segs):
    lib = _lib.load()
    arr = (_lib.AdamSeg * max(len(segs), 1))()
    for i, (p, g, m, v, n) in enumerate(segs):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p, g, m, v, n
    h = C.c_void_p()
    _lib.check(lib.hint_adam_multi_create(arr, len(segs), C.byref(h)), "hint_adam_multi_create")
    return h


@pytest.mark.timeout(120)
def test_multi_step_is_bit_identical_to_flat_arena_step():
    """one 16-byte aligned segment of 10007 floats (the inputs of test_adam_kernel_matches_torch): both kernels run
    hint::adam_update on the same scalars, so p, m and v agree bit for bit after every step"""
    lib = _lib.load()
    n = 10007
    torch.manual_seed(1)
    p = torch.randn(n + 1, device=DEV)[:n].clone()
    g = 20 * torch.randn(n, device=DEV)
    m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    p2, g2, m2, v2 = p.clone(), g.clone(), m.clone(), v.clone()
    assert all(t.data_ptr() % 16 == 0 for t in (p2, g2, m2, v2))
    h = multi_create([(p2.data_ptr(), g2.data_ptr(), m2.data_ptr(), v2.data_ptr(), n)])
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for step in range(1, 4):
            assert lib.hint_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, 3e-4, 0.9, 0.95,
                                      1e-4, 1.86e-5, 0.5, 5.0, 0, stream) == 0
            assert lib.hint_adam_multi_step(h, step, 3e-4, 0.9, 0.95, 1e-4, 1.86e-5, 0.5, 5.0, 0, stream) == 0
            torch.cuda.synchronize()
            assert bits_equal(p, p2) and bits_equal(m, m2) and bits_equal(v, v2), step
            assert bits_equal(g, g2)
        # zero_grads clears exactly the gradients
        assert lib.hint_adam_multi_step(h, 4, 3e-4, 0.9, 0.95, 1e-4, 1.86e-5, 0.5, 5.0, 1, stream) == 0
        assert lib.hint_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 4, 3e-4, 0.9, 0.95,
                                  1e-4, 1.86e-5, 0.5, 5.0, 1, stream) == 0
        torch.cuda.synchronize()
        assert bits_equal(p, p2) and bits_equal(m, m2) and bits_equal(v, v2)
        assert int((g2 != 0).sum()) == 0 and int((g != 0).sum()) == 0
    finally:
        lib.hint_adam_multi_destroy(h)


@pytest.mark.timeout(180)
def test_segments_of_every_alignment_between_guard_bands():
    """40 segments cut out of four larger buffers at float offsets 0..3 chosen independently for p, g, m and v, NaN guard
    words everywhere else: three steps equal torch.optim.Adam on the clamped gradients (the project's optimizer tolerance,
    test_adam_kernel_matches_torch's) and no word outside the segments changes"""
    lib = _lib.load()
    lengths = [0, 1, 3, 4, 5, 1023, 70001, 2, 7, 8, 63, 64, 1024, 1025, 1027, 1028, 2047, 2048, 2051, 4099]
    rng = np.random.RandomState(7)
    cases = []
    for i, n in enumerate(lengths):                       # every length once with a common offset (16 bytes per lane behind
        cases.append((n, (i % 4,) * 4))                   # a head of 0..3 floats) and once with independent ones
        cases.append((n, tuple(int(o) for o in rng.randint(0, 4, size=4))))
    cases[13] = (70001, (1, 3, 0, 2))
    assert len(cases) == 40 and any(len(set(o)) == 1 for _, o in cases) and any(len(set(o)) > 1 for _, o in cases)
    GAP = 64                                              # guard floats between segments
    total = sum((n + 3) // 4 * 4 + GAP + 4 for n, _ in cases) + GAP
    bufs = [torch.full((total,), NAN_BITS, dtype=torch.int32, device=DEV) for _ in range(4)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    masks = [torch.zeros(total, dtype=torch.bool, device=DEV) for _ in range(4)]
    torch.manual_seed(3)
    segs, where, refs, grads, cur = [], [], [], [], GAP
    for n, offs in cases:
        p0 = torch.randn(n, device=DEV); g0 = 20 * torch.randn(n, device=DEV)
        m0 = 0.1 * torch.randn(n, device=DEV); v0 = 0.1 * torch.rand(n, device=DEV)
        at = []
        for b, mask, o, val in zip(bufs, masks, offs, (p0, g0, m0, v0)):
            b[cur + o:cur + o + n] = val.view(torch.int32)
            mask[cur + o:cur + o + n] = True
            at.append(cur + o)
        where.append(at)
        segs.append(tuple(b.data_ptr() + 4 * a for b, a in zip(bufs, at)) + (n,))
        refs.append((p0.clone().requires_grad_(True), m0, v0)); grads.append(g0)
        cur += (n + 3) // 4 * 4 + GAP + 4
    for (n, offs), s in zip(cases, segs):
        assert tuple((a % 16) // 4 for a in s[:4]) == offs
    # the reference: torch.optim.Adam from the same moments on the clamped, scaled gradients
    opt = torch.optim.Adam([r[0] for r in refs], lr=3e-4, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)
    for pr, m0, v0 in refs:
        opt.state[pr] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    h = multi_create(segs)
    try:
        for step in range(1, 4):
            for (pr, _, _), g0 in zip(refs, grads):
                pr.grad = (g0 * 0.5).clamp(-5, 5)
            opt.step()
            assert lib.hint_adam_multi_step(h, step, 3e-4, 0.9, 0.95, 1e-4, 1.86e-5, 0.5, 5.0, 0,
                                            torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
    finally:
        lib.hint_adam_multi_destroy(h)
    for b, mask in zip(bufs, masks):
        assert int(((b != NAN_BITS) & ~mask).sum()) == 0, "a word outside the segments changed"
    for (n, offs), at, (pr, _, _), g0 in zip(cases, where, refs, grads):
        got = [b[a:a + n].view(torch.float32) for b, a in zip(bufs, at)]
        st = opt.state[pr]
        np.testing.assert_allclose(got[0].cpu().numpy(), pr.detach().cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=str((n, offs)))
        np.testing.assert_allclose(got[2].cpu().numpy(), st["exp_avg"].cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=str((n, offs)))
        np.testing.assert_allclose(got[3].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=str((n, offs)))
        assert bits_equal(got[1], g0), (n, offs)           # zero_grads = 0: the gradients are read only


@pytest.mark.timeout(180)
@pytest.mark.parametrize("fuse_chain", [True, False])
@pytest.mark.parametrize("mode", ["direct", "autograd"])
def test_drop_in_on_golden_trajectory(mode, fuse_chain):
    """the loop body of test_reference_training_loop_body_on_module_path with ClampAdam(..., grad_clamp=5.0) and the clamp
    loop deleted, on the five recorded reference steps: that test's assertions"""
    case = CHAIN_CASES[1]
    c, nodes, shapes, params, perms, xs, g = load_chain_case(case)
    prev = hint_amd.set_param_grad_mode(mode)
    try:
        model = build_flow(case, params, perms)
        model.fuse_chain = fuse_chain
        params_trainable = list(filter(lambda p: p.requires_grad, model.parameters()))
        optim = hint_amd.ClampAdam(params_trainable, grad_clamp=5.0, **HYPER)
        history = []
        for x_np in xs:
            optim.zero_grad()
            x = torch.from_numpy(x_np).to(DEV)
            z = model(x)
            log_jacobian = model.log_jacobian(x, run_forward=False)
            batch_losses = [0.5 * torch.sum(z ** 2, dim=1).mean(), -log_jacobian.mean()]
            loss_total = sum(batch_losses)
            history.append([l.item() for l in batch_losses])
            loss_total.backward()
            optim.step()
    finally:
        hint_amd.set_param_grad_mode(prev)
    np.testing.assert_allclose(np.array(history), g["losses"], rtol=1e-4, atol=1e-5)
    for bi, blk in enumerate(model.blocks):
        for k, v in blk.state_dict().items():
            assert rel_err(v.cpu().numpy(), g[f"final:{bi}:{k}"]) < 1e-3, (bi, k)
            check_update(params[bi][k], v.cpu().numpy(), g[f"final:{bi}:{k}"], (bi, k))
    assert optim.launches == len(xs)


# ---- a small model with a foreign module, driven by the reference loop's statements ------------------------------------------
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.flow = hint_amd.HintFlow(6, 3, [24, 12])
        self.lin = torch.nn.Linear(6, 5)


def make_net(seed=11):
    torch.manual_seed(seed)
    net = Net().to(DEV)
    for p in net.parameters():
        p.data.add_(0.02 * torch.randn_like(p))
    return net


def net_loss(net, x):
    z = net.flow(x)
    log_jacobian = net.flow.log_jacobian(x, run_forward=False)
    return 0.5 * torch.sum(z ** 2, dim=1).mean() - log_jacobian.mean() + 40.0 * net.lin(x).pow(2).mean()


def make_optim(kind, params, **kw):
    if kind == "clampadam":
        return hint_amd.ClampAdam(params, grad_clamp=5.0, **HYPER, **kw)
    return torch.optim.Adam(params, **HYPER, **kw)


def one_step(net, opt, x, skip=None, set_to_none=True):
    """train_unconditional.py:114-144 for one batch; skip: a module whose parameters lose their gradients before the step"""
    params = [p for p in net.parameters() if p.requires_grad]
    opt.zero_grad(set_to_none=set_to_none)
    net_loss(net, x).backward()
    if skip is not None:
        for p in skip.parameters():
            p.grad = None
    if not isinstance(opt, hint_amd.ClampAdam):
        for p in params:
            if p.grad is not None:
                p.grad.data.clamp_(-5.00, 5.00)
    opt.step()


def snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def worst(a, b):
    """largest per-tensor rel_err between two snapshots"""
    return max(rel_err(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)


def batches(n, B=256, d=6, seed=5):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(B, d, device=DEV, generator=gen) for _ in range(n)]


@pytest.mark.timeout(240)
def test_matches_torch_adam_with_scheduler_and_skipped_block():
    """12 steps with StepLR(4, 0.5); on steps 5-6 one block's parameters have no gradient.  After every step the weights
    under ClampAdam equal those under clamp loop + torch.optim.Adam, and the skipped block's step count lags by 2 in both."""
    A = make_net()
    B_ = copy.deepcopy(A)
    Cn = copy.deepcopy(A)                                   # the noise floor: torch against itself
    opts = [make_optim("adam", list(A.parameters()), foreach=True), make_optim("clampadam", list(B_.parameters())),
            make_optim("adam", list(Cn.parameters()), foreach=False)]
    scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=4, gamma=0.5) for o in opts]
    floor = err = 0.0
    for k, x in enumerate(batches(12), start=1):
        for net, opt, sch in zip((A, B_, Cn), opts, scheds):
            one_step(net, opt, x, skip=net.flow.blocks[1] if k in (5, 6) else None)
            sch.step()
        a = snapshot(A)
        err = max(err, worst(snapshot(B_), a))
        floor = max(floor, worst(snapshot(Cn), a))
        assert opts[1].param_groups[0]["lr"] == opts[0].param_groups[0]["lr"]
    print(f"ClampAdam vs torch.optim.Adam: worst per-tensor rel_err {err:.3e}; torch foreach vs single-tensor: {floor:.3e}; "
          f"bound {MODEL_TOL:.3e}")
    assert opts[1].param_groups[0]["lr"] == pytest.approx(HYPER["lr"] * 0.125)
    for net, opt in zip((A, B_), opts):
        for name, p in net.named_parameters():
            want = 10 if name.startswith("flow.blocks.1.") else 12
            assert float(opt.state[p]["step"]) == want, (name, type(opt).__name__)
    for p in B_.parameters():                                # torch's keys, shapes and step form
        st, ref = opts[1].state[p], opts[0].state[next(iter(A.parameters()))]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert st["step"].shape == ref["step"].shape and st["step"].dtype == ref["step"].dtype \
            and st["step"].device == ref["step"].device
    assert err < MODEL_TOL, (err, floor)


@pytest.mark.timeout(240)
def test_state_interchange_with_torch_adam():
    """3 steps, state_dict() through torch.save / torch.load into the OTHER optimizer class, 3 more steps: equal to an
    uninterrupted torch.optim.Adam run, both ways"""
    xs = batches(6, seed=6)
    ref = make_net()
    nets = {"clamp->adam": copy.deepcopy(ref), "adam->clamp": copy.deepcopy(ref)}
    ref_opt = make_optim("adam", list(ref.parameters()))
    for x in xs:
        one_step(ref, ref_opt, x)
    want = snapshot(ref)
    for name, net in nets.items():
        first, second = ("clampadam", "adam") if name == "clamp->adam" else ("adam", "clampadam")
        opt = make_optim(first, list(net.parameters()))
        for x in xs[:3]:
            one_step(net, opt, x)
        buf = io.BytesIO()
        torch.save(opt.state_dict(), buf)
        buf.seek(0)
        sd = torch.load(buf, weights_only=False)
        opt2 = make_optim(second, list(net.parameters()))
        opt2.load_state_dict(sd)
        if second == "clampadam":
            assert opt2.param_groups[0]["grad_clamp"] == 5.0
            flat = {t.untyped_storage().data_ptr() for st in opt2.state.values() for t in (st["exp_avg"], st["exp_avg_sq"])}
            assert len(flat) == 2, "the moments live in two flat buffers, not in the loaded tensors"
        else:
            # the copies state_dict() hands out are nobody's views: stepping `opt` again must not move opt2's state
            assert not ({t.untyped_storage().data_ptr() for st in opt.state.values() for t in st.values()}
                        & {t.untyped_storage().data_ptr() for st in opt2.state.values() for t in st.values()})
        for x in xs[3:]:
            one_step(net, opt2, x)
        assert all(float(opt2.state[p]["step"]) == 6 for p in net.parameters())
        e = worst(snapshot(net), want)
        print(f"{name}: worst per-tensor rel_err {e:.3e} (bound {MODEL_TOL:.3e})")
        assert e < MODEL_TOL, (name, e)


@pytest.mark.timeout(240)
def test_rebound_storage_is_followed_and_tables_rebuilt_only_then():
    """p.data = ..., a load_state_dict of the model and fresh gradient tensors between steps: the next step updates the
    tensors the model now uses (torch.optim.Adam driven the same way agrees), and the device table is rebuilt exactly when
    a parameter's or a gradient's address moved"""
    prev = hint_amd.set_param_grad_mode("direct")
    try:
        A = make_net()
        B_ = copy.deepcopy(A)
        oa, ob = make_optim("adam", list(A.parameters())), make_optim("clampadam", list(B_.parameters()))
        xs = batches(8, seed=8)
        sd0 = {k: v.clone() for k, v in A.state_dict().items()}
        held = []

        def keys():
            return [p.data_ptr() for p in B_.parameters()] + [p.grad.data_ptr() for p in B_.parameters()]

        def both(x, before=None, must_move=None):
            builds, k0 = ob.table_builds, (keys() if ob.table_builds else None)
            for net, opt in ((A, oa), (B_, ob)):
                if before is not None:
                    before(net)
                # (nothing is to move: zero the gradients in place - where a freed gradient of the foreign module comes
                # back is the allocator's choice)
                one_step(net, opt, x, set_to_none=must_move is not False)
            e = worst(snapshot(B_), snapshot(A))
            assert e < MODEL_TOL, e
            moved = keys() != k0
            if must_move is not None:
                assert moved == must_move
            assert ob.table_builds == builds + (1 if moved else 0), (ob.table_builds, builds, moved)

        both(xs[0])
        assert ob.table_builds == 1
        both(xs[1], must_move=False)                          # arena views and cached gradient views: nothing moved

        def rebind(net):                                      # train_unconditional.py:165-167
            gen = torch.Generator(device=DEV).manual_seed(21)
            for p in net.parameters():
                p.data = 0.005 * torch.randn(p.shape, device=DEV, generator=gen)
        both(xs[2], rebind, must_move=True)                   # (the foreign Linear's weights stay where they were put)
        both(xs[3], must_move=False)
        both(xs[4], lambda net: net.load_state_dict(sd0))     # (copies in place or not: rebuilt exactly if something moved)

        hint_amd.set_param_grad_mode("autograd")              # gradients become autograd's own tensors

        def fresh_grads(net):
            held.append([p.grad for p in net.parameters()])   # the old ones stay alive, so the new ones are elsewhere
        both(xs[5], fresh_grads, must_move=True)
        both(xs[6], fresh_grads, must_move=True)
        assert all(float(ob.state[p]["step"]) == 7 for p in B_.parameters())
        # what the step updated is what the model reads
        with torch.no_grad():
            za, zb = A.flow(xs[7]), B_.flow(xs[7])
        assert rel_err(zb.cpu().numpy(), za.cpu().numpy()) < 1e-4
    finally:
        hint_amd.set_param_grad_mode(prev)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("fuse_chain", [False, True])
def test_pack_cache_sees_the_step(fuse_chain):
    """with set_pack_cache(True) a forward after ClampAdam.step() reads the new weights: bit for bit the forward of an
    identical model under the default re-pack"""
    x, x2 = batches(2, seed=9)
    outs = []
    for cache in (False, True):
        prev = H.set_pack_cache(cache)
        try:
            net = make_net()
            net.flow.fuse_chain = fuse_chain
            opt = make_optim("clampadam", list(net.parameters()))
            one_step(net, opt, x)
            with torch.no_grad():
                z1 = net.flow(x2)
            one_step(net, opt, x2)
            with torch.no_grad():
                z2 = net.flow(x2)
                J2 = net.flow.log_jacobian(x2, run_forward=False)
            outs.append((z1, z2, J2))
        finally:
            H.set_pack_cache(prev)
    assert not bits_equal(outs[0][0], outs[0][1])             # the second step did move the weights
    for a, b in zip(outs[0], outs[1]):
        assert bits_equal(a, b)


@pytest.mark.timeout(240)
def test_conditional_model_many_arenas():
    """three steps of train_conditional.py:120-150 on ConditionalHintFlow (twelve modules, each with an arena of its own):
    ClampAdam over all parameters against clamp loop + torch.optim.Adam"""
    torch.manual_seed(4)
    nx, ny, nb, hidden, B = 10, 3, 4, 24, 256
    m1 = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden).to(DEV)
    for p in m1.parameters():
        p.data.add_(0.02 * torch.randn_like(p))
    m2 = copy.deepcopy(m1)
    xs = [torch.randn(B, nx, device=DEV) for _ in range(3)]
    ys = [torch.randn(B, ny, device=DEV) for _ in range(3)]
    assert sum(1 for m in m1.modules() if hasattr(m, "tree")) == 12
    losses = []
    for model, kind in ((m1, "adam"), (m2, "clampadam")):
        params = [p for p in model.parameters() if p.requires_grad]
        optim = make_optim(kind, params)
        hist = []
        for x, y in zip(xs, ys):
            optim.zero_grad()
            z_y, z_x = model([y, x])
            z = torch.cat([z_x, z_y], dim=-1)
            log_jacobian = model.log_jacobian(run_forward=False)
            batch_losses = [0.5 * torch.sum(z ** 2, dim=1).mean(), -log_jacobian.mean()]
            sum(batch_losses).backward()
            if kind == "adam":
                for p in params:
                    p.grad.data.clamp_(-5.00, 5.00)
            optim.step()
            hist.append([l.item() for l in batch_losses])
        losses.append(hist)
    assert optim.launches == 3 and optim.table_builds == 1
    np.testing.assert_allclose(np.array(losses[1]), np.array(losses[0]), rtol=1e-4, atol=1e-5)
    e = worst(snapshot(m2), snapshot(m1))
    print(f"conditional model: worst per-tensor rel_err {e:.3e} (bound {MODEL_TOL:.3e})")
    assert e < MODEL_TOL, e


@pytest.mark.timeout(240)
def test_one_launch_per_group_and_step():
    """cfg 2 (POWER d = 6, 8 blocks: 288 parameter tensors): one hint_adam_multi_step per param group and step, and one
    hint_adam_multi_create per group over 10 unchanged steps"""
    import bench
    cfg = bench.WORKLOADS["power_hint_8"]
    torch.manual_seed(0)
    model = hint_amd.HintFlow(cfg["d"], cfg["n_blocks"], cfg["c_internal"]).to(DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    assert len(params) == 288
    for p in params:
        p.data = 0.005 * torch.randn_like(p.data)
    x = torch.randn(512, cfg["d"], device=DEV)
    for groups in (1, 2):
        if groups == 1:
            optim = hint_amd.ClampAdam(params, grad_clamp=5.0, **HYPER)
        else:
            optim = hint_amd.ClampAdam([{"params": params[:100], "lr": 1e-4}, {"params": params[100:]}], grad_clamp=5.0, **HYPER)
        lib = _lib.load()
        calls = {"create": 0, "step": 0}

        class Counting:                                       # the library with the two entry points counted
            def __getattr__(self, name):
                fn = getattr(lib, name)
                if name == "hint_adam_multi_create" or name == "hint_adam_multi_step":
                    def counted(*a, _fn=fn, _k=name.rsplit("_", 1)[1]):
                        calls[_k] += 1
                        return _fn(*a)
                    return counted
                return fn
        real_load = _lib.load
        hint_amd.optim._lib.load = lambda: Counting()
        try:
            for _ in range(10):
                optim.zero_grad()
                z = model(x)
                (0.5 * torch.sum(z ** 2, dim=1).mean() - model.log_jacobian(x, run_forward=False).mean()).backward()
                optim.step()
        finally:
            hint_amd.optim._lib.load = real_load
        torch.cuda.synchronize()
        assert calls == {"create": groups, "step": 10 * groups}, calls
        assert optim.launches == 10 * groups and optim.table_builds == groups
    assert all(torch.isfinite(p).all() for p in params)
