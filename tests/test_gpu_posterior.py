"""GPU tests of the fused posterior sampler of the conditional model (ConditionalHintFlow.sample_conditional / x_lane_forward):
the y lane on the distinct observations, the ExternalAffineCouplings' coefficients (hint_block_ext_coeffs) and one chained launch
over the x lane with the couplings as the blocks' affine steps (hint_chain_set_block_affine) - against the graph of
conditional_hint_4_full.py:55-95 composed from float64 oracle blocks, and against the module route."""
import ctypes as C

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib
from hint_amd.conditional import ConditionalFlowTrainer
from instance_cases import multi_pass_b, plan_dispatch, ragged
from oracle import hint_oracle as orc
from test_gpu_conditional import oracle_nodes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(12, 4, 3, 32),          # hac_x on the general kernels with subtree groups (both instances: FLY up to 4096 rows, not beyond)
          (100, 4, 4, 224),        # conditional_hint_4_full.py:58-94 at full size
          (8, 2, 2, 32)]           # hac_x on the wave-local kernels, which have no affine step: the sampler takes the module route
IDS = ["nx12", "nx100", "nx8_wave_local"]
WAVE_LOCAL = (8, 2, 2, 32)


def make_model(nx, ny, nb, hidden, seed=2):
    torch.manual_seed(seed)
    m = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden).to(DEV)
    # weights that keep the x lane O(1) in BOTH directions: the samplers start from z ~ N(0, 1), and torch's default init (what
    # test_gpu_conditional.py perturbs) maps that to |x| ~ 1e3 .. 1e4 at nx = 12, where no fp32 result is within 1e-4 of the row
    # scale of a float64 one; 0.03 * randn is the full-size model's init (train_conditional.py:160-162 re-initialises that way)
    for p in m.parameters():
        p.data = (0.03 if nx >= 50 else 0.07) * torch.randn_like(p)
    return m


def oracle_params(m):
    return {name: {k: v.detach().double().cpu() for k, v in sub.state_dict().items()}
            for name, sub in m.named_modules() if hasattr(sub, "tree")}


def oracle_conditions(m, P, y):
    """the y lane before ac_y_i, i = 0 .. n_blocks - 1 (float64)"""
    conds, yo = [], y.double().cpu()
    for i in range(m.n_blocks):
        if i > 0:
            yo = yo @ m.perm_y[i].W.double().cpu()
        conds.append(yo)
        sub = m.ac_y[i]
        yo, _ = orc.block_apply(oracle_nodes(sub.tree, 0), P[f"ac_y.{i}"], yo, [], clamp=sub.tree.clamp)
    return conds


def oracle_x_lane(m, P, conds, x, rev):
    """the x lane of the two-lane graph given its conditions ([1, ny] rows broadcast): (out, J) in float64"""
    xo = x.double().cpu()
    conds = [c.expand(xo.shape[0], -1) for c in conds]
    ny = conds[0].shape[1]
    J = torch.zeros(xo.shape[0], dtype=torch.float64)
    order = reversed(range(m.n_blocks)) if rev else range(m.n_blocks)
    for i in order:
        hx, ex = m.hac_x[i], m.ac_y_to_x[i]
        if not rev:
            if i > 0:
                xo = xo @ m.perm_x[i].W.double().cpu()
            xo, j = orc.block_apply(oracle_nodes(hx.tree, 0), P[f"hac_x.{i}"], xo, [], clamp=hx.tree.clamp); J = J + j
            xo, j = orc.block_apply(oracle_nodes(ex.tree, ny), P[f"ac_y_to_x.{i}"], xo, [conds[i]], clamp=ex.tree.clamp); J = J + j
        else:
            xo, j = orc.block_apply(oracle_nodes(ex.tree, ny), P[f"ac_y_to_x.{i}"], xo, [conds[i]], rev=True, clamp=ex.tree.clamp); J = J + j
            xo, j = orc.block_apply(oracle_nodes(hx.tree, 0), P[f"hac_x.{i}"], xo, [], rev=True, clamp=hx.tree.clamp); J = J + j
            if i > 0:
                xo = xo @ m.perm_x[i].W.double().cpu().t()
    return xo, J


def fused(m, B):
    """True when the sampler runs the x lane as one chained launch at batch size B (not the module route)"""
    return not m._posterior()._wave_local(B)


def batch_sizes(m):
    """1, 200, 4096 and a ragged size for which the x lane's launch goes round its tile loop more than once"""
    lib = _lib.load()
    plan = m.hac_x[0].tree.engine(torch.device(DEV)).plan
    d0 = plan_dispatch(lib, plan, 4096)
    return {"1": 1, "200": 200, "4096": 4096, "multi": multi_pass_b(d0["num_cu"], d0["nr"])}


def check_rows(got, ref, rows, what):
    """|got - ref| <= 1e-4 of the row's scale (max(1, largest entry of the oracle's row)), rows = the checked row indices"""
    g = got.detach().double().cpu()[rows]
    r = ref[rows] if ref.shape[0] != len(rows) else ref
    scale = torch.clamp(r.reshape(r.shape[0], -1).abs().max(dim=1).values, min=1.0)
    err = ((g - r).reshape(r.shape[0], -1).abs().max(dim=1).values / scale).max().item()
    assert err < 1e-4, f"{what}: max error {err:.3g} of the row scale"


@pytest.mark.parametrize("mode", ["broadcast", "per_row"])
@pytest.mark.parametrize("bkey", ["1", "200", "4096", "multi"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sample_conditional_and_x_lane_forward_match_oracle(shape, bkey, mode):
    nx, ny, nb, hidden = shape
    m = make_model(nx, ny, nb, hidden)
    B = batch_sizes(m)[bkey]
    assert fused(m, B) == (shape != WAVE_LOCAL)
    if bkey == "multi" and shape != WAVE_LOCAL:
        d = plan_dispatch(_lib.load(), m.hac_x[0].tree.engine(torch.device(DEV)).plan, B)
        assert d["passes"] >= 2 and ragged(d), d
    g = torch.Generator().manual_seed(7)
    z = torch.randn(B, nx, generator=g)
    y = torch.randn(1 if mode == "broadcast" else B, ny, generator=g)
    # the oracle on at most 600 rows: the first 300 and the last 300 (the ragged tail of the last pass)
    rows = list(range(B)) if B <= 600 else list(range(300)) + list(range(B - 300, B))
    P = oracle_params(m)
    ysub = y if mode == "broadcast" else y[rows]
    conds = oracle_conditions(m, P, ysub)

    yarg = y[0].to(DEV) if (mode == "broadcast" and B % 2 == 0) else y.to(DEV)        # ([ny] and [1, ny] both)
    x, Jx = m.sample_conditional(yarg, z.to(DEV))
    assert x.shape == (B, nx) and Jx.shape == (B,)
    xo, Jo = oracle_x_lane(m, P, conds, z[rows], rev=True)
    check_rows(x, xo, rows, "x")
    check_rows(Jx, Jo, rows, "J_x (inverse)")

    # the same chain forward, from the oracle's own samples: z back and the forward log-det
    xin = torch.zeros(B, nx)
    xin[rows] = xo.float()
    zf, Jf = m.x_lane_forward(xin.to(DEV), yarg)
    zo, Jfo = oracle_x_lane(m, P, conds, xo.float(), rev=False)
    check_rows(zf, zo, rows, "z_x (forward)")
    check_rows(Jf, Jfo, rows, "J_x (forward)")


@pytest.mark.parametrize("D,dc,h,R", [(100, 4, 224, 1), (100, 4, 224, 4096), (5, 2, 16, 77), (33, 3, 40, 17)])
def test_ext_coeffs_match_oracle_mlp(D, dc, h, R):
    """hint_block_ext_coeffs = (clamp 0.636 atan(s), t) of the coupling's s / t nets on the condition rows (hint.py:56-60)"""
    torch.manual_seed(3)
    mod = hint_amd.ExternalAffineCoupling([(D,)], dims_c=[(dc,)], F_args={"internal_size": h}).to(DEV)
    for p in mod.parameters():
        p.data = 0.1 * torch.randn_like(p)
    c = torch.randn(R, dc)
    eng = mod.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    eng.pack()
    coef = torch.full((R, 2, D), float("nan"), device=DEV)
    lib = _lib.load()
    cd = c.to(DEV)
    _lib.check(lib.hint_block_ext_coeffs(eng.plan, eng.arena.data_ptr(), eng.packed.data_ptr(), cd.data_ptr(), R, coef.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "hint_block_ext_coeffs")
    torch.cuda.synchronize()
    P = {k: v.detach().double().cpu() for k, v in mod.tree.state_dict().items()}
    s = orc._mlp(P, "s", c.double())
    t = orc._mlp(P, "t", c.double())
    a = mod.tree.clamp * 0.636 * torch.atan(s)
    got = coef.double().cpu()
    scale = max(1.0, t.abs().max().item(), a.abs().max().item())
    assert (got[:, 0] - a).abs().max().item() < 1e-5 * scale
    assert (got[:, 1] - t).abs().max().item() < 1e-5 * scale


def test_ext_coeffs_refuses_other_plans():
    m = make_model(100, 4, 2, 224)
    lib = _lib.load()
    e = m.hac_x[0].tree.engine(torch.device(DEV))
    e.ensure_arena(); e.pack()
    buf = torch.empty(4, device=DEV)
    assert lib.hint_block_ext_coeffs(e.plan, e.arena.data_ptr(), e.packed.data_ptr(), buf.data_ptr(), 1, buf.data_ptr(), None) != 0
    assert b"ExternalAffineCoupling" in lib.hint_last_error()


@pytest.mark.parametrize("mode", ["broadcast", "per_row"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sample_conditional_equals_module_route(shape, mode):
    """model_inverse of the reference config: m([z_y, z_x], rev=True)[1] with z_y the y lane's forward of y"""
    nx, ny, nb, hidden = shape
    m = make_model(nx, ny, nb, hidden)
    B = 333
    torch.manual_seed(11)
    z = torch.randn(B, nx, device=DEV)
    y = torch.randn(1 if mode == "broadcast" else B, ny, device=DEV)
    with torch.no_grad():
        yB = y.expand(B, -1).contiguous()
        zy, _ = m([yB, torch.zeros(B, nx, device=DEV)])
        _, xm = m([zy, z], rev=True)
        Jm = m.x_jac().clone()
    x, Jx = m.sample_conditional(y, z)
    scale = max(1.0, xm.abs().max().item())
    assert (x - xm).abs().max().item() < 1e-4 * scale
    assert (Jx - Jm).abs().max().item() < 1e-4 * max(1.0, Jm.abs().max().item())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_x_lane_forward_equals_forward_and_inverts_sampler(shape):
    nx, ny, nb, hidden = shape
    m = make_model(nx, ny, nb, hidden)
    B = 257
    torch.manual_seed(5)
    x = torch.randn(B, nx, device=DEV)
    y = torch.randn(B, ny, device=DEV)
    with torch.no_grad():
        _, zx_ref = m([y, x])
        Jx_ref = m.x_jac().clone()
    zx, Jx = m.x_lane_forward(x, y)
    assert (zx - zx_ref).abs().max().item() < 1e-4 * max(1.0, zx_ref.abs().max().item())
    assert (Jx - Jx_ref).abs().max().item() < 1e-4 * max(1.0, Jx_ref.abs().max().item())
    for yy in (y, y[3]):
        xs, Js = m.sample_conditional(yy, zx)
        z2, J2 = m.x_lane_forward(xs, yy)
        assert (z2 - zx).abs().max().item() < 1e-4 * max(1.0, zx.abs().max().item())
        assert (J2 + Js).abs().max().item() < 1e-4 * max(1.0, Js.abs().max().item())


def test_sampler_follows_a_trainer_step():
    """the sampler re-packs: after a ConditionalFlowTrainer step (which updates the weights in place) it samples the new model"""
    m = make_model(100, 4, 4, 224)
    B = 128
    torch.manual_seed(9)
    z = torch.randn(B, 100, device=DEV)
    y = torch.randn(4, device=DEV)
    x0, _ = m.sample_conditional(y, z)
    tr = ConditionalFlowTrainer(m, lr=1e-3, use_graph=False, seed=1)
    l0, l1 = tr.step(torch.randn(256, 100, device=DEV), torch.randn(256, 4, device=DEV))
    assert np.isfinite(float(l0) + float(l1))
    torch.cuda.synchronize()
    x1, J1 = m.sample_conditional(y, z)
    assert (x1 - x0).abs().max().item() > 1e-5           # the weights moved
    with torch.no_grad():
        yB = y.expand(B, -1).contiguous()
        zy, _ = m([yB, torch.zeros(B, 100, device=DEV)])
        _, xm = m([zy, z], rev=True)
        Jm = m.x_jac().clone()
    assert (x1 - xm).abs().max().item() < 1e-4 * max(1.0, xm.abs().max().item())
    assert (J1 - Jm).abs().max().item() < 1e-4 * max(1.0, Jm.abs().max().item())


def test_affine_step_is_inference_only():
    """a chain built for training (blocks with a tape) refuses the affine step; an inference chain takes it, and
    hint_chain_set_block clears it"""
    m = make_model(100, 4, 2, 224)
    lib = _lib.load()
    e = m.hac_x[0].tree.engine(torch.device(DEV))
    e.ensure_arena(); e.pack()
    B = 64
    coef = torch.zeros(2, 100, device=DEV)
    tape = torch.empty(e.sizes(B)[0], device=DEV)
    h = C.c_void_p()
    _lib.check(lib.hint_chain_create(e.plan, 1, B, C.byref(h)), "hint_chain_create")
    try:
        _lib.check(lib.hint_chain_set_block(h, 0, e.arena.data_ptr(), e.packed.data_ptr(), None, tape.data_ptr(), None, 0, None),
                   "hint_chain_set_block")
        assert lib.hint_chain_set_block_affine(h, 0, coef.data_ptr(), 0) != 0
        assert b"inference only" in lib.hint_last_error()
        _lib.check(lib.hint_chain_set_block(h, 0, e.arena.data_ptr(), e.packed.data_ptr(), None, None, None, 0, None),
                   "hint_chain_set_block")
        _lib.check(lib.hint_chain_set_block_affine(h, 0, coef.data_ptr(), 0), "hint_chain_set_block_affine")
        assert lib.hint_chain_set_block_affine(h, 0, coef.data_ptr(), 7) != 0          # neither broadcast nor a whole row
        assert lib.hint_chain_set_block_affine(h, 1, coef.data_ptr(), 0) != 0          # no such block
        # zero coefficients: the chain with the step is the plain block
        _lib.check(lib.hint_chain_commit(h), "hint_chain_commit")
        x = torch.randn(B, 100, device=DEV)
        z, J = torch.empty_like(x), torch.empty(B, device=DEV)
        _lib.check(lib.hint_chain_forward(h, x.data_ptr(), None, z.data_ptr(), J.data_ptr(), None, None,
                                          torch.cuda.current_stream().cuda_stream), "hint_chain_forward")
        with torch.no_grad():
            zr, Jr = e.apply(x, None, rev=False)
        torch.cuda.synchronize()
        assert (z - zr).abs().max().item() < 1e-5 * max(1.0, zr.abs().max().item())
        assert (J - Jr).abs().max().item() < 1e-5 * max(1.0, Jr.abs().max().item())
    finally:
        lib.hint_chain_destroy(h)


def test_sampler_shapes():
    m = make_model(100, 4, 2, 224)
    z = torch.randn(10, 100, device=DEV)
    for bad_y in (torch.randn(3, 4, device=DEV), torch.randn(10, 5, device=DEV), torch.randn(2, 10, 4, device=DEV)):
        with pytest.raises(hint_amd.HintAmdError):
            m.sample_conditional(bad_y, z)
    with pytest.raises(hint_amd.HintAmdError):
        m.sample_conditional(torch.randn(4, device=DEV), torch.randn(10, 99, device=DEV))
    with pytest.raises(hint_amd.HintAmdError):
        m.x_lane_forward(torch.randn(10, 100), torch.randn(4))
    x, J = m.sample_conditional(torch.randn(4, device=DEV), torch.randn(0, 100, device=DEV))
    assert x.shape == (0, 100) and J.shape == (0,)
    zx, Jx = m.x_lane_forward(torch.randn(0, 100, device=DEV), torch.randn(0, 4, device=DEV))
    assert zx.shape == (0, 100) and Jx.shape == (0,)
