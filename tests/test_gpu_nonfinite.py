"""NaN and inf in the DATA, a cotangent or a gradient (tests/nonfinite_cases.py; tests/test_nonfinite_cpu.py checks the cases
without a GPU).

1. The fused clamp + Adam step on the optimizer's element table, three steps in a row, against the statements it replaces
   (clamp_ only when grad_clamp > 0, then torch.optim.Adam(foreach=False) from the same moments, fp32 on the same device): every
   element of p, m and v has the reference's class (NaN, +inf, -inf, finite), the finite ones agree to test_gpu_optim.py's
   rtol 1e-5 / atol 1e-6; hint_adam_step_dev, hint_adam_multi_step and ClampAdam.step() give hint_adam_step's bits.
2. Spoiled rows on every row-kernel family: the same batch runs clean and spoiled at the same shape; every row that is not
   spoiled keeps its bits (forward, inverse, backward part A under spoiled inputs and under spoiled cotangents), and a spoiled
   row's objective 0.5 |z|^2 - J (its inverse x) is non-finite where the float64 oracle's is.  Which J and which weight-gradient
   tensors stay finite on the device is recorded in nonfinite.json (HINT_TEST_RECORDS, test_records/ by default), not asserted.
3. A row exactly ON a ReLU kink: relu'(0) = 0, as torch has it.
4. A training step on a batch with one NaN row poisons the model on every route, as the reference loop's does, and the clean
   steps in front of it still match float64 oracle training."""
import json
import math
import os

import numpy as np
import pytest
import torch

import hint_amd
import nonfinite_cases as nf
import session_script as ss
from guarded import NAN_BITS, bits_equal
from hint_amd import _lib
from hint_amd._core import PackGroup
from instance_cases import instances_of, knob_env, plan_dispatch
from oracle import hint_oracle as orc
from test_gpu_instances import TOL_GW, TOL_GX, err
from test_gpu_optim import multi_create
from test_gpu_trainer_session import build_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(section, name, value):
    out = os.environ.get("HINT_TEST_RECORDS") or os.path.join(ROOT, "test_records")
    try:
        os.makedirs(out, exist_ok=True)
        f = os.path.join(out, "nonfinite.json")
        have = json.load(open(f)) if os.path.exists(f) else {}
        have.setdefault(section, {})[name] = value
        json.dump(have, open(f, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits_or_both_nan(a, b):
    """element by element: the same bits, or a NaN in both (guarded.bits_equal without the NaNs' payloads)"""
    return (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))


# ==== 1. the optimizer's element table ===========================================================================================
H = nf.HYPER
ADAM_ARGS = (H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["weight_decay"])


class FlatTable:
    """the table's segments in four flat buffers (p, g, m, v), every segment on a 16-byte boundary, NaN guard words between"""

    def __init__(self, t):
        self.t, self.offs, cur = t, [], 4
        for n in t.lengths:
            self.offs.append(cur)
            cur += (n + 3) // 4 * 4 + 4
        self.total = cur
        self.bufs = [torch.full((cur,), NAN_BITS, dtype=torch.int32, device=DEV) for _ in range(4)]
        self.mask = torch.zeros(cur, dtype=torch.bool, device=DEV)
        for b, col in zip(self.bufs, (t.p, t.g, t.m, t.v)):
            assert b.data_ptr() % 16 == 0
            for off, a in zip(self.offs, col):
                b[off:off + len(a)] = torch.from_numpy(a.copy()).to(DEV).view(torch.int32)
        for off, n in zip(self.offs, t.lengths):
            self.mask[off:off + n] = True

    def ptrs(self, si):
        return [b.data_ptr() + 4 * self.offs[si] for b in self.bufs]

    def seg(self, q, si):
        off = self.offs[si]
        return self.bufs[q][off:off + self.t.lengths[si]].view(torch.float32)

    def state(self):
        """per segment (p, m, v) clones"""
        return [tuple(self.seg(q, si).clone() for q in (0, 2, 3)) for si in range(len(self.offs))]

    def check_rest(self):
        for b in self.bufs:
            assert int(((b != NAN_BITS) & ~self.mask).sum()) == 0, "a word outside the segments changed"
        for si, g in enumerate(self.t.g):
            assert bits_equal(self.seg(1, si), torch.from_numpy(g).to(DEV)), "zero_grads = 0: the gradients are read only"


def run_step(clamp, scale):
    """hint_adam_step, segment by segment -> [per step: per segment (p, m, v)]"""
    lib = _lib.load()
    ft = FlatTable(nf.table(scale))
    out = []
    for step in range(1, nf.STEPS + 1):
        for si, n in enumerate(ft.t.lengths):
            assert lib.hint_adam_step(*ft.ptrs(si), n, step, *ADAM_ARGS, scale, clamp, 0, stream()) == 0
        torch.cuda.synchronize()
        out.append(ft.state())
    ft.check_rest()
    return out


def run_step_dev(clamp, scale):
    """hint_adam_step_dev with opt_state written by the step prologue (hint_pack_group_run_ex) in front of every step"""
    lib = _lib.load()
    ft = FlatTable(nf.table(scale))
    blk = hint_amd.HierarchicalAffineCouplingBlock([(6,)], c_internal=[24, 12]).to(DEV)
    eng = blk.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    eng.pack()
    group = PackGroup([eng], torch.device(DEV))
    zero_buf = torch.ones(8, device=DEV)
    rng = torch.tensor([99, 0], dtype=torch.int64, device=DEV)
    opt = torch.tensor([H["lr"], H["betas"][0], H["betas"][1], nf.NAN, nf.NAN, 0, 0, 0], dtype=torch.float32, device=DEV)
    out = []
    try:
        for step in range(1, nf.STEPS + 1):
            group.run(zero_buf, rng, opt)
            for si, n in enumerate(ft.t.lengths):
                assert lib.hint_adam_step_dev(*ft.ptrs(si), n, opt.data_ptr(), *ADAM_ARGS[1:], scale, clamp, 0, stream()) == 0
            torch.cuda.synchronize()
            assert int(rng[1]) == step
            f3, f4 = float(np.float32(float(np.float32(H["lr"])) / (1.0 - float(np.float32(H["betas"][0])) ** step))), \
                float(np.float32(1.0 / math.sqrt(1.0 - float(np.float32(H["betas"][1])) ** step)))
            assert (float(opt[3]), float(opt[4])) == (f3, f4), ("the prologue's factors are not hint_adam_step's", step)
            out.append(ft.state())
    finally:
        group.close()
    ft.check_rest()
    return out


def run_multi(clamp, scale):
    lib = _lib.load()
    ft = FlatTable(nf.table(scale))
    h = multi_create([tuple(ft.ptrs(si)) + (n,) for si, n in enumerate(ft.t.lengths)])
    out = []
    try:
        for step in range(1, nf.STEPS + 1):
            assert lib.hint_adam_multi_step(h, step, *ADAM_ARGS, scale, clamp, 0, stream()) == 0
            torch.cuda.synchronize()
            out.append(ft.state())
    finally:
        lib.hint_adam_multi_destroy(h)
    ft.check_rest()
    return out


def run_clampadam(clamp, scale):
    """ClampAdam.step() on parameters whose .grad holds the table, the moments loaded from a torch.optim.Adam state_dict"""
    t = nf.table(scale)
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in t.p]
    seed = torch.optim.Adam(ps, **H)
    for p, m, v in zip(ps, t.m, t.v):
        seed.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.from_numpy(m.copy()).to(DEV),
                         "exp_avg_sq": torch.from_numpy(v.copy()).to(DEV)}
    opt = hint_amd.ClampAdam(ps, grad_clamp=clamp, grad_scale=scale, **H)
    opt.load_state_dict(seed.state_dict())
    assert opt.param_groups[0]["grad_clamp"] == clamp and opt.param_groups[0]["grad_scale"] == scale
    for p, g in zip(ps, t.g):
        p.grad = torch.from_numpy(g.copy()).to(DEV)
    out = []
    for _ in range(nf.STEPS):
        opt.step()
        torch.cuda.synchronize()
        out.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps])
    for p, g in zip(ps, t.g):
        assert bits_equal(p.grad, torch.from_numpy(g).to(DEV))
    return out


_STEP = {}


def step_result(clamp, scale):
    if (clamp, scale) not in _STEP:
        _STEP[(clamp, scale)] = run_step(clamp, scale)
    return _STEP[(clamp, scale)]


@pytest.mark.parametrize("clamp,scale", nf.RUNS)
def test_adam_step_keeps_nan_and_inf_as_torch_does(clamp, scale):
    """hint_adam_step on the element table against clamp_ + torch.optim.Adam(foreach=False) on the same device, after each of
    three steps: the class of every element of p, m, v, and the finite elements to rtol 1e-5 / atol 1e-6.  Before the clamp
    became a compare-select (it was fminf(fmaxf(g, -c), c), and "no clamp" a clamp at 3.0e38) this failed on every NaN class
    and, with grad_clamp = 0, on the inf and 3.3e38 classes."""
    t = nf.table(scale)
    ref = nf.torch_reference(t, clamp, scale, device=DEV)
    got = step_result(clamp, scale)
    names = np.array(t.names)
    wrong_class, wrong_value, compared = set(), set(), 0
    for step in range(nf.STEPS):
        for si, ci in enumerate(t.cls):
            for q, what in enumerate("pmv"):
                a, r = got[step][si][q], ref[step][si][q]
                ca, cr = nf.class_of(a), nf.class_of(r)
                bad = ca != cr
                wrong_class |= {(step + 1, what, n) for n in names[ci[bad]]}
                fin = (cr == 0) & ~bad
                an, rn = a.cpu().numpy(), r.cpu().numpy()
                off = np.zeros(len(ci), dtype=bool)
                off[fin] = np.abs(an[fin] - rn[fin]) > 1e-6 + 1e-5 * np.abs(rn[fin])
                wrong_value |= {(step + 1, what, n) for n in names[ci[off]]}
                assert a.shape == r.shape == (len(ci),)
                compared += a.numel()                                # (its class, and its value where the class is finite)
    assert compared == 3 * nf.STEPS * sum(t.lengths)                 # no element is left out
    print(f"grad_clamp {clamp} grad_scale {scale}: {len(wrong_class)} (step, tensor, class) with another class than torch's, "
          f"{len(wrong_value)} finite ones beyond the tolerance")
    assert not wrong_class, sorted(wrong_class)
    assert not wrong_value, sorted(wrong_value)


@pytest.mark.parametrize("clamp,scale", nf.RUNS)
@pytest.mark.parametrize("route", ["step_dev", "multi", "clampadam"])
def test_every_route_takes_hint_adam_step_bits_on_the_table(route, clamp, scale):
    """hint_adam_step_dev (opt_state from the step prologue), hint_adam_multi_step and ClampAdam.step(): the bits of
    hint_adam_step after each of the three steps, NaN for NaN"""
    want = step_result(clamp, scale)
    got = {"step_dev": run_step_dev, "multi": run_multi, "clampadam": run_clampadam}[route](clamp, scale)
    t = nf.table(scale)
    names = np.array(t.names)
    for step in range(nf.STEPS):
        for si, ci in enumerate(t.cls):
            for q, what in enumerate("pmv"):
                a, b = got[step][si][q].reshape(-1), want[step][si][q]
                same = same_bits_or_both_nan(a, b).cpu().numpy()
                assert same.all(), (route, step + 1, what, sorted(set(names[ci[~same]])))


# ==== 2. spoiled rows ============================================================================================================
def spoil_cotangents(gz, gJ, plan, seed=6):
    gz, gJ = gz.clone(), gJ.clone()
    rng = np.random.RandomState(seed)
    for r, what in plan.items():
        lane = int(rng.randint(gz.shape[1]))
        if what == "nan row":
            gz[r] = nf.NAN
            gJ[r] = nf.NAN
        elif what == "nan condition":
            gJ[r] = nf.NAN
        else:
            val = {"nan lane": nf.NAN, "+inf lane": nf.INF, "-inf lane": -nf.INF}[what]
            gz[r, lane] = val
            if r % 2:
                gJ[r] = val
    return gz, gJ


def assert_dispatch(case, lib, plan):
    disp = plan_dispatch(lib, plan, case.B)
    got = instances_of(disp, case.entry)
    assert got == case.expect, f"{case.name}: runs {got}, declared {case.expect}"
    assert disp["nr"] == case.nr and disp["groups"] == 3, (case.name, disp["nr"], disp["groups"])


class BlockRig:
    def __init__(self, case, lib, P=None):
        self.case = case
        if P is None:
            _, P = nf.block_params(case)
        self.blk = hint_amd.HierarchicalAffineCouplingBlock([(case.d,)], dims_c=[(case.dc,)] if case.dc else [],
                                                            c_internal=list(case.widths))
        self.blk.load_state_dict(P)
        self.blk = self.blk.to(DEV)
        assert_dispatch(case, lib, self.blk.tree.engine(torch.device(DEV)).plan)

    def run(self, x, c, zi, ci, gz, gJ):
        """forward + backward on (x, c) under (gz, gJ), inverse on (zi, ci) -> dict of device tensors"""
        blk, case = self.blk, self.case
        blk.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        cd = [c.to(DEV).requires_grad_(True)] if case.dc else []
        (z,) = blk([xd], c=cd)
        J = blk.jacobian(None)
        ((z * gz.to(DEV)).sum() + (J * gJ.to(DEV)).sum()).backward()
        out = dict(z=z.detach(), J=J.detach(), gx=xd.grad, gc=cd[0].grad if case.dc else None,
                   gw={k: p.grad.clone() for k, p in blk.named_parameters()})
        with torch.no_grad():
            (xi,) = blk([zi.to(DEV)], c=[ci.to(DEV)] if case.dc else [], rev=True)
            out["xi"], out["Ji"] = xi.clone(), blk.jacobian(None).clone()
        torch.cuda.synchronize()
        return out


class ChainRig:
    """two blocks through hint_chain_forward / hint_chain_backward / hint_chain_inverse (run_chain of test_gpu_instances.py)"""

    def __init__(self, case, lib):
        self.case, self.lib = case, lib
        ref = nf.chain_oracle(case)
        flow = hint_amd.HintFlow(case.d, case.n_blocks, list(case.widths), ndim_c=case.dc)
        for i, blk in enumerate(flow.blocks):
            blk.load_state_dict({k: v.float() for k, v in ref.params[i].items()})
            if ref.perms[i] is not None:
                flow.perms[i].W.copy_(ref.perms[i].float())
        self.tr = tr = hint_amd.FlowTrainer(flow.to(DEV), noise=0.0, use_graph=False)
        assert tr._chainable
        tr._check_arenas()
        tr._pack_all()
        self.chain = tr._chain_for(case.B)
        assert_dispatch(case, lib, tr.engines[0].plan)

    def run(self, x, c, zi, ci, gz, gJ):
        lib, tr, B = self.lib, self.tr, self.case.B
        xd, gzd, gJd = x.to(DEV).contiguous(), gz.to(DEV).contiguous(), gJ.to(DEV).contiguous()
        z, J, gx = torch.empty_like(xd), torch.empty(B, device=DEV), torch.empty_like(xd)
        _lib.check(lib.hint_chain_forward(self.chain, xd.data_ptr(), None, z.data_ptr(), J.data_ptr(), None, None, stream()),
                   "hint_chain_forward")
        _lib.check(lib.hint_chain_backward(self.chain, xd.data_ptr(), None, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(), None,
                                           1.0, 0.0, 0, stream()), "hint_chain_backward")
        torch.cuda.synchronize()
        gw = {}
        for bi, ((a, b), eng) in enumerate(zip(tr.slices, tr.engines)):
            names = {id(p): n for n, p in tr.flow.blocks[bi].named_parameters()}
            for p, g in zip(eng.params, eng.split_flat(tr.G[a:b])):
                gw[f"{bi}:{names[id(p)]}"] = g.clone()
        with torch.no_grad():
            xi, Ji = tr.sample(zi.to(DEV), None)
        torch.cuda.synchronize()
        return dict(z=z, J=J, gx=gx, gc=None, gw=gw, xi=xi.clone(), Ji=Ji.clone())


def finite_tensors(gw):
    """{subnet.layer.kind: how many weight-gradient tensors of that kind are finite} (e.g. "t.4.bias")"""
    out = {}
    for k, g in gw.items():
        if bool(torch.isfinite(g).all()):
            kind = ".".join(k.split(".")[-3:])
            out[kind] = out.get(kind, 0) + 1
    return out


def rows_keep_their_bits(name, what, clean, spoiled, keep):
    for k in what:
        if clean[k] is None:
            continue
        a, b = clean[k][keep], spoiled[k][keep]
        assert bool(torch.isfinite(a).all()), (name, k, "the clean run is not finite")
        if not bits_equal(a, b):
            rows = torch.nonzero(keep.to(a.device))[(a.reshape(a.shape[0], -1).view(torch.int32)
                                                     != b.reshape(b.shape[0], -1).view(torch.int32)).any(dim=1)].flatten()
            raise AssertionError(f"{name}: {k} of unspoiled rows {rows.tolist()} changed when other rows were spoiled")


@pytest.mark.parametrize("case", nf.ROW_CASES + nf.CHAIN_CASES, ids=lambda c: c.name)
def test_spoiled_rows_leave_their_neighbours_alone(case, monkeypatch):
    lib = _lib.load()
    knob_env(monkeypatch, lib, case.knobs)
    try:
        rig = (ChainRig if case.entry == "chain" else BlockRig)(case, lib)
        x, c, zi, gz, gJ = nf.row_inputs(case)
        plan = nf.spoil_plan(case)
        xs, cs = nf.spoil(x, c, plan)
        zs, _ = nf.spoil(zi, c, {r: w for r, w in plan.items() if w != "nan condition"})
        gzs, gJs = spoil_cotangents(gz, gJ, plan)
        clean = rig.run(x, c, zi, c, gz, gJ)
        again = rig.run(x, c, zi, c, gz, gJ)
        spoiled = rig.run(xs, cs, zs, cs, gz, gJ)
        cot = rig.run(x, c, zi, c, gzs, gJs)
    finally:
        monkeypatch.undo()
        lib.hint_debug_reload_knobs()
    obj_bad, inv_bad, mask = nf.oracle_rows(case.name)
    keep = ~mask
    everything = torch.ones(case.B, dtype=torch.bool)
    rows_keep_their_bits(case.name + " (the same run twice)", ("z", "J", "xi", "Ji", "gx", "gc"), clean, again, everything)
    rows_keep_their_bits(case.name, ("z", "J", "xi", "Ji", "gx", "gc"), clean, spoiled, keep)
    rows_keep_their_bits(case.name + " (spoiled cotangents)", ("gx", "gc"), clean, cot, keep)
    rows_keep_their_bits(case.name + " (spoiled cotangents)", ("z", "J"), clean, cot, everything)
    # the class of the spoiled rows: the float64 oracle's
    obj = (0.5 * (spoiled["z"] ** 2).sum(1) - spoiled["J"]).cpu()
    finite_obj = [r for r in torch.nonzero(obj_bad).flatten().tolist() if math.isfinite(float(obj[r]))]
    assert not finite_obj, (case.name, "objective finite on the device, non-finite in the oracle",
                            {r: plan[r] for r in finite_obj})
    xi_ok = torch.isfinite(spoiled["xi"]).all(dim=1).cpu()
    finite_inv = [r for r in torch.nonzero(inv_bad).flatten().tolist() if bool(xi_ok[r])]
    assert not finite_inv, (case.name, "inverse x finite on the device, non-finite in the oracle",
                            {r: plan[r] for r in finite_inv})
    # what is NOT guaranteed, for the record: J alone and the weight gradients' NaN pattern
    rows = sorted(plan)
    record("rows", case.name, {
        "spoiled rows": len(rows),
        "J finite (forward)": {w: int(sum(math.isfinite(float(spoiled["J"][r])) for r in rows if plan[r] == w))
                               for w in sorted(set(plan.values()))},
        "gx row finite (spoiled input)": int(torch.isfinite(spoiled["gx"][mask]).all(dim=1).sum()),
        "gx row finite (spoiled cotangent)": int(torch.isfinite(cot["gx"][mask]).all(dim=1).sum()),
        "weight gradient tensors finite (spoiled input)": finite_tensors(spoiled["gw"]),
        "weight gradient tensors finite (spoiled cotangent)": finite_tensors(cot["gw"]),
        "weight gradient tensors": len(spoiled["gw"]),
    })


def test_ext_coeffs_keep_a_non_finite_condition():
    """hint_block_ext_coeffs (the ExternalAffineCoupling's per-row coefficients, a function of the condition alone): rows whose
    condition is finite keep their bits when other rows hold NaN or inf, and a row whose coefficients are non-finite in the
    float64 oracle has non-finite coefficients (before the rows were poisoned at the load, its ReLUs returned 0 for the NaN
    pre-activations and the coefficients came out finite)"""
    torch.manual_seed(3)
    D, dc, h, R = 33, 3, 40, 37
    mod = hint_amd.ExternalAffineCoupling([(D,)], dims_c=[(dc,)], F_args={"internal_size": h}).to(DEV)
    for p in mod.parameters():
        p.data = 0.1 * torch.randn_like(p)
    eng = mod.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    eng.pack()
    lib = _lib.load()
    c = torch.randn(R, dc)
    cs = c.clone()
    spoiled = {0: ("lane", nf.NAN), 7: ("lane", nf.INF), 16: ("lane", -nf.INF), 17: ("row", nf.NAN), 21: ("lane", nf.NAN),
               R - 1: ("lane", nf.NAN)}
    for i, (r, (what, val)) in enumerate(spoiled.items()):
        if what == "row":
            cs[r] = val
        else:
            cs[r, i % dc] = val
    outs = []
    for cc in (c, cs):
        coef = torch.full((R, 2, D), 7.0, device=DEV)
        cd = cc.to(DEV)
        _lib.check(lib.hint_block_ext_coeffs(eng.plan, eng.arena.data_ptr(), eng.packed.data_ptr(), cd.data_ptr(), R,
                                             coef.data_ptr(), stream()), "hint_block_ext_coeffs")
        torch.cuda.synchronize()
        outs.append(coef)
    keep = torch.ones(R, dtype=torch.bool)
    keep[list(spoiled)] = False
    assert bool(torch.isfinite(outs[0]).all()) and bits_equal(outs[0][keep], outs[1][keep])
    P = {k: v.detach().double().cpu() for k, v in mod.tree.state_dict().items()}
    s64, t64 = orc._mlp(P, "s", cs.double()), orc._mlp(P, "t", cs.double())
    bad = ~(torch.isfinite(s64).all(dim=1) & torch.isfinite(t64).all(dim=1))
    assert bool(bad[~keep].all()) and not bool(bad[keep].any())           # (the oracle: every spoiled row, and only those)
    got_bad = ~torch.isfinite(outs[1]).reshape(R, -1).all(dim=1).cpu()
    assert bool(got_bad[bad].all()), [r for r in spoiled if not bool(got_bad[r])]


def test_posterior_sampler_keeps_a_nan_observation():
    """sample_conditional / x_lane_forward with one observation per row (the fused chain: coefficients + ONE chained launch):
    a NaN in one row's y leaves the other rows' bits alone and makes that row's x (its objective, forward) non-finite, as the
    two-lane graph in float64 does"""
    from test_gpu_posterior import make_model, fused, oracle_conditions, oracle_params, oracle_x_lane
    nx, ny, nb, hidden = 12, 4, 3, 32
    m = make_model(nx, ny, nb, hidden)
    B = 37
    assert fused(m, B)
    g = torch.Generator().manual_seed(7)
    z, y = torch.randn(B, nx, generator=g), torch.randn(B, ny, generator=g)
    ys = y.clone()
    rows = [0, 20, B - 1]
    ys[0, 1], ys[20], ys[B - 1, 3] = nf.NAN, nf.NAN, nf.NAN
    keep = torch.ones(B, dtype=torch.bool)
    keep[rows] = False
    P = oracle_params(m)
    conds = oracle_conditions(m, P, ys)
    xo, _ = oracle_x_lane(m, P, conds, z, rev=True)
    zo, Jo = oracle_x_lane(m, P, conds, z, rev=False)
    assert not bool(torch.isfinite(xo[rows]).all(dim=1).any()) and not bool(torch.isfinite(0.5 * (zo ** 2).sum(1) - Jo)[rows].any())
    x0, J0 = m.sample_conditional(y.to(DEV), z.to(DEV))
    x1, J1 = m.sample_conditional(ys.to(DEV), z.to(DEV))
    assert bits_equal(x0[keep], x1[keep]) and bits_equal(J0[keep], J1[keep])
    assert not bool(torch.isfinite(x1[rows]).all(dim=1).any()), "a sample from a NaN observation is finite"
    f0, K0 = m.x_lane_forward(z.to(DEV), y.to(DEV))
    f1, K1 = m.x_lane_forward(z.to(DEV), ys.to(DEV))
    assert bits_equal(f0[keep], f1[keep]) and bits_equal(K0[keep], K1[keep])
    assert not bool(torch.isfinite(0.5 * (f1 ** 2).sum(1) - K1)[rows].any()), "the x-lane density of a NaN observation is finite"


# ==== 3. a row exactly on a kink ================================================================================================
def test_rows_exactly_on_a_relu_kink_take_torchs_subgradient():
    """b1 = 0 and all-zero rows of x and c: the first-layer pre-activations those rows see before any coupling has written
    their lanes are exactly 0, and only those rows carry cotangents.  g_x, g_c and every weight-gradient tensor against the
    float64 oracle (torch: relu'(0) = 0) at test_gpu_instances.py's tolerances - the suite waives rows NEAR a kink everywhere;
    this is the one ON it."""
    lib = _lib.load()
    case, nodes, P, x, c, gz, gJ = nf.kink_setup()
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    x64, c64 = x.double().requires_grad_(True), c.double().requires_grad_(True)
    z64, J64 = orc.block_apply(nodes, P64, x64, [c64], rev=False)
    ((z64 * gz.double()).sum() + (J64 * gJ.double()).sum()).backward()
    rig = BlockRig(case, lib, P)
    out = rig.run(x, c, x, c, gz, gJ)
    assert err(out["gx"], x64.grad) <= TOL_GX, ("d/dx", err(out["gx"], x64.grad))
    assert err(out["gc"], c64.grad) <= TOL_GX, ("d/dc", err(out["gc"], c64.grad))
    gmax = max(float(v.grad.abs().max()) for v in P64.values())
    zero_in_oracle = 0
    for k, v in P64.items():
        r = v.grad
        e = float((out["gw"][k].double().cpu() - r).abs().max())
        assert e <= TOL_GW * float(r.abs().max()) + 1e-7 * gmax, (k, e, float(r.abs().max()))
        zero_in_oracle += int(float(r.abs().max()) == 0.0)
    assert zero_in_oracle > 0            # (first layers behind the kink: their gradient is exactly zero under relu'(0) = 0)


# ==== 4. a poisoned step ========================================================================================================
def clean_steps_tolerance(got, ref64, ref32):
    """the session rule (session_script.tolerances): 4 x the float32 oracle's own deviation from the float64 oracle, at least
    4 ulp of fp32, at most CAPS"""
    tol = min(ss.CAPS["losses"], 4.0 * max(ss.scalar_dev(ref32, ref64), ss.ULP))
    dev = ss.scalar_dev(got, ref64)
    return dev, tol


_REF32 = {}


def flow_ref32(flow_name):
    """the float32 oracle's loss pairs of the two clean steps (the tolerance's yardstick)"""
    if flow_name not in _REF32:
        be = ss.OracleBackend(ss.FLOWS[flow_name], torch.float32)
        _REF32[flow_name] = np.array([be.step(x, c) for x, c in nf.poisoned_batches(flow_name)[:2]], dtype=np.float64)
    return _REF32[flow_name]


def check_poisoned(name, losses, nll, tensors, ref_losses, ref32):
    """losses [4, 2] of the session, the nll behind it, tensors = (P, M, V) (each a tensor or a list of tensors)"""
    losses = np.asarray(losses, dtype=np.float64)
    total = losses.sum(axis=1)
    print(f"{name}: l0 + l1 per step {total.tolist()}, nll {nll}")
    dev, tol = clean_steps_tolerance(losses[:2], ref_losses[:2], ref32)
    print(f"    clean steps: loss pair deviation {dev:.2e} (tolerance {tol:.2e})")
    assert dev <= tol, (name, "the clean steps in front of the spoiled one", dev, tol)
    assert not math.isfinite(total[2]), (name, "the spoiled step's loss is finite", total[2])
    assert not math.isfinite(total[3]), (name, "the clean step behind the spoiled one has a finite loss", total[3])
    assert not math.isfinite(nll), (name, "nll behind the spoiled step is finite", nll)
    for what, ts in zip("PMV", tensors):
        ts = ts if isinstance(ts, (list, tuple)) else [ts]
        n = sum(int(torch.isnan(t).sum()) for t in ts)
        print(f"    {what}: {n} NaN elements of {sum(t.numel() for t in ts)}")
        assert n > 0, (name, f"no NaN in {what} behind a step on a batch with a NaN row")


def to_dev(t):
    return t.to(DEV) if t is not None else None


@pytest.mark.parametrize("fuse", ["0", "1"], ids=["HINT_FUSE_ADAM=0", "HINT_FUSE_ADAM=1"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("flow_name", list(ss.FLOWS))
def test_flow_trainer_poisoned_step_poisons_the_model(flow_name, use_graph, fuse, monkeypatch):
    """two clean steps, a step on a batch with one NaN row, a clean step, nll(): FlowTrainer ends up as float64 oracle training
    does - non-finite losses from the spoiled step on, NaN in P, M and V"""
    monkeypatch.setenv("HINT_FUSE_ADAM", fuse)
    ref = nf.poisoned_reference(flow_name)
    bt = nf.poisoned_batches(flow_name)
    tr = build_trainer(flow_name, use_graph)
    losses = []
    for x, c in bt[:4]:
        l0, l1 = tr.step(to_dev(x), to_dev(c))
        losses.append([float(l0), float(l1)])
    nll = tr.nll(to_dev(bt[4][0]), to_dev(bt[4][1]))
    torch.cuda.synchronize()
    check_poisoned(f"FlowTrainer {flow_name} graph={use_graph} fuse={fuse}", losses, nll, (tr.P, tr.M, tr.V), ref["losses"],
                   flow_ref32(flow_name))


def build_flow(flow_name):
    spec = ss.FLOWS[flow_name]
    params, perms = ss.initial_weights(spec)
    flow = hint_amd.HintFlow(spec["d"], spec["n_blocks"], list(spec["widths"]), ndim_c=spec["dc"])
    for i, blk in enumerate(flow.blocks):
        blk.load_state_dict({k: v.clone() for k, v in params[i].items()})
        if perms[i] is not None:
            flow.perms[i].W.copy_(perms[i])
    return flow.to(DEV)


@pytest.mark.parametrize("optimizer", ["clampadam", "reference loop"])
@pytest.mark.parametrize("flow_name", list(ss.FLOWS))
def test_module_route_poisoned_step_poisons_the_model(flow_name, optimizer):
    """the reference's loop body on the modules (train_unconditional.py:114-144): with loss.backward() + ClampAdam, and verbatim
    with clamp_ + torch.optim.Adam"""
    ref = nf.poisoned_reference(flow_name)
    bt = nf.poisoned_batches(flow_name)
    model = build_flow(flow_name)
    d = ss.FLOWS[flow_name]["d"]
    params_trainable = list(filter(lambda p: p.requires_grad, model.parameters()))
    kw = dict(lr=ss.LR, betas=ss.BETAS, eps=ss.EPS, weight_decay=ss.WD)
    optim = hint_amd.ClampAdam(params_trainable, grad_clamp=5.0, **kw) if optimizer == "clampadam" \
        else torch.optim.Adam(params_trainable, **kw)
    losses = []
    for x, c in bt[:4]:
        optim.zero_grad()
        x, c = to_dev(x), to_dev(c)
        z = model(x, c=c)
        log_jacobian = model.log_jacobian(run_forward=False)
        batch_losses = [0.5 * torch.sum(z ** 2, dim=1).mean(), -log_jacobian.mean()]
        sum(batch_losses).backward()
        if optimizer != "clampadam":
            for p in params_trainable:
                p.grad.data.clamp_(-5.00, 5.00)
        optim.step()
        losses.append([l.item() for l in batch_losses])
    with torch.no_grad():
        x, c = to_dev(bt[4][0]), to_dev(bt[4][1])
        z = model(x, c=c)
        nll = float(0.5 * torch.sum(z ** 2, dim=1).mean() - model.log_jacobian(run_forward=False).mean()) \
            + 0.5 * d * math.log(2 * math.pi)
    st = [optim.state[p] for p in params_trainable]
    check_poisoned(f"module route {flow_name} {optimizer}", losses, nll,
                   ([p.detach() for p in params_trainable], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st]),
                   ref["losses"], flow_ref32(flow_name))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("spoil_in", ["x", "y"])
def test_conditional_trainer_poisoned_step_poisons_the_model(spoil_in, use_graph):
    """ConditionalFlowTrainer on a small two-lane model, the NaN row once in x and once in y, against the statements of
    train_conditional.py:120-150 on oracle blocks in float64 (OracleComposition of test_gpu_conditional.py)"""
    from test_gpu_conditional import OracleComposition
    torch.manual_seed(4)
    nx, ny, nb, hidden, B = 10, 3, 2, 24, nf.POISON_B
    m = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden).to(DEV)
    for p in m.parameters():
        p.data.add_(0.02 * torch.randn_like(p))
    g = torch.Generator().manual_seed(17)
    bt = [(torch.randn(B, nx, generator=g), torch.randn(B, ny, generator=g)) for _ in range(5)]
    (bt[2][0] if spoil_in == "x" else bt[2][1])[nf.POISON_ROW] = nf.NAN
    refs = {}
    for dt in (torch.float64, torch.float32):
        oc = OracleComposition(m, dtype=dt)
        oc.make_optimizer(ss.LR)
        n = 4 if dt == torch.float64 else 2
        refs[dt] = np.array([oc.train_step(x, y)[0] for x, y in bt[:n]], dtype=np.float64)
        if dt == torch.float64:
            with torch.no_grad():
                xo, yo, jx, jy, _ = oc.forward(*bt[4])
            ref_nll = float(0.5 * (torch.cat([xo, yo], dim=-1) ** 2).sum(1).mean() - (jx + jy).mean())
            assert not np.isfinite(refs[dt].sum(axis=1)[2:]).any() and not math.isfinite(ref_nll)   # the reference is poisoned
            assert any(bool(torch.isnan(p).any()) for p in oc.plist)
    tr = hint_amd.ConditionalFlowTrainer(m, noise=0.0, use_graph=use_graph)
    losses = []
    for x, y in bt[:4]:
        l0, l1 = tr.step(x.to(DEV), y.to(DEV))
        losses.append([float(l0), float(l1)])
    with torch.no_grad():
        z_y, z_x = m([bt[4][1].to(DEV), bt[4][0].to(DEV)])
        z = torch.cat([z_x, z_y], dim=-1)
        nll = float(0.5 * torch.sum(z ** 2, dim=1).mean() - m.log_jacobian(run_forward=False).mean())
    torch.cuda.synchronize()
    check_poisoned(f"ConditionalFlowTrainer spoiled {spoil_in} graph={use_graph}", losses, nll, (tr.P, tr.M, tr.V),
                   refs[torch.float64], refs[torch.float32])
