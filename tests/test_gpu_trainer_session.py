"""GPU tests of trainer SESSIONS: FlowTrainer and ConditionalFlowTrainer keep state between calls - a captured graph per batch
shape, chains per batch size, a device step counter, Adam's factors, loss accumulators, pack keys - and a real run changes the
batch shape, evaluates, samples and decays the learning rate between steps.  The scripts of tests/session_script.py do that on one
live trainer; every compared quantity is checked against float64 oracle training of the same session, at the tolerances
tests/test_session_script_cpu.py calibrates (4 x the float32 oracle's own deviation).  Also: the trainers' input contract."""
import copy

import numpy as np
import pytest
import torch

import hint_amd
import session_script as ss
from hint_amd.hint import HintAmdError
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build_trainer(flow_name, use_graph, noise=0.0, seed=None):
    spec = ss.FLOWS[flow_name]
    params, perms = ss.initial_weights(spec)
    flow = hint_amd.HintFlow(spec["d"], spec["n_blocks"], list(spec["widths"]), ndim_c=spec["dc"])
    for i, blk in enumerate(flow.blocks):
        blk.load_state_dict({k: v.clone() for k, v in params[i].items()})
        if perms[i] is not None:
            flow.perms[i].W.copy_(perms[i])
    flow = flow.to(DEV)
    return hint_amd.FlowTrainer(flow, noise=noise, use_graph=use_graph, use_chain=spec["use_chain"], seed=seed)


def to_dev(t):
    return t.to(DEV) if t is not None else None


class TrainerBackend:
    """session_script.run_session's events on a live FlowTrainer; after every event the device-side step state is checked
    against the host's"""

    def __init__(self, tr, hook=None):
        self.tr, self.hook = tr, hook
        self.lr_of_last_step = None

    def step(self, x, c):
        self.lr_of_last_step = self.tr.lr
        l0, l1 = self.tr.step(to_dev(x), to_dev(c))
        return [float(l0), float(l1)]

    def input_buffers(self, x, c):
        tr = self.tr
        xd, cd = to_dev(x), to_dev(c)
        bx, bc = tr.input_buffers(torch.zeros_like(xd), torch.zeros_like(cd) if cd is not None else None)
        if tr.use_graph:
            assert bx is tr._static["x"] and bc is tr._static["c"]
        bx.copy_(xd)                              # the "data pipeline" writes the batch in place
        if bc is not None:
            bc.copy_(cd)
        self.lr_of_last_step = tr.lr
        l0, l1 = tr.step(bx, bc)
        return [float(l0), float(l1)]

    def step_many(self, xs, cs):
        self.lr_of_last_step = self.tr.lr
        self.tr.step_many(to_dev(xs), to_dev(cs))
        return self.tr.step_losses().cpu().numpy().astype(np.float64).tolist()

    def eval_nll(self, x, c):
        return self.tr.nll(to_dev(x), to_dev(c))

    def sample(self, z, c):
        x, J = self.tr.sample(to_dev(z), to_dev(c))
        return x.cpu().numpy().astype(np.float64), J.cpu().numpy().astype(np.float64)

    def module_forward(self, x, c):
        flow = self.tr.flow
        with torch.enable_grad():                 # the autograd route's forward (its own pooled chain and tapes), no backward
            z = flow(to_dev(x), c=to_dev(c))
            J = flow.log_jacobian(run_forward=False)
        return z.detach().cpu().numpy().astype(np.float64), J.detach().cpu().numpy().astype(np.float64)

    def set_lr(self, factor):
        self.tr.lr = self.tr.lr * factor

    def repack(self, scale):
        with torch.no_grad():
            for p in self.tr.flow.parameters():
                p.mul_(scale)
        self.tr.repack()

    def after_event(self, i, ev):
        tr = self.tr
        t = tr.step_count
        assert int(tr.rng_state[1]) == t, (i, ev, int(tr.rng_state[1]), t)
        if t > 0:
            # Adam's factors of the step that ran last, as its prologue wrote them (a learning-rate change shows at the next step)
            f1, f2 = ss.adam_factors(self.lr_of_last_step, t)
            got = tr.opt_state.double().cpu().numpy()
            assert abs(got[3] - f1) <= 1e-6 * f1 and abs(got[4] - f2) <= 1e-6 * f2, (i, ev, t, got[3], f1, got[4], f2)
        if self.hook is not None:
            self.hook(i, ev)


def named_arena(tr, arena):
    """-> per block {state_dict key: the slice of a flat arena (M, V, G) that belongs to that parameter}"""
    out = []
    for eng, (a, b), blk in zip(tr.engines, tr.slices, tr.flow.blocks):
        names = {id(p): n for n, p in blk.named_parameters()}
        out.append({names[id(p)]: v.detach().cpu().numpy().astype(np.float64) for p, v in zip(eng.params, eng.split_flat(arena[a:b]))})
    return out


def fwd_close(got, ref, what):
    """TOL_FWD of test_gpu_instances.py: of the largest magnitude (at least 1)"""
    d = float(np.abs(got - ref).max())
    lim = ss.TOL_FWD * max(1.0, float(np.abs(ref).max()))
    print(f"    {what}: max deviation {d:.2e} (limit {lim:.2e})")
    return [] if d <= lim else [(what, d, lim)]


def compare_session(tr, rec, script, flow_name, noise=0.0):
    """every compared quantity of a finished session against the float64 oracle's; prints each figure, returns the misses"""
    ref, tol = ss.reference(script, flow_name, noise), ss.tolerances(script, flow_name, noise)
    bad = []
    assert ref["dropped"] <= ss.MAX_DROPPED * ref["picked"], (ref["dropped"], ref["picked"])     # the kink rule stays a rare exception
    step_dev = np.max(np.abs(rec["losses"] - ref["losses"]) / (0.1 + np.abs(ref["losses"])), axis=1)
    print(f"\n{script}/{flow_name} graph={tr.use_graph}: tolerances " + " ".join(f"{k}={v:.2e}" for k, v in tol.items()))
    print("    loss pair deviation per step: " + " ".join(f"{v:.1e}" for v in step_dev))
    if step_dev.max() > tol["losses"]:
        bad.append(("losses", int(step_dev.argmax()), float(step_dev.max()), tol["losses"]))
    if len(ref["nll"]):
        nll_dev = np.abs(rec["nll"] - ref["nll"]) / (0.1 + np.abs(ref["nll"]))
        print("    nll deviation per evaluation: " + " ".join(f"{v:.1e}" for v in nll_dev))
        if nll_dev.max() > tol["nll"]:
            bad.append(("nll", int(nll_dev.argmax()), float(nll_dev.max()), tol["nll"]))
    for n, ((x, J), (xr, Jr)) in enumerate(zip(rec["samples"], ref["samples"])):
        bad += fwd_close(x, xr, f"sample {n} x") + fwd_close(J, Jr, f"sample {n} J")
    for n, ((z, J), (zr, Jr)) in enumerate(zip(rec["forwards"], ref["forwards"])):
        bad += fwd_close(z, zr, f"module forward {n} z") + fwd_close(J, Jr, f"module forward {n} J")
    assert len(rec["samples"]) == len(ref["samples"]) and len(rec["forwards"]) == len(ref["forwards"])
    final = [{k: v.detach().cpu().numpy().astype(np.float64) for k, v in blk.state_dict().items()} for blk in tr.flow.blocks]
    upd = ss.update_devs(ref["initial"], final, ref["final"])
    worst = max(upd, key=upd.get)
    print(f"    update vector: worst tensor {worst} {upd[worst]:.2e}")
    bad += [("update", k, v, tol["update"]) for k, v in upd.items() if v > tol["update"]]
    torch.cuda.synchronize()
    g_max = float(tr.G.abs().max())
    print(f"    gradient arena after the session: max |G| = {g_max:.1e}")
    if g_max != 0.0:
        bad.append(("G", g_max))
    M, V = named_arena(tr, tr.M), named_arena(tr, tr.V)
    mdev = {(bi, k): max(ss.norm_dev(M[bi][k], m), ss.norm_dev(V[bi][k], v))
            for bi, blk in enumerate(ref["moments"]) for k, (m, v) in blk.items()}
    worst = max(mdev, key=mdev.get)
    print(f"    Adam moments: worst tensor {worst} {mdev[worst]:.2e}")
    bad += [("moments", k, v, tol["update"]) for k, v in mdev.items() if v > tol["update"]]
    return bad


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("flow_name", list(ss.FLOWS))
@pytest.mark.parametrize("script", list(ss.SCRIPTS))
def test_session_matches_float64_oracle_training(script, flow_name, use_graph):
    """a whole session on one live trainer: every step's loss pair, every evaluation NLL, every sample and module forward, the
    update vector of every tensor and Adam's moments against float64 oracle training; after every event the device step counter
    equals the host's and opt_state holds that step's factors"""
    tr = build_trainer(flow_name, use_graph)
    assert tr._chainable == ss.FLOWS[flow_name]["use_chain"]
    rec = ss.run_session(script, ss.FLOWS[flow_name], TrainerBackend(tr), ss.reference(script, flow_name)["rows"])
    assert tr.step_count == len(rec["losses"])
    bad = compare_session(tr, rec, script, flow_name)
    assert not bad, bad


NOISY = [(s, f, g) for (s, f) in ss.NOISY_SESSIONS for g in ((True, False) if s == "epochs" else (True,))]


@pytest.mark.parametrize("script,flow_name,use_graph", NOISY, ids=[f"{s}-{f}-{'graph' if g else 'eager'}" for s, f, g in NOISY])
def test_noisy_session_matches_float64_oracle_training(script, flow_name, use_graph):
    """the sessions with the training noise ON (the trainers' default; every other oracle comparison turns it off): the oracle
    trains step t on x + noise * normals(seed, t) of tests/noise_oracle.py, the trainer draws in its forward kernel - the same
    comparisons as the noise-free sessions (loss pairs, NLLs, samples, forwards, update vectors, moments, the device counter and
    Adam's factors after every event), at tolerances calibrated the same way.  `epochs` on every flow, captured and eager -
    block-by-block launches included, where the first block's launch draws; `mixed` (step_many) on the captured trainer"""
    noise = ss.NOISY_SESSIONS[(script, flow_name)]
    tr = build_trainer(flow_name, use_graph, noise=noise, seed=ss.NOISE_SEED)
    assert tr._chainable == ss.FLOWS[flow_name]["use_chain"] and int(tr.rng_state[0]) == ss.NOISE_SEED
    rec = ss.run_session(script, ss.FLOWS[flow_name], TrainerBackend(tr), ss.reference(script, flow_name, noise)["rows"])
    assert tr.step_count == len(rec["losses"])
    bad = compare_session(tr, rec, script, flow_name, noise)
    assert not bad, bad


@pytest.mark.parametrize("flow_name", ["wl_d6", "gen_d43"])
def test_graph_and_eager_twins_draw_the_same_noise(flow_name):
    """the same seed, noise on: the captured trainer (whose every re-capture runs two warm-up prologues) and the eager one see the
    same noise stream and bias corrections at every step of the epochs script - the steps behind each re-capture included"""
    recs = {}
    for use_graph in (True, False):
        tr = build_trainer(flow_name, use_graph, noise=0.01, seed=1234)
        recs[use_graph] = ss.run_session("epochs", ss.FLOWS[flow_name], TrainerBackend(tr),
                                         ss.reference("epochs", flow_name)["rows"])["losses"]
    print("\ngraph:", recs[True].tolist(), "\neager:", recs[False].tolist())
    assert np.allclose(recs[True], recs[False], rtol=1e-5, atol=1e-6), np.abs(recs[True] - recs[False]).max(axis=1)
    # (and the noise is on: the noise-free oracle's losses are not these)
    assert not np.allclose(recs[True], ss.reference("epochs", flow_name)["losses"], rtol=1e-5, atol=1e-6)


def test_chain_eviction_keeps_the_live_graph():
    """many_sizes: step() walks through more batch sizes than the trainer keeps chains for while the step_many graph captured at
    the first size is live; that size's chain is never rebuilt, and the return to it takes the oracle's steps"""
    script, flow_name = "many_sizes", "wl_d6"
    tr = build_trainer(flow_name, True)
    events = ss.SCRIPTS[script]
    first = events[0][2]
    seen = {"handle": None, "sizes": set(), "most": 0}

    def hook(i, ev):
        assert len(tr._chains) <= 8, (i, ev, sorted(tr._chains))
        seen["most"] = max(seen["most"], len(tr._chains))
        if ev[0] in ("step", "step_many"):
            seen["sizes"].add(ev[-1])
        assert tr._graph_many is not None and tr._static_many["x"].shape[1] == first
        entry = tr._chains[first]
        if seen["handle"] is None:
            seen["handle"] = (entry[0], entry[0].value, entry[2][0].data_ptr())
        assert entry[0] is seen["handle"][0] and entry[0].value == seen["handle"][1], (i, ev)       # never rebuilt ...
        assert entry[2][0].data_ptr() == seen["handle"][2], (i, ev)                                   # ... its tapes where they were

    rec = ss.run_session(script, ss.FLOWS[flow_name], TrainerBackend(tr, hook), ss.reference(script, flow_name)["rows"])
    assert len(seen["sizes"]) > 8 and seen["most"] == 8        # the eviction did run
    ref, tol = ss.reference(script, flow_name), ss.tolerances(script, flow_name)
    back = [k for k, ev in enumerate(events) if ev == events[0]][1]          # the second step_many at the first size
    n_before = sum(ev[1] if ev[0] == "step_many" else 1 for ev in events[:back] if ev[0] in ("step", "step_many"))
    rows = slice(n_before, n_before + events[0][1] + 1)                       # its iterations and the step() behind them
    dev = ss.scalar_dev(rec["losses"][rows], ref["losses"][rows])
    print(f"\nreturn to the first size: loss pair deviation {dev:.2e} (tolerance {tol['losses']:.2e})")
    assert dev <= tol["losses"]


def _steps(tr, batches, many=False):
    out = []
    for x, c in batches:
        if many:
            tr.step_many(x, c)
            out += tr.step_losses().cpu().numpy().tolist()
        else:
            l0, l1 = tr.step(x, c)
            out.append([float(l0), float(l1)])
    torch.cuda.synchronize()
    return np.array(out)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_strided_and_typed_inputs_equal_their_contiguous_copy(use_graph):
    """any strides and any floating dtype give what the contiguous fp32 copy gives.  Before the trainers validated their inputs,
    clone() / empty_like() kept a dense transpose's strides and the kernels read column-major memory as rows (NOTES.md §11): the
    transposed cases are the ones that code misses."""
    g = torch.Generator().manual_seed(21)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    B, K = 192, 3
    spec = ss.FLOWS["wl_d6"]
    d = spec["d"]
    wide = rnd(B, d + 5)
    cases = {
        "transposed dense batch": ([(rnd(d, B).t(), None) for _ in range(3)], False),
        "column slice of a wider table": ([(wide[:, 2:2 + d], None), (wide[:, 5:5 + d], None)], False),
        "[B, K, d] table transposed for step_many": ([(rnd(B, K, d).transpose(0, 1), None) for _ in range(2)], True),
        "float64 batch": ([(rnd(B, d).double(), None) for _ in range(2)], False),
        "float16 batch": ([(rnd(B, d).half(), None) for _ in range(2)], False),
    }
    for what, (batches, many) in cases.items():
        assert not all(x.is_contiguous() and x.dtype == torch.float32 for x, _ in batches)
        t1, t2 = build_trainer("wl_d6", use_graph), build_trainer("wl_d6", use_graph)
        got = _steps(t1, batches, many)
        want = _steps(t2, [(x.float().contiguous(), None) for x, _ in batches], many)
        print(f"\n{what} (graph={use_graph}): first loss pair {got[0].tolist()} / contiguous copy {want[0].tolist()}, "
              f"largest relative deviation {np.max(np.abs(got - want) / np.abs(want)):.2e}")
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (what, got, want)
        assert rel_err(t1.P.cpu().numpy(), t2.P.cpu().numpy()) < 1e-4, what
        if use_graph:       # the captured step with the optimizer folded in is deterministic (test_optimizer_folded_into_the_reduction_...)
            assert torch.equal(t1.P, t2.P) and torch.equal(t1.M, t2.M) and torch.equal(t1.V, t2.V), what
    # a strided condition, in step() and in sample()
    spec = ss.FLOWS["cond_d9"]
    d, dc = spec["d"], spec["dc"]
    t1, t2 = build_trainer("cond_d9", use_graph), build_trainer("cond_d9", use_graph)
    batches = [(rnd(B, d), rnd(dc, B).t()), (rnd(d, B).t(), rnd(B, 2 * dc)[:, ::2]), (rnd(B, d), rnd(B, dc).double())]
    got = _steps(t1, batches)
    want = _steps(t2, [(x.float().contiguous(), c.float().contiguous()) for x, c in batches])
    print(f"\nstrided c (graph={use_graph}): {got.tolist()} / contiguous copy {want.tolist()}")
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
    assert rel_err(t1.P.cpu().numpy(), t2.P.cpu().numpy()) < 1e-4
    if use_graph:
        assert torch.equal(t1.P, t2.P)
    t2.P.copy_(t1.P)                                    # the same weights for the two sample() calls
    t2.repack()
    z, c = rnd(d, 77).t(), rnd(dc, 77).t()
    x1, J1 = t1.sample(z, c)
    x2, J2 = t2.sample(z.contiguous(), c.contiguous())
    assert torch.equal(x1, x2) and torch.equal(J1, J2)
    n1, n2 = t1.nll(z.double(), c), t2.nll(z.contiguous(), c.contiguous())
    assert n1 == n2, (n1, n2)


def test_strided_and_typed_inputs_conditional_trainer():
    """ConditionalFlowTrainer, graph and eager: transposed x, strided and float64 y against their contiguous fp32 copies"""
    g = torch.Generator().manual_seed(22)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    nx, ny, nb, hidden, B = 10, 3, 2, 24, 160
    torch.manual_seed(4)
    m0 = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden).to(DEV)
    for p in m0.parameters():
        p.data.add_(0.02 * torch.randn_like(p))
    batches = [(rnd(nx, B).t(), rnd(B, ny)), (rnd(B, nx), rnd(B, 2 * ny)[:, ::2]), (rnd(B, nx).double(), rnd(ny, B).t().double())]
    for use_graph in (True, False):
        out = []
        for contiguous in (False, True):
            m = copy.deepcopy(m0)
            tr = hint_amd.ConditionalFlowTrainer(m, noise=0.0, use_graph=use_graph)
            losses = []
            for x, y in batches:
                if contiguous:
                    x, y = x.float().contiguous(), y.float().contiguous()
                l0, l1 = tr.step(x, y)
                losses.append([float(l0), float(l1)])
            torch.cuda.synchronize()
            out.append((np.array(losses), tr.P.clone(), tr.M.clone(), tr.V.clone()))
        same = [torch.equal(a, b) for a, b in zip(out[0][1:], out[1][1:])]
        print(f"\nconditional (graph={use_graph}): {out[0][0].tolist()} / contiguous copy {out[1][0].tolist()}; "
              f"P, M, V bit-identical: {same}")
        assert np.allclose(out[0][0], out[1][0], rtol=1e-5, atol=1e-6)
        for a, b in zip(out[0][1:], out[1][1:]):
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-4
        if use_graph:       # weight gradients are reduced slab by slab in a fixed order and clamp + Adam ride in that reduction:
            assert all(same), same          # only the two loss sums take float atomics, and nothing reads them back


class _NoLaunch:
    """stands in for the C library: touching it at all fails the test (a refusal must come before any library call)"""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} on a refused input")


def test_refused_inputs_launch_nothing():
    B = 32
    tr = build_trainer("wl_d6", True)
    trc = build_trainer("cond_d9", False)
    d, dcond, dc = 6, 9, 2
    x, xc, c = torch.randn(B, d, device=DEV), torch.randn(B, dcond, device=DEV), torch.randn(B, dc, device=DEV)
    xs = torch.randn(2, B, d, device=DEV)
    tr.step(x)                                    # live state: a captured graph the refusals must leave alone
    trc.step(xc, c)
    torch.manual_seed(4)
    m = hint_amd.ConditionalHintFlow(10, 3, 2, 24).to(DEV)
    ctr = hint_amd.ConditionalFlowTrainer(m, noise=0.0, use_graph=True)
    cx, cy = torch.randn(B, 10, device=DEV), torch.randn(B, 3, device=DEV)
    ctr.step(cx, cy)
    torch.cuda.synchronize()
    before = (tr.step_count, tr.P.clone(), ctr.step_count, ctr.P.clone())
    # (every object that holds a library handle of its own: the trainers, their runners, and the re-pack groups of both)
    libs = [(o, o.lib) for o in (tr, tr._runner, tr._runner._pack_group, trc, trc._runner, trc._runner._pack_group,
                                 ctr, ctr._pack_group)]
    for o, _ in libs:
        o.lib = _NoLaunch()
    try:
        single = (tr.step, tr.input_buffers, tr.sample, tr.nll, tr.timed_step)
        refused = []
        for f in single:
            refused += [(f, (x.cpu(),)),                                     # not on the trainer's device
                        (f, (x[0],)), (f, (xs,)),                            # wrong rank
                        (f, (x[:, :5],)), (f, (torch.randn(B, d + 1, device=DEV),)),     # wrong lane width
                        (f, (x, c)),                                         # c for an unconditional flow
                        (f, (x.long(),)), (f, (x.cpu().numpy(),))]           # not a floating tensor
        for f in (tr.step_many, tr.input_buffers_many):
            refused += [(f, (xs.cpu(),)), (f, (x,)), (f, (xs[:, :, :5],)), (f, (xs, torch.randn(2, B, dc, device=DEV)))]
        for f in (trc.step, trc.input_buffers, trc.sample, trc.nll):
            refused += [(f, (xc,)),                                          # c missing for a conditional flow
                        (f, (xc, c.cpu())), (f, (xc.cpu(), c)),
                        (f, (xc, c[:-1])), (f, (xc, c[:1])),                 # c's row count differs from x's
                        (f, (xc, c[:, :1])), (f, (xc, c[:, 0]))]
        refused += [(trc.step_many, (xc.unsqueeze(0), c))]                   # [K, B, d] with a [B, dc] condition
        for f in (ctr.step, ctr.input_buffers):
            refused += [(f, (cx.cpu(), cy)), (f, (cx, cy.cpu())), (f, (cx, cy[:-1])), (f, (cx[:, :9], cy)), (f, (cx, cy[:, :2])),
                        (f, (cx[0], cy)), (f, (cx, cy.long()))]
        for f, args in refused:
            with pytest.raises(HintAmdError):
                f(*args)
    finally:
        for o, lib in libs:
            o.lib = lib
    assert (tr.step_count, ctr.step_count) == (before[0], before[2])
    assert torch.equal(tr.P, before[1]) and torch.equal(ctr.P, before[3])
    l0, _ = tr.step(x)                            # and the trainers go on
    ctr.step(cx, cy)
    assert np.isfinite(float(l0))


# ---- ConditionalFlowTrainer: a short session against the float64 composition of oracle blocks ----------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_conditional_trainer_session_matches_float64_oracle(use_graph):
    """two batch sizes and back, a learning-rate change and sample_conditional between steps on one live ConditionalFlowTrainer:
    loss pairs (rtol 1e-4 / atol 1e-5) and the update vector of every tensor (5e-2, check_update) as
    test_trainer_reproduces_reference_adam_steps grants them, samples as test_conditional_flow_matches_oracle_composition
    (1e-4); the device step counter follows the host's"""
    torch.manual_seed(4)
    nx, ny, nb, hidden = 10, 3, 2, 24
    m = hint_amd.ConditionalHintFlow(nx, ny, nb, hidden).to(DEV)
    for p in m.parameters():
        p.data.add_(0.02 * torch.randn_like(p))
    from test_gpu_conditional import OracleComposition          # the float64 composition of oracle blocks, its clamp + Adam
    lr = ss.LR
    ref = OracleComposition(m, torch.float64)
    ref.make_optimizer(lr, betas=ss.BETAS, eps=ss.EPS, weight_decay=ss.WD)
    initial = {n: {k: v.detach().clone().numpy() for k, v in d_.items()} for n, d_ in ref.P.items()}
    tr = hint_amd.ConditionalFlowTrainer(m, noise=0.0, use_graph=use_graph, lr=lr)
    g = torch.Generator().manual_seed(23)
    events = [("step", 256), ("step", 256), ("step", 100), ("sample", 64), ("step", 100), ("set_lr", 0.5), ("step", 256),
              ("sample", 256), ("step", 256), ("step", 100)]
    t = 0
    for i, ev in enumerate(events):
        if ev[0] == "step":
            x, y = torch.randn(ev[1], nx, generator=g), torch.randn(ev[1], ny, generator=g)
            l0, l1 = tr.step(x.to(DEV), y.to(DEV))
            got, want = [float(l0), float(l1)], ref.train_step(x, y)[0]
            t += 1
            print(f"\nstep {t} (B={ev[1]}): {got} / oracle {want}")
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=f"event {i} {ev}")
            if use_graph:       # (the eager trainer steps Adam from the host: its factors never pass through opt_state)
                f1, f2 = ss.adam_factors(lr, t)
                o = tr.opt_state.double().cpu().numpy()
                assert abs(o[3] - f1) <= 1e-6 * f1 and abs(o[4] - f2) <= 1e-6 * f2, (i, ev, o, f1, f2)
        elif ev[0] == "set_lr":
            lr = lr * ev[1]
            tr.lr = lr
            for grp in ref.opt.param_groups:
                grp["lr"] = lr
        else:
            y, zx = torch.randn(ev[1], ny, generator=g), torch.randn(ev[1], nx, generator=g)
            xg, Jg = m.sample_conditional(y.to(DEV), zx.to(DEV))
            xo, Jo = (t_.numpy() for t_ in ref.sample_conditional(y, zx))
            np.testing.assert_allclose(xg.cpu().numpy(), xo, rtol=1e-4, atol=1e-4, err_msg=f"event {i} {ev}")
            np.testing.assert_allclose(Jg.cpu().numpy(), Jo, rtol=1e-4, atol=1e-4, err_msg=f"event {i} {ev}")
        assert tr.step_count == t and int(tr.rng_state[1]) == t, (i, ev, tr.step_count, int(tr.rng_state[1]))
    assert (tr._graph is not None) == use_graph
    for n, sub, _ in ref.mods:
        sd = sub.state_dict()
        for k, p in ref.P[n].items():
            dev = ss.norm_dev(sd[k].detach().cpu().double().numpy() - initial[n][k], p.detach().numpy() - initial[n][k])
            assert dev < 5e-2, (n, k, dev)
            assert rel_err(sd[k].detach().cpu().numpy(), p.detach().numpy()) < 1e-3, (n, k)
