"""Device tests of the plus-shape fit (hint_amd.curves plus_fit_grad / plus_dominant_angle / plus_fit_starts / fit_plus_shapes,
hint_plusfit_run) against the float64 restatement and the rules of tests/plusfit_oracle.py:
  1. loss and gradient of single evaluations (n_steps = 0) and of every traced step of a 400-step fit, on decided evaluations;
  2. the update rule on every traced step, decided or not, and the selection, bit for bit;
  3. short fits (1, 2, 5 steps) against fit64 from the same starts;
  4. whole fits against fit64 and against what the reference returned;
  5. the early stop; 6. the starts and the angle; 7. invariance, guard-banded outputs, non-finite inputs, graph capture, P = 2.
Sizes: P in 2, 100, 257, 1024; N in 1, 3, 9; S in 1, 2, 3, 9; max_groups in 0, 1, 2."""
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import curves
import curve_oracle as co
import plusfit_oracle as pfo
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("params", "loss", "best", "n_run", "all_params", "all_loss", "grad", "trace")
INTS = ("best", "n_run")
FIT = dict(lr=pfo.LR, angle_lr=pfo.ANGLE_LR, gamma=pfo.GAMMA, momentum=pfo.MOMENTUM, corner_decay=True, stop_loss=0.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def run(curve, starts, n_steps=0, want=ALL, max_groups=0, out=None, c=1.0, P=pfo.FIT_P, **kw):
    """one hint_plusfit_run on device tensors; curve [N, 4K] is traced at P"""
    k = curve.shape[1] // 4 if curve.dim() == 2 else 0
    p = P if k else curve.shape[1]
    want = tuple(n for n in want if n != "trace" or n_steps > 0)
    args = dict(FIT)
    args.update(kw)
    return curves._pf_run(curve, k, p, starts, n_steps, corner_weight=c, want=want, max_groups=max_groups, out=out, **args)


def same_bits(a, b, names=None):
    for k in names or a.keys():
        if not (bits_equal(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k])):
            return False
    return True


def compare(name, b, dB, c, params, losses, grads):
    """device evaluations of a case's rows against evaluate64 at the device's own parameters: first the cap - at most 25 % of
    the case's evaluations may be undecided - then the decided ones against the bounds"""
    und, total, rl, rg = 0, 0, 0.0, np.zeros(9)
    for n in range(len(b)):
        cw = c[n] if isinstance(c, (list, tuple, np.ndarray)) else c
        u, l, g = pfo.compare_evaluations(b[n], dB[n], cw, params[n], losses[n], grads[n])
        und, total, rl, rg = und + u, total + len(params[n]), max(rl, l), np.maximum(rg, g)
    print(f"{name}: {und} of {total} evaluations undecided; worst error / bound: loss {rl:.3g}, gradient "
          f"{np.array2string(rg, precision=3)}")
    assert und <= 0.25 * total, (name, und, total)
    assert rl <= 1.0 and (rg <= 1.0).all(), (name, rl, rg)


# ---- 1. single evaluations ----
@pytest.mark.parametrize("name,source,P,N,S,c,zero,clamped", pfo.EVAL_CASES, ids=[e[0] for e in pfo.EVAL_CASES])
def test_loss_and_gradient_of_an_evaluation(name, source, P, N, S, c, zero, clamped):
    curve, b, dB, params = pfo.eval_case(source, P, N, S, 500 + P, zero, clamped)
    cd, sd = dev(curve), dev(params)
    for mg in (0, 1, 2):
        res = run(cd, sd, 0, c=c, P=P, max_groups=mg)
        if mg == 0:
            first = res
        assert same_bits(res, first)
    assert bits_equal(first["all_params"], sd)                            # n_steps = 0: the starts themselves
    assert (first["n_run"] == S).all()                                    # stop_loss = 0 never stops
    L, G = host(first["all_loss"]), host(first["grad"])
    if P > 2:
        compare(f"evaluation {name}", b, dB, c, params, L, G)
    else:
        assert np.isfinite(L).all() and np.isfinite(G).all()
    best = host(first["best"])
    for n in range(N):
        assert best[n] == pfo._select(L[n], S)
    rows = torch.arange(N, device=DEV)
    assert bits_equal(first["loss"], first["all_loss"][rows, first["best"].long()])
    assert bits_equal(first["params"], first["all_params"][rows, first["best"].long()])
    # the loss is the two terms of hint_plus_run, combined once in double: within two fp32 roundings of the host's combination
    terms = host(curves._plus_run(sd[:, 0].contiguous(), cd, curve.shape[1] // 4 if cd.dim() == 2 else 0, P,
                                  want=("loss",))["loss"]).astype(np.float64)
    comb = terms[:, 0] + c * terms[:, 1]
    assert (np.abs(L[:, 0] - comb) <= 2 * 2 * pfo.U * (np.abs(terms[:, 0]) + abs(c) * np.abs(terms[:, 1]))).all()


def test_plus_fit_grad_is_the_evaluation():
    curve, b, dB, params = pfo.eval_case("traced", 100, 5, 1, 77, (), ())
    cd, sd = dev(curve), dev(params[:, 0])
    for c in (1.0, 0.37, 0.0):
        loss, grad = hint_amd.plus_fit_grad(cd, sd, c)
        res = run(cd, dev(params), 0, c=c)
        assert loss.shape == (5,) and grad.shape == (5, 9)
        assert bits_equal(loss, res["all_loss"][:, 0]) and bits_equal(grad, res["grad"][:, 0])
        old = hint_amd.plus_fit_loss(cd, sd, c)
        assert np.abs(host(old).astype(np.float64) - host(loss)).max() <= 4 * pfo.U * np.abs(host(loss)).max()
    one = hint_amd.plus_fit_grad(cd, sd[2], 1.0)                          # [9] params serve every row
    assert bits_equal(one[0][2:3], hint_amd.plus_fit_grad(cd, sd, 1.0)[0][2:3])
    with pytest.raises(hint_amd.HintAmdError, match="plus_fit_grad: params requires grad"):
        hint_amd.plus_fit_grad(cd, sd.clone().requires_grad_(True))


def test_golden_gradients_of_the_reference():
    g = np.load(os.path.join(ROOT, "tests", "golden", f"plusfit_{pfo.GOLDEN_GRAD['name']}.npz"))
    x, params = g["x"], g["params"]
    b, dB = co.points64(x, pfo.FIT_P), pfo.delta_B(x)
    for w, c in enumerate(pfo.GOLDEN_GRAD["weights"]):
        loss, grad = hint_amd.plus_fit_grad(dev(x), dev(params), c)
        compare(f"golden gradients c = {c}", b, dB, c, params[:, None], host(loss)[:, None], host(grad)[:, None])
        # and against the reference's own numbers, at the bounds plus what evaluate64 deviates from it (CPU test: 1e-12)
        for n in range(len(x)):
            _, g64, info = pfo.evaluate64(b[n], params[n], c)
            E = pfo.bound_E(info, dB[n])
            if pfo.undecided(info, E):
                continue
            assert (np.abs(host(grad)[n] - g["ref_grad"][n, w]) <= pfo.grad_bound(g64, info, E, c) + 1e-12).all(), n
            assert abs(host(loss)[n] - g["ref_loss"][n, w]) <= pfo.loss_bound(info, E, c) + 1e-12


# ---- the traced source is the given one, bit for bit, at every size ----
@pytest.mark.parametrize("P", (2, 100, 257, 1024))
def test_the_traced_source_gives_the_bits_of_the_given_one(P):
    N, S, steps = 3, 2, 5
    x, base = pfo.plus_rows(600 + P, N)
    xd = dev(x)
    pts = hint_amd.trace_fourier_curves(xd, P)
    starts = dev(np.stack([pfo.eval_params(base, 601 + P + s) for s in range(S)], 1))
    a, b = run(xd, starts, steps, P=P), run(pts, starts, steps)
    assert same_bits(a, b)
    assert torch.isfinite(a["trace"]).all() and torch.isfinite(a["params"]).all()
    for s in range(S):
        for n in range(N):
            assert pfo.check_update_rule(host(a["trace"][n, s]), host(a["all_params"][n, s])) <= 1.0


# ---- 1b and 2. every step of a 400-step fit ----
@pytest.fixture(scope="module")
def long_fit():
    N = 3
    x, _ = pfo.plus_rows(701, N)
    xd = dev(x)
    starts = hint_amd.plus_fit_starts(xd)[:, :2].contiguous()
    params, loss, extra = hint_amd.fit_plus_shapes(xd, starts=starts, stop_loss=0.0, return_all=True, return_trace=True)
    return x, starts, dict(params=params, loss=loss, **extra)


def test_every_traced_step_of_a_fit_against_float64(long_fit):
    x, starts, res = long_fit
    b, dB = co.points64(x, pfo.FIT_P), pfo.delta_B(x)
    tr = host(res["trace"])
    assert tr.shape == (3, 2, 400, 19)
    t = tr.reshape(3, -1, 19)
    cw = np.tile(1.0 - np.arange(400) / 400, 2)                           # the corner weight of step i, checked through the loss
    compare("traced steps", b, dB, [cw] * 3, t[:, :, :9], t[:, :, 9], t[:, :, 10:])


def test_update_rule_on_every_step_and_the_selection_bit_for_bit(long_fit):
    x, starts, res = long_fit
    tr, ap = host(res["trace"]), host(res["all_params"])
    assert bits_equal(res["trace"][:, :, 0, :9], starts)                  # a fit begins at its start
    worst = 0.0
    for n in range(3):
        for s in range(2):
            worst = max(worst, pfo.check_update_rule(tr[n, s], ap[n, s]))
    print(f"update rule: worst error {worst:.3g} ulp")
    assert worst <= 1.0
    assert bits_equal(res["all_loss"], res["trace"][:, :, -1, 9])         # the loss of the last step before its update
    al = host(res["all_loss"])
    rows = torch.arange(3, device=DEV)
    for n in range(3):
        assert host(res["best"])[n] == pfo._select(al[n], 2) and host(res["n_run"])[n] == 2
    assert bits_equal(res["loss"], res["all_loss"][rows, res["best"].long()])
    assert bits_equal(res["params"], res["all_params"][rows, res["best"].long()])
    params, loss = hint_amd.fit_plus_shapes(dev(x), starts=starts, stop_loss=0.0)
    assert bits_equal(params, res["params"]) and bits_equal(loss, res["loss"])
    full = run(dev(x), starts, 400)
    assert same_bits(full, res, ("params", "loss", "best", "n_run", "all_params", "all_loss", "trace"))
    assert bits_equal(full["grad"], res["trace"][:, :, -1, 10:])


# ---- 3. short fits ----
def _fit_case(seed, N, angle_of=None):
    x, _ = pfo.plus_rows(seed, N)
    b, b32 = co.points64(x, pfo.FIT_P), co.trace32(x, pfo.FIT_P)
    return x, b, b32


@pytest.mark.parametrize("steps", pfo.SHORT["steps"])
def test_short_fits_against_fit64(steps):
    N = pfo.SHORT["rows"]
    x, b, b32 = _fit_case(pfo.SHORT["seed"], N)
    st = np.stack([pfo.starts64(b[n], pfo.angle64(b[n])[0])[:3] for n in range(N)]).astype(np.float32)
    refs = [pfo.fit64(b[n], st[n], steps, stop_loss=0.0) for n in range(N)]
    tol = 16 * max(pfo.fit_dev(pfo.emulate32(b32[n], st[n], steps, stop_loss=0.0), refs[n]) for n in range(N))
    res = run(dev(x), dev(st), steps)
    devs = [pfo.fit_dev(dict(all_params=host(res["all_params"])[n], all_loss=host(res["all_loss"])[n]), refs[n]) for n in range(N)]
    print(f"{steps} steps: tolerance {tol:.3g} (16 x the emulation's largest deviation), device deviations " +
          ", ".join(f"{d:.3g}" for d in devs))
    assert tol < 1e-4 and max(devs) <= tol
    for n in range(N):
        al = np.sort(refs[n]["all_loss"])
        if al[1] - al[0] > 2 * tol:
            assert int(host(res["best"])[n]) == refs[n]["best"]


# ---- 4. whole fits ----
@pytest.mark.parametrize("which", ("fixture", "more"))
def test_whole_fits_against_fit64_and_the_reference(which):
    if which == "fixture":
        g = np.load(os.path.join(ROOT, "tests", "golden", f"plusfit_{pfo.GOLDEN_FIT['name']}.npz"))
        x = g["x"]
        xd = dev(x)
        angle = dev(g["ref_angle"].astype(np.float32))
    else:
        x, _ = pfo.plus_rows(pfo.WHOLE["seed"], pfo.WHOLE["rows"])
        xd = dev(x)
        angle = hint_amd.plus_dominant_angle(xd)
    N = len(x)
    starts = hint_amd.plus_fit_starts(xd, angle)                          # nine; the stop keeps most rows at one
    params, loss, extra = hint_amd.fit_plus_shapes(xd, starts=starts, return_all=True)
    st = host(starts)
    b, b32 = co.points64(x, pfo.FIT_P), co.trace32(x, pfo.FIT_P)
    refs = [pfo.fit64(b[n], st[n]) for n in range(N)]
    emus = [pfo.emulate32(b32[n], st[n]) for n in range(N)]
    ks = [min(e["n_run"], r["n_run"]) for e, r in zip(emus, refs)]
    tol_l = 16 * max(np.abs(e["all_loss"][:k] - r["all_loss"][:k]).max() for e, r, k in zip(emus, refs, ks))
    tol_p = 16 * max(pfo.param_diff(e["all_params"][:k], r["all_params"][:k]) for e, r, k in zip(emus, refs, ks))
    got = dict(params=host(params), loss=host(loss), **{k: host(v) for k, v in extra.items()})
    d_loss = d_par = 0.0
    for n in range(N):
        first = refs[n]["all_loss"][:refs[n]["n_run"]]
        if np.abs(first - pfo.STOP).min() > tol_l:                        # the deciding losses are clear of the threshold
            assert got["n_run"][n] == refs[n]["n_run"], n
        k = min(int(got["n_run"][n]), refs[n]["n_run"])
        d_loss = max(d_loss, np.abs(got["all_loss"][n, :k] - refs[n]["all_loss"][:k]).max())
        d_par = max(d_par, pfo.param_diff(got["all_params"][n, :k], refs[n]["all_params"][:k]))
    print(f"{which}: loss tolerance {tol_l:.3g}, device {d_loss:.3g}; parameter tolerance {tol_p:.3g}, device {d_par:.3g}; "
          f"starts run {got['n_run'].tolist()}")
    assert d_loss <= tol_l and d_par <= tol_p
    if which == "fixture":
        # the reference's own run from the same angle (fit64 against it: 2e-5, tests/test_plusfit_cpu.py)
        for n in range(N):
            if got["n_run"][n] == g["ref_n_run"][n]:
                assert pfo.param_diff(got["params"][n], g["ref_params"][n]) <= tol_p + 2e-5, n
        assert (got["n_run"] == g["ref_n_run"]).sum() >= N - 1


# ---- 5. early stop ----
def test_early_stop_leaves_the_remaining_starts_unrun():
    N, S, steps = 3, 3, 5
    x, base = pfo.plus_rows(901, N)
    xd = dev(x)
    starts = dev(np.stack([pfo.eval_params(base, 902 + s) for s in range(S)], 1))
    free = run(xd, starts, steps)
    al = host(free["all_loss"]).astype(np.float64)
    assert (host(free["n_run"]) == S).all()
    # midway between two observed losses of start 0: the rows below it stop after one start
    l0 = np.sort(al[:, 0])
    stop = float(0.5 * (l0[0] + l0[1]))
    res = run(xd, starts, steps, stop_loss=stop)
    want = np.array([next((s + 1 for s in range(S) if al[n, s] < stop), S) for n in range(N)])
    assert host(res["n_run"]).tolist() == want.tolist() and 1 in want and want.max() > 1
    qn = torch.tensor(0x7fc00000, dtype=torch.int32, device=DEV)
    for n in range(N):
        k = int(want[n])
        for name in ("all_params", "all_loss", "grad", "trace"):
            assert bits_equal(res[name][n, :k], free[name][n, :k]), (n, name)
        assert bits_equal(res["all_params"][n, k:], starts[n, k:])
        assert (res["all_loss"][n, k:] == float("inf")).all()
        assert (res["grad"][n, k:].contiguous().view(torch.int32) == qn).all()
        assert (res["trace"][n, k:].contiguous().view(torch.int32) == qn).all()
        assert int(res["best"][n]) == pfo._select(al[n], k)
    # a stop_loss that is <= 0 or NaN never stops; the comparison is strict
    for never in (0.0, -1.0, float("nan")):
        assert same_bits(run(xd, starts, steps, stop_loss=never), free)
    exact = run(xd, starts, steps, stop_loss=float(l0[0]))
    assert int(exact["n_run"][int(np.argmin(al[:, 0]))]) > 1


# ---- 6. starts and angle ----
def test_starts_and_angle_against_the_oracle():
    N = 12
    x, _ = pfo.plus_rows(1001, N)
    xd = dev(x)
    b = co.points64(x, pfo.FIT_P)
    S, dB = co.scale(x), pfo.delta_B(x)
    angle = host(hint_amd.plus_dominant_angle(xd)).astype(np.float64)
    starts = host(hint_amd.plus_fit_starts(xd)).astype(np.float64)
    assert starts.shape == (N, 9, 9)
    decided = 0
    for n in range(N):
        a64, ok = pfo.angle64(b[n])
        want = pfo.starts64(b[n], angle[n])
        e_centre = dB[n] + (pfo.FIT_P + 2) * pfo.U * S[n]                 # a point's error, and an fp32 sum of P of them
        assert np.abs(starts[n, :, 6:8] - want[:, 6:8]).max() <= e_centre, n
        assert np.array_equal(starts[n, :, :6], want[:, :6]) and (starts[n, :, 8] == np.float32(angle[n])).all()
        if ok:                                                            # the same inliers: the slope's rounding alone
            decided += 1
            assert abs(pfo.angle_diff(angle[n], a64)) <= 1e-4, (n, angle[n], a64)
    print(f"dominant angle: {decided} of {N} rows decided")
    assert decided >= 0.5 * N
    # given points: the same angle and starts as the traced route's
    pts = hint_amd.trace_fourier_curves(xd, pfo.FIT_P)
    assert bits_equal(hint_amd.plus_dominant_angle(pts), hint_amd.plus_dominant_angle(xd))
    assert bits_equal(hint_amd.plus_fit_starts(pts), hint_amd.plus_fit_starts(xd))
    # a row's angle does not depend on the batch or the chunk (16 rows a chunk at P = 100)
    x2, _ = pfo.plus_rows(1002, 18)
    full = hint_amd.plus_dominant_angle(dev(x2))
    for r in (0, 15, 16, 17):
        assert bits_equal(hint_amd.plus_dominant_angle(dev(x2[r:r + 1])), full[r:r + 1])
    with pytest.raises(hint_amd.HintAmdError, match="plus_dominant_angle: .*at most 128 points"):
        hint_amd.plus_dominant_angle(hint_amd.trace_fourier_curves(xd, 129))
    given = hint_amd.plus_fit_starts(hint_amd.trace_fourier_curves(xd, 129), dev(angle.astype(np.float32)))
    assert given.shape == (N, 9, 9) and torch.isfinite(given).all()


# ---- 7. invariance and safety ----
def _inv_case(N=9, S=2):
    x, base = pfo.plus_rows(1101, N)
    return dev(x), dev(np.stack([pfo.eval_params(base, 1102 + s) for s in range(S)], 1))


def _shapes(N, S, steps):
    return dict(params=(N, 9), loss=(N,), best=(N,), n_run=(N,), all_params=(N, S, 9), all_loss=(N, S), grad=(N, S, 9),
                trace=(N, S, steps, 19))


def test_a_rows_bits_do_not_depend_on_the_batch_the_position_the_grid_or_the_outputs():
    xd, sd = _inv_case()
    N, S, steps = 9, 2, 5
    full = run(xd, sd, steps)
    for r in (0, 4, 8):                                                   # N = 1 against the same row among 9
        assert same_bits(run(xd[r:r + 1], sd[r:r + 1], steps), {k: v[r:r + 1] for k, v in full.items()})
    assert same_bits(run(xd[:3], sd[:3], steps), {k: v[:3] for k, v in full.items()})
    for mg in (1, 2):                                                     # a workgroup serves several rows, one after the other
        assert same_bits(run(xd, sd, steps, max_groups=mg), full)
    assert same_bits(run(xd, sd, steps), full)                            # two runs
    for fill in (float("nan"), 1e30):
        pre = {}
        for k, s in _shapes(N, S, steps).items():
            t = torch.full(s, fill, dtype=torch.float32, device=DEV)
            pre[k] = t.view(torch.int32) if k in INTS else t
        assert same_bits(run(xd, sd, steps, out=pre), full)
    for S1 in (1, 3):                                                     # a start's result does not depend on the other starts
        s3 = torch.cat([sd, sd[:, :1]], 1)[:, :S1].contiguous()
        part = run(xd, s3, steps)
        assert bits_equal(part["all_params"][:, 0], full["all_params"][:, 0]) and bits_equal(part["trace"][:, 0], full["trace"][:, 0])
        if S1 == 3:                                                       # the third start repeats the first: a tie goes to the first
            assert bits_equal(part["all_loss"][:, 2], part["all_loss"][:, 0]) and (part["best"] != 2).all()
    nine = torch.cat([sd] * 5, 1)[:, :9].contiguous()                     # S = 9
    many = run(xd, nine, steps)
    assert bits_equal(many["trace"][:, :2], full["trace"]) and bits_equal(many["trace"][:, 8], full["trace"][:, 0])


@pytest.mark.parametrize("source", ("traced", "given"))
def test_each_output_alone_and_all_together_on_guarded_buffers(source):
    N, S, steps, P = 5, 3, 2, 257
    x, base = pfo.plus_rows(1201, N)
    curve = x if source == "traced" else co.points64(x, P).astype(np.float32)
    starts = np.stack([pfo.eval_params(base, 1202 + s) for s in range(S)], 1)
    gc, gs = (Guarded(v.size).set(torch.from_numpy(v)) for v in (curve, starts))
    snaps = [g.snapshot() for g in (gc, gs)]
    cd, sd = gc.view(*curve.shape), gs.view(N, S, 9)
    shapes = _shapes(N, S, steps)
    # the stop makes rows leave starts unrun: every word of every output is written all the same
    stop = float(np.median(host(run(cd, sd, steps, P=P)["all_loss"])[:, 0]))

    def guarded_run(names, fill, seed):
        bufs = {k: Guarded(int(np.prod(shapes[k])), fill=fill, seed=seed + i, align=16 if seed % 2 else 256,
                           dtype=torch.int32 if k in INTS else torch.float32) for i, k in enumerate(names)}
        out = run(cd, sd, steps, tuple(names), seed % 3, {k: bufs[k].view(*shapes[k]) for k in names}, P=P, stop_loss=stop)
        torch.cuda.synchronize()
        for k, gb in bufs.items():
            gb.check_guards(f"{names} {fill}: {k}")
        for g, s, what in zip((gc, gs), snaps, ("curve", "starts")):
            g.check_unchanged(s, what)
        return {k: v.clone() for k, v in out.items()}

    first = guarded_run(ALL, "zero", 0)
    assert 1 <= int(first["n_run"].min()) < int(first["n_run"].max())
    for rep, fill in enumerate(FILLS):
        assert same_bits(guarded_run(ALL, fill, 10 * rep + 1), first)
    for i, name in enumerate(ALL):
        assert same_bits(guarded_run((name,), "nan", 50 + i), first, (name,))
    assert same_bits(run(cd, sd, steps, P=P, stop_loss=stop), first)


def test_non_finite_rows_fault_nothing_and_leave_the_others_alone():
    xd, sd = _inv_case()
    steps = 5
    good = run(xd, sd, steps)
    keep = [0, 2, 4, 6, 8]
    for i, bad in enumerate((float("nan"), float("inf"), float("-inf"), 1e30)):
        xb, sb = xd.clone(), sd.clone()
        xb[1, i], xb[3] = bad, bad                                        # one coefficient; a whole row
        sb[5, 0, i], sb[7, 1] = bad, bad                                  # one parameter of one start; a whole start
        res = run(xb, sb, steps)
        torch.cuda.synchronize()
        assert same_bits({k: v[keep] for k, v in res.items()}, {k: v[keep] for k, v in good.items()})
        assert bits_equal(res["trace"][5, 1], good["trace"][5, 1])        # the other start of a row with a bad start
        if bad != bad:                                                    # a bad start loses to a good one
            assert int(res["best"][7]) == 0
        pts = hint_amd.trace_fourier_curves(xd, pfo.FIT_P)
        pts[2, 7, 1] = bad
        given = run(pts, sd, steps)
        torch.cuda.synchronize()
        assert same_bits({k: v[[0, 1, 3, 8]] for k, v in given.items()}, {k: v[[0, 1, 3, 8]] for k, v in good.items()})
        # the angle and the starts of given points with a bad row: plain torch, the good rows' bits unchanged
        a_good, a_bad = hint_amd.plus_dominant_angle(hint_amd.trace_fourier_curves(xd, pfo.FIT_P)), hint_amd.plus_dominant_angle(pts)
        torch.cuda.synchronize()
        assert bits_equal(a_bad[[0, 1, 3, 8]], a_good[[0, 1, 3, 8]])
    assert same_bits(run(xd, sd, steps), good)
    sb = sd.clone()                                                       # every start NaN: start 0 is the row's
    sb[4] = float("nan")
    res = run(xd, sb, 0)
    assert int(res["best"][4]) == 0 and torch.isnan(res["loss"][4])


def test_capture_in_a_graph_and_two_replays():
    xd, sd = _inv_case()
    kw = dict(starts=sd, n_steps=5, return_all=True, return_trace=True)
    eager = hint_amd.fit_plus_shapes(xd, **kw)
    eager_g = hint_amd.plus_fit_grad(xd, sd[:, 0])                        # (also loads the kernel before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        params, loss, extra = hint_amd.fit_plus_shapes(xd, **kw)
        gl, gg = hint_amd.plus_fit_grad(xd, sd[:, 0])
    for _ in range(2):
        for t in (params, loss, extra["all_params"], extra["all_loss"], extra["trace"], gl, gg):
            t.fill_(float("nan"))
        extra["best"].fill_(-7)
        extra["n_run"].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(params, eager[0]) and bits_equal(loss, eager[1]) and same_bits(extra, eager[2])
        assert bits_equal(gl, eager_g[0]) and bits_equal(gg, eager_g[1])


def test_a_curve_of_two_equal_points_stays_finite_over_a_whole_fit():
    x, _ = pfo.plus_rows(1301, 3)
    xd = dev(x)
    pts = hint_amd.trace_fourier_curves(xd, 2)
    assert bits_equal(pts[:, 0], pts[:, 1])
    starts = hint_amd.plus_fit_starts(pts, torch.zeros(3, device=DEV))[:, :2].contiguous()
    fit = run(xd, starts, 400, P=2)
    assert torch.isfinite(fit["params"]).all() and torch.isfinite(fit["loss"]).all() and torch.isfinite(fit["trace"]).all()
    assert (hint_amd.plus_dominant_angle(pts) == 0).all()                 # no pair of distinct x: no candidate


def test_argument_errors_name_the_function():
    xd, sd = _inv_case(3, 2)
    with pytest.raises(hint_amd.HintAmdError, match="fit_plus_shapes: starts must have shape"):
        hint_amd.fit_plus_shapes(xd, starts=sd[:, :, :4])
    with pytest.raises(hint_amd.HintAmdError, match="fit_plus_shapes: n_steps must be 0..1024"):
        hint_amd.fit_plus_shapes(xd, starts=sd, n_steps=1025)
    with pytest.raises(hint_amd.HintAmdError, match="fit_plus_shapes: both starts and angle"):
        hint_amd.fit_plus_shapes(xd, starts=sd, angle=torch.zeros(3, device=DEV))
    with pytest.raises(hint_amd.HintAmdError, match="plus_fit_starts: angle must have shape"):
        hint_amd.plus_fit_starts(xd, torch.zeros(4, device=DEV))
    with pytest.raises(hint_amd.HintAmdError, match="fit_plus_shapes: starts requires grad"):
        hint_amd.fit_plus_shapes(xd, starts=sd.clone().requires_grad_(True))
    p, l, extra = hint_amd.fit_plus_shapes(xd, starts=sd, n_steps=0, return_trace=True)
    assert extra["trace"].shape == (3, 2, 0, 19)
