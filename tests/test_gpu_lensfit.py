"""Device tests of the lens-shape fit (hint_amd.curves lens_fit_grad / lens_fit_starts / fit_lens_shapes, hint_lensfit_run) against
the float64 restatement and the rules of tests/lensfit_oracle.py:
  1. loss and gradient of single evaluations (n_steps = 0) and of every traced step of a 100-step fit, on decided evaluations;
  2. the update rule on every traced step, decided or not, and the selection, bit for bit;
  3. short fits (1, 2, 5 steps) against fit64 from the same starts;
  4. whole fits against fit64 and against what the reference returned; lens_fit_starts against starts64;
  5. invariance, guard-banded outputs, non-finite inputs, graph capture, the smallest sizes.
Sizes: (P, M) in (2, 1), (100, 130), (257, 1023), (1024, 1024).  At the two large ones a curve's neighbouring points are nearer to
each other than the rule for a decided minimum allows for, so the oracle is met there on scattered given points (points spread
over the plane are decided) and the traced source is tied to the given one bit for bit at every size."""
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import curves
import curve_oracle as co
import lensfit_oracle as lo
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("params", "loss", "best", "all_params", "all_loss", "grad", "trace")
SIZES = ((2, 1), (100, 130), (257, 1023), (1024, 1024))
FIT = dict(lr=lo.LR, angle_lr=lo.ANGLE_LR, gamma=lo.GAMMA, momentum=lo.MOMENTUM)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def run(curve, proto, starts, n_steps=0, want=ALL, max_groups=0, out=None, w=1.0, P=lo.FIT_P, **kw):
    """one hint_lensfit_run on device tensors; curve [N, 4K] is traced at P"""
    k = curve.shape[1] // 4 if curve.dim() == 2 else 0
    p = P if k else curve.shape[1]
    want = tuple(n for n in want if n != "trace" or n_steps > 0)
    args = dict(FIT)
    args.update(kw)
    return curves._lf_run(curve, k, p, proto, starts, n_steps, weight=w, want=want, max_groups=max_groups, out=out, **args)


def same_bits(a, b, names=None):
    for k in names or a.keys():
        if not (bits_equal(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k])):
            return False
    return True


def scatter(seed, n, count, spread=3.0):
    """points spread over a square: fp32 [n, count, 2]"""
    return np.random.RandomState(seed).uniform(-spread / 2, spread / 2, (n, count, 2)).astype(np.float32)


def eval_case(source, P, M, N, S, seed):
    """(curve fp32, the float64 points [N, P, 2], delta_B [N], prototype fp32 [M, 2], starts fp32 [N, S, 4])"""
    if source == "scatter":
        curve = scatter(seed, N, P)
        b, dB, proto = curve.astype(np.float64), np.zeros(N), scatter(seed + 1, 1, M, 2.0)[0]
    else:
        x = lo.lens_rows(seed, N)
        b, dB = co.points64(x, P), lo.delta_B(x)
        proto = lo.lens_prototype(M) if M > 1 else np.array([[0.75, -0.5]], np.float32)      # (one centred point is the origin)
        if source == "given":
            curve = b.astype(np.float32)
            b, dB = curve.astype(np.float64), np.zeros(N)
        else:
            curve = x
    if source == "scatter" or P != lo.FIT_P:
        starts = lo.golden_grad_params(seed, N * S).reshape(N, S, 4)
    else:
        starts = lo.near_params(proto, b, seed, S)
    return curve, b, dB, proto, starts


_ratios = {}


def compare(name, proto, b, dB, w, params, losses, grads):
    """device evaluations of a case's rows (lists, one entry a row) against evaluate64 at the device's own parameters: first the
    cap - at most 25 % of the case's evaluations may be undecided - then the decided ones against the bounds"""
    und, total, rl, rg = 0, 0, 0.0, np.zeros(4)
    for n in range(len(b)):
        u, l, g = lo.compare_evaluations(proto, b[n], dB[n], w, params[n], losses[n], grads[n])
        und, total, rl, rg = und + u, total + len(params[n]), max(rl, l), np.maximum(rg, g)
    _ratios[name] = (rl, rg)
    print(f"{name}: {und} of {total} evaluations undecided; worst error / bound: loss {rl:.3g}, gradient "
          f"{np.array2string(rg, precision=3)}")
    assert und <= 0.25 * total, (name, und, total)
    assert rl <= 1.0 and (rg <= 1.0).all(), (name, rl, rg)


# ---- 1. single evaluations ----
@pytest.mark.parametrize("source,P,M,N,S,w", (("traced", 100, 130, 9, 3, 1.0), ("given", 100, 130, 3, 2, 0.25),
                                              ("traced", 2, 1, 3, 1, 1.0), ("given", 2, 1, 1, 2, 0.25),
                                              ("scatter", 257, 1023, 3, 2, 1.0), ("scatter", 1024, 1024, 3, 3, 0.25)))
def test_loss_and_gradient_of_an_evaluation(source, P, M, N, S, w):
    curve, b, dB, proto, starts = eval_case(source, P, M, N, S, 500 + P + M)
    for mg in (0, 1, 2):
        res = run(dev(curve), dev(proto), dev(starts), 0, w=w, P=P, max_groups=mg)
        if mg == 0:
            first = res
        assert same_bits(res, first)
    assert bits_equal(first["all_params"], dev(starts))                   # n_steps = 0: the starts themselves
    L, G = host(first["all_loss"]), host(first["grad"])
    compare(f"evaluation {source} P {P} M {M}", proto, b, dB, w, starts, L, G)
    # the row's result is the first minimum of the starts' losses
    best = host(first["best"])
    for n in range(N):
        assert best[n] == lo._select(L[n])
    rows = torch.arange(N, device=DEV)
    assert bits_equal(first["loss"], first["all_loss"][rows, first["best"].long()])
    assert bits_equal(first["params"], first["all_params"][rows, first["best"].long()])


def test_lens_fit_grad_is_the_evaluation_and_lens_fit_loss_its_loss():
    curve, b, dB, proto, starts = eval_case("traced", 100, 130, 5, 1, 77)
    cd, pd, sd = dev(curve), dev(proto), dev(starts[:, 0])
    for w in (1.0, 0.25):
        loss, grad = hint_amd.lens_fit_grad(cd, pd, sd, w)
        res = run(cd, pd, dev(starts), 0, w=w)
        assert loss.shape == (5,) and grad.shape == (5, 4)
        assert bits_equal(loss, res["all_loss"][:, 0]) and bits_equal(grad, res["grad"][:, 0])
        # lens_fit_loss rounds the two means to fp32 before it weights them: equal up to those roundings
        old = hint_amd.lens_fit_loss(cd, pd, sd, w)
        assert (host(old).astype(np.float64) - host(loss)).__abs__().max() <= 4 * lo.U * np.abs(host(loss)).max()
    one = hint_amd.lens_fit_grad(cd, pd, sd[2], 1.0)                       # [4] params serve every row
    assert bits_equal(one[0][2:3], hint_amd.lens_fit_grad(cd, pd, sd, 1.0)[0][2:3])
    with pytest.raises(hint_amd.HintAmdError, match="lens_fit_loss: params requires grad"):
        hint_amd.lens_fit_loss(cd, pd, sd.clone().requires_grad_(True))


# ---- the traced source is the given one, bit for bit, at every size ----
@pytest.mark.parametrize("P,M", SIZES)
def test_the_traced_source_gives_the_bits_of_the_given_one(P, M):
    N, S, steps = 3, 2, 5
    x = lo.lens_rows(600 + P, N)
    proto = dev(lo.lens_prototype(M))
    xd = dev(x)
    pts = hint_amd.trace_fourier_curves(xd, P)
    starts = dev(lo.golden_grad_params(601 + P, N * S).reshape(N, S, 4))
    a, b = run(xd, proto, starts, steps, P=P), run(pts, proto, starts, steps)
    assert same_bits(a, b)
    assert torch.isfinite(a["trace"]).all() and torch.isfinite(a["params"]).all()
    for s in range(S):                                                    # the update rule holds on the many-points path too
        for n in range(N):
            assert lo.check_update_rule(host(a["trace"][n, s]), host(a["all_params"][n, s])) <= 1.0


# ---- 1b and 2. every step of a 100-step fit ----
@pytest.fixture(scope="module")
def long_fit():
    N = 3
    x = lo.lens_rows(701, N)
    proto = lo.lens_prototype(130)
    xd, pd = dev(x), dev(proto)
    starts = hint_amd.lens_fit_starts(xd)
    params, loss, extra = hint_amd.fit_lens_shapes(xd, pd, return_all=True, return_trace=True)
    res = dict(params=params, loss=loss, **extra)
    return x, proto, starts, res


def test_every_traced_step_of_a_fit_against_float64(long_fit):
    x, proto, starts, res = long_fit
    b, dB = co.points64(x, lo.FIT_P), lo.delta_B(x)
    tr = host(res["trace"])
    assert tr.shape == (3, 2, 100, 9)
    t = tr.reshape(3, -1, 9)
    compare("traced steps", proto, b, dB, 1.0, t[:, :, :4], t[:, :, 4], t[:, :, 5:])


def test_update_rule_on_every_step_and_the_selection_bit_for_bit(long_fit):
    x, proto, starts, res = long_fit
    tr, ap = host(res["trace"]), host(res["all_params"])
    assert bits_equal(res["trace"][:, :, 0, :4], starts)                  # a fit begins at its start
    worst = 0.0
    for n in range(3):
        for s in range(2):                                                # (a second start's first step uses buf = g_0)
            worst = max(worst, lo.check_update_rule(tr[n, s], ap[n, s]))
    print(f"update rule: worst error {worst:.3g} ulp")
    assert worst <= 1.0
    assert bits_equal(res["all_loss"], res["trace"][:, :, -1, 4])         # the loss of the last step before its update
    al = host(res["all_loss"])
    rows = torch.arange(3, device=DEV)
    for n in range(3):
        assert host(res["best"])[n] == lo._select(al[n])
    assert bits_equal(res["loss"], res["all_loss"][rows, res["best"].long()])
    assert bits_equal(res["params"], res["all_params"][rows, res["best"].long()])
    # without the extras: the same two tensors
    params, loss = hint_amd.fit_lens_shapes(dev(x), dev(proto))
    assert bits_equal(params, res["params"]) and bits_equal(loss, res["loss"])
    # grad of a fit is the last step's gradient
    full = run(dev(x), dev(proto), starts, 100)
    assert same_bits(full, res, ("params", "loss", "best", "all_params", "all_loss", "trace"))
    assert bits_equal(full["grad"], res["trace"][:, :, -1, 5:])


# ---- 3. short fits ----
@pytest.mark.parametrize("steps", lo.SHORT["steps"])
def test_short_fits_against_fit64(steps):
    proto = lo.lens_prototype(130)
    x, b, dB, st = lo.short_rows()
    b32 = co.trace32(x, lo.FIT_P)
    refs = [lo.fit64(proto, b[n], st[n], steps) for n in range(len(x))]
    tol = 16 * max(lo.fit_dev(lo.emulate32(proto, b32[n], st[n], steps), refs[n]) for n in range(len(x)))
    res = run(dev(x), dev(proto), dev(st), steps)
    devs = [lo.fit_dev(dict(all_params=host(res["all_params"])[n], all_loss=host(res["all_loss"])[n]), refs[n])
            for n in range(len(x))]
    print(f"{steps} steps: tolerance {tol:.3g} (16 x the emulation's largest deviation), device deviations " +
          ", ".join(f"{d:.3g}" for d in devs))
    assert tol < 1e-5 and max(devs) <= tol
    assert [int(v) for v in host(res["best"])] == [r["best"] for r in refs]


# ---- 4. whole fits ----
def _whole(x, proto):
    """device fit from lens_fit_starts, fit64 and the emulation from the same starts: (device result, references, tolerances)"""
    xd, pd = dev(x), dev(proto)
    starts = hint_amd.lens_fit_starts(xd)
    params, loss, extra = hint_amd.fit_lens_shapes(xd, pd, return_all=True)
    st = host(starts)
    b, b32 = co.points64(x, lo.FIT_P), co.trace32(x, lo.FIT_P)
    refs = [lo.fit64(proto, b[n], st[n]) for n in range(len(x))]
    emus = [lo.emulate32(proto, b32[n], st[n]) for n in range(len(x))]
    tol_l = 16 * max(np.abs(e["all_loss"] - r["all_loss"]).max() for e, r in zip(emus, refs))
    tol_p = 16 * max(lo.param_diff(e["all_params"], r["all_params"]) for e, r in zip(emus, refs))
    return dict(params=host(params), loss=host(loss), best=host(extra["best"]), all_params=host(extra["all_params"]),
                all_loss=host(extra["all_loss"])), refs, tol_l, tol_p


@pytest.mark.parametrize("which", ("fixture", "more"))
def test_whole_fits_against_fit64_and_the_reference(which):
    if which == "fixture":
        g = np.load(os.path.join(ROOT, "tests", "golden", f"lensfit_{lo.GOLDEN_FIT['name']}.npz"))
        x, proto = g["x"], g["prototype"]
    else:
        x, proto = lo.lens_rows(801, 8), lo.lens_prototype(130)
    got, refs, tol_l, tol_p = _whole(x, proto)
    d_loss = max(np.abs(got["all_loss"][n] - refs[n]["all_loss"]).max() for n in range(len(x)))
    d_par = max(lo.param_diff(got["all_params"][n], refs[n]["all_params"]) for n in range(len(x)))
    print(f"{which}: loss tolerance {tol_l:.3g}, device {d_loss:.3g}; parameter tolerance {tol_p:.3g} (the emulation's own "
          f"deviation lies along flat directions), device {d_par:.3g}")
    assert d_loss <= tol_l and d_par <= tol_p
    for n in range(len(x)):
        if abs(refs[n]["all_loss"][0] - refs[n]["all_loss"][1]) > 2 * tol_l:
            assert got["best"][n] == refs[n]["best"]
        assert abs(got["loss"][n] - refs[n]["loss"]) <= tol_l
    assert all(abs(r["all_loss"][0] - r["all_loss"][1]) > 4e-3 for r in refs)     # so every row's selection was compared
    if which == "fixture":                                                        # what the reference itself returned
        d_ref = max(lo.param_diff(got["params"][n], g["ref_params"][n]) for n in range(len(x)))
        print(f"fixture: device parameters against the reference's: {d_ref:.3g} (tolerance {tol_p + 2e-6:.3g})")
        assert d_ref <= tol_p + 2e-6                                              # (2e-6: fit64 against the reference, CPU test)


def test_lens_fit_starts_against_starts64():
    x = co.gauss(901, 24, 5)
    keep = co.unambiguous(x, lo.FIT_P)
    assert keep.sum() >= 12
    x = x[keep]
    got = host(hint_amd.lens_fit_starts(dev(x))).astype(np.float64)
    b = co.points64(x, lo.FIT_P)
    S, fb, dB = co.scale(x), co.feature_bound(x), lo.delta_B(x)
    fars = np.empty(len(x))                                               # the farthest pair's distance, per row
    for n in range(len(x)):
        want = lo.starts64(b[n])
        i, j = np.unravel_index(((b[n][:, None] - b[n][None]) ** 2).sum(-1).argmax(), (lo.FIT_P, lo.FIT_P))
        far = fars[n] = np.linalg.norm(b[n][j] - b[n][i])
        e_centre = dB[n] + (lo.FIT_P + 2) * lo.U * S[n]                   # a point's error, and an fp32 sum of P of them
        e_angle = 2 * fb[n] / far + 16 * lo.U * np.pi                     # atan2 is 1 / |v|-Lipschitz per component; roundings
        assert np.abs(got[n, :, :2] - want[:, :2]).max() <= e_centre, n
        assert (got[n, :, 2] == 2.0).all()
        assert np.abs(lo.angle_diff(got[n, :, 3], want[:, 3])).max() <= e_angle, n
        assert 0.0 <= got[n, 1, 3] < 2 * np.pi + 1e-6
    # given points: plain torch on the [N, P, P] matrix - the same pair, so the same starts up to the feature's rounding
    pts = hint_amd.trace_fourier_curves(dev(x), lo.FIT_P)
    given = host(hint_amd.lens_fit_starts(pts)).astype(np.float64)
    assert np.abs(given[:, :, :3] - got[:, :, :3]).max() <= 4 * lo.U * S.max() * lo.FIT_P
    # (either side's angle is within 2 fb / far + 16 u pi of the float64 one, by the reasoning above)
    assert (np.abs(lo.angle_diff(given[:, :, 3], got[:, :, 3])).max(1) <= 2 * (2 * fb / fars + 16 * lo.U * np.pi)).all()


# ---- 5. invariance and safety ----
def _inv_case(N=9, S=2):
    x = lo.lens_rows(1001, N)
    return dev(x), dev(lo.lens_prototype(130)), dev(lo.golden_grad_params(1002, N * S).reshape(N, S, 4))


def test_a_rows_bits_do_not_depend_on_the_batch_the_position_the_grid_or_the_outputs():
    xd, pd, sd = _inv_case()
    N, S, steps = 9, 2, 5
    full = run(xd, pd, sd, steps)
    for r in (0, 4, 8):                                                   # N = 1 against the same row among 9
        assert same_bits(run(xd[r:r + 1], pd, sd[r:r + 1], steps), {k: v[r:r + 1] for k, v in full.items()})
    assert same_bits(run(xd[:3], pd, sd[:3], steps), {k: v[:3] for k, v in full.items()})
    for mg in (1, 2):                                                     # a workgroup serves several rows, one after the other
        assert same_bits(run(xd, pd, sd, steps, max_groups=mg), full)
    assert same_bits(run(xd, pd, sd, steps), full)                        # two runs
    shapes = dict(params=(N, 4), loss=(N,), best=(N,), all_params=(N, S, 4), all_loss=(N, S), grad=(N, S, 4),
                  trace=(N, S, steps, 9))
    for fill in (float("nan"), 1e30):
        pre = {}
        for k, s in shapes.items():
            t = torch.full(s, fill, dtype=torch.float32, device=DEV)
            pre[k] = t.view(torch.int32) if k == "best" else t
        assert same_bits(run(xd, pd, sd, steps, out=pre), full)
    for S1 in (1, 3):                                                     # a start's result does not depend on the other starts
        s3 = torch.cat([sd, sd[:, :1]], 1)[:, :S1].contiguous()
        part = run(xd, pd, s3, steps)
        assert bits_equal(part["all_params"][:, 0], full["all_params"][:, 0]) and bits_equal(part["trace"][:, 0], full["trace"][:, 0])
        if S1 == 3:                                                       # the third start repeats the first: a tie goes to the first
            assert bits_equal(part["all_loss"][:, 2], part["all_loss"][:, 0]) and (part["best"] != 2).all()


@pytest.mark.parametrize("source", ("traced", "given"))
def test_each_output_alone_and_all_together_on_guarded_buffers(source):
    N, S, steps, P, M = 5, 3, 2, 257, 1023
    x = lo.lens_rows(1101, N)
    curve = x if source == "traced" else co.points64(x, P).astype(np.float32)
    proto, starts = lo.lens_prototype(M), lo.golden_grad_params(1102, N * S).reshape(N, S, 4)
    gc, gp, gs = (Guarded(v.size).set(torch.from_numpy(v)) for v in (curve, proto, starts))
    snaps = [g.snapshot() for g in (gc, gp, gs)]
    cd, pd, sd = gc.view(*curve.shape), gp.view(M, 2), gs.view(N, S, 4)
    shapes = dict(params=(N, 4), loss=(N,), best=(N,), all_params=(N, S, 4), all_loss=(N, S), grad=(N, S, 4),
                  trace=(N, S, steps, 9))

    def guarded_run(names, fill, seed):
        bufs = {k: Guarded(int(np.prod(shapes[k])), fill=fill, seed=seed + i, align=16 if seed % 2 else 256,
                           dtype=torch.int32 if k == "best" else torch.float32) for i, k in enumerate(names)}
        out = run(cd, pd, sd, steps, tuple(names), seed % 3, {k: bufs[k].view(*shapes[k]) for k in names}, P=P)
        torch.cuda.synchronize()
        for k, gb in bufs.items():
            gb.check_guards(f"{names} {fill}: {k}")
        for g, s, what in zip((gc, gp, gs), snaps, ("curve", "prototype", "starts")):
            g.check_unchanged(s, what)
        return {k: v.clone() for k, v in out.items()}

    first = guarded_run(ALL, "zero", 0)
    for rep, fill in enumerate(FILLS):
        assert same_bits(guarded_run(ALL, fill, 10 * rep + 1), first)
    for i, name in enumerate(ALL):
        assert same_bits(guarded_run((name,), "nan", 50 + i), first, (name,))
    assert same_bits(run(cd, pd, sd, steps, P=P), first)


def test_non_finite_rows_fault_nothing_and_leave_the_others_alone():
    xd, pd, sd = _inv_case()
    steps = 5
    good = run(xd, pd, sd, steps)
    keep = [0, 2, 4, 6, 8]
    for i, bad in enumerate((float("nan"), float("inf"), float("-inf"), 1e30)):
        xb, sb = xd.clone(), sd.clone()
        xb[1, i], xb[3] = bad, bad                                        # one coefficient; a whole row
        sb[5, 0, i], sb[7, 1] = bad, bad                                  # one parameter of one start; a whole start
        res = run(xb, pd, sb, steps)
        torch.cuda.synchronize()
        assert same_bits({k: v[keep] for k, v in res.items()}, {k: v[keep] for k, v in good.items()})
        assert bits_equal(res["trace"][5, 1], good["trace"][5, 1])        # the other start of a row with a bad start
        # a bad start loses to a good one
        if bad != bad:
            assert int(res["best"][7]) == 0
        # the prototype is shared, so a bad point in it reaches every row: nothing faults, and the next run is as before
        pb = pd.clone()
        pb[i, i % 2] = bad
        run(xd, pb, sd, steps)
        torch.cuda.synchronize()
        pts = hint_amd.trace_fourier_curves(xd, lo.FIT_P)
        pts[2, 7, 1] = bad
        given = run(pts, pd, sd, steps)
        torch.cuda.synchronize()
        assert same_bits({k: v[[0, 1, 3, 8]] for k, v in given.items()}, {k: v[[0, 1, 3, 8]] for k, v in good.items()})
    assert same_bits(run(xd, pd, sd, steps), good)
    # every start NaN: start 0 is the row's
    sb = sd.clone()
    sb[4] = float("nan")
    res = run(xd, pd, sb, 0)
    assert int(res["best"][4]) == 0 and torch.isnan(res["loss"][4])


def test_non_finite_given_points_through_the_default_starts():
    """lens_fit_starts on given points is plain torch on the [P, P] distances: a row that holds NaN or inf takes no index from
    them, nothing faults, and the good rows' starts and fits are the bits of a run without the bad rows"""
    xd, pd, _ = _inv_case()
    pts = hint_amd.trace_fourier_curves(xd, lo.FIT_P)
    good_s = hint_amd.lens_fit_starts(pts)
    good = hint_amd.fit_lens_shapes(pts, pd, n_steps=5, return_all=True)
    keep = [0, 2, 4, 6, 7]
    for bad in (float("nan"), float("inf"), float("-inf")):
        pb = pts.clone()
        pb[1, 7, 1], pb[3], pb[5, :, 0] = bad, bad, bad                   # one value; a whole row; one coordinate of every point
        pb[8, lo.FIT_P - 1] = bad                                         # the last point of the last row
        starts = hint_amd.lens_fit_starts(pb)
        res = hint_amd.fit_lens_shapes(pb, pd, n_steps=5, return_all=True)
        torch.cuda.synchronize()
        assert bits_equal(starts[keep], good_s[keep])
        assert bits_equal(res[0][keep], good[0][keep]) and bits_equal(res[1][keep], good[1][keep])
        assert same_bits({k: v[keep] for k, v in res[2].items()}, {k: v[keep] for k, v in good[2].items()})
        xb = xd.clone()                                                   # coefficients: the kernels' own path
        xb[1, 3], xb[3] = bad, bad
        res = hint_amd.fit_lens_shapes(xb, pd, n_steps=5, return_all=True)
        ref = hint_amd.fit_lens_shapes(xd, pd, n_steps=5, return_all=True)
        torch.cuda.synchronize()
        assert bits_equal(res[0][keep], ref[0][keep]) and bits_equal(res[1][keep], ref[1][keep])
    assert bits_equal(hint_amd.lens_fit_starts(pts), good_s)


def test_given_points_starts_are_chunked_over_rows_and_a_rows_bits_do_not_depend_on_the_chunk():
    P, N = 1024, 18                                                       # 2^24 / P^2 = 16 rows a chunk: two chunks
    pts = hint_amd.trace_fourier_curves(dev(lo.lens_rows(1301, N)), P)
    full = hint_amd.lens_fit_starts(pts)
    for r in (0, 15, 16, 17):
        assert bits_equal(hint_amd.lens_fit_starts(pts[r:r + 1]), full[r:r + 1])
    assert torch.isfinite(full).all()


def test_capture_in_a_graph_and_two_replays():
    xd, pd, sd = _inv_case()
    eager = hint_amd.fit_lens_shapes(xd, pd, starts=sd, n_steps=5, return_all=True, return_trace=True)
    eager_g = hint_amd.lens_fit_grad(xd, pd, sd[:, 0])                    # (also loads the kernel before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        params, loss, extra = hint_amd.fit_lens_shapes(xd, pd, starts=sd, n_steps=5, return_all=True, return_trace=True)
        gl, gg = hint_amd.lens_fit_grad(xd, pd, sd[:, 0])
    for _ in range(2):
        for t in (params, loss, extra["all_params"], extra["all_loss"], extra["trace"], gl, gg):
            t.fill_(float("nan"))
        extra["best"].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(params, eager[0]) and bits_equal(loss, eager[1]) and same_bits(extra, eager[2])
        assert bits_equal(gl, eager_g[0]) and bits_equal(gg, eager_g[1])


def test_one_prototype_point_and_a_curve_of_two_equal_points():
    """M = 1, P = 2 (traced: B_1 repeats B_0 bit for bit): both curve points select the one prototype point, the prototype point
    selects j = 0, and L = (1 + w) D exactly"""
    x = lo.lens_rows(1201, 3)
    xd = dev(x)
    pts = hint_amd.trace_fourier_curves(xd, 2)
    assert bits_equal(pts[:, 0], pts[:, 1])
    proto = np.array([[0.75, -0.5]], np.float32)
    starts = lo.golden_grad_params(1202, 3).reshape(3, 1, 4)
    for w in (1.0, 0.25, 0.0):
        res = run(xd, dev(proto), dev(starts), 0, w=w, P=2)
        for n in range(3):
            A = lo.ho.template32(proto, starts[n, 0])[0]
            e = co._f32(A - host(pts)[n, 0].astype(np.float64))
            D = co._fma(e[1], e[1], co._f32(e[0] * e[0]))
            assert host(res["all_loss"])[n, 0] == np.float32((1 + w) * D)
            assert host(res["grad"])[n, 0, 0] == np.float32(2 * (1 + w) * e[0])
    fit = run(xd, dev(proto), dev(starts), 100, P=2)
    assert torch.isfinite(fit["params"]).all() and torch.isfinite(fit["loss"]).all()
