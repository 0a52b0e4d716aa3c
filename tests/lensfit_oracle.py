"""Float64 restatement of the lens-shape fit (hint_amd.curves lens_fit_grad / lens_fit_starts / fit_lens_shapes, include/hint_amd.h
hint_lensfit_run), a float32 emulation of the contract's operation order with deliberately wrong variants, and the rules device
results are compared by.  Written fresh from the contract; nothing of the reference is used.

Per row: B = the curve's P points, a = the prototype [M, 2], p = (x, y, scale, angle).  q = a R with R = [[cos, sin], [-sin, cos]]
(row vectors), A = q scale + (x, y), e = A_i - B_j, D = |e|^2, mA_i = min_j D (lowest j), mB_j = min_i D (lowest i);
  L = mean_j mB_j + w mean_i mA_i
  g = sum over the M + P selected pairs of 2 c (e.x, e.y, e . q, scale (e.y q.x - e.x q.y)),  c = w / M or 1 / P
and the schedule of torch's SGD(momentum, dampening 0) under StepLR(step_size 1): buf = g_0, then momentum buf + g_i;
p_(i+1) = p_i - lr_i buf, lr_i = lr gamma^i (angle_lr for the angle).  A start's loss is L_(n_steps - 1); the row's result is the
start with the smallest loss, the first on a tie.

The rules.  u = 2^-24 and E is hausdorff_oracle's bound on a distance at these parameters (bound_E below).
  decided   a minimum is decided when the gap to the best candidate whose coordinates differ from the chosen one exceeds
            2 (2 sqrt(D_second) E + E^2): two squared distances, each off by at most 2 d E + E^2, cannot then change order.  An
            evaluation is compared only when all M + P minima are decided - then device and oracle select the same pairs.
  loss      |L - L64| <= (1 + |w|) e_ch,  e_ch = 2 d_max E + E^2 (hausdorff_oracle's chamfer bound; d_max the root of the largest
            selected minimum)
  gradient  with the pairs equal, each component of e is off by at most E, q by at most 3 u R (R = max_i (|a.x| + |a.y|): a
            product, an fma, cs and sn rounded), the products e . q by 2 R E + 4 u R d_max each term, and the weights sum to
            1 + |w|; with 2 c in front and one rounding of g:
              x, y    2 (1 + |w|) E + u |g|
              scale   2 (1 + |w|) R (E + 4 u d_max) + u |g|
              angle   |scale| times the scale's bound, + u |g|
"""
import numpy as np

import curve_oracle as co
import hausdorff_oracle as ho
from curve_oracle import _f32, _fma

U = 2.0 ** -24
LR, ANGLE_LR, MOMENTUM, GAMMA, N_STEPS = 0.1, 0.01, 0.2, 0.1 ** (1 / 100), 100

# fixtures tests/golden/lensfit_<name>.npz (tests/golden/make_lensfit_golden.py)
GOLDEN_GRAD = dict(name="grad_n16", seed=301, rows=16, points=130, weights=(1.0, 0.25))
# The fit fixtures.  The reference's run is float32; where one of its steps picks another nearest point than float64 does, its
# angle - the flattest direction, stepped with the small rate - ends a few 1e-6 away.  fit_n8 (seed 312) is the first of four
# seeds tried on which all eight rows follow float64 throughout and meet 2e-6; fit_edge_n8 (seed 311) keeps such a row (row 3:
# 9.9e-6 in the angle) and is compared at 16 x what a float32 run of the same procedure (emulate32) deviates from float64 on its
# rows - the whole fits' rule - with the other seven rows still at 2e-6
GOLDEN_FIT = dict(name="fit_n8", seed=312, rows=8, points=130)
GOLDEN_FIT_EDGE = dict(name="fit_edge_n8", seed=311, rows=8, points=130, divergent=(3,))
FIT_P = 100

WRONG = ("angle stepped with lr", "no momentum", "no decay", "Nesterov", "decay before the first step", "one direction only",
         "R transposed in the angle term", "loss after the last update")


# ---- inputs ----
def _two_arcs(r0, r1, d, n0, n1):
    """the rim of the intersection of the discs (0, 0), r0 and (d, 0), r1, counter-clockwise: n0 points on the first disc's arc,
    n1 on the second's, neither repeating the other's first point"""
    xs = (d * d + r0 * r0 - r1 * r1) / (2 * d)
    ys = np.sqrt(r0 * r0 - xs * xs)
    t0, t1 = np.arctan2(ys, xs), np.arctan2(ys, d - xs)
    f0 = np.linspace(-t0, t0, n0, endpoint=False)
    f1 = np.linspace(np.pi - t1, np.pi + t1, n1, endpoint=False)
    return np.concatenate([np.stack([r0 * np.cos(f0), r0 * np.sin(f0)], 1), np.stack([d + r1 * np.cos(f1), r1 * np.sin(f1)], 1)]), \
        (2 * t0 * r0, 2 * t1 * r1)


def lens_prototype(M=130):
    """an analytic asymmetric lens, fp32 [M, 2]: discs of radius 1.5 at (0, 0) and 3.0 at (3.6, 0), the points shared between
    the arcs by arc length, centred.  (hausdorff_oracle.lens_template is symmetric under a half turn: the two starts tie on it)"""
    _, (l0, l1) = _two_arcs(1.5, 3.0, 3.6, 2, 2)
    n0 = min(max(int(round(M * l0 / (l0 + l1))), 1 if M > 1 else 0), M - 1) if M > 1 else 1
    pts, _ = _two_arcs(1.5, 3.0, 3.6, n0, M - n0)
    return (pts - pts.mean(0)).astype(np.float32)


def fourier_coeffs(points, K):
    """flat [4 K] coefficients of a closed polygon's points [n, 2]: the discrete Fourier sums over m = -K/2 .. K/2, divided by n,
    in the layout of flatten_coeffs (real parts of both axes, then imaginary parts)"""
    n = len(points)
    ms = np.arange(-(K // 2), K // 2 + 1)
    a = (points[:, :, None] * np.exp(-2j * np.pi * ms[None, None, :] * np.arange(n)[:, None, None] / n)).sum(0) / n   # [2, K]
    return np.concatenate([a.real.reshape(-1), a.imag.reshape(-1)])


def lens_rows(seed, N, K=5):
    """analytic lens-like coefficient rows [N, 4 K] fp32: two discs of radii r0 in [1, 2) and 2 r0, centres 0.8 (r0 + r1) apart
    at a random angle, 64 points per arc, centred and moved by 0.5 randn"""
    rs = np.random.RandomState(seed)
    out = np.empty((N, 4 * K), np.float32)
    for n in range(N):
        r0 = rs.uniform(1.0, 2.0)
        ang = rs.uniform(-np.pi, np.pi)
        off = 0.5 * rs.randn(2)
        pts, _ = _two_arcs(r0, 2 * r0, 0.8 * 3 * r0, 64, 64)
        R = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
        pts = (pts - pts.mean(0)) @ R + off
        out[n] = fourier_coeffs(pts, K)
    return out


def golden_grad_params(seed, N):
    """(x, y, scale, angle) near a fit's working range: centres near 0, scales 0.7 .. 2.2, every angle"""
    rs = np.random.RandomState(seed + 1000)
    return np.stack([0.3 * rs.randn(N), 0.3 * rs.randn(N), rs.uniform(0.7, 2.2, N), rs.uniform(-np.pi, np.pi, N)], 1).astype(np.float32)


# ---- float64 ----
def bound_E(a32, b, p, dB=0.0):
    """hausdorff_oracle's E at parameters p: 2 (delta_A + delta_B) + 4 u (the largest distance between a template and a curve point)"""
    a32 = np.asarray(a32, np.float64)
    p = np.asarray(p, np.float64)
    dA = 4 * U * (abs(p[2]) * np.abs(a32).sum(1).max() + max(abs(p[0]), abs(p[1])))
    A = ho.template64(a32, p)
    far = np.sqrt(((A[:, None, :] - np.asarray(b, np.float64)[None, :, :]) ** 2).sum(-1).max())
    return 2 * (dA + dB) + 4 * U * far


def delta_B(x):
    """hausdorff_oracle's bound on a traced curve point, per row of x [N, 4 K]"""
    x = np.asarray(x)
    return (2 * (x.shape[1] // 4) + 2) * U * co.scale(x)


def _gaps(D, at, pts, axis):
    """per minimum along `axis` of D [M, P]: (gap, D_second) to the best candidate whose coordinates differ from the chosen
    point's (pts: the points the minimum chooses among); inf where there is none"""
    Dm = D if axis == 1 else D.T                         # [own, candidates]
    chosen = pts[at]                                     # [own, 2]
    same = (pts[None, :, :] == chosen[:, None, :]).all(-1)
    second = np.where(same, np.inf, Dm).min(1)
    return second - Dm[np.arange(len(at)), at], second


def evaluate64(a, b, p, w=1.0, one_direction=False, transposed=False):
    """(L, g [4], info) at parameters p: info holds mA, mB, the selected indices ja, ib, per minimum the gap to the best candidate
    whose coordinates differ from the chosen one and that candidate's D (gapA, secondA, gapB, secondB), and d_max"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    x, y, sc, ang = (float(v) for v in np.asarray(p, np.float64))
    cs, sn = np.cos(ang), np.sin(ang)
    q = np.stack([a[:, 0] * cs - a[:, 1] * sn, a[:, 0] * sn + a[:, 1] * cs], 1)
    A = q * sc + np.array([x, y])
    e = A[:, None, :] - b[None, :, :]
    D = (e ** 2).sum(-1)
    ja, ib = D.argmin(1), D.argmin(0)
    M, P = D.shape
    mA, mB = D[np.arange(M), ja], D[ib, np.arange(P)]
    wA = 0.0 if one_direction else w
    L = mB.mean() + wA * mA.mean()
    g = np.zeros(4)
    sign = -1.0 if transposed else 1.0                   # (dq / d angle taken from the transposed R: the angle term's sign flips)
    for ee, qq, c in ((e[np.arange(M), ja], q, wA / M), (e[ib, np.arange(P)], q[ib], 1.0 / P)):
        ang_term = sign * sc * (ee[:, 1] * qq[:, 0] - ee[:, 0] * qq[:, 1])
        g += 2 * c * np.array([ee[:, 0].sum(), ee[:, 1].sum(), (ee * qq).sum(), ang_term.sum()])
    gapA, secondA = _gaps(D, ja, b, 1)
    gapB, secondB = _gaps(D, ib, A, 0)
    return L, g, dict(mA=mA, mB=mB, ja=ja, ib=ib, gapA=gapA, secondA=secondA, gapB=gapB, secondB=secondB,
                      d_max=np.sqrt(max(mA.max(), mB.max())))


def undecided(info, E):
    """how many of the M + P minima are not decided at the bound E"""
    n = 0
    for gap, second in ((info["gapA"], info["secondA"]), (info["gapB"], info["secondB"])):
        fin = np.isfinite(second)
        n += int((gap[fin] <= 2 * (2 * np.sqrt(second[fin]) * E + E * E)).sum())
    return n


def loss_bound(info, E, w):
    return (1 + abs(w)) * (2 * info["d_max"] * E + E * E)


def grad_bound(a32, p, g, info, E, w):
    R = np.abs(np.asarray(a32, np.float64)).sum(1).max()
    g = np.abs(np.asarray(g, np.float64))
    xy = 2 * (1 + abs(w)) * E
    sc = 2 * (1 + abs(w)) * R * (E + 4 * U * info["d_max"])
    return np.array([xy, xy, sc, abs(float(p[2])) * sc]) + U * g


def starts64(b):
    """[2, 4]: the reference's two starts of a row's points b [P, 2]"""
    b = np.asarray(b, np.float64)
    d = ((b[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    i, j = np.unravel_index(d.argmax(), d.shape)
    v = b[j] - b[i]
    ang = -np.arctan2(v[0], v[1])
    c = b.mean(0)
    return np.array([[c[0], c[1], 2.0, ang], [c[0], c[1], 2.0, (ang + np.pi) % (2 * np.pi)]])


def _select(losses, n_run=None):
    """the first smallest loss, a NaN larger than a number, among the first n_run starts (all of them unless given)"""
    best = 0
    for s in range(1, len(losses) if n_run is None else n_run):
        if losses[s] < losses[best] or (np.isnan(losses[best]) and not np.isnan(losses[s])):
            best = s
    return best


def fit64(a, b, starts, n_steps=N_STEPS, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA, w=1.0, wrong=None, E=None):
    """the fit of one row in float64: dict of params [4], loss, best, all_params [S, 4], all_loss [S], grad [S, 4],
    trace [S, n_steps, 9] and - when E (the bound) is given - undecided [S, evaluations]: the undecided minima of every
    evaluation.  wrong: one of WRONG"""
    assert wrong is None or wrong in WRONG
    starts = np.asarray(starts, np.float64)
    S = len(starts)
    out = dict(all_params=np.empty((S, 4)), all_loss=np.empty(S), grad=np.empty((S, 4)), trace=np.empty((S, n_steps, 9)),
               undecided=np.zeros((S, max(n_steps, 1)), np.int64))
    kw = dict(one_direction=wrong == "one direction only", transposed=wrong == "R transposed in the angle term")
    for s in range(S):
        p = starts[s].copy()
        rates = np.array([lr, lr, lr, lr if wrong == "angle stepped with lr" else angle_lr])
        if wrong == "decay before the first step":
            rates = rates * gamma
        buf = np.zeros(4)
        L, g, info = evaluate64(a, b, p, w, **kw)
        for i in range(max(n_steps, 1)):
            if i:
                L, g, info = evaluate64(a, b, p, w, **kw)
            if E is not None:
                out["undecided"][s, i] = undecided(info, E if np.isscalar(E) else E(p))
            if n_steps == 0:
                break
            out["trace"][s, i] = np.concatenate([p, [L], g])
            buf = g.copy() if i == 0 or wrong == "no momentum" else momentum * buf + g
            step = g + momentum * buf if wrong == "Nesterov" else buf
            p = p - rates * step
            if wrong != "no decay":
                rates = rates * gamma
        if wrong == "loss after the last update" and n_steps:
            L = evaluate64(a, b, p, w, **kw)[0]
        out["all_params"][s], out["all_loss"][s], out["grad"][s] = p, L, g
    best = _select(out["all_loss"])
    out.update(best=best, params=out["all_params"][best], loss=out["all_loss"][best])
    return out


# ---- a float32 emulation of the contract's operation order (items 1 - 7), fp32 values held in float64 ----
def evaluate32(a, b, p, w=1.0, one_direction=False, transposed=False):
    """(L, g [4]) as fp32 values by the contract: a [M, 2], b [P, 2] and p hold fp32 values"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float64)
    x, y, sc, ang = (float(np.float32(v)) for v in p)
    cs, sn = float(np.float32(np.cos(ang))), float(np.float32(np.sin(ang)))
    qx = _fma(-a[:, 1], sn, _f32(a[:, 0] * cs))
    qy = _fma(a[:, 1], cs, _f32(a[:, 0] * sn))
    A = np.stack([_fma(qx, sc, x), _fma(qy, sc, y)], 1)
    assert np.array_equal(A, ho.template32(a, np.asarray(p, np.float32)))        # the placement is hint_hausdorff_run's
    ex = _f32(A[:, None, 0] - b[None, :, 0])
    ey = _f32(A[:, None, 1] - b[None, :, 1])
    D = _fma(ey, ey, _f32(ex * ex))
    M, P = D.shape
    ja, ib = D.argmin(1), D.argmin(0)                    # (the first among equals)
    sums = []
    for ii, jj in ((ib, np.arange(P)), (np.arange(M), ja)):
        e0, e1, q0, q1 = ex[ii, jj], ey[ii, jj], qx[ii], qy[ii]
        dot = _fma(e1, q1, _f32(e0 * q0))
        cross = (-1.0 if transposed else 1.0) * _fma(e1, q0, -_f32(e0 * q1))
        sums.append(np.array([D[ii, jj].sum(), e0.sum(), e1.sum(), dot.sum(), cross.sum()]))
    SB, SA = sums
    wA = 0.0 if one_direction else w
    t = SB / P + wA * (SA / M)
    L = float(_f32(t[0]))
    g = _f32(np.array([2 * t[1], 2 * t[2], 2 * t[3], 2 * sc * t[4]]))
    return L, g


def emulate32(a, b, starts, n_steps=N_STEPS, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA, w=1.0, wrong=None):
    """fit64's outputs (without `undecided`) by the contract's fp32 operation order; a, b, starts hold fp32 values"""
    assert wrong is None or wrong in WRONG
    starts = np.asarray(starts, np.float32).astype(np.float64)
    S = len(starts)
    out = dict(all_params=np.empty((S, 4)), all_loss=np.empty(S), grad=np.empty((S, 4)), trace=np.empty((S, n_steps, 9)))
    kw = dict(one_direction=wrong == "one direction only", transposed=wrong == "R transposed in the angle term")
    mom = float(np.float32(momentum))
    for s in range(S):
        p = starts[s].copy()
        rates = np.array([lr, lr, lr, lr if wrong == "angle stepped with lr" else angle_lr], np.float64)
        if wrong == "decay before the first step":
            rates = rates * gamma
        buf = np.zeros(4)
        L, g = evaluate32(a, b, p, w, **kw)
        for i in range(n_steps):
            if i:
                L, g = evaluate32(a, b, p, w, **kw)
            out["trace"][s, i] = np.concatenate([p, [L], g])
            buf = g.copy() if i == 0 or wrong == "no momentum" else _fma(mom, buf, g)
            step = _fma(mom, buf, g) if wrong == "Nesterov" else buf
            p = _fma(-_f32(rates), step, p)
            if wrong != "no decay":
                rates = rates * gamma
        if wrong == "loss after the last update" and n_steps:
            L = evaluate32(a, b, p, w, **kw)[0]
        out["all_params"][s], out["all_loss"][s], out["grad"][s] = p, L, g
    best = _select(out["all_loss"])
    out.update(best=best, params=out["all_params"][best], loss=out["all_loss"][best])
    return out


def angle_diff(a, b):
    """a - b reduced to [-pi, pi): fitted angles are compared up to whole turns"""
    return (np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2 * np.pi) - np.pi


def param_diff(a, b):
    """the largest difference of two parameter sets [..., 4], the angle up to whole turns"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(max(np.abs(a[..., :3] - b[..., :3]).max(), np.abs(angle_diff(a[..., 3], b[..., 3])).max()))


# ---- what the CPU and the device tests share ----
# the rows of the short fits: the rows of lens_rows(seed, draw) whose float64 trajectories from starts64 are decided at every
# evaluation of 5 steps of both starts (4 of the first 96; the tests assert it of each and leave none out)
SHORT = dict(seed=401, draw=49, rows=(3, 8, 38, 48), steps=(1, 2, 5))


def short_rows():
    """(x [4, 20], the float64 points [4, 100, 2], delta_B [4], starts [4, 2, 4] fp32) of the short fits"""
    x = lens_rows(SHORT["seed"], SHORT["draw"])[list(SHORT["rows"])]
    b = co.points64(x, FIT_P)
    return x, b, delta_B(x), np.stack([starts64(r) for r in b]).astype(np.float32)


def fit_dev(got, ref):
    """the largest deviation of a fit's per-start parameters (angles up to whole turns) and losses from ref's"""
    return max(param_diff(got["all_params"], ref["all_params"]),
               float(np.abs(np.asarray(got["all_loss"], np.float64) - ref["all_loss"]).max()))


def compare_evaluations(a32, b, dB, w, params, losses, grads):
    """evaluations (L, g) at the fp32 parameters `params` [n, 4] against evaluate64 there: (how many are undecided, the worst
    loss error / bound and the worst gradient error / bound [4] over the decided ones)"""
    n_und, r_loss, r_grad = 0, 0.0, np.zeros(4)
    for p, L, g in zip(np.asarray(params, np.float64), np.asarray(losses, np.float64), np.asarray(grads, np.float64)):
        L64, g64, info = evaluate64(a32, b, p, w)
        E = bound_E(a32, b, p, dB)
        if undecided(info, E):
            n_und += 1
            continue
        with np.errstate(divide="ignore", invalid="ignore"):              # (a zero bound is met by a zero error alone)
            err, bound = np.abs(np.append(g - g64, L - L64)), np.append(grad_bound(a32, p, g64, info, E, w), loss_bound(info, E, w))
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        rl, rg = r[4], r[:4]
        r_loss = max(r_loss, rl if np.isfinite(rl) else np.inf)
        r_grad = np.maximum(r_grad, np.where(np.isfinite(rg), rg, np.inf))
    return n_und, r_loss, r_grad


def check_update_rule(trace, all_params, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA):
    """the update rule on a traced fit of one start, every step: p_(i+1) - recorded as the next step's parameters, the last one
    as all_params - against fma(-lr_i, buf_i, p_i) with buf rebuilt from the traced gradients: the largest error in units of
    one fp32 ulp of the larger magnitude.  A record is p, L, g: the number of parameters is read from its width, and the last
    one is the angle"""
    trace = np.asarray(trace, np.float32).astype(np.float64)
    n, npar = len(trace), (trace.shape[1] - 1) // 2
    nxt = np.concatenate([trace[1:, :npar], np.asarray(all_params, np.float32).astype(np.float64)[None]])
    rates = np.array([lr] * (npar - 1) + [angle_lr], np.float64)
    mom = float(np.float32(momentum))
    buf, worst = None, 0.0
    for i in range(n):
        g = trace[i, npar + 1:]
        buf = g.copy() if i == 0 else _fma(mom, buf, g)
        want = _fma(-_f32(rates), buf, trace[i, :npar])
        big = np.maximum(np.abs(want), np.abs(nxt[i]))
        ulp = np.spacing(big.astype(np.float32)).astype(np.float64)
        err = np.abs(nxt[i] - want) / ulp
        worst = max(worst, float(np.where(np.isfinite(err), err, np.inf).max()))
        rates = rates * gamma
    return worst


def near_params(a, b, seed, S, steps=40):
    """[N, S, 4] fp32 parameters in a fit's working range for the rows' points b [N, P, 2]: where fit64 stands after `steps`
    steps from the reference's starts, moved by 0.01 randn.  (Far from the curve every distance is large and so is the
    allowance of the rule for a decided minimum: parameters drawn at large leave a third of the evaluations undecided)"""
    rs = np.random.RandomState(seed)
    out = np.empty((len(b), S, 4))
    for n in range(len(b)):
        fit = fit64(a, b[n], starts64(b[n]), steps)["all_params"]
        for s in range(S):
            out[n, s] = fit[s % 2] + 0.01 * rs.randn(4)
    return out.astype(np.float32)
