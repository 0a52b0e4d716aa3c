"""Float64 restatement of the plus-shape fit (hint_amd.curves plus_fit_grad / plus_dominant_angle / plus_fit_starts /
fit_plus_shapes, include/hint_amd.h hint_plusfit_run), a float32 emulation of the contract's operation order with deliberately
wrong variants, and the rules device results are compared by.  Written fresh from the contract; nothing of the reference is used.

Per row: B = the curve's P points, p = (xlength, ylength, xwidth, ywidth, xshift, yshift, xoffset, yoffset, angle), W_0..W_11 the
placed vertices (plus_oracle), segment s = (W_s, W_(s+1)), kept iff its local vertices differ, nk of them.  For a point b and its
segment s (the first nearest): t = len / L, v = (W_s - b) + t (W_(s+1) - W_s);
  L = mean_j |v_j|^2 + c mean over the kept s of min_j |W_s - B_j|^2
  dL / dW_k = (2 / P) sum_j ([s_j = k] v_j (1 - t_j) + [s_j + 1 = k] v_j t_j) + [k kept] (2 c / nk) (W_k - B_j*(k))
chained to the nine parameters through W = V R + (xoffset, yoffset), the vertex tables and the four clamps (the derivative to the
branch taken; on equality to the unclamped side).  The schedule is torch's SGD(momentum, dampening 0) under StepLR(step_size 1):
buf = g_0, then momentum buf + g_i; p_(i+1) = p_i - lr_i buf, lr_i = lr gamma^i (angle_lr for the angle); step i of n uses the
corner weight c (1 - i / n).  A start's loss is L_(n - 1); a start whose loss is < stop_loss ends the row; the row's result is
the start that ran with the smallest loss, the first on a tie.

The rules.  u = 2^-24; E is plus_oracle's bound E' on a distance at these parameters (bound_E below: 2 (delta_A + delta_B) + 12 u
far); Lmin the shortest kept segment; R = max_k (|V_k.x| + |V_k.y|); d_max the root of the largest selected squared distance.
  decided   a point's segment is decided when the gap of its squared distance to the best candidate whose nearest point differs
            (by more than 1e-9: two adjacent segments that both clamp to their shared vertex give the same value and the same
            derivative, so they are no tie) exceeds 2 (2 sqrt(D_second) E + E^2); a corner's curve point likewise, among the
            points whose coordinates differ from the chosen one's; a clamp is decided when its two arguments differ by more than
            4 u (|shift| + |length| / 2 + |width| / 2 + 0.01).  An evaluation is compared only when all of these are decided.
  zero width  at a width of exactly 0 the two long sides of that bar coincide: every point nearest to the bar ties between them
            (the same nearest point, the same value), and the tie decides the sign of that width's derivative and nothing else
            (the reference's own choice there is torch.min's tie order).  That one component - xwidth's at xwidth = 0, ywidth's
            at ywidth = 0 - is not compared on such a row; the loss and the other eight are.
  loss      |L - L64| <= (1 + |c|) (2 d_max E + E^2)
  gradient  with the selections equal, v is off by at most E per component and t = len / L by dt = 2 E / Lmin + 4 u, so a
            product v (1 - t) or v t by E + d_max dt + u d_max; the weights 2 / P of the P points sum to 2, the corner's
            2 |c| / nk over nk differences, each off by E, to 2 |c|:
              eW = 2 (E + d_max (dt + u)) + 2 |c| E          bounds sum_k |gW_k - gW64_k| per axis
            The chain multiplies by cs, sn (|cs| + |sn| <= sqrt 2 < 2, both rounded: 2 u relative, products and sums 6 u more)
            and adds with weights 1 or 1/2:
              offsets                   eW + u |g|
              lengths, widths, shifts   2 eW + 8 u G + u |g|,      G = sum_k (|gW64_k.x| + |gW64_k.y|)
              angle                     R (2 eW + 8 u G) + u |g|   (q_k = V_k R is formed in double from fp32 V, cs, sn)
  fits      a whole or a short fit is compared with fit64 from the same starts at 16 x the largest deviation of the fp32
            emulation (emulate32) from fit64 on the same rows.
"""
import numpy as np

import curve_oracle as co
import lensfit_oracle as lfo
import plus_oracle as po
from curve_oracle import _f32, _fma
from lensfit_oracle import _select  # noqa: F401  (the tests' too)

U = 2.0 ** -24
LR, ANGLE_LR, MOMENTUM, GAMMA, N_STEPS, STOP = 0.1, 0.01, 0.2, 0.1 ** (1 / 400), 400, 0.005
XYSHIFTS = ((0, 0), (-1.5, -1.5), (-1.5, 0), (-1.5, 1.5), (0, -1.5), (0, 1.5), (1.5, -1.5), (1.5, 0), (1.5, 1.5))
FIT_P = 100
RESIDUAL = 0.05

# fixtures tests/golden/plusfit_<name>.npz (tests/golden/make_plusfit_golden.py)
GOLDEN_GRAD = dict(name="grad_n16", seed=511, rows=16, weights=(1.0, 0.37, 0.0))
GOLDEN_FIT = dict(name="fit_n6", seed=521, rows=6, np_seed=7)

# variants of the evaluation and of the schedule that a test must tell from the contract
WRONG = ("t not clamped", "all of the derivative to the first vertex", "clamp derivative to the wrong branch",
         "corner weight constant", "corner weight decayed one step early", "angle stepped with lr", "no momentum",
         "R transposed in the angle term", "loss after the last update")
WRONG_EVAL = ("t not clamped", "all of the derivative to the first vertex", "clamp derivative to the wrong branch",
              "R transposed in the angle term", "corner mean over 12 with a dropped segment")
WRONG_STOP = ("no early stop", "stop compared with <=")


# ---- inputs ----
def plus_rows(seed, N, K=25):
    """(x [N, 4 K] fp32, the shapes' parameters [N, 9]): plus-like curves - the outline of plus_oracle.draw_params rows, 60
    points an edge, through lensfit_oracle.fourier_coeffs"""
    params = po.draw_params(seed, N)
    seg, keep = po.segments64(params)
    kb = po.keep_bits(keep)
    out = np.empty((N, 4 * K), np.float32)
    t = np.arange(60) / 60.0
    for n in range(N):
        pts = [seg[n, s, 0][None, :] + t[:, None] * (seg[n, s, 1] - seg[n, s, 0])[None, :] for s in range(12) if kb[n, s]]
        out[n] = lfo.fourier_coeffs(np.concatenate(pts), K)
    return out, params


def eval_params(base, seed, zero_width=(), clamped=()):
    """[N, 9] fp32 parameters near the shapes `base` [N, 9], moved by 0.05 randn; rows in zero_width get xwidth = 0 (two dropped
    segments), rows in clamped xlength = 1 and ywidth = 2 (a clamp of the x arm acts whatever the shift, or both do)"""
    p = np.asarray(base, np.float64) + 0.05 * np.random.RandomState(seed).randn(*np.shape(base))
    for r in zero_width:
        p[r, 2] = 0.0
    for r in clamped:
        p[r, 0], p[r, 3] = 1.0, 2.0
    return p.astype(np.float32)


def delta_B(x):
    return lfo.delta_B(x)


# ---- float64 ----
def _local(p):
    """(the eight clamped coordinates in PL_VX / PL_VY order, the four `free` flags: l, r, t, b - the clamp did not act - and
    the four margins between a clamp's arguments)"""
    xl, yl, xw, yw, xs, ys = (float(v) for v in p[:6])
    xtop, yright = xw / 2, yw / 2
    a = (xs - xl / 2, xs + xl / 2, ys + yl / 2, ys - yl / 2)                 # unclamped xleft, xright, ytop, ybottom
    b = (-yright - 0.01, yright + 0.01, xtop + 0.01, -xtop - 0.01)
    free = (a[0] <= b[0], a[1] >= b[1], a[2] >= b[2], a[3] <= b[3])
    xleft, xright = min(a[0], b[0]), max(a[1], b[1])
    ytop, ybottom = max(a[2], b[2]), min(a[3], b[3])
    c = np.array([xleft, -yright, yright, xright, xtop, ytop, -xtop, ybottom])
    return c, free, np.abs(np.array(a) - np.array(b))


IX = np.array(po.VX)                 # vertex k takes c[IX[k]], c[4 + IY[k]]
IY = np.array(po.VY)
_CY = np.array([4, 5, 6, 7])[IY]


def _chain(gW, c, free, cs, sn, wrong=None):
    """the nine derivatives from dL / dW [12, 2]"""
    V = np.stack([c[IX], c[_CY]], 1)
    q = np.stack([V[:, 0] * cs - V[:, 1] * sn, V[:, 0] * sn + V[:, 1] * cs], 1)
    sign = -1.0 if wrong == "R transposed in the angle term" else 1.0
    gan = sign * (gW[:, 1] * q[:, 0] - gW[:, 0] * q[:, 1]).sum()
    gV = np.stack([gW[:, 0] * cs + gW[:, 1] * sn, gW[:, 1] * cs - gW[:, 0] * sn], 1)
    gc = np.zeros(8)
    np.add.at(gc, IX, gV[:, 0])
    np.add.at(gc, _CY, gV[:, 1])
    if wrong == "clamp derivative to the wrong branch":
        free = tuple(not f for f in free)
    gxl = gyl = gxs = gys = 0.0
    gxw, gyw = 0.5 * gc[4] - 0.5 * gc[6], 0.5 * gc[2] - 0.5 * gc[1]
    if free[0]:
        gxs, gxl = gxs + gc[0], gxl - 0.5 * gc[0]
    else:
        gyw -= 0.5 * gc[0]
    if free[1]:
        gxs, gxl = gxs + gc[3], gxl + 0.5 * gc[3]
    else:
        gyw += 0.5 * gc[3]
    if free[2]:
        gys, gyl = gys + gc[5], gyl + 0.5 * gc[5]
    else:
        gxw += 0.5 * gc[5]
    if free[3]:
        gys, gyl = gys + gc[7], gyl - 0.5 * gc[7]
    else:
        gxw -= 0.5 * gc[7]
    return np.array([gxl, gyl, gxw, gyw, gxs, gys, gW[:, 0].sum(), gW[:, 1].sum(), gan])


def evaluate64(b, p, c=1.0, wrong=None):
    """(L, g [9], info) at parameters p with corner weight c.  info: the selections (seg [P], t [P], corner [12]), per point
    and per kept corner the gap to the best candidate that differs and that candidate's squared distance, the clamps' margins,
    d_max, Lmin, R, G"""
    b = np.asarray(b, np.float64)
    p = np.asarray(p, np.float64)
    P = len(b)
    cc, free, margins = _local(p)
    V = np.stack([cc[IX], cc[_CY]], 1)
    kept = (V != np.roll(V, -1, 0)).any(1)
    cs, sn = np.cos(p[8]), np.sin(p[8])
    W = np.stack([V[:, 0] * cs - V[:, 1] * sn + p[6], V[:, 0] * sn + V[:, 1] * cs + p[7]], 1)
    W1 = np.roll(W, -1, 0)
    nv = W1 - W
    Ls = np.sqrt((nv ** 2).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = nv / Ls[:, None]
    ap = W[:, None, :] - b[None, :, :]                                       # [12, P, 2]
    dot = -(ap * nv[:, None, :]).sum(2)
    ln = np.clip(dot, 0.0, Ls[:, None])
    v = ap + ln[:, :, None] * nv[:, None, :]
    d2 = np.where(kept[:, None], (v ** 2).sum(2), np.inf)
    seg = d2.argmin(0)
    pts = np.arange(P)
    dmin, vsel = d2[seg, pts], v[seg, pts]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (dot if wrong == "t not clamped" else ln)[seg, pts] / Ls[seg]
    gW = np.zeros((12, 2))
    if wrong == "all of the derivative to the first vertex":
        np.add.at(gW, seg, 2.0 / P * vsel)
    else:
        np.add.at(gW, seg, 2.0 / P * vsel * (1 - t)[:, None])
        np.add.at(gW, (seg + 1) % 12, 2.0 / P * vsel * t[:, None])
    D = ((W[:, None, :] - b[None, :, :]) ** 2).sum(2)                        # [12, P]
    jc = D.argmin(1)
    cmin = D[np.arange(12), jc]
    nk = int(kept.sum())
    div = 12 if wrong == "corner mean over 12 with a dropped segment" else nk
    gW[kept] += 2.0 * c / div * (W - b[jc])[kept]
    L = dmin.mean() + c * cmin[kept].sum() / div
    g = _chain(gW, cc, free, cs, sn, wrong)
    # the gaps: a segment's nearest point is b + v
    near = b[None, :, :] + v
    same = (np.abs(near - near[seg, pts][None, :, :]).max(2) <= 1e-9) | ~kept[:, None]
    second = np.where(same, np.inf, d2).min(0)
    same_c = (b[None, :, :] == b[jc][:, None, :]).all(2)
    second_c = np.where(same_c, np.inf, D).min(1)
    info = dict(seg=seg, t=t, corner=jc, kept=kept, gap=second - dmin, second=second, gap_c=(second_c - cmin)[kept],
                second_c=second_c[kept], margins=margins,
                margin_bound=4 * U * (np.abs(p[[4, 4, 5, 5]]) + np.abs(p[[0, 0, 1, 1]]) / 2 + np.abs(p[[3, 3, 2, 2]]) / 2 + 0.01),
                d_max=np.sqrt(max(dmin.max(), cmin[kept].max())), Lmin=Ls[kept].min(), R=np.abs(V).sum(1).max(),
                G=np.abs(gW).sum(), skip=np.array([False, False, p[2] == 0, p[3] == 0] + [False] * 5), far=np.sqrt(D.max()), dA=12 * U * (np.abs(V).sum(1).max() + np.abs(p[6:8]).max()))
    return L, g, info


def bound_E(info, dB=0.0):
    return 2 * (info["dA"] + dB) + 12 * U * info["far"]


def undecided(info, E):
    """how many of the P segments, the nk corner points and the four clamps are not decided at the bound E"""
    n = 0
    for gap, second in ((info["gap"], info["second"]), (info["gap_c"], info["second_c"])):
        fin = np.isfinite(second)
        n += int((gap[fin] <= 2 * (2 * np.sqrt(second[fin]) * E + E * E)).sum())
    return n + int((info["margins"] <= info["margin_bound"]).sum())


def loss_bound(info, E, c):
    return (1 + abs(c)) * (2 * info["d_max"] * E + E * E)


def grad_bound(g, info, E, c):
    """[9]; inf where the component is not compared (the zero-width rule)"""
    g = np.abs(np.asarray(g, np.float64))
    dt = 2 * E / info["Lmin"] + 4 * U
    eW = 2 * (E + info["d_max"] * (dt + U)) + 2 * abs(c) * E
    par = 2 * eW + 8 * U * info["G"]
    return np.where(info["skip"], np.inf, np.array([par] * 6 + [eW, eW, info["R"] * par]) + U * g)


def starts64(b, angle):
    """[9, 9]: the reference's nine starts of a row's points b [P, 2] at the dominant angle"""
    cx, cy = np.asarray(b, np.float64).mean(0)
    return np.array([[5.0, 5.0, 2.0, 2.0, xs, ys, cx, cy, angle] for xs, ys in XYSHIFTS])


def angle64(b, tol=1e-5):
    """(angle, decided) of a row's points b [P, 2]: every pair i < j with x_i != x_j is a candidate line, its inliers the points
    within RESIDUAL of it in y, the winner the first pair in row-major order with the most inliers, the angle atan of the slope
    of the least-squares line through the winner's inliers.  decided: no pair within one inlier of the winner's count has a
    residual within tol of the threshold, so counts taken in fp32 give the same winner"""
    b = np.asarray(b, np.float64)
    x, y = b[:, 0], b[:, 1]
    P = len(b)
    i, j = np.triu_indices(P, 1)
    ok = x[i] != x[j]
    i, j = i[ok], j[ok]
    if len(i) == 0:
        return 0.0, True
    slope = (y[j] - y[i]) / (x[j] - x[i])
    resid = np.abs(y[None, :] - (slope[:, None] * x[None, :] + (y[i] - slope * x[i])[:, None]))
    cnt = (resid <= RESIDUAL).sum(1)
    w = int(cnt.argmax())
    close = cnt >= cnt[w] - 1
    decided = bool((np.abs(resid[close] - RESIDUAL) > tol).all())
    inl = resid[w] <= RESIDUAL
    xm, ym = x[inl].mean(), y[inl].mean()
    sxx, sxy = ((x[inl] - xm) ** 2).sum(), ((x[inl] - xm) * (y[inl] - ym)).sum()
    return (float(np.arctan(sxy / sxx)) if sxx > 0 else 0.0), decided


def corner_weight(c, i, n_steps, decay=True, wrong=None):
    if not decay or n_steps == 0 or wrong == "corner weight constant":
        return c
    return c * (1 - (i + 1 if wrong == "corner weight decayed one step early" else i) / n_steps)


def _fit(ev, fma, f32, b, starts, n_steps, lr, angle_lr, momentum, gamma, c, decay, stop_loss, wrong, und):
    assert wrong is None or wrong in WRONG + WRONG_STOP
    S = len(starts)
    out = dict(all_params=starts.copy(), all_loss=np.full(S, np.inf), grad=np.full((S, 9), np.nan),
               trace=np.full((S, n_steps, 19), np.nan), undecided=np.zeros((S, max(n_steps, 1)), np.int64))
    n_run = 0
    for s in range(S):
        p = starts[s].copy()
        rates = np.array([lr] * 8 + [lr if wrong == "angle stepped with lr" else angle_lr], np.float64)
        buf = np.zeros(9)
        for i in range(max(n_steps, 1)):
            cw = corner_weight(c, i, n_steps, decay, wrong)
            L, g, info = ev(b, p, cw, wrong if wrong in WRONG_EVAL else None)
            if und is not None:
                out["undecided"][s, i] = und(info)
            if n_steps == 0:
                break
            out["trace"][s, i] = np.concatenate([p, [L], g])
            buf = g.copy() if i == 0 or wrong == "no momentum" else fma(momentum, buf, g)
            p = fma(-f32(rates), buf, p)
            rates = rates * gamma
        if wrong == "loss after the last update" and n_steps:
            L = ev(b, p, corner_weight(c, n_steps - 1, n_steps, decay), None)[0]
        out["all_params"][s], out["all_loss"][s], out["grad"][s] = p, L, g
        n_run = s + 1
        if wrong != "no early stop" and stop_loss > 0 and (L <= stop_loss if wrong == "stop compared with <=" else L < stop_loss):
            break
    best = _select(out["all_loss"], n_run)
    out.update(best=best, n_run=n_run, params=out["all_params"][best], loss=out["all_loss"][best])
    return out


def fit64(b, starts, n_steps=N_STEPS, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA, c=1.0, decay=True,
          stop_loss=STOP, wrong=None, dB=None):
    """the fit of one row in float64: dict of params [9], loss, best, n_run, all_params [S, 9], all_loss [S], grad [S, 9],
    trace [S, n_steps, 19] and - when dB (the bound on a curve point) is given - undecided [S, evaluations]"""
    und = None if dB is None else (lambda info: undecided(info, bound_E(info, dB)))
    return _fit(lambda b_, p, cw, w: evaluate64(b_, p, cw, w), lambda a, x, y: a * x + y, lambda v: v, np.asarray(b, np.float64),
                np.asarray(starts, np.float64), n_steps, lr, angle_lr, momentum, gamma, c, decay, stop_loss, wrong, und)


# ---- a float32 emulation of the contract's operation order, fp32 values held in float64 ----
def evaluate32(b, p, c=1.0, wrong=None):
    """(L, g [9], None) as fp32 values by the contract; b [P, 2] and p hold fp32 values"""
    b = np.asarray(b, np.float64)
    p = np.asarray(np.asarray(p, np.float32), np.float64)
    P = len(b)
    V = po.local32(p)
    kept = (V != np.roll(V, -1, 0)).any(1)
    W = po.place32(V, p)
    W1 = np.roll(W, -1, 0)
    nv = _f32(W1 - W)
    Ls = _f32(np.sqrt(_fma(nv[:, 1], nv[:, 1], _f32(nv[:, 0] * nv[:, 0]))))
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = _f32(nv / Ls[:, None])
    ap = _f32(W[:, None, :] - b[None, :, :])
    dot = -_fma(ap[:, :, 1], nv[:, None, 1], _f32(ap[:, :, 0] * nv[:, None, 0]))
    ln = np.maximum(0.0, np.minimum(Ls[:, None], dot))
    vx, vy = _fma(ln, nv[:, None, 0], ap[:, :, 0]), _fma(ln, nv[:, None, 1], ap[:, :, 1])
    d2 = np.where(kept[:, None], _fma(vy, vy, _f32(vx * vx)), np.inf)
    seg = d2.argmin(0)                                                       # (the first among equals)
    pts = np.arange(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = _f32(ln[seg, pts] / Ls[seg])
    om = _f32(1.0 - t)
    G = np.zeros((12, 2))
    for comp, vv in enumerate((vx[seg, pts], vy[seg, pts])):
        np.add.at(G[:, comp], seg, _f32(vv * om))
        np.add.at(G[:, comp], (seg + 1) % 12, _f32(vv * t))
    dx, dy = _f32(W[:, None, 0] - b[None, :, 0]), _f32(W[:, None, 1] - b[None, :, 1])
    D = _fma(dy, dy, _f32(dx * dx))
    jc = D.argmin(1)
    nk = int(kept.sum())
    gW = 2.0 / P * G
    gW[kept] += (2.0 * c / nk) * np.stack([dx[np.arange(12), jc], dy[np.arange(12), jc]], 1)[kept]
    L = float(_f32(d2[seg, pts].sum() / P + c * (D[np.arange(12), jc][kept].sum() / nk)))
    # the clamps' branches from the fp32 arguments; the chain in double from the fp32 V, cs, sn
    xl, yl, xw, yw, xs, ys = (float(v) for v in p[:6])
    hx, hy, xtop, yright = _f32(0.5 * xl), _f32(0.5 * yl), _f32(0.5 * xw), _f32(0.5 * yw)
    c32 = po.C32
    free = (_f32(xs - hx) <= _f32(-yright - c32), _f32(xs + hx) >= _f32(yright + c32),
            _f32(ys + hy) >= _f32(xtop + c32), _f32(ys - hy) <= _f32(-xtop - c32))
    cc = np.array([V[0, 0], V[1, 0], V[3, 0], V[5, 0], V[0, 1], V[2, 1], V[6, 1], V[8, 1]])
    cs, sn = float(np.float32(np.cos(p[8]))), float(np.float32(np.sin(p[8])))
    return L, _f32(_chain(gW, cc, free, cs, sn)), None


def emulate32(b, starts, n_steps=N_STEPS, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA, c=1.0, decay=True,
              stop_loss=STOP, wrong=None):
    """fit64's outputs by the contract's fp32 operation order; b and starts hold fp32 values"""
    return _fit(lambda b_, p, cw, w: evaluate32(b_, p, cw, w), _fma, _f32, np.asarray(b, np.float64),
                np.asarray(starts, np.float32).astype(np.float64), n_steps, lr, angle_lr, float(np.float32(momentum)), gamma, c,
                decay, stop_loss, wrong, None)


def angle_diff(a, b):
    return lfo.angle_diff(a, b)


def param_diff(a, b):
    """the largest difference of two parameter sets [..., 9], the angle up to whole turns"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(max(np.abs(a[..., :8] - b[..., :8]).max(), np.abs(angle_diff(a[..., 8], b[..., 8])).max()))


def fit_dev(got, ref, n_run=None):
    """the largest deviation of a fit's per-start parameters and losses from ref's, over the starts that ran"""
    k = ref["n_run"] if n_run is None else n_run
    return max(param_diff(np.asarray(got["all_params"])[:k], ref["all_params"][:k]),
               float(np.abs(np.asarray(got["all_loss"], np.float64)[:k] - ref["all_loss"][:k]).max()))


# ---- what the CPU and the device tests share ----
def compare_evaluations(b, dB, c, params, losses, grads):
    """evaluations (L, g) at the fp32 parameters `params` [n, 9] against evaluate64 there: (how many are undecided, the worst
    loss error / bound and the worst gradient error / bound [9] over the decided ones)"""
    n_und, r_loss, r_grad = 0, 0.0, np.zeros(9)
    cs = np.broadcast_to(np.asarray(c, np.float64), (len(params),))
    for p, L, g, cw in zip(np.asarray(params, np.float64), np.asarray(losses, np.float64), np.asarray(grads, np.float64), cs):
        L64, g64, info = evaluate64(b, p, cw)
        E = bound_E(info, dB)
        if undecided(info, E):
            n_und += 1
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            err, bound = np.abs(np.append(g - g64, L - L64)), np.append(grad_bound(g64, info, E, cw), loss_bound(info, E, cw))
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        r = np.where(np.isfinite(r), r, np.inf)
        r_loss, r_grad = max(r_loss, r[9]), np.maximum(r_grad, r[:9])
    return n_und, r_loss, r_grad


def check_update_rule(trace, all_params, lr=LR, angle_lr=ANGLE_LR, momentum=MOMENTUM, gamma=GAMMA):
    """lensfit_oracle's, which reads the nine parameters from the trace's width, at this fit's schedule"""
    return lfo.check_update_rule(trace, all_params, lr, angle_lr, momentum, gamma)


# the rows of the evaluation tests: (name, source, P, N, S, corner weight, rows of zero width, rows with active clamps).  At P =
# 257 and 1024 a curve's neighbouring points lie nearer to each other than the rule for a decided corner point allows for, so
# there the oracle is met on given points scattered over the plane, and the traced source is tied to the given one bit for bit
EVAL_CASES = (("traced 100", "traced", 100, 9, 3, 1.0, (2,), (4,)), ("given 100", "given", 100, 3, 2, 0.37, (1,), (2,)),
              ("traced 100 w0", "traced", 100, 9, 1, 0.0, (0,), (1,)), ("traced 2", "traced", 2, 3, 1, 1.0, (), ()),
              ("scatter 257", "scatter", 257, 3, 2, 0.37, (1,), (2,)), ("scatter 1024", "scatter", 1024, 3, 3, 1.0, (0,), (1,)))


def eval_case(source, P, N, S, seed, zero, clamped):
    """(curve fp32, the float64 points [N, P, 2], delta_B [N], parameters fp32 [N, S, 9])"""
    x, base = plus_rows(seed, N)
    params = np.stack([eval_params(base, seed + 1 + s, zero, clamped) for s in range(S)], 1)
    if source == "scatter":
        # of 4 P points drawn over the square, the first P whose segment is decided, four times over, at all S parameters: a
        # point a hair past the end of a segment ties with the neighbour that clamps to the shared vertex, and among 1024 points
        # spread at large every evaluation holds a few
        cand = np.random.RandomState(seed).uniform(-3, 3, (N, 4 * P, 2)).astype(np.float32)
        curve = np.empty((N, P, 2), np.float32)
        for n in range(N):
            ok = np.ones(4 * P, bool)
            for s in range(S):
                info = evaluate64(cand[n], params[n, s], 1.0)[2]
                E = bound_E(info)
                ok &= info["gap"] > 8 * (2 * np.sqrt(np.minimum(info["second"], 1e30)) * E + E * E)
            assert ok.sum() >= P
            curve[n] = cand[n][ok][:P]
        b, dB = curve.astype(np.float64), np.zeros(N)
    else:
        b, dB = co.points64(x, P), delta_B(x)
        curve = x
        if source == "given":
            curve = b.astype(np.float32)
            b, dB = curve.astype(np.float64), np.zeros(N)
    return curve, b, dB, params


SHORT = dict(seed=601, rows=4, steps=(1, 2, 5))
WHOLE = dict(seed=701, rows=6)
