"""Float64 oracle of the polygon overlap (hint_amd.curves polygon_overlap / lens_iou_dice / plus_iou_dice, include/hint_amd.h
hint_overlap_run): two independent methods for the area of the intersection, a float32 emulation of the contract's operation
order with deliberately wrong variants, the crossing count with its margins, and the rules device results are compared by.
Written fresh from the contract; nothing of the reference is used (its two functions need shapely, which is not a dependency).

Per row: C = the curve's P vertices, T = the template's M vertices, both closed (edge i: vertex i -> vertex (i + 1) mod n);
y0 = the smallest y of all of them, h = y - y0.
  method A  I = | sum_e sum_f sign_e sign_f (the integral over the common x-interval of e and f of min(h_e, h_f)) |, split at the
            crossing of the two heights: the integral of the product of the two winding numbers (pair_terms64, overlap64)
  method B  the curve clipped against a convex polygon, half-plane by half-plane (Sutherland-Hodgman), and the shoelace area of
            what is left: the integral of the curve's winding number over the convex polygon (clip_area).  The lens prototype is
            convex; the plus is the union of its two arms, so clip(Rx) + clip(Ry) - clip(Rx and Ry) (plus_overlap_b).
  area(P) = | sum_e 0.5 (x1 - x0) (h0 + h1) |; I is cut to [0, min(area_C, area_T)]; IoU = I / (area_C + area_T - I),
  DICE = 2 I / (area_C + area_T), NaN where the denominator is 0.

The rules.  u = 2^-24.  A device row is compared with overlap64 of the very vertices the kernel uses (the fp32 curve points and
the fp32 placed template, as float64), so only the arithmetic of the terms is in question.  With S = sum |term| over the pairs and
S_C, S_T = sum |area term| over the edges:
  e_I = c u S, e_C = c u S_C, e_T = c u S_T;  the cut to [0, min(area_C, area_T)] is 1-Lipschitz in each argument, so the cut I is
  off by at most e_Ic = max(e_I, e_C, e_T);  areas: e + u |value| (the output's rounding)
  IoU   with D = area_C + area_T - I and e_D = e_C + e_T + e_Ic:  (e_Ic D + I e_D) / (D (D - e_D)) + u IoU
  DICE  with D = area_C + area_T and e_D = e_C + e_T:  2 (e_Ic D + I e_D) / (D (D - e_D)) + u DICE
c = C_TOL: the smallest power of two for which the fp32 emulation (emulate32) stays within a quarter of e_I, e_C and e_T on every
row of every ledger case (tests/test_overlap_cpu.py asserts that it is that power).  Why a relative bound per term holds: every
height is a sum of two non-negative products whose weights are quotients of single differences (relative error a few u, however
steep the edge), and where the heights cross the crossing's height is at least (1 - ta) max(ea, fa), which bounds the effect of the
cancellation in da = ea - fa relative to the term itself.
  crossings  a determinant det(p, q, s) = (q - p) x (s - p) is computed in fp32 with two rounded differences per factor, a rounded
            product and an fma: its error is below 4 u (|ux vy| + |uy vx|) - the margin.  A sign is certain when |det64| exceeds
            the margin, or when the margin is 0 (then both are exactly 0).  A pair is decided when one of its two sign tests is
            certainly false or both are certainly true; a row's count is compared only when all its pairs are decided.
"""
import numpy as np

import hausdorff_oracle as ho
import lensfit_oracle as lfo
import plus_oracle as po
import plusfit_oracle as pfo
from curve_oracle import _f32, _fma, trace32

U = 2.0 ** -24
TILE = 1024
C_TOL = 8.0
MIN_POINTS, MAX_POINTS, MAX_M = 3, 1024, 4096

WRONG = ("closing edge dropped", "tile seam edge dropped", "no split at the crossing", "baseline 0", "IoU denominator without - I",
         "R transposed", "adjacent pairs counted as crossings")


# ---- float64: method A ----
def _edges(v):
    """(x0, y0, x1, y1) of the closed polygon v [n, 2]"""
    w = np.roll(v, -1, axis=0)
    return v[:, 0], v[:, 1], w[:, 0], w[:, 1]


def _height(x0, h0, x1, h1, q):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip((q - x0) / (x1 - x0), 0.0, 1.0)
    return h0 + t * (h1 - h0)


def pair_terms64(C, T, keep_t=None, split=True, base=None):
    """the signed terms [P, M] of every curve edge against every template edge, in float64"""
    C, T = np.asarray(C, np.float64), np.asarray(T, np.float64)
    y0 = min(C[:, 1].min(), T[:, 1].min()) if base is None else base
    ex0, ey0, ex1, ey1 = (a[:, None] for a in _edges(C))
    fx0, fy0, fx1, fy1 = (a[None, :] for a in _edges(T))
    eh0, eh1, fh0, fh1 = ey0 - y0, ey1 - y0, fy0 - y0, fy1 - y0
    a = np.maximum(np.minimum(ex0, ex1), np.minimum(fx0, fx1))
    b = np.minimum(np.maximum(ex0, ex1), np.maximum(fx0, fx1))
    live = a < b
    w = np.where(live, b - a, 0.0)
    ea, eb = _height(ex0, eh0, ex1, eh1, a), _height(ex0, eh0, ex1, eh1, b)
    fa, fb = _height(fx0, fh0, fx1, fh1, a), _height(fx0, fh0, fx1, fh1, b)
    da, db = ea - fa, eb - fb
    ma, mb = np.minimum(ea, fa), np.minimum(eb, fb)
    cross = (da * db < 0) & live
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(cross, da / (da - db), 0.0)
    hc = ea + tau * (eb - ea)
    total = np.where(cross & split, hc + tau * ma + (1 - tau) * mb, ma + mb)
    sign = np.where((ex1 < ex0) != (fx1 < fx0), -1.0, 1.0)
    term = np.where(live, sign * 0.5 * w * total, 0.0)
    if keep_t is not None:
        term = term * np.asarray(keep_t, np.float64)[None, :]
    return term


def area_terms64(v, y0):
    x0, y0_, x1, y1 = _edges(np.asarray(v, np.float64))
    return 0.5 * (x1 - x0) * ((y0_ - y0) + (y1 - y0))


def _scores(at, ac, inter):
    inter = min(max(inter, 0.0), min(at, ac))
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.float64(inter) / np.float64(at + ac - inter)
        dice = np.float64(2 * inter) / np.float64(at + ac)
    return inter, float(iou), float(dice)


def overlap64(C, T):
    """one row: dict of area_T, area_C, I (cut), I_raw, iou, dice and the sums of magnitudes S, S_C, S_T"""
    C, T = np.asarray(C, np.float64), np.asarray(T, np.float64)
    y0 = min(C[:, 1].min(), T[:, 1].min())
    term = pair_terms64(C, T)
    tc, tt = area_terms64(C, y0), area_terms64(T, y0)
    at, ac, raw = abs(tt.sum()), abs(tc.sum()), abs(term.sum())
    inter, iou, dice = _scores(at, ac, raw)
    return dict(area_T=at, area_C=ac, I=inter, I_raw=raw, iou=iou, dice=dice, S=np.abs(term).sum(), S_C=np.abs(tc).sum(),
                S_T=np.abs(tt).sum())


# ---- float64: method B ----
def shoelace(v):
    """the signed area of the closed chain v [n, 2] (0 for fewer than 3 points), taken about its first point"""
    v = np.asarray(v, np.float64)
    if len(v) < 3:
        return 0.0
    v = v - v[0]
    w = np.roll(v, -1, axis=0)
    return 0.5 * float((v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1]).sum())


def clip_chain(subject, clip):
    """Sutherland-Hodgman: the closed chain `subject` cut by every half-plane of the convex polygon `clip` (either orientation;
    clip edges of no length define no half-plane and are skipped)"""
    clip = np.asarray(clip, np.float64)
    if shoelace(clip) < 0:
        clip = clip[::-1]
    pts = np.asarray(subject, np.float64)
    for k in range(len(clip)):
        A, B = clip[k], clip[(k + 1) % len(clip)]
        d = B - A
        if d[0] == 0 and d[1] == 0:
            continue
        if len(pts) == 0:
            break
        side = d[0] * (pts[:, 1] - A[1]) - d[1] * (pts[:, 0] - A[0])        # >= 0: inside
        nxt, side_n = np.roll(pts, -1, axis=0), np.roll(side, -1)
        inside, inside_n = side >= 0, side_n >= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            s = side / (side - side_n)
            hit = pts + s[:, None] * (nxt - pts)
        cand = np.stack([pts, hit], 1).reshape(-1, 2)
        mask = np.stack([inside, inside != inside_n], 1).reshape(-1)
        pts = cand[mask]
    return pts


def clip_area(C, clip):
    """| the integral of the curve's winding number over the convex polygon `clip` |, signed by the curve's own orientation"""
    return shoelace(clip_chain(C, clip))


def convex_overlap_b(C, T):
    """method B for a convex template: (area_T, area_C, I)"""
    return abs(shoelace(T)), abs(shoelace(C)), abs(clip_area(C, T))


def plus_arms(W):
    """the two arms and their common square of the plus outline W [12, 2] (hint_plus_desc's vertex order), as three quadrilaterals"""
    W = np.asarray(W, np.float64)
    return W[[0, 11, 6, 5]], W[[2, 9, 8, 3]], W[[1, 10, 7, 4]]


def plus_overlap_b(C, W):
    """method B for the plus: clip(Rx) + clip(Ry) - clip(Rx and Ry), every piece signed by the curve's orientation"""
    rx, ry, rc = plus_arms(W)
    inter = abs(clip_area(C, rx) + clip_area(C, ry) - clip_area(C, rc))
    at = abs(shoelace(rx)) + abs(shoelace(ry)) - abs(shoelace(rc))
    return at, abs(shoelace(C)), inter


# ---- crossings ----
def _det(p, q, s):
    ux, uy, vx, vy = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], s[..., 0] - p[..., 0], s[..., 1] - p[..., 1]
    return ux * vy - uy * vx, 4 * U * (np.abs(ux * vy) + np.abs(uy * vx))


def _pair_mask(P, adjacent=False):
    i, j = np.arange(P)[:, None], np.arange(P)[None, :]
    if adjacent:
        return i < j
    return (i + 1 < j) & ~((i == 0) & (j == P - 1))


def crossings64(C):
    """(the proper crossings of the closed curve C [P, 2] among the pairs the contract tests, whether every pair is decided at
    the fp32 margin)"""
    C = np.asarray(C, np.float64)
    P = len(C)
    a0, a1 = C[:, None, :], np.roll(C, -1, axis=0)[:, None, :]
    b0, b1 = C[None, :, :], np.roll(C, -1, axis=0)[None, :, :]
    dets = [_det(a0, a1, b0), _det(a0, a1, b1), _det(b0, b1, a0), _det(b0, b1, a1)]
    sure = [(np.abs(d) > m) | (m == 0) for d, m in dets]
    sgn = [np.sign(d) for d, _ in dets]
    opp1, opp2 = sgn[0] * sgn[1] < 0, sgn[2] * sgn[3] < 0
    s1, s2 = sure[0] & sure[1], sure[2] & sure[3]
    # an edge of no length gives the same two determinants (or zeros): never opposite, whatever the rounding
    flat = ((a0 == a1).all(-1) | (b0 == b1).all(-1))
    mask = _pair_mask(P)
    decided = flat | (s1 & ~opp1) | (s2 & ~opp2) | (s1 & s2)
    count = int((opp1 & opp2 & mask & ~flat).sum())
    return count, bool(decided[mask].all())


# ---- the float32 emulation of the header's operation order ----
def _height32(x0, h0, x1, h1, r, q):
    """item 3: u1 = min((q - x0) r, 1), u0 = min((x1 - q) r, 1), h = fma(u1, h1, u0 h0), cut to the edge's own heights"""
    with np.errstate(invalid="ignore", over="ignore"):
        u1 = np.fmin(_f32(_f32(q - x0) * r), 1.0)
        u0 = np.fmin(_f32(_f32(x1 - q) * r), 1.0)
        h = _fma(u1, h1, _f32(u0 * h0))
    return np.fmax(np.fmin(h0, h1), np.fmin(np.fmax(h0, h1), h))


def _recip32(dx):
    with np.errstate(divide="ignore"):
        return _f32(1.0 / dx)


def place32(T, params=None, wrong=None):
    """the template as the kernel places it (hausdorff_oracle.template32)"""
    return ho.template32(T, params, "R transposed" if wrong == "R transposed" else None)


def emulate32(C, T, params=None, wrong=None):
    """one row in the header's fp32 order (hint_overlap_desc items 1 - 7): C [P, 2] and T [M, 2] fp32 vertices, T placed by
    params first if given.  The double sums are numpy's (their association moves nothing a test can see).  dict of area_T,
    area_C, I, I_raw, iou, dice, crossings"""
    assert wrong is None or wrong in WRONG, wrong
    C = np.asarray(C, np.float32).astype(np.float64)
    T = place32(T, params, wrong)
    P, M = len(C), len(T)
    y0 = 0.0 if wrong == "baseline 0" else min(C[:, 1].min(), T[:, 1].min())
    keep_t = np.ones(M)
    if wrong == "closing edge dropped":
        keep_t[M - 1] = 0.0
    if wrong == "tile seam edge dropped":
        keep_t[TILE - 1::TILE] = 0.0
        keep_t[M - 1] = 1.0

    def edges(v):
        x0, y0_, x1, y1 = _edges(v)
        h0, h1 = _f32(y0_ - y0), _f32(y1 - y0)
        dx = _f32(x1 - x0)
        return x0, h0, x1, h1, dx, _recip32(dx)

    ex0, eh0, ex1, eh1, edx, er = edges(C)
    fx0, fh0, fx1, fh1, fdx, fr = edges(T)
    tc = _f32(_f32(0.5 * edx) * _f32(eh0 + eh1))
    tt = _f32(_f32(0.5 * fdx) * _f32(fh0 + fh1)) * keep_t
    ex0, eh0, ex1, eh1, er = (a[:, None] for a in (ex0, eh0, ex1, eh1, er))
    fx0, fh0, fx1, fh1, fr = (a[None, :] for a in (fx0, fh0, fx1, fh1, fr))
    a = np.maximum(np.minimum(ex0, ex1), np.minimum(fx0, fx1))
    b = np.minimum(np.maximum(ex0, ex1), np.maximum(fx0, fx1))
    live = a < b
    w = _f32(b - a)
    ea, eb = _height32(ex0, eh0, ex1, eh1, er, a), _height32(ex0, eh0, ex1, eh1, er, b)
    fa, fb = _height32(fx0, fh0, fx1, fh1, fr, a), _height32(fx0, fh0, fx1, fh1, fr, b)
    da, db = _f32(ea - fa), _f32(eb - fb)
    ma, mb = np.fmin(ea, fa), np.fmin(eb, fb)
    cross = ((da < 0) & (db > 0)) | ((da > 0) & (db < 0))
    if wrong == "no split at the crossing":
        cross = np.zeros_like(cross)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = _f32(da - db)
        ta, tb = _f32(da / den), _f32(-db / den)
        hc = _fma(ta, eb, _f32(tb * ea))
        split = _f32(hc + _fma(ta, ma, _f32(tb * mb)))
        v = _f32(_f32(0.5 * w) * np.where(cross, split, _f32(ma + mb)))
    sign = np.where((ex1 < ex0) != (fx1 < fx0), -1.0, 1.0)
    term = np.where(live, sign * v, 0.0) * keep_t[None, :]
    at, ac, raw = abs(tt.sum()), abs(tc.sum()), abs(term.sum())
    inter, iou, dice = _scores(at, ac, raw)
    if wrong == "IoU denominator without - I":
        iou = inter / (at + ac) if at + ac > 0 else float("nan")
    return dict(area_T=float(_f32(at)), area_C=float(_f32(ac)), I=float(_f32(inter)), I_raw=raw, raw_C=ac, raw_T=at,
                iou=float(_f32(iou)), dice=float(_f32(dice)), crossings=crossings32(C, wrong))


def crossings32(C, wrong=None):
    """item 7 in fp32: det = fma(ux, vy, -(uy vx)) of rounded differences, strict signs"""
    C = np.asarray(C, np.float64)
    P = len(C)
    a0, a1 = C[:, None, :], np.roll(C, -1, axis=0)[:, None, :]
    b0, b1 = C[None, :, :], np.roll(C, -1, axis=0)[None, :, :]

    def det(p, q, s):
        ux, uy = _f32(q[..., 0] - p[..., 0]), _f32(q[..., 1] - p[..., 1])
        vx, vy = _f32(s[..., 0] - p[..., 0]), _f32(s[..., 1] - p[..., 1])
        return _fma(ux, vy, -_f32(uy * vx))

    d1, d2, d3, d4 = det(a0, a1, b0), det(a0, a1, b1), det(b0, b1, a0), det(b0, b1, a1)
    if wrong == "adjacent pairs counted as crossings":
        return int(((d1 * d2 <= 0) & (d3 * d4 <= 0) & _pair_mask(P, adjacent=True)).sum())
    return int(((d1 * d2 < 0) & (d3 * d4 < 0) & _pair_mask(P)).sum())


# ---- the rules ----
def bounds(ref, c=C_TOL):
    """the bounds of one row's outputs from overlap64's dict: dict of area_T, area_C, I, iou, dice"""
    eI, eC, eT = c * U * ref["S"], c * U * ref["S_C"], c * U * ref["S_T"]
    eIc = max(eI, eC, eT)
    out = dict(area_T=eT + U * ref["area_T"], area_C=eC + U * ref["area_C"], I=eIc + U * ref["I"])
    at, ac, inter = ref["area_T"], ref["area_C"], ref["I"]
    d, ed = at + ac - inter, eC + eT + eIc
    out["iou"] = (eIc * d + inter * ed) / (d * (d - ed)) + U * ref["iou"] if d > ed else np.inf
    d, ed = at + ac, eC + eT
    out["dice"] = 2 * (eIc * d + inter * ed) / (d * (d - ed)) + U * ref["dice"] if d > ed else np.inf
    return out


def raw_shares(ref, em):
    """the emulation's (or a device's raw sums') error as a share of u S, u S_C, u S_T: what C_TOL is taken from"""
    return (abs(em["I_raw"] - ref["I_raw"]) / (U * ref["S"]) if ref["S"] > 0 else 0.0,
            abs(em["raw_C"] - ref["area_C"]) / (U * ref["S_C"]) if ref["S_C"] > 0 else 0.0,
            abs(em["raw_T"] - ref["area_T"]) / (U * ref["S_T"]) if ref["S_T"] > 0 else 0.0)


def ratio(ref, got, c=C_TOL):
    """error / bound, the worst over the outputs in `got` (a dict with any of area_T, area_C, I, iou, dice); inf for a value
    that is not finite where the oracle's is"""
    bd = bounds(ref, c)
    worst = 0.0
    for name, v in got.items():
        if name not in bd:
            continue
        want = ref[name]
        if np.isnan(want):
            worst = max(worst, 0.0 if np.isnan(v) else np.inf)
            continue
        err = abs(float(v) - want)
        worst = max(worst, err / bd[name] if bd[name] > 0 else (0.0 if err == 0 else np.inf))
        if not np.isfinite(v):
            worst = np.inf
    return worst


# ---- the ledger of cases (tests/test_overlap_cpu.py, tests/test_gpu_overlap.py) ----
def wobble_curves(seed, N, P, lobes=3):
    """[N, P, 2] fp32 given curves, not closed (the closing edge has a length): r = 1 + 0.3 cos(lobes th + phase), scaled,
    turned and moved at random; every other row runs clockwise"""
    rs = np.random.RandomState(seed)
    out = np.empty((N, P, 2), np.float32)
    for n in range(N):
        th = 2 * np.pi * (np.arange(P) + rs.uniform(0, 1)) / P
        if n % 2:
            th = -th
        r = rs.uniform(0.8, 1.6) * (1 + 0.3 * np.cos(lobes * th + rs.uniform(0, 6)))
        out[n] = np.stack([r * np.cos(th), r * np.sin(th)], 1) + 0.3 * rs.randn(2)
    return out


def polygon_template(M):
    """[M, 2] fp32: the analytic lens of lensfit_oracle at M >= 4 points, a triangle at 3"""
    if M == 3:
        return np.array([[-1.0, -0.7], [1.2, -0.4], [0.1, 1.1]], np.float32)
    return lfo.lens_prototype(M)


def ragged_templates(sizes):
    """(a_points [T, 2] fp32, offsets int64 [N + 1]): polygon_template of every size, one after the other"""
    parts = [polygon_template(m) for m in sizes]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def lens_case(seed=301, N=16, M=130):
    """the lens rows of the fit's fixtures: x [N, 20], the prototype [M, 2], params [N, 4]"""
    return lfo.lens_rows(seed, N), lfo.lens_prototype(M), lfo.golden_grad_params(seed, N)


def plus_case(seed=511, N=16, zero_width=(2,), clamped=(4,), angle=None):
    """the plus rows of the fit's fixtures: x [N, 100], params [N, 9] near the shapes (zero widths and acting clamps in the rows
    named); angle: None keeps the drawn angles, a number sets every row's"""
    x, base = pfo.plus_rows(seed, N)
    p = pfo.eval_params(base, seed + 7, zero_width, clamped)
    if angle is not None:
        p[:, 8] = angle
    return x, p


def plus_vertices32(params):
    """the twelve placed vertices [N, 12, 2] in the contract's fp32 order (plus_oracle's emulation)"""
    out = np.empty((len(params), 12, 2))
    for n, p in enumerate(np.asarray(params, np.float32)):
        out[n] = po.place32(po.local32(p), p)
    return out


def plus_vertices64(params):
    """the twelve placed vertices [N, 12, 2] in float64"""
    seg, _ = po.segments64(np.asarray(params, np.float64))
    return np.asarray(seg)[:, :, 0, :]


# name, curve source, P, template ("shared", M) / ("ragged", sizes) / ("plus",), rows, with params
LEDGER = (
    ("lens traced 100 x 130", "lens", 100, ("shared", 130), 16, True),
    ("plus traced 100, 511", "plus511", 100, ("plus",), 16, False),
    ("plus traced 100, 521", "plus521", 100, ("plus",), 6, False),
    ("given 3 x 3", "given", 3, ("shared", 3), 5, False),
    ("given 256 x 1024", "given", 256, ("shared", 1024), 3, True),
    ("given 257 x 1025", "given", 257, ("shared", 1025), 3, False),
    ("traced 1024 x 2049", "lens", 1024, ("shared", 2049), 2, True),
    ("given 100 x 4096", "given", 100, ("shared", 4096), 2, True),
    ("ragged 3..1500", "lens", 100, ("ragged", (3, 130, 1500, 1025, 17, 700, 3)), 7, True),
    ("given 100 x 130, far from the origin", "far", 100, ("shared", 130), 4, True),
)
FAR = (300.0, -1000.0)             # the last case's curves and placements are moved there: the baseline must follow


def ledger_case(name):
    """a ledger case's inputs: dict of curve (x [N, 4K] or points [N, P, 2], fp32), P, points32 [N, P, 2] (the fp32 emulation of
    the trace, or the given points), and a_points / offsets / params (any may be None) or plus_params"""
    row = {c[0]: c for c in LEDGER}[name]
    _, source, P, tmpl, N, with_params = row
    seed = 900 + [c[0] for c in LEDGER].index(name)
    out = dict(name=name, P=P, a_points=None, offsets=None, params=None, plus_params=None)
    if source in ("given", "far"):
        out["curve"] = wobble_curves(seed, N, P)
        if source == "far":
            out["curve"] = (out["curve"].astype(np.float64) + np.array(FAR)).astype(np.float32)
        out["points32"] = out["curve"].astype(np.float64)
    else:
        if source == "lens":
            x = lfo.lens_rows(301 if tmpl == ("shared", 130) else seed, N)
        else:
            x, pp = plus_case(511, 16) if source == "plus511" else plus_case(521, 6, zero_width=(1,), clamped=(3,))
            out["plus_params"] = pp
        out["curve"] = x
        out["points32"] = trace32(x, P)
    if tmpl[0] == "shared":
        out["a_points"] = polygon_template(tmpl[1])
    elif tmpl[0] == "ragged":
        out["a_points"], out["offsets"] = ragged_templates(tmpl[1])
    if with_params:
        out["params"] = lfo.golden_grad_params(301 if name.startswith("lens traced") else seed, N)
        if source == "far":
            out["params"][:, :2] = (0.2 * out["params"][:, :2] + np.array(FAR)).astype(np.float32)
    return out


def row_template32(case, n, wrong=None):
    """row n's placed template in the contract's fp32 order, as float64 [M, 2]"""
    if case["plus_params"] is not None:
        return plus_vertices32(case["plus_params"][n:n + 1])[0]
    a = ho.row_template(case["a_points"], case["offsets"], n)
    return place32(a, None if case["params"] is None else case["params"][n], wrong)


def row_emulate32(case, n, wrong=None):
    """emulate32 of row n of a ledger case"""
    if case["plus_params"] is not None:
        if wrong == "R transposed":
            p = np.array(case["plus_params"][n], np.float32)
            return emulate32(case["points32"][n], po.place32(po.local32(p), p, "R transposed"), None, None)
        return emulate32(case["points32"][n], row_template32(case, n), None, wrong)
    a = ho.row_template(case["a_points"], case["offsets"], n)
    return emulate32(case["points32"][n], a, None if case["params"] is None else case["params"][n], wrong)
