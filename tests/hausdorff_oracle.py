"""Float64 restatement of the curve-to-template distances (hint_amd.curves hausdorff_distances / chamfer_distances,
include/hint_amd.h hint_hausdorff_run) and the rule device results are compared by.  Written fresh from the contract; nothing of
the reference is used.  The curve's points come from tests/curve_oracle.py (points64, scale).

The contract, per row: B = the curve's P points (traced from x [4K], or given), A = the row's template points [M, 2], moved - if
params = (x, y, scale, angle) are given - to (A R) scale + (x, y) with row vectors and R = [[cos, sin], [-sin, cos]];
  mA_i = min_j |A_i - B_j|^2,  mB_j = min_i |A_i - B_j|^2
  max_h = sqrt(max of all M + P minima),  avg_h = mean of their M + P roots,  chamfer = (mean_j mB_j, mean_i mA_i)

The comparison rule.  u = 2^-24, S = curve_oracle.scale(x).  A device point is within
  delta_B = (2K + 2) u S                 of the float64 curve point (traced; 0 for given points), and within
  delta_A = 4 u (|scale| max_i (|a.x| + |a.y|) + max(|x|, |y|))     of the float64 template point (0 without params)
per coordinate-wise statement of hint_amd.h's operation order.  Min, max and mean are 1-Lipschitz in the sup norm, so
  |max_h - max_h64| <= E = 2 (delta_A + delta_B) + 4 u max_ij |a_i - b_j|      (two moved end points; sub, product, fma, root)
  |avg_h - avg_h64| <= E + u avg_h64                                            (the mean's own rounding)
  |chamfer - chamfer64| <= 2 max_h64 E + E^2   per component                    ((d + e)^2 - d^2 with d <= max_h64, |e| <= E)
"""
import numpy as np

import curve_oracle as co
from curve_oracle import _f32, _fma, trace32

U = 2.0 ** -24

# fixtures tests/golden/hausdorff_<name>.npz (tests/golden/make_hausdorff_golden.py): K = 5, curve_oracle.gauss(seed, rows, 5), the
# template lens_template(points), params drawn by golden_params
GOLDEN_CASES = (
    dict(name="lens_n64", seed=201, rows=64, points=130),
    dict(name="lens_n8", seed=202, rows=8, points=257),
)
GOLDEN_P = 1000            # the dense trace of run_experiments.py:148
GOLDEN_FIT_P = 100         # the points of the fit's loss (run_experiments.py:147)
GOLDEN_WEIGHTS = (1.0, 0.25)


def lens_template(M=130, R=1.5):
    """an analytic lens: the intersection of two discs of radius R whose rims cross at (+-1, 0) - two arcs, M points, fp32"""
    h = np.sqrt(R * R - 1.0)
    th0 = np.arctan2(h, 1.0)
    up, lo = M - M // 2, M // 2
    a = np.linspace(th0, np.pi - th0, up, endpoint=False)
    b = np.linspace(np.pi + th0, 2 * np.pi - th0, lo, endpoint=False)
    pts = np.concatenate([np.stack([R * np.cos(a), R * np.sin(a) - h], 1), np.stack([R * np.cos(b), R * np.sin(b) + h], 1)])
    return pts.astype(np.float32)


def golden_params(seed, N):
    """(x, y, scale, angle) per row: centres near 0, scales 0.5 .. 2.5, every angle"""
    rs = np.random.RandomState(seed + 1000)
    return np.stack([0.3 * rs.randn(N), 0.3 * rs.randn(N), rs.uniform(0.5, 2.5, N), rs.uniform(-np.pi, np.pi, N)], 1).astype(np.float32)


def template64(a, params=None):
    """the moved template [M, 2] in float64"""
    a = np.asarray(a, np.float64)
    if params is None:
        return a
    x, y, s, ang = (float(v) for v in np.asarray(params, np.float64))
    R = np.array([[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
    return (a @ R) * s + np.array([x, y])


def row64(a, b):
    """max_h, avg_h, (chamfer0, chamfer1) and the largest distance between a template and a curve point, of one row"""
    mA, mB, far = co.minima64(a, b)
    both = np.concatenate([mA, mB])
    return np.sqrt(both.max()), np.sqrt(both).mean(), (mB.mean(), mA.mean()), np.sqrt(far)


def row_template(a_points, offsets, n):
    return a_points if offsets is None else a_points[int(offsets[n]):int(offsets[n + 1])]


def distances64(curve, a_points, params=None, offsets=None, P=None):
    """dict of max_h [N], avg_h [N], chamfer [N, 2] in float64 and the rule's bounds E [N], e_avg [N], e_ch [N].  curve: x [N, 4K]
    (traced at P) or points [N, P, 2]"""
    curve = np.asarray(curve)
    traced = curve.ndim == 2
    N = curve.shape[0]
    b_all = co.points64(curve, P) if traced else np.asarray(curve, np.float64)
    dB = (2 * (curve.shape[1] // 4) + 2) * U * co.scale(curve) if traced else np.zeros(N)
    out = dict(max_h=np.empty(N), avg_h=np.empty(N), chamfer=np.empty((N, 2)), E=np.empty(N))
    for n in range(N):
        a32 = np.asarray(row_template(a_points, offsets, n), np.float64)
        pr = None if params is None else np.asarray(params[n], np.float64)
        a = template64(a32, pr)
        dA = 0.0 if pr is None else 4 * U * (abs(pr[2]) * np.abs(a32).sum(1).max() + max(abs(pr[0]), abs(pr[1])))
        mh, av, ch, far = row64(a, b_all[n])
        out["max_h"][n], out["avg_h"][n], out["chamfer"][n] = mh, av, ch
        out["E"][n] = 2 * (dA + dB[n]) + 4 * U * far
    out["e_avg"] = out["E"] + U * out["avg_h"]
    out["e_ch"] = 2 * out["max_h"] * out["E"] + out["E"] ** 2
    return out


def ratios(ref, max_h=None, avg_h=None, chamfer=None):
    """error / bound per row, the worst over the quantities given ([N]; inf where a value is not finite or a zero bound is missed)"""
    r = np.zeros(len(ref["E"]))
    for got, want, bound in ((max_h, ref["max_h"], ref["E"]), (avg_h, ref["avg_h"], ref["e_avg"]),
                             (None if chamfer is None else np.asarray(chamfer, np.float64)[:, 0], ref["chamfer"][:, 0], ref["e_ch"]),
                             (None if chamfer is None else np.asarray(chamfer, np.float64)[:, 1], ref["chamfer"][:, 1], ref["e_ch"])):
        if got is None:
            continue
        err = np.abs(np.asarray(got, np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        r = np.maximum(r, np.where(np.isfinite(q), q, np.inf))
    return r


def check(ref, max_h=None, avg_h=None, chamfer=None):
    """the comparison rule: (rows that fail it, the worst error / bound)"""
    r = ratios(ref, max_h, avg_h, chamfer)
    return np.nonzero(~(r <= 1.0))[0], float(r.max())


# ---- a float32 emulation of the contract's operation order (and deliberately wrong variants of it), for the CPU tests ----
def template32(a, pr, wrong=None):
    a = np.asarray(a, np.float32).astype(np.float64)
    if pr is None:
        return a
    x, y, sc, ang = (float(v) for v in np.asarray(pr, np.float32))
    cs, sn = float(np.float32(np.cos(ang))), float(np.float32(np.sin(ang)))
    if wrong == "R transposed":
        sn = -sn
    qx = _fma(-a[:, 1], sn, _f32(a[:, 0] * cs))
    qy = _fma(a[:, 1], cs, _f32(a[:, 0] * sn))
    if wrong == "scale after the translation":
        return np.stack([_f32(_f32(qx + x) * sc), _f32(_f32(qy + y) * sc)], 1)
    return np.stack([_fma(qx, sc, x), _fma(qy, sc, y)], 1)


WRONG = ("one direction only", "mean over M", "end point dropped", "R transposed", "scale after the translation",
         "neighbour's first point", "squares for roots")


def emulate32(curve, a_points, params=None, offsets=None, P=None, wrong=None):
    """(max_h [N], avg_h [N], chamfer [N, 2]) as fp32 values by the contract's operation order; wrong: one of WRONG"""
    assert wrong is None or wrong in WRONG
    curve = np.asarray(curve)
    b_all = trace32(curve, P) if curve.ndim == 2 else np.asarray(curve, np.float32).astype(np.float64)
    N = b_all.shape[0]
    max_h, avg_h, chamfer = np.empty(N, np.float32), np.empty(N, np.float32), np.empty((N, 2), np.float32)
    for n in range(N):
        a_row = row_template(a_points, offsets, n)
        if wrong == "neighbour's first point" and offsets is not None and int(offsets[n + 1]) < len(a_points):
            a_row = a_points[int(offsets[n]):int(offsets[n + 1]) + 1]
        a = template32(a_row, None if params is None else params[n], wrong)
        b = b_all[n][:-1] if wrong == "end point dropped" else b_all[n]
        mA, mB = co.minima32(a, b)
        both = mA if wrong == "one direction only" else np.concatenate([mA, mB])
        roots = both if wrong == "squares for roots" else _f32(np.sqrt(both))
        max_h[n] = roots.max()
        avg_h[n] = roots.sum() / (len(a) if wrong == "mean over M" else len(roots))
        chamfer[n] = (mB.sum() / len(mB), mA.sum() / len(mA))
    return max_h, avg_h, chamfer
