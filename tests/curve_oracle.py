"""Float64 restatement of the lens-shape simulator (hint_amd.curves, include/hint_amd.h hint_curve_run) and the rule device
results are compared by.  Written fresh from the contract; nothing of the reference is used.  Everything is chunked over rows,
so that the [chunk, P (P - 1) / 2] pair arrays stay small.

The contract, for x [N, 4K] (x[:, :2K] real parts as [2 axes, K], x[:, 2K:] imaginary parts, frequency m = k - K//2):
  points    p[t, axis] = sum_k re[axis, k] cos(2 pi m t / (P - 1)) - im[axis, k] sin(2 pi m t / (P - 1)),  t = 0 .. P - 1
  D(i, j)   = |p_i - p_j|^2 for i < j; the chosen pair is the first maximum in row-major (i, j) order
  features  (p_j.y - p_i.y, p_j.x - p_i.x)  [+ noise * eps]
  dist      = |features - target|;  mean = sum(dist) / N

The comparison rule.  For a row let A = max over the two axes of sum_k (|re| + |im|) and u = 2^-24.  A point coordinate computed
in fp32 carries at most (2K + 2) u A of error (2K products, their sum, a rounded twiddle), hence D at most
tau = (8 sqrt(2) (2K + 2) + 12) u A^2.  The device's features must lie within (2 (2K + 2) + 1) u A per component of the float64
features of SOME pair whose float64 D is at least Dmax - 2 tau.  A row is unambiguous when that band holds one pair.
"""
import numpy as np

U = 2.0 ** -24
CHUNK = 256
GAUSS_W5 = np.array([.1, .3, 1, .6, .2])

# fixtures tests/golden/curve_<name>.npz (tests/golden/make_curve_golden.py): K = 5, P = 100, the unambiguous rows of gauss(seed, draw, 5)
GOLDEN_CASES = (
    dict(name="n512_features", seed=101, draw=640, rows=512, distance=False),
    dict(name="n300_distance", seed=102, draw=400, rows=300, distance=True),
    dict(name="n64_distance", seed=103, draw=100, rows=64, distance=True),
)


def gauss(seed, N, K):
    """the seeded Gaussian family: lens-like decay over the frequencies for K = 5, randn / 5 otherwise"""
    g = np.random.RandomState(seed).randn(N, 4 * K)
    if K == 5:
        return (g * np.tile(GAUSS_W5, 4)).astype(np.float32)
    return (g / 5).astype(np.float32)


def ellipse(a, b, K=5):
    """x(t) = a cos, y(t) = b sin: only the m = +1 coefficient is non-zero - real a on axis 0, imaginary -b on axis 1"""
    x = np.zeros((1, 4 * K), np.float32)
    k = K // 2 + 1
    x[0, k] = a                        # re[axis 0, m = +1]
    x[0, 2 * K + K + k] = -b           # im[axis 1, m = +1]
    return x


def twiddles(K, P):
    """cos, sin [P, K] in float64, the angle reduced exactly first"""
    m = np.arange(K) - K // 2
    t = np.arange(P)
    r = (np.abs(m)[None, :] * t[:, None]) % (P - 1)
    ang = 2.0 * np.pi * r / (P - 1)
    return np.cos(ang), np.sin(ang) * np.sign(m)[None, :]


def points64(x, P):
    """[n, P, 2] float64"""
    x = np.asarray(x, np.float64)
    n, C = x.shape
    K = C // 4
    re, im = x[:, :2 * K].reshape(n, 2, K), x[:, 2 * K:].reshape(n, 2, K)
    c, s = twiddles(K, P)
    return np.einsum("nak,tk->nta", re, c) - np.einsum("nak,tk->nta", im, s)


def scale(x):
    """A per row"""
    x = np.abs(np.asarray(x, np.float64))
    n, C = x.shape
    K = C // 4
    return (x[:, :2 * K].reshape(n, 2, K) + x[:, 2 * K:].reshape(n, 2, K)).sum(2).max(1)


def tau(x):
    K = x.shape[1] // 4
    return (8 * np.sqrt(2.0) * (2 * K + 2) + 12) * U * scale(x) ** 2


def feature_bound(x):
    K = x.shape[1] // 4
    return (2 * (2 * K + 2) + 1) * U * scale(x)


def _pairs(p):
    """all pairs i < j in row-major order of a chunk of points [c, P, 2]: D [c, pairs], features [c, pairs, 2]"""
    iu, ju = np.triu_indices(p.shape[1], 1)
    d = p[:, ju, :] - p[:, iu, :]                       # p_j - p_i
    return iu, ju, (d ** 2).sum(2), d[:, :, ::-1]       # features = (dy, dx)


def features64(x, P, chunk=CHUNK):
    """float64 features [N, 2], the chosen pair [N, 2] (i, j) and its D [N]"""
    x = np.asarray(x)
    N = x.shape[0]
    feat, pair, dmax = np.empty((N, 2)), np.empty((N, 2), np.int64), np.empty(N)
    for a in range(0, N, chunk):
        p = points64(x[a:a + chunk], P)
        iu, ju, D, f = _pairs(p)
        best = D.argmax(1)                              # the first maximum
        rows = np.arange(len(best))
        feat[a:a + chunk] = f[rows, best]
        pair[a:a + chunk, 0], pair[a:a + chunk, 1] = iu[best], ju[best]
        dmax[a:a + chunk] = D[rows, best]
    return feat, pair, dmax


def band_counts(x, P, chunk=CHUNK):
    """pairs within 2 tau of the maximum, per row"""
    x = np.asarray(x)
    out = np.empty(x.shape[0], np.int64)
    T = tau(x)
    for a in range(0, x.shape[0], chunk):
        _, _, D, _ = _pairs(points64(x[a:a + chunk], P))
        out[a:a + chunk] = (D >= (D.max(1) - 2 * T[a:a + chunk])[:, None]).sum(1)
    return out


def unambiguous(x, P, chunk=CHUNK):
    return band_counts(x, P, chunk) == 1


def band_check(x, y_dev, P, chunk=CHUNK):
    """the comparison rule: (rows that fail it, worst ratio of the nearest band pair's feature error to the feature bound).
    The ratio of a row is min over the band's pairs of (max component error / bound); a row fails when it is above 1 (or the
    device's value is not finite).  Rows of scale 0 (all points equal) must give exactly (0, 0)."""
    x, y_dev = np.asarray(x), np.asarray(y_dev, np.float64)
    assert y_dev.shape == (x.shape[0], 2)
    T, B = tau(x), feature_bound(x)
    ratio = np.empty(x.shape[0])
    for a in range(0, x.shape[0], chunk):
        _, _, D, f = _pairs(points64(x[a:a + chunk], P))
        t, b, yd = T[a:a + chunk], B[a:a + chunk], y_dev[a:a + chunk]
        band = D >= (D.max(1) - 2 * t)[:, None]
        err = np.abs(f - yd[:, None, :]).max(2)         # [c, pairs]
        err = np.where(band & np.isfinite(err), err, np.inf).min(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio[a:a + chunk] = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return np.nonzero(~(ratio <= 1.0))[0], float(ratio.max())


def distances64(y, target):
    return np.sqrt(((np.asarray(y, np.float64) - np.asarray(target, np.float64).reshape(1, 2)) ** 2).sum(1))


def golden_draw(case):
    """the rows a fixture was cut from: (gauss(seed, draw, 5), mask of its unambiguous rows)"""
    x = gauss(case["seed"], case["draw"], 5)
    return x, unambiguous(x, 100)


def golden_eps(case):
    """what numpy's global generator yields after np.random.seed(seed): the reference's noise for the distance fixtures"""
    return np.random.RandomState(case["seed"]).randn(case["rows"], 2)


# ---- what the oracles of the curve-to-point-set distances share (tests/hausdorff_oracle.py, tests/plus_oracle.py) ----
def minima64(a, b, chunk=512):
    """(mA [M], mB [P], the largest squared distance) of the [M, P] matrix of squared distances, in chunks of rows"""
    mA, mB, far = np.empty(len(a)), np.full(len(b), np.inf), 0.0
    for i in range(0, len(a), chunk):
        D = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(2)
        mA[i:i + chunk] = D.min(1)
        mB = np.minimum(mB, D.min(0))
        far = max(far, D.max())
    return mA, mB, far


# a float32 emulation of the contract's operation order, for the CPU tests
def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _fma(a, b, c):
    """fp32 fma of fp32 values held in float64: the product is exact in float64, the sum is rounded to 53 bits and then to 24"""
    return _f32(a * b + c)


def trace32(x, P):
    """[N, P, 2]: fp32 fma over k ascending, real term then imaginary term, twiddles rounded to fp32 after the exact reduction"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, K = x.shape[0], x.shape[1] // 4
    re, im = x[:, :2 * K].reshape(n, 2, K), x[:, 2 * K:].reshape(n, 2, K)
    c, s = twiddles(K, P)
    c, s = _f32(c), _f32(s)
    acc = np.zeros((n, P, 2))
    for k in range(K):
        acc = _fma(re[:, None, :, k], c[None, :, None, k], acc)
        acc = _fma(-im[:, None, :, k], s[None, :, None, k], acc)
    return acc


def minima32(a, b, chunk=512):
    """(mA [M], mB [P]) of D = fma(dy, dy, dx dx) in fp32, a - b, in chunks of rows"""
    mA, mB = np.empty(len(a)), np.full(len(b), np.inf)
    for i in range(0, len(a), chunk):
        dx, dy = _f32(a[i:i + chunk, None, 0] - b[None, :, 0]), _f32(a[i:i + chunk, None, 1] - b[None, :, 1])
        D = _fma(dy, dy, _f32(dx * dx))
        mA[i:i + chunk] = D.min(1)
        mB = np.minimum(mB, D.min(0))
    return mA, mB
