"""Test-side float64 evaluation of the ABC selection (hint_amd.nearest_rows / quantile_abc), written from the definition:

    D64   = ((y64 - t64)^2).sum(1), summed over j = 0, 1, .., ny - 1;  a D64 that is not finite counts as +inf
    order = np.lexsort((arange(N), D64))            rows by (D, row number)

The kernel evaluates D in fp32 (j ascending, the first term a rounded product, then fused multiply-adds), so on random data it is
compared through `check_rule`; where fp32 arithmetic is exact (small integers) the order itself must agree.  The fixtures' inputs
(tests/golden/abc_*.npz) are regenerated from their seeds by golden_inputs; the random GPU cases by random_inputs.
"""
import numpy as np

# (N, ny, n): what the reference's quantile_ABC was run on (tests/golden/make_abc_golden.py)
GOLDEN_CASES = [dict(name=f"n{N}_ny{ny}_n{n}", N=N, ny=ny, n=n, seed=2000 + 13 * N + ny)
                for N, ny, n in ((5000, 2, 100), (4099, 1, 64), (8200, 4, 333), (70000, 2, 4000), (3000, 5, 2998))]
GOLDEN_DX = 3


def golden_inputs(case):
    """y ~ N(0, 1) [N, ny], y_target ~ N(0, 1) [1, ny], x ~ N(0, 1) [N, 3] with the row number in its last column (fp32)"""
    rs = np.random.RandomState(case["seed"])
    y = rs.standard_normal((case["N"], case["ny"])).astype(np.float32)
    t = rs.standard_normal((1, case["ny"])).astype(np.float32)
    x = rs.standard_normal((case["N"], GOLDEN_DX)).astype(np.float32)
    x[:, -1] = np.arange(case["N"], dtype=np.float32)
    return x, y, t


def random_inputs(N, ny, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((N, ny)).astype(np.float32), rs.standard_normal(ny).astype(np.float32)


def checksum(arrays):
    return float(sum(np.abs(a.astype(np.float64)).sum() + (a.astype(np.float64) * np.arange(1, a.size + 1).reshape(a.shape)
                                                           ).sum() / a.size for a in arrays))


def distances64(y, t):
    """D64 [N]: squared distances in float64, +inf where the sum is not finite"""
    y64 = np.asarray(y, dtype=np.float64)
    t64 = np.asarray(t, dtype=np.float64).reshape(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        D = ((y64 - t64) ** 2).sum(1)
    D[~np.isfinite(D)] = np.inf
    return D


def _fma32(d, acc):
    """fp32 fma(d, d, acc), correctly rounded: d (an fp32 value held in float64) squares exactly in float64; the sum is rounded to
    odd there (its error from the two-sum identity), so the second rounding, to fp32, lands where a single one would"""
    p, a = d * d, acc.astype(np.float64)
    s = p + a
    v = s - p
    err = (p - (s - v)) + (a - v)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def distances32(y, t):
    """D [N] as the kernel defines it: fp32, j ascending, the first term a rounded product, then fused multiply-adds, every
    operation rounded once; +inf where it is not finite"""
    y = np.asarray(y, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.zeros(y.shape[0], dtype=np.float32)
        for j in range(y.shape[1]):
            D = _fma32((y[:, j] - t[j]).astype(np.float64), D)
    D[~np.isfinite(D)] = np.inf
    return D


def order64(y, t):
    """(D64, order): order = rows by (D64, row number)"""
    D = distances64(y, t)
    return D, np.lexsort((np.arange(D.shape[0]), D))


def eps_rule(ny):
    """twice the fp32 evaluation's worst relative error of D: one rounding for the difference, two for the square, ny - 1 for the sum"""
    return (ny + 2) * 2.0 ** -23


def band_count(D, order, k, ny):
    """rows with |D64 - B| <= eps B other than the boundary row itself, B = D64 at rank k - 1"""
    B = D[order[k - 1]]
    eps = eps_rule(ny)
    return int((np.abs(D - B) <= eps * B).sum()) - 1


def check_rule(y, t, k, idx, dist):
    """the comparison rule for random data; idx, dist: the k results as numpy arrays.  Returns the band count."""
    ny = y.shape[1]
    D, order = order64(y, t)
    N = D.shape[0]
    eps = eps_rule(ny)
    B = D[order[k - 1]]
    band = band_count(D, order, k, ny)
    print(f"N {N} ny {ny} k {k}: B {B:.9g}, rows in the band {band}")
    assert band <= 0.01 * k, f"badly chosen input: {band} rows within eps of rank k - 1 (k = {k})"
    idx = np.asarray(idx, dtype=np.int64)
    dist = np.asarray(dist)
    assert idx.shape == (k,) and dist.shape == (k,) and dist.dtype == np.float32
    assert idx.min() >= 0 and idx.max() < N and np.unique(idx).size == k, "indices out of range or repeated"
    assert (D[idx] <= B * (1.0 + eps)).all(), "a returned row is farther than rank k - 1 allows"
    must = np.nonzero(D < B * (1.0 - eps))[0]
    missing = np.setdiff1d(must, idx)
    assert missing.size == 0, f"{missing.size} rows nearer than rank k - 1 were not returned, e.g. {missing[:5]}"
    want = np.sqrt(D[idx])
    err = np.abs(dist.astype(np.float64) - want)
    tol = (ny + 4) * 2.0 ** -23 * want
    worst = float((err / np.maximum(want, 1e-300)).max())
    print(f"  worst relative dist error {worst:.3g} (bound {(ny + 4) * 2.0 ** -23:.3g})")
    assert (err <= tol).all(), f"dist off by {worst:.3g} relative"
    step = np.diff(dist.astype(np.float64))
    assert (step >= 0).all(), "dist decreases"
    # sqrt maps neighbouring fp32 values of D to one dist, so rows of equal dist may differ in D: they are in (D, row number) order
    D32 = distances32(y, t)[idx].astype(np.float64)
    same, dD = step == 0, np.diff(D32)
    assert ((dD[same] > 0) | ((dD[same] == 0) & (np.diff(idx)[same] > 0))).all(), "rows of equal dist are not in (D, row number) order"
    return band


def ulps_apart(a, b):
    """largest distance in units of the last place between two fp32 arrays of non-negative numbers (inf == inf is 0)"""
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


# the grid is full here and a workgroup owns more than 4096 rows: three turns of the histogram loop (256 x 8 rows each) and two
# tiles of the compaction pass (256 x 16), the last of each partial (asserted through hint_abc_geometry by the GPU tests)
BIG_N = 5500003


def random_cases(R, G):
    """(N, ny, k, seed) of the GPU tests' seeded N(0, 1) cases; R: rows per workgroup at small N, G: the largest grid.
    Every ny in {1, 2, 3, 4, 5, 7, 32}; N around 64, around R, 3 R + 17, the smallest N that uses all G workgroups (+ 1), and BIG_N;
    k in {1, 2, N - 1, N, 4002, 8192} where N allows."""
    full = (G - 1) * R + 1
    cases = [(3 * R + 17, ny, 100) for ny in (1, 2, 3, 4, 5, 7, 32)]
    for N in (1, 63, 64, 65):
        cases += [(N, 2, k) for k in sorted({1, 2, N - 1, N}) if 1 <= k <= N]
    for N in (R - 1, R, R + 1):
        cases += [(N, 3, k) for k in (1, N - 1, N)]
    cases += [(3 * R + 17, 2, k) for k in (2, 4002, 3 * R + 16, 3 * R + 17)]
    cases += [(4 * R + 1, 2, 8192), (4 * R + 1, 5, 8192)]
    cases += [(full, 2, 4002), (full + 1, 2, 4002), (full + 1, 3, 1)]
    cases += [(BIG_N, 2, 4002)]                     # rows per workgroup above 4096: every streaming loop takes several turns
    return [(N, ny, k, 3000 + i) for i, (N, ny, k) in enumerate(cases)]
