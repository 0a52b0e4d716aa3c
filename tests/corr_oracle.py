"""Test-side evaluation of the correlation matrix and the correlation MSE (run_experiments.py:212-221 of the reference), written
fresh: the float64 statement - the three numpy calls - and a higher-precision evaluation in np.longdouble (80-bit extended on
x86-64; the module refuses to import where long double is no wider than that, instead of degrading to float64).

Tolerance of a device result, per entry of the matrix (bounds):
    |got - longdouble| <= max(4 e64, (R + slabs + 16) 2^-52)
  e64   |np.corrcoef - longdouble| on the same input: the reference's own error (about 5e-16 on the test inputs)
  R, slabs   rows per slab and slab count of the run (hint_corr_job).  An entry's sum S_ij is `slabs` chains of R double fused
        multiply-adds plus the sum of the slabs: to first order its error is at most (R + slabs) 2^-53 sum |u_i u_j|, and
        sum |u_i u_j| <= sqrt(S_ii S_jj) (Cauchy-Schwarz), which is the divisor - so (R + slabs) 2^-53 absolute on r.  The same
        holds for S_ii and S_jj under their square roots (half each); centring, the two roots, the product and the division add
        a few units of 2^-53 more: 16 covers them, and the whole is doubled for room.
and for the MSE, mean of (r - t)^2:   2 max|r - t| max(entry bound) + 2^-50 mse   (the derivative of a square, and the rounding of
the sum and the division).
"""
import warnings

import numpy as np

assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is not wider than float64 here: the oracle would check nothing"

GOLDEN_CASES = [dict(name="n4000_d20", n=4000, d=20, seed=4020), dict(name="n333_d100", n=333, d=100, seed=3433)]


def golden_inputs(case):
    """x = z A + b (dense mixing, fp32) and a second sample of a nearby model, whose corrcoef is the case's corr_true"""
    rs = np.random.RandomState(case["seed"])
    n, d = case["n"], case["d"]
    A = rs.standard_normal((d, d)) / np.sqrt(d) + 0.5 * np.eye(d)
    b = rs.standard_normal(d)
    x = (rs.standard_normal((n, d)) @ A + b).astype(np.float32)
    A2 = A + 0.1 * rs.standard_normal((d, d)) / np.sqrt(d)
    y = (rs.standard_normal((n, d)) @ A2 + b).astype(np.float32)
    return x, y


def checksum(arrays):
    return float(sum(np.abs(a.astype(np.float64)).sum() + (a.astype(np.float64) * np.arange(1, a.size + 1).reshape(a.shape)
                                                           ).sum() / a.size for a in arrays))


def corrcoef64(x):
    """np.corrcoef(x.T) as the reference calls it (float64 [d, d]; numpy returns a scalar for d = 1)"""
    x = np.asarray(x)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.asarray(np.corrcoef(x.astype(np.float64).T), dtype=np.float64).reshape(x.shape[1], x.shape[1])


def mse64(corr, corr_true):
    """np.nanmean(np.square(corr - corr_true)) (NaN when every difference is NaN)"""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return float(np.nanmean(np.square(np.asarray(corr, dtype=np.float64) - np.asarray(corr_true, dtype=np.float64))))


def corrcoef_ld(x):
    """the same matrix in np.longdouble from the fp32 input (exact conversion): centre, Gram, normalise, clip"""
    xl = np.asarray(x).astype(np.longdouble)
    n, d = xl.shape
    with np.errstate(all="ignore"):
        u = xl - xl.sum(axis=0) / np.longdouble(n)
        S = np.empty((d, d), dtype=np.longdouble)
        for i in range(d):                                  # (column by column: no [n, d, d] temporary)
            S[i, i:] = (u[:, i:] * u[:, i:i + 1]).sum(axis=0)
            S[i:, i] = S[i, i:]
        sd = np.sqrt(np.diag(S))
        r = S / (sd[:, None] * sd[None, :])
        return np.clip(r, np.longdouble(-1), np.longdouble(1))


def mse_ld(corr_ld, corr_true):
    df = corr_ld - np.asarray(corr_true).astype(np.longdouble)
    ok = ~np.isnan(df)
    return float((df[ok] * df[ok]).sum() / np.longdouble(ok.sum())) if ok.any() else float("nan")


def geometry(n, d):
    """(T, R, slabs) of a run on [n, d], from the library's own job table"""
    from hint_amd import _lib
    lib = _lib.load()
    T, R, slabs = (int(lib.hint_corr_job(n, d, -1, f)) for f in (1, 2, 3))
    assert T > 0 and R > 0 and slabs > 0, (lib.hint_last_error() or b"").decode()
    return T, R, slabs


def bounds(x):
    """-> (corr64, corr_ld, e64, bound): numpy's matrix, the longdouble one, numpy's error and the per-entry bound (NaN where the
    entry is NaN)"""
    x = np.asarray(x)
    _, R, slabs = geometry(*x.shape)
    c64, cl = corrcoef64(x), corrcoef_ld(x)
    with np.errstate(all="ignore"):
        e64 = np.abs(c64.astype(np.longdouble) - cl).astype(np.float64)
        bound = np.fmax(4.0 * e64, (R + slabs + 16) * 2.0 ** -52)
    bound[np.isnan(c64)] = np.nan
    return c64, cl, e64, bound


def mse_bound(corr_ld, corr_true, bound, mse):
    """2 max|r - t| max(entry bound) + 2^-50 mse over the entries that are compared (0 when none is)"""
    df = np.abs(corr_ld - np.asarray(corr_true).astype(np.longdouble))
    ok = ~np.isnan(df)
    if not ok.any():
        return 0.0
    return float(2.0 * df[ok].max() * np.nanmax(bound[ok]) + 2.0 ** -50 * mse)
