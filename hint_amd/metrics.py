"""multi_mmd / MultiMMD: the sample-quality metric of the reference's evaluation loop on the fused kernels of hint_mmd.hip.

    multi_mmd(sample, gt_sample)                                       rejection_sampling.py:56-73, called at :135-213

costs three N x N GEMMs and about thirty passes over N x N temporaries there; here it is hint_mmd_run: four small launches,
no N x N matrix in memory, a bit-reproducible result.  MultiMMD keeps one ground-truth set and its YY term, for loops that score
many samples against it (compare_conditional: eight models per run).  No gradient is implemented and there is no CPU fallback.

    corrcoef(x), corr_mse(x, corr_true), CorrelationTarget                  run_experiments.py:212-221 (test_likelihood)

are np.corrcoef(x.T) and np.nanmean(np.square(corr - corr_true)) in double on the kernels of hint_corr.hip: the sample stays on
the device, numpy's NaN entries are kept, the result is bit-reproducible.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import _run_desc

__all__ = ["multi_mmd", "MultiMMD", "DEFAULT_WIDTHS_EXPONENTS", "mmd_jobs", "corrcoef", "corr_mse", "CorrelationTarget", "corr_jobs"]

DEFAULT_WIDTHS_EXPONENTS = ((0.5, 1), (0.2, 1), (0.2, 0.5))      # rejection_sampling.py:56
MAX_KERNELS = 8


def _check_kernels(widths_exponents) -> Tuple[Tuple[float, float], ...]:
    try:
        ks = tuple((float(C), float(a)) for C, a in widths_exponents)
    except (TypeError, ValueError) as e:
        raise HintAmdError(f"multi_mmd: widths_exponents must be a sequence of (width, exponent) pairs: {e}") from e
    if not 1 <= len(ks) <= MAX_KERNELS:
        raise HintAmdError(f"multi_mmd: widths_exponents must hold 1..{MAX_KERNELS} kernels (got {len(ks)})")
    for k, (C, a) in enumerate(ks):
        if not (C > 0 and math.isfinite(C)):
            raise HintAmdError(f"multi_mmd: width of kernel {k} must be positive and finite (got {C})")
        if not (a > 0 and math.isfinite(a)):
            raise HintAmdError(f"multi_mmd: exponent of kernel {k} must be positive and finite (got {a})")
    return ks


def _check_set(t, name: str, who: str = "multi_mmd") -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise HintAmdError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    if t.dim() != 2:
        raise HintAmdError(f"{who}: {name} must be 2-D [samples, features] (got shape {tuple(t.shape)})")
    if not t.is_cuda:
        raise HintAmdError(f"{who}: {name} is on {t.device}; the metric is a GPU kernel and there is no CPU fallback")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise HintAmdError(f"{who}: {name} is empty (shape {tuple(t.shape)})")
    if not t.is_floating_point():
        raise HintAmdError(f"{who}: {name} is {t.dtype}; expected a floating-point tensor")
    if t.requires_grad and torch.is_grad_enabled():
        raise HintAmdError(f"{who}: {name} requires grad, and no gradient of the metric is implemented; "
                           "call it under torch.no_grad() or detach the input")
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():         # (copies only where needed)
        t = t.to(torch.float32).contiguous()
    return t


def _check_pair(x: torch.Tensor, y: torch.Tensor):
    if x.device != y.device:
        raise HintAmdError(f"multi_mmd: x is on {x.device} and y on {y.device}")
    if x.shape[1] != y.shape[1]:
        raise HintAmdError(f"multi_mmd: x has {x.shape[1]} features and y has {y.shape[1]}")


def _run(x: torch.Tensor, y: torch.Tensor, ks, yy=None) -> torch.Tensor:
    """out = [MMD, mean XX, mean YY, mean XY] of checked fp32 sets on one device (yy: a device float, mean YY known)"""
    n_x, n_y, d = x.shape[0], y.shape[0], x.shape[1]
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    desc = _lib.MmdDesc()
    desc.x, desc.y, desc.n_x, desc.n_y, desc.d, desc.n_kernels = x.data_ptr(), y.data_ptr(), n_x, n_y, d, len(ks)
    for k, (C, a) in enumerate(ks):
        desc.width[k], desc.exponent[k] = C, a
    desc.yy = None if yy is None else yy.data_ptr()
    desc.out = out.data_ptr()
    _run_desc("hint_mmd_run", desc, x.device, (n_x, n_y, d))
    return out


def mmd_jobs(n_x: int, n_y: int, with_yy: bool = False):
    """the pair launch's work items, (kind, tile row, tile column, weight) each, and the tile edge T.  Host only."""
    lib = _lib.load()
    n = lib.hint_mmd_job(n_x, n_y, int(with_yy), -1, 0)
    _lib.check(1 if n < 0 else 0, "hint_mmd_job")
    T = lib.hint_mmd_job(n_x, n_y, int(with_yy), -1, 1)
    return [tuple(lib.hint_mmd_job(n_x, n_y, int(with_yy), j, f) for f in range(4)) for j in range(n)], T


def multi_mmd(x: torch.Tensor, y: torch.Tensor, widths_exponents: Sequence = DEFAULT_WIDTHS_EXPONENTS) -> torch.Tensor:
    """the reference's multi_mmd(x, y) (biased V-statistic, all pairs) as a 0-dim fp32 tensor on the inputs' device; sets of
    different sizes take each term's own mean"""
    ks = _check_kernels(widths_exponents)
    x, y = _check_set(x, "x"), _check_set(y, "y")
    _check_pair(x, y)
    return _run(x, y, ks)[0]


class MultiMMD:
    """multi_mmd against one ground-truth set y: mmd(x) returns multi_mmd(x, y) bit for bit, with the YY term computed once
    (when the object is made).  `terms` holds [mean XX, mean YY, mean XY] of the last call."""

    def __init__(self, y: torch.Tensor, widths_exponents: Sequence = DEFAULT_WIDTHS_EXPONENTS):
        self.kernels = _check_kernels(widths_exponents)
        self.y = _check_set(y, "y")
        # mean YY depends on y and the kernels alone (the common centre is y's mean): one row of y stands in for x
        first = _run(self.y[:1], self.y, self.kernels)
        self.yy = first[2:3].clone()
        self.terms = first[1:4]

    def mmd(self, x: torch.Tensor) -> torch.Tensor:
        x = _check_set(x, "x")
        _check_pair(x, self.y)
        out = _run(x, self.y, self.kernels, yy=self.yy)
        self.terms = out[1:4]
        return out[0]

    __call__ = mmd


# ---- correlation matrix / correlation MSE (hint_corr.hip): run_experiments.py:212-221 ----

def corr_jobs(n: int, d: int):
    """the Gram launch's work items, (slab, tile row, tile column, first row, rows) each, with the tile edge T, the rows per
    slab R and the slab count.  Host only."""
    lib = _lib.load()
    count = lib.hint_corr_job(n, d, -1, 0)
    _lib.check(1 if count < 0 else 0, "hint_corr_job")
    T, R, slabs = (lib.hint_corr_job(n, d, -1, f) for f in (1, 2, 3))
    return [tuple(lib.hint_corr_job(n, d, j, f) for f in range(5)) for j in range(count)], T, R, slabs


def _check_target(t, d: int, device, who: str) -> torch.Tensor:
    """corr_true as a contiguous float64 [d, d] tensor on `device` (fp32 -> fp64 is exact)"""
    if not isinstance(t, torch.Tensor):
        try:
            t = torch.as_tensor(t)
        except (TypeError, ValueError, RuntimeError) as e:
            raise HintAmdError(f"{who}: corr_true must be a tensor or an array (got {type(t).__name__})") from e
    if t.dtype not in (torch.float32, torch.float64):
        raise HintAmdError(f"{who}: corr_true is {t.dtype}; expected float32 or float64")
    if tuple(t.shape) != (d, d):
        raise HintAmdError(f"{who}: corr_true has shape {tuple(t.shape)}; x has {d} columns, so expected ({d}, {d})")
    return t.detach().to(device=device, dtype=torch.float64).contiguous()


def _corr_run(x: torch.Tensor, target, want_corr: bool):
    """(out[4], corr or None) of a checked fp32 x and a checked float64 target (or None) on x's device"""
    n, d = x.shape
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    corr = torch.empty((d, d), dtype=torch.float64, device=x.device) if want_corr else None
    desc = _lib.CorrDesc()
    desc.x, desc.n, desc.d = x.data_ptr(), n, d
    desc.target = None if target is None else target.data_ptr()
    desc.corr = None if corr is None else corr.data_ptr()
    desc.out = out.data_ptr()
    _run_desc("hint_corr_run", desc, x.device, (n, d))
    return out, corr


def corrcoef(x: torch.Tensor) -> torch.Tensor:
    """np.corrcoef(x.T) of a sample x [n, d] (rows are samples) as a float64 [d, d] tensor on x's device, numpy's NaNs included"""
    x = _check_set(x, "x", "corrcoef")
    return _corr_run(x, None, True)[1]


def corr_mse(x: torch.Tensor, corr_true) -> torch.Tensor:
    """np.nanmean(np.square(np.corrcoef(x.T) - corr_true)) as a 0-dim float64 tensor on x's device (run_experiments.py:212-221)"""
    x = _check_set(x, "x", "corr_mse")
    t = _check_target(corr_true, x.shape[1], x.device, "corr_mse")
    return _corr_run(x, t, False)[0][0]


class CorrelationTarget:
    """corr_mse against one ground-truth correlation matrix, kept on the device as float64: mse(x) returns corr_mse(x, corr_true)
    bit for bit.  `corr` is the last sample's matrix; `terms` holds [sum of squares, entries compared, NaN entries of corr] of the
    last call.  from_sample(x) takes corr_true from a ground-truth sample (rejection_sampling.py:105-132)."""

    def __init__(self, corr_true):
        if not isinstance(corr_true, torch.Tensor):
            corr_true = torch.as_tensor(corr_true)
        if corr_true.dim() != 2 or corr_true.shape[0] != corr_true.shape[1] or corr_true.shape[0] < 1:
            raise HintAmdError(f"CorrelationTarget: corr_true must be a square matrix (got shape {tuple(corr_true.shape)})")
        self._given = corr_true
        self.target = None          # float64 on the device of the first sample
        self.corr = None
        self.terms = None

    @classmethod
    def from_sample(cls, x: torch.Tensor) -> "CorrelationTarget":
        o = cls(corrcoef(x))
        o.target = o._given
        return o

    def mse(self, x: torch.Tensor) -> torch.Tensor:
        x = _check_set(x, "x", "CorrelationTarget.mse")
        if self.target is None or self.target.device != x.device or self.target.shape[0] != x.shape[1]:
            self.target = _check_target(self._given, x.shape[1], x.device, "CorrelationTarget.mse")
        out, self.corr = _corr_run(x, self.target, True)
        self.terms = out[1:4]
        return out[0]

    __call__ = mse
