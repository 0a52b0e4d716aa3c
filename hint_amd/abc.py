"""nearest_rows / quantile_abc: the ground-truth posterior sample of the reference's evaluation loop on the kernels of hint_abc.hip.

    quantile_ABC(x, y, y_target, n=4000)                               rejection_sampling.py:88-96, called at :188

is a scipy distance_matrix of one target against 1e8 observations, a full np.argsort and a gather there, on the CPU; here it is
hint_abc_run - a radix select over the bit pattern of the squared distances, exact and bit-reproducible, with a workspace that
does not grow with N - plus one gather.  Rows are ordered by (D_i, i), D_i = sum_j (y_ij - t_j)^2 in fp32 (j ascending, fused
multiply-adds); a D_i that is not finite sorts last.  No gradient is implemented and there is no CPU fallback.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import _run_desc

__all__ = ["nearest_rows", "quantile_abc"]

MAX_K = 8192
MAX_NY = 32
MAX_ROWS = 1 << 30


def _check_y(y, who: str) -> torch.Tensor:
    if not isinstance(y, torch.Tensor):
        raise HintAmdError(f"{who}: y must be a tensor (got {type(y).__name__})")
    if y.dim() != 2:
        raise HintAmdError(f"{who}: y must be 2-D [observations, features] (got shape {tuple(y.shape)})")
    if not y.is_cuda:
        raise HintAmdError(f"{who}: y is on {y.device}; the selection is a GPU kernel and there is no CPU fallback")
    if not y.is_floating_point():
        raise HintAmdError(f"{who}: y is {y.dtype}; expected a floating-point tensor")
    if y.shape[0] < 1 or y.shape[0] > MAX_ROWS:
        raise HintAmdError(f"{who}: y must hold 1..{MAX_ROWS} rows (got shape {tuple(y.shape)})")
    if y.shape[1] < 1 or y.shape[1] > MAX_NY:
        raise HintAmdError(f"{who}: y must hold 1..{MAX_NY} features (got shape {tuple(y.shape)})")
    y = y.detach()
    if y.dtype != torch.float32 or not y.is_contiguous():          # (copies only where needed)
        y = y.to(torch.float32).contiguous()
    return y


def _check_target(target, y: torch.Tensor, who: str, name: str) -> torch.Tensor:
    try:
        t = target if isinstance(target, torch.Tensor) else torch.as_tensor(target)
    except (TypeError, ValueError, RuntimeError) as e:
        raise HintAmdError(f"{who}: {name} must be a tensor or an array-like of {y.shape[1]} numbers: {e}") from e
    ny = y.shape[1]
    if tuple(t.shape) not in ((ny,), (1, ny)):
        raise HintAmdError(f"{who}: {name} must have shape [{ny}] or [1, {ny}] (got {tuple(t.shape)})")
    return t.detach().to(device=y.device, dtype=torch.float32).contiguous().reshape(ny)


def _check_count(v, who: str, name: str, least: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise HintAmdError(f"{who}: {name} must be an int (got {type(v).__name__})")
    if v < least:
        raise HintAmdError(f"{who}: {name} must be >= {least} (got {v})")
    return v


def _run(y: torch.Tensor, t: torch.Tensor, k: int):
    n, ny = y.shape
    idx = torch.empty(k, dtype=torch.int32, device=y.device)
    dist = torch.empty(k, dtype=torch.float32, device=y.device)
    desc = _lib.AbcDesc()
    desc.y, desc.target, desc.n_rows, desc.ny, desc.k = y.data_ptr(), t.data_ptr(), n, ny, k
    desc.idx, desc.dist = idx.data_ptr(), dist.data_ptr()
    _run_desc("hint_abc_run", desc, y.device, (n, ny, k))
    return idx, dist


def nearest_rows(y: torch.Tensor, target, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the k rows of y [N, ny] nearest to target ([ny] or [1, ny]): (idx int64 [k], dist fp32 [k]) on y's device, ascending in
    (distance, row number); exact, and the same bits on every run"""
    who = "nearest_rows"
    y = _check_y(y, who)
    t = _check_target(target, y, who, "target")
    k = _check_count(k, who, "k", 1)
    if k > min(y.shape[0], MAX_K):
        raise HintAmdError(f"{who}: k must be 1..min(len(y), {MAX_K}) (got {k} with {y.shape[0]} rows)")
    idx, dist = _run(y, t, k)
    return idx.to(torch.int64), dist


def quantile_abc(x, y: torch.Tensor, y_target, n: int = 4000, skip: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """the reference's quantile_ABC(x, y, y_target, n): (sample [n, dx], threshold).  The sample is x at ranks skip .. skip + n - 1
    of the order, ascending in distance, on x's device (x: a tensor on the device or on the host); the default skip = 1 drops the
    nearest row as the reference's np.argsort(d)[1:] does.  threshold = the distance of rank skip + n, a 0-dim fp32 tensor."""
    who = "quantile_abc"
    y = _check_y(y, who)
    t = _check_target(y_target, y, who, "y_target")
    n = _check_count(n, who, "n", 1)
    skip = _check_count(skip, who, "skip", 0)
    if not isinstance(x, torch.Tensor):
        raise HintAmdError(f"{who}: x must be a tensor (got {type(x).__name__})")
    if x.dim() < 1 or x.shape[0] != y.shape[0]:
        raise HintAmdError(f"{who}: x has {x.shape[0] if x.dim() else 0} rows and y has {y.shape[0]}")
    k = skip + n + 1
    if y.shape[0] < k:
        raise HintAmdError(f"{who}: y holds {y.shape[0]} rows; skip + n + 1 = {k} are needed")
    if k > MAX_K:
        raise HintAmdError(f"{who}: skip + n + 1 = {k} is above the limit of {MAX_K} rows")
    idx, dist = _run(y, t, k)
    pick = idx[skip:skip + n].to(device=x.device, dtype=torch.int64)
    return x.detach().index_select(0, pick), dist[skip + n]
