"""curve_features / lens_forward_process / target_distances / mean_target_distance: the lens-shape simulator of the reference's
evaluation loop on the kernel of hint_curve.hip.

    LensShapeModel.forward_process(x, noise=0.05)                      data.py:127-139 (over trace_fourier_curves, data.py:51-57)
    mean_target_distance(model, y_target, x)                           rejection_sampling.py:99-102, called at :204

are a Python loop over rows there - trace the Fourier curve at 100 points, build the 100 x 100 pdist / squareform matrix, take
its argmax - on the CPU, behind a device-to-host copy; here they are one launch of hint_curve_run (two with the mean) that
reads x once and writes y, the distances and their mean, with no host synchronisation.  x is [N, 4K] fp32 in the layout of
flatten_coeffs (data.py:30-40), K odd, 1 <= K <= 25.  The arithmetic and its order are fixed (include/hint_amd.h), so a row's
result does not depend on the batch and two runs agree bit for bit.  The reference draws its noise from numpy's global
generator; here eps is an argument, or torch.randn on the device.  No gradient is implemented and there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError

__all__ = ["curve_features", "lens_forward_process", "target_distances", "mean_target_distance"]

MAX_COEFFS = 25
MIN_POINTS, MAX_POINTS = 2, 128
MAX_ROWS = 1 << 30


def _check_x(x, who: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise HintAmdError(f"{who}: x must be a tensor (got {type(x).__name__})")
    if x.dim() != 2:
        raise HintAmdError(f"{who}: x must be 2-D [rows, 4 K coefficients] (got shape {tuple(x.shape)})")
    if not x.is_cuda:
        raise HintAmdError(f"{who}: x is on {x.device}; the simulator is a GPU kernel and there is no CPU fallback")
    if not x.is_floating_point():
        raise HintAmdError(f"{who}: x is {x.dtype}; expected a floating-point tensor")
    _check_shape(tuple(x.shape), who)
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():          # (copies only where needed)
        x = x.to(torch.float32).contiguous()
    return x


def _check_shape(shape, who: str) -> int:
    n, c = shape
    if n < 1 or n > MAX_ROWS:
        raise HintAmdError(f"{who}: x must hold 1..{MAX_ROWS} rows (got shape {shape})")
    if c % 4 != 0 or (c // 4) % 2 != 1 or c // 4 > MAX_COEFFS:
        raise HintAmdError(f"{who}: x must hold 4 K columns with K odd, 1..{MAX_COEFFS} (got shape {shape})")
    return c // 4


def _check_points(v, who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise HintAmdError(f"{who}: n_points must be an int (got {type(v).__name__})")
    if v < MIN_POINTS or v > MAX_POINTS:
        raise HintAmdError(f"{who}: n_points must be {MIN_POINTS}..{MAX_POINTS} (got {v})")
    return v


def _check_noise(v, who: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise HintAmdError(f"{who}: noise must be a number (got {type(v).__name__})")
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        raise HintAmdError(f"{who}: noise must be finite (got {v})")
    return v


def _check_target(target, n_rows: int, device, who: str) -> torch.Tensor:
    """[2], [1, 2], or - as the reference passes it (rejection_sampling.py:195, :101) - expanded to [N, 2], of which row 0 counts"""
    try:
        t = target if isinstance(target, torch.Tensor) else torch.as_tensor(target)
    except (TypeError, ValueError, RuntimeError) as e:
        raise HintAmdError(f"{who}: y_target must be a tensor or an array-like of 2 numbers: {e}") from e
    if tuple(t.shape) not in ((2,), (1, 2), (n_rows, 2)):
        raise HintAmdError(f"{who}: y_target must have shape [2], [1, 2] or [{n_rows}, 2] (got {tuple(t.shape)})")
    if t.dim() == 2:
        t = t[0]
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _check_eps(eps, x: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(eps, torch.Tensor):
        raise HintAmdError(f"{who}: eps must be a tensor (got {type(eps).__name__})")
    if tuple(eps.shape) != (x.shape[0], 2):
        raise HintAmdError(f"{who}: eps must have shape [{x.shape[0]}, 2] (got {tuple(eps.shape)})")
    if eps.device != x.device:
        raise HintAmdError(f"{who}: eps is on {eps.device} and x on {x.device}")
    return eps.detach().to(torch.float32).contiguous()


def _noise_args(x: torch.Tensor, noise, eps, generator, who: str):
    noise = _check_noise(noise, who)
    if eps is not None:
        return noise, _check_eps(eps, x, who)
    if noise == 0.0:
        return 0.0, None
    if generator is not None and not isinstance(generator, torch.Generator):
        raise HintAmdError(f"{who}: generator must be a torch.Generator (got {type(generator).__name__})")
    return noise, torch.randn(x.shape[0], 2, device=x.device, dtype=torch.float32, generator=generator)


def _run(x: torch.Tensor, n_points: int, eps: Optional[torch.Tensor] = None, noise: float = 0.0,
         target: Optional[torch.Tensor] = None, want_dist: bool = False, want_mean: bool = False, max_groups: int = 0):
    """one hint_curve_run on checked arguments: (y [N, 2], dist [N] or None, mean 0-dim or None)"""
    lib = _lib.load()
    n, c = x.shape
    with torch.cuda.device(x.device):
        y = torch.empty(n, 2, dtype=torch.float32, device=x.device)
        dist = torch.empty(n, dtype=torch.float32, device=x.device) if want_dist else None
        mean = torch.empty((), dtype=torch.float32, device=x.device) if want_mean else None
        desc = _lib.CurveDesc()
        desc.x, desc.n_rows, desc.n_coeffs, desc.n_points = x.data_ptr(), n, c // 4, n_points
        desc.eps, desc.noise = (eps.data_ptr() if eps is not None else None), noise
        desc.target = target.data_ptr() if target is not None else None
        desc.y = y.data_ptr()
        desc.dist = dist.data_ptr() if want_dist else None
        desc.mean = mean.data_ptr() if want_mean else None
        desc.max_groups = max_groups
        ws = None
        if want_mean:
            nbytes = lib.hint_curve_workspace_bytes(n, c // 4, n_points)
            if nbytes == 0:
                _lib.check(1, "hint_curve_workspace_bytes")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            desc.workspace, desc.workspace_bytes = ws.data_ptr(), nbytes
        st = lib.hint_curve_run(desc, torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(st, "hint_curve_run")
    return y, dist, mean


def curve_features(x: torch.Tensor, n_points: int = 100) -> torch.Tensor:
    """the simulator without noise: for each row of x [N, 4K] the vector between the two curve points farthest apart, as
    (dy, dx) - forward_process(x, noise=0) of the reference - [N, 2] fp32 on x's device"""
    who = "curve_features"
    x = _check_x(x, who)
    return _run(x, _check_points(n_points, who))[0]


def lens_forward_process(x: torch.Tensor, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                         generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """the reference's LensShapeModel.forward_process(x, noise): curve_features(x) + noise * eps, eps [N, 2] given or drawn with
    torch.randn on x's device (from generator, if one is given); noise = 0 without eps is curve_features"""
    who = "lens_forward_process"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise)[0]


def target_distances(x: torch.Tensor, y_target, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                     generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """|lens_forward_process(x, noise) - y_target| per row, [N] fp32"""
    who = "target_distances"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    t = _check_target(y_target, x.shape[0], x.device, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise, t, want_dist=True)[1]


def mean_target_distance(x: torch.Tensor, y_target, noise: float = 0.05, *, eps: Optional[torch.Tensor] = None,
                         generator: Optional[torch.Generator] = None, n_points: int = 100) -> torch.Tensor:
    """the reference's mean_target_distance(model, y_target, x) for the lens-shape model: the mean of target_distances, summed in
    double in a fixed order, a 0-dim fp32 tensor on x's device.  y_target may be [2], [1, 2] or, as the reference passes it,
    already expanded to [N, 2] (row 0 counts)"""
    who = "mean_target_distance"
    x = _check_x(x, who)
    n_points = _check_points(n_points, who)
    t = _check_target(y_target, x.shape[0], x.device, who)
    noise, eps = _noise_args(x, noise, eps, generator, who)
    return _run(x, n_points, eps, noise, t, want_mean=True)[2]
