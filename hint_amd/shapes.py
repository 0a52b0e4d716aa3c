"""The lens-shape prior sampler and points -> Fourier coefficients on the device (hint_amd/csrc/hint_shapegen.hip): what feeds the
evaluation pipeline.

    sample_lens_prior(n, seed)             LensShapeModel.sample_prior(n)                   data.py:102-111
    sample_lens_joint(n, seed, noise)      LensShapeModel.sample_joint(n)                   data.py:113-125
    lens_rings(draws)                      generate_lens_shape's centred ring               data.py:85-100
    lens_draws(n, seed)                    the four draws of each row, (u_r, u_t, n_x, n_y)
    fourier_coeffs(points, n_coeffs)       flatten_coeffs(fourier_coeffs(points, n_coeffs)) data.py:42-49, :30-33

The lens is the intersection of two regular 64-gons in closed form (include/hint_amd.h hint_lensgen_desc states every step); no
polygon library is involved, and THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION - clockwise from the crossing point
where the boundary passes onto the first circle - because the reference takes whatever its polygon library returns.  Rows are a
function of (seed, offset + i) alone (Philox4x32-10): a prior of 1e8 rows drawn in chunks at any boundaries has the bits of one call.
One launch per call, nothing goes to the host, no autograd.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import MAX_SAMPLE_ROWS, _check_draws, _check_no_grad, _check_real, _outputs, _rejected, _run_desc, _sample_args
from .curves import lens_forward_process

__all__ = ["sample_lens_prior", "sample_lens_joint", "lens_rings", "lens_draws", "fourier_coeffs"]

MAX_ROWS = MAX_SAMPLE_ROWS
RING_POINTS = 32
MAX_COEFFS = 25
MAX_POINTS = 1024
MAX_POINT_ROWS = 1 << 24
_F32, _I32 = torch.float32, torch.int32
_DRAWS = ("u_r", "u_t", "n_x", "n_y")
_LENS_TABLE = lambda n: dict(x=((n, 20), _F32), ring=((n, RING_POINTS, 2), _F32), counts=((n,), _I32), eps=((n, 2), _F32),  # noqa: E731
                             draws_out=((n, 4), _F32))


def _lens_run(n: int, seed: int, offset: int, dev: torch.device, draws: Optional[torch.Tensor], want, out=None,
              max_groups: int = 0, who: str = "hint_lensgen_run"):
    """one hint_lensgen_run on checked arguments: the outputs named in `want` as a dict (`out`: the tests' guarded buffers)"""
    desc = _lib.LensGenDesc()
    desc.n_rows, desc.seed, desc.offset, desc.max_groups = n, seed, offset, max_groups
    desc.draws = draws.data_ptr() if draws is not None else None
    res = _outputs(desc, _LENS_TABLE(n), want, out, dev)
    ws = _run_desc("hint_lensgen_run", desc, dev, (n,), out)
    if draws is not None:
        _rejected(ws[:desc.workspace_bytes], "u_r or u_t outside [0, 1], or a draw that is not finite", who)
    res["workspace"] = ws
    return res


def sample_lens_prior(n: int, seed: int, *, offset: int = 0, device=None, draws: Optional[torch.Tensor] = None,
                      return_ring: bool = False):
    """the reference's LensShapeModel.sample_prior(n): x [n, 20] fp32 on the device, row i a function of (seed, offset + i) alone.
    draws [n, 4] = (u_r, u_t, n_x, n_y) replaces the Philox stream (seed and offset then go unused; the rows are checked, which
    reads one number back).  return_ring: (x, ring [n, 32, 2], counts [n]) - the closed, centred, zero-padded ring x is made of"""
    who = "sample_lens_prior"
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who, _DRAWS)
    res = _lens_run(n, seed, offset, dev, draws, ["x", "ring", "counts"] if return_ring else ["x"], who=who)
    return (res["x"], res["ring"], res["counts"]) if return_ring else res["x"]


def sample_lens_joint(n: int, seed: int, noise: float = 0.05, *, offset: int = 0, device=None,
                      draws: Optional[torch.Tensor] = None, return_eps: bool = False):
    """the reference's LensShapeModel.sample_joint(n): (x [n, 20], y [n, 2]) with y = lens_forward_process(x, noise, eps=eps), eps
    the stream-1 draws of (seed, offset + i).  return_eps: (x, y, eps)"""
    who = "sample_lens_joint"
    noise = _check_real(noise, "noise", who, nonneg=False)
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who, _DRAWS)
    res = _lens_run(n, seed, offset, dev, draws, ["x", "eps"], who=who)
    y = lens_forward_process(res["x"], noise, eps=res["eps"])
    return (res["x"], y, res["eps"]) if return_eps else (res["x"], y)


def lens_rings(draws: torch.Tensor):
    """(ring [n, 32, 2], counts [n] int32) of draws [n, 4]: the closed ring of each lens, centred and noised as generate_lens_shape
    returns it, zero-padded behind its 31 or 32 points; fourier_coeffs(ring, 5, counts) is sample_lens_prior's x up to rounding"""
    who = "lens_rings"
    draws = _check_draws(draws, None, who, _DRAWS)
    res = _lens_run(draws.shape[0], 0, 0, draws.device, draws, ["x", "ring", "counts"], who=who)
    return res["ring"], res["counts"]


def lens_draws(n: int, seed: int, *, offset: int = 0, device=None) -> torch.Tensor:
    """the draws sample_lens_prior(n, seed, offset=offset) uses, [n, 4] = (u_r, u_t, n_x, n_y)"""
    who = "lens_draws"
    n, seed, offset, dev, _ = _sample_args(n, seed, offset, device, None, who, _DRAWS)
    return _lens_run(n, seed, offset, dev, None, ["x", "draws_out"], who=who)["draws_out"]


def _fcoef_run(points: torch.Tensor, n_coeffs: int, counts: Optional[torch.Tensor], out=None, max_groups: int = 0,
               who: str = "hint_fcoef_run"):
    n, p = points.shape[0], points.shape[1]
    dev = points.device
    desc = _lib.FcoefDesc()
    desc.points, desc.counts = points.data_ptr(), (counts.data_ptr() if counts is not None else None)
    desc.n_rows, desc.p_max, desc.n_coeffs, desc.max_groups = n, p, n_coeffs, max_groups
    res = _outputs(desc, dict(x=((n, 4 * n_coeffs), _F32)), ["x"], out, dev)
    ws = _run_desc("hint_fcoef_run", desc, dev, (n, p, n_coeffs), out)
    if counts is not None:
        _rejected(ws[:desc.workspace_bytes], f"every count must be n_coeffs..{p}", who)
    return res["x"]


def fourier_coeffs(points: torch.Tensor, n_coeffs: int, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the reference's flatten_coeffs(fourier_coeffs(points[i, :counts[i]], n_coeffs)) of every row: points [N, P, 2] on the GPU,
    counts [N] integers or None (every row has P points) -> [N, 4 n_coeffs] fp32, the layout trace_fourier_curves reads.  n_coeffs
    is odd, at most 25, and n_coeffs <= counts[i] <= P <= 1024 (a smaller count would narrow the reference's output; it is
    refused, which reads one number back when counts is given)"""
    who = "fourier_coeffs"
    if not isinstance(points, torch.Tensor):
        raise HintAmdError(f"{who}: points must be a tensor (got {type(points).__name__})")
    if points.dim() != 3 or points.shape[2] != 2:
        raise HintAmdError(f"{who}: points must be [N, P, 2] (got shape {tuple(points.shape)})")
    if not points.is_cuda:
        raise HintAmdError(f"{who}: points is on {points.device}; the transform is a GPU kernel and there is no CPU fallback")
    if not points.is_floating_point():
        raise HintAmdError(f"{who}: points is {points.dtype}; expected a floating-point tensor")
    _check_no_grad(points, "points", who)
    if isinstance(n_coeffs, bool) or not isinstance(n_coeffs, int) or n_coeffs < 1 or n_coeffs > MAX_COEFFS or n_coeffs % 2 == 0:
        raise HintAmdError(f"{who}: n_coeffs must be an odd int, 1..{MAX_COEFFS} (got {n_coeffs!r})")
    n, p = points.shape[0], points.shape[1]
    if n < 1 or n > MAX_POINT_ROWS:
        raise HintAmdError(f"{who}: points must hold 1..{MAX_POINT_ROWS} rows (got shape {tuple(points.shape)})")
    if p < n_coeffs or p > MAX_POINTS:
        raise HintAmdError(f"{who}: points must hold n_coeffs = {n_coeffs}..{MAX_POINTS} points a row (got shape {tuple(points.shape)})")
    points = points.detach()
    if points.dtype != torch.float32 or not points.is_contiguous():
        points = points.to(torch.float32).contiguous()
    if counts is not None:
        if not isinstance(counts, torch.Tensor):
            raise HintAmdError(f"{who}: counts must be a tensor (got {type(counts).__name__})")
        if tuple(counts.shape) != (n,):
            raise HintAmdError(f"{who}: counts must have shape [{n}] (got {tuple(counts.shape)})")
        if counts.is_floating_point() or counts.dtype == torch.bool:
            raise HintAmdError(f"{who}: counts is {counts.dtype}; expected an integer tensor")
        if counts.device != points.device:
            raise HintAmdError(f"{who}: counts is on {counts.device} and points on {points.device}")
        counts = counts.to(torch.int32).contiguous()
    return _fcoef_run(points, n_coeffs, counts, who=who)
