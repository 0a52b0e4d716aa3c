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
from .curves import _check_no_grad, _check_real, _outputs, lens_forward_process

__all__ = ["sample_lens_prior", "sample_lens_joint", "lens_rings", "lens_draws", "fourier_coeffs"]

MAX_ROWS = 1 << 30
RING_POINTS = 32
MAX_COEFFS = 25
MAX_POINTS = 1024
MAX_POINT_ROWS = 1 << 24
_F32, _I32 = torch.float32, torch.int32
_LENS_TABLE = lambda n: dict(x=((n, 20), _F32), ring=((n, RING_POINTS, 2), _F32), counts=((n,), _I32), eps=((n, 2), _F32),  # noqa: E731
                             draws_out=((n, 4), _F32))


def _check_int(v, name: str, who: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise HintAmdError(f"{who}: {name} must be an int (got {type(v).__name__})")
    if v < lo or v > hi:
        raise HintAmdError(f"{who}: {name} must be {lo}..{hi} (got {v})")
    return v


def _check_device(device, who: str) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise HintAmdError(f"{who}: no GPU is available; the sampler is a GPU kernel and there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    try:
        dev = torch.device(device)
    except (TypeError, RuntimeError) as e:
        raise HintAmdError(f"{who}: device must name a device (got {device!r})") from e
    if dev.type != "cuda":
        raise HintAmdError(f"{who}: device is {dev}; the sampler is a GPU kernel and there is no CPU fallback")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _check_draws(draws, n: Optional[int], who: str) -> torch.Tensor:
    if not isinstance(draws, torch.Tensor):
        raise HintAmdError(f"{who}: draws must be a tensor (got {type(draws).__name__})")
    if draws.dim() != 2 or draws.shape[1] != 4 or draws.shape[0] < 1 or draws.shape[0] > MAX_ROWS:
        raise HintAmdError(f"{who}: draws must be [1..{MAX_ROWS}, 4] = (u_r, u_t, n_x, n_y) (got shape {tuple(draws.shape)})")
    if n is not None and draws.shape[0] != n:
        raise HintAmdError(f"{who}: draws holds {draws.shape[0]} rows and n is {n}")
    if not draws.is_cuda:
        raise HintAmdError(f"{who}: draws is on {draws.device}; the sampler is a GPU kernel and there is no CPU fallback")
    if not draws.is_floating_point():
        raise HintAmdError(f"{who}: draws is {draws.dtype}; expected a floating-point tensor")
    _check_no_grad(draws, "draws", who)
    draws = draws.detach()
    if draws.dtype != torch.float32 or not draws.is_contiguous():
        draws = draws.to(torch.float32).contiguous()
    return draws


def _sample_args(n, seed, offset, device, draws, who: str):
    n = _check_int(n, "n", who, 1, MAX_ROWS)
    seed = _check_int(seed, "seed", who, 0, 2 ** 64 - 1)
    offset = _check_int(offset, "offset", who, 0, 2 ** 64 - 1 - n)
    if draws is not None:
        draws = _check_draws(draws, n, who)
        if device is not None and _check_device(device, who) != draws.device:
            raise HintAmdError(f"{who}: draws is on {draws.device} and device is {device}")
        return n, seed, offset, draws.device, draws
    return n, seed, offset, _check_device(device, who), None


def _rejected(ws: torch.Tensor, what: str, who: str) -> None:
    """the one host read of the paths that take rows from the caller: the workspace's words add up to the rejected rows"""
    bad = int(ws.view(torch.int32).sum().item())
    if bad:
        raise HintAmdError(f"{who}: {bad} row(s) rejected: {what}")


def _lens_run(n: int, seed: int, offset: int, dev: torch.device, draws: Optional[torch.Tensor], want, out=None,
              max_groups: int = 0, who: str = "hint_lensgen_run"):
    """one hint_lensgen_run on checked arguments: the outputs named in `want` as a dict (`out`: the tests' guarded buffers)"""
    lib = _lib.load()
    with torch.cuda.device(dev):
        desc = _lib.LensGenDesc()
        desc.n_rows, desc.seed, desc.offset, desc.max_groups = n, seed, offset, max_groups
        desc.draws = draws.data_ptr() if draws is not None else None
        res = _outputs(desc, _LENS_TABLE(n), want, out, dev)
        nbytes = lib.hint_lensgen_workspace_bytes(n)
        if nbytes == 0:
            _lib.check(1, "hint_lensgen_workspace_bytes")
        ws = out["workspace"] if out is not None and "workspace" in out else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        desc.workspace, desc.workspace_bytes = ws.data_ptr(), nbytes
        st = lib.hint_lensgen_run(desc, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "hint_lensgen_run")
    if draws is not None:
        _rejected(ws[:nbytes], "u_r or u_t outside [0, 1], or a draw that is not finite", who)
    res["workspace"] = ws
    return res


def sample_lens_prior(n: int, seed: int, *, offset: int = 0, device=None, draws: Optional[torch.Tensor] = None,
                      return_ring: bool = False):
    """the reference's LensShapeModel.sample_prior(n): x [n, 20] fp32 on the device, row i a function of (seed, offset + i) alone.
    draws [n, 4] = (u_r, u_t, n_x, n_y) replaces the Philox stream (seed and offset then go unused; the rows are checked, which
    reads one number back).  return_ring: (x, ring [n, 32, 2], counts [n]) - the closed, centred, zero-padded ring x is made of"""
    who = "sample_lens_prior"
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who)
    res = _lens_run(n, seed, offset, dev, draws, ["x", "ring", "counts"] if return_ring else ["x"], who=who)
    return (res["x"], res["ring"], res["counts"]) if return_ring else res["x"]


def sample_lens_joint(n: int, seed: int, noise: float = 0.05, *, offset: int = 0, device=None,
                      draws: Optional[torch.Tensor] = None, return_eps: bool = False):
    """the reference's LensShapeModel.sample_joint(n): (x [n, 20], y [n, 2]) with y = lens_forward_process(x, noise, eps=eps), eps
    the stream-1 draws of (seed, offset + i).  return_eps: (x, y, eps)"""
    who = "sample_lens_joint"
    noise = _check_real(noise, "noise", who, nonneg=False)
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who)
    res = _lens_run(n, seed, offset, dev, draws, ["x", "eps"], who=who)
    y = lens_forward_process(res["x"], noise, eps=res["eps"])
    return (res["x"], y, res["eps"]) if return_eps else (res["x"], y)


def lens_rings(draws: torch.Tensor):
    """(ring [n, 32, 2], counts [n] int32) of draws [n, 4]: the closed ring of each lens, centred and noised as generate_lens_shape
    returns it, zero-padded behind its 31 or 32 points; fourier_coeffs(ring, 5, counts) is sample_lens_prior's x up to rounding"""
    who = "lens_rings"
    draws = _check_draws(draws, None, who)
    res = _lens_run(draws.shape[0], 0, 0, draws.device, draws, ["x", "ring", "counts"], who=who)
    return res["ring"], res["counts"]


def lens_draws(n: int, seed: int, *, offset: int = 0, device=None) -> torch.Tensor:
    """the draws sample_lens_prior(n, seed, offset=offset) uses, [n, 4] = (u_r, u_t, n_x, n_y)"""
    who = "lens_draws"
    n, seed, offset, dev, _ = _sample_args(n, seed, offset, device, None, who)
    return _lens_run(n, seed, offset, dev, None, ["x", "draws_out"], who=who)["draws_out"]


def _fcoef_run(points: torch.Tensor, n_coeffs: int, counts: Optional[torch.Tensor], out=None, max_groups: int = 0,
               who: str = "hint_fcoef_run"):
    lib = _lib.load()
    n, p = points.shape[0], points.shape[1]
    dev = points.device
    with torch.cuda.device(dev):
        desc = _lib.FcoefDesc()
        desc.points, desc.counts = points.data_ptr(), (counts.data_ptr() if counts is not None else None)
        desc.n_rows, desc.p_max, desc.n_coeffs, desc.max_groups = n, p, n_coeffs, max_groups
        res = _outputs(desc, dict(x=((n, 4 * n_coeffs), _F32)), ["x"], out, dev)
        nbytes = lib.hint_fcoef_workspace_bytes(n, p, n_coeffs)
        if nbytes == 0:
            _lib.check(1, "hint_fcoef_workspace_bytes")
        ws = out["workspace"] if out is not None and "workspace" in out else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        desc.workspace, desc.workspace_bytes = ws.data_ptr(), nbytes
        st = lib.hint_fcoef_run(desc, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "hint_fcoef_run")
    if counts is not None:
        _rejected(ws[:nbytes], f"every count must be n_coeffs..{p}", who)
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
