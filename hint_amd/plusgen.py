"""The plus-shape sampler on the device (hint_amd/csrc/hint_plusgen.hip): prior, joint, targeted and conditional rows, what feeds
the plus shape's evaluation pipeline.

    sample_plus_prior(n, seed)                  PlusShapeModel.sample_prior(n)                              data.py:229-238
    sample_plus_joint(n, seed)                  PlusShapeModel.sample_joint(n)                              data.py:240-252
    sample_plus_targeted(n, seed, target)       generate_plus_shape(forward=True, target=target), n times   data.py:188-227
    sample_plus_conditional(target, n, seed)    the rejection loop of correlation_conditional               rejection_sampling.py:113-127
    plus_outlines(draws, target)                generate_plus_shape's coords and label                      data.py:188-227
    plus_draws(n, seed)                         the nine draws of each row

The union of the two bars is taken in closed form (include/hint_amd.h hint_plusgen_desc states every step); no polygon library is
involved, and THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION - clockwise from the first corner met clockwise from the
negative x axis - because the reference takes whatever its polygon library returns.  Rows are a function of (seed, row, target)
alone (Philox4x32-10): chunks at any boundaries have the bits of one call, and a gather by row has the bits of the contiguous
call.  One launch per call, no autograd.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import MAX_SAMPLE_ROWS, _check_device, _check_draws, _check_int, _check_real, _outputs, _rejected, _run_desc, _sample_args

__all__ = ["sample_plus_prior", "sample_plus_joint", "sample_plus_targeted", "sample_plus_conditional", "plus_outlines",
           "plus_draws"]

MAX_ROWS = MAX_SAMPLE_ROWS
OUTLINE_POINTS = 128
_DRAWS = ("u_xl", "u_yl", "u_xw", "u_yw", "u_xs", "u_ys", "u_a", "n_x", "n_y")
N_DRAWS = len(_DRAWS)
_F32, _I32 = torch.float32, torch.int32
_TABLE = lambda n: dict(x=((n, 100), _F32), y=((n, 4), _F32), outline=((n, OUTLINE_POINTS, 2), _F32), counts=((n,), _I32),  # noqa: E731
                        corners=((n,), _I32), draws_out=((n, N_DRAWS), _F32))
_REFUSED = "a uniform outside [0, 1], or a draw that is not finite"


def _check_target(target, who: str):
    """a target (cx, cy, angle, ratio) as four Python floats that are exact fp32 values, or None"""
    if target is None:
        return None
    if isinstance(target, torch.Tensor):
        if target.is_cuda:
            raise HintAmdError(f"{who}: target is on {target.device}; it is a host value (a sequence of 4 numbers or a CPU tensor)")
        target = target.detach().reshape(-1).tolist()
    try:
        t = [float(v) for v in target]
    except (TypeError, ValueError) as e:
        raise HintAmdError(f"{who}: target must be 4 numbers (cx, cy, angle, ratio) (got {target!r})") from e
    if len(t) != 4:
        raise HintAmdError(f"{who}: target must be 4 numbers (cx, cy, angle, ratio) (got {len(t)})")
    t = [_check_real(v, f"target[{i}]", who, nonneg=False) for i, v in enumerate(t)]
    t = torch.tensor(t, dtype=torch.float64).to(torch.float32).tolist()
    if not all(math.isfinite(v) for v in t):
        raise HintAmdError(f"{who}: target must be finite in fp32 (got {target!r})")
    if t[3] < 0.25 or t[3] > 4.0:
        raise HintAmdError(f"{who}: target[3], the ratio, must be 0.25..4 (got {t[3]})")
    return t


def _plus_run(n: int, seed: int, offset: int, dev: torch.device, draws: Optional[torch.Tensor], want, target=None,
              rows: Optional[torch.Tensor] = None, out=None, max_groups: int = 0, who: str = "hint_plusgen_run"):
    """one hint_plusgen_run on checked arguments: the outputs named in `want` as a dict (`out`: the tests' guarded buffers).
    rows: uint64-as-int64 [n] on the device, the Philox rows of a gather"""
    desc = _lib.PlusGenDesc()
    desc.n_rows, desc.seed, desc.offset, desc.max_groups = n, seed, offset, max_groups
    desc.draws = draws.data_ptr() if draws is not None else None
    desc.rows = rows.data_ptr() if rows is not None else None
    tgt = (C.c_float * 4)(*target) if target is not None else None              # (read during the call; alive until it returns)
    desc.target = tgt
    res = _outputs(desc, _TABLE(n), want, out, dev)
    ws = _run_desc("hint_plusgen_run", desc, dev, (n,), out)
    if draws is not None:
        _rejected(ws[:desc.workspace_bytes], _REFUSED, who)
    res["workspace"] = ws
    return res


def sample_plus_prior(n: int, seed: int, *, offset: int = 0, device=None, draws: Optional[torch.Tensor] = None,
                      return_outline: bool = False):
    """the reference's PlusShapeModel.sample_prior(n): x [n, 100] fp32 on the device, row i a function of (seed, offset + i) alone.
    draws [n, 9] = (u_xl, u_yl, u_xw, u_yw, u_xs, u_ys, u_a, n_x, n_y) replaces the Philox stream (seed and offset then go unused;
    the rows are checked, which reads one number back).  return_outline: (x, outline [n, 128, 2], counts [n]) - the dense, placed,
    zero-padded outline x is made of"""
    who = "sample_plus_prior"
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who, _DRAWS)
    res = _plus_run(n, seed, offset, dev, draws, ["x", "outline", "counts"] if return_outline else ["x"], who=who)
    return (res["x"], res["outline"], res["counts"]) if return_outline else res["x"]


def sample_plus_joint(n: int, seed: int, *, offset: int = 0, device=None, draws: Optional[torch.Tensor] = None):
    """the reference's PlusShapeModel.sample_joint(n): (x [n, 100], y [n, 4]) in one launch, y = (center_x, center_y, angle,
    xwidth / ywidth); x is sample_plus_prior's, bit for bit"""
    who = "sample_plus_joint"
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who, _DRAWS)
    res = _plus_run(n, seed, offset, dev, draws, ["x", "y"], who=who)
    return res["x"], res["y"]


def sample_plus_targeted(n: int, seed: int, target, *, offset: int = 0, device=None, draws: Optional[torch.Tensor] = None):
    """generate_plus_shape(forward=True, target=target) for every row: (x [n, 100], y [n, 4]).  target = (cx, cy, angle, ratio), a
    host value, 0.25 <= ratio <= 4: the row's angle is target[2] and its widths have the ratio target[3]; cx and cy are not read"""
    who = "sample_plus_targeted"
    target = _check_target(target, who)
    if target is None:
        raise HintAmdError(f"{who}: target must be 4 numbers (cx, cy, angle, ratio) (got None)")
    n, seed, offset, dev, draws = _sample_args(n, seed, offset, device, draws, who, _DRAWS)
    res = _plus_run(n, seed, offset, dev, draws, ["x", "y"], target=target, who=who)
    return res["x"], res["y"]


def plus_outlines(draws: torch.Tensor, target=None):
    """(outline [n, 128, 2], counts [n] int32, y [n, 4]) of draws [n, 9]: the dense outline of each plus, centred, rotated and
    offset as generate_plus_shape returns it, zero-padded behind its 54..106 points, and its label;
    fourier_coeffs(outline, 25, counts) is sample_plus_prior's x up to rounding"""
    who = "plus_outlines"
    target = _check_target(target, who)
    draws = _check_draws(draws, None, who, _DRAWS)
    res = _plus_run(draws.shape[0], 0, 0, draws.device, draws, ["y", "outline", "counts"], target=target, who=who)
    return res["outline"], res["counts"], res["y"]


def plus_draws(n: int, seed: int, *, offset: int = 0, device=None) -> torch.Tensor:
    """the draws sample_plus_prior(n, seed, offset=offset) uses, [n, 9]"""
    who = "plus_draws"
    n, seed, offset, dev, _ = _sample_args(n, seed, offset, device, None, who, _DRAWS)
    return _plus_run(n, seed, offset, dev, None, ["y", "draws_out"], who=who)["draws_out"]


def sample_plus_conditional(target, n: int, seed: int, radius: float = 0.05, *, chunk: int = 1 << 20, max_rows: int = 1 << 30,
                            device=None):
    """the ground-truth conditional sample of rejection_sampling.py:113-127: (x [n, 100], y [n, 4], tried).  Candidates are the
    targeted rows 0, 1, 2, .. of `seed`; labels-only launches run over consecutive ranges of `chunk` rows, and a row is kept when
    |y - target| < radius - the squared distance in fp32, ((e0^2 + e1^2) + (e2^2 + e3^2)) < fl(radius^2), e = y - target.  Once n
    rows are kept, one gathered launch makes x and y of exactly the first n, in row order; `tried` is the n-th kept row's index + 1,
    the candidates the reference's loop would have drawn.  The result is a function of (seed, target, radius, n) alone, not of
    chunk.  Each chunk reads one number back.  Raises when max_rows candidates did not yield n"""
    who = "sample_plus_conditional"
    target = _check_target(target, who)
    if target is None:
        raise HintAmdError(f"{who}: target must be 4 numbers (cx, cy, angle, ratio) (got None)")
    n = _check_int(n, "n", who, 1, MAX_ROWS)
    seed = _check_int(seed, "seed", who, 0, 2 ** 64 - 1)
    chunk = _check_int(chunk, "chunk", who, 1, MAX_ROWS)
    max_rows = _check_int(max_rows, "max_rows", who, 1, 2 ** 62)
    radius = _check_real(radius, "radius", who, nonneg=True)
    dev = _check_device(device, who)
    t = torch.tensor(target, dtype=_F32, device=dev)
    r2 = torch.tensor(radius * radius, dtype=torch.float64).to(_F32).to(dev)
    kept, have, start = [], 0, 0
    while have < n and start < max_rows:
        m = min(chunk, max_rows - start)
        y = _plus_run(m, seed, start, dev, None, ["y"], target=target, who=who)["y"]
        s = (y - t).square()
        idx = torch.nonzero(((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) < r2).reshape(-1) + start
        kept.append(idx)
        have += int(idx.numel())                                               # (the one host read of a chunk)
        start += m
    if have < n:
        raise HintAmdError(f"{who}: {start} candidates gave {have} rows within {radius} of the target, fewer than n = {n} "
                           f"(max_rows = {max_rows})")
    rows = torch.cat(kept)[:n].contiguous()
    tried = int(rows[-1].item()) + 1
    res = _plus_run(n, seed, 0, dev, None, ["x", "y"], target=target, rows=rows, who=who)
    return res["x"], res["y"], tried
