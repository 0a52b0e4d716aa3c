"""What the wrappers of the descriptor entry points (curves, metrics, abc, shapes, plusgen, householder) share: the one call of
such an entry point, the outputs of a call, and the argument checks more than one module uses.  Internal."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError


_SIZERS = {}        # hint_<op>_run -> hint_<op>_workspace_bytes


def _run_desc(entry: str, desc, dev, size_args=None, out=None, before=None) -> Optional[torch.Tensor]:
    """one hint_<op>_run on the filled descriptor, on the current stream of `dev` - the descriptor's `stream` field where it has
    one, the second argument elsewhere.  size_args: the call needs a workspace of hint_<op>_workspace_bytes(*size_args) - the
    tensor `out` holds as "workspace" (the tests' guarded buffers) or a new one, which is returned.  before: called under the
    device, right before the entry point"""
    lib = _lib.load()                                       # (every call: the stream tests put a recording library in its place)
    ws = None
    with torch.cuda.device(dev):
        if size_args is not None:
            sizer = _SIZERS.get(entry) or _SIZERS.setdefault(entry, entry[:-len("run")] + "workspace_bytes")
            nbytes = getattr(lib, sizer)(*size_args)
            if nbytes == 0:
                _lib.check(1, sizer)
            ws = out["workspace"] if out is not None and "workspace" in out else torch.empty(nbytes, dtype=torch.uint8, device=dev)
            desc.workspace, desc.workspace_bytes = ws.data_ptr(), nbytes
        stream = torch.cuda.current_stream(dev).cuda_stream
        if before is not None:
            before()
        if hasattr(desc, "stream"):
            desc.stream = stream
            st = getattr(lib, entry)(desc)
        else:
            st = getattr(lib, entry)(desc, stream)
    if st != 0:
        _lib.check(st, entry)
    return ws


def _outputs(desc, table, want, out, dev):
    """the outputs named in `want` as a dict, by table = name -> (shape, dtype): the tensor `out` holds under the name (the tests'
    guarded buffers) or a new one.  Sets the descriptor's pointer of every name of the table, None where it is not wanted"""
    res = {}
    for name in want:
        shape, dtype = table[name]
        res[name] = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
    for name in table:
        setattr(desc, name, res[name].data_ptr() if name in res else None)
    return res


def _check_real(v, name: str, who: str, nonneg: bool = True) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise HintAmdError(f"{who}: {name} must be a number (got {type(v).__name__})")
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        raise HintAmdError(f"{who}: {name} must be finite (got {v})")
    if nonneg and v < 0.0:
        raise HintAmdError(f"{who}: {name} must be >= 0 (got {v})")
    return v


def _check_no_grad(t: torch.Tensor, name: str, who: str) -> None:
    if t.requires_grad and torch.is_grad_enabled():
        raise HintAmdError(f"{who}: {name} requires grad, and no gradient is implemented; call it under torch.no_grad() or "
                           "detach the input")


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


# ---- the samplers (shapes, plusgen): a row's draws, len(names) of them, and the arguments of a sampling call ----
MAX_SAMPLE_ROWS = 1 << 30


def _check_draws(draws, n: Optional[int], who: str, names) -> torch.Tensor:
    if not isinstance(draws, torch.Tensor):
        raise HintAmdError(f"{who}: draws must be a tensor (got {type(draws).__name__})")
    if draws.dim() != 2 or draws.shape[1] != len(names) or draws.shape[0] < 1 or draws.shape[0] > MAX_SAMPLE_ROWS:
        raise HintAmdError(f"{who}: draws must be [1..{MAX_SAMPLE_ROWS}, {len(names)}] = ({', '.join(names)}) "
                           f"(got shape {tuple(draws.shape)})")
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


def _sample_args(n, seed, offset, device, draws, who: str, names):
    n = _check_int(n, "n", who, 1, MAX_SAMPLE_ROWS)
    seed = _check_int(seed, "seed", who, 0, 2 ** 64 - 1)
    offset = _check_int(offset, "offset", who, 0, 2 ** 64 - 1 - n)
    if draws is not None:
        draws = _check_draws(draws, n, who, names)
        if device is not None and _check_device(device, who) != draws.device:
            raise HintAmdError(f"{who}: draws is on {draws.device} and device is {device}")
        return n, seed, offset, draws.device, draws
    return n, seed, offset, _check_device(device, who), None


def _rejected(ws: torch.Tensor, what: str, who: str) -> None:
    """the one host read of the paths that take rows from the caller: the workspace's words add up to the rejected rows"""
    bad = int(ws.view(torch.int32).sum().item())
    if bad:
        raise HintAmdError(f"{who}: {bad} row(s) rejected: {what}")
