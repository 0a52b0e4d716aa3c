"""The trainable Householder permutation between blocks: what the reference's lens-shape and plus-shape configs put there as
FrEIA's `HouseholderPerm(fixed=False, n_reflections=ndim)` (configs/lens_shape/unconditional_hint_2_full.py:62-65).

FrEIA is neither vendored by the reference nor installed here, so the parameterisation is THIS LIBRARY'S DEFINITION (FrEIA parity
unpinned, as for `FixedOrthogonal`): `Vs` fp32 [n, d], row i the vector v_i,
    H_i = I - 2 v_i v_i^T / (v_i . v_i),    W = H_0 H_1 .. H_(n-1),    forward y = x W,  rev y = x W^T,  log-det 0.
The kernels are hint_amd/csrc/hint_householder.hip behind `hint_householder_run` (include/hint_amd.h states the arithmetic).
There is no CPU implementation.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import hint as _hint
from ._ops import _run_desc
from .hint import HintAmdError, _mark_launch

MAX_D, MAX_N, MAX_B = 128, 256, 1 << 22


def _run(op: int, dev, *, B: int = 1, d: int, n: int = 1, transpose: bool = False, Vs=None, W=None, x=None, y=None, g_y=None,
         g_x=None, g_W=None, g_V=None, workspace=None):
    """one hint_householder_run on the current stream of `dev`; a grad run without a workspace allocates what it needs"""
    ptr = lambda t: t.data_ptr() if t is not None else None
    desc = _lib.HouseholderDesc()
    desc.op, desc.transpose, desc.B, desc.d, desc.n = op, int(bool(transpose)), B, d, n
    desc.Vs, desc.W, desc.x, desc.y = ptr(Vs), ptr(W), ptr(x), ptr(y)
    desc.g_y, desc.g_x, desc.g_W, desc.g_V = ptr(g_y), ptr(g_x), ptr(g_W), ptr(g_V)
    if workspace is not None:
        desc.workspace, desc.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    needs_ws = op == _lib.HOUSEHOLDER_GRAD and workspace is None and (g_W is not None or g_V is not None)
    _run_desc("hint_householder_run", desc, dev, (op, B, d, n) if needs_ws else None, before=_mark_launch)


def _check_rows(x, d: int, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise HintAmdError(f"{what}: hint_amd has no CPU implementation; move the module and the data to the GPU")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != d:
        raise HintAmdError(f"{what}: expected a float32 tensor [B, {d}], got {tuple(x.shape)} {x.dtype}")
    if x.shape[0] > MAX_B:
        raise HintAmdError(f"{what}: B = {x.shape[0]} is above the limit of {MAX_B} rows")
    return x


class _HouseholderFn(torch.autograd.Function):
    """y = x W(Vs) or x W(Vs)^T as one autograd node: BUILD into a fresh W and APPLY forward, one GRAD run backward that asks for
    the gradients autograd needs and no others.  x, Vs and W are saved through save_for_backward: torch's version check covers
    an in-place change between the two passes."""

    @staticmethod
    def forward(ctx, x, Vs, rev):
        n, d = Vs.shape
        dev = x.device
        xc, vc = x.detach().contiguous(), Vs.detach().contiguous()
        W = torch.empty(d, d, dtype=torch.float32, device=dev)
        y = torch.empty_like(xc)
        _run(_lib.HOUSEHOLDER_BUILD, dev, d=d, n=n, Vs=vc, W=W)
        _run(_lib.HOUSEHOLDER_APPLY, dev, B=xc.shape[0], d=d, n=n, transpose=rev, W=W, x=xc, y=y)
        ctx.rev = bool(rev)
        ctx.save_for_backward(xc, vc, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, Vs, W = ctx.saved_tensors
        n, d = Vs.shape
        gy = gy.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gV = torch.empty_like(Vs) if ctx.needs_input_grad[1] else None
        _run(_lib.HOUSEHOLDER_GRAD, x.device, B=x.shape[0], d=d, n=n, transpose=ctx.rev, Vs=Vs, W=W, x=x, g_y=gy, g_x=gx, g_V=gV)
        return gx, gV, None


class HouseholderPerm(nn.Module):
    """x -> x W with W the product of n Householder reflections of the rows of `Vs`; FrEIA-protocol module (list in / list out).
    fixed=True keeps `Vs` without a gradient (it is in the state_dict either way).  Init: 0.2 randn(n, d) + eye(n, d), from a
    generator seeded by `seed` or from the global generator."""

    def __init__(self, dims_in, dims_c=[], n_reflections: Optional[int] = None, fixed: bool = False, seed: Optional[int] = None):
        super().__init__()
        if len(dims_c) > 0:
            raise HintAmdError("HouseholderPerm: the conditional variant (dims_c) is not implemented")
        d = int(dims_in[0][0])
        n = d if n_reflections is None else int(n_reflections)
        if not 1 <= d <= MAX_D:
            raise HintAmdError(f"HouseholderPerm: d = {d} is outside 1..{MAX_D}")
        if not 1 <= n <= MAX_N:
            raise HintAmdError(f"HouseholderPerm: n_reflections = {n} is outside 1..{MAX_N}")
        self.d, self.n, self.fixed = d, n, bool(fixed)
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        init = 0.2 * torch.randn(n, d, generator=gen) + torch.eye(n, d)
        self.Vs = nn.Parameter(init.to(torch.float32), requires_grad=not fixed)
        self._Wbuf: Optional[torch.Tensor] = None       # [d, d] on Vs's device: its address is what chain handles hold
        self._Wkey = None

    # the buffer's address is captured by chain handles of THIS object: a copy builds its own
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_Wbuf"], state["_Wkey"] = None, None
        return state

    def __deepcopy__(self, memo):
        import copy
        buf, key = self._Wbuf, self._Wkey
        self._Wbuf = self._Wkey = None
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                setattr(new, k, copy.deepcopy(v, memo))
        finally:
            self._Wbuf, self._Wkey = buf, key
        return new

    def matrix(self) -> torch.Tensor:
        """the current W [d, d] in the module's own buffer (a stable address per device), rebuilt by BUILD on the current stream.
        Trainable: on every call - ClampAdam writes parameters through raw pointers, which `Vs._version` does not see - unless
        set_pack_cache(True) is on and neither Vs nor the weight generation moved.  fixed=True: once per device and value of Vs."""
        Vs = self.Vs
        if not Vs.is_cuda:
            raise HintAmdError("HouseholderPerm: hint_amd has no CPU implementation; move the module and the data to the GPU")
        dev = Vs.device
        if self._Wbuf is None or self._Wbuf.device != dev:
            self._Wbuf = torch.empty(self.d, self.d, dtype=torch.float32, device=dev)
            self._Wkey = None
        key = (Vs.data_ptr(), Vs._version, _hint._WEIGHT_GEN)
        if (self.fixed or _hint._PACK_CACHE) and self._Wkey == key:
            return self._Wbuf
        vc = Vs.detach()
        _run(_lib.HOUSEHOLDER_BUILD, dev, d=self.d, n=self.n, Vs=vc if vc.is_contiguous() else vc.contiguous(), W=self._Wbuf)
        self._Wkey = key
        return self._Wbuf

    def forward(self, x, c=[], rev=False):
        if len(c) > 0:
            raise HintAmdError("HouseholderPerm: the conditional variant is not implemented")
        x0 = _check_rows(x[0], self.d, "HouseholderPerm")
        if not self.Vs.is_cuda or self.Vs.device != x0.device:
            raise HintAmdError("HouseholderPerm: the module and its input must be on one GPU (no CPU implementation)")
        if x0.shape[0] == 0:
            return [x0.new_empty(0, self.d)]
        if torch.is_grad_enabled() and (x0.requires_grad or self.Vs.requires_grad):
            return [_HouseholderFn.apply(x0, self.Vs, bool(rev))]
        W = self.matrix()
        xc = x0.detach().contiguous()
        y = torch.empty_like(xc)
        _run(_lib.HOUSEHOLDER_APPLY, xc.device, B=xc.shape[0], d=self.d, n=self.n, transpose=rev, W=W, x=xc, y=y)
        return [y]

    def jacobian(self, x, c=[], rev=False):
        return 0.0

    def output_dims(self, input_dims):
        return input_dims


def perm_matrix(m) -> torch.Tensor:
    """the [d, d] matrix a flow's fused launches read for the permutation module `m`: a FixedOrthogonal's stored W, a
    HouseholderPerm's current one (rebuilt on the current stream when stale)"""
    return m.matrix() if isinstance(m, HouseholderPerm) else m.W


def trainable(m) -> bool:
    return isinstance(m, HouseholderPerm) and m.Vs.requires_grad
