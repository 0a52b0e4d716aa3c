"""ClampAdam: the optimizer statements of the reference loop in one launch, for a loop that keeps everything else.

    for p in params_trainable: p.grad.data.clamp_(-5.00, 5.00)        train_unconditional.py:140-141
    optim.step()                     (torch.optim.Adam, L2 decay)     train_unconditional.py:144, 174-176

cost 3.3-3.9 ms per step on a model of 288 parameter tensors: 288 clamp launches and torch's Adam over 288
tensors.  ClampAdam is a torch.optim.Optimizer (param_groups, schedulers, state_dict as usual) whose step() hands a table of
(parameter, gradient, exp_avg, exp_avg_sq) segments to hint_adam_multi_step: one kernel launch per param group, whatever
buffers the parameters live in.  It reads nothing of hint_amd.hint but what the tensors show (data_ptr, grad, numel), so it
serves any fp32 CUDA parameters.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import hint as _hint
from ._lib import HintAmdError

__all__ = ["ClampAdam", "coalesce_segments", "chunk_segments"]

Seg = Tuple[int, int, int, int, int]        # addresses of p, g, m, v and the number of floats

# a hole of up to this many floats between two parameters (an arena's padding to 16 bytes) is mirrored in the moment buffers,
# so that the moments keep the parameters' alignment; a wider one starts a new run
_MIRROR_GAP = 64


def coalesce_segments(segs: Sequence[Seg]) -> List[Seg]:
    """merge every segment whose p, g, m and v all start where the previous one's end; drop empty ones"""
    out: List[Seg] = []
    for p, g, m, v, n in segs:
        if n == 0:
            continue
        if out:
            P, G, M, V, N = out[-1]
            if p == P + 4 * N and g == G + 4 * N and m == M + 4 * N and v == V + 4 * N:
                out[-1] = (P, G, M, V, N + n)
                continue
        out.append((p, g, m, v, n))
    return out


def _seg_array(segs: Sequence[Seg]):
    arr = (_lib.AdamSeg * max(len(segs), 1))()
    for i, (p, g, m, v, n) in enumerate(segs):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p, g, m, v, n
    return arr


def chunk_segments(segs: Sequence[Seg]) -> List[Tuple[int, int, int]]:
    """the work items hint_adam_multi_create cuts a segment table into: (segment, first float, floats).  Host only."""
    lib = _lib.load()
    arr = _seg_array(segs)
    n = lib.hint_adam_multi_chunk(arr, len(segs), -1, 0)
    _lib.check(1 if n < 0 else 0, "hint_adam_multi_chunk")
    return [tuple(lib.hint_adam_multi_chunk(arr, len(segs), c, f) for f in range(3)) for c in range(n)]


def layout_moments(ptrs: Sequence[int], numels: Sequence[int]) -> Tuple[List[int], int]:
    """float offsets of every parameter's moments in a flat buffer (and the buffer's length) such that a moment has its
    parameter's address modulo 16 and parameters that follow each other closely keep their distance"""
    offs, end, prev_ptr, prev_off = [], 0, None, 0
    for ptr, n in zip(ptrs, numels):
        gap = (ptr - prev_ptr) if prev_ptr is not None else -1
        if prev_ptr is not None and gap % 4 == 0 and prev_off + gap // 4 >= end and gap // 4 <= end - prev_off + _MIRROR_GAP:
            off = prev_off + gap // 4
        else:
            off = (end + 3) // 4 * 4 + ((ptr >> 2) & 3)
        offs.append(off)
        end = max(end, off + n)
        prev_ptr, prev_off = ptr, off
    return offs, end


class _Part:
    """the parameters of one group that take the same step number on one device: one handle, one launch"""
    __slots__ = ("device", "step", "handle", "index", "all")

    def __init__(self, device, step, handle, index, covers_all):
        self.device, self.step, self.handle, self.index, self.all = device, step, handle, index, covers_all


class _Group:
    """what the optimizer keeps per param group: the flat moment buffers, the step counts and the device tables"""

    def __init__(self):
        self.pkey: Optional[List[int]] = None       # parameter addresses the moments were laid out for
        self.gkey: Optional[List[int]] = None       # gradient addresses (0: none) the tables were built from
        self.bufs = {}                              # device -> (exp_avg flat, exp_avg_sq flat)
        self.offs: List[int] = []
        self.steps: Optional[torch.Tensor] = None   # CPU, one count per parameter; state[p]["step"] is a 0-dim view
        self.parts: List[_Part] = []
        self.dirty = True


class ClampAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, no AMSGrad) with the gradient scaled by `grad_scale`, then clamped to
    +-`grad_clamp` (0: no clamp), for all parameters of a group in one kernel launch.

    Non-finite gradients take the step `p.grad.data.clamp_(-c, c)` + `torch.optim.Adam.step()` take: the clamp is torch.clamp's,
    so a NaN gradient stays NaN and makes that element of p, exp_avg and exp_avg_sq NaN for good (a diverged run shows, it does
    not keep "training"), +-inf becomes +-grad_clamp, and with grad_clamp = 0 nothing at all is clamped: an inf gradient makes
    both moments inf and the parameter NaN, as torch.optim.Adam alone does (tests/test_gpu_nonfinite.py).

    state[p] holds torch's keys (`step`, `exp_avg`, `exp_avg_sq`) with torch's shapes; the moments are views into flat buffers
    this object owns.  state_dict() returns copies, load_state_dict() copies into the flat buffers, and both exchange with
    torch.optim.Adam over the same parameters.  `table_builds` counts how often the device tables were rebuilt (parameters or
    gradients moved), `launches` the kernel launches."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 grad_clamp=0.0, grad_scale=1.0):
        if isinstance(lr, torch.Tensor):
            raise HintAmdError("ClampAdam: a tensor lr belongs to capturable optimizers; pass a float")
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                         ("differentiable", differentiable), ("decoupled_weight_decay", decoupled_weight_decay)):
            if on:
                raise HintAmdError(f"ClampAdam does not support {name}=True")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= grad_clamp:
            raise ValueError(f"Invalid grad_clamp value: {grad_clamp}")
        # (every key torch.optim.Adam reads from a group, so that a saved group loads into it; foreach / fused choose between
        # torch's own implementations and mean nothing here)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                        grad_clamp=grad_clamp, grad_scale=grad_scale)
        self._groups: List[_Group] = []
        self.table_builds = 0
        self.launches = 0
        super().__init__(params, defaults)

    # ---- construction and bookkeeping ------------------------------------------------------------------------------
    @staticmethod
    def _check_param(p: torch.Tensor, what: str):
        if p.is_sparse or p.layout != torch.strided:
            raise HintAmdError(f"ClampAdam: {what} is not a dense tensor")
        if not p.is_cuda:
            raise HintAmdError(f"ClampAdam: {what} is on {p.device}; the step is a GPU kernel and there is no CPU fallback")
        if p.dtype != torch.float32:
            raise HintAmdError(f"ClampAdam: {what} is {p.dtype}; the kernel is fp32 only")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        gi = len(self.param_groups) - 1
        group = self.param_groups[gi]
        for name in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"):
            if group.get(name):
                raise HintAmdError(f"ClampAdam does not support {name}=True (param group {gi})")
        for i, p in enumerate(group["params"]):
            self._check_param(p, self._name(gi, i, p))

    @staticmethod
    def _name(gi: int, i: int, p: torch.Tensor) -> str:
        return f"parameter {i} of param group {gi} (shape {tuple(p.shape)})"

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_groups", [])
        self.__dict__.setdefault("table_builds", 0)
        self.__dict__.setdefault("launches", 0)
        for g in self.param_groups:
            g.setdefault("grad_clamp", self.defaults["grad_clamp"])
            g.setdefault("grad_scale", self.defaults["grad_scale"])
        for rec in self._groups:
            rec.dirty = True

    def __getstate__(self):
        st = dict(super().__getstate__())
        for k in ("_groups", "table_builds", "launches"):
            st.pop(k, None)
        return st

    def _free(self, rec: _Group):
        for part in rec.parts:
            if part.handle:
                _lib.load().hint_adam_multi_destroy(part.handle)
                part.handle = None
        rec.parts = []

    def __del__(self):
        try:
            for rec in self._groups:
                self._free(rec)
        except Exception:
            pass

    # ---- state exchange ----------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch's layout; every tensor is a copy (the live ones are views into this object's flat buffers)"""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)         # (marks every group dirty through __setstate__)
        self._sync()                                # copy what came in into the flat buffers now, keep no foreign storage

    # ---- tables --------------------------------------------------------------------------------------------------------
    @staticmethod
    def _keys(params):
        pkey = [p.data_ptr() for p in params]
        gkey = []
        for p in params:
            g = p.grad
            gkey.append(0 if g is None else g.data_ptr())
        return pkey, gkey

    def _sync(self):
        while len(self._groups) < len(self.param_groups):
            self._groups.append(_Group())
        for gi, group in enumerate(self.param_groups):
            rec = self._groups[gi]
            params = group["params"]
            try:
                pkey, gkey = self._keys(params)
            except RuntimeError:                      # a tensor without storage (sparse gradient): _rebuild names it
                pkey = gkey = None
            if rec.dirty or pkey is None or pkey != rec.pkey or gkey != rec.gkey:
                self._rebuild(gi, group, rec)

    def _rebuild(self, gi: int, group, rec: _Group):
        params = group["params"]
        grads = [p.grad for p in params]
        for i, (p, g) in enumerate(zip(params, grads)):
            what = self._name(gi, i, p)
            self._check_param(p, what)
            if not p.is_contiguous():
                raise HintAmdError(f"ClampAdam: {what} is not contiguous")
            if g is not None:
                self._check_param(g, "the gradient of " + what)
                if g.device != p.device or g.numel() != p.numel():
                    raise HintAmdError(f"ClampAdam: the gradient of {what} is on {g.device} with {g.numel()} elements")
                if not g.is_contiguous():
                    raise HintAmdError(f"ClampAdam: the gradient of {what} is not contiguous")
        pkey, gkey = self._keys(params)
        numels = [p.numel() for p in params]
        devices = [p.device for p in params]
        # the moments' layout follows the parameters' addresses; it is redone (and the moments moved) when one of them moved
        if rec.pkey != pkey or rec.steps is None or len(rec.offs) != len(params):
            offs, bufs = [0] * len(params), {}
            for dev in dict.fromkeys(devices):
                idx = [i for i, d in enumerate(devices) if d == dev]
                o, total = layout_moments([pkey[i] for i in idx], [numels[i] for i in idx])
                for i, oi in zip(idx, o):
                    offs[i] = oi
                bufs[dev] = (torch.zeros(max(total, 4), dtype=torch.float32, device=dev),
                             torch.zeros(max(total, 4), dtype=torch.float32, device=dev))
            steps = torch.zeros(len(params), dtype=torch.float32)
            if rec.steps is not None and rec.steps.numel() == len(params):
                steps.copy_(rec.steps)
            rec.offs, rec.bufs, rec.steps = offs, bufs, steps
        views = []
        for p, off, n, dev in zip(params, rec.offs, numels, devices):
            m, v = rec.bufs[dev]
            views.append((m[off:off + n].view(p.shape), v[off:off + n].view(p.shape)))
        # state: what is there (an earlier layout's views, tensors load_state_dict brought) moves into the views; a parameter
        # that has a gradient for the first time starts at zero (torch's lazy initialisation)
        for i, (p, g) in enumerate(zip(params, grads)):
            st = self.state[p] if p in self.state else None
            mv, vv = views[i]
            if st is not None and len(st) > 0:
                for name, view in (("exp_avg", mv), ("exp_avg_sq", vv)):
                    t = st[name]
                    if t.data_ptr() != view.data_ptr() or t.shape != view.shape:
                        view.copy_(t)
                        st[name] = view
                s = st["step"]
                if not (isinstance(s, torch.Tensor) and s.data_ptr() == rec.steps[i].data_ptr()):
                    rec.steps[i] = float(s)
                    st["step"] = rec.steps[i]
            elif g is not None:
                mv.zero_()
                vv.zero_()
                rec.steps[i] = 0
                st = self.state[p]
                st["step"], st["exp_avg"], st["exp_avg_sq"] = rec.steps[i], mv, vv
        # one table per (device, step count) among the parameters that have a gradient
        self._free(rec)
        active = [i for i, g in enumerate(grads) if g is not None]
        sets, counts = {}, rec.steps.tolist()
        for i in active:
            sets.setdefault((devices[i], int(counts[i])), []).append(i)
        lib = _lib.load()
        for (dev, step), idx in sets.items():
            segs = coalesce_segments([(pkey[i], gkey[i], views[i][0].data_ptr(), views[i][1].data_ptr(), numels[i])
                                      for i in idx])
            handle = C.c_void_p()
            with torch.cuda.device(dev):
                _lib.check(lib.hint_adam_multi_create(_seg_array(segs), len(segs), C.byref(handle)), "hint_adam_multi_create")
            covers_all = len(idx) == len(params)
            rec.parts.append(_Part(dev, step, handle, None if covers_all else torch.tensor(idx, dtype=torch.long), covers_all))
        rec.pkey, rec.gkey, rec.dirty = pkey, gkey, False
        self.table_builds += 1

    # ---- the step ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._sync()
        lib = _lib.load()
        for group, rec in zip(self.param_groups, self._groups):
            b1, b2 = group["betas"]
            for part in rec.parts:
                part.step += 1
                with torch.cuda.device(part.device):
                    st = lib.hint_adam_multi_step(part.handle, part.step, float(group["lr"]), float(b1), float(b2),
                                                  float(group["eps"]), float(group["weight_decay"]),
                                                  float(group["grad_scale"]), float(group["grad_clamp"]), 0,
                                                  torch.cuda.current_stream(part.device).cuda_stream)
                _lib.check(st, "hint_adam_multi_step")
                self.launches += 1
                if part.all:
                    rec.steps.add_(1)
                else:
                    rec.steps[part.index] += 1
        _hint.weights_changed()       # (the modules' packed weight copies are stale: set_pack_cache)
        return loss
