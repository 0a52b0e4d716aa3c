"""What FlowTrainer (train.py), ConditionalFlowTrainer (conditional.py) and ChainRunner (flow.py) have in common: the cached
one-launch re-pack of a list of engines (PackGroup) and the trainers' core (TrainerCore): model-wide flat arenas, the
data-parallel start, the device-side step state, the loss pair and the two fused clamp+Adam launchers."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib, dp


def slice_layout(sizes):
    """-> ([(begin, end) of every entry, back to back in the given order], total)"""
    slices, cursor = [], 0
    for n in sizes:
        slices.append((cursor, cursor + n))
        cursor += n
    return slices, cursor


def rank_seed(seed: int, rank: int) -> int:
    """the noise stream's seed on a rank: every rank of a data-parallel job draws its own stream (63 bits: an int64 tensor
    holds it)"""
    return (seed + 0x9E3779B97F4A7C15 * rank) & (2 ** 63 - 1)


class PackGroup:
    """one launch re-packs every engine of a list (hint_pack_group_*): the handle is built on first use and rebuilt whenever an
    arena or packed buffer moved"""

    def __init__(self, engines, device: torch.device):
        self.lib = _lib.load()
        self.engines, self.device = engines, device
        self._handle, self._key = None, None

    def close(self):
        if self._handle:
            self.lib.hint_pack_group_destroy(self._handle)
        self._handle, self._key = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, zero_buf=None, rng_state=None, opt_state=None):
        """with zero_buf / rng_state / opt_state the launch is a training step's prologue (hint_pack_group_run_ex): it also
        clears zero_buf, advances the step / noise counter and writes Adam's factors of that step to opt_state"""
        key = tuple((e.arena.data_ptr(), e.packed.data_ptr()) for e in self.engines)
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            if self._key != key:
                self.close()
                n = len(self.engines)
                plans = (C.c_void_p * n)(*[e.plan.value for e in self.engines])
                params = (C.c_void_p * n)(*[e.arena.data_ptr() for e in self.engines])
                packed = (C.c_void_p * n)(*[e.packed.data_ptr() for e in self.engines])
                handle = C.c_void_p()
                _lib.check(self.lib.hint_pack_group_create(plans, params, packed, n, C.byref(handle)), "hint_pack_group_create")
                self._handle, self._key = handle, key
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if zero_buf is not None or rng_state is not None:
                st = self.lib.hint_pack_group_run_ex(self._handle, ptr(zero_buf), zero_buf.numel() if zero_buf is not None else 0,
                                                     ptr(rng_state), ptr(opt_state), stream)
            else:
                st = self.lib.hint_pack_group_run(self._handle, stream)
        _lib.check(st, "hint_pack_group_run")


class _LossPair:
    """what step() returns on every path: unpacks to the two loss terms as DEVICE SCALARS (torch tensors: `l0 + l1`,
    `sum(batch_losses)`, `torch.stack`, `.item()` all work), evaluated when it is unpacked so that no torch kernel runs inside the
    step or its captured graph.  The sums live in a buffer the next step's prologue clears: unpack before stepping again
    (FlowTrainer.step and ConditionalFlowTrainer.step return the same type)."""

    def __init__(self, trainer):
        self._t = trainer

    def __iter__(self):
        return iter(self._t.last_losses())


class TrainerCore:
    """The state both trainers keep and the launches both make on it.  `engines` is the model's engines in arena order."""

    def __init__(self, flow, engines, device: torch.device, lr: float, betas, eps: float, weight_decay: float, grad_clamp: float,
                 noise: float, use_graph: bool, group, seed: Optional[int], learned_perms: bool = False):
        from .householder import trainable        # (householder.py imports hint.py: not at module level here)
        learned = [m for m in flow.modules() if trainable(m)]
        if learned and not learned_perms:
            # (the chained backward does not emit dL/dW of a permutation; FlowTrainer's block-by-block route does, on request)
            raise _lib.HintAmdError(f"{type(self).__name__}: the model has trainable Householder permutations (learned_perms=True), "
                                    "which the fused step does not train; use the module route - loss.backward() and "
                                    "hint_amd.ClampAdam over model.parameters() - for such a model, or, for a HintFlow, "
                                    "FlowTrainer(flow, learned_perms=True)")
        self.lib = _lib.load()
        self.flow, self.device, self.group = flow, device, group
        self._lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.grad_clamp, self.noise = grad_clamp, noise
        self.use_graph = use_graph
        self.step_count = 0
        self._last_B = None                     # rows of the most recent step (last_losses)
        # model-wide arenas (parameters / gradients / Adam moments); every engine is bound to its slice
        self.engines = engines
        self.slices, self.n_floats = slice_layout([e.total for e in engines])
        # the trainable permutations' Vs (all [n, d], FlowTrainer(learned_perms=True)) lie behind every block slice, perm_stride
        # floats apart: block offsets are those of a model without them, and the arena-wide clamp + Adam steps them as well
        self.perm_mods = learned
        self.perm_base = self.n_floats
        self.perm_stride = -(-learned[0].Vs.numel() // 4) * 4 if learned else 0
        self.n_floats += len(learned) * self.perm_stride
        self.P, self.G, self.M, self.V = (torch.zeros(self.n_floats, dtype=torch.float32, device=device) for _ in range(4))
        for e, (a, b) in zip(engines, self.slices):
            e.bind_external_arena(self.P[a:b])
            e.ensure_arena()
            e.pack()
        self._bind_perms()
        rank, world = dp.world_info(group)
        if world > 1:
            # data-parallel replicas must start from the same weights (the reference idiom
            # p.data = init_scale*randn_like(p) draws per-process values): rank 0's win; M and V are zero
            src = torch.distributed.get_global_rank(group, 0) if group is not None else 0
            torch.distributed.broadcast(self.P, src=src, group=group)
            # ... and from the same buffers: the fixed permutations between the blocks and the node permutations of
            # reshuffle=True trees are drawn per process as well (hint.py:36-39 / power_hint_8.py:59-62), and the
            # kernels read them - replicas with different matrices would sum gradients of different functions
            for buf in flow.buffers():
                if buf.is_cuda and buf.numel() > 0:
                    torch.distributed.broadcast(buf, src=src, group=group)
            for e in engines:
                e._perm_key = None         # (composed permutations are rebuilt from the received matrices)
                e.pack()
        self.loss_acc = torch.zeros(64, 2, dtype=torch.float32, device=device)   # per-slot partial loss sums
        # device-side step state.  rng_state = {seed, step}: the in-kernel noise generator's, and the step count the re-pack
        # launch's prologue advances.  opt_state = {lr, beta1, beta2, lr/(1-beta1^t), 1/sqrt(1-beta2^t), ...}: Adam's
        # hyper-parameters and per-step factors, written by that prologue and read by the captured optimizer launches
        # (hint_adam_step_dev and the fused reductions), so nothing in a graph depends on the host's step count
        if seed is None:            # (not from torch's global generator: building a trainer must not shift the caller's random stream)
            seed = int.from_bytes(os.urandom(8), "little") >> 2
        self.rng_state = torch.tensor([rank_seed(seed, rank), 0], dtype=torch.int64, device=device)
        self.opt_state = torch.tensor([lr, betas[0], betas[1], 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    def perm_slice(self, j: int, arena: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the [n, d] view of trainable permutation j's slice of an arena (default: P)"""
        m = self.perm_mods[j]
        a = self.perm_base + j * self.perm_stride
        return (self.P if arena is None else arena)[a:a + m.n * m.d].view(m.n, m.d)

    def _bind_perms(self) -> bool:
        """every trainable permutation's Vs.data is a view of its P slice; one rebound from outside (p.data = ..., .to()) is
        copied back in.  -> whether any was"""
        moved = False
        for j, m in enumerate(self.perm_mods):
            view = self.perm_slice(j)
            if m.Vs.data_ptr() != view.data_ptr() or m.Vs.device != self.device:
                if m.Vs.dtype != torch.float32:
                    raise _lib.HintAmdError("hint_amd kernels are fp32 only (parameter dtype %s)" % m.Vs.dtype)
                with torch.no_grad():
                    view.copy_(m.Vs.data.to(self.device))
                    m.Vs.data = view
                moved = True
        return moved

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):          # learning-rate schedules (train_unconditional.py:191-199) need no re-capture:
        self._lr = float(value)
        self.opt_state[0:1].fill_(self._lr)     # the captured optimizer launches read it on the device (fill_: no host copy, so a
                                                # schedule that sets it every step never waits for the stream)

    def last_losses(self):
        """the two loss terms (0.5 |z|^2 mean = -log p(z), -log|det J| mean) of the most recent step's local shard as device
        scalars (train_unconditional.py:162 labels).  The sums live in a buffer the next step's prologue clears: read them
        before stepping again."""
        s = self.loss_acc.sum(dim=0)
        return s[0] / self._last_B, -s[1] / self._last_B

    @staticmethod
    def _dist_on() -> bool:
        return torch.distributed.is_available() and torch.distributed.is_initialized()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the fused clamp+Adam launch over the whole arena; scale = 1/world turns the all-reduced sum into the mean ----
    def _adam_host(self, scale: float):
        """stepped by the host: Adam's factors come from step_count, which this advances"""
        self.step_count += 1
        with torch.cuda.device(self.device):
            st = self.lib.hint_adam_step(self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.V.data_ptr(),
                                         self.n_floats, self.step_count, self.lr, self.betas[0], self.betas[1],
                                         self.eps, self.wd, scale, self.grad_clamp, 1, self._stream())
        _lib.check(st, "hint_adam_step")

    def _adam_dev(self, scale: float = 1.0):
        """stepped on the device: the factors are read from opt_state (capturable: nothing in it depends on the host's step
        count)"""
        with torch.cuda.device(self.device):
            st = self.lib.hint_adam_step_dev(self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.V.data_ptr(),
                                             self.n_floats, self.opt_state.data_ptr(), self.betas[0], self.betas[1],
                                             self.eps, self.wd, scale, self.grad_clamp, 1, self._stream())
        _lib.check(st, "hint_adam_step_dev")

    def _adam_warm_load(self):
        """loads the optimizer kernel with a launch outside a capture (on a 4 x 4 scratch)"""
        scratch = torch.zeros(4, 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.lib.hint_adam_step(scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr(),
                                    scratch[3].data_ptr(), 4, 1, 0.0, 0.9, 0.95, 1e-4, 0.0, 1.0, 0.0, 0, self._stream())
