"""Device-resident epochs (hint_amd/csrc/hint_epoch.hip): what stands between a data set and the training step.

    DeviceDataset(x, y)                     TensorDataset(x, y) resident on the device                  data.py:484-487, :503-506
      .gather(epoch, first_batch, n, B)     n shuffled batches of DataLoader(shuffle=True, drop_last=True), one launch
      .standardize() / .moments()           (x - mean) / std with np.mean / np.std of chosen rows        data.py:337-339
      .split(n_train), .n_batches(B)
    epoch_indices(n_rows, seed, epoch, first, count)    the source rows of an epoch's positions
    reference_lr(epoch, ...)                the learning rate main(c) trains an epoch with               train_unconditional.py:177-201

THE ORDER OF AN EPOCH IS THIS LIBRARY'S DEFINITION (include/hint_amd.h hint_epoch_desc states it): a keyed permutation, a function
of (n_rows, seed, epoch, position) alone - the reference's order is torch's host generator and cannot be pinned.  Chunks of an
epoch at any boundaries have the bits of one call, a data-parallel rank computes its own shard with no communication, and a run
resumes mid-epoch from (seed, epoch, first_batch).  FlowTrainer.fit_epoch / .evaluate and ConditionalFlowTrainer.fit_epoch run on
it.  Nothing here synchronises the host; there is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import HintAmdError
from ._ops import _check_device, _check_int, _check_no_grad, _run_desc

__all__ = ["DeviceDataset", "epoch_indices", "reference_lr"]

MAX_ROWS = 1 << 40
MAX_D = 128
_F32, _F64, _I64 = torch.float32, torch.float64, torch.int64


def _check_table(t, name: str, who: str, rows: Optional[int] = None) -> torch.Tensor:
    """a resident table: a floating [N, d] device tensor, 1 <= d <= 128 -> fp32 with unit column stride (a column slice of a wider
    table stays the view it is; anything else is copied once)"""
    if not isinstance(t, torch.Tensor):
        raise HintAmdError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[0] > MAX_ROWS or t.shape[1] < 1 or t.shape[1] > MAX_D:
        raise HintAmdError(f"{who}: {name} must be [1..{MAX_ROWS}, 1..{MAX_D}] (got shape {tuple(t.shape)})")
    if rows is not None and t.shape[0] != rows:
        raise HintAmdError(f"{who}: {name} holds {t.shape[0]} rows and x {rows}")
    if not t.is_cuda:
        raise HintAmdError(f"{who}: {name} is on {t.device}; the data set lives on a GPU and there is no CPU fallback")
    if not t.is_floating_point():
        raise HintAmdError(f"{who}: {name} is {t.dtype}; expected a floating-point tensor")
    _check_no_grad(t, name, who)
    t = t.detach()
    if t.dtype != _F32:
        t = t.to(_F32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) > (1 << 22):
        t = t.contiguous()
    return t


def shard_positions(first_batch: int, n: int, batch_size: int, rank: int, world: int):
    """(first, count, block, block_stride) of hint_epoch_desc for rank `rank` of `world` and global batches first_batch ..
    first_batch + n - 1: global batch g covers positions [g B world, (g + 1) B world), the rank the rank-th B of them"""
    first = (first_batch * world + rank) * batch_size
    return (first, n * batch_size, 0, 0) if world == 1 else (first, n * batch_size, batch_size, batch_size * world)


def _gather_run(x, y, n_rows: int, seed: int, epoch: int, shuffle: bool, pos, dev, want=("out_x",), cursor=None, out=None,
                max_groups: int = 0):
    """one hint_epoch_run gather on checked arguments; pos = (first, count, block, block_stride).  -> dict of the outputs named in
    `want` (out_x [count, d], out_y [count, dy], indices_out [count]) and the workspace (`out`: buffers to use, by those names)"""
    first, count, block, stride = pos
    desc = _lib.EpochDesc()
    desc.op, desc.shuffle, desc.epoch, desc.max_groups = _lib.EPOCH_GATHER, int(bool(shuffle)), epoch, max_groups
    desc.n_rows, desc.seed, desc.first, desc.count, desc.block, desc.block_stride = n_rows, seed, first, count, block, stride
    desc.d = x.shape[1] if x is not None else 1
    res = {}

    def buf(name, shape, dtype):
        res[name] = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
        return res[name].data_ptr()

    if x is not None:
        desc.x, desc.x_stride = x.data_ptr(), x.stride(0)
        desc.out_x = buf("out_x", (count, x.shape[1]), _F32)
    if y is not None and "out_y" in want:
        desc.y, desc.y_stride, desc.dy = y.data_ptr(), y.stride(0), y.shape[1]
        desc.out_y = buf("out_y", (count, y.shape[1]), _F32)
    if "indices_out" in want:
        desc.indices_out = buf("indices_out", (count,), _I64)
    desc.cursor = cursor.data_ptr() if cursor is not None else None
    res["workspace"] = _run_desc("hint_epoch_run", desc, dev, (_lib.EPOCH_GATHER, n_rows, count, desc.d), out)
    return res


def _check_cursor(cursor, dev, who: str):
    if cursor is None:
        return None
    if not isinstance(cursor, torch.Tensor) or cursor.dtype != _I64 or cursor.shape != (2,) or cursor.device != dev \
            or not cursor.is_contiguous():
        raise HintAmdError(f"{who}: cursor must be a contiguous int64 tensor [2] = (epoch, first) on {dev}")
    return cursor


class DeviceDataset:
    """x [N, d] (and y [N, dy]) as resident fp32 device tensors, with a keyed shuffle: seed (0 .. 2^64 - 1) and the epoch number fix
    the order of an epoch; shuffle=False keeps the rows' order.  The tensors are used in place (a column slice of a wider table
    stays a view); they are copied only where they are not fp32 with unit column stride."""

    def __init__(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, seed: int = 0, shuffle: bool = True):
        who = "DeviceDataset"
        self.x = _check_table(x, "x", who)
        self.y = _check_table(y, "y", who, rows=self.x.shape[0]) if y is not None else None
        if self.y is not None and self.y.device != self.x.device:
            raise HintAmdError(f"{who}: y is on {self.y.device} and x on {self.x.device}")
        self.seed = _check_int(seed, "seed", who, 0, 2 ** 64 - 1)
        if not isinstance(shuffle, bool):
            raise HintAmdError(f"{who}: shuffle must be a bool (got {type(shuffle).__name__})")
        self.shuffle = shuffle
        self.last_workspace = None               # the latest gather's int32 words: their sum is the rows it rejected

    n_rows = property(lambda self: self.x.shape[0])
    d = property(lambda self: self.x.shape[1])
    dy = property(lambda self: self.y.shape[1] if self.y is not None else 0)
    device = property(lambda self: self.x.device)

    def __len__(self) -> int:
        return self.x.shape[0]

    def n_batches(self, batch_size: int, world: int = 1) -> int:
        """global batches of an epoch: N // (batch_size * world), the tail dropped (drop_last=True)"""
        batch_size = _check_int(batch_size, "batch_size", "DeviceDataset.n_batches", 1, MAX_ROWS)
        world = _check_int(world, "world", "DeviceDataset.n_batches", 1, 1 << 20)
        return self.n_rows // (batch_size * world)

    def split(self, n_train: int):
        """(rows [0, n_train), rows [n_train, N)) as data sets that are views of this one, with its seed and shuffle"""
        n_train = _check_int(n_train, "n_train", "DeviceDataset.split", 1, self.n_rows - 1)
        cut = lambda t, a, b: t[a:b] if t is not None else None     # noqa: E731
        return tuple(DeviceDataset(self.x[a:b], cut(self.y, a, b), self.seed, self.shuffle)
                     for a, b in ((0, n_train), (n_train, self.n_rows)))

    # ---- statistics ----------------------------------------------------------------------------------------------------
    def _rows(self, row0, rows, who: str):
        row0 = _check_int(row0, "row0", who, 0, self.n_rows - 1)
        rows = self.n_rows - row0 if rows is None else _check_int(rows, "rows", who, 1, self.n_rows - row0)
        return row0, rows

    def _stat_desc(self, op: int, row0: int, rows: int, mean: torch.Tensor, std: torch.Tensor):
        desc = _lib.EpochDesc()
        desc.op, desc.n_rows, desc.d, desc.first, desc.count = op, self.n_rows, self.d, row0, rows
        desc.x, desc.x_stride = self.x.data_ptr(), self.x.stride(0)
        desc.mean, desc.std = mean.data_ptr(), std.data_ptr()
        return desc

    def moments(self, row0: int = 0, rows: Optional[int] = None, out=None):
        """(mean [d], std [d]) of x's columns over rows [row0, row0 + rows) as double device tensors: np.mean and np.std (ddof 0) in
        double, two passes in a fixed order"""
        row0, rows = self._rows(row0, rows, "DeviceDataset.moments")
        mean = out["mean"] if out is not None and "mean" in out else torch.empty(self.d, dtype=_F64, device=self.device)
        std = out["std"] if out is not None and "std" in out else torch.empty(self.d, dtype=_F64, device=self.device)
        desc = self._stat_desc(_lib.EPOCH_MOMENTS, row0, rows, mean, std)
        _run_desc("hint_epoch_run", desc, self.device, (_lib.EPOCH_MOMENTS, self.n_rows, rows, self.d), out)
        return mean, std

    def apply_moments(self, mean: torch.Tensor, std: torch.Tensor, row0: int = 0, rows: Optional[int] = None, out=None):
        """x[i, j] = (float)(((double)x[i, j] - mean[j]) / std[j]) over rows [row0, row0 + rows), in place (out: a table of x's
        shape to write instead).  mean, std: double [d] device tensors - the statistics of other rows, or of another data set
        (train+val statistics on the test rows, as load_data_normalised applies them)"""
        who = "DeviceDataset.apply_moments"
        row0, rows = self._rows(row0, rows, who)
        for name, t in (("mean", mean), ("std", std)):
            if not isinstance(t, torch.Tensor) or t.dtype != _F64 or t.shape != (self.d,) or t.device != self.device \
                    or not t.is_contiguous():
                raise HintAmdError(f"{who}: {name} must be a contiguous float64 tensor [{self.d}] on {self.device}")
        dst = self.x if out is None else out
        if dst is not self.x and (not isinstance(dst, torch.Tensor) or dst.dtype != _F32 or dst.shape != self.x.shape
                                  or dst.device != self.device or dst.stride(1) != 1 or dst.stride(0) < self.d):
            raise HintAmdError(f"{who}: out must be an fp32 tensor {tuple(self.x.shape)} on {self.device} with unit column stride")
        desc = self._stat_desc(_lib.EPOCH_STANDARDIZE, row0, rows, mean, std)
        desc.out_x, desc.out_stride = dst.data_ptr(), dst.stride(0)
        _run_desc("hint_epoch_run", desc, self.device, (_lib.EPOCH_STANDARDIZE, self.n_rows, rows, self.d))
        return dst

    def standardize(self, stats_rows=None):
        """x <- (x - mean) / std in place over ALL rows, the statistics taken from rows stats_rows = (row0, rows) (default: all
        rows) - data.py:337-339 takes them from train+val.  -> (mean, std) as double device tensors.  A constant column divides
        by zero as numpy does (NaN, +-inf)"""
        if stats_rows is None:
            stats_rows = (0, self.n_rows)
        if not isinstance(stats_rows, (tuple, list)) or len(stats_rows) != 2:
            raise HintAmdError(f"DeviceDataset.standardize: stats_rows must be (row0, rows) (got {stats_rows!r})")
        mean, std = self.moments(stats_rows[0], stats_rows[1])
        self.apply_moments(mean, std)
        return mean, std

    # ---- batches -------------------------------------------------------------------------------------------------------
    def _batch_args(self, epoch, first_batch, n, batch_size, rank, world, who: str):
        epoch = _check_int(epoch, "epoch", who, 0, 2 ** 32 - 1)
        batch_size = _check_int(batch_size, "batch_size", who, 1, MAX_ROWS)
        world = _check_int(world, "world", who, 1, 1 << 20)
        rank = _check_int(rank, "rank", who, 0, world - 1)
        total = self.n_rows // (batch_size * world)
        if total < 1:
            raise HintAmdError(f"{who}: {self.n_rows} rows hold no batch of {batch_size} x {world} rows")
        first_batch = _check_int(first_batch, "first_batch", who, 0, total - 1)
        n = _check_int(n, "n", who, 1, total - first_batch)
        return epoch, first_batch, n, batch_size, rank, world

    def gather(self, epoch: int, first_batch: int, n: int, batch_size: int, rank: int = 0, world: int = 1, out=None,
               cursor: Optional[torch.Tensor] = None):
        """batches first_batch .. first_batch + n - 1 of epoch `epoch` as xs [n, B, d] - with y, (xs [n, B, d], ys [n, B, dy]) -
        written by ONE launch on the current stream.  Of `world` ranks, rank `rank` takes the rank-th B rows of every global batch
        of B * world.  out: the tensor(s) to write, e.g. a trainer's own input buffers.  cursor: an int64 [2] device tensor
        (epoch, first position) read by the kernel in place of epoch and first_batch - a captured gather replays at a new place
        after cursor.copy_ / fill_; rows it puts past the end are NaN and counted in `last_workspace` (int32 words, their sum)"""
        who = "DeviceDataset.gather"
        epoch, first_batch, n, B, rank, world = self._batch_args(epoch, first_batch, n, batch_size, rank, world, who)
        bufs = {}
        outs = (out,) if isinstance(out, torch.Tensor) else (tuple(out) if out is not None else ())
        if outs and len(outs) != (2 if self.y is not None else 1):
            raise HintAmdError(f"{who}: out must be {'(xs, ys)' if self.y is not None else 'xs'}")
        for name, t, w in zip(("out_x", "out_y"), outs, (self.d, self.dy)):
            if not isinstance(t, torch.Tensor) or t.dtype != _F32 or tuple(t.shape) != (n, B, w) or t.device != self.device \
                    or not t.is_contiguous():
                raise HintAmdError(f"{who}: out's {name[-1]}s must be a contiguous fp32 tensor [{n}, {B}, {w}] on {self.device}")
            bufs[name] = t
        res = _gather_run(self.x, self.y, self.n_rows, self.seed, epoch, self.shuffle, shard_positions(first_batch, n, B, rank, world),
                          self.device, want=("out_x", "out_y"), cursor=_check_cursor(cursor, self.device, who), out=bufs)
        self.last_workspace = res["workspace"].view(torch.int32)
        xs = res["out_x"].view(n, B, self.d)
        return xs if self.y is None else (xs, res["out_y"].view(n, B, self.dy))

    def indices(self, epoch: int, first: int, count: int) -> torch.Tensor:
        """the source rows of positions first .. first + count - 1 of epoch `epoch`, int64 [count]"""
        return epoch_indices(self.n_rows, self.seed, epoch, first, count, self.device, shuffle=self.shuffle)


def epoch_indices(n_rows: int, seed: int, epoch: int, first: int, count: int, device=None, shuffle: bool = True) -> torch.Tensor:
    """the source rows of positions first .. first + count - 1 of an epoch of a data set of n_rows rows, int64 [count] on the
    device: what DeviceDataset(x, seed=seed).gather reads, without the rows"""
    who = "epoch_indices"
    n_rows = _check_int(n_rows, "n_rows", who, 1, MAX_ROWS)
    seed = _check_int(seed, "seed", who, 0, 2 ** 64 - 1)
    epoch = _check_int(epoch, "epoch", who, 0, 2 ** 32 - 1)
    first = _check_int(first, "first", who, 0, n_rows - 1)
    count = _check_int(count, "count", who, 1, n_rows - first)
    dev = _check_device(device, who)
    return _gather_run(None, None, n_rows, seed, epoch, shuffle, (first, count, 0, 0), dev, want=("indices_out",))["indices_out"]


def reference_lr(epoch: int, lr_init: float, n_epochs: int, final_decay: float, pre_low_lr: int = 0) -> float:
    """the learning rate main(c) trains epoch `epoch` (0-based) with (train_unconditional.py:177-201): Adam at lr_init, a
    StepLR(step_size=1, gamma=final_decay ** (1 / n_epochs)) stepped after every epoch, and the group's lr OVERWRITTEN with
    lr_init * 3e-2 at the start of each of the first pre_low_lr epochs.  StepLR.step() multiplies whatever the group holds, so the
    overwritten value is what decays from then on: the run never returns to lr_init -
        epoch < pre_low_lr:   lr_init * 3e-2
        otherwise:            (lr_init * 3e-2 if pre_low_lr > 0 else lr_init) * gamma ** (epoch - max(pre_low_lr - 1, 0))
    (the products taken one at a time, as the scheduler takes them)"""
    who = "reference_lr"
    n_epochs = _check_int(n_epochs, "n_epochs", who, 1, 1 << 30)
    epoch = _check_int(epoch, "epoch", who, 0, 1 << 30)
    pre_low_lr = _check_int(pre_low_lr, "pre_low_lr", who, 0, 1 << 30)
    gamma = float(final_decay) ** (1.0 / n_epochs)
    lr = float(lr_init)
    for e in range(epoch + 1):
        if e < pre_low_lr:
            lr = float(lr_init) * 3e-2
        if e == epoch:
            return lr
        lr = lr * gamma
    return lr
