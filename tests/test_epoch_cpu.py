"""CPU-side checks of the device-resident epochs (no GPU): hint_epoch_index - the host's twin of the kernel's permutation, compiled
from the same header - equals tests/epoch_oracle.py exactly; the map is a bijection, moves, differs between epochs and seeds and is
uniform; header, exports and binding agree with the ABI still 8; every host check of hint_epoch_run comes before any device call and
names its field; the workspace is monotone and under its stated bound; the sharding arithmetic; reference_lr against a real Adam +
StepLR driven as main(c) drives them; and hint_epochperm.hpp alone under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, data
from hint_amd._lib import HintAmdError
from fake_device import OnGpu
import epoch_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_epoch_index", "hint_epoch_workspace_bytes", "hint_epoch_run")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
MAX_N, WS_BOUND = 1 << 40, 1 << 20
FIELDS = ("op", "shuffle", "d", "dy", "epoch", "max_groups", "n_rows", "seed", "first", "count", "block", "block_stride", "x",
          "x_stride", "y", "y_stride", "cursor", "out_x", "out_stride", "out_y", "indices_out", "mean", "std", "workspace",
          "workspace_bytes", "stream")
EPOCHS = (0, 1, 2 ** 32 - 1)
SEEDS = (0, 1, 2 ** 64 - 1)
BIG = (1024, 1025, 4096, 4097, 65537, 2 ** 40)


def big_positions(n):
    """0, 1, N // 2, N - 2, N - 1 and 64 fixed others (tools/epochperm_check.cpp walks the same)"""
    return [0, 1 % n, n // 2, max(n - 2, 0), n - 1] + [((k * 0x9E3779B97F4A7C15 % 2 ** 64) >> 11) % n for k in range(1, 65)]


def host_index(n, seed, epoch, positions, shuffle=1):
    lib = _lib.load()
    return np.array([lib.hint_epoch_index(n, seed, epoch, shuffle, int(p)) for p in positions], dtype=np.int64)


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    for cite in ("data.py:484-487", ":503-506", "data.py:337-339"):
        assert cite in header, cite
    assert "THE ORDER OF AN EPOCH IS THIS LIBRARY'S DEFINITION" in header
    assert "#define HINT_AMD_ABI_VERSION 8" in header and lib.hint_abi_version() == _lib.ABI_VERSION == 8
    assert re.search(r"int hint_epoch_run\(const hint_epoch_desc\* desc\);", header)        # the stream is not a parameter
    assert re.search(r"int64_t hint_epoch_index\(int64_t n_rows, uint64_t seed, uint32_t epoch, int32_t shuffle, int64_t pos\);", header)
    # the definition is the header's, word for word what hint_epochperm.hpp implements
    for text in ("h = max(1, ceil(bitlength(N-1) / 2))", "(L, R) -> (R, L ^ F_r(R))", "{R, r, epoch, 0x45504F43}",
                 "v = p; do v = feistel(v); while (v >= N)", "capped at 256 applications", "the loop never runs on"):
        assert text in header, text
    P = _lib.EpochDesc
    assert C.sizeof(P) == 184
    assert [getattr(P, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20] + list(range(24, 184, 8))
    body = re.search(r"typedef struct hint_epoch_desc \{(.*?)\} hint_epoch_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in P._fields_] == list(FIELDS), names
    assert (_lib.EPOCH_GATHER, _lib.EPOCH_MOMENTS, _lib.EPOCH_STANDARDIZE) == (0, 1, 2)
    for k, v in (("GATHER", 0), ("MOMENTS", 1), ("STANDARDIZE", 2)):
        assert f"#define HINT_EPOCH_{k} {v}" in header
    for name in data.__all__:
        assert getattr(hint_amd, name) is getattr(data, name)
    assert set(data.__all__) == {"DeviceDataset", "epoch_indices", "reference_lr"}
    mk = open(os.path.join(ROOT, "hint_amd", "csrc", "Makefile")).read()
    assert "hint_epoch.hip" in mk and "hint_epochperm.hpp" in mk
    for fn in ("fit_epoch", "evaluate"):
        assert callable(getattr(hint_amd.FlowTrainer, fn))
    assert callable(hint_amd.ConditionalFlowTrainer.fit_epoch) and not hasattr(hint_amd.ConditionalFlowTrainer, "evaluate")


def test_host_twin_equals_the_oracle_on_every_position_of_small_tables():
    for n in range(1, 301):
        for epoch, seed in ((0, 0), (1, 2 ** 64 - 1), (2 ** 32 - 1, 1)):
            want = eo.epoch_order(n, seed, epoch)
            got = host_index(n, seed, epoch, range(n))
            assert (got == want).all(), (n, epoch, seed)
            assert sorted(got.tolist()) == list(range(n)), (n, epoch, seed)
    for n in (1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 300):             # ... and over the whole grid of epochs and seeds
        for epoch in EPOCHS:
            for seed in SEEDS:
                assert (host_index(n, seed, epoch, range(n)) == eo.epoch_order(n, seed, epoch)).all(), (n, epoch, seed)


def test_host_twin_equals_the_oracle_on_large_tables():
    for n in BIG:
        pos = big_positions(n)
        assert len(pos) == 69 and all(0 <= p < n for p in pos)
        for epoch in EPOCHS:
            for seed in SEEDS:
                want = eo.source_rows(n, seed, epoch, pos)
                got = host_index(n, seed, epoch, pos)
                assert (got == want).all() and (got >= 0).all() and (got < n).all(), (n, epoch, seed)
    assert eo.half_bits(1) == 1 and eo.half_bits(2) == 1 and eo.half_bits(4) == 1 and eo.half_bits(5) == 2
    assert eo.half_bits(1024) == 5 and eo.half_bits(1025) == 6 and eo.half_bits(2 ** 40) == 20
    for n in list(range(2, 300)) + list(BIG):
        M = 4 ** eo.half_bits(n)
        assert n <= M < 4 * n, (n, M)


def test_bijection_and_the_longest_walk():
    """every N <= 5000 at one (seed, epoch); the tables of one h are walked together"""
    longest, at = 0, None
    by_h = {}
    for n in range(1, 5001):
        by_h.setdefault(eo.half_bits(n), []).append(n)
    for h, ns in sorted(by_h.items()):
        pos = np.concatenate([np.arange(n, dtype=np.uint64) for n in ns])
        per = np.concatenate([np.full(n, n, dtype=np.uint64) for n in ns])
        rows, steps = eo.source_rows(per, 7, 3, pos, with_steps=True)
        assert (rows >= 0).all()
        a = 0
        for n in ns:
            assert (np.sort(rows[a:a + n]) == np.arange(n)).all(), n
            if steps[a:a + n].max() > longest:
                longest, at = int(steps[a:a + n].max()), n
            a += n
    assert (eo.source_rows(np.full(300, 300, dtype=np.uint64), 7, 3, np.arange(300)) == eo.epoch_order(300, 7, 3)).all()
    print(f"longest walk over N = 1..5000 at (seed 7, epoch 3): {longest} applications, at N = {at}")
    assert 1 <= longest <= eo.WALK_CAP


def test_the_map_moves_and_differs_between_epochs_and_seeds():
    for n in (8, 9, 16, 100, 1000, 4097):
        ident = np.arange(n)
        orders = [eo.epoch_order(n, 0, e) for e in range(10)]
        assert all((o != ident).any() for o in orders), n
        assert len({o.tobytes() for o in orders}) == 10, n
        seeds = [eo.epoch_order(n, s, 0) for s in range(10)]
        assert all((o != ident).any() for o in seeds), n
        assert len({o.tobytes() for o in seeds}) == 10, n
    lib = _lib.load()
    assert [lib.hint_epoch_index(100, 0, e, 1, 5) for e in range(10)] == [int(eo.source_rows(100, 0, e, [5])[0]) for e in range(10)]


def test_uniformity_of_position_0_over_4096_epochs():
    """N = 16, seed 0: binomial(4096, 1/16) = 256 +- 6 * 15.49 -> every bin 163 .. 349"""
    img = np.array([eo.source_rows(16, 0, e, [0])[0] for e in range(4096)])
    counts = np.bincount(img, minlength=16)
    print("bins:", counts.tolist())
    assert len(counts) == 16 and counts.min() >= 163 and counts.max() <= 349, counts.tolist()
    assert (host_index(16, 0, 17, [0]) == img[17]).all()


def test_shuffle_0_is_the_identity_and_bad_arguments_return_minus_1():
    lib = _lib.load()
    for n in (1, 2, 17, 4097, 2 ** 40):
        pos = big_positions(n)
        assert (host_index(n, 5, 3, pos, shuffle=0) == np.array(pos)).all()
        assert (eo.source_rows(n, 5, 3, pos, shuffle=False) == np.array(pos)).all()
    for args, text in (((0, 0, 0, 1, 0), "n_rows must be 1..1099511627776 (got 0)"),
                       ((-4, 0, 0, 1, 0), "n_rows must be 1..1099511627776 (got -4)"),
                       ((2 ** 40 + 1, 0, 0, 1, 0), "n_rows must be 1..1099511627776"),
                       ((10, 0, 0, 1, 10), "pos must be 0..n_rows - 1 = 9 (got 10)"),
                       ((10, 0, 0, 1, -1), "pos must be 0..n_rows - 1 = 9 (got -1)"),
                       ((10, 0, 0, 0, 10), "pos must be 0..n_rows - 1 = 9 (got 10)")):
        assert lib.hint_epoch_index(*args) == -1
        assert text in lib.hint_last_error().decode(), (args, lib.hint_last_error())


# ---- hint_epoch_run's host checks ----
def epoch_desc(op=0, n=1000, count=256, d=6, dy=0):
    lib = _lib.load()
    e = _lib.EpochDesc()
    e.op, e.shuffle, e.d, e.dy, e.epoch, e.n_rows, e.seed, e.first, e.count = op, 1, d, dy, 3, n, 7, 0, count
    e.x, e.x_stride, e.out_x, e.out_stride, e.workspace = BASE, d, BASE + (1 << 32), d, BASE + (2 << 32)
    if dy:
        e.y, e.y_stride, e.out_y = BASE + (3 << 32), dy, BASE + (4 << 32)
    if op != 0:
        e.mean, e.std = BASE + (5 << 32), BASE + (6 << 32)
    e.workspace_bytes = lib.hint_epoch_workspace_bytes(op, n, count, d)
    assert e.workspace_bytes > 0
    return e


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_epoch_run(C.byref(desc) if desc is not None else None)
    return st, (lib.hint_last_error() or b"").decode()


def refused(text, op=0, dy=0, **fields):
    e = epoch_desc(op=op, dy=dy)
    for k, v in fields.items():
        setattr(e, k, v)
    st, msg = run_msg(e)
    assert st != 0 and text in msg, (fields, text, msg)


def test_epoch_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "hint_epoch_run: desc is null" in msg, msg
    for op in (0, 1, 2):
        refused("workspace is null", op=op, workspace=None)
        refused("n_rows must be 1..1099511627776 (got 0)", op=op, n_rows=0)
        refused("n_rows must be 1..1099511627776", op=op, n_rows=MAX_N + 1)
        refused("count must be 1..n_rows = 1000 (got 0)", op=op, count=0)
        refused("count must be 1..n_rows = 1000 (got 1001)", op=op, count=1001)
        refused("d must be 1..128 (got 0)", op=op, d=0)
        refused("d must be 1..128 (got 129)", op=op, d=129)
        refused("max_groups must be >= 0", op=op, max_groups=-1)
        refused("x is null", op=op, x=None)
        refused("x_stride must be 0..4194304 floats (got -1)", op=op, x_stride=-1)
        refused("x_stride must be 0..4194304 floats", op=op, x_stride=(1 << 22) + 1)
        refused("first must be >= 0 (got -1)", op=op, first=-1)
        refused("first + count must be <= n_rows", op=op, first=745)
        refused("first + count must be <= n_rows", op=op, first=1000)
        refused("x must be 4-byte aligned", op=op, x=BASE + 2)
        refused("workspace must be 16-byte aligned", op=op, workspace=BASE + (2 << 32) + 8)
    for bad in (3, -1):
        e = epoch_desc()
        e.op = bad
        st, msg = run_msg(e)
        assert st != 0 and f"op must be 0 (gather), 1 (moments) or 2 (standardize) (got {bad})" in msg, msg
    # gather
    refused("dy must be 0..128 (got -1)", dy=-1)
    refused("dy must be 0..128 (got 129)", dy=129)
    refused("out_x is null", out_x=None)
    refused("y and dy must be given together (dy = 4)", dy=4, y=None)
    refused("y and dy must be given together (dy = 0)", y=BASE + (3 << 32))
    refused("out_y is null", dy=4, out_y=None)
    refused("y_stride must be 0..4194304 floats (got -2)", dy=4, y_stride=-2)
    refused("block must be 0 (contiguous positions) or 1..block_stride", block=-1)
    refused("block must be 0 (contiguous positions) or 1..block_stride", block=64, block_stride=63)
    refused("block must be 0 (contiguous positions) or 1..block_stride", block_stride=-5)
    refused("first + count must be <= n_rows", block=64, block_stride=2 ** 40)
    refused("first + count must be <= n_rows", cursor=BASE + (7 << 32), block=64, block_stride=400)     # the offset alone is past the end
    refused("x is null (a gather of indices_out alone may leave it out)", x=None, indices_out=BASE + (8 << 32), dy=4)
    for field, align in (("y", 4), ("out_x", 4), ("out_y", 4), ("cursor", 8), ("indices_out", 8)):
        refused(f"{field} must be {align}-byte aligned", dy=4, **{field: BASE + (9 << 32) + align // 2})
    # moments, standardize
    for op in (1, 2):
        refused("mean and std must be given", op=op, mean=None)
        refused("mean and std must be given", op=op, std=None)
        for field in ("mean", "std"):
            refused(f"{field} must be 8-byte aligned", op=op, **{field: BASE + (9 << 32) + 4})
    refused("out_x is null", op=2, out_x=None)
    refused("out_stride must be 6..4194304 floats (got 5)", op=2, out_stride=5)
    refused("out_x must be 4-byte aligned", op=2, out_x=BASE + 1)
    # at the limits themselves only the workspace size is left to refuse
    for op, n, count, d in ((0, 1000, 256, 6), (0, MAX_N, MAX_N, 128), (1, MAX_N, MAX_N, 128), (2, 1000, 1000, 1)):
        e = epoch_desc(op=op, n=n, count=count, d=d)
        e.workspace_bytes -= 1
        st, msg = run_msg(e)
        assert st != 0 and "workspace_bytes" in msg and "too small (hint_epoch_workspace_bytes" in msg, msg


def test_the_block_form_that_fits_is_not_refused_for_its_positions():
    """4 blocks of 64 at stride 256: the last position is 3 * 256 + 63 = 831 < 1000 - the next check (the workspace's size) speaks"""
    e = epoch_desc()
    e.block, e.block_stride, e.workspace_bytes = 64, 256, 0
    st, msg = run_msg(e)
    assert st != 0 and "too small" in msg, msg
    e = epoch_desc()
    e.block, e.block_stride, e.first, e.workspace_bytes = 64, 256, 169, 0          # 169 + 831 = 1000: one past the end
    st, msg = run_msg(e)
    assert st != 0 and "first + count must be <= n_rows" in msg, msg
    e.first = 168
    st, msg = run_msg(e)
    assert st != 0 and "too small" in msg, msg


def test_workspace_is_monotone_and_under_its_stated_bound():
    lib = _lib.load()
    for args, text in (((3, 10, 10, 6), "op must be"), ((0, 0, 1, 6), "n_rows must be"), ((0, 10, 11, 6), "count must be"),
                       ((0, 10, 0, 6), "count must be"), ((1, 10, 10, 0), "d must be"), ((2, 10, 10, 129), "d must be")):
        assert lib.hint_epoch_workspace_bytes(*args) == 0 and text in lib.hint_last_error().decode(), args
    counts = [1, 2, 63, 64, 65, 255, 256, 257, 4099, 65536, 10 ** 6, 524287, 524288, 524289, 10 ** 8, 2 ** 31 + 1, MAX_N]
    counts.sort()
    for op, bound in ((0, 32 << 10), (1, WS_BOUND), (2, 16)):
        for d in (1, 6, 128):
            sizes = [lib.hint_epoch_workspace_bytes(op, MAX_N, c, d) for c in counts]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and 16 <= s <= bound for s in sizes), (op, d, sizes)
    assert lib.hint_epoch_workspace_bytes(0, MAX_N, MAX_N, 128) == 32 << 10
    assert lib.hint_epoch_workspace_bytes(1, MAX_N, MAX_N, 128) == WS_BOUND
    assert lib.hint_epoch_workspace_bytes(0, 10, 1, 6) == 16 and lib.hint_epoch_workspace_bytes(1, 10, 1, 1) == 16


def test_python_wrappers_reject_bad_arguments_without_a_gpu():
    cpu = torch.zeros(5, 6)
    gpu = OnGpu(torch.zeros(50, 6))
    bad_calls = [
        (lambda: hint_amd.DeviceDataset([1.0]), "DeviceDataset: x must be a tensor (got list)"),
        (lambda: hint_amd.DeviceDataset(cpu), "DeviceDataset: x is on cpu"),
        (lambda: hint_amd.DeviceDataset(torch.zeros(5)), "x must be [1..1099511627776, 1..128] (got shape (5,))"),
        (lambda: hint_amd.DeviceDataset(torch.zeros(5, 129)), "x must be [1..1099511627776, 1..128]"),
        (lambda: hint_amd.DeviceDataset(torch.zeros(0, 6)), "x must be [1..1099511627776, 1..128]"),
        (lambda: hint_amd.DeviceDataset(OnGpu(torch.zeros(5, 6, dtype=torch.int32))), "x is torch.int32; expected a floating-point tensor"),
        (lambda: hint_amd.DeviceDataset(OnGpu(torch.zeros(5, 6, requires_grad=True))), "x requires grad"),
        (lambda: hint_amd.DeviceDataset(gpu, OnGpu(torch.zeros(49, 2))), "y holds 49 rows and x 50"),
        (lambda: hint_amd.DeviceDataset(gpu, torch.zeros(50, 2)), "y is on cpu"),
        (lambda: hint_amd.DeviceDataset(gpu, seed=-1), "seed must be 0..18446744073709551615 (got -1)"),
        (lambda: hint_amd.DeviceDataset(gpu, seed=1.5), "seed must be an int"),
        (lambda: hint_amd.DeviceDataset(gpu, shuffle=1), "shuffle must be a bool"),
        (lambda: hint_amd.DeviceDataset(gpu).n_batches(0), "batch_size must be 1.."),
        (lambda: hint_amd.DeviceDataset(gpu).n_batches(8, world=0), "world must be 1.."),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 1, 64), "50 rows hold no batch of 64 x 1 rows"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 1, 16, world=4), "50 rows hold no batch of 16 x 4 rows"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(-1, 0, 1, 8), "epoch must be 0..4294967295 (got -1)"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(2 ** 32, 0, 1, 8), "epoch must be 0..4294967295"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 6, 1, 8), "first_batch must be 0..5 (got 6)"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 4, 3, 8), "n must be 1..2 (got 3)"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 1, 8, rank=2, world=2), "rank must be 0..1 (got 2)"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 2, 8, out=cpu), "out's xs must be a contiguous fp32 tensor [2, 8, 6]"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 2, 8, out=(cpu, cpu)), "out must be xs"),
        (lambda: hint_amd.DeviceDataset(gpu).gather(0, 0, 2, 8, cursor=torch.zeros(2)), "cursor must be a contiguous int64 tensor [2]"),
        (lambda: hint_amd.DeviceDataset(gpu).moments(50, 1), "row0 must be 0..49 (got 50)"),
        (lambda: hint_amd.DeviceDataset(gpu).moments(40, 11), "rows must be 1..10 (got 11)"),
        (lambda: hint_amd.DeviceDataset(gpu).standardize(stats_rows=7), "stats_rows must be (row0, rows)"),
        (lambda: hint_amd.DeviceDataset(gpu).standardize(stats_rows=(0, 51)), "rows must be 1..50 (got 51)"),
        (lambda: hint_amd.DeviceDataset(gpu).apply_moments(torch.zeros(6), torch.zeros(6)), "mean must be a contiguous float64 tensor [6]"),
        (lambda: hint_amd.DeviceDataset(gpu).split(50), "n_train must be 1..49 (got 50)"),
        (lambda: hint_amd.epoch_indices(0, 0, 0, 0, 1), "n_rows must be 1..1099511627776 (got 0)"),
        (lambda: hint_amd.epoch_indices(10, 0, 0, 10, 1), "first must be 0..9 (got 10)"),
        (lambda: hint_amd.epoch_indices(10, 0, 0, 4, 7), "count must be 1..6 (got 7)"),
        (lambda: hint_amd.epoch_indices(10, 2 ** 64, 0, 0, 1), "seed must be 0.."),
        (lambda: hint_amd.epoch_indices(10, 0, 0, 0, 1, device="cpu"), "no CPU fallback"),
        (lambda: hint_amd.reference_lr(-1, 1e-2, 50, 0.1, 3), "epoch must be 0.."),
        (lambda: hint_amd.reference_lr(0, 1e-2, 0, 0.1, 3), "n_epochs must be 1.."),
    ]
    for call, text in bad_calls:
        with pytest.raises(HintAmdError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))


def test_sharding_arithmetic_and_drop_last():
    B = 7
    for world in (1, 2, 3, 8):
        for g0, n in ((0, 1), (3, 4)):
            per_rank = []
            for rank in range(world):
                first, count, block, stride = data.shard_positions(g0, n, B, rank, world)
                assert count == n * B
                i = np.arange(count)
                pos = first + (i // block * stride + i % block if block > 0 else i)
                assert (pos == eo.rank_positions(g0, n, B, rank, world)).all()
                per_rank.append(pos.reshape(n, B))
            for k in range(n):                                    # the ranks' shares of a global batch: disjoint, their union the batch
                batch = np.concatenate([p[k] for p in per_rank])
                lo = (g0 + k) * B * world
                assert (batch == np.arange(lo, lo + B * world)).all(), (world, g0, k)
    ds = hint_amd.DeviceDataset(OnGpu(torch.zeros(64 * 5 + 7, 6)))
    assert ds.n_batches(64) == 5 and ds.n_batches(64, world=2) == 2 and ds.n_batches(64, world=3) == 1 and ds.n_batches(64, world=8) == 0
    assert ds.n_batches(327) == 1 and ds.n_batches(328) == 0 and len(ds) == 327 and (ds.d, ds.dy) == (6, 0)
    a, b = hint_amd.DeviceDataset(OnGpu(torch.zeros(50, 6)), OnGpu(torch.zeros(50, 2)), seed=9, shuffle=False).split(30)
    assert (a.n_rows, b.n_rows, a.dy, b.seed, b.shuffle) == (30, 20, 2, 9, False)
    assert b.x.data_ptr() == a.x.data_ptr() + 30 * 6 * 4                          # views, not copies


@pytest.mark.parametrize("n_epochs,pre_low_lr", [(50, 3), (5, 0), (4, 6)])
def test_reference_lr_is_what_adam_and_steplr_produce(n_epochs, pre_low_lr):
    """main(c), train_unconditional.py:174-201: the lr the optimizer holds while epoch i trains"""
    lr_init, final_decay = 1e-2, 0.1
    p = torch.nn.Parameter(torch.zeros(3))
    optim = torch.optim.Adam([p], lr=lr_init, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)
    sched = torch.optim.lr_scheduler.StepLR(optim, step_size=1, gamma=final_decay ** (1.0 / n_epochs))
    seen = []
    for i_epoch in range(n_epochs):
        if i_epoch < pre_low_lr:
            for group in optim.param_groups:
                group["lr"] = lr_init * 3e-2
        seen.append(optim.param_groups[0]["lr"])            # what train_epoch's optim.step() uses
        p.grad = torch.ones(3)
        optim.step()
        sched.step()
    got = [hint_amd.reference_lr(e, lr_init, n_epochs, final_decay, pre_low_lr) for e in range(n_epochs)]
    assert all(abs(g - s) <= 1e-12 * abs(s) for g, s in zip(got, seen)), list(zip(got, seen))
    if pre_low_lr > 0:
        assert max(got) == lr_init * 3e-2                   # the overwritten value is what decays: lr_init is never trained with
    else:
        assert got[0] == lr_init and abs(got[-1] - lr_init * final_decay ** ((n_epochs - 1) / n_epochs)) <= 1e-12


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tools/epochperm_check.cpp: host code with its own main, compiled with -fsanitize=address,undefined and run as a child;
    its lines (N, weighted sum of the source rows, longest walk) equal the oracle's"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler found"
    exe = str(tmp_path / "epochperm_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "epochperm_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [tuple(int(v) for v in ln.split()) for ln in res.stdout.strip().split("\n")]
    assert [ln[0] for ln in lines] == list(range(1, 301)) + list(BIG)
    for n, total, longest in lines:
        pos = np.arange(n, dtype=np.uint64) if n <= 300 else np.array(big_positions(n), dtype=np.uint64)
        want, steps = 0, 0
        for epoch in EPOCHS:
            for seed in SEEDS:
                rows, st = eo.source_rows(n, seed, epoch, pos, with_steps=True)
                want += sum(int(v) * (int(p) + 1) for v, p in zip(rows, pos))
                steps = max(steps, int(st.max()))
        assert total == want % 2 ** 64 and longest == steps, (n, total, want % 2 ** 64, longest, steps)
