"""GPU tests of the device-resident epochs (hint_amd/csrc/hint_epoch.hip, hint_amd/data.py, FlowTrainer.fit_epoch / .evaluate,
ConditionalFlowTrainer.fit_epoch): the gather's indices against tests/epoch_oracle.py exactly and its rows against index_select bit
for bit, chunk and rank-shard invariance, guard-banded poisoned buffers, the cursor form captured in a graph and its one rejected
row, a table past 2^31 elements, the column statistics inside the bounds tests/epoch_oracle.py derives, the standardisation bit for
bit, an epoch of fit_epoch against step() over the oracle's batches bit for bit, evaluate against the float64 oracle, and every
route on a gated non-default stream.  The regime boundaries of the three kernels run here at the smallest sizes that reach them -
the moments' slab cap (1024 x 256 rows and one more), a second trip of the standardisation's and the gather's tile loops (2048 x
256 rows and one more, and max_groups) - and the three ops past 2^31 elements in tests/test_gpu_large_rows.py::test_epoch."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, data
import epoch_oracle as eo
import session_script as ss
import stream_gate
from guarded import NAN_BITS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module", autouse=True)
def leave_torchs_stream_pool_where_it_was():
    """The trainers of this file take streams from torch's pool (a warm-up stream per captured graph).  The pool hands its 32 streams
    out in turn, and with a few hardware queues a process which of them shares a queue with the null stream depends on how many
    were handed out before (NOTES.md, the plus-shape sampler): tests/test_gpu_streams.py's canary failed in the whole suite with
    this file in front of it.  So the file hands out a multiple of 32: it notes the first stream, and behind the last test draws
    until the pool stands where it stood (drawing a stream issues nothing to the device)"""
    first = torch.cuda.Stream().cuda_stream
    yield
    torch.cuda.synchronize()
    for _ in range(64):
        if torch.cuda.Stream().cuda_stream == first:
            break
    else:
        raise AssertionError("torch's stream pool did not come round")
    for _ in range(31):                                     # ... and the one drawn at the start: the next one handed out is `first`
        torch.cuda.Stream()


def table(n, d, seed, wide=0):
    """fp32 [n, d] on the device; wide: a column slice of a table `wide` columns wider (row stride d + wide)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, d + wide, generator=g).to(DEV)
    return t[:, wide // 2:wide // 2 + d] if wide else t


def order(n, epoch, first=0, count=None, seed=SEED):
    count = n - first if count is None else count
    return torch.from_numpy(eo.source_rows(n, seed, epoch, np.arange(first, first + count, dtype=np.uint64))).to(DEV)


def guarded_gather(x, y, n, epoch, pos, fill, seed=SEED, cursor=None, max_groups=0):
    """one gather into poisoned, guard-banded buffers: -> (dict of tensors, [(name, Guarded)])"""
    count = pos[1]
    d, dy = x.shape[1], y.shape[1] if y is not None else 0
    nbytes = _lib.load().hint_epoch_workspace_bytes(_lib.EPOCH_GATHER, n, count, d)
    g = dict(out_x=Guarded(count * d, fill=fill, seed=1), indices_out=Guarded(2 * count, fill=fill, seed=2, dtype=torch.int32),
             workspace=Guarded(nbytes // 4, fill=fill, seed=3, dtype=torch.int32))
    if y is not None:
        g["out_y"] = Guarded(count * dy, fill=fill, seed=4)
    bufs = dict(out_x=g["out_x"].view(count, d), indices_out=g["indices_out"].words.view(torch.int64), workspace=g["workspace"].t)
    if y is not None:
        bufs["out_y"] = g["out_y"].view(count, dy)
    res = data._gather_run(x, y, n, seed, epoch, True, pos, torch.device(DEV), want=("out_x", "out_y", "indices_out"), cursor=cursor,
                           out=bufs, max_groups=max_groups)
    assert res["workspace"].data_ptr() == g["workspace"].ptr and res["out_x"].data_ptr() == g["out_x"].ptr
    return res, list(g.items())


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 1000, 4097, 65537])
def test_indices_equal_the_oracle_exactly(n):
    for epoch, seed in ((0, 0), (3, SEED), (2 ** 32 - 1, 2 ** 64 - 1)):
        got = hint_amd.epoch_indices(n, seed, epoch, 0, n, device=DEV)
        assert got.dtype == torch.int64 and torch.equal(got, order(n, epoch, seed=seed)), (n, epoch, seed)
        assert torch.equal(got.sort().values, torch.arange(n, device=DEV))
    assert torch.equal(hint_amd.epoch_indices(n, SEED, 3, 0, n, device=DEV, shuffle=False), torch.arange(n, device=DEV))
    first = n // 3
    assert torch.equal(hint_amd.epoch_indices(n, SEED, 3, first, n - first, device=DEV), order(n, 3, first))


@pytest.mark.parametrize("d,dy,wide", [(1, 0, 0), (6, 0, 0), (6, 1, 0), (43, 4, 0), (100, 4, 0), (128, 128, 0), (6, 1, 5), (43, 0, 3)])
def test_gathered_rows_equal_index_select_in_guarded_buffers(d, dy, wide):
    """every output in a poisoned, guard-banded buffer: nothing outside [count, d] is written, every word of the workspace is,
    and the words sum to 0.  wide: x (and y) are column slices of a wider table"""
    n, epoch = 1000, 7
    x = table(n, d, 1, wide)
    y = table(n, dy, 2, wide) if dy else None
    assert (x.stride(0) == d + wide) and (wide == 0 or not x.is_contiguous())
    idx = order(n, epoch)
    for fill, first, count in (("nan", 0, n), ("junk", 131, 600), ("junk", n - 1, 1)):
        res, guards = guarded_gather(x, y, n, epoch, (first, count, 0, 0), fill)
        torch.cuda.synchronize()
        for name, g in guards:
            g.check_guards(f"{name} d={d} dy={dy} {fill}")
        want = idx[first:first + count]
        assert torch.equal(res["indices_out"], want)
        assert bits_equal(res["out_x"], x.index_select(0, want))
        if dy:
            assert bits_equal(res["out_y"], y.index_select(0, want))
        assert bool((res["workspace"] == 0).all())                     # (poisoned before: every word was written)
    ds = hint_amd.DeviceDataset(x, y, seed=SEED)
    assert ds.x.data_ptr() == x.data_ptr()                             # the slice stays a view
    out = ds.gather(epoch, 1, 3, 100)
    xs = out[0] if dy else out
    assert bits_equal(xs.reshape(300, d), x.index_select(0, idx[100:400]))
    if dy:
        assert bits_equal(out[1].reshape(300, dy), y.index_select(0, idx[100:400]))
    # a smaller grid than the default one: the tail of the workspace is cleared, the rows are the same
    res, guards = guarded_gather(x, y, n, epoch, (0, n, 0, 0), "junk", max_groups=1)
    torch.cuda.synchronize()
    assert bits_equal(res["out_x"], x.index_select(0, idx)) and bool((res["workspace"] == 0).all())
    for name, g in guards:
        g.check_guards(f"{name} one workgroup")


def test_chunks_at_any_boundaries_give_the_bits_of_one_call():
    n, epoch = 300, 2
    x, y = table(n, 6, 3), table(n, 1, 4)
    ds = hint_amd.DeviceDataset(x, y, seed=SEED)
    whole = data._gather_run(ds.x, ds.y, n, SEED, epoch, True, (0, n, 0, 0), ds.device, want=("out_x", "out_y", "indices_out"))
    again = data._gather_run(ds.x, ds.y, n, SEED, epoch, True, (0, n, 0, 0), ds.device, want=("out_x", "out_y", "indices_out"))
    cuts = [0, 7, 64, 65, n]
    for bounds in (list(range(n + 1)), cuts):
        parts = [data._gather_run(ds.x, ds.y, n, SEED, epoch, True, (a, b - a, 0, 0), ds.device, want=("out_x", "out_y", "indices_out"))
                 for a, b in zip(bounds, bounds[1:])]
        for k in ("out_x", "out_y", "indices_out"):
            assert bits_equal(torch.cat([p[k] for p in parts]), whole[k]) and bits_equal(again[k], whole[k]), (len(bounds), k)
    assert torch.equal(whole["indices_out"], order(n, epoch))


@pytest.mark.parametrize("world", [2, 3])
def test_rank_shards_concatenate_to_the_global_batch(world):
    B, n_b, epoch = 16, 4, 5
    n = B * world * n_b + 11
    ds = hint_amd.DeviceDataset(table(n, 6, 5), table(n, 2, 6), seed=SEED)
    assert ds.n_batches(B, world) == n_b
    gx, gy = ds.gather(epoch, 1, n_b - 1, B * world)                     # one rank, global batches 1..
    for rank in range(world):
        xs, ys = ds.gather(epoch, 1, n_b - 1, B, rank, world)
        assert xs.shape == (n_b - 1, B, 6) and ys.shape == (n_b - 1, B, 2)
        assert bits_equal(xs, gx.view(n_b - 1, world, B, 6)[:, rank]) and bits_equal(ys, gy.view(n_b - 1, world, B, 2)[:, rank])
        pos = torch.from_numpy(eo.rank_positions(1, n_b - 1, B, rank, world)).to(DEV)
        assert bits_equal(xs.reshape(-1, 6), ds.x.index_select(0, order(n, epoch).index_select(0, pos)))
    assert int(ds.last_workspace.sum()) == 0


def test_cursor_form_one_captured_graph_at_three_positions():
    n, count, d = 1000, 300, 6
    x = table(n, d, 7)
    dev = torch.device(DEV)
    cursor = torch.tensor([0, 0], dtype=torch.int64, device=DEV)
    nbytes = _lib.load().hint_epoch_workspace_bytes(_lib.EPOCH_GATHER, n, count, d)
    bufs = dict(out_x=torch.empty(count, d, device=DEV), indices_out=torch.empty(count, dtype=torch.int64, device=DEV),
                workspace=torch.empty(nbytes, dtype=torch.uint8, device=DEV))
    run = lambda: data._gather_run(x, None, n, SEED, 99, True, (5, count, 0, 0), dev, want=("out_x", "indices_out"),      # noqa: E731
                                   cursor=cursor, out=bufs)
    run()                                                              # (loads the kernel before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for epoch, first in ((0, 0), (4, 123), (2 ** 32 - 1, n - count)):
        cursor.copy_(torch.tensor([epoch, first], dtype=torch.int64))
        bufs["out_x"].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = data._gather_run(x, None, n, SEED, epoch, True, (first, count, 0, 0), dev, want=("out_x", "indices_out"))
        assert bits_equal(bufs["out_x"], eager["out_x"]) and torch.equal(bufs["indices_out"], eager["indices_out"]), (epoch, first)
        assert torch.equal(bufs["indices_out"], order(n, epoch, first, count))
        assert int(bufs["workspace"].view(torch.int32).sum()) == 0


def test_a_cursor_one_past_the_range_rejects_exactly_one_row():
    """an out-of-range position, not a fault: first = N - count + 1 puts the last row at position N"""
    n, count, d, epoch = 1000, 300, 6, 4
    x, y = table(n, d, 8), table(n, 2, 9)
    first = n - count + 1
    cursor = torch.tensor([epoch, first], dtype=torch.int64, device=DEV)
    res, guards = guarded_gather(x, y, n, 0, (0, count, 0, 0), "junk", cursor=cursor)
    torch.cuda.synchronize()
    for name, g in guards:
        g.check_guards(name)
    idx = order(n, epoch, first, count - 1)
    assert torch.equal(res["indices_out"][:-1], idx) and int(res["indices_out"][-1]) == -1
    assert bits_equal(res["out_x"][:-1], x.index_select(0, idx)) and bits_equal(res["out_y"][:-1], y.index_select(0, idx))
    assert bool(torch.isnan(res["out_x"][-1]).all()) and bool(torch.isnan(res["out_y"][-1]).all())
    ws = res["workspace"]
    assert int(ws.sum()) == 1 and int((ws != 0).sum()) == 1


def test_a_table_past_2_31_elements():
    """N = 2^25 + 1 rows of 100 floats (13.4 GB, torch.empty storage): known values only in the source rows the epoch's last 256
    positions read; element offsets up to 3.4e9"""
    n, d, count, epoch = 2 ** 25 + 1, 100, 256, 1
    need = n * d * 4 + (1 << 28)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free")
    x = torch.empty(n, d, dtype=torch.float32, device=DEV)
    try:
        idx = order(n, epoch, n - count, count)
        assert int(idx.max()) * d >= 2 ** 31 and len(set(idx.tolist())) == count
        vals = table(count, d, 10)
        x[idx] = vals
        ds = hint_amd.DeviceDataset(x, seed=SEED)
        res = data._gather_run(ds.x, None, n, SEED, epoch, True, (n - count, count, 0, 0), ds.device, want=("out_x", "indices_out"))
        assert torch.equal(res["indices_out"], idx) and bits_equal(res["out_x"], vals)
        assert int(res["workspace"].view(torch.int32).sum()) == 0
    finally:
        del x
        torch.cuda.empty_cache()


SLAB_EDGE = 1024 * 256              # EP_MAX_SLABS slabs of EP_TILE rows: the most rows at which a slab holds 256 rows
GRID_EDGE = 2048 * 256              # EP_MAX_WG workgroups of EP_TILE rows: the most rows the tile loops take in one trip


@pytest.mark.parametrize("n,d,row0,rows", [(1, 1, 0, 1), (2, 6, 0, 2), (1000, 6, 0, 1000), (70001, 43, 0, 70001), (70001, 43, 1234, 50000),
                                           (1000, 6, 999, 1), (SLAB_EDGE, 6, 0, SLAB_EDGE), (SLAB_EDGE + 1, 6, 0, SLAB_EDGE + 1)])
def test_moments_against_numpy_float64_inside_the_derived_bounds(n, d, row0, rows):
    """(the last two: the slab cap - 1024 slabs of 256 rows, then 1020 slabs of 257 rows, one of 5 and three empty ones)"""
    ws = _lib.load().hint_epoch_workspace_bytes(_lib.EPOCH_MOMENTS, n, rows, d)
    assert ws == -(-8 * d * min(1024, -(-rows // 256)) // 16) * 16                  # one double per slab and column
    x = table(n, d, 11, wide=3) * 3.0 + 1.5
    ds = hint_amd.DeviceDataset(x, seed=1)
    nbytes = _lib.load().hint_epoch_workspace_bytes(_lib.EPOCH_MOMENTS, n, rows, d)
    gm, gs = Guarded(2 * d, fill="nan", dtype=torch.int32), Guarded(2 * d, fill="nan", dtype=torch.int32)
    gw = Guarded(nbytes // 4, fill="junk", dtype=torch.int32)
    mean, std = ds.moments(row0, rows, out=dict(mean=gm.words.view(torch.float64), std=gs.words.view(torch.float64), workspace=gw.t))
    torch.cuda.synchronize()
    for name, g in (("mean", gm), ("std", gs), ("workspace", gw)):
        g.check_guards(name)
    x64 = x[row0:row0 + rows].double().cpu().numpy()
    e_m, e_s = eo.moment_bounds(x64)
    dm, dsd = np.abs(mean.cpu().numpy() - x64.mean(axis=0)), np.abs(std.cpu().numpy() - x64.std(axis=0))
    print(f"\nmoments N={rows} d={d}: mean off by {dm.max():.3g} (bound {2 * e_m.min():.3g}), std by {dsd.max():.3g} (bound {2 * e_s.min():.3g})")
    assert (dm <= 2 * e_m).all() and (dsd <= 2 * e_s).all(), (dm / e_m, dsd / e_s)
    m2, s2 = ds.moments(row0, rows)
    assert bits_equal(m2, mean) and bits_equal(s2, std)                # two runs: equal bits


def test_standardize_is_torchs_double_arithmetic_bit_for_bit():
    n, d = 5000, 6
    x0 = table(n, d, 12, wide=2) * 2.0 - 0.7
    x0[:, 4] = 3.25                                                    # a constant column: std 0
    x0[7, 4] = 3.25
    ds = hint_amd.DeviceDataset(x0.clone(), seed=1)
    mean, std = ds.moments(100, 3000)
    assert float(std[4]) == 0.0
    want = ((x0.double() - mean) / std).float()
    out = torch.full((n, d + 3), float("nan"), device=DEV)[:, 1:1 + d]          # out of place, into a strided table
    assert ds.apply_moments(mean, std, out=out) is out
    assert bits_equal(out, want) and bits_equal(ds.x, x0)
    assert bool(torch.isnan(out[:, 4]).all())                          # 0 / 0, as numpy
    part = ds.x.clone()
    ds2 = hint_amd.DeviceDataset(part, seed=1)
    ds2.apply_moments(mean, std, 10, 1000)                             # in place, a row range
    assert bits_equal(part[10:1010], want[10:1010]) and bits_equal(part[:10], x0[:10]) and bits_equal(part[1010:], x0[1010:])
    x1 = x0.clone()
    x1[:, 4] += torch.arange(n, device=DEV) % 2                        # constant over the statistics' rows only: +-inf elsewhere
    x1[100:3100, 4] = 3.25
    ds3 = hint_amd.DeviceDataset(x1.clone(), seed=1)
    m3, s3 = ds3.standardize(stats_rows=(100, 3000))                   # statistics of a range, applied in place to all rows
    assert bits_equal(ds3.x, ((x1.double() - m3) / s3).float()) and bool(torch.isinf(ds3.x[:100, 4]).any())
    a, b = hint_amd.DeviceDataset(x0.clone(), seed=1).split(4000)      # train statistics on the test rows
    ma, sa = a.standardize()
    b.apply_moments(ma, sa)
    assert bits_equal(b.x, ((x0[4000:].double() - ma) / sa).float())


def standardize_run(ds, mean, std, out, max_groups=0):
    """one hint_epoch_run STANDARDIZE of all rows of ds.x into `out`, with the descriptor's max_groups (DeviceDataset passes none)"""
    desc = ds._stat_desc(_lib.EPOCH_STANDARDIZE, 0, ds.n_rows, mean, std)
    desc.out_x, desc.out_stride, desc.max_groups = out.data_ptr(), out.stride(0), max_groups
    data._run_desc("hint_epoch_run", desc, ds.device, (_lib.EPOCH_STANDARDIZE, ds.n_rows, ds.n_rows, ds.d))


@pytest.mark.parametrize("n,max_groups", [(GRID_EDGE + 1, 0), (1000, 1)])
def test_standardize_tile_loop_takes_a_second_trip(n, max_groups):
    """more tiles than workgroups - one row past the default grid's 2048 tiles, and four tiles on one workgroup: out of place into
    a poisoned, guard-banded buffer, every element torch's double arithmetic bit for bit, no word left unwritten"""
    d = 6
    x = table(n, d, 21) * 2.0 - 0.7
    ds = hint_amd.DeviceDataset(x, seed=1)
    mean, std = ds.moments()
    g = Guarded(n * d, fill="nan")
    standardize_run(ds, mean, std, g.view(n, d), max_groups)
    torch.cuda.synchronize()
    g.check_guards(f"standardize n={n} max_groups={max_groups}")
    assert int((g.words == NAN_BITS).sum()) == 0
    assert bits_equal(g.view(n, d), ((x.double() - mean) / std).float())
    again = torch.empty(n, d, device=DEV)
    standardize_run(ds, mean, std, again, 3)                            # another grid: the same bits
    assert bits_equal(again, g.view(n, d))


def test_gather_tile_loop_takes_a_second_trip_on_the_default_grid():
    """count = 2048 x 256 + 1: the default grid's first workgroup takes a second tile, of one row.  The indices are a permutation
    and the oracle's at the tile edges and a picket; the rows are index_select's bit for bit"""
    n, d, epoch = GRID_EDGE + 1, 6, 9
    x = table(n, d, 22)
    res, guards = guarded_gather(x, None, n, epoch, (0, n, 0, 0), "nan")
    torch.cuda.synchronize()
    for name, g in guards:
        g.check_guards(name)
        assert int((g.words == NAN_BITS).sum()) == 0, name
    idx = res["indices_out"]
    assert torch.equal(idx.sort().values, torch.arange(n, device=DEV)) and int(res["workspace"].sum()) == 0
    pos = np.unique(np.concatenate([np.arange(0, n, 997), np.arange(300), np.arange(GRID_EDGE - 300, n)])).astype(np.uint64)
    want = torch.from_numpy(eo.source_rows(n, SEED, epoch, pos)).to(DEV)
    assert torch.equal(idx[torch.from_numpy(pos.astype(np.int64)).to(DEV)], want)
    assert bits_equal(res["out_x"], x.index_select(0, idx))


# ---- trainers ----
SPEC = dict(d=6, widths=(32, 16), n_blocks=3, dc=0, use_chain=True)
B, N = 64, 64 * 5 + 7


def build_flow(spec=SPEC):
    params, perms = ss.initial_weights(spec)
    flow = hint_amd.HintFlow(spec["d"], spec["n_blocks"], list(spec["widths"]), ndim_c=spec["dc"])
    for i, blk in enumerate(flow.blocks):
        blk.load_state_dict({k: v.clone() for k, v in params[i].items()})
        if perms[i] is not None:
            flow.perms[i].W.copy_(perms[i])
    return flow.to(DEV)


def trainer(use_graph, noise=0.01, seed=77):
    return hint_amd.FlowTrainer(build_flow(), noise=noise, use_graph=use_graph, seed=seed)


def stepped_twin(make, ds, epoch, batches, dy=False):
    """a second trainer with the same seed stepped with step() over x.index_select(0, oracle indices), batch by batch"""
    tr = make()
    idx = order(ds.n_rows, epoch, seed=ds.seed)
    losses = []
    for g in batches:
        rows = idx[g * B:(g + 1) * B]
        args = (ds.x.index_select(0, rows),) + ((ds.y.index_select(0, rows),) if dy else ())
        l0, l1 = tr.step(*args)
        losses.append(torch.stack([l0, l1]))
    return tr, torch.stack(losses)


@pytest.mark.parametrize("use_graph", [True, False])
def test_fit_epoch_equals_step_over_the_oracles_batches_bit_for_bit(use_graph):
    ds = hint_amd.DeviceDataset(table(N, 6, 13), seed=SEED)
    assert ds.n_batches(B) == 5                                        # the tail of 7 rows is dropped
    tr = trainer(use_graph)
    losses = tr.fit_epoch(ds, 3, B, chunk=2)                           # two step_many of 2, one step()
    twin, want = stepped_twin(lambda: trainer(use_graph), ds, 3, range(5))
    assert losses.shape == (5, 2) and tr.step_count == twin.step_count == 5
    assert bits_equal(tr.P, twin.P) and bits_equal(tr.M, twin.M) and bits_equal(tr.V, twin.V)
    # (the loss sums alone take float atomics: the tolerance of the graph / eager twins of tests/test_gpu_trainer_session.py)
    assert np.allclose(losses.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6), (losses, want)
    assert tr.use_graph is use_graph and (tr._graph_many is not None) == use_graph
    # first_batch continues an epoch begun with max_batches to the bits of the uninterrupted one
    tr2 = trainer(use_graph)
    la = tr2.fit_epoch(ds, 3, B, max_batches=2, chunk=2)
    lb = tr2.fit_epoch(ds, 3, B, first_batch=2, chunk=2)
    assert la.shape == (2, 2) and lb.shape == (3, 2) and bits_equal(tr2.P, tr.P) and bits_equal(tr2.V, tr.V)
    assert np.allclose(torch.cat([la, lb]).cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert tr2.fit_epoch(ds, 3, B, max_batches=2, first_batch=2).shape == (0, 2)


def test_fit_epoch_on_the_conditional_trainer():
    nx, ny = 10, 3
    torch.manual_seed(5)
    m0 = hint_amd.ConditionalHintFlow(nx, ny, 2, 24).to(DEV)
    ds = hint_amd.DeviceDataset(table(N, nx, 14), table(N, ny, 15), seed=SEED)
    make = lambda: hint_amd.ConditionalFlowTrainer(copy.deepcopy(m0), use_graph=True, seed=78)      # noqa: E731
    tr = make()
    losses = tr.fit_epoch(ds, 1, B, chunk=2)
    twin, want = stepped_twin(make, ds, 1, range(5), dy=True)
    assert losses.shape == (5, 2) and tr.step_count == twin.step_count == 5
    assert bits_equal(tr.P, twin.P) and bits_equal(tr.M, twin.M) and bits_equal(tr.V, twin.V)
    assert np.allclose(losses.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6), (losses, want)


def test_evaluate_against_the_float64_oracle_and_its_own_noise_stream():
    ds = hint_amd.DeviceDataset(table(N, 6, 16), seed=SEED)
    tr = trainer(True)
    oracle = ss.OracleBackend(SPEC).flow
    x64 = ds.x.double().cpu()
    for bs, mb in ((B, 0), (None, 0), (100, 2)):
        got = tr.evaluate(ds, batch_size=bs, noise=0.0, max_batches=mb)
        size = N if bs is None else bs
        nb = N // size if mb == 0 else min(N // size, mb)
        pairs = []
        with torch.no_grad():
            for k in range(nb):
                z, J = oracle.forward(x64[k * size:(k + 1) * size])
                pairs.append([float(v) for v in oracle.loss_terms(z, J)])
        want = np.mean(pairs, axis=0)
        dev = ss.scalar_dev(got.cpu().numpy(), want)
        print(f"\nevaluate batch_size={bs} max_batches={mb}: {got.tolist()} / oracle {want.tolist()}: deviation {dev:.2e}")
        assert got.shape == (2,) and dev <= ss.CAPS["losses"]          # the loss tolerance of tests/test_gpu_trainer_session.py
    # with noise, two evaluations draw different numbers; the same epoch and count draw the same
    a, b = tr.evaluate(ds, B, noise=0.01), tr.evaluate(ds, B, noise=0.01)
    assert not bits_equal(a, b) and float((a - b).abs().max()) < 0.05
    # an evaluation between two training steps changes no bit of training
    xs = [table(B, 6, 20 + i) for i in range(3)]
    plain, mixed = trainer(True), trainer(True)
    for i, x in enumerate(xs):
        plain.step(x)
        mixed.step(x)
        if i < 2:
            mixed.evaluate(ds, B)                                       # (the trainer's noise, 0.01)
        assert bits_equal(plain.P, mixed.P) and bits_equal(plain.M, mixed.M) and bits_equal(plain.V, mixed.V), i
    assert torch.equal(plain.rng_state, mixed.rng_state) and plain.step_count == mixed.step_count == 3


def test_evaluate_walks_the_modules_of_a_flow_that_is_not_chained():
    ds = hint_amd.DeviceDataset(table(N, 6, 16), seed=SEED)
    chained = trainer(True).evaluate(ds, B, noise=0.0)
    walked = hint_amd.FlowTrainer(build_flow(), use_graph=False, use_chain=False, seed=77).evaluate(ds, B, noise=0.0)
    assert ss.scalar_dev(walked.cpu().numpy(), chained.cpu().numpy()) <= ss.CAPS["losses"]


@contextlib.contextmanager
def independent_stream():
    """a non-blocking stream of this test's own that does not share a hardware queue with the null stream, destroyed behind it (as
    tests/test_gpu_plusgen.py's side_stream: a stream of torch's pool would live on).  A process opens a few hardware queues and
    its streams share them, so which stream shares the null stream's depends on what ran before: up to eight streams are tried
    with tests/test_gpu_streams.py's canary, turned round - a copy on the stream must end while a gate holds the null stream shut -
    and the first that passes is used.  Without one the harness is blind, and the test fails saying so"""
    hip = _lib.load()                                        # (the HIP runtime's symbols resolve through the library's dependencies)
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
    raws, found = [], None
    src, dst = torch.arange(4096, dtype=torch.float32, device=DEV), torch.zeros(4096, device=DEV)
    try:
        for attempt in range(8):
            raw = C.c_void_p()
            assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0 and raw.value      # 1: hipStreamNonBlocking
            raws.append(raw)
            s = torch.cuda.ExternalStream(raw.value)
            torch.cuda.synchronize()
            gate = stream_gate.Gate(torch.cuda.default_stream(), 30.0).open()
            with torch.cuda.stream(s):
                dst.copy_(src)
            s.synchronize()
            closed = gate.still_closed()
            torch.cuda.synchronize()
            if closed:
                found = s
                print(f"\nside stream {attempt} runs independently of the null stream")
                break
        assert found is not None, "the harness is blind on this machine: every side stream waited for the gated null stream"
        yield found
    finally:
        torch.cuda.synchronize()
        for raw in raws:
            assert hip.hipStreamDestroy(raw) == 0


def test_everything_enqueues_behind_a_gate_on_a_non_default_stream():
    """gather, standardize, fit_epoch and evaluate S-gated and null-gated on a side stream (tests/stream_gate.py): nothing goes to
    the null stream and nothing blocks the host.  The trainers are built, and their graphs captured, before the gates"""
    x0, y0 = table(N, 6, 17), table(N, 2, 18)

    def make_data(fill, role):
        gx = Guarded(N * 6).set(x0)
        late = stream_gate.late_inputs([(gx, None)])
        ds = hint_amd.DeviceDataset(gx.view(N, 6), y0, seed=SEED)

        def call():
            xs, ys = ds.gather(2, 1, 3, B)
            mean, std = ds.standardize(stats_rows=(7, 200))
            xs2, _ = ds.gather(2, 0, 2, B)
            return dict(xs=xs, ys=ys, mean=mean, std=std, xs2=xs2, x=ds.x, ws=ds.last_workspace)
        return stream_gate.Seq(call, late, [("x", gx)])

    # (built outside the side stream's life: a pool stream first used beside a raw stream would keep another hardware queue)
    trs = {}
    for role in ("ref", "S"):
        ds = hint_amd.DeviceDataset(x0.clone(), seed=SEED)
        tr = trainer(True)
        tr.fit_epoch(ds, 0, B, chunk=2)                                # (captures both graphs)
        tr.evaluate(ds, B)
        torch.cuda.synchronize()
        state = [getattr(tr, k).clone() for k in ("P", "M", "V", "G", "rng_state", "opt_state")]
        trs[role] = (tr, state, tr.step_count, tr._eval_count)
    with independent_stream() as S:
        stream_gate.run_case("epoch_gather_standardize", make_data, S)

        def make_fit(fill, role):
            tr, state, steps, evals = trs[role]
            for k, v in zip(("P", "M", "V", "G", "rng_state", "opt_state"), state):
                getattr(tr, k).copy_(v)
            tr.step_count, tr._eval_count = steps, evals
            for e in tr.engines:
                e._pack_key = None
            gx = Guarded(N * 6).set(x0)
            late = stream_gate.late_inputs([(gx, None)])
            ds = hint_amd.DeviceDataset(gx.view(N, 6), seed=SEED)

            def call():
                losses = tr.fit_epoch(ds, 1, B, chunk=2)
                ev = tr.evaluate(ds, B)
                return dict(losses=losses, ev=ev, P=tr.P.clone(), V=tr.V.clone())
            return stream_gate.Seq(call, late, [("x", gx)], loose=("losses", "ev"))
        stream_gate.run_case("epoch_fit_evaluate", make_fit, S)
