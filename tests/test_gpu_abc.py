"""GPU tests of hint_amd.nearest_rows / quantile_abc / hint_abc_run against the test-side float64 evaluation (tests/abc_oracle.py).

The order under test: rows by (D_i, i), D_i = sum_j (y_ij - t_j)^2 in fp32 with j = 0, 1, .., ny - 1 in that order (the first term a
rounded product, then fused multiply-adds); a D_i that is not finite counts as +inf.

Exact cases (small integers: fp32 arithmetic is exact) must give the oracle's indices element for element and sqrt(D) within one
unit of the last place.  Seeded N(0, 1) cases go through the comparison rule of abc_oracle.check_rule, eps = (ny + 2) 2^-23:
  every returned index has D64 <= B (1 + eps), B = D64 at rank k - 1;   every index with D64 < B (1 - eps) is returned;
  dist within (ny + 4) 2^-23 relative of sqrt(D64);   dist non-decreasing, rows of equal dist in (D, row number) order, D in fp32 as
  defined above (sqrt maps neighbouring D to one dist, so the issue's "idx increasing among equal dist" holds only where D is equal);
  and at most 1 % of k rows (other than the boundary row) lie within eps B of B - asserted, so that a bad input fails loudly.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib
from hint_amd._lib import HintAmdError
import abc_oracle as ao
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = _lib.load().hint_abc_geometry(1, 1, 1)                 # rows per workgroup at small N
G = _lib.load().hint_abc_geometry(1 << 30, 1, 0)           # the largest grid


def geometry(N, ny):
    """(workgroups of the streaming passes, rows each owns) from hint_abc_geometry"""
    lib = _lib.load()
    return lib.hint_abc_geometry(N, ny, 0), lib.hint_abc_geometry(N, ny, 1)


def nearest(y, t, k):
    """(idx int64, dist fp32) as numpy arrays, through nearest_rows"""
    idx, dist = hint_amd.nearest_rows(torch.as_tensor(y).to(DEV), torch.as_tensor(t), k)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.shape == dist.shape == (k,)
    assert idx.device == dist.device == torch.device(DEV)
    return idx.cpu().numpy(), dist.cpu().numpy()


def check_exact(y, t, k):
    """idx equals the oracle's element for element; dist is sqrt(D) within 1 ulp"""
    D, order = ao.order64(y, t)
    idx, dist = nearest(y, t, k)
    assert np.array_equal(idx, order[:k]), (idx[:10], order[:10])
    ulps = ao.ulps_apart(dist, np.sqrt(D[order[:k]]).astype(np.float32))
    assert ulps <= 1, ulps
    return idx, dist


# ---- 1. exact cases ----
def test_exact_integer_lattice_with_heavy_ties():
    rs = np.random.RandomState(1)
    for ny in (2, 3, 4):
        y = rs.randint(-12, 13, size=(3 * R + 17, ny)).astype(np.float32)          # sums of squares far below 2^24
        t = rs.randint(-5, 6, size=ny).astype(np.float32)
        D, _ = ao.order64(y, t)
        assert np.unique(D).size < D.size // 4                                      # D is an integer <= ny 17^2: at most 1157 values
        for k in (1, 500, 4002):
            check_exact(y, t, k)


def test_exact_every_row_identical():
    for N, ny in ((2 * R + 5, 2), (R + 1, 5)):
        y = np.tile(np.arange(1, ny + 1, dtype=np.float32), (N, 1))
        t = np.zeros(ny, dtype=np.float32)
        for k in (1, 700, min(N, 8192)):
            idx, dist = check_exact(y, t, k)
            assert np.array_equal(idx, np.arange(k))
            assert (dist == np.float32(np.sqrt(sum(j * j for j in range(1, ny + 1))))).all()


def test_exact_ties_straddle_rank_k_and_a_workgroup_boundary():
    N = 3 * R + 17
    g, r = geometry(N, 1)
    assert g == 4 and r == R
    y = np.full((N, 1), 100.0, dtype=np.float32)
    near = [7, R + 50, 2 * R + 3, 2 * R + 700, N - 1]       # five rows at D = 0.25
    y[near, 0] = 0.5
    ties = list(range(R - 4, R + 4))                        # eight rows at D = 1, four on each side of the boundary of workgroups 0 and 1 ...
    y[ties, 0] = 1.0
    y[2 * R - 1, 0] = y[2 * R, 0] = -1.0                    # ... and two more across the next one
    ties += [2 * R - 1, 2 * R]
    t = np.zeros(1, dtype=np.float32)
    for k in range(5, 5 + 10 + 3):                          # rank k - 1 at every position inside the tie group, and past it
        idx, dist = check_exact(y, t, k)
        assert sorted(idx[:5]) == sorted(near)
        assert list(idx[5:]) == (ties + [0, 1, 2])[:k - 5]


def test_exact_keys_that_differ_in_the_lowest_mantissa_bits():
    """rows (2896, b), b = 0 .. 60, against 0: D = 8386816 + b^2 is near 2^23 and steps by single units - the last digit decides"""
    rs = np.random.RandomState(2)
    b = rs.permutation(61).astype(np.float32)
    y = np.stack([np.full(61, 2896.0, dtype=np.float32), b], axis=1)
    t = np.zeros(2, dtype=np.float32)
    for k in (1, 2, 30, 61):
        idx, _ = check_exact(y, t, k)
        assert np.array_equal(y[idx, 1], np.arange(k, dtype=np.float32))
    big = np.concatenate([np.full((R + 3, 2), 3000.0, dtype=np.float32), y])      # the same rows behind a workgroup of far ones
    idx, _ = check_exact(big, t, 61)
    assert np.array_equal(big[idx, 1], np.arange(61, dtype=np.float32))


def test_exact_row_equal_to_the_target():
    rs = np.random.RandomState(3)
    y = rs.randint(-50, 51, size=(R + 100, 3)).astype(np.float32)
    t = np.array([3.0, -7.0, 11.0], dtype=np.float32)
    y[(y == t).all(1)] += 1.0
    y[777] = t
    idx, dist = check_exact(y, t, 3)
    assert idx[0] == 777 and dist[0] == 0.0


def test_exact_rows_with_inf_or_nan_sort_last():
    rs = np.random.RandomState(4)
    N = 300
    y = rs.randint(-20, 21, size=(N, 2)).astype(np.float32)
    t = np.array([1.0, -2.0], dtype=np.float32)
    bad = [5, 17, 100, 250]
    y[5, 0], y[17, 1], y[100, 0], y[250] = np.inf, np.nan, -np.inf, (np.nan, np.inf)
    idx, dist = check_exact(y, t, N - len(bad))             # never selected while N - bad >= k
    assert not set(idx) & set(bad) and np.isfinite(dist).all()
    idx, dist = check_exact(y, t, N)                        # k = N: the last rows, by the canonical key (+inf) and then by index
    assert list(idx[-4:]) == bad and np.isposinf(dist[-4:]).all() and np.isfinite(dist[:-4]).all()
    idx, dist = check_exact(y, t, N - 2)
    assert list(idx[-2:]) == bad[:2]


def big_geometry():
    g, r = geometry(ao.BIG_N, 2)
    assert g == G and 4096 < r < 2 * 4096       # a workgroup's rows: tile 0 = [0, 4096) and a partial tile 1 of the compaction pass
    return g, r


def test_exact_ties_in_different_tiles_of_a_workgroup_and_across_workgroups():
    """rows_per_workgroup > 4096: offsets are carried from tile to tile, tiles without a candidate are skipped before ones with"""
    N = ao.BIG_N
    g, r = big_geometry()
    y = np.zeros((N, 2), dtype=np.float32)
    y[:, 0] = 100.0
    # rows at D = 0.25 (all returned): alone in a second tile behind an empty first one, in both tiles, in the last workgroup's tail
    near = [10 * r + 4096 + 7, 11 * r + 5, 11 * r + 4095, 11 * r + 4096, 12 * r + r - 1, 500 * r + 3000, 500 * r + 5000, N - 1]
    # rows at D = 1: in both tiles of workgroup 3 (a lesser row between them), on the tile boundary of workgroup 4, across the
    # boundary of workgroups 7 and 8, in a second tile only, and far down the grid
    ties = [3 * r + 10, 3 * r + 2047, 3 * r + 4095, 3 * r + 4096, 3 * r + r - 1, 4 * r, 4 * r + 4095, 4 * r + 4096, 4 * r + 4097,
            8 * r - 1, 8 * r, 9 * r + 4100, 9 * r + r - 1, 700 * r + 1, 700 * r + 4999, (g - 1) * r + 2]
    near.append(3 * r + 3000)
    assert ties == sorted(ties) and len(set(near) | set(ties)) == len(near) + len(ties) and max(near + ties) < N
    y[near, 0], y[ties, 0] = 0.5, 1.0
    y[ties[::2], 0] = -1.0
    t = np.zeros(2, dtype=np.float32)
    D, order = ao.order64(y, t)                              # once, for every k
    yd = torch.from_numpy(y).to(DEV)
    for k in list(range(len(near), len(near) + len(ties) + 1)) + [len(near) + len(ties) + 3, 4002]:
        idx, dist = hint_amd.nearest_rows(yd, t, k)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert np.array_equal(idx, order[:k]), (k, idx[:30], order[:30])
        assert list(idx[:len(near)]) == sorted(near)
        assert list(idx[len(near):len(near) + len(ties)]) == ties[:k - len(near)]
        assert ao.ulps_apart(dist, np.sqrt(D[order[:k]]).astype(np.float32)) <= 1


def test_exact_integer_lattice_with_several_tiles_per_workgroup():
    """121 x 121 lattice points over BIG_N rows: every distance is shared by hundreds of rows in every tile of every workgroup"""
    N = ao.BIG_N
    big_geometry()
    rs = np.random.RandomState(6)
    y = rs.randint(-60, 61, size=(N, 2)).astype(np.float32)
    t = np.array([3.0, -4.0], dtype=np.float32)
    D, order = ao.order64(y, t)
    yd = torch.from_numpy(y).to(DEV)
    for k in (500, 4002, 8192):
        assert D[order[k - 1]] == D[order[k]]                # ties straddle rank k - 1
        idx, dist = hint_amd.nearest_rows(yd, t, k)
        assert np.array_equal(idx.cpu().numpy(), order[:k])
        assert ao.ulps_apart(dist.cpu().numpy(), np.sqrt(D[order[:k]]).astype(np.float32)) <= 1


# ---- 2. and 3. seeded N(0, 1) shapes under the comparison rule ----
@pytest.mark.parametrize("case", ao.random_cases(R, G), ids=lambda c: "N%d_ny%d_k%d" % c[:3])
def test_random_shapes(case):
    N, ny, k, seed = case
    y, t = ao.random_inputs(N, ny, seed)
    idx, dist = nearest(y, t, k)
    ao.check_rule(y, t, k, idx, dist)


def test_the_largest_cases_use_every_workgroup():
    full = (G - 1) * R + 1
    assert geometry(full, 2) == (G, R) and geometry(full - 1, 2)[0] == G - 1
    assert {c[0] for c in ao.random_cases(R, G)} >= {1, 63, 64, 65, R - 1, R, R + 1, 3 * R + 17, full, full + 1, ao.BIG_N}
    g, r = geometry(ao.BIG_N, 2)
    assert g == G and 4096 < r < 2 * 4096 and ao.BIG_N % r not in (0, 2048, 4096)     # several turns of each loop, partial last ones


@pytest.mark.parametrize("case", ao.GOLDEN_CASES, ids=lambda c: c["name"])
def test_goldens_against_the_recorded_reference_output(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"abc_{case['name']}.npz"))
    x, y, t = ao.golden_inputs(case)
    assert abs(ao.checksum([x, y, t]) - float(g["in_checksum"])) < 1e-6
    n, ny = case["n"], case["ny"]
    k = n + 2
    idx, dist = nearest(y, t, k)
    band = ao.check_rule(y, t, k, idx, dist)
    assert band == 0                                         # ... so the k rows are the float64 order's first k, as a set
    ref_rows = g["ref_rows"].astype(np.int64)
    assert set(ref_rows) <= set(idx)
    thr = float(g["ref_threshold"])
    assert abs(float(dist[-1]) - thr) <= (ny + 4) * 2.0 ** -23 * thr
    # the reference's call itself: quantile_ABC(x, y, y_target, n) with x on the host
    sample, threshold = hint_amd.quantile_abc(torch.from_numpy(x), torch.from_numpy(y).to(DEV), torch.from_numpy(t), n=n)
    assert sample.device.type == "cpu" and sample.shape == (n, x.shape[1]) and threshold.shape == ()
    assert np.array_equal(sample[:, -1].numpy().astype(np.int64), idx[1:n + 1])
    # no other row lies within eps of rank 0 or of rank n either, so fp32 drops and keeps the rows the reference does
    D, order = ao.order64(y, t)
    assert ao.band_count(D, order, 1, ny) == 0 and ao.band_count(D, order, n + 1, ny) == 0
    assert sorted(idx[1:n + 1]) == sorted(ref_rows)
    assert float(threshold) == float(dist[n + 1])


def test_quantile_abc_is_nearest_rows_plus_a_gather():
    N, ny, n = 3 * R + 17, 2, 100
    y, t = ao.random_inputs(N, ny, 77)
    rs = np.random.RandomState(78)
    x = rs.standard_normal((N, 4)).astype(np.float32)
    yd = torch.from_numpy(y).to(DEV)
    for skip in (0, 1):
        idx, dist = hint_amd.nearest_rows(yd, t, skip + n + 1)
        for xt in (torch.from_numpy(x), torch.from_numpy(x).to(DEV)):
            sample, threshold = hint_amd.quantile_abc(xt, yd, t.reshape(1, ny), n=n, skip=skip)
            assert sample.device == xt.device and sample.shape == (n, 4) and sample.dtype == torch.float32
            assert bits_equal(sample.cpu(), torch.from_numpy(x)[idx[skip:skip + n].cpu()])
            assert threshold.shape == () and threshold.dtype == torch.float32 and threshold.device == yd.device
            assert bits_equal(threshold, dist[skip + n])
    with pytest.raises(HintAmdError, match="x has 10 rows and y has"):
        hint_amd.quantile_abc(torch.from_numpy(x[:10]), yd, t, n=n)
    with pytest.raises(HintAmdError, match=r"skip \+ n \+ 1 = 52 are needed"):
        hint_amd.quantile_abc(torch.from_numpy(x[:51]), yd[:51], t, n=50)
    with pytest.raises(HintAmdError, match="above the limit of 8192"):
        hint_amd.quantile_abc(torch.zeros(8193, 1), torch.zeros(8193, ny, device=DEV), t, n=8191)     # enough rows, too many asked for
    with pytest.raises(HintAmdError, match=r"k must be 1..min\(len\(y\), 8192\)"):
        hint_amd.nearest_rows(yd[:50], t, 51)
    with pytest.raises(HintAmdError, match=r"target must have shape \[2\] or \[1, 2\]"):
        hint_amd.nearest_rows(yd, np.zeros(3, dtype=np.float32), 5)
    with pytest.raises(HintAmdError, match="floating-point"):
        hint_amd.nearest_rows(yd.long(), t, 5)


def test_python_contract_copies_only_where_needed_and_every_load_path_agrees():
    N = R + 37
    for ny in (2, 4, 3):
        y, t = ao.random_inputs(N, ny, 90 + ny)
        yd = torch.from_numpy(y).to(DEV)
        want_i, want_d = hint_amd.nearest_rows(yd, t, 300)
        # a view one float past an aligned address: rows of ny = 2 / 4 are then read by the 4-byte path
        flat = torch.zeros(N * ny + 1, device=DEV)
        flat[1:] = yd.reshape(-1)
        off = flat[1:].view(N, ny)
        assert off.is_contiguous() and off.data_ptr() % 8 == 4
        got_i, got_d = hint_amd.nearest_rows(off, t, 300)
        assert torch.equal(got_i, want_i) and bits_equal(got_d, want_d)
        # other dtypes and non-contiguous views are copied; the target may live anywhere
        got_i, got_d = hint_amd.nearest_rows(yd.double(), torch.from_numpy(t).to(DEV).double(), 300)
        assert torch.equal(got_i, want_i) and bits_equal(got_d, want_d)
        wide = torch.zeros(N, 2 * ny, device=DEV)
        wide[:, ::2] = yd
        got_i, got_d = hint_amd.nearest_rows(wide[:, ::2], list(map(float, t)), 300)
        assert torch.equal(got_i, want_i) and bits_equal(got_d, want_d)
    torch.cuda.synchronize()


# ---- hint_abc_run on guard-banded buffers ----
def run_desc(y, target, n_rows, ny, k, idx, dist, ws, ws_bytes, sync=True):
    lib = _lib.load()
    desc = _lib.AbcDesc()
    desc.y, desc.target, desc.n_rows, desc.ny, desc.k = y, target, n_rows, ny, k
    desc.idx, desc.dist, desc.workspace, desc.workspace_bytes = idx, dist, ws, ws_bytes
    _lib.check(lib.hint_abc_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_abc_run")
    if sync:                              # (tests/test_gpu_streams.py issues it behind a gate and must not wait)
        torch.cuda.synchronize()


@pytest.mark.parametrize("align", (16, 256))
@pytest.mark.parametrize("kind", ("lattice_ny3", "random_ny2", "random_ny4"))
def test_run_is_reproducible_and_ignores_what_outputs_and_workspace_held(kind, align):
    """hint_abc_run on guard-banded buffers, with idx, dist and the workspace filled with zeros, NaNs or junk: the same bits
    every time, guards intact, inputs unchanged"""
    lib = _lib.load()
    if kind == "lattice_ny3":
        N, ny, k = 2 * R + 9, 3, 700
        rs = np.random.RandomState(5)
        y = rs.randint(-12, 13, size=(N, ny)).astype(np.float32)          # heavy ties, also at rank k - 1
        t = np.array([1.0, 0.0, -2.0], dtype=np.float32)
    else:
        ny = int(kind[-1])
        N, k = (2 * R + 1, 4002) if kind == "random_ny2" else (R + 1, R + 1)
        assert k <= N
        y, t = ao.random_inputs(N, ny, 6 + ny)
    gy = Guarded(N * ny, align=align).set(torch.from_numpy(y))
    gt = Guarded(ny, align=align).set(torch.from_numpy(t))
    assert gy.ptr % 32 == (16 if align == 16 else 0)
    nbytes = lib.hint_abc_workspace_bytes(N, ny, k)
    assert nbytes % 4 == 0
    sy, st = gy.snapshot(), gt.snapshot()
    first = None
    fills = [("zero", "zero"), ("zero", "zero")] + [(a, b) for a in FILLS[1:] for b in FILLS[1:]]
    for rep, (fill_o, fill_w) in enumerate(fills):
        gi = Guarded(k, fill=fill_o, seed=rep, dtype=torch.int32, align=align)
        gd = Guarded(k, fill=fill_o, seed=50 + rep, align=align)
        gw = Guarded(nbytes // 4, fill=fill_w, seed=100 + rep, align=align)
        run_desc(gy.ptr, gt.ptr, N, ny, k, gi.ptr, gd.ptr, gw.ptr, nbytes)
        what = f"outputs {fill_o}, workspace {fill_w}"
        gi.check_guards(what + ": idx")
        gd.check_guards(what + ": dist")
        gw.check_guards(what + ": workspace")
        gy.check_unchanged(sy, what + ": y")
        gt.check_unchanged(st, what + ": target")
        if first is None:
            first = (gi.t.clone(), gd.t.clone())
        assert torch.equal(gi.t, first[0]) and bits_equal(gd.t, first[1]), what
    idx, dist = first[0].cpu().numpy().astype(np.int64), first[1].cpu().numpy()
    if kind == "lattice_ny3":
        D, order = ao.order64(y, t)
        assert D[order[k - 1]] == D[order[k]]                            # ties straddle rank k - 1
        assert np.array_equal(idx, order[:k]) and ao.ulps_apart(dist, np.sqrt(D[order[:k]]).astype(np.float32)) <= 1
    else:
        ao.check_rule(y, t, k, idx, dist)
    # the Python route returns the same bits
    pi, pd = hint_amd.nearest_rows(gy.view(N, ny), gt.view(ny), k)
    assert torch.equal(pi, first[0].to(torch.int64)) and bits_equal(pd, first[1])


# ---- 4. captured in a graph ----
def test_captured_in_a_single_stream_graph_and_replayed_on_a_new_target():
    N, ny, k = 3 * R + 17, 2, 4002
    y, t = ao.random_inputs(N, ny, 31)
    _, t2 = ao.random_inputs(8, ny, 32)
    yd, td = torch.from_numpy(y).to(DEV), torch.from_numpy(t).to(DEV)
    eager_i, eager_d = hint_amd.nearest_rows(yd, td, k)                 # (also loads the kernels before the capture)
    eager_i, eager_d = eager_i.clone(), eager_d.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx, dist = hint_amd.nearest_rows(yd, td, k)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager_i) and bits_equal(dist, eager_d)
    td.copy_(torch.from_numpy(t2))                                      # a new target in the same buffer
    g.replay()
    torch.cuda.synchronize()
    want_i, want_d = hint_amd.nearest_rows(yd, td, k)
    assert torch.equal(idx, want_i) and bits_equal(dist, want_d)
    assert not torch.equal(idx, eager_i)
    ao.check_rule(y, t2, k, idx.cpu().numpy(), dist.cpu().numpy())
