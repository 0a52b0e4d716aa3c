"""hint_amd.curves on the device against the float64 oracle of tests/curve_oracle.py (its docstring states the comparison rule):
the band rule on the seeded Gaussian family at every size the kernel takes another path, the tie rule on ellipses, the fixtures
recorded from the reference, eps / noise / target, the invariants (reproducible, a row's bits independent of the batch and the
grid, guard-banded outputs over every fill, non-finite rows), and graph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves
import curve_oracle as co
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -24
TILE = _lib.load().hint_curve_geometry(1, 5, 100, 1)                      # rows a workgroup has in flight


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def run(x, P=100, eps=None, noise=0.0, target=None, want_dist=False, want_mean=False, max_groups=0):
    """the checked-argument route below the public functions, which also takes max_groups"""
    return curves._run(x, P, eps, noise, target, want_dist, want_mean, max_groups)


def assert_band(x, y_dev, P, what):
    bad, worst = co.band_check(x, y_dev.cpu().numpy(), P)
    print(f"{what}: worst feature error / bound {worst:.3g}")
    assert len(bad) == 0, (what, bad[:10], worst)


# ---- 1. the band rule on the Gaussian family ----
SIZES = (1, 63, 64, 65, TILE - 1, TILE + 1)
MULTI_TURN_N = 2 * TILE * 3 + TILE + 1          # max_groups = 2: seven wavefronts take 4 turns, the eighth a ragged 1


@pytest.mark.parametrize("K,P", ((5, 100), (1, 7), (3, 2), (3, 3), (5, 64), (5, 65), (25, 128), (25, 100)))
def test_band_rule_on_the_gaussian_family(K, P):
    lib = _lib.load()
    x = co.gauss(1000 * K + P, max(SIZES + (MULTI_TURN_N,)), K)
    xd = dev(x)
    for N in SIZES:
        y = hint_amd.curve_features(xd[:N], n_points=P)
        assert y.shape == (N, 2) and y.dtype == torch.float32 and y.device == xd.device
        assert_band(x[:N], y, P, f"K {K} P {P} N {N}")
        if K == 1:
            assert bits_equal(y, torch.zeros_like(y))                     # every point is the same point: exactly (+0, +0)
    N = MULTI_TURN_N
    rows = -(-N // (2 * TILE))
    assert rows >= 3 and N % rows != 0 and N > (2 * TILE - 1) * rows      # every wavefront has rows, the last fewer
    y2 = run(xd[:N], P, max_groups=2)[0]
    assert_band(x[:N], y2, P, f"K {K} P {P} N {N} on two workgroups")
    assert lib.hint_curve_geometry(N, K, P, 0) > 2
    assert bits_equal(y2, hint_amd.curve_features(xd[:N], n_points=P))    # ... and the default grid gives the same bits
    assert bits_equal(y2, run(xd[:N], P, max_groups=1)[0])                # one workgroup: 4 wavefronts x 7 turns


# ---- 2. the tie rule where it matters ----
@pytest.mark.parametrize("a,b", ((2, 1), (1, 2), (3, 0.5)))
def test_tie_rule_on_ellipses(a, b):
    x = co.ellipse(a, b)
    y = hint_amd.curve_features(dev(x), n_points=101).cpu().numpy().astype(np.float64)
    bound = co.feature_bound(x)[0]
    print(f"ellipse ({a}, {b}): features {y[0]}, bound {bound:.3g}")
    # (dy, dx): a > b: the first of the tied pairs (0, 50), (50, 100) is (0, 50), so dx = -2a, never +2a; b > a: (25, 75), dy = -2b
    want = np.array([0.0, -2.0 * a]) if a > b else np.array([-2.0 * b, 0.0])
    assert np.abs(y[0] - want).max() <= bound
    assert len(co.band_check(x, y, 101)[0]) == 0


# ---- 3. the fixtures recorded from the reference ----
@pytest.mark.parametrize("case", co.GOLDEN_CASES, ids=lambda c: c["name"])
def test_fixtures_recorded_from_the_reference(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"curve_{case['name']}.npz"))
    x, ref_y = g["x"], g["ref_y"]
    n = len(x)
    xd = dev(x)
    y = hint_amd.curve_features(xd).cpu().numpy().astype(np.float64)
    B = co.feature_bound(x)
    ratio = (np.abs(y - ref_y).max(1) / B).max()
    print(f"{case['name']}: worst feature error / bound {ratio:.3g}")
    assert ratio <= 1.0                                                   # every row
    if not case["distance"]:
        return
    eps = co.golden_eps(case)
    t = g["y_target"]
    mean = hint_amd.mean_target_distance(xd, dev(t), 0.05, eps=dev(eps))
    assert mean.shape == () and mean.dtype == torch.float32
    d = co.distances64(ref_y + 0.05 * eps, t)
    bound = np.mean(np.sqrt(2.0) * B + 4 * U * d) + U * d.mean()
    ref = float(g["ref_mean"])
    print(f"{case['name']}: mean {mean.item():.9g}, reference {ref:.9g}, difference {abs(mean.item() - ref):.3g}, bound {bound:.3g}")
    assert abs(mean.item() - ref) <= bound
    # as the reference passes the target: expanded to [N, 2]
    expanded = dev(t)[None, :].expand(n, 2)
    assert bits_equal(hint_amd.mean_target_distance(xd, expanded, 0.05, eps=dev(eps)), mean)


# ---- 4. eps / noise / target ----
def test_eps_noise_and_target():
    N, P = 301, 100
    x = co.gauss(21, N, 5)
    xd = dev(x)
    rs = np.random.RandomState(22)
    e, t = rs.randn(N, 2).astype(np.float32), np.array([0.7, -1.1], np.float32)
    ed, td = dev(e), dev(t)
    cf = hint_amd.curve_features(xd)
    assert_band(x, cf, P, "curve_features")
    noise = 0.05
    y = hint_amd.lens_forward_process(xd, noise, eps=ed)
    want = cf.double() + float(np.float32(noise)) * ed.double()           # one fp32 rounding of this
    assert ((y.double() - want).abs() <= 2.0 ** -23 * want.abs() + 1e-37).all()
    assert not bits_equal(y, cf)
    assert bits_equal(hint_amd.lens_forward_process(xd, 0.0), cf)
    assert bits_equal(hint_amd.lens_forward_process(xd, 0), cf)
    assert bits_equal(hint_amd.lens_forward_process(xd, 0.0, eps=ed), cf)
    # distances: the device's arithmetic on its own features, against float64 (sub, square, fma, sqrt: 4 u)
    for nz, kw in ((0.0, {}), (noise, dict(eps=ed))):
        d = hint_amd.target_distances(xd, td, nz, **kw)
        assert d.shape == (N,) and d.dtype == torch.float32
        yy = hint_amd.lens_forward_process(xd, nz, **kw)
        d64 = co.distances64(yy.cpu().numpy(), t)
        err = np.abs(d.cpu().numpy().astype(np.float64) - d64)
        print(f"noise {nz}: worst distance error / (4 u dist) {(err / (4 * U * d64)).max():.3g}")
        assert (err <= 4 * U * d64).all()
        # ... and against the oracle's features: |dist - dist64| <= sqrt(2) feature bound + 4 u dist where the band holds one pair
        keep = co.unambiguous(x, P)
        f64 = co.features64(x, P)[0] + nz * e.astype(np.float64)
        o64 = co.distances64(f64, t)
        lim = np.sqrt(2.0) * (co.feature_bound(x) + U * np.abs(f64).max(1)) + 4 * U * o64
        assert keep.mean() >= 0.70 and (np.abs(d.cpu().numpy() - o64) <= lim)[keep].all()
        m = hint_amd.mean_target_distance(xd, td, nz, **kw)
        m64 = d.double().sum().item() / N
        assert abs(m.item() - m64) <= 2.0 ** -23 * m64                    # the double sum of its own distances, rounded once
        for tt in (td[None, :], td[None, :].expand(N, 2), td[None, :].expand(N, 2).contiguous(), t.tolist()):
            assert bits_equal(hint_amd.mean_target_distance(xd, tt, nz, **kw), m)
            assert bits_equal(hint_amd.target_distances(xd, tt, nz, **kw), d)
        # the mean's bits may depend on the grid (the order of the sum does), its value hardly
        y2, d2, m2 = run(xd, P, kw.get("eps"), nz, td, True, True, max_groups=3)
        assert bits_equal(y2, yy) and bits_equal(d2, d) and abs(m2.item() - m64) <= 2.0 ** -23 * m64
    # a generator: equal seeds agree bit for bit, and the noise is torch.randn's
    g1, g2 = torch.Generator(device=DEV).manual_seed(5), torch.Generator(device=DEV).manual_seed(5)
    a, b = hint_amd.lens_forward_process(xd, noise, generator=g1), hint_amd.lens_forward_process(xd, noise, generator=g2)
    assert bits_equal(a, b)
    drawn = torch.randn(N, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert bits_equal(a, hint_amd.lens_forward_process(xd, noise, eps=drawn))
    assert not bits_equal(a, hint_amd.lens_forward_process(xd, noise, generator=g1))
    m1 = hint_amd.mean_target_distance(xd, td, generator=torch.Generator(device=DEV).manual_seed(9))
    m2 = hint_amd.mean_target_distance(xd, td, generator=torch.Generator(device=DEV).manual_seed(9))
    assert bits_equal(m1, m2)
    # copies only where needed: float64 and non-contiguous x give the bits of their fp32 contiguous copy
    assert bits_equal(hint_amd.curve_features(xd.double()), cf)
    wide = torch.zeros(N, 40, device=DEV)
    wide[:, ::2] = xd
    assert bits_equal(hint_amd.curve_features(wide[:, ::2]), cf)


# ---- 5. invariants ----
def test_rows_do_not_depend_on_the_batch_or_the_grid():
    N = 157
    for K, P in ((5, 100), (25, 128), (3, 3)):
        xd = dev(co.gauss(31 + K, N, K))
        td = dev(np.array([0.2, 0.4], np.float32))
        y, d, _ = run(xd, P, target=td, want_dist=True, want_mean=True)
        y1, d1, _ = run(xd, P, target=td, want_dist=True, want_mean=True)
        assert bits_equal(y, y1) and bits_equal(d, d1)                    # two runs
        for r in (0, 77, N - 1):                                          # a row alone
            ya, da, _ = run(xd[r:r + 1].contiguous(), P, target=td, want_dist=True)
            assert bits_equal(ya[0], y[r]) and bits_equal(da[0], d[r])
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(DEV)      # every row somewhere else
        yp, dp, _ = run(xd[perm].contiguous(), P, target=td, want_dist=True)
        assert bits_equal(yp, y[perm]) and bits_equal(dp, d[perm])
        for mg in (1, 2, 7, 10 ** 6):
            ym, dm, _ = run(xd, P, target=td, want_dist=True, want_mean=True, max_groups=mg)
            assert bits_equal(ym, y) and bits_equal(dm, d), mg


def run_desc(x, N, K, P, eps, noise, target, y, dist, mean, ws, nbytes, max_groups=0, sync=True):
    lib = _lib.load()
    desc = _lib.CurveDesc()
    desc.x, desc.n_rows, desc.n_coeffs, desc.n_points, desc.eps, desc.noise, desc.target = x, N, K, P, eps, noise, target
    desc.y, desc.dist, desc.mean, desc.workspace, desc.workspace_bytes, desc.max_groups = y, dist, mean, ws, nbytes, max_groups
    st = lib.hint_curve_run(C.byref(desc), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.hint_last_error()
    if sync:                              # (tests/test_gpu_streams.py issues it behind a gate and must not wait)
        torch.cuda.synchronize()


@pytest.mark.parametrize("align", (16, 256))
@pytest.mark.parametrize("K,P,N", ((5, 100, 203), (25, 128, 66), (1, 2, 5)))
def test_run_ignores_what_outputs_and_workspace_held(K, P, N, align):
    """hint_curve_run on guard-banded buffers, with y, dist, mean and the workspace filled with zeros, NaNs or junk: the same
    bits every time, guards intact, inputs unchanged"""
    lib = _lib.load()
    x = co.gauss(41, N, K)
    rs = np.random.RandomState(42)
    gx = Guarded(N * 4 * K, align=align).set(torch.from_numpy(x))
    ge = Guarded(N * 2, align=align).set(torch.from_numpy(rs.randn(N, 2).astype(np.float32)))
    gt = Guarded(2, align=align).set(torch.tensor([0.5, -0.25]))
    nbytes = lib.hint_curve_workspace_bytes(N, K, P)
    assert nbytes % 4 == 0
    sx, se, st = gx.snapshot(), ge.snapshot(), gt.snapshot()
    first = None
    fills = [("zero", "zero"), ("zero", "zero")] + [(a, b) for a in FILLS[1:] for b in FILLS[1:]]
    for rep, (fill_o, fill_w) in enumerate(fills):
        gy = Guarded(2 * N, fill=fill_o, seed=rep, align=align)
        gd = Guarded(N, fill=fill_o, seed=50 + rep, align=align)
        gm = Guarded(1, fill=fill_o, seed=70 + rep, align=align)
        gw = Guarded(nbytes // 4, fill=fill_w, seed=100 + rep, align=256)
        run_desc(gx.ptr, N, K, P, ge.ptr, 0.05, gt.ptr, gy.ptr, gd.ptr, gm.ptr, gw.ptr, nbytes, max_groups=rep % 3)
        what = f"outputs {fill_o}, workspace {fill_w}"
        for gb, name in ((gy, "y"), (gd, "dist"), (gm, "mean"), (gw, "workspace")):
            gb.check_guards(f"{what}: {name}")
        for gb, snap, name in ((gx, sx, "x"), (ge, se, "eps"), (gt, st, "target")):
            gb.check_unchanged(snap, f"{what}: {name}")
        if first is None:
            first = (gy.t.clone(), gd.t.clone(), gm.t.clone())
        assert bits_equal(gy.t, first[0]) and bits_equal(gd.t, first[1]), what
        if rep % 3 == 0:
            assert bits_equal(gm.t, first[2]), what                       # (the same grid: the same order of the sum)
    assert bool(torch.isfinite(first[0]).all()) and bool(torch.isfinite(first[1]).all()) and bool(torch.isfinite(first[2]).all())
    # the Python route returns the same bits
    xd, ed, td = gx.view(N, 4 * K), ge.view(N, 2), gt.view(2)
    assert bits_equal(hint_amd.lens_forward_process(xd, 0.05, eps=ed, n_points=P).reshape(-1), first[0])
    assert bits_equal(hint_amd.target_distances(xd, td, 0.05, eps=ed, n_points=P), first[1])
    assert bits_equal(hint_amd.mean_target_distance(xd, td, 0.05, eps=ed, n_points=P).reshape(1), first[2])
    # without a target nothing but y is written; without mean the workspace is not touched (it may be null)
    gy = Guarded(2 * N, fill="nan", align=align)
    run_desc(gx.ptr, N, K, P, None, 0.0, None, gy.ptr, None, None, None, 0)
    gy.check_guards("y alone")
    assert bits_equal(gy.view(N, 2), hint_amd.curve_features(xd, n_points=P))


def test_rows_that_are_not_finite_leave_the_others_alone():
    N, P = 97, 100
    x = co.gauss(51, N, 5)
    xd = dev(x)
    td = dev(np.array([0.1, 0.2], np.float32))
    y, d, _ = run(xd, P, target=td, want_dist=True)
    bad = x.copy()
    spoiled = (0, 1, 2, 3, 40, 41, 64, 96)
    for n, r in enumerate(spoiled):
        bad[r, (3 * n) % 20] = (np.nan, np.inf, -np.inf)[n % 3]
    bad[41] = np.nan
    yb, db, mb = run(dev(bad), P, target=td, want_dist=True, want_mean=True, max_groups=2)
    torch.cuda.synchronize()
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[list(spoiled)] = False
    assert bits_equal(yb[keep], y[keep]) and bits_equal(db[keep], d[keep])
    assert_band(x[keep.cpu().numpy()], yb[keep], P, "finite rows beside non-finite ones")


# ---- 6. captured in a graph ----
def test_captured_in_a_graph_and_replayed_on_new_inputs():
    N, P = 4000, 100
    x, x2 = co.gauss(61, N, 5), co.gauss(62, N, 5)
    xd, td = dev(x), dev(np.array([1.0, -0.5], np.float32))
    ed = torch.randn(N, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    eager_d = hint_amd.target_distances(xd, td, 0.05, eps=ed).clone()     # (also loads the kernels before the capture)
    eager_m = hint_amd.mean_target_distance(xd, td, 0.05, eps=ed).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d = hint_amd.target_distances(xd, td, 0.05, eps=ed)
        m = hint_amd.mean_target_distance(xd, td, 0.05, eps=ed)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(d, eager_d) and bits_equal(m, eager_m)
    xd.copy_(dev(x2))                                                     # new samples in the same buffer
    g.replay()
    torch.cuda.synchronize()
    assert bits_equal(d, hint_amd.target_distances(xd, td, 0.05, eps=ed)) and not bits_equal(d, eager_d)
    assert bits_equal(m, hint_amd.mean_target_distance(xd, td, 0.05, eps=ed))
    y = hint_amd.lens_forward_process(xd, 0.0)
    assert_band(x2, y, P, "after the replay")
