"""hint_amd.curves trace_fourier_curves / hausdorff_distances / chamfer_distances / lens_fit_loss on the device against the float64
oracle of tests/hausdorff_oracle.py (its docstring states the comparison rule): the bound rule at every size the kernel takes
another path (traced and given curves, shared and ragged templates, with and without params), the traced points and their tie to
hint_curve_run, exact cases, the fixtures recorded from the reference, the invariants (a row's bits independent of the batch, the
position and the grid; guard-banded outputs over every fill; non-finite and bad ragged rows), and graph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves
from hint_amd._lib import HintAmdError
import curve_oracle as co
import hausdorff_oracle as ho
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -24
_geo = _lib.load().hint_hausdorff_geometry
TILE = _geo(1, 2, 1, 2)                                                   # template points of an LDS tile
IN_FLIGHT = _geo(1, 2, 1, 1)                                              # rows a workgroup has in flight
NS = tuple(sorted({1, 3, 2 * IN_FLIGHT + 1, 5}))                          # 2 * IN_FLIGHT + 1: one more than a max_groups = 2 grid holds
NMAX = max(NS)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def run(curve, P, tpl, offsets=None, params=None, points=False, max_groups=0):
    """the checked-argument route below the public functions, which also takes max_groups: (max_h, avg_h, chamfer, points)"""
    k = curve.shape[1] // 4 if curve.dim() == 2 else 0
    return curves._hd_run(curve, k, P, tpl, offsets, params, True, True, points, max_groups)


def assert_rule(ref, out, what, rows=None):
    mh, av, ch = (host(t) for t in out[:3])
    if rows is not None:
        ref = {k: v[rows] for k, v in ref.items()}
    bad, worst = ho.check(ref, mh, av, ch)
    print(f"{what}: worst error / bound {worst:.3g}")
    assert len(bad) == 0, (what, bad[:10], worst)


# ---- 1. the bound rule ----
KP = ((1, 2), (3, 33), (5, 63), (5, 64), (5, 65), (5, 100), (5, 257), (25, 1000), (5, 1024))
MS = (1, 2, 63, 65, 256, 257, TILE - 1, TILE, TILE + 1, 4096)
# the product thinned: every (K, P) and every M at least once, the largest of either with the smallest of the other
SHARED = (((1, 2), (1, 4096)), ((3, 33), (2, TILE + 1)), ((5, 63), (65, 256)), ((5, 64), (257, TILE - 1)), ((5, 65), (TILE, 63)),
          ((5, 100), (130, TILE + 1)), ((5, 257), (256, 2)), ((25, 1000), (1000, 257)), ((5, 1024), (4096, 1)))


def test_the_thinned_product_covers_every_value():
    assert tuple(kp for kp, _ in SHARED) == KP
    assert set(MS) <= {m for _, ms in SHARED for m in ms}
    assert {1, 3, 2 * IN_FLIGHT + 1} <= set(NS)


@pytest.mark.parametrize("KP_,Ms", SHARED, ids=lambda v: "-".join(map(str, v)))
def test_bound_rule_on_shared_templates(KP_, Ms):
    K, P = KP_
    x = co.gauss(100 * K + P, NMAX, K)
    xd = dev(x)
    b32 = co.points64(x, P).astype(np.float32)                            # the given source: some curve's points, as fp32 data
    bd = dev(b32)
    for M in Ms:
        tpl = ho.lens_template(M)
        td = dev(tpl)
        pr = ho.golden_params(K + P + M, NMAX)
        prd = dev(pr)
        ref_p, ref_0, ref_b = ho.distances64(x, tpl, pr, P=P), ho.distances64(x, tpl, None, P=P), ho.distances64(b32, tpl, pr)
        for N in NS:
            rows = slice(0, N)
            out = run(xd[:N], P, td, params=prd[:N])
            assert out[0].shape == (N,) and out[1].shape == (N,) and out[2].shape == (N, 2)
            assert all(t.dtype == torch.float32 and t.device == xd.device for t in out[:3])
            assert_rule(ref_p, out, f"K {K} P {P} M {M} N {N} traced, params", rows)
            assert_rule(ref_0, run(xd[:N], P, td), f"K {K} P {P} M {M} N {N} traced, no params", rows)
            given = run(bd[:N], P, td, params=prd[:N])
            assert_rule(ref_b, given, f"K {K} P {P} M {M} N {N} given, params", rows)
            if N > 2:                                                     # more rows than a grid of two holds at a time
                two = run(xd[:N], P, td, params=prd[:N], max_groups=2)
                assert all(bits_equal(a, b) for a, b in zip(two[:3], out[:3]))
        # the public functions return the same bits
        mh, av = hint_amd.hausdorff_distances(xd, td, prd, n_points=P)
        ch = hint_amd.chamfer_distances(xd, td, prd, n_points=P)
        full = run(xd, P, td, params=prd)
        assert bits_equal(mh, full[0]) and bits_equal(av, full[1]) and bits_equal(ch, full[2])
        mh, av = hint_amd.hausdorff_distances(bd, td, prd, n_points=7)    # n_points is ignored for points
        assert bits_equal(mh, given[0]) and bits_equal(av, given[1])


@pytest.mark.parametrize("K,P", ((5, 100), (3, 33), (25, 1000)))
def test_bound_rule_on_ragged_templates(K, P):
    lens = [1, 2, TILE - 1, TILE + 1, 4096, 130, TILE]                    # mixed in one call
    N = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tpl = np.concatenate([ho.lens_template(m) * np.float32(1 + 0.1 * i) for i, m in enumerate(lens)])
    x = co.gauss(7 * K + P, N, K)
    pr = ho.golden_params(K + P, N)
    xd, td, prd, od = dev(x), dev(tpl), dev(pr), dev(offsets, torch.int64)
    b32 = co.points64(x, P).astype(np.float32)
    for params, pd, name in ((pr, prd, "params"), (None, None, "no params")):
        ref = ho.distances64(x, tpl, params, offsets, P=P)
        out = run(xd, P, td, od, pd)
        assert_rule(ref, out, f"K {K} P {P} ragged traced, {name}")
        assert all(bits_equal(a, b) for a, b in zip(run(xd, P, td, od, pd, max_groups=2)[:3], out[:3]))
    assert_rule(ho.distances64(b32, tpl, pr, offsets), run(dev(b32), P, td, od, prd), f"K {K} P {P} ragged given, params")
    # offsets from the host (a list, a CPU tensor) are checked and uploaded: the same bits
    with_params = run(xd, P, td, od, prd)
    mh, av = hint_amd.hausdorff_distances(xd, td, prd, offsets=offsets.tolist(), n_points=P)
    assert bits_equal(mh, with_params[0]) and bits_equal(av, with_params[1])
    ch = hint_amd.chamfer_distances(xd, td, prd, offsets=torch.from_numpy(offsets), n_points=P)
    assert bits_equal(ch, with_params[2])
    with pytest.raises(HintAmdError, match="offsets must ascend"):
        hint_amd.hausdorff_distances(xd, td, prd, offsets=(offsets + 1).tolist(), n_points=P)


# ---- 2. the traced points ----
def fma32(a, b, c):
    """the exactly rounded fp32 fma of fp32 values (float64 arrays holding them): a b is exact in float64; the float64 sum s and
    its exact residual e (two-sum) decide the rounding - s alone unless s is a tie between two fp32 values and e is not 0"""
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    toward = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & (s == (r.astype(np.float64) + toward.astype(np.float64)) / 2) & (e != 0)
    return np.where(tie & (np.sign(e) == np.sign(d)), toward, r).astype(np.float32)


def first_maximum_features(pts):
    """hint_curve_run's rule on fp32 points [N, P, 2]: D = fma(dy, dy, dx dx) of p_i - p_j, i < j, the first maximum in
    row-major order; features (p_j.y - p_i.y, p_j.x - p_i.x) in fp32"""
    iu, ju = np.triu_indices(pts.shape[1], 1)
    d = pts[:, iu, :] - pts[:, ju, :]                                      # fp32 subtractions
    dy = d[:, :, 1].astype(np.float64)
    D = fma32(dy, dy, (d[:, :, 0] * d[:, :, 0]).astype(np.float64))                  # (the product: one fp32 rounding)
    best = D.argmax(1)
    rows = np.arange(len(pts))
    f = pts[rows, ju[best], :] - pts[rows, iu[best], :]
    return f[:, ::-1]


def test_fma32_is_the_exactly_rounded_fma():
    # a b = 2^36 - 2^-10: added to c it lies just below the middle of two fp32 values, and the float64 sum IS that middle
    a = np.array([2.0 ** 36 * (1 + 2.0 ** -23), 2.0 ** 36 * (1 + 2.0 ** -23), 3.0, 2.0 ** -24])
    b = np.array([1 - 2.0 ** -23, 1 - 2.0 ** -23, 5.0, 1.0])
    c = np.array([2.0 ** 60 + 2.0 ** 37, 2.0 ** 60, 2.0, 1.0])
    assert all(np.array_equal(v, v.astype(np.float32).astype(np.float64)) for v in (a, b, c))
    want = np.array([2.0 ** 60 + 2.0 ** 37, 2.0 ** 60, 17.0, 1.0], np.float32)       # (the last: an exact tie, to even)
    assert np.array_equal(fma32(a, b, c), want)
    assert (a * b + c).astype(np.float32)[0] == np.float32(2.0 ** 60 + 2.0 ** 38)    # rounding twice gets the first one wrong


@pytest.mark.parametrize("K,P", KP)
def test_traced_points(K, P):
    N = 37
    x = co.gauss(300 + K + P, N, K)
    xd = dev(x)
    pts = hint_amd.trace_fourier_curves(xd, n_points=P)
    assert pts.shape == (N, P, 2) and pts.dtype == torch.float32 and pts.device == xd.device
    dB = (2 * K + 2) * U * co.scale(x)
    err = np.abs(host(pts) - co.points64(x, P)).max((1, 2))
    print(f"K {K} P {P}: worst point error / delta_B {(err / dB).max():.3g}")
    assert (err <= dB).all()
    assert bits_equal(pts[:, P - 1], pts[:, 0])                           # the angle is reduced exactly
    # the same points next to the distances, on any grid
    for mg in (0, 1, 2):
        assert bits_equal(run(xd, P, dev(ho.lens_template(7)), points=True, max_groups=mg)[3], pts)
    if P <= 128:                                                          # the tie to hint_curve_kernel: its points are these bits
        want = first_maximum_features(pts.cpu().numpy())
        assert bits_equal(hint_amd.curve_features(xd, n_points=P), dev(want))
    else:
        with pytest.raises(HintAmdError, match="n_points must be 2..128"):
            hint_amd.curve_features(xd, n_points=P)
    if K == 5 and P == 100:
        assert bits_equal(hint_amd.trace_fourier_curves(xd), pts)         # the default, as the reference's
        assert bits_equal(hint_amd.trace_fourier_curves(xd.double(), P), pts)
        with pytest.raises(HintAmdError, match="x requires grad"):
            hint_amd.trace_fourier_curves(xd.clone().requires_grad_(), P)
        with torch.no_grad():
            assert bits_equal(hint_amd.trace_fourier_curves(xd.clone().requires_grad_(), P), pts)


# ---- 3. exact cases ----
@pytest.mark.parametrize("P", (2, 100, 257, 1024))
def test_a_template_equal_to_the_curve_gives_exact_zeros(P):
    N = 5
    b = np.random.RandomState(P).randn(N, P, 2).astype(np.float32)
    offsets = (np.arange(N + 1) * P).astype(np.int64)
    mh, av, ch, _ = run(dev(b), P, dev(b.reshape(-1, 2)), dev(offsets, torch.int64))
    for t in (mh, av, ch):
        assert bits_equal(t, torch.zeros_like(t))                         # +0, every bit
    mh, av, ch, _ = run(dev(b[:1]), P, dev(b[0]))                         # ... and shared
    assert bits_equal(mh, torch.zeros_like(mh)) and bits_equal(av, torch.zeros_like(av)) and bits_equal(ch, torch.zeros_like(ch))


@pytest.mark.parametrize("P", (2, 63, 1000))
def test_a_single_point_at_distance_r_gives_exactly_r(P):
    b = np.tile(np.array([1.0, 2.0], np.float32), (3, P, 1))
    mh, av, ch, _ = run(dev(b), P, dev(np.array([[4.0, 6.0]], np.float32)))
    assert bits_equal(mh, torch.full_like(mh, 5.0)) and bits_equal(av, torch.full_like(av, 5.0))
    assert bits_equal(ch, torch.full_like(ch, 25.0))
    # ... and moved there by params: (1.5, 2) scaled by 2 and moved by (1, 2), angle 0 (cos = 1, sin = 0: every step exact)
    pr = np.tile(np.array([1.0, 2.0, 2.0, 0.0], np.float32), (3, 1))
    mh, av, ch, _ = run(dev(b), P, dev(np.array([[1.5, 2.0]], np.float32)), params=dev(pr))
    assert bits_equal(mh, torch.full_like(mh, 5.0)) and bits_equal(av, torch.full_like(av, 5.0))
    assert bits_equal(ch, torch.full_like(ch, 25.0))


# ---- 4. the fixtures recorded from the reference ----
@pytest.mark.parametrize("case", ho.GOLDEN_CASES, ids=lambda c: c["name"])
def test_fixtures_recorded_from_the_reference(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"hausdorff_{case['name']}.npz"))
    x, tpl, pr = g["x"], g["template"], g["params"]
    xd, td, prd = dev(x), dev(tpl), dev(pr)
    ref = ho.distances64(x, tpl, pr, P=ho.GOLDEN_P)                        # for the bounds; the values are the reference's
    mh, av = hint_amd.hausdorff_distances(xd, td, prd)                    # n_points = 1000 is the default
    r_max, r_avg = np.abs(host(mh) - g["ref_max_h"]) / ref["E"], np.abs(host(av) - g["ref_avg_h"]) / ref["e_avg"]
    print(f"{case['name']}: worst max_h error / bound {r_max.max():.3g}, avg_h {r_avg.max():.3g}")
    assert (r_max <= 1).all() and (r_avg <= 1).all()
    pts = host(hint_amd.trace_fourier_curves(xd, ho.GOLDEN_P))
    dB = 12 * U * co.scale(x)
    assert np.abs(pts[0] - g["ref_points_first"]).max() <= dB[0] + 3e-14 and np.abs(pts[-1] - g["ref_points_last"]).max() <= dB[-1] + 3e-14
    # the loss of the fit, on the 100 points the fit sees: chamfer0 + w chamfer1, then one product and one sum in fp32
    fit = ho.distances64(x, tpl, pr, P=ho.GOLDEN_FIT_P)
    for w, weight in enumerate(ho.GOLDEN_WEIGHTS):
        loss = hint_amd.lens_fit_loss(xd, td, prd, weight)
        assert loss.shape == (len(x),) and loss.dtype == torch.float32
        want = g["ref_loss"][:, w]
        bound = (1 + weight) * fit["e_ch"] + 2 * U * np.abs(want)
        r = np.abs(host(loss) - want) / bound
        print(f"{case['name']}: weight {weight}: worst loss error / bound {r.max():.3g}")
        assert (r <= 1).all()
    ch = hint_amd.chamfer_distances(xd, td, prd, n_points=ho.GOLDEN_FIT_P)
    assert bits_equal(hint_amd.lens_fit_loss(xd, td, prd), ch[:, 0] + ch[:, 1])
    # the fit's own points as input: the same bits as tracing them here
    p100 = hint_amd.trace_fourier_curves(xd)
    assert bits_equal(hint_amd.lens_fit_loss(p100, td, prd, 0.25), hint_amd.lens_fit_loss(xd, td, prd, 0.25))


# ---- 5. invariants ----
def ragged_case(K, P, lens, seed):
    N = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tpl = np.concatenate([ho.lens_template(m) * np.float32(1 + 0.1 * i) for i, m in enumerate(lens)])
    return co.gauss(seed, N, K), tpl, ho.golden_params(seed, N), offsets


@pytest.mark.parametrize("K,P", ((5, 100), (5, 257), (25, 1000)))
def test_rows_do_not_depend_on_the_batch_the_position_or_the_grid(K, P):
    lens = [130, 1, TILE + 1, 64, 257, 2, 2 * TILE + 3, 130, 65]
    N = len(lens)
    x, tpl, pr, offsets = ragged_case(K, P, lens, 40 + K + P)
    xd, td, prd, od = dev(x), dev(tpl), dev(pr), dev(offsets, torch.int64)
    out = run(xd, P, td, od, prd, points=True)
    again = run(xd, P, td, od, prd, points=True)
    assert all(bits_equal(a, b) for a, b in zip(out, again))             # two runs
    for mg in (1, 2, 3, 10 ** 6):
        assert all(bits_equal(a, b) for a, b in zip(out, run(xd, P, td, od, prd, points=True, max_groups=mg))), mg
    for r in (0, 2, 6, N - 1):                                            # a row alone, its template shared
        one = run(xd[r:r + 1].contiguous(), P, td[offsets[r]:offsets[r + 1]].contiguous(), None, prd[r:r + 1].contiguous(), points=True)
        assert all(bits_equal(a[0], b[r]) for a, b in zip(one, out)), r
    perm = np.random.RandomState(3).permutation(N)                        # every row somewhere else
    tpl_p = np.concatenate([tpl[offsets[r]:offsets[r + 1]] for r in perm])
    off_p = np.concatenate([[0], np.cumsum([lens[r] for r in perm])]).astype(np.int64)
    pd = torch.from_numpy(perm).to(DEV)
    moved = run(xd[pd].contiguous(), P, dev(tpl_p), dev(off_p, torch.int64), prd[pd].contiguous(), points=True)
    assert all(bits_equal(a, b[pd]) for a, b in zip(moved, out))
    # the given source on the traced points: the same distances
    given = run(out[3], P, td, od, prd)
    assert all(bits_equal(a, b) for a, b in zip(given[:3], out[:3]))
    # copies only where needed: other floating dtypes and strides give the bits of their fp32 contiguous copy
    mh, av = hint_amd.hausdorff_distances(xd.double(), td.double(), prd.double(), offsets=od, n_points=P)
    assert bits_equal(mh, out[0]) and bits_equal(av, out[1])
    wide = torch.zeros(N, 8 * K, device=DEV)
    wide[:, ::2] = xd
    assert bits_equal(hint_amd.chamfer_distances(wide[:, ::2], td, prd, offsets=od, n_points=P), out[2])
    with pytest.raises(HintAmdError, match="template requires grad"):
        hint_amd.hausdorff_distances(xd, td.clone().requires_grad_(), prd, offsets=od, n_points=P)
    with pytest.raises(HintAmdError, match="params is on cpu"):
        hint_amd.hausdorff_distances(xd, td, prd.cpu(), offsets=od, n_points=P)


def run_desc(x, b, N, K, P, a, offs, prm, T, max_h, avg_h, chamfer, points, max_groups=0, sync=True):
    lib = _lib.load()
    desc = _lib.HausdorffDesc()
    desc.x, desc.b_points, desc.n_rows, desc.n_coeffs, desc.n_points = x, b, N, K, P
    desc.a_points, desc.a_offsets, desc.a_params, desc.n_template = a, offs, prm, T
    desc.max_h, desc.avg_h, desc.chamfer, desc.points, desc.max_groups = max_h, avg_h, chamfer, points, max_groups
    st = lib.hint_hausdorff_run(C.byref(desc), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.hint_last_error()
    if sync:                              # (tests/test_gpu_streams.py issues it behind a gate and must not wait)
        torch.cuda.synchronize()


@pytest.mark.parametrize("align", (16, 256))
@pytest.mark.parametrize("K,P,lens", ((5, 100, (130, 1, 2, 65)), (25, 1000, (TILE + 1, 7)), (1, 2, (1, 3, 2))))
def test_run_ignores_what_the_outputs_held(K, P, lens, align):
    """hint_hausdorff_run on guard-banded buffers, with max_h, avg_h, chamfer and points filled with zeros, NaNs or junk: the same
    bits every time, guards intact, inputs unchanged"""
    N = len(lens)
    x, tpl, pr, offsets = ragged_case(K, P, lens, 50 + K)
    T = len(tpl)
    gx = Guarded(N * 4 * K, align=align).set(torch.from_numpy(x))
    ga = Guarded(2 * T, align=align).set(torch.from_numpy(tpl))
    gp = Guarded(4 * N, align=align).set(torch.from_numpy(pr))
    go = Guarded(2 * (N + 1), align=align, dtype=torch.int64).set(torch.from_numpy(offsets).view(torch.int32))
    snaps = [g.snapshot() for g in (gx, ga, gp, go)]
    first = None
    for rep, fill in enumerate(("zero",) + FILLS):
        outs = [Guarded(n, fill=fill, seed=10 * rep + i, align=align) for i, n in enumerate((N, N, 2 * N, 2 * N * P))]
        run_desc(gx.ptr, None, N, K, P, ga.ptr, go.ptr, gp.ptr, T, *(g.ptr for g in outs), max_groups=rep % 3)
        for gb, name in zip(outs, ("max_h", "avg_h", "chamfer", "points")):
            gb.check_guards(f"outputs {fill}: {name}")
        for gb, snap, name in zip((gx, ga, gp, go), snaps, ("x", "a_points", "a_params", "a_offsets")):
            gb.check_unchanged(snap, f"outputs {fill}: {name}")
        if first is None:
            first = [g.t.clone() for g in outs]
        assert all(bits_equal(g.t, f) for g, f in zip(outs, first)), fill
    assert all(bool(torch.isfinite(f).all()) for f in first)
    # the Python route returns the same bits
    xd, td, prd, od = gx.view(N, 4 * K), ga.view(T, 2), gp.view(N, 4), go.raw[go.off:go.off + 2 * (N + 1)].view(torch.int64)
    out = run(xd, P, td, od, prd, points=True)
    assert all(bits_equal(a.reshape(-1), f) for a, f in zip(out, first))
    # one output alone: the others may be null, and the given source reads b_points as it read its own trace
    for i in range(3):
        gb = Guarded((N, N, 2 * N)[i], fill="nan", align=align)
        ptrs = [None, None, None, None]
        ptrs[i] = gb.ptr
        run_desc(None, outs[3].ptr, N, 0, P, ga.ptr, go.ptr, gp.ptr, T, *ptrs)
        gb.check_guards(f"output {i} alone")
        assert bits_equal(gb.t, first[i])
    gq = Guarded(2 * N * P, fill="nan", align=align)
    run_desc(gx.ptr, None, N, K, P, gx.ptr, None, None, 1, None, None, None, gq.ptr)      # points alone: no template is read
    gq.check_guards("points alone")
    assert bits_equal(gq.t, first[3])


def test_rows_that_are_not_finite_and_bad_ragged_rows_leave_the_others_alone():
    K, P = 5, 100
    lens = [130, 7, 65, 1, TILE + 1, 33, 2, 64, 9]
    N = len(lens)
    x, tpl, pr, offsets = ragged_case(K, P, lens, 61)
    T = len(tpl)
    td = dev(tpl)
    good = run(dev(x), P, td, dev(offsets, torch.int64), dev(pr), points=True)
    torch.cuda.synchronize()
    # rows whose inputs are not finite
    bx, bp = x.copy(), pr.copy()
    bx[0, 3], bx[4, 0], bx[8] = np.nan, np.inf, -np.inf
    bp[2, 3], bp[6, 2], bp[7, 0] = np.inf, np.nan, -np.inf
    spoiled = [0, 2, 4, 6, 7, 8]
    out = run(dev(bx), P, td, dev(offsets, torch.int64), dev(bp), points=True, max_groups=2)
    torch.cuda.synchronize()
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[spoiled] = False
    assert all(bits_equal(a[keep], b[keep]) for a, b in zip(out, good))
    btpl = tpl.copy()
    btpl[offsets[5] + 3] = np.nan                                          # one template point of row 5
    out = run(dev(x), P, dev(btpl), dev(offsets, torch.int64), dev(pr))
    torch.cuda.synchronize()
    keep[:] = True
    keep[5] = False
    assert all(bits_equal(a[keep], b[keep]) for a, b in zip(out[:3], good[:3]))
    # ragged rows with a bad length - offsets on the device, where nobody checked them: 0 points, more than 4096, a negative
    # length, a range past the end of a_points, a negative start.  Such rows get NaN; every other row is what its range gives
    alone = lambda r, o0, o1: run(dev(x[r:r + 1]), P, dev(tpl[o0:o1]), None, dev(pr[r:r + 1]))      # noqa: E731
    for bad_offsets in ([0, 130, 130, 202, 203, 1228, T - 75, T - 73, T - 9, T],          # row 1: 0 points
                        [0, 130, 137, 202, 203, 203 + 4097, T - 75, T - 73, T - 9, T],    # row 4: 4097 points, row 5: a negative length
                        [0, 130, 137, 100, 203, 1228, T - 75, T - 73, T + 1, T],          # rows 2, 8: negative lengths, row 7: past the end
                        [-3, 130, 137, 202, 203, 1228, T - 75, T - 73, T - 9, T + (1 << 40)]):       # row 0: a negative start, row 8: far past the end
        bo = np.array(bad_offsets, np.int64)
        out = run(dev(x), P, td, dev(bo, torch.int64), dev(pr), points=True, max_groups=2)
        torch.cuda.synchronize()
        n_bad = 0
        for r in range(N):
            o0, o1 = int(bo[r]), int(bo[r + 1])
            if o0 < 0 or o1 > T or not 1 <= o1 - o0 <= 4096:
                n_bad += 1
                assert bool(torch.isnan(out[0][r])) and bool(torch.isnan(out[1][r])) and bool(torch.isnan(out[2][r]).all()), (bad_offsets, r)
            else:
                one = alone(r, o0, o1)
                assert all(bits_equal(a[0], b[r]) for a, b in zip(one[:3], out[:3])), (bad_offsets, r)
        assert n_bad >= 1
        assert bits_equal(out[3], good[3])                                # the points do not depend on the template
    # a length above 4096 inside a_points
    big = ho.lens_template(5000)
    out = run(dev(x[:2]), P, dev(big), dev(np.array([0, 4097, 5000], np.int64), torch.int64), dev(pr[:2]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0][0])) and bool(torch.isnan(out[1][0])) and bool(torch.isnan(out[2][0]).all())
    one = run(dev(x[1:2]), P, dev(big[4097:]), None, dev(pr[1:2]))
    assert all(bits_equal(a[0], b[1]) for a, b in zip(one[:3], out[:3]))
    # the host refuses such offsets when it can see them
    with pytest.raises(HintAmdError, match="offsets must ascend by 1..4096"):
        hint_amd.hausdorff_distances(dev(x), td, dev(pr), offsets=[0, 130, 130, 202, 203, 1228, T - 75, T - 73, T - 9, T], n_points=P)


# ---- 6. captured in a graph ----
def test_captured_in_a_graph_and_replayed_on_new_inputs():
    N, K, P, M = 64, 5, 257, 130
    x, x2 = co.gauss(71, N, K), co.gauss(72, N, K)
    pr = ho.golden_params(73, N)
    xd, td, prd = dev(x), dev(ho.lens_template(M)), dev(pr)
    eager = hint_amd.hausdorff_distances(xd, td, prd, n_points=P)         # (also loads the kernel before the capture)
    eager_c = hint_amd.chamfer_distances(xd, td, prd, n_points=P)
    eager_p = hint_amd.trace_fourier_curves(xd, P)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mh, av = hint_amd.hausdorff_distances(xd, td, prd, n_points=P)
        ch = hint_amd.chamfer_distances(xd, td, prd, n_points=P)
        pts = hint_amd.trace_fourier_curves(xd, P)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(mh, eager[0]) and bits_equal(av, eager[1]) and bits_equal(ch, eager_c) and bits_equal(pts, eager_p)
    xd.copy_(dev(x2))                                                     # new samples in the same buffer
    prd.copy_(dev(ho.golden_params(74, N)))
    g.replay()
    torch.cuda.synchronize()
    now = hint_amd.hausdorff_distances(xd, td, prd, n_points=P)
    assert bits_equal(mh, now[0]) and bits_equal(av, now[1]) and not bits_equal(mh, eager[0])
    assert bits_equal(ch, hint_amd.chamfer_distances(xd, td, prd, n_points=P))
    assert_rule(ho.distances64(x2, ho.lens_template(M), ho.golden_params(74, N), P=P), (mh, av, ch), "after the replay")
