"""CPU-side checks of hint_amd.curves and the hint_curve_* entry points (no GPU): header, exports and binding agree, every
argument check of hint_curve_run comes before any device call and names its field, hint_curve_geometry and
hint_curve_workspace_bytes keep their limits, the Python functions refuse bad arguments by name, the test-side float64
evaluation (tests/curve_oracle.py) reproduces the outputs recorded from the reference's forward_process and
mean_target_distance, and its comparison rule accepts itself and rejects a sign flip, swapped components and a neighbouring
pair."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves
from hint_amd._lib import HintAmdError
import curve_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_curve_workspace_bytes", "hint_curve_run", "hint_curve_geometry")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
U = 2.0 ** -24


def good_desc(n_rows=4000, K=5, P=100):
    lib = _lib.load()
    desc = _lib.CurveDesc()
    desc.x, desc.eps, desc.target, desc.y, desc.dist, desc.mean, desc.workspace = (BASE + (i << 28) for i in range(7))
    desc.n_rows, desc.n_coeffs, desc.n_points, desc.noise, desc.max_groups = n_rows, K, P, 0.05, 0
    desc.workspace_bytes = lib.hint_curve_workspace_bytes(n_rows, K, P)
    assert desc.workspace_bytes > 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_curve_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert set(_lib.exported_symbols()) == declared
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    for cite in ("data.py:127-139", "data.py:51-57", "data.py:30-40", "rejection_sampling.py:99-102", ":204",
                 "rejection_sampling.py:76-85"):
        assert cite in header, cite
    # pointer, int64, 2 int32, pointer, float (+ 4 bytes of padding), 5 pointers, size_t, int32 (+ 4)
    D = _lib.CurveDesc
    assert C.sizeof(D) == 8 + 8 + 8 + 8 + 8 + 5 * 8 + 8 + 8 == 96
    assert (D.n_rows.offset, D.n_points.offset, D.eps.offset, D.noise.offset, D.target.offset) == (8, 20, 24, 32, 40)
    assert (D.mean.offset, D.workspace_bytes.offset, D.max_groups.offset) == (64, 80, 88)
    struct = re.search(r"typedef struct hint_curve_desc \{(.*?)\} hint_curve_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f[0] for f in D._fields_]                          # the same fields in the same order
    for fn in ("curve_features", "lens_forward_process", "target_distances", "mean_target_distance"):
        assert getattr(hint_amd, fn) is getattr(curves, fn)
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("x", "y"):
        desc = good_desc()
        setattr(desc, field, None)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} is null" in msg, msg
    for bad in (0, -3, (1 << 30) + 1):
        desc = good_desc()
        desc.n_rows = bad
        st, msg = run_msg(desc)
        assert st != 0 and "n_rows must be 1..1073741824" in msg and f"got {bad}" in msg, msg
    for bad in (0, -1, 2, 4, 24, 26, 27):
        desc = good_desc()
        desc.n_coeffs = bad
        st, msg = run_msg(desc)
        assert st != 0 and "n_coeffs must be odd and 1..25" in msg and f"got {bad}" in msg, msg
    for bad in (-1, 0, 1, 129):
        desc = good_desc()
        desc.n_points = bad
        st, msg = run_msg(desc)
        assert st != 0 and "n_points must be 2..128" in msg and f"got {bad}" in msg, msg
    for field in ("dist", "mean"):
        desc = good_desc()
        desc.target = None
        setattr(desc, "mean" if field == "dist" else "dist", None)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} needs a target" in msg, msg
    desc = good_desc()
    desc.max_groups = -1
    st, msg = run_msg(desc)
    assert st != 0 and "max_groups must be >= 0" in msg, msg
    for bad in (float("nan"), float("inf")):
        desc = good_desc()
        desc.noise = bad
        st, msg = run_msg(desc)
        assert st != 0 and "noise must be finite" in msg, msg
    for field in ("x", "eps", "target", "y", "dist", "mean"):
        desc = good_desc()
        setattr(desc, field, BASE + (9 << 28) + 2)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} must be 4-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace = None
    st, msg = run_msg(desc)
    assert st != 0 and "workspace is null" in msg, msg
    desc = good_desc()
    desc.workspace = BASE + (6 << 28) + 8
    st, msg = run_msg(desc)
    assert st != 0 and "workspace must be 16-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace_bytes -= 1
    st, msg = run_msg(desc)
    assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_workspace_bytes_rejects_what_run_rejects_and_does_not_grow_with_n():
    lib = _lib.load()
    for args, what in (((0, 5, 100), "n_rows"), (((1 << 30) + 1, 5, 100), "n_rows"), ((10, 0, 100), "n_coeffs"),
                       ((10, 4, 100), "n_coeffs"), ((10, 27, 100), "n_coeffs"), ((10, 5, 1), "n_points"), ((10, 5, 129), "n_points")):
        assert lib.hint_curve_workspace_bytes(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    cap, tile = lib.hint_curve_geometry(1, 1, 2, 3), lib.hint_curve_geometry(1, 1, 2, 1)
    small = lib.hint_curve_workspace_bytes(1, 1, 2)
    assert small == cap * tile * 8                                        # one double per wavefront of the largest grid
    for args in ((4000, 5, 100), (10 ** 8, 5, 100), (1 << 30, 25, 128)):
        assert lib.hint_curve_workspace_bytes(*args) == small <= 1 << 20


def test_geometry_is_consistent():
    lib = _lib.load()
    assert lib.hint_curve_geometry(0, 5, 100, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert lib.hint_curve_geometry(10, 6, 100, 0) == -1 and "n_coeffs" in lib.hint_last_error().decode()
    assert lib.hint_curve_geometry(10, 5, 200, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert lib.hint_curve_geometry(10, 5, 100, 4) == -1 and "field" in lib.hint_last_error().decode()
    assert lib.hint_curve_geometry(10, 5, 100, -1) == -1
    tile, cap = lib.hint_curve_geometry(1, 5, 100, 1), lib.hint_curve_geometry(1, 5, 100, 3)
    assert tile == 4 and cap >= 256
    for N in (1, 2, tile - 1, tile, tile + 1, 63, 64, 65, 4000, tile * cap - 1, tile * cap, tile * cap + 1, 10 ** 8, 1 << 30):
        for K, P in ((5, 100), (1, 2), (25, 128)):
            g, tl, r, c = (lib.hint_curve_geometry(N, K, P, f) for f in range(4))
            assert (tl, c) == (tile, cap)
            assert 1 <= g <= cap and r >= 1
            assert g * tile * r >= N                                      # the wavefronts' ranges cover every row
            assert g == min(cap, -(-N // tile)) and r == -(-N // (g * tile))
            assert g * tile * (r - 1) < N                                 # no smaller row count would do
    assert lib.hint_curve_geometry(4000, 5, 100, 0) == 1000 and lib.hint_curve_geometry(4000, 5, 100, 2) == 1
    assert lib.hint_curve_geometry(10 ** 8, 5, 100, 0) == cap


def test_python_argument_errors():
    x, t = torch.randn(50, 20), torch.randn(2)
    for fn, args in ((hint_amd.curve_features, (x,)), (hint_amd.lens_forward_process, (x,)),
                     (hint_amd.target_distances, (x, t)), (hint_amd.mean_target_distance, (x, t))):
        with pytest.raises(HintAmdError, match=fn.__name__ + ": x is on cpu.*no CPU fallback"):
            fn(*args)
        with pytest.raises(HintAmdError, match=fn.__name__ + ": x must be a tensor"):
            fn(x.numpy(), *args[1:])
        with pytest.raises(HintAmdError, match=fn.__name__ + ": x must be 2-D"):
            fn(x[0], *args[1:])
    # the remaining checks sit behind the device check: they are reached through the helpers the public functions call
    for shape in ((0, 20), (5, 0), (5, 19), (5, 8), (5, 16), (5, 104), (5, 108)):
        with pytest.raises(HintAmdError, match="curve_features: x must hold"):
            curves._check_shape(shape, "curve_features")
    assert [curves._check_shape((3, 4 * k), "f") for k in (1, 3, 5, 25)] == [1, 3, 5, 25]
    for bad, what in ((1, "n_points must be 2..128"), (129, "n_points must be 2..128"), (100.0, "n_points must be an int"),
                      (True, "n_points must be an int")):
        with pytest.raises(HintAmdError, match="lens_forward_process: " + what):
            curves._check_points(bad, "lens_forward_process")
    assert curves._check_points(2, "f") == 2 and curves._check_points(128, "f") == 128
    for bad, what in (("a", "noise must be a number"), (None, "noise must be a number"), (float("nan"), "noise must be finite"),
                      (float("inf"), "noise must be finite")):
        with pytest.raises(HintAmdError, match="target_distances: " + what):
            curves._check_real(bad, "noise", "target_distances", nonneg=False)
    for bad in (torch.randn(3), torch.randn(2, 3), torch.randn(7, 2), torch.randn(1, 1, 2)):
        with pytest.raises(HintAmdError, match=r"mean_target_distance: y_target must have shape \[2\], \[1, 2\] or \[50, 2\]"):
            curves._check_target(bad, 50, "cpu", "mean_target_distance")
    with pytest.raises(HintAmdError, match="y_target must be a tensor or an array-like"):
        curves._check_target(object(), 50, "cpu", "mean_target_distance")
    want = torch.tensor([1.5, -2.0])
    for ok in (want, want[None], want[None].expand(50, 2), [1.5, -2.0], np.array([[1.5, -2.0]])):
        got = curves._check_target(ok, 50, "cpu", "f")
        assert got.shape == (2,) and got.dtype == torch.float32 and torch.equal(got, want)
    for bad, what in ((np.zeros((50, 2)), "eps must be a tensor"), (torch.zeros(50), "eps must have shape"),
                      (torch.zeros(49, 2), "eps must have shape")):
        with pytest.raises(HintAmdError, match="lens_forward_process: " + what):
            curves._check_eps(bad, x, "lens_forward_process")
    with pytest.raises(HintAmdError, match="generator must be a torch.Generator"):
        curves._noise_args(x, 0.05, None, 3, "lens_forward_process")
    assert curves._noise_args(x, 0, None, None, "f") == (0.0, None)       # noise = 0: no eps is drawn, the call is curve_features


@pytest.mark.parametrize("case", co.GOLDEN_CASES, ids=lambda c: c["name"])
def test_float64_oracle_reproduces_the_reference_outputs(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"curve_{case['name']}.npz"))
    x, ref_y = g["x"], g["ref_y"]
    n = case["rows"]
    assert x.shape == (n, 20) and x.dtype == np.float32 and ref_y.shape == (n, 2) and ref_y.dtype == np.float64
    draw, keep = co.golden_draw(case)
    assert keep.mean() >= 0.70                                            # a bad family fails loudly
    assert np.array_equal(draw[keep][:n], x)                              # the fixture's rows: the unambiguous ones of the draw
    assert co.unambiguous(x, 100).all()
    feat, pair, _ = co.features64(x, 100)
    assert np.abs(feat - ref_y).max() <= 1e-12
    assert (pair[:, 0] < pair[:, 1]).all()
    if not case["distance"]:
        assert "ref_mean" not in g.files
        return
    assert int(g["seed"]) == case["seed"]
    # the reference: forward_process(x) = features + 0.05 randn in float64, cast to fp32, then sub, square, sum, sqrt, mean in fp32
    y = feat + 0.05 * co.golden_eps(case)
    d = co.distances64(y, g["y_target"])
    ref = float(g["ref_mean"])
    # per row: each component of y rounded to fp32 (u |y|, sqrt(2) u max|y| on the distance), then four rounded operations
    # (4 u dist); the fp32 mean of n values in any order: (n - 1) u mean, and its own rounding
    bound = np.mean(np.sqrt(2.0) * U * np.abs(y).max(1) + 4 * U * d) + n * U * d.mean()
    print(f"{case['name']}: oracle mean {d.mean():.9g}, reference {ref:.9g}, difference {abs(d.mean() - ref):.3g}, bound {bound:.3g}")
    assert abs(d.mean() - ref) <= bound


def _family(K, P, seed=7, N=600):
    x = co.gauss(seed, N, K)
    return x, co.unambiguous(x, P)


def test_band_rule_accepts_the_oracle_itself():
    for K, P in ((5, 100), (1, 7), (3, 2), (3, 3), (25, 128)):
        x = co.gauss(3, 200, K)
        feat, _, _ = co.features64(x, P)
        bad, worst = co.band_check(x, feat, P)
        assert len(bad) == 0 and worst == 0.0, (K, P, bad, worst)
        # ... and the oracle's value rounded to fp32, and moved by 0.9 of the feature bound
        bad, worst = co.band_check(x, feat.astype(np.float32), P)
        assert len(bad) == 0 and worst < 0.1, (K, P, worst)
        bad, worst = co.band_check(x, feat + 0.9 * co.feature_bound(x)[:, None] * np.array([1.0, -1.0]), P)
        assert len(bad) == 0 and worst <= 0.9 + 1e-9, (K, P, worst)
    # the seeded families are mostly unambiguous
    for K, P, least in ((5, 100, 0.85), (25, 128, 0.85)):
        x, keep = _family(K, P)
        print(f"K = {K}, P = {P}: {keep.mean():.3f} unambiguous")
        assert keep.mean() >= least


def test_band_rule_rejects_a_sign_flip_swapped_components_and_a_neighbouring_pair():
    P = 100
    x, keep = _family(5, P)
    assert keep.mean() >= 0.70
    x = x[keep]
    feat, pair, _ = co.features64(x, P)
    B = co.feature_bound(x)
    rows = np.arange(len(x))
    # a band of one pair: the rule is |device - that pair's features| <= bound per component
    bad, _ = co.band_check(x, -feat, P)
    assert np.array_equal(bad, rows[(2 * np.abs(feat)).max(1) > B])
    assert len(bad) == len(x)
    bad, _ = co.band_check(x, feat[:, ::-1], P)
    assert np.array_equal(bad, rows[np.abs(feat[:, 0] - feat[:, 1]) > B])
    assert len(bad) >= 0.99 * len(x)
    # the pair next to the chosen one, (i, j + 1) or (i, j - 1): outside the band by the definition of unambiguous
    p = co.points64(x, P)
    j2 = np.where(pair[:, 1] + 1 < P, pair[:, 1] + 1, pair[:, 1] - 1)
    assert (j2 != pair[:, 0]).all()
    near = (p[rows, j2] - p[rows, pair[:, 0]])[:, ::-1]
    bad, _ = co.band_check(x, near, P)
    assert np.array_equal(bad, rows[np.abs(near - feat).max(1) > B])
    assert len(bad) >= 0.99 * len(x)
    # a value that is not finite fails; an all-zero row must give exactly zero
    y = feat.copy()
    y[5, 1] = np.nan
    assert np.array_equal(co.band_check(x, y, P)[0], [5])
    z = np.zeros((2, 20), np.float32)
    assert len(co.band_check(z, np.zeros((2, 2)), P)[0]) == 0
    assert np.array_equal(co.band_check(z, np.array([[0.0, 0.0], [0.0, 1e-30]]), P)[0], [1])


def test_ellipses_have_the_tied_diameters_the_tie_test_needs():
    for a, b in ((2, 1), (1, 2), (3, 0.5)):
        x = co.ellipse(a, b)
        p = co.points64(x, 101)[0]
        assert np.allclose(p[0], [a, 0]) and np.allclose(p[25], [0, b]) and np.allclose(p[50], [-a, 0]) and np.allclose(p[75], [0, -b])
        assert np.array_equal(p[100], p[0])                               # the angle is reduced exactly
        _, pair, _ = co.features64(x, 101)
        if a > b:
            assert tuple(pair[0]) == (0, 50) and co.band_counts(x, 101)[0] == 2          # (0, 50) ties with (50, 100)
        else:
            assert tuple(pair[0]) == (25, 75) and co.band_counts(x, 101)[0] == 1
