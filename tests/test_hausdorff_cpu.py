"""CPU-side checks of the curve-to-template distances (hint_amd.curves trace_fourier_curves / hausdorff_distances /
chamfer_distances / lens_fit_loss, the hint_hausdorff_* entry points; no GPU): header, exports and binding agree, every argument
check of hint_hausdorff_run comes before any device call and names its field, hint_hausdorff_workspace_bytes and
hint_hausdorff_geometry agree with it, the Python functions refuse bad arguments by name, the test-side float64 evaluation
(tests/hausdorff_oracle.py) reproduces what was recorded from the reference's functions, and its comparison rule accepts a
float32 emulation of the contract and rejects seven wrong ones."""
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
import hausdorff_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_hausdorff_workspace_bytes", "hint_hausdorff_run", "hint_hausdorff_geometry")
PUBLIC = ("trace_fourier_curves", "hausdorff_distances", "chamfer_distances", "lens_fit_loss")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
POINTERS = ("x", "b_points", "a_points", "a_offsets", "a_params", "max_h", "avg_h", "chamfer", "points")


def good_desc(source="x", ragged=False, n_rows=1000, K=5, P=1000, T=130):
    desc = _lib.HausdorffDesc()
    for i, f in enumerate(POINTERS):
        setattr(desc, f, BASE + (i << 28))
    if source == "x":
        desc.b_points = None
    else:
        desc.x, desc.points = None, None
    if not ragged:
        desc.a_offsets = None
    desc.n_rows, desc.n_coeffs, desc.n_points, desc.n_template, desc.max_groups = n_rows, K, P, T, 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_hausdorff_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def rejected(what, source="x", ragged=False, **fields):
    desc = good_desc(source, ragged)
    for k, v in fields.items():
        setattr(desc, k, v)
    st, msg = run_msg(desc)
    assert st != 0 and what in msg, (fields, msg)
    return msg


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
    for cite in ("run_experiments.py:147-159", "eval_shapes.py:82-95", "data.py:51-57", "best_shape_fit.py:143-149",
                 "best_shape_fit.py:195-199", ":275-277", ":153-156", "best_shape_fit.py:203-209"):
        assert cite in header, cite
    D = _lib.HausdorffDesc
    struct = re.search(r"typedef struct hint_hausdorff_desc \{(.*?)\} hint_hausdorff_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f[0] for f in D._fields_]                          # the same fields in the same order
    # 2 pointers, int64, 2 int32, 3 pointers, int64, 4 pointers, int32 (+ 4 bytes of padding)
    assert C.sizeof(D) == 16 + 8 + 8 + 24 + 8 + 32 + 8 == 104
    assert (D.n_rows.offset, D.n_points.offset, D.a_points.offset, D.n_template.offset, D.max_h.offset, D.max_groups.offset) == \
        (16, 28, 32, 56, 64, 96)
    for fn in PUBLIC:
        assert getattr(hint_amd, fn) is getattr(curves, fn) and fn in curves.__all__
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)
    # the curve descriptor is as it was
    assert C.sizeof(_lib.CurveDesc) == 96


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for source in ("x", "b_points"):
        for ragged in (False, True):
            rejected("a_points is null", source, ragged, a_points=None)
    rejected("both x and b_points", b_points=BASE + (1 << 28), points=None)
    rejected("x and b_points are both null", x=None)
    rejected("points is an output of the traced source only", "b_points", points=BASE + (8 << 28))
    rejected("no output requested", max_h=None, avg_h=None, chamfer=None, points=None)
    rejected("no output requested", "b_points", max_h=None, avg_h=None, chamfer=None)
    for bad in (0, -3, (1 << 30) + 1):
        assert f"got {bad}" in rejected("n_rows must be 1..1073741824", n_rows=bad)
    for bad in (0, -1, 2, 4, 24, 26, 27):
        assert f"got {bad}" in rejected("n_coeffs must be odd and 1..25", n_coeffs=bad)
    for bad in (-1, 0, 1, 1025):
        for source in ("x", "b_points"):
            assert f"got {bad}" in rejected("n_points must be 2..1024", source, n_points=bad)
    for bad in (0, -5):
        for ragged in (False, True):
            assert f"got {bad}" in rejected("n_template must be >= 1", ragged=ragged, n_template=bad)
    assert "got 4097" in rejected("template must hold 1..4096 points", n_template=4097)
    rejected("more than n_rows x 4096 points", ragged=True, n_rows=3, n_template=3 * 4096 + 1)
    rejected("max_groups must be >= 0", max_groups=-1)
    for field in POINTERS:
        source, ragged = ("b_points" if field == "b_points" else "x"), field == "a_offsets"
        want = "a_offsets must be 8-byte aligned" if ragged else f"{field} must be 4-byte aligned"
        for off in ((2, 4) if ragged else (2,)):
            rejected(want, source, ragged, **{field: BASE + (9 << 28) + off})


def test_workspace_bytes_agrees_with_run_and_does_not_grow_with_n():
    lib = _lib.load()
    for args, what in (((0, 5, 1000, 130), "n_rows"), (((1 << 30) + 1, 5, 1000, 130), "n_rows"), ((10, -1, 1000, 130), "n_coeffs"),
                       ((10, 4, 1000, 130), "n_coeffs"), ((10, 27, 1000, 130), "n_coeffs"), ((10, 5, 1, 130), "n_points"),
                       ((10, 5, 1025, 130), "n_points"), ((10, 0, 1025, 130), "n_points"), ((10, 5, 1000, 0), "template"),
                       ((10, 5, 1000, 4097), "template")):
        lib.hint_hausdorff_workspace_bytes(10, 5, 100, 10)                # a good call in between leaves the message empty
        assert lib.hint_last_error().decode() == ""
        assert lib.hint_hausdorff_workspace_bytes(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    # what run takes, workspace_bytes takes: no workspace at any size (the descriptor names none)
    for args in ((1, 1, 2, 1), (1000, 5, 1000, 1000), (1 << 16, 5, 1000, 1000), (1 << 30, 25, 1024, 4096), (10, 0, 1000, 130)):
        assert lib.hint_hausdorff_workspace_bytes(*args) == 0
        assert lib.hint_last_error().decode() == "", args
    assert "workspace" not in [f[0] for f in _lib.HausdorffDesc._fields_]


def test_geometry_is_consistent():
    lib = _lib.load()
    geo = lib.hint_hausdorff_geometry
    assert geo(0, 1000, 130, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert geo(10, 1025, 130, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert geo(10, 1000, 4097, 0) == -1 and "template" in lib.hint_last_error().decode()
    assert geo(10, 1000, 0, 0) == -1 and "template" in lib.hint_last_error().decode()
    assert geo(10, 1000, 130, 5) == -1 and "field" in lib.hint_last_error().decode()
    assert geo(10, 1000, 130, -1) == -1
    tile, cap = geo(1, 2, 1, 2), geo(1, 2, 1, 3)
    assert 256 <= tile <= 4096 and tile % 256 == 0 and cap >= 256
    for N in (1, 2, 3, cap - 1, cap, cap + 1, 1 << 16, 1 << 30):
        for P, M in ((1000, 1000), (2, 1), (1024, 4096), (100, tile), (100, tile + 1)):
            g, rows, tl, c, tiles = (geo(N, P, M, f) for f in range(5))
            assert (rows, tl, c) == (1, tile, cap)
            assert g == min(N, cap)                                       # workgroup w takes rows w, w + g, ...: every row is taken
            assert tiles == -(-M // tile) and (tiles - 1) * tile < M <= tiles * tile


def test_python_argument_errors():
    x, tpl, pr = torch.randn(50, 20), torch.randn(130, 2), torch.randn(50, 4)
    with pytest.raises(HintAmdError, match="trace_fourier_curves: x is on cpu.*no CPU fallback"):
        hint_amd.trace_fourier_curves(x)
    with pytest.raises(HintAmdError, match="trace_fourier_curves: x must be a tensor"):
        hint_amd.trace_fourier_curves(x.numpy())
    with pytest.raises(HintAmdError, match="trace_fourier_curves: x must be 2-D"):
        hint_amd.trace_fourier_curves(x[0])
    with pytest.raises(HintAmdError, match="trace_fourier_curves: x requires grad"):
        hint_amd.trace_fourier_curves(x.clone().requires_grad_())
    for fn, args in ((hint_amd.hausdorff_distances, (x, tpl, pr)), (hint_amd.chamfer_distances, (x, tpl, pr)),
                     (hint_amd.lens_fit_loss, (x, tpl, pr))):
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu.*no CPU fallback"):
            fn(*args)
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu"):
            fn(torch.randn(50, 100, 2), tpl, pr)
        with pytest.raises(HintAmdError, match=name + ": curve must be a tensor"):
            fn(x.numpy(), tpl, pr)
        for bad in (x[0], torch.randn(2, 3, 2, 2)):
            with pytest.raises(HintAmdError, match=name + r": curve must be \[rows, 4 K\] coefficients or \[rows, P, 2\] points"):
                fn(bad, tpl, pr)
    with pytest.raises(HintAmdError, match="lens_fit_loss: lens_fit_weight must be a number"):
        hint_amd.lens_fit_loss(x, tpl, pr, "1")
    with pytest.raises(HintAmdError, match="lens_fit_loss: lens_fit_weight must be a number"):
        hint_amd.lens_fit_loss(x, tpl, pr, float("nan"))
    with pytest.raises(HintAmdError, match="lens_fit_loss: params must be a tensor"):
        hint_amd.lens_fit_loss(x, tpl, None)
    # the remaining checks sit behind the device check: they are reached through the helpers the public functions call
    who = "hausdorff_distances"
    for name, bad, what in (("template", tpl.numpy(), "template must be a tensor"), ("template", tpl, "template is on cpu"),
                            ("params", torch.zeros(3, dtype=torch.int64), "params is on cpu")):
        with pytest.raises(HintAmdError, match=who + ": " + what):
            curves._check_dev_tensor(bad, name, who)
    for shape in ((0, 20), (5, 0), (5, 19), (5, 8), (5, 16), (5, 104)):
        with pytest.raises(HintAmdError, match=who + ": x must hold"):
            curves._check_curve_shape(shape, 1000, who)
    for bad, what in ((1, "n_points must be 2..1024"), (1025, "n_points must be 2..1024"), (1000.0, "n_points must be an int"),
                      (True, "n_points must be an int")):
        with pytest.raises(HintAmdError, match=who + ": " + what):
            curves._check_curve_shape((5, 20), bad, who)
        with pytest.raises(HintAmdError, match="trace_fourier_curves: " + what):
            curves._check_dense_points(bad, "trace_fourier_curves")
    assert curves._check_curve_shape((5, 20), 1000, who) == (5, 5, 1000)
    assert curves._check_curve_shape((5, 100), 2, who) == (5, 25, 2)
    assert curves._check_curve_shape((5, 1024, 2), None, who) == (5, 0, 1024)        # points: n_points is not looked at
    assert curves._check_curve_shape((5, 2, 2), 7, who) == (5, 0, 2)
    for shape, what in (((5, 1, 2), "2..1024 points a row"), ((5, 1025, 2), "2..1024 points a row"), ((0, 100, 2), "rows"),
                        ((5, 100, 3), r"\[rows, P, 2\] points")):
        with pytest.raises(HintAmdError, match=who + ": curve must .*" + what):
            curves._check_curve_shape(shape, 1000, who)
    for shape, ragged, what in (((130,), False, r"template must be \[points, 2\]"), ((130, 3), False, r"template must be \[points, 2\]"),
                                ((0, 2), False, "template is empty"), ((0, 2), True, "template is empty"),
                                ((4097, 2), False, "a shared template must hold 1..4096 points")):
        with pytest.raises(HintAmdError, match=who + ": " + what):
            curves._check_template_shape(shape, ragged, who)
    assert curves._check_template_shape((4096, 2), False, who) == 4096 and curves._check_template_shape((9000, 2), True, who) == 9000
    good = [0, 1, 3, 4099, 4100]
    got = curves._check_offsets(good, 4, 4100, who)
    assert got.dtype == torch.int64 and got.tolist() == good
    assert curves._check_offsets(np.array(good, np.int32), 4, 4100, who).tolist() == good
    for bad, T, what in (([1, 2, 3, 4, 4100], 4100, "ascend from 0"), ([0, 1, 3, 4099, 4100], 4101, "ascend from 0"),
                         ([0, 1, 1, 4097, 4100], 4100, r"ascend by 1..4096 points a row \(row 1: 0\)"),
                         ([0, 3, 2, 5, 4100], 4100, r"ascend by 1..4096 points a row \(row 1: -1\)"),
                         ([0, 1, 2, 3, 4100], 4100, r"ascend by 1..4096 points a row \(row 3: 4097\)"),
                         ([0, 1, 2, 4100], 4100, r"offsets must have shape \[5\]"),
                         ([[0, 1, 2, 3, 4100]], 4100, r"offsets must have shape \[5\]"),
                         ([0.0, 1.0, 2.0, 3.0, 4100.0], 4100, "expected an integer tensor"),
                         ("abc", 4100, "offsets must be a tensor or an array-like")):
        with pytest.raises(HintAmdError, match=who + ": .*" + what):
            curves._check_offsets(bad, 4, T, who)
    for shape in ((3,), (50, 3), (49, 4), (1, 1, 4)):
        with pytest.raises(HintAmdError, match=who + r": params must have shape \[4\], \[1, 4\] or \[50, 4\]"):
            curves._check_params_shape(shape, 50, who)
    for shape in ((4,), (1, 4), (50, 4)):
        curves._check_params_shape(shape, 50, who)


@pytest.mark.parametrize("case", ho.GOLDEN_CASES, ids=lambda c: c["name"])
def test_float64_oracle_reproduces_the_reference_outputs(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"hausdorff_{case['name']}.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"hausdorff_{case['name']}.npz")) < 100_000
    n = case["rows"]
    x, tpl, pr = g["x"], g["template"], g["params"]
    assert x.dtype == tpl.dtype == pr.dtype == np.float32
    assert np.array_equal(x, co.gauss(case["seed"], n, 5))               # the fixture's inputs are the seeded ones
    assert np.array_equal(tpl, ho.lens_template(case["points"])) and np.array_equal(pr, ho.golden_params(case["seed"], n))
    ref = ho.distances64(x, tpl, pr, P=ho.GOLDEN_P)
    assert np.abs(ref["max_h"] - g["ref_max_h"]).max() <= 1e-12
    assert np.abs(ref["avg_h"] - g["ref_avg_h"]).max() <= 1e-12
    fit = ho.distances64(x, tpl, pr, P=ho.GOLDEN_FIT_P)
    for w, weight in enumerate(ho.GOLDEN_WEIGHTS):
        assert np.abs(fit["chamfer"][:, 0] + weight * fit["chamfer"][:, 1] - g["ref_loss"][:, w]).max() <= 1e-12
    p = co.points64(x, ho.GOLDEN_P)
    assert np.abs(p[0] - g["ref_points_first"]).max() <= 3e-14 and np.abs(p[-1] - g["ref_points_last"]).max() <= 3e-14
    assert (pr[:, 3] != 0).all() and (ref["max_h"] > 0.01).all()


# (K, P, M) of the issue's float32 emulation, and one ragged case that mixes lengths
EMULATED = ((5, 1000, 257), (25, 1000, 1000), (5, 100, 130), (1, 2, 1), (3, 33, 7))


def _case(K, P, M, N=6, seed=5):
    x = co.gauss(seed + K + P, N, K)
    return x, ho.lens_template(M), ho.golden_params(seed + M, N)


@pytest.mark.parametrize("K,P,M", EMULATED)
def test_rule_accepts_a_float32_emulation_of_the_contract(K, P, M):
    x, tpl, pr = _case(K, P, M)
    for params in (pr, None):
        ref = ho.distances64(x, tpl, params, P=P)
        mh, av, ch = ho.emulate32(x, tpl, params, P=P)
        r_h, r_c = ho.ratios(ref, mh, av), ho.ratios(ref, chamfer=ch)
        print(f"K {K} P {P} M {M} params {params is not None}: max_h / avg_h error / bound {r_h.max():.3g}, chamfer {r_c.max():.3g}")
        assert len(ho.check(ref, mh, av, ch)[0]) == 0
        # the bounds leave room: a correct implementation uses a fraction of them (chamfer: confirmed here, by this emulation)
        assert r_h.max() <= 0.5 and r_c.max() <= 0.5
        # the given-points source: the emulation's own trace as b_points, no trace error allowed for
        b = ho.trace32(x, P).astype(np.float32)
        ref_b = ho.distances64(b, tpl, params)
        assert len(ho.check(ref_b, *ho.emulate32(b, tpl, params))[0]) == 0
    # traced points within delta_B
    dB = (2 * K + 2) * ho.U * co.scale(x)
    assert (np.abs(ho.trace32(x, P) - co.points64(x, P)).max((1, 2)) <= dB).all()


def test_rule_accepts_the_emulation_on_ragged_templates():
    K, P, N = 5, 100, 5
    x = co.gauss(11, N, K)
    lens = [1, 2, 130, 1025, 33]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    tpl = np.concatenate([ho.lens_template(m) * (1 + 0.1 * i) for i, m in enumerate(lens)])
    pr = ho.golden_params(12, N)
    ref = ho.distances64(x, tpl, pr, offsets, P=P)
    assert len(ho.check(ref, *ho.emulate32(x, tpl, pr, offsets, P=P))[0]) == 0
    # ... and each row is what the row alone gives
    for n in range(N):
        one = ho.distances64(x[n:n + 1], tpl[offsets[n]:offsets[n + 1]], pr[n:n + 1], P=P)
        assert one["max_h"][0] == ref["max_h"][n] and one["avg_h"][0] == ref["avg_h"][n]


@pytest.mark.parametrize("wrong", ho.WRONG)
def test_rule_rejects_wrong_implementations(wrong):
    """on a non-circular template with every angle away from 0, each wrong variant misses the oracle by more than 10 x the bound
    in every row - so the rule has something to reject - and the rule rejects it"""
    K, P, N = 5, 100, 8
    x = co.gauss(21, N, K)
    pr = ho.golden_params(22, N)
    pr[:, 3] = np.where(np.abs(pr[:, 3]) < 0.3, 0.3 + np.abs(pr[:, 3]), pr[:, 3])       # angle != 0
    pr[:, 2] = np.where(np.abs(pr[:, 2] - 1) < 0.2, 1.3, pr[:, 2])                       # scale != 1
    lens = [130, 65, 131, 7, 130, 64, 257, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    tpl = np.concatenate([ho.lens_template(m) * (1 + 0.1 * i) for i, m in enumerate(lens)])
    assert (np.abs(pr[:, 3]) >= 0.3).all() and (np.abs(pr[:, :2]).max(1) > 0.01).all()
    ref = ho.distances64(x, tpl, pr, offsets, P=P)
    right = ho.emulate32(x, tpl, pr, offsets, P=P)
    assert len(ho.check(ref, *right)[0]) == 0
    mh, av, ch = ho.emulate32(x, tpl, pr, offsets, P=P, wrong=wrong)
    r = ho.ratios(ref, mh, av, ch)
    rows = np.arange(N - 1) if wrong == "neighbour's first point" else np.arange(N)      # (the last row has no neighbour)
    print(f"{wrong}: error / bound per row {np.array2string(r, precision=3)}")
    assert (r[rows] > 10.0).all(), (wrong, r)
    bad, _ = ho.check(ref, mh, av, ch)
    assert set(rows) <= set(bad.tolist())
    # a value that is not finite fails; identical point sets must give exactly zero
    mh2 = right[0].copy()
    mh2[3] = np.nan
    assert 3 in ho.check(ref, mh2, right[1], right[2])[0]
    b = ho.lens_template(64)[None].repeat(2, 0)
    same = ho.distances64(b, ho.lens_template(64))
    assert (same["max_h"] == 0).all() and (same["E"] > 0).all() and (same["e_ch"] > 0).all()
    assert len(ho.check(same, np.zeros(2), np.zeros(2), np.zeros((2, 2)))[0]) == 0
