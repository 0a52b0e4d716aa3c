"""CPU tests of the polygon overlap (hint_overlap_run, hint_amd.curves polygon_overlap / lens_iou_dice / plus_iou_dice): the symbols
and the descriptor, the host argument checks, and the float64 oracle itself - its two methods against each other and against
closed forms, the tolerance constant's rule, the wrong variants, the crossing counts."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves
from hint_amd._lib import HintAmdError
import hausdorff_oracle as ho
import overlap_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_overlap_workspace_bytes", "hint_overlap_run", "hint_overlap_geometry")
PUBLIC = ("polygon_overlap", "lens_iou_dice", "plus_iou_dice", "lens_shape_scores", "plus_shape_scores")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
POINTERS = ("x", "b_points", "a_points", "a_offsets", "a_params", "plus_params", "areas", "iou", "dice", "crossings")
OUTPUTS = POINTERS[6:]
# methods A and B in float64: the largest difference seen on the ledger is 7.1e-15 (areas of order 1 to 20, coordinates below 8);
# 1e-13 is ~14 x that.  Coordinates of magnitude R > 1 carry R times the rounding into every operation on them, so the bound is
# 1e-13 max(1, R) (the case far from the origin, R = 1000: 2.4e-14 seen)
AB_TOL = 1e-13
CASES = [c[0] for c in oo.LEDGER]


def good_desc(source="x", template="points", n_rows=1000, K=5, P=100, M=130):
    desc = _lib.OverlapDesc()
    for i, f in enumerate(POINTERS):
        setattr(desc, f, BASE + (i << 28))
    if source == "x":
        desc.b_points = None
    else:
        desc.x = None
    if template == "points":
        desc.plus_params = None
    else:
        desc.a_points = desc.a_offsets = desc.a_params = None
    desc.a_offsets = None
    desc.n_rows, desc.n_coeffs, desc.n_points, desc.n_template, desc.max_groups = n_rows, K, P, M, 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_overlap_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def rejected(what, source="x", template="points", **fields):
    desc = good_desc(source, template)
    for k, v in fields.items():
        setattr(desc, k, v)
    st, msg = run_msg(desc)
    assert st != 0 and what in msg, (fields, msg)
    return msg


# ---- the C ABI ----
def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert set(_lib.exported_symbols()) == declared
    assert "#define HINT_AMD_ABI_VERSION 8" in header and lib.hint_abi_version() == _lib.ABI_VERSION == 8
    for cite in ("best_shape_fit.py:265-271", "best_shape_fit.py:133-139", "run_experiments.py:144-167", "eval_shapes.py:82-103"):
        assert cite in header, cite
    D = _lib.OverlapDesc
    struct = re.search(r"typedef struct hint_overlap_desc \{(.*?)\} hint_overlap_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f[0] for f in D._fields_]                          # the same fields in the same order
    # 2 pointers, int64, 2 int32, 3 pointers, int64, 5 pointers, int32 (+ padding)
    assert C.sizeof(D) == 16 + 8 + 8 + 24 + 8 + 40 + 8 == 112
    assert [getattr(D, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104]
    for fn in PUBLIC:
        assert getattr(hint_amd, fn) is getattr(curves, fn) and fn in curves.__all__
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)
    # the descriptors before this one are as they were
    assert C.sizeof(_lib.HausdorffDesc) == 104 and C.sizeof(_lib.PlusDesc) == 96


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for source in ("x", "b_points"):
        for template in ("points", "plus"):
            rejected("no output requested", source, template, **{f: None for f in OUTPUTS})
    rejected("both a_points and plus_params", plus_params=BASE + (5 << 28))
    for need in ("areas", "iou", "dice"):                                # each output that reads the template asks for one
        others = {f: None for f in ("areas", "iou", "dice") if f != need}
        rejected("a_points and plus_params are both null", a_points=None, a_params=None, **others)
    rejected("a_offsets is given without a_points", template="plus", a_offsets=BASE + (3 << 28))
    rejected("a_params is given without a_points", template="plus", a_params=BASE + (4 << 28))
    rejected("both x and b_points", b_points=BASE + (1 << 28))
    rejected("x and b_points are both null", x=None)
    rejected("x and b_points are both null", x=None, areas=None, iou=None, dice=None)           # crossings needs the curve too
    for bad in (0, -3, (1 << 30) + 1):
        assert f"got {bad}" in rejected("n_rows must be 1..1073741824", n_rows=bad)
    for bad in (0, -1, 2, 4, 24, 26, 27):
        assert f"got {bad}" in rejected("n_coeffs must be odd and 1..25", n_coeffs=bad)
    assert "got 1" in rejected("n_points must be", "b_points", n_coeffs=4, n_points=1)          # (n_coeffs: ignored with b_points)
    for bad in (-1, 0, 1, 1025):
        for source in ("x", "b_points"):
            assert f"got {bad}" in rejected("n_points must be", source, n_points=bad)
    for source in ("x", "b_points"):
        assert "got 2" in rejected("n_points must be 3..1024", source, n_points=2)
    for bad in (-1, 0, 2):
        assert f"got {bad}" in rejected("n_template must be >= 3", n_template=bad)
    assert "got 4097" in rejected("a row's template must hold 3..4096 points", n_template=4097)
    rejected("is more than n_rows x 4096 points", a_offsets=BASE + (3 << 28), n_rows=2, n_template=2 * 4096 + 1)
    rejected("max_groups must be >= 0", max_groups=-1)
    for field in POINTERS:
        source = "b_points" if field == "b_points" else "x"
        template = "plus" if field == "plus_params" else "points"
        if field == "a_offsets":
            rejected("a_offsets must be 8-byte aligned", a_offsets=BASE + (3 << 28) + 4)
        rejected(f"{field} must be ", source, template, **{field: BASE + (9 << 28) + 2})
    # crossings alone reads no template: neither source is needed, and n_template is then not looked at
    desc = good_desc()
    desc.a_points, desc.a_params, desc.areas, desc.iou, desc.dice, desc.n_template = None, None, None, None, None, 0
    desc.n_rows = 0                                                      # (rejected all the same, so nothing is launched here)
    st, msg = run_msg(desc)
    assert st != 0 and "n_rows" in msg and "template" not in msg and "null" not in msg


def test_workspace_bytes_agrees_with_run_and_needs_none():
    lib = _lib.load()
    ws = lib.hint_overlap_workspace_bytes
    for args, what in (((0, 5, 100, 130), "n_rows"), (((1 << 30) + 1, 5, 100, 130), "n_rows"), ((10, -1, 100, 130), "n_coeffs"),
                       ((10, 4, 100, 130), "n_coeffs"), ((10, 27, 100, 130), "n_coeffs"), ((10, 5, 2, 130), "n_points"),
                       ((10, 5, 1025, 130), "n_points"), ((10, 0, 2, 130), "n_points"), ((10, 5, 100, 2), "template"),
                       ((10, 5, 100, 4097), "template")):
        ws(10, 5, 100, 130)                                              # a good call in between leaves the message empty
        assert lib.hint_last_error().decode() == ""
        assert ws(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    for args in ((1, 1, 3, 3), (1000, 25, 1000, 12), (1 << 16, 5, 100, 130), (1 << 30, 25, 1024, 4096), (10, 0, 100, 130)):
        assert ws(*args) == 0
        assert lib.hint_last_error().decode() == "", args
    assert "workspace" not in [f[0] for f in _lib.OverlapDesc._fields_]


def test_geometry_is_consistent():
    lib = _lib.load()
    geo = lib.hint_overlap_geometry
    assert geo(0, 100, 130, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert geo(10, 1025, 130, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert geo(10, 2, 130, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert geo(10, 100, 2, 0) == -1 and "template" in lib.hint_last_error().decode()
    assert geo(10, 100, 4097, 0) == -1 and "template" in lib.hint_last_error().decode()
    assert geo(10, 100, 130, 5) == -1 and "field" in lib.hint_last_error().decode()
    assert geo(10, 100, 130, -1) == -1
    tile, cap = geo(1, 3, 3, 2), geo(1, 3, 3, 3)
    assert tile == oo.TILE and cap >= 256 and cap % 256 == 0
    for N in (1, 2, 3, cap - 1, cap, cap + 1, 1 << 16, 1 << 30):
        for P in (3, 100, 1024):
            for M in (3, 12, 130, 1024, 1025, 4096):
                g, rows, tl, c, tiles = (geo(N, P, M, f) for f in range(5))
                assert (rows, tl, c) == (1, tile, cap) and tiles == -(-M // tile)
                assert g == min(N, cap)                                   # workgroup w takes rows w, w + g, ...: every row is taken


def test_python_argument_errors():
    x, pts, proto, pr4, pr9 = torch.randn(50, 20), torch.randn(50, 100, 2), torch.randn(130, 2), torch.randn(50, 4), torch.randn(50, 9)
    calls = ((hint_amd.polygon_overlap, (proto,)), (hint_amd.lens_iou_dice, (proto, pr4)), (hint_amd.plus_iou_dice, (pr9,)))
    for fn, rest in calls:
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu.*no CPU fallback"):
            fn(x, *rest)
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu"):
            fn(pts, *rest)
        with pytest.raises(HintAmdError, match=name + ": curve must be a tensor"):
            fn(x.numpy(), *rest)
        for bad in (x[0], torch.randn(2, 3, 2, 2)):
            with pytest.raises(HintAmdError, match=name + r": curve must be \[rows, 4 K\] coefficients or \[rows, P, 2\] points"):
                fn(bad, *rest)
        with pytest.raises(HintAmdError, match=name + ": curve requires grad"):       # (behind the device check: the helper)
            curves._check_no_grad(x.clone().requires_grad_(True), "curve", name)
    with pytest.raises(HintAmdError, match="lens_iou_dice: params must be a tensor"):
        hint_amd.lens_iou_dice(x, proto, None)
    for fn, rest in ((hint_amd.lens_shape_scores, (proto,)), (hint_amd.plus_shape_scores, ())):
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": x is on cpu.*no CPU fallback"):
            fn(x, *rest)
        with pytest.raises(HintAmdError, match=name + ": x must be a tensor"):
            fn(x.numpy(), *rest)
        with pytest.raises(HintAmdError, match=name + ": x requires grad"):
            fn(x.clone().requires_grad_(True), *rest)
        with pytest.raises(HintAmdError, match=name + ": x must be 2-D"):
            fn(pts, *rest)
    # the remaining checks sit behind the device check: they are reached through the helpers the public functions call
    who = "polygon_overlap"
    assert curves.MIN_POLYGON_POINTS == oo.MIN_POINTS == 3
    assert curves._check_curve_shape((7, 2, 2), 100, who) == (7, 0, 2)   # two points pass the shared check; _polygon_curve refuses
    assert curves._check_template_shape((3, 2), False, who) == 3
    with pytest.raises(HintAmdError, match=who + ": a shared template must hold"):
        curves._check_template_shape((4097, 2), False, who)
    assert curves._check_template_shape((5000, 2), True, who) == 5000


# ---- the oracle ----
@functools.lru_cache(maxsize=None)
def case_rows(name):
    """per row of a ledger case: (overlap64 of the kernel's fp32 vertices, emulate32, crossings64)"""
    case = oo.ledger_case(name)
    rows = []
    for n in range(len(case["curve"])):
        Cn = case["points32"][n]
        rows.append((oo.overlap64(Cn, oo.row_template32(case, n)), oo.row_emulate32(case, n), oo.crossings64(Cn)))
    return case, rows


def template64(case, n):
    """row n's template placed in float64 (the plus from its parameters, so that its arms are exact rectangles)"""
    if case["plus_params"] is not None:
        return oo.plus_vertices64(case["plus_params"][n:n + 1])[0]
    a = ho.row_template(case["a_points"], case["offsets"], n)
    return ho.template64(a, None if case["params"] is None else case["params"][n])


@pytest.mark.parametrize("name", CASES)
def test_the_two_methods_agree_on_every_ledger_case(name):
    case = oo.ledger_case(name)
    worst = 0.0
    for n in range(len(case["curve"])):
        Cn, T = case["points32"][n], template64(case, n)
        a = oo.overlap64(Cn, T)
        at, ac, inter = oo.plus_overlap_b(Cn, T) if case["plus_params"] is not None else oo.convex_overlap_b(Cn, T)
        worst = max(worst, abs(a["I_raw"] - inter), abs(a["area_T"] - at), abs(a["area_C"] - ac))
        assert a["area_T"] > 0.01 and a["area_C"] > 0.01
    big = max(1.0, float(np.abs(case["points32"]).max()))
    print(f"{name}: methods A and B differ by at most {worst:.2e} (coordinates up to {big:.0f})")
    assert worst <= AB_TOL * big, worst


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def test_closed_forms():
    # two axis-aligned rectangles: 3 x 2 and 2 x 3 sharing 1.5 x 1; vertical edges on both
    a, b = rect(0.0, 0.0, 3.0, 2.0), rect(1.5, 1.0, 3.5, 4.0)
    for Cv, Tv in ((a, b), (b, a), (a[::-1], b), (a, b[::-1]), (a[::-1], b[::-1]), (np.roll(a, 2, 0), b)):
        r = oo.overlap64(Cv, Tv)
        assert abs(r["I"] - 1.5) < 1e-15 and {round(r["area_C"], 12), round(r["area_T"], 12)} == {6.0}
        assert abs(r["iou"] - 1.5 / 10.5) < 1e-15 and abs(r["dice"] - 3.0 / 12.0) < 1e-15
        e = oo.emulate32(Cv, Tv)
        assert (e["area_T"], e["area_C"], e["I"]) == (6.0, 6.0, 1.5) and e["crossings"] == 0     # exact in fp32 too
        assert abs(oo.convex_overlap_b(Cv, Tv)[2] - 1.5) < 1e-15
    # a polygon with itself, either orientation, a shared vertex list: IoU = DICE = 1
    w = oo.wobble_curves(5, 1, 37)[0].astype(np.float64)
    for Tv in (w, w[::-1], np.roll(w, 5, 0)):
        r = oo.overlap64(w, Tv)
        assert abs(r["iou"] - 1) < 1e-14 and abs(r["dice"] - 1) < 1e-14 and abs(r["I"] - r["area_C"]) < 1e-14
        e = oo.emulate32(w, Tv)
        assert oo.ratio(r, {k: e[k] for k in ("area_T", "area_C", "I", "iou", "dice")}) <= 0.25
    # disjoint polygons - apart in x, apart in y, touching along an edge: exactly 0
    for Tv in (rect(4.0, 0.0, 5.0, 1.0), rect(0.0, 3.0, 3.0, 5.0), rect(3.0, 0.0, 4.0, 2.0), rect(0.0, 2.0, 3.0, 2.5)):
        r, e = oo.overlap64(a, Tv), oo.emulate32(a, Tv)
        assert r["I"] == 0.0 and r["iou"] == 0.0 and r["dice"] == 0.0 and e["I"] == 0.0 and e["iou"] == 0.0
    # a figure-eight: one proper crossing; its two lobes wind in opposite senses, so a rectangle over both halves sees them cancel
    eight = np.array([[0.0, 0.0], [2.0, 2.0], [2.0, 0.0], [0.0, 2.0]])
    assert oo.crossings64(eight) == (1, True) and oo.crossings32(eight) == 1
    assert oo.overlap64(eight, rect(-1.0, -1.0, 3.0, 3.0))["I_raw"] < 1e-15
    left = oo.overlap64(eight, rect(-1.0, -1.0, 1.0, 3.0))                # the left lobe alone: a triangle of area 1
    assert abs(left["I_raw"] - 1.0) < 1e-15 and left["area_C"] == 0.0 and left["I"] == 0.0      # (cut to the curve's own area)
    assert oo.crossings64(a) == (0, True) and oo.crossings64(w) == (0, True)
    # P = 3 against M = 3: two triangles, against the clipped polygon
    t0, t1 = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]]), np.array([[1.0, 1.0], [5.0, 1.0], [1.0, 5.0]])
    assert abs(oo.overlap64(t0, t1)["I"] - 2.0) < 1e-15 and abs(oo.convex_overlap_b(t0, t1)[2] - 2.0) < 1e-15
    assert oo.crossings64(t0) == (0, True)
    # a plus with xwidth = 0 (its x arm has no area; vertices repeat), angle exactly 0 and 1e-4 (vertical and almost vertical
    # edges): the area is the y arm's, and the overlap with a covering rectangle is the plus itself
    for ang in (0.0, 1e-4):
        for xw in (0.0, 0.8):
            p = np.array([[4.0, 5.0, xw, 1.0, 0.3, -0.2, 0.1, 0.2, ang]], np.float32)
            for W in (oo.plus_vertices64(p)[0], oo.plus_vertices32(p)[0]):
                want = 1.0 * 5.0 + 4.0 * xw - 1.0 * xw
                cover = rect(-6.0, -6.0, 6.0, 6.0)
                r = oo.overlap64(cover, W)
                assert abs(r["area_T"] - want) < 1e-5 and abs(r["I"] - want) < 1e-5 and abs(r["iou"] - want / 144.0) < 1e-6
                e = oo.emulate32(cover, W)
                assert oo.ratio(r, {k: e[k] for k in ("area_T", "area_C", "I", "iou", "dice")}) <= 0.25
            W = oo.plus_vertices64(p)[0]
            half = rect(0.1, -6.0, 6.0, 6.0)                              # x >= the plus's centre line
            assert abs(oo.overlap64(half, W)["I_raw"] - oo.plus_overlap_b(half, W)[2]) < AB_TOL
            assert abs(oo.plus_overlap_b(cover, W)[0] - want) < 1e-5
    # no area at all: NaN
    flat = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    r = oo.overlap64(flat, flat)
    assert np.isnan(r["iou"]) and np.isnan(r["dice"]) and r["I"] == 0.0


def test_c_tol_is_the_smallest_power_of_two_that_keeps_the_emulation_within_a_quarter():
    worst, where = 0.0, None
    for name in CASES:
        _, rows = case_rows(name)
        for n, (ref, em, _) in enumerate(rows):
            s = max(oo.raw_shares(ref, em))
            if s > worst:
                worst, where = s, (name, n)
            assert oo.ratio(ref, {k: em[k] for k in ("area_T", "area_C", "I", "iou", "dice")}) <= 0.25, (name, n)
    print(f"worst share of u S: {worst:.3f} at {where}; C_TOL = {oo.C_TOL}")
    assert 4 * worst <= oo.C_TOL, (worst, where)
    assert 4 * worst > oo.C_TOL / 2, (worst, where)                       # the power below would not do
    assert np.log2(oo.C_TOL) == int(np.log2(oo.C_TOL))


CATCHES = {"closing edge dropped": ("given 3 x 3", "lens traced 100 x 130"), "tile seam edge dropped": ("given 257 x 1025",),
           "no split at the crossing": ("lens traced 100 x 130",), "baseline 0": ("given 100 x 130, far from the origin",),
           "IoU denominator without - I": ("plus traced 100, 511",), "R transposed": ("lens traced 100 x 130", "plus traced 100, 511"),
           "adjacent pairs counted as crossings": ("given 3 x 3", "plus traced 100, 511")}


@pytest.mark.parametrize("wrong", oo.WRONG)
def test_rule_rejects_wrong_implementations(wrong):
    assert set(CATCHES) == set(oo.WRONG)
    for name in CATCHES[wrong]:
        case, rows = case_rows(name)
        caught = 0
        for n, (ref, _, (count, decided)) in enumerate(rows):
            em = oo.row_emulate32(case, n, wrong)
            if wrong.startswith("adjacent"):
                caught += decided and em["crossings"] != count
            else:
                caught += oo.ratio(ref, {k: em[k] for k in ("area_T", "area_C", "I", "iou", "dice")}) > 1.0
        assert caught >= 1, (wrong, name)


def test_crossing_counts_are_decided_on_every_ledger_row_and_some_are_positive():
    positive = 0
    for name in CASES:
        _, rows = case_rows(name)
        left_out = [n for n, (_, _, (_, decided)) in enumerate(rows) if not decided]
        assert not left_out, (name, left_out)                            # float64 alone leaves out none (so <= 10 % holds)
        for n, (_, em, (count, _)) in enumerate(rows):
            assert em["crossings"] == count, (name, n)
            positive += count > 0
    assert positive >= 1
    _, rows = case_rows("plus traced 100, 511")
    assert sum(c > 0 for _, _, (c, _) in rows) >= 1
