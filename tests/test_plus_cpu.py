"""CPU-side checks of the plus shape's fit loss and distances (hint_amd.curves plus_segments / plus_outline_counts /
plus_fit_terms / plus_fit_loss / plus_hausdorff_distances, the hint_plus_* entry points; no GPU): header, exports and binding agree,
every argument check of hint_plus_run comes before any device call and names its field, hint_plus_workspace_bytes and
hint_plus_geometry agree with it, the Python functions refuse bad arguments by name, the test-side float64 evaluation
(tests/plus_oracle.py) reproduces what was recorded from the reference's functions, and its comparison rule accepts a float32
emulation of the contract with half of every bound to spare and rejects nine wrong ones."""
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
import plus_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_plus_workspace_bytes", "hint_plus_run", "hint_plus_geometry")
PUBLIC = ("plus_segments", "plus_outline_counts", "plus_fit_terms", "plus_fit_loss", "plus_hausdorff_distances")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
POINTERS = ("x", "b_points", "params", "segments", "keep", "counts", "loss", "max_h", "avg_h")
OUTPUTS = POINTERS[3:]


def good_desc(source="x", n_rows=1000, K=25, P=1000):
    desc = _lib.PlusDesc()
    for i, f in enumerate(POINTERS):
        setattr(desc, f, BASE + (i << 28))
    if source == "x":
        desc.b_points = None
    else:
        desc.x = None
    desc.n_rows, desc.n_coeffs, desc.n_points, desc.max_dist, desc.max_groups = n_rows, K, P, 0.02, 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_plus_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def rejected(what, source="x", **fields):
    desc = good_desc(source)
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
    for cite in ("best_shape_fit.py:15-22", "best_shape_fit.py:26-50", "best_shape_fit.py:54-65", "best_shape_fit.py:153-156",
                 "data.py:176-186", "eval_shapes.py:82-95"):
        assert cite in header, cite
    D = _lib.PlusDesc
    struct = re.search(r"typedef struct hint_plus_desc \{(.*?)\} hint_plus_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f[0] for f in D._fields_]                          # the same fields in the same order
    # 2 pointers, int64, 2 int32, pointer, float, int32, 6 pointers
    assert C.sizeof(D) == 16 + 8 + 8 + 8 + 8 + 48 == 96
    assert [getattr(D, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 40, 44, 48, 56, 64, 72, 80, 88]
    assert D.max_dist.size == 4 and D.keep.size == 8
    for fn in PUBLIC:
        assert getattr(hint_amd, fn) is getattr(curves, fn) and fn in curves.__all__
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)
    # the descriptors before this one are as they were
    assert C.sizeof(_lib.HausdorffDesc) == 104 and C.sizeof(_lib.CurveDesc) == 96


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for source in ("x", "b_points"):
        rejected("params is null", source, params=None)
    rejected("both x and b_points", b_points=BASE + (1 << 28))
    for need in ("loss", "max_h", "avg_h"):                              # each output that reads the curve asks for a source
        others = {f: None for f in ("loss", "max_h", "avg_h") if f != need}
        rejected("x and b_points are both null", x=None, **others)
    for source in ("x", "b_points"):
        rejected("no output requested", source, **{f: None for f in OUTPUTS})
    for bad in (0, -3, (1 << 30) + 1):
        assert f"got {bad}" in rejected("n_rows must be 1..1073741824", n_rows=bad)
        assert f"got {bad}" in rejected("n_rows must be 1..1073741824", n_rows=bad, x=None, loss=None, max_h=None, avg_h=None)
    for bad in (0, -1, 2, 4, 24, 26, 27):
        assert f"got {bad}" in rejected("n_coeffs must be odd and 1..25", n_coeffs=bad)
    for bad in (-1, 0, 1, 1025):
        for source in ("x", "b_points"):
            assert f"got {bad}" in rejected("n_points must be 2..1024", source, n_points=bad)
    for bad in (0.0, -0.02, float("nan"), float("inf"), float("-inf")):
        rejected("max_dist must be finite and > 0", max_dist=bad)
    rejected("max_groups must be >= 0", max_groups=-1)
    for field in POINTERS:
        source = "b_points" if field == "b_points" else "x"
        rejected(f"{field} must be 4-byte aligned", source, **{field: BASE + (9 << 28) + 2})
    # without loss, max_h and avg_h the curve is not read: no source is needed, and its sizes are then not looked at
    desc = good_desc()
    desc.x, desc.loss, desc.max_h, desc.avg_h, desc.n_coeffs, desc.n_points = None, None, None, None, 0, 0
    desc.n_rows = 0                                                      # (rejected all the same, so nothing is launched here)
    st, msg = run_msg(desc)
    assert st != 0 and "n_rows" in msg and "n_points" not in msg and "null" not in msg


def test_workspace_bytes_agrees_with_run_and_does_not_grow_with_n():
    lib = _lib.load()
    for args, what in (((0, 5, 1000), "n_rows"), (((1 << 30) + 1, 5, 1000), "n_rows"), ((10, -1, 1000), "n_coeffs"),
                       ((10, 4, 1000), "n_coeffs"), ((10, 27, 1000), "n_coeffs"), ((10, 5, 1), "n_points"),
                       ((10, 5, 1025), "n_points"), ((10, 0, 1025), "n_points")):
        lib.hint_plus_workspace_bytes(10, 5, 100)                        # a good call in between leaves the message empty
        assert lib.hint_last_error().decode() == ""
        assert lib.hint_plus_workspace_bytes(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    for args in ((1, 1, 2), (1000, 25, 1000), (1 << 16, 25, 1000), (1 << 30, 25, 1024), (10, 0, 1000)):
        assert lib.hint_plus_workspace_bytes(*args) == 0
        assert lib.hint_last_error().decode() == "", args
    assert "workspace" not in [f[0] for f in _lib.PlusDesc._fields_]


def test_geometry_is_consistent():
    lib = _lib.load()
    geo = lib.hint_plus_geometry
    assert geo(0, 1000, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert geo(10, 1025, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert geo(10, 1000, 5) == -1 and "field" in lib.hint_last_error().decode()
    assert geo(10, 1000, -1) == -1
    tile, cap, most = geo(1, 2, 2), geo(1, 2, 3), geo(1, 2, 4)
    assert 256 <= tile <= 4096 and tile % 256 == 0 and cap >= 256 and most == po.MAX_M == curves.MAX_OUTLINE_POINTS
    for N in (1, 2, 3, cap - 1, cap, cap + 1, 1 << 16, 1 << 30):
        for P in (2, 100, 1000, 1024):
            g, rows, tl, c, m = (geo(N, P, f) for f in range(5))
            assert (rows, tl, c, m) == (1, tile, cap, most)
            assert g == min(N, cap)                                       # workgroup w takes rows w, w + g, ...: every row is taken


def test_python_argument_errors():
    x, pts, pr = torch.randn(50, 20), torch.randn(50, 100, 2), torch.randn(50, 9)
    for fn in (hint_amd.plus_segments, hint_amd.plus_outline_counts):
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": params is on cpu.*no CPU fallback"):
            fn(pr)
        with pytest.raises(HintAmdError, match=name + ": params must be a tensor"):
            fn(pr.numpy())
    for bad, what in ((0, "must be finite and > 0"), (-1.0, "must be finite and > 0"), (float("nan"), "must be finite and > 0"), (float("inf"), "must be finite and > 0"),
                      ("0.02", "must be a number"), (True, "must be a number")):
        with pytest.raises(HintAmdError, match="plus_outline_counts: max_dist " + what):
            hint_amd.plus_outline_counts(pr, bad)
        with pytest.raises(HintAmdError, match="plus_hausdorff_distances: max_dist " + what):
            hint_amd.plus_hausdorff_distances(x, pr, max_dist=bad)
    for fn in (hint_amd.plus_fit_terms, hint_amd.plus_fit_loss, hint_amd.plus_hausdorff_distances):
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu.*no CPU fallback"):
            fn(x, pr)
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu"):
            fn(pts, pr)
        with pytest.raises(HintAmdError, match=name + ": curve must be a tensor"):
            fn(x.numpy(), pr)
        for bad in (x[0], torch.randn(2, 3, 2, 2)):
            with pytest.raises(HintAmdError, match=name + r": curve must be \[rows, 4 K\] coefficients or \[rows, P, 2\] points"):
                fn(bad, pr)
    for bad in ("1", float("nan"), True):
        with pytest.raises(HintAmdError, match="plus_fit_loss: corner_weight must be a number"):
            hint_amd.plus_fit_loss(x, pr, bad)
    # the remaining checks sit behind the device check: they are reached through the helpers the public functions call
    who = "plus_fit_terms"
    with pytest.raises(HintAmdError, match=who + ": params is on cpu"):
        curves._plus_params(pr, 50, who)
    for shape in ((8,), (50, 8), (49, 9), (1, 1, 9), (2, 9)):
        with pytest.raises(HintAmdError, match=who + r": params must have shape \[9\], \[1, 9\] or \[50, 9\]: xlength"):
            curves._check_plus_params_shape(shape, 50, who)
    for shape in ((9,), (1, 9), (50, 9)):
        curves._check_plus_params_shape(shape, 50, who)
    for shape in ((8,), (0, 9), (5, 10), (1, 1, 9)):
        with pytest.raises(HintAmdError, match=r"plus_segments: params must have shape \[9\] or \[rows, 9\]"):
            curves._check_plus_params_shape(shape, None, "plus_segments")
    for shape in ((9,), (1, 9), (77, 9)):
        curves._check_plus_params_shape(shape, None, "plus_segments")
    assert curves._check_max_dist(0.02, who) == 0.02 and curves._check_max_dist(1, who) == 1.0


@pytest.mark.parametrize("case", po.GOLDEN_CASES, ids=lambda c: c["name"])
def test_float64_oracle_reproduces_the_reference_outputs(case):
    path = os.path.join(ROOT, "tests", "golden", f"plus_{case['name']}.npz")
    g = np.load(path)
    assert os.path.getsize(path) < 100_000
    n = case["rows"]
    x, pr = g["x"], g["params"]
    assert x.dtype == pr.dtype == np.float32 and 8 <= n <= 16
    assert np.array_equal(x, co.gauss(case["seed"], n, case["K"]))       # the fixture's inputs are the seeded ones
    assert np.array_equal(pr, po.golden_params(case))
    assert (po.half_gap(pr, po.GOLDEN_MAX_DIST) > 1e-3).all()
    ref = po.plus64(pr, x, po.GOLDEN_P, po.GOLDEN_MAX_DIST)
    assert np.array_equal(ref["M"], g["ref_outline_points"]) and np.array_equal(ref["counts"].sum(1), ref["M"])
    assert np.abs(ref["max_h"] - g["ref_max_h"]).max() <= 1e-12
    assert np.abs(ref["avg_h"] - g["ref_avg_h"]).max() <= 1e-12
    fit = po.plus64(pr, x, po.GOLDEN_FIT_P, distances=False)
    for w, weight in enumerate(po.GOLDEN_WEIGHTS):
        assert np.abs(fit["loss"][:, 0] + weight * fit["loss"][:, 1] - g["ref_loss"][:, w]).max() <= 1e-12
    kb = po.keep_bits(ref["keep"])
    assert np.array_equal(kb.sum(1), g["ref_n_segments"])
    for j in range(n):                                                   # the reference's list is the kept segments, in order
        assert np.abs(ref["segments"][j][kb[j]] - g["ref_segments"][j, :kb[j].sum()]).max() <= 1e-12
        assert np.isnan(g["ref_segments"][j, kb[j].sum():]).all()
    for j in case["zero"]:
        assert kb[j].sum() == 10 and not kb[j][5] and not kb[j][11]
    assert sorted(np.nonzero(kb.sum(1) < 12)[0].tolist()) == sorted(case["zero"])


def test_the_fixtures_cover_both_k_and_dropped_segments():
    assert {c["K"] for c in po.GOLDEN_CASES} == {5, 25}
    assert any(len(c["zero"]) == 2 for c in po.GOLDEN_CASES)


# (K, P) and max_dist of the issue's float32 emulation; max_dist = 10 gives M = 12, one point per edge
EMULATED = ((5, 100), (25, 1000), (1, 2), (3, 33))
MAX_DISTS = (0.02, 0.2, 10.0)
_worst = {}


@pytest.mark.parametrize("K,P", EMULATED)
def test_rule_accepts_a_float32_emulation_of_the_contract_below_half_of_every_bound(K, P):
    N = 4 if P == 1000 else 6
    x = co.gauss(40 + K + P, N, K)
    pr = po.draw_params(50 + K + P, N, MAX_DISTS, zero={1: (3,)})         # one row with dropped segments
    assert pr[1, 3] == 0 and po.keep_bits(po.segments64(pr)[1]).sum(1).tolist() == [12, 10] + [12] * (N - 2)
    for md in MAX_DISTS:
        assert (po.half_gap(pr, md) > 1e-3).all()                        # no row is excluded from a comparison
        for curve, name in ((x, "traced"), (po.emulate32(pr)["segments"][:, :, 0, :].astype(np.float32), "given")):
            ref = po.plus64(pr, curve, P, md)
            got = po.emulate32(pr, curve, P, md)
            assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["keep"], ref["keep"])
            if md == 10.0:
                assert (ref["M"] == po.keep_bits(ref["keep"]).sum(1)).all() and ref["M"].max() == 12
            r = po.ratios(ref, got["segments"], got["loss"], got["max_h"], got["avg_h"])
            line = ", ".join(f"{k} {v.max():.3g}" for k, v in r.items())
            print(f"K {K} P {P} max_dist {md} {name}: error / bound {line}")
            for k, v in r.items():
                _worst[k] = max(_worst.get(k, 0.0), float(v.max()))
                assert v.max() <= 0.5, (k, v)
            assert len(po.check(ref, segments=got["segments"], loss=got["loss"], max_h=got["max_h"], avg_h=got["avg_h"])[0]) == 0
    print("worst so far: " + ", ".join(f"{k} {v:.3g}" for k, v in _worst.items()))


def _wrong_case(wrong, N=6):
    """params on which the wrong variant has something to get wrong in every row"""
    pr = po.draw_params(71, N, (0.2,))
    pr[:, 8] = np.where(np.abs(pr[:, 8]) < 0.3, 0.3 + np.abs(pr[:, 8]), pr[:, 8])            # angle != 0
    pr[:, 8] = np.where(np.abs(np.abs(pr[:, 8]) - np.pi) < 0.3, 2.0, pr[:, 8])               # ... and != +-pi
    pr[:, 6:8] = np.where(np.abs(pr[:, 6:8]) < 0.2, 0.3, pr[:, 6:8])                         # offsets != 0
    if wrong == "clamp from the clamped partner":
        pr[:, 4] = pr[:, 0] / 2 - np.float32(0.1)                        # xleft = -0.1: the clamp moves it to yleft - 0.01 <= -0.21
    if wrong in ("dropped segment kept", "mean over 12 corners"):
        pr[:, 2] = 0.0
    return pr


@pytest.mark.parametrize("wrong", po.WRONG)
def test_rule_rejects_wrong_implementations(wrong):
    """each wrong variant misses the oracle by more than 10 x the bound in every row - so the rule has something to reject - and
    the rule rejects it"""
    K, P, md = 5, 100, 0.2
    pr = _wrong_case(wrong)
    N = len(pr)
    x = (co.gauss(72, N, K) * np.float32(3)).astype(np.float32)          # curves of the outline's size
    ref = po.plus64(pr, x, P, md)
    right = po.emulate32(pr, x, P, md)
    names = ("segments", "loss", "max_h", "avg_h")
    assert len(po.check(ref, **{k: right[k] for k in names})[0]) == 0
    got = po.emulate32(pr, x, P, md, wrong=wrong)
    r = po.worst(ref, **{k: got[k] for k in names})
    print(f"{wrong}: error / bound per row {np.array2string(r, precision=3)}")
    assert (r > 10.0).all(), (wrong, r)
    assert set(range(N)) <= set(po.check(ref, **{k: got[k] for k in names})[0].tolist())
    if wrong == "dropped segment kept":
        assert (got["counts"] != ref["counts"]).any(1).all()             # ... and the integers differ as well
    # a value that is not finite fails
    mh = right["max_h"].copy()
    mh[3] = np.nan
    assert 3 in po.check(ref, max_h=mh)[0]


def test_round_half_up_is_told_apart_through_counts():
    """a constructed quotient of exactly n + 0.5: angle 0, dyadic parameters, ywidth = 0.625 and max_dist = 0.25 give 2.5 on the two
    horizontal end edges of the y bar - 2 points by the contract (round half to even), 3 by round half up"""
    pr = np.array([[4, 4, 1, 0.625, 0.25, -0.5, 0.5, -0.25, 0]], np.float32)
    q = po.quotients(pr, 0.25)
    assert q[0, 2] == 2.5 and q[0, 8] == 2.5
    ref = po.plus64(pr, max_dist=0.25)
    right, up = po.emulate32(pr, max_dist=0.25), po.emulate32(pr, max_dist=0.25, half_up=True)
    assert np.array_equal(right["counts"], ref["counts"]) and ref["counts"][0, 2] == ref["counts"][0, 8] == 2
    assert up["counts"][0, 2] == up["counts"][0, 8] == 3 and not np.array_equal(up["counts"], ref["counts"])
    # 3.5 goes up to 4 under both: the rule is half to even, not half down
    assert po.counts64(np.array([[4, 4, 1, 0.875, 0.25, -0.5, 0.5, -0.25, 0]], np.float32), 0.25)[0, 2] == 4


def test_find_max_dist_hits_the_sizes_the_device_tests_need():
    pr = po.draw_params(5, 3)
    for target in (12, 1022, 1024, 1026, 2 * 1024 + 300, 4094, 4096, 4098):      # (even: the edges come in equal pairs)
        md, r = po.find_max_dist(pr, target)
        assert md == float(np.float32(md)) and po.counts64(pr[r:r + 1], md).sum() == target
        assert (po.half_gap(pr, md) > 1e-3).all()
