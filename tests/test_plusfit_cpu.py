"""Host-side tests of the plus-shape fit (no GPU): the ABI's declarations and argument checks, the Python argument errors, the
float64 restatement of tests/plusfit_oracle.py against what the real reference recorded (tests/golden/plusfit_*.npz), and the
comparison rules themselves - they accept a float32 emulation of the contract and reject deliberately wrong variants."""
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
import plusfit_oracle as pfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_plusfit_workspace_bytes", "hint_plusfit_run", "hint_plusfit_geometry")
PUBLIC = ("plus_fit_grad", "plus_dominant_angle", "plus_fit_starts", "fit_plus_shapes")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
POINTERS = ("x", "b_points", "starts", "params", "loss", "best", "n_run", "all_params", "all_loss", "grad", "trace")
OUTPUTS = POINTERS[3:]


def good_desc(source="x", n_rows=1000, K=25, P=100):
    desc = _lib.PlusFitDesc()
    for i, f in enumerate(POINTERS):
        setattr(desc, f, BASE + (i << 28))
    if source == "x":
        desc.b_points = None
    else:
        desc.x = None
    desc.n_rows, desc.n_coeffs, desc.n_points, desc.n_starts, desc.n_steps = n_rows, K, P, 9, 400
    desc.lr, desc.angle_lr, desc.gamma, desc.momentum, desc.corner_weight, desc.stop_loss = 0.1, 0.01, pfo.GAMMA, 0.2, 1.0, 0.005
    desc.corner_decay, desc.max_groups = 1, 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_plusfit_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def rejected(what, source="x", **fields):
    desc = good_desc(source)
    for k, v in fields.items():
        setattr(desc, k, v)
    st, msg = run_msg(desc)
    assert st != 0 and what in msg, (fields, msg)
    return msg


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"plusfit_{name}.npz"))


# ---- the ABI ----
def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert set(_lib.exported_symbols()) == declared
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    for cite in ("best_shape_fit.py:93-129", "best_shape_fit.py:54-65", "best_shape_fit.py:108-118", "eval_shapes.py:85-87"):
        assert cite in header, cite
    kernel = open(os.path.join(ROOT, "hint_amd", "csrc", "hint_plusfit.hip")).read()
    for cite in ("best_shape_fit.py:93-129", "best_shape_fit.py:54-65", "eval_shapes.py:85-87"):
        assert cite in kernel.split("#include")[0], cite
    D = _lib.PlusFitDesc
    struct = re.search(r"typedef struct hint_plusfit_desc \{(.*?)\} hint_plusfit_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f[0] for f in D._fields_]                          # the same fields in the same order
    # 2 pointers, int64, 2 int32, pointer, 2 int32, 6 doubles, 2 int32, 8 pointers
    assert C.sizeof(D) == 16 + 8 + 8 + 8 + 8 + 48 + 8 + 64 == 168
    assert [getattr(D, f).offset for f in fields] == [0, 8, 16, 24, 28, 32, 40, 44, 48, 56, 64, 72, 80, 88, 96, 100, 104, 112,
                                                      120, 128, 136, 144, 152, 160]
    assert D.stop_loss.size == 8 and D.corner_decay.size == 4 and D.n_run.size == 8
    for fn in PUBLIC:
        assert getattr(hint_amd, fn) is getattr(curves, fn) and fn in curves.__all__
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)
    # the descriptors before this one are as they were
    assert C.sizeof(_lib.LensFitDesc) == 168 and C.sizeof(_lib.PlusDesc) == 96 and C.sizeof(_lib.HausdorffDesc) == 104
    makefile = open(os.path.join(ROOT, "hint_amd", "csrc", "Makefile")).read()
    assert "hint_plusfit.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, re.M).group(1)
    assert "hint_plusgeom.hpp" in re.search(r"^HDRS\s*:=(.*)$", makefile, re.M).group(1)
    # both plus kernels take the geometry from the one header
    for src in ("hint_plus.hip", "hint_plusfit.hip"):
        text = open(os.path.join(ROOT, "hint_amd", "csrc", src)).read()
        assert '#include "hint_plusgeom.hpp"' in text and "PL_VX =" not in text and "pl_segment(rw" in text, src
    # both fits take the driver - the state, the trace record, the update rule, the selection - from the one header
    assert "hint_fit.hpp" in re.search(r"^HDRS\s*:=(.*)$", makefile, re.M).group(1)
    assert "__fmaf_rn(momentum" in open(os.path.join(ROOT, "hint_amd", "csrc", "hint_fit.hpp")).read()
    for src in ("hint_lensfit.hip", "hint_plusfit.hip"):
        text = open(os.path.join(ROOT, "hint_amd", "csrc", src)).read()
        assert '#include "hint_fit.hpp"' in text and "__fmaf_rn(momentum" not in text and "fit_step(st" in text, src


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for source in ("x", "b_points"):
        rejected("starts is null", source, starts=None)
        rejected("no output requested", source, **{f: None for f in OUTPUTS})
    rejected("both x and b_points", b_points=BASE + (1 << 28))
    rejected("x and b_points are both null", x=None)
    for bad in (0, -3, (1 << 30) + 1):
        assert f"got {bad}" in rejected("n_rows must be 1..1073741824", n_rows=bad)
    for bad in (0, -1, 2, 4, 24, 26, 27):
        assert f"got {bad}" in rejected("n_coeffs must be odd and 1..25", n_coeffs=bad)
    rejected("n_points", "b_points", n_coeffs=4, n_points=1)            # with b_points, n_coeffs is not looked at
    for bad in (-1, 0, 1, 1025):
        for source in ("x", "b_points"):
            assert f"got {bad}" in rejected("n_points must be 2..1024", source, n_points=bad)
    for bad in (0, -1, 17):
        assert f"got {bad}" in rejected("n_starts must be 1..16", n_starts=bad)
    for bad in (-1, 1025):
        assert f"got {bad}" in rejected("n_steps must be 0..1024", n_steps=bad)
    rejected("trace holds a record per step", n_steps=0)
    for field in ("lr", "angle_lr", "gamma", "momentum"):
        for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
            rejected(f"{field} must be finite and >= 0", **{field: bad})
    for bad in (float("nan"), float("inf"), float("-inf")):
        rejected("corner_weight must be finite", corner_weight=bad)
    rejected("max_groups must be >= 0", max_groups=-1)
    for field in POINTERS:
        source = "b_points" if field == "b_points" else "x"
        rejected(f"{field} must be 4-byte aligned", source, **{field: BASE + (12 << 28) + 2})
    # the limits themselves pass the size checks, and any stop_loss does: the first complaint is then about something later
    rejected("max_groups", n_starts=16, n_steps=1024, n_points=1024, n_coeffs=25, max_groups=-1)
    for stop in (0.0, -1.0, float("nan"), float("inf")):
        rejected("max_groups", n_starts=1, n_steps=0, trace=None, n_points=2, n_coeffs=1, lr=0.0, angle_lr=0.0, gamma=0.0,
                 momentum=0.0, corner_weight=-2.0, stop_loss=stop, corner_decay=0, max_groups=-1)


def test_workspace_bytes_agrees_with_run_and_does_not_grow_with_n():
    lib = _lib.load()
    ws = lib.hint_plusfit_workspace_bytes
    for args, what in (((0, 5, 100, 9, 400), "n_rows"), (((1 << 30) + 1, 5, 100, 9, 400), "n_rows"), ((10, 4, 100, 9, 400), "n_coeffs"),
                       ((10, 27, 100, 9, 400), "n_coeffs"), ((10, 5, 1, 9, 400), "n_points"), ((10, 0, 1025, 9, 400), "n_points"),
                       ((10, 5, 100, 0, 400), "n_starts"), ((10, 5, 100, 17, 400), "n_starts"), ((10, 5, 100, 9, -1), "n_steps"),
                       ((10, 5, 100, 9, 1025), "n_steps")):
        ws(10, 5, 100, 9, 400)                                           # a good call in between leaves the message empty
        assert lib.hint_last_error().decode() == ""
        assert ws(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    for args in ((1, 1, 2, 1, 0), (1000, 25, 100, 9, 400), (1 << 30, 25, 1024, 16, 1024), (10, 0, 1000, 9, 400)):
        assert ws(*args) == 0
        assert lib.hint_last_error().decode() == "", args
    assert "workspace" not in [f[0] for f in _lib.PlusFitDesc._fields_]


def test_geometry_is_consistent():
    lib = _lib.load()
    geo = lib.hint_plusfit_geometry
    assert geo(0, 100, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert geo(10, 1025, 0) == -1 and "n_points" in lib.hint_last_error().decode()
    assert geo(10, 100, 5) == -1 and "field" in lib.hint_last_error().decode()
    assert geo(10, 100, -1) == -1
    per, cap, most = geo(1, 2, 2), geo(1, 2, 3), geo(1, 2, 4)
    assert per == 4 and most == curves.MAX_STARTS == 16 and cap >= 256
    for N in (1, 2, 3, cap - 1, cap, cap + 1, 1 << 16, 1 << 30):
        for P in (2, 100, 1024):
            g, rows, pp, c, m = (geo(N, P, f) for f in range(5))
            assert (rows, pp, c, m) == (1, per, cap, most)
            assert g == min(N, cap)                                       # workgroup w takes rows w, w + g, ...: every row is taken


def test_python_argument_errors():
    x, pts, pr = torch.randn(50, 20), torch.randn(50, 100, 2), torch.randn(50, 9)
    for fn, args in ((hint_amd.plus_fit_grad, (pr,)), (hint_amd.fit_plus_shapes, ()), (hint_amd.plus_fit_starts, ()),
                     (hint_amd.plus_dominant_angle, ())):
        name = fn.__name__
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu.*no CPU fallback"):
            fn(x, *args)
        with pytest.raises(HintAmdError, match=name + ": curve is on cpu"):
            fn(pts, *args)
        with pytest.raises(HintAmdError, match=name + ": curve must be a tensor"):
            fn(x.numpy(), *args)
        for bad in (x[0], torch.randn(2, 3, 2, 2)):
            with pytest.raises(HintAmdError, match=name + r": curve must be \[rows, 4 K\] coefficients or \[rows, P, 2\] points"):
                fn(bad, *args)
    for bad in ("1", float("nan"), float("inf"), True):
        with pytest.raises(HintAmdError, match="plus_fit_grad: corner_weight must be"):
            hint_amd.plus_fit_grad(x, pr, bad)
        with pytest.raises(HintAmdError, match="fit_plus_shapes: corner_weight must be"):
            hint_amd.fit_plus_shapes(x, corner_weight=bad)
    with pytest.raises(HintAmdError, match="plus_fit_grad: params must be a tensor"):
        hint_amd.plus_fit_grad(x, None)
    for name in ("lr", "angle_lr", "momentum", "gamma"):
        for bad, what in ((-0.1, "must be >= 0"), (float("nan"), "must be finite"), (float("inf"), "must be finite"),
                          ("0.1", "must be a number"), (True, "must be a number")):
            with pytest.raises(HintAmdError, match=f"fit_plus_shapes: {name} {what}"):
                hint_amd.fit_plus_shapes(x, **{name: bad})
    for bad, what in ((-1, r"must be 0\.\.1024"), (1025, r"must be 0\.\.1024"), (1.0, "must be an int"), (True, "must be an int")):
        with pytest.raises(HintAmdError, match="fit_plus_shapes: n_steps " + what):
            hint_amd.fit_plus_shapes(x, n_steps=bad)
    for bad in ("0.005", True, None):
        with pytest.raises(HintAmdError, match="fit_plus_shapes: stop_loss must be a number"):
            hint_amd.fit_plus_shapes(x, stop_loss=bad)
    with pytest.raises(HintAmdError, match="fit_plus_shapes: corner_decay must be a bool"):
        hint_amd.fit_plus_shapes(x, corner_decay=1)
    # the remaining checks sit behind the device check: they are reached through the helpers the public functions call
    who = "fit_plus_shapes"
    for shape in ((50, 9), (50, 0, 9), (50, 17, 9), (49, 2, 9), (50, 2, 4), (2, 9)):
        with pytest.raises(HintAmdError, match=who + r": starts must have shape \[50, S, 9\] with S 1\.\.16"):
            curves._check_plus_starts_shape(shape, 50, who)
    assert curves._check_plus_starts_shape((50, 1, 9), 50, who) == 1 and curves._check_plus_starts_shape((50, 16, 9), 50, who) == 16
    assert curves._check_number(float("nan"), "stop_loss", who) != curves._check_number(float("nan"), "stop_loss", who)
    assert curves._check_number(-1, "stop_loss", who) == -1.0
    assert len(curves.PLUS_STARTS) == 9 and curves.PLUS_STARTS == tuple((float(a), float(b)) for a, b in pfo.XYSHIFTS)
    # the tree sum lens_fit_starts and plus_fit_starts share: exact on small integers, whatever the count
    for p in (1, 2, 3, 100, 129):
        v = torch.arange(2 * p, dtype=torch.float32).reshape(1, p, 2)
        assert torch.equal(curves._tree_sum(v), v.sum(1))


# ---- the float64 restatement against the reference's record ----
def test_evaluate64_reproduces_the_reference_loss_and_its_autograd_gradient():
    g = golden(pfo.GOLDEN_GRAD["name"])
    x, params = g["x"], g["params"]
    assert (params[[3, 7], 0] == 1.0).all() and (params[[5, 11], 1] == 0.5).all()
    b = co.points64(x, pfo.FIT_P)
    worst, clamps = 0.0, 0
    for n in range(len(x)):
        for w, c in enumerate(pfo.GOLDEN_GRAD["weights"]):
            L, grad, info = pfo.evaluate64(b[n], params[n], c)
            worst = max(worst, abs(L - g["ref_loss"][n, w]), np.abs(grad - g["ref_grad"][n, w]).max())
        clamps += int(not all(pfo._local(params[n].astype(np.float64))[1]))
    print(f"evaluate64 against the reference's float64 autograd: {worst:.3g}; rows with an active clamp: {clamps}")
    assert worst <= 1e-12 and clamps >= 4


def test_fit64_reproduces_the_reference_fit():
    g = golden(pfo.GOLDEN_FIT["name"])
    x = g["x"]
    b = co.trace32(x, pfo.FIT_P)                                          # the reference fits the float32 points
    assert g["ref_n_run"].max() > 1                                       # a row of the fixture made the reference run on
    worst = 0.0
    for n in range(len(x)):
        ref = pfo.fit64(b[n], pfo.starts64(b[n], g["ref_angle"][n]))
        assert ref["n_run"] == g["ref_n_run"][n], n
        worst = max(worst, pfo.param_diff(ref["params"], g["ref_params"][n]))
    print(f"fit64 from the recorded RANSAC angle against the reference's float32 fit: {worst:.3g}")
    assert worst <= 2e-5


# ---- the rules ----
@pytest.mark.parametrize("name,source,P,N,S,c,zero,clamped", [e for e in pfo.EVAL_CASES if e[2] > 2],
                         ids=[e[0] for e in pfo.EVAL_CASES if e[2] > 2])
def test_rules_accept_a_float32_emulation_below_half_of_every_bound(name, source, P, N, S, c, zero, clamped):
    """on exactly the cases of tests/test_gpu_plusfit.py: the cap on undecided evaluations holds, and the emulation of the
    contract's operation order stays below half of every bound"""
    curve, b, dB, params = pfo.eval_case(source, P, N, S, 500 + P, zero, clamped)
    b32 = co.trace32(curve, P) if curve.ndim == 2 else curve.astype(np.float64)
    und, rl, rg = 0, 0.0, np.zeros(9)
    for n in range(N):
        ev = [pfo.evaluate32(b32[n], params[n, s], c) for s in range(S)]
        u, l, gr = pfo.compare_evaluations(b[n], dB[n], c, params[n], [e[0] for e in ev], [e[1] for e in ev])
        und, rl, rg = und + u, max(rl, l), np.maximum(rg, gr)
    print(f"{name}: {und} of {N * S} undecided; emulation error / bound: loss {rl:.3g}, gradient {np.array2string(rg, precision=3)}")
    assert und <= 0.25 * N * S
    assert rl <= 0.5 and (rg <= 0.5).all()
    for r in zero:                                                        # a zero width drops two segments and skips one component
        info = pfo.evaluate64(b[r], params[r, 0], c)[2]
        assert info["kept"].sum() == 10 and info["skip"].tolist() == [False, False, True] + [False] * 6
    for r in clamped:
        assert not all(pfo._local(params[r, 0].astype(np.float64))[1][:2])          # a clamp of the x arm acts


@pytest.mark.parametrize("wrong", pfo.WRONG_EVAL)
def test_evaluation_rule_rejects_wrong_gradients(wrong):
    name, source, P, N, S, c, zero, clamped = pfo.EVAL_CASES[0]
    curve, b, dB, params = pfo.eval_case(source, P, N, S, 500 + P, zero, clamped)
    rows = zero if wrong.startswith("corner mean over 12") else [n for n in range(N) if n not in zero]
    factors = []
    for n in rows:
        L, g, info = pfo.evaluate64(b[n], params[n, 0], c)
        Lw, gw, _ = pfo.evaluate64(b[n], params[n, 0], c, wrong)
        E = pfo.bound_E(info, dB[n])
        with np.errstate(invalid="ignore"):
            r = np.append(np.abs(gw - g) / pfo.grad_bound(g, info, E, c), abs(Lw - L) / pfo.loss_bound(info, E, c))
        factors.append(np.nanmax(r))
    print(f"{wrong}: error / bound per row " + " ".join(f"{f:.3g}" for f in factors))
    # a single evaluation near a fit need not show a variant on every row (a point seldom projects past a segment's end there,
    # and a row's angle derivative may be next to nothing): some row does, by far; the fits below show each on every row
    assert max(factors) > 8.0


def test_update_rule_check_accepts_the_emulation_and_sees_a_buffer_that_is_not_reset():
    x, _ = pfo.plus_rows(pfo.SHORT["seed"], 1)
    b32 = co.trace32(x, pfo.FIT_P)[0]
    st = pfo.starts64(b32, 0.3)[:2].astype(np.float32)
    fit = pfo.emulate32(b32, st, 20, stop_loss=0.0)
    for s in range(2):
        assert pfo.check_update_rule(fit["trace"][s], fit["all_params"][s]) == 0.0
    assert pfo.check_update_rule(fit["trace"][0], fit["all_params"][0], momentum=0.0) > 1.0
    assert pfo.check_update_rule(fit["trace"][0], fit["all_params"][0], angle_lr=pfo.LR) > 1.0
    joined = np.concatenate([fit["trace"][0], fit["trace"][1]])           # the second start must begin with buf = g_0
    assert pfo.check_update_rule(joined[19:], fit["all_params"][1]) > 1.0


def _short():
    N = pfo.SHORT["rows"]
    x, _ = pfo.plus_rows(pfo.SHORT["seed"], N)
    b, b32 = co.points64(x, pfo.FIT_P), co.trace32(x, pfo.FIT_P)
    st = np.stack([pfo.starts64(b[n], pfo.angle64(b[n])[0])[:3] for n in range(N)]).astype(np.float32)
    return x, b, b32, st


@pytest.mark.parametrize("wrong", pfo.WRONG)
def test_short_fit_rule_rejects_wrong_implementations(wrong):
    """the fits' tolerance (16 x the emulation's largest deviation from fit64) is below 1/8 of what every wrong variant misses
    fit64 by, on every row - at 5 steps, where a step of the corner weight's decay is a fifth"""
    x, b, b32, st = _short()
    steps = pfo.SHORT["steps"][-1]
    refs = [pfo.fit64(b[n], st[n], steps, stop_loss=0.0) for n in range(len(x))]
    tol = 16 * max(pfo.fit_dev(pfo.emulate32(b32[n], st[n], steps, stop_loss=0.0), refs[n]) for n in range(len(x)))
    miss = [pfo.fit_dev(pfo.fit64(b[n], st[n], steps, stop_loss=0.0, wrong=wrong), refs[n]) for n in range(len(x))]
    print(f"{wrong}: tolerance {tol:.3g}; misses / tolerance " + " ".join(f"{m / tol:.3g}" for m in miss))
    assert tol < 1e-4 and min(miss) > 8 * tol


def test_the_stop_rule_is_strict_and_ends_the_row():
    x, b, b32, st = _short()
    free = pfo.fit64(b[0], st[0], 5, stop_loss=0.0)
    assert free["n_run"] == 3
    l0 = free["all_loss"][0]
    assert pfo.fit64(b[0], st[0], 5, stop_loss=l0 * 1.01)["n_run"] == 1
    assert pfo.fit64(b[0], st[0], 5, stop_loss=l0)["n_run"] > 1                                    # strict
    assert pfo.fit64(b[0], st[0], 5, stop_loss=l0, wrong="stop compared with <=")["n_run"] == 1
    assert pfo.fit64(b[0], st[0], 5, stop_loss=l0 * 1.01, wrong="no early stop")["n_run"] == 3
    stopped = pfo.fit64(b[0], st[0], 5, stop_loss=l0 * 1.01)
    assert stopped["best"] == 0 and np.isinf(stopped["all_loss"][1:]).all() and np.isnan(stopped["grad"][1:]).all()
    assert np.array_equal(stopped["all_params"][1:], st[0][1:].astype(np.float64))
    for never in (0.0, -1.0, float("nan")):
        assert pfo.fit64(b[0], st[0], 5, stop_loss=never)["n_run"] == 3


def test_the_angles_winner_is_decided_on_most_rows():
    x, _ = pfo.plus_rows(1001, 12)
    b = co.points64(x, pfo.FIT_P)
    res = [pfo.angle64(r) for r in b]
    assert sum(ok for _, ok in res) >= 9                                  # 75 %
    assert all(-np.pi / 2 <= a <= np.pi / 2 for a, _ in res)
    # a straight line's angle, whatever else there is
    t = np.linspace(-2, 2, 40)
    line = np.stack([t, 0.5 * t + 0.1], 1)
    noise = np.random.RandomState(3).uniform(-3, 3, (20, 2))
    a, ok = pfo.angle64(np.concatenate([noise, line]))
    assert abs(a - np.arctan(0.5)) < 1e-3
