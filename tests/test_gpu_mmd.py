"""GPU tests of hint_amd.multi_mmd / MultiMMD / hint_mmd_run against the test-side float64 evaluation (tests/mmd_oracle.py).

Tolerance, for the MMD and for each of its three terms:   |got - float64| <= max(4 e32, 2^-22 S)
  e32   the error of the Gram-trick formulation in fp32 torch ops (mmd_oracle.gram_terms32) on the same inputs, in the same test;
        the factor 4 because that error is erratic from case to case
  S     mean XX + mean YY + 2 mean XY of the float64 evaluation; 2^-22 S is twice what rounding three fp32 means costs
Every case's got / e32 / bound goes to mmd_errors.json (pytest -q swallows prints) in the directory HINT_TEST_RECORDS names,
test_records/ in the repository by default.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, metrics
from hint_amd._lib import HintAmdError
import mmd_oracle as mo
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = _lib.load().hint_mmd_job(1, 1, 0, -1, 1)
NAMES = ("mmd", "xx", "yy", "xy")


def record(name, got, want, e32, bound):
    out = os.environ.get("HINT_TEST_RECORDS") or os.path.join(ROOT, "test_records")
    try:
        os.makedirs(out, exist_ok=True)
        f = os.path.join(out, "mmd_errors.json")
        have = json.load(open(f)) if os.path.exists(f) else {}
        have[name] = {n: {"got": g, "float64": w, "error": abs(g - w), "e32": e, "bound": b}
                      for n, g, w, e, b in zip(NAMES, got, want, e32, bound)}
        json.dump(have, open(f, "w"), indent=1)
    except OSError:
        pass


def make_sets(n_x, n_y, d, seed, offset=0.0, scale=1.0):
    """x ~ offset + scale N(0, 1), y ~ offset + scale (0.3 + 1.2 N(0, 1)), fp32"""
    rs = np.random.RandomState(seed)
    x = (offset + scale * rs.standard_normal((n_x, d))).astype(np.float32)
    y = (offset + scale * (0.3 + 1.2 * rs.standard_normal((n_y, d)))).astype(np.float32)
    return x, y


def run_all(x, y, kernels=mo.DEFAULT):
    """[MMD, mean XX, mean YY, mean XY] as floats, through both public routes (which must agree bit for bit)"""
    xd, yd = torch.as_tensor(x).to(DEV), torch.as_tensor(y).to(DEV)
    one = hint_amd.multi_mmd(xd, yd, kernels)
    assert one.shape == () and one.dtype == torch.float32 and one.device == xd.device
    m = hint_amd.MultiMMD(yd, kernels)
    two = m.mmd(xd)
    assert m.terms.shape == (3,)
    assert bits_equal(one, two), (float(one), float(two))
    return [float(one)] + [float(t) for t in m.terms]


def check(name, x, y, kernels=mo.DEFAULT, want=None):
    got = run_all(x, y, kernels)
    want, e32, bound = mo.bounds(x, y, kernels, want)
    record(name, got, want, e32, bound)
    for n, g, w, e, b in zip(NAMES, got, want, e32, bound):
        print(f"{name} {n}: got {g:.9g} float64 {w:.9g} error {abs(g - w):.3g} e32 {e:.3g} bound {b:.3g}")
    for n, g, w, b in zip(NAMES, got, want, bound):
        assert abs(g - w) <= b, f"{name} {n}: got {g!r}, float64 {w!r}, error {abs(g - w):.3g} > bound {b:.3g}"
    assert abs(got[0] - (got[1] + got[2] - 2.0 * got[3])) <= 2.0 ** -23 * (abs(got[0]) + 1e-30) + 1e-45       # out[0] is built from the stored means
    return got, want, bound


@pytest.mark.parametrize("case", mo.GOLDEN_CASES, ids=lambda c: c["name"])
def test_goldens(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"mmd_{case['name']}.npz"))
    x, y = mo.golden_inputs(case)
    assert abs(mo.checksum([x, y]) - float(g["in_checksum"])) < 1e-6
    got, want, bound = check("golden_" + case["name"], x, y, case["kernels"])
    # ... and the reference's recorded output itself, which carries its own fp32 error
    assert abs(got[0] - float(g["ref_mmd"])) <= bound[0] + abs(float(g["ref_mmd"]) - want[0])


RAGGED = [(1, 1, 1), (1, 17, 3), (15, 16, 4), (17, 33, 5), (T + 1, 2 * T + 1, 20), (3 * T - 3, 2 * T + 5, 100),
          (3 * T - 3, 3 * T - 3, 131)]


@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes(shape):
    n_x, n_y, d = shape
    x, y = make_sets(n_x, n_y, d, seed=100 + n_x + 7 * n_y + d)
    check("ragged_%dx%dx%d" % shape, x, y)
    check("ragged_other_%dx%dx%d" % shape, x, y, mo.OTHER)


def test_hard_data_offset_30():
    """every coordinate offset by 30: r_i + r_j is about 36000 while D stays about 50 - fails unless both sets are centred and a
    row against itself gives exactly 0"""
    n = 2 * T + 5
    x, y = make_sets(n, n, 20, seed=7, offset=30.0)
    got, want, bound = check("offset30", x, y)
    # the same sets without the offset are another draw of fp32 roundings of the same points: the value moves little
    x0, y0 = make_sets(n, n, 20, seed=7)
    assert abs(got[0] - mo.mmd_terms64(x0, y0)[0]) <= 1e-4 * want[0]


def test_hard_data_small_scale():
    n = 2 * T + 5
    x, y = make_sets(n, n, 20, seed=8, scale=0.1)          # D << C: every kernel value is close to k(0), the terms cancel
    check("scale0.1", x, y)
    check("scale0.1_other", x, y, mo.OTHER)


def test_identical_sets_give_zero_within_the_floor():
    n = 2 * T + 5
    x, _ = make_sets(n, n, 20, seed=9)
    got, want, bound = check("y_is_x", x, x.copy())
    S = want[1] + want[2] + 2.0 * want[3]
    assert want[0] == 0.0 and abs(got[0]) <= 2.0 ** -22 * S
    assert got[1] == got[2]                                  # XX and YY ran on the same bits


def test_multimmd_is_bit_identical_with_fewer_jobs():
    n_x, n_y, d = 2 * T + 5, 3 * T - 3, 20
    x, y = make_sets(n_x, n_y, d, seed=11)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    m = hint_amd.MultiMMD(yd)
    yy0 = m.terms[1].clone()
    for k in range(3):                                       # several samples against one ground truth
        xk = xd * (1.0 + 0.1 * k)
        assert bits_equal(m.mmd(xk), hint_amd.multi_mmd(xk, yd))
        assert bits_equal(m.terms[1], yy0)
    assert bits_equal(m(xd), hint_amd.multi_mmd(xd, yd))
    full, _ = metrics.mmd_jobs(n_x, n_y, False)
    fewer, _ = metrics.mmd_jobs(n_x, n_y, True)
    nty = -(-n_y // T)
    assert len(full) - len(fewer) == nty * (nty + 1) // 2 and all(j[0] != 1 for j in fewer)


def run_desc(x, y, n_x, n_y, d, kernels, out, ws, ws_bytes, yy=None, sync=True):
    lib = _lib.load()
    desc = _lib.MmdDesc()
    desc.x, desc.y, desc.n_x, desc.n_y, desc.d, desc.n_kernels = x, y, n_x, n_y, d, len(kernels)
    for k, (Cw, a) in enumerate(kernels):
        desc.width[k], desc.exponent[k] = Cw, a
    desc.yy, desc.out, desc.workspace, desc.workspace_bytes = yy, out, ws, ws_bytes
    _lib.check(lib.hint_mmd_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_mmd_run")
    if sync:                              # (tests/test_gpu_streams.py issues it behind a gate and must not wait)
        torch.cuda.synchronize()


@pytest.mark.parametrize("with_yy", (False, True), ids=("full", "yy_given"))
def test_run_is_reproducible_and_ignores_what_out_and_workspace_held(with_yy):
    """hint_mmd_run on guard-banded buffers: x and y 16 bytes past an alignment boundary with odd d, out and the workspace
    filled with zeros, NaNs or junk - the same bits every time, guards intact, inputs unchanged"""
    lib = _lib.load()
    n_x, n_y, d = T + 3, 2 * T + 1, 7
    x, y = make_sets(n_x, n_y, d, seed=21)
    gx = Guarded(n_x * d, align=16).set(torch.from_numpy(x))
    gy = Guarded(n_y * d, align=16).set(torch.from_numpy(y))
    assert gx.ptr % 32 == 16 and gy.ptr % 32 == 16
    nbytes = lib.hint_mmd_workspace_bytes(n_x, n_y, d)
    assert nbytes % 4 == 0
    gyy = Guarded(1)
    first = None
    if with_yy:
        o, w = Guarded(4), Guarded(nbytes // 4)
        run_desc(gx.ptr, gy.ptr, n_x, n_y, d, mo.DEFAULT, o.ptr, w.ptr, nbytes)
        gyy.set(o.t[2:3].clone())
        full = o.t.clone()
    sx, sy, syy = gx.snapshot(), gy.snapshot(), gyy.snapshot()
    for rep, (fill_o, fill_w) in enumerate([("zero", "zero"), ("zero", "zero")] + [(a, b) for a in FILLS[1:] for b in FILLS[1:]]):
        go = Guarded(4, fill=fill_o, seed=rep)
        gw = Guarded(nbytes // 4, fill=fill_w, seed=100 + rep)
        run_desc(gx.ptr, gy.ptr, n_x, n_y, d, mo.DEFAULT, go.ptr, gw.ptr, nbytes, yy=gyy.ptr if with_yy else None)
        what = f"out {fill_o}, workspace {fill_w}"
        go.check_guards(what + ": out")
        gw.check_guards(what + ": workspace")
        gx.check_unchanged(sx, what + ": x")
        gy.check_unchanged(sy, what + ": y")
        gyy.check_unchanged(syy, what + ": yy")
        assert bool(torch.isfinite(go.t).all()), what
        if first is None:
            first = go.t.clone()
        assert bits_equal(go.t, first), what
    if with_yy:
        assert bits_equal(first, full)
    want, e32, bound = mo.bounds(x, y)
    assert abs(float(first[0]) - want[0]) <= bound[0]


def test_captured_in_a_single_stream_graph_and_replayed_on_new_contents():
    n_x, n_y, d = 2 * T + 5, T + 1, 20
    x, y = make_sets(n_x, n_y, d, seed=31)
    x2, _ = make_sets(n_x, n_y, d, seed=32)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    eager = hint_amd.multi_mmd(xd, yd).clone()              # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hint_amd.multi_mmd(xd, yd)
    g.replay()
    torch.cuda.synchronize()
    assert bits_equal(out, eager)
    xd.copy_(torch.from_numpy(x2 * 1.5))
    g.replay()
    torch.cuda.synchronize()
    assert bits_equal(out, hint_amd.multi_mmd(xd, yd))
    assert not bits_equal(out, eager)
    want, e32, bound = mo.bounds(x2 * 1.5, y)
    assert abs(float(out) - want[0]) <= bound[0]


def test_swapping_the_sets_changes_nothing_within_the_bound():
    x, y = make_sets(2 * T + 5, T + 1, 20, seed=41)
    a, want, bound = check("swap_xy", x, y)
    b, _, _ = check("swap_yx", y, x)
    assert abs(a[0] - b[0]) <= bound[0]
    assert abs(a[1] - b[2]) <= bound[1] and abs(a[2] - b[1]) <= bound[2] and abs(a[3] - b[3]) <= bound[3]


def test_python_contract():
    x, y = make_sets(40, 30, 6, seed=51)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    want = hint_amd.multi_mmd(xd, yd)
    # copies are made where needed: other dtypes, non-contiguous views
    assert bits_equal(hint_amd.multi_mmd(xd.double(), yd.half().float().double()), hint_amd.multi_mmd(xd, yd.half().float()))
    wide = torch.zeros(40, 12, device=DEV)
    wide[:, ::2] = xd
    assert not wide[:, ::2].is_contiguous() and bits_equal(hint_amd.multi_mmd(wide[:, ::2], yd), want)
    assert bits_equal(hint_amd.multi_mmd(xd, yd, [(0.5, 1), (0.2, 1), (0.2, 0.5)]), want)
    with pytest.raises(HintAmdError, match="empty"):
        hint_amd.multi_mmd(xd[:0], yd)
    with pytest.raises(HintAmdError, match="empty"):
        hint_amd.MultiMMD(yd[:, :0])
    with pytest.raises(HintAmdError, match="6 features.*5"):
        hint_amd.multi_mmd(xd, yd[:, :5])
    with pytest.raises(HintAmdError, match="2-D"):
        hint_amd.multi_mmd(xd, yd[0])
    with pytest.raises(HintAmdError, match="cpu.*no CPU fallback"):
        hint_amd.multi_mmd(xd, yd.cpu())
    with pytest.raises(HintAmdError, match="floating-point"):
        hint_amd.multi_mmd(xd.long(), yd)
    xg = xd.clone().requires_grad_(True)
    with pytest.raises(HintAmdError, match="no gradient of the metric is implemented"):
        hint_amd.multi_mmd(xg, yd)
    with pytest.raises(HintAmdError, match="no gradient"):
        hint_amd.MultiMMD(yd).mmd(xg)
    with torch.no_grad():
        assert bits_equal(hint_amd.multi_mmd(xg, yd), want)
    assert bits_equal(hint_amd.multi_mmd(xg.detach(), yd), want)
    with pytest.raises(HintAmdError, match="exponent of kernel 0"):
        hint_amd.multi_mmd(xd, yd, [(0.5, 0.0)])
    torch.cuda.synchronize()


def test_evaluation_size_against_a_float64_gram_evaluation_on_the_gpu():
    """N = M = 4000, d = 100: what compare_unconditional / compare_conditional score per model and run"""
    g = torch.Generator(device=DEV).manual_seed(61)
    x = torch.randn(4000, 100, generator=g, device=DEV)
    y = 0.05 + 1.05 * torch.randn(4000, 100, generator=g, device=DEV)
    want = mo.gram_terms64(x, y)
    check("n4000_d100", x, y, want=want)
