"""GPU tests of hint_amd.corrcoef / corr_mse / CorrelationTarget / hint_corr_run against the test-side evaluations of
tests/corr_oracle.py: numpy's float64 statement (whose NaN pattern and counts must be met exactly) and the np.longdouble
evaluation (which every entry and the MSE must meet within the bounds derived there: per entry max(4 e64, (R + slabs + 16) 2^-52)).
Every case's figures go to corr_errors.json (pytest -q swallows prints) in the directory HINT_TEST_RECORDS names, test_records/
in the repository by default.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib
from hint_amd._lib import HintAmdError
import corr_oracle as co
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, R, _ = co.geometry(1, 1)
CAP = co.geometry(1 << 24, 1)[2]


def record(name, rec):
    out = os.environ.get("HINT_TEST_RECORDS") or os.path.join(ROOT, "test_records")
    try:
        os.makedirs(out, exist_ok=True)
        f = os.path.join(out, "corr_errors.json")
        have = json.load(open(f)) if os.path.exists(f) else {}
        have[name] = rec
        json.dump(have, open(f, "w"), indent=1)
    except OSError:
        pass


def bits64(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def gaussian(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def mixed(n, d, seed):
    """dense mixing z @ A + b: every pair of columns is correlated"""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((d, d)) / np.sqrt(d) + 0.5 * np.eye(d)
    return (rs.standard_normal((n, d)) @ A + rs.standard_normal(d)).astype(np.float32)


def hard_columns(n, seed):
    """20 columns: 1 a duplicate of 0, 2 = -2.5 x column 0, 3 = column 0 + 1e-3 noise, 4 the constant 3.0 (zero variance in
    float64, exactly), 5 and 6 offset by 100 and 1e4 at unit spread, 7 and 8 scaled by 1e-6 and 1e6, the rest mixed Gaussians"""
    rs = np.random.RandomState(seed)
    x = mixed(n, 20, seed + 1).astype(np.float64)
    x[:, 1] = x[:, 0]
    x[:, 2] = -2.5 * x[:, 0]
    x[:, 3] = x[:, 0] + 1e-3 * rs.standard_normal(n)
    x[:, 4] = 3.0
    x[:, 5] += 100.0
    x[:, 6] += 1e4
    x[:, 7] *= 1e-6
    x[:, 8] *= 1e6
    x = x.astype(np.float32)
    x[:, 1] = x[:, 0]
    return x


def targets_for(x, seed):
    """the identity; the corrcoef of a second sample; that with NaN entries; that in fp32"""
    n, d = x.shape
    second = co.corrcoef64(mixed(max(n, 3), d, seed + 77))
    holes = second.copy()
    holes[0, :] = np.nan
    holes[d // 2, d - 1] = np.nan
    return {"identity": np.eye(d), "second": second, "holes": holes, "fp32": second.astype(np.float32)}


def device_corr(x):
    xd = torch.as_tensor(x).to(DEV)
    a = hint_amd.corrcoef(xd)
    assert a.shape == (x.shape[1], x.shape[1]) and a.dtype == torch.float64 and a.device == xd.device
    return xd, a


def check_entries(what, got, c64, cl, bound):
    """NaN pattern equal to numpy's (no entry waived), every other entry within its bound of the longdouble value"""
    nan64 = np.isnan(c64)
    assert np.array_equal(np.isnan(np.asarray(cl, dtype=np.float64)), nan64), f"{what}: the two oracles disagree on the NaN pattern"
    assert np.array_equal(np.isnan(got), nan64), f"{what}: NaN pattern differs from numpy's at {np.argwhere(np.isnan(got) != nan64)[:8].tolist()}"
    ok = ~nan64
    err = np.abs(got.astype(np.longdouble) - cl).astype(np.float64)
    worst = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    assert worst <= 1.0, f"{what}: an entry is {worst:.3g} of its bound off the longdouble value (max error {err[ok].max():.3g})"
    assert (np.abs(got[ok]) <= 1.0).all(), what
    return (float(err[ok].max()) if ok.any() else 0.0), worst


def check(name, x, seed=0):
    n, d = x.shape
    xd, a = device_corr(x)
    assert bits64(a, hint_amd.corrcoef(xd)), f"{name}: two runs differ"
    assert bits64(a, a.t()), f"{name}: corr is not symmetric bit for bit"
    got = a.cpu().numpy()
    c64, cl, e64, bound = co.bounds(x)
    max_err, worst = check_entries(name, got, c64, cl, bound)
    ok = ~np.isnan(c64)
    rec = {"n": n, "d": d, "nan_entries": int((~ok).sum()), "max_error": max_err, "max_e64": float(e64[ok].max()) if ok.any() else 0.0,
           "min_bound": float(bound[ok].min()) if ok.any() else 0.0, "worst_error_over_bound": worst, "mse": {}}
    print(f"{name}: corr max error {max_err:.3g} e64 {rec['max_e64']:.3g} bound {rec['min_bound']:.3g} worst ratio {worst:.3g}")

    for tname, t in targets_for(x, seed).items():
        m64 = co.mse64(c64, t)
        ml = co.mse_ld(cl, t)
        mb = co.mse_bound(cl, t, bound, ml)
        with np.errstate(invalid="ignore"):
            count = int((~np.isnan(c64 - t.astype(np.float64))).sum())
        td = torch.as_tensor(t)                                 # on the host: the library moves it
        one = hint_amd.corr_mse(xd, td)
        assert one.shape == () and one.dtype == torch.float64 and one.device == xd.device
        ct = hint_amd.CorrelationTarget(td.to(DEV))
        two = ct.mse(xd)
        assert bits64(one, two), f"{name}/{tname}: corr_mse {float(one)!r} != CorrelationTarget.mse {float(two)!r}"
        assert bits64(ct.corr, a), f"{name}/{tname}: CorrelationTarget.corr differs from corrcoef"
        assert bits64(one, hint_amd.corr_mse(xd, td)), f"{name}/{tname}: two runs differ"
        assert ct.terms.shape == (3,) and ct.terms.dtype == torch.float64
        ssum, cnt, nans = (float(v) for v in ct.terms)
        assert cnt == count, f"{name}/{tname}: {cnt} entries compared, numpy compares {count}"
        assert nans == int((~ok).sum()), f"{name}/{tname}: {nans} NaN entries reported, corr has {int((~ok).sum())}"
        g = float(one)
        rec["mse"][tname] = {"got": g, "float64": m64, "error": abs(g - ml), "e64": abs(m64 - ml), "bound": mb, "count": count}
        print(f"{name}/{tname}: got {g:.17g} float64 {m64:.17g} error {abs(g - ml):.3g} e64 {abs(m64 - ml):.3g} bound {mb:.3g}")
        if count == 0:
            assert np.isnan(g) and np.isnan(m64) and ssum == 0.0, f"{name}/{tname}: nothing to compare, got {g!r}"
        else:
            assert abs(g - ml) <= mb, f"{name}/{tname}: got {g!r}, longdouble {ml!r}, error {abs(g - ml):.3g} > bound {mb:.3g}"
            assert abs(g - ssum / cnt) <= 2.0 ** -52 * g
    record(name, rec)

    # permuted rows; permuted columns; a column scaled by a power of two: the same matrix (permuted) within the same bounds
    rs = np.random.RandomState(seed + 5)
    pr, pc = rs.permutation(n), rs.permutation(d)
    check_entries(name + " rows permuted", device_corr(x[pr])[1].cpu().numpy(), c64, cl, bound)
    ix = np.ix_(pc, pc)
    check_entries(name + " columns permuted", device_corr(np.ascontiguousarray(x[:, pc]))[1].cpu().numpy(), c64[ix], cl[ix], bound[ix])
    xs = x.copy()
    xs[:, d // 3] *= np.float32(2.0 ** 7)
    xs[:, d - 1] *= np.float32(2.0 ** -9)
    check_entries(name + " columns scaled", device_corr(xs)[1].cpu().numpy(), c64, cl, bound)
    return got, c64, cl, bound


SHAPES = [(1, 1), (2, 1), (2, 2), (3, 17), (5, T - 1), (6, T), (7, T + 1), (R - 1, 2 * T + 1), (R + 1, 33), (3 * R - 3, 100),
          (9, 512), (CAP * R + R + 1, 3)]


def test_geometry_the_shapes_rely_on():
    assert co.geometry(3 * R - 3, 100)[1:] == (R, 3) and 3 * R - 3 < 1024 and (3 * R - 3) % R != 0        # three slabs, a ragged last one
    n = SHAPES[-1][0]
    assert n > CAP * R and co.geometry(n, 3)[1] > R and co.geometry(n, 3)[2] == CAP                       # past the slab cap
    assert co.geometry(R + 1, 33)[2] == 2 and co.geometry(R - 1, 33)[2] == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_shapes(shape):
    n, d = shape
    check("gauss_%dx%d" % shape, gaussian(n, d, seed=1000 + 7 * n + d), seed=n + d)


@pytest.mark.parametrize("shape", [(3, 17), (R + 1, 33), (3 * R - 3, 100)], ids=lambda s: "x".join(map(str, s)))
def test_dense_mixing(shape):
    n, d = shape
    check("mixed_%dx%d" % shape, mixed(n, d, seed=2000 + n + d), seed=n)


def test_hard_columns():
    x = hard_columns(3 * R - 3, seed=31)
    got, c64, cl, bound = check("hard_columns", x, seed=31)
    assert np.isnan(got[4]).all() and np.isnan(got[:, 4]).all() and int(np.isnan(got).sum()) == 2 * 20 - 1      # the constant column
    assert got[0, 1] == 1.0 or abs(got[0, 1] - 1.0) <= bound[0, 1]
    assert abs(got[0, 2] + 1.0) <= bound[0, 2] and 0.0 < 1.0 - got[0, 3] < 1e-5


def test_one_nan_and_one_inf_element():
    x = mixed(2 * R + 9, 2 * T + 3, seed=41)
    x[R + 3, 5] = np.nan
    x[7, T + 2] = np.inf
    got, c64, cl, bound = check("nan_inf", x, seed=41)
    bad = np.zeros(x.shape[1], dtype=bool)
    bad[[5, T + 2]] = True
    assert np.array_equal(np.isnan(got), bad[:, None] | bad[None, :])        # their rows and columns, and nothing else
    # ... and the other entries are those of the sample without the two columns (which sit in other tiles there)
    keep = np.flatnonzero(~bad)
    sub = device_corr(np.ascontiguousarray(x[:, keep]))[1].cpu().numpy()
    assert np.abs(sub - got[np.ix_(keep, keep)]).max() <= 2 * bound[np.ix_(keep, keep)].max()
    x[3, 0] = -np.inf
    check("nan_inf_neginf", x, seed=42)


@pytest.mark.parametrize("case", co.GOLDEN_CASES, ids=lambda c: c["name"])
def test_goldens(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"corr_{case['name']}.npz"))
    x, y = co.golden_inputs(case)
    assert abs(co.checksum([x, y]) - float(g["in_checksum"])) < 1e-6
    got, c64, cl, bound = check("golden_" + case["name"], x, seed=case["seed"])
    # the recorded outputs themselves, which carry numpy's own error
    rec_err = np.abs(g["corr"].astype(np.longdouble) - cl).astype(np.float64)
    assert (np.abs(got - g["corr"]) <= bound + rec_err).all()
    xd = torch.from_numpy(x).to(DEV)
    m = float(hint_amd.corr_mse(xd, torch.from_numpy(g["corr_true"])))
    ml = co.mse_ld(cl, g["corr_true"])
    mb = co.mse_bound(cl, g["corr_true"], bound, ml)
    print(f"golden {case['name']}: mse got {m:.17g} recorded {float(g['mse']):.17g} longdouble {ml:.17g} bound {mb:.3g}")
    assert abs(m - ml) <= mb and abs(m - float(g["mse"])) <= mb + abs(float(g["mse"]) - ml)
    # from_sample is correlation_conditional's np.corrcoef(sample.T)
    ct = hint_amd.CorrelationTarget.from_sample(torch.from_numpy(y).to(DEV))
    _, cly, _, boundy = co.bounds(y)
    assert (np.abs(ct.target.cpu().numpy().astype(np.longdouble) - cly) <= boundy).all()
    m2 = float(ct.mse(xd))
    assert abs(m2 - ml) <= mb + 2.0 * float(np.abs(cl - cly).max()) * float(boundy.max())


def run_desc(x, n, d, target, corr, out, ws, ws_bytes, sync=True):
    lib = _lib.load()
    desc = _lib.CorrDesc()
    desc.x, desc.n, desc.d, desc.target, desc.corr, desc.out = x, n, d, target, corr, out
    desc.workspace, desc.workspace_bytes = ws, ws_bytes
    _lib.check(lib.hint_corr_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_corr_run")
    if sync:                              # (tests/test_gpu_streams.py issues it behind a gate and must not wait)
        torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ("both", "corr_only", "target_only"))
def test_run_writes_every_byte_and_stays_inside_its_buffers(mode):
    """hint_corr_run on guard-banded buffers: x 16 bytes past an alignment boundary with odd d and a ragged last slab; corr, out
    and the workspace filled with zeros, NaNs or junk - the same bits every time (so every byte of corr and out is written),
    guards intact, x and the target unchanged"""
    lib = _lib.load()
    n, d = 2 * R + 5, 2 * T + 3
    x = mixed(n, d, seed=21)
    x[:, 6] = 3.0                                            # NaN entries among the outputs as well
    t = co.corrcoef64(mixed(n, d, seed=22))
    gx = Guarded(n * d, align=16).set(torch.from_numpy(x))
    gt = Guarded(2 * d * d, dtype=torch.float64).set(torch.from_numpy(t))
    assert gx.ptr % 32 == 16
    nbytes = lib.hint_corr_workspace_bytes(n, d)
    assert nbytes % 4 == 0
    sx, st = gx.snapshot(), gt.snapshot()
    first = None
    for rep, (fill_o, fill_w) in enumerate([("zero", "zero"), ("zero", "zero")] + [(a, b) for a in FILLS[1:] for b in FILLS[1:]]):
        go = Guarded(2 * 4, fill=fill_o, seed=rep, dtype=torch.float64)
        gc = Guarded(2 * d * d, fill=fill_o, seed=50 + rep, dtype=torch.float64)
        gw = Guarded(nbytes // 4, fill=fill_w, seed=100 + rep)
        run_desc(gx.ptr, n, d, gt.ptr if mode != "corr_only" else None, gc.ptr if mode != "target_only" else None, go.ptr, gw.ptr,
                 nbytes)
        what = f"{mode}: out and corr {fill_o}, workspace {fill_w}"
        go.check_guards(what + ": out")
        gc.check_guards(what + ": corr")
        gw.check_guards(what + ": workspace")
        gx.check_unchanged(sx, what + ": x")
        gt.check_unchanged(st, what + ": target")
        now = (go.t.clone(), gc.t.clone())
        if mode == "target_only":                            # corr was not handed over: untouched
            fresh = Guarded(2 * d * d, fill=fill_o, seed=50 + rep, dtype=torch.float64)
            assert torch.equal(gc.raw, fresh.raw), what
            now = (now[0], None)
        if first is None:
            first = now
        assert bits64(now[0], first[0]), what
        assert now[1] is None or bits64(now[1], first[1]), what
    out = first[0].cpu().numpy()
    c64, cl, e64, bound = co.bounds(x)
    if mode != "target_only":
        check_entries(mode, first[1].view(d, d).cpu().numpy(), c64, cl, bound)
    if mode == "corr_only":
        assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == 0.0
    else:
        ml = co.mse_ld(cl, t)
        assert abs(out[0] - ml) <= co.mse_bound(cl, t, bound, ml) and out[2] == (d - 1) ** 2
    assert out[3] == 2 * d - 1


def test_captured_in_a_single_stream_graph_and_replayed_on_new_contents():
    x, x2 = mixed(2 * R + 5, 20, seed=61), mixed(2 * R + 5, 20, seed=62)
    t = torch.from_numpy(co.corrcoef64(mixed(300, 20, seed=63))).to(DEV)
    xd = torch.from_numpy(x).to(DEV)
    eager = hint_amd.corr_mse(xd, t).clone()                # (also loads the kernels before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hint_amd.corr_mse(xd, t)
    g.replay()
    torch.cuda.synchronize()
    assert bits64(out, eager)
    xd.copy_(torch.from_numpy(x2))
    g.replay()
    torch.cuda.synchronize()
    assert bits64(out, hint_amd.corr_mse(xd, t)) and not bits64(out, eager)
    _, cl, _, bound = co.bounds(x2)
    ml = co.mse_ld(cl, t.cpu().numpy())
    assert abs(float(out) - ml) <= co.mse_bound(cl, t.cpu().numpy(), bound, ml)


def test_python_contract():
    x = mixed(40, 6, seed=51)
    xd = torch.from_numpy(x).to(DEV)
    t = torch.from_numpy(co.corrcoef64(mixed(40, 6, seed=52)))
    want = hint_amd.corr_mse(xd, t)
    # the target: fp32 or fp64, a tensor or an array, on any device
    assert bits64(hint_amd.corr_mse(xd, t.to(DEV)), want) and bits64(hint_amd.corr_mse(xd, t.numpy()), want)
    assert bits64(hint_amd.corr_mse(xd, t.float()), hint_amd.corr_mse(xd, t.float().double()))
    spread = torch.zeros(6, 12, dtype=torch.float64)
    spread[:, ::2] = t
    assert not spread[:, ::2].is_contiguous() and bits64(hint_amd.corr_mse(xd, spread[:, ::2]), want)
    # copies of x are made where needed: other dtypes, non-contiguous views
    assert bits64(hint_amd.corr_mse(xd.double(), t), want)
    wide = torch.zeros(40, 12, device=DEV)
    wide[:, ::2] = xd
    assert not wide[:, ::2].is_contiguous() and bits64(hint_amd.corrcoef(wide[:, ::2]), hint_amd.corrcoef(xd))
    for bad in (t[:5], t[:, :5], t[0], torch.zeros(7, 7)):
        with pytest.raises(HintAmdError, match="corr_true has shape"):
            hint_amd.corr_mse(xd, bad)
        with pytest.raises(HintAmdError):
            hint_amd.CorrelationTarget(bad).mse(xd)
    with pytest.raises(HintAmdError, match="float32 or float64"):
        hint_amd.corr_mse(xd, t.half())
    with pytest.raises(HintAmdError, match="empty"):
        hint_amd.corrcoef(xd[:0])
    with pytest.raises(HintAmdError, match="empty"):
        hint_amd.corr_mse(xd[:, :0], t)
    with pytest.raises(HintAmdError, match="2-D"):
        hint_amd.corrcoef(xd[0])
    with pytest.raises(HintAmdError, match="floating-point"):
        hint_amd.corrcoef(xd.long())
    with pytest.raises(HintAmdError, match="d = 513.*limit"):
        hint_amd.corrcoef(torch.zeros(3, 513, device=DEV))
    xg = xd.clone().requires_grad_(True)
    for call in (hint_amd.corrcoef, lambda v: hint_amd.corr_mse(v, t), hint_amd.CorrelationTarget(t).mse,
                 hint_amd.CorrelationTarget.from_sample):
        with pytest.raises(HintAmdError, match="no gradient of the metric is implemented"):
            call(xg)
    with torch.no_grad():
        assert bits64(hint_amd.corr_mse(xg, t), want)
    assert bits64(hint_amd.corr_mse(xg.detach(), t), want)
    ct = hint_amd.CorrelationTarget(t)
    assert ct.corr is None and ct.terms is None
    assert bits64(ct(xd), want) and bits64(ct.corr, hint_amd.corrcoef(xd))
    torch.cuda.synchronize()
