"""CPU-side checks of hint_amd.corrcoef / corr_mse / CorrelationTarget and the hint_corr_* entry points (no GPU): header,
exports and binding agree, every argument check of hint_corr_run comes before any device call and names its field, the job
table covers every (slab, tile row, tile column >= tile row) exactly once with slabs that partition the rows, the workspace is
monotone and under its stated bound, and the test-side evaluations (tests/corr_oracle.py) agree with the recorded outputs and
with closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, metrics
from hint_amd._lib import HintAmdError
import corr_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_corr_workspace_bytes", "hint_corr_run", "hint_corr_job")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
MAX_N, MAX_D = 1 << 24, 512
WORKSPACE_BOUND = 68 << 20      # what include/hint_amd.h states


def good_desc(n=1000, d=37):
    lib = _lib.load()
    desc = _lib.CorrDesc()
    desc.x, desc.target, desc.corr = BASE, BASE + (1 << 24), BASE + (2 << 24)
    desc.out, desc.workspace = BASE + (3 << 24), BASE + (4 << 24)
    desc.n, desc.d = n, d
    desc.workspace_bytes = lib.hint_corr_workspace_bytes(n, d)
    assert desc.workspace_bytes > 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_corr_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert "run_experiments.py:212-221" in header and "rejection_sampling.py:105-132" in header
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    # a pointer, 2 int32, 4 pointers, a size_t
    D = _lib.CorrDesc
    assert C.sizeof(D) == 8 + 2 * 4 + 4 * 8 + 8 == 56
    assert [getattr(D, f).offset for f in ("x", "n", "d", "target", "corr", "out", "workspace", "workspace_bytes")] == \
        [0, 8, 12, 16, 24, 32, 40, 48]
    assert hint_amd.corrcoef is metrics.corrcoef and hint_amd.corr_mse is metrics.corr_mse
    assert hint_amd.CorrelationTarget is metrics.CorrelationTarget


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("x", "out", "workspace"):
        desc = good_desc()
        setattr(desc, field, None)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} is null" in msg, msg
    desc = good_desc()
    desc.target = desc.corr = None
    st, msg = run_msg(desc)
    assert st != 0 and "target and corr are both null" in msg, msg
    for field in ("n", "d"):
        for bad in (0, -3):
            desc = good_desc()
            setattr(desc, field, bad)
            st, msg = run_msg(desc)
            assert st != 0 and f"{field} must be >= 1" in msg, msg
    desc = good_desc()
    desc.d = MAX_D + 1
    st, msg = run_msg(desc)
    assert st != 0 and "d = 513" in msg and "limit" in msg, msg
    desc = good_desc()
    desc.n = MAX_N + 1
    st, msg = run_msg(desc)
    assert st != 0 and "n = 16777217" in msg and "limit" in msg, msg
    for field, align in (("x", 4), ("target", 8), ("corr", 8), ("out", 8), ("workspace", 16)):
        desc = good_desc()
        setattr(desc, field, BASE + (5 << 24) + align // 2)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} must be {align}-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace_bytes -= 1
    st, msg = run_msg(desc)
    assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg
    # at the limits themselves only the workspace size is left to refuse
    desc = good_desc(MAX_N, MAX_D)
    desc.workspace_bytes -= 1
    st, msg = run_msg(desc)
    assert st != 0 and "too small" in msg, msg


def test_workspace_bytes_and_job_reject_bad_sizes():
    lib = _lib.load()
    for n, d, what in ((0, 5, "n must be >= 1"), (5, 0, "d must be >= 1"), (5, MAX_D + 1, "limit"), (MAX_N + 1, 5, "limit")):
        assert lib.hint_corr_workspace_bytes(n, d) == 0 and what in lib.hint_last_error().decode()
        assert lib.hint_corr_job(n, d, -1, 0) == -1 and what in lib.hint_last_error().decode()
    count = lib.hint_corr_job(700, 40, -1, 0)
    assert count == 3 * 6
    for j, f in ((count, 0), (-2, 0), (0, 5), (0, -1), (-1, 4)):
        assert lib.hint_corr_job(700, 40, j, f) == -1 and "no job" in lib.hint_last_error().decode()


def test_geometry_tile_edge_slab_rows_and_cap():
    T, R, slabs = co.geometry(1, 1)
    assert T == 16 and R <= 256 and slabs == 1             # the f64 MFMA's tile; the smallest R is at most 256
    R0 = R
    cap = 0
    for n in (1, 2, R0 - 1, R0, R0 + 1, 3 * R0 - 3, 10000, 64 * R0, 64 * R0 + 1, 100000, MAX_N - 1, MAX_N):
        _, R, slabs = co.geometry(n, 7)
        assert R >= R0 and R % 4 == 0 and slabs == -(-n // R), n
        cap = max(cap, slabs)
    assert cap <= 64 and co.geometry(MAX_N, 7)[2] == cap   # the slab count is capped: R grows with n instead
    assert co.geometry(3 * R0 - 3, 100)[1:] == (R0, 3)      # three slabs, a ragged last one, below 1024 rows
    assert 3 * R0 - 3 < 1024


@pytest.mark.parametrize("shape", [(1, 1), (5, 15), (6, 16), (7, 17), (255, 33), (257, 33), (765, 100), (9, 512), (16641, 4),
                                   (100000, 40)], ids=lambda s: "x".join(map(str, s)))
def test_job_table_covers_every_slab_tile_once_and_slabs_partition_the_rows(shape):
    n, d = shape
    jobs, T, R, slabs = metrics.corr_jobs(n, d)
    nt = -(-d // T)
    want = {(s, i, j) for s in range(slabs) for i in range(nt) for j in range(i, nt)}
    assert len(jobs) == len(want) and {j[:3] for j in jobs} == want          # ... so each appears exactly once
    rows = {}
    for s, ti, tj, r0, nr in jobs:
        assert rows.setdefault(s, (r0, nr)) == (r0, nr)                      # one row range per slab
    pos = 0
    for s in range(slabs):
        r0, nr = rows[s]
        assert r0 == pos == s * R and 1 <= nr <= R
        pos += nr
    assert pos == n


def test_workspace_is_monotone_and_under_the_stated_bound():
    lib = _lib.load()
    ns = [1, 2, 255, 256, 257, 765, 4000, 10000, 16384, 16385, 16641, 100000, 1 << 20, MAX_N - 1, MAX_N]
    ds = [1, 15, 16, 17, 20, 100, 256, 511, 512]
    table = [[lib.hint_corr_workspace_bytes(n, d) for d in ds] for n in ns]
    for a in range(len(ns)):
        for b in range(len(ds)):
            assert table[a][b] > 0 and table[a][b] % 256 == 0
            assert a == 0 or table[a][b] >= table[a - 1][b], (ns[a], ds[b])
            assert b == 0 or table[a][b] >= table[a][b - 1], (ns[a], ds[b])
    assert table[-1][-1] <= WORKSPACE_BOUND
    # column sums, one 16 x 16 tile of doubles per job, and the summed tiles
    for n, d in ((1, 1), (765, 100), (10000, 100), (MAX_N, MAX_D)):
        T, R, slabs = co.geometry(n, d)
        nt = -(-d // T)
        tri = nt * (nt + 1) // 2
        need = (slabs + 1) * tri * T * T * 8
        assert need <= lib.hint_corr_workspace_bytes(n, d) <= need + 64 * nt * T * 8, (n, d)
    assert lib.hint_corr_workspace_bytes(10000, 100) < 3 << 20


@pytest.mark.parametrize("case", co.GOLDEN_CASES, ids=lambda c: c["name"])
def test_oracle_agrees_with_the_recorded_outputs(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"corr_{case['name']}.npz"))
    x, y = co.golden_inputs(case)
    assert (int(g["seed"]), int(g["n"]), int(g["d"])) == (case["seed"], case["n"], case["d"])
    assert abs(co.checksum([x, y]) - float(g["in_checksum"])) < 1e-6, "regenerated inputs differ from the fixture's"
    d = case["d"]
    assert g["corr"].shape == g["corr_true"].shape == (d, d) and g["corr"].dtype == np.float64
    # the float64 statement on the regenerated inputs: a BLAS of another build may order the sums differently
    c64, cl, e64, bound = co.bounds(x)
    print(f"{case['name']}: max e64 {e64.max():.3g}, max bound {bound.max():.3g}, mse {float(g['mse']):.9g}")
    assert e64.max() < 1e-14 and bound.max() < 1e-12                # (the bound says something)
    assert np.abs(g["corr"] - c64).max() <= 2 * e64.max() + 2.0 ** -50
    assert np.abs(g["corr_true"] - co.corrcoef64(y)).max() <= 1e-14
    assert np.abs(g["corr"].astype(np.longdouble) - cl).max() <= 1e-14
    mse = co.mse64(g["corr"], g["corr_true"])
    assert abs(mse - float(g["mse"])) <= 2.0 ** -50 * mse and mse > 1e-6
    assert abs(co.mse_ld(cl, g["corr_true"]) - mse) <= co.mse_bound(cl, g["corr_true"], bound, mse)


def test_oracle_closed_forms():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((50, 5)).astype(np.float32)
    x[:, 1] = x[:, 0]                       # a duplicate: 1
    x[:, 2] = -2.0 * x[:, 0]                # negated and scaled (exactly, in fp32): -1
    x[:, 3] = 3.0                           # constant: zero variance, a NaN row and column
    for f in (co.corrcoef64, co.corrcoef_ld):
        c = np.asarray(f(x), dtype=np.float64)
        assert abs(c[0, 1] - 1.0) <= 1e-15 and abs(c[0, 2] + 1.0) <= 1e-15 and abs(c[1, 2] + 1.0) <= 1e-15
        assert np.isnan(c[3]).all() and np.isnan(c[:, 3]).all() and int(np.isnan(c).sum()) == 9
        assert abs(c[4, 4] - 1.0) <= 1e-15 and abs(c[0, 4]) < 0.6 and c[0, 4] == c[4, 0]
    # two points per column: r = +-1 by the sign of the slopes
    two = np.array([[0.0, 1.0, 5.0], [1.0, 3.0, 2.0]], dtype=np.float32)
    sign = np.array([[1, 1, -1], [1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    assert np.abs(np.asarray(co.corrcoef_ld(two), dtype=np.float64) - sign).max() <= 1e-15
    assert np.abs(co.corrcoef64(two) - sign).max() <= 1e-15
    # one row: every entry NaN, and a mean over nothing is NaN
    one = np.asarray(co.corrcoef_ld(x[:1]), dtype=np.float64)
    assert np.isnan(one).all() and np.isnan(co.corrcoef64(x[:1])).all() and co.corrcoef64(x[:1, :1]).shape == (1, 1)
    assert np.isnan(co.mse64(one, np.eye(5))) and np.isnan(co.mse_ld(one.astype(np.longdouble), np.eye(5)))
    # the MSE against the identity counts the non-NaN entries only
    c = co.corrcoef64(x)
    ok = ~np.isnan(c)
    assert abs(co.mse64(c, np.eye(5)) - np.square(c - np.eye(5))[ok].sum() / 16) <= 1e-15


def test_python_api_argument_errors():
    x = torch.randn(6, 3)
    for call, who in ((lambda t: hint_amd.corrcoef(t), "corrcoef"), (lambda t: hint_amd.corr_mse(t, torch.eye(3)), "corr_mse"),
                      (lambda t: hint_amd.CorrelationTarget(torch.eye(3)).mse(t), "CorrelationTarget.mse")):
        with pytest.raises(HintAmdError, match=who + ": x is on cpu.*no CPU fallback"):
            call(x)
        with pytest.raises(HintAmdError, match="2-D"):
            call(x[0])
        with pytest.raises(HintAmdError, match="must be a tensor"):
            call(x.numpy())
    with pytest.raises(HintAmdError, match="CorrelationTarget.*square"):
        hint_amd.CorrelationTarget(torch.zeros(3, 4))
    with pytest.raises(HintAmdError, match="CorrelationTarget.*square"):
        hint_amd.CorrelationTarget(torch.zeros(3))
    with pytest.raises(HintAmdError, match="x is on cpu"):
        hint_amd.CorrelationTarget.from_sample(x)
    # the target's own checks (they run before any device work)
    dev = torch.device("cpu")
    with pytest.raises(HintAmdError, match=r"corr_true has shape \(3, 4\).*expected \(3, 3\)"):
        metrics._check_target(torch.zeros(3, 4), 3, dev, "corr_mse")
    with pytest.raises(HintAmdError, match=r"corr_true has shape \(2, 2\)"):
        metrics._check_target(np.zeros((2, 2)), 3, dev, "corr_mse")
    with pytest.raises(HintAmdError, match="expected float32 or float64"):
        metrics._check_target(torch.zeros(3, 3, dtype=torch.int64), 3, dev, "corr_mse")
    with pytest.raises(HintAmdError, match="expected float32 or float64"):
        metrics._check_target(torch.zeros(3, 3, dtype=torch.float16), 3, dev, "corr_mse")
    t32 = torch.tensor([[1.0, 0.1], [0.1, 1.0]], dtype=torch.float32)
    t = metrics._check_target(t32, 2, dev, "corr_mse")
    assert t.dtype == torch.float64 and t.is_contiguous() and torch.equal(t.float(), t32)       # fp32 -> fp64 is exact
    assert metrics._check_target(t.t(), 2, dev, "corr_mse").is_contiguous()
