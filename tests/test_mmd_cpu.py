"""CPU-side checks of hint_amd.multi_mmd and the hint_mmd_* entry points (no GPU): header, exports and binding agree, every
argument check of hint_mmd_run comes before any device call and names its field, the job table covers every tile of the three
pair matrices exactly once with the right weights, and the test-side float64 evaluation (tests/mmd_oracle.py) agrees with the
reference's recorded outputs and with a closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, metrics
from hint_amd._lib import HintAmdError
import mmd_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_mmd_workspace_bytes", "hint_mmd_run", "hint_mmd_job")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them


def good_desc(n_x=100, n_y=90, d=7):
    lib = _lib.load()
    desc = _lib.MmdDesc()
    desc.x, desc.y, desc.out, desc.workspace = BASE, BASE + (1 << 24), BASE + (2 << 24), BASE + (3 << 24)
    desc.n_x, desc.n_y, desc.d, desc.n_kernels = n_x, n_y, d, 3
    for k, (Cw, a) in enumerate(mo.DEFAULT):
        desc.width[k], desc.exponent[k] = Cw, a
    desc.yy = None
    desc.workspace_bytes = lib.hint_mmd_workspace_bytes(n_x, n_y, d)
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_mmd_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    # 2 pointers, 4 int32, 2 x 8 floats, 3 pointers, a size_t
    assert C.sizeof(_lib.MmdDesc) == 2 * 8 + 4 * 4 + 2 * 8 * 4 + 3 * 8 + 8 == 128
    assert _lib.MmdDesc.yy.offset == 96 and _lib.MmdDesc.workspace_bytes.offset == 120
    assert hint_amd.multi_mmd is metrics.multi_mmd and hint_amd.MultiMMD is metrics.MultiMMD
    assert metrics.DEFAULT_WIDTHS_EXPONENTS == mo.DEFAULT


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("x", "y", "out", "workspace"):
        desc = good_desc()
        setattr(desc, field, None)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} is null" in msg, msg
    for field in ("n_x", "n_y", "d"):
        for bad in (0, -3):
            desc = good_desc()
            setattr(desc, field, bad)
            st, msg = run_msg(desc)
            assert st != 0 and f"{field} must be >= 1" in msg, msg
    desc = good_desc()
    desc.d = 4097                                       # the documented limits: d <= 4096 (>= 1024), n <= 2^20
    st, msg = run_msg(desc)
    assert st != 0 and "d = 4097" in msg and "limit" in msg, msg
    for field in ("n_x", "n_y"):
        desc = good_desc()
        setattr(desc, field, (1 << 20) + 1)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} = 1048577" in msg and "limit" in msg, msg
    for bad in (0, 9, -1):
        desc = good_desc()
        desc.n_kernels = bad
        st, msg = run_msg(desc)
        assert st != 0 and "n_kernels must be 1..8" in msg, msg
    for field in ("width", "exponent"):
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            desc = good_desc()
            getattr(desc, field)[1] = bad
            st, msg = run_msg(desc)
            assert st != 0 and f"{field}[1]" in msg and "positive" in msg, msg
    for field in ("x", "y", "out", "yy"):
        desc = good_desc()
        setattr(desc, field, BASE + (5 << 24) + 2)
        st, msg = run_msg(desc)
        assert st != 0 and "4-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace = BASE + (3 << 24) + 8
    st, msg = run_msg(desc)
    assert st != 0 and "workspace must be 16-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace_bytes -= 1
    st, msg = run_msg(desc)
    assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_workspace_bytes_and_job_reject_bad_sizes():
    lib = _lib.load()
    assert lib.hint_mmd_workspace_bytes(0, 5, 5) == 0 and "n_x must be >= 1" in lib.hint_last_error().decode()
    assert lib.hint_mmd_workspace_bytes(5, 5, 4097) == 0 and "limit" in lib.hint_last_error().decode()
    assert lib.hint_mmd_workspace_bytes(5, (1 << 20) + 1, 5) == 0 and "n_y" in lib.hint_last_error().decode()
    # two padded copies, their norms, the column sums and one double per job
    T = lib.hint_mmd_job(1, 1, 0, -1, 1)
    need = 2 * T * 16 * 4 + 2 * T * 4 + 16 * 16 * 8 + 3 * 8
    assert need <= lib.hint_mmd_workspace_bytes(1, 1, 1) <= need + 256
    assert lib.hint_mmd_workspace_bytes(4000, 4000, 100) < 8 << 20
    assert lib.hint_mmd_job(0, 5, 0, -1, 0) == -1 and "n_x" in lib.hint_last_error().decode()
    n = lib.hint_mmd_job(5, 5, 0, -1, 0)
    assert n == 3
    for j, f in ((n, 0), (-2, 0), (0, 4), (0, -1), (-1, 2)):
        assert lib.hint_mmd_job(5, 5, 0, j, f) == -1 and "no job" in lib.hint_last_error().decode()


def _sizes():
    T = _lib.load().hint_mmd_job(1, 1, 0, -1, 1)
    return T, (1, T - 1, T, T + 1, 3 * T - 3)


def test_tile_edge_is_a_multiple_of_the_mfma_tile():
    T, _ = _sizes()
    assert T >= 16 and T % 16 == 0


@pytest.mark.parametrize("with_yy", (0, 1))
def test_job_table_covers_every_tile_once_with_the_right_weights(with_yy):
    T, ns = _sizes()
    for n_x in ns:
        for n_y in ns:
            jobs, T2 = metrics.mmd_jobs(n_x, n_y, bool(with_yy))
            assert T2 == T
            ntx, nty = -(-n_x // T), -(-n_y // T)
            want = {(0, i, j) for i in range(ntx) for j in range(i, ntx)} | {(2, i, j) for i in range(ntx) for j in range(nty)}
            if not with_yy:
                want |= {(1, i, j) for i in range(nty) for j in range(i, nty)}
            assert len(jobs) == len(want), (n_x, n_y)
            assert {j[:3] for j in jobs} == want, (n_x, n_y)              # ... so each appears exactly once
            pairs = [0, 0, 0]
            for kind, ti, tj, w in jobs:
                nA, nB = (n_y if kind == 1 else n_x), (n_x if kind == 0 else n_y)
                assert w == (2 if kind != 2 and ti != tj else 1)
                pairs[kind] += w * min(T, nA - ti * T) * min(T, nB - tj * T)
            assert pairs == [n_x * n_x, 0 if with_yy else n_y * n_y, n_x * n_y], (n_x, n_y)


def test_job_decode_at_the_row_limit():
    """the triangular decode goes through a square root: its ends and seeded interior entries at 2^20 rows"""
    lib = _lib.load()
    T, _ = _sizes()
    n = 1 << 20
    nt = n // T
    tri = nt * (nt + 1) // 2
    assert lib.hint_mmd_job(n, n, 0, -1, 0) == 2 * tri + nt * nt < 2 ** 31
    assert lib.hint_mmd_job(n, n, 1, -1, 0) == tri + nt * nt
    rs = np.random.RandomState(5)
    picks = [(0, 0), (0, nt - 1), (1, 1), (nt - 2, nt - 2), (nt - 2, nt - 1), (nt - 1, nt - 1)]
    picks += [tuple(sorted(p)) for p in rs.randint(0, nt, size=(200, 2)).tolist()]
    for ti, tj in picks:
        j = ti * nt - ti * (ti - 1) // 2 + (tj - ti)
        for base, kind in ((0, 0), (tri, 1)):
            got = tuple(lib.hint_mmd_job(n, n, 0, base + j, f) for f in range(4))
            assert got == (kind, ti, tj, 1 if ti == tj else 2), (ti, tj, got)
    last = 2 * tri + nt * nt - 1
    assert tuple(lib.hint_mmd_job(n, n, 0, last, f) for f in range(4)) == (2, nt - 1, nt - 1, 1)


@pytest.mark.parametrize("case", mo.GOLDEN_CASES, ids=lambda c: c["name"])
def test_float64_evaluation_agrees_with_the_reference_outputs(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"mmd_{case['name']}.npz"))
    x, y = mo.golden_inputs(case)
    assert (int(g["seed"]), int(g["n"]), int(g["d"])) == (case["seed"], case["n"], case["d"])
    assert np.array_equal(g["kernels"], np.asarray(case["kernels"], dtype=np.float64))
    assert abs(mo.checksum([x, y]) - float(g["in_checksum"])) < 1e-6, "regenerated inputs differ from the fixture's"
    want = mo.mmd_terms64(x, y, case["kernels"])
    bound = mo.gram32_error_bound(x, y, case["kernels"])          # the recorded output is fp32 Gram arithmetic
    err = abs(want[0] - float(g["ref_mmd"]))
    print(f"{case['name']}: float64 {want[0]:.9g} reference {float(g['ref_mmd']):.9g} |difference| {err:.3g} bound {bound:.3g}")
    assert bound < 1e-4 * want[0]                                  # (the bound says something)
    assert err <= bound
    # the float64 Gram evaluation (the large GPU case's reference) is the same number
    assert abs(mo.gram_terms64(x, y, case["kernels"])[0] - want[0]) <= 1e-12


def test_closed_form_two_points():
    """x = {0}, y = {t e_1}: XX = YY = k(0), XY = k(t^2), so MMD = 2 (k(0) - k(t^2)); k(0) = sum a^a"""
    for kernels in (mo.DEFAULT, mo.OTHER, ((2.0, 3.0),)):
        k0 = sum(a ** a for C, a in kernels)
        for t in (0.0, 0.25, 3.0):
            x = np.zeros((1, 4))
            y = np.zeros((1, 4))
            y[0, 1] = t
            kt = sum(C ** a * ((C + t * t) / a) ** (-a) for C, a in kernels)
            got = mo.mmd_terms64(x, y, kernels)
            assert abs(got[0] - 2.0 * (k0 - kt)) <= 1e-14 * k0
            assert abs(got[1] - k0) <= 1e-14 * k0 and abs(got[2] - k0) <= 1e-14 * k0 and abs(got[3] - kt) <= 1e-14 * k0


def test_python_api_refuses_cpu_tensors_and_bad_kernels():
    x, y = torch.randn(6, 3), torch.randn(5, 3)
    with pytest.raises(HintAmdError, match="x is on cpu.*no CPU fallback"):
        hint_amd.multi_mmd(x, y)
    with pytest.raises(HintAmdError, match="y is on cpu.*no CPU fallback"):
        hint_amd.MultiMMD(y)
    with pytest.raises(HintAmdError, match="2-D"):
        hint_amd.multi_mmd(x[0], y)
    for bad, what in (((), "1..8"), ([(0.5, 1)] * 9, "1..8"), ([(0.0, 1)], "width of kernel 0"), ([(0.5, 1), (0.2, -1)], "exponent of kernel 1"),
                      ([(float("nan"), 1)], "width of kernel 0"), ([(0.5,)], "pairs"), (3, "pairs")):
        with pytest.raises(HintAmdError, match=what):
            hint_amd.multi_mmd(x, y, bad)
