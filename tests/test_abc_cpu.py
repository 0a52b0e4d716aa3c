"""CPU-side checks of hint_amd.nearest_rows / quantile_abc and the hint_abc_* entry points (no GPU): header, exports and binding
agree, every argument check of hint_abc_run comes before any device call and names its field, hint_abc_geometry is consistent
with itself, the Python functions refuse bad arguments by name, and the test-side float64 evaluation (tests/abc_oracle.py)
reproduces the outputs recorded from the reference's quantile_ABC exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, abc
from hint_amd._lib import HintAmdError
import abc_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_abc_workspace_bytes", "hint_abc_run", "hint_abc_geometry")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them


def good_desc(n_rows=5000, ny=3, k=100):
    lib = _lib.load()
    desc = _lib.AbcDesc()
    desc.y, desc.target, desc.idx, desc.dist, desc.workspace = (BASE + (i << 28) for i in range(5))
    desc.n_rows, desc.ny, desc.k = n_rows, ny, k
    desc.workspace_bytes = lib.hint_abc_workspace_bytes(n_rows, ny, k)
    assert desc.workspace_bytes > 0
    return desc


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_abc_run(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert set(_lib.exported_symbols()) == declared                  # the exported symbols equal the header's
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    assert "rejection_sampling.py:88-96" in header and ":188" in header
    # 2 pointers, an int64, 2 int32, 3 pointers, a size_t
    assert C.sizeof(_lib.AbcDesc) == 2 * 8 + 8 + 2 * 4 + 3 * 8 + 8 == 64
    assert _lib.AbcDesc.n_rows.offset == 16 and _lib.AbcDesc.k.offset == 28 and _lib.AbcDesc.workspace_bytes.offset == 56
    assert hint_amd.nearest_rows is abc.nearest_rows and hint_amd.quantile_abc is abc.quantile_abc
    # every caller buffer rides in the const descriptor: no entry point has a writable pointer among its parameters
    for name in NEW:
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        for p in params.split(","):
            assert "*" not in p or p.strip().startswith("const ") or p.strip() == "void* stream", (name, p)


def test_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("y", "target", "idx", "dist", "workspace"):
        desc = good_desc()
        setattr(desc, field, None)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} is null" in msg, msg
    for bad in (0, -3, (1 << 30) + 1):
        desc = good_desc()
        desc.n_rows = bad
        st, msg = run_msg(desc)
        assert st != 0 and "n_rows must be 1..1073741824" in msg and f"got {bad}" in msg, msg
    for bad in (0, -1, 33):
        desc = good_desc()
        desc.ny = bad
        st, msg = run_msg(desc)
        assert st != 0 and "ny must be 1..32" in msg and f"got {bad}" in msg, msg
    for n_rows, bad in ((5000, 0), (5000, -2), (5000, 5001), (100000, 8193)):
        desc = good_desc(n_rows)
        desc.k = bad
        st, msg = run_msg(desc)
        assert st != 0 and "k must be 1..min(n_rows, 8192)" in msg and f"got {bad}" in msg, msg
    for field in ("y", "target", "idx", "dist"):
        desc = good_desc()
        setattr(desc, field, BASE + (7 << 28) + 2)
        st, msg = run_msg(desc)
        assert st != 0 and f"{field} must be 4-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace = BASE + (4 << 28) + 8
    st, msg = run_msg(desc)
    assert st != 0 and "workspace must be 16-byte aligned" in msg, msg
    desc = good_desc()
    desc.workspace_bytes -= 1
    st, msg = run_msg(desc)
    assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_workspace_bytes_rejects_what_run_rejects_and_does_not_grow_with_n():
    lib = _lib.load()
    for args, what in (((0, 2, 1), "n_rows"), (((1 << 30) + 1, 2, 1), "n_rows"), ((10, 0, 1), "ny"), ((10, 33, 1), "ny"),
                       ((10, 2, 0), "k must"), ((10, 2, 11), "k must"), ((100000, 2, 8193), "k must")):
        assert lib.hint_abc_workspace_bytes(*args) == 0, args
        assert what in lib.hint_last_error().decode(), args
    assert lib.hint_abc_workspace_bytes(1, 1, 1) > 0
    at_1e8 = lib.hint_abc_workspace_bytes(10 ** 8, 2, 4002)
    assert 0 < at_1e8 <= 9 << 20
    assert lib.hint_abc_workspace_bytes(1 << 30, 32, 8192) <= 9 << 20          # bounded, whatever N is
    R, G = lib.hint_abc_geometry(1, 1, 1), lib.hint_abc_geometry(1 << 30, 1, 0)
    # it depends on N through the number of workgroups alone: 2^30 rows need what the smallest N on the full grid needs
    assert lib.hint_abc_workspace_bytes(1 << 30, 2, 4002) == lib.hint_abc_workspace_bytes((G - 1) * R + 1, 2, 4002) >= at_1e8


def test_geometry_is_consistent():
    lib = _lib.load()
    assert lib.hint_abc_geometry(0, 2, 0) == -1 and "n_rows" in lib.hint_last_error().decode()
    assert lib.hint_abc_geometry(10, 0, 0) == -1 and "ny" in lib.hint_last_error().decode()
    assert lib.hint_abc_geometry(10, 2, 3) == -1 and "field" in lib.hint_last_error().decode()
    assert lib.hint_abc_geometry(10, 2, -1) == -1
    R = lib.hint_abc_geometry(1, 1, 1)
    G = lib.hint_abc_geometry(1 << 30, 1, 0)
    passes = lib.hint_abc_geometry(1, 1, 2)
    assert R >= 256 and G >= 256 and passes >= 2
    full = (G - 1) * R + 1
    for N in (1, 2, R - 1, R, R + 1, 3 * R + 17, full - 1, full, full + 1, G * R, G * R + 1, 10 ** 8, (1 << 30) - 1, 1 << 30):
        for ny in (1, 2, 32):
            g, r, p = (lib.hint_abc_geometry(N, ny, f) for f in range(3))
            assert p == passes
            assert 1 <= g <= G and r >= R
            assert g * r >= N > (g - 1) * r, (N, g, r)        # contiguous ranges [w r, min(N, (w + 1) r)), none of them empty
    assert lib.hint_abc_geometry(full - 1, 2, 0) == G - 1 and lib.hint_abc_geometry(full, 2, 0) == G


def test_python_argument_errors():
    y, t = torch.randn(50, 3), torch.randn(3)
    with pytest.raises(HintAmdError, match="nearest_rows: y is on cpu.*no CPU fallback"):
        hint_amd.nearest_rows(y, t, 5)
    with pytest.raises(HintAmdError, match="quantile_abc: y is on cpu.*no CPU fallback"):
        hint_amd.quantile_abc(torch.randn(50, 2), y, t, n=5)
    with pytest.raises(HintAmdError, match="y must be a tensor"):
        hint_amd.nearest_rows(y.numpy(), t, 5)
    with pytest.raises(HintAmdError, match="y must be 2-D"):
        hint_amd.nearest_rows(y[0], t, 5)
    # the remaining checks sit behind the device check; a meta tensor says is_cuda = False too, so they are reached through the
    # helpers the public functions call
    fake = torch.empty(50, 3)
    with pytest.raises(HintAmdError, match=r"target must have shape \[3\] or \[1, 3\]"):
        abc._check_target(torch.randn(4), fake, "nearest_rows", "target")
    with pytest.raises(HintAmdError, match=r"y_target must have shape"):
        abc._check_target(torch.randn(2, 3), fake, "quantile_abc", "y_target")
    with pytest.raises(HintAmdError, match="target must be a tensor or an array-like"):
        abc._check_target(object(), fake, "nearest_rows", "target")
    assert abc._check_target([[1, 2, 3]], fake, "nearest_rows", "target").shape == (3,)
    assert abc._check_target(np.ones((1, 3)), fake, "nearest_rows", "target").dtype == torch.float32
    for bad, what in ((0, "k must be >= 1"), (-1, "k must be >= 1"), (2.5, "k must be an int"), (True, "k must be an int")):
        with pytest.raises(HintAmdError, match=what):
            abc._check_count(bad, "nearest_rows", "k", 1)
    with pytest.raises(HintAmdError, match="skip must be >= 0"):
        abc._check_count(-1, "quantile_abc", "skip", 0)


@pytest.mark.parametrize("case", ao.GOLDEN_CASES, ids=lambda c: c["name"])
def test_float64_order_reproduces_the_reference_outputs_exactly(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"abc_{case['name']}.npz"))
    x, y, t = ao.golden_inputs(case)
    n = case["n"]
    assert (int(g["seed"]), int(g["N"]), int(g["ny"]), int(g["n"])) == (case["seed"], case["N"], case["ny"], n)
    assert abs(ao.checksum([x, y, t]) - float(g["in_checksum"])) < 1e-6, "regenerated inputs differ from the fixture's"
    assert np.array_equal(x[:, -1], np.arange(case["N"], dtype=np.float32))
    D, order = ao.order64(y, t)
    assert np.unique(D).size == D.size                                   # no exact ties: the reference's order among them is unspecified
    assert np.array_equal(order[1:n + 1], g["ref_rows"].astype(np.int64))        # np.argsort(d)[1:][:n]
    assert float(np.sqrt(D[order[n + 1]])) == float(g["ref_threshold"])           # d[sort[n]]
    assert ao.band_count(D, order, n + 2, case["ny"]) == 0


def test_random_cases_satisfy_the_band_condition():
    """the GPU tests' comparison rule needs at most 1 % of k rows within eps of rank k - 1: it depends on the inputs alone"""
    lib = _lib.load()
    R, G = lib.hint_abc_geometry(1, 1, 1), lib.hint_abc_geometry(1 << 30, 1, 0)
    cases = ao.random_cases(R, G)
    assert {c[1] for c in cases} == {1, 2, 3, 4, 5, 7, 32}
    orders = {}
    for N, ny, k, seed in cases:
        assert 1 <= k <= min(N, 8192)
        y, t = ao.random_inputs(N, ny, seed)
        D, order = ao.order64(y, t)
        band = ao.band_count(D, order, k, ny)
        assert band <= 0.01 * k, (N, ny, k, seed, band)
        orders[(N, ny, k)] = band
    assert len(orders) == len(cases)
