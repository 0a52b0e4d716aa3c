"""CPU-side checks of hint_amd.sample_plus_* / plus_outlines / plus_draws and the hint_plusgen_* entry points (no GPU): header,
exports and binding agree with the ABI still 8, every argument check comes before any device call and names its field, the
workspace is monotone and under its stated bound, and the test-side definition (tests/plusgen_oracle.py) agrees with the
reference's recorded outputs, with tests/noise_oracle.py's Philox, with a second construction of the ring, with the stated
pattern shares and point counts, and with its own fp32 evaluation inside the derived bounds; every wrong variant is rejected by
the rule, and the seeds of the GPU tests leave out no more rows than the cap."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, plusgen
from hint_amd._lib import HintAmdError
from fake_device import OnGpu
import noise_oracle as no
import plusgen_oracle as po
from plusgen_cases import (CONDITIONAL, HIGH, N_BIG, SEED, SHARES, TARGETS, corner_case_draws, pattern_draws, sweep_arms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("hint_plusgen_workspace_bytes", "hint_plusgen_run")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
MAX_N, WS_BOUND = 1 << 30, 32 << 10
FIELDS = ("n_rows", "seed", "offset", "rows", "draws", "target", "x", "y", "outline", "counts", "corners", "draws_out", "workspace",
          "workspace_bytes", "max_groups", "stream")


def plus_desc(n=1000):
    lib = _lib.load()
    d = _lib.PlusGenDesc()
    d.n_rows, d.seed, d.offset = n, 7, 0
    d.x, d.y, d.outline, d.counts, d.corners, d.draws_out, d.workspace = (BASE + (i << 28) for i in range(7))
    d.workspace_bytes = lib.hint_plusgen_workspace_bytes(n)
    assert d.workspace_bytes > 0
    return d


def run_msg(desc):
    lib = _lib.load()
    st = lib.hint_plusgen_run(C.byref(desc) if desc is not None else None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    for cite in ("data.py:176-252", "data.py:190-202", "data.py:195-200", "best_shape_fit.py:28-29", "data.py:176-186", "data.py:211-222",
                 "rejection_sampling.py:113-127", "rejection_sampling.py:76-85", "data.py:466-489"):
        assert cite in header, cite
    assert header.count("THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION") == 2
    assert "EQUALITY (measure zero) IS \"ARM ABSENT\"" in header and "THE STREAM IS A\n *                    FIELD OF THE DESCRIPTOR" in header
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    assert re.search(r"int hint_plusgen_run\(const hint_plusgen_desc\* desc\);", header)      # the stream is not a parameter
    P = _lib.PlusGenDesc
    assert C.sizeof(P) == 128
    assert [getattr(P, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120]
    body = re.search(r"typedef struct hint_plusgen_desc \{(.*?)\} hint_plusgen_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f for f, _ in P._fields_] == list(FIELDS), names
    for name in plusgen.__all__:
        assert getattr(hint_amd, name) is getattr(plusgen, name)
    assert set(plusgen.__all__) == {"sample_plus_prior", "sample_plus_joint", "sample_plus_targeted", "sample_plus_conditional",
                                    "plus_outlines", "plus_draws"}


def test_plusgen_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg(None)
    assert st != 0 and "desc is null" in msg, msg
    d = plus_desc()
    d.x = d.y = None
    st, msg = run_msg(d)
    assert st != 0 and "x and y are both null" in msg, msg
    d = plus_desc()
    d.workspace = None
    st, msg = run_msg(d)
    assert st != 0 and "workspace is null" in msg, msg
    for bad in (0, -3, MAX_N + 1):
        d = plus_desc()
        d.n_rows = bad
        st, msg = run_msg(d)
        assert st != 0 and "n_rows must be 1.." in msg and str(bad) in msg, msg
    d = plus_desc()
    d.offset = 2 ** 64 - 1000
    st, msg = run_msg(d)
    assert st != 0 and "offset + n_rows" in msg, msg
    d = plus_desc()
    d.rows, d.draws = BASE + (8 << 28), BASE + (9 << 28)
    st, msg = run_msg(d)
    assert st != 0 and "rows and draws are both given" in msg, msg
    d = plus_desc()
    d.max_groups = -1
    st, msg = run_msg(d)
    assert st != 0 and "max_groups must be >= 0" in msg, msg
    for i, bad in ((0, float("nan")), (1, float("inf")), (2, float("-inf")), (3, float("nan"))):
        d = plus_desc()
        t = [0.1, 0.2, 0.3, 1.0]
        t[i] = bad
        d.target = (C.c_float * 4)(*t)
        st, msg = run_msg(d)
        assert st != 0 and f"target[{i}] is not finite" in msg, msg
    for bad in (0.2499, 4.001, -1.0, 0.0):
        d = plus_desc()
        d.target = (C.c_float * 4)(0.1, 0.2, 0.3, bad)
        st, msg = run_msg(d)
        assert st != 0 and "target[3], the ratio, must be 0.25..4" in msg, msg
    for field, align in (("rows", 8), ("draws", 4), ("x", 16), ("y", 16), ("outline", 8), ("counts", 4), ("corners", 4), ("draws_out", 4),
                         ("workspace", 16)):
        d = plus_desc()
        setattr(d, field, BASE + (9 << 28) + align // 2)
        st, msg = run_msg(d)
        assert st != 0 and f"{field} must be {align}-byte aligned" in msg, msg
    for n in (1000, MAX_N):                                  # at the limit itself only the workspace size is left to refuse
        d = plus_desc(n)
        d.workspace_bytes -= 1
        st, msg = run_msg(d)
        assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_workspace_is_monotone_and_under_its_stated_bound():
    lib = _lib.load()
    for bad in (0, -1, MAX_N + 1):
        assert lib.hint_plusgen_workspace_bytes(bad) == 0 and "n_rows must be" in lib.hint_last_error().decode()
    ns = [1, 2, 4, 5, 15, 16, 17, 63, 64, 65, 4099, 32767, 32768, 32769, 10 ** 5, 10 ** 7, 10 ** 8, MAX_N]
    sizes = [lib.hint_plusgen_workspace_bytes(n) for n in ns]
    assert sizes[0] == 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == WS_BOUND
    assert all(s % 16 == 0 for s in sizes)


def test_python_wrappers_reject_bad_arguments_without_a_gpu():
    cpu = torch.zeros(5, 9)
    t = (0.1, 0.2, 0.3, 1.5)
    bad_calls = [
        (lambda: hint_amd.sample_plus_prior(0, 1), "n must be 1.."),
        (lambda: hint_amd.sample_plus_prior(2.0, 1), "n must be an int"),
        (lambda: hint_amd.sample_plus_prior(True, 1), "n must be an int"),
        (lambda: hint_amd.sample_plus_prior((1 << 30) + 1, 1), "n must be 1.."),
        (lambda: hint_amd.sample_plus_prior(5, -1), "seed must be 0.."),
        (lambda: hint_amd.sample_plus_prior(5, 2 ** 64), "seed must be 0.."),
        (lambda: hint_amd.sample_plus_prior(5, 1, offset=2 ** 64 - 3), "offset must be 0.."),
        (lambda: hint_amd.sample_plus_prior(5, 1, device="cpu"), "no CPU fallback"),
        (lambda: hint_amd.sample_plus_prior(5, 1, device=3.5), "device must name a device"),
        (lambda: hint_amd.sample_plus_prior(5, 1, draws=[1.0]), "draws must be a tensor"),
        (lambda: hint_amd.sample_plus_prior(5, 1, draws=torch.zeros(5, 4)), "draws must be [1.."),
        (lambda: hint_amd.sample_plus_prior(6, 1, draws=cpu), "draws holds 5 rows and n is 6"),
        (lambda: hint_amd.sample_plus_prior(5, 1, draws=cpu), "draws is on cpu"),
        (lambda: hint_amd.sample_plus_joint(0, 1), "sample_plus_joint: n must be 1.."),
        (lambda: hint_amd.plus_draws(5, 1.5), "plus_draws: seed must be an int"),
        (lambda: hint_amd.plus_outlines(cpu), "plus_outlines: draws is on cpu"),
        (lambda: hint_amd.plus_outlines(torch.zeros(5, 9, dtype=torch.int32)), "draws must be [1.."[:5]),
        (lambda: hint_amd.plus_outlines(cpu, target=(1, 2, 3)), "target must be 4 numbers"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, None), "target must be 4 numbers"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, 3.0), "target must be 4 numbers"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, (0.0, 0.0, 0.0, 0.2)), "the ratio, must be 0.25..4"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, (0.0, 0.0, 0.0, 4.5)), "the ratio, must be 0.25..4"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, (0.0, float("nan"), 0.0, 1.0)), "target[1] must be finite"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, (0.0, 0.0, 1e39, 1.0)), "finite in fp32"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, ("a", 0, 0, 1)), "target must be 4 numbers"),
        (lambda: hint_amd.sample_plus_targeted(5, 1, t, device="cpu"), "no CPU fallback"),
        (lambda: hint_amd.sample_plus_conditional(t, 0, 1), "n must be 1.."),
        (lambda: hint_amd.sample_plus_conditional(t, 5, 1, radius=-0.1), "radius must be >= 0"),
        (lambda: hint_amd.sample_plus_conditional(t, 5, 1, radius=float("nan")), "radius must be finite"),
        (lambda: hint_amd.sample_plus_conditional(t, 5, 1, chunk=0), "chunk must be 1.."),
        (lambda: hint_amd.sample_plus_conditional(t, 5, 1, max_rows=0), "max_rows must be 1.."),
        (lambda: hint_amd.sample_plus_conditional(None, 5, 1), "target must be 4 numbers"),
        (lambda: hint_amd.sample_plus_conditional(t, 5, 1, device="cpu"), "no CPU fallback"),
    ]
    for call, text in bad_calls:
        with pytest.raises(HintAmdError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))
    g = torch.zeros(5, 9, requires_grad=True)
    with pytest.raises(HintAmdError):
        hint_amd.plus_outlines(g)


def test_the_sampler_argument_checks_word_every_refusal_as_recorded():
    """every branch of the draws / sampling-argument checks the samplers share, through this module's wrappers, the whole text"""
    who, shape = "sample_plus_prior", "[1..1073741824, 9] = (u_xl, u_yl, u_xw, u_yw, u_xs, u_ys, u_a, n_x, n_y)"
    ok = torch.zeros(10, 9)
    fallback = "the sampler is a GPU kernel and there is no CPU fallback"
    no_grad = "requires grad, and no gradient is implemented; call it under torch.no_grad() or detach the input"
    bad_calls = [
        (lambda: hint_amd.sample_plus_prior(0, 1), f"{who}: n must be 1..1073741824 (got 0)"),
        (lambda: hint_amd.sample_plus_prior((1 << 30) + 1, 1), f"{who}: n must be 1..1073741824 (got 1073741825)"),
        (lambda: hint_amd.sample_plus_prior(2.0, 1), f"{who}: n must be an int (got float)"),
        (lambda: hint_amd.sample_plus_prior(True, 1), f"{who}: n must be an int (got bool)"),
        (lambda: hint_amd.sample_plus_prior(10, -1), f"{who}: seed must be 0..18446744073709551615 (got -1)"),
        (lambda: hint_amd.sample_plus_prior(10, 2 ** 64), f"{who}: seed must be 0..18446744073709551615 (got 18446744073709551616)"),
        (lambda: hint_amd.sample_plus_prior(10, "1"), f"{who}: seed must be an int (got str)"),
        (lambda: hint_amd.sample_plus_prior(10, 1, offset=2 ** 64 - 5),
         f"{who}: offset must be 0..18446744073709551605 (got 18446744073709551611)"),
        (lambda: hint_amd.sample_plus_prior(10, 1, offset=-1), f"{who}: offset must be 0..18446744073709551605 (got -1)"),
        (lambda: hint_amd.sample_plus_prior(10, 1, device="cpu"), f"{who}: device is cpu; {fallback}"),
        (lambda: hint_amd.sample_plus_prior(10, 1, device=3.5), f"{who}: device must name a device (got 3.5)"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=[[0.5] * 9] * 10), f"{who}: draws must be a tensor (got list)"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=torch.zeros(10, 4)), f"{who}: draws must be {shape} (got shape (10, 4))"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=torch.zeros(10)), f"{who}: draws must be {shape} (got shape (10,))"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=torch.zeros(0, 9)), f"{who}: draws must be {shape} (got shape (0, 9))"),
        (lambda: hint_amd.sample_plus_prior(9, 1, draws=ok), f"{who}: draws holds 10 rows and n is 9"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=ok), f"{who}: draws is on cpu; {fallback}"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=OnGpu(ok.to(torch.int32))),
         f"{who}: draws is torch.int32; expected a floating-point tensor"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=OnGpu(ok.clone().requires_grad_(True))), f"{who}: draws {no_grad}"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=OnGpu(ok), device="cuda:0"), f"{who}: draws is on cuda:1 and device is cuda:0"),
        (lambda: hint_amd.sample_plus_prior(10, 1, draws=OnGpu(ok), device="cpu"), f"{who}: device is cpu; {fallback}"),
        (lambda: hint_amd.sample_plus_joint(0, 1), "sample_plus_joint: n must be 1..1073741824 (got 0)"),
        (lambda: hint_amd.sample_plus_joint(10, 1, draws=torch.zeros(10, 4)), f"sample_plus_joint: draws must be {shape} (got shape (10, 4))"),
        (lambda: hint_amd.plus_draws(10, 1, offset=2 ** 64 - 5),
         "plus_draws: offset must be 0..18446744073709551605 (got 18446744073709551611)"),
        (lambda: hint_amd.plus_outlines(0.5), "plus_outlines: draws must be a tensor (got float)"),
        (lambda: hint_amd.plus_outlines(torch.zeros(3, 4)), f"plus_outlines: draws must be {shape} (got shape (3, 4))"),
        (lambda: hint_amd.plus_outlines(torch.zeros(3, 9)), f"plus_outlines: draws is on cpu; {fallback}"),
        (lambda: hint_amd.plus_outlines(OnGpu(torch.zeros(3, 9, dtype=torch.int64))),
         "plus_outlines: draws is torch.int64; expected a floating-point tensor"),
        (lambda: hint_amd.plus_outlines(OnGpu(torch.zeros(3, 9, requires_grad=True))), f"plus_outlines: draws {no_grad}"),
        (lambda: hint_amd.sample_plus_targeted(10, 1, (0.0, 0.0, 0.3, 1.5), draws=torch.zeros(10, 4)),
         f"sample_plus_targeted: draws must be {shape} (got shape (10, 4))"),
        (lambda: hint_amd.sample_plus_targeted(9, 1, (0.0, 0.0, 0.3, 1.5), draws=ok), "sample_plus_targeted: draws holds 10 rows and n is 9"),
    ]
    for call, text in bad_calls:
        with pytest.raises(HintAmdError) as e:
            call()
        assert str(e.value) == text, (text, str(e.value))
    with torch.no_grad():                                   # (no gradient is asked for: the check after it refuses the call)
        with pytest.raises(HintAmdError) as e:
            hint_amd.sample_plus_prior(10, 1, draws=OnGpu(ok.clone().requires_grad_(True)), device="cuda:0")
    assert str(e.value) == f"{who}: draws is on cuda:1 and device is cuda:0"


def test_draws_are_noise_oracles_philox_chunked_gathered_and_across_the_carry():
    s = np.float32(2.0 ** -32)
    for off in (0, 12345, HIGH):
        n = 40
        d = po.draws(SEED, off, n)
        rows = np.arange(n, dtype=np.uint64) + np.uint64(off)
        for stream, cols in ((0, (0, 1, 2, 3)), (1, (4, 5, 6))):
            c = no.philox4x32_10((rows & no.MASK, rows >> np.uint64(32), stream, 0x504C5553), (SEED & 0xFFFFFFFF, SEED >> 32))
            for w, col in zip(c, cols):
                assert (d[:, col] == (w.astype(np.float32) * s).astype(np.float64)).all(), (off, stream, col)
        c = no.philox4x32_10((rows & no.MASK, rows >> np.uint64(32), 2, 0x504C5553), (SEED & 0xFFFFFFFF, SEED >> 32))
        u0 = np.minimum((c[0].astype(np.float32) + np.float32(1)) * s, np.float32(1)).astype(np.float64)
        u1 = (c[1].astype(np.float32) * s).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u0))
        assert np.allclose(d[:, 7], r * np.cos(2 * np.pi * u1), rtol=0, atol=1e-15) and np.allclose(d[:, 8], r * np.sin(2 * np.pi * u1), rtol=0, atol=1e-15)
        assert (d[:, :7] >= 0).all() and (d[:, :7] <= 1).all()
        # chunks at any boundaries, and a gather, are the contiguous call
        parts = np.concatenate([po.draws(SEED, off + a, b - a) for a, b in ((0, 1), (1, 7), (7, 40))])
        assert (parts == d).all()
        pick = np.array([39, 0, 5, 5, 17])
        assert (po.draws(SEED, 0, len(pick), rows=rows[pick]) == d[pick]).all()
    hi = po.draws(SEED, HIGH, 10)
    assert (hi[5:] == po.draws(SEED, 2 ** 32, 5)).all() and (hi[:5] != po.draws(SEED, 0, 5)).any()    # the carry into the high word
    assert (po.draws(SEED, 0, 10) != po.draws(SEED + 1, 0, 10)).all(axis=1).any()


def test_the_two_ring_constructions_agree_and_the_patterns_have_their_shares():
    d = po.draws(77, 0, 120000).astype(np.float32)
    c = po.local_coords(d)
    V1, n1 = po.ring_sorted(c)
    V2, n2 = po.ring_table(c)
    assert (n1 == n2).all() and np.array_equal(np.nan_to_num(V1, nan=-99.0), np.nan_to_num(V2, nan=-99.0))
    m = po.arms(c)
    assert ((n1 == 12) == (m == 15)).all() and set(np.unique(n1).tolist()) == {8, 12}
    m = sweep_arms()
    assert sorted(np.unique(m).tolist()) == sorted(SHARES)
    for mask, share in SHARES.items():
        got = float((m == mask).mean())
        se = np.sqrt(share * (1 - share) / len(m))
        assert abs(got - share) <= 5 * se + 0.0005, (mask, got, share)      # (the table's shares are rounded to their last digit)
    # the ring is closed, axis-aligned, clockwise (negative shoelace area), free of duplicates and of collinear vertices, and for
    # the full plus it is the vertex order of plus_segments_from_params
    V, nc = V2[:5000], n2[:5000]
    for i in range(len(V)):
        r = V[i, :nc[i]]
        e = np.roll(r, -1, axis=0) - r
        assert ((e[:, 0] == 0) != (e[:, 1] == 0)).all()
        assert ((e[:, 0] == 0) != (np.roll(e, -1, axis=0)[:, 0] == 0)).all()                 # edges alternate: nothing collinear
        assert 0.5 * np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]) < 0
        assert r[0, 0] < 0 and r[0, 1] > 0                                                   # the first corner is in the upper left
    full = np.nonzero(po.arms(c) == 15)[0][:100]
    vx, vy = 0x011223322110, 0x667766445544                                                  # hint_plusgeom.hpp PL_VX / PL_VY
    for s in range(12):
        assert (V2[full, s, 0] == c[full, (vx >> (4 * s)) & 15]).all() and (V2[full, s, 1] == c[full, (vy >> (4 * s)) & 15]).all()
    d, masks = pattern_draws()
    assert (po.arms(po.local_coords(d)) == masks).all() and len(set(masks.tolist())) == 9


def test_point_counts_stay_inside_their_range_and_the_storage():
    """N = the sum of the counts: between 54 and 106 by the perimeter's bounds - the union is orthogonally convex, so its perimeter
    is its bounding box's, between 2 (3 + 3) = 12 and 2 (5 + 5) = 20, that is 60 to 100 steps of 0.2, and each of at most 12 edges
    rounds by at most half a point - and 128 are stored"""
    d = po.draws(78, 0, 60000).astype(np.float32)
    c = po.local_coords(d)
    V, nc = po.ring_table(c)
    N = po.edge_counts(V, nc)[0].sum(axis=1)
    print(f"N over 60000 prior rows: {N.min()}..{N.max()}, {len(np.unique(N))} values")
    assert po.N_RANGE[0] <= N.min() and N.max() <= po.N_RANGE[1] < po.POINTS and len(np.unique(N)) >= 40
    d = corner_case_draws()
    w = po.sample(d)
    assert po.N_RANGE[0] <= w["counts"].min() and w["counts"].max() <= po.N_RANGE[1], (w["counts"].min(), w["counts"].max())
    assert (w["counts"] != po.sample(d, variant="half_up")["counts"]).any()
    for t in TARGETS:
        Nt = po.sample(po.draws(79, 0, 3000).astype(np.float32), t)["counts"]
        assert po.N_RANGE[0] <= Nt.min() and Nt.max() <= po.N_RANGE[1], (t, Nt.min(), Nt.max())


def test_the_oracle_reproduces_the_references_recorded_outputs():
    f = np.load(os.path.join(GOLDEN, "plusgen_rings.npz"))
    d, V, nc = f["draws"], f["rings"], f["corners"]
    assert sorted(set(f["arms"].tolist())) == [5, 6, 7, 9, 10, 11, 13, 14, 15]
    c = po.local_coords(d)
    for ring in (po.ring_sorted(c), po.ring_table(c)):
        assert (ring[1] == nc).all() and np.array_equal(np.nan_to_num(ring[0], nan=-99.0), np.nan_to_num(V, nan=-99.0))
    dense, N = po.densify(V, nc)
    assert (N == f["counts"]).all()
    assert np.abs(dense - f["dense"]).max() <= 4 * 2.0 ** -52 * 4          # float64 rounding of values below 4
    assert np.abs(po.coeffs(f["dense"], f["counts"]) - f["ref25"]).max() <= 1e-13
    assert f["counts"][-1] != po.densify(V[-1:], nc[-1:], half_up=True)[1][0]       # the reference rounds half to even


def test_fp32_floor_lies_inside_the_derived_bounds():
    d = po.draws(SEED, 0, N_BIG).astype(np.float32)
    res, rows = po.fp32_floor(d)
    print(f"fp32 floor over {rows} rows, error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert po.passes(res) and rows >= 0.99 * N_BIG
    assert res["outline"] >= 0.002                             # ... and is a floor: the bounds are not vacuous by orders of magnitude
    for t in TARGETS:
        res, rows = po.fp32_floor(d[:1027], t)
        assert po.passes(res) and rows >= 0.99 * 1027, (t, res)
    assert po.K_POINT == 236 and po.K_Y == 185 and po.k_coef(100) == 338


def test_every_wrong_variant_is_rejected_by_the_rule():
    d = np.concatenate([po.draws(SEED, 0, 300).astype(np.float32), pattern_draws()[0]])
    keep = ~po.ambiguous(d)
    w = po.sample(d)
    assert po.passes(po.compare(po.sample(d), w, keep))
    for v in po.WRONG:
        if v == "half_up":
            continue
        res = po.compare(po.sample(d, variant=v), w, keep)
        assert not po.passes(res), (v, res)
    # half-up rounding shows only at an exact half-integer, which the dyadic corner cases have (every row is compared there)
    d = corner_case_draws()
    w = po.sample(d)
    assert po.passes(po.compare(po.sample(d), w))
    res = po.compare(po.sample(d, variant="half_up"), w)
    assert res["counts"] > 0 and not po.passes(res), res
    for t in TARGETS:
        dt = po.draws(SEED, 0, 200).astype(np.float32)
        wt = po.sample(dt, t)
        assert not po.passes(po.compare(po.sample(dt, t, variant="r_transposed"), wt, ~po.ambiguous(dt, t), t)) or t[2] == 0.0


def test_the_gpu_tests_seeds_leave_out_no_more_rows_than_the_cap():
    shares = {}
    for n, off in ((N_BIG, 0), (10, HIGH)):
        shares[f"philox {off}"] = float(po.ambiguous(po.draws(SEED, off, n).astype(np.float32)).mean())
    for t in TARGETS:
        shares[f"target {t}"] = float(po.ambiguous(po.draws(SEED, 0, 1027).astype(np.float32), t).mean())
    shares["patterns"] = float(po.ambiguous(pattern_draws()[0]).mean())
    print(shares)
    assert all(v <= po.MAX_AMBIGUOUS for v in shares.values()), shares
    arm, half = po.slacks(po.draws(SEED + 3, 0, 100000).astype(np.float32))
    print(f"of 1e5 rows: {float((arm < 1e-4).mean()):.1e} within 1e-4 of a vanishing arm, {float((half < 1e-4).mean()):.1e} of a half-integer")
    assert float(((arm < po.ARM_MARGIN) | (half < po.HALF_MARGIN)).mean()) <= po.MAX_AMBIGUOUS / 10
    # the conditional test: the oracle's own selection, no candidate near the boundary, none of the selected rows ambiguous
    target, radius, n, seed, m = CONDITIONAL
    dd = po.draws(seed, 0, m)
    idx, tried, d2 = po.select(po.sample(dd, target)["y"], target, radius, n)
    assert idx is not None and len(idx) == n and tried <= m
    assert np.abs(np.sqrt(d2[:tried].astype(np.float64)) - radius).min() > 1e-4
    assert not po.ambiguous(dd[idx].astype(np.float32), target).any()
    assert po.select(po.sample(dd[:50], target)["y"], target, radius, n)[0] is None


def test_the_target_formulas_and_the_label():
    d = po.draws(5, 0, 2000).astype(np.float32)
    for t in TARGETS + ((0.0, 0.0, 0.3, 0.9999999), (0.0, 0.0, 0.3, 1.0000001)):
        r = float(np.float32(t[3]))
        xl, yl, xw, yw, xs, ys, ang = po.params(d, t)
        want = 0.5 * r + (2 - 0.5 * r) * d[:, 2].astype(np.float64) if r >= 1 else 0.5 + (2 * r - 0.5) * d[:, 2].astype(np.float64)
        assert np.array_equal(xw, want) and np.array_equal(yw, xw / r)
        assert xw.min() >= 0.5 and xw.max() <= 2.0 and yw.min() >= 0.5 - 1e-12 and yw.max() <= 2.0 + 1e-12       # widths stay in [0.5, 2]
        assert (ang == float(np.float32(t[2]))).all()
        w = po.sample(d, t)
        assert (w["y"][:, 2] == float(np.float32(t[2]))).all()
        assert np.abs(w["y"][:, 3] - r).max() <= 4 * 2.0 ** -52 * r            # within rounding of the ratio
        assert set(np.unique(w["corners"]).tolist()) <= {8, 12} and len(np.unique(w["arms"])) <= 9
        g = po.sample(d, t, np.float32, mask=w["arms"].astype(np.int64))
        assert np.abs(g["y"][:, 3].astype(np.float64) - r).max() <= po.K_RATIO * po.U * r
    for r, (lo, hi) in ((0.25, (0.5, 0.5)), (1.0, (0.5, 2.0)), (4.0, (2.0, 2.0))):
        xw = po.params(np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0, 0]], dtype=np.float32), (0, 0, 0, r))[2]
        assert (xw[0], xw[1]) == (lo, hi)
    w = po.sample(d)                                           # the prior: y[:, 2] is the angle, y[:, 3] the ratio of the widths
    xl, yl, xw, yw, xs, ys, ang = po.params(d)
    assert np.array_equal(w["y"][:, 2], ang) and np.array_equal(w["y"][:, 3], xw / yw) and ang.max() <= np.pi / 2
    # center is where the bars' common origin lands: inside the figure's bounding box
    lo, hi = w["outline"].min(axis=1, initial=np.inf, where=w["outline"] != 0), w["outline"].max(axis=1, initial=-np.inf, where=w["outline"] != 0)
    assert (w["y"][:, :2] >= lo).all() and (w["y"][:, :2] <= hi).all()
