"""CPU-side checks of hint_amd.sample_lens_prior / sample_lens_joint / lens_rings / fourier_coeffs and the hint_lensgen_* /
hint_fcoef_* entry points (no GPU): header, exports and binding agree, every argument check comes before any device call and
names its field, the workspaces are monotone and under their stated bounds, and the test-side definition
(tests/shapegen_oracle.py) agrees with the reference's recorded outputs, with tests/noise_oracle.py's Philox, with closed forms,
with a second construction of the ring, and with its own fp32 evaluation inside the derived bounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, shapes
from hint_amd._lib import HintAmdError
from fake_device import OnGpu
import noise_oracle as no
import shapegen_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("hint_lensgen_workspace_bytes", "hint_lensgen_run", "hint_fcoef_workspace_bytes", "hint_fcoef_run")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
LENS_MAX_N, FCOEF_MAX_N, MAX_P, MAX_K = 1 << 30, 1 << 24, 1024, 25
LENS_WS_BOUND, FCOEF_WS_BOUND = 32 << 10, 128 << 10      # what include/hint_amd.h states


def lens_desc(n=1000):
    lib = _lib.load()
    d = _lib.LensGenDesc()
    d.n_rows, d.seed, d.offset = n, 7, 0
    d.draws, d.x, d.ring, d.counts, d.eps, d.draws_out, d.workspace = (BASE + (i << 28) for i in range(7))
    d.workspace_bytes = lib.hint_lensgen_workspace_bytes(n)
    assert d.workspace_bytes > 0
    return d


def fcoef_desc(n=100, p=64, k=5):
    lib = _lib.load()
    d = _lib.FcoefDesc()
    d.points, d.counts, d.x, d.workspace = (BASE + (i << 28) for i in range(4))
    d.n_rows, d.p_max, d.n_coeffs = n, p, k
    d.workspace_bytes = lib.hint_fcoef_workspace_bytes(n, p, k)
    assert d.workspace_bytes > 0
    return d


def run_msg(entry, desc):
    lib = _lib.load()
    st = getattr(lib, entry)(C.byref(desc) if desc is not None else None, None)
    return st, (lib.hint_last_error() or b"").decode()


def test_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    for cite in ("data.py:85-125", "rejection_sampling.py:76-85", "data.py:466-489", "data.py:42-49"):
        assert cite in header, cite
    assert "THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION" in header
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    L, F = _lib.LensGenDesc, _lib.FcoefDesc
    assert C.sizeof(L) == 96 and C.sizeof(F) == 64
    assert [getattr(L, f).offset for f in ("n_rows", "seed", "offset", "draws", "x", "ring", "counts", "eps", "draws_out", "workspace",
                                           "workspace_bytes", "max_groups")] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88]
    assert [getattr(F, f).offset for f in ("points", "counts", "n_rows", "p_max", "n_coeffs", "x", "workspace", "workspace_bytes",
                                           "max_groups")] == [0, 8, 16, 24, 28, 32, 40, 48, 56]
    # the header's structs, field by field in the binding's order
    for struct, cls in (("hint_lensgen_desc", L), ("hint_fcoef_desc", F)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], (struct, names)
    for name in ("sample_lens_prior", "sample_lens_joint", "lens_rings", "lens_draws", "fourier_coeffs"):
        assert getattr(hint_amd, name) is getattr(shapes, name)


def test_lensgen_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg("hint_lensgen_run", None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("x", "workspace"):
        d = lens_desc()
        setattr(d, field, None)
        st, msg = run_msg("hint_lensgen_run", d)
        assert st != 0 and f"{field} is null" in msg, msg
    for bad in (0, -3, LENS_MAX_N + 1):
        d = lens_desc()
        d.n_rows = bad
        st, msg = run_msg("hint_lensgen_run", d)
        assert st != 0 and "n_rows must be 1.." in msg and str(bad) in msg, msg
    d = lens_desc()
    d.offset = 2 ** 64 - 1000
    st, msg = run_msg("hint_lensgen_run", d)
    assert st != 0 and "offset + n_rows" in msg, msg
    d = lens_desc()
    d.max_groups = -1
    st, msg = run_msg("hint_lensgen_run", d)
    assert st != 0 and "max_groups must be >= 0" in msg, msg
    for field, align in (("draws", 16), ("x", 16), ("ring", 8), ("counts", 4), ("eps", 8), ("draws_out", 16), ("workspace", 16)):
        d = lens_desc()
        setattr(d, field, BASE + (9 << 28) + align // 2)
        st, msg = run_msg("hint_lensgen_run", d)
        assert st != 0 and f"{field} must be {align}-byte aligned" in msg, msg
    for n in (1000, LENS_MAX_N):                             # at the limit itself only the workspace size is left to refuse
        d = lens_desc(n)
        d.workspace_bytes -= 1
        st, msg = run_msg("hint_lensgen_run", d)
        assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_fcoef_run_rejects_bad_arguments_before_any_device_call():
    st, msg = run_msg("hint_fcoef_run", None)
    assert st != 0 and "desc is null" in msg, msg
    for field in ("points", "x", "workspace"):
        d = fcoef_desc()
        setattr(d, field, None)
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and f"{field} is null" in msg, msg
    for bad in (0, -1, FCOEF_MAX_N + 1):
        d = fcoef_desc()
        d.n_rows = bad
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and "n_rows must be 1.." in msg, msg
    for bad in (0, -5, 4, 26, 27):
        d = fcoef_desc()
        d.n_coeffs = bad
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and "n_coeffs must be odd" in msg, msg
    for k, bad in ((5, 4), (25, 24), (5, MAX_P + 1), (5, 0)):
        d = fcoef_desc(k=k)
        d.p_max = bad
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and "p_max must be n_coeffs.." in msg, msg
    d = fcoef_desc()
    d.max_groups = -2
    st, msg = run_msg("hint_fcoef_run", d)
    assert st != 0 and "max_groups must be >= 0" in msg, msg
    for field, align in (("points", 8), ("counts", 4), ("x", 4), ("workspace", 16)):
        d = fcoef_desc()
        setattr(d, field, BASE + (9 << 28) + align // 2)
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and f"{field} must be {align}-byte aligned" in msg, msg
    for shape in ((100, 64, 5), (FCOEF_MAX_N, MAX_P, MAX_K)):
        d = fcoef_desc(*shape)
        d.workspace_bytes -= 1
        st, msg = run_msg("hint_fcoef_run", d)
        assert st != 0 and "workspace_bytes" in msg and "too small" in msg, msg


def test_workspaces_are_monotone_and_under_their_stated_bounds():
    lib = _lib.load()
    for bad in (0, -1, LENS_MAX_N + 1):
        assert lib.hint_lensgen_workspace_bytes(bad) == 0 and "n_rows must be" in lib.hint_last_error().decode()
    for bad in ((0, 64, 5), (10, 64, 4), (10, 4, 5), (10, MAX_P + 1, 5), (FCOEF_MAX_N + 1, 64, 5)):
        assert lib.hint_fcoef_workspace_bytes(*bad) == 0 and "must be" in lib.hint_last_error().decode()
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 4099, 10 ** 5, 524287, 524288, 524289, 10 ** 7, 10 ** 8, LENS_MAX_N]
    sizes = [lib.hint_lensgen_workspace_bytes(n) for n in ns]
    assert sizes[0] == 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == LENS_WS_BOUND
    assert all(s % 16 == 0 for s in sizes)
    for k in (1, 5, 25):
        ns = [n for n in (1, 19, 20, 21, 4099, 10 ** 5, 10 ** 6, FCOEF_MAX_N)]
        sizes = [lib.hint_fcoef_workspace_bytes(n, 64, k) for n in ns]
        assert sizes[0] == 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] <= FCOEF_WS_BOUND
    assert lib.hint_fcoef_workspace_bytes(FCOEF_MAX_N, MAX_P, MAX_K) == FCOEF_WS_BOUND


def test_python_wrappers_reject_bad_arguments_without_a_gpu():
    bad_calls = [
        (lambda: hint_amd.sample_lens_prior(0, 1), "n must be 1.."),
        (lambda: hint_amd.sample_lens_prior(2.0, 1), "n must be an int"),
        (lambda: hint_amd.sample_lens_prior(True, 1), "n must be an int"),
        (lambda: hint_amd.sample_lens_prior(10, -1), "seed must be 0.."),
        (lambda: hint_amd.sample_lens_prior(10, 2 ** 64), "seed must be 0.."),
        (lambda: hint_amd.sample_lens_prior(10, 1, offset=2 ** 64 - 5), "offset must be 0.."),
        (lambda: hint_amd.sample_lens_prior(10, 1, device="cpu"), "no CPU fallback"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=[[0.5] * 4] * 10), "draws must be a tensor"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(10, 3)), "draws must be ["),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(9, 4)), "draws holds 9 rows and n is 10"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(10, 4)), "no CPU fallback"),
        (lambda: hint_amd.sample_lens_joint(10, 1, noise=float("nan")), "noise must be finite"),
        (lambda: hint_amd.sample_lens_joint(10, 1, noise="0.05"), "noise must be a number"),
        (lambda: hint_amd.lens_rings(torch.zeros(4)), "draws must be ["),
        (lambda: hint_amd.lens_rings(torch.zeros(3, 4)), "no CPU fallback"),
        (lambda: hint_amd.lens_draws(-1, 1), "n must be 1.."),
        (lambda: hint_amd.fourier_coeffs(np.zeros((3, 40, 2)), 5), "points must be a tensor"),
        (lambda: hint_amd.fourier_coeffs(torch.zeros(3, 40), 5), "points must be [N, P, 2]"),
        (lambda: hint_amd.fourier_coeffs(torch.zeros(3, 40, 2), 5), "no CPU fallback"),
    ]
    for call, what in bad_calls:
        with pytest.raises(HintAmdError) as e:
            call()
        assert what in str(e.value), (what, str(e.value))


def test_the_sampler_argument_checks_word_every_refusal_as_recorded():
    """every branch of the draws / sampling-argument checks the samplers share, through this module's wrappers, the whole text"""
    who, shape = "sample_lens_prior", "[1..1073741824, 4] = (u_r, u_t, n_x, n_y)"
    ok = torch.zeros(10, 4)
    fallback = "the sampler is a GPU kernel and there is no CPU fallback"
    no_grad = "requires grad, and no gradient is implemented; call it under torch.no_grad() or detach the input"
    bad_calls = [
        (lambda: hint_amd.sample_lens_prior(0, 1), f"{who}: n must be 1..1073741824 (got 0)"),
        (lambda: hint_amd.sample_lens_prior((1 << 30) + 1, 1), f"{who}: n must be 1..1073741824 (got 1073741825)"),
        (lambda: hint_amd.sample_lens_prior(2.0, 1), f"{who}: n must be an int (got float)"),
        (lambda: hint_amd.sample_lens_prior(True, 1), f"{who}: n must be an int (got bool)"),
        (lambda: hint_amd.sample_lens_prior(10, -1), f"{who}: seed must be 0..18446744073709551615 (got -1)"),
        (lambda: hint_amd.sample_lens_prior(10, 2 ** 64), f"{who}: seed must be 0..18446744073709551615 (got 18446744073709551616)"),
        (lambda: hint_amd.sample_lens_prior(10, "1"), f"{who}: seed must be an int (got str)"),
        (lambda: hint_amd.sample_lens_prior(10, 1, offset=2 ** 64 - 5),
         f"{who}: offset must be 0..18446744073709551605 (got 18446744073709551611)"),
        (lambda: hint_amd.sample_lens_prior(10, 1, offset=-1), f"{who}: offset must be 0..18446744073709551605 (got -1)"),
        (lambda: hint_amd.sample_lens_prior(10, 1, device="cpu"), f"{who}: device is cpu; {fallback}"),
        (lambda: hint_amd.sample_lens_prior(10, 1, device=3.5), f"{who}: device must name a device (got 3.5)"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=[[0.5] * 4] * 10), f"{who}: draws must be a tensor (got list)"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(10, 9)), f"{who}: draws must be {shape} (got shape (10, 9))"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(10)), f"{who}: draws must be {shape} (got shape (10,))"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=torch.zeros(0, 4)), f"{who}: draws must be {shape} (got shape (0, 4))"),
        (lambda: hint_amd.sample_lens_prior(9, 1, draws=ok), f"{who}: draws holds 10 rows and n is 9"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=ok), f"{who}: draws is on cpu; {fallback}"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=OnGpu(ok.to(torch.int32))),
         f"{who}: draws is torch.int32; expected a floating-point tensor"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=OnGpu(ok.clone().requires_grad_(True))), f"{who}: draws {no_grad}"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=OnGpu(ok), device="cuda:0"), f"{who}: draws is on cuda:1 and device is cuda:0"),
        (lambda: hint_amd.sample_lens_prior(10, 1, draws=OnGpu(ok), device="cpu"), f"{who}: device is cpu; {fallback}"),
        (lambda: hint_amd.sample_lens_joint(0, 1), "sample_lens_joint: n must be 1..1073741824 (got 0)"),
        (lambda: hint_amd.sample_lens_joint(10, 1, draws=torch.zeros(10, 9)), f"sample_lens_joint: draws must be {shape} (got shape (10, 9))"),
        (lambda: hint_amd.lens_draws(10, 1, offset=2 ** 64 - 5),
         "lens_draws: offset must be 0..18446744073709551605 (got 18446744073709551611)"),
        (lambda: hint_amd.lens_rings(0.5), "lens_rings: draws must be a tensor (got float)"),
        (lambda: hint_amd.lens_rings(torch.zeros(3, 9)), f"lens_rings: draws must be {shape} (got shape (3, 9))"),
        (lambda: hint_amd.lens_rings(torch.zeros(3, 4)), f"lens_rings: draws is on cpu; {fallback}"),
        (lambda: hint_amd.lens_rings(OnGpu(torch.zeros(3, 4, dtype=torch.int64))),
         "lens_rings: draws is torch.int64; expected a floating-point tensor"),
        (lambda: hint_amd.lens_rings(OnGpu(torch.zeros(3, 4, requires_grad=True))), f"lens_rings: draws {no_grad}"),
    ]
    for call, text in bad_calls:
        with pytest.raises(HintAmdError) as e:
            call()
        assert str(e.value) == text, (text, str(e.value))
    with torch.no_grad():                                   # (no gradient is asked for: the check after it refuses the call)
        with pytest.raises(HintAmdError) as e:
            hint_amd.sample_lens_prior(10, 1, draws=OnGpu(ok.clone().requires_grad_(True)), device="cuda:0")
    assert str(e.value) == f"{who}: draws is on cuda:1 and device is cuda:0"


# ---- the definition ----
def test_oracle_dft_is_the_references_on_the_recorded_fixtures():
    for name in ("fcoef_rings", "fcoef_outlines"):
        f = np.load(os.path.join(GOLDEN, name + ".npz"))
        pts, cnt = f["points"], f["counts"]
        assert pts.dtype == np.float64 and (pts.astype(np.float32) == pts).all()       # fp32 values: a GPU test feeds the same numbers
        for k in (5, 25):
            ref = f[f"ref{k}"]
            assert ref.shape == (len(pts), 4 * k)
            got = so.coeffs(pts, cnt, k)
            assert np.abs(got - ref).max() <= 1e-12, (name, k, np.abs(got - ref).max())
    f = np.load(os.path.join(GOLDEN, "fcoef_rings.npz"))
    assert sorted(set(f["counts"].tolist())) == [31, 32]
    ring, cnt = so.rings(f["draws"])                        # the fixture's rings are the oracle's own, rounded to fp32
    assert (cnt == f["counts"]).all() and np.abs(ring - f["points"]).max() <= 2.0 ** -23 * np.abs(ring).max()


def test_oracle_philox_is_noise_oracles():
    seed, offset, n = 0x123456789ABCDEF, 2 ** 32 - 5, 10
    ur, ut = so.uniforms(seed, offset, n)
    row = offset + np.arange(n, dtype=np.uint64)
    c = no.philox4x32_10((row & no.MASK, row >> np.uint64(32), 0, 0x4C454E53), (seed & 0xFFFFFFFF, seed >> 32))
    s = np.float32(2.0 ** -32)
    assert (ur == c[0].astype(np.float32) * s).all() and (ut == c[1].astype(np.float32) * s).all()
    assert ur.dtype == np.float32 and (ur >= 0).all() and (ur <= 1).all()
    assert (row >> np.uint64(32)).min() == 0 and (row >> np.uint64(32)).max() == 1         # the counter's high word changes inside
    # chunking: rows are a function of (seed, offset + i)
    d = so.draws(seed, offset, n)
    assert (np.concatenate([so.draws(seed, offset, 3), so.draws(seed, offset + 3, n - 3)]) == d).all()
    assert (so.draws(seed + 1, offset, n) != d).any()
    # the tag and the stream separate this stream from the training noise and from eps
    t = no.philox4x32_10((row & no.MASK, row >> np.uint64(32), 0, no.TAG), (seed & 0xFFFFFFFF, seed >> 32))
    assert (t[0] != c[0]).any()
    assert (so.eps_draws(seed, offset, n) != d[:, 2:4]).any()
    # moments of a long stream
    big = so.draws(3, 0, 200000)
    assert abs(big[:, 0].mean() - 0.5) < 5 / np.sqrt(12 * 200000) and abs(big[:, 1].mean() - 0.5) < 5 / np.sqrt(12 * 200000)
    assert abs(big[:, 2:].mean()) < 5 / np.sqrt(400000) and abs(big[:, 2:].var() - 1) < 5 * np.sqrt(2 / 400000)


def test_vertex_count_range_from_a_sweep_of_u_t():
    ut = (np.arange(100000) + 0.5) / 100000
    d = np.stack([np.full_like(ut, 0.25), ut, 0 * ut, 0 * ut], axis=1)
    ia, ib, slack = so.classify(d)
    counts = ia.sum(axis=1) + ib.sum(axis=1) + 2
    assert (int(counts.min()), int(counts.max())) == so.COUNT_RANGE == (30, 31)
    assert set(ia.sum(axis=1)) == {19, 20} and set(ib.sum(axis=1)) == {8, 9}
    share31 = float((counts == 31).mean())
    assert 0.08 < share31 < 0.11, share31
    # the count does not depend on r0 (the figure scales)
    d2 = d[::97].copy()
    d2[:, 0] = np.linspace(0, 1, len(d2))
    assert (so.open_counts(d2) == counts[::97]).all()
    assert float((slack < so.MARGIN).mean()) <= so.MAX_AMBIGUOUS


def test_kernel_classification_rule_agrees_with_brute_force():
    rng = np.random.RandomState(1)
    ut = np.concatenate([(np.arange(50000) + 0.5) / 50000, np.arange(4097) / 4096.0, rng.rand(50000)])
    d = np.stack([rng.rand(len(ut)), ut, 0 * ut, 0 * ut], axis=1).astype(np.float32)
    ia, ib, slack = so.classify(d)
    jlo, nA, klo, nB, ok = so.window_runs(d)
    keep = slack >= so.MARGIN
    assert float((~keep).mean()) <= so.MAX_AMBIGUOUS
    rj, rk = np.argmax(ia & ~np.roll(ia, 1, axis=1), axis=1), np.argmax(ib & ~np.roll(ib, 1, axis=1), axis=1)
    same = ok & (jlo == rj) & (nA == ia.sum(axis=1)) & (klo == rk) & (nB == ib.sum(axis=1))
    assert same[keep].all(), int((~same[keep]).sum())
    assert ok.all()                                         # draws in range are never rejected, ambiguous or not


def test_clipped_ring_is_the_ring_of_the_definition():
    d = so.draws(5, 0, 300)
    ring, cnt = so.rings(d)
    ring2, cnt2 = so.direct_rings(d)
    assert (cnt == cnt2).all() and (cnt - 1 == so.open_counts(d)).all()
    assert np.abs(ring - ring2).max() <= 1e-13
    for i in range(len(d)):
        r = ring[i, :cnt[i]]
        assert (r[0] == r[-1]).all() and (ring[i, cnt[i]:] == 0).all()
        e = np.roll(r[:-1], -1, axis=0) - r[:-1]
        nxt = np.roll(e, -1, axis=0)
        assert (e[:, 0] * nxt[:, 1] - e[:, 1] * nxt[:, 0] < 1e-12).all()       # clockwise and convex
        area = 0.5 * np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1])
        assert area < 0                                                          # clockwise


def test_dc_coefficient_is_minus_half_the_noise():
    d = so.draws(9, 100, 200)
    x, ring, cnt = so.sample(d)
    assert np.abs(x[:, 2] + 0.5 * d[:, 2]).max() <= 1e-14 and np.abs(x[:, 7] + 0.5 * d[:, 3]).max() <= 1e-14
    assert np.abs(x[:, [12, 17]]).max() <= 1e-14            # ... and it is real
    # a real signal: a[-m] is the conjugate of a[m]
    assert np.abs(x[:, 0:5] - x[:, 4::-1]).max() <= 1e-14 and np.abs(x[:, 10:15] + x[:, 14:9:-1]).max() <= 1e-14


def test_fp32_floor_is_inside_the_bounds():
    d = so.draws(21, 0, 1500, np.float32)
    ring_floor, coef_floor, rows = so.fp32_floor(d)
    print(f"fp32 floor over {rows} rows: ring {ring_floor:.1f} u A (bound {so.K_RING}), coefficients {coef_floor:.1f} u A (bound {so.K_COEF})")
    assert rows >= 0.99 * len(d)
    assert 1.0 < ring_floor <= so.K_RING and 1.0 < coef_floor <= so.K_COEF
    # fourier_coeffs alone, on the recorded outlines
    f = np.load(os.path.join(GOLDEN, "fcoef_outlines.npz"))
    for i, c in enumerate(f["counts"]):
        p = f["points"][i, :c]
        for k in (5, 25):
            err = np.abs(so.dft(p, k, np.float32) - f[f"ref{k}"][i]).max() / (so.U * np.abs(p).max())
            assert err <= so.k_fcoef(c), (c, k, err)
