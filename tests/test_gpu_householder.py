"""GPU tests of the Householder permutation (hint_householder_run, hint_amd.HouseholderPerm, the flows' learned_perms switch)
against the float64 statement of tests/householder_oracle.py.  The bounds, u = 2^-24:
  BUILD  per entry |W - W64| <= 2^-23 |W64| + 1e-11: one rounding to fp32 (2^-24, a factor of two to spare) plus two float64
         evaluations in different orders (about n (2 d + 8) 2^-53 with all norms <= 1)
  APPLY  per entry |y - y64| <= (d + 8) u (|x| |W64|)_ij: gamma of at most d + 3 fp32 multiply-adds in any order, 2 u for W's own
         rounding, slack to d + 8; g_x the same with g_y for x
  g_W    per entry <= (min(B, R / 4) + 8) u (|x|^T |g_y|)_ij, R the slab's rows from hint_householder_geometry.  Derivation, from
         the kernel's order of operations (include/hint_amd.h): within a slab of R rows each of four wavefronts adds every fourth
         k-block of 4 rows on the MFMA, so one accumulator is a chain of at most R / 4 fp32 products (and of at most B: products
         with the exact zeros of rows past B add nothing and round nothing) - at most min(B, R / 4) roundings on partial sums that
         never exceed the slab's sum of |x| |g_y|; three fp32 additions join the four wavefronts' partial tiles; the slabs of an
         entry are added in double (2^-53 each: nothing at this scale); the sum is rounded to fp32 once at the store.  To first
         order that is min(B, R / 4) + 4 roundings, each at most u times the entry's sum of |x| |g_y|; + 8 leaves the rest as
         slack.  The slab count does not enter: every slab's chain is bounded against its own share of the sum.  It is never
         looser than (B + 8) u, the bound this file held before, and at B = 2^22 (R = 65536, 64 slabs) it is 1 / 256 of it:
         9.8e-4 of the entry's magnitude where a slab left out moves an entry of same-signed data by 1 / 64.
  g_V    rel_err < 1e-4, the project's gradient tolerance (tests/test_gpu_parity.py).  d = 1 is the exception: W = (-1)^n does not
         depend on Vs, so the gradient is exactly zero and a relative error has no denominator; the closed form's two terms, each
         4 |G| / |v| in magnitude and the outcome of at most a dozen double operations, cancel: |g_V| <= 64 2^-53 4 |G| / |v|.
The regimes no small batch reaches run at the smallest B that reaches them, each taken from hint_householder_geometry or from the
apply grid's rule (tests/large_cases.py HH_TRIP; tests/test_large_cases_cpu.py holds the constants against the kernel's text): the
last B with R = 256 and the first with R > 256, a second trip of the apply kernel's tile loop, a last trip on which part of the
workgroups idle, and the documented limit B = 2^22, d = 128 itself (tests/large_cases.py LIMITED names that test).  There the
references are float64 on the device in row chunks, x and g_y are randn + 2 (sums that do not cancel: a slab left out cannot
hide inside the bound, which the test asserts from the geometry), y and g_x lie in guard-banded buffers over the NaN pattern, and
the probe rows - head, tail, two rows on either side of every multiple of HH_TRIP, where a workgroup begins its next trip - equal
a small call on the same rows bit for bit (the header's promise that any split of the batch gives the bits of one call).
The worst measured ratio to every bound goes to householder_errors.json (pytest -q swallows prints) in the directory
HINT_TEST_RECORDS names, test_records/ in the repository by default."""
import contextlib
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, householder as hh
from hint_amd._lib import HintAmdError
import householder_oracle as ho
import large_cases as lc
import stream_gate
from guarded import FILLS, NAN_BITS, Guarded, bits_equal
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BUILD, APPLY, GRAD = 0, 1, 2
SLAB = _lib.load().hint_householder_geometry(1, 1, 0)
BS = (1, 15, 16, 17, SLAB + 1, 2 * SLAB + 5)
# the edges: d = 1; the tile edge (16, 17); where hh_lds's ld takes its 16 more (32, 33); the ldx 68 / 132 switch and the build
# kernel's second entry per lane (63, 64, 65); the most reflections (n = 256)
DN = sorted({(d, n) for d in (2, 5, 20, 100, 128) for n in (1, 2, d, d + 3)}
            | {(d, n) for d in (1, 16, 17, 32, 33, 63, 64, 65) for n in (1, d)} | {(20, 256), (128, 256)})
WORST = {}


def geometry(B, d):
    """(R, slabs) of a grad run over B rows"""
    lib = _lib.load()
    R, slabs = int(lib.hint_householder_geometry(B, d, 0)), int(lib.hint_householder_geometry(B, d, 1))
    assert R >= SLAB and R % 16 == 0 and (slabs - 1) * R < B <= slabs * R
    return R, slabs


def gw_factor(B, d):
    """the g_W bound's factor of (|x|^T |g_y|)_ij (the module docstring derives it)"""
    return (min(B, geometry(B, d)[0] // 4) + 8) * U


def record(name, rec):
    out = os.environ.get("HINT_TEST_RECORDS") or os.path.join(ROOT, "test_records")
    try:
        os.makedirs(out, exist_ok=True)
        f = os.path.join(out, "householder_errors.json")
        have = json.load(open(f)) if os.path.exists(f) else {}
        have[name] = rec
        json.dump(have, open(f, "w"), indent=1)
    except OSError:
        pass


def worst(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    record("worst_ratio_to_bound", WORST)


def ratio(got, want, bound):
    """largest |got - want| / bound over the entries (bound > 0 wherever want can differ from got)"""
    err = (got.double().cpu() - want).abs()
    assert bool(torch.isfinite(err).all())
    return float((err / bound.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def case(d, n):
    """Vs (fp32, the module's initialisation), the statement's W in float64, and the rows of the largest batch"""
    Vs = ho.init_Vs(n, d, seed=1000 * d + n)
    g = torch.Generator().manual_seed(d * 7 + n)
    x = torch.randn(BS[-1], d, generator=g)
    gy = torch.randn(BS[-1], d, generator=g)
    return Vs, ho.W(Vs), x, gy


def ws_bytes(B, d, n):
    nbytes = _lib.load().hint_householder_workspace_bytes(GRAD, B, d, n)
    assert nbytes > 0
    return nbytes


def build(Vs):
    n, d = Vs.shape
    W = torch.empty(d, d, device=DEV)
    hh._run(BUILD, DEV, d=d, n=n, Vs=Vs, W=W)
    return W


def apply(x, W, rev):
    y = torch.empty_like(x)
    hh._run(APPLY, DEV, B=x.shape[0], d=x.shape[1], transpose=rev, W=W, x=x, y=y)
    return y


def grad(x, gy, W, Vs, rev, want=("g_x", "g_W", "g_V")):
    n, d = Vs.shape
    out = {"g_x": torch.empty_like(x), "g_W": torch.empty(d, d, device=DEV), "g_V": torch.empty_like(Vs)}
    out = {k: v for k, v in out.items() if k in want}
    hh._run(GRAD, DEV, B=x.shape[0], d=d, n=n, transpose=rev, Vs=Vs, W=W, x=x, g_y=gy, **out)
    return out


# ---- the three ops against the statement ----
@pytest.mark.parametrize("d,n", DN)
def test_build_apply_grad_against_the_statement(d, n):
    Vs, W64, xs, gys = case(d, n)
    Vd = Vs.to(DEV)
    W = build(Vd)
    assert bits_equal(W, build(Vd))
    worst("build", ratio(W, W64, 2.0 ** -23 * W64.abs() + 1e-11))
    assert ratio(W, W64, 2.0 ** -23 * W64.abs() + 1e-11) <= 1.0
    for B in BS:
        x, gy = xs[:B].contiguous(), gys[:B].contiguous()
        xd, gyd = x.to(DEV), gy.to(DEV)
        for rev in (False, True):
            M = W64.t() if rev else W64
            y = apply(xd, W, rev)
            assert bits_equal(y, apply(xd, W, rev))
            r = ratio(y, x.double() @ M, (d + 8) * U * ho.abs_products(x, M))
            worst("apply", r)
            assert r <= 1.0, (B, rev, r)
            got = grad(xd, gyd, W, Vd, rev)
            again = grad(xd, gyd, W, Vd, rev)
            assert all(bits_equal(got[k], again[k]) for k in got)
            gx64, gW64, gV64 = ho.grads(x, Vs, gy, rev)
            r = ratio(got["g_x"], gx64, (d + 8) * U * ho.abs_products(gy, M.t()))
            worst("g_x", r)
            assert r <= 1.0, (B, rev, r)
            a, b = (gy, x) if rev else (x, gy)
            assert gw_factor(B, d) <= (B + 8) * U
            r = ratio(got["g_W"], gW64, gw_factor(B, d) * ho.abs_products(a.t(), b))
            worst("g_W", r)
            assert r <= 1.0, (B, rev, r)
            if d == 1:                                      # the gradient is exactly zero: two terms of 4 |G| / |v| cancel
                cancel = 64 * 2.0 ** -53 * 4 * ho.abs_products(a.t(), b) / Vs.double().abs()
                r = max(ratio(got["g_V"], torch.zeros(n, d, dtype=torch.float64), cancel), float((gV64.abs() / cancel).max()))
                worst("g_V_d1_over_cancellation_bound", r)
                assert r <= 1.0, (B, rev, r)
                continue
            e = rel_err(got["g_V"].cpu().numpy(), gV64.numpy())
            worst("g_V_rel_err_over_1e-4", e / 1e-4)
            assert e < 1e-4, (B, rev, e)


def test_apply_in_three_ragged_calls_gives_the_bits_of_one():
    for d, n in ((5, 5), (100, 103)):
        Vs, _, xs, _ = case(d, n)
        W = build(Vs.to(DEV))
        x = xs.to(DEV)
        for rev in (False, True):
            whole = apply(x, W, rev)
            cuts = (0, 7, SLAB + 19, x.shape[0])
            parts = [apply(x[a:b].contiguous(), W, rev) for a, b in zip(cuts, cuts[1:])]
            assert bits_equal(whole, torch.cat(parts))


# ---- the regimes of a large batch, and the limit ----
def first_B(pred, lo, hi):
    """the smallest B in lo..hi with pred(B); pred is monotone"""
    assert pred(hi) and not pred(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def regime_batches():
    """{name: B}, each from the geometry query or the apply grid's rule"""
    grows = first_B(lambda B: geometry(B, 5)[0] > SLAB, SLAB, hh.MAX_B)         # the first B whose slabs hold more than SLAB rows
    assert geometry(grows - 1, 128) == (SLAB, 64) and geometry(grows, 128)[0] == SLAB + 16         # (the geometry ignores d)
    groups = lambda B: -(-(-(-B // lc.HH_T)) // lc.HH_APPLY_WAVES)                                 # noqa: E731
    trip = first_B(lambda B: groups(B) > lc.HH_MAX_GRID, 1, hh.MAX_B)           # the first B with more workgroups than the grid
    assert trip == lc.HH_TRIP + 1
    out = {"last_R_256": grows - 1, "first_R_above_256": grows,
           "second_trip": lc.HH_TRIP + lc.HH_T + 1,                              # the second trip: a whole tile and one of one row
           "idle_last_trip": 2 * lc.HH_TRIP + lc.HH_TRIP // 2 + 5}               # the third trip: half the workgroups have no tile
    assert groups(out["second_trip"]) == lc.HH_MAX_GRID + 1 and out["second_trip"] % lc.HH_T
    assert 2 * lc.HH_MAX_GRID < groups(out["idle_last_trip"]) < 3 * lc.HH_MAX_GRID and out["idle_last_trip"] % lc.HH_T
    return out


REGIMES = regime_batches()
REF_CHUNK = lc.CHUNK_ELEMS // 4       # elements of a float64 temporary of the device references: 0.5 GiB
assert REF_CHUNK <= lc.CHUNK_ELEMS


def row_chunks(B, d):
    step = max(1, REF_CHUNK // d)
    return [(a, min(B, a + step)) for a in range(0, B, step)]


def rows_ratio(got, src, M64, k):
    """largest |got - src M| / (k u |src| |M|) over the entries: float64 on the device, in row chunks"""
    out = 0.0
    for a, b in row_chunks(*src.shape):
        s = src[a:b].double()
        err = (got[a:b].double() - s @ M64).abs_()
        bound = (s.abs_() @ M64.abs()).mul_(k * U).clamp_min_(1e-300)
        assert bool(torch.isfinite(err).all())
        out = max(out, float(err.div_(bound).max()))
    return out


def gram64(a, b):
    """(a^T b, |a|^T |b|) in float64 on the device, in row chunks"""
    d = a.shape[1]
    G, A = torch.zeros(d, d, dtype=torch.float64, device=DEV), torch.zeros(d, d, dtype=torch.float64, device=DEV)
    for lo, hi in row_chunks(*a.shape):
        u, v = a[lo:hi].double(), b[lo:hi].double()
        G += u.t() @ v
        A += u.abs_().t() @ v.abs_()
    return G, A


def trip_probes(B):
    """head, tail, and two rows on either side of every multiple of HH_TRIP inside the batch"""
    rows = set(range(min(64, B))) | set(range(max(0, B - 80), B))
    for m in range(lc.HH_TRIP, B + 2, lc.HH_TRIP):
        rows |= {r for r in (m - 2, m - 1, m, m + 1) if 0 <= r < B}
    return torch.tensor(sorted(rows), dtype=torch.int64, device=DEV)


def no_nan_words(g, what):
    left = lc.count_words(g.words, NAN_BITS)
    assert left == 0, f"{what}: {left} words were never written"


def large_batch(B, d, n, tag):
    """apply and grad at both transposes over B rows of randn + 2, as the module docstring says"""
    R, slabs = geometry(B, d)
    assert 1.0 / slabs >= 10 * (R // 4 + 8) * U, (R, slabs)             # a slab left out moves an entry by ten bounds at least
    Vs = ho.init_Vs(n, d, seed=1000 * d + n)
    Vd, W64 = Vs.to(DEV), ho.W(Vs).to(DEV)
    W = build(Vd)
    g = torch.Generator(device=DEV).manual_seed(B % 100003 + d)
    x, gy = torch.empty(B, d, device=DEV), torch.empty(B, d, device=DEV)
    for t in (x, gy):
        lc.fill_chunked(t, lambda m: torch.randn(m, d, generator=g, device=DEV).add_(2.0), REF_CHUNK)
    rt = trip_probes(B)
    xp, gyp = x[rt].contiguous(), gy[rt].contiguous()
    ws = torch.empty(ws_bytes(B, d, n), dtype=torch.uint8, device=DEV)
    y, g_x = Guarded(B * d, "nan"), Guarded(B * d, "nan")
    for rev in (False, True):
        M = W64.t() if rev else W64
        what = f"B {B} d {d} rev {rev}"
        y.fill("nan")
        hh._run(APPLY, DEV, B=B, d=d, transpose=rev, W=W, x=x, y=y.view(B, d))
        torch.cuda.synchronize()
        y.check_guards(what + ": y")
        no_nan_words(y, what + ": y")
        r = rows_ratio(y.view(B, d), x, M, d + 8)
        worst(tag + "apply", r)
        assert r <= 1.0, (what, r)
        assert bits_equal(y.view(B, d)[rt], apply(xp, W, rev)), what + ": a probe row's bits depend on its position"
        g_x.fill("nan")
        got = {"g_x": g_x.view(B, d), "g_W": torch.empty(d, d, device=DEV), "g_V": torch.empty(n, d, device=DEV)}
        hh._run(GRAD, DEV, B=B, d=d, n=n, transpose=rev, Vs=Vd, W=W, x=x, g_y=gy, workspace=ws, **got)
        torch.cuda.synchronize()
        g_x.check_guards(what + ": g_x")
        no_nan_words(g_x, what + ": g_x")
        r = rows_ratio(got["g_x"], gy, M.t(), d + 8)
        worst(tag + "g_x", r)
        assert r <= 1.0, (what, r)
        small = grad(xp, gyp, W, Vd, rev, want=("g_x",))
        assert bits_equal(got["g_x"][rt], small["g_x"]), what + ": a probe row's bits of g_x depend on its position"
        a, b = (gy, x) if rev else (x, gy)
        G64, A64 = gram64(a, b)
        r = ratio(got["g_W"], G64.cpu(), (gw_factor(B, d) * A64).cpu())
        worst(tag + "g_W", r)
        assert r <= 1.0, (what, r)
        e = rel_err(got["g_V"].cpu().numpy(), ho.g_V_from_g_W(Vs, G64.cpu()).numpy())
        worst(tag + "g_V_rel_err_over_1e-4", e / 1e-4)
        assert e < 1e-4, (what, e)
        # two grad runs give equal bits (the second g_x goes where y was: y has been checked)
        y.fill("nan")
        again = {"g_x": y.view(B, d), "g_W": torch.empty(d, d, device=DEV), "g_V": torch.empty(n, d, device=DEV)}
        hh._run(GRAD, DEV, B=B, d=d, n=n, transpose=rev, Vs=Vd, W=W, x=x, g_y=gy, workspace=ws, **again)
        torch.cuda.synchronize()
        assert all(bits_equal(got[k], again[k]) for k in got), what + ": two grad runs differ"
        print(f"householder {what}: R {R}, {slabs} slabs; ratios " + ", ".join(f"{k[len(tag):]} {v:.3g}" for k, v in WORST.items()
                                                                                 if k.startswith(tag)))


@pytest.mark.parametrize("d", (5, 100))
@pytest.mark.parametrize("regime", list(REGIMES))
def test_large_batch_regimes(regime, d):
    large_batch(REGIMES[regime], d, d, "large_B_")


LIMIT_BYTES = 4 * 4 * hh.MAX_B * hh.MAX_D + 6 * 8 * REF_CHUNK      # x, g_y, y, g_x; six float64 temporaries of a reference chunk


@pytest.mark.timeout(120)
def test_the_row_limit():
    """B = 2^22, d = 128, n = 128: the documented limit, where the last element offset is 2^29 - 1 (tests/large_cases.py LIMITED)"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < LIMIT_BYTES:
        pytest.skip(f"needs {LIMIT_BYTES / lc.GIB:.1f} GiB of device memory, {free / lc.GIB:.1f} GiB are free")
    assert _lib.load().hint_householder_workspace_bytes(GRAD, hh.MAX_B + 1, hh.MAX_D, hh.MAX_D) == 0
    try:
        large_batch(hh.MAX_B, hh.MAX_D, hh.MAX_D, "limit_B_")
    finally:
        torch.cuda.empty_cache()


def test_nan_patterns():
    Vs, _, xs, _ = case(20, 23)
    V = Vs.clone()
    V[1] = 0.0
    W = build(V.to(DEV))
    assert bool(torch.isnan(W).all())                       # every row of W passes through H_1
    W = build(Vs.to(DEV))
    x = xs[:40].clone()
    x[3, 7] = float("nan")
    for rev in (False, True):
        y = apply(x.to(DEV), W, rev)
        bad = torch.isnan(y).any(dim=1).cpu()
        assert bool(torch.isnan(y[3]).all()) and bad.sum().item() == 1


# ---- guard bands, poisoned outputs, optional outputs ----
@pytest.mark.parametrize("d,n,B", [(20, 23, SLAB + 1), (100, 2, 17), (128, 128, 2 * SLAB + 5)])
def test_guarded_outputs_on_every_fill(d, n, B):
    Vs, _, xs, gys = case(d, n)
    nbytes = ws_bytes(B, d, n)
    results = {}
    for fill in FILLS:
        gV, gx, ggy = Guarded(n * d).set(Vs), Guarded(B * d).set(xs[:B]), Guarded(B * d).set(gys[:B])
        consts = [gV, gx, ggy]
        snaps = [g.snapshot() for g in consts]
        W, y = Guarded(d * d, fill, seed=1), Guarded(B * d, fill, seed=2)
        g_x, g_W, g_V = Guarded(B * d, fill, seed=3), Guarded(d * d, fill, seed=4), Guarded(n * d, fill, seed=5)
        ws = Guarded(nbytes // 4, fill, align=16, seed=6)
        Vt, xt, gyt = gV.view(n, d), gx.view(B, d), ggy.view(B, d)
        hh._run(BUILD, DEV, d=d, n=n, Vs=Vt, W=W.view(d, d))
        hh._run(APPLY, DEV, B=B, d=d, transpose=False, W=W.view(d, d), x=xt, y=y.view(B, d))
        hh._run(GRAD, DEV, B=B, d=d, n=n, Vs=Vt, W=W.view(d, d), x=xt, g_y=gyt, g_x=g_x.view(B, d), g_W=g_W.view(d, d),
                g_V=g_V.view(n, d), workspace=ws.t.view(torch.uint8))
        torch.cuda.synchronize()
        outs = {"W": W, "y": y, "g_x": g_x, "g_W": g_W, "g_V": g_V}
        for k, g in list(outs.items()) + [("workspace", ws)]:
            g.check_guards(f"{fill}: {k}")
        for g, s, k in zip(consts, snaps, ("Vs", "x", "g_y")):
            g.check_unchanged(s, f"{fill}: {k}")
        results[fill] = {k: g.words.clone() for k, g in outs.items()}
        if fill == "nan":
            for k, g in outs.items():
                assert int((g.words == NAN_BITS).sum()) == 0, f"{k}: words the run did not write"
        # an output that is not asked for is not touched; the others keep their bits
        for asked in (("g_x",), ("g_W",), ("g_V",), ("g_x", "g_V")):
            bufs = {"g_x": Guarded(B * d, fill, seed=7), "g_W": Guarded(d * d, fill, seed=8), "g_V": Guarded(n * d, fill, seed=9)}
            before = {k: g.snapshot() for k, g in bufs.items()}
            shapes = {"g_x": (B, d), "g_W": (d, d), "g_V": (n, d)}
            hh._run(GRAD, DEV, B=B, d=d, n=n, Vs=Vt, W=W.view(d, d), x=xt, g_y=gyt, workspace=ws.t.view(torch.uint8),
                    **{k: bufs[k].view(*shapes[k]) for k in asked})
            torch.cuda.synchronize()
            for k, g in bufs.items():
                if k in asked:
                    g.check_guards(f"{fill} {asked}: {k}")
                    assert torch.equal(g.words, results[fill][k]), (fill, asked, k)
                else:
                    g.check_unchanged(before[k], f"{fill} {asked}: {k} (not asked)")
            ws.check_guards(f"{fill} {asked}: workspace")
    for fill in FILLS[1:]:
        for k in results[fill]:
            assert torch.equal(results[fill][k], results[FILLS[0]][k]), (fill, k)


# ---- a gated non-default stream ----
@contextlib.contextmanager
def side_stream():
    """a non-blocking stream of this test's own, destroyed behind it (a stream from torch's pool would live on and shift which
    hardware queue later test files' streams share)"""
    hip = _lib.load()
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
    raw = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0 and raw.value      # 1: hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(raw.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0


def test_three_ops_on_a_gated_non_default_stream():
    """the stream is a field of the descriptor: build, apply and grad S-gated and null-gated on a side stream, still_closed()
    asserted (tests/stream_gate.py), the results equal to the null-stream bits"""
    d, n, B = 20, 23, SLAB + 1
    Vs, _, xs, gys = case(d, n)
    nbytes = ws_bytes(B, d, n)
    streams = []

    def make(fill, role):
        gV, gx, ggy = Guarded(n * d).set(Vs), Guarded(B * d).set(xs[:B]), Guarded(B * d).set(gys[:B])
        late = stream_gate.late_inputs([(gV, None), (gx, None), (ggy, None)])
        W, y = Guarded(d * d, fill, seed=1), Guarded(B * d, fill, seed=2)
        g_x, g_W, g_V = Guarded(B * d, fill, seed=3), Guarded(d * d, fill, seed=4), Guarded(n * d, fill, seed=5)
        ws = Guarded(nbytes // 4, fill, align=16, seed=6)

        def call():
            streams.append((role, torch.cuda.current_stream().cuda_stream))
            Vt, xt, gyt, Wt = gV.view(n, d), gx.view(B, d), ggy.view(B, d), W.view(d, d)
            hh._run(BUILD, DEV, d=d, n=n, Vs=Vt, W=Wt)
            hh._run(APPLY, DEV, B=B, d=d, transpose=False, W=Wt, x=xt, y=y.view(B, d))
            hh._run(GRAD, DEV, B=B, d=d, n=n, Vs=Vt, W=Wt, x=xt, g_y=gyt, g_x=g_x.view(B, d), g_W=g_W.view(d, d),
                    g_V=g_V.view(n, d), workspace=ws.t.view(torch.uint8))
            return {"W": W.t, "y": y.t, "g_x": g_x.t, "g_W": g_W.t, "g_V": g_V.t}
        guards = [("W", W), ("y", y), ("g_x", g_x), ("g_W", g_W), ("g_V", g_V), ("workspace", ws), ("Vs", gV), ("x", gx), ("g_y", ggy)]
        return stream_gate.Seq(call, late, guards)
    with side_stream() as S:
        stream_gate.run_case("hint_householder_run", make, S)
        assert {st for role, st in streams if role == "S"} == {S.cuda_stream} and S.cuda_stream != 0
        assert {st for role, st in streams if role == "ref"} == {0}


# ---- graph capture ----
@pytest.mark.parametrize("d,n,B", [(20, 20, SLAB + 1), (100, 103, 33)])
def test_captured_ops_follow_vs_changed_in_place(d, n, B):
    Vs, _, xs, gys = case(d, n)
    Vd, x, gy = Vs.to(DEV), xs[:B].to(DEV), gys[:B].to(DEV)
    W, y = torch.empty(d, d, device=DEV), torch.empty(B, d, device=DEV)
    outs = {"g_x": torch.empty(B, d, device=DEV), "g_W": torch.empty(d, d, device=DEV), "g_V": torch.empty(n, d, device=DEV)}
    ws = torch.empty(ws_bytes(B, d, n), dtype=torch.uint8, device=DEV)

    def ops():
        hh._run(BUILD, DEV, d=d, n=n, Vs=Vd, W=W)
        hh._run(APPLY, DEV, B=B, d=d, transpose=True, W=W, x=x, y=y)
        hh._run(GRAD, DEV, B=B, d=d, n=n, transpose=True, Vs=Vd, W=W, x=x, g_y=gy, workspace=ws, **outs)
    ops()                                                   # (warm-up: nothing of the first launch's setup is captured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops()
    new = ho.init_Vs(n, d, seed=77).to(DEV)
    Wn = build(new)
    want = dict(grad(x, gy, Wn, new, True), W=Wn, y=apply(x, Wn, True))
    Vd.copy_(new)
    for rep in range(2):
        for t in [W, y] + list(outs.values()):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(outs, W=W, y=y)
        for k in want:
            assert bits_equal(got[k], want[k]), (rep, k)


# ---- the module ----
@pytest.mark.parametrize("d,n", [(5, 5), (20, 3), (100, 100)])
def test_module_inverts_itself_and_its_gradients_meet_the_statement(d, n):
    m = hint_amd.HouseholderPerm([(d,)], n_reflections=n, seed=3).to(DEV)
    x = torch.randn(70, d, device=DEV)
    with torch.no_grad():
        (y,) = m([x])
        (xr,) = m([y], rev=True)
        assert m([x[:0]])[0].shape == (0, d)
    assert rel_err(xr.cpu().numpy(), x.cpu().numpy()) < 1e-5
    assert y.data_ptr() != x.data_ptr() and m.matrix().data_ptr() == m.matrix().data_ptr()
    gy = torch.randn(70, d, device=DEV)
    for rev in (False, True):
        m.Vs.grad = None
        xg = x.clone().requires_grad_(True)
        (out,) = m([xg], rev=rev)
        (out * gy).sum().backward()
        gx64, _, gV64 = ho.grads(x.cpu(), m.Vs.detach().cpu(), gy.cpu(), rev)
        assert rel_err(out.detach().cpu().numpy(), ho.apply(x.cpu(), m.Vs.detach().cpu(), rev).numpy()) < 1e-5
        e_x, e_V = rel_err(xg.grad.cpu().numpy(), gx64.numpy()), rel_err(m.Vs.grad.cpu().numpy(), gV64.numpy())
        worst("module_grad_rel_err_over_1e-4", max(e_x, e_V) / 1e-4)
        assert e_x < 1e-4 and e_V < 1e-4, (rev, e_x, e_V)
    f = hint_amd.HouseholderPerm([(d,)], n_reflections=n, fixed=True, seed=3).to(DEV)
    xg = x.clone().requires_grad_(True)
    (out,) = f([xg])
    out.sum().backward()
    assert f.Vs.grad is None and xg.grad is not None and bits_equal(out.detach(), y)
    with pytest.raises(HintAmdError):
        m([x.cpu()])


def test_matrix_is_rebuilt_on_every_call_unless_the_pack_cache_or_fixed_says_otherwise():
    """a zeroed buffer shows whether matrix() ran BUILD again: always by default (ClampAdam writes Vs through raw pointers);
    under set_pack_cache(True) only when Vs's address or version, or the weight generation (a ClampAdam step), moved;
    fixed=True by the same key whatever the switch"""
    m = hint_amd.HouseholderPerm([(5,)], seed=3).to(DEV)
    f = hint_amd.HouseholderPerm([(5,)], fixed=True, seed=3).to(DEV)
    want = m.matrix().clone()
    ptr = m.matrix().data_ptr()

    def rebuilt(mod):
        mod._Wbuf.zero_()
        W = mod.matrix()
        assert W.data_ptr() == mod._Wbuf.data_ptr()
        return bool(W.abs().sum() > 0)
    assert rebuilt(m) and bits_equal(m.matrix(), want) and m.matrix().data_ptr() == ptr
    f.matrix()
    assert not rebuilt(f)
    f._Wkey = None
    assert bits_equal(f.matrix(), want)
    prev = hint_amd.set_pack_cache(True)
    try:
        m.matrix()
        assert not rebuilt(m)
        with torch.no_grad():
            m.Vs.mul_(1.5)                                  # a version bump (what torch's optimizers do)
        assert rebuilt(m)
        assert not rebuilt(m)
        (out,) = m([torch.randn(8, 5, device=DEV)])
        out.sum().backward()
        hint_amd.ClampAdam(m.parameters(), lr=1e-2).step()  # raw-pointer writes: the weight generation moves
        assert rebuilt(m) and m.matrix().data_ptr() == ptr
        assert rel_err(m.matrix().cpu().numpy(), ho.W(m.Vs.detach().cpu()).numpy()) < 1e-6
    finally:
        hint_amd.set_pack_cache(prev)
    assert rebuilt(m)


def test_vs_changed_in_place_between_forward_and_backward_is_an_error():
    m = hint_amd.HouseholderPerm([(5,)], seed=3).to(DEV)
    (out,) = m([torch.randn(8, 5, device=DEV)])
    with torch.no_grad():
        m.Vs.mul_(2.0)
    with pytest.raises(RuntimeError):
        out.sum().backward()


# ---- the flows ----
def nll(z, J):
    return (0.5 * (z ** 2).sum(1) - J).mean()


def fixed_twin(flow, make):
    """the same flow on the existing route: every HouseholderPerm replaced by FixedOrthogonal(W=perm.matrix())"""
    twin = make().to(DEV)
    twin.load_state_dict(flow.state_dict(), strict=False)
    for name in ("perms", "perm_x", "perm_y"):
        for i, p in enumerate(getattr(flow, name, [])):
            if isinstance(p, hint_amd.HouseholderPerm):
                getattr(twin, name)[i] = hint_amd.FixedOrthogonal([(p.d,)], W=p.matrix().clone()).to(DEV)
    return twin


def close(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(b).max())))


def block_grads(flow):
    return {k: p.grad.clone() for k, p in flow.named_parameters() if "perm" not in k}


def test_learned_flow_equals_the_fixed_route_and_vs_grad_follows_the_chain_rule():
    torch.manual_seed(0)
    flow = hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True).to(DEV)
    twin = fixed_twin(flow, lambda: hint_amd.HintFlow(20, 2, [32, 16]))
    x = torch.randn(64, 20, device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    za = flow(xa)
    Ja = flow.log_jacobian(run_forward=False)
    nll(za, Ja).backward()
    zb = twin(xb)
    Jb = twin.log_jacobian(run_forward=False)
    nll(zb, Jb).backward()
    close(za, zb)
    close(Ja, Jb)
    ga, gb = block_grads(flow), block_grads(twin)
    assert ga.keys() == gb.keys() and len(ga) > 0
    for k in ga:
        assert rel_err(ga[k].cpu().numpy(), gb[k].cpu().numpy()) < 1e-4, k
    assert rel_err(xa.grad.cpu().numpy(), xb.grad.cpu().numpy()) < 1e-4
    # dL/dW from torch autograd on the FixedOrthogonal flow, walking its modules; the statement's chain rule takes it to Vs
    Wc = twin.perms[1].W.detach().clone().requires_grad_(True)
    twin.perms[1].W = Wc
    twin.fuse_chain = False
    z = twin(x)
    nll(z, twin.log_jacobian(run_forward=False)).backward()
    want = ho.g_V_from_g_W(flow.perms[1].Vs.detach().cpu(), Wc.grad.cpu())
    e = rel_err(flow.perms[1].Vs.grad.cpu().numpy(), want.numpy())
    worst("flow_vs_grad_rel_err_over_1e-4", e / 1e-4)
    assert e < 1e-4, e


def test_learned_flow_with_reshuffle_blocks_and_a_first_permutation_walks_its_modules():
    """reshuffle=True blocks compose their node matrices with the flow's on the host, keyed on a version no kernel advances: a
    learned flow of such blocks walks its modules with gradients off as well, and equals the fixed route"""
    torch.manual_seed(5)
    kw = dict(perm_first=True, reshuffle=True)
    flow = hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True, **kw).to(DEV)
    twin = fixed_twin(flow, lambda: hint_amd.HintFlow(20, 2, [32, 16], **kw))
    x = torch.randn(64, 20, device=DEV)
    with torch.no_grad():
        for rev in (False, True):
            za, zb = flow(x, rev=rev), twin(x, rev=rev)
            assert flow._runner is None or 64 not in flow._runner._infer
            close(za, zb)
            close(flow.log_jacobian(run_forward=False), twin.log_jacobian(run_forward=False))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    nll(flow(xa), flow.log_jacobian(run_forward=False)).backward()
    nll(twin(xb), twin.log_jacobian(run_forward=False)).backward()
    assert rel_err(xa.grad.cpu().numpy(), xb.grad.cpu().numpy()) < 1e-4
    assert all(p.Vs.grad is not None and bool(torch.isfinite(p.Vs.grad).all()) for p in flow.perms)


def test_learned_conditional_flow_equals_the_fixed_route():
    torch.manual_seed(1)
    flow = hint_amd.ConditionalHintFlow(20, 2, 2, 32, learned_perms=True).to(DEV)
    twin = fixed_twin(flow, lambda: hint_amd.ConditionalHintFlow(20, 2, 2, 32))
    Wx = twin.perm_x[1].W.detach().clone().requires_grad_(True)
    Wy = twin.perm_y[1].W.detach().clone().requires_grad_(True)
    twin.perm_x[1].W, twin.perm_y[1].W = Wx, Wy
    x, y = torch.randn(64, 20, device=DEV), torch.randn(64, 2, device=DEV)
    res = []
    for f in (flow, twin):
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        zy, zx = f([yg, xg])
        J = f.log_jacobian(run_forward=False)
        (nll(zx, f.x_jac()) + nll(zy, J - f.x_jac())).backward()
        res.append((zy, zx, J, xg.grad, yg.grad))
    for a, b in zip(res[0][:3], res[1][:3]):
        close(a, b)
    for a, b in zip(res[0][3:], res[1][3:]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-4
    ga, gb = block_grads(flow), block_grads(twin)
    assert ga.keys() == gb.keys() and len(ga) > 0
    for k in ga:
        assert rel_err(ga[k].cpu().numpy(), gb[k].cpu().numpy()) < 1e-4, k
    for perm, Wc in ((flow.perm_x[1], Wx), (flow.perm_y[1], Wy)):
        want = ho.g_V_from_g_W(perm.Vs.detach().cpu(), Wc.grad.cpu())
        assert rel_err(perm.Vs.grad.cpu().numpy(), want.numpy()) < 1e-4
    # sampling and the x-lane density: the fused chains read the rebuilt matrices
    with torch.no_grad():
        zx = torch.randn(64, 20, device=DEV)
        for a, b in zip(flow.sample_conditional(y, zx), twin.sample_conditional(y, zx)):
            close(a, b)
        for a, b in zip(flow.x_lane_forward(x, y), twin.x_lane_forward(x, y)):
            close(a, b)


def test_inference_of_a_learned_flow_takes_the_fused_route_and_sees_clamp_adam():
    lib = _lib.load()
    torch.manual_seed(2)
    flow = hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True).to(DEV)
    x = torch.randn(64, 20, device=DEV)
    opt = hint_amd.ClampAdam(flow.parameters(), lr=1e-2, grad_clamp=5.0)
    before = None
    for step in range(2):
        with torch.no_grad():
            for rev in (False, True):
                flow.fuse_chain = True
                zf = flow(x, rev=rev)
                Jf = flow.log_jacobian(run_forward=False)
                assert lib.hint_debug_last_lds_bytes(0) > 0
                assert flow._runner is not None and 64 in flow._runner._infer        # the chained inference launch ran
                flow.fuse_chain = False
                zw = flow(x, rev=rev)
                Jw = flow.log_jacobian(run_forward=False)
                flow.fuse_chain = True
                close(zf, zw)
                close(Jf, Jw)
                if not rev:
                    if before is not None:
                        assert not torch.allclose(zf, before)          # the step moved Vs and the fused route saw it
                    before = zf.clone()
        if step == 0:
            z = flow(x)
            nll(z, flow.log_jacobian(run_forward=False)).backward()
            v0 = flow.perms[1].Vs.detach().clone()
            opt.step()
            assert not torch.equal(v0, flow.perms[1].Vs.detach())


def test_reference_loop_with_clamp_adam_trains_vs():
    """ten steps of train_unconditional.py:114-144's loop body over all parameters, Vs included: ClampAdam against
    clamp_ + torch.optim.Adam from the same start"""
    torch.manual_seed(4)
    a = hint_amd.HintFlow(6, 3, [32, 16], learned_perms=True).to(DEV)
    b = copy.deepcopy(a)
    xs = [torch.randn(256, 6, device=DEV) for _ in range(10)]
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)
    hist = []
    for model, fused in ((a, True), (b, False)):
        params = [p for p in model.parameters() if p.requires_grad]
        assert any(p is model.perms[1].Vs for p in params)
        optim = hint_amd.ClampAdam(params, grad_clamp=5.0, **kw) if fused else torch.optim.Adam(params, **kw)
        v0 = model.perms[1].Vs.detach().clone()
        losses = []
        for x in xs:
            optim.zero_grad()
            z = model(x)
            log_jacobian = model.log_jacobian(x, run_forward=False)
            batch_losses = [0.5 * torch.sum(z ** 2, dim=1).mean(), -log_jacobian.mean()]
            losses.append([l.item() for l in batch_losses])
            sum(batch_losses).backward()
            if not fused:
                for p in params:
                    p.grad.data.clamp_(-5.00, 5.00)
            optim.step()
        hist.append(np.array(losses))
        assert not torch.equal(v0, model.perms[1].Vs.detach())
        for i in (1, 2):
            W = model.perms[i].matrix().double()
            assert float((W @ W.t() - torch.eye(6, dtype=torch.float64, device=DEV)).abs().max()) < 1e-5
    np.testing.assert_allclose(hist[0], hist[1], rtol=1e-3, atol=0)


def test_trainers_refuse_trainable_permutations():
    with pytest.raises(HintAmdError, match="ClampAdam"):
        hint_amd.FlowTrainer(hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True).to(DEV))
    with pytest.raises(HintAmdError, match="ClampAdam"):
        hint_amd.ConditionalFlowTrainer(hint_amd.ConditionalHintFlow(20, 2, 2, 32, learned_perms=True).to(DEV))


# ---- one timing record, no threshold ----
def test_timing_record_against_the_torch_composition():
    d = n = 100
    B = 4096
    m = hint_amd.HouseholderPerm([(d,)], n_reflections=n, seed=9).to(DEV)
    V = m.Vs.detach().clone().requires_grad_(True)
    x = torch.randn(B, d, device=DEV)

    def ours():
        m.Vs.grad = None
        xg = x.detach().requires_grad_(True)
        (y,) = m([xg])
        y.sum().backward()

    def composed():
        V.grad = None
        xg = x.detach().requires_grad_(True)
        W = torch.eye(d, device=DEV)
        for i in range(n):
            v = V[i]
            W = W - torch.outer(W @ v, v) * (2.0 / torch.dot(v, v))
        (xg @ W).sum().backward()

    def median_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))
    ours(), composed()
    assert rel_err(m.Vs.grad.cpu().numpy(), V.grad.cpu().numpy()) < 1e-3
    rec = {"d": d, "n": n, "B": B, "householder_ms": median_ms(ours), "torch_composition_ms": median_ms(composed)}
    record("timing_forward_backward", rec)
    print(rec)
