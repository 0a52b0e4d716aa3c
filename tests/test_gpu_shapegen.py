"""hint_amd.sample_lens_prior / sample_lens_joint / lens_rings / lens_draws / fourier_coeffs on the GPU against
tests/shapegen_oracle.py (float64, the ring by Sutherland-Hodgman clipping) under that file's comparison rule, against the
reference's recorded fourier_coeffs outputs, and against themselves: Philox and explicit draws, chunking, grids, two runs,
rotations, guard-banded poisoned buffers, moments."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, shapes
from hint_amd._lib import HintAmdError
import shapegen_oracle as so
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
SEED = 0x5EED0123456789AB
N_BIG = 4099
HIGH = 2 ** 32 - 5                 # with n = 10 the row counter's high word changes inside the call
# (n, offset): the sizes around a wavefront's 64 rows, more than one workgroup, and the counter's carry
CASES = [(1, 0), (63, 1), (64, 0), (65, 64), (N_BIG, 0), (10, HIGH)]
CASE_IDS = [f"n{n}_off{o}" for n, o in CASES]
# the normals come from the hardware's log2 / sin / cos, as the training noise does: the bound tests/test_gpu_noise.py holds those to
NORMAL_BOUND = 2.0 ** -13
U = so.U


def cpu64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def reference():
    """{offset: (draws fp32 [n, 4] as the device made them, x64, ring64, counts, keep)} for every row any test compares: computed once"""
    out = {}
    for n, off in ((N_BIG, 0), (10, HIGH)):
        d = hint_amd.lens_draws(n, SEED, offset=off, device=DEV).cpu().numpy()
        x, ring, cnt = so.sample(d)
        out[off] = (d, x, ring, cnt, ~so.ambiguous(d))
    return out


def ref_rows(reference, n, off):
    base = HIGH if off >= HIGH else 0
    return tuple(v[off - base:off - base + n] for v in reference[base])


def test_draws_are_the_oracles_philox(reference):
    for off, n in ((0, N_BIG), (HIGH, 10)):
        d = reference[off][0]
        ur, ut = so.uniforms(SEED, off, n)
        assert (d[:, 0] == ur).all() and (d[:, 1] == ut).all()               # exact: part of the definition
        want = so.draws(SEED, off, n)
        err = float(np.abs(d[:, 2:] - want[:, 2:]).max())
        print(f"offset {off}: normals differ from float64 Box-Muller by at most {err:.3e} (bound {NORMAL_BOUND:.2e})")
        assert err <= NORMAL_BOUND
    assert (reference[0][0][:10] != reference[HIGH][0]).any()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_philox_path_and_explicit_draws_give_equal_bits(case):
    n, off = case
    x, ring, cnt = hint_amd.sample_lens_prior(n, SEED, offset=off, device=DEV, return_ring=True)
    d = hint_amd.lens_draws(n, SEED, offset=off, device=DEV)
    x2, ring2, cnt2 = hint_amd.sample_lens_prior(n, 0, draws=d, return_ring=True)
    assert x.shape == (n, 20) and ring.shape == (n, 32, 2) and cnt.shape == (n,) and cnt.dtype == torch.int32
    assert bits_equal(x, x2) and bits_equal(ring, ring2) and torch.equal(cnt, cnt2)
    r3, c3 = hint_amd.lens_rings(d)
    assert bits_equal(ring, r3) and torch.equal(cnt, c3)
    assert bits_equal(x, hint_amd.sample_lens_prior(n, SEED, offset=off, device=DEV))      # ... and with no ring asked for
    assert torch.isfinite(x).all()


def test_chunks_grids_and_two_runs_give_equal_bits():
    whole = hint_amd.sample_lens_prior(N_BIG, SEED, device=DEV)
    parts = [hint_amd.sample_lens_prior(n, SEED, offset=o, device=DEV) for n, o in ((1, 0), (63, 1), (4035, 64))]
    assert bits_equal(whole, torch.cat(parts))
    assert bits_equal(whole, hint_amd.sample_lens_prior(N_BIG, SEED, device=DEV))
    for groups in (1, 3):
        res = shapes._lens_run(N_BIG, SEED, 0, torch.device(DEV), None, ["x", "ring", "counts"], max_groups=groups)
        assert bits_equal(whole, res["x"]), groups
    high = hint_amd.sample_lens_prior(10, SEED, offset=HIGH, device=DEV)
    parts = [hint_amd.sample_lens_prior(n, SEED, offset=o, device=DEV) for n, o in ((5, HIGH), (5, 2 ** 32))]
    assert bits_equal(high, torch.cat(parts))
    assert not bits_equal(high, whole[:10])
    assert not bits_equal(whole, hint_amd.sample_lens_prior(N_BIG, SEED + 1, device=DEV))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_ring_counts_and_coefficients_against_the_oracle(case, reference):
    n, off = case
    d, x64, ring64, cnt64, keep = ref_rows(reference, n, off)
    x, ring, cnt = hint_amd.sample_lens_prior(n, SEED, offset=off, device=DEV, return_ring=True)
    x, ring, cnt = cpu64(x), cpu64(ring), cnt.cpu().numpy()
    left_out = float((~keep).mean())
    assert left_out <= so.MAX_AMBIGUOUS, left_out
    assert set(cnt.tolist()) <= {31, 32}
    assert (cnt[keep] == cnt64[keep]).all()
    if n == N_BIG:
        assert set(cnt.tolist()) == {31, 32}                # both twiddle tables are exercised
    A = so.scale(ring64)
    e_ring = np.abs(ring - ring64).reshape(n, -1).max(axis=1) / (U * A)
    e_x = np.abs(x - x64).max(axis=1) / (U * A)
    print(f"n {n} offset {off}: {int((~keep).sum())} ambiguous rows left out; worst ring error {e_ring[keep].max():.1f} u A "
          f"(bound {so.K_RING}), worst coefficient error {e_x[keep].max():.1f} u A (bound {so.K_COEF})")
    assert (e_ring[keep] <= so.K_RING).all() and (e_x[keep] <= so.K_COEF).all()
    for i in range(n):                                      # zero padding behind the closed ring
        assert (ring[i, cnt[i]:] == 0).all()


def test_rotating_theta_rotates_the_coefficients():
    """theta + 2 pi k / 64 maps A onto itself and turns B, the lens and its ring clockwise by that angle: every coefficient pair
    (axis 0, axis 1) turns with it.  Needs no oracle."""
    g = torch.Generator().manual_seed(3)
    n = 257
    ur = torch.rand(n, generator=g)
    ut = torch.randint(0, 2048, (n,), generator=g).float() / 4096.0          # in [0, 0.5), on a grid: u_t + k / 64 is exact
    d0 = torch.stack([ur, ut, torch.zeros(n), torch.zeros(n)], dim=1).to(DEV)
    x0, ring0, cnt0 = hint_amd.sample_lens_prior(n, 0, draws=d0, return_ring=True)
    A = cpu64(ring0).reshape(n, -1).__abs__().max(axis=1)
    x0 = cpu64(x0).reshape(n, 2, 2, 5)                                        # [row, re | im, axis, m]
    for k in (1, 5, 17, 31):
        d = d0.clone()
        d[:, 1] += k / 64.0
        x, ring, cnt = hint_amd.sample_lens_prior(n, 0, draws=d, return_ring=True)
        assert torch.equal(cnt, cnt0)
        phi = 2 * np.pi * k / 64
        R = np.array([[np.cos(phi), np.sin(phi)], [-np.sin(phi), np.cos(phi)]])
        want = np.einsum("ab,npbm->npam", R, x0)
        err = np.abs(cpu64(x).reshape(n, 2, 2, 5) - want).reshape(n, -1).max(axis=1) / (U * A)
        print(f"k {k}: worst {err.max():.1f} u A (bound {2 * so.K_COEF})")
        assert (err <= 2 * so.K_COEF).all()


def fixture(name):
    f = np.load(os.path.join(GOLDEN, name + ".npz"))
    return f["points"], f["counts"], {5: f["ref5"], 25: f["ref25"]}


def check_fcoef(pts, cnt, k, want, what):
    x = hint_amd.fourier_coeffs(torch.from_numpy(pts.astype(np.float32)).to(DEV), k,
                                None if cnt is None else torch.from_numpy(cnt).to(DEV))
    assert x.shape == (len(pts), 4 * k) and x.dtype == torch.float32
    counts = np.full(len(pts), pts.shape[1]) if cnt is None else cnt
    for i, c in enumerate(counts):
        err = np.abs(cpu64(x[i]) - want[i]).max() / (U * np.abs(pts[i, :c]).max())
        assert err <= so.k_fcoef(c), (what, k, i, int(c), err)
    return x


@pytest.mark.parametrize("k", (5, 25))
def test_fourier_coeffs_against_the_reference(k):
    rings, rc, rref = fixture("fcoef_rings")
    check_fcoef(rings, rc, k, rref[k], "rings, ragged 31 | 32")
    outl, oc, oref = fixture("fcoef_outlines")
    assert outl.shape[1] == 300 and len(set(oc.tolist())) == len(oc)
    check_fcoef(outl, oc, k, oref[k], "outlines, ragged 100..300")
    wide = np.full((len(outl), 1024, 2), np.nan)            # P_max = 1024; what lies behind a row's count is never read
    for i, c in enumerate(oc):
        wide[i, :c] = outl[i, :c]
    a = check_fcoef(wide, oc, k, oref[k], "outlines in P_max = 1024")
    b = hint_amd.fourier_coeffs(torch.from_numpy(outl.astype(np.float32)).to(DEV), k, torch.from_numpy(oc).to(DEV))
    assert bits_equal(a, b)                                  # a row does not depend on P_max
    # every row of one length, no counts; count == n_coeffs; a full row of 1024 (the oracle's DFT is held to the reference at 1e-12)
    same = outl[:, :100]
    check_fcoef(same, None, k, so.coeffs(same, np.full(len(same), 100), k), "no counts")
    few = np.full(len(outl), k, dtype=np.int32)
    check_fcoef(outl, few, k, so.coeffs(outl, few, k), "count == n_coeffs")
    rng = np.random.RandomState(8)
    full = rng.randn(3, 1024, 2).astype(np.float32).astype(np.float64)
    check_fcoef(full, None, k, so.coeffs(full, np.full(3, 1024), k), "1024 points")


def test_fourier_coeffs_of_the_lens_ring_is_the_samplers_x():
    x, ring, cnt = hint_amd.sample_lens_prior(300, SEED, device=DEV, return_ring=True)
    y = hint_amd.fourier_coeffs(ring, 5, cnt)
    A = cpu64(ring).reshape(300, -1).__abs__().max(axis=1)
    err = np.abs(cpu64(x) - cpu64(y)).max(axis=1) / (U * A)
    assert (err <= 2 * so.k_fcoef(32)).all(), err.max()      # each within k_fcoef of the exact coefficients of the same ring


def test_joint_sample_is_the_simulator_on_the_prior_sample(reference):
    noise = 0.05
    x, y, eps = hint_amd.sample_lens_joint(N_BIG, SEED, noise, device=DEV, return_eps=True)
    assert y.shape == (N_BIG, 2) and eps.shape == (N_BIG, 2)
    assert bits_equal(y, hint_amd.lens_forward_process(x, noise, eps=eps))
    assert bits_equal(x, hint_amd.sample_lens_prior(N_BIG, SEED, device=DEV))
    x2, y2 = hint_amd.sample_lens_joint(N_BIG, SEED, noise, device=DEV)
    assert bits_equal(x, x2) and bits_equal(y, y2)
    assert float(np.abs(cpu64(eps) - so.eps_draws(SEED, 0, N_BIG)).max()) <= NORMAL_BOUND
    xa, ya, ea = hint_amd.sample_lens_joint(63, SEED, noise, offset=1, device=DEV, return_eps=True)
    assert bits_equal(xa, x[1:64]) and bits_equal(ea, eps[1:64]) and bits_equal(ya, y[1:64])
    assert not bits_equal(y, hint_amd.lens_forward_process(x, 0.0))


def lens_desc_run(n, seed, off, draws, gx, gring, gcnt, geps, gdraws, gws, nbytes):
    lib = _lib.load()
    desc = _lib.LensGenDesc()
    desc.n_rows, desc.seed, desc.offset, desc.max_groups = n, seed, off, 0
    desc.draws = draws
    desc.x, desc.ring, desc.counts, desc.eps, desc.draws_out = gx.ptr, gring.ptr, gcnt.ptr, geps.ptr, gdraws.ptr
    desc.workspace, desc.workspace_bytes = gws.ptr, nbytes
    _lib.check(lib.hint_lensgen_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_lensgen_run")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ("philox", "draws"))
def test_lensgen_writes_every_promised_element_and_nothing_beyond(mode):
    """hint_lensgen_run on guard-banded buffers filled with zeros, NaNs or junk, a ragged last tile: the same bits every time (so
    every element of every output and of the workspace is written), guards intact, the draws unchanged"""
    lib = _lib.load()
    n = 64 * 5 + 37
    nbytes = lib.hint_lensgen_workspace_bytes(n)
    gd = Guarded(4 * n).set(hint_amd.lens_draws(n, SEED, device=DEV))
    sd = gd.snapshot()
    first = None
    for rep, fill in enumerate(("zero",) + FILLS):
        bufs = [Guarded(20 * n, fill=fill, seed=rep), Guarded(64 * n, fill=fill, seed=10 + rep),
                Guarded(n, fill=fill, seed=20 + rep, dtype=torch.int32), Guarded(2 * n, fill=fill, seed=30 + rep),
                Guarded(4 * n, fill=fill, seed=40 + rep), Guarded(nbytes // 4, fill=fill, seed=50 + rep, dtype=torch.int32)]
        lens_desc_run(n, SEED, 0, gd.ptr if mode == "draws" else None, *bufs, nbytes)
        for b, name in zip(bufs, ("x", "ring", "counts", "eps", "draws_out", "workspace")):
            b.check_guards(f"{mode}, {fill}: {name}")
        gd.check_unchanged(sd, f"{mode}, {fill}: draws")
        now = [b.words.clone() for b in bufs]
        if first is None:
            first = now
        for a, b, name in zip(now, first, ("x", "ring", "counts", "eps", "draws_out", "workspace")):
            assert torch.equal(a, b), (mode, fill, name)
    x, ring, cnt = hint_amd.sample_lens_prior(n, SEED, device=DEV, return_ring=True)
    assert torch.equal(first[0], x.reshape(-1).view(torch.int32)) and torch.equal(first[1], ring.reshape(-1).view(torch.int32))
    assert torch.equal(first[2], cnt) and int(first[5].sum()) == 0
    assert torch.equal(first[4], gd.words)


def test_fcoef_writes_every_promised_element_and_nothing_beyond():
    lib = _lib.load()
    outl, oc, _ = fixture("fcoef_outlines")
    n, p, k = len(outl), outl.shape[1], 25
    gp = Guarded(2 * n * p, align=16).set(torch.from_numpy(outl.astype(np.float32)))
    gc = Guarded(n, dtype=torch.int32).set(torch.from_numpy(oc))
    sp, sc = gp.snapshot(), gc.snapshot()
    nbytes = lib.hint_fcoef_workspace_bytes(n, p, k)
    first = None
    for rep, fill in enumerate(("zero",) + FILLS):
        gx, gw = Guarded(4 * k * n, fill=fill, seed=rep, align=16), Guarded(nbytes // 4, fill=fill, seed=9 + rep, dtype=torch.int32)
        desc = _lib.FcoefDesc()
        desc.points, desc.counts, desc.n_rows, desc.p_max, desc.n_coeffs = gp.ptr, gc.ptr, n, p, k
        desc.x, desc.workspace, desc.workspace_bytes, desc.max_groups = gx.ptr, gw.ptr, nbytes, 0
        _lib.check(lib.hint_fcoef_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_fcoef_run")
        torch.cuda.synchronize()
        gx.check_guards(f"{fill}: x")
        gw.check_guards(f"{fill}: workspace")
        gp.check_unchanged(sp, f"{fill}: points")
        gc.check_unchanged(sc, f"{fill}: counts")
        now = (gx.words.clone(), gw.words.clone())
        first = first or now
        assert torch.equal(now[0], first[0]) and torch.equal(now[1], first[1]), fill
    x = hint_amd.fourier_coeffs(torch.from_numpy(outl.astype(np.float32)).to(DEV), k, torch.from_numpy(oc).to(DEV))
    assert torch.equal(first[0], x.reshape(-1).view(torch.int32)) and int(first[1].sum()) == 0


def test_rows_outside_the_definition_are_refused():
    d = hint_amd.lens_draws(100, SEED, device=DEV)
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        for col in ((0, 1, 2, 3) if bad != bad or bad == float("inf") else (0, 1)):
            e = d.clone()
            e[41, col] = bad
            with pytest.raises(HintAmdError, match="1 row"):
                hint_amd.sample_lens_prior(100, 0, draws=e)
    # the rejected row is NaN and disturbs no other row
    e = d.clone()
    e[41, 1] = 1.5
    res = shapes._lens_run(100, 0, 0, torch.device(DEV), None, ["x", "counts"])
    with pytest.raises(HintAmdError):
        shapes._lens_run(100, 0, 0, torch.device(DEV), e, ["x"])
    lib = _lib.load()
    x = torch.zeros(100, 20, device=DEV)
    cnt = torch.full((100,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.hint_lensgen_workspace_bytes(100), dtype=torch.uint8, device=DEV)
    desc = _lib.LensGenDesc()
    desc.n_rows, desc.draws, desc.x, desc.counts = 100, e.data_ptr(), x.data_ptr(), cnt.data_ptr()
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.hint_lensgen_run(C.byref(desc), torch.cuda.current_stream().cuda_stream), "hint_lensgen_run")
    good = hint_amd.sample_lens_prior(100, 0, draws=d)
    keep = torch.arange(100, device=DEV) != 41
    assert torch.isnan(x[41]).all() and int(cnt[41]) == 0 and int(ws.view(torch.int32).sum()) == 1
    assert bits_equal(x[keep], good[keep]) and res["x"].shape == (100, 20)
    pts = torch.randn(6, 40, 2, device=DEV)
    for bad in (4, 41, 0, -1):
        c = torch.full((6,), 40, dtype=torch.int32, device=DEV)
        c[2] = bad
        with pytest.raises(HintAmdError, match="1 row"):
            hint_amd.fourier_coeffs(pts, 5, c)


def test_moments_of_the_dc_coefficient_on_a_million_rows():
    """a[c, 0] = -0.5 n_c up to rounding: mean 0 and variance 1 / 4, within 5 standard errors"""
    n = 10 ** 6
    x = hint_amd.sample_lens_prior(n, SEED + 7, device=DEV)
    assert torch.isfinite(x).all()
    for col in (2, 7):
        v = x[:, col].double()
        mean, var = float(v.mean()), float(v.var())
        print(f"a[{col // 5}, 0]: mean {mean:.3e} (5 se {5 * 0.5 / np.sqrt(n):.3e}), variance {var:.6f} (0.25 +- {5 * 0.25 * np.sqrt(2.0 / n):.6f})")
        assert abs(mean) <= 5 * 0.5 / np.sqrt(n)
        assert abs(var - 0.25) <= 5 * 0.25 * np.sqrt(2.0 / n)
    assert float(x[:, [12, 17]].abs().max()) <= 1e-5         # the DC coefficient is real
