"""The lens-shape prior sampler as a specification, in numpy.  TEST INFRASTRUCTURE - nothing here is imported by the library.

The definition (include/hint_amd.h hint_lensgen_desc).  A row has four draws, u_r, u_t in [0, 1] and n_x, n_y:
    r0 = 1 + u_r, r1 = 2 r0, theta = 2 pi u_t, D = 0.8 (r0 + r1), c1 = D (sin theta, cos theta)            (data.py:87-93)
    e_j = (cos(2 pi j / 64), -sin(2 pi j / 64)), A_j = r0 e_j, B_j = c1 + r1 e_j, j = 0..63: two clockwise 64-gons
    ring = P, the A_j strictly inside B (clockwise), Q, the B_j strictly inside A (clockwise), P again   (closed: data.py:98)
    ring -= mean(closed ring) + 0.5 (n_x, n_y)                                                           (data.py:99)
    a[c, m] = (1 / N) sum_n ring[n, c] exp(-2 pi i m n / N), m = -2..2, N the closed count               (data.py:42-49)
    x = [Re a[0, :], Re a[1, :], Im a[0, :], Im a[1, :]]                                                 (data.py:30-33)
The order of the ring's vertices is this project's own definition (the reference takes whatever its polygon library returns).

The ring is built here by an algorithm that shares nothing with the kernel's: Sutherland-Hodgman clipping of A by the 64
half-planes of B, then rotated to start at P.  The kernel classifies vertices from the polygons' regularity instead.

Draws: Philox4x32-10 as tests/noise_oracle.py states it, counter = {row lo, row hi, stream, 0x4C454E53}, key = {seed lo, seed hi},
row = offset + i.  Stream 0: u_r = (float)c0 2^-32, u_t = (float)c1 2^-32, (n_x, n_y) = one Box-Muller call on
(min(((float)c2 + 1) 2^-32, 1), (float)c3 2^-32).  Stream 1: the observation noise eps, the Box-Muller pair of (c0, c1).

THE COMPARISON RULE.  u = 2^-24, the relative error of one fp32 rounding; lengths below are in units of r0 (the figure scales
with r0, and the kernel builds it at r0 = 1).
  classification  a vertex v of one polygon is inside the other when s = max_k n_k . (v - centre) - R apothem < 0.  In fp32: sin
      and cos of theta within 2 ulp = 4 u, times 2.4 (a rounded constant, a rounded product): the centre is off by
      2.4 (4 + 1 + 1) u = 14.4 u; v - centre adds the vertex's own u and the rounding of a value below 3.4: 14.4 + 1 + 3.4 = 18.8 u;
      the dot product with a unit normal (each entry off by u) adds the normal's error on 3.4 and two roundings of values below
      3.4: 18.8 + 3.4 + 6.8 = 29 u; less the rounded apothem term (2 u): 31 u.  MARGIN = 32 u = 2^-19: a row with any
      |s| < MARGIN r0 is AMBIGUOUS and is not compared (one vertex more or fewer shifts every later index).  At most 1 % of a
      test's rows may be ambiguous; the tests assert it.
  ring            an A vertex u; a B vertex 14.4 + 2 + 1.1 = 17.5 u; a crossing point X = V0 + t (V1 - V0), t = s0 / (s0 - s1):
      s0, s1 are off by 32 u each and s0 - s1 is at least 0.091 (an edge of A, 0.0981 long, meets B's edge within 22 degrees of
      its normal), so t is off by 32 u / 0.091 = 352 u and X by 352 u x 0.0981 + 1 u + 1 u = 37 u.
      mean: 32 terms with partial sums below 32 x 1.1 = 35, 31 roundings of at most 35 u, divided by 32: 34 u; the points' own
      errors average (20 x 1 + 9 x 17.5 + 3 x 37) / 32 = 9 u; the division 1 u: 44 u.
      centred point = r0 (p - mean) - n / 2: 37 + 44 + 1.2 (the difference) + 1.2 (the fused product and sum) = 84 u in units
      of r0.  A centred lens has a coordinate of magnitude 0.55 r0 at least (its long axis is 1.636 r0, seen at 45 degrees at
      worst), so r0 <= 1.82 A:  K_RING = 84 x 1.82 = 153.
  coefficients    the mean of N products of centred points with twiddles, accumulated by fused multiply-adds: the points' 153 u A
      and, per sum, N u A of accumulation (N <= 32), u A of the twiddles' rounding and u A of the division: K_COEF = 153 + 34 = 187.
  fourier_coeffs on given points has the last line only: K_FCOEF(count) = count + 2, in units of u A.
A is the row's largest centred coordinate magnitude.  These bounds are derived, never tuned on device output; fp32_floor()
evaluates the definition's formulas in numpy float32 (direct_rings) and tests/test_shapegen_cpu.py asserts that this floor lies inside them."""
import numpy as np

from noise_oracle import MASK, philox4x32_10  # noqa: F401

TAG = 0x4C454E53            # counter word 3: "LENS"
SIDES = 64
U = 2.0 ** -24
MARGIN = 32 * U
K_RING, K_COEF = 153.0, 187.0
N_COEFFS = 5
COUNT_RANGE = (30, 31)      # open ring; test_shapegen_cpu.py establishes it by a sweep
MAX_AMBIGUOUS = 0.01


def k_fcoef(count):
    return count + 2.0


# ---- draws ----
def philox_words(seed: int, offset: int, n: int, stream: int):
    seed = int(seed) & (2 ** 64 - 1)
    row = (int(offset) + np.arange(n, dtype=np.uint64)) if n else np.zeros(0, np.uint64)
    c = philox4x32_10((row & MASK, row >> np.uint64(32), stream, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    return [w.astype(np.float32) for w in c]              # (float)c: round to nearest even


def _box_muller(f0, f1, dtype):
    one, scale = np.float32(1.0), np.float32(2.0 ** -32)
    u0 = np.minimum((f0 + one) * scale, one).astype(dtype)
    u1 = (f1 * scale).astype(dtype)
    r, a = np.sqrt(dtype(-2.0) * np.log(u0)), dtype(2.0 * np.pi) * u1
    return r * np.cos(a), r * np.sin(a)


def uniforms(seed: int, offset: int, n: int):
    """(u_r, u_t): exact fp32 values, part of the definition"""
    f = philox_words(seed, offset, n, 0)
    s = np.float32(2.0 ** -32)
    return f[0] * s, f[1] * s


def draws(seed: int, offset: int, n: int, dtype=np.float64):
    """[n, 4] = (u_r, u_t, n_x, n_y); the normals evaluated in `dtype` from the fp32 uniforms"""
    dtype = np.dtype(dtype).type
    f = philox_words(seed, offset, n, 0)
    s = np.float32(2.0 ** -32)
    nx, ny = _box_muller(f[2], f[3], dtype)
    return np.stack([(f[0] * s).astype(dtype), (f[1] * s).astype(dtype), nx, ny], axis=1)


def eps_draws(seed: int, offset: int, n: int, dtype=np.float64):
    """[n, 2]: the observation noise of sample_lens_joint"""
    f = philox_words(seed, offset, n, 1)
    ex, ey = _box_muller(f[0], f[1], np.dtype(dtype).type)
    return np.stack([ex, ey], axis=1)


# ---- geometry ----
def _unit(dtype):
    j = np.arange(SIDES)
    return np.stack([np.cos(2 * np.pi * j / SIDES), -np.sin(2 * np.pi * j / SIDES)], axis=1).astype(dtype)


def _normals(dtype):
    """outward unit normal of edge k (from vertex k to vertex k + 1) and the apothem of the unit polygon"""
    k = np.arange(SIDES) + 0.5
    return (np.stack([np.cos(2 * np.pi * k / SIDES), -np.sin(2 * np.pi * k / SIDES)], axis=1).astype(dtype),
            dtype(np.cos(np.pi / SIDES)))


def polygons(d, dtype=np.float64):
    """d [n, >= 2] -> r0 [n], A [n, 64, 2], B [n, 64, 2], c1 [n, 2]"""
    dtype = np.dtype(dtype).type
    d = np.asarray(d)
    ur, ut = d[:, 0].astype(dtype), d[:, 1].astype(dtype)
    r0 = dtype(1.0) + ur
    r1 = dtype(2.0) * r0
    theta = dtype(2.0 * np.pi) * ut
    D = dtype(0.8) * (r0 + r1)
    c1 = np.stack([D * np.sin(theta), D * np.cos(theta)], axis=1)
    e = _unit(dtype)
    return r0, r0[:, None, None] * e[None], c1[:, None, :] + r1[:, None, None] * e[None], c1


def classify(d, chunk=4096):
    """brute force, float64: inside_A [n, 64] (A_j strictly inside B), inside_B [n, 64], slack [n] = the smallest |s| / r0"""
    d = np.asarray(d, dtype=np.float64)
    nrm, apo = _normals(np.float64)
    ia, ib, sl = [], [], []
    for i in range(0, len(d), chunk):
        r0, A, B, c1 = polygons(d[i:i + chunk])
        sa = np.max((A - c1[:, None, :]) @ nrm.T, axis=2) - apo * 2.0 * r0[:, None]      # A's vertices against B
        sb = np.max(B @ nrm.T, axis=2) - apo * r0[:, None]                                # B's vertices against A
        ia.append(sa < 0)
        ib.append(sb < 0)
        sl.append(np.minimum(np.abs(sa).min(axis=1), np.abs(sb).min(axis=1)) / r0)
    return np.concatenate(ia), np.concatenate(ib), np.concatenate(sl)


def open_counts(d):
    ia, ib, _ = classify(d)
    return ia.sum(axis=1) + ib.sum(axis=1) + 2


def ambiguous(d):
    return classify(d)[2] < MARGIN


def clip_ring(A, B, c1, r1, dtype=np.float64):
    """one row: the closed ring of A n B by Sutherland-Hodgman, starting at P; [count + 1, 2]"""
    dtype = np.dtype(dtype).type
    nrm, apo = _normals(dtype)
    h = apo * r1
    poly = A.copy()
    s_all = (A - c1) @ nrm.T - h                           # [64 vertices, 64 half-planes]
    for k in np.nonzero((s_all > 0).any(axis=0))[0]:       # a half-plane that cuts no vertex of A cuts nothing of a part of A
        s = (poly - c1) @ nrm[k] - h
        nxt, sn = np.roll(poly, -1, axis=0), np.roll(s, -1)
        cross = (s < 0) != (sn < 0)
        den = np.where(cross, s - sn, dtype(1.0))
        both = np.stack([poly, poly + (s / den)[:, None] * (nxt - poly)], axis=1)       # [vertex, (itself | its edge's crossing)]
        poly = both[np.stack([s < 0, cross], axis=1)]
    is_a = (poly[:, None, :] == A[None, :, :]).all(axis=2).any(axis=1)     # (kept vertices of A pass through bit for bit)
    first = np.nonzero(is_a & ~np.roll(is_a, 1))[0]
    assert len(first) == 1, "the vertices of A inside B are one cyclic run"
    p = (first[0] - 1) % len(poly)
    poly = np.roll(poly, -p, axis=0)
    return np.concatenate([poly, poly[:1]], axis=0)


def rings(d, dtype=np.float64):
    """d [n, 4] -> (ring [n, 32, 2] closed, centred and noised, zero-padded; counts [n] closed)"""
    dt = np.dtype(dtype).type
    d = np.asarray(d)
    r0, A, B, c1 = polygons(d, dtype)
    out = np.zeros((len(d), 32, 2), dtype=dtype)
    cnt = np.zeros(len(d), dtype=np.int32)
    for i in range(len(d)):
        ring = clip_ring(A[i], B[i], c1[i], dt(2.0) * r0[i], dtype)
        assert len(ring) <= 32
        ring = ring - (ring.mean(axis=0, dtype=dtype) + dt(0.5) * d[i, 2:4].astype(dtype))
        out[i, :len(ring)] = ring
        cnt[i] = len(ring)
    return out, cnt


def direct_rings(d, dtype=np.float64):
    """section 1's formulas as they stand, in `dtype`, vectorised: the float64 classification picks the vertices, the crossing
    points come from the two crossing edge pairs.  Same result as rings() (the CPU test holds the two together in float64); in
    float32 it is the fp32 floor of the definition"""
    dt = np.dtype(dtype).type
    d = np.asarray(d)
    n = len(d)
    ia, ib, _ = classify(d)
    r0, A, B, c1 = polygons(d, dtype)
    nrm, apo = _normals(dt)
    rows = np.arange(n)
    jlo, klo = np.argmax(ia & ~np.roll(ia, 1, axis=1), axis=1), np.argmax(ib & ~np.roll(ib, 1, axis=1), axis=1)
    nA, nB = ia.sum(axis=1), ib.sum(axis=1)

    def crossing(j0, k):                                   # A's edge (j0, j0 + 1) with the line of B's edge (k, k + 1)
        v0, v1, nk = A[rows, j0 % SIDES], A[rows, (j0 + 1) % SIDES], nrm[k % SIDES]
        h = apo * dt(2.0) * r0
        s0, s1 = ((v0 - c1) * nk).sum(axis=1) - h, ((v1 - c1) * nk).sum(axis=1) - h
        return v0 + (s0 / (s0 - s1))[:, None] * (v1 - v0)

    P, Q = crossing(jlo - 1, klo + nB - 1), crossing(jlo + nA - 1, klo - 1)
    out = np.zeros((n, 32, 2), dtype=dtype)
    cnt = (nA + nB + 3).astype(np.int32)
    pos = np.arange(32)[None, :]
    ja, kb = (jlo[:, None] + pos - 1) % SIDES, (klo[:, None] + pos - 2 - nA[:, None]) % SIDES
    out = np.where((pos >= 1)[..., None] & (pos <= nA[:, None])[..., None], A[rows[:, None], ja], out)
    out = np.where((pos >= nA[:, None] + 2)[..., None] & (pos <= (nA + nB)[:, None] + 1)[..., None], B[rows[:, None], kb], out)
    out = np.where((pos == nA[:, None] + 1)[..., None], Q[:, None, :], out)
    out = np.where(((pos == 0) | (pos == (cnt - 1)[:, None]))[..., None], P[:, None, :], out)
    valid = (pos < cnt[:, None])[..., None]
    mean = out.sum(axis=1, dtype=dtype) / cnt[:, None].astype(dtype)
    out = np.where(valid, out - (mean + dt(0.5) * d[:, 2:4].astype(dtype))[:, None, :], dt(0.0))
    return out.astype(dtype), cnt


HALF_A, HALF_B = np.float32(9.7598), np.float32(4.2937)


def window_runs(d):
    """THE KERNEL'S classification rule (hint_shapegen.hip), restated in numpy float32 so that the CPU suite can hold it to the
    brute-force one: each end of each run is settled among four candidate vertices around the circles' crossing, each tested
    against the half-planes around the one the crossing points at.  -> (jlo, nA, klo, nB, ok)"""
    f = np.float32
    d = np.asarray(d, dtype=np.float32)
    h = np.arange(128)
    hs = np.stack([np.cos(2 * np.pi * h / 128), -np.sin(2 * np.pi * h / 128)], axis=1).astype(np.float32)
    apo = f(np.cos(np.pi / 64))
    ut = d[:, 1]
    c = f(2.4) * np.stack([np.sin(2 * np.pi * ut.astype(np.float64)), np.cos(2 * np.pi * ut.astype(np.float64))], axis=1).astype(np.float32)
    js = f(64.0) * ut - f(16.0)
    ks = js + f(32.0)
    fa_lo, fa_hi = np.floor(js - HALF_A).astype(np.int64), np.floor(js + HALF_A).astype(np.int64)
    fb_lo, fb_hi = np.floor(ks - HALF_B).astype(np.int64), np.floor(ks + HALF_B).astype(np.int64)

    def slack(v, e0, w, r_apo):
        m = np.full(len(v), -np.inf, dtype=np.float32)
        for i in range(-(w // 2), w // 2 + 1):
            nk = hs[2 * ((e0 + i) & 63) + 1]
            m = np.maximum(m, nk[:, 1] * v[:, 1] + nk[:, 0] * v[:, 0])
        return m - r_apo

    a_out = a_in = b_out = b_in = 0
    for i in range(4):
        a_out = a_out + ~(slack(hs[2 * ((fa_lo - 1 + i) & 63)] - c, fb_hi, 3, f(2) * apo) < 0)
        a_in = a_in + (slack(hs[2 * ((fa_hi - 1 + i) & 63)] - c, fb_lo, 3, f(2) * apo) < 0)
        b_out = b_out + ~(slack(f(2) * hs[2 * ((fb_lo - 1 + i) & 63)] + c, fa_hi, 5, apo) < 0)
        b_in = b_in + (slack(f(2) * hs[2 * ((fb_hi - 1 + i) & 63)] + c, fa_lo, 5, apo) < 0)
    jlo, jhi, klo, khi = fa_lo - 1 + a_out, fa_hi - 2 + a_in, fb_lo - 1 + b_out, fb_hi - 2 + b_in
    nA, nB = jhi - jlo + 1, khi - klo + 1
    ok = np.ones(len(d), dtype=bool)
    for v in (a_out, a_in, b_out, b_in):
        ok &= (v >= 1) & (v <= 3)
    ok &= (nA + nB + 2 >= COUNT_RANGE[0]) & (nA + nB + 2 <= COUNT_RANGE[1])
    return jlo & 63, nA, klo & 63, nB, ok


def dft(points, n_coeffs, dtype=np.float64):
    """one row: points [count, 2] -> the 4 n_coeffs floats of flatten_coeffs(fourier_coeffs(points, n_coeffs)), written from the
    definition with the angle reduced in integers"""
    dt = np.dtype(dtype).type
    N = len(points)
    ms = np.arange(-(n_coeffs // 2), n_coeffs // 2 + 1)
    r = (ms[None, :] * np.arange(N)[:, None]) % N
    ang = (2.0 * np.pi * r / N)
    cs, sn = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
    p = np.asarray(points, dtype=dtype)
    re = (p[:, :, None] * cs[:, None, :]).sum(axis=0, dtype=dtype) / dt(N)
    im = -(p[:, :, None] * sn[:, None, :]).sum(axis=0, dtype=dtype) / dt(N)
    return np.concatenate([re.reshape(-1), im.reshape(-1)])


def coeffs(ring, counts, n_coeffs=N_COEFFS, dtype=np.float64):
    return np.stack([dft(ring[i, :counts[i]], n_coeffs, dtype) for i in range(len(ring))])


def sample(d, dtype=np.float64):
    """d [n, 4] -> (x [n, 20], ring, counts)"""
    ring, cnt = rings(d, dtype)
    return coeffs(ring, cnt, N_COEFFS, dtype), ring, cnt


def scale(ring):
    """A per row: the largest centred coordinate magnitude"""
    return np.abs(ring).reshape(len(ring), -1).max(axis=1)


def fp32_floor(d):
    """the same formulas in numpy float32 against float64 on the unambiguous rows of d: (worst ring error / (u A), worst
    coefficient error / (u A), rows compared).  Rows whose float32 clip disagrees in count are ambiguous by definition"""
    d = np.asarray(d, dtype=np.float32)
    keep = ~ambiguous(d)
    x64, r64, c64 = sample(d[keep], np.float64)
    r32, c32 = direct_rings(d[keep], np.float32)
    assert (c64 == c32).all()
    x32 = coeffs(r32, c32, N_COEFFS, np.float32)
    A = scale(r64)
    return (float((np.abs(r32 - r64).reshape(len(A), -1).max(axis=1) / (U * A)).max()),
            float((np.abs(x32 - x64).max(axis=1) / (U * A)).max()), int(keep.sum()))
