"""The plus-shape sampler as a specification, in numpy.  TEST INFRASTRUCTURE - nothing here is imported by the library.

The definition (include/hint_amd.h hint_plusgen_desc).  A row has nine draws, u_xl, u_yl, u_xw, u_yw, u_xs, u_ys,
u_a in [0, 1] and n_x, n_y standard normal; t = (cx, cy, angle, ratio) is an optional target, 0.25 <= ratio <= 4:
    xlength = 3 + 2 u_xl, ylength = 3 + 2 u_yl, xshift = -1.5 + 3 u_xs, yshift = -1.5 + 3 u_ys                 (data.py:190-202)
    xwidth = 0.5 + 1.5 u_xw, ywidth = 0.5 + 1.5 u_yw, angle = (pi / 2) u_a;  with a target: xwidth = ratio / 2 + (2 - ratio / 2) u_xw
        (ratio >= 1) or 0.5 + (2 ratio - 0.5) u_xw, ywidth = xwidth / ratio, angle = t[2]                     (data.py:195-200, :216)
    c = (xleft, yleft, yright, xright; xtop, ytop, xbottom, ybottom): xleft = xshift - xlength / 2, xright = xshift + xlength / 2,
        xtop = xwidth / 2 = -xbottom, yright = ywidth / 2 = -yleft, ybottom = yshift - ylength / 2, ytop = yshift + ylength / 2
    ring = the corners of the union of the boxes [xleft, xright] x [xbottom, xtop] and [yleft, yright] x [ybottom, ytop], clockwise
        from the first corner met clockwise from the negative x axis (THIS PROJECT'S DEFINITION: the reference takes whatever its
        polygon library returns); 12 or 8 corners
    dense = densify_polyline(ring, 0.2) (data.py:176-186): edge i from E = V_i to S = V_(i+1) gives count_i = max(1, rint(len / 0.2))
        points t S + (1 - t) E, t = j / (count_i - 1) (E alone when count_i = 1); N = sum of the counts
    mean = mean(dense); p = (dense - mean) R + 0.5 (n_x, n_y), R = [[cos a, sin a], [-sin a, cos a]]            (data.py:211-222)
    center = (-mean) R + 0.5 (n_x, n_y);  y = (center_x, center_y, angle, xwidth / ywidth)                     (data.py:203-225)
    x = flatten_coeffs(fourier_coeffs(p, 25)), 100 floats                                                      (data.py:30-33, :42-49)

The ring is built here by an algorithm that shares nothing with the kernel's table (ring_sorted): the eight box corners plus the
eight candidate edge-edge crossings, those kept that are not strictly inside the other box (corners) or that are proper crossings,
sorted clockwise by angle about the origin from the negative x axis - the union is star-shaped about the origin because both bars
are convex and contain it.  ring_table is a second construction, from the quadrant table of the header; test_plusgen_cpu.py holds
the two together.

Draws: Philox4x32-10 as tests/noise_oracle.py states it, counter = {row lo, row hi, stream, 0x504C5553}, key = {seed lo, seed hi}.
Stream 0: u_xl, u_yl, u_xw, u_yw = (float)c 2^-32; stream 1: u_xs, u_ys, u_a (the fourth word unused); stream 2: (n_x, n_y) = one
Box-Muller call on (min(((float)c0 + 1) 2^-32, 1), (float)c1 2^-32).

THE COMPARISON RULE.  u = 2^-24, the relative error of one fp32 rounding.  Absolute errors below are in units of u (lengths are
of order 1: every local coordinate is at most 4 in magnitude, a width at most 2, a centred point at most 5).
  local coordinate  a length or shift is one fused multiply-add: one rounding of a value below 5 (1.5 for a shift): 5 u and 1.5 u;
      half a length is exact: 2.5 u; xleft = xshift - xlength / 2: 1.5 + 2.5 + one rounding of a value below 4 = 8 u.  A width
      coordinate: 2 u halved = 1 u; with a target ywidth = xwidth / ratio carries at most (1.5 / ratio + 4) u <= 10 u, halved 5 u.
      E_LOCAL = 8.
  arms              xleft < yleft and its three likes compare two local coordinates, off by 8 u and 5 u: the fp32 decision is the
      exact one unless the arm is shorter than 13 u.  ARM_MARGIN = 16 u = 2^-20: a row with an arm (present or absent) within it is
      AMBIGUOUS.
  counts            an edge's length is the difference of two local coordinates: 8 + 8 u and one rounding of a value below 5:
      21 u; len / 0.2 is off by 105 u (the double division adds nothing at this scale).  HALF_MARGIN = 128 u = 2^-17: a row with an
      edge whose len / 0.2 lies within it of a half-integer is AMBIGUOUS.  Ambiguous rows are not compared (a point more or fewer
      shifts every later index); at most MAX_AMBIGUOUS = 1 % of a test's rows may be, and every test that drops rows asserts it.
      With a target ratio of 0.25 or 4 the widths are the constants 0.5 and 2, exact in fp32: an edge whose length is a width
      carries no error and is exempt (0.5 / 0.2 = 2.5 rounds to 2 in every row, by round-half-to-even).
      Rows built from dyadic draws, whose fp32 chain up to the edge length is exact, are compared whatever their slack (the tests
      pass keep = all rows for them): that is where round-half-to-even shows.
  dense point       t = j / (count - 1): relative u; 1 - t: 2 u absolute; (1 - t) E: 4 x 2 + 8 (1 - t) + one rounding (4 u);
      t S adds 8 t + 4; the fused sum one rounding of a value below 4: 8 + 8 + 4 + 4 + 4 = 28 u.  E_DENSE = 28.
  mean              a summation tree in which no term passes through more than h additions is off by at most h u sum |p_i|
      (Higham, Accuracy and Stability, section 4.2).  The kernel's tree - sixteen interleaved partial sums of at most seven terms,
      then the sixteen in order - has h = 6 + 15 = 21: 21 u x 4 N, divided by N: 84 u; the points' own 28 u; the division's
      rounding of a value below 4: E_MEAN = 84 + 28 + 4 = 116.
  placed point      d = p - mean: 28 + 116 + one rounding of a value below 5 = 149 u.  cos and sin are true values rounded once (u
      each); in the prior mode the angle itself is fl(fl(pi / 2) u_a), off by 3.2 u from (pi / 2) u_a, which turns d by at most
      5 x 3.2 = 16 u.  d R: 149 (|cos| + |sin|) <= 211, the entries' errors on 5: 5 + 5, the product's rounding 5, the fused sum's
      7.1 (a rotated point is below 5 sqrt 2): 233 u; with the angle 249 u.  Adding the offset rounds a value of at most A once.
      A, the row's largest placed coordinate magnitude, is at least 1.06: the x bar is at least 3 long, so its rotated extent is
      at least 3 / sqrt 2 along one axis, and one end of an interval that long is at least 1.06 from zero wherever the offset put
      it.  K_POINT = 249 / 1.06 + 1 = 236, in units of u A.
  y                 center = (-mean) R + offset: 116 x 1.4143 = 164, the entries' errors on |mean| <= 4: 4 + 4, roundings 4 + 5.7,
      the angle 4 x 3.2 = 13: 195 u; the offset's rounding of a value inside the figure, at most A: K_Y = 195 / 1.06 + 1 = 185.
      y[2] = angle: two roundings of a value below 1.58: ANGLE_ERR = 4 u (absolute; 0 with a target).  y[3] = xwidth / ywidth: each
      width is off by 2 u on a value of at least 0.5 (relative 4 u), the division rounds once: K_RATIO = 9, relative; with a target
      the same bound holds ((1.5 / ratio + 4) u on ywidth >= 0.5 x ... is within it for ratio >= 0.25: relative 8 u at most).
  coefficient       the mean of N products of placed points with twiddles, accumulated by fused multiply-adds: the points' 236 u A
      and, per sum, N u A of accumulation, u A of the twiddles' rounding and u A of the division: K_COEF(N) = 238 + N.
These bounds are derived, never tuned on device output; fp32_floor() evaluates the definition's formulas in numpy float32 and
tests/test_plusgen_cpu.py asserts that this floor lies inside them and records how far."""
import numpy as np

from noise_oracle import MASK, philox4x32_10
from shapegen_oracle import _box_muller

TAG = 0x504C5553            # counter word 3: "PLUS"
U = 2.0 ** -24
ARM_MARGIN = 16 * U
HALF_MARGIN = 128 * U
E_LOCAL, E_DENSE, E_MEAN = 8.0, 28.0, 116.0
K_POINT, K_Y, K_RATIO, ANGLE_ERR = 236.0, 185.0, 9.0, 4.0 * U
MAX_AMBIGUOUS = 0.01
N_COEFFS = 25
POINTS = 128                # storage of a dense outline
N_RANGE = (54, 106)         # from the perimeter's bounds; test_plusgen_cpu.py establishes it
MAX_DIST = 0.2
WRONG = ("r_transposed", "offset_first", "corner_mean", "half_up", "ccw", "late_start", "notch_filled")


def k_coef(count):
    return K_POINT + 2.0 + count


# ---- draws ----
def philox_words(seed: int, rows, stream: int):
    seed = int(seed) & (2 ** 64 - 1)
    rows = np.asarray(rows, dtype=np.uint64)
    c = philox4x32_10((rows & MASK, rows >> np.uint64(32), stream, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    return [w.astype(np.float32) for w in c]              # (float)c: round to nearest even


def row_ids(offset: int, n: int):
    return (np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & (2 ** 64 - 1)))


def draws(seed: int, offset: int, n: int, dtype=np.float64, rows=None):
    """[n, 9] = (u_xl, u_yl, u_xw, u_yw, u_xs, u_ys, u_a, n_x, n_y); the uniforms are exact fp32 values, part of the definition; the
    normals are evaluated in `dtype` from the fp32 uniforms.  rows: the Philox rows themselves (a gather)"""
    dtype = np.dtype(dtype).type
    rows = row_ids(offset, n) if rows is None else np.asarray(rows, dtype=np.uint64)
    s = np.float32(2.0 ** -32)
    f0, f1, f2 = (philox_words(seed, rows, k) for k in range(3))
    nx, ny = _box_muller(f2[0], f2[1], dtype)
    cols = [f0[0] * s, f0[1] * s, f0[2] * s, f0[3] * s, f1[0] * s, f1[1] * s, f1[2] * s]
    return np.stack([c.astype(dtype) for c in cols] + [nx, ny], axis=1)


# ---- geometry ----
def params(d, target=None, dtype=np.float64):
    """-> xlength, ylength, xwidth, ywidth, xshift, yshift, angle, each [n]"""
    dt = np.dtype(dtype).type
    d = np.asarray(d).astype(dtype)
    xl, yl = dt(3) + dt(2) * d[:, 0], dt(3) + dt(2) * d[:, 1]
    xs, ys = dt(-1.5) + dt(3) * d[:, 4], dt(-1.5) + dt(3) * d[:, 5]
    if target is None:
        xw, yw = dt(0.5) + dt(1.5) * d[:, 2], dt(0.5) + dt(1.5) * d[:, 3]
        ang = dt(np.pi / 2) * d[:, 6]
    else:
        r = dt(np.float32(target[3]))
        xw = dt(0.5) * r + (dt(2) - dt(0.5) * r) * d[:, 2] if r >= 1 else dt(0.5) + (dt(2) * r - dt(0.5)) * d[:, 2]
        yw = xw / r
        ang = np.full(len(d), dt(np.float32(target[2])), dtype=dtype)
    return xl, yl, xw, yw, xs, ys, ang


def local_coords(d, target=None, dtype=np.float64):
    """[n, 8] = (xleft, yleft, yright, xright; xtop, ytop, xbottom, ybottom), the order of PL_VX / PL_VY"""
    dt = np.dtype(dtype).type
    xl, yl, xw, yw, xs, ys, _ = params(d, target, dtype)
    h = dt(0.5)
    return np.stack([xs - h * xl, -(h * yw), h * yw, xs + h * xl, h * xw, ys + h * yl, -(h * xw), ys - h * yl], axis=1)


def arms(c):
    """bit 0 left, 1 right, 2 top, 3 bottom: the arm is present (equality: absent)"""
    return ((c[:, 0] < c[:, 1]) * 1 + (c[:, 3] > c[:, 2]) * 2 + (c[:, 5] > c[:, 4]) * 4 + (c[:, 7] < c[:, 6]) * 8).astype(np.int64)


def ring_sorted(c):
    """the first construction: -> (V [n, 12, 2] padded with NaN, corners [n])"""
    xl, yl, yr, xr, xt, yt, xb, yb = (c[:, i] for i in range(8))
    cand, keep = [], []
    inside = lambda px, py, x0, x1, y0, y1: (px > x0) & (px < x1) & (py > y0) & (py < y1)   # noqa: E731
    for px in (xl, xr):                        # the x box's corners
        for py in (xt, xb):
            cand.append((px, py))
            keep.append(~inside(px, py, yl, yr, yb, yt))
    for px in (yl, yr):                        # the y box's corners
        for py in (yt, yb):
            cand.append((px, py))
            keep.append(~inside(px, py, xl, xr, xb, xt))
    for px in (yl, yr):                        # the x box's horizontal edges with the y box's vertical edges
        for py in (xt, xb):
            cand.append((px, py))
            keep.append((px > xl) & (px < xr) & (py > yb) & (py < yt))
    for px in (xl, xr):                        # the x box's vertical edges with the y box's horizontal edges
        for py in (yt, yb):
            cand.append((px, py))
            keep.append((py > xb) & (py < xt) & (px > yl) & (px < yr))
    P = np.stack([np.stack(p, axis=1) for p in cand], axis=1)          # [n, 16, 2]
    K = np.stack(keep, axis=1)
    key = np.mod(np.pi - np.arctan2(P[..., 1], P[..., 0]), 2 * np.pi)  # clockwise from the negative x axis
    key = np.where(K, key, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :12]
    V = np.take_along_axis(P, order[..., None], axis=1)
    nc = K.sum(axis=1)
    V = np.where((np.arange(12)[None, :] < nc[:, None])[..., None], V, np.nan)
    return V, nc


def _quadrant_table(notch_filled=False):
    """mask -> (x indices, y indices, corners): the table of include/hint_amd.h, quadrant by quadrant, clockwise"""
    ax, bx, cx, dy = (0, 3, 3, 0), (4, 4, 6, 6), (1, 2, 2, 1), (5, 5, 7, 7)
    xarm, yarm = (0, 1, 1, 0), (2, 2, 3, 3)
    tab = {}
    for mask in range(16):
        ring = []
        for q in range(4):
            xa, ya, xfirst = (mask >> xarm[q]) & 1, (mask >> yarm[q]) & 1, q % 2 == 0
            X, I, Y, F = (ax[q], bx[q]), (cx[q], bx[q]), (cx[q], dy[q]), (ax[q], dy[q])
            if xa and ya:
                ring += [X, I, Y] if xfirst else [Y, I, X]
            elif xa:
                ring += [X]
            elif ya:
                ring += [Y]
            else:
                mid = I if notch_filled else F
                ring += [Y, mid, X] if xfirst else [X, mid, Y]
        tab[mask] = ring
    return tab


def ring_table(c, mask=None, notch_filled=False):
    """the second construction, from the quadrant table; mask: the arms decided elsewhere (the fp32 floor takes float64's)"""
    mask = arms(c) if mask is None else mask
    tab = _quadrant_table(notch_filled)
    V = np.full((len(c), 12, 2), np.nan, dtype=c.dtype)
    nc = np.zeros(len(c), dtype=np.int64)
    for m in np.unique(mask):
        rows = np.nonzero(mask == m)[0]
        ring = tab[int(m)]
        nc[rows] = len(ring)
        for s, (ix, iy) in enumerate(ring):
            V[rows, s, 0], V[rows, s, 1] = c[rows, ix], c[rows, iy]
    return V, nc


def edge_counts(V, nc, half_up=False):
    """-> (counts [n, 12] of the real edges, 0 behind them; q [n, 12] = len / 0.2 in float64 of the lengths as V's dtype has them)"""
    n = len(V)
    e = np.arange(12)[None, :]
    nxt = np.take_along_axis(V, ((e + 1) % nc[:, None])[..., None], axis=1)
    real = e < nc[:, None]
    ln = np.where(real, np.abs(nxt - V).max(axis=2), 0).astype(V.dtype)
    q = ln.astype(np.float64) / MAX_DIST
    r = np.floor(q + 0.5) if half_up else np.rint(q)
    return np.where(real, np.maximum(1, r), 0).astype(np.int64).reshape(n, 12), q, nxt


def densify(V, nc, dtype=np.float64, half_up=False):
    """-> (dense [n, 128, 2] zero-padded, N [n])"""
    dt = np.dtype(dtype).type
    V = V.astype(dtype)
    cnt, _, nxt = edge_counts(V, nc, half_up)
    N = cnt.sum(axis=1)
    assert (N <= POINTS).all()
    pre = np.cumsum(cnt, axis=1) - cnt
    pos = np.arange(POINTS)[None, :]
    edge = (pos[..., None] >= np.where(cnt > 0, pre, POINTS + 1)[:, None, :]).sum(axis=2) - 1           # [n, 128]
    edge = np.clip(edge, 0, 11)
    j = pos - np.take_along_axis(pre, edge, axis=1)
    ce = np.take_along_axis(cnt, edge, axis=1)
    t = np.where(ce > 1, j.astype(dtype) / np.maximum(ce - 1, 1).astype(dtype), dt(0)).astype(dtype)[..., None]
    E = np.take_along_axis(np.nan_to_num(V), edge[..., None], axis=1)
    S = np.take_along_axis(np.nan_to_num(nxt), edge[..., None], axis=1)
    p = np.where(t == 0, E, t * S + (dt(1) - t) * E)
    return np.where((pos < N[:, None])[..., None], p, dt(0)).astype(dtype), N


def dft(points, n_coeffs=N_COEFFS, dtype=np.float64):
    """rows of one count: points [rows, N, 2] -> [rows, 4 n_coeffs], the angle reduced in integers"""
    dt = np.dtype(dtype).type
    N = points.shape[1]
    ms = np.arange(-(n_coeffs // 2), n_coeffs // 2 + 1)
    ang = 2.0 * np.pi * ((ms[None, :] * np.arange(N)[:, None]) % N) / N
    cs, sn = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
    p = np.asarray(points, dtype=dtype)
    re = np.einsum("rnc,nm->rcm", p, cs).astype(dtype) / dt(N)
    im = -np.einsum("rnc,nm->rcm", p, sn).astype(dtype) / dt(N)
    return np.concatenate([re.reshape(len(p), -1), im.reshape(len(p), -1)], axis=1)


def coeffs(outline, counts, n_coeffs=N_COEFFS, dtype=np.float64):
    x = np.zeros((len(outline), 4 * n_coeffs), dtype=dtype)
    for N in np.unique(counts):
        rows = np.nonzero(counts == N)[0]
        x[rows] = dft(outline[rows, :N], n_coeffs, dtype)
    return x


def sample(d, target=None, dtype=np.float64, variant=None, mask=None):
    """d [n, 9] -> dict(x [n, 100], y [n, 4], outline [n, 128, 2], counts, corners, arms, mean, local); variant: one of WRONG"""
    assert variant is None or variant in WRONG
    dt = np.dtype(dtype).type
    d = np.asarray(d)
    c = local_coords(d, target, dtype)
    mask = arms(local_coords(d, target, np.float64)) if mask is None else mask
    V, nc = ring_table(c, mask, notch_filled=variant == "notch_filled")
    if variant in ("ccw", "late_start"):
        e = np.arange(12)[None, :]
        idx = (-e) % nc[:, None] if variant == "ccw" else (e + 1) % nc[:, None]
        V = np.where((e < nc[:, None])[..., None], np.take_along_axis(V, idx[..., None], axis=1), np.nan)
    dense, N = densify(V, nc, dtype, half_up=variant == "half_up")
    fN = N.astype(dtype)[:, None]
    live = (np.arange(POINTS)[None, :] < N[:, None])[..., None]
    if variant == "corner_mean":
        mean = np.nansum(V, axis=1).astype(dtype) / nc.astype(dtype)[:, None]
    else:
        mean = dense.sum(axis=1, dtype=dtype) / fN
    xl, yl, xw, yw, xs, ys, ang = params(d, target, dtype)
    cs, sn = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
    off = dt(0.5) * d[:, 7:9].astype(dtype)

    def rotate(p):                                          # p R, R = [[cos, sin], [-sin, cos]] ([[cos, -sin], [sin, cos]] transposed)
        s = -sn if variant == "r_transposed" else sn
        return np.stack([p[..., 0] * cs[:, None] - p[..., 1] * s[:, None], p[..., 0] * s[:, None] + p[..., 1] * cs[:, None]], axis=-1)

    cen = dense - mean[:, None, :]
    if variant == "offset_first":
        out = rotate(cen + off[:, None, :])
        center = rotate((-mean + off)[:, None, :])[:, 0]
    else:
        out = rotate(cen) + off[:, None, :]
        center = rotate((-mean)[:, None, :])[:, 0] + off
    out = np.where(live, out, dt(0)).astype(dtype)
    y = np.stack([center[:, 0], center[:, 1], ang, xw / yw], axis=1).astype(dtype)
    return dict(x=coeffs(out, N, N_COEFFS, dtype), y=y, outline=out, counts=N.astype(np.int32), corners=nc.astype(np.int32),
                arms=mask.astype(np.int32), mean=mean, local=c)


def geometry_center(d, target=None):
    """float64: (-mean) R of every row, the part of center that the normals do not touch"""
    c = local_coords(d, target)
    V, nc = ring_table(c)
    dense, N = densify(V, nc)
    mean = dense.sum(axis=1) / N[:, None]
    ang = params(d, target)[6]
    cs, sn = np.cos(ang), np.sin(ang)
    return np.stack([-mean[:, 0] * cs + mean[:, 1] * sn, -mean[:, 0] * sn - mean[:, 1] * cs], axis=1)


def scale(outline):
    """A per row: the largest placed coordinate magnitude"""
    return np.abs(outline).reshape(len(outline), -1).max(axis=1)


def slacks(d, target=None):
    """float64: (the shortest arm, present or absent; the smallest distance of an edge's len / 0.2 from a half-integer).  With a
    target whose ratio is 0.25 or 4 the coefficient of u_xw is zero and both widths are constants that fp32 holds exactly (0.5 and
    2): the edges across a bar's end, whose length is a width, carry no error and are left out of the second slack"""
    c = local_coords(d, target, np.float64)
    arm = np.min(np.abs(np.stack([c[:, 0] - c[:, 1], c[:, 3] - c[:, 2], c[:, 5] - c[:, 4], c[:, 7] - c[:, 6]], axis=1)), axis=1)
    V, nc = ring_table(c)
    _, q, nxt = edge_counts(V, nc)
    live = np.arange(12)[None, :] < nc[:, None]
    if target is not None and float(np.float32(target[3])) in (0.25, 4.0):
        ey, sy, ex, sx = V[..., 1], nxt[..., 1], V[..., 0], nxt[..., 0]
        xt, xb, yl, yr = c[:, 4, None], c[:, 6, None], c[:, 1, None], c[:, 2, None]
        width = ((ey == xt) & (sy == xb)) | ((ey == xb) & (sy == xt)) | ((ex == yl) & (sx == yr)) | ((ex == yr) & (sx == yl))
        live = live & ~width
    half = np.where(live, np.abs(q - np.floor(q) - 0.5), np.inf).min(axis=1)
    return arm, half


def ambiguous(d, target=None):
    arm, half = slacks(d, target)
    return (arm < ARM_MARGIN) | (half < HALF_MARGIN)


def compare(got, want, keep=None, target=None):
    """THE RULE on dicts of x, y, outline, counts, corners (got: any dtype; want: float64 from sample()): -> the worst ratios of
    error to bound over the rows of `keep` (counts, corners: the share of rows that differ).  passes() is all of them <= 1 / == 0"""
    keep = np.ones(len(want["x"]), dtype=bool) if keep is None else keep
    A = scale(want["outline"])[keep]
    N = want["counts"][keep].astype(np.float64)
    res = dict(counts=float((np.asarray(got["counts"])[keep] != want["counts"][keep]).mean()),
               corners=float((np.asarray(got["corners"])[keep] != want["corners"][keep]).mean()))
    f = lambda a: np.asarray(a, dtype=np.float64)[keep]     # noqa: E731
    n = int(keep.sum())
    res["outline"] = float((np.abs(f(got["outline"]) - f(want["outline"])).reshape(n, -1).max(axis=1) / (K_POINT * U * A)).max())
    res["x"] = float((np.abs(f(got["x"]) - f(want["x"])).max(axis=1) / ((K_POINT + 2.0 + N) * U * A)).max())
    gy, wy = f(got["y"]), f(want["y"])
    res["center"] = float((np.abs(gy[:, :2] - wy[:, :2]).max(axis=1) / (K_Y * U * A)).max())
    res["angle"] = float(np.abs(gy[:, 2] - wy[:, 2]).max() / ANGLE_ERR) if target is None else float((gy[:, 2] != wy[:, 2]).any())
    res["ratio"] = float((np.abs(gy[:, 3] - wy[:, 3]) / (K_RATIO * U * wy[:, 3])).max())
    return res


def passes(res):
    return res["counts"] == 0 and res["corners"] == 0 and all(np.isfinite(v) and v <= 1.0 for v in res.values())


def fp32_floor(d, target=None):
    """the same formulas in numpy float32 against float64 on the unambiguous rows of d: compare()'s ratios and the rows compared"""
    d = np.asarray(d, dtype=np.float32)
    keep = ~ambiguous(d, target)
    w = sample(d, target, np.float64)
    g = sample(d, target, np.float32, mask=w["arms"].astype(np.int64))
    return compare(g, w, keep, target), int(keep.sum())


def select(y, target, radius, n):
    """the rejection loop of rejection_sampling.py:113-127 on labels in row order: the indices of the first n rows with
    |y - target| < radius - the squared distance in fp32, ((e0^2 + e1^2) + (e2^2 + e3^2)) < fl(radius^2) - and how many rows were
    tried (the index of the n-th accepted row + 1); None where fewer than n are accepted"""
    e = np.asarray(y, dtype=np.float32) - np.asarray(target, dtype=np.float32)[None, :]
    s = e * e
    d2 = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    idx = np.nonzero(d2 < np.float32(float(radius) * float(radius)))[0]
    if len(idx) < n:
        return None, len(y), d2
    return idx[:n], int(idx[n - 1]) + 1, d2
