"""GPU tests of the polygon overlap (hint_overlap_run): every ledger case of tests/overlap_oracle.py against the float64 oracle
at its bound, closed forms, both curve sources, the plus outline against the same vertices given as a polygon, invariance (the
batch, the position, the grid, what the outputs held), guard-banded outputs, rows that cannot be served, the two evaluation
wrappers against their parts, and graph capture."""
import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import curves
import lensfit_oracle as lfo
import overlap_oracle as oo
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("areas", "iou", "dice", "crossings")
WORDS = dict(areas=3, iou=1, dice=1, crossings=1)                          # 4-byte words a row


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def shapes(N):
    return dict(areas=(N, 3), iou=(N,), dice=(N,), crossings=(N,))


def run(curve, P=100, polygon=None, offsets=None, params=None, plus_params=None, want=ALL, max_groups=0, out=None):
    """the checked-argument route below the public functions, which also takes max_groups and buffers to write into"""
    k = 0 if curve.dim() == 3 else curve.shape[1] // 4
    return curves._ov_run(curve, k, curve.shape[1] if k == 0 else P, polygon, offsets, params, plus_params, want, max_groups, out)


def same_bits(a, b, names=ALL):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in names)


def case_inputs(case):
    """the device tensors of a ledger case, as run()'s keyword arguments (curve first)"""
    kw = dict(P=case["P"])
    for src, dst in (("a_points", "polygon"), ("params", "params"), ("plus_params", "plus_params")):
        if case[src] is not None:
            kw[dst] = dev(case[src])
    if case["offsets"] is not None:
        kw["offsets"] = dev(case["offsets"], torch.int64)
    return dev(case["curve"]), kw


def device_points(case, curve):
    """the curve's vertices as the kernel sees them: the device's own trace, or the given points"""
    return (hint_amd.trace_fourier_curves(curve, case["P"]) if curve.dim() == 2 else curve).cpu().numpy().astype(np.float64)


def device_template(case, kw, n):
    """row n's placed template as the kernel sees it: the device's own plus vertices, or the emulated placement"""
    if case["plus_params"] is not None:
        return hint_amd.plus_segments(kw["plus_params"][n:n + 1])[0][0, :, 0].cpu().numpy().astype(np.float64)
    return oo.row_template32(case, n)


def got_row(out, n):
    a = out["areas"][n].double().cpu().numpy()
    return dict(area_T=a[0], area_C=a[1], I=a[2], iou=float(out["iou"][n]), dice=float(out["dice"][n]))


# ---- 1. the bound rule, on guard-banded and poisoned outputs ----
@pytest.mark.parametrize("name", [c[0] for c in oo.LEDGER])
def test_every_ledger_case_within_the_oracles_bound(name):
    case = oo.ledger_case(name)
    curve, kw = case_inputs(case)
    N = curve.shape[0]
    bufs = {k: Guarded(WORDS[k] * N, fill="nan", seed=3, dtype=torch.int32 if k == "crossings" else torch.float32) for k in ALL}
    out = run(curve, out={k: bufs[k].view(*shapes(N)[k]) for k in ALL}, **kw)
    torch.cuda.synchronize()
    for k, gb in bufs.items():
        gb.check_guards(f"{name}: {k}")
    pts = device_points(case, curve)
    worst, left_out, positive = 0.0, 0, 0
    for n in range(N):
        ref = oo.overlap64(pts[n], device_template(case, kw, n))
        r = oo.ratio(ref, got_row(out, n))
        worst = max(worst, r)
        assert r <= 1.0, (name, n, r, ref, got_row(out, n))
        count, decided = oo.crossings64(pts[n])
        left_out += not decided
        positive += count > 0
        if decided:
            assert int(out["crossings"][n]) == count, (name, n)
    print(f"{name}: worst error / bound {worst:.3f} (c = {oo.C_TOL:g}); {left_out} of {N} rows' crossings undecided, "
          f"{positive} rows cross themselves")
    assert left_out <= 0.1 * N
    if name == "plus traced 100, 511":
        assert positive >= 1


def test_closed_forms_on_the_device():
    a = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 2.0], [0.0, 2.0]], np.float32)
    b = np.array([[1.5, 1.0], [3.5, 1.0], [3.5, 4.0], [1.5, 4.0]], np.float32)
    for Cv, Tv in ((a, b), (b, a), (a[::-1], b), (a, b[::-1]), (np.roll(a, 2, 0), b)):
        r = hint_amd.polygon_overlap(dev(Cv)[None], dev(Tv))
        assert r.areas.tolist() == [[6.0, 6.0, 1.5]] and r.crossings.tolist() == [0]             # exact in fp32
        assert abs(float(r.iou) - 1.5 / 10.5) <= 2 ** -24 and abs(float(r.dice) - 0.25) <= 2 ** -24
    for Tv in ([[4.0, 0.0], [5.0, 0.0], [5.0, 1.0], [4.0, 1.0]], [[0.0, 3.0], [3.0, 3.0], [3.0, 5.0], [0.0, 5.0]],
               [[3.0, 0.0], [4.0, 0.0], [4.0, 2.0], [3.0, 2.0]]):                                 # disjoint, touching: exactly 0
        r = hint_amd.polygon_overlap(dev(a)[None], dev(np.array(Tv, np.float32)))
        assert float(r.areas[0, 2]) == 0.0 and float(r.iou) == 0.0 and float(r.dice) == 0.0
    w = oo.wobble_curves(5, 4, 37)
    for n in range(4):                                                   # a polygon with itself, either orientation
        for Tv in (w[n], w[n][::-1]):
            r = hint_amd.polygon_overlap(dev(w[n])[None], dev(Tv))
            ref = oo.overlap64(w[n], Tv)
            assert oo.ratio(ref, got_row(r._asdict(), 0)) <= 1.0 and abs(float(r.iou) - 1.0) < 1e-5
    eight = np.array([[0.0, 0.0], [2.0, 2.0], [2.0, 0.0], [0.0, 2.0]], np.float32)
    r = hint_amd.polygon_overlap(dev(eight)[None], dev(a))
    assert r.crossings.tolist() == [1] and float(r.areas[0, 1]) == 0.0 and float(r.areas[0, 2]) == 0.0
    flat = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]], np.float32)                             # no area at all: NaN
    r = hint_amd.polygon_overlap(dev(flat)[None], dev(flat))
    assert torch.isnan(r.iou).all() and torch.isnan(r.dice).all() and r.areas.tolist() == [[0.0, 0.0, 0.0]]


# ---- 2. sources ----
def test_a_traced_curve_and_its_points_given_agree_bit_for_bit():
    x, proto, params = (dev(v) for v in oo.lens_case(301, 16))
    for P in (3, 100, 257):
        pts = hint_amd.trace_fourier_curves(x, P)
        t, g = hint_amd.polygon_overlap(x, proto, params, n_points=P), hint_amd.polygon_overlap(pts, proto, params)
        assert all(bits_equal(u, v) for u, v in zip(t[:3], g[:3])) and torch.equal(t.crossings, g.crossings)
    t, g = hint_amd.lens_iou_dice(x, proto, params), hint_amd.polygon_overlap(x, proto, params, n_points=100)
    assert bits_equal(t[0], g.iou) and bits_equal(t[1], g.dice) and torch.equal(t[2], g.crossings)
    only = run(x, want=("crossings",))["crossings"]                       # crossings alone: no template at all
    assert torch.equal(only, g.crossings)


def test_the_plus_outline_is_its_twelve_vertices_given_as_a_polygon_bit_for_bit():
    x, pr = oo.plus_case(511, 16)
    x, pr = dev(x), dev(pr)
    seg, keep = hint_amd.plus_segments(pr)
    assert int(keep[2]) != 0xFFF                                          # a zero width: dropped segments, repeated vertices
    verts = seg[:, :, 0, :].reshape(-1, 2).contiguous()
    ref = hint_amd.polygon_overlap(x, verts, offsets=torch.arange(0, 12 * 16 + 1, 12, device=DEV))
    iou, dice, cr = hint_amd.plus_iou_dice(x, pr)
    assert bits_equal(iou, ref.iou) and bits_equal(dice, ref.dice) and torch.equal(cr, ref.crossings)
    assert bool(((iou > 0) & (iou <= 1)).all())


# ---- 3. invariance ----
@pytest.mark.parametrize("kind", ("lens", "plus"))
def test_a_rows_bits_do_not_depend_on_the_batch_the_position_the_grid_or_the_outputs(kind):
    N = 300
    idx = np.arange(N) % 16
    if kind == "lens":
        x, proto, params = oo.lens_case(301, 16)
        xd, kw = dev(x[idx]), dict(polygon=dev(proto), params=dev(params[idx]))
    else:
        x, pr = oo.plus_case(511, 16)
        xd, kw = dev(x[idx]), dict(plus_params=dev(pr[idx]))

    def sub(sl, **more):
        return run(xd[sl], **{k: (v[sl] if k != "polygon" else v) for k, v in kw.items()}, **more)

    full = sub(slice(0, N))
    for r in (0, 3, N - 1):
        assert same_bits(sub(slice(r, r + 1)), {k: v[r:r + 1] for k, v in full.items()})
    assert same_bits({k: v[:16] for k, v in full.items()}, {k: v[N - 28:N - 12] for k, v in full.items()})     # rows 0..15 again
    for mg in (1, 7):
        assert same_bits(sub(slice(0, 40), max_groups=mg), {k: v[:40] for k, v in full.items()})
    assert same_bits(sub(slice(0, N)), full)                              # two runs
    for fill in (float("nan"), 1e30):
        pre = {k: torch.full(s, fill, dtype=torch.float32, device=DEV) for k, s in shapes(N).items()}
        pre["crossings"] = pre["crossings"].view(torch.int32)
        assert same_bits(sub(slice(0, N), out=pre), full)


# ---- 4. each output alone, all together, on guard-banded buffers; null outputs are not written ----
@pytest.mark.parametrize("source", ("traced", "given"))
def test_each_output_alone_and_all_together_on_guarded_buffers(source):
    N, P = 5, 257
    x, proto, params = oo.lens_case(305, N, 1025)
    curve = x if source == "traced" else oo.wobble_curves(7, N, P)
    gc, gt, gp = (Guarded(v.size).set(torch.from_numpy(v)) for v in (curve, proto, params))
    snaps = [g.snapshot() for g in (gc, gt, gp)]
    cd, td, pd = gc.view(*curve.shape), gt.view(*proto.shape), gp.view(N, 4)

    def guarded_run(names, fill, seed):
        bufs = {k: Guarded(WORDS[k] * N, fill=fill, seed=seed + i, align=16 if seed % 2 else 256,
                           dtype=torch.int32 if k == "crossings" else torch.float32) for i, k in enumerate(names)}
        out = run(cd, P, td, None, pd, None, tuple(names), seed % 3, {k: bufs[k].view(*shapes(N)[k]) for k in names})
        torch.cuda.synchronize()
        for k, gb in bufs.items():
            gb.check_guards(f"{names} {fill}: {k}")
        for g, s, what in zip((gc, gt, gp), snaps, ("curve", "polygon", "params")):
            g.check_unchanged(s, what)
        return {k: v.clone() for k, v in out.items()}

    first = guarded_run(ALL, "zero", 0)
    for rep, fill in enumerate(FILLS):
        assert same_bits(guarded_run(ALL, fill, 10 * rep + 1), first)
    for i, name in enumerate(ALL):
        assert same_bits(guarded_run((name,), "nan", 50 + i), first, (name,))
    assert same_bits(guarded_run(("iou", "crossings"), "junk", 70), first, ("iou", "crossings"))
    assert same_bits(run(cd, P, td, None, pd), first)


# ---- 5. rows that cannot be served ----
def test_rows_that_cannot_be_served_get_nan_and_leave_the_others_alone():
    N = 9
    x, proto, params = oo.lens_case(307, N)
    clean = run(dev(x), polygon=dev(proto), params=dev(params))
    xb, pb = x.copy(), params.copy()
    xb[1, 3], xb[4, 0], pb[6, 2], pb[7, 3] = np.nan, np.inf, np.nan, np.inf
    bad_rows, good_rows = [1, 4, 6, 7], [0, 2, 3, 5, 8]
    out = run(dev(xb), polygon=dev(proto), params=dev(pb))
    for k in ("areas", "iou", "dice"):
        assert bool(torch.isnan(out[k][bad_rows]).all()), k
    assert out["crossings"][bad_rows].tolist() == [-1] * 4
    assert same_bits({k: v[good_rows] for k, v in out.items()}, {k: v[good_rows] for k, v in clean.items()})
    # crossings alone looks at the curve only: a bad placement does not reach it
    only = run(dev(xb), want=("crossings",))["crossings"]
    assert only[[1, 4]].tolist() == [-1, -1] and torch.equal(only[[0, 2, 3, 5, 6, 7, 8]], clean["crossings"][[0, 2, 3, 5, 6, 7, 8]])
    # a template vertex that is not finite; given points that are not
    tb = proto.copy()
    tb[77, 1] = np.nan
    out = run(dev(x), polygon=dev(tb))
    assert bool(torch.isnan(out["iou"]).all()) and out["crossings"].tolist() == [-1] * N
    pts = oo.wobble_curves(9, 3, 100)
    pts[1, 50, 0] = np.nan
    out, ok = run(dev(pts), polygon=dev(proto)), run(dev(oo.wobble_curves(9, 3, 100)), polygon=dev(proto))
    assert bool(torch.isnan(out["areas"][1]).all()) and int(out["crossings"][1]) == -1
    assert same_bits({k: v[[0, 2]] for k, v in out.items()}, {k: v[[0, 2]] for k, v in ok.items()})
    # the plus: a parameter that is not finite
    xp, pr = oo.plus_case(521, 6, zero_width=(1,), clamped=(3,))
    clean = run(dev(xp), plus_params=dev(pr))
    prb = pr.copy()
    prb[2, 8], prb[5, 0] = np.nan, np.inf
    out = run(dev(xp), plus_params=dev(prb))
    assert bool(torch.isnan(out["dice"][[2, 5]]).all()) and out["crossings"][[2, 5]].tolist() == [-1, -1]
    assert same_bits({k: v[[0, 1, 3, 4]] for k, v in out.items()}, {k: v[[0, 1, 3, 4]] for k, v in clean.items()})


def test_ragged_rows_with_a_bad_range_get_nan_and_read_nothing():
    good_sizes = (3, 130, 1500, 17)
    parts = [oo.polygon_template(m) for m in good_sizes]
    # one call: rows 0, 1, 2 and 4 are the good templates; row 3 owns two points, row 5 a range past the end of a_points
    a_points = np.concatenate(parts[:3] + [np.zeros((2, 2), np.float32)] + parts[3:])
    T = len(a_points)
    off = np.array([0, 3, 133, 1633, 1635, T, T + 40], np.int64)          # (on the device: the kernel judges them)
    N = 6
    x, params = lfo.lens_rows(311, N), lfo.golden_grad_params(311, N)
    ga = Guarded(2 * T).set(torch.from_numpy(a_points))                   # the guards would show in a result, never fault
    out = run(dev(x), polygon=ga.view(T, 2), offsets=dev(off, torch.int64), params=dev(params))
    for k in ("areas", "iou", "dice"):
        assert bool(torch.isnan(out[k][[3, 5]]).all()), k
    assert out["crossings"][[3, 5]].tolist() == [-1, -1]
    rows = [0, 1, 2, 4]
    a_good, off_good = oo.ragged_templates(good_sizes)
    good = run(dev(x[rows]), polygon=dev(a_good), offsets=dev(off_good, torch.int64), params=dev(params[rows]))
    assert same_bits({k: v[rows] for k, v in out.items()}, good)
    assert bool(torch.isfinite(good["iou"]).all())
    neg = run(dev(x[:1]), polygon=ga.view(T, 2), offsets=torch.tensor([-5, 30], device=DEV), params=dev(params[:1]))
    assert bool(torch.isnan(neg["iou"]).all()) and neg["crossings"].tolist() == [-1]                # a negative start


# ---- 6. the evaluation loop's columns ----
def test_lens_shape_scores_is_the_composition_of_the_public_calls_bit_for_bit():
    x, proto = dev(lfo.lens_rows(312, 6)), dev(lfo.lens_prototype(130))
    s = hint_amd.lens_shape_scores(x, proto)
    params, _ = hint_amd.fit_lens_shapes(x, proto)
    ov = hint_amd.polygon_overlap(hint_amd.trace_fourier_curves(x, 100), proto, params)
    mh, av = hint_amd.hausdorff_distances(hint_amd.trace_fourier_curves(x, 1000), proto, params)
    assert bits_equal(s.params, params) and bits_equal(s.iou, ov.iou) and bits_equal(s.dice, ov.dice)
    assert torch.equal(s.crossings, ov.crossings) and bits_equal(s.max_h, mh) and bits_equal(s.avg_h, av)
    assert s._fields == ("iou", "dice", "max_h", "avg_h", "crossings", "params")
    print("lens scores: IoU", s.iou.tolist(), "DICE", s.dice.tolist(), "crossings", s.crossings.tolist())
    assert bool(((s.iou > 0) & (s.iou <= 1) & (s.dice >= s.iou)).all())   # DICE >= IoU always: 2 (C + T - I) >= C + T


def test_plus_shape_scores_is_the_composition_of_the_public_calls_bit_for_bit():
    x = dev(oo.plus_case(521, 6)[0])
    s = hint_amd.plus_shape_scores(x)
    params, _ = hint_amd.fit_plus_shapes(x)
    iou, dice, cr = hint_amd.plus_iou_dice(hint_amd.trace_fourier_curves(x, 100), params)
    mh, av = hint_amd.plus_hausdorff_distances(hint_amd.trace_fourier_curves(x, 1000), params)
    assert bits_equal(s.params, params) and bits_equal(s.iou, iou) and bits_equal(s.dice, dice)
    assert torch.equal(s.crossings, cr) and bits_equal(s.max_h, mh) and bits_equal(s.avg_h, av)
    print("plus scores: IoU", s.iou.tolist(), "DICE", s.dice.tolist(), "crossings", s.crossings.tolist())
    assert s.params.shape == (6, 9) and bool(((s.iou > 0) & (s.iou <= 1) & (s.dice >= s.iou)).all())


# ---- 7. graph capture ----
def test_capture_in_a_graph_and_two_replays():
    x, proto, params = (dev(v) for v in oo.lens_case(301, 16))
    xp, pr = (dev(v) for v in oo.plus_case(511, 16))
    eager = hint_amd.polygon_overlap(x, proto, params)                    # (also loads the kernel before the capture)
    eager_p = hint_amd.plus_iou_dice(xp, pr)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ov = hint_amd.polygon_overlap(x, proto, params)
        pl = hint_amd.plus_iou_dice(xp, pr)
    for _ in range(2):
        for t in (ov.iou, ov.dice, ov.areas, pl[0], pl[1]):
            t.fill_(float("nan"))
        ov.crossings.fill_(-7)
        pl[2].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(bits_equal(u, v) for u, v in zip(ov[:3], eager[:3])) and torch.equal(ov.crossings, eager.crossings)
        assert bits_equal(pl[0], eager_p[0]) and bits_equal(pl[1], eager_p[1]) and torch.equal(pl[2], eager_p[2])
