"""hint_amd.curves plus_segments / plus_outline_counts / plus_fit_terms / plus_fit_loss / plus_hausdorff_distances on the device
against the float64 oracle of tests/plus_oracle.py (its docstring states the comparison rule): the bound rule at every outline
size at which the kernel takes another path (one point an edge, one tile to the point, one point more, tiles and a remainder, the
most a row may have), traced and given curves, the integers equal, the fixtures recorded from the reference, exact cases, rows of
zero width, rows that cannot be served next to rows that can, the invariants (a row's bits independent of the batch, the position,
the grid and what the outputs held; guard-banded outputs), and graph capture."""
import os

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves
from hint_amd._lib import HintAmdError
import curve_oracle as co
import plus_oracle as po
from guarded import FILLS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_geo = _lib.load().hint_plus_geometry
TILE, CAP, MOST = _geo(1, 2, 2), _geo(1, 2, 3), _geo(1, 2, 4)
ALL = ("segments", "keep", "counts", "loss", "max_h", "avg_h")
WORDS = dict(segments=48, keep=1, counts=12, loss=2, max_h=1, avg_h=1)     # 4-byte words a row


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def run(params, curve=None, P=0, max_dist=0.02, want=ALL, max_groups=0, out=None):
    """the checked-argument route below the public functions, which also takes max_groups and buffers to write into"""
    k = 0 if curve is None or curve.dim() == 3 else curve.shape[1] // 4
    return curves._plus_run(params, curve, k, P, max_dist, want, max_groups, out)


def same_bits(a, b, names=ALL):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in names)


def assert_rule(ref, out, what):
    got = dict(segments=host(out["segments"]), loss=host(out["loss"]), max_h=host(out["max_h"]), avg_h=host(out["avg_h"]))
    r = po.ratios(ref, **got)
    print(f"{what}: error / bound " + ", ".join(f"{k} {v.max():.3g}" for k, v in r.items()))
    assert np.array_equal(out["keep"].cpu().numpy(), ref["keep"]), what
    assert np.array_equal(out["counts"].cpu().numpy(), ref["counts"]), what           # integers: equal, on every row
    bad, worst = po.check(ref, **got)
    assert len(bad) == 0, (what, bad[:10], worst)
    return {k: float(v.max()) for k, v in r.items()}


# ---- 1. the bound rule ----
# (K, P), N and the outline size one row is steered to (the sizes are even: the outline's edges come in pairs of equal extent).
# The product thinned: every (K, P), every N and every size at least once; the large N with the small P
SIZES = (12, TILE - 2, TILE, TILE + 2, 2 * TILE + 300, MOST - 2)
CASES = (((5, 2), 67, 12), ((5, 100), 67, TILE), ((25, 257), 3, TILE - 2), ((25, 1000), 3, TILE + 2), ((5, 1024), 3, 2 * TILE + 300),
         ((25, 1000), 1, MOST - 2), ((5, 100), 1, 12), ((5, 1024), 1, TILE))


def test_the_thinned_product_covers_every_value():
    assert {c[0] for c in CASES} == {(5, 2), (5, 100), (25, 257), (25, 1000), (5, 1024)}
    assert {c[1] for c in CASES} == {1, 3, 67} and {c[2] for c in CASES} == set(SIZES)
    assert TILE == 1024 and MOST == 4096


@pytest.mark.parametrize("KP,N,size", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bound_rule(KP, N, size):
    K, P = KP
    pr = po.draw_params(3 * K + P + N, N, ())
    order = np.argsort(-po.quotients(pr, 1.0).sum(1))                     # the largest outline first: no row goes past `size`
    md, r = po.find_max_dist(pr, size, rows=order)
    assert (po.half_gap(pr, md) > 1e-3).all()                             # so float64 and fp32 counts must agree, on every row
    x = (co.gauss(100 * K + P, N, K) * np.float32(3)).astype(np.float32)  # curves of the outline's size
    b32 = co.points64(x, P).astype(np.float32)                            # the given source: some curve's points, as fp32 data
    prd = dev(pr)
    for curve, name in ((x, "traced"), (b32, "given")):
        ref = po.plus64(pr, curve, P, md)
        assert ref["M"][r] == size and ref["M"].max() <= MOST
        out = run(prd, dev(curve), P, md)
        assert out["segments"].shape == (N, 12, 2, 2) and out["counts"].shape == (N, 12) and out["loss"].shape == (N, 2)
        assert out["keep"].dtype == out["counts"].dtype == torch.int32 and out["max_h"].shape == out["avg_h"].shape == (N,)
        assert_rule(ref, out, f"K {K} P {P} N {N} M {size} {name}")
        if N > 2:
            assert same_bits(run(prd, dev(curve), P, md, max_groups=2), out)
    # the public functions return the same bits
    xd = dev(x)
    full = run(prd, xd, P, md)
    mh, av = hint_amd.plus_hausdorff_distances(xd, prd, max_dist=md, n_points=P)
    assert bits_equal(mh, full["max_h"]) and bits_equal(av, full["avg_h"])
    assert bits_equal(hint_amd.plus_fit_terms(xd, prd, n_points=P), full["loss"])
    seg, keep = hint_amd.plus_segments(prd)
    assert bits_equal(seg, full["segments"]) and torch.equal(keep, full["keep"])
    assert torch.equal(hint_amd.plus_outline_counts(prd, md), full["counts"])
    mh, av = hint_amd.plus_hausdorff_distances(dev(b32), prd, max_dist=md, n_points=7)       # n_points is ignored for points
    given = run(prd, dev(b32), P, md)
    assert bits_equal(mh, given["max_h"]) and bits_equal(av, given["avg_h"])


def test_fit_loss_is_the_terms_weighted_and_traces_at_100_points():
    N, K = 5, 25
    pr, x = dev(po.draw_params(9, N)), dev(co.gauss(9, N, K))
    terms = hint_amd.plus_fit_terms(x, pr)
    assert bits_equal(terms, run(pr, x, 100, want=("loss",))["loss"])
    for w in (1.0, 0.5, 0):
        assert bits_equal(hint_amd.plus_fit_loss(x, pr, w), terms[:, 0] + float(w) * terms[:, 1])
    assert bits_equal(hint_amd.plus_fit_loss(x, pr), terms[:, 0] + terms[:, 1])
    one = hint_amd.plus_fit_terms(x, pr[2])                               # [9]: the same parameters for every row
    assert bits_equal(one, hint_amd.plus_fit_terms(x, pr[2:3].expand(N, 9)))
    with pytest.raises(HintAmdError, match="plus_fit_terms: params requires grad"):
        hint_amd.plus_fit_terms(x, pr.clone().requires_grad_())
    with pytest.raises(HintAmdError, match=r"plus_fit_terms: params must have shape \[9\], \[1, 9\] or \[5, 9\]"):
        hint_amd.plus_fit_terms(x, pr[:3])
    with pytest.raises(HintAmdError, match="plus_segments: params is torch.int64"):
        hint_amd.plus_segments(torch.zeros(9, dtype=torch.int64, device=DEV))


# ---- 2. the fixtures recorded from the reference ----
@pytest.mark.parametrize("case", po.GOLDEN_CASES, ids=lambda c: c["name"])
def test_fixtures_of_the_reference_within_the_bounds(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"plus_{case['name']}.npz"))
    x, pr, n = g["x"], g["params"], case["rows"]
    xd, prd = dev(x), dev(pr)
    ref = po.plus64(pr, x, po.GOLDEN_P, po.GOLDEN_MAX_DIST)
    fit = po.plus64(pr, x, po.GOLDEN_FIT_P, distances=False)
    mh, av = hint_amd.plus_hausdorff_distances(xd, prd)                   # the defaults are the reference's: 1000 points, 0.02
    r_h = np.maximum(np.abs(host(mh) - g["ref_max_h"]) / ref["E"], np.abs(host(av) - g["ref_avg_h"]) / ref["e_avg"])
    worst = [r_h.max()]
    for w, weight in enumerate(po.GOLDEN_WEIGHTS):
        loss = host(hint_amd.plus_fit_loss(xd, prd, weight))
        bound = fit["e_loss"][:, 0] + weight * fit["e_loss"][:, 1] + po.U * np.abs(g["ref_loss"][:, w])     # (and the sum's rounding)
        worst.append((np.abs(loss - g["ref_loss"][:, w]) / bound).max())
    seg, keep = hint_amd.plus_segments(prd)
    counts = hint_amd.plus_outline_counts(prd).cpu().numpy()
    kb = po.keep_bits(keep.cpu().numpy())
    assert np.array_equal(kb.sum(1), g["ref_n_segments"]) and np.array_equal(counts.sum(1), g["ref_outline_points"])
    for j in range(n):                                                    # the reference's list is the kept segments, in order
        err = np.abs(host(seg)[j][kb[j]] - g["ref_segments"][j, :kb[j].sum()]).max()
        worst.append(err / ref["dA"][j])
    print(f"{case['name']}: worst error / bound against the reference's values {max(worst):.3g}")
    assert max(worst) <= 1.0, worst


# ---- 3. exact cases ----
def test_a_curve_through_the_outlines_vertices_has_corner_term_zero():
    pr = dev(po.draw_params(31, 7))
    seg, _ = hint_amd.plus_segments(pr)
    b = seg[:, :, 0, :].contiguous()                                      # [N, 12, 2]: the vertices' own bits
    terms = hint_amd.plus_fit_terms(b, pr)
    assert (terms[:, 1] == 0).all() and (terms[:, 0] >= 0).all() and (terms[:, 0] < 1e-10).all()


def test_points_on_an_axis_parallel_dyadic_outline_have_segment_term_zero():
    pr = np.array([[4, 3, 1, 0.5, 0.5, -0.5, 0.25, -0.75, 0], [3, 3, 1, 1, 0, 0, 0, 0, 0]], np.float32)
    seg, keep = hint_amd.plus_segments(dev(pr))
    assert (keep == 0xfff).all() and np.array_equal(host(seg), po.segments64(pr)[0])         # angle 0, dyadic: exact
    s = host(seg)
    b = np.concatenate([s[:, :, 0, :], 0.5 * (s[:, :, 0, :] + s[:, :, 1, :]), 0.25 * s[:, :, 0, :] + 0.75 * s[:, :, 1, :]], 1)
    terms = hint_amd.plus_fit_terms(dev(b), dev(pr))
    assert (terms[:, 0] == 0).all() and (terms[:, 1] == 0).all()


def test_the_generated_outline_is_the_host_built_template_bit_for_bit():
    """every edge of extent 1 and 17 points an edge: t = i / 16 and the interpolation are exact, so the host builds the outline's
    bits; through hausdorff_distances with that template max_h and avg_h are the bits of plus_hausdorff_distances"""
    pr = np.array([[3, 3, 1, 1, 0, 0, 0.5, -0.25, 0]], np.float32)
    md = float(np.float32(1 / 16.7))
    counts = hint_amd.plus_outline_counts(dev(pr), md)
    assert (counts == 17).all()
    seg = po.segments64(pr)[0][0]
    tpl = po.outline64(seg, [17] * 12).astype(np.float32)
    assert np.array_equal(tpl.astype(np.float64), po.outline64(seg, [17] * 12)) and len(tpl) == 204
    for shift in ((0.0, 0.0), (0.125, -0.0625)):
        b = dev((tpl + np.array(shift, np.float32))[None])
        mh, av = hint_amd.plus_hausdorff_distances(b, dev(pr), max_dist=md)
        mh2, av2 = hint_amd.hausdorff_distances(b, dev(tpl))
        assert bits_equal(mh, mh2) and bits_equal(av, av2)
        assert (float(mh) == 0.0) == (shift == (0.0, 0.0))


# ---- 4. rows of zero width ----
def test_zero_width_rows_drop_segments_and_divide_by_the_kept_count():
    N, K, P, md = 6, 5, 100, 0.2
    # row 1: xwidth = 0, segments 5 and 11; row 3: ywidth = 0, segments 2 and 8; row 4: both
    pr = po.draw_params(41, N, (md,), zero={1: (2,), 3: (3,), 4: (2, 3)})
    assert (pr[1, 2], pr[3, 3], pr[4, 2], pr[4, 3]) == (0, 0, 0, 0) and (pr[[0, 2, 5], 2:4] > 0).all()
    assert (po.half_gap(pr, md) > 1e-3).all()
    x = (co.gauss(42, N, K) * np.float32(3)).astype(np.float32)
    ref = po.plus64(pr, x, P, md)
    out = run(dev(pr), dev(x), P, md)
    assert out["keep"].tolist() == [0xfff, 0xfff & ~0x820, 0xfff, 0xfff & ~0x104, 0xfff & ~0x924, 0xfff]
    assert (out["counts"].cpu().numpy()[~po.keep_bits(ref["keep"])] == 0).all()
    assert_rule(ref, out, "zero widths")
    # the mean over 12 corners would miss the rule on the rows that keep fewer
    wrong = host(out["loss"]).copy()
    wrong[:, 1] *= po.keep_bits(ref["keep"]).sum(1) / 12.0
    assert sorted(po.check(ref, loss=wrong)[0].tolist()) == [1, 3, 4]


# ---- 5. rows that cannot be served ----
def test_rows_that_cannot_be_served_get_nan_and_leave_the_others_alone():
    K, P, md = 5, 100, 0.02
    good = po.draw_params(51, 4, (md,))
    bad = po.draw_params(52, 5, ())
    bad[0, :2] = 40.0                                                     # an outline of some 8000 points
    bad[1, 0] = np.nan
    bad[2, 8] = np.inf
    bad[3, 6] = -np.inf
    bad[4, :2] = 3e6                                                      # quotients past the cut, finite
    pr = np.stack([good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], bad[4], good[3]])
    rows_good, rows_bad = [0, 2, 5, 8], [1, 3, 4, 6, 7]
    x = (co.gauss(53, len(pr), K) * np.float32(3)).astype(np.float32)
    out = run(dev(pr), dev(x), P, md)
    torch.cuda.synchronize()                                              # nothing faulted
    alone = run(dev(pr[rows_good]), dev(x[rows_good]), P, md)
    assert same_bits({k: v[rows_good] for k, v in out.items()}, alone)
    assert torch.isnan(out["max_h"][rows_bad]).all() and torch.isnan(out["avg_h"][rows_bad]).all()
    assert (out["counts"][rows_bad] == -1).all() and (out["counts"][rows_good] > 0).all()
    assert torch.isfinite(out["max_h"][rows_good]).all()
    # the over-long rows' segments, keep and loss need no outline: as the oracle has them
    for r in (1, 7):
        ref = po.plus64(pr[r:r + 1], x[r:r + 1], P, md, distances=False)
        assert ref["M"][0] > MOST and out["keep"][r].item() == ref["keep"][0]
        assert len(po.check(ref, segments=host(out["segments"][r:r + 1]), loss=host(out["loss"][r:r + 1]))[0]) == 0
    # one point under the limit is served, the next size is not
    one = po.draw_params(54, 1, ())
    md_in, _ = po.find_max_dist(one, MOST)
    md_out, _ = po.find_max_dist(one, MOST + 2)
    assert hint_amd.plus_outline_counts(dev(one), md_in).sum().item() == MOST
    assert (hint_amd.plus_outline_counts(dev(one), md_out) == -1).all()
    mh, _ = hint_amd.plus_hausdorff_distances(dev(x[:1]), dev(one), max_dist=md_in, n_points=P)
    assert torch.isfinite(mh).all()
    assert torch.isnan(hint_amd.plus_hausdorff_distances(dev(x[:1]), dev(one), max_dist=md_out, n_points=P)[0]).all()


# ---- 6. invariance ----
def test_a_rows_bits_do_not_depend_on_the_batch_the_position_the_grid_or_the_outputs():
    K, P, md = 5, 100, 0.2
    N = CAP + 1                                                           # one row more than the default grid has workgroups
    pr = po.draw_params(61, 8, ())[np.arange(N) % 8]
    x = (co.gauss(62, 8, K) * np.float32(3)).astype(np.float32)[np.arange(N) % 8]
    prd, xd = dev(pr), dev(x)
    full = run(prd, xd, P, md)
    for r in (0, 3, N - 1):
        assert same_bits(run(prd[r:r + 1], xd[r:r + 1], P, md), {k: v[r:r + 1] for k, v in full.items()})
    assert same_bits({k: v[:8] for k, v in full.items()}, {k: v[N - 9:N - 1] for k, v in full.items()})      # rows 0..7 again
    for mg in (1, 7):
        assert same_bits(run(prd[:40], xd[:40], P, md, max_groups=mg), {k: v[:40] for k, v in full.items()})
    assert same_bits(run(prd, xd, P, md), full)                           # two runs
    shapes = dict(segments=(N, 12, 2, 2), keep=(N,), counts=(N, 12), loss=(N, 2), max_h=(N,), avg_h=(N,))
    for fill in (float("nan"), 1e30):
        pre = {}
        for k, s in shapes.items():
            t = torch.full(s, fill, dtype=torch.float32, device=DEV)
            pre[k] = t.view(torch.int32) if k in ("keep", "counts") else t
        assert same_bits(run(prd, xd, P, md, out=pre), full)


# ---- 7. each output alone, all together, on guard-banded buffers ----
@pytest.mark.parametrize("source", ("traced", "given"))
def test_each_output_alone_and_all_together_on_guarded_buffers(source):
    N, K, P, md = 5, 5, 257, 0.02
    pr = po.draw_params(71, N, (md,))
    x = (co.gauss(72, N, K) * np.float32(3)).astype(np.float32)
    curve = x if source == "traced" else co.points64(x, P).astype(np.float32)
    gp = Guarded(9 * N).set(torch.from_numpy(pr))
    gc = Guarded(curve.size).set(torch.from_numpy(curve))
    snaps = [gp.snapshot(), gc.snapshot()]
    prd, cd = gp.view(N, 9), gc.view(*curve.shape)

    def guarded_run(names, fill, seed):
        bufs = {k: Guarded(WORDS[k] * N, fill=fill, seed=seed + i, align=16 if seed % 2 else 256,
                           dtype=torch.int32 if k in ("keep", "counts") else torch.float32) for i, k in enumerate(names)}
        shapes = dict(segments=(N, 12, 2, 2), keep=(N,), counts=(N, 12), loss=(N, 2), max_h=(N,), avg_h=(N,))
        need_curve = any(k in names for k in ("loss", "max_h", "avg_h"))
        out = run(prd, cd if need_curve else None, P if need_curve else 0, md, tuple(names), seed % 3,
                  {k: bufs[k].view(*shapes[k]) for k in names})
        for k, gb in bufs.items():
            gb.check_guards(f"{names} {fill}: {k}")
        gp.check_unchanged(snaps[0], "params")
        gc.check_unchanged(snaps[1], "curve")
        return {k: v.clone() for k, v in out.items()}

    first = guarded_run(ALL, "zero", 0)
    for rep, fill in enumerate(FILLS):
        assert same_bits(guarded_run(ALL, fill, 10 * rep + 1), first)
    for i, name in enumerate(ALL):
        assert same_bits(guarded_run((name,), "nan", 50 + i), first, (name,))
    assert same_bits(guarded_run(("segments", "keep", "counts"), "junk", 70), first, ("segments", "keep", "counts"))
    assert same_bits(run(prd, cd, P, md), first)


# ---- 8. graph capture ----
def test_capture_in_a_graph_and_two_replays():
    N, K, P, md = 9, 25, 1000, 0.02
    prd = dev(po.draw_params(81, N, (md,)))
    xd = dev((co.gauss(82, N, K) * np.float32(3)).astype(np.float32))
    eager = hint_amd.plus_hausdorff_distances(xd, prd)                    # (also loads the kernel before the capture)
    eager_l = hint_amd.plus_fit_terms(xd, prd)
    eager_s = hint_amd.plus_segments(prd)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mh, av = hint_amd.plus_hausdorff_distances(xd, prd)
        terms = hint_amd.plus_fit_terms(xd, prd)
        seg, keep = hint_amd.plus_segments(prd)
    for _ in range(2):
        for t in (mh, av, terms, seg):
            t.fill_(float("nan"))
        keep.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(mh, eager[0]) and bits_equal(av, eager[1]) and bits_equal(terms, eager_l)
        assert bits_equal(seg, eager_s[0]) and torch.equal(keep, eager_s[1])
