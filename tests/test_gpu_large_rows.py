"""The descriptor kernels past 2^31 elements: every case of tests/large_cases.py ROW_CASES runs its entry point once at the smallest
size at which the named array holds more than 2^31 elements (so element indices pass 2^31 and byte offsets pass 2^31 and 2^32 in
one call), with every output in a guard-banded buffer that held the NaN pattern before the call.

What each case asserts: the guards are intact (no write far from the buffer); no NaN-pattern word is left in a per-row output
(no row skipped by a wrapped index); on the probe rows - head, ragged tail, a picket, both sides of the three crossings - the
float64 oracle of the kernel at that oracle's own bounds, and, where the project promises that a row's bits do not depend on its
position, bit equality with a small call on the same rows; whole-batch reductions against float64 on the device, in chunks.
Inputs are seeded and generated on the device in row chunks; at most one case is alive at a time and its memory is handed back
in a finally.  A case skips, naming the figure, only when the device has less free memory than it declares.
The plus-shape sampler has a case for each of its two wide arrays (they leave the kernel by different code), with the Philox row
counter's high word changing inside the call; the epoch case runs the three epoch ops in turn on one table, the output
re-poisoned between them, and compares the WHOLE gathered and standardised tables bit for bit, in chunks.  Entry points whose
documented limits keep every offset below 2^31 run at those limits in their own files (tests/large_cases.py LIMITED)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, curves, data
import abc_oracle as ao
import corr_oracle as cro
import curve_oracle as co
import epoch_oracle as eo
import hausdorff_oracle as ho
import lensfit_oracle as lo
import overlap_oracle as oo
import plusfit_oracle as pfo
import plus_oracle as po
import plusgen_oracle as pgo
import large_cases as lc
import shapegen_oracle as so
from guarded import NAN_BITS, Guarded, bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CASES = lc.ROW_CASES


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def nan_out(bufs, name, n_words, dtype=torch.float32):
    bufs[name] = Guarded(n_words, fill="nan", dtype=dtype)
    return bufs[name]


def check_written(bufs, names, what):
    """guards intact on every guarded buffer; no word of the named per-row outputs still holds the NaN pattern"""
    for name, g in bufs.items():
        if isinstance(g, Guarded):
            g.check_guards(f"{what}: {name}")
    for name in names:
        left = lc.count_words(bufs[name].words, NAN_BITS)
        assert left == 0, f"{what}: {left} words of {name} were never written"


def probes(case, extra=()):
    rows = lc.probe_rows(case["N"], case["width"], extra, case["crossings"])
    for r in case["crossings"]:
        assert r - 1 in rows and r in rows and r < case["N"]
    return rows, torch.tensor(rows, dtype=torch.int64, device=DEV)


def report(case, t0, **figures):
    print(f"{case['name']}: N {case['N']}, {case['bytes'] / lc.GIB:.2f} GiB, {time.time() - t0:.1f} s; "
          + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))


@pytest.mark.timeout(120)
def test_curve():
    case = CASES["curve"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, K, w = case["N"], case["params"]["K"], case["width"]
    assert N * w > lc.EDGE
    try:
        g = gen(101)
        x = bufs["x"] = torch.empty(N, w, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, w, generator=g, device=DEV) / 5)          # curve_oracle.gauss's family
        rows, rt = probes(case)
        xp = x[rt].contiguous()
        xh = xp.cpu().numpy()
        target = torch.tensor([0.7, -1.1], device=DEV)
        worst = {}
        for P in case["params"]["P"]:                   # P = 2: every feature is (0, 0); P = 3: they depend on the row's x
            nbytes = lib.hint_curve_workspace_bytes(N, K, P)
            gy, gd, gm = nan_out(bufs, "y", 2 * N), nan_out(bufs, "dist", N), nan_out(bufs, "mean", 1)
            gw = nan_out(bufs, "workspace", nbytes // 4)
            desc = _lib.CurveDesc()
            desc.x, desc.n_rows, desc.n_coeffs, desc.n_points, desc.eps, desc.noise = x.data_ptr(), N, K, P, None, 0.0
            desc.target, desc.y, desc.dist, desc.mean = target.data_ptr(), gy.ptr, gd.ptr, gm.ptr
            desc.workspace, desc.workspace_bytes, desc.max_groups = gw.ptr, nbytes, 0
            _lib.check(lib.hint_curve_run(C.byref(desc), stream()), "hint_curve_run")
            torch.cuda.synchronize()
            check_written(bufs, ("y", "dist", "mean"), f"curve P {P}")
            y, d = gy.view(N, 2), gd.view(N)
            yp, dp = y[rt], d[rt]
            bad, worst[P] = co.band_check(xh, host(yp), P)
            assert len(bad) == 0, (P, [rows[i] for i in bad[:10]], worst[P])
            if P == 3:
                assert bool((yp != 0).any(dim=1).all())                                      # the features do depend on x
            ys, ds, _ = curves._run(xp, P, None, 0.0, target, True, False, 0)                 # the same rows as one small call
            assert bits_equal(ys, yp) and bits_equal(ds, dp), f"P {P}: a probe row's bits depend on its position"
            d64 = co.distances64(host(yp), host(target))
            assert (np.abs(host(dp) - d64) <= 4 * U * d64).all()
            m64 = lc.sum64_chunked(d) / N                # float64 of the kernel's own dist, which the probe rows check
            assert abs(float(gm.t[0]) - m64) <= 2.0 ** -23 * m64, (P, float(gm.t[0]), m64)
        report(case, t0, **{f"band_P{P}": v for P, v in worst.items()})
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_hausdorff_points():
    case = CASES["hausdorff_points"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, w = case["N"], case["width"]
    K, P, M = (case["params"][k] for k in ("K", "P", "M"))
    assert N * w > lc.EDGE
    try:
        g = gen(201)
        scale = torch.tensor(np.tile(co.GAUSS_W5, 4), dtype=torch.float32, device=DEV)
        x = bufs["x"] = torch.empty(N, 4 * K, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, 4 * K, generator=g, device=DEV) * scale)
        pr = bufs["params"] = torch.empty(N, 4, device=DEV)                                  # hausdorff_oracle.golden_params's ranges
        pr[:, :2] = 0.3 * torch.randn(N, 2, generator=g, device=DEV)
        pr[:, 2] = 0.5 + 2.0 * torch.rand(N, generator=g, device=DEV)
        pr[:, 3] = (2 * torch.rand(N, generator=g, device=DEV) - 1) * np.pi
        tpl = ho.lens_template(M)
        td = torch.from_numpy(tpl).to(DEV)
        gp = nan_out(bufs, "points", N * w)
        gmh, gav, gch = nan_out(bufs, "max_h", N), nan_out(bufs, "avg_h", N), nan_out(bufs, "chamfer", 2 * N)
        desc = _lib.HausdorffDesc()
        desc.x, desc.b_points, desc.n_rows, desc.n_coeffs, desc.n_points = x.data_ptr(), None, N, K, P
        desc.a_points, desc.a_offsets, desc.a_params, desc.n_template = td.data_ptr(), None, pr.data_ptr(), M
        desc.max_h, desc.avg_h, desc.chamfer, desc.points, desc.max_groups = gmh.ptr, gav.ptr, gch.ptr, gp.ptr, 0
        _lib.check(lib.hint_hausdorff_run(C.byref(desc), stream()), "hint_hausdorff_run")
        torch.cuda.synchronize()
        check_written(bufs, ("points", "max_h", "avg_h", "chamfer"), "hausdorff")
        rows, rt = probes(case)
        xp, prp = x[rt].contiguous(), pr[rt].contiguous()
        out = (gmh.view(N)[rt], gav.view(N)[rt], gch.view(N, 2)[rt], gp.view(N, P, 2)[rt])
        xh = xp.cpu().numpy()
        ref = ho.distances64(xh, tpl, prp.cpu().numpy(), P=P)
        bad, worst = ho.check(ref, host(out[0]), host(out[1]), host(out[2]))
        assert len(bad) == 0, ([rows[i] for i in bad[:10]], worst)
        dB = (2 * K + 2) * U * co.scale(xh)
        err = np.abs(host(out[3]) - co.points64(xh, P)).max((1, 2))
        assert (err <= dB).all(), [rows[i] for i in np.nonzero(err > dB)[0][:10]]
        small = curves._hd_run(xp, K, P, td, None, prp, True, True, True, 0)                  # the same rows as one small call
        for a, b, name in zip(small, out, ("max_h", "avg_h", "chamfer", "points")):
            assert bits_equal(a, b), f"{name}: a probe row's bits depend on its position"
        report(case, t0, rule=worst, points=float((err / dB).max()))
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_hausdorff_ragged():
    """ragged templates: a_points [T, 2] with T > 2^30 points, so the int64 offsets themselves pass 2^30 and the element index of
    a row's first template point passes 2^31"""
    case = CASES["hausdorff_ragged"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, K, P, T = case["N"], case["params"]["K"], case["params"]["P"], case["params"]["T"]
    assert 2 * T > lc.EDGE and T > 1 << 30 and T == lc.ragged_offset(N)
    try:
        g = gen(211)
        a = bufs["a_points"] = torch.empty(T, 2, device=DEV)
        lc.fill_chunked(a, lambda n: torch.randn(n, 2, generator=g, device=DEV))
        off = bufs["a_offsets"] = torch.empty(N + 1, dtype=torch.int64, device=DEV)
        step = lc.CHUNK_ELEMS // 2
        for lo in range(0, N + 1, step):
            n = torch.arange(lo, min(N + 1, lo + step), dtype=torch.int64, device=DEV)
            off[lo:lo + step] = 3 * n + (n + 4) // 5
        assert int(off[0]) == 0 and int(off[-1]) == T
        x = bufs["x"] = torch.empty(N, 4 * K, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, 4 * K, generator=g, device=DEV))
        gmh, gav = nan_out(bufs, "max_h", N), nan_out(bufs, "avg_h", N)
        desc = _lib.HausdorffDesc()
        desc.x, desc.b_points, desc.n_rows, desc.n_coeffs, desc.n_points = x.data_ptr(), None, N, K, P
        desc.a_points, desc.a_offsets, desc.a_params, desc.n_template = a.data_ptr(), off.data_ptr(), None, T
        desc.max_h, desc.avg_h, desc.chamfer, desc.points, desc.max_groups = gmh.ptr, gav.ptr, None, None, 0
        _lib.check(lib.hint_hausdorff_run(C.byref(desc), stream()), "hint_hausdorff_run")
        torch.cuda.synchronize()
        check_written(bufs, ("max_h", "avg_h"), "ragged hausdorff")
        rows, rt = probes(case)
        lens = [lc.ragged_offset(r + 1) - lc.ragged_offset(r) for r in rows]
        assert set(lens) == {3, 4}
        o2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = torch.cat([torch.arange(lc.ragged_offset(r), lc.ragged_offset(r + 1), device=DEV) for r in rows])
        assert torch.equal(off[rt], torch.tensor([lc.ragged_offset(r) for r in rows], device=DEV))
        tp, xp = a[take].contiguous(), x[rt].contiguous()                                    # the probe rows' templates, compacted
        out = (gmh.view(N)[rt], gav.view(N)[rt])
        ref = ho.distances64(xp.cpu().numpy(), tp.cpu().numpy(), None, o2, P=P)
        bad, worst = ho.check(ref, host(out[0]), host(out[1]))
        assert len(bad) == 0, ([rows[i] for i in bad[:10]], worst)
        small = curves._hd_run(xp, K, P, tp, torch.from_numpy(o2).to(DEV), None, True, False, False, 0)
        assert bits_equal(small[0], out[0]) and bits_equal(small[1], out[1]), "a probe row's bits depend on its position"
        report(case, t0, rule=worst)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_plus():
    case = CASES["plus"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, w = case["N"], case["width"]
    K, P, md = (case["params"][k] for k in ("K", "P", "max_dist"))
    assert N * w > lc.EDGE
    try:
        g = gen(221)
        u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, device=DEV)        # noqa: E731
        pr = bufs["params"] = torch.empty(N, 9, device=DEV)                                  # plus_oracle.draw_params's ranges
        for col, (lo, hi) in enumerate(((3, 6), (3, 6), (.4, 2.2), (.4, 2.2), (-1.5, 1.5), (-1.5, 1.5))):
            pr[:, col] = u(N, lo, hi)
        pr[:, 6:8] = 0.5 * torch.randn(N, 2, generator=g, device=DEV)
        pr[:, 8] = u(N, -np.pi, np.pi)
        x = bufs["x"] = torch.empty(N, 4 * K, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, 4 * K, generator=g, device=DEV) * 0.6)   # curves of the outline's size
        gs, gk, gc_ = nan_out(bufs, "segments", N * w), nan_out(bufs, "keep", N, torch.int32), nan_out(bufs, "counts", 12 * N, torch.int32)
        gl, gmh, gav = nan_out(bufs, "loss", 2 * N), nan_out(bufs, "max_h", N), nan_out(bufs, "avg_h", N)
        desc = _lib.PlusDesc()
        desc.x, desc.b_points, desc.n_rows, desc.n_coeffs, desc.n_points = x.data_ptr(), None, N, K, P
        desc.params, desc.max_dist, desc.max_groups = pr.data_ptr(), md, 0
        desc.segments, desc.keep, desc.counts, desc.loss, desc.max_h, desc.avg_h = gs.ptr, gk.ptr, gc_.ptr, gl.ptr, gmh.ptr, gav.ptr
        _lib.check(lib.hint_plus_run(C.byref(desc), stream()), "hint_plus_run")
        torch.cuda.synchronize()
        check_written(bufs, ("segments", "keep", "counts", "loss", "max_h", "avg_h"), "plus")
        rows, rt = probes(case)
        xp, prp = x[rt].contiguous(), pr[rt].contiguous()
        out = dict(segments=gs.view(N, 12, 2, 2)[rt], keep=gk.view(N)[rt], counts=gc_.view(N, 12)[rt], loss=gl.view(N, 2)[rt],
                   max_h=gmh.view(N)[rt], avg_h=gav.view(N)[rt])
        prh = prp.cpu().numpy()
        assert (po.half_gap(prh, md) > 1e-3).all()                                            # float64 and fp32 counts must agree
        ref = po.plus64(prh, xp.cpu().numpy(), P, md)
        assert np.array_equal(out["keep"].cpu().numpy(), ref["keep"]) and np.array_equal(out["counts"].cpu().numpy(), ref["counts"])
        bad, worst = po.check(ref, segments=host(out["segments"]), loss=host(out["loss"]), max_h=host(out["max_h"]),
                              avg_h=host(out["avg_h"]))
        assert len(bad) == 0, ([rows[i] for i in bad[:10]], worst)
        small = curves._plus_run(prp, xp, K, P, md, tuple(out), 0, None)                      # the same rows as one small call
        for name in out:
            same = torch.equal(small[name].view(torch.int32), out[name].view(torch.int32))
            assert same, f"{name}: a probe row's bits depend on its position"
        report(case, t0, rule=worst)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_overlap():
    case = CASES["overlap"]
    lc.require_memory(case)
    bufs, t0 = {}, time.time()
    N, w = case["N"], case["width"]
    K, P, M = (case["params"][k] for k in ("K", "P", "M"))
    assert N * w > lc.EDGE
    try:
        g = gen(801)
        x = bufs["x"] = torch.empty(N, 4 * K, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, 4 * K, generator=g, device=DEV))
        tpl = oo.polygon_template(M)
        td = torch.from_numpy(tpl).to(DEV)
        ga = nan_out(bufs, "areas", N * w)
        curves._ov_run(x, K, P, td, None, None, None, ("areas",), 0, dict(areas=ga.view(N, 3)))
        torch.cuda.synchronize()
        check_written(bufs, ("areas",), "overlap")
        rows, rt = probes(case)
        xp = x[rt].contiguous()
        got = ga.view(N, 3)[rt]
        small = curves._ov_run(xp, K, P, td, None, None, None, ("areas",), 0, None)["areas"]
        assert bits_equal(small, got), "a probe row's bits depend on its position"
        xh, gh = host(xp), host(got)
        worst = 0.0
        for i in range(len(rows)):
            pts = np.tile(xh[i, :2], (P, 1))                                                  # K = 1: every vertex is (re x, re y), exactly
            ref = oo.overlap64(pts, tpl)
            r = oo.ratio(ref, dict(area_T=gh[i, 0], area_C=gh[i, 1], I=gh[i, 2]))
            assert r <= 1.0, (rows[i], r, ref, gh[i])
            worst = max(worst, r)
        assert (gh[:, 0] > 0).all() and len(set(gh[:, 0].tolist())) > 1                        # the rows are not all one value
        report(case, t0, rule=worst)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("kind", ("lensfit", "plusfit"))
def test_fit_trace(kind):
    """a fit whose trace passes 2^31 elements (no early stop: stop_loss = 0; a constant corner weight).  On the probe rows: every
    output bit for bit the one of a small call; on every eighth of them and on the crossing rows the update rule over the whole
    trace, and the traced (p, L, g) of the first, middle and last steps against the float64 evaluation at the traced p"""
    case = CASES[kind]
    lc.require_memory(case)
    bufs, t0 = {}, time.time()
    N, w = case["N"], case["width"]
    K, P, S, steps, M, n_par = (case["params"][k] for k in ("K", "P", "S", "n_steps", "M", "n_par"))
    assert N * w > lc.EDGE and w == S * steps * (2 * n_par + 1)
    lens = kind == "lensfit"
    # the lens fit of a curve of one distinct point (P = 2) ends with the prototype shrunk onto that point, where no nearest point
    # is decided at the oracle's bound: a fiftieth of the reference's rates keeps the 128 steps in the starts' neighbourhood
    sched = dict(lr=lo.LR / 50, angle_lr=lo.ANGLE_LR / 50, gamma=lo.GAMMA, momentum=lo.MOMENTUM) if lens else \
        dict(lr=pfo.LR, angle_lr=pfo.ANGLE_LR, gamma=pfo.GAMMA, momentum=pfo.MOMENTUM)
    try:
        g = gen(601 if lens else 701)
        u = lambda n, a, b: a + (b - a) * torch.rand(n, generator=g, device=DEV)             # noqa: E731
        scale = torch.tensor(np.tile(co.GAUSS_W5, 4), dtype=torch.float32, device=DEV) * (1.0 if lens else 3.0)
        x = bufs["x"] = torch.empty(N, 4 * K, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, 4 * K, generator=g, device=DEV) * scale)
        starts = bufs["starts"] = torch.empty(N, S, n_par, device=DEV)
        if lens:                                          # lensfit_oracle.golden_grad_params's ranges
            starts[..., :2] = 0.3 * torch.randn(N, S, 2, generator=g, device=DEV)
            starts[..., 2] = u(N * S, 0.7, 2.2).view(N, S)
            starts[..., 3] = u(N * S, -np.pi, np.pi).view(N, S)
            proto = lo.lens_prototype(M)
        else:                                             # plus_oracle.draw_params's ranges
            for col, (a, b) in enumerate(((3, 6), (3, 6), (.4, 2.2), (.4, 2.2), (-1.5, 1.5), (-1.5, 1.5))):
                starts[..., col] = u(N * S, a, b).view(N, S)
            starts[..., 6:8] = 0.5 * torch.randn(N, S, 2, generator=g, device=DEV)
            starts[..., 8] = u(N * S, -np.pi, np.pi).view(N, S)
        shapes = dict(params=(N, n_par), loss=(N,), best=(N,), all_params=(N, S, n_par), all_loss=(N, S), grad=(N, S, n_par),
                      trace=(N, S, steps, 2 * n_par + 1))
        if not lens:
            shapes["n_run"] = (N,)
        ints = ("best", "n_run")
        out = {}
        for name, shape in shapes.items():
            gb = nan_out(bufs, name, int(np.prod(shape)), torch.int32 if name in ints else torch.float32)
            out[name] = gb.view(*shape)

        def run(curve, st, into=None):
            if lens:
                return curves._lf_run(curve, K, P, pd, st, steps, weight=1.0, want=tuple(shapes), out=into, **sched)
            return curves._pf_run(curve, K, P, st, steps, corner_weight=1.0, corner_decay=False, stop_loss=0.0, want=tuple(shapes),
                                  out=into, **sched)
        pd = torch.from_numpy(proto).to(DEV) if lens else None
        run(x, starts, out)
        torch.cuda.synchronize()
        check_written(bufs, tuple(shapes), kind)
        rows, rt = probes(case)
        xp, sp = x[rt].contiguous(), starts[rt].contiguous()
        small = run(xp, sp)
        for name in shapes:
            same = torch.equal(small[name].view(torch.int32), out[name][rt].view(torch.int32))
            assert same, f"{name}: a probe row's bits depend on its position"
        if not lens:
            assert bool((out["n_run"][rt] == S).all())                                        # nothing stopped early
        tr, ap = small["trace"].cpu().numpy(), small["all_params"].cpu().numpy()
        assert np.isfinite(tr).all()
        assert torch.equal(small["trace"][:, :, 0, :n_par].view(torch.int32), sp.view(torch.int32))    # a fit begins at its start
        sub = sorted({i for i in range(0, len(rows), 8)} | {rows.index(r + o) for r in case["crossings"] for o in (-1, 0)})
        xh = xp.cpu().numpy()
        b, dB = co.points64(xh, P), (lo.delta_B(xh) if lens else pfo.delta_B(xh))
        at = [0, 1, 2, steps // 2, steps - 2, steps - 1]
        rule, und, total, rl, rg = 0.0, 0, 0, 0.0, 0.0
        for i in sub:
            for s in range(S):
                rule = max(rule, (lo if lens else pfo).check_update_rule(tr[i, s], ap[i, s], **sched))
            rec = tr[i][:, at].reshape(-1, 2 * n_par + 1)
            pp, LL, gg = rec[:, :n_par], rec[:, n_par], rec[:, n_par + 1:]
            u_, l_, g_ = lo.compare_evaluations(proto, b[i], dB[i], 1.0, pp, LL, gg) if lens else \
                pfo.compare_evaluations(b[i], dB[i], 1.0, pp, LL, gg)
            und, total, rl, rg = und + u_, total + len(pp), max(rl, l_), max(rg, float(np.max(g_)))
        assert rule <= 1.0, rule
        assert und <= 0.25 * total, (und, total)                                              # the cap of the fits' own tests
        assert rl <= 1.0 and rg <= 1.0, (rl, rg)
        report(case, t0, update_rule_ulp=rule, loss=rl, grad=rg, undecided=und / total)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_lensgen():
    case = CASES["lensgen"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, w, seed, off = case["N"], case["width"], case["params"]["seed"], case["params"]["offset"]
    assert N * w > lc.EDGE and off < 2 ** 32 < off + N                                       # the high word changes mid-call
    try:
        nbytes = lib.hint_lensgen_workspace_bytes(N)
        gx, gr = nan_out(bufs, "x", 20 * N), nan_out(bufs, "ring", w * N)
        gc_, ge = nan_out(bufs, "counts", N, torch.int32), nan_out(bufs, "eps", 2 * N)
        gdr, gw = nan_out(bufs, "draws_out", 4 * N), nan_out(bufs, "workspace", nbytes // 4, torch.int32)
        desc = _lib.LensGenDesc()
        desc.n_rows, desc.seed, desc.offset, desc.max_groups, desc.draws = N, seed, off, 0, None
        desc.x, desc.ring, desc.counts, desc.eps, desc.draws_out = gx.ptr, gr.ptr, gc_.ptr, ge.ptr, gdr.ptr
        desc.workspace, desc.workspace_bytes = gw.ptr, nbytes
        _lib.check(lib.hint_lensgen_run(C.byref(desc), stream()), "hint_lensgen_run")
        torch.cuda.synchronize()
        check_written(bufs, ("x", "ring", "counts", "eps", "draws_out", "workspace"), "lensgen")
        assert int(gw.words.sum()) == 0                                                      # no Philox row is rejected
        flip = 2 ** 32 - off                                                                 # the first row of high word 1
        rows, rt = probes(case, extra=(flip - 2, flip - 1, flip, flip + 1))
        x, ring, cnt, eps = gx.view(N, 20), gr.view(N, 32, 2), gc_.view(N), ge.view(N, 2)
        for first, n in lc.runs_of(rows):                                                    # a small call at offset + row
            xs, _, es = hint_amd.sample_lens_joint(n, seed, 0.0, offset=off + first, device=DEV, return_eps=True)
            x2, rs, cs = hint_amd.sample_lens_prior(n, seed, offset=off + first, device=DEV, return_ring=True)
            sl = slice(first, first + n)
            assert bits_equal(xs, x[sl]) and bits_equal(x2, x[sl]) and bits_equal(rs, ring[sl]), first
            assert torch.equal(cs, cnt[sl]) and bits_equal(es, eps[sl]), first
        d = gdr.view(N, 4)[rt].cpu().numpy()
        x64, ring64, cnt64 = so.sample(d)
        keep = ~so.ambiguous(d)
        assert (~keep).mean() <= so.MAX_AMBIGUOUS
        xh, rh, ch = host(x[rt]), host(ring[rt]), cnt[rt].cpu().numpy()
        assert set(ch.tolist()) <= {31, 32} and (ch[keep] == cnt64[keep]).all()
        A = so.scale(ring64)
        e_ring = np.abs(rh - ring64).reshape(len(rows), -1).max(axis=1) / (U * A)
        e_x = np.abs(xh - x64).max(axis=1) / (U * A)
        assert (e_ring[keep] <= so.K_RING).all() and (e_x[keep] <= so.K_COEF).all()
        at = 0
        for first, n in lc.runs_of(rows):                                                    # the draws are the oracle's Philox at
            ur, ut = so.uniforms(seed, off + first, n)                                       # counter offset + row, high word included
            assert (d[at:at + n, 0] == ur).all() and (d[at:at + n, 1] == ut).all(), first
            at += n
        report(case, t0, ring=float(e_ring[keep].max()), coeffs=float(e_x[keep].max()))
    finally:
        lc.release(bufs)


PLUSGEN_TABLE = dict(x=((100,), torch.float32), y=((4,), torch.float32), outline=((128, 2), torch.float32), counts=((), torch.int32),
                     corners=((), torch.int32), draws_out=((9,), torch.float32))
NORMAL_BOUND = 2.0 ** -13            # the hardware's log2 / sin / cos, as tests/test_gpu_plusgen.py holds the sampler's normals


def plusgen_case(name):
    """hint_plusgen_run with one wide array (the other NULL) past 2^31 elements, the Philox row counter's high word changing inside
    the call.  On the probe rows and the four rows around the flip: the bits of small calls of the public samplers at offset +
    first (a row is a function of (seed, row) alone), the draws the oracle's Philox at offset + row, and the float64 oracle under
    its own rule on the rows that are not ambiguous"""
    case = CASES[name]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, w, named, seed, off = case["N"], case["width"], case["named"], case["params"]["seed"], case["params"]["offset"]
    assert N * w > lc.EDGE and off < 2 ** 32 < off + N                                       # the high word changes mid-call
    try:
        nbytes = lib.hint_plusgen_workspace_bytes(N)
        desc = _lib.PlusGenDesc()
        desc.n_rows, desc.seed, desc.offset, desc.max_groups, desc.draws, desc.rows, desc.target = N, seed, off, 0, None, None, None
        out = {}
        for field, (shape, dtype) in PLUSGEN_TABLE.items():
            elems = dict((a, n) for a, n, _ in case["arrays"]).get(field)
            if elems is None:
                setattr(desc, field, None)
                continue
            assert elems == N * int(np.prod(shape))
            g = nan_out(bufs, field, elems, dtype)
            setattr(desc, field, g.ptr)
            out[field] = g.view(N, *shape)
        assert named in out and ("x" in out) != ("outline" in out)
        gw = nan_out(bufs, "workspace", nbytes // 4, torch.int32)
        desc.workspace, desc.workspace_bytes, desc.stream = gw.ptr, nbytes, stream()
        _lib.check(lib.hint_plusgen_run(C.byref(desc)), "hint_plusgen_run")
        torch.cuda.synchronize()
        check_written(bufs, tuple(out) + ("workspace",), name)
        assert int(gw.words.sum()) == 0                                                      # no Philox row is rejected
        flip = 2 ** 32 - off                                                                 # the first row of high word 1
        rows, rt = probes(case, extra=(flip - 2, flip - 1, flip, flip + 1))
        assert {flip - 2, flip - 1, flip, flip + 1} <= set(rows)
        for first, n in lc.runs_of(rows):                                                    # small calls at offset + first
            sl = slice(first, first + n)
            xs, ys = hint_amd.sample_plus_joint(n, seed, offset=off + first, device=DEV)
            assert bits_equal(ys, out["y"][sl]), first
            if named == "x":
                assert bits_equal(xs, out["x"][sl]) and bits_equal(hint_amd.sample_plus_prior(n, seed, offset=off + first, device=DEV),
                                                                   out["x"][sl]), first
            else:
                _, o2, c2 = hint_amd.sample_plus_prior(n, seed, offset=off + first, device=DEV, return_outline=True)
                o3, c3, y3 = hint_amd.plus_outlines(out["draws_out"][sl].contiguous())
                assert bits_equal(o2, out["outline"][sl]) and torch.equal(c2, out["counts"][sl]), first
                assert bits_equal(o3, out["outline"][sl]) and torch.equal(c3, out["counts"][sl]) and bits_equal(y3, out["y"][sl]), first
        d = out["draws_out"][rt].cpu().numpy()
        at, e_normal = 0, 0.0
        for first, n in lc.runs_of(rows):                                                    # the draws are the oracle's Philox at
            want_d = pgo.draws(seed, off + first, n)                                         # counter offset + row, high word included
            assert (d[at:at + n, :7] == want_d[:, :7].astype(np.float32)).all(), first       # exact: part of the definition
            e_normal = max(e_normal, float(np.abs(d[at:at + n, 7:] - want_d[:, 7:]).max()))
            at += n
        assert e_normal <= NORMAL_BOUND, e_normal
        want = pgo.sample(d)
        keep = ~pgo.ambiguous(d)
        assert (~keep).mean() <= pgo.MAX_AMBIGUOUS
        # (the oracle's rule takes every output: what this case leaves NULL is given as the oracle's own, and not reported)
        got = {k: (out[k][rt].cpu().numpy() if k in out else want[k]) for k in ("x", "y", "outline", "counts")}
        if "corners" in out:
            c = out["corners"][rt].cpu().numpy()
            got["corners"] = c & 15
            assert ((c >> 4)[keep] == want["arms"][keep]).all()
            cnt = got["counts"]
            assert all((got["outline"][i, cnt[i]:] == 0).all() for i in range(len(rows)))    # zero padding behind the outline
        else:
            got["corners"] = want["corners"]
        res = pgo.compare(got, want, keep)
        assert pgo.passes(res), res
        given = set(out) | {"center", "angle", "ratio"}
        report(case, t0, normals=e_normal, ambiguous=float((~keep).mean()), **{k: v for k, v in res.items() if k in given})
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_plusgen_outline():
    plusgen_case("plusgen_outline")


@pytest.mark.timeout(120)
def test_plusgen_x():
    plusgen_case("plusgen_x")


@pytest.mark.timeout(120)
def test_fcoef():
    case = CASES["fcoef"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, w, p_max, K = case["N"], case["width"], case["params"]["p_max"], case["params"]["K"]
    assert N * w > lc.EDGE
    try:
        g = gen(301)
        pts = bufs["points"] = torch.empty(N, p_max, 2, device=DEV)
        lc.fill_chunked(pts, lambda n: torch.randn(n, p_max, 2, generator=g, device=DEV))
        cnt = bufs["counts"] = torch.randint(K, p_max + 1, (N,), generator=g, device=DEV, dtype=torch.int32)    # ragged
        cnt[:3] = torch.tensor([K, p_max, p_max - 1], dtype=torch.int32)
        cnt[-2:] = torch.tensor([p_max, K], dtype=torch.int32)
        nbytes = lib.hint_fcoef_workspace_bytes(N, p_max, K)
        gx, gw = nan_out(bufs, "x", 4 * K * N), nan_out(bufs, "workspace", nbytes // 4, torch.int32)
        desc = _lib.FcoefDesc()
        desc.points, desc.counts, desc.n_rows, desc.p_max, desc.n_coeffs = pts.data_ptr(), cnt.data_ptr(), N, p_max, K
        desc.x, desc.workspace, desc.workspace_bytes, desc.max_groups = gx.ptr, gw.ptr, nbytes, 0
        _lib.check(lib.hint_fcoef_run(C.byref(desc), stream()), "hint_fcoef_run")
        torch.cuda.synchronize()
        check_written(bufs, ("x", "workspace"), "fcoef")
        assert int(gw.words.sum()) == 0                                                      # no row is rejected
        rows, rt = probes(case)
        ph, chh, xh = host(pts[rt]), cnt[rt].cpu().numpy(), host(gx.view(N, 4 * K)[rt])
        want = so.coeffs(ph, chh, K)
        worst = 0.0
        for i, c in enumerate(chh):
            e = np.abs(xh[i] - want[i]).max() / (U * np.abs(ph[i, :c]).max())
            worst = max(worst, e / so.k_fcoef(c))
            assert e <= so.k_fcoef(c), (rows[i], int(c), e)
        report(case, t0, coeffs_over_bound=worst)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_abc():
    case = CASES["abc"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, ny, k = case["N"], case["params"]["ny"], case["params"]["k"]
    assert N * ny > lc.EDGE and N == case["limit"]
    try:
        g = gen(401)
        t = torch.tensor([1.0, -2.0, 0.5], device=DEV)
        y = bufs["y"] = torch.empty(N, ny, device=DEV)

        def background(n):                               # every row at distance >= 10: the first coordinate alone is that far
            b = torch.randn(n, ny, generator=g, device=DEV)
            b[:, 0] = t[0] + 10.0 + 5.0 * torch.rand(n, generator=g, device=DEV)
            return b
        lc.fill_chunked(y, background)
        plant = lc.abc_plant_rows(case)
        order = np.random.RandomState(5).permutation(k)                                      # distances not in row order
        r = (order + 1) / 128.0                                                              # distinct, < 1, exact in fp32
        yp = t[None, :].repeat(k, 1)
        yp[:, 0] += torch.tensor(r, dtype=torch.float32, device=DEV)
        y[torch.tensor(plant, device=DEV)] = yp
        D64, rank = ao.order64(yp.cpu().numpy(), t.cpu().numpy())                             # from the planted rows alone
        want_idx, want_dist = np.asarray(plant, dtype=np.int64)[rank], np.sqrt(D64[rank])
        nearest = float("inf")
        step = lc.CHUNK_ELEMS // 4 // ny
        keep = torch.ones(N, dtype=torch.bool, device=DEV)
        keep[torch.tensor(plant, device=DEV)] = False
        for a in range(0, N, step):                                                          # the background really is far
            D = ((y[a:a + step].double() - t.double()) ** 2).sum(1)
            nearest = min(nearest, float(D[keep[a:a + step]].min()))
        del keep
        assert nearest > float(D64.max()) and nearest >= 100.0
        nbytes = lib.hint_abc_workspace_bytes(N, ny, k)
        gi, gd = nan_out(bufs, "idx", k, torch.int32), nan_out(bufs, "dist", k)
        gw = nan_out(bufs, "workspace", nbytes // 4, torch.int32)
        desc = _lib.AbcDesc()
        desc.y, desc.target, desc.n_rows, desc.ny, desc.k = y.data_ptr(), t.data_ptr(), N, ny, k
        desc.idx, desc.dist, desc.workspace, desc.workspace_bytes = gi.ptr, gd.ptr, gw.ptr, nbytes
        _lib.check(lib.hint_abc_run(C.byref(desc), stream()), "hint_abc_run")
        torch.cuda.synchronize()
        check_written(bufs, ("idx", "dist"), "abc")
        idx, dist = gi.view(k).cpu().numpy().astype(np.int64), host(gd.view(k))
        assert (idx == want_idx).all(), (idx, want_idx)
        err = np.abs(dist - want_dist)
        assert (err <= (ny + 4) * 2.0 ** -23 * want_dist).all()                               # abc_oracle.check_rule's bound
        # the Python wrappers: int64 idx, and the gather of quantile_abc at rows past 2^29
        idx2, dist2 = hint_amd.nearest_rows(y, t, k)
        assert idx2.dtype == torch.int64 and (idx2.cpu().numpy() == want_idx).all() and bits_equal(dist2, gd.view(k))
        xs = bufs["x"] = torch.arange(N, dtype=torch.int32, device=DEV)
        sample, thr = hint_amd.quantile_abc(xs, y, t, n=k - 2, skip=1)
        assert (sample.cpu().numpy() == want_idx[1:k - 1]).all() and float(thr) == float(gd.view(k)[k - 1])
        report(case, t0, dist_rel=float((err / want_dist).max()), background=nearest)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_corr():
    case = CASES["corr"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, d = case["N"], case["params"]["d"]
    assert N * d > lc.EDGE and N <= case["limit"]
    try:
        g = gen(501)
        A = torch.randn(d, d, generator=g, device=DEV) / d ** 0.5 + 0.5 * torch.eye(d, device=DEV)
        b = torch.randn(d, generator=g, device=DEV)
        x = bufs["x"] = torch.empty(N, d, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, d, generator=g, device=DEV) @ A + b, 1 << 26)      # dense mixing: no r near 0
        # the reference: float64 on the device, the rows in chunks of c - column means first, then the Gram matrix of the centred
        # rows as a sum of per-chunk Gram matrices: an entry is chains of c fused multiply-adds plus the sum of the chunks
        c = 1 << 15
        chunks = -(-N // c)
        mean = torch.zeros(d, dtype=torch.float64, device=DEV)
        for a in range(0, N, c):
            mean += x[a:a + c].double().sum(0)
        mean /= N
        S = torch.zeros(d, d, dtype=torch.float64, device=DEV)
        for a in range(0, N, c):
            u = x[a:a + c].double() - mean
            S += u.t() @ u
        sd = S.diagonal().sqrt()
        r64 = (S / (sd[:, None] * sd[None, :])).clamp(-1, 1)
        tgt = bufs["target"] = torch.eye(d, dtype=torch.float64, device=DEV)
        nbytes = lib.hint_corr_workspace_bytes(N, d)
        gc_, go = nan_out(bufs, "corr", 2 * d * d, torch.float64), nan_out(bufs, "out", 8, torch.float64)
        gw = nan_out(bufs, "workspace", nbytes // 4)
        desc = _lib.CorrDesc()
        desc.x, desc.n, desc.d, desc.target, desc.corr, desc.out = x.data_ptr(), N, d, tgt.data_ptr(), gc_.ptr, go.ptr
        desc.workspace, desc.workspace_bytes = gw.ptr, nbytes
        _lib.check(lib.hint_corr_run(C.byref(desc), stream()), "hint_corr_run")
        torch.cuda.synchronize()
        check_written(bufs, ("corr", "out"), "corr")
        got = gc_.view(d, d)
        _, R, slabs = cro.geometry(N, d)
        # corr_oracle's bound of a device entry, plus the same first-order bound for the reference's own sums
        bound = (R + slabs + 16) * 2.0 ** -52 + (c + chunks + 16) * 2.0 ** -52
        err = float((got - r64).abs().max())
        assert err <= bound, (err, bound)
        assert torch.equal(got, got.t())
        out = go.view(4).cpu().numpy()
        df = got - tgt
        mse = float((df * df).sum() / (d * d))                                               # float64 of the kernel's own corr
        # two sums of d^2 non-negative terms in double, in two orders: each within d^2 2^-53 relative of the exact sum
        assert out[2] == d * d and out[3] == 0 and abs(out[0] - mse) <= 2 * d * d * 2.0 ** -53 * mse, (out, mse)
        assert abs(out[0] - out[1] / out[2]) <= 2.0 ** -52 * out[0]
        report(case, t0, entry_err=err, bound=bound)
    finally:
        lc.release(bufs)


@pytest.mark.timeout(120)
def test_epoch():
    """the three epoch ops in turn on one table x [N, 100] past 2^31 elements, the output re-poisoned between them.
    GATHER, a whole shuffled epoch (count = N: the output's element offsets base * d pass 2^31 as the source's do): the indices
    are a permutation and the oracle's at the probe positions, every row of the output is x.index_select's bit for bit.
    MOMENTS over all rows (the slab cap: 1024 slabs of far more than 256 rows): against float64 column sums made on the device in
    chunks, within the 2 E_m and 2 E_s tests/epoch_oracle.py derives, evaluated for this N; two runs give equal bits.
    STANDARDIZE out of place (the tile loop's later trips): every element torch's double arithmetic, bit for bit"""
    case = CASES["epoch"]
    lc.require_memory(case)
    lib, bufs, t0 = _lib.load(), {}, time.time()
    N, d, seed, epoch = case["N"], case["params"]["d"], case["params"]["seed"], case["params"]["epoch"]
    dev = torch.device(DEV)
    assert N * d > lc.EDGE and case["width"] == d
    try:
        g = gen(901)
        x = bufs["x"] = torch.empty(N, d, device=DEV)
        lc.fill_chunked(x, lambda n: torch.randn(n, d, generator=g, device=DEV).mul_(3.0).add_(1.5))
        go, gi = nan_out(bufs, "out_x", N * d), nan_out(bufs, "indices_out", 2 * N, torch.int32)
        nbytes = lib.hint_epoch_workspace_bytes(_lib.EPOCH_GATHER, N, N, d)
        gw = nan_out(bufs, "workspace", nbytes // 4, torch.int32)
        out, idx = go.view(N, d), gi.words.view(torch.int64)
        # ---- gather ----
        data._gather_run(x, None, N, seed, epoch, True, (0, N, 0, 0), dev, want=("out_x", "indices_out"),
                         out=dict(out_x=out, indices_out=idx, workspace=gw.t))
        torch.cuda.synchronize()
        check_written(bufs, ("out_x", "indices_out", "workspace"), "epoch gather")
        assert int(gw.words.sum()) == 0                                                      # no position is rejected
        assert torch.equal(idx.sort().values, torch.arange(N, device=DEV))                   # a permutation of the rows
        rows, rt = probes(case)
        want = eo.source_rows(N, seed, epoch, np.asarray(rows, dtype=np.uint64))
        assert torch.equal(idx[rt], torch.from_numpy(want).to(DEV))
        assert not torch.equal(idx[rt], rt)                                                  # (shuffled)
        step = lc.CHUNK_ELEMS // d
        for a in range(0, N, step):
            assert bits_equal(out[a:a + step], x.index_select(0, idx[a:a + step])), a
        # ---- moments ----
        gm, gs = nan_out(bufs, "mean", 2 * d, torch.int32), nan_out(bufs, "std", 2 * d, torch.int32)
        mbytes = lib.hint_epoch_workspace_bytes(_lib.EPOCH_MOMENTS, N, N, d)
        gmw = nan_out(bufs, "moments_workspace", mbytes // 4, torch.int32)
        ds = hint_amd.DeviceDataset(x, seed=seed)
        assert ds.x.data_ptr() == x.data_ptr()                                               # the table is used in place
        mean, std = ds.moments(0, N, out=dict(mean=gm.words.view(torch.float64), std=gs.words.view(torch.float64), workspace=gmw.t))
        torch.cuda.synchronize()
        check_written(bufs, ("mean", "std", "moments_workspace"), "epoch moments")
        cs = lc.CHUNK_ELEMS // 4 // d                                                        # a float64 temporary of 0.5 GiB
        zero = lambda: torch.zeros(d, dtype=torch.float64, device=DEV)                       # noqa: E731
        s1, sa, s2 = zero(), zero(), zero()
        for a in range(0, N, cs):
            v = x[a:a + cs].double()
            s1 += v.sum(0)
            sa += v.abs_().sum(0)
        m64, a64 = s1 / N, sa / N
        for a in range(0, N, cs):
            s2 += x[a:a + cs].double().sub_(m64).square_().sum(0)
        sd64 = (s2 / N).sqrt()
        e_m = (N + 1) * eo.U * a64                                                           # epoch_oracle's E_m and E_s for this N: the
        e_s = ((N + 4) / 2 + 1) * eo.U * (sd64 + e_m) + e_m                                  # device and the reference each stay within them
        dm, dsd = (mean - m64).abs(), (std - sd64).abs()
        assert bool((dm <= 2 * e_m).all()) and bool((dsd <= 2 * e_s).all()), (dm / e_m, dsd / e_s)
        assert float((2 * e_m / a64).max()) < 1e-8                                           # (256 rows left out move a mean by 1e-5 of it)
        m2, sd2 = ds.moments(0, N)
        assert bits_equal(m2, mean) and bits_equal(sd2, std)                                 # two runs: equal bits
        # ---- standardize, out of place ----
        go.fill("nan")
        assert ds.apply_moments(mean, std, out=out) is out
        torch.cuda.synchronize()
        check_written(bufs, ("out_x",), "epoch standardize")
        for a in range(0, N, cs):
            assert bits_equal(out[a:a + cs], x[a:a + cs].double().sub_(mean).div_(std).float()), a
        report(case, t0, mean_over_2Em=float((dm / (2 * e_m)).max()), std_over_2Es=float((dsd / (2 * e_s)).max()),
               Em_over_mean_abs=float((e_m / a64).max()))
    finally:
        lc.release(bufs)
