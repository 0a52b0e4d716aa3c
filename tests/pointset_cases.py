"""The cases of tests/golden/pointset_bits.npz and tests/golden/plusfit_bits.npz: small launches of hint_hausdorff_run,
hint_plus_run, hint_lensfit_run and hint_plusfit_run whose output bits were recorded once (tests/golden/make_pointset_bits.py) and
must never move again (tests/test_gpu_pointset_bits.py).  Every operation of the four kernels is a correctly rounded intrinsic in
an order that include/hint_amd.h fixes, so a change that only moves code changes no bit.

Every case has 5 rows on 2 workgroups: a workgroup takes 2-3 rows in turn and reuses its LDS between them.  The inputs come from
the oracles' seeded generators; the fixture keeps a sha256 of each, so that a drift of a generator is reported as such and not as
a change of the kernels.  Hausdorff (K, P, M): every K of 1, 5, 25; every P of 2, 100, 256, 257 (the step from one curve point a
thread to two), 1000, 1024; every M of 1, 1023, 1024, 1025 (around one LDS tile), 4096, the ragged case all five at once.  Plus:
the same K and P; max_dist steers the largest row's outline to one tile to the point, to one tile and two points (an outline's
edges come in pairs of equal count, so its size is always even: 1025 does not exist), to more than three tiles and to the most a
row may have, next to a row that is past it.  Lens fit (K, P, M, S starts, n_steps, weight): every K of 0 (given points), 1, 5, 25;
every number 1..4 of points a thread holds of the curve (P = 2, 100 / 257 / 600 / 1024) and of the prototype (M = 1, 130 / 300 /
700 / 1023, 1024); 1, 2 and 16 starts; the evaluation alone (n_steps 0, no trace), one step and five; both weights; all outputs,
and params and loss alone.  Plus fit (K, P, S starts, n_steps, corner weight, its decay, stop_loss): every K of 0, 1, 5, 25; every
number 1..4 of curve points a thread holds (P = 2, 100 / 257 / 600 / 1024); 1, 2, 3 and 16 starts; the evaluation alone, one step
and five; a row of zero width (ten kept segments) and a clamped row under the pinned steps; the decaying corner weight; an early
stop after one, two and three starts, with the starts that did not run; all outputs, and params and loss alone."""
import hashlib

import numpy as np

import curve_oracle as co
import hausdorff_oracle as ho
import lensfit_oracle as lo
import plus_oracle as po
import plusfit_oracle as pfo

ROWS, GROUPS = 5, 2
RAGGED = (1, 1023, 1024, 1025, 4096)
# name -> (seed, K (0: given points), P, M or None (points alone), mode)
HAUSDORFF = {
    "hd_k1_p2_m1": (1, 1, 2, 1, "shared"),
    "hd_k5_p100_m1023_params": (2, 5, 100, 1023, "params"),
    "hd_k25_p256_m1024": (3, 25, 256, 1024, "shared"),
    "hd_k5_p257_ragged": (4, 5, 257, sum(RAGGED), "ragged"),
    "hd_k25_p1000_m4096_params": (5, 25, 1000, 4096, "params"),
    "hd_given_p1024_m1025": (6, 0, 1024, 1025, "shared"),
    "hd_k25_p1024_points_alone": (7, 25, 1024, None, "points"),
}
PLUS_ALL = ("segments", "keep", "counts", "loss", "max_h", "avg_h")
# name -> (seed, K, P, the outline size of the largest row that is served, rows of zero width, the row past 4096 points, outputs)
PLUS = {
    "pl_k1_p2_m1024": (11, 1, 2, 1024, {}, None, PLUS_ALL),
    "pl_k5_p100_m1026": (12, 5, 100, 1026, {}, None, PLUS_ALL),
    "pl_k25_p256_m3500": (13, 25, 256, 3500, {}, None, PLUS_ALL),
    "pl_k5_p257_zero_width": (14, 5, 257, 2348, {1: (2,), 3: (2, 3)}, None, PLUS_ALL),
    "pl_k25_p1000_m4096_one_row_over": (15, 25, 1000, 4096, {}, 2, PLUS_ALL),
    "pl_k5_p1024_m1024": (16, 5, 1024, 1024, {}, None, PLUS_ALL),
    "pl_k25_p100_loss_alone": (17, 25, 100, 1026, {}, None, ("loss",)),
}
LENSFIT_ALL = ("params", "loss", "best", "all_params", "all_loss", "grad", "trace")
# name -> (seed, K (0: given points), P, M, starts, n_steps, weight, the curve's generator, outputs)
LENSFIT = {
    "lf_k1_p2_m1_s1_eval": (21, 1, 2, 1, 1, 0, 1.0, "gauss", LENSFIT_ALL[:-1]),        # (n_steps 0 has no trace)
    "lf_k5_p100_m130_s2_n5": (22, 5, 100, 130, 2, 5, 1.0, "lens", LENSFIT_ALL),
    "lf_k25_p257_m1023_s16_n1_w025": (23, 25, 257, 1023, 16, 1, 0.25, "gauss", LENSFIT_ALL),
    "lf_given_p1024_m1024_s2_n5": (24, 0, 1024, 1024, 2, 5, 1.0, "lens", LENSFIT_ALL),
    "lf_k5_p600_m300_s1_n1_w025": (25, 5, 600, 300, 1, 1, 0.25, "gauss", LENSFIT_ALL),
    "lf_k5_p100_m700_s2_n5_params_loss_alone": (26, 5, 100, 700, 2, 5, 1.0, "lens", ("params", "loss")),
}
PLUSFIT_ALL = ("params", "loss", "best", "n_run", "all_params", "all_loss", "grad", "trace")
# name -> (seed, K (0: given points), P, starts, n_steps, corner_weight, corner_decay, stop_loss, outputs)
PLUSFIT = {
    "pf_k1_p2_s1_eval": (431, 1, 2, 1, 0, 1.0, False, 0.0, PLUSFIT_ALL[:-1]),           # (n_steps 0 has no trace)
    "pf_k5_p100_s2_n5_decay": (441, 5, 100, 2, 5, 1.0, True, 0.0, PLUSFIT_ALL),
    "pf_k25_p257_s3_n1_stop": (432, 25, 257, 3, 1, 1.0, False, 0.1, PLUSFIT_ALL),
    "pf_given_p1024_s16_n1_w037": (451, 0, 1024, 16, 1, 0.37, False, 0.0, PLUSFIT_ALL),
    "pf_k5_p600_s2_n5_params_loss_alone": (461, 5, 600, 2, 5, 1.0, True, 0.0, ("params", "loss")),
}
# what a case's rows hold beside plusfit_oracle.eval_params' draw: rows of zero width and clamped rows, and (row, start, the move
# of xoffset) that puts a start's loss far above the stop case's stop_loss
PLUSFIT_ROWS = {"pf_k5_p100_s2_n5_decay": dict(zero_width=(1,), clamped=(3,))}
PLUSFIT_MOVES = {"pf_k25_p257_s3_n1_stop": ((0, 0, 0.6), (2, 0, 0.6), (2, 1, 0.6))}
HASHED = ("points", "segments")          # outputs the fixture keeps as a sha256


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def inputs(name):
    """the case's input arrays (a dict; max_dist, where there is one, as a 0-d fp32 array)"""
    if name in HAUSDORFF:
        seed, K, P, M, mode = HAUSDORFF[name]
        x = co.gauss(100 + seed, ROWS, K or 5)
        inp = dict(curve=x if K else co.points64(x, P).astype(np.float32))
        if mode == "ragged":
            inp["template"] = np.concatenate([ho.lens_template(m) for m in RAGGED])
            inp["offsets"] = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
        elif mode != "points":
            inp["template"] = ho.lens_template(M)
        if mode == "params":
            inp["params"] = ho.golden_params(seed, ROWS)
        return inp
    if name in LENSFIT:
        seed, K, P, M, S, _, _, gen, _ = LENSFIT[name]
        x = lo.lens_rows(400 + seed, ROWS, K or 5) if gen == "lens" else co.gauss(400 + seed, ROWS, K or 5)
        return dict(curve=x if K else co.points64(x, P).astype(np.float32),
                    prototype=lo.lens_prototype(M) if M > 1 else np.array([[0.75, -0.5]], np.float32),
                    starts=lo.golden_grad_params(seed, ROWS * S).reshape(ROWS, S, 4))
    if name in PLUSFIT:
        seed, K, P, S = PLUSFIT[name][:4]
        x, base = pfo.plus_rows(seed, ROWS, K or 5)
        starts = np.stack([pfo.eval_params(base, seed + 1 + s, **PLUSFIT_ROWS.get(name, {})) for s in range(S)], 1)
        for r, s, move in PLUSFIT_MOVES.get(name, ()):
            starts[r, s, 6] += np.float32(move)
        return dict(curve=x if K else co.points64(x, P).astype(np.float32), starts=starts)
    seed, K, P, size, zero, over, _ = PLUS[name]
    pr = po.draw_params(200 + seed, ROWS, (), zero=zero)
    if over is not None:
        pr[over, :2] = 40.0                                  # an outline of twice the served rows' points
    served = [r for r in np.argsort(-po.quotients(pr, 1.0).sum(1)) if r != over]      # the largest first: none goes past `size`
    md, _ = po.find_max_dist(pr, size, rows=served)
    return dict(params=pr, curve=(co.gauss(300 + seed, ROWS, K) * np.float32(3)).astype(np.float32), max_dist=np.float32(md))


def check_plus_rows(name, inp):
    """the CPU condition: every row is served (counts >= 0) but the one meant not to be, and the largest served outline has the
    size the case is named for"""
    _, _, _, size, zero, over, _ = PLUS[name]
    ref = po.plus64(inp["params"], max_dist=float(inp["max_dist"]))
    unserved = np.nonzero((ref["counts"] < 0).any(1))[0].tolist()
    assert unserved == ([] if over is None else [over]), (name, unserved)
    assert ref["M"][[r for r in range(ROWS) if r != over]].max() == size, (name, ref["M"])
    for r, cols in zero.items():
        assert (ref["counts"][r] == 0).sum() == 2 * len(cols), (name, r, ref["counts"][r])


def check_plusfit_rows(name, inp):
    """the CPU conditions of a plus-fit case: with every start run in float64 no loss lies within a factor 1.5 of stop_loss, the
    float32 emulation and float64 agree on the starts that run, every emulated word of a start that runs is finite, and the stop
    case ends its rows after one, two and three starts.  Returns n_run [ROWS]"""
    _, K, P, S, n_steps, cw, decay, stop, _ = PLUSFIT[name]
    kw = dict(n_steps=n_steps, c=cw, decay=decay)
    n_run = []
    for r in range(ROWS):
        b32 = (co.points64(inp["curve"][r:r + 1], P)[0] if K else inp["curve"][r]).astype(np.float32).astype(np.float64)
        losses = pfo.fit64(b32, inp["starts"][r], stop_loss=0.0, **kw)["all_loss"]
        assert np.isfinite(losses).all() and not ((losses > stop / 1.5) & (losses < stop * 1.5)).any(), (name, r, losses)
        f64, f32 = pfo.fit64(b32, inp["starts"][r], stop_loss=stop, **kw), pfo.emulate32(b32, inp["starts"][r], stop_loss=stop, **kw)
        assert f64["n_run"] == f32["n_run"] and f64["best"] == f32["best"], (name, r, f64["n_run"], f32["n_run"])
        k = f32["n_run"]
        assert all(np.isfinite(f32[o][:k]).all() for o in ("all_params", "all_loss", "grad", "trace")), (name, r)
        n_run.append(k)
    if stop > 0:
        assert set(n_run) == {1, 2, 3}, (name, n_run)
    if name in PLUSFIT_ROWS:
        assert (inp["starts"][list(PLUSFIT_ROWS[name]["zero_width"]), :, 2] == 0).all()
    return np.array(n_run)


def run(name, inp):
    """the case on the device: a dict of its outputs as numpy arrays"""
    import torch
    from hint_amd import curves
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    if name in HAUSDORFF:
        _, K, P, M, mode = HAUSDORFF[name]
        t = lambda k: dev(inp[k]) if k in inp else None                          # noqa: E731
        out = curves._hd_run(dev(inp["curve"]), K, P, t("template"), t("offsets"), t("params"), want_h=M is not None,
                             want_chamfer=M is not None, want_points=K > 0, max_groups=GROUPS)
        out = dict(zip(("max_h", "avg_h", "chamfer", "points"), out))
    elif name in LENSFIT:
        _, K, P, _, _, n_steps, w, _, want = LENSFIT[name]
        out = curves._lf_run(dev(inp["curve"]), K, P, dev(inp["prototype"]), dev(inp["starts"]), n_steps, lo.LR, lo.ANGLE_LR,
                             lo.GAMMA, lo.MOMENTUM, w, want, GROUPS)
    elif name in PLUSFIT:
        _, K, P, _, n_steps, cw, decay, stop, want = PLUSFIT[name]
        out = curves._pf_run(dev(inp["curve"]), K, P, dev(inp["starts"]), n_steps, pfo.LR, pfo.ANGLE_LR, pfo.GAMMA, pfo.MOMENTUM, cw,
                             decay, stop, want, GROUPS)
    else:
        _, K, P, _, _, _, want = PLUS[name]
        out = curves._plus_run(dev(inp["params"]), dev(inp["curve"]), K, P, float(inp["max_dist"]), want, GROUPS)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def record(name, inp, out):
    """what the fixture keeps of a case, {key: array}: a sha256 of every input array (max_dist itself), the outputs raw or hashed"""
    rec = {f"{name}/in/{k}": v if k == "max_dist" else np.array(sha(v)) for k, v in inp.items()}
    for k, v in out.items():
        rec[f"{name}/out/{k}"] = np.array(sha(v)) if k in HASHED else v
    return rec
