"""hint_amd.sample_plus_prior / sample_plus_joint / sample_plus_targeted / sample_plus_conditional / plus_outlines / plus_draws on
the GPU against tests/plusgen_oracle.py (float64, the ring by sorting corners and crossings about the origin) under that file's
comparison rule, and against themselves: Philox and explicit draws, chunking, grids, two runs, a gather by row, labels only,
rotations, guard-banded poisoned buffers, graph capture, a gated non-default stream, moments."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import hint_amd
from hint_amd import _lib, plusgen
from hint_amd._lib import HintAmdError
import plusgen_oracle as po
import stream_gate
from guarded import FILLS, Guarded, bits_equal
from plusgen_cases import (CONDITIONAL, HIGH, MOMENT_SEED, N_BIG, SEED, TARGETS, corner_case_draws, corner_share,
                           geometry_moments, pattern_draws)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (n, offset): one row, the sizes around a wavefront's 4 rows and a workgroup's 16 and 64, more than one workgroup, the counter's carry
CASES = [(1, 0), (63, 1), (64, 0), (65, 64), (N_BIG, 0), (10, HIGH)]
CASE_IDS = [f"n{n}_off{o}" for n, o in CASES]
NORMAL_BOUND = 2.0 ** -13      # the hardware's log2 / sin / cos, as tests/test_gpu_noise.py and test_gpu_shapegen.py hold them
U = po.U
ALL = ["x", "y", "outline", "counts", "corners", "draws_out"]


def same(a, b):
    """bit-for-bit equality of two tensors of a 4-byte type"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def cpu64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def run(n, seed=SEED, offset=0, draws=None, want=ALL, **kw):
    return plusgen._plus_run(n, seed, offset, torch.device(DEV), draws, want, **kw)


def host(res):
    """a run's outputs as the oracle's dict: corners split into the count and the arms"""
    out = {k: v.cpu().numpy() for k, v in res.items() if k in ("x", "y", "outline", "counts")}
    c = res["corners"].cpu().numpy()
    out["corners"], out["arms"] = c & 15, c >> 4
    return out


def check(got, d, target=None, keep=None, what=""):
    """got against the oracle's float64 sample of the draws d under THE RULE; keep None: drop the ambiguous rows, within the cap"""
    want = po.sample(d, target)
    if keep is None:
        keep = ~po.ambiguous(d, target)
        left_out = float((~keep).mean())
        assert left_out <= po.MAX_AMBIGUOUS, left_out
    res = po.compare(got, want, keep, target)
    print(f"{what}: {int((~keep).sum())} of {len(d)} rows left out; error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert po.passes(res), res
    assert (got["arms"][keep] == want["arms"][keep]).all()
    n = got["counts"]
    for i in range(len(d)):                                  # zero padding behind the outline
        assert (got["outline"][i, n[i]:] == 0).all()
    return want


@pytest.fixture(scope="module")
def device_draws():
    """{offset: the draws [n, 9] as the device made them}: read once"""
    return {off: hint_amd.plus_draws(n, SEED, offset=off, device=DEV).cpu().numpy() for n, off in ((N_BIG, 0), (10, HIGH))}


def test_draws_are_the_oracles_philox(device_draws):
    for off, n in ((0, N_BIG), (HIGH, 10)):
        d, want = device_draws[off], po.draws(SEED, off, n)
        assert (d[:, :7] == want[:, :7].astype(np.float32)).all()              # exact: part of the definition
        err = float(np.abs(d[:, 7:] - want[:, 7:]).max())
        print(f"offset {off}: normals differ from float64 Box-Muller by at most {err:.3e} (bound {NORMAL_BOUND:.2e})")
        assert err <= NORMAL_BOUND
    assert (device_draws[0][:10] != device_draws[HIGH]).any()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_philox_path_and_explicit_draws_give_equal_bits(case):
    n, off = case
    a = run(n, offset=off)
    b = run(n, 0, 0, draws=a["draws_out"])
    for k in ALL:
        assert a[k].shape == plusgen._TABLE(n)[k][0] and a[k].dtype == plusgen._TABLE(n)[k][1]
        assert same(a[k], b[k]), k
    x, outline, counts = hint_amd.sample_plus_prior(n, SEED, offset=off, device=DEV, return_outline=True)
    assert bits_equal(x, a["x"]) and bits_equal(outline, a["outline"]) and torch.equal(counts, a["counts"])
    assert bits_equal(hint_amd.sample_plus_prior(n, SEED, offset=off, device=DEV), a["x"])          # ... with nothing else asked for
    x2, y2 = hint_amd.sample_plus_joint(n, SEED, offset=off, device=DEV)
    assert bits_equal(x2, a["x"]) and bits_equal(y2, a["y"])
    o3, c3, y3 = hint_amd.plus_outlines(a["draws_out"])
    assert bits_equal(o3, a["outline"]) and torch.equal(c3, a["counts"]) and bits_equal(y3, a["y"])
    assert torch.isfinite(a["x"]).all() and torch.isfinite(a["y"]).all()


def test_chunks_grids_and_two_runs_give_equal_bits():
    whole = run(N_BIG)
    parts = [run(n, offset=o) for n, o in ((1, 0), (63, 1), (4035, 64))]
    again = run(N_BIG)
    for k in ALL:
        assert same(whole[k], torch.cat([p[k] for p in parts])), k
        assert same(whole[k], again[k]), k
    for groups in (1, 3):
        res = run(N_BIG, max_groups=groups)
        for k in ALL:
            assert same(whole[k], res[k]), (groups, k)
        assert int(res["workspace"].view(torch.int32).sum()) == 0
    high = run(10, offset=HIGH)
    parts = [run(n, offset=o) for n, o in ((5, HIGH), (5, 2 ** 32))]
    for k in ("x", "y"):
        assert bits_equal(high[k], torch.cat([p[k] for p in parts])), k
    assert not bits_equal(high["x"], whole["x"][:10])
    assert not bits_equal(whole["x"], run(N_BIG, seed=SEED + 1)["x"])


def test_a_gather_by_row_has_the_bits_of_the_contiguous_call():
    whole = run(N_BIG)
    g = torch.Generator().manual_seed(5)
    pick = torch.cat([torch.tensor([0, N_BIG - 1, 64, 63, 63]), torch.randint(0, N_BIG, (200,), generator=g)])
    got = run(len(pick), want=["x", "y", "counts"], rows=pick.to(DEV))
    for k in ("x", "y", "counts"):
        assert torch.equal(got[k].view(torch.int32), whole[k][pick.to(DEV)].view(torch.int32)), k
    high = run(10, offset=HIGH)
    rows = torch.arange(HIGH, HIGH + 10, dtype=torch.int64)
    got = run(10, want=["x", "y"], rows=rows.flip(0).to(DEV))
    assert bits_equal(got["x"].flip(0), high["x"]) and bits_equal(got["y"].flip(0), high["y"])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_labels_only_gives_the_full_calls_labels(case):
    n, off = case
    full = run(n, offset=off)
    only = run(n, offset=off, want=["y"])
    assert bits_equal(only["y"], full["y"])
    some = run(n, offset=off, want=["y", "counts", "corners"])
    assert bits_equal(some["y"], full["y"]) and torch.equal(some["counts"], full["counts"]) and torch.equal(some["corners"], full["corners"])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_philox_rows_against_the_oracle(case, device_draws):
    n, off = case
    base = HIGH if off >= HIGH else 0
    d = device_draws[base][off - base:off - base + n]
    got = host(run(n, offset=off))
    want = check(got, d, what=f"n {n} offset {off}")
    if n == N_BIG:
        assert set(np.unique(got["corners"]).tolist()) == {8, 12} and len(np.unique(got["arms"])) == 9
        assert got["counts"].min() >= po.N_RANGE[0] and got["counts"].max() <= po.N_RANGE[1]
        assert len(np.unique(want["counts"])) >= 30          # the per-row twiddle table is built for many N


def test_every_pattern_and_the_corner_cases_against_the_oracle():
    d, masks = pattern_draws()
    got = host(run(len(d), 0, 0, draws=torch.from_numpy(d).to(DEV)))
    check(got, d, what="nine patterns")
    assert (got["arms"] == masks).all() and sorted(set(masks.tolist())) == [5, 6, 7, 9, 10, 11, 13, 14, 15]
    # dyadic draws: the fp32 chain up to an edge's length is exact, so every row is compared, the exact half-integers included
    d = corner_case_draws()
    got = host(run(len(d), 0, 0, draws=torch.from_numpy(d).to(DEV)))
    want = check(got, d, keep=np.ones(len(d), dtype=bool), what="corner cases of the N sweep")
    assert (want["counts"] != po.sample(d, variant="half_up")["counts"]).any()    # round-half-to-even is exercised
    assert got["counts"].max() <= po.N_RANGE[1] and got["counts"].min() >= po.N_RANGE[0]


def test_fourier_coeffs_of_the_outline_is_the_samplers_x():
    n = 300
    x, outline, counts = hint_amd.sample_plus_prior(n, SEED, device=DEV, return_outline=True)
    y = hint_amd.fourier_coeffs(outline, 25, counts)
    A = np.abs(cpu64(outline)).reshape(n, -1).max(axis=1)
    N = counts.cpu().numpy()
    err = np.abs(cpu64(x) - cpu64(y)).max(axis=1) / (U * A)
    print(f"worst {err.max():.2f} u A (bound 2 (N + 2) >= {2 * (N.min() + 2)})")
    assert (err <= 2 * (N + 2.0)).all()                      # each within (N + 2) u A of the exact coefficients of the same outline


def test_turning_the_angle_turns_coefficients_and_center():
    """the same draws with u_a changed turn every coefficient pair (axis 0, axis 1) and center - offset by the same matrix: with
    zero normals, x' = x R(da) and center' = center R(da).  Needs no oracle."""
    n = 257
    g = torch.Generator().manual_seed(3)
    d0 = torch.rand(n, 9, generator=g)
    d0[:, 6] = torch.randint(0, 512, (n,), generator=g).float() / 1024.0     # u_a in [0, 0.5) on a grid: u_a + k / 8 is exact
    d0[:, 7:] = 0
    a = run(n, 0, 0, draws=d0.to(DEV))
    A = np.abs(cpu64(a["outline"])).reshape(n, -1).max(axis=1)
    N = a["counts"].cpu().numpy()
    x0, c0 = cpu64(a["x"]).reshape(n, 2, 2, 25), cpu64(a["y"])[:, :2]        # [row, re | im, axis, m]
    for k in (1, 3, 4):
        d = d0.clone()
        d[:, 6] += k / 8.0
        b = run(n, 0, 0, draws=d.to(DEV))
        assert torch.equal(a["counts"], b["counts"]) and torch.equal(a["corners"], b["corners"])
        phi = (np.pi / 2) * k / 8
        R = np.array([[np.cos(phi), np.sin(phi)], [-np.sin(phi), np.cos(phi)]])
        ex = np.abs(cpu64(b["x"]).reshape(n, 2, 2, 25) - np.einsum("npam,ab->npbm", x0, R)).reshape(n, -1).max(axis=1) / (U * A)
        ec = np.abs(cpu64(b["y"])[:, :2] - c0 @ R).max(axis=1) / (U * A)
        print(f"k {k}: coefficients {float((ex / (2 * po.k_coef(N))).max()):.3g}, center {float(ec.max() / (2 * po.K_Y)):.3g} of the bound")
        assert (ex <= 2 * po.k_coef(N)).all() and (ec <= 2 * po.K_Y).all()


@pytest.mark.parametrize("target", TARGETS, ids=[f"ratio{t[3]}" for t in TARGETS])
def test_targeted_rows_against_the_oracle(target, device_draws):
    n = 1027
    d = device_draws[0][:n]
    res = run(n, want=["x", "y", "outline", "counts", "corners"], target=plusgen._check_target(target, "test"))
    check(host(res), d, target=target, what=f"target {target}")
    x, y = hint_amd.sample_plus_targeted(n, SEED, target, device=DEV)
    assert bits_equal(x, res["x"]) and bits_equal(y, res["y"])
    assert (y[:, 2] == np.float32(target[2])).all()
    o, c, y2 = hint_amd.plus_outlines(torch.from_numpy(d).to(DEV), target=target)
    assert bits_equal(y2, y) and bits_equal(o, res["outline"])


def test_conditional_sample_is_the_oracles_selection_whatever_the_chunk():
    target, radius, n, seed, m = CONDITIONAL
    x, y, tried = hint_amd.sample_plus_conditional(target, n, seed, radius, chunk=1000, device=DEV)
    assert x.shape == (n, 100) and y.shape == (n, 4)
    d = po.draws(seed, 0, m)
    want = po.sample(d, target)
    idx, tried64, d2 = po.select(want["y"], target, radius, n)
    assert idx is not None and tried == tried64 <= m
    assert np.abs(np.sqrt(d2[:tried64].astype(np.float64)) - radius).min() > 1e-4       # no candidate near the boundary
    dd = hint_amd.plus_draws(tried, seed, device=DEV).cpu().numpy()[idx]
    assert not po.ambiguous(dd, target).any()
    got = dict(x=x.cpu().numpy(), y=y.cpu().numpy(), outline=want["outline"][idx], counts=want["counts"][idx], corners=want["corners"][idx])
    res = po.compare(got, {k: v[idx] for k, v in want.items()}, None, target)
    assert po.passes(res), res
    for chunk in (257, 1 << 20):
        x2, y2, t2 = hint_amd.sample_plus_conditional(target, n, seed, radius, chunk=chunk, device=DEV)
        assert bits_equal(x, x2) and bits_equal(y, y2) and t2 == tried
    xt, yt = hint_amd.sample_plus_targeted(tried, seed, target, device=DEV)
    pick = torch.from_numpy(idx).to(DEV)
    assert bits_equal(x, xt[pick]) and bits_equal(y, yt[pick])
    with pytest.raises(HintAmdError, match="fewer than n"):
        hint_amd.sample_plus_conditional(target, n, seed, radius, chunk=64, max_rows=100, device=DEV)


def desc_run(n, seed, off, draws, bufs, nbytes, target=None, stream=None):
    lib = _lib.load()
    desc = _lib.PlusGenDesc()
    desc.n_rows, desc.seed, desc.offset, desc.max_groups = n, seed, off, 0
    desc.draws = draws
    gx, gy, go, gc, gk, gd, gw = bufs
    desc.x, desc.y, desc.outline, desc.counts, desc.corners, desc.draws_out = gx.ptr, gy.ptr, go.ptr, gc.ptr, gk.ptr, gd.ptr
    desc.workspace, desc.workspace_bytes = gw.ptr, nbytes
    tgt = (C.c_float * 4)(*target) if target is not None else None
    desc.target = tgt
    desc.stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _lib.check(lib.hint_plusgen_run(C.byref(desc)), "hint_plusgen_run")


NAMES = ("x", "y", "outline", "counts", "corners", "draws_out", "workspace")


def guarded_outputs(n, nbytes, fill, rep):
    return [Guarded(100 * n, fill=fill, seed=rep), Guarded(4 * n, fill=fill, seed=10 + rep), Guarded(256 * n, fill=fill, seed=20 + rep),
            Guarded(n, fill=fill, seed=30 + rep, dtype=torch.int32), Guarded(n, fill=fill, seed=40 + rep, dtype=torch.int32),
            Guarded(9 * n, fill=fill, seed=50 + rep), Guarded(nbytes // 4, fill=fill, seed=60 + rep, dtype=torch.int32)]


@pytest.mark.parametrize("mode", ("philox", "draws", "target"))
def test_plusgen_writes_every_promised_element_and_nothing_beyond(mode):
    """hint_plusgen_run on guard-banded buffers filled with zeros, NaNs or junk, a ragged last tile: the same bits every time (so
    every element of every output and of the workspace is written), guards intact, the draws unchanged"""
    lib = _lib.load()
    n = 16 * 5 + 7
    nbytes = lib.hint_plusgen_workspace_bytes(n)
    gd = Guarded(9 * n).set(hint_amd.plus_draws(n, SEED, device=DEV))
    sd = gd.snapshot()
    target = [0.1, -0.2, 0.7, 0.4] if mode == "target" else None
    first = None
    for rep, fill in enumerate(("zero",) + FILLS):
        bufs = guarded_outputs(n, nbytes, fill, rep)
        desc_run(n, SEED, 0, gd.ptr if mode == "draws" else None, bufs, nbytes, target)
        torch.cuda.synchronize()
        for b, name in zip(bufs, NAMES):
            b.check_guards(f"{mode}, {fill}: {name}")
        gd.check_unchanged(sd, f"{mode}, {fill}: draws")
        now = [b.words.clone() for b in bufs]
        first = first or now
        for a, b, name in zip(now, first, NAMES):
            assert torch.equal(a, b), (mode, fill, name)
    res = run(n, target=target)
    for w, k in zip(first, ALL):
        assert torch.equal(w, res[k].reshape(-1).view(torch.int32)), k
    assert int(first[6].sum()) == 0 and torch.equal(first[5], gd.words)


def test_rows_outside_the_definition_are_refused_and_disturb_no_neighbour():
    n = 100
    d = hint_amd.plus_draws(n, SEED, device=DEV)
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        for col in (range(9) if bad != bad or bad == float("inf") else range(7)):
            e = d.clone()
            e[41, col] = bad
            with pytest.raises(HintAmdError, match="1 row"):
                hint_amd.sample_plus_prior(n, 0, draws=e)
    e = d.clone()
    e[41, 4], e[42, 8], e[99, 0] = 1.5, float("nan"), -1.0
    lib = _lib.load()
    nbytes = lib.hint_plusgen_workspace_bytes(n)
    bufs = guarded_outputs(n, nbytes, "junk", 0)
    desc_run(n, 0, 0, e.data_ptr(), bufs, nbytes)
    torch.cuda.synchronize()
    good = run(n, 0, 0, draws=d)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[[41, 42, 99]] = False
    x, y, o, c, k = (bufs[i].view(*s) for i, s in enumerate(((n, 100), (n, 4), (n, 128, 2), (n,), (n,))))
    assert torch.isnan(x[~keep]).all() and torch.isnan(y[~keep]).all() and (o[~keep] == 0).all()
    assert (c[~keep] == 0).all() and (k[~keep] == 0).all() and int(bufs[6].words.sum()) == 3
    assert bits_equal(x[keep], good["x"][keep]) and bits_equal(y[keep], good["y"][keep]) and bits_equal(o[keep], good["outline"][keep])
    assert torch.equal(c[keep], good["counts"][keep]) and torch.equal(k[keep], good["corners"][keep])


def test_graph_capture_with_two_replays():
    n = 16 * 9 + 3
    lib = _lib.load()
    nbytes = lib.hint_plusgen_workspace_bytes(n)
    want = run(n)                                            # (also loads the kernel before the capture)
    bufs = guarded_outputs(n, nbytes, "nan", 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        desc_run(n, SEED, 0, None, bufs, nbytes)
    for rep in range(2):
        for b in bufs:
            b.fill("junk", seed=rep)
        graph.replay()
        torch.cuda.synchronize()
        for b, name in zip(bufs, NAMES):
            b.check_guards(f"replay {rep}: {name}")
        for b, k in zip(bufs, ALL):
            assert torch.equal(b.words, want[k].reshape(-1).view(torch.int32)), (rep, k)


@contextlib.contextmanager
def side_stream():
    """a non-blocking stream of this test's own, destroyed behind it.  A stream taken from torch's pool lives as long as the
    process, and every such stream shifts which hardware queue the streams of the test files that run later come to share:
    tests/test_gpu_streams.py's canary depends on its side stream and the null stream not sharing one"""
    hip = _lib.load()                                        # (the HIP runtime's symbols resolve through the library's dependencies)
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p), C.c_uint], [C.c_void_p]
    raw = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0 and raw.value      # 1: hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(raw.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0


def test_run_on_a_gated_non_default_stream():
    """hint_plusgen_run takes its stream from the descriptor: the run S-gated and null-gated on a side stream, still_closed()
    asserted (tests/stream_gate.py), as tests/test_gpu_streams.py does for the entry points of its ledger"""
    lib = _lib.load()
    n = 16 * 5 + 7
    nbytes = lib.hint_plusgen_workspace_bytes(n)
    d = hint_amd.plus_draws(n, SEED, device=DEV)
    streams = []

    def make(fill, role):
        bufs = guarded_outputs(n, nbytes, fill, 0)
        gd = Guarded(9 * n).set(d)
        late = stream_gate.late_inputs([(gd, None)])

        def call():
            st = torch.cuda.current_stream().cuda_stream
            streams.append((role, st))
            desc_run(n, 0, 0, gd.ptr, bufs, nbytes, stream=st)
            return {name: b.t for name, b in zip(NAMES, bufs)}
        return stream_gate.Seq(call, late, list(zip(NAMES, bufs)) + [("draws", gd)])
    with side_stream() as S:
        stream_gate.run_case("hint_plusgen_run", make, S, finite=False)
        assert {st for role, st in streams if role == "S"} == {S.cuda_stream} and S.cuda_stream != 0
        assert {st for role, st in streams if role == "ref"} == {0}


def test_moments_on_a_million_rows():
    """center = (-mean) R + 0.5 (n_x, n_y): the two parts are independent, the normals' has mean 0 and variance 1 / 4, and the CPU
    sweep of the oracle gives the moments of the geometry's.  Mean and variance of y[:, 0:2], and the share of 8-corner rows
    against the sweep's, each within 5 standard errors of the difference of two samples"""
    n = 10 ** 6
    res = run(n, seed=MOMENT_SEED, want=["y", "corners"])
    assert torch.isfinite(res["y"]).all()
    gm, gv, g4, rows = geometry_moments()
    for c in range(2):
        v = res["y"][:, c].double()
        mean, var = float(v.mean()), float(v.var())
        m4 = float(((v - mean) ** 4).mean())
        se_mean = np.sqrt(var / n + gv[c] / rows)
        se_var = np.sqrt((m4 - var ** 2) / n + (g4[c] - gv[c] ** 2) / rows)
        print(f"y[:, {c}]: mean {mean:.5f} (sweep {gm[c]:.5f}, 5 se {5 * se_mean:.5f}), variance {var:.5f} "
              f"(sweep {gv[c]:.5f} + 0.25, 5 se {5 * se_var:.5f})")
        assert abs(mean - gm[c]) <= 5 * se_mean and abs(var - (gv[c] + 0.25)) <= 5 * se_var
    share, rows = corner_share()
    got = float(((res["corners"] & 15) == 8).double().mean())
    se = np.sqrt(share * (1 - share) * (1.0 / n + 1.0 / rows))
    print(f"share of 8-corner rows {got:.5f}, the CPU sweep's {share:.5f} over {rows} rows, 5 se {5 * se:.5f}")
    assert abs(got - share) <= 5 * se
