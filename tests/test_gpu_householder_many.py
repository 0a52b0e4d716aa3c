"""GPU tests of hint_householder_many_run: the matrices, row work and gradients of the m trainable permutations of one flow
(FlowTrainer(learned_perms=True)).  The oracle-free statement is the header's: every output has the bits of m single
hint_householder_run calls.  Against float64 (tests/householder_oracle.py) the bounds are those tests/test_gpu_householder.py
derives: g_W per entry (min(B, R / 4) + 8) u (|x|^T |g_y|), g_V rel_err < 1e-4.  x and g_y are randn + 2: sums that do not cancel,
so a slab left out cannot hide inside the bound.  The items of a job lie a stride apart; the tests give every stride a gap of its
own and hold the gaps (and the guards around the buffers) against the NaN pattern they were filled with.  The finish keeps its
two d x d double matrices in LDS up to d = 94 (HH_FIN_LDS_D of hint_householder.hip, held against the kernel's text below) and in
the workspace beyond: d = 94 and d = 95 run beside the sizes the issue names, and both variants must give the single run's bits."""
import functools

import pytest
import torch

from hint_amd import _lib
from hint_amd._ops import _run_desc
import householder_oracle as ho
import stream_gate
from guarded import FILLS, NAN_BITS, Guarded, bits_equal
from test_gpu_householder import BS, DEV, SLAB, build, geometry, grad, gw_factor, ratio, side_stream
from util import rel_err

pytestmark = pytest.mark.gpu
BUILD, ROWS, FINISH = _lib.HOUSEHOLDER_MANY_BUILD, _lib.HOUSEHOLDER_MANY_ROWS, _lib.HOUSEHOLDER_MANY_FINISH
GRAD = _lib.HOUSEHOLDER_GRAD
RUN = "hint_householder_many_run"


def slot_bytes(B, d, n):
    nbytes = _lib.load().hint_householder_workspace_bytes(GRAD, B, d, n)
    assert nbytes > 0 and nbytes % 16 == 0
    return nbytes


def many(op, m, d, n, B=1, **f):
    """one hint_householder_many_run on the current stream; tensors give their addresses"""
    job = _lib.HouseholderMany()
    job.op, job.m, job.B, job.d, job.n = op, m, B, d, n
    for k, v in f.items():
        setattr(job, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    _run_desc(RUN, job, DEV)


class Items:
    """m items of `item` floats, `gap` floats apart, in one guarded buffer: the layout of a strided field of the job"""

    def __init__(self, m, item, gap, fill="nan", seed=0):
        self.m, self.item, self.stride = m, item, item + gap
        self.g = Guarded((m - 1) * self.stride + item, fill, seed=seed)
        self.fill = fill
        self.before = self.g.words.clone()

    @property
    def t(self):
        return self.g.t

    def set(self, j, values):
        self.g.t[j * self.stride:j * self.stride + self.item].copy_(values.reshape(-1))
        self.before = self.g.words.clone()
        return self

    def get(self, j, *shape):
        return self.g.t[j * self.stride:j * self.stride + self.item].view(*shape)

    def check(self, what, written=True):
        """the guards hold, the gaps between the items hold what they held, and (nan fill) every word of every item was written"""
        self.g.check_guards(what)
        for j in range(self.m - 1):
            a, b = j * self.stride + self.item, (j + 1) * self.stride
            assert torch.equal(self.g.words[a:b], self.before[a:b]), f"{what}: the gap behind item {j} changed"
        if written and self.fill == "nan":
            for j in range(self.m):
                left = int((self.g.words[j * self.stride:j * self.stride + self.item] == NAN_BITS).sum())
                assert left == 0, f"{what}: {left} words of item {j} were never written"


@functools.lru_cache(maxsize=None)
def vs_of(d, n, j):
    """permutation j's Vs: the module's initialisation from a seed of its own, moved a little further"""
    g = torch.Generator().manual_seed(31 * d + 7 * n + j)
    return (ho.init_Vs(n, d, seed=1000 * d + n + 17 * j) + 0.05 * torch.randn(n, d, generator=g)).contiguous()


@functools.lru_cache(maxsize=None)
def rows_of(d, j):
    """(x, g_y) of permutation j at the largest batch: randn + 2"""
    g = torch.Generator().manual_seed(d * 13 + j)
    return torch.randn(BS[-1], d, generator=g) + 2.0, torch.randn(BS[-1], d, generator=g) + 2.0


def vs_items(m, d, n, gap=4):
    V = Items(m, n * d, gap, "nan")
    for j in range(m):
        V.set(j, vs_of(d, n, j).to(DEV))
    return V


# ---- BUILD ----
BUILD_DN = sorted({(d, n) for d in (1, 2, 16, 17, 63, 64, 65, 100, 128) for n in (1, d, d + 3)} | {(20, 256)})


@pytest.mark.parametrize("d,n", BUILD_DN)
def test_build_has_the_bits_of_m_single_builds(d, n):
    for m in (1, 3, 64):
        V = vs_items(m, d, n)
        W = Items(m, d * d, 12, "nan", seed=1)
        many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
        torch.cuda.synchronize()
        W.check(f"build d {d} n {n} m {m}: W")
        V.check("Vs", written=False)
        singles = [build(V.get(j, n, d).contiguous()) for j in range(m)]
        for j in range(m):
            assert bits_equal(W.get(j, d, d), singles[j]), (d, n, m, j)
        if m >= 3 and d > 1:                                        # (Vs varies per permutation; at d = 1 W = (-1)^n whatever Vs)
            assert not bits_equal(singles[0], singles[1])
        again = Items(m, d * d, 12, "junk", seed=2)
        many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=again.t, w_stride=again.stride)
        for j in range(m):
            assert bits_equal(again.get(j, d, d), singles[j])


# ---- ROWS + FINISH ----
def rows_finish(m, d, n, B, V, W, ws, want_gw=True, fill="nan", seed=0, gx_for=None):
    """op rows for every permutation, then op finish -> (g_x items [m], g_W Items or None, g_V Items)"""
    gx_for = range(m) if gx_for is None else gx_for
    g_x = [Guarded(B * d, fill, seed=seed + 10 + j) for j in range(m)]
    g_W = Items(m, d * d, 8, fill, seed=seed + 1) if want_gw else None
    g_V = Items(m, n * d, 20, fill, seed=seed + 2)
    stride = ws.numel() * ws.element_size() // (4 * m)
    for j in range(m):
        x, gy = (t[:B].contiguous().to(DEV) for t in rows_of(d, j))
        many(ROWS, m, d, n, B, j=j, W=W.t, w_stride=W.stride, x=x, g_y=gy, g_x=g_x[j].view(B, d) if j in gx_for else None,
             workspace=ws, workspace_bytes=ws.numel() * ws.element_size(), ws_stride=stride)
    many(FINISH, m, d, n, B, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride, g_W=g_W.t if want_gw else None,
         gw_stride=g_W.stride if want_gw else 0, g_V=g_V.t, gv_stride=g_V.stride, workspace=ws,
         workspace_bytes=ws.numel() * ws.element_size(), ws_stride=stride)
    torch.cuda.synchronize()
    return g_x, g_W, g_V


def built(m, d, n):
    V = vs_items(m, d, n)
    W = Items(m, d * d, 12, "nan", seed=1)
    many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
    return V, W


FIN_LDS_D = 94


def test_the_finish_switches_variants_where_the_tests_say():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hint_amd", "csrc", "hint_householder.hip")).read()
    assert int(re.search(r"constexpr int HH_FIN_LDS_D = (\d+);", text).group(1)) == FIN_LDS_D
    assert "if (d <= HH_FIN_LDS_D)" in text and "hint_hh_finish_many_kernel<true>" in text and "hint_hh_finish_many_kernel<false>" in text


# d: one tile and less (2), two tiles (20), the build kernel's second entry per lane and five tiles (65), the last d whose finish
# keeps its matrices in LDS and the first that keeps them in the workspace (94, 95), the flagship (100), the limit (128);
# B: a row, the tile edge, one slab and a row, two slabs and five rows
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("d", (2, 20, 65, FIN_LDS_D, FIN_LDS_D + 1, 100, 128))
def test_rows_and_finish_have_the_bits_of_single_grads_and_meet_float64(d, B):
    n = d
    assert BS == (1, 15, 16, 17, SLAB + 1, 2 * SLAB + 5)
    R, slabs = geometry(B, d)
    assert slabs == (1 if B <= SLAB else 2 if B == SLAB + 1 else 3)
    for m in (1, 3):
        V, W = built(m, d, n)
        ws = Guarded(m * slot_bytes(B, d, n) // 4, "nan", align=16, seed=6)
        g_x, g_W, g_V = rows_finish(m, d, n, B, V, W, ws.t.view(torch.uint8))
        ws.check_guards("workspace")
        g_W.check(f"d {d} B {B} m {m}: g_W")
        g_V.check(f"d {d} B {B} m {m}: g_V")
        ws.fill("junk", seed=9)
        ax, aW, aV = rows_finish(m, d, n, B, V, W, ws.t.view(torch.uint8), fill="junk", seed=50)
        for j in range(m):
            x, gy = (t[:B].contiguous() for t in rows_of(d, j))
            Vj, Wj = V.get(j, n, d).contiguous(), W.get(j, d, d).contiguous()
            g_x[j].check_guards("g_x")
            assert int((g_x[j].words == NAN_BITS).sum()) == 0
            # the oracle-free check: nothing was reordered
            single = grad(x.to(DEV), gy.to(DEV), Wj, Vj, False)
            assert bits_equal(g_x[j].view(B, d), single["g_x"]), (m, j, "g_x")
            assert bits_equal(g_W.get(j, d, d), single["g_W"]), (m, j, "g_W")
            assert bits_equal(g_V.get(j, n, d), single["g_V"]), (m, j, "g_V")
            # two runs (on another fill of every output and of the workspace) give equal bits
            assert bits_equal(ax[j].view(B, d), g_x[j].view(B, d)) and bits_equal(aW.get(j, d, d), g_W.get(j, d, d))
            assert bits_equal(aV.get(j, n, d), g_V.get(j, n, d))
            # float64
            G64 = x.double().t() @ gy.double()
            r = ratio(g_W.get(j, d, d), G64, gw_factor(B, d) * ho.abs_products(x.t(), gy))
            e = rel_err(g_V.get(j, n, d).cpu().numpy(), ho.g_V_from_g_W(vs_of(d, n, j), G64).numpy())
            print(f"many d {d} B {B} m {m} j {j}: g_W ratio to bound {r:.3g}, g_V rel_err {e:.3g}")
            assert r <= 1.0, (m, j, r)
            assert e < 1e-4, (m, j, e)


def test_more_reflections_than_columns_and_sixty_four_permutations():
    """n = d + 3 (the walk is longer than the matrix is wide) and m = 64 (the limit) at a batch of two slabs"""
    for m, d, n, B in ((3, 20, 23, SLAB + 1), (64, 17, 17, 33)):
        V, W = built(m, d, n)
        ws = Guarded(m * slot_bytes(B, d, n) // 4, "nan", align=16, seed=6)
        g_x, g_W, g_V = rows_finish(m, d, n, B, V, W, ws.t.view(torch.uint8))
        ws.check_guards("workspace")
        g_W.check("g_W")
        g_V.check("g_V")
        for j in (range(m) if m < 8 else (0, 1, 31, 62, 63)):
            x, gy = (t[:B].contiguous() for t in rows_of(d, j))
            single = grad(x.to(DEV), gy.to(DEV), W.get(j, d, d).contiguous(), V.get(j, n, d).contiguous(), False)
            assert bits_equal(g_x[j].view(B, d), single["g_x"]) and bits_equal(g_W.get(j, d, d), single["g_W"])
            assert bits_equal(g_V.get(j, n, d), single["g_V"])
            e = rel_err(g_V.get(j, n, d).cpu().numpy(), ho.grads(x, vs_of(d, n, j), gy, False)[2].numpy())
            assert e < 1e-4, (m, j, e)


def test_optional_outputs_left_out_are_not_touched_and_the_others_keep_their_bits():
    m, d, n, B = 3, 20, 20, SLAB + 1
    V, W = built(m, d, n)
    ws = torch.empty(m * slot_bytes(B, d, n), dtype=torch.uint8, device=DEV)
    g_x, g_W, g_V = rows_finish(m, d, n, B, V, W, ws)
    for fill in FILLS:
        ws.fill_(0xA5)
        bx, bW, bV = rows_finish(m, d, n, B, V, W, ws, want_gw=False, fill=fill, seed=70, gx_for=(1,))
        assert bW is None
        bV.check(f"{fill}: g_V without g_W")
        for j in range(m):
            assert bits_equal(bV.get(j, n, d), g_V.get(j, n, d)), (fill, j)
            bx[j].check_guards("g_x")
            if j == 1:
                assert bits_equal(bx[j].view(B, d), g_x[j].view(B, d))
            else:                                           # not asked for: the fill is still there
                want = Guarded(B * d, fill, seed=70 + 10 + j)
                assert torch.equal(bx[j].words, want.words), (fill, j)


@pytest.mark.parametrize("d,n,B,m", [(20, 23, SLAB + 1, 3), (FIN_LDS_D, 97, SLAB + 1, 2), (FIN_LDS_D + 1, 95, 17, 2), (100, 100, 17, 2),
                                     (128, 128, 2 * SLAB + 5, 3)])
def test_guarded_outputs_on_every_fill(d, n, B, m):
    """every output over zeros, the NaN pattern and junk, the workspace poisoned likewise: the guards and the gaps hold, every
    word of every output is written, the inputs keep their bits, and the results do not depend on what the buffers held"""
    results = {}
    for fill in FILLS:
        V = vs_items(m, d, n)
        W = Items(m, d * d, 12, fill, seed=1)
        xs = [Guarded(B * d).set(rows_of(d, j)[0][:B]) for j in range(m)]
        gys = [Guarded(B * d).set(rows_of(d, j)[1][:B]) for j in range(m)]
        snaps = [g.snapshot() for g in xs + gys + [V.g]]
        ws = Guarded(m * slot_bytes(B, d, n) // 4, fill, align=16, seed=6)
        g_x = [Guarded(B * d, fill, seed=20 + j) for j in range(m)]
        g_W, g_V = Items(m, d * d, 8, fill, seed=3), Items(m, n * d, 20, fill, seed=4)
        wsb = dict(workspace=ws.t.view(torch.uint8), workspace_bytes=4 * ws.n, ws_stride=ws.n // m)
        many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
        for j in range(m):
            many(ROWS, m, d, n, B, j=j, W=W.t, w_stride=W.stride, x=xs[j].view(B, d), g_y=gys[j].view(B, d),
                 g_x=g_x[j].view(B, d), **wsb)
        many(FINISH, m, d, n, B, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride, g_W=g_W.t, gw_stride=g_W.stride,
             g_V=g_V.t, gv_stride=g_V.stride, **wsb)
        torch.cuda.synchronize()
        for k, it in (("W", W), ("g_W", g_W), ("g_V", g_V)):
            it.check(f"{fill}: {k}")
        ws.check_guards(f"{fill}: workspace")
        for j in range(m):
            g_x[j].check_guards(f"{fill}: g_x {j}")
            if fill == "nan":
                assert int((g_x[j].words == NAN_BITS).sum()) == 0
        for g, s in zip(xs + gys + [V.g], snaps):
            g.check_unchanged(s, f"{fill}: an input")
        results[fill] = [torch.cat([it.get(j, it.item) for j in range(m)]).clone() for it in (W, g_W, g_V)] \
            + [g.words.clone().view(torch.float32) for g in g_x]
    for fill in FILLS[1:]:
        for a, b in zip(results[fill], results[FILLS[0]]):
            assert bits_equal(a, b), fill


def test_a_zero_row_spoils_its_own_permutation_only():
    m, d, n, B = 3, 20, 23, 40
    V = vs_items(m, d, n)
    bad = vs_of(d, n, 1).clone()
    bad[2] = 0.0
    V.set(1, bad.to(DEV))
    W = Items(m, d * d, 12, "nan", seed=1)
    many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
    ws = torch.empty(m * slot_bytes(B, d, n), dtype=torch.uint8, device=DEV)
    g_x, g_W, g_V = rows_finish(m, d, n, B, V, W, ws)
    for j in range(m):
        for t in (W.get(j, d, d), g_V.get(j, n, d)):
            if j == 1:
                assert bool(torch.isnan(t).all()), j       # every row of W_1 passes through the zero reflection
            else:
                assert bool(torch.isfinite(t).all()), j
        assert bool(torch.isfinite(g_W.get(j, d, d)).all())  # (x^T g_y does not pass through W)
    assert bool(torch.isnan(g_x[1].view(B, d)).all()) and bool(torch.isfinite(g_x[0].view(B, d)).all())
    assert bool(torch.isfinite(g_x[2].view(B, d)).all())
    W.check("W")
    g_V.check("g_V")


# ---- a gated non-default stream ----
def test_three_ops_on_a_gated_non_default_stream():
    """the stream is a field of the struct: build, rows and finish S-gated and null-gated on a side stream, still_closed()
    asserted (tests/stream_gate.py), the results equal to the null-stream bits"""
    m, d, n, B = 3, 20, 23, SLAB + 1
    streams = []

    def make(fill, role):
        V = vs_items(m, d, n)
        xs = [Guarded(B * d).set(rows_of(d, j)[0][:B]) for j in range(m)]
        gys = [Guarded(B * d).set(rows_of(d, j)[1][:B]) for j in range(m)]
        late = stream_gate.late_inputs([(V.g, None)] + [(g, None) for g in xs + gys])
        W = Items(m, d * d, 12, fill, seed=1)
        g_x = [Guarded(B * d, fill, seed=20 + j) for j in range(m)]
        g_W, g_V = Items(m, d * d, 8, fill, seed=3), Items(m, n * d, 20, fill, seed=4)
        ws = Guarded(m * slot_bytes(B, d, n) // 4, fill, align=16, seed=6)

        def call():
            streams.append((role, torch.cuda.current_stream().cuda_stream))
            wsb = dict(workspace=ws.t.view(torch.uint8), workspace_bytes=4 * ws.n, ws_stride=ws.n // m)
            many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
            for j in range(m):
                many(ROWS, m, d, n, B, j=j, W=W.t, w_stride=W.stride, x=xs[j].view(B, d), g_y=gys[j].view(B, d),
                     g_x=g_x[j].view(B, d), **wsb)
            many(FINISH, m, d, n, B, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride, g_W=g_W.t, gw_stride=g_W.stride,
                 g_V=g_V.t, gv_stride=g_V.stride, **wsb)
            out = {f"g_x{j}": g_x[j].t for j in range(m)}
            for k, it in (("W", W), ("g_W", g_W), ("g_V", g_V)):
                for j in range(m):
                    out[f"{k}{j}"] = it.get(j, it.item)
            return out
        guards = [("W", W.g), ("g_W", g_W.g), ("g_V", g_V.g), ("workspace", ws), ("Vs", V.g)] \
            + [(f"g_x{j}", g) for j, g in enumerate(g_x)] + [(f"x{j}", g) for j, g in enumerate(xs)] \
            + [(f"g_y{j}", g) for j, g in enumerate(gys)]
        return stream_gate.Seq(call, late, guards)
    with side_stream() as S:
        stream_gate.run_case(RUN, make, S)
        assert {st for role, st in streams if role == "S"} == {S.cuda_stream} and S.cuda_stream != 0
        assert {st for role, st in streams if role == "ref"} == {0}


# ---- graph capture ----
@pytest.mark.parametrize("d,n,B,m", [(20, 20, SLAB + 1, 3), (100, 103, 33, 2)])
def test_captured_ops_follow_vs_changed_in_place(d, n, B, m):
    V = vs_items(m, d, n)
    W = Items(m, d * d, 12, "nan", seed=1)
    rows = [tuple(t[:B].contiguous().to(DEV) for t in rows_of(d, j)) for j in range(m)]
    g_x = [torch.empty(B, d, device=DEV) for _ in range(m)]
    g_W, g_V = Items(m, d * d, 8, "nan", seed=3), Items(m, n * d, 20, "nan", seed=4)
    ws = torch.empty(m * slot_bytes(B, d, n), dtype=torch.uint8, device=DEV)
    wsb = dict(workspace=ws, workspace_bytes=ws.numel(), ws_stride=ws.numel() // (4 * m))

    def ops():
        many(BUILD, m, d, n, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride)
        for j in range(m):
            many(ROWS, m, d, n, B, j=j, W=W.t, w_stride=W.stride, x=rows[j][0], g_y=rows[j][1], g_x=g_x[j], **wsb)
        many(FINISH, m, d, n, B, Vs=V.t, vs_stride=V.stride, W=W.t, w_stride=W.stride, g_W=g_W.t, gw_stride=g_W.stride,
             g_V=g_V.t, gv_stride=g_V.stride, **wsb)
    ops()                                                   # (warm-up: nothing of the first launch's setup is captured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops()
    for j in range(m):
        V.set(j, ho.init_Vs(n, d, seed=77 + j).to(DEV))      # in place: the captured launches hold the buffer's address
    # eager, on the new values
    ops()
    torch.cuda.synchronize()
    want = [t.clone() for t in g_x] + [it.g.words.clone() for it in (W, g_W, g_V)]
    singles = [build(V.get(j, n, d).contiguous()) for j in range(m)]
    for rep in range(2):
        for t in g_x:
            t.fill_(float("nan"))
        for it in (W, g_W, g_V):
            for j in range(m):
                it.get(j, it.item).fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = list(g_x) + [it.g.words for it in (W, g_W, g_V)]
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (rep, k)
        for j in range(m):
            assert bits_equal(W.get(j, d, d), singles[j])
