"""Every C entry point that takes a stream, and every Python route, on a gated non-default stream (harness: tests/stream_gate.py,
ledger: tests/stream_cases.py).

Every other GPU test runs on the legacy null stream, which orders itself against all blocking streams: there a launch on the
wrong stream, a missing wait between two of the library's streams or a host-synchronous copy still gives the right bits.  Here
each call sequence runs with a non-blocking side stream S current, once with the device side of S held shut (the inputs are
refilled behind the gate) and once with the null stream held shut, and must issue everything without waiting for either; every
output is compared bit for bit with the same sequence on the default stream.  The two self-tests come first: if one of them
fails the harness cannot see on this machine and nothing below means anything.

A proxy of the library records every call of an entry point with a stream parameter together with the stream it was handed:
a test fails when an entry point its ledger line names was not called on S, or when any call got a third stream."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stream_gate as sg
from guarded import NAN_BITS, Guarded
from instance_cases import CASES
from oracle import hint_oracle as orc
from poison_cases import DEV, Rig, check, stream
from stream_cases import ROUTES, STREAM_TESTS
from stream_gate import Seq, late_inputs, run_case

pytestmark = pytest.mark.gpu
FAMILIES = {"wl": "wl_nr1_block", "n3": "n3_cond_block_big_s", "subtree": "subtree_block_big_s", "fly": "fly_block_big_s"}


class SpyLib:
    """the library, with every call of an entry point of STREAM_TESTS recorded as (name, stream handle)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in STREAM_TESTS:
            return fn

        def recorded(*a):
            self.calls.append((name, int(a[-1] or 0)))
            return fn(*a)
        return recorded


@pytest.fixture(scope="module")
def lib():
    from hint_amd import _lib
    real = _lib.load()
    spy = SpyLib(real)
    _lib._lib = spy                     # _lib.load() hands this out: the Python routes' calls are recorded as well
    try:
        yield spy
    finally:
        _lib._lib = real


@pytest.fixture(scope="module")
def S():
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and torch.cuda.default_stream().cuda_stream == 0
    return s


@pytest.fixture(autouse=True)
def fresh_calls(lib):
    torch.cuda.synchronize()
    lib.calls.clear()
    yield
    torch.cuda.synchronize()


def covered(lib, S, test):
    """every entry point whose ledger line names `test` was called with S, and no call got a stream other than S or null"""
    on_s = {n for n, st in lib.calls if st == S.cuda_stream}
    want = {fn for fn, t in STREAM_TESTS.items() if t.split("::")[1] == test}
    assert want, test
    assert want <= on_s, f"{test}: never called on S: {sorted(want - on_s)}"
    other = sorted({(n, hex(st)) for n, st in lib.calls if st not in (0, S.cuda_stream)})
    assert not other, f"{test}: calls on a third stream: {other}"


def case_of(name):
    return next(c for c in CASES if c.name == name)


def chain_case(kind, n_blocks=2):
    """a two-block chain of the wave-local tree, of the FLY tree, or of the conditional n3 tree, 100 rows"""
    d, dc, widths, scale = {"wl": (6, 0, (24, 12), 0.05), "fly": (100, 0, (32, 16, 8), 0.03), "n3": (8, 3, (64, 32, 16), 0.05)}[kind]
    return SimpleNamespace(name=f"{kind}_chain", entry="chain", d=d, dc=dc, widths=widths, scale=scale, big_s=0.0,
                           n_blocks=n_blocks, knobs={}, B=lambda cu: 100)


class Build:
    """the buffers of one built case: late inputs (staged, the live buffer holds NAN_BITS), poisoned outputs and scratch"""

    def __init__(self, fill):
        self.fill, self.late, self.guards, self.k = fill, [], [], 0

    def late_g(self, name, g):
        self.late += late_inputs([(g, None)])
        self.guards.append((name, g))
        return g

    def inp(self, name, values):
        if values is None:
            return None
        v = values.contiguous()
        dtype = v.dtype if v.element_size() == 4 else torch.float32
        g = Guarded(v.numel() * v.element_size() // 4, dtype=dtype)
        g.set(v if v.element_size() == 4 else v.view(-1).view(torch.int32))
        return self.late_g(name, g)

    def out(self, name, n, dtype=torch.float32, fill=None, align=256):
        self.k += 1
        g = Guarded(max(int(n), 1), fill=fill or self.fill, seed=self.k, dtype=dtype, align=align)
        self.guards.append((name, g))
        return g


def ptr(g):
    return None if g is None else g.ptr


# ---- the harness proves it can see ----------------------------------------------------------------------------------------

def test_00_canary_side_stream_and_null_stream_run_independently(S):
    """S-gated setup: the refill of `live` is queued behind the gate on S, and a plain copy of `live` is issued on the default
    stream on purpose.  It must see the NaN pattern: a non-blocking stream and the null stream run independently under this
    machine's queue settings.  If this fails the harness is blind here - every other test of this file proves nothing."""
    live = Guarded(4096)
    late = late_inputs([(live, torch.arange(4096, dtype=torch.float32))])
    dst = Guarded(4096, fill="zero")
    torch.cuda.synchronize()
    gate = sg.Gate(S, 50.0).open()
    with torch.cuda.stream(S):
        sg.refill(SimpleNamespace(late=late))
    dst.words.copy_(live.words)                         # default stream: does not wait for S
    torch.cuda.default_stream().synchronize()
    closed = gate.still_closed()
    S.synchronize()
    torch.cuda.synchronize()
    assert closed, "the harness is blind on this machine: the gate on S had ended before the default stream's copy was done"
    assert bool((dst.words == NAN_BITS).all()), \
        "the harness is blind on this machine: a copy on the default stream waited for the gated side stream"
    assert bool((live.t == torch.arange(4096, device=DEV)).all())
    dst.check_guards("canary dst"); live.check_guards("canary live")


def block_make(lib, rig, B, forward_stream=None):
    """pack -> forward with tape -> backward -> inverse of one block; forward_stream: the seeded mistake's stream for the forward"""
    case = rig.case
    d, dc = case.d, case.dc
    host_in = rig.inputs(B)
    tape_n, ws_n = rig.sizes(B)
    plan = rig.plan

    def make(fill, role):
        b = Build(fill)
        params = b.late_g("params", rig.flat_params(0, fill))
        x, c, zi, gz, gJ = (b.inp(n, t) for n, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        packed = b.out("packed", lib.hint_plan_packed_floats(plan))
        z, J, xi, Ji, gx = b.out("z", B * d), b.out("J", B), b.out("xi", B * d), b.out("Ji", B), b.out("gx", B * d)
        gc = b.out("gc", B * dc) if dc else None
        tape, ws, gp = b.out("tape", tape_n), b.out("ws", ws_n), b.out("gp", rig.total)

        def call():
            st = stream()
            check(lib.hint_block_pack(plan, params.ptr, packed.ptr, st), "hint_block_pack")
            check(lib.hint_block_forward(plan, params.ptr, packed.ptr, x.ptr, ptr(c), z.ptr, J.ptr, tape.ptr, B,
                                         st if forward_stream is None else forward_stream), "hint_block_forward")
            check(lib.hint_block_backward(plan, params.ptr, packed.ptr, x.ptr, tape.ptr, ptr(c), gz.ptr, gJ.ptr, gx.ptr, ptr(gc),
                                          gp.ptr, 0, ws.ptr, 4 * ws_n, B, st), "hint_block_backward")
            check(lib.hint_block_inverse(plan, params.ptr, packed.ptr, zi.ptr, ptr(c), xi.ptr, Ji.ptr, B, st), "hint_block_inverse")
            out = dict(packed=packed.t, z=z.t, J=J.t, xi=xi.t, Ji=Ji.t, gx=gx.t, gp=gp.t)
            if dc:
                out["gc"] = gc.t
            return out
        return Seq(call, b.late, b.guards)
    return make


def test_01_seeded_mistake_is_reported(lib, S):
    """the smallest wave-local block with hint_block_forward handed stream 0 while everything else sits on gated S: the forward
    runs before the pack and before its input exists, and the S-gated comparison must say so"""
    rig = Rig(case_of(FAMILIES["wl"]), lib)
    good, bad = block_make(lib, rig, 100), block_make(lib, rig, 100, forward_stream=0)
    ref = sg.reference("seeded mistake", good, sg.FILLS[0])
    sg.warm_up("seeded mistake", good, S)
    sg.s_gated("seeded mistake: the right stream", good, S, 20.0, ref)
    try:
        with pytest.raises(AssertionError, match="differs from the default-stream run"):
            sg.s_gated("seeded mistake", bad, S, 20.0, ref)
    except (Exception, pytest.fail.Exception) as e:              # (pytest.raises' own failure is not an AssertionError)
        raise AssertionError("the harness is blind on this machine: a forward on the null stream, ahead of the gated pack and of "
                             f"its input, went unnoticed ({e})")
    torch.cuda.synchronize()


# ---- the C entry points ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", list(FAMILIES))
def test_block_families(lib, S, fam):
    case = case_of(FAMILIES[fam])
    rig = Rig(case, lib)
    run_case(f"block {fam}", block_make(lib, rig, case.B(0)), S)
    covered(lib, S, "test_block_families")


@pytest.mark.parametrize("fam", ["wl", "n3", "fly"])
def test_ex_forms(lib, S, fam):
    """the _ex forms with a fused permutation, J_in and loss_acc (g_J = NULL, gz_scale / gJ_const: what the module route passes)"""
    case = case_of(FAMILIES[fam])
    rig = Rig(case, lib)
    B, d, dc, plan = case.B(0), case.d, case.dc, rig.plan
    host_in = rig.inputs(B)
    perm_h = orc.random_orthogonal(d, seed=7, dtype=torch.float64).float()
    jin_h = torch.randn(B, generator=torch.Generator().manual_seed(3))
    tape_n, ws_n = rig.sizes(B)

    def make(fill, role):
        b = Build(fill)
        params = b.late_g("params", rig.flat_params(0, fill))
        x, c, zi, gz, _ = (b.inp(n, t) for n, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        perm, J_in = b.inp("perm", perm_h), b.inp("J_in", jin_h)
        packed = b.out("packed", lib.hint_plan_packed_floats(plan))
        z, J, tape, loss = b.out("z", B * d), b.out("J", B), b.out("tape", tape_n), b.out("loss", 128, fill="zero")
        xi, Ji, gx = b.out("xi", B * d), b.out("Ji", B), b.out("gx", B * d)
        gc, gp, ws = (b.out("gc", B * dc) if dc else None), b.out("gp", rig.total), b.out("ws", ws_n)

        def call():
            st = stream()
            check(lib.hint_block_pack(plan, params.ptr, packed.ptr, st), "hint_block_pack")
            check(lib.hint_block_forward_ex(plan, params.ptr, packed.ptr, x.ptr, ptr(c), z.ptr, J.ptr, tape.ptr, perm.ptr, J_in.ptr,
                                            loss.ptr, B, st), "hint_block_forward_ex")
            check(lib.hint_block_backward_ex(plan, params.ptr, packed.ptr, None, tape.ptr, ptr(c), z.ptr, None, gx.ptr, ptr(gc),
                                             gp.ptr, 0, ws.ptr, 4 * ws_n, perm.ptr, 1.0 / B, -1.0 / B, B, st), "hint_block_backward_ex")
            check(lib.hint_block_inverse_ex(plan, params.ptr, packed.ptr, zi.ptr, ptr(c), xi.ptr, Ji.ptr, perm.ptr, J_in.ptr, B, st),
                  "hint_block_inverse_ex")
            out = dict(z=z.t, J=J.t, xi=xi.t, Ji=Ji.t, gx=gx.t, gp=gp.t, loss=loss.t)
            if dc:
                out["gc"] = gc.t
            return out
        return Seq(call, b.late, b.guards, loose=("loss",))
    run_case(f"_ex forms {fam}", make, S)
    covered(lib, S, "test_ex_forms")


class Chain:
    """a training (or inference) chain of a Rig on guarded buffers, committed on the default stream when the case is built"""

    def __init__(self, b, rig, B, fill, tape=True, param_ptrs=None, perms=None, commit=True):
        lib, plan, nb = rig.lib, rig.plan, rig.n_blocks
        tape_n, ws_n = rig.sizes(B)
        self.lib, self.ws_n = lib, ws_n
        self.params = [b.late_g(f"params{i}", rig.flat_params(i, fill)) for i in range(nb)] if param_ptrs is None else []
        self.pp = [g.ptr for g in self.params] if param_ptrs is None else param_ptrs
        self.packed = [b.out(f"packed{i}", lib.hint_plan_packed_floats(plan)) for i in range(nb)]
        perms = rig.perms if perms is None else perms
        self.perms = [b.inp(f"perm{i}", p) for i, p in enumerate(perms)]
        self.tapes = [b.out(f"tape{i}", tape_n) if tape else None for i in range(nb)]
        self.wss = [b.out(f"ws{i}", ws_n) if tape else None for i in range(nb)]
        self.gps = [b.out(f"gp{i}", rig.total) if tape else None for i in range(nb)]
        self.ch = C.c_void_p()
        check(lib.hint_chain_create(plan, nb, B, C.byref(self.ch)), "hint_chain_create")
        for i in range(nb):
            check(lib.hint_chain_set_block(self.ch, i, self.pp[i], self.packed[i].ptr, ptr(self.perms[i]), ptr(self.tapes[i]),
                                           ptr(self.wss[i]), 4 * ws_n if tape else 0, ptr(self.gps[i])), "hint_chain_set_block")
        if commit:
            self.commit()

    def commit(self):
        check(self.lib.hint_chain_commit(self.ch), "hint_chain_commit")

    def pack(self, plan, st):
        for p, k in zip(self.pp, self.packed):
            check(self.lib.hint_block_pack(plan, p, k.ptr, st), "hint_block_pack")

    def close(self):
        self.lib.hint_chain_destroy(self.ch)


@pytest.mark.parametrize("kind", ["wl", "fly"])
def test_chains(lib, S, kind):
    """pack of both blocks -> hint_chain_forward -> hint_chain_backward -> hint_chain_inverse of a two-block chain"""
    rig = Rig(chain_case(kind), lib)
    B, d, plan = 100, rig.case.d, rig.plan
    host_in = rig.inputs(B)

    def make(fill, role):
        b = Build(fill)
        ch = Chain(b, rig, B, fill)
        x, _, zi, gz, gJ = (b.inp(n, t) for n, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        z, J, xi, Ji, gx = b.out("z", B * d), b.out("J", B), b.out("xi", B * d), b.out("Ji", B), b.out("gx", B * d)

        def call():
            st = stream()
            ch.pack(plan, st)
            check(lib.hint_chain_forward(ch.ch, x.ptr, None, z.ptr, J.ptr, None, None, st), "hint_chain_forward")
            check(lib.hint_chain_backward(ch.ch, x.ptr, None, gz.ptr, gJ.ptr, gx.ptr, None, 1.0, 0.0, 0, st), "hint_chain_backward")
            check(lib.hint_chain_inverse(ch.ch, zi.ptr, None, xi.ptr, Ji.ptr, None, st), "hint_chain_inverse")
            return dict(z=z.t, J=J.t, xi=xi.t, Ji=Ji.t, gx=gx.t, **{f"gp{i}": g.t for i, g in enumerate(ch.gps)})
        return Seq(call, b.late, b.guards, close=ch.close)
    run_case(f"chain {kind}", make, S)
    covered(lib, S, "test_chains")


def test_noisy_forwards(lib, S):
    """hint_block_forward_noisy and hint_chain_forward_noisy (Philox keyed by rng_state, x_noisy written)"""
    rig = Rig(chain_case("wl"), lib)
    B, d, plan = 100, rig.case.d, rig.plan
    host_in = rig.inputs(B)

    def make(fill, role):
        b = Build(fill)
        ch = Chain(b, rig, B, fill, perms=[None] * rig.n_blocks)
        x = b.inp("x", host_in[0])
        rng = b.inp("rng", torch.tensor([42, 3], dtype=torch.int64))
        outs = {k: b.out(k, n) for k, n in (("xn_b", B * d), ("z_b", B * d), ("J_b", B), ("xn_c", B * d), ("z_c", B * d), ("J_c", B))}

        def call():
            st = stream()
            ch.pack(plan, st)
            check(lib.hint_block_forward_noisy(plan, ch.pp[0], ch.packed[0].ptr, x.ptr, None, outs["z_b"].ptr, outs["J_b"].ptr,
                                               ch.tapes[0].ptr, None, None, None, 0.25, rng.ptr, outs["xn_b"].ptr, B, st),
                  "hint_block_forward_noisy")
            check(lib.hint_chain_forward_noisy(ch.ch, x.ptr, None, outs["z_c"].ptr, outs["J_c"].ptr, None, None, 0.25, rng.ptr,
                                               outs["xn_c"].ptr, st), "hint_chain_forward_noisy")
            return {k: g.t for k, g in outs.items()}
        return Seq(call, b.late, b.guards, close=ch.close)
    run_case("noisy forwards", make, S)
    covered(lib, S, "test_noisy_forwards")


def test_backward_parts_and_wgrad_ranges(lib, S):
    """hint_chain_forward, part A alone (hint_chain_backward_parts, parts = 1), then part B in two block ranges
    (hint_chain_wgrad_range [0, 1) and [1, 2)) on the conditional n3 chain"""
    rig = Rig(chain_case("n3"), lib)
    B, d, dc, plan = 100, rig.case.d, rig.case.dc, rig.plan
    host_in = rig.inputs(B)

    def make(fill, role):
        b = Build(fill)
        ch = Chain(b, rig, B, fill)
        x, c, _, gz, gJ = (b.inp(n, t) for n, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        z, J, gx, gc = b.out("z", B * d), b.out("J", B), b.out("gx", B * d), b.out("gc", B * dc)

        def call():
            st = stream()
            ch.pack(plan, st)
            check(lib.hint_chain_forward(ch.ch, x.ptr, c.ptr, z.ptr, J.ptr, None, None, st), "hint_chain_forward")
            check(lib.hint_chain_backward_parts(ch.ch, x.ptr, c.ptr, gz.ptr, gJ.ptr, gx.ptr, gc.ptr, 1.0, 0.0, 0, 1, st),
                  "hint_chain_backward_parts")
            check(lib.hint_chain_wgrad_range(ch.ch, x.ptr, c.ptr, 0, 1, 2, st), "hint_chain_wgrad_range")
            check(lib.hint_chain_wgrad_range(ch.ch, x.ptr, c.ptr, 0, 0, 1, st), "hint_chain_wgrad_range")
            return dict(z=z.t, J=J.t, gx=gx.t, gc=gc.t, **{f"gp{i}": g.t for i, g in enumerate(ch.gps)})
        return Seq(call, b.late, b.guards, close=ch.close)
    run_case("backward parts + wgrad ranges", make, S)
    covered(lib, S, "test_backward_parts_and_wgrad_ranges")


@pytest.mark.parametrize("mode", ["chain", "gathered"])
def test_fused_adam(lib, S, mode):
    """hint_chain_backward_adam on a chain; hint_block_forward_ex + hint_block_backward_rows per block and one
    hint_chain_wgrad_adam over the gathered blocks: the parameters are slices of the arena P the fused step writes"""
    rig = Rig(chain_case("n3"), lib)
    B, d, dc, plan, nb, total = 100, rig.case.d, rig.case.dc, rig.plan, rig.n_blocks, rig.total
    gap = 4 * 37
    n = gap + nb * (total + gap)
    offs = [gap + i * (total + gap) for i in range(nb)]
    host_in = rig.inputs(B)
    opt_h = torch.tensor([1e-3, 0.9, 0.95, 1e-3 / (1 - 0.9 ** 3), 1 / math.sqrt(1 - 0.95 ** 3)], dtype=torch.float32)
    xs_h = [torch.randn(B, d, generator=torch.Generator().manual_seed(40 + i)) for i in range(nb)]

    def make(fill, role):
        b = Build(fill)
        P, M, V = (b.out(k, n, align=16) for k in "PMV")
        M.t.copy_(Guarded(n, fill="junk", seed=600).t * 1e-3)
        V.t.copy_(Guarded(n, fill="junk", seed=601).t.abs() * 1e-6)
        for i in range(nb):
            P.t[offs[i]:offs[i] + total].copy_(rig.flat_params(i, "zero").t)
        for g in (P, M, V):                                   # the arenas are inputs as well: staged, NaN until the refill
            b.late += late_inputs([(g, None)])
        views = [P.ptr + 4 * o for o in offs]
        ch = Chain(b, rig, B, fill, param_ptrs=views, commit=False, perms=None if mode == "chain" else [None] * nb)
        x, c, _, gz, gJ = (b.inp(k, t) for k, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        opt = b.inp("opt_state", opt_h)
        gx, gc = b.out("gx", B * d), b.out("gc", B * dc)
        zs, Js = [b.out(f"z{i}", B * d) for i in range(nb)], [b.out(f"J{i}", B) for i in range(nb)]
        xs = [b.inp(f"x{i}", t) for i, t in enumerate(xs_h)] if mode == "gathered" else []
        if mode == "gathered":
            for i in range(nb):
                check(lib.hint_chain_set_block_io(ch.ch, i, xs[i].ptr, c.ptr, None), "hint_chain_set_block_io")
        ch.commit()

        def call():
            st = stream()
            ch.pack(plan, st)
            if mode == "chain":
                check(lib.hint_chain_forward(ch.ch, x.ptr, c.ptr, zs[0].ptr, Js[0].ptr, None, None, st), "hint_chain_forward")
                check(lib.hint_chain_backward_adam(ch.ch, x.ptr, c.ptr, gz.ptr, gJ.ptr, gx.ptr, gc.ptr, 1.0, 0.0, P.ptr, M.ptr, V.ptr,
                                                   n, opt.ptr, 0.9, 0.95, 1e-4, 1e-5, 1.0, 5.0, st), "hint_chain_backward_adam")
            else:
                for i in range(nb):
                    check(lib.hint_block_forward_ex(plan, views[i], ch.packed[i].ptr, xs[i].ptr, c.ptr, zs[i].ptr, Js[i].ptr,
                                                    ch.tapes[i].ptr, None, None, None, B, st), "hint_block_forward_ex")
                    check(lib.hint_block_backward_rows(plan, views[i], ch.packed[i].ptr, xs[i].ptr, ch.tapes[i].ptr, c.ptr, gz.ptr,
                                                       gJ.ptr, gx.ptr, gc.ptr, ch.wss[i].ptr, 4 * ch.ws_n, None, 1.0, 0.0, B, st),
                          "hint_block_backward_rows")
                check(lib.hint_chain_wgrad_adam(ch.ch, None, None, P.ptr, M.ptr, V.ptr, n, opt.ptr, 0.9, 0.95, 1e-4, 1e-5, 1.0, 5.0,
                                                st), "hint_chain_wgrad_adam")
            return dict(gx=gx.t, gc=gc.t, z0=zs[0].t, J0=Js[0].t,          # the blocks' slices of the arenas (the gaps hold the fill)
                        **{f"{k}{i}": g.t[o:o + total] for k, g in zip("PMV", (P, M, V)) for i, o in enumerate(offs)})
        return Seq(call, b.late, b.guards, close=ch.close)
    run_case(f"fused adam {mode}", make, S)
    on_s = {k for k, st in lib.calls if st == S.cuda_stream}
    want = {"chain": {"hint_chain_backward_adam"}, "gathered": {"hint_chain_wgrad_adam", "hint_block_backward_rows"}}[mode]
    assert want <= on_s, sorted(want - on_s)


@pytest.mark.parametrize("fam", ["wl", "n3", "fly"])
def test_inverse_backward(lib, S, fam):
    """hint_block_inverse -> hint_block_inverse_backward (about a dozen launches and two copies per tree level in one
    caller-supplied workspace), with a fused permutation and, on the conditional tree, with g_c; the warm-up builds the level plans"""
    case = case_of(FAMILIES[fam])
    rig = Rig(case, lib)
    B, d, dc, plan = case.B(0), case.d, case.dc, rig.plan
    nbytes = int(lib.hint_plan_inverse_workspace_bytes(plan, B))
    assert nbytes > 0, lib.hint_last_error()
    host_in = rig.inputs(B)
    perm_h = orc.random_orthogonal(d, seed=9, dtype=torch.float64).float()

    def make(fill, role):
        b = Build(fill)
        params = b.late_g("params", rig.flat_params(0, fill))
        _, c, zi, gz, gJ = (b.inp(k, t) for k, t in zip(("x", "c", "zi", "gz", "gJ"), host_in))
        perm = b.inp("perm", perm_h)
        packed = b.out("packed", lib.hint_plan_packed_floats(plan))
        xo, J, gzo, gp, ws = b.out("xo", B * d), b.out("J", B), b.out("gz_out", B * d), b.out("gp", rig.total), b.out("ws", nbytes // 4 + 1)
        gc = b.out("gc", B * dc) if dc else None

        def call():
            st = stream()
            check(lib.hint_block_pack(plan, params.ptr, packed.ptr, st), "hint_block_pack")
            check(lib.hint_block_inverse_ex(plan, params.ptr, packed.ptr, zi.ptr, ptr(c), xo.ptr, J.ptr, perm.ptr, None, B, st),
                  "hint_block_inverse_ex")
            check(lib.hint_block_inverse_backward(plan, params.ptr, xo.ptr, ptr(c), gz.ptr, gJ.ptr, gzo.ptr, ptr(gc), gp.ptr, 0, ws.ptr,
                                                  nbytes, perm.ptr, B, st), "hint_block_inverse_backward")
            out = dict(xo=xo.t, J=J.t, gz=gzo.t, gp=gp.t)
            if dc:
                out["gc"] = gc.t
            return out
        return Seq(call, b.late, b.guards)
    run_case(f"inverse backward {fam}", make, S)
    covered(lib, S, "test_inverse_backward")


def test_ext_coeffs_and_affine_chain(lib, S):
    """hint_block_ext_coeffs, then forward and inverse of an inference chain whose first block takes a per-row affine step from
    the coefficients (hint_chain_set_block_affine)"""
    import hint_amd
    D, dc, h, R = 100, 4, 224, 100
    torch.manual_seed(3)
    mod = hint_amd.ExternalAffineCoupling([(D,)], dims_c=[(dc,)], F_args={"internal_size": h}).to(DEV)
    for p in mod.parameters():
        p.data = 0.1 * torch.randn_like(p)
    eng = mod.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    eng.pack()
    torch.cuda.synchronize()
    rig = Rig(chain_case("fly"), lib)
    c_h = torch.randn(R, dc, generator=torch.Generator().manual_seed(5))
    x_h = torch.randn(R, D, generator=torch.Generator().manual_seed(8))

    def make(fill, role):
        b = Build(fill)
        c, x = b.inp("c", c_h), b.inp("x", x_h)
        coef = b.out("coef", R * 2 * D)
        ch = Chain(b, rig, R, fill, tape=False, commit=False)
        check(lib.hint_chain_set_block_affine(ch.ch, 0, coef.ptr, 2 * D), "hint_chain_set_block_affine")
        ch.commit()
        z, J, xi, Ji = b.out("z", R * D), b.out("J", R), b.out("xi", R * D), b.out("Ji", R)

        def call():
            st = stream()
            ch.pack(rig.plan, st)
            check(lib.hint_block_ext_coeffs(eng.plan, eng.arena.data_ptr(), eng.packed.data_ptr(), c.ptr, R, coef.ptr, st),
                  "hint_block_ext_coeffs")
            check(lib.hint_chain_forward(ch.ch, x.ptr, None, z.ptr, J.ptr, None, None, st), "hint_chain_forward")
            check(lib.hint_chain_inverse(ch.ch, x.ptr, None, xi.ptr, Ji.ptr, None, st), "hint_chain_inverse")
            return dict(coef=coef.t, z=z.t, J=J.t, xi=xi.t, Ji=Ji.t)
        return Seq(call, b.late, b.guards, close=ch.close)
    run_case("ext coeffs + affine chain", make, S)
    covered(lib, S, "test_ext_coeffs_and_affine_chain")


def test_pack_group(lib, S):
    """hint_pack_group_run_ex (clear, pack, rng and opt_state prologue) and hint_pack_group_run"""
    rig = Rig(chain_case("n3", 3), lib)
    nb, plan = rig.n_blocks, rig.plan
    packed_n = lib.hint_plan_packed_floats(plan)

    def make(fill, role):
        b = Build(fill)
        params = [b.late_g(f"params{i}", rig.flat_params(i, fill, 1)) for i in range(nb)]
        packed = [b.out(f"packed{i}", packed_n) for i in range(nb)]
        packed2 = [b.out(f"packed_b{i}", packed_n) for i in range(nb)]
        grps = []
        for pk in (packed, packed2):
            grp = C.c_void_p()
            check(lib.hint_pack_group_create((C.c_void_p * nb)(*([plan.value] * nb)), (C.c_void_p * nb)(*[g.ptr for g in params]),
                                             (C.c_void_p * nb)(*[g.ptr for g in pk]), nb, C.byref(grp)), "hint_pack_group_create")
            grps.append(grp)
        zb = b.out("zero_buf", 300, fill="junk")
        rng = b.inp("rng", torch.tensor([123, 6], dtype=torch.int64))
        opt = b.inp("opt", torch.tensor([2e-3, 0.9, 0.95, float("nan"), float("nan")]))

        def call():
            st = stream()
            check(lib.hint_pack_group_run_ex(grps[0], zb.ptr, 131, rng.ptr, opt.ptr, st), "hint_pack_group_run_ex")
            check(lib.hint_pack_group_run(grps[1], st), "hint_pack_group_run")
            return dict(zb=zb.t, rng=rng.t, opt=opt.t[:5], **{f"packed{i}": g.t for i, g in enumerate(packed)},
                        **{f"packed_b{i}": g.t for i, g in enumerate(packed2)})
        return Seq(call, b.late, b.guards, close=lambda: [lib.hint_pack_group_destroy(g) for g in grps])
    # opt_state[3..4] start as NaN by design (the prologue writes them): the reference's finiteness check looks at them written
    run_case("pack group", make, S)
    covered(lib, S, "test_pack_group")


def test_adam_steps(lib, S):
    """hint_adam_step, hint_adam_step_dev and hint_adam_multi_step (two segments of odd sizes), each on its own buffers"""
    n, extra = 4 * 1000 + 3, 61
    seg_n = (1001, 2 * 1024 + 7)

    def make(fill, role):
        b = Build(fill)

        def pgmv(tag, m):
            bufs = [b.out(f"{tag}{k}", m, fill="junk", align=16) for k in "PGMV"]
            bufs[2].t.mul_(1e-3)
            bufs[3].t.copy_(bufs[3].t.abs() * 1e-3)
            for g in bufs:
                b.late += late_inputs([(g, None)])
            return bufs
        host_bufs, dev_bufs = pgmv("host_", n + extra), pgmv("dev_", n + extra)
        segs = [pgmv(f"seg{i}_", m) for i, m in enumerate(seg_n)]
        opt = b.inp("opt", torch.tensor([1e-3, 0.9, 0.95, 1e-3 / (1 - 0.9 ** 4), 1 / math.sqrt(1 - 0.95 ** 4)]))
        from hint_amd._lib import AdamSeg
        arr = (AdamSeg * len(segs))()
        for i, (sb, m) in enumerate(zip(segs, seg_n)):
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = sb[0].ptr, sb[1].ptr, sb[2].ptr, sb[3].ptr, m
        h = C.c_void_p()
        check(lib.hint_adam_multi_create(arr, len(segs), C.byref(h)), "hint_adam_multi_create")

        def call():
            st = stream()
            P, G, M, V = host_bufs
            check(lib.hint_adam_step(P.ptr, G.ptr, M.ptr, V.ptr, n, 4, 1e-3, 0.9, 0.95, 1e-4, 1e-5, 0.5, 5.0, 1, st), "hint_adam_step")
            P, G, M, V = dev_bufs
            check(lib.hint_adam_step_dev(P.ptr, G.ptr, M.ptr, V.ptr, n, opt.ptr, 0.9, 0.95, 1e-4, 1e-5, 0.5, 5.0, 1, st),
                  "hint_adam_step_dev")
            check(lib.hint_adam_multi_step(h, 4, 1e-3, 0.9, 0.95, 1e-4, 1e-5, 0.5, 5.0, 0, st), "hint_adam_multi_step")
            return {name: g.t for name, g in b.guards if name != "opt"}
        return Seq(call, b.late, b.guards, close=lambda: lib.hint_adam_multi_destroy(h))
    run_case("adam steps", make, S)
    covered(lib, S, "test_adam_steps")


# ---- the eleven descriptor entry points, at the shapes of their own poison tests ----------------------------------------------

def _desc_mmd(lib):
    import mmd_oracle as mo
    from test_gpu_mmd import T, make_sets, run_desc
    n_x, n_y, d = T + 3, 2 * T + 1, 7
    x_h, y_h = (torch.from_numpy(a) for a in make_sets(n_x, n_y, d, seed=21))
    nbytes = lib.hint_mmd_workspace_bytes(n_x, n_y, d)

    def make(fill, role):
        b = Build(fill)
        x, y, out, ws = b.inp("x", x_h), b.inp("y", y_h), b.out("out", 4), b.out("ws", nbytes // 4)

        def call():
            run_desc(x.ptr, y.ptr, n_x, n_y, d, mo.DEFAULT, out.ptr, ws.ptr, nbytes, sync=False)
            return dict(out=out.t)
        return Seq(call, b.late, b.guards)
    return make


def _desc_abc(lib):
    import abc_oracle as ao
    from test_gpu_abc import R, run_desc
    N, ny, k = R + 1, 4, R + 1
    y_h, t_h = (torch.from_numpy(a) for a in ao.random_inputs(N, ny, 6 + ny))
    nbytes = lib.hint_abc_workspace_bytes(N, ny, k)

    def make(fill, role):
        b = Build(fill)
        y, t = b.inp("y", y_h), b.inp("target", t_h)
        idx, dist, ws = b.out("idx", k, dtype=torch.int32), b.out("dist", k), b.out("ws", nbytes // 4)

        def call():
            run_desc(y.ptr, t.ptr, N, ny, k, idx.ptr, dist.ptr, ws.ptr, nbytes, sync=False)
            return dict(idx=idx.t, dist=dist.t)
        return Seq(call, b.late, b.guards)
    return make


def _desc_corr(lib):
    import corr_oracle as co
    from test_gpu_corr import mixed, run_desc
    n, d = 1001, 37
    x_h = torch.from_numpy(mixed(n, d, seed=21))
    t_h = torch.from_numpy(co.corrcoef64(mixed(n, d, seed=22)))
    nbytes = lib.hint_corr_workspace_bytes(n, d)

    def make(fill, role):
        b = Build(fill)
        x, t = b.inp("x", x_h), b.inp("target", t_h)
        out, corr, ws = b.out("out", 2 * 4), b.out("corr", 2 * d * d), b.out("ws", nbytes // 4)

        def call():
            run_desc(x.ptr, n, d, t.ptr, corr.ptr, out.ptr, ws.ptr, nbytes, sync=False)
            return dict(out=out.words.view(torch.float64), corr=corr.words.view(torch.float64))
        return Seq(call, b.late, b.guards)
    return make


def _desc_curve(lib):
    import curve_oracle as co
    from test_gpu_curve import run_desc
    K, P, N = 5, 100, 203
    x_h = torch.from_numpy(co.gauss(41, N, K))
    e_h = torch.from_numpy(np.random.RandomState(42).randn(N, 2).astype(np.float32))
    nbytes = lib.hint_curve_workspace_bytes(N, K, P)

    def make(fill, role):
        b = Build(fill)
        x, e, t = b.inp("x", x_h), b.inp("eps", e_h), b.inp("target", torch.tensor([0.5, -0.25]))
        y, dist, mean, ws = b.out("y", 2 * N), b.out("dist", N), b.out("mean", 1), b.out("ws", nbytes // 4)

        def call():
            run_desc(x.ptr, N, K, P, e.ptr, 0.05, t.ptr, y.ptr, dist.ptr, mean.ptr, ws.ptr, nbytes, sync=False)
            return dict(y=y.t, dist=dist.t, mean=mean.t)
        return Seq(call, b.late, b.guards)
    return make


def _desc_hausdorff(lib):
    from test_gpu_hausdorff import ragged_case, run_desc
    K, P, lens = 5, 100, (130, 1, 2, 65)
    N = len(lens)
    x_h, tpl_h, pr_h, off_h = (torch.from_numpy(a) for a in ragged_case(K, P, lens, 50 + K))
    T = len(tpl_h)

    def make(fill, role):
        b = Build(fill)
        x, a, p, o = b.inp("x", x_h), b.inp("a_points", tpl_h), b.inp("a_params", pr_h), b.inp("a_offsets", off_h)
        outs = [b.out(k, n) for k, n in (("max_h", N), ("avg_h", N), ("chamfer", 2 * N), ("points", 2 * N * P))]

        def call():
            run_desc(x.ptr, None, N, K, P, a.ptr, o.ptr, p.ptr, T, *(g.ptr for g in outs), sync=False)
            return {k: g.t for k, g in zip(("max_h", "avg_h", "chamfer", "points"), outs)}
        return Seq(call, b.late, b.guards)
    return make


def _runner_case(inputs, shapes, ints, run):
    """a case over one of the checked-argument runners below the public functions (curves._plus_run, _lf_run, _pf_run, _ov_run,
    shapes._lens_run, _fcoef_run: they take the buffers to write into): inputs {name: host tensor}, shapes {output: shape}"""
    def make(fill, role):
        b = Build(fill)
        live = {k: b.inp(k, v) for k, v in inputs.items()}
        views = {k: live[k].view(*v.shape) for k, v in inputs.items()}
        bufs = {k: b.out(k, int(np.prod(s)), dtype=torch.int32 if k in ints else torch.float32) for k, s in shapes.items()}
        out = {k: bufs[k].view(*s) for k, s in shapes.items()}

        def call():
            run(views, out)
            return {k: v for k, v in out.items() if k != "workspace"}
        return Seq(call, b.late, b.guards)
    return make


def _desc_plus(lib):
    import curve_oracle as co
    import plus_oracle as po
    from test_gpu_plus import ALL, run
    N, K, P, md = 5, 5, 257, 0.02
    inputs = dict(params=torch.from_numpy(po.draw_params(71, N, (md,))),
                  curve=torch.from_numpy((co.gauss(72, N, K) * np.float32(3)).astype(np.float32)))
    shapes = dict(segments=(N, 12, 2, 2), keep=(N,), counts=(N, 12), loss=(N, 2), max_h=(N,), avg_h=(N,))
    return _runner_case(inputs, shapes, ("keep", "counts"), lambda v, out: run(v["params"], v["curve"], P, md, ALL, 0, out))


def _desc_lensfit(lib):
    import lensfit_oracle as lo
    from test_gpu_lensfit import ALL, run
    N, S, steps, P, M = 5, 3, 2, 257, 1023
    inputs = dict(curve=torch.from_numpy(lo.lens_rows(1101, N)), proto=torch.from_numpy(lo.lens_prototype(M)),
                  starts=torch.from_numpy(lo.golden_grad_params(1102, N * S).reshape(N, S, 4)))
    shapes = dict(params=(N, 4), loss=(N,), best=(N,), all_params=(N, S, 4), all_loss=(N, S), grad=(N, S, 4), trace=(N, S, steps, 9))
    return _runner_case(inputs, shapes, ("best",), lambda v, out: run(v["curve"], v["proto"], v["starts"], steps, ALL, 0, out, P=P))


def _desc_plusfit(lib):
    import plusfit_oracle as pfo
    from test_gpu_plusfit import ALL, INTS, _shapes, run
    N, S, steps, P = 5, 3, 2, 257
    x, base = pfo.plus_rows(1201, N)
    starts = np.stack([pfo.eval_params(base, 1202 + s) for s in range(S)], 1)
    inputs = dict(curve=torch.from_numpy(x), starts=torch.from_numpy(starts))
    return _runner_case(inputs, _shapes(N, S, steps), INTS, lambda v, out: run(v["curve"], v["starts"], steps, ALL, 0, out, P=P))


def _desc_overlap(lib):
    import overlap_oracle as oo
    from test_gpu_overlap import ALL, run, shapes
    N, P = 5, 257
    x, proto, params = oo.lens_case(305, N, 1025)
    inputs = dict(curve=torch.from_numpy(x), polygon=torch.from_numpy(proto), params=torch.from_numpy(params))
    return _runner_case(inputs, shapes(N), ("crossings",),
                        lambda v, out: run(v["curve"], P, v["polygon"], None, v["params"], None, ALL, 0, out))


SEED = 0x5EED0123456789AB


def _desc_lensgen(lib):
    from hint_amd import shapes
    n = 64 * 5 + 37
    nbytes = lib.hint_lensgen_workspace_bytes(n)
    table = dict(x=(n, 20), ring=(n, 32, 2), counts=(n,), eps=(n, 2), draws_out=(n, 4), workspace=(nbytes,))
    want = ["x", "ring", "counts", "eps", "draws_out"]

    def run(v, out):
        o = dict(out)
        o["workspace"] = out["workspace"].view(torch.uint8)[:nbytes]
        shapes._lens_run(n, SEED, 0, torch.device(DEV), None, want, out=o)
    shp = dict(table)
    shp["workspace"] = (nbytes // 4 + 1,)
    return _runner_case({}, shp, ("counts", "workspace"), run)


def _desc_fcoef(lib):
    from hint_amd import shapes
    n, k = 64 * 5 + 37, 5
    ring = shapes._lens_run(n, SEED, 0, torch.device(DEV), None, ["x", "ring"])["ring"].cpu()
    p = ring.shape[1]
    nbytes = lib.hint_fcoef_workspace_bytes(n, p, k)

    def run(v, out):
        shapes._fcoef_run(v["points"], k, None, out=dict(x=out["x"], workspace=out["workspace"].view(torch.uint8)[:nbytes]))
    return _runner_case(dict(points=ring), dict(x=(n, 4 * k), workspace=(nbytes // 4 + 1,)), ("workspace",), run)


DESCRIPTORS = dict(mmd=_desc_mmd, abc=_desc_abc, corr=_desc_corr, curve=_desc_curve, hausdorff=_desc_hausdorff, plus=_desc_plus,
                   lensfit=_desc_lensfit, plusfit=_desc_plusfit, overlap=_desc_overlap, lensgen=_desc_lensgen, fcoef=_desc_fcoef)


@pytest.mark.parametrize("which", list(DESCRIPTORS))
def test_descriptors(lib, S, which):
    run_case(f"hint_{which}_run", DESCRIPTORS[which](lib), S)
    on_s = {n for n, st in lib.calls if st == S.cuda_stream}
    assert f"hint_{which}_run" in on_s, sorted(on_s)
    other = sorted({(n, hex(st)) for n, st in lib.calls if st not in (0, S.cuda_stream)})
    assert not other, other


# ---- the Python routes: twin modules, the reference on the default stream ------------------------------------------------------

def host_sync_of(name):
    """the route's ledger entry: None, or the line that synchronises the host by contract"""
    return ROUTES[name][1]


def dev_inputs(b, host):
    """{name: host tensor} -> {name: live device tensor}: staged, NaN until the refill behind the gate"""
    live = {}
    for k, v in host.items():
        t = torch.empty(v.shape, dtype=v.dtype, device=DEV)
        t.copy_(v)
        b.late += late_inputs([(t, None)])
        live[k] = t
    return live


def twins(build):
    """the same module twice from the same seed: one for the default-stream reference, one for the runs on S"""
    out = {}
    for role in ("ref", "S"):
        torch.manual_seed(1234)
        out[role] = build()
    return out


def grads_of(mod):
    return {f"grad {k}": p.grad for k, p in mod.named_parameters() if p.grad is not None}


def module_case(mods, host, run):
    """forward + backward of a module: run(module, live inputs) -> outputs; every p.grad is an output as well"""
    def make(fill, role):
        b = Build(fill)
        mod = mods[role]
        for p in mod.parameters():
            p.grad = None
        live = dev_inputs(b, host)

        def call():
            out = run(mod, {k: (v.detach().requires_grad_(True) if v.is_floating_point() else v) for k, v in live.items()})
            out.update(grads_of(mod))
            return out
        return Seq(call, b.late, b.guards)
    return make


def nll_backward(z, J, leaves):
    (0.5 * (z ** 2).sum(1) - J).mean().backward()
    return {f"g_{k}": v.grad for k, v in leaves.items() if v.grad is not None}


BLOCKS = {"wl": (6, 0, (24, 12), 100), "n3": (8, 3, (64, 32, 16), 333)}


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "rev"])
@pytest.mark.parametrize("fam", list(BLOCKS))
def test_block_module(lib, S, fam, rev):
    """HierarchicalAffineCouplingBlock: forward + backward, and rev=True + backward (hint_block_inverse_backward under autograd)"""
    import hint_amd
    d, dc, widths, B = BLOCKS[fam]
    mods = twins(lambda: hint_amd.HierarchicalAffineCouplingBlock([(d,)], dims_c=[(dc,)] if dc else [], c_internal=list(widths)).to(DEV))
    g = torch.Generator().manual_seed(5)
    host = dict(x=torch.randn(B, d, generator=g))
    if dc:
        host["c"] = torch.randn(B, dc, generator=g)

    def run(mod, v):
        (z,) = mod([v["x"]], c=[v["c"]] if dc else [], rev=rev)
        J = mod.jacobian(None)
        return dict(z=z.detach(), J=J.detach(), **nll_backward(z, J, v))
    name = f"block_{'rev' if rev else 'forward'}_{fam}"
    run_case(name, module_case(mods, host, run), S, host_sync=host_sync_of(name))
    assert {n for n, st in lib.calls if st == S.cuda_stream} >= ({"hint_block_inverse_ex", "hint_block_inverse_backward"} if rev else
                                                                 {"hint_block_forward_ex", "hint_block_backward_ex"})


def test_external_coupling(lib, S):
    import hint_amd
    D, dc, B = 12, 4, 100
    mods = twins(lambda: hint_amd.ExternalAffineCoupling([(D,)], dims_c=[(dc,)], F_args={"internal_size": 32}).to(DEV))
    g = torch.Generator().manual_seed(6)
    host = dict(x=torch.randn(B, D, generator=g), c=torch.randn(B, dc, generator=g))

    def run(mod, v):
        (z,) = mod([v["x"]], c=[v["c"]])
        J = mod.jacobian(None)
        return dict(z=z.detach(), J=J.detach(), **nll_backward(z, J, v))
    run_case("external_affine_coupling", module_case(mods, host, run), S, host_sync=host_sync_of("external_affine_coupling"))


@pytest.mark.parametrize("route", ["fused", "blockwise_reshuffle"])
def test_hint_flow(lib, S, route):
    """HintFlow on the fused route (_ChainFn: pooled chain instances per (B, stream)) and block by block with reshuffle=True"""
    import hint_amd
    B = 100

    def build():
        flow = hint_amd.HintFlow(8, 3, [64, 32, 16], reshuffle=(route != "fused")).to(DEV)
        flow.fuse_chain = route == "fused"
        return flow
    mods = twins(build)
    host = dict(x=torch.randn(B, 8, generator=torch.Generator().manual_seed(7)))

    def run(mod, v):
        z = mod(v["x"])
        J = mod.log_jacobian(run_forward=False)
        return dict(z=z.detach(), J=J.detach(), **nll_backward(z, J, v))
    run_case(f"hint_flow_{route}", module_case(mods, host, run), S, host_sync=host_sync_of(f"hint_flow_{route}"))
    on_s = {n for n, st in lib.calls if st == S.cuda_stream}
    assert on_s >= ({"hint_chain_forward", "hint_chain_backward"} if route == "fused" else {"hint_block_forward_ex"}), sorted(on_s)


def cond_model():
    import hint_amd
    cm = hint_amd.ConditionalHintFlow(12, 4, 3, 32)
    for p in cm.parameters():
        p.data = 0.07 * torch.randn_like(p)
    return cm.to(DEV)


@pytest.mark.parametrize("route", ["forward", "sample_broadcast", "sample_per_row", "x_lane"])
def test_conditional_flow(lib, S, route):
    """ConditionalHintFlow.forward + backward (twelve modules under autograd), sample_conditional with one observation and with
    one per row, x_lane_forward"""
    B = 100
    mods = twins(cond_model)
    g = torch.Generator().manual_seed(8)
    host = dict(x=torch.randn(B, 12, generator=g), y=torch.randn(1 if route == "sample_broadcast" else B, 4, generator=g))

    def run(mod, v):
        if route == "forward":
            zy, zx = mod([v["y"], v["x"]])
            J = mod.log_jacobian(run_forward=False)
            return dict(zy=zy.detach(), zx=zx.detach(), J=J.detach(), **nll_backward(torch.cat([zx, zy], 1), J, v))
        x, y = v["x"].detach(), v["y"].detach()
        out, J = mod.x_lane_forward(x, y) if route == "x_lane" else mod.sample_conditional(y, x)
        return dict(out=out, J=J)
    run_case(f"conditional_{route}", module_case(mods, host, run), S, host_sync=host_sync_of(f"conditional_{route}"))


def test_posterior_sampler_chains_are_keyed_by_stream(S):
    """white box: _PosteriorSampler._chains owns the coefficient buffer the chain reads, so two streams never share one - two
    streams get two coef buffers, and a third call on the first stream reuses the first"""
    cm = cond_model()
    ps = cm._posterior()
    B = 100                                             # (nx = 12 runs on the general kernels: the fused route)
    x, y = torch.randn(B, 12, device=DEV), torch.randn(1, 4, device=DEV)
    torch.cuda.synchronize()
    if ps._wave_local(B) or not ps.fusable:
        pytest.fail("the conditional model's x lane does not take the fused route at this batch: the test needs another shape")
    S2 = torch.cuda.Stream()
    ptrs = []
    for st in (S, S2, S):
        with torch.cuda.stream(st):
            cm.sample_conditional(y, x)
            ptrs.append(ps._chain(B, False)[1].data_ptr())
        st.synchronize()
    assert ptrs[0] != ptrs[1], "two streams share one coef buffer"
    assert ptrs[2] == ptrs[0], "the first stream's chain was not reused"
    assert all(len(k) == 3 for k in ps._chains), list(ps._chains)


def test_clamp_adam(lib, S):
    """ClampAdam.step twice on three parameters of odd sizes; the gradients arrive behind the gate"""
    import hint_amd
    shapes_ = [(1001,), (37, 5), (4,)]
    g = torch.Generator().manual_seed(9)
    p0 = [torch.randn(s, generator=g) for s in shapes_]
    host = {f"g{i}": torch.randn(s, generator=g) * 3 for i, s in enumerate(shapes_)}

    def build():
        params = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
        for p in params:
            p.grad = torch.zeros_like(p)
        opt = hint_amd.ClampAdam(params, lr=1e-2, betas=(0.9, 0.95), eps=1e-4, weight_decay=1e-5, grad_clamp=5.0)
        opt.step()                                   # builds the segment table (a synchronous upload: not what is under test)
        return SimpleNamespace(params=params, opt=opt)
    mods = {role: build() for role in ("ref", "S")}

    def make(fill, role):
        b = Build(fill)
        m = mods[role]
        with torch.no_grad():
            for p, v in zip(m.params, p0):
                p.copy_(v)
                st = m.opt.state[p]
                st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
        for rec in m.opt._groups:
            rec.steps.zero_()
            for part in rec.parts:
                part.step = 0
        for i, p in enumerate(m.params):             # the live gradients: staged, NaN until the refill
            p.grad.copy_(host[f"g{i}"])
            b.late += late_inputs([(p.grad, None)])

        def call():
            m.opt.step()
            m.opt.step()
            out = {f"p{i}": p.detach() for i, p in enumerate(m.params)}
            out.update({f"m{i}": m.opt.state[p]["exp_avg"] for i, p in enumerate(m.params)})
            out.update({f"v{i}": m.opt.state[p]["exp_avg_sq"] for i, p in enumerate(m.params)})
            return out
        return Seq(call, b.late, b.guards)
    run_case("clamp_adam_step", make, S, host_sync=host_sync_of("clamp_adam_step"))
    assert "hint_adam_multi_step" in {n for n, st in lib.calls if st == S.cuda_stream}


# ---- trainers: built and first stepped inside the S context; every run starts from the same restored state --------------------

STATE = ("P", "M", "V", "G", "rng_state", "opt_state")


def snap(tr):
    return SimpleNamespace(t=[getattr(tr, k).clone() for k in STATE], step=tr.step_count, noise=tr.noise, lr=tr._lr)


def restore(tr, s):
    for k, v in zip(STATE, s.t):
        getattr(tr, k).copy_(v)
    tr.step_count, tr.noise, tr._lr = s.step, s.noise, s.lr          # (opt_state[0], the device's copy of lr, is restored above)
    for e in tr.engines:
        e._pack_key = None


def trainer_twins(build, first, S):
    """the reference trainer on the default stream, the other built and first stepped with S current"""
    out = {}
    for role in ("ref", "S"):
        torch.manual_seed(4321)
        if role == "S":
            with torch.cuda.stream(S):
                tr = build()
                first(tr)
            S.synchronize()
        else:
            tr = build()
            first(tr)
        torch.cuda.synchronize()
        out[role] = SimpleNamespace(tr=tr, snap=snap(tr))
    return out


def trainer_case(trs, host, steps):
    """steps(trainer, live inputs, record): record(tag, loss pair) keeps the losses (atomic sums: 1e-6) and a copy of P"""
    def make(fill, role):
        b = Build(fill)
        t = trs[role]
        restore(t.tr, t.snap)
        live = dev_inputs(b, host)

        def call():
            out = {}

            def record(tag, pair):
                l0, l1 = pair
                out[f"loss {tag}"] = torch.stack([l0, l1])
                out[f"P {tag}"] = t.tr.P.clone()
            steps(t.tr, live, record)
            out["M"], out["V"] = t.tr.M.clone(), t.tr.V.clone()
            return out
        return Seq(call, b.late, b.guards, loose=[f"loss {i}" for i in range(8)])
    return make


def small_flow():
    import hint_amd
    return hint_amd.HintFlow(8, 3, [64, 32, 16]).to(DEV)


@pytest.mark.parametrize("route", ["eager", "graph", "graph_noisy", "step_many"])
def test_flow_trainer(lib, S, route):
    """FlowTrainer.step eager (two noise-free steps - the second at another learning rate - then a noisy one), captured (a replay per step: two noise-free steps; one
    noisy step of a trainer captured with noise) and step_many (three iterations in one replay)"""
    import hint_amd
    B = 100
    g = torch.Generator().manual_seed(10)
    host = {f"x{i}": torch.randn(B, 8, generator=g) for i in range(3)}
    xs0 = torch.stack([host[f"x{i}"] for i in range(3)]).to(DEV)
    noise = 0.25 if route == "graph_noisy" else 0.0
    build = lambda: hint_amd.FlowTrainer(small_flow(), noise=noise, use_graph=route != "eager", seed=77)       # noqa: E731
    first = (lambda tr: tr.step_many(xs0)) if route == "step_many" else (lambda tr: tuple(tr.step(xs0[0])))
    trs = trainer_twins(build, first, S)

    def steps(tr, v, record):
        if route == "step_many":
            tr.step_many(torch.stack([v["x0"], v["x1"], v["x2"]]))
            ls = tr.step_losses()
            record(0, (ls[:, 0], ls[:, 1]))
            return
        record(0, tr.step(v["x0"]))
        if route != "graph_noisy":
            tr.lr = 2e-4                                 # a schedule's statement: the device's copy is set without a host copy
            record(1, tr.step(v["x1"]))
        if route == "eager":
            tr.noise = 0.25
            record(2, tr.step(v["x2"]))
    run_case(f"flow_trainer_{route}", trainer_case(trs, host, steps), S, host_sync=host_sync_of(f"flow_trainer_{route}"))
    if route == "eager":
        assert {n for n, st in lib.calls if st == S.cuda_stream} >= {"hint_chain_forward_noisy", "hint_pack_group_run_ex", "hint_adam_step"}


@pytest.mark.parametrize("route", ["eager", "eager_noise_switch", "graph"])
def test_conditional_trainer(lib, S, route):
    """ConditionalFlowTrainer.step eager and captured, two steps each; eager_noise_switch turns `noise` off between the steps:
    the re-commit of hac_x_0's gathered chain, which synchronises the stream by design (host_sync in the ledger)"""
    import hint_amd
    B = 100
    g = torch.Generator().manual_seed(11)
    host = dict(x0=torch.randn(B, 12, generator=g), y0=torch.randn(B, 4, generator=g), x1=torch.randn(B, 12, generator=g),
                y1=torch.randn(B, 4, generator=g))
    x0, y0 = host["x0"].to(DEV), host["y0"].to(DEV)
    build = lambda: hint_amd.ConditionalFlowTrainer(cond_model(), use_graph=route == "graph", seed=1234)       # noqa: E731
    trs = trainer_twins(build, lambda tr: tuple(tr.step(x0, y0)), S)

    def steps(tr, v, record):
        record(0, tr.step(v["x0"], v["y0"]))
        if route == "eager_noise_switch":
            tr.noise = 0.0
        record(1, tr.step(v["x1"], v["y1"]))
    run_case(f"conditional_trainer_{route}", trainer_case(trs, host, steps), S, host_sync=host_sync_of(f"conditional_trainer_{route}"))


# ---- the wrappers of metrics.py, abc.py, curves.py and shapes.py, each once at its smallest test shape ------------------------

def _wrap_metrics(v, put, extra):
    import hint_amd
    from hint_amd import metrics
    put("multi_mmd", hint_amd.multi_mmd(v["a"], v["bset"]))
    put("MultiMMD", metrics.MultiMMD(v["bset"])(v["a"]))
    put("corrcoef", metrics.corrcoef(v["a"]))
    put("corr_mse", metrics.corr_mse(v["bset"], extra["tcorr"]))
    put("CorrelationTarget", metrics.CorrelationTarget(extra["tcorr"])(v["bset"]))


def _wrap_abc(v, put, extra):
    import hint_amd
    put("nearest_rows", hint_amd.nearest_rows(v["yobs"], v["tgt"], 17))
    put("quantile_abc", hint_amd.quantile_abc(v["xrows"], v["yobs"], v["tgt"], n=20))


def _wrap_curves_distances(v, put, extra):
    import hint_amd
    x, pr, pp, lp, px = v["coef"], v["proto"], v["pparams"], v["lparams"], v["pcoef"]
    put("curve_features", hint_amd.curve_features(x))
    put("lens_forward_process", hint_amd.lens_forward_process(x, 0.05, eps=v["eps"]))
    put("target_distances", hint_amd.target_distances(x, v["ytarget"], 0.05, eps=v["eps"]))
    put("mean_target_distance", hint_amd.mean_target_distance(x, v["ytarget"], 0.05, eps=v["eps"]))
    put("trace_fourier_curves", hint_amd.trace_fourier_curves(x, 100))
    put("hausdorff_distances", hint_amd.hausdorff_distances(x, pr, lp, n_points=100))
    put("chamfer_distances", hint_amd.chamfer_distances(x, pr, lp, n_points=100))
    put("lens_fit_loss", hint_amd.lens_fit_loss(x, pr, lp))
    put("plus_segments", hint_amd.plus_segments(pp))
    put("plus_outline_counts", hint_amd.plus_outline_counts(pp))
    put("plus_fit_terms", hint_amd.plus_fit_terms(px, pp))
    put("plus_fit_loss", hint_amd.plus_fit_loss(px, pp))
    put("plus_hausdorff_distances", hint_amd.plus_hausdorff_distances(px, pp, n_points=100))
    put("polygon_overlap", hint_amd.polygon_overlap(x, pr, lp))
    put("lens_iou_dice", hint_amd.lens_iou_dice(x, pr, lp))
    put("plus_iou_dice", hint_amd.plus_iou_dice(px, pp))


def _wrap_curves_fits(v, put, extra):
    import hint_amd
    x, pr, pp, lp, px = v["coef"], v["proto"], v["pparams"], v["lparams"], v["pcoef"]
    put("lens_fit_grad", hint_amd.lens_fit_grad(x, pr, lp))
    put("lens_fit_starts", hint_amd.lens_fit_starts(x))
    put("fit_lens_shapes", hint_amd.fit_lens_shapes(x, pr, n_steps=3, return_all=True))
    put("plus_fit_grad", hint_amd.plus_fit_grad(px, pp))
    put("plus_dominant_angle", hint_amd.plus_dominant_angle(px))
    put("plus_fit_starts", hint_amd.plus_fit_starts(px))
    put("fit_plus_shapes", hint_amd.fit_plus_shapes(px, n_steps=3, return_all=True))
    put("lens_shape_scores", tuple(hint_amd.lens_shape_scores(x, pr)))
    put("plus_shape_scores", tuple(hint_amd.plus_shape_scores(px)))


def _wrap_shapes(v, put, extra):
    import hint_amd
    N = 37
    prior = hint_amd.sample_lens_prior(N, SEED, device=DEV, return_ring=True)
    put("sample_lens_prior", prior)
    put("sample_lens_joint", hint_amd.sample_lens_joint(N, SEED, 0.05, device=DEV, return_eps=True))
    put("lens_draws", hint_amd.lens_draws(N, SEED, device=DEV))
    put("fourier_coeffs", hint_amd.fourier_coeffs(prior[1], 5))


def _wrap_shapes_checked_rows(v, put, extra):
    """the paths that take rows from the caller refuse bad ones, which reads one number back (shapes._rejected)"""
    import hint_amd
    ring, counts = hint_amd.lens_rings(v["draws"])
    put("lens_rings", (ring, counts))
    put("sample_lens_prior(draws)", hint_amd.sample_lens_prior(v["draws"].shape[0], 0, draws=v["draws"]))
    put("fourier_coeffs(counts)", hint_amd.fourier_coeffs(ring, 5, counts))


WRAPPERS = dict(metrics=_wrap_metrics, abc=_wrap_abc, curves_distances=_wrap_curves_distances, curves_fits=_wrap_curves_fits,
                shapes=_wrap_shapes, shapes_checked_rows=_wrap_shapes_checked_rows)


@pytest.mark.parametrize("group", list(WRAPPERS))
def test_wrappers(lib, S, group):
    import curve_oracle as co
    import hint_amd
    import lensfit_oracle as lo
    import plus_oracle as po
    from hint_amd import metrics
    N, K = 5, 5
    g = torch.Generator().manual_seed(12)
    host = dict(metrics=lambda: dict(a=torch.randn(67, 7, generator=g), bset=0.3 + 1.2 * torch.randn(131, 7, generator=g)),
                abc=lambda: dict(yobs=torch.randn(300, 4, generator=g), tgt=torch.randn(4, generator=g),
                                 xrows=torch.randn(300, 3, generator=g)),
                shapes=lambda: {},
                shapes_checked_rows=lambda: dict(draws=hint_amd.lens_draws(37, SEED, device=DEV).cpu()))
    curves_in = lambda: dict(coef=torch.from_numpy(lo.lens_rows(1101, N)), proto=torch.from_numpy(lo.lens_prototype(130)),     # noqa: E731
                             lparams=torch.from_numpy(lo.golden_grad_params(1102, N)),
                             pcoef=torch.from_numpy((co.gauss(72, N, K) * np.float32(3)).astype(np.float32)),
                             pparams=torch.from_numpy(po.draw_params(71, N, (0.02,))), eps=torch.randn(N, 2, generator=g),
                             ytarget=torch.tensor([0.5, -0.25]))
    host = host.get(group, curves_in)()
    extra = {}
    if group == "metrics":
        extra["tcorr"] = metrics.corrcoef(host["bset"].to(DEV)).clone()
    torch.cuda.synchronize()
    fn = WRAPPERS[group]

    def make(fill, role):
        b = Build(fill)
        v = dev_inputs(b, host)

        def call():
            out = {}

            def put(name, res):
                for i, t in enumerate(res if isinstance(res, (tuple, list)) else [res]):
                    if isinstance(t, torch.Tensor):
                        out[f"{name}.{i}"] = t
                    elif isinstance(t, dict):
                        out.update({f"{name}.{i}.{k}": u for k, u in t.items()})
            fn(v, put, extra)
            return out
        return Seq(call, b.late, b.guards)
    # (NaN and inf are legitimate values of some of these columns: the reference run's finiteness is not asserted here)
    run_case(f"wrappers_{group}", make, S, host_sync=host_sync_of(f"wrappers_{group}"), finite=False)
    want = dict(metrics={"hint_mmd_run", "hint_corr_run"}, abc={"hint_abc_run"},
                curves_distances={"hint_curve_run", "hint_hausdorff_run", "hint_plus_run", "hint_overlap_run"},
                curves_fits={"hint_lensfit_run", "hint_plusfit_run"}, shapes={"hint_lensgen_run", "hint_fcoef_run"},
                shapes_checked_rows={"hint_lensgen_run", "hint_fcoef_run"})[group]
    on_s = {n for n, st in lib.calls if st == S.cuda_stream}
    assert want <= on_s, sorted(want - on_s)


# ---- cross-stream reuse (un-gated, bit-exact) -------------------------------------------------------------------------------------

def fwd_bwd(mod, x_dev, flow):
    for p in mod.parameters():
        p.grad = None
    x = x_dev.detach().requires_grad_(True)
    if flow:
        z = mod(x)
        J = mod.log_jacobian(run_forward=False)
    else:
        (z,) = mod([x])
        J = mod.jacobian(None)
    (0.5 * (z ** 2).sum(1) - J).mean().backward()
    return dict(z=z.detach(), J=J.detach(), gx=x.grad, **grads_of(mod))


@pytest.mark.parametrize("what", ["block", "flow"])
def test_one_module_on_five_stream_keys(lib, S, what):
    """one block / one HintFlow on the default stream, then S1 .. S4, then the default stream again, each use ordered behind the
    previous one with wait_stream: five (B, stream) keys, so hint.py's tape and workspace pools and flow.py's acquire go through
    their eviction branches; every use gives the first use's bits"""
    import hint_amd
    torch.manual_seed(21)
    mod = small_flow() if what == "flow" else hint_amd.HierarchicalAffineCouplingBlock([(8,)], c_internal=[64, 32, 16]).to(DEV)
    x = torch.randn(100, 8, device=DEV)
    torch.cuda.synchronize()
    streams = [torch.cuda.default_stream(), S] + [torch.cuda.Stream() for _ in range(3)] + [torch.cuda.default_stream()]
    first, prev = None, None
    for i, st in enumerate(streams):
        if prev is not None:
            st.wait_stream(prev)
        with torch.cuda.stream(st):
            out = fwd_bwd(mod, x, what == "flow")
        st.synchronize()
        got = sg.host(out)
        if first is None:
            first = got
            assert all(bool(torch.isfinite(v).all()) for v in first.values())
        sg.compare(f"{what}: use {i} on stream {st.cuda_stream:#x}", got, first)
        prev = st
    keys = set(mod._runner._pool) if what == "flow" else set(mod.tree._engine._ws)
    assert len({k[1] for k in keys}) < 5, "five stream keys did not reach the eviction branch"
    torch.cuda.synchronize()


def test_backward_called_on_another_stream(lib, S):
    """a forward on S1 whose loss.backward() is called while S2 is current gives the default stream's gradients"""
    import hint_amd
    torch.manual_seed(22)
    mod = hint_amd.HierarchicalAffineCouplingBlock([(8,)], c_internal=[64, 32, 16]).to(DEV)
    x_dev = torch.randn(100, 8, device=DEV)
    ref = sg.host(fwd_bwd(mod, x_dev, False))
    torch.cuda.synchronize()
    S2 = torch.cuda.Stream()
    for p in mod.parameters():
        p.grad = None
    with torch.cuda.stream(S):
        x = x_dev.detach().requires_grad_(True)
        (z,) = mod([x])
        J = mod.jacobian(None)
        loss = (0.5 * (z ** 2).sum(1) - J).mean()
    with torch.cuda.stream(S2):
        S2.wait_stream(S)
        loss.backward()
    S2.synchronize(); S.synchronize()
    torch.cuda.synchronize()
    sg.compare("backward on another stream", sg.host(dict(z=z.detach(), J=J.detach(), gx=x.grad, **grads_of(mod))), ref)


def test_graph_captured_under_one_stream_replayed_under_another(lib, S):
    """a FlowTrainer whose step is captured with S current and replayed with S2 current (after S2.wait_stream(S)) gives the bits
    of the same steps replayed on the default stream"""
    import hint_amd
    g = torch.Generator().manual_seed(23)
    xs = [torch.randn(100, 8, generator=g).to(DEV) for _ in range(3)]
    torch.cuda.synchronize()

    def run(capture_stream, replay_stream):
        torch.manual_seed(24)
        out = {}
        with torch.cuda.stream(capture_stream):
            tr = hint_amd.FlowTrainer(small_flow(), noise=0.0, use_graph=True, seed=5)
            out["loss 0"] = torch.stack(tuple(tr.step(xs[0])))
        replay_stream.wait_stream(capture_stream)
        with torch.cuda.stream(replay_stream):
            for i in (1, 2):
                out[f"loss {i}"] = torch.stack(tuple(tr.step(xs[i])))
                out[f"P {i}"] = tr.P.clone()
        replay_stream.synchronize()
        torch.cuda.synchronize()
        return sg.host(out)
    ref = run(torch.cuda.default_stream(), torch.cuda.default_stream())
    S2 = torch.cuda.Stream()
    got = run(S, S2)
    sg.compare("graph captured under S, replayed under S2", got, ref, loose=("loss 0", "loss 1", "loss 2"))
