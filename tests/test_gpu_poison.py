"""Every C entry point that writes device memory, on poisoned scratch and guard-banded buffers.

The library's own callers hand it `torch.empty` memory, which in a long process holds whatever the caching allocator had in it
last.  Here outputs, tapes, workspaces, gradient arenas, the packed weights (before the pack) and the gaps of the flat
parameter buffers are filled with zeros (clean), with a NaN bit pattern or with finite junk, every buffer sits between two
64 KiB NaN guards (tests/guarded.py), and:
  A. every ledger case (tests/instance_cases.py) at its own batch size, at B = 1 and at a ragged batch whose last part-B split
     is partial gives bit-identical outputs under every fill and payload alignment, leaves every guard and const input as it
     was, and (NaN fill, cotangents on the first and last 300 rows) matches the float64 oracle;
  B. the memory promises of include/hint_amd.h hold: accumulation, B = 0, x aliasing z, the fused Adam's untouched arenas,
     loss_acc, the pack prologue, the noisy forwards, the inverse's backward, the external couplings and the Adam steps.
  C. the product's eager paths (trainers, module route, sampler) on torch's caching allocator filled with NaN give the same
     bits as on one filled with zeros.
Graph-captured steps allocate from a private memory pool that none of this reaches; their kernels are the ones part A runs.

Audit (from the code, before the first GPU run):
  - No word of a poisoned buffer becomes an address, a row or tile index, a loop bound or a barrier count.  Those come from
    the plan's device tables (meta, records, part-B jobs, the `real` map, twmap), the chain table and the launch arguments,
    none of which is poisoned.  split_workspace / bind_tape (hint_abi.cpp) only offset the caller's pointers by sizes of the
    plan.  Slabs, g1 / g2, g_s | g_t, the tape's lanes, s values and activations are operands of arithmetic; the sign bytes are
    loaded as mask bits (hint_rows.hpp); the reduction (hint_wreduce_kernel) selects real elements by the `real` map.
  - Not poisoned: rng_state, opt_state[0..2], plans, chain tables, and the inputs (x, c, z of the inverse, g_z, g_J, perm, the
    parameters themselves): they are guarded and must come back bit for bit.
  - Alignment: the "offset" runs put every row tensor (x, c, z, J, g_x, g_c, g_z, g_J), the workspaces and g_params 16 bytes
    past a 256-byte boundary.  The header promises 16 bytes for workspace and g_params and the library checks it; the row
    tensors are read and written as single floats (load_tile / store_tile in hint_device.hpp) and through buffer resources
    with 4-byte loads (rows_rsrc in hint_wgrad.hip).  The tape, the packed weights and perm stay at 256 bytes: the header
    promises no alignment for them and every caller in the library passes a whole torch allocation.
  - The packed buffer is poisoned before the pack like every other buffer; the pack writes all of it (check_pack_writes_all).
Part C runs the product's own Python paths on a caching allocator whose free blocks hold NaN (test_product_paths_on_nan_cache)."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

from guarded import NAN_BITS, Guarded, bits_equal
from instance_cases import CASES, knob_env, multi_pass_b, plan_dispatch
from oracle import hint_oracle as orc
from poison_cases import DEV, Rig, check, stream
from test_gpu_instances import KINK, Spy, check_fwd, check_grads

pytestmark = pytest.mark.gpu
RUNS = (("nan", 256), ("junk", 256), ("junk", 16))     # compared with ("zero", 256)
EDGE = 300                                             # rows with cotangents at each end of the batch (oracle run)


@pytest.fixture
def lib():
    from hint_amd import _lib
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return _lib.load()


def partial_split_b(lib, plan, B0):
    """a ragged batch (B % 16 != 0) whose last part-B split holds fewer rows than the others (dw_splits / dw_rows)"""
    for k in range(400):
        B = max(B0 // 2, 21) + 37 * k
        disp = plan_dispatch(lib, plan, B)
        last = B - (disp["dw_splits"] - 1) * disp["dw_rows"]
        if B % 16 and 0 < last < disp["dw_rows"] and disp["dw_splits"] > 1:
            return B
    raise AssertionError("no batch with a partial last split")


def check_pack_writes_all(lib, rig, i=0):
    """the pack writes every float of the packed buffer (hint_plan_packed_floats): fragment tiles, the vector blobs with their
    padding, the biases and the slack behind them - packing into a NaN-filled and into a junk-filled buffer gives the same bits"""
    n = lib.hint_plan_packed_floats(rig.plan)
    params = rig.flat_params(i, "zero")
    a, b = Guarded(n, fill="nan"), Guarded(n, fill="junk", seed=5)
    for g in (a, b):
        check(lib.hint_block_pack(rig.plan, params.ptr, g.ptr, stream()), "hint_block_pack")
    torch.cuda.synchronize()
    a.check_guards("pack"); b.check_guards("pack")
    unwritten = int((a.words != b.words).sum())
    assert unwritten == 0, f"{rig.case.name}: the pack leaves {unwritten} of {n} packed floats unwritten"


def compare(name, got, ref):
    for k in ("z", "J", "xi", "Ji", "gx", "gc"):
        if ref[k] is not None:
            assert bits_equal(got[k], ref[k]), f"{name}: {k} differs from the clean run"
    for i, (a, b) in enumerate(zip(got["gp"], ref["gp"])):
        assert bits_equal(a, b), f"{name}: g_params of block {i} differs from the clean run ({int((a.view(torch.int32) != b.view(torch.int32)).sum())} words)"
    for i, (a, b) in enumerate(zip(got["packed"], ref["packed"])):
        assert bits_equal(a, b), f"{name}: packed weights of block {i} differ"


def oracle_rows(rig, B, rows):
    """float64 oracle on the given rows: (kept rows mask, reference dict with full-size gx / gc, cotangents on the host)"""
    case = rig.case
    x, c, zi, gz, gJ = rig.inputs(B)
    xs = x[rows].double().requires_grad_(True)
    cs = [c[rows].double().requires_grad_(True)] if case.dc else []
    if case.entry == "chain":
        for P in rig.ref.params:
            for p in P.values():
                p.grad = None
                p.requires_grad_(True)
        with Spy(len(rows)) as spy:
            z64, J64 = rig.ref.forward(xs, tuple(cs))
        Pd = rig.ref.params
    else:
        Pd = [{k: v.double().requires_grad_(True) for k, v in rig.P[0].items()}]
        with Spy(len(rows)) as spy:
            z64, J64 = orc.block_apply(rig.nodes, Pd[0], xs, cs, rev=False)
    keep = spy.kink > KINK
    gzs, gJs = gz[rows] * keep[:, None], gJ[rows] * keep
    ((z64 * gzs.double()).sum() + (J64 * gJs.double()).sum()).backward()
    with torch.no_grad():
        if case.entry == "chain":
            xi64, Ji64 = rig.ref.inverse(zi[rows].double(), tuple(t.detach() for t in cs))
        else:
            xi64, Ji64 = orc.block_apply(rig.nodes, {k: v.detach() for k, v in Pd[0].items()}, zi[rows].double(),
                                         [t.detach() for t in cs], rev=True)
    gz_full, gJ_full = torch.zeros_like(gz), torch.zeros_like(gJ)
    gz_full[rows], gJ_full[rows] = gzs, gJs
    gx = torch.zeros(B, case.d, dtype=torch.float64)
    gx[rows] = xs.grad
    gc = None
    if case.dc:
        gc = torch.zeros(B, case.dc, dtype=torch.float64)
        gc[rows] = cs[0].grad
    ref = dict(z=z64.detach(), J=J64.detach(), xi=xi64, Ji=Ji64, gx=gx, gc=gc,
               gw={(i, k): v.grad for i, P in enumerate(Pd) for k, v in P.items()})
    return keep, ref, (x, c, zi, gz_full, gJ_full)


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.timeout(900)) for c in CASES], ids=[c.name for c in CASES])
def test_ledger_under_poison(case, lib, monkeypatch):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    knob_env(monkeypatch, lib, case.knobs)
    try:
        rig = Rig(case, lib)
        check_pack_writes_all(lib, rig)
        B0 = case.B(cu)
        for B in (B0, 1, partial_split_b(lib, rig.plan, B0)):
            name = f"{case.name} B={B}"
            host = rig.inputs(B)
            clean = rig.run(B, "zero", 256, host)
            for k, v in clean.items():
                if isinstance(v, torch.Tensor):
                    assert torch.isfinite(v).all(), f"{name}: clean run: {k} not finite"
            for j, (fill, align) in enumerate(RUNS):
                got = rig.run(B, fill, align, host, seed=1000 * (j + 1))
                compare(f"{name} {fill}/{align}", got, clean)
            # the oracle on the NaN-filled run: cotangents on the first and last EDGE rows only (the dispatch is B's)
            rows = torch.unique(torch.cat([torch.arange(min(EDGE, B)), torch.arange(max(B - EDGE, 0), B)]))
            keep, ref, host = oracle_rows(rig, B, rows)
            got = rig.run(B, "nan", 256, host, seed=7)
            for k in ("z", "J"):
                check_fwd(f"{name} {k}", got[k][rows], ref[k])
            check_fwd(f"{name} inverse x", got["xi"][rows], ref["xi"])
            check_fwd(f"{name} inverse J", got["Ji"][rows], ref["Ji"])
            gw = {(i, n): got["gp"][i][off:off + cnt].view(rig.P[i][n].shape)
                  for i in range(rig.n_blocks) for n, off, cnt in rig.layout}
            check_grads(name, got["gx"], got["gc"], gw, ref)
            dropped = len(rows) - int(keep.sum())
            assert dropped <= (case.kink_cap + 0.05) * len(rows), f"{name}: {dropped} of {len(rows)} rows next to a ReLU kink"
    finally:
        monkeypatch.undo()
        lib.hint_debug_reload_knobs()


# ---- B: the header's memory promises ----------------------------------------------------------------------------------------

def contract_case(n_blocks=3, B=None):
    """a conditional tree on the general kernels (hint_bwd_kernel_n3), as a chain of n_blocks with fixed permutations"""
    return SimpleNamespace(name="contract", entry="chain", d=8, dc=3, widths=(64, 32, 16), scale=0.05, big_s=0.0,
                           n_blocks=n_blocks, knobs={}, B=lambda cu: B if B else 16 * cu + 9)


class ChainBufs:
    """a training chain of a Rig on guarded buffers: params (gaps filled), packed, tapes, workspaces, g_params"""

    def __init__(self, rig, B, fill, align=256, seed=0, gp_fill=None, tape=True, perms=None, param_ptrs=None, commit=True):
        lib, plan = rig.lib, rig.plan
        self.rig, self.B = rig, B
        tape_n, ws_n = rig.sizes(B)
        nb = rig.n_blocks
        self.params = [rig.flat_params(i, fill, seed) for i in range(nb)] if param_ptrs is None else []
        pp = [g.ptr for g in self.params] if param_ptrs is None else param_ptrs
        self.packed = [Guarded(lib.hint_plan_packed_floats(plan), fill=fill, seed=seed + 50 + i) for i in range(nb)]
        for i in range(nb):
            check(lib.hint_block_pack(plan, pp[i], self.packed[i].ptr, stream()), "hint_block_pack")
        perms = rig.perms if perms is None else perms
        self.perms = [None if p is None else Guarded(p.numel()).set(p) for p in perms]
        self.tapes = [Guarded(tape_n, fill=fill, seed=seed + 60 + i) for i in range(nb)] if tape else [None] * nb
        self.ws_n = ws_n
        self.wss = [Guarded(ws_n, fill=fill, align=align, seed=seed + 70 + i) for i in range(nb)] if tape else [None] * nb
        self.gps = [Guarded(rig.total, fill=gp_fill or fill, align=align, seed=seed + 80 + i) for i in range(nb)] if tape else [None] * nb
        self.ch = C.c_void_p()
        check(lib.hint_chain_create(plan, nb, B, C.byref(self.ch)), "hint_chain_create")
        p = lambda g: None if g is None else g.ptr                                        # noqa: E731
        for i in range(nb):
            check(lib.hint_chain_set_block(self.ch, i, pp[i], self.packed[i].ptr, p(self.perms[i]), p(self.tapes[i]),
                                           p(self.wss[i]), 4 * ws_n if tape else 0, p(self.gps[i])), "hint_chain_set_block")
        if commit:
            check(lib.hint_chain_commit(self.ch), "hint_chain_commit")

    def guards(self, what):
        for k in ("params", "packed", "perms", "tapes", "wss", "gps"):
            for i, g in enumerate(getattr(self, k)):
                if g is not None:
                    g.check_guards(f"{what}: {k}[{i}]")

    def close(self):
        self.rig.lib.hint_chain_destroy(self.ch)


def rows_in(rig, B, seed=11, align=256):
    x, c, zi, gz, gJ = rig.inputs(B, seed)
    G = lambda t: None if t is None else Guarded(t.numel(), align=align).set(t)        # noqa: E731
    return SimpleNamespace(x=G(x), c=G(c), zi=G(zi), gz=G(gz), gJ=G(gJ), host=(x, c, zi, gz, gJ))


def ptr(g):
    return None if g is None else g.ptr


def ulp_close(got, ref_a, ref_b, what):
    """got == ref_a + ref_b within 2 ulp of max(|ref_a|, |ref_b|)"""
    exp = ref_a.double() + ref_b.double()
    mag = torch.maximum(ref_a.abs(), ref_b.abs()).double()
    ulp = torch.where(mag > 0, torch.pow(2.0, torch.floor(torch.log2(mag.clamp(min=1e-38))) - 23), torch.full_like(mag, 1e-45))
    bad = int(((got.double() - exp).abs() > 2 * ulp).sum())
    assert bad == 0, f"{what}: {bad} elements are not R + gradient within 2 ulp"


def gap_mask(rig):
    m = torch.ones(rig.total, dtype=torch.bool)
    for off, n in rig.covered():
        m[off:off + n] = False
    return m


def test_accumulate(lib):
    """accumulate != 0 adds to g_params: R + clean within 2 ulp, the padding keeps R bit for bit, blocks outside a
    hint_chain_wgrad_range keep R; accumulate = 0 leaves the padding exactly zero"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    rig = Rig(contract_case(3), lib)
    B = 16 * cu + 9
    gap = gap_mask(rig)
    inp = rows_in(rig, B)
    nb = rig.n_blocks
    R = [torch.empty(rig.total, device=DEV).copy_(Guarded(rig.total, fill="junk", seed=300 + i).t).cpu() for i in range(nb)]
    # block entry: hint_block_backward on block 0's parameters
    for acc in (0, 1):
        cb = ChainBufs(rig, B, "nan", gp_fill="nan")
        clean = ChainBufs(rig, B, "zero")
        for bufs in (clean, cb):
            z, J = Guarded(B * rig.case.d), Guarded(B)
            gx, gc = Guarded(B * rig.case.d, fill="nan"), Guarded(B * rig.case.dc, fill="nan")
            if bufs is cb and acc:
                bufs.gps[0].set(R[0])
            check(lib.hint_block_forward(rig.plan, bufs.params[0].ptr, bufs.packed[0].ptr, inp.x.ptr, inp.c.ptr, z.ptr, J.ptr,
                                         bufs.tapes[0].ptr, B, stream()), "hint_block_forward")
            check(lib.hint_block_backward(rig.plan, bufs.params[0].ptr, bufs.packed[0].ptr, inp.x.ptr, bufs.tapes[0].ptr, inp.c.ptr,
                                          inp.gz.ptr, inp.gJ.ptr, gx.ptr, gc.ptr, bufs.gps[0].ptr, acc if bufs is cb else 0,
                                          bufs.wss[0].ptr, 4 * bufs.ws_n, B, stream()), "hint_block_backward")
        torch.cuda.synchronize()
        g0, got = clean.gps[0].t.cpu(), cb.gps[0].t.cpu()
        if acc:
            ulp_close(got[~gap], R[0][~gap], g0[~gap], "hint_block_backward accumulate")
            assert bits_equal(got[gap], R[0][gap]), "hint_block_backward accumulate: padding changed"
        else:
            assert bits_equal(got, g0), "hint_block_backward accumulate=0: differs from the clean run"
            assert bool((got[gap] == 0).all()), "hint_block_backward accumulate=0: padding not zero"
        cb.guards("hint_block_backward"); cb.close(); clean.close()

    # chain entries: the whole backward, the two parts, and part B of the inner block only
    def chain_run(bufs, mode, acc):
        gx, gc = Guarded(B * rig.case.d, fill="nan"), Guarded(B * rig.case.dc, fill="nan")
        z, J = Guarded(B * rig.case.d, fill="nan"), Guarded(B, fill="nan")
        check(lib.hint_chain_forward(bufs.ch, inp.x.ptr, inp.c.ptr, z.ptr, J.ptr, None, None, stream()), "hint_chain_forward")
        if mode == "backward":
            check(lib.hint_chain_backward(bufs.ch, inp.x.ptr, inp.c.ptr, inp.gz.ptr, inp.gJ.ptr, gx.ptr, gc.ptr, 1.0, 0.0, acc,
                                          stream()), "hint_chain_backward")
        else:
            check(lib.hint_chain_backward_parts(bufs.ch, inp.x.ptr, inp.c.ptr, inp.gz.ptr, inp.gJ.ptr, gx.ptr, gc.ptr, 1.0, 0.0,
                                                acc, 1, stream()), "hint_chain_backward_parts")
            if mode == "parts":
                check(lib.hint_chain_backward_parts(bufs.ch, inp.x.ptr, inp.c.ptr, None, None, None, None, 1.0, 0.0, acc, 2,
                                                    stream()), "hint_chain_backward_parts")
            else:
                check(lib.hint_chain_wgrad_range(bufs.ch, inp.x.ptr, inp.c.ptr, acc, 1, 2, stream()), "hint_chain_wgrad_range")
        torch.cuda.synchronize()
        for g in (gx, gc, z, J):
            g.check_guards(f"{mode}: row outputs")
        return [g.t.cpu() for g in bufs.gps]

    clean = ChainBufs(rig, B, "zero")
    g0 = chain_run(clean, "backward", 0)
    clean.close()
    for mode in ("backward", "parts", "range"):
        for acc in (0, 1):
            cb = ChainBufs(rig, B, "nan", align=16)
            if acc:
                for i in range(nb):
                    cb.gps[i].set(R[i])
            got = chain_run(cb, mode, acc)
            cb.guards(f"{mode} accumulate={acc}")
            for i in range(nb):
                what = f"{mode} accumulate={acc} block {i}"
                if mode == "range" and i != 1:
                    if acc:
                        assert bits_equal(got[i], R[i]), f"{what}: outside the range, g_params changed"
                    else:
                        assert bool(torch.isnan(got[i]).all()), f"{what}: outside the range, g_params was written"
                    continue
                if acc:
                    ulp_close(got[i][~gap], R[i][~gap], g0[i][~gap], what)
                    assert bits_equal(got[i][gap], R[i][gap]), f"{what}: padding changed"
                else:
                    assert bits_equal(got[i], g0[i]), f"{what}: differs from the clean run"
                    assert bool((got[i][gap] == 0).all()), f"{what}: padding not zero"
            cb.close()


def test_batch_zero(lib):
    """B = 0 changes no payload or guard byte of any entry point that takes B - except g_params, zeroed when accumulate = 0"""
    rig = Rig(contract_case(1), lib)
    plan, d = rig.plan, rig.case.d
    bufs = ChainBufs(rig, 16, "nan")
    st = stream()
    names = ("x", "c", "z", "J", "tape", "perm", "J_in", "loss", "xn", "gx", "gc", "gp", "ws")
    G = {k: Guarded(max(4096, rig.total + 64), fill="nan") for k in names}
    rng = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    p, pk = bufs.params[0].ptr, bufs.packed[0].ptr
    Pp = {k: g.ptr for k, g in G.items()}
    calls = {
        "hint_block_forward": lambda: lib.hint_block_forward(plan, p, pk, Pp["x"], Pp["c"], Pp["z"], Pp["J"], Pp["tape"], 0, st),
        "hint_block_forward_ex": lambda: lib.hint_block_forward_ex(plan, p, pk, Pp["x"], Pp["c"], Pp["z"], Pp["J"], Pp["tape"],
                                                                   Pp["perm"], Pp["J_in"], Pp["loss"], 0, st),
        "hint_block_forward_noisy": lambda: lib.hint_block_forward_noisy(plan, p, pk, Pp["x"], Pp["c"], Pp["z"], Pp["J"], Pp["tape"],
                                                                         None, Pp["J_in"], Pp["loss"], 0.5, rng.data_ptr(), Pp["xn"], 0, st),
        "hint_block_inverse": lambda: lib.hint_block_inverse(plan, p, pk, Pp["z"], Pp["c"], Pp["x"], Pp["J"], 0, st),
        "hint_block_inverse_ex": lambda: lib.hint_block_inverse_ex(plan, p, pk, Pp["z"], Pp["c"], Pp["x"], Pp["J"], Pp["perm"],
                                                                   Pp["J_in"], 0, st),
        "hint_block_backward_rows": lambda: lib.hint_block_backward_rows(plan, p, pk, Pp["x"], Pp["tape"], Pp["c"], Pp["z"], Pp["J"],
                                                                         Pp["gx"], Pp["gc"], Pp["ws"], 16384, None, 1.0, 0.0, 0, st),
    }
    for acc in (0, 1):
        calls[f"hint_block_backward acc={acc}"] = lambda acc=acc: lib.hint_block_backward(
            plan, p, pk, Pp["x"], Pp["tape"], Pp["c"], Pp["z"], Pp["J"], Pp["gx"], Pp["gc"], Pp["gp"], acc, Pp["ws"], 16384, 0, st)
        calls[f"hint_block_backward_ex acc={acc}"] = lambda acc=acc: lib.hint_block_backward_ex(
            plan, p, pk, Pp["x"], Pp["tape"], Pp["c"], Pp["z"], Pp["J"], Pp["gx"], Pp["gc"], Pp["gp"], acc, Pp["ws"], 16384, None,
            1.0, 0.0, 0, st)
        calls[f"hint_block_inverse_backward acc={acc}"] = lambda acc=acc: lib.hint_block_inverse_backward(
            plan, p, Pp["x"], Pp["c"], Pp["z"], Pp["J"], Pp["gx"], Pp["gc"], Pp["gp"], acc, Pp["ws"], 16384, None, 0, st)
    for name, fn in calls.items():
        for g in G.values():
            g.fill("nan")
        check(fn(), name)
        torch.cuda.synchronize()
        for k, g in G.items():
            g.check_guards(f"{name} B=0: {k}")
            if k == "gp" and "acc=0" in name:
                assert bool((g.t[:rig.total] == 0).all()), f"{name} B=0: g_params not zeroed"
                assert bool((g.words[rig.total:] == NAN_BITS).all()), f"{name} B=0: zeroed past param_floats"
            else:
                assert bool((g.words == NAN_BITS).all()), f"{name} B=0: {k} changed"
    bufs.close()


@pytest.mark.parametrize("front_perm", [False, True], ids=["perm_from_block1", "perm_on_every_block"])
def test_aliasing(lib, front_perm):
    """hint_chain_forward / hint_chain_inverse with x == z on a multi-pass ragged batch: bit-identical to the separate call"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = multi_pass_b(cu, 1)
    rig = Rig(contract_case(3, B), lib)
    disp = plan_dispatch(lib, rig.plan, B)
    assert disp["passes"] >= 2 and disp["groups"] % disp["grid"], disp
    perms = list(rig.perms)
    if front_perm:
        perms[0] = orc.random_orthogonal(rig.case.d, seed=99, dtype=torch.float64).float()
    bufs = ChainBufs(rig, B, "nan", tape=False, perms=perms)
    inp = rows_in(rig, B)
    d = rig.case.d
    for name, fn, src in (("hint_chain_forward", lib.hint_chain_forward, inp.x), ("hint_chain_inverse", lib.hint_chain_inverse, inp.zi)):
        out, J = Guarded(B * d, fill="nan"), Guarded(B, fill="nan")
        extra = (None, None) if name == "hint_chain_forward" else (None,)
        check(fn(bufs.ch, src.ptr, inp.c.ptr, out.ptr, J.ptr, *extra, stream()), name)
        al, J2 = Guarded(B * d).set(src.t), Guarded(B, fill="nan")
        check(fn(bufs.ch, al.ptr, inp.c.ptr, al.ptr, J2.ptr, *extra, stream()), name + " aliased")
        torch.cuda.synchronize()
        for g in (out, J, al, J2):
            g.check_guards(name)
        assert torch.isfinite(out.t).all(), name
        assert bits_equal(al.t, out.t), f"{name}: x == z differs from the separate call"
        assert bits_equal(J2.t, J.t), f"{name}: J with x == z differs"
    bufs.close()


def test_fused_adam_arenas(lib):
    """hint_chain_backward_adam and hint_chain_wgrad_adam (after hint_block_backward_rows): the NaN-filled gradient arena stays
    bit for bit, so do the gaps of P, M and V around and between the blocks' slices; the slices equal the clean run's"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * cu + 9
    rig = Rig(contract_case(3), lib)
    nb, total, d, dc = rig.n_blocks, rig.total, rig.case.d, rig.case.dc
    gap = 4 * 37                                     # floats before, between and after the slices (16-byte multiples)
    n = gap + nb * (total + gap)
    offs = [gap + i * (total + gap) for i in range(nb)]
    inp = rows_in(rig, B)
    opt = torch.tensor([1e-3, 0.9, 0.95, 0.0, 0.0], dtype=torch.float64)
    opt[3], opt[4] = 1e-3 / (1 - 0.9 ** 3), 1 / math.sqrt(1 - 0.95 ** 3)
    opt_state = opt.float().to(DEV)
    inside = torch.zeros(n, dtype=torch.bool)
    for o in offs:
        inside[o:o + total] = True

    def arenas(fill):
        A = [Guarded(n, fill=fill, align=16, seed=500 + k) for k in range(3)]      # P, M, V
        M0, V0 = Guarded(n, fill="junk", seed=600), Guarded(n, fill="junk", seed=601)
        A[1].t.copy_(M0.t * 1e-3)
        A[2].t.copy_(V0.t.abs() * 1e-6)
        for i in range(nb):
            src = rig.flat_params(i, "zero")
            A[0].t[offs[i]:offs[i] + total].copy_(src.t)
        if fill != "zero":                      # the gaps around and between the slices
            for g in A:
                g.words[~inside.to(DEV)] = NAN_BITS
        return A

    def run(mode, fill):
        A = arenas(fill)
        views = [A[0].ptr + 4 * o for o in offs]       # every block's parameters are its slice of P: the fused step writes there
        bufs = ChainBufs(rig, B, fill, gp_fill="nan", param_ptrs=views, commit=False,
                        perms=None if mode == "chain" else [None] * nb)      # (gathered blocks ran without a fused permutation)
        gx, gc = Guarded(B * d, fill=fill), Guarded(B * dc, fill=fill)
        if mode == "chain":
            check(lib.hint_chain_commit(bufs.ch), "hint_chain_commit")
            z, J = Guarded(B * d, fill=fill), Guarded(B, fill=fill)
            check(lib.hint_chain_forward(bufs.ch, inp.x.ptr, inp.c.ptr, z.ptr, J.ptr, None, None, stream()), "hint_chain_forward")
            check(lib.hint_chain_backward_adam(bufs.ch, inp.x.ptr, inp.c.ptr, inp.gz.ptr, inp.gJ.ptr, gx.ptr, gc.ptr, 1.0, 0.0,
                                               A[0].ptr, A[1].ptr, A[2].ptr, n, opt_state.data_ptr(), 0.9, 0.95, 1e-4, 1e-5,
                                               1.0, 5.0, stream()), "hint_chain_backward_adam")
        else:
            # every block as a launch of its own on its own input (hint_block_forward_ex + hint_block_backward_rows), then one
            # part B with the step for all of them over a chain of gathered blocks
            xs = [Guarded(B * d).set(torch.randn(B, d, generator=torch.Generator().manual_seed(40 + i))) for i in range(nb)]
            for i in range(nb):
                z, J = Guarded(B * d, fill=fill), Guarded(B, fill=fill)
                check(lib.hint_block_forward_ex(rig.plan, views[i], bufs.packed[i].ptr, xs[i].ptr, inp.c.ptr, z.ptr, J.ptr,
                                                bufs.tapes[i].ptr, None, None, None, B, stream()), "hint_block_forward_ex")
                check(lib.hint_block_backward_rows(rig.plan, views[i], bufs.packed[i].ptr, xs[i].ptr, bufs.tapes[i].ptr, inp.c.ptr,
                                                   inp.gz.ptr, inp.gJ.ptr, gx.ptr, gc.ptr, bufs.wss[i].ptr, 4 * bufs.ws_n, None,
                                                   1.0, 0.0, B, stream()), "hint_block_backward_rows")
                check(lib.hint_chain_set_block_io(bufs.ch, i, xs[i].ptr, inp.c.ptr, None), "hint_chain_set_block_io")
            check(lib.hint_chain_commit(bufs.ch), "hint_chain_commit")
            check(lib.hint_chain_wgrad_adam(bufs.ch, None, None, A[0].ptr, A[1].ptr, A[2].ptr, n, opt_state.data_ptr(), 0.9, 0.95,
                                            1e-4, 1e-5, 1.0, 5.0, stream()), "hint_chain_wgrad_adam")
        torch.cuda.synchronize()
        for k, g in enumerate(A):
            g.check_guards(f"{mode} {fill}: arena {'PMV'[k]}")
        for i, g in enumerate(bufs.gps):
            assert bool((g.words == NAN_BITS).all()), f"{mode} {fill}: the gradient arena of block {i} was written"
            g.check_guards(f"{mode} {fill}: g_params {i}")
        out = [g.t.cpu() for g in A]
        bufs.close()
        return out

    for mode in ("chain", "gathered"):
        clean = run(mode, "zero")
        got = run(mode, "nan")
        for k in range(3):
            assert torch.isfinite(clean[k][inside]).all(), f"{mode}: clean {'PMV'[k]} not finite"
            assert bits_equal(got[k][inside], clean[k][inside]), f"{mode}: slices of {'PMV'[k]} differ from the clean run"
            assert bool((got[k][~inside].view(torch.int32) == NAN_BITS).all()), f"{mode}: a gap of {'PMV'[k]} changed"
        # the clean run's gap elements of P inside a block's slice (its padding) are not stepped either
        pad = torch.cat([gap_mask(rig) for _ in range(nb)])
        Pin = clean[0][inside]
        assert bool((Pin[pad] == 0).all()), f"{mode}: the padding inside a block's slice of P was stepped"


def test_loss_acc_accumulates(lib):
    """loss_acc is added to: (result - prefill) = the clean sums within 1e-6 relative; nothing behind slot 64 is touched"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = multi_pass_b(cu, 1)
    rig = Rig(contract_case(2, B), lib)
    inp = rows_in(rig, B)
    res = {}
    for fill in ("zero", "junk"):
        bufs = ChainBufs(rig, B, "nan" if fill == "junk" else "zero")
        loss = Guarded(128, fill=fill, seed=77)
        pre = loss.t.cpu().double()
        z, J = Guarded(B * rig.case.d, fill="nan"), Guarded(B, fill="nan")
        check(lib.hint_chain_forward(bufs.ch, inp.x.ptr, inp.c.ptr, z.ptr, J.ptr, None, loss.ptr, stream()), "hint_chain_forward")
        torch.cuda.synchronize()
        loss.check_guards("loss_acc")
        res[fill] = (loss.t.cpu().double() - pre, pre)
        bufs.close()
    clean = res["zero"][0]
    delta, pre = res["junk"]
    tol = 1e-6 * (pre.abs() + clean.abs()) + 1e-6 * float(clean.abs().max())
    assert bool(((delta - clean).abs() <= tol).all()), "loss_acc: result - prefill differs from the clean sums"
    assert float(clean.abs().sum()) > 0


def test_pack_group_run_ex(lib):
    """clears exactly zero_floats floats, packs every block as the clean run does, advances rng_state[1] by one and writes
    Adam's step factors into opt_state[3], [4]"""
    rig = Rig(contract_case(3), lib)
    nb = rig.n_blocks
    packed_n = lib.hint_plan_packed_floats(rig.plan)
    outs = {}
    for fill in ("zero", "nan", "junk"):
        params = [rig.flat_params(i, fill, 1) for i in range(nb)]
        packed = [Guarded(packed_n, fill=fill, seed=90 + i) for i in range(nb)]
        plans = (C.c_void_p * nb)(*([rig.plan.value] * nb))
        pp = (C.c_void_p * nb)(*[g.ptr for g in params])
        kp = (C.c_void_p * nb)(*[g.ptr for g in packed])
        grp = C.c_void_p()
        check(lib.hint_pack_group_create(plans, pp, kp, nb, C.byref(grp)), "hint_pack_group_create")
        zb = Guarded(300, fill="junk", seed=3)
        before = zb.t.clone()
        rng = Guarded(4, dtype=torch.int64).set(torch.tensor([123, 6], dtype=torch.int64))
        opt = Guarded(5).set(torch.tensor([2e-3, 0.9, 0.95, float("nan"), float("nan")]))
        try:
            check(lib.hint_pack_group_run_ex(grp, zb.ptr, 131, rng.ptr, opt.ptr, stream()), "hint_pack_group_run_ex")
            if fill == "zero":
                check(lib.hint_pack_group_run(grp, stream()), "hint_pack_group_run")
            torch.cuda.synchronize()
        finally:
            lib.hint_pack_group_destroy(grp)
        for g in params + packed + [zb, rng, opt]:
            g.check_guards(f"pack group {fill}")
        assert bool((zb.t[:131] == 0).all()) and bits_equal(zb.t[131:], before[131:]), "zero_buf: not exactly zero_floats cleared"
        r = rng.t.cpu()
        assert r[0] == 123 and r[1] == 7, f"rng_state: {r.tolist()}"
        o = opt.t.cpu().double()
        lr, b1, b2 = (float(v) for v in o[:3])           # (the kernel computes from the float32 values it reads)
        assert (lr, b1, b2) == tuple(float(torch.tensor(v)) for v in (2e-3, 0.9, 0.95)), "opt_state[0..2] changed"
        f3, f4 = lr / (1 - b1 ** 7), 1 / math.sqrt(1 - b2 ** 7)
        assert abs(o[3] - f3) <= 1e-7 * f3, f"opt_state[3] {float(o[3])} != {f3}"
        assert abs(o[4] - f4) <= 1e-7 * f4, f"opt_state[4] {float(o[4])} != {f4}"
        outs[fill] = [g.t.cpu() for g in packed]
    for fill in ("nan", "junk"):
        for i in range(nb):
            assert bits_equal(outs[fill][i], outs["zero"][i]), f"pack group {fill}: packed block {i} differs"


def test_noisy_forwards(lib):
    """hint_block_forward_noisy and hint_chain_forward_noisy write every x_noisy element, bit-identical under every fill"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * cu + 9
    rig = Rig(contract_case(2), lib)
    d = rig.case.d
    inp = rows_in(rig, B)
    rng = torch.tensor([42, 3], dtype=torch.int64, device=DEV)
    res = {}
    for fill, align in (("zero", 256),) + RUNS:
        bufs = ChainBufs(rig, B, fill, align=align, perms=[None] * rig.n_blocks)
        got = []
        for kind in ("block", "chain"):
            xn, z = (Guarded(B * d, fill=fill, align=align, seed=s) for s in (1, 2))
            J = Guarded(B, fill=fill, align=align, seed=3)
            if kind == "block":
                check(lib.hint_block_forward_noisy(rig.plan, bufs.params[0].ptr, bufs.packed[0].ptr, inp.x.ptr, inp.c.ptr, z.ptr,
                                                   J.ptr, bufs.tapes[0].ptr, None, None, None, 0.25, rng.data_ptr(), xn.ptr, B,
                                                   stream()), "hint_block_forward_noisy")
            else:
                check(lib.hint_chain_forward_noisy(bufs.ch, inp.x.ptr, inp.c.ptr, z.ptr, J.ptr, None, None, 0.25, rng.data_ptr(),
                                                   xn.ptr, stream()), "hint_chain_forward_noisy")
            torch.cuda.synchronize()
            for g in (xn, z, J):
                g.check_guards(f"{kind} noisy {fill}")
            got.append([g.t.cpu() for g in (xn, z, J)])
        bufs.guards(f"noisy {fill}")
        bufs.close()
        res[(fill, align)] = got
    x = inp.host[0].reshape(-1)
    for k, got in res.items():
        for kind, (xn, z, J) in zip(("block", "chain"), got):
            assert torch.isfinite(xn).all() and (xn - x).abs().max() < 3.0 and (xn != x).float().mean() > 0.99, \
                f"{kind} noisy {k}: x_noisy not fully written"
        for a, b in zip(got, res[("zero", 256)]):
            for u, v in zip(a, b):
                assert bits_equal(u, v), f"noisy forwards {k}: differ from the clean run"


def test_inverse_backward_poisoned_workspace(lib):
    """hint_block_inverse_backward with poisoned workspace and outputs: bit-identical to the clean run"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * cu + 9
    for case in [c for c in CASES if c.name in ("n3_cond_block_big_s", "wl_nr1_block", "fly_block_big_s")]:
        rig = Rig(case, lib)
        d, dc = case.d, case.dc
        nbytes = int(lib.hint_plan_inverse_workspace_bytes(rig.plan, B))
        assert nbytes > 0, lib.hint_last_error()
        inp = rows_in(rig, B)
        res = {}
        for fill, align in (("zero", 256),) + RUNS:
            params = rig.flat_params(0, fill)
            packed = Guarded(lib.hint_plan_packed_floats(rig.plan), fill=fill)
            check(lib.hint_block_pack(rig.plan, params.ptr, packed.ptr, stream()), "hint_block_pack")
            xo, J = Guarded(B * d, fill=fill, align=align), Guarded(B, fill=fill, align=align)
            check(lib.hint_block_inverse(rig.plan, params.ptr, packed.ptr, inp.zi.ptr, ptr(inp.c), xo.ptr, J.ptr, B, stream()),
                  "hint_block_inverse")
            gz = Guarded(B * d, fill=fill, align=align, seed=1)
            gc = Guarded(B * dc, fill=fill, align=align, seed=2) if dc else None
            gp = Guarded(rig.total, fill=fill, align=align, seed=3)
            ws = Guarded(nbytes // 4 + 1, fill=fill, align=align, seed=4)
            check(lib.hint_block_inverse_backward(rig.plan, params.ptr, xo.ptr, ptr(inp.c), inp.gz.ptr, inp.gJ.ptr, gz.ptr, ptr(gc),
                                                  gp.ptr, 0, ws.ptr, nbytes, None, B, stream()), "hint_block_inverse_backward")
            torch.cuda.synchronize()
            for g in (params, packed, xo, J, gz, gc, gp, ws):
                if g is not None:
                    g.check_guards(f"{case.name} inverse backward {fill}")
            res[(fill, align)] = [g.t.cpu() for g in (xo, J, gz, gp) + ((gc,) if dc else ())]
        assert all(torch.isfinite(t).all() for t in res[("zero", 256)]), f"{case.name} inverse backward: clean run not finite"
        for k, got in res.items():
            for u, v in zip(got, res[("zero", 256)]):
                assert bits_equal(u, v), f"{case.name} inverse backward {k}: differs from the clean run"


def test_ext_coeffs_and_affine_chain(lib):
    """hint_block_ext_coeffs on poisoned coef_out (R = 0 writes nothing) and an inference chain with a per-row affine step
    (hint_chain_set_block_affine) on poisoned outputs: bit-identical to the clean run"""
    import hint_amd
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    D, dc, h, R = 100, 4, 224, 16 * cu + 9
    torch.manual_seed(3)
    mod = hint_amd.ExternalAffineCoupling([(D,)], dims_c=[(dc,)], F_args={"internal_size": h}).to(DEV)
    for p in mod.parameters():
        p.data = 0.1 * torch.randn_like(p)
    eng = mod.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    eng.pack()
    c = Guarded(R * dc).set(torch.randn(R, dc))
    rig = Rig(next(cs for cs in CASES if cs.name == "fly_block_big_s"), lib)       # d = 100 on the general kernels
    res = {}
    for fill, align in (("zero", 256),) + RUNS:
        coef = Guarded(R * 2 * D, fill=fill, align=align)
        check(lib.hint_block_ext_coeffs(eng.plan, eng.arena.data_ptr(), eng.packed.data_ptr(), c.ptr, 0, coef.ptr, stream()), "R=0")
        torch.cuda.synchronize()
        assert bits_equal(coef.t, Guarded(R * 2 * D, fill=fill, align=align).t), "hint_block_ext_coeffs R = 0 wrote something"
        check(lib.hint_block_ext_coeffs(eng.plan, eng.arena.data_ptr(), eng.packed.data_ptr(), c.ptr, R, coef.ptr, stream()),
              "hint_block_ext_coeffs")
        bufs = ChainBufs(rig, R, fill, tape=False)
        check(lib.hint_chain_set_block_affine(bufs.ch, 0, coef.ptr, 2 * D), "hint_chain_set_block_affine")
        check(lib.hint_chain_commit(bufs.ch), "hint_chain_commit")
        x = Guarded(R * D).set(torch.randn(R, D, generator=torch.Generator().manual_seed(8)))
        outs = []
        for name, fn in (("forward", lib.hint_chain_forward), ("inverse", lib.hint_chain_inverse)):
            z, J = Guarded(R * D, fill=fill, align=align), Guarded(R, fill=fill, align=align)
            extra = (None, None) if name == "forward" else (None,)
            check(fn(bufs.ch, x.ptr, None, z.ptr, J.ptr, *extra, stream()), f"hint_chain_{name}")
            torch.cuda.synchronize()
            z.check_guards(name); J.check_guards(name)
            outs += [z.t.cpu(), J.t.cpu()]
        coef.check_guards("coef")
        bufs.close()
        res[(fill, align)] = [coef.t.cpu()] + outs
    for k, got in res.items():
        for u, v in zip(got, res[("zero", 256)]):
            assert torch.isfinite(v).all() and bits_equal(u, v), f"ext coeffs / affine chain {k}: differs from the clean run"


@pytest.mark.parametrize("n", [4 * 1000 + 1, 4 * 1000 + 3, 4 * 70000 + 1])
@pytest.mark.parametrize("dev", [False, True], ids=["host_step", "dev_step"])
def test_adam_steps(lib, n, dev):
    """hint_adam_step(_dev) at n = 4k+1, 4k+3: nothing past n changes, zero_grads clears exactly n floats, the step matches
    torch's float64 Adam"""
    extra = 61
    P, G, M, V = (Guarded(n + extra, fill="junk", align=16, seed=s) for s in (1, 2, 3, 4))
    M.t.mul_(1e-3)
    V.t.copy_(V.t.abs() * 1e-3)
    before = [g.t.clone() for g in (P, G, M, V)]
    opt = torch.tensor([1e-3, 0.9, 0.95, 1e-3 / (1 - 0.9 ** 4), 1 / math.sqrt(1 - 0.95 ** 4)], dtype=torch.float32, device=DEV)
    if dev:
        st = lib.hint_adam_step_dev(P.ptr, G.ptr, M.ptr, V.ptr, n, opt.data_ptr(), 0.9, 0.95, 1e-4, 1e-5, 0.5, 5.0, 1, stream())
    else:
        st = lib.hint_adam_step(P.ptr, G.ptr, M.ptr, V.ptr, n, 4, 1e-3, 0.9, 0.95, 1e-4, 1e-5, 0.5, 5.0, 1, stream())
    check(st, "hint_adam_step")
    torch.cuda.synchronize()
    for name, g, b in zip("PGMV", (P, G, M, V), before):
        g.check_guards(name)
        assert bits_equal(g.t[n:], b[n:]), f"adam n={n}: {name} changed past n"
    assert bool((G.t[:n] == 0).all()), f"adam n={n}: zero_grads did not clear n floats"
    p0, g0, m0, v0 = (b[:n].double().cpu() for b in before)
    g = (g0 * 0.5).clamp(-5, 5) + 1e-5 * p0
    m = 0.9 * m0 + 0.1 * g
    v = 0.95 * v0 + 0.05 * g * g
    p = p0 - (1e-3 / (1 - 0.9 ** 4)) * m / (v.sqrt() / math.sqrt(1 - 0.95 ** 4) + 1e-4)
    assert float((P.t[:n].double().cpu() - p).abs().max()) <= 1e-5 * float(p.abs().max()), f"adam n={n}: P"
    assert float((M.t[:n].double().cpu() - m).abs().max()) <= 1e-5 * float(m.abs().max()), f"adam n={n}: M"


@pytest.mark.parametrize("name", ["n3_cond_block_big_s", "wl_nr1_block_big_s", "fly_block_big_s"])
def test_ex_forms(lib, name):
    """hint_block_forward_ex / hint_block_inverse_ex / hint_block_backward_ex on a real batch with a fused permutation, J_in,
    loss_acc, g_J = NULL and gz_scale / gJ_const (what the module route's engine passes): bit-identical under every fill"""
    case = next(c for c in CASES if c.name == name)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * cu + 9
    rig = Rig(case, lib)
    d, dc = case.d, case.dc
    inp = rows_in(rig, B)
    perm = Guarded(d * d).set(orc.random_orthogonal(d, seed=7, dtype=torch.float64).float())
    J_in = Guarded(B).set(torch.randn(B, generator=torch.Generator().manual_seed(3)))
    tape_n, ws_n = rig.sizes(B)
    res = {}
    for fill, align in (("zero", 256),) + RUNS:
        params = rig.flat_params(0, fill)
        packed = Guarded(lib.hint_plan_packed_floats(rig.plan), fill=fill)
        check(lib.hint_block_pack(rig.plan, params.ptr, packed.ptr, stream()), "hint_block_pack")
        A = lambda n, s: Guarded(n, fill=fill, align=align, seed=s)                  # noqa: E731
        z, J, tape, loss = A(B * d, 1), A(B, 2), Guarded(tape_n, fill=fill, seed=3), Guarded(128)
        xi, Ji = A(B * d, 4), A(B, 5)
        gx, gc, gp, ws = A(B * d, 6), (A(B * dc, 7) if dc else None), A(rig.total, 8), A(ws_n, 9)
        check(lib.hint_block_forward_ex(rig.plan, params.ptr, packed.ptr, inp.x.ptr, ptr(inp.c), z.ptr, J.ptr, tape.ptr, perm.ptr,
                                        J_in.ptr, loss.ptr, B, stream()), "hint_block_forward_ex")
        # x = NULL: with a fused permutation the backward reads the permuted input from the tape
        check(lib.hint_block_backward_ex(rig.plan, params.ptr, packed.ptr, None, tape.ptr, ptr(inp.c), z.ptr, None, gx.ptr, ptr(gc),
                                         gp.ptr, 0, ws.ptr, 4 * ws_n, perm.ptr, 1.0 / B, -1.0 / B, B, stream()),
              "hint_block_backward_ex")
        check(lib.hint_block_inverse_ex(rig.plan, params.ptr, packed.ptr, inp.zi.ptr, ptr(inp.c), xi.ptr, Ji.ptr, perm.ptr,
                                        J_in.ptr, B, stream()), "hint_block_inverse_ex")
        torch.cuda.synchronize()
        bufs = dict(params=params, packed=packed, z=z, J=J, tape=tape, loss=loss, xi=xi, Ji=Ji, gx=gx, gc=gc, gp=gp, ws=ws)
        for k, g in bufs.items():
            if g is not None:
                g.check_guards(f"{name} _ex {fill}/{align}: {k}")
        res[(fill, align)] = {k: bufs[k].t.cpu() for k in ("packed", "z", "J", "xi", "Ji", "gx", "gc", "gp") if bufs[k] is not None}
        res[(fill, align)]["loss"] = loss.t.cpu().double()
    clean = res[("zero", 256)]
    for k, v in clean.items():
        assert torch.isfinite(v).all(), f"{name} _ex: clean {k} not finite"
    for key, got in res.items():
        for k, v in got.items():
            if k == "loss":     # atomically accumulated: the order of the slots' additions varies
                assert float((v - clean[k]).abs().max()) <= 1e-6 * float(clean[k].abs().max()), f"{name} _ex {key}: loss_acc"
            else:
                assert bits_equal(v, clean[k]), f"{name} _ex {key}: {k} differs from the clean run"


# ---- C: the product's own paths on a poisoned caching allocator --------------------------------------------------------------

def engines_of(*modules):
    return [m.tree.engine(torch.device(DEV)) for mod in modules for m in mod.modules() if hasattr(m, "tree")]


def product_run(fill, B=1000):
    """the product's eager paths with torch's caching allocator primed with freed blocks that hold `fill`: -> every result"""
    import gc
    import hint_amd
    from hint_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    flow = hint_amd.HintFlow(8, 3, [64, 32, 16]).to(DEV)
    flow_mod = hint_amd.HintFlow(8, 3, [64, 32, 16]).to(DEV)
    blk = hint_amd.HierarchicalAffineCouplingBlock([(8,)], dims_c=[(3,)], c_internal=[64, 32, 16]).to(DEV)
    cm = hint_amd.ConditionalHintFlow(12, 4, 3, 32)
    for p in cm.parameters():
        p.data = 0.07 * torch.randn_like(p)
    cm = cm.to(DEV)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, 8, generator=g).to(DEV) for _ in range(3)]
    cxs = [torch.randn(B, 12, generator=g).to(DEV) for _ in range(3)]
    cys = [torch.randn(B, 4, generator=g).to(DEV) for _ in range(3)]
    xb, cb = torch.randn(B, 8, generator=g).to(DEV), torch.randn(B, 3, generator=g).to(DEV)
    zx, ys = torch.randn(B, 12, generator=g).to(DEV), torch.randn(1, 4, generator=g).to(DEV)
    # the sizes the product will ask for, and a spread around them
    sizes = set()
    for e in engines_of(flow, flow_mod, blk, cm):
        tape_n, ws_b = e.sizes(B)
        for n in (tape_n, ws_b // 4, lib.hint_plan_packed_floats(e.plan), e.total, B * e.d, B * max(e.dc, 1), B, 128):
            sizes.update({n, n + 7, int(n * 1.1) + 1, max(1, int(n * 0.9))})
    tape_n = engines_of(flow)[0].sizes(B)[0]
    # a flow and its ChainRunner refer to each other: what an earlier run (or test) left is freed by the cycle collector
    # alone, and until it runs empty_cache cannot release the segments it holds - the probe below may then land on stale data
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    bits = NAN_BITS if fill == "nan" else 0
    primed = [torch.empty(n, dtype=torch.int32, device=DEV).fill_(bits) for n in sorted(sizes) for _ in range(3)]
    del primed
    probe = torch.empty(tape_n, dtype=torch.float32, device=DEV)
    if fill == "nan":
        assert bool(torch.isnan(probe).all()), "torch.empty of the tape size does not return the NaN-filled block"
    else:
        assert bool((probe == 0).all())
    del probe
    out = {}
    tr = hint_amd.FlowTrainer(flow, noise=0.0, use_graph=False)
    out["flow_losses"] = [[float(v) for v in tr.step(x)] for x in xs]
    out.update(flow_P=tr.P.cpu(), flow_M=tr.M.cpu(), flow_V=tr.V.cpu())
    with torch.no_grad():
        xi, Ji = tr.sample(xs[0][:333])
    out.update(flow_sample=xi.cpu(), flow_sample_J=Ji.cpu())
    ctr = hint_amd.ConditionalFlowTrainer(cm, use_graph=False, seed=1234)
    out["cond_losses"] = [[float(v) for v in ctr.step(x, y)] for x, y in zip(cxs, cys)]
    out.update(cond_P=ctr.P.cpu(), cond_M=ctr.M.cpu(), cond_V=ctr.V.cpu())
    sx, sJ = cm.sample_conditional(ys, zx)
    out.update(cond_sample=sx.cpu(), cond_sample_J=sJ.cpu())
    # module route: a whole flow (the fused chain) and one conditional block, forward and backward
    for name, mod, c in (("flow", flow_mod, None), ("block", blk, cb)):
        x = xb.clone().requires_grad_(True)
        cc = c.clone().requires_grad_(True) if c is not None else None
        if name == "flow":
            z = mod(x)
            J = mod.log_jacobian(run_forward=False)
        else:
            (z,) = mod([x], c=[cc])
            J = mod.jacobian(None)
        (0.5 * (z ** 2).sum(1) - J).mean().backward()
        out[f"{name}_z"], out[f"{name}_J"], out[f"{name}_gx"] = z.detach().cpu(), J.detach().cpu(), x.grad.cpu()
        if cc is not None:
            out[f"{name}_gc"] = cc.grad.cpu()
        for k, p in mod.named_parameters():
            out[f"{name}_grad_{k}"] = p.grad.cpu()
    torch.cuda.synchronize()
    return out


def test_product_paths_on_nan_cache():
    """FlowTrainer and ConditionalFlowTrainer (eager, three steps each), the module route's forward and backward and
    sample_conditional give the same bits - P, M, V and every output; the losses within 1e-6 (atomic sums) - whether the caching
    allocator's free blocks hold NaN or zeros.  (Graph-captured steps allocate from a private pool this does not reach.)"""
    a = product_run("nan")
    b = product_run("zero")
    assert a.keys() == b.keys()
    for k in a:
        if k.endswith("losses"):
            for u, v in zip(a[k], b[k]):
                for p, q in zip(u, v):
                    assert math.isfinite(p) and abs(p - q) <= 1e-6 * max(1.0, abs(q)), f"{k}: {u} vs {v}"
        else:
            assert torch.isfinite(b[k]).all(), f"{k}: not finite on the zero-filled cache"
            assert bits_equal(a[k], b[k]), f"{k}: differs between the NaN- and the zero-filled cache"
