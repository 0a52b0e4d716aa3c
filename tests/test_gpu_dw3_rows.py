"""The row jobs of backward part B (hint_wgrad.hip dw_rows: dW3 | db3 of units with at most four outputs as 4x4x1 MFMAs, one
wavefront per job and batch split; HINT_DW3_ROWS) against the float64 oracle and against the jobs they replace.

Per tree and entry point (one block through hint_block_*, a 3-block chain through hint_chain_*), with the knob forced on and
forced off, and per batch size - 1, 15, 16, 17 (around one 16-row step), 100 (Bp = 112: seven one-step splits) and 4096 + 17
(eight splits of 33 steps, the last one partial):
  - the W3 and b3 gradients of every subnet and the whole flat gradient of every block against the oracle: 1e-4 of the tensor's
    (the flat gradient's) largest entry.  Rows within KINK of a ReLU kink in the oracle get zero cotangents, as in the chain tests
    (tests/test_gpu_instances.py); the inputs' seeds are chosen per case so that the oracle alone keeps their share under the
    ledger's cap of 6 % at every batch size (SEEDS; test_seed_keeps_kink_share_under_cap asserts it without a GPU).  The two
    3-block chains of the (140, 70) tree cannot: a block of that tree alone shows 2.3 % (its twelve ReLU layers), three of them
    6.3 .. 7.7 % whatever the seed (seeds 11 .. 38, 4113 rows), so they take the geometry ledger's rule for such chains
    (wgrad_geometry.CHAIN_KINK_CAP: the largest share the oracle shows plus 3 points): 10 %
  - two runs with accumulate = 0 are bit-identical (the second on a NaN-filled workspace: every slab element that the reduction
    reads is written by a job first), the gaps between the tensors are cleared
  - a run with accumulate = 1 on top of that gradient gives exactly twice it (x + x is exact), again on NaN-filled slabs, and
    leaves the gaps alone
  - knob on against knob off: every tensor but W3 / b3 bit-identical (their jobs are the same), W3 / b3 within DIFF_BOUND of
    their largest entry (the sums differ in order only: off = per wavefront the rows 4 kq + i of every other 16-row step, combined
    over lanes, wavefronts and splits; on = per split in row order)."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

from hint_amd import _lib
from guarded import NAN_BITS, bits_equal
from test_gpu_instances import KINK, Spy

DEV = "cuda:0"
# the smallest seed from 11 on with which the oracle keeps every batch size of the case under its cap
SEEDS = {("d6", "block"): 13, ("d6", "chain"): 21, ("d2_r1", "block"): 11, ("d2_r1", "chain"): 11, ("d8_r4", "block"): 11,
         ("d8_r4", "chain"): 11, ("d6_dc4", "block"): 14, ("d6_dc4", "chain"): 38}
TOL = 1e-4                      # of the tensor's largest entry
KINK_CAP = 0.06                 # instance_cases.Case.kink_cap
CHAIN_KINK_CAP = {("d6", "chain"): 0.10, ("d6_dc4", "chain"): 0.10}       # (see above)
# largest |on - off| / max |off| of a W3 / b3 tensor seen on an MI355X over all cases and batch sizes: 8.0e-6 (d2_r1 block, B = 100;
# 7.5e-6 d8_r4 block, B = 17; at most 2.7e-6 elsewhere - NOTES.md section 16), times 4 as the summation order is all that differs
DIFF_BOUND = 4 * 8.0e-6
BATCHES = (1, 15, 16, 17, 100, 4096 + 17)
KNOB = "HINT_DW3_ROWS"

TREES = {"d6": (6, 0, (140, 70)), "d2_r1": (2, 0, (17,)), "d8_r4": (8, 0, (64, 16)), "d6_dc4": (6, 4, (140, 70))}
CASES = [(t, e) for t in TREES for e in ("block", "chain")]


def case_of(tree, entry):
    d, dc, widths = TREES[tree]
    return SimpleNamespace(name=f"{tree}-{entry}", entry=entry, d=d, dc=dc, widths=widths, scale=0.05, big_s=0.0, n_blocks=3, knobs={},
                           seed=SEEDS[(tree, entry)], kink_cap=CHAIN_KINK_CAP.get((tree, entry), KINK_CAP))


class Model:
    """the float32 weights of a case (as poison_cases.Rig draws them) and its float64 oracle; no GPU"""

    def __init__(self, case):
        from oracle import hint_oracle as orc
        self.case = case
        dims_c = [(case.dc,)] if case.dc else []
        if case.entry == "chain":
            self.ref = orc.OracleFlow(case.d, case.n_blocks, list(case.widths), dims_c=dims_c, seed=3, init_scale=case.scale,
                                      dtype=torch.float64)
            self.ref.params = [{k: v.float().double() for k, v in P.items()} for P in self.ref.params]
            self.ref.perms = [None if p is None else p.float().double() for p in self.ref.perms]
            self.P64 = self.ref.params
        else:
            self.nodes = orc.build_nodes(case.d, dims_c, list(case.widths))
            self.P64 = [{k: v.double() for k, v in orc.init_params(self.nodes, seed=5, scale=case.scale).items()}]

    def inputs(self, B):
        g = torch.Generator().manual_seed(self.case.seed)
        x = torch.randn(B, self.case.d, generator=g)
        c = torch.randn(B, self.case.dc, generator=g) if self.case.dc else None
        gz = torch.randn(B, self.case.d, generator=g)
        gJ = torch.randn(B, generator=g)
        return x, c, gz, gJ

    def oracle(self, B):
        """-> (inputs with the kink rows' cotangents zeroed, kink rows, {(block, name): float64 gradient})"""
        from oracle import hint_oracle as orc
        x, c, gz, gJ = self.inputs(B)
        P = [{k: v.detach().clone().requires_grad_(True) for k, v in Pb.items()} for Pb in self.P64]
        xs = x.double()
        cs = [c.double()] if self.case.dc else []
        with Spy(B) as spy:
            if self.case.entry == "chain":
                keep_params = self.ref.params
                self.ref.params = P
                try:
                    z, J = self.ref.forward(xs, tuple(cs))
                finally:
                    self.ref.params = keep_params
            else:
                z, J = orc.block_apply(self.nodes, P[0], xs, cs, rev=False)
        keep = spy.kink > KINK
        gz, gJ = gz * keep[:, None], gJ * keep
        ((z * gz.double()).sum() + (J * gJ.double()).sum()).backward()
        return (x, c, gz, gJ), B - int(keep.sum()), {(i, k): v.grad for i, Pb in enumerate(P) for k, v in Pb.items()}


@functools.lru_cache(maxsize=None)
def model(tree, entry):
    return Model(case_of(tree, entry))


@functools.lru_cache(maxsize=None)
def reference(tree, entry, B):
    return model(tree, entry).oracle(B)


@pytest.mark.parametrize("tree,entry", CASES, ids=[f"{t}-{e}" for t, e in CASES])
def test_seed_keeps_kink_share_under_cap(tree, entry):
    """the oracle alone (no GPU): with the case's seed no batch of it has more than the ledger's cap of rows next to a ReLU kink"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for B in BATCHES:
        _, dropped, _ = reference(tree, entry, B)
        print(f"{tree}-{entry} B={B}: {dropped} row(s) next to a ReLU kink")
        assert dropped <= model(tree, entry).case.kink_cap * B, (tree, entry, B, dropped)


class Device:
    """one plan (built under the knob set at construction) and the case's weights on the GPU, as direct C-ABI calls"""

    def __init__(self, m, lib):
        from poison_cases import descs_and_plan
        self.m, self.lib, case = m, lib, m.case
        self.blk, self.eng, self.layout = descs_and_plan(lib, case.d, case.dc, case.widths)
        self.plan, self.total = self.eng.plan, self.eng.total
        self.nb = len(m.P64)
        self.real = torch.zeros(self.total, dtype=torch.bool)
        for _, off, n in self.layout:
            self.real[off:off + n] = True
        self.params, self.packed = [], []
        st = torch.cuda.current_stream().cuda_stream
        for Pb in m.P64:
            flat = torch.zeros(self.total, device=DEV)
            for name, off, n in self.layout:
                flat[off:off + n] = Pb[name].float().reshape(-1).to(DEV)
            packed = torch.empty(lib.hint_plan_packed_floats(self.plan), device=DEV)
            _lib.check(lib.hint_block_pack(self.plan, flat.data_ptr(), packed.data_ptr(), st), "hint_block_pack")
            self.params.append(flat)
            self.packed.append(packed)
        self.perms = [None] * self.nb
        if case.entry == "chain":
            self.perms = [None if p is None else p.float().to(DEV).contiguous() for p in m.ref.perms]

    def run(self, B, host, gps, accumulate, ws_nan):
        """training forward + backward of the batch; gps: one flat gradient buffer per block (written or added to)"""
        lib, plan, case = self.lib, self.plan, self.m.case
        st = torch.cuda.current_stream().cuda_stream
        x, c, gz, gJ = host
        xd, gzd, gJd = x.to(DEV).contiguous(), gz.to(DEV).contiguous(), gJ.to(DEV).contiguous()
        cd = c.to(DEV).contiguous() if case.dc else None
        cp = cd.data_ptr() if case.dc else None
        ws_n = max(int(lib.hint_plan_workspace_bytes(plan, B)) // 4, 4)
        tapes = [torch.zeros(max(lib.hint_plan_tape_floats(plan, B), 1), device=DEV) for _ in range(self.nb)]
        wss = [torch.empty(ws_n, dtype=torch.int32, device=DEV).fill_(NAN_BITS if ws_nan else 0) for _ in range(self.nb)]
        z, J, gx = torch.empty(B, case.d, device=DEV), torch.empty(B, device=DEV), torch.empty(B, case.d, device=DEV)
        gc = torch.zeros(B, case.dc, device=DEV) if case.dc else None
        gcp = gc.data_ptr() if case.dc else None
        if case.entry == "block":
            _lib.check(lib.hint_block_forward(plan, self.params[0].data_ptr(), self.packed[0].data_ptr(), xd.data_ptr(), cp,
                                              z.data_ptr(), J.data_ptr(), tapes[0].data_ptr(), B, st), "hint_block_forward")
            _lib.check(lib.hint_block_backward(plan, self.params[0].data_ptr(), self.packed[0].data_ptr(), xd.data_ptr(),
                                               tapes[0].data_ptr(), cp, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(), gcp,
                                               gps[0].data_ptr(), accumulate, wss[0].data_ptr(), 4 * ws_n, B, st), "hint_block_backward")
        else:
            ch = C.c_void_p()
            _lib.check(lib.hint_chain_create(plan, self.nb, B, C.byref(ch)), "hint_chain_create")
            try:
                for i in range(self.nb):
                    _lib.check(lib.hint_chain_set_block(ch, i, self.params[i].data_ptr(), self.packed[i].data_ptr(),
                                                        None if self.perms[i] is None else self.perms[i].data_ptr(),
                                                        tapes[i].data_ptr(), wss[i].data_ptr(), 4 * ws_n, gps[i].data_ptr()),
                               "hint_chain_set_block")
                _lib.check(lib.hint_chain_commit(ch), "hint_chain_commit")
                _lib.check(lib.hint_chain_forward(ch, xd.data_ptr(), cp, z.data_ptr(), J.data_ptr(), None, None, st), "hint_chain_forward")
                _lib.check(lib.hint_chain_backward(ch, xd.data_ptr(), cp, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(), gcp, 1.0, 0.0,
                                                   accumulate, st), "hint_chain_backward")
                torch.cuda.synchronize()
            finally:
                lib.hint_chain_destroy(ch)
        torch.cuda.synchronize()

    def gradients(self, B, host):
        """-> the flat gradients of the blocks (host); asserts determinism, poisoned slabs, accumulate = 1 and the gaps on the way"""
        name = f"{self.m.case.name} B={B}"
        sentinel = 12345.0
        new = lambda: [torch.full((self.total,), sentinel, device=DEV) for _ in range(self.nb)]     # noqa: E731
        g0, g1 = new(), new()
        self.run(B, host, g0, 0, ws_nan=False)
        self.run(B, host, g1, 0, ws_nan=True)
        out = []
        for i in range(self.nb):
            a, b = g0[i].cpu(), g1[i].cpu()
            assert bool(torch.isfinite(b[self.real]).all()), f"{name}: block {i}: non-finite gradient from NaN-filled slabs"
            assert bits_equal(a, b), f"{name}: block {i}: two runs differ ({int((a.view(torch.int32) != b.view(torch.int32)).sum())} words)"
            assert bool((a[~self.real] == 0).all()), f"{name}: block {i}: accumulate = 0 clears the gaps between the tensors"
            out.append(a)
            g1[i][~self.real.to(DEV)] = sentinel
        self.run(B, host, g1, 1, ws_nan=True)
        for i in range(self.nb):
            b = g1[i].cpu()
            assert bits_equal(b[self.real], 2 * out[i][self.real]), f"{name}: block {i}: accumulate = 1 is not g + g"
            assert bool((b[~self.real] == sentinel).all()), f"{name}: block {i}: accumulate = 1 wrote a gap"
        return out


def is_w3(name):
    return ".4." in name            # the subnets' last layer: s.4.weight, s.4.bias, t.4.weight, t.4.bias


@pytest.mark.gpu
@pytest.mark.parametrize("tree,entry", CASES, ids=[f"{t}-{e}" for t, e in CASES])
def test_row_jobs_vs_oracle_and_vs_generic_jobs(tree, entry, monkeypatch):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib = _lib.load()
    m = model(tree, entry)
    worst_ref, worst_diff = {}, {}
    try:
        devs = {}
        for knob in ("1", "0"):
            monkeypatch.setenv(KNOB, knob)
            lib.hint_debug_reload_knobs()
            devs[knob] = Device(m, lib)
        for B in BATCHES:
            host, dropped, ref = reference(tree, entry, B)
            assert dropped <= m.case.kink_cap * B, (tree, entry, B, dropped)
            got = {knob: dev.gradients(B, host) for knob, dev in devs.items()}
            layout = devs["1"].layout
            fails = []
            for knob in ("1", "0"):
                for i in range(devs[knob].nb):
                    flat_ref = torch.zeros(devs[knob].total, dtype=torch.float64)
                    for n, off, cnt in layout:
                        r = ref[(i, n)].reshape(-1)
                        flat_ref[off:off + cnt] = r
                        if is_w3(n):
                            e = float((got[knob][i][off:off + cnt].double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
                            worst_ref[(knob, "W3|b3")] = max(worst_ref.get((knob, "W3|b3"), 0.0), e)
                            if e > TOL:
                                fails.append((knob, B, i, n, e))
                    real = devs[knob].real
                    e = float((got[knob][i].double() - flat_ref)[real].abs().max()) / max(float(flat_ref.abs().max()), 1e-30)
                    worst_ref[(knob, "flat")] = max(worst_ref.get((knob, "flat"), 0.0), e)
                    if e > TOL:
                        fails.append((knob, B, i, "flat gradient", e))
            for i in range(devs["1"].nb):
                for n, off, cnt in layout:
                    on, off_ = got["1"][i][off:off + cnt], got["0"][i][off:off + cnt]
                    if is_w3(n):
                        e = float((on.double() - off_.double()).abs().max()) / max(float(off_.abs().max()), 1e-30)
                        worst_diff[B] = max(worst_diff.get(B, 0.0), e)
                        if e > DIFF_BOUND:
                            fails.append(("on vs off", B, i, n, e))
                    elif not bits_equal(on, off_):
                        fails.append(("on vs off: not bit-identical", B, i, n, 0.0))
            print(f"{tree}-{entry} B={B}: kink rows {dropped}; worst vs oracle so far "
                  + ", ".join(f"{k[0]}/{k[1]} {v:.2e}" for k, v in sorted(worst_ref.items()))
                  + f"; on vs off W3|b3 {worst_diff[B]:.2e}")
            assert not fails, fails
    finally:
        monkeypatch.undo()
        lib.hint_debug_reload_knobs()
        print(f"{tree}-{entry}: on vs off, largest relative difference of a W3 | b3 tensor per batch size: "
              + ", ".join(f"B={B} {v:.2e}" for B, v in worst_diff.items()) + f" (bound {DIFF_BOUND:.1e})")
