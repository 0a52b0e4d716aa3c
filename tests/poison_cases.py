"""What the poison tests (tests/test_gpu_poison.py) run, and which of them covers each C entry point that writes device memory.

ENTRY_TESTS names, for every hint_* function of include/hint_amd.h that takes a non-const device pointer, the test that runs it
on poisoned, guard-banded buffers; EXCLUDED lists the functions with such a parameter that write no device memory themselves,
each with the reason.  tests/test_poison_table_cpu.py parses the header and fails, naming the function, when one is in neither.

Rig builds one ledger case (tests/instance_cases.py) for direct C-ABI calls: the plan of the case's tree, its parameters (the
same float32 values tests/test_gpu_instances.py gives the oracle) laid out in flat guarded buffers, and run() - forward,
inverse and backward of a block or a chain, every buffer guarded and filled as asked."""
import ctypes as C

import torch

from guarded import Guarded, poison_gaps

DEV = "cuda:0"
T = "tests/test_gpu_poison.py::"

ENTRY_TESTS = {
    "hint_block_pack": T + "test_ledger_under_poison",
    "hint_pack_group_run": T + "test_pack_group_run_ex",
    "hint_pack_group_run_ex": T + "test_pack_group_run_ex",
    "hint_block_forward": T + "test_ledger_under_poison",
    "hint_block_inverse": T + "test_ledger_under_poison",
    "hint_block_backward": T + "test_ledger_under_poison",
    "hint_block_forward_ex": T + "test_ex_forms",
    "hint_block_inverse_ex": T + "test_ex_forms",
    "hint_block_backward_ex": T + "test_ex_forms",
    "hint_block_inverse_backward": T + "test_inverse_backward_poisoned_workspace",
    "hint_chain_set_block": T + "test_ledger_under_poison",
    "hint_chain_forward": T + "test_ledger_under_poison",
    "hint_chain_forward_noisy": T + "test_noisy_forwards",
    "hint_chain_backward": T + "test_ledger_under_poison",
    "hint_chain_backward_parts": T + "test_accumulate",
    "hint_chain_wgrad_range": T + "test_accumulate",
    "hint_chain_inverse": T + "test_aliasing",
    "hint_chain_backward_adam": T + "test_fused_adam_arenas",
    "hint_chain_wgrad_adam": T + "test_fused_adam_arenas",
    "hint_block_forward_noisy": T + "test_noisy_forwards",
    "hint_block_backward_rows": T + "test_fused_adam_arenas",
    "hint_block_ext_coeffs": T + "test_ext_coeffs_and_affine_chain",
    "hint_adam_step": T + "test_adam_steps",
    "hint_adam_step_dev": T + "test_adam_steps",
}

EXCLUDED = {
    "hint_plan_create": "host out-parameter (the plan handle); uploads plan tables it allocates itself",
    "hint_plan_check": "host-only dry run: stats is host memory",
    "hint_plan_describe": "writes a host int32 array",
    "hint_plan_dispatch": "writes a host int32 array",
    "hint_plan_check_dispatch": "host-only: writes a host int32 array",
    "hint_plan_check_digest": "host-only: writes a host uint64 array",
    "hint_plan_paths": "writes a host int32 array",
    "hint_plan_check_paths": "host-only: writes a host int32 array",
    "hint_pack_group_create": "records the packed pointers (written by hint_pack_group_run*); copies a table it allocates",
    "hint_chain_create": "host out-parameter (the chain handle)",
    "hint_chain_set_block_io": "records pointers only; the chain's part B reads them",
    "hint_chain_set_block_affine": "records a const pointer; the affine chain is run by test_ext_coeffs_and_affine_chain",
}


def descs_and_plan(lib, d, dc, widths):
    """a module of the tree, its engine (device plan) and its parameters' (name, offset, numel) in the flat layout"""
    import hint_amd
    blk = hint_amd.HierarchicalAffineCouplingBlock([(d,)], dims_c=[(dc,)] if dc else [], c_internal=list(widths)).to(DEV)
    eng = blk.tree.engine(torch.device(DEV))
    names = {id(p): n for n, p in blk.named_parameters()}
    layout = [(names[id(p)], off, n) for p, off, n in zip(eng.params, eng.offsets, eng.numels)]
    return blk, eng, layout


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(st, what):
    from hint_amd import _lib
    _lib.check(st, what)


class Rig:
    """one ledger case as direct C-ABI calls (block: hint_block_*; chain: hint_chain_*) on guarded buffers"""

    def __init__(self, case, lib):
        from oracle import hint_oracle as orc
        from test_gpu_instances import big_s
        self.case, self.lib = case, lib
        self.blk, self.eng, self.layout = descs_and_plan(lib, case.d, case.dc, case.widths)
        self.plan = self.eng.plan
        self.total = self.eng.total
        assert self.total == lib.hint_plan_param_floats(self.plan)
        self.n_blocks = case.n_blocks if case.entry == "chain" else 1
        dims_c = [(case.dc,)] if case.dc else []
        if case.entry == "chain":
            self.ref = orc.OracleFlow(case.d, case.n_blocks, list(case.widths), dims_c=dims_c, seed=3, init_scale=case.scale,
                                      dtype=torch.float64)
            self.ref.params = [{k: v.float().double() for k, v in P.items()} for P in self.ref.params]
            if case.big_s:
                self.ref.params = [big_s(P, case.big_s) for P in self.ref.params]
            self.ref.perms = [None if p is None else p.float().double() for p in self.ref.perms]
            self.P = [{k: v.float() for k, v in P.items()} for P in self.ref.params]
            self.perms = [None if p is None else p.float() for p in self.ref.perms]
        else:
            self.nodes = orc.build_nodes(case.d, dims_c, list(case.widths))
            P = orc.init_params(self.nodes, seed=5, scale=case.scale)
            if case.big_s:
                P = big_s(P, case.big_s)
            self.P, self.perms = [P], [None]

    def covered(self):
        return [(off, n) for _, off, n in self.layout]

    def flat_params(self, i, fill, seed=0):
        """block i's flat parameters in a guarded buffer, the gaps between tensors filled with `fill`"""
        g = Guarded(self.total)
        for name, off, n in self.layout:
            g.words[off:off + n].copy_(self.P[i][name].reshape(-1).to(DEV).view(torch.int32))
        poison_gaps(g.words, self.covered(), self.total, fill, seed + 17 * i)
        return g

    def sizes(self, B):
        tape = self.lib.hint_plan_tape_floats(self.plan, B)
        ws = int(self.lib.hint_plan_workspace_bytes(self.plan, B))
        assert tape >= 0 and ws % 4 == 0
        return max(tape, 1), max(ws // 4, 4)

    def inputs(self, B, seed=11, rows=None):
        """x, c, zi (finite), gz, gJ on the host; rows = None: cotangents on every row, else only on those rows"""
        g = torch.Generator().manual_seed(seed)
        d, dc = self.case.d, self.case.dc
        x = torch.randn(B, d, generator=g)
        c = torch.randn(B, dc, generator=g) if dc else None
        zi = torch.randn(B, d, generator=g)
        gz = torch.randn(B, d, generator=g)
        gJ = torch.randn(B, generator=g)
        if rows is not None:
            m = torch.zeros(B, dtype=torch.bool)
            m[rows] = True
            gz, gJ = gz * m[:, None], gJ * m
        return x, c, zi, gz, gJ

    def run(self, B, fill, align, host_inputs, seed=0):
        """forward (training: tape), backward (accumulate = 0) and inverse on buffers filled with `fill`; every guard and every
        const input checked afterwards.  -> dict of host copies of every output (gp: one flat gradient per block)"""
        lib, plan, st = self.lib, self.plan, stream()
        d, dc, nb = self.case.d, self.case.dc, self.n_blocks
        x, c, zi, gz, gJ = host_inputs
        tape_n, ws_n = self.sizes(B)
        A = lambda n, s: Guarded(n, fill=fill, align=align, seed=seed + s)            # noqa: E731  outputs and scratch
        I = lambda t: Guarded(t.numel(), align=align).set(t)                          # noqa: E731  inputs
        params = [self.flat_params(i, fill, seed) for i in range(nb)]
        packed_n = lib.hint_plan_packed_floats(plan)
        packed = [Guarded(packed_n, fill=fill, seed=seed + 100 + i) for i in range(nb)]      # (poisoned before the pack)
        perms = [None if p is None else Guarded(p.numel()).set(p) for p in self.perms]
        xg, zig, gzg, gJg = I(x), I(zi), I(gz), I(gJ)
        cg = I(c) if dc else None
        consts = [g for g in [xg, zig, gzg, gJg, cg] + perms if g is not None]
        snaps = [g.snapshot() for g in consts]
        z, J, xi, Ji, gx = A(B * d, 1), A(B, 2), A(B * d, 3), A(B, 4), A(B * d, 5)
        gc = A(B * dc, 6) if dc else None
        tapes = [Guarded(tape_n, fill=fill, seed=seed + 7 + i) for i in range(nb)]
        wss = [A(ws_n, 20 + i) for i in range(nb)]
        gps = [A(self.total, 40 + i) for i in range(nb)]
        cp = cg.ptr if dc else None
        for i in range(nb):
            check(lib.hint_block_pack(plan, params[i].ptr, packed[i].ptr, st), "hint_block_pack")
        param_snaps = [g.snapshot() for g in params]
        if self.case.entry == "block":
            check(lib.hint_block_forward(plan, params[0].ptr, packed[0].ptr, xg.ptr, cp, z.ptr, J.ptr, tapes[0].ptr, B, st),
                  "hint_block_forward")
            check(lib.hint_block_backward(plan, params[0].ptr, packed[0].ptr, xg.ptr, tapes[0].ptr, cp, gzg.ptr, gJg.ptr, gx.ptr,
                                          gc.ptr if dc else None, gps[0].ptr, 0, wss[0].ptr, 4 * ws_n, B, st),
                  "hint_block_backward")
            check(lib.hint_block_inverse(plan, params[0].ptr, packed[0].ptr, zig.ptr, cp, xi.ptr, Ji.ptr, B, st),
                  "hint_block_inverse")
        else:
            ch = C.c_void_p()
            check(lib.hint_chain_create(plan, nb, B, C.byref(ch)), "hint_chain_create")
            try:
                for i in range(nb):
                    check(lib.hint_chain_set_block(ch, i, params[i].ptr, packed[i].ptr, None if perms[i] is None else perms[i].ptr,
                                                   tapes[i].ptr, wss[i].ptr, 4 * ws_n, gps[i].ptr), "hint_chain_set_block")
                check(lib.hint_chain_commit(ch), "hint_chain_commit")
                check(lib.hint_chain_forward(ch, xg.ptr, cp, z.ptr, J.ptr, None, None, st), "hint_chain_forward")
                check(lib.hint_chain_backward(ch, xg.ptr, cp, gzg.ptr, gJg.ptr, gx.ptr, gc.ptr if dc else None, 1.0, 0.0, 0, st),
                      "hint_chain_backward")
                check(lib.hint_chain_inverse(ch, zig.ptr, cp, xi.ptr, Ji.ptr, None, st), "hint_chain_inverse")
                torch.cuda.synchronize()
            finally:
                lib.hint_chain_destroy(ch)
        torch.cuda.synchronize()
        for g, s in zip(consts, snaps):
            g.check_unchanged(s, f"{self.case.name} B={B} {fill}: input")
        for i, (g, s) in enumerate(zip(params, param_snaps)):
            g.check_unchanged(s, f"{self.case.name} B={B} {fill}: params of block {i}")
        named = dict(z=z, J=J, xi=xi, Ji=Ji, gx=gx, gc=gc, **{f"packed{i}": g for i, g in enumerate(packed)},
                     **{f"tape{i}": g for i, g in enumerate(tapes)}, **{f"workspace{i}": g for i, g in enumerate(wss)},
                     **{f"g_params{i}": g for i, g in enumerate(gps)})
        for k, g in named.items():
            if g is not None:
                g.check_guards(f"{self.case.name} B={B} {fill}: {k}")
        out = dict(z=z.t.view(B, d).cpu(), J=J.t.cpu(), xi=xi.t.view(B, d).cpu(), Ji=Ji.t.cpu(), gx=gx.t.view(B, d).cpu(),
                   gc=gc.t.view(B, dc).cpu() if dc else None, gp=[g.t.cpu() for g in gps],
                   packed=[g.t.cpu() for g in packed])
        return out
