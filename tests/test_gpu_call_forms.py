"""Every call form of the block and chain C ABI on every kernel family against the float64 oracle, one group of forms of one family
per test (tests/call_forms.py is the ledger; tests/test_call_forms_cpu.py checks it without a GPU).

Per test: the family's batch size is resolved for the device's CU count, and hint_plan_dispatch on the real plan must show the declared
instances before anything is compared.  The calls are direct C-ABI calls through hint_amd._lib on plain torch.empty buffers (guard
bands and poisoned scratch are tests/test_gpu_poison.py's job; only what the header documents as read - loss_acc, an accumulated
g_params, Adam's moments - is initialised).  Rows come from one kink-free pool per family and group of forms: candidates next to a
ReLU kink in the float64 oracle are discarded beforehand (the Spy rule, KINK, the ledger's caps), no row is waived.  Tolerances are
check_fwd / check_grads and TOL_* of tests/test_gpu_instances.py: a dropped term is an error of order 1
(test_a_natural_mistake_is_far_over_the_bound).  Each test prints its worst error over bound per form before it asserts.

Behind the oracle comparisons every test holds the launch to tests/golden/launch_bits.json (tests/golden/make_launch_bits.py wrote
it): a sha256 of every generated input and of every tensor the forms hand back, the dynamic LDS bytes of the last forward and
backward launch and the tape and workspace sizes at that B - the host launch path's decisions, bit for bit.  The bits belong to
the CU count they were recorded on: on another device the test fails and says so."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from hint_amd import _lib
import call_forms as cf
from instance_cases import plan_dispatch
from poison_cases import check, descs_and_plan, stream
from test_gpu_instances import TOL_FWD, TOL_GW, TOL_GX, check_fwd, check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = (TOL_FWD, TOL_GX, TOL_GW)
NB = cf.N_BLOCKS


class Rig:
    """the plan of a family's tree, three blocks' parameters as slices of one arena, packed; tapes, workspaces and a gradient arena"""

    def __init__(self, fam, lib, B):
        self.fam, self.lib, self.B = fam, lib, B
        self.blk, self.eng, self.layout = descs_and_plan(lib, fam.d, fam.dc, fam.widths)
        self.plan, self.total = self.eng.plan, self.eng.total
        assert self.total == lib.hint_plan_param_floats(self.plan) and self.total % 4 == 0
        self.nodes, self.P, W = cf.make_params(fam)
        self.W = [w.to(DEV).contiguous() for w in W]
        self.arena = torch.zeros(NB * self.total, device=DEV)
        self.shapes = {name: self.P[0][name].shape for name, _, _ in self.layout}
        for i in range(NB):
            for name, off, n in self.layout:
                self.arena[i * self.total + off:i * self.total + off + n] = self.P[i][name].reshape(-1).to(DEV)
        self.params = [self.arena[i * self.total:(i + 1) * self.total] for i in range(NB)]
        self.packed = [torch.empty(lib.hint_plan_packed_floats(self.plan), device=DEV) for _ in range(NB)]
        for i in range(NB):
            check(lib.hint_block_pack(self.plan, self.params[i].data_ptr(), self.packed[i].data_ptr(), stream()), "hint_block_pack")
        self.tape_n = max(lib.hint_plan_tape_floats(self.plan, B), 1)
        self.ws_bytes = int(lib.hint_plan_workspace_bytes(self.plan, B))
        self.tapes = [torch.empty(self.tape_n, device=DEV) for _ in range(NB)]
        self.wss = [torch.empty(max(self.ws_bytes // 4, 4), device=DEV) for _ in range(NB)]
        self.G = torch.empty(NB * self.total, device=DEV)
        self.gps = [self.G[i * self.total:(i + 1) * self.total] for i in range(NB)]
        self.real = torch.zeros(self.total, dtype=torch.bool, device=DEV)        # the flat layout's real elements (not padding)
        for _, off, n in self.layout:
            self.real[off:off + n] = True

    def assert_dispatch(self, entry):
        disp = plan_dispatch(self.lib, self.plan, self.B)
        print(f"{self.fam.name} ({entry}): B={self.B} on {disp['num_cu']} CUs: nw={disp['nw']} nr={disp['nr']} alt4={disp['alt4']} tiles={disp['tiles']} "
              f"grid={disp['grid']} fwd={disp['fwd']} bwd={disp['bwd']} dw=<{disp['dw_small']},{disp['dw_wide']}> dw_splits={disp['dw_splits']} "
              f"dw_rows={disp['dw_rows']}")
        m = cf.family_mismatch(self.fam, disp, self.B, entry)
        assert m is None, m

    def split(self, flat):
        """{tensor name: gradient} of one block's flat gradient"""
        return {name: flat[off:off + n].view(self.shapes[name]) for name, off, n in self.layout}

    def chain(self, perms, io):
        """a training chain over the three blocks; io[i] = (x_in, c_in, g_add) tensors or None"""
        lib = self.lib
        h = C.c_void_p()
        check(lib.hint_chain_create(self.plan, NB, self.B, C.byref(h)), "hint_chain_create")
        for i in range(NB):
            check(lib.hint_chain_set_block(h, i, self.params[i].data_ptr(), self.packed[i].data_ptr(), ptr(perms[i]), self.tapes[i].data_ptr(),
                                           self.wss[i].data_ptr(), self.ws_bytes, self.gps[i].data_ptr()), "hint_chain_set_block")
            check(lib.hint_chain_set_block_io(h, i, *[ptr(t) for t in io[i]]), "hint_chain_set_block_io")
        check(lib.hint_chain_commit(h), "hint_chain_commit")
        return h


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(rows):
    return {k: v.to(DEV).contiguous() for k, v in rows.items()}


class Worst:
    """worst error over bound per form, printed whatever the assertions do"""

    def __init__(self, fam):
        self.fam, self.w = fam, {}

    def add(self, form, got, ref):
        for k, v in cf.ratios(got, ref, TOL).items():
            if v >= self.w.get(form, (-1.0, None))[0]:
                self.w[form] = (v, k)

    def note(self, form, v, what):
        if v >= self.w.get(form, (-1.0, None))[0]:
            self.w[form] = (v, what)

    def print(self):
        for form, (v, k) in sorted(self.w.items()):
            print(f"call form {form} on {self.fam.name}: worst error over bound {v:.3f} at {k}")


def check_loss_acc(worst, form, loss, z, J):
    """the 64 slots summed in double against the double sum of the device's own z and J: (B + 64) 2^-24 sum |term| is the summation
    order alone (z and J themselves meet the oracle elsewhere)"""
    B = z.shape[0]
    slots = loss.double().cpu().view(-1, 2)[:64]
    t0, t1 = 0.5 * (z.double().cpu() ** 2).sum(dim=1), J.double().cpu()
    for k, t in ((0, t0), (1, t1)):
        bound = (B + 64) * 2.0 ** -24 * float(t.abs().sum())
        e = abs(float(slots[:, k].sum()) - float(t.sum()))
        worst.note(form, e / bound, f"loss_acc[.][{k}]")
        assert e <= bound, (form, "loss_acc", k, e, bound)
    assert bool((loss.view(-1)[128:] == 0).all())


def grads_ok(name, got, ref):
    check_grads(name, got["gx"], got.get("gc"), got["gw"], ref)


# ------------------------------------------------------------------------------------------------------ F1, F2, F3: one block
def run_block_forms(rig, worst):
    fam, lib, B, st = rig.fam, rig.lib, rig.B, stream()
    d, dc, plan = fam.d, fam.dc, rig.plan
    rows = cf.block_rows(fam, B)
    r = dev(rows)
    c = r.get("c")
    p0, pk0, W0 = rig.params[0].data_ptr(), rig.packed[0].data_ptr(), rig.W[0].data_ptr()
    E = lambda *s: torch.empty(*s, device=DEV)                                        # noqa: E731
    # F1
    z, J, tape, loss = E(B, d), E(B), rig.tapes[0], torch.zeros(192, device=DEV)
    check(lib.hint_block_forward_ex(plan, p0, pk0, r["x"].data_ptr(), ptr(c), z.data_ptr(), J.data_ptr(), tape.data_ptr(), W0,
                                    r["J_in"].data_ptr(), loss.data_ptr(), B, st), "hint_block_forward_ex")
    torch.cuda.synchronize()
    ref = cf.oracle_F1(fam, rows)
    worst.add("F1", dict(z=z, J=J), ref)
    check_loss_acc(worst, "F1", loss, z, J)
    check_fwd("F1 z", z, ref["z"])
    check_fwd("F1 J", J, ref["J"])
    # F2
    xi, Ji = E(B, d), E(B)
    check(lib.hint_block_inverse_ex(plan, p0, pk0, r["zi"].data_ptr(), ptr(c), xi.data_ptr(), Ji.data_ptr(), W0, r["J_in"].data_ptr(), B, st),
          "hint_block_inverse_ex")
    torch.cuda.synchronize()
    ref = cf.oracle_F2(fam, rows)
    worst.add("F2", dict(xi=xi, Ji=Ji), ref)
    check_fwd("F2 inverse x", xi, ref["xi"])
    check_fwd("F2 inverse J", Ji, ref["Ji"])
    # F3, first pass: the NLL's gradient - g_z := the device's z, g_J = NULL, x = NULL (the tape's top slice)
    first, second = cf.oracle_F3(fam, rows)
    gx, gc, gp, ws = E(B, d), (E(B, dc) if dc else None), rig.gps[0], rig.wss[0]
    check(lib.hint_block_backward_ex(plan, p0, pk0, None, tape.data_ptr(), ptr(c), z.data_ptr(), None, gx.data_ptr(), ptr(gc), gp.data_ptr(), 0,
                                     ws.data_ptr(), rig.ws_bytes, W0, 1.0 / B, -1.0 / B, B, st), "hint_block_backward_ex")
    torch.cuda.synchronize()
    got = dict(gx=gx, gc=gc, gw=rig.split(gp))
    worst.add("F3", got, first)
    # second pass: per-row g_J, gz_scale = 0.37, accumulate = 1 onto a random R of every tensor's own size
    R = torch.zeros(rig.total)
    g = torch.Generator().manual_seed(3)
    for name, off, n in rig.layout:
        R[off:off + n] = torch.randn(n, generator=g) * float(second["gw"][name].abs().max())
    gp2 = rig.gps[1]
    gp2.copy_(R)
    gx2, gc2 = E(B, d), (E(B, dc) if dc else None)
    check(lib.hint_block_backward_ex(plan, p0, pk0, None, tape.data_ptr(), ptr(c), r["gz"].data_ptr(), r["gJ"].data_ptr(), gx2.data_ptr(), ptr(gc2),
                                     gp2.data_ptr(), 1, ws.data_ptr(), rig.ws_bytes, W0, cf.GZ_SCALE2, 0.0, B, st), "hint_block_backward_ex")
    torch.cuda.synchronize()
    got2 = dict(gx=gx2, gc=gc2, gw=rig.split(gp2.double().cpu() - R.double()))       # result = R + gradient
    worst.add("F3", got2, second)
    grads_ok("F3 first pass", got, first)
    grads_ok("F3 second pass (accumulate)", got2, second)
    assert torch.equal(gp2.cpu()[~rig.real.cpu()], R[~rig.real.cpu()]), "accumulate: the arena's padding changed"
    return r, dict(z=z, J=J, loss=loss, xi=xi, Ji=Ji, gx=gx, gc=gc, gp=gp[rig.real], gx2=gx2, gc2=gc2, gp2=gp2[rig.real])


# ------------------------------------------------------------------------------------------------------ F4, F5: the chain
def run_chain_forms(rig, worst):
    fam, lib, B, st = rig.fam, rig.lib, rig.B, stream()
    d, dc = fam.d, fam.dc
    rows = cf.chain_rows(fam, B)
    r = dev(rows)
    c = r.get("c")
    E = lambda *s: torch.empty(*s, device=DEV)                                        # noqa: E731
    h = rig.chain([None, rig.W[1], rig.W[2]], [(None, None, r[f"g_add{i}"]) for i in range(NB)])
    try:
        z, J, loss = E(B, d), E(B), torch.zeros(192, device=DEV)
        check(lib.hint_chain_forward(h, r["x"].data_ptr(), ptr(c), z.data_ptr(), J.data_ptr(), r["J_in"].data_ptr(), loss.data_ptr(), st),
              "hint_chain_forward")
        gx, gc = E(B, d), (E(B, dc) if dc else None)
        args = (h, r["x"].data_ptr(), ptr(c), r["gz"].data_ptr(), r["gJ"].data_ptr())
        check(lib.hint_chain_backward(*args, gx.data_ptr(), ptr(gc), 1.0, 0.0, 0, st), "hint_chain_backward")
        torch.cuda.synchronize()
        ref = cf.oracle_F4(fam, rows)
        G4 = rig.G.clone()
        got = dict(z=z, J=J, gx=gx, gc=gc, gw={(i, k): v for i in range(NB) for k, v in rig.split(G4[i * rig.total:(i + 1) * rig.total]).items()})
        worst.add("F4", got, ref)
        check_loss_acc(worst, "F4", loss, z, J)
        check_fwd("F4 z", z, ref["z"])
        check_fwd("F4 J", J, ref["J"])
        grads_ok("F4", got, ref)
        # F5: the halves one by one, then the weight gradients bucket by bucket - the bits of the single call
        real = rig.real.repeat(NB)
        junk = torch.randn(NB * rig.total, generator=torch.Generator().manual_seed(9)).to(DEV)
        rig.G.copy_(junk)
        gx5, gc5 = E(B, d), (E(B, dc) if dc else None)
        check(lib.hint_chain_backward_parts(*args, gx5.data_ptr(), ptr(gc5), 1.0, 0.0, 0, 1, st), "hint_chain_backward_parts")
        check(lib.hint_chain_backward_parts(*args, gx5.data_ptr(), ptr(gc5), 1.0, 0.0, 0, 2, st), "hint_chain_backward_parts")
        torch.cuda.synchronize()
        same = torch.equal(gx5, gx) and (not dc or torch.equal(gc5, gc)) and torch.equal(rig.G[real], G4[real])
        worst.note("F5", 0.0 if same else float("inf"), "parts 1 then 2")
        assert same, "F5: hint_chain_backward_parts 1 then 2 differs from the single call"
        rig.G.copy_(junk)
        check(lib.hint_chain_wgrad_range(h, r["x"].data_ptr(), ptr(c), 0, 2, 3, st), "hint_chain_wgrad_range")
        check(lib.hint_chain_wgrad_range(h, r["x"].data_ptr(), ptr(c), 0, 0, 2, st), "hint_chain_wgrad_range")
        torch.cuda.synchronize()
        same = torch.equal(rig.G[real], G4[real])
        worst.note("F5", 0.0 if same else float("inf"), "wgrad_range [2,3) then [0,2)")
        assert same, "F5: hint_chain_wgrad_range [2,3) then [0,2) differs from the single call"
        return r, dict(z=z, J=J, loss=loss, gx=gx, gc=gc, G=G4[real])
    finally:
        lib.hint_chain_destroy(h)


# ------------------------------------------------------------------------------------------------ F6, F7: gathered part B
def run_gathered_forms(rig, worst):
    fam, lib, B, st = rig.fam, rig.lib, rig.B, stream()
    d, dc, plan = fam.d, fam.dc, rig.plan
    rows = cf.gathered_rows(fam, B)
    r = dev(rows)
    E = lambda *s: torch.empty(*s, device=DEV)                                        # noqa: E731
    perms = [None, rig.W[1], None]
    cs = [r.get(f"c{i}") for i in range(NB)]
    # block 1 has a fused permutation: no x_in, part B reads its permuted input from the tape's top slice
    h = rig.chain(perms, [(None if perms[i] is not None else r[f"x{i}"], cs[i], None) for i in range(NB)])
    try:
        out = [dict(z=E(B, d), J=E(B), gx=E(B, d), gc=E(B, dc) if dc else None) for _ in range(NB)]

        def rows_launches():
            for i in range(NB):
                o, p, pk = out[i], rig.params[i].data_ptr(), rig.packed[i].data_ptr()
                check(lib.hint_block_forward_ex(plan, p, pk, r[f"x{i}"].data_ptr(), ptr(cs[i]), o["z"].data_ptr(), o["J"].data_ptr(),
                                                rig.tapes[i].data_ptr(), ptr(perms[i]), None, None, B, st), "hint_block_forward_ex")
                check(lib.hint_block_backward_rows(plan, p, pk, r[f"x{i}"].data_ptr(), rig.tapes[i].data_ptr(), ptr(cs[i]), r[f"gz{i}"].data_ptr(),
                                                   r[f"gJ{i}"].data_ptr(), o["gx"].data_ptr(), ptr(o["gc"]), rig.wss[i].data_ptr(), rig.ws_bytes,
                                                   ptr(perms[i]), 1.0, 0.0, B, st), "hint_block_backward_rows")
        rows_launches()
        check(lib.hint_chain_wgrad_range(h, None, None, 0, 0, NB, st), "hint_chain_wgrad_range")
        torch.cuda.synchronize()
        refs = cf.oracle_F6(fam, rows)
        G6 = rig.G.clone()
        for i in range(NB):
            out[i]["gw"] = rig.split(G6[i * rig.total:(i + 1) * rig.total])
            worst.add("F6", out[i], refs[i])
        for i in range(NB):
            check_fwd(f"F6 block {i} z", out[i]["z"], refs[i]["z"])
            check_fwd(f"F6 block {i} J", out[i]["J"], refs[i]["J"])
            grads_ok(f"F6 block {i}", out[i], refs[i])
        # F7: the same rows launches, then part B with the step in its reduction.  beta1 = 0, lr = 0, no decay, a clamp far above every
        # gradient: exp_avg = the gradient (hint_adam.hpp: m = 0 m + 1 g), the weights stay
        rows_launches()
        n = NB * rig.total
        P0 = rig.arena.clone()
        M, V = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        rig.G.fill_(7.0)
        opt_state = torch.tensor([0.0, 0.0, 0.95, 0.0, 1.0], device=DEV)
        clamp = 1e30
        assert float(G6[rig.real.repeat(NB)].abs().max()) < clamp
        check(lib.hint_chain_wgrad_adam(h, None, None, rig.arena.data_ptr(), M.data_ptr(), V.data_ptr(), n, opt_state.data_ptr(), 0.0, 0.95, 1e-4,
                                        0.0, 1.0, clamp, st), "hint_chain_wgrad_adam")
        torch.cuda.synchronize()
        real = rig.real.repeat(NB)
        same = torch.equal(M[real], G6[real])
        worst.note("F7", 0.0 if same else float("inf"), "exp_avg")
        assert same, f"F7: exp_avg differs from F6's gradient in {int((M[real] != G6[real]).sum())} elements"
        assert torch.equal(rig.arena, P0), "F7: lr = 0 moved the weights"
        assert bool((rig.G == 7.0).all()), "F7: the gradient arena was written"
        assert bool((M[~real] == 0).all()) and bool((V[~real] == 0).all()), "F7: padding of the moments was stepped"
        return r, dict(G=G6[real], arena=rig.arena, exp_avg=M, exp_avg_sq=V,
                       **{f"{k}{i}": out[i][k] for i in range(NB) for k in ("z", "J", "gx", "gc")})
    finally:
        lib.hint_chain_destroy(h)


RUN = {"F1-F3": ("block", run_block_forms), "F4-F5": ("chain", run_chain_forms), "F6-F7": ("block", run_gathered_forms)}
COMPARES = {"F1": run_block_forms, "F2": run_block_forms, "F3": run_block_forms, "F4": run_chain_forms, "F5": run_chain_forms,
            "F6": run_gathered_forms, "F7": run_gathered_forms}
CASES = [(g, fam.name) for fam in cf.FAMILIES for g, forms in cf.GROUPS.items() if all((f, fam.name) in cf.pairs() for f in forms)]


BITS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_bits.json")
LOSS_SLOTS = 64         # loss_acc: float atomics into this many slots - one summation order only while no two workgroups share a slot


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(lib, group, fam_name, cu):
    """one (group, family) against the oracle -> its record for tests/golden/launch_bits.json"""
    fam = cf.FAMILY[fam_name]
    B = cf.resolve_B(lib, fam, cu)
    rig = Rig(fam, lib, B)
    entry, run = RUN[group]
    rig.assert_dispatch(entry)
    worst = Worst(fam)
    try:
        ins, outs = run(rig, worst)
    finally:
        worst.print()
    if plan_dispatch(lib, rig.plan, B)["grid"] > LOSS_SLOTS:
        outs.pop("loss", None)
    ins = dict(ins, params=rig.arena, **{f"W{i}": w for i, w in enumerate(rig.W)})
    return dict(cu=cu, B=B, lds_fwd=lib.hint_debug_last_lds_bytes(0), lds_bwd=lib.hint_debug_last_lds_bytes(1),
                tape_floats=lib.hint_plan_tape_floats(rig.plan, B), workspace_bytes=int(lib.hint_plan_workspace_bytes(rig.plan, B)),
                inputs={k: sha(v) for k, v in sorted(ins.items())}, outputs={k: sha(v) for k, v in sorted(outs.items()) if v is not None})


@pytest.mark.parametrize("group,fam_name", CASES, ids=[f"{f}-{g}" for g, f in CASES])
def test_call_forms_vs_oracle(group, fam_name):
    torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 oracle: a GPU box has many host cores)
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    with open(BITS_PATH) as f:
        bits = json.load(f)
    want = bits["cases"][f"{group}/{fam_name}"]
    assert cu == want["cu"], (f"{BITS_PATH} was recorded on a device of {want['cu']} CUs and this one has {cu}: batch sizes, grids and "
                              "summation orders follow the CU count, so the recorded bits say nothing here")
    got = run_case(lib, group, fam_name, cu)
    dropped = {k.split(":")[1] for k in bits["dropped"] if k.startswith(f"{group}/{fam_name}:")}
    assert set(got["outputs"]) == set(want["outputs"]) | dropped, (sorted(got["outputs"]), sorted(want["outputs"]), sorted(dropped))
    got["outputs"] = {k: v for k, v in got["outputs"].items() if k not in dropped}
    assert got["inputs"] == want["inputs"], f"{group}/{fam_name}: a generated input drifted: look at tests/call_forms.py, not at the kernels"
    diff = sorted(k for k in want if k != "outputs" and got[k] != want[k]) + sorted(k for k, v in want["outputs"].items() if got["outputs"][k] != v)
    assert not diff, (f"{group}/{fam_name}: not the recorded bits", diff, {k: (got[k], want[k]) for k in diff if k in want})
