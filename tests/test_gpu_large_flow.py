"""The flow kernels with a tape past 2^31 floats: one case per row-kernel family (tests/large_cases.py FLOW_CASES), each on its
ledger tree (tests/instance_cases.py) as one block through hint_block_pack / forward / backward / inverse.

B is the smallest batch for which hint_plan_tape_floats(plan, B) > 2^31, found by bisection on the device plan, rounded up to the
row tile, plus 5.  x, c and the inverse's z are seeded and generated on the device; the cotangents g_z, g_J are non-zero on the
probe rows only, so g_x, g_c and every weight gradient of the whole batch are those of the probe rows alone, and the float64
oracle (oracle_block_rows of tests/test_gpu_instances.py, at that file's tolerances) runs on a few hundred rows.  Probe rows: head,
ragged tail, a picket, and both sides of the rows at which a tape section's float index crosses 2^29 and 2^30 (the 2^31 crossing
lies in the last rows' share of the tape: the tail).  A probe row next to a ReLU kink keeps zero cotangents, as in the ledger,
and its successor joins the probe rows in its place; the share must stay within the family's kink_cap.  Every output, the tape,
the workspace and the gradient sit between guards and hold the NaN pattern before the call."""
import ctypes as C
import time

import pytest
import torch

from hint_amd import _lib
import instance_cases as ic
import large_cases as lc
import poison_cases as pc
from guarded import NAN_BITS, Guarded
from test_gpu_instances import TOL_FWD, TOL_GW, TOL_GX, block_params, oracle_block_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def close_fwd(what, got, ref):
    d = float((got.double().cpu() - ref).abs().max())
    assert d <= TOL_FWD * max(1.0, float(ref.abs().max())), (what, d, float(ref.abs().max()))
    return d / max(1.0, float(ref.abs().max()))


def nan_free(bufs, name, n):
    bufs[name] = Guarded(n, fill="nan")
    return bufs[name]


def rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("family", list(lc.FLOW_CASES))
def test_block_with_a_tape_past_2_31_floats(family):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    case = lc.ledger_case(family)
    lib, st, t0, bufs = _lib.load(), pc.stream(), time.time(), {}
    d, dc = case.d, case.dc
    blk, eng, layout = pc.descs_and_plan(lib, d, dc, case.widths)
    plan, total = eng.plan, eng.total
    nr = ic.plan_dispatch(lib, plan, 1 << 21)["nr"]
    B, first = lc.flow_batch(lambda b: lib.hint_plan_tape_floats(plan, b), nr)
    tape_n, ws_bytes = lib.hint_plan_tape_floats(plan, B), int(lib.hint_plan_workspace_bytes(plan, B))
    assert tape_n > lc.EDGE and lib.hint_plan_tape_floats(plan, first - 1) <= lc.EDGE and B % (16 * nr) == 5
    disp = ic.plan_dispatch(lib, plan, B)
    want = tuple(s.replace(", true>", ", false>") for s in case.expect) if family == "wave_local" else case.expect
    assert ic.instances_of(disp, "block") == want, (ic.instances_of(disp, "block"), want)
    assert disp["passes"] >= 2
    stats = (C.c_int64 * 16)()
    descs, n_nodes = ic.descs_for(d, dc, case.widths)
    assert lib.hint_plan_check(descs, n_nodes, d, dc, 4.0, stats) == 0
    L, WT = int(stats[1]), int(stats[2])
    assert lc.tape_floats_predicted(L, d, WT, disp["lean"], B) == tape_n                      # the layout the probe rows are laid on
    cross = lc.flow_crossings(lc.tape_sections(L, d, WT, disp["lean"], B), B)
    print(f"{family}: B {B}, tape {tape_n} floats, workspace {ws_bytes} bytes ({ws_bytes // 4} floats, "
          f"{'past' if ws_bytes // 4 > lc.EDGE else 'below'} 2^31), crossings {cross}, passes {disp['passes']}")
    peak = 4 * tape_n + ws_bytes + 4 * B * (6 * d + 2 * dc + 4) + lc.SLACK
    assert peak <= lc.CAP
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < peak:
        pytest.skip(f"{family}: needs {peak / lc.GIB:.1f} GiB of device memory, {free / lc.GIB:.1f} GiB are free")
    try:
        g = gen(11)
        x = bufs["x"] = torch.randn(B, d, generator=g, device=DEV)
        c = bufs["c"] = torch.randn(B, dc, generator=g, device=DEV) if dc else None
        zi = bufs["zi"] = torch.randn(B, d, generator=g, device=DEV)
        nodes, P = block_params(case)
        hg = torch.Generator().manual_seed(12)

        def take(rows):
            rt = torch.tensor(rows, device=DEV)
            n = len(rows)
            return (x[rt].cpu(), c[rt].cpu() if dc else None, zi[rt].cpu(), torch.randn(n, d, generator=hg), torch.randn(n, generator=hg))
        rows = lc.probe_rows(B, d, crossings=sorted(cross.values()))
        _, keep, _, _ = oracle_block_rows(case, nodes, P, take(rows))                         # the oracle decides beforehand
        kinked = [r for r, k in zip(rows, keep.tolist()) if not k]
        rows = sorted(set(rows) | {r + 1 for r in kinked if r + 1 < B})
        host_rows = take(rows)
        (_, _, _, gz_r, gJ_r), keep, _, ref = oracle_block_rows(case, nodes, P, host_rows)
        dropped = len(rows) - int(keep.sum())
        print(f"{family}: {len(rows)} probe rows, {dropped} next to a ReLU kink (zero cotangents)")
        assert dropped <= case.kink_cap * len(rows)
        rt = torch.tensor(rows, device=DEV)
        gz = bufs["gz"] = torch.zeros(B, d, device=DEV)
        gJ = bufs["gJ"] = torch.zeros(B, device=DEV)
        gz[rt], gJ[rt] = gz_r.to(DEV), gJ_r.to(DEV)

        params = bufs["params"] = Guarded(total)
        for name, off, n in layout:
            params.words[off:off + n].copy_(P[name].reshape(-1).to(DEV).view(torch.int32))
        A = lambda name, n: bufs.setdefault(name, Guarded(n, fill="nan"))                     # noqa: E731
        packed = A("packed", lib.hint_plan_packed_floats(plan))
        z, J, xi, Ji, gx = A("z", B * d), A("J", B), A("xi", B * d), A("Ji", B), A("gx", B * d)
        gc_ = A("gc", B * dc) if dc else None
        tape, ws, gp = A("tape", tape_n), A("workspace", ws_bytes // 4), A("g_params", total)
        cp = c.data_ptr() if dc else None
        pc.check(lib.hint_block_pack(plan, params.ptr, packed.ptr, st), "hint_block_pack")
        pc.check(lib.hint_block_forward(plan, params.ptr, packed.ptr, x.data_ptr(), cp, z.ptr, J.ptr, tape.ptr, B, st),
                 "hint_block_forward")
        pc.check(lib.hint_block_backward(plan, params.ptr, packed.ptr, x.data_ptr(), tape.ptr, cp, gz.data_ptr(), gJ.data_ptr(),
                                         gx.ptr, gc_.ptr if dc else None, gp.ptr, 0, ws.ptr, ws_bytes, B, st), "hint_block_backward")
        pc.check(lib.hint_block_inverse(plan, params.ptr, packed.ptr, zi.data_ptr(), cp, xi.ptr, Ji.ptr, B, st), "hint_block_inverse")
        torch.cuda.synchronize()
        for name, b in bufs.items():
            if isinstance(b, Guarded):
                b.check_guards(f"{family}: {name}")
        for name in ("z", "J", "xi", "Ji", "gx") + (("gc",) if dc else ()):
            left = lc.count_words(bufs[name].words, NAN_BITS)
            assert left == 0, f"{family}: {left} words of {name} were never written"
        worst = dict(z=close_fwd("z", z.view(B, d)[rt], ref["z"]), J=close_fwd("J", J.view(B)[rt], ref["J"]),
                     xi=close_fwd("inverse x", xi.view(B, d)[rt], ref["xi"]), Ji=close_fwd("inverse J", Ji.view(B)[rt], ref["Ji"]))
        gxv = gx.view(B, d)
        worst["gx"] = rel(gxv[rt], ref["gx"])
        assert worst["gx"] <= TOL_GX, ("d/dx", worst["gx"])
        if dc:
            worst["gc"] = rel(gc_.view(B, dc)[rt], ref["gc"])
            assert worst["gc"] <= TOL_GX, ("d/dc", worst["gc"])
        other = torch.ones(B, dtype=torch.bool, device=DEV)
        other[rt] = False
        for name, t in (("gx", gxv),) + ((("gc", gc_.view(B, dc)),) if dc else ()):           # zero cotangents: exactly zero
            assert not bool(((t != 0).any(dim=1) & other).any()), f"{family}: {name} of a row without cotangents is not zero"
        gmax = max(float(v.abs().max()) for v in ref["gw"].values())
        flat = gp.t
        worst["gw"] = 0.0
        for name, off, n in layout:
            r = ref["gw"][name]
            e = float((flat[off:off + n].double().cpu().reshape(r.shape) - r).abs().max())
            assert e <= TOL_GW * float(r.abs().max()) + 1e-7 * gmax, (family, name, e, float(r.abs().max()))
            worst["gw"] = max(worst["gw"], e / max(float(r.abs().max()), 1e-30))
        print(f"{family}: {time.time() - t0:.1f} s; worst errors " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    finally:
        lc.release(bufs)


@pytest.mark.timeout(240)
def test_trainer_loss_sums_at_a_tape_past_2_31_floats():
    """one FlowTrainer._fwd_bwd (noise = 0, lr = 0) of the wave-local tree at the same B, through the chain entry points (the
    chain instances of the wave-local kernels; one block with its permutation - the two tapes and workspaces of a chain of 2
    are 32 GB): the two loss sums equal the float64 sums of the chain forward's own z and J to 1e-5 relative, the fp32
    accumulation bound of the 64 loss slots.  The in-kernel noise is not probed here: its element index is B d = 1.8e7 at this
    B, far from 2^31 (a tape of 1 TB would be needed to reach it)."""
    import hint_amd
    case = lc.ledger_case("wave_local")
    lib, bufs = _lib.load(), {}
    torch.manual_seed(0)
    flow = hint_amd.HintFlow(case.d, 1, list(case.widths), perm_first=True).to(DEV)
    for p in flow.parameters():
        p.data.mul_(0.3)
    tr = hint_amd.FlowTrainer(flow, noise=0.0, use_graph=False, lr=0.0)
    assert tr._chainable
    plan = tr.engines[0].plan
    B, _ = lc.flow_batch(lambda b: lib.hint_plan_tape_floats(plan, b), ic.plan_dispatch(lib, plan, 1 << 21)["nr"])
    tape_n, ws_bytes = lib.hint_plan_tape_floats(plan, B), int(lib.hint_plan_workspace_bytes(plan, B))
    assert tape_n > lc.EDGE
    disp = ic.plan_dispatch(lib, plan, B)
    assert ic.instances_of(disp, "chain") == case.expect, (ic.instances_of(disp, "chain"), case.expect)
    peak = 4 * tape_n + ws_bytes + 4 * B * (4 * case.d + 2) + lc.SLACK
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < peak:
        pytest.skip(f"trainer: needs {peak / lc.GIB:.1f} GiB of device memory, {free / lc.GIB:.1f} GiB are free")
    try:
        x = bufs["x"] = torch.randn(B, case.d, generator=gen(21), device=DEV)
        tr._check_arenas()
        tr.G.zero_()
        tr._fwd_bwd(x, None)
        torch.cuda.synchronize()
        s = tr.loss_acc.double().sum(dim=0).cpu()
        G = tr.G.clone()
        assert bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
        # the same forward once more, into buffers of the test's own: z, J and the loss sums of one launch
        chain = tr._chain_for(B)
        z, J = nan_free(bufs, "z", B * case.d), nan_free(bufs, "J", B)
        acc = bufs["acc"] = torch.zeros_like(tr.loss_acc)
        pc.check(lib.hint_chain_forward(chain, x.data_ptr(), None, z.ptr, J.ptr, None, acc.data_ptr(), pc.stream()), "hint_chain_forward")
        torch.cuda.synchronize()
        z.check_guards("trainer: z")
        J.check_guards("trainer: J")
        assert lc.count_words(z.words, NAN_BITS) == 0 and lc.count_words(J.words, NAN_BITS) == 0
        s2 = acc.double().sum(dim=0).cpu()
        want = (0.5 * float((z.t.double() ** 2).sum()), float(J.t.double().sum()))             # (B d = 1.8e7 doubles: 146 MB)
        print(f"trainer: B {B}, loss sums {s.tolist()}, again {s2.tolist()}, float64 of z and J {want}")
        for got in (s, s2):
            assert abs(float(got[0]) - want[0]) <= 1e-5 * abs(want[0]) and abs(float(got[1]) - want[1]) <= 1e-5 * abs(want[1])
        with torch.no_grad():                                                                # rows of the inference route: the same z
            rows = lc.probe_rows(B, case.d)
            rt = torch.tensor(rows, device=DEV)
            zs = flow(x[rt].contiguous())
            Js = flow.log_jacobian(run_forward=False)
        assert float((zs - z.view(B, case.d)[rt]).abs().max()) <= TOL_FWD * max(1.0, float(zs.abs().max()))
        assert float((Js - J.view(B)[rt]).abs().max()) <= TOL_FWD * max(1.0, float(Js.abs().max()))
    finally:
        tr = flow = chain = None                          # the chain's tape and workspace go with the trainer
        lc.release(bufs)

