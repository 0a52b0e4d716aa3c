"""The planner's fallback plans and the row kernels' size limits against the float64 oracle (oracle/hint_oracle.py), one case of the
path ledger at a time (tests/plan_path_cases.py; tests/test_plan_paths_cpu.py checks the ledger without a GPU).

Per case: hint_plan_paths on the live plan must return the declared path tuple and hint_plan_dispatch the declared wavefront
variant before anything is compared - a device with another CU count fails here instead of testing something else.  Then what
run_block / run_chain of tests/test_gpu_instances.py do, with that file's metrics and tolerances: forward z and J, inverse x and J,
d/dx, d/dc and every weight-gradient tensor under random per-row cotangents g_z, g_J.  The rows are the case's kink-free rows (no
row is waived).  The r = 128 coupling goes through the oracle node of test_gpu_conditional.oracle_nodes and has its inverse
differentiated as well, at the bounds of tests/test_gpu_inverse_grad.py."""
import pytest
import torch

import hint_amd
from hint_amd import _lib
from instance_cases import plan_dispatch
from plan_path_cases import (CASES, INV_TOL_G, INV_TOL_W, INV_TOL_X, PATHS, fwd_shares, grad_shares, inv_grad_shares, module_of,
                             plan_paths, prepared)
from test_gpu_instances import TOL_FWD, TOL_GW, TOL_GX, Spy, check_fwd, check_grads, err, make_chain_pair  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_paths(case, lib, plan, B):
    got = plan_paths(lib, plan, B)
    disp = plan_dispatch(lib, plan, B)
    print(f"{case.name}: B={B} on {disp['num_cu']} CUs: nw={disp['nw']} variant={disp['alt4']} grid={disp['grid']} "
          f"passes={disp['passes']} paths={dict(zip(PATHS, got))}")
    assert got == tuple(case.paths), f"{case.name}: the plan reaches {got}, declared {tuple(case.paths)}"
    assert disp["nw"] == case.nw and disp["alt4"] == (1 if case.nw == 4 else 0), (case.name, disp["nw"], disp["alt4"], case.nw)


def report(case, fig, shares):
    worst = max(shares, key=shares.get)
    print(f"{case.name}: {fig['discarded']} of {fig['pool']} candidates next to a ReLU kink discarded; worst error against float64 "
          f"as a share of its tolerance: {shares[worst]:.3f} ({worst})")


def loaded(case, P):
    mod = module_of(case)
    mod.load_state_dict(P)
    return mod.to(DEV)


def run_block(case, lib, cu):
    m, rows, ref, fig = prepared(case, cu)
    B = case.B(cu)
    blk = loaded(case, m.P)
    assert_paths(case, lib, blk.tree.engine(torch.device(DEV)).plan, B)
    xd = rows["x"].to(DEV).requires_grad_(True)
    cd = [rows["c"].to(DEV).requires_grad_(True)] if case.dc else []
    (z,) = blk([xd], c=cd)
    J = blk.jacobian(None)
    check_fwd("z", z, ref["z"])
    check_fwd("J", J, ref["J"])
    ((z * rows["gz"].to(DEV)).sum() + (J * rows["gJ"].to(DEV)).sum()).backward()
    named = dict(blk.named_parameters())
    got = dict(z=z, J=J, gx=xd.grad, gc=cd[0].grad if case.dc else None, gw={k: named[k].grad for k in ref["gw"]})
    check_grads(case.name, got["gx"], got["gc"], got["gw"], ref)
    with torch.no_grad():
        (xi,) = blk([rows["zi"].to(DEV)], c=[t.detach() for t in cd], rev=True)
        Ji = blk.jacobian(None)
    check_fwd("inverse x", xi, ref["xi"])
    check_fwd("inverse J", Ji, ref["Ji"])
    got.update(xi=xi, Ji=Ji)
    shares = dict(fwd_shares(got, ref))
    shares.update(grad_shares(got, ref))
    if case.entry == "coupling":
        shares.update(run_inverse_grads(case, m, rows, ref["inv"]))
    report(case, fig, shares)


def run_inverse_grads(case, m, rows, ref):
    """the inverse under autograd on a module of its own (the same weights): x, d/dz, d/dc and every weight tensor"""
    mod = loaded(case, m.P)
    zd = rows["zi"].to(DEV).requires_grad_(True)
    cd = rows["c"].to(DEV).requires_grad_(True)
    (x,) = mod([zd], c=[cd], rev=True)
    J = mod.jacobian(None, rev=True)
    check_fwd("inverse J", J, ref["J"])
    ((x * rows["gz"].to(DEV)).sum() + (J * rows["gJ"].to(DEV)).sum()).backward()
    assert err(x, ref["out"]) < INV_TOL_X
    assert err(zd.grad, ref["gx"]) < INV_TOL_G, ("inverse d/dz", err(zd.grad, ref["gx"]))
    assert err(cd.grad, ref["gc"]) < INV_TOL_G, ("inverse d/dc", err(cd.grad, ref["gc"]))
    named = dict(mod.named_parameters())
    for k, r in ref["gw"].items():
        assert err(named[k].grad, r) < INV_TOL_W, ("inverse", k, err(named[k].grad, r))
    return inv_grad_shares(dict(out=x, gx=zd.grad, gc=cd.grad, gw={k: named[k].grad for k in ref["gw"]}), ref)


def run_chain(case, lib, cu):
    m, rows, ref, fig = prepared(case, cu)
    B = case.B(cu)
    _, flow = make_chain_pair(case)
    for i, blk in enumerate(flow.blocks):          # (the ledger's model is the flow make_chain_pair builds)
        for k, v in blk.state_dict().items():
            if (i, k) in m.P:
                assert torch.equal(v.cpu(), m.P[(i, k)]), (i, k)
    tr = hint_amd.FlowTrainer(flow, noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    chain = tr._chain_for(B)
    assert_paths(case, lib, tr.engines[0].plan, B)
    st = torch.cuda.current_stream().cuda_stream
    xd = rows["x"].to(DEV)
    cd = rows["c"].to(DEV) if case.dc else None
    cp = cd.data_ptr() if case.dc else None
    z, J = torch.empty_like(xd), torch.empty(B, device=DEV)
    _lib.check(lib.hint_chain_forward(chain, xd.data_ptr(), cp, z.data_ptr(), J.data_ptr(), None, None, st), "hint_chain_forward")
    gx = torch.empty_like(xd)
    gc = torch.zeros_like(cd) if case.dc else None
    gzd, gJd = rows["gz"].to(DEV).contiguous(), rows["gJ"].to(DEV).contiguous()
    _lib.check(lib.hint_chain_backward(chain, xd.data_ptr(), cp, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(),
                                       gc.data_ptr() if case.dc else None, 1.0, 0.0, 0, st), "hint_chain_backward")
    torch.cuda.synchronize()
    check_fwd("z", z, ref["z"])
    check_fwd("J", J, ref["J"])
    gw = {}
    for bi, ((a, b), eng) in enumerate(zip(tr.slices, tr.engines)):
        for p, g in zip(eng.params, eng.split_flat(tr.G[a:b])):
            name = [n for n, q in flow.blocks[bi].named_parameters() if q is p][0]
            gw[(bi, name)] = g
    check_grads(case.name, gx, gc, gw, ref)
    with torch.no_grad():
        xi, Ji = tr.sample(rows["zi"].to(DEV), cd)
    check_fwd("inverse x", xi, ref["xi"])
    check_fwd("inverse J", Ji, ref["Ji"])
    got = dict(z=z, J=J, xi=xi, Ji=Ji, gx=gx, gc=gc, gw=gw)
    shares = dict(fwd_shares(got, ref))
    shares.update(grad_shares(got, ref))
    report(case, fig, shares)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_plan_path_vs_oracle(case):
    torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 oracle: a GPU box has many host cores)
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    (run_chain if case.entry == "chain" else run_block)(case, lib, cu)
