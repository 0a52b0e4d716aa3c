"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI by
the module mirror, against (1) the golden vectors of the real reference, (2) the CPU oracle on
fresh seeded inputs, (3) size-independent properties at the BASELINE sizes.

Tolerances (fp32; north_star: log-likelihood within 1e-4 relative): z, J rtol 1e-5 / atol 1e-5
scaled by the tensor's magnitude; gradients 1e-4 relative to the tensor's max-abs (the backward kernels
read the forward's taped activations)."""
import numpy as np
import pytest
import torch

import hint_amd
from oracle import hint_oracle as orc
from util import BLOCK_CASES, case_perms, load_block_case, rel_err, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_block(c, params=None, perms=None):
    blk = hint_amd.HierarchicalAffineCouplingBlock([(c["d"],)], dims_c=c["dims_c"], c_internal=list(c["c_internal"]),
                                                   clamp=c["clamp"], max_splits=c["max_splits"],
                                                   min_split_size=c["min_split_size"],
                                                   reshuffle=c.get("reshuffle", False))
    if params is not None:
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}
        for path, W in (perms or {}).items():          # reshuffle=True fixtures carry the node matrices
            sd[path + ".perm.W"] = torch.from_numpy(np.ascontiguousarray(W))
        blk.load_state_dict(sd)
    return blk.to(DEV)


def kink_distance(nodes, P, x, cond, clamp=4.0):
    """per row: the hidden pre-activation of the float32 oracle closest to zero, relative to the row's largest one"""
    pre = []
    relu = torch.relu

    def spy(t):
        pre.append(t.detach().abs())
        return relu(t)
    torch.relu = spy
    try:
        with torch.no_grad():
            orc.block_apply(nodes, P, x, cond, rev=False, clamp=clamp)
    finally:
        torch.relu = relu
    allp = torch.cat([p.reshape(p.shape[0], -1) for p in pre if p.numel() > 0], dim=1)
    return allp.min(dim=1).values / allp.max(dim=1).values.clamp(min=1.0)


def close(a, b, rtol=1e-5, atol=1e-5):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    scale = max(1.0, float(np.abs(b).max())) if np.size(b) else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: c["name"])
def test_block_vs_reference_golden(case):
    c, nodes, shapes, params, x_np, conds_np, g = load_block_case(case)
    blk = make_block(c, params, case_perms(g))
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    conds = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in conds_np]
    (z,) = blk([x], c=conds)
    J = blk.jacobian(None)
    # how far the float32 reference itself is from the exact result (float64 oracle on the same inputs): for an
    # ill-conditioned block (big_s: scales e^+-4 on |z| ~ 5e3) that is 2e-4 in J, and another float32 evaluation order
    # may deviate from the reference by as much; everywhere else this term is below the 1e-5 floor
    P64 = to_torch(params, torch.float64)
    z64, J64 = orc.block_apply(nodes, P64, torch.from_numpy(x_np).double(), [torch.from_numpy(a).double() for a in conds_np],
                               rev=False, clamp=c["clamp"], perms=({k: torch.from_numpy(v).double() for k, v in case_perms(g).items()} or None))
    ref_z = float(np.abs(z64.numpy() - g["z"]).max()) / max(1.0, float(np.abs(g["z"]).max()))
    ref_J = float(np.abs(J64.numpy() - g["J"]).max()) / max(1.0, float(np.abs(g["J"]).max()))
    close(z, g["z"], atol=max(1e-5, 4 * ref_z))
    close(J, g["J"], atol=max(1e-5, 4 * ref_J))
    L = (0.5 * torch.sum(z ** 2, dim=1) - J).mean()
    assert abs(L.item() - float(g["L"])) <= 1e-4 * abs(float(g["L"]))     # north_star tolerance
    L.backward()
    assert rel_err(x.grad.cpu().numpy(), g["gx"]) < 1e-4
    for i, cc in enumerate(conds):
        assert rel_err(cc.grad.cpu().numpy(), g[f"gc{i}"]) < 1e-4
    named = dict(blk.named_parameters())
    for k in shapes:
        assert rel_err(named[k].grad.cpu().numpy(), g["g:" + k]) < 1e-4, k
    with torch.no_grad():
        (xr,) = blk([z.detach()], c=[cc.detach() for cc in conds], rev=True)
        Jr = blk.jacobian(None)
        (xi,) = blk([x.detach()], c=[cc.detach() for cc in conds], rev=True)
        Ji = blk.jacobian(None)
    # the inverse of an ill-conditioned block (big_s: scales e^+-4 on |z| ~ 5e3) is noise in fp32
    # for the reference too; bound our deviation by the reference's own round-trip error
    ref_rt = float(np.abs(g["x_rec"] - x_np).max())
    ref_jj = float(np.abs(g["J"] + g["J_rev"]).max())
    close(xr, g["x_rec"], rtol=1e-4, atol=max(2e-5, 4 * ref_rt))
    close(Jr, g["J_rev"], atol=max(1e-5, 4 * ref_jj))
    assert rel_err(xi.cpu().numpy(), g["x_inv"]) < 1e-4
    close(Ji, g["J_inv"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("d,widths,dc,B", [
    (6, [140, 70, 35, 17], 0, 4096),      # BASELINE config 2 (one block)
    (8, [128, 64, 32, 16], 0, 1000),      # config 3 shape, ragged batch
    (43, [67, 33, 16, 8], 0, 515),        # config 5 shape
    (100, [224, 112, 56], 0, 130),        # config 4 x-lane block
    (100, [224, 112, 56], 4, 77),         # conditional_recursive_cinn_4 style
    (6, [200, 100, 50, 25], 0, 1),        # single row
    (6, [200, 100, 50, 25], 0, 17),
    (6, [512, 256, 128], 0, 200),         # the reference's *_big configs: h > 384, nets planned one at a time
    (8, [472, 400, 64], 2, 333),          # two split levels, condition
    (5, [385], 0, 64),                    # just over the split threshold, max_splits by list length
    # more row tiles than CUs (B > 16 x 256): the plan variant the launch then picks, every gradient against the oracle
    (6, [140, 70, 35, 17], 0, 4112),
    (6, [140, 70, 35, 17], 0, 8192),
    (8, [128, 64, 32, 16], 0, 8192),
    (43, [67, 33, 16, 8], 0, 6000),
    (8, [64, 32, 16], 3, 5000),
])
def test_block_vs_oracle_seeded(d, widths, dc, B):
    dims_c = [(dc,)] if dc else []
    nodes = orc.build_nodes(d, dims_c, widths)
    P = orc.init_params(nodes, seed=11, scale=None)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, d, generator=gen)
    cond = [torch.randn(B, dc, generator=gen)] if dc else []
    c = dict(d=d, dims_c=dims_c, c_internal=widths, clamp=4.0, max_splits=-1, min_split_size=2)
    blk = make_block(c, {k: v.numpy() for k, v in P.items()})

    def run(x, cond):
        Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        xo = x.clone().requires_grad_(True)
        co = [t.clone().requires_grad_(True) for t in cond]
        zo, Jo = orc.block_apply(nodes, Po, xo, co, rev=False)
        Lo = (0.5 * torch.sum(zo ** 2, dim=1) - Jo).mean()
        Lo.backward()
        blk.zero_grad()
        xg = x.to(DEV).requires_grad_(True)
        cg = [t.to(DEV).requires_grad_(True) for t in cond]
        (z,) = blk([xg], c=cg)
        J = blk.jacobian(None)
        L = (0.5 * torch.sum(z ** 2, dim=1) - J).mean()
        L.backward()
        close(z, zo.detach().numpy())
        close(J, Jo.detach().numpy())
        assert abs(L.item() - Lo.item()) <= 1e-4 * abs(Lo.item())
        return xg, cg, xo, co, Po

    xg, cg, xo, co, Po = run(x, cond)
    row_err = (xg.grad.cpu() - xo.grad).abs().max(dim=1).values / (xo.grad.abs().max() + 1e-30)
    if row_err.max().item() >= 1e-4:
        # A row one of whose hidden pre-activations rounds to the other side of zero than in the float32 oracle gets the
        # other ReLU subgradient (either is correct).  Accept at most KINK_ROWS such rows, each verified to sit within
        # KINK_EPS of a kink in the oracle, and compare everything again without them.
        KINK_ROWS, KINK_EPS = 3, 1e-5
        bad = torch.nonzero(row_err > 3e-5).flatten()
        dist = kink_distance(nodes, P, x, cond)
        print(f"rows off in g_x: {[(int(i), float(row_err[i]), float(dist[i])) for i in bad]}")
        assert 0 < len(bad) <= KINK_ROWS and all(dist[i].item() <= KINK_EPS for i in bad), \
            [(int(i), float(row_err[i]), float(dist[i])) for i in bad[:10]]
        keep = torch.ones(B, dtype=torch.bool)
        keep[bad] = False
        xg, cg, xo, co, Po = run(x[keep], [t[keep] for t in cond])
    assert rel_err(xg.grad.cpu().numpy(), xo.grad.numpy()) < 1e-4
    for a, b in zip(cg, co):
        assert rel_err(a.grad.cpu().numpy(), b.grad.numpy()) < 1e-4
    named = dict(blk.named_parameters())
    for k, p in Po.items():
        assert rel_err(named[k].grad.cpu().numpy(), p.grad.numpy()) < 2e-4, k


@pytest.mark.parametrize("d,widths,B", [(6, [140, 70, 35, 17], 4096), (8, [128, 64, 32, 16], 8192),
                                        (43, [67, 33, 16, 8], 4096), (6, [512, 256, 128], 1000)])
def test_full_size_properties(d, widths, B):
    """encode -> decode round trip, J_fwd + J_rev = 0, row independence: a row's result does not depend on where in
    the batch it sits (bit-identical), nor - up to the summation order of the K-split, which differs between the
    8-wavefront plan of batches up to 16 rows x CUs and the 4-wavefront plan of larger ones - on the batch size."""
    torch.manual_seed(0)
    blk = hint_amd.HierarchicalAffineCouplingBlock([(d,)], c_internal=widths).to(DEV)
    x = torch.randn(B, d, device=DEV)
    with torch.no_grad():
        (z,) = blk([x]); J = blk.jacobian(None)
        (xr,) = blk([z], rev=True); Jr = blk.jacobian(None)
        (z_small,) = blk([x[37:101]]); J_small = blk.jacobian(None)
        (z_roll,) = blk([x.roll(48, 0)]); J_roll = blk.jacobian(None)
    assert (xr - x).abs().max().item() < 1e-4
    assert (J + Jr).abs().max().item() < 1e-4
    assert torch.equal(z_roll.roll(-48, 0), z) and torch.equal(J_roll.roll(-48, 0), J)
    if B <= 4096:
        assert torch.equal(z[37:101], z_small) and torch.equal(J[37:101], J_small)
    else:
        assert (z[37:101] - z_small).abs().max().item() < 2e-6 * max(1.0, z_small.abs().max().item())
        assert (J[37:101] - J_small).abs().max().item() < 2e-6 * max(1.0, J_small.abs().max().item())


def test_parameter_rebinding_and_empty_batch():
    """train_unconditional.py:165-167 rebinds p.data; the arena must follow."""
    c = dict(d=6, dims_c=[], c_internal=[32, 16], clamp=4.0, max_splits=-1, min_split_size=2)
    blk = make_block(c)
    x = torch.randn(64, 6, device=DEV)
    with torch.no_grad():
        (z0,) = blk([x])
        for p in blk.parameters():
            p.data = 0.005 * torch.randn_like(p.data)
        (z1,) = blk([x])
    assert not torch.allclose(z0, z1)
    nodes = orc.build_nodes(6, (), [32, 16])
    P = {k: v.cpu() for k, v in blk.state_dict().items()}
    zo, _ = orc.block_apply(nodes, P, x.cpu(), (), rev=False)
    close(z1, zo.numpy())
    with torch.no_grad():
        (ze,) = blk([torch.empty(0, 6, device=DEV)])
    assert ze.shape == (0, 6) and blk.jacobian(None).shape == (0,)


def test_persistent_tile_loop_large_batch():
    """more row-tile pairs than the launch has workgroups (grid is capped at 8 per CU): the wave-local kernels go round
    their tile loop twice, the second pass ragged, re-using the LDS tables and prefetching the first group's lists again
    (B follows the CU count; hint_plan_dispatch shows the passes before anything is compared)"""
    from instance_cases import multi_pass_b, plan_dispatch
    torch.manual_seed(1)
    d, widths = 6, [24, 12]
    B = multi_pass_b(torch.cuda.get_device_properties(0).multi_processor_count, 2)
    blk = hint_amd.HierarchicalAffineCouplingBlock([(d,)], c_internal=widths).to(DEV)
    disp = plan_dispatch(blk.tree.engine(torch.device(DEV)).lib, blk.tree.engine(torch.device(DEV)).plan, B)
    assert disp["passes"] >= 2 and disp["groups"] % disp["grid"] != 0, disp
    x = torch.randn(B, d, device=DEV)
    nodes = orc.build_nodes(d, (), widths)
    P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    xo = x.cpu().clone().requires_grad_(True)
    zo, Jo = orc.block_apply(nodes, P, xo, (), rev=False)
    Lo = (0.5 * (zo ** 2).sum(1) - Jo).mean()
    Lo.backward()
    xg = x.clone().requires_grad_(True)
    (z,) = blk([xg]); J = blk.jacobian(None)
    L = (0.5 * (z ** 2).sum(1) - J).mean()
    L.backward()
    close(z, zo.detach().numpy())
    close(J, Jo.detach().numpy())
    assert rel_err(xg.grad.cpu().numpy(), xo.grad.numpy()) < 1e-4
    named = dict(blk.named_parameters())
    for k, p in P.items():
        assert rel_err(named[k].grad.cpu().numpy(), p.grad.numpy()) < 2e-4, k
    with torch.no_grad():
        (xr,) = blk([z.detach()], rev=True)
    assert (xr - x).abs().max().item() < 1e-4
