"""Weight gradients at every batch-split geometry of backward part B against the float64 oracle (oracle/hint_oracle.py), one tree's
worth of one target family per test (tests/wgrad_geometry.py; tests/test_wgrad_geometry_cpu.py checks that ledger without a GPU).

Per test: the family's targets are resolved for the device's CU count, and per batch size hint_plan_dispatch on the real plan must
show the declared dw_splits, dw_rows and grid before anything is compared.  Then z, J, d/dx, d/dc and every weight-gradient tensor
under random per-row cotangents g_z, g_J, with check_fwd / check_grads and the tolerances of tests/test_gpu_instances.py.  One
16-row step dropped or counted twice moves every gradient tensor by more than 20 times its bound even at the largest batch used here
(test_one_step_is_far_over_the_bound in the CPU test), a single row the median tensor by 28 .. 190 times.

Rows: one pool per tree (and per chain length), every batch a prefix of it, so batches differ in length alone.  No row is waived:
candidates whose float64 pre-activations come within KINK of a ReLU kink (the Spy rule; for chains over the whole chain) are
discarded before the pool is used - at most the ledger's cap of them - and the others kept in order, so every row of every batch
carries non-zero cotangents.  The oracle runs once per pool: its rows' weight gradients are added up in float64 from one batch size
to the next.  The batch sizes of one block object run from the largest to the smallest: where a tape or a workspace is used again,
finite stale rows of the larger batch lie behind the live ones (the NaN-poison tests do not model that)."""
import functools

import pytest
import torch

import hint_amd
from hint_amd import _lib
import wgrad_geometry as wg
from instance_cases import instances_of, plan_dispatch
from oracle import hint_oracle as orc
from test_gpu_instances import KINK, TOL_FWD, TOL_GW, TOL_GX, Spy, check_fwd, check_grads, err      # noqa: F401 (imported, not restated)

DEV = "cuda:0"
SEED = 11
SENTINEL = 12345.0


# ------------------------------------------------------------------------------------------------------- pool and oracle
def _forward64(tree, n_blocks, P64, perms, x64, c64):
    """float64 forward of one block (n_blocks = 0) or of a chain with a permutation in front of every block"""
    nodes = orc.build_nodes(tree.d, [(tree.dc,)] if tree.dc else [], list(tree.widths))
    cl = [c64] if tree.dc else []
    if n_blocks == 0:
        return orc.block_apply(nodes, P64[0], x64, cl, rev=False)
    J = torch.zeros(x64.shape[0], dtype=torch.float64)
    for P, W in zip(P64, perms):
        x64, Ji = orc.block_apply(nodes, P, x64 @ W, cl, rev=False)
        J = J + Ji
    return x64, J


def make_params(tree, n_blocks):
    """float32 weights of every block, and the chain's float32 permutation matrices (one in front of EVERY block)"""
    nodes = orc.build_nodes(tree.d, [(tree.dc,)] if tree.dc else [], list(tree.widths))
    P = [orc.init_params(nodes, seed=5 + 1000 * i, scale=tree.scale) for i in range(max(n_blocks, 1))]
    perms = [orc.random_orthogonal(tree.d, seed=21 + i) for i in range(n_blocks)]
    return P, perms


@functools.lru_cache(maxsize=4)
def pool(tree_name, n_blocks, n_rows):
    """n_rows kink-free rows (x, c, g_z, g_J) of the tree's pool: candidates are drawn once, those next to a ReLU kink in the float64
    oracle discarded (at most the cap), the first n_rows of the others kept in order"""
    tree = wg.TREE[tree_name]
    cap = wg.chain_kink_cap(tree, n_blocks) if n_blocks else tree.kink_cap
    N = int(n_rows / (1.0 - cap)) + 16
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(N, tree.d, generator=g)
    c = torch.randn(N, tree.dc, generator=g) if tree.dc else None
    gz = torch.randn(N, tree.d, generator=g)
    gJ = torch.randn(N, generator=g)
    P, perms = make_params(tree, n_blocks)
    with torch.no_grad(), Spy(N) as spy:
        _forward64(tree, n_blocks, [{k: v.double() for k, v in p.items()} for p in P], [w.double() for w in perms], x.double(),
                   c.double() if tree.dc else None)
    keep = spy.kink > KINK
    dropped = N - int(keep.sum())
    print(f"{tree_name} ({n_blocks or 1} block(s)): {dropped} of {N} candidates next to a ReLU kink discarded ({dropped / N:.1%}, cap {cap:.1%})")
    assert dropped <= cap * N, f"{tree_name}: {dropped} of {N} candidates next to a ReLU kink (cap {cap:.1%})"
    idx = torch.nonzero(keep)[:n_rows, 0]
    assert idx.numel() == n_rows
    x, gz, gJ = x[idx].contiguous(), gz[idx].contiguous(), gJ[idx].contiguous()
    c = c[idx].contiguous() if tree.dc else None
    assert bool((gz.abs().sum(dim=1) > 0).all()) and bool((gJ != 0).all())         # every row carries non-zero cotangents
    return x, c, gz, gJ, dropped / N


def oracle_prefixes(tree, n_blocks, rows, sizes):
    """{B: reference of the batch rows[:B]} for every B of `sizes`: z, J, d/dx, d/dc row by row from one pass over the pool, the
    weight gradients added up in float64 over the rows between one size and the next"""
    x, c, gz, gJ = rows
    P, perms = make_params(tree, n_blocks)
    P64 = [{k: v.double().requires_grad_(True) for k, v in p.items()} for p in P]
    W64 = [w.double() for w in perms]
    sizes = sorted(set(sizes))
    out, parts, cum, lo = {}, [], None, 0
    for B in sizes:
        xs = x[lo:B].double().requires_grad_(True)
        cs = c[lo:B].double().requires_grad_(True) if tree.dc else None
        z, J = _forward64(tree, n_blocks, P64, W64, xs, cs)
        leaves = [p for Pb in P64 for p in Pb.values()]
        grads = torch.autograd.grad((z * gz[lo:B].double()).sum() + (J * gJ[lo:B].double()).sum(), [xs] + ([cs] if tree.dc else []) + leaves)
        parts.append((z.detach(), J.detach(), grads[0], grads[1] if tree.dc else None))
        gw = grads[2 if tree.dc else 1:]
        cum = list(gw) if cum is None else [a + b for a, b in zip(cum, gw)]
        keys = [(i, k) if n_blocks else k for i, Pb in enumerate(P64) for k in Pb]
        out[B] = dict(gw=dict(zip(keys, cum)))
        lo = B
    z, J, gx, gc = (torch.cat([p[j] for p in parts]) if parts[0][j] is not None else None for j in range(4))
    for B, ref in out.items():
        ref.update(z=z[:B], J=J[:B], gx=gx[:B], gc=gc[:B] if tree.dc else None)
    return P, perms, out


# ------------------------------------------------------------------------------------------------------------ GPU side
class Worst:
    """worst relative error per quantity over the batches of a test, with the B where it occurred"""

    def __init__(self, name):
        self.name, self.w = name, {}

    def add(self, what, e, B):
        if e >= self.w.get(what, (-1.0, 0))[0]:
            self.w[what] = (e, B)

    def record(self, B, z, J, gx, gc, gw, ref):
        """the figures first (they are printed whatever happens next), then the assertions"""
        self.add("z", float((z.detach().double().cpu() - ref["z"]).abs().max()) / max(1.0, float(ref["z"].abs().max())), B)
        self.add("J", float((J.detach().double().cpu() - ref["J"]).abs().max()) / max(1.0, float(ref["J"].abs().max())), B)
        self.add("d/dx", err(gx, ref["gx"]), B)
        if gc is not None:
            self.add("d/dc", err(gc, ref["gc"]), B)
        gmax = max(float(v.abs().max()) for v in ref["gw"].values())
        for k, r in ref["gw"].items():
            # (the same measure check_grads bounds: the error over TOL_GW |r|max + 1e-7 gmax is at most 1 when it passes)
            e = float((gw[k].detach().double().cpu() - r).abs().max())
            self.add("dW (of its bound)", e / (TOL_GW * float(r.abs().max()) + 1e-7 * gmax), B)
            self.add("dW", e / max(float(r.abs().max()), 1e-30), B)

    def print(self):
        print(f"{self.name}: worst " + "; ".join(f"{k} {e:.2e} at B={B}" for k, (e, B) in self.w.items())
              + f"  (bounds: z, J {TOL_FWD:g}; d/dx, d/dc {TOL_GX:g}; dW {TOL_GW:g} + floor)")


def assert_geometry(geo, lib, plan, cu):
    """dispatch before comparison: the real plan shows the declared split, rows per split and grid, and the tree's part-B instance"""
    disp = plan_dispatch(lib, plan, geo.B)
    assert disp["num_cu"] == cu
    assert instances_of(disp, "block")[3] == geo.tree.dw, (geo.id, instances_of(disp, "block")[3], geo.tree.dw)
    if geo.n_chain > 1:
        # (hint_plan_dispatch reports one block's split: a chain's is the ledger's, resolved for this device - wgrad_geometry.Dispatcher;
        #  the rest of the decision is the real plan's)
        assert (disp["grid"], disp["wl"]) == (geo.grid, geo.wl), (geo.id, disp)
        m = wg.check(lib, geo, cu)
    else:
        m = geo.mismatch(disp)
    assert m is None, m
    (f0, f1) = geo.steps
    print(f"{geo.id}: B={geo.B} on {cu} CUs: splits={geo.splits} rows_per_wg={geo.rows} steps {f0} / {f1} grid={geo.grid} {geo.map}")


def make_block(tree, P):
    blk = hint_amd.HierarchicalAffineCouplingBlock([(tree.d,)], dims_c=[(tree.dc,)] if tree.dc else [], c_internal=list(tree.widths))
    blk.load_state_dict(P)
    return blk.to(DEV)


def run_block_batch(tree, blk, rows, B, clear=True):
    """forward and backward of rows[:B] through the module route -> (z, J, d/dx, d/dc, {name: weight gradient})"""
    x, c, gz, gJ = rows
    if clear:
        for p in blk.parameters():
            p.grad = None
    xd = x[:B].to(DEV).requires_grad_(True)
    cd = [c[:B].to(DEV).requires_grad_(True)] if tree.dc else []
    (z,) = blk([xd], c=cd)
    J = blk.jacobian(None)
    ((z * gz[:B].to(DEV)).sum() + (J * gJ[:B].to(DEV)).sum()).backward()
    return z, J, xd.grad, cd[0].grad if tree.dc else None, {k: p.grad for k, p in blk.named_parameters()}


def run_blocks(tree, geos, lib, cu, worst, n_pool):
    """one block object, the geometries' batch sizes from the largest to the smallest"""
    geos = sorted({g.B: g for g in geos}.values(), key=lambda g: -g.B)
    rows = pool(tree.name, 0, n_pool)[:4]
    P, _, refs = oracle_prefixes(tree, 0, rows, [g.B for g in geos])
    blk = make_block(tree, P[0])
    eng = blk.tree.engine(torch.device(DEV))
    for g in geos:
        assert_geometry(g, lib, eng.plan, cu)
        z, J, gx, gc, gw = run_block_batch(tree, blk, rows, g.B)
        ref = refs[g.B]
        worst.record(g.B, z, J, gx, gc, gw, ref)
        check_fwd("z", z, ref["z"])
        check_fwd("J", J, ref["J"])
        check_grads(g.id, gx, gc, gw, ref)


def run_chains(tree, n_blocks, geos, lib, cu, worst):
    """one trainer, hint_chain_forward / hint_chain_backward as test_gpu_instances.run_chain drives them, largest batch first"""
    geos = sorted({g.B: g for g in geos}.values(), key=lambda g: -g.B)
    rows = pool(tree.name, n_blocks, geos[0].B)[:4]
    x, c, gz, gJ = rows
    P, perms, refs = oracle_prefixes(tree, n_blocks, rows, [g.B for g in geos])
    flow = hint_amd.HintFlow(tree.d, n_blocks, list(tree.widths), ndim_c=tree.dc, perm_first=True)
    for i, blk in enumerate(flow.blocks):
        blk.load_state_dict(P[i])
        assert flow.has_perm(i)
        flow.perms[i].W.copy_(perms[i])
    flow = flow.to(DEV)
    tr = hint_amd.FlowTrainer(flow, noise=0.0, use_graph=False)
    assert tr._chainable
    tr._check_arenas()
    tr._pack_all()
    st = torch.cuda.current_stream().cuda_stream
    for g in geos:
        B = g.B
        chain = tr._chain_for(B)
        assert_geometry(g, lib, tr.engines[0].plan, cu)
        xd = x[:B].to(DEV)
        cd = c[:B].to(DEV) if tree.dc else None
        cp = cd.data_ptr() if tree.dc else None
        z, J = torch.empty_like(xd), torch.empty(B, device=DEV)
        _lib.check(lib.hint_chain_forward(chain, xd.data_ptr(), cp, z.data_ptr(), J.data_ptr(), None, None, st), "hint_chain_forward")
        gx = torch.empty_like(xd)
        gc = torch.zeros_like(cd) if tree.dc else None
        gzd, gJd = gz[:B].to(DEV).contiguous(), gJ[:B].to(DEV).contiguous()
        _lib.check(lib.hint_chain_backward(chain, xd.data_ptr(), cp, gzd.data_ptr(), gJd.data_ptr(), gx.data_ptr(),
                                           gc.data_ptr() if tree.dc else None, 1.0, 0.0, 0, st), "hint_chain_backward")
        torch.cuda.synchronize()
        gw = {}
        for bi, ((a, b), eng) in enumerate(zip(tr.slices, tr.engines)):
            for p, gp in zip(eng.params, eng.split_flat(tr.G[a:b])):
                name = [n for n, q in flow.blocks[bi].named_parameters() if q is p][0]
                gw[(bi, name)] = gp
        ref = refs[B]
        worst.record(B, z, J, gx, gc, gw, ref)
        check_fwd("z", z, ref["z"])
        check_fwd("J", J, ref["J"])
        check_grads(g.id, gx, gc, gw, ref)


CASES = [(t.name, f) for t in wg.TREES for f in wg.families_of(t)]


@pytest.mark.gpu
@pytest.mark.parametrize("tree_name,family", CASES, ids=[f"{t}-{f}" for t, f in CASES])
def test_geometry_vs_oracle(tree_name, family):
    torch.set_num_threads(min(16, torch.get_num_threads()))      # (the float64 oracle: a GPU box has many host cores)
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tree = wg.TREE[tree_name]
    geos = wg.Resolver(lib, tree, cu).family(family)
    assert geos
    n_pool = wg.pool_rows(lib, tree, cu)        # (default knobs: resolved in front of any forced_env)
    worst = Worst(f"{tree_name}/{family}")
    try:
        if family.startswith("chain"):
            run_chains(tree, int(family[5:]), geos, lib, cu, worst)
        elif family == "forced":
            for g in geos:          # (a block object per knob value: the workspace of a batch size is sized by its split count)
                with wg.forced_env(lib, g.knobs["HINT_DW_SPLITS"]):
                    run_blocks(tree, [g], lib, cu, worst, n_pool)
        else:
            run_blocks(tree, geos, lib, cu, worst, n_pool)
    finally:
        lib.hint_debug_reload_knobs()
        worst.print()


@pytest.mark.gpu
@pytest.mark.parametrize("tree_name", ["production", "lean_d100"])
def test_accumulate_over_two_geometries(tree_name):
    """a `steps` size and then a `tiny` size without clearing .grad: the sum is the oracle's sum, and the padding floats between the
    tensors of the gradient arena keep the sentinel they held (hint_wreduce_kernel adds to real elements only; with the thin slabs
    of the d = 100 tree through `g[dst] + r`)"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib = _lib.load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tree = wg.TREE[tree_name]
    res = wg.Resolver(lib, tree, cu)
    first = next(g for g in res.steps() if g.rows == 80)
    second = next(g for g in res.tiny() if g.B == 35)
    rows = pool(tree.name, 0, wg.pool_rows(lib, tree, cu))[:4]
    P, _, refs = oracle_prefixes(tree, 0, rows, [first.B, second.B])
    blk = make_block(tree, P[0])
    eng = blk.tree.engine(torch.device(DEV))
    eng.ensure_arena()
    flat, views = eng.grad_views()
    pad = torch.ones(eng.total, dtype=torch.bool, device=DEV)
    for off, n in zip(eng.offsets, eng.numels):
        pad[off:off + n] = False
    assert int(pad.sum()) > 0
    flat.zero_()
    flat[pad] = SENTINEL
    for p, v in zip(eng.params, views):         # gradients "left by an earlier backward": both passes add to them
        p.grad = v
    worst = Worst(f"{tree_name}/accumulate")
    try:
        for g in (first, second):
            assert_geometry(g, lib, eng.plan, cu)
            z, J, gx, gc, gw = run_block_batch(tree, blk, rows, g.B, clear=False)
        assert all(p.grad is v for p, v in zip(eng.params, views))
        ref = dict(refs[second.B])
        ref["gw"] = {k: refs[first.B]["gw"][k] + refs[second.B]["gw"][k] for k in ref["gw"]}
        worst.record(second.B, z, J, gx, gc, gw, ref)
        check_grads(f"{tree_name}/accumulate", gx, gc, gw, ref)
        assert bool((flat[pad] == SENTINEL).all()), "padding of the gradient arena was written"
    finally:
        worst.print()
