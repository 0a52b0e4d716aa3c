"""The path ledger: the plans the planner falls back to when a block does not fit the 160 KiB LDS at the first attempt, and the
size limits of the row kernels, as GPU cases of tests/test_gpu_plan_paths.py.

hint_plan.cpp's plan_for() walks a ladder - 64, 48, 32, 16 fragment tiles per group, around that nw, nw / 2 .. 1 wavefronts sharing
one unit's rows - and thresholds decide whether a level is cut into several groups, whether the thin layers' vectors ride in LDS
whole, a group's slice at a time or not at all, whether the backward's slot table sits in LDS, whether rows compute dW1 | db1.  Each is
a data-driven branch inside the row kernels that the instance ledger (tests/instance_cases.py) does not select by: a case here names
its entry point, its tree, its batch size as a function of the device's CU count, its initialisation and the PATH TUPLE it is
declared to reach (hint_plan_paths, include/hint_amd.h).  tests/test_plan_paths_cpu.py checks all of it against
hint_plan_check_paths without a GPU; the GPU test asserts the same on the live plan before it compares anything.

Rows: the tests/call_forms.py rule.  A pool of candidate rows is drawn once, the float64 oracle discards those with a hidden
pre-activation within KINK of a ReLU kink, the first B of the others are kept in order and no row is waived afterwards."""
import ctypes as C
import functools
from dataclasses import dataclass
from typing import Tuple

import torch

from oracle import hint_oracle as orc

PATHS = ["tile_cap", "unit_waves", "groups", "levels", "thin_fwd", "thin_bwd", "spill_fwd", "spill_bwd", "slots_lds", "rowdw",
         "r_tiles", "cin_tiles"]                      # include/hint_amd.h, HINT_PATH_FIELDS
THIN_L2, THIN_WHOLE, THIN_GROUP = 0, 1, 2             # fields thin_fwd / thin_bwd
POOL = 256                      # candidate rows of a 37-row case
ROWS_FEW = 37                   # three row tiles, the last one ragged
Z_MAX = 50.0                    # the oracle's |z| and |J| on the kept rows stay below this (a max-relative tolerance means something)
SEED_ROWS, SEED_PARAMS = 11, 5


@dataclass(frozen=True)
class PathCase:
    name: str
    entry: str                  # "block" | "chain" | "coupling" (an ExternalAffineCoupling: one node, k = 0, through the module route)
    d: int
    dc: int
    widths: tuple
    paths: Tuple[int, ...]      # declared: fields 0-11 of hint_plan_paths for the variant the batch runs on
    nw: int = 8                 # declared: wavefronts per workgroup of that variant (4: the plan's 4-wavefront variant)
    many: bool = False          # 16 x CUs + 5 rows (more row tiles than CUs: what picks a 4-wavefront variant) instead of 37
    n_blocks: int = 1           # (chain cases)
    scale: float = 0.03         # init "randn": every tensor scale * randn, as the instance ledger's d = 100 cases
    offset: float = 0.0         # > 0: init "offset" with this output scale (below)
    big_s: float = 0.0          # (never: the field test_gpu_instances.make_chain_pair reads)

    def B(self, cu: int) -> int:
        return 16 * cu + 5 if self.many else ROWS_FEW

    def pool(self, cu: int) -> int:
        """candidate rows: 256 for the 37-row cases; twice the batch otherwise (at most half a pool may be discarded)"""
        return POOL if not self.many else 2 * self.B(cu)


# The path tuples are what hint_plan_check_paths returned for these trees at 256 CUs when the ledger was written (re-derived, not
# assumed); tests/test_plan_paths_cpu.py fails when one moves.
#        tile_cap unit_waves groups levels thin_fwd thin_bwd spill_fwd spill_bwd slots_lds rowdw r_tiles cin_tiles
CASES = [
    # ---- the ladder's tile_cap steps on the 8-wavefront plan
    PathCase("cap48_d128", "block", 128, 0, (32, 16), (48, 8, 10, 7, 2, 0, 0, 0, 0, 1, 4, 4)),
    PathCase("cap48_cond_d64", "block", 64, 30, (64, 32), (48, 8, 9, 6, 2, 2, 1, 1, 1, 0, 2, 4)),
    PathCase("cap16_cin128_d56", "block", 56, 100, (32,), (16, 8, 13, 6, 0, 2, 0, 0, 1, 0, 2, 8)),
    PathCase("cap16_cin128_d128", "block", 128, 64, (64, 32), (16, 8, 33, 7, 2, 2, 1, 1, 0, 0, 4, 8)),
    PathCase("cap32_cin128_r50", "block", 100, 78, (48,), (32, 8, 18, 7, 2, 2, 1, 1, 0, 0, 4, 8)),
    # ... and the same two narrow-h trees at more row tiles than CUs.  Neither has a 4-wavefront variant, and no plan below the
    # ladder's first step can have one: the variant must fit the LDS twice (80 KiB), a smaller tile_cap or fewer unit_waves is
    # tried only when the attempt before needed more than 160 KiB, and one step at best halves the per-group region (32 -> 16 tiles,
    # or half the slabs) and leaves the fixed part.  The cases keep the batch size a 4-wavefront variant would run at and declare
    # the 8-wavefront plan that runs it.
    PathCase("cap48_cond_d64_many", "block", 64, 30, (64, 32), (48, 8, 9, 6, 2, 2, 1, 1, 1, 0, 2, 4), many=True),
    PathCase("cap16_cin128_d56_many", "block", 56, 100, (32,), (16, 8, 13, 6, 0, 2, 0, 0, 1, 0, 2, 8), many=True),
    # ---- the ladder's unit_waves steps (a wide root over narrow deep levels: the oracle stays cheap)
    PathCase("waves4_d128", "block", 128, 0, (420, 16), (32, 4, 11, 7, 2, 0, 1, 0, 0, 0, 4, 4)),
    PathCase("waves2_d128", "block", 128, 0, (512, 16), (32, 2, 11, 7, 2, 0, 1, 0, 0, 0, 4, 4)),
    PathCase("waves1_d128", "block", 128, 0, (600, 16), (32, 1, 11, 7, 2, 0, 1, 0, 0, 0, 4, 4)),
    # ---- every level cut to one group per node.  With some 10^5 hidden pre-activations per row a plain random init leaves no
    #      row away from a kink, so the init keeps them away by construction (init_offset); each unit's ReLU mask is then
    #      nearly constant over the rows.  That is accepted here: the case aims at addressing (groups, slabs, staged slices), and
    #      mask handling is the instance ledger's job.
    PathCase("group_per_node_d64", "block", 64, 0, (385,), (64, 8, 63, 6, 2, 0, 1, 0, 0, 0, 2, 2), offset=0.1),
    # ---- the first attempt, whole thin blobs, on both wavefront variants of one plan; cin = 128 on a plan that has the variant
    PathCase("first_attempt_nw8", "block", 12, 0, (48, 24), (64, 8, 3, 3, 1, 1, 0, 0, 1, 0, 1, 1)),
    PathCase("first_attempt_nw4", "block", 12, 0, (48, 24), (64, 4, 3, 3, 1, 1, 0, 0, 1, 0, 1, 1), nw=4, many=True),
    PathCase("cin128_nw4", "block", 4, 126, (16, 16), (64, 4, 2, 2, 1, 1, 0, 0, 1, 0, 1, 8), nw=4, many=True),
    # ---- r = 128: eight tail tiles of outputs (k = 0, all 128 lanes transformed, s and t see the condition only)
    PathCase("r128_coupling", "coupling", 128, 4, (64,), (64, 8, 1, 1, 1, 0, 0, 0, 1, 0, 8, 1)),
    # ---- two chained blocks at d = 128: 2 x 64 KiB of permutation matrices, over PERM_LDS_MAX, stay in global memory
    #      (scale 0.02: at 0.03 one leaf's b3 gradient cancels over the 37 rows so far that the float32 oracle itself uses 0.32 of its
    #       tolerance; at 0.02 the worst tensor uses 0.04)
    PathCase("cap48_d128_chain", "chain", 128, 0, (32, 16), (48, 8, 10, 7, 2, 0, 0, 0, 0, 1, 4, 4), n_blocks=2, scale=0.02),
]


# ---- trees, parameters ----
def module_of(case):
    """the hint_amd module of a block or coupling case (on the CPU: a parameter container until it is moved to the device)"""
    import hint_amd
    if case.entry == "coupling":
        return hint_amd.ExternalAffineCoupling([(case.d,)], dims_c=[(case.dc,)], F_args={"internal_size": case.widths[0]})
    return hint_amd.HierarchicalAffineCouplingBlock([(case.d,)], dims_c=[(case.dc,)] if case.dc else [],
                                                    c_internal=list(case.widths))


def descs_of(case):
    """the C node table of the case's tree and the clamp its plan is made with"""
    from hint_amd.hint import node_descs
    tree = module_of(case).tree
    nodes = tree._flat_nodes()
    descs, _, _, _ = node_descs(nodes)
    return descs, len(nodes), tree.clamp


def oracle_tree(case):
    """(oracle nodes, clamp) of the case's tree"""
    if case.entry == "coupling":
        from test_gpu_conditional import oracle_nodes
        tree = module_of(case).tree
        return oracle_nodes(tree, case.dc), tree.clamp
    return orc.build_nodes(case.d, [(case.dc,)] if case.dc else [], list(case.widths)), 4.0


def init_offset(nodes, a, seed):
    """hidden pre-activations away from zero by construction: hidden biases of random sign and magnitude in [2, 3], every weight
    a / sqrt(fan_in) * randn and the last bias a * randn (a: the output scale)"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for key, shp in orc.param_shapes(nodes).items():
        last = ".4." in key
        if key.endswith("weight"):
            P[key] = (a / max(shp[1], 1) ** 0.5 * torch.randn(shp, generator=g, dtype=torch.float64)).float()
        elif last:
            P[key] = (a * torch.randn(shp, generator=g, dtype=torch.float64)).float()
        else:
            sign = torch.randint(0, 2, shp, generator=g).double() * 2 - 1
            P[key] = (sign * (2 + torch.rand(shp, generator=g, dtype=torch.float64))).float()
    return P


def init_params(case, nodes, seed=SEED_PARAMS):
    return init_offset(nodes, case.offset, seed) if case.offset > 0 else orc.init_params(nodes, seed=seed, scale=case.scale)


def chain_ref(case):
    """the float64 OracleFlow of a chain case on float32 weights and matrices: what test_gpu_instances.make_chain_pair builds"""
    ref = orc.OracleFlow(case.d, case.n_blocks, list(case.widths), dims_c=[(case.dc,)] if case.dc else (), seed=3,
                         init_scale=case.scale, dtype=torch.float64)
    ref.params = [{k: v.float().double() for k, v in P.items()} for P in ref.params]
    ref.perms = [None if p is None else p.float().double() for p in ref.perms]
    return ref


# ---- rows ----
def draw(case, N):
    g = torch.Generator().manual_seed(SEED_ROWS)
    r = dict(x=torch.randn(N, case.d, generator=g), zi=torch.randn(N, case.d, generator=g), gz=torch.randn(N, case.d, generator=g),
             gJ=torch.randn(N, generator=g))
    if case.dc:
        r["c"] = torch.randn(N, case.dc, generator=g)
    return r


class Model:
    """a case's float32 parameters and its oracle in a dtype: forward / inverse of rows, gradients under per-row cotangents"""

    def __init__(self, case):
        self.case = case
        if case.entry == "chain":
            self.flow = chain_ref(case)
            self.P = {(i, k): v.float() for i, P in enumerate(self.flow.params) for k, v in P.items()}
        else:
            self.nodes, self.clamp = oracle_tree(case)
            self.P = init_params(case, self.nodes)

    def apply(self, P, x, c, rev):
        case = self.case
        if case.entry == "chain":
            f = self.flow
            old = f.params, f.perms
            f.params = [{k: P[(i, k)] for k in old[0][i]} for i in range(case.n_blocks)]
            f.perms = [None if p is None else p.to(x.dtype) for p in old[1]]
            try:
                return (f.inverse if rev else f.forward)(x, tuple(c))
            finally:
                f.params, f.perms = old
        return orc.block_apply(self.nodes, P, x, c, rev=rev, clamp=self.clamp)

    def grads(self, rows, dtype, rev):
        """one direction under the rows' cotangents: outputs and d/d(input), d/dc, every weight tensor"""
        leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)      # (a copy: the shared rows and parameters stay as they are)
        P = {k: leaf(v) for k, v in self.P.items()}
        x = leaf(rows["zi" if rev else "x"])
        c = [leaf(rows["c"])] if self.case.dc else []
        out, J = self.apply(P, x, c, rev)
        ((out * rows["gz"].to(dtype)).sum() + (J * rows["gJ"].to(dtype)).sum()).backward()
        return dict(out=out.detach(), J=J.detach(), gx=x.grad, gc=c[0].grad if c else None, gw={k: v.grad for k, v in P.items()})

    def reference(self, rows, dtype=torch.float64):
        """what the GPU test compares: forward z, J and its gradients, inverse x, J (the coupling: the inverse's gradients too)"""
        f = self.grads(rows, dtype, rev=False)
        ref = dict(z=f["out"], J=f["J"], gx=f["gx"], gc=f["gc"], gw=f["gw"])
        if self.case.entry == "coupling":
            ref["inv"] = self.grads(rows, dtype, rev=True)
            ref["xi"], ref["Ji"] = ref["inv"]["out"], ref["inv"]["J"]
        else:
            with torch.no_grad():
                P = {k: v.to(dtype) for k, v in self.P.items()}
                ref["xi"], ref["Ji"] = self.apply(P, rows["zi"].to(dtype), [rows["c"].to(dtype)] if self.case.dc else [], True)
        return ref


@functools.lru_cache(maxsize=None)
def prepared(case, cu):
    """(model, the case's B rows, its float64 reference, figures): computed once per case and CU count, shared, never changed"""
    from test_gpu_instances import KINK, Spy
    m = Model(case)
    N, B = case.pool(cu), case.B(cu)
    pool = draw(case, N)
    with torch.no_grad(), Spy(N) as spy:
        P = {k: v.double() for k, v in m.P.items()}
        m.apply(P, pool["x"].double(), [pool["c"].double()] if case.dc else [], False)
    keep = spy.kink > KINK
    idx = torch.nonzero(keep)[:B, 0]
    rows = {k: v[idx].contiguous() for k, v in pool.items()}
    fig = dict(pool=N, discarded=N - int(keep.sum()), found=int(idx.numel()), B=B)
    if idx.numel() < B:
        return m, rows, None, fig
    ref = m.reference(rows)
    fig["z_max"] = max(float(ref["z"].abs().max()), float(ref["xi"].abs().max()))
    fig["J_max"] = max(float(ref["J"].abs().max()), float(ref["Ji"].abs().max()))
    return m, rows, ref, fig


# ---- the metrics of test_gpu_instances.check_fwd / check_grads as shares of their tolerances ----
def _diff(a, b):
    return float((a.detach().double().cpu() - b).abs().max())


def fwd_shares(got, ref):
    """got: dict with z, J, xi, Ji -> {name: error / what check_fwd allows}"""
    from test_gpu_instances import TOL_FWD
    return {k: _diff(got[k], ref[k]) / (TOL_FWD * max(1.0, float(ref[k].abs().max()))) for k in ("z", "J", "xi", "Ji")}


def grad_shares(got, ref):
    """got: dict with gx, gc, gw -> {name: error / what check_grads allows}"""
    from test_gpu_instances import TOL_GW, TOL_GX, err
    out = {"d/dx": err(got["gx"], ref["gx"]) / TOL_GX}
    if ref["gc"] is not None:
        out["d/dc"] = err(got["gc"], ref["gc"]) / TOL_GX
    gmax = max(float(v.abs().max()) for v in ref["gw"].values())
    for k, r in ref["gw"].items():
        out[k] = _diff(got["gw"][k], r) / (TOL_GW * float(r.abs().max()) + 1e-7 * gmax)
    return out


INV_TOL_X, INV_TOL_G, INV_TOL_W = 1e-4, 1e-4, 2e-4      # tests/test_gpu_inverse_grad.py::test_external_coupling_inverse_grads


def inv_grad_shares(got, ref):
    """the coupling's inverse under autograd, max-relative per tensor (util.rel_err) -> {name: error / that test's bound}"""
    from test_gpu_instances import err
    out = {"inv x": err(got["out"], ref["out"]) / INV_TOL_X, "inv d/dz": err(got["gx"], ref["gx"]) / INV_TOL_G,
           "inv d/dc": err(got["gc"], ref["gc"]) / INV_TOL_G}
    for k, r in ref["gw"].items():
        out["inv " + k] = err(got["gw"][k], r) / INV_TOL_W
    return out


# ---- the planner's report ----
def check_paths(lib, case, cu):
    """hint_plan_check_paths: the path tuple of a host-only plan of the case's tree for its batch on a device of cu CUs"""
    descs, n, clamp = descs_of(case)
    out = (C.c_int32 * len(PATHS))()
    st = lib.hint_plan_check_paths(descs, n, case.d, case.dc, clamp, case.B(cu), cu, out, len(PATHS))
    assert st == 0, lib.hint_last_error().decode()
    return tuple(out)


def plan_paths(lib, plan, B):
    """hint_plan_paths: the same of a device plan"""
    out = (C.c_int32 * len(PATHS))()
    st = lib.hint_plan_paths(plan, B, out, len(PATHS))
    assert st == 0, lib.hint_last_error().decode()
    return tuple(out)


def check_variant(lib, case, cu):
    """(wavefronts per workgroup, 1 when it is the 4-wavefront variant) hint_plan_check_dispatch shows for the case's batch"""
    from instance_cases import DISPATCH
    descs, n, clamp = descs_of(case)
    out = (C.c_int32 * len(DISPATCH))()
    st = lib.hint_plan_check_dispatch(descs, n, case.d, case.dc, clamp, case.B(cu), cu, out, len(DISPATCH))
    assert st == 0, lib.hint_last_error().decode()
    disp = dict(zip(DISPATCH, list(out)))
    return disp["nw"], disp["alt4"]
