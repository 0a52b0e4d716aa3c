"""The call-form ledger: every call form of the block and chain C ABI (include/hint_amd.h) against every kernel family it is written
in, each pair compared with the float64 oracle by tests/test_gpu_call_forms.py.

The instance ledger (instance_cases.py) pins WHICH kernel runs and the geometry ledger (wgrad_geometry.py) what part B's loops do with
the batch; both drive the kernels through one plain call.  This one lists the other call forms - perm, J_in, loss_acc, gz_scale,
gJ_const, g_J = NULL, x = NULL, accumulate, hint_chain_backward_parts / hint_chain_wgrad_range, hint_block_backward_rows,
hint_chain_set_block_io (x_in, c_in, g_add), hint_chain_wgrad_adam - as FORMS, each with the source files its code lives in, and the
kernel families as FAMILIES (trees of the instance ledger, batch sizes resolved through hint_plan_check_dispatch for a CU count).  A
form needs a case in every family that is compiled from one of its files; a pair that cannot exist is listed in EXCLUDED with the
reason.  tests/test_call_forms_cpu.py checks the ledger, and - with the oracle alone - that the natural mistake of every form moves a
compared tensor by at least ten times its tolerance on the ledger's own inputs.

The oracles of the forms live here as well (float64, CPU): the GPU test and the CPU sensitivity check share them."""
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from instance_cases import CASES, instances_of
from oracle import hint_oracle as orc
from wgrad_geometry import Dispatcher, Tree

SEED = 11
N_BLOCKS = 3                    # blocks of the chain forms (F4, F5) and of the gathered forms (F6, F7)
GZ_SCALE2 = 0.37                # gz_scale of F3's second pass
MIN_CANDIDATES = 512            # pool candidates at least: the kink caps bound a share, and the share of 60 candidates is noise
MAX_SCAN_TILES = 4096          # the `first` batch sizes are looked for up to this many 16-row tiles


# ------------------------------------------------------------------------------------------------------------ families
@dataclass(frozen=True)
class Family:
    name: str
    case: str                   # the instance_cases.CASES entry whose tree, weight scale and kink cap this family takes
    batch: object               # 37, or ("nr", 2) / ("alt4", 1): the smallest ragged B whose dispatch shows that field value
    expect: Tuple[str, str, str, str]       # (forward, inverse, backward part A, part B) as a single block; chained launches: CH = true
    declare: Tuple[Tuple[str, int], ...]    # dispatch fields the family is here for
    files: Tuple[str, ...]                  # the sources its kernels are compiled from

    @property
    def _case(self):
        return next(c for c in CASES if c.name == self.case)

    @property
    def d(self):
        return self._case.d

    @property
    def dc(self):
        return self._case.dc

    @property
    def widths(self):
        return tuple(self._case.widths)

    @property
    def scale(self):
        return self._case.scale

    @property
    def kink_cap(self):
        """share of pool candidates that may be discarded next to a ReLU kink, one block: the geometry ledger's caps"""
        return 0.19 if self.d == 40 else 0.06

    def chain_kink_cap(self, n_blocks=N_BLOCKS):
        """.. a candidate of a chain or of a gathered group goes when ANY of its n blocks is next to a kink: 1 - (1 - cap)^n"""
        return 1.0 - (1.0 - self.kink_cap) ** n_blocks

    @property
    def tree(self) -> Tree:
        return Tree(self.name, self.d, self.dc, self.widths, "", self.case)

    def expect_for(self, entry: str):
        if entry == "block":
            return self.expect
        return tuple(s.replace(", false>", ", true>") if s.startswith("hint_wl_") else s for s in self.expect)


WL = ("hint_wl_fwd.hip", "hint_wl_bwd.hip", "hint_wgrad.hip")
GEN = ("hint_fwd.hip", "hint_bwd.hip", "hint_wgrad.hip")
_WLX = lambda nr: (f"hint_wl_apply_kernel<false, {nr}, false>", f"hint_wl_apply_kernel<true, {nr}, false>",      # noqa: E731
                   f"hint_wl_bwd_kernel<{nr}, false>", "hint_wgrad_kernel<false, false>")
_GENX = lambda fly, bwd, dw: (f"hint_apply_kernel<false, {fly}>", f"hint_apply_kernel<true, {fly}>", bwd,        # noqa: E731
                              f"hint_wgrad_kernel<{dw}>")

FAMILIES = [
    Family("wl1", "wl_nr1_block", 37, _WLX(1), (("wl", 1), ("nr", 1)), WL),
    Family("wl2", "wl_nr1_block", ("nr", 2), _WLX(2), (("wl", 1), ("nr", 2)), WL),
    Family("n3c", "n3_cond_block_big_s", 37, _GENX("false", "hint_bwd_kernel_n3", "false, false"),
           (("fwd", 1), ("bwd", 2), ("alt4", 0)), GEN),
    Family("n3c_alt4", "n3_cond_block_big_s", ("alt4", 1), _GENX("false", "hint_bwd_kernel_n3", "false, false"),
           (("fwd", 1), ("bwd", 2), ("alt4", 1), ("nw", 4)), GEN),
    Family("bwdc", "bwd_cond_block_big_s", 37, _GENX("false", "hint_bwd_kernel", "false, false"), (("fwd", 1), ("bwd", 1)), GEN),
    Family("fly", "fly_block_multi", 37, _GENX("true", "hint_bwd_kernel_fly", "true, true"),
           (("fwd", 2), ("bwd", 3), ("rowdw", 1), ("fuse_dw1", 1)), GEN),
    Family("sub", "subtree_block_big_s", 37, _GENX("false", "hint_bwd_kernel_n3", "true, true"),
           (("fwd", 1), ("bwd", 2), ("n_sub", 2), ("leanw", 1)), GEN),
    Family("leanw", "dw_wide_alt4_block", 37, _GENX("true", "hint_bwd_kernel_fly", "false, true"), (("leanw", 1), ("n_sub", 0)), GEN),
]
FAMILY = {f.name: f for f in FAMILIES}


def files_of(disp: Dict[str, int]):
    """the sources a dispatch decision's kernels are compiled from (hint_bwd.hip is also built as _n3 and _fly)"""
    return ("hint_wl_fwd.hip" if disp["fwd"] == 0 else "hint_fwd.hip", "hint_wl_bwd.hip" if disp["bwd"] == 0 else "hint_bwd.hip",
            "hint_wgrad.hip")


_RESOLVED: Dict[tuple, int] = {}


def resolve_B(lib, fam: Family, cu: int) -> int:
    """the family's batch size on a device of cu CUs, through hint_plan_check_dispatch (never hard-coded)"""
    if fam.batch == 37:
        return 37
    key = (fam.name, cu)
    if key not in _RESOLVED:
        field, value = fam.batch
        disp = Dispatcher(lib, fam.tree)
        # the decision follows the tile count: the smallest B of every tile count is ragged (B % 16 == 1)
        _RESOLVED[key] = next(B for B in (16 * (t - 1) + 1 for t in range(2, MAX_SCAN_TILES)) if disp(B, cu)[field] == value)
    return _RESOLVED[key]


def family_mismatch(fam: Family, disp: Dict[str, int], B: int, entry: str = "block") -> Optional[str]:
    """None when a dispatch decision is what the family declares; else what differs"""
    got = instances_of(disp, entry)
    if got != fam.expect_for(entry):
        return f"{fam.name}: B={B} on {disp['num_cu']} CUs runs {got}, declared {fam.expect_for(entry)}"
    for k, v in fam.declare:
        if disp[k] != v:
            return f"{fam.name}: B={B} on {disp['num_cu']} CUs dispatches {k}={disp[k]}, declared {v}"
    if files_of(disp) != fam.files:
        return f"{fam.name}: compiled from {files_of(disp)}, declared {fam.files}"
    if B % 16 == 0 or disp["tiles"] < 3:
        return f"{fam.name}: B={B} is not ragged over three or more tiles"
    return None


# --------------------------------------------------------------------------------------------------------------- forms
@dataclass(frozen=True)
class Form:
    name: str
    what: str
    files: Tuple[str, ...]          # where its code lives: a case in every family compiled from one of them
    mistakes: Tuple[str, ...]       # the natural mistakes the sensitivity check puts into the oracle


FWD_FILES = ("hint_wl_fwd.hip", "hint_fwd.hip")
BWD_FILES = ("hint_wl_bwd.hip", "hint_bwd.hip")
DW_FILES = ("hint_wgrad.hip",)

FORMS = [
    Form("F1", "hint_block_forward_ex: perm, per-row J_in, loss_acc", FWD_FILES, ("J_in dropped",)),
    Form("F2", "hint_block_inverse_ex: perm, J_in", FWD_FILES, ("J_in dropped",)),
    Form("F3", "hint_block_backward_ex behind F1: g_z = z with gz_scale = 1/B, g_J = NULL with gJ_const = -1/B, perm, x = NULL; "
               "then per-row g_J, gz_scale = 0.37, accumulate = 1 onto R", BWD_FILES + DW_FILES,
         ("gz_scale taken as 1", "gJ_const ignored", "top slice replaced by the unpermuted x")),
    Form("F4", "chain of 3 blocks, perms in front of blocks 1 and 2: forward with J_in and loss_acc, hint_chain_backward with a "
               "g_add per block", FWD_FILES + BWD_FILES + DW_FILES,
         ("J_in dropped", "g_add dropped on block 0", "g_add dropped on block 1", "g_add dropped on block 2",
          "g_add behind the permutation")),
    Form("F5", "hint_chain_backward_parts 1 then 2; hint_chain_wgrad_range [2,3) then [0,2): bit-identical to F4", BWD_FILES + DW_FILES, ()),
    Form("F6", "gathered part B: three blocks with their own x_in (and c_in), one with a fused perm and x_in = NULL; "
               "hint_block_forward_ex + hint_block_backward_rows each, one hint_chain_wgrad_range", FWD_FILES + BWD_FILES + DW_FILES,
         ("c_in replaced by another block's c", "x_in replaced by the first block's x", "top slice replaced by the unpermuted x")),
    Form("F7", "hint_chain_wgrad_adam behind F6's rows launches (beta1 = 0, lr = 0): exp_avg = F6's gradient bit for bit", DW_FILES, ()),
]
FORM = {f.name: f for f in FORMS}
GROUPS = {"F1-F3": ("F1", "F2", "F3"), "F4-F5": ("F4", "F5"), "F6-F7": ("F6", "F7")}      # forms that run behind each other in one test

# (form, family) pairs that cannot exist, and why.  (None: every kernel family implements every form - the wave-local kernels
#  have no condition, so F6 runs there without c_in, as the ledger says.)
EXCLUDED: Dict[Tuple[str, str], str] = {}
# mistakes that cannot be made in a family, and why
MISTAKE_EXCLUDED = {("c_in replaced by another block's c", fam.name): "the tree has no condition" for fam in FAMILIES if fam.dc == 0}


def required_pairs():
    """every (form, family) the forms' source files call for"""
    return [(fo.name, fa.name) for fo in FORMS for fa in FAMILIES if set(fo.files) & set(fa.files)]


def pairs():
    """.. that exist: what the GPU test compares with the oracle"""
    return [p for p in required_pairs() if p not in EXCLUDED]


# -------------------------------------------------------------------------------------------------- parameters and rows
def nodes_of(fam):
    return orc.build_nodes(fam.d, [(fam.dc,)] if fam.dc else [], list(fam.widths))


def make_params(fam):
    """float32 weights of three blocks and three fixed orthogonal matrices.  F1-F3: block 0 behind W[0]; F4 / F5: the chain
    block 0, W[1] block 1, W[2] block 2; F6 / F7: blocks 0, 1, 2 on their own inputs, W[1] fused in front of block 1"""
    nodes = nodes_of(fam)
    P = [orc.init_params(nodes, seed=5 + 1000 * i, scale=fam.scale) for i in range(N_BLOCKS)]
    W = [orc.random_orthogonal(fam.d, seed=21 + i) for i in range(N_BLOCKS)]
    return nodes, P, W


def _p64(P, grad=True):
    return {k: v.double().requires_grad_(grad) for k, v in P.items()}


def _c(fam, c):
    return [c] if fam.dc else []


def kink_free(name, n_rows, cap, draw, forward):
    """n_rows kink-free rows: candidates are drawn once (draw(N, generator) -> dict of [N, ..] tensors), those whose float64
    pre-activations come within KINK of a ReLU kink anywhere in forward(rows) discarded (at most `cap` of them: the Spy rule of
    tests/test_gpu_instances.py), the first n_rows of the others kept in order.  No row is waived afterwards."""
    from test_gpu_instances import KINK, Spy
    N = max(int(n_rows / (1.0 - cap)) + 16, MIN_CANDIDATES)
    rows = draw(N, torch.Generator().manual_seed(SEED))
    with torch.no_grad(), Spy(N) as spy:
        forward(rows)
    keep = spy.kink > KINK
    dropped = N - int(keep.sum())
    print(f"{name}: {dropped} of {N} candidates next to a ReLU kink discarded ({dropped / N:.1%}, cap {cap:.1%})")
    assert dropped <= cap * N, f"{name}: {dropped} of {N} candidates next to a ReLU kink (cap {cap:.1%})"
    idx = torch.nonzero(keep)[:n_rows, 0]
    assert idx.numel() == n_rows, (name, idx.numel(), n_rows)
    return {k: v[idx].contiguous() for k, v in rows.items()}


def block_rows(fam, B):
    """rows of F1-F3: x, c, zi (the inverse's input), random cotangents gz, gJ, a random per-row J_in"""
    nodes, P, W = make_params(fam)

    def draw(N, g):
        r = dict(x=torch.randn(N, fam.d, generator=g), zi=torch.randn(N, fam.d, generator=g), gz=torch.randn(N, fam.d, generator=g),
                 gJ=torch.randn(N, generator=g), J_in=torch.randn(N, generator=g))
        if fam.dc:
            r["c"] = torch.randn(N, fam.dc, generator=g)
        return r

    def forward(r):
        orc.block_apply(nodes, _p64(P[0], False), r["x"].double() @ W[0].double(), _c(fam, r["c"].double() if fam.dc else None))
    return kink_free(f"{fam.name}/F1-F3", B, fam.kink_cap, draw, forward)


def chain_rows(fam, B):
    """rows of F4 / F5: x, c, gz, gJ, J_in and one g_add per block"""
    nodes, P, W = make_params(fam)

    def draw(N, g):
        r = dict(x=torch.randn(N, fam.d, generator=g), gz=torch.randn(N, fam.d, generator=g), gJ=torch.randn(N, generator=g),
                 J_in=torch.randn(N, generator=g))
        for i in range(N_BLOCKS):
            r[f"g_add{i}"] = torch.randn(N, fam.d, generator=g)
        if fam.dc:
            r["c"] = torch.randn(N, fam.dc, generator=g)
        return r

    def forward(r):
        u = r["x"].double()
        for i in range(N_BLOCKS):
            if i > 0:
                u = u @ W[i].double()
            u, _ = orc.block_apply(nodes, _p64(P[i], False), u, _c(fam, r["c"].double() if fam.dc else None))
    return kink_free(f"{fam.name}/F4-F5", B, fam.chain_kink_cap(), draw, forward)


def gathered_rows(fam, B):
    """rows of F6 / F7: per block i its own x{i}, c{i}, gz{i}, gJ{i}"""
    nodes, P, W = make_params(fam)

    def draw(N, g):
        r = {}
        for i in range(N_BLOCKS):
            r[f"x{i}"] = torch.randn(N, fam.d, generator=g)
            r[f"gz{i}"] = torch.randn(N, fam.d, generator=g)
            r[f"gJ{i}"] = torch.randn(N, generator=g)
            if fam.dc:
                r[f"c{i}"] = torch.randn(N, fam.dc, generator=g)
        return r

    def forward(r):
        for i in range(N_BLOCKS):
            u = r[f"x{i}"].double()
            orc.block_apply(nodes, _p64(P[i], False), u @ W[1].double() if i == 1 else u, _c(fam, r[f"c{i}"].double() if fam.dc else None))
    return kink_free(f"{fam.name}/F6-F7", B, fam.chain_kink_cap(), draw, forward)


# ------------------------------------------------------------------------------- a wrong first-layer operand (part B's mistakes)
class _LinearWrongOperand(torch.autograd.Function):
    """y = v W^T + b whose weight gradient is formed with another operand, as a part B that reads the wrong rows would form it"""

    @staticmethod
    def forward(ctx, v, v_wrong, W, b):
        ctx.save_for_backward(v_wrong, W)
        return v @ W.t() + b

    @staticmethod
    def backward(ctx, g):
        v_wrong, W = ctx.saved_tensors
        return g @ W, None, g.t() @ v_wrong, g.sum(dim=0)


class WrongOperand:
    """while active, the oracle's first-layer weight gradients are formed from a wrong operand: x_wrong in place of the block's
    input lanes (the deepest level's nodes, which read the block's input itself) and / or c_wrong in place of the condition
    (every node).  Forward values, d/dx and d/dc stay right: this is a mistake of part B's operand addressing alone."""

    def __init__(self, nodes, x_wrong=None, c_wrong=None):
        self.by_path = {n.path: n for n in nodes}
        self.deepest = max(n.depth for n in nodes)
        self.x_wrong, self.c_wrong = x_wrong, c_wrong

    def __enter__(self):
        self.orig = orc._mlp

        def mlp(P, prefix, v):
            n = self.by_path[prefix.rsplit(".", 1)[0]]
            vw = v.detach().clone()
            if self.x_wrong is not None and n.depth == self.deepest:
                vw[:, :n.k] = self.x_wrong[:, n.off:n.off + n.k]
            if self.c_wrong is not None:
                vw[:, n.k:] = self.c_wrong
            h1 = torch.relu(_LinearWrongOperand.apply(v, vw, P[prefix + ".0.weight"], P[prefix + ".0.bias"]))
            h2 = torch.relu(torch.nn.functional.linear(h1, P[prefix + ".2.weight"], P[prefix + ".2.bias"]))
            return torch.nn.functional.linear(h2, P[prefix + ".4.weight"], P[prefix + ".4.bias"])
        orc._mlp = mlp
        return self

    def __exit__(self, *exc):
        orc._mlp = self.orig


class _Nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


# -------------------------------------------------------------------------------------------------------------- oracles
def oracle_F1(fam, rows, mistake=None):
    """z, J of block 0 on x @ W[0], plus J_in"""
    nodes, P, W = make_params(fam)
    with torch.no_grad():
        z, J = orc.block_apply(nodes, _p64(P[0], False), rows["x"].double() @ W[0].double(), _c(fam, rows["c"].double() if fam.dc else None))
    if mistake != "J_in dropped":
        J = J + rows["J_in"].double()
    return dict(z=z, J=J)


def oracle_F2(fam, rows, mistake=None):
    """include/hint_amd.h: x = block^-1(z) @ perm^T, J = J_in + the negated log-det (hint.py:83)"""
    nodes, P, W = make_params(fam)
    with torch.no_grad():
        xi, Ji = orc.block_apply(nodes, _p64(P[0], False), rows["zi"].double(), _c(fam, rows["c"].double() if fam.dc else None), rev=True)
    if mistake != "J_in dropped":
        Ji = Ji + rows["J_in"].double()
    return dict(xi=xi @ W[0].double().t(), Ji=Ji)


def oracle_F3(fam, rows, mistake=None):
    """-> (first pass, second pass), each dict(gx, gc, gw).  First: the gradient of the NLL mean(0.5 |z|^2) - mean(J) of F1's
    outputs (g_z = z times 1/B, d/dJ = -1/B for every row).  Second: of 0.37 <g_z, z> + <g_J, J> with per-row cotangents (what
    accumulate = 1 adds to R)"""
    nodes, P, W = make_params(fam)
    B = rows["x"].shape[0]
    out = []
    for second in (False, True):
        P64 = _p64(P[0])
        x = rows["x"].double().requires_grad_(True)
        c = rows["c"].double().requires_grad_(True) if fam.dc else None
        wrong = WrongOperand(nodes, x_wrong=rows["x"].double()) if mistake == "top slice replaced by the unpermuted x" else _Nothing()
        with wrong:
            z, J = orc.block_apply(nodes, P64, x @ W[0].double(), _c(fam, c))
            J = J + rows["J_in"].double()
            if second:
                L = GZ_SCALE2 * (z * rows["gz"].double()).sum() + (J * rows["gJ"].double()).sum()
            else:
                sz = 1.0 if mistake == "gz_scale taken as 1" else 1.0 / B
                sJ = 0.0 if mistake == "gJ_const ignored" else -1.0 / B
                L = sz * 0.5 * (z ** 2).sum() + sJ * J.sum()
            L.backward()
        out.append(dict(gx=x.grad, gc=c.grad if fam.dc else None, gw={k: v.grad for k, v in P64.items()}))
    return out[0], out[1]


def oracle_F4(fam, rows, mistake=None):
    """the chain block 0 -> W[1], block 1 -> W[2], block 2: z, J (+ J_in), and the gradients of <g_z, z> + <g_J, J> + sum_i
    <g_add_i, u_i>, u_i = block i's input after its permutation - the whole definition of g_add"""
    nodes, P, W = make_params(fam)
    P64 = [_p64(p) for p in P]
    x = rows["x"].double().requires_grad_(True)
    c = rows["c"].double().requires_grad_(True) if fam.dc else None
    u, J, extra = x, torch.zeros(x.shape[0], dtype=torch.float64), 0.0
    for i in range(N_BLOCKS):
        pre = u
        if i > 0:
            u = u @ W[i].double()
        if mistake != f"g_add dropped on block {i}":
            extra = extra + (rows[f"g_add{i}"].double() * (pre if mistake == "g_add behind the permutation" else u)).sum()
        u, Ji = orc.block_apply(nodes, P64[i], u, _c(fam, c))
        J = J + Ji
    if mistake != "J_in dropped":
        J = J + rows["J_in"].double()
    ((u * rows["gz"].double()).sum() + (J * rows["gJ"].double()).sum() + extra).backward()
    return dict(z=u.detach(), J=J.detach(), gx=x.grad, gc=c.grad if fam.dc else None,
                gw={(i, k): v.grad for i, p in enumerate(P64) for k, v in p.items()})


def oracle_F6(fam, rows, mistake=None):
    """per block i, alone on its own input: z, J, d/dx, d/dc and the weight gradients of <g_z_i, z> + <g_J_i, J>; W[1] fused in
    front of block 1"""
    nodes, P, W = make_params(fam)
    out = []
    for i in range(N_BLOCKS):
        P64 = _p64(P[i])
        x = rows[f"x{i}"].double().requires_grad_(True)
        c = rows[f"c{i}"].double().requires_grad_(True) if fam.dc else None
        xw = cw = None
        if mistake == "c_in replaced by another block's c":
            cw = rows[f"c{(i + 1) % N_BLOCKS}"].double()
        if mistake == "x_in replaced by the first block's x" and i == 2:
            xw = rows["x0"].double()
        if mistake == "top slice replaced by the unpermuted x" and i == 1:
            xw = rows["x1"].double()
        with (WrongOperand(nodes, xw, cw) if (xw is not None or cw is not None) else _Nothing()):
            z, J = orc.block_apply(nodes, P64, x @ W[1].double() if i == 1 else x, _c(fam, c))
            ((z * rows[f"gz{i}"].double()).sum() + (J * rows[f"gJ{i}"].double()).sum()).backward()
        out.append(dict(z=z.detach(), J=J.detach(), gx=x.grad, gc=c.grad if fam.dc else None, gw={k: v.grad for k, v in P64.items()}))
    return out


ROWS = {"F1": block_rows, "F2": block_rows, "F3": block_rows, "F4": chain_rows, "F6": gathered_rows}
ORACLES = {"F1": oracle_F1, "F2": oracle_F2, "F3": oracle_F3, "F4": oracle_F4, "F6": oracle_F6}


# ------------------------------------------------------------------------------------- error over bound, as the checks bound it
def ratios(got, ref, tol):
    """{quantity: error / bound} of every compared tensor of one reference dict, with the measures of check_fwd (z, J, xi, Ji: TOL_FWD
    of the largest magnitude, at least 1) and check_grads (gx, gc: TOL_GX of the largest entry; every weight-gradient tensor: TOL_GW
    of its largest entry + 1e-7 of the largest weight gradient).  A ratio of at most 1 passes.  tol = (TOL_FWD, TOL_GX, TOL_GW)"""
    tol_fwd, tol_gx, tol_gw = tol
    out = {}
    for k in ("z", "J", "xi", "Ji"):
        if ref.get(k) is not None:
            out[k] = float((got[k].detach().double().cpu() - ref[k]).abs().max()) / (tol_fwd * max(1.0, float(ref[k].abs().max())))
    for k in ("gx", "gc"):
        if ref.get(k) is not None:
            out[k] = float((got[k].detach().double().cpu() - ref[k]).abs().max()) / (tol_gx * max(float(ref[k].abs().max()), 1e-30))
    if ref.get("gw"):
        gmax = max(float(v.abs().max()) for v in ref["gw"].values())
        for k, r in ref["gw"].items():
            e = float((got["gw"][k].detach().double().cpu() - r).abs().max())
            out[("gw", k)] = e / (tol_gw * float(r.abs().max()) + 1e-7 * gmax)
    return out
