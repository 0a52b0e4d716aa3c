"""Non-finite values in the data: the cases of tests/test_gpu_nonfinite.py, checked without a GPU by tests/test_nonfinite_cpu.py.

THE OPTIMIZER'S ELEMENT TABLE.  One small set of segments carries every class of gradient element (CLASSES) at every 16-byte lane
position of a vector body and in the scalar tail of the ragged lengths 1, 3, 5, 1023, 1025, 1027; p, m and v are finite and
seeded.  A RUN is (grad_clamp, grad_scale): the clamp on and off, at a scale of 1 and at one that overflows the product
g * grad_scale of the +-1e38 class.  The reference is the pair of statements the fused step replaces - clamp_ (only when
grad_clamp > 0) and torch.optim.Adam(foreach=False) from the same moments - three steps in a row.  The magnitudes keep away from
the fp32 overflow edge, where (1 - b2) * g * g changes class with the order of its two products: adam_fp32 evaluates both orders.

SPOILED ROWS.  ROW_CASES holds one block case per row-kernel family of instance_cases.ROW_FAMILIES (and CHAIN_CASES two chains) at
the smallest batch with two full tiles and a ragged third, B = 2 * 16 * nr + 5; spoil_plan() says which rows are spoiled and with
what.  The same batch runs twice, clean and spoiled: the rows that are not spoiled must keep their bits, the float64 oracle
decides which spoiled rows have a non-finite objective.

A POISONED STEP.  poisoned_session(): two clean steps, one whose batch has a NaN row, a clean step and an nll() on the flows of
session_script.FLOWS, against OracleFlow.train_step in float64."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np
import torch

import session_script as ss
from instance_cases import DW, GEN_F, WL_F
from oracle import hint_oracle as orc

NAN, INF = float("nan"), float("inf")

# ---- the optimizer's element table ------------------------------------------------------------------------------------------
CLAMP = 5.0
RUNS = [(CLAMP, 1.0), (0.0, 1.0), (CLAMP, 4.0), (0.0, 4.0)]           # (grad_clamp, grad_scale); 1e38 * 4 overflows
STEPS = 3
HYPER = dict(lr=3e-4, betas=(0.9, 0.95), eps=1e-4, weight_decay=1.86e-5)         # test_gpu_optim.py's
RAGGED = (1, 3, 5, 1023, 1025, 1027)                                  # test_segments_of_every_alignment_between_guard_bands
NEG_NAN_BITS = np.uint32(0xFFC00000)                                  # a quiet NaN with the sign bit set


def classes(scale: float):
    """[(name, g, zero): the gradient value of a class at this grad_scale; zero: p = v = 0 there (g = 0: the 0 / eps case)]"""
    c = CLAMP / scale                                                 # g * scale is exactly the clamp (scale is a power of two)
    out = [("+nan", NAN, False), ("-nan", "-nan", False), ("+inf", INF, False), ("-inf", -INF, False)]
    for name, mag in (("3.3e38", 3.3e38), ("1e38", 1e38), ("1e30", 1e30), ("1e15", 1e15), ("clamp", c), ("zero", 0.0),
                      ("subnormal", 1e-40), ("ordinary", 0.7), ("beyond clamp", 23.5)):
        out += [("+" + name, mag, False), ("-" + name, -mag, False)]
    out += [("+0 / eps", 0.0, True), ("-0 / eps", -0.0, True)]
    return out


def _f32(values):
    """float32 array of a class column; "-nan" is the NaN with the sign bit set"""
    a = np.array([NAN if v == "-nan" else v for v in values], dtype=np.float32)
    a.view(np.uint32)[[i for i, v in enumerate(values) if v == "-nan"]] = NEG_NAN_BITS
    return a


@dataclass
class Table:
    lengths: list                   # floats per segment
    cls: list                       # per segment: the class index of every element
    p: list                         # per segment float32 arrays
    g: list
    m: list
    v: list
    names: list


@functools.lru_cache(maxsize=None)
def table(scale: float) -> Table:
    """the segments: a body with the class list behind 0, 1, 2 and 3 ordinary elements (every class at every lane position), then
    rounds of the ragged lengths whose scalar tails (the last n % 4 elements) walk through the class list"""
    cl = classes(scale)
    nc = len(cl)
    ordinary = [i for i, c in enumerate(cl) if c[0] == "+ordinary"][0]
    body = []
    for j in range(4):
        body += [ordinary] * ((-len(body)) % 4) + [ordinary] * j + list(range(nc))
    body += [ordinary] * ((-len(body)) % 4)
    lengths, cls, k = [len(body)], [np.array(body)], 0
    rounds = -(-nc // sum(n % 4 for n in RAGGED))
    for _ in range(rounds):
        for n in RAGGED:
            start = (k - (n - n % 4)) % nc                            # the tail's first element is class k
            cls.append((start + np.arange(n)) % nc)
            lengths.append(n)
            k += n % 4
    rng = np.random.RandomState(3)
    gcol = _f32([c[1] for c in cl])
    zero = np.array([c[2] for c in cl])
    t = Table(lengths, cls, [], [], [], [], [c[0] for c in cl])
    for ci in cls:
        n = len(ci)
        p = rng.randn(n).astype(np.float32)
        m = (0.1 * rng.randn(n)).astype(np.float32)
        v = (0.1 * rng.rand(n)).astype(np.float32)
        p[zero[ci]] = 0.0
        v[zero[ci]] = 0.0
        t.p.append(p); t.g.append(gcol[ci].copy()); t.m.append(m); t.v.append(v)
    return t


def coverage(t: Table):
    """({(class, lane) in a vector body}, {class in a scalar tail}) with every segment on a 16-byte boundary"""
    body, tail = set(), set()
    for ci in t.cls:
        n4 = len(ci) // 4 * 4
        body |= {(int(c), i % 4) for i, c in enumerate(ci[:n4])}
        tail |= {int(c) for c in ci[n4:]}
    return body, tail


def class_of(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, element by element (numpy array or torch tensor)"""
    a = torch.as_tensor(a)
    return (torch.isnan(a).to(torch.int8) + 2 * (a == INF).to(torch.int8) + 3 * (a == -INF).to(torch.int8)).cpu().numpy()


def adam_fp32(p, g, m, v, step, clamp, scale, order):
    """one step of hint::adam_update in numpy float32 (no fused multiply-add); order 0: ((1 - b2) * g) * g, 1: (1 - b2) * (g * g)"""
    f = np.float32
    b1, b2 = (f(b) for b in HYPER["betas"])
    with np.errstate(all="ignore"):
        gj = g * f(scale)
        if clamp > 0:
            gj = np.where(gj < -f(clamp), -f(clamp), np.where(gj > f(clamp), f(clamp), gj)).astype(f)
        gj = gj + f(HYPER["weight_decay"]) * p
        m = b1 * m + (f(1) - b1) * gj
        sq = ((f(1) - b2) * gj) * gj if order == 0 else (f(1) - b2) * (gj * gj)
        v = b2 * v + sq
        lr_t = f(HYPER["lr"] / (1.0 - HYPER["betas"][0] ** step))
        bc2 = f(1.0 / np.sqrt(1.0 - HYPER["betas"][1] ** step))
        p = p - lr_t * (m / (np.sqrt(v) * bc2 + f(HYPER["eps"])))
    return p.astype(f), m.astype(f), v.astype(f)


def torch_reference(t: Table, clamp: float, scale: float, device="cpu"):
    """the statements the header cites, in fp32 on `device`: [per step: per segment (p, m, v) tensors]"""
    ps = [torch.from_numpy(p.copy()).to(device).requires_grad_(True) for p in t.p]
    gs = [torch.from_numpy(g.copy()).to(device) for g in t.g]
    opt = torch.optim.Adam(ps, foreach=False, **HYPER)
    for p, m, v in zip(ps, t.m, t.v):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.from_numpy(m.copy()).to(device),
                        "exp_avg_sq": torch.from_numpy(v.copy()).to(device)}
    out = []
    for _ in range(STEPS):
        for p, g in zip(ps, gs):
            p.grad = g.mul(scale)
            if clamp > 0:
                p.grad.data.clamp_(-clamp, clamp)
        opt.step()
        out.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps])
    return out


# ---- spoiled rows -----------------------------------------------------------------------------------------------------------
@dataclass
class RowCase:
    name: str
    entry: str                       # "block" | "chain"
    d: int
    dc: int
    widths: tuple
    nr: int                          # rows per lane group the case is declared to run (wave-local row pairs: 2)
    expect: Tuple[str, str, str, str]
    n_blocks: int = 1
    scale: float = 0.05
    knobs: Dict[str, str] = field(default_factory=dict)

    @property
    def B(self) -> int:
        """two full 16 * nr-row tiles and a ragged third"""
        return 2 * 16 * self.nr + 5


ROW_CASES = [
    RowCase("wl_nr1", "block", 6, 0, (24, 12), 1, WL_F(1, "false") + ("hint_wl_bwd_kernel<1, false>", DW("false", "false"))),
    RowCase("wl_nr2", "block", 6, 0, (24, 12), 2, WL_F(2, "false") + ("hint_wl_bwd_kernel<2, false>", DW("false", "false")),
            knobs={"HINT_WL_NR": "2"}),
    RowCase("n3_cond", "block", 8, 3, (64, 32, 16), 1, GEN_F("false") + ("hint_bwd_kernel_n3", DW("false", "false"))),
    RowCase("bwd_cond", "block", 40, 2, (128, 64), 1, GEN_F("false") + ("hint_bwd_kernel", DW("false", "false"))),
    RowCase("subtree", "block", 43, 0, (67, 33, 16, 8), 1, GEN_F("false") + ("hint_bwd_kernel_n3", DW("true", "true"))),
    RowCase("fly", "block", 100, 0, (32, 16, 8), 1, GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")), scale=0.03),
]
CHAIN_CASES = [
    RowCase("wl_chain", "chain", 6, 0, (140, 70, 35, 17), 1, WL_F(1, "true") + ("hint_wl_bwd_kernel<1, true>", DW("false", "false")),
            n_blocks=2),
    RowCase("fly_chain", "chain", 100, 0, (32, 16, 8), 1, GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")),
            n_blocks=2, scale=0.03),
]
CONTENTS = ("nan lane", "+inf lane", "-inf lane", "nan row", "nan condition")


def spoil_plan(case: RowCase):
    """{row: content}: row 0, the last row of the ragged tile, a row in the middle of a full tile, both rows of one row pair and
    one row of another (nr = 2: rows r and r + 16 of a 32-row tile share their lanes' registers), and the whole second tile;
    the contents cycle ("nan condition" only where the case has a condition)"""
    nr, B = case.nr, case.B
    tile = 16 * nr
    rows = [0, B - 1, 7]
    if nr == 2:
        rows += [3, 3 + 16, 5]                                        # a whole pair (3, 19) and one row (5) of the pair (5, 21)
    rows += list(range(tile, 2 * tile))
    contents = [c for c in CONTENTS if c != "nan condition" or case.dc > 0]
    return {r: contents[i % len(contents)] for i, r in enumerate(dict.fromkeys(rows))}


def spoil(x, c, plan, lane_seed=5):
    """copies of x [B, d] and c [B, dc] (or None) with the plan's rows spoiled"""
    x, c = x.clone(), (c.clone() if c is not None else None)
    rng = np.random.RandomState(lane_seed)
    for r, what in plan.items():
        lane = int(rng.randint(x.shape[1]))
        if what == "nan row":
            x[r] = NAN
        elif what == "nan condition":
            c[r, int(rng.randint(c.shape[1]))] = NAN
        else:
            x[r, lane] = {"nan lane": NAN, "+inf lane": INF, "-inf lane": -INF}[what]
    return x, c


def row_inputs(case: RowCase, seed=11):
    """clean x, c, z (the inverse's input), g_z, g_J of a case, float32"""
    g = torch.Generator().manual_seed(seed)
    B = case.B
    x = torch.randn(B, case.d, generator=g)
    c = torch.randn(B, case.dc, generator=g) if case.dc else None
    zi = torch.randn(B, case.d, generator=g)
    gz = torch.randn(B, case.d, generator=g)
    gJ = torch.randn(B, generator=g)
    return x, c, zi, gz, gJ


def block_params(case: RowCase):
    nodes = orc.build_nodes(case.d, [(case.dc,)] if case.dc else [], list(case.widths))
    return nodes, orc.init_params(nodes, seed=5, scale=case.scale)


def chain_oracle(case: RowCase):
    """OracleFlow in float64 on float32-representable weights (make_chain_pair of test_gpu_instances.py)"""
    ref = orc.OracleFlow(case.d, case.n_blocks, list(case.widths), seed=3, init_scale=case.scale, dtype=torch.float64)
    ref.params = [{k: v.float().double() for k, v in P.items()} for P in ref.params]
    ref.perms = [None if p is None else p.float().double() for p in ref.perms]
    return ref


@functools.lru_cache(maxsize=None)
def oracle_rows(name: str):
    """the float64 oracle on the spoiled batch of a case: boolean rows [B] - objective 0.5 |z|^2 - J non-finite, inverse x row
    non-finite (the spoiled values in z), and the spoiled-row mask"""
    case = next(c for c in ROW_CASES + CHAIN_CASES if c.name == name)
    x, c, zi, _, _ = row_inputs(case)
    plan = spoil_plan(case)
    xs, cs = spoil(x, c, plan)
    zs, _ = spoil(zi, c, {r: w for r, w in plan.items() if w != "nan condition"})
    cd = [cs.double()] if case.dc else ()
    with torch.no_grad():
        if case.entry == "block":
            nodes, P = block_params(case)
            P64 = {k: v.double() for k, v in P.items()}
            z, J = orc.block_apply(nodes, P64, xs.double(), cd, rev=False)
            xi, _ = orc.block_apply(nodes, P64, zs.double(), cd, rev=True)
        else:
            ref = chain_oracle(case)
            z, J = ref.forward(xs.double(), tuple(cd))
            xi, _ = ref.inverse(zs.double(), tuple(cd))
    obj = 0.5 * (z ** 2).sum(1) - J
    mask = torch.zeros(case.B, dtype=torch.bool)
    mask[list(plan)] = True
    return ~torch.isfinite(obj), ~torch.isfinite(xi).all(dim=1), mask


# ---- the exact kink ---------------------------------------------------------------------------------------------------------
KINK_CASE = RowCase("kink_cond", "block", 8, 3, (64, 32, 16), 1, GEN_F("false") + ("hint_bwd_kernel_n3", DW("false", "false")))
KINK_ROWS = (0, 9, 17, 36)          # all-zero rows of x and c (B = 37: the first and the last row among them)


def kink_setup():
    """a block whose first-layer biases are all zero and a batch with all-zero rows of x and c: on those rows every first-layer
    pre-activation is exactly 0 in any summation order, and torch's relu'(0) = 0 is the only convention in play"""
    case = KINK_CASE
    nodes, P = block_params(case)
    P = {k: (torch.zeros_like(v) if k.endswith(".0.bias") else v) for k, v in P.items()}
    x, c, _, gz, gJ = row_inputs(case, seed=12)
    keep = torch.zeros(case.B, dtype=torch.bool)
    keep[list(KINK_ROWS)] = True
    x[keep] = 0.0
    c[keep] = 0.0
    return case, nodes, P, x, c, gz * keep[:, None], gJ * keep


# ---- a poisoned step --------------------------------------------------------------------------------------------------------
POISON_B = ss.RAGGED            # 173
POISON_ROW = 77


def poisoned_batches(flow_name: str):
    """[(x, c)] of the four steps and the nll batch, float32: step 3's row POISON_ROW is NaN"""
    spec = ss.FLOWS[flow_name]
    g = torch.Generator().manual_seed(4242)
    out = []
    for i in range(5):
        x = torch.randn(POISON_B, spec["d"], generator=g)
        c = torch.randn(POISON_B, spec["dc"], generator=g) if spec["dc"] else None
        if i == 2:
            x[POISON_ROW] = NAN
        out.append((x, c))
    return out


@functools.lru_cache(maxsize=None)
def poisoned_reference(flow_name: str):
    """OracleFlow.train_step in float64 on poisoned_batches: dict(losses [4, 2], nll, nan_params: tensors with a NaN)"""
    be = ss.OracleBackend(ss.FLOWS[flow_name], torch.float64)
    bt = poisoned_batches(flow_name)
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    try:
        losses = [be.step(x, c) for x, c in bt[:4]]
        nll = be.eval_nll(*bt[4])
    finally:
        torch.set_num_threads(nt)
    nan_params = sum(1 for p in be.flow.parameters() if bool(torch.isnan(p).any()))
    return dict(losses=np.array(losses, dtype=np.float64), nll=float(nll), nan_params=nan_params,
                n_params=len(be.flow.parameters()))
