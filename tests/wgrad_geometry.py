"""The geometry ledger of backward part B (hint_amd/csrc/hint_wgrad.hip: hint_wgrad_kernel<SMALL, WIDE> and hint_wreduce_kernel): how
a batch is cut into splits, 16-row steps per wavefront, dw_solo8 iterations and thin slabs, and the batch sizes that reach every
such shape.  The instance ledger (instance_cases.py) pins WHICH kernel runs; this one pins what that kernel's own loops do with the
batch, which wgrad_splits() (hint_abi.cpp) and the kernel decide.

One tree per part-B code path (TREES: the trees of instance_cases.CASES, so the instance each lands on is pinned there), and per
tree a list of TARGETS.  A target names a geometry - "rows_per_wg = 48, every split full, one valid row in the last block" - not a
batch size: a Resolver finds B with hint_plan_check_dispatch for a CU count (no device needed; on the GPU the device's count) and
states what the dispatch must show (dw_splits, dw_rows, grid).  tests/test_wgrad_geometry_cpu.py checks the resolved ledger and
what it reaches at 256 and 128 CUs; tests/test_gpu_wgrad_geometry.py asserts the same with hint_plan_dispatch on the real plan and
then compares every batch with the float64 oracle."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from instance_cases import CASES, DISPATCH, descs_for, knob_env

# ---- what the ledger mirrors of hint_wgrad.hip (tests/test_wgrad_geometry_cpu.py reads these lines back from the source)
DW_WAVES = 2            # "#define HINT_DW_WAVES 2": wavefront w of a shared job takes the 16-row blocks w, w + DW_WAVES, .. of its split
SOLO8_BLOCKS = 8        # dw_solo8: "constexpr int NS = 8;" 16-row blocks per iteration of `while (bb + 16 * NS <= cx.b_end)`
SOLO8_ROWS = 16 * SOLO8_BLOCKS      # 128 rows per dw_solo8 iteration; what is left of the split goes to dw_gen through cx.bb0
DW_LEAN_RING = 3        # "#define HINT_DW_LEAN_RING 3": dw_lean's ring is pre-filled with RING - 1 sets: fills of 1, 2, 3, 4+ steps differ
SOURCE_LINES = {"DW_WAVES": r"#define HINT_DW_WAVES (\d+)", "SOLO8_BLOCKS": r"constexpr int NS = (\d+);",
                "DW_LEAN_RING": r"#define HINT_DW_LEAN_RING (\d+)"}


# ---------------------------------------------------------------------------------------------------------------- trees
@dataclass(frozen=True)
class Tree:
    name: str
    d: int
    dc: int
    widths: tuple
    path: str                   # the part-B path it is here for
    case: str                   # the instance_cases.CASES entry whose tree this is (its part-B instance is pinned there)
    thin: bool = False          # fuse_dw1: first-layer gradients come as one slab per workgroup of the backward kernel
    chain: bool = False         # also run as a chain of 2 and 3 blocks

    @property
    def _case(self):
        return next(c for c in CASES if c.name == self.case)

    @property
    def dw(self) -> str:        # hint_wgrad_kernel<SMALL, WIDE> instance
        c = self._case
        assert (c.d, c.dc, tuple(c.widths)) == (self.d, self.dc, self.widths), (self.name, self.case)
        return c.expect[3]

    @property
    def solo(self) -> bool:     # SMALL: single-tile jobs, one (job, split) per wavefront
        return self.dw.startswith("hint_wgrad_kernel<true")

    @property
    def scale(self) -> float:
        return self._case.scale

    @property
    def kink_cap(self) -> float:
        """share of pool candidates that may be discarded next to a ReLU kink: the instance ledger's caps (6 %, the d = 40 tree 19 %).
        Seen with the oracle alone, seeds 11..13, 4224 candidates: 0.3 % (24,12); 2.1-2.6 % production; 1.0-1.3 % d=8; 14.9-16.1 % d=40;
        2.3-2.9 % d=43; 3.1-3.6 % d=100; 5.1-5.3 % (448,64); 1.5-2.0 % d=12"""
        return 0.19 if self.d == 40 else 0.06


TREES = [
    Tree("wl_24_12", 6, 0, (24, 12), "wave-local, <false, false>", "wl_nr1_block"),
    Tree("production", 6, 0, (140, 70, 35, 17), "3x3 tiles with 12-byte loads (pvec / qvec)", "wl_nr1_chain", chain=True),
    Tree("cond_d8", 8, 3, (64, 32, 16), "a c operand with rows = B", "n3_cond_block_big_s"),
    Tree("general_d40", 40, 2, (128, 64), "general non-lean", "bwd_cond_block_big_s"),
    Tree("subtree_d43", 43, 0, (67, 33, 16, 8), "<true, true>: solo jobs, dw_solo8, lean-wide", "subtree_block_big_s", chain=True),
    Tree("lean_d100", 100, 0, (32, 16, 8), "lean dw_lean, thin slabs", "fly_block_multi", thin=True),
    Tree("split_root", 6, 0, (448, 64), "<true, false>, split root", "dw_small_split_root_block"),
    Tree("wide_d12", 12, 0, (48, 24), "<false, true>", "dw_wide_alt4_block"),
]
TREE = {t.name: t for t in TREES}

# a chain whose kink share (the Spy rule over the whole chain) is over the tree's cap gets a cap of its own here: (tree, n_blocks) ->
# the share the oracle shows plus 3 points (as MAX_KINK_ROWS does).  Seen, seed 11, some 420 candidates: production 2 blocks 3.4 %,
# 3 blocks 4.9 %; subtree_d43 2 blocks 3.9 % (all under the trees' 6 %), subtree_d43 3 blocks 6.2 %
CHAIN_KINK_CAP = {("subtree_d43", 3): 0.092}


def chain_kink_cap(tree: Tree, n_blocks: int) -> float:
    return CHAIN_KINK_CAP.get((tree.name, n_blocks), tree.kink_cap)


# ------------------------------------------------------------------------------------------------------------- dispatch
class Dispatcher:
    """hint_plan_check_dispatch of one tree with the node table built once (a call is then a millisecond)"""

    def __init__(self, lib, tree: Tree):
        self.lib, self.tree = lib, tree
        self.descs, self.n = descs_for(tree.d, tree.dc, tree.widths)
        self.out = (C.c_int32 * len(DISPATCH))()

    def __call__(self, B: int, cu: int, n_chain: int = 1) -> Dict[str, int]:
        """the launch decision for B rows on cu CUs.  n_chain > 1: part B of a chain of n_chain blocks.  The entry point reports
        one block's split; a chain's differs only through `splits * n_wjobs * n_chain < num_cu` in wgrad_splits (hint_abi.cpp),
        which for integers is `splits * n_wjobs < ceil(num_cu / n_chain)`: dw_splits and dw_rows are taken from the decision for
        that many CUs, everything else from the decision for cu"""
        t = self.tree
        st = self.lib.hint_plan_check_dispatch(self.descs, self.n, t.d, t.dc, 4.0, B, cu, self.out, len(DISPATCH))
        assert st == 0, self.lib.hint_last_error().decode()
        disp = dict(zip(DISPATCH, list(self.out)))
        if n_chain > 1:
            st = self.lib.hint_plan_check_dispatch(self.descs, self.n, t.d, t.dc, 4.0, B, -(-cu // n_chain), self.out, len(DISPATCH))
            assert st == 0, self.lib.hint_last_error().decode()
            sub = dict(zip(DISPATCH, list(self.out)))
            disp["dw_splits"], disp["dw_rows"] = sub["dw_splits"], sub["dw_rows"]
        return disp


def pad16(B: int) -> int:
    return (B + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------- what a geometry is
def split_rows(splits: int, rows: int, B: int) -> List[int]:
    """padded rows of every split: hint_wgrad_kernel's b_begin = split * rows_per_wg, b_end = min(Bp, b_begin + rows_per_wg)"""
    Bp = pad16(B)
    return [min(Bp, (s + 1) * rows) - s * rows for s in range(splits)]


def wave_steps(n_rows: int) -> Tuple[int, ...]:
    """16-row steps of every wavefront of a shared job over a split of n_rows (padded) rows: cx.bb0 = b_begin + 16 wave, cx.step =
    16 DW_WAVES"""
    k = n_rows // 16
    return tuple(max(0, (k - w + DW_WAVES - 1) // DW_WAVES) for w in range(DW_WAVES))


def solo8(n_rows: int) -> Tuple[int, int]:
    """(dw_solo8 iterations, 16-row blocks left for dw_gen) of a solo job over a split of n_rows (padded) rows"""
    return n_rows // SOLO8_ROWS, n_rows % SOLO8_ROWS // 16


def mapping(disp_wl: int, splits: int, n_chain: int) -> str:
    """how hint_wgrad_kernel maps block ids to (item, split): `(splits & 7) == 0` is the XCD mapping, anything else the plain one; a
    chain whose jobs the planner sorted (the wave-local plans: P->wsorted) runs the XCD mapping interleaved over its blocks
    (launch_wgrad: grid_pb < 0)"""
    if splits & 7:
        return "plain"
    return "interleaved" if disp_wl and n_chain > 1 else "xcd"


@dataclass
class Geo:
    """a resolved target: the batch size and what the dispatch must show for it"""
    tree: Tree
    family: str
    label: str                  # the geometry in words
    B: int
    splits: int                 # declared dw_splits
    rows: int                   # declared dw_rows (rows_per_wg)
    grid: int                   # declared workgroups of the row kernels = thin slabs where the tree has them
    wl: int = 0
    n_chain: int = 1
    knobs: Dict[str, str] = field(default_factory=dict)

    @property
    def split_rows(self):
        return split_rows(self.splits, self.rows, self.B)

    @property
    def steps(self):            # per-wavefront steps of the first (full) and of the last split
        r = self.split_rows
        return wave_steps(r[0]), wave_steps(r[-1])

    @property
    def last_valid(self):       # rows of the last 16-row block that are inside the batch (the x and c operands end there)
        return self.B - (pad16(self.B) - 16)

    @property
    def map(self):
        return mapping(self.wl, self.splits, self.n_chain)

    @property
    def id(self):
        return f"{self.tree.name}/{self.family}/{self.label}"

    def mismatch(self, disp: Dict[str, int]) -> Optional[str]:
        """None when a dispatch decision shows what this geometry declares; else what differs"""
        got = (disp["dw_splits"], disp["dw_rows"], disp["grid"])
        if got != (self.splits, self.rows, self.grid):
            return (f"{self.id}: B={self.B} on {disp['num_cu']} CUs dispatches (dw_splits, dw_rows, grid) = {got}, "
                    f"declared {(self.splits, self.rows, self.grid)}")
        r = self.split_rows
        if min(r) < 16 or sum(r) != pad16(self.B):
            return f"{self.id}: B={self.B}: splits of {r} rows do not tile the {pad16(self.B)} padded rows"
        return None


# --------------------------------------------------------------------------------------------------------------- targets
TINY = range(1, 50)                                          # every B: 1..4 splits, every residue of the last block, rows_per_wg = 16
STEP_ROWS = tuple(range(16, 161, 16))                        # rows_per_wg of the `steps` targets
STEP_PAIRS = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5)]       # .. and the steps of wavefronts 0, 1 there
SOLO8_TARGET_ROWS = (112, 128, 144, 256, 272)                # dw_solo8: 0, 1, 1, 2, 2 iterations; remainder, none, remainder, none, remainder
FORCED = (3, 12, 64)                                         # HINT_DW_SPLITS
FORCED_TREES = ("production", "subtree_d43")
THIN_GRIDS = (1, 2, 7, 8, 9, 55, 56, 57, 63, 64, 65, 71, 72, 73, 127, 128, 129)    # hint_wreduce_kernel: `w + 56 < thin_slabs`, per q = 0..7
CHAIN_BLOCKS = (2, 3)
FAMILIES = ("tiny", "steps", "solo8", "splits", "forced", "thin")


_TABLES: Dict[tuple, Dict[int, Tuple[int, int]]] = {}


class Resolver:
    """targets -> batch sizes, for one tree and CU count"""

    def __init__(self, lib, tree: Tree, cu: int):
        self.lib, self.tree, self.cu = lib, tree, cu
        self.disp = Dispatcher(lib, tree)

    def geo(self, family, label, B, n_chain=1, knobs=None, **declared) -> Geo:
        """the geometry at B as the dispatch for (cu, n_chain) shows it, with `declared` values in its place where the target states them"""
        d = self.disp(B, self.cu, n_chain)
        g = Geo(self.tree, family, label, B, d["dw_splits"], d["dw_rows"], d["grid"], d["wl"], n_chain, dict(knobs or {}))
        for k, v in declared.items():
            setattr(g, k, v)
        return g

    def table(self, n_chain: int = 1) -> Dict[int, Tuple[int, int]]:
        """padded batch size -> (dw_splits, dw_rows), every multiple of 16 up to 4 * 16 * num_cu (the split depends on B through
        rows_padded(B) alone; default knobs).  Kept per (tree, CU count, chain length): a dispatch call builds a host plan"""
        key = (self.tree.name, self.cu, n_chain)
        if key not in _TABLES:
            out = {}
            for Bp in range(16, 4 * 16 * self.cu + 16, 16):
                d = self.disp(Bp, self.cu, n_chain)
                out[Bp] = (d["dw_splits"], d["dw_rows"])
            _TABLES[key] = out
        return _TABLES[key]

    # -- one family at a time
    def tiny(self):
        return [self.geo("tiny", f"B={B}", B) for B in TINY]

    def _rows_target(self, family, R, n_chain=1):
        """rows_per_wg = R at the split count S dispatched there (of the largest batch with that R): every split full with one
        valid row in the last block, and the shortest last split the dispatch allows (one row while R <= 128 at 8 splits)"""
        tab = self.table(n_chain)
        have = [Bp for Bp, (_, r) in tab.items() if r == R]
        assert have, f"{self.tree.name}: no batch up to {max(tab)} rows has rows_per_wg = {R}"
        S = tab[max(have)][0]
        full = S * R
        assert tab.get(full) == (S, R), f"{self.tree.name}: {S} full splits of {R} rows dispatch as {tab.get(full)}"
        short = min(Bp for Bp in have if tab[Bp] == (S, R))
        return S, [self.geo(family, f"R={R} full, last block 1 row", full - 15, n_chain, splits=S, rows=R),
                   self.geo(family, f"R={R} short last split", short - 15, n_chain, splits=S, rows=R)]

    def steps(self):
        return [g for R in STEP_ROWS for g in self._rows_target("steps", R)[1]]

    def solo8(self):
        if not self.tree.solo:
            return []
        return [self._rows_target("solo8", R)[1][0] for R in SOLO8_TARGET_ROWS]

    def changes(self, n_chain=1) -> List[int]:
        """every B in 2 .. 4 * 16 * num_cu whose dw_splits differs from B - 1's: multiples of 16 scanned, then refined"""
        tab = self.table(n_chain)
        out = []
        for Bp in sorted(tab)[1:]:
            if tab[Bp][0] != tab[Bp - 16][0]:
                first = next(B for B in range(Bp - 15, Bp + 1) if self.disp(B, self.cu, n_chain)["dw_splits"] != tab[Bp - 16][0])
                out.append(first)
        return out

    def splits(self):
        out = []
        for B in self.changes():
            out += self._sides("splits", B)
        return out

    def _sides(self, family, B, n_chain=1):
        a, b = self.geo(family, "", B - 1, n_chain), self.geo(family, "", B, n_chain)
        a.label, b.label = f"{a.splits}->{b.splits} splits: last B before", f"{a.splits}->{b.splits} splits: first B after"
        return [a, b]

    def forced(self):
        """HINT_DW_SPLITS = 3, 12 (a non-multiple-of-8 mapping where the default takes the XCD mapping) and 64 (a long slab sum), each at
        the B nearest to 1000 whose dispatch then shows exactly that many splits, 7 valid rows in the last block.  To be resolved
        with the knob set (forced_env)"""
        if self.tree.name not in FORCED_TREES:
            return []
        out = []
        for f in FORCED:
            with forced_env(self.lib, f):
                hit = [Bp for Bp in range(800, 1216, 16) if self.disp(Bp, self.cu)["dw_splits"] == f]
                assert hit, f"{self.tree.name}: HINT_DW_SPLITS={f} gives {f} splits at no batch of 800..1200 rows"
                Bp = min(hit, key=lambda b: abs(b - 1000))
                out.append(self.geo("forced", f"HINT_DW_SPLITS={f}", Bp - 9, knobs={"HINT_DW_SPLITS": str(f)}, splits=f))
        return out

    def thin(self):
        if not self.tree.thin:
            return []
        return [self.geo("thin", f"{g} slabs, last block {v} row(s)", B, grid=g)
                for g in THIN_GRIDS for B, v in ((16 * g, 16), (16 * g - 15, 1))]

    def chain(self, n_blocks):
        """part B of a chain of n_blocks blocks (a permutation on every block): one tiny size below 8 splits (so not interleaved),
        one `steps` size, and both sides of one change of the split count (the first one past 8 splits)"""
        if not self.tree.chain:
            return []
        fam = f"chain{n_blocks}"
        out = [self.geo(fam, "tiny B=37", 37, n_blocks)]
        assert out[0].splits < 8
        out.append(self._rows_target(fam, 48, n_blocks)[1][0])
        tab = self.table(n_blocks)
        B = next(B for B in self.changes(n_blocks) if tab[pad16(B - 1)][0] == 8)
        return out + self._sides(fam, B, n_blocks)

    def family(self, name) -> List[Geo]:
        return self.chain(int(name[5:])) if name.startswith("chain") else getattr(self, name)()

    def all(self) -> List[Geo]:
        return [g for f in FAMILIES + tuple(f"chain{n}" for n in CHAIN_BLOCKS) for g in self.family(f)]


class forced_env:
    """HINT_DW_SPLITS set for the library (and cleared again): wgrad_splits reads the knob at every dispatch"""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        import pytest
        self.mp = pytest.MonkeyPatch()
        knob_env(self.mp, self.lib, {"HINT_DW_SPLITS": str(self.value)})

    def __exit__(self, *exc):
        self.mp.undo()
        self.lib.hint_debug_reload_knobs()


def families_of(tree: Tree) -> List[str]:
    """the target families a tree has (the GPU test's parametrisation)"""
    out = ["tiny", "steps", "splits"]
    if tree.solo:
        out.append("solo8")
    if tree.name in FORCED_TREES:
        out.append("forced")
    if tree.thin:
        out.append("thin")
    if tree.chain:
        out += [f"chain{n}" for n in CHAIN_BLOCKS]
    return out


_POOL_ROWS: Dict[tuple, int] = {}


def pool_rows(lib, tree: Tree, cu: int) -> int:
    """rows of the tree's pool: the largest batch of any of its one-block targets (every family's batches are prefixes of ONE pool)"""
    key = (tree.name, cu)
    if key not in _POOL_ROWS:
        _POOL_ROWS[key] = max(g.B for g in Resolver(lib, tree, cu).all() if g.n_chain == 1)
    return _POOL_ROWS[key]


def check(lib, geo: Geo, cu: int, disp: Optional[Dispatcher] = None) -> Optional[str]:
    """a resolved geometry against hint_plan_check_dispatch (its knobs set): None, or what differs"""
    disp = disp or Dispatcher(lib, geo.tree)
    if geo.knobs:
        with forced_env(lib, geo.knobs["HINT_DW_SPLITS"]):
            return geo.mismatch(disp(geo.B, cu, geo.n_chain))
    return geo.mismatch(disp(geo.B, cu, geo.n_chain))


def table_lines(geos: List[Geo]) -> List[str]:
    out = [f"{'tree':12s} {'family':7s} {'geometry':44s} {'B':>6s} {'S':>3s} {'R':>4s} {'steps w0,w1 first / last split':>30s} "
           f"{'solo8 it,rem':>12s} {'last':>4s} {'grid':>5s} map"]
    for g in geos:
        r = g.split_rows
        (f0, f1) = g.steps
        s8 = f"{solo8(r[0])} {solo8(r[-1])}" if g.tree.solo else ""
        out.append(f"{g.tree.name:12s} {g.family:7s} {g.label:44s} {g.B:6d} {g.splits:3d} {g.rows:4d} {str(f0) + ' / ' + str(f1):>30s} "
                   f"{s8:>12s} {g.last_valid:4d} {g.grid:5d} {g.map}")
    return out
