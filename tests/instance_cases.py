"""The instance ledger: every row and part-B kernel instance the library compiles, and the GPU cases of
tests/test_gpu_instances.py that are meant to reach them.

A case names its entry point (one block through the module route, or a chain of blocks through hint_chain_*), the tree, the
condition width, a batch size written as a function of the device's CU count, and the four instances it is declared to run
(forward, inverse, backward part A, part B).  `MULTI` cases are declared to go round the row kernels' tile loop
`for (tg = blockIdx.x; tg < groups; tg += gridDim.x)` at least twice, with a ragged last pass (some workgroups do one pass
fewer).  tests/test_dispatch_cpu.py checks all of it against hint_plan_check_dispatch without a GPU; the GPU test asserts the
same with hint_plan_dispatch on the device it runs on before it compares anything."""
import ctypes as C
import re
import subprocess
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

DISPATCH = ["wl", "nr", "nw", "alt4", "tiles", "groups", "grid", "passes", "fwd", "bwd", "dw_small", "dw_wide", "dw_splits",
            "dw_rows", "n_sub", "lean", "leanw", "rowdw", "fuse_dw1", "num_cu"]        # include/hint_amd.h, HINT_DISPATCH_FIELDS

# the row kernels and part B (nm -C names without the argument list); the other kernels (pack, zero, reduction, optimizer,
# inverse-gradient helpers) are not chosen by the planner
INSTANCE_RE = re.compile(r"\b(hint_(?:wl_apply|wl_bwd|apply|bwd|wgrad)_kernel(?:_n3|_fly)?(?:<[^>()]*>)?)\(")


def compiled_instances(lib_path):
    """every row and part-B kernel instance in the library's symbol table"""
    out = subprocess.run(["nm", "-C", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return sorted({m.group(1) for line in out.splitlines() for m in [INSTANCE_RE.search(line)] if m})


def _b(v):
    return "true" if v else "false"


def instances_of(disp: Dict[str, int], entry: str) -> Tuple[str, str, str, str]:
    """(forward, inverse, backward, part B) instance of a dispatch decision (hint_plan_dispatch) for an entry point"""
    ch = _b(entry == "chain")
    if disp["fwd"] == 0:
        fwd = tuple(f"hint_wl_apply_kernel<{_b(rev)}, {disp['nr']}, {ch}>" for rev in (False, True))
    else:
        fwd = tuple(f"hint_apply_kernel<{_b(rev)}, {_b(disp['fwd'] == 2)}>" for rev in (False, True))
    bwd = [f"hint_wl_bwd_kernel<{disp['nr']}, {ch}>", "hint_bwd_kernel", "hint_bwd_kernel_n3", "hint_bwd_kernel_fly"][disp["bwd"]]
    return fwd + (bwd, f"hint_wgrad_kernel<{_b(disp['dw_small'])}, {_b(disp['dw_wide'])}>")


def families(disp: Dict[str, int]):
    """the row-kernel families a decision runs (the ledger wants a multi-pass case with a ragged last pass for each)"""
    f = {0: "wl forward", 1: "general forward FLY off", 2: "general forward FLY on"}[disp["fwd"]], \
        {0: "wl backward", 1: "bwd", 2: "n3", 3: "fly"}[disp["bwd"]]
    return set(f) | ({"subtree"} if disp["n_sub"] > 0 else set())


ROW_FAMILIES = {"wl forward", "wl backward", "general forward FLY off", "general forward FLY on", "bwd", "n3", "fly", "subtree"}


def multi_pass_b(cu: int, nr: int) -> int:
    """rows for one and a half grids of tile groups (grid capped at 8 workgroups per CU): two passes, the second ragged"""
    return 16 * nr * 12 * cu + 5


@dataclass
class Case:
    name: str
    entry: str                       # "block" | "chain"
    d: int
    dc: int
    widths: tuple
    batch: Callable[[int], int]      # B(num_cu)
    expect: Tuple[str, str, str, str]
    multi: bool = False              # declared: >= 2 passes of the tile loop, the last one ragged
    n_blocks: int = 1                # (chain cases)
    scale: float = 0.05              # weights randn * scale: s of order 1
    big_s: float = 0.0               # > 0: the root's s subnet's last layer times this: |s| >= 10 on many rows (atan's tail)
    knobs: Dict[str, str] = field(default_factory=dict)
    kink_cap: float = 0.06           # share of rows that may get zero cotangents next to a ReLU kink (the float64 oracle decides;
                                     # the caps are the shares seen at 256 CUs plus a margin: 0 .. 4.5 %, the d = 40 tree 16 %)

    def B(self, cu: int) -> int:
        return self.batch(cu)


WL_F = lambda nr, ch: (f"hint_wl_apply_kernel<false, {nr}, {ch}>", f"hint_wl_apply_kernel<true, {nr}, {ch}>")  # noqa: E731
GEN_F = lambda fly: (f"hint_apply_kernel<false, {fly}>", f"hint_apply_kernel<true, {fly}>")                    # noqa: E731
DW = lambda s, w: f"hint_wgrad_kernel<{s}, {w}>"                                                                 # noqa: E731

CASES = [
    # ---- wave-local kernels: one tile per workgroup (8-wavefront plan), row pairs on the 4- and on the 8-wavefront plan
    Case("wl_nr1_block", "block", 6, 0, (24, 12), lambda cu: 100,
         WL_F(1, "false") + ("hint_wl_bwd_kernel<1, false>", DW("false", "false"))),
    Case("wl_nr1_block_big_s", "block", 6, 0, (24, 12), lambda cu: 16 * cu - 3,
         WL_F(1, "false") + ("hint_wl_bwd_kernel<1, false>", DW("false", "false")), big_s=210.0),
    Case("wl_pairs_alt4_block_multi", "block", 6, 0, (24, 12), lambda cu: multi_pass_b(cu, 2),
         WL_F(2, "false") + ("hint_wl_bwd_kernel<2, false>", DW("false", "false")), multi=True),
    Case("wl_nr1_chain", "chain", 6, 0, (140, 70, 35, 17), lambda cu: 200,
         WL_F(1, "true") + ("hint_wl_bwd_kernel<1, true>", DW("false", "false")), n_blocks=2),
    Case("wl_pairs_nw8_chain_multi", "chain", 6, 0, (140, 70, 35, 17), lambda cu: multi_pass_b(cu, 2),
         WL_F(2, "true") + ("hint_wl_bwd_kernel<2, true>", DW("false", "false")), multi=True, n_blocks=2),
    # ---- general kernels without lean general groups: hint_apply_kernel<REV, false>
    Case("n3_alt4_cond_block_multi", "block", 8, 3, (64, 32, 16), lambda cu: multi_pass_b(cu, 1),
         GEN_F("false") + ("hint_bwd_kernel_n3", DW("false", "false")), multi=True),
    Case("n3_cond_block_big_s", "block", 8, 3, (64, 32, 16), lambda cu: 333,
         GEN_F("false") + ("hint_bwd_kernel_n3", DW("false", "false")), big_s=380.0),
    Case("bwd_cond_block_multi", "block", 40, 2, (128, 64), lambda cu: multi_pass_b(cu, 1),
         GEN_F("false") + ("hint_bwd_kernel", DW("false", "false")), multi=True, kink_cap=0.19),
    Case("bwd_cond_block_big_s", "block", 40, 2, (128, 64), lambda cu: 16 * cu + 7,
         GEN_F("false") + ("hint_bwd_kernel", DW("false", "false")), big_s=100.0, kink_cap=0.19),
    Case("subtree_block_multi", "block", 43, 0, (67, 33, 16, 8), lambda cu: multi_pass_b(cu, 1),
         GEN_F("false") + ("hint_bwd_kernel_n3", DW("true", "true")), multi=True),
    Case("subtree_block_big_s", "block", 43, 0, (67, 33, 16, 8), lambda cu: 200,
         GEN_F("false") + ("hint_bwd_kernel_n3", DW("true", "true")), big_s=120.0),
    # ---- lean general groups (the d = 100 trees, narrower than the workloads' so that the float64 oracle stays quick):
    #      hint_apply_kernel<REV, true>, hint_bwd_kernel_fly, a subtree level and rows that compute dW1 | db1 themselves
    Case("fly_block_multi", "block", 100, 0, (32, 16, 8), lambda cu: multi_pass_b(cu, 1),
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")), multi=True, scale=0.03),
    Case("fly_block_big_s", "block", 100, 0, (32, 16, 8), lambda cu: 160,
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")), scale=0.03, big_s=160.0, kink_cap=0.09),
    Case("fly_chain_multi", "chain", 100, 0, (32, 16, 8), lambda cu: multi_pass_b(cu, 1),
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")), multi=True, n_blocks=2, scale=0.03, kink_cap=0.09),
    # ---- the other part-B instances: single-tile jobs without lean-wide groups (split h > 384 root), lean-wide without them
    Case("dw_small_split_root_block", "block", 6, 0, (448, 64), lambda cu: 300,
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "false"))),
    Case("dw_wide_alt4_block", "block", 12, 0, (48, 24), lambda cu: 16 * cu + 100,
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("false", "true"))),
    # ---- knobs
    Case("knob_wl_nr1_block_multi", "block", 6, 0, (24, 12), lambda cu: multi_pass_b(cu, 1),
         WL_F(1, "false") + ("hint_wl_bwd_kernel<1, false>", DW("false", "false")), multi=True, knobs={"HINT_WL_NR": "1"}),
    Case("knob_no_bwd_fly_rowdw_block", "block", 100, 0, (32, 16, 8), lambda cu: 16 * cu + 9,
         GEN_F("true") + ("hint_bwd_kernel", DW("true", "true")), scale=0.03, knobs={"HINT_NO_BWD_FLY": "1"}),
    Case("knob_no_fuse_dw1_block", "block", 100, 0, (32, 16, 8), lambda cu: 100,
         GEN_F("true") + ("hint_bwd_kernel_fly", DW("true", "true")), scale=0.03, knobs={"HINT_FUSE_DW1": "0"}, kink_cap=0.1),
    Case("knob_dw_small_wl_block", "block", 6, 0, (24, 12), lambda cu: 100,
         WL_F(1, "false") + ("hint_wl_bwd_kernel<1, false>", DW("true", "false")), knobs={"HINT_DW_SMALL": "1"}),
]

# knobs with no case of their own, and why
KNOBS_EXCLUDED = {
    "HINT_WL=0": "routes wave-local trees to the general kernels: instances the default cases run",
    "HINT_SUB=0 / HINT_LEAN=0 / HINT_LEANW=0": "remove subtree / lean / lean-wide groups: plans of instances the default cases run",
    "HINT_NW / HINT_LEANW_MAX / HINT_PF": "experiment sizes (wavefronts, thin-layer width, L2 warm-up), no instance of their own "
                                          "(HINT_DW_SPLITS: the `forced` targets of wgrad_geometry.py)",
}


def descs_for(d, dc, widths):
    """the C node table of a block of this shape (the same table hint_amd builds for the module)"""
    import hint_amd
    from hint_amd.hint import node_descs
    blk = hint_amd.HierarchicalAffineCouplingBlock([(d,)], dims_c=[(dc,)] if dc else [], c_internal=list(widths))
    nodes = blk.tree._flat_nodes()
    descs, _, _, _ = node_descs(nodes)
    return descs, len(nodes)


def check_dispatch(lib, d, dc, widths, B, num_cu, clamp=4.0) -> Dict[str, int]:
    """hint_plan_check_dispatch: the launch decision of a host-only plan on a device of num_cu CUs"""
    descs, n = descs_for(d, dc, widths)
    out = (C.c_int32 * len(DISPATCH))()
    st = lib.hint_plan_check_dispatch(descs, n, d, dc, clamp, B, num_cu, out, len(DISPATCH))
    assert st == 0, lib.hint_last_error().decode()
    return dict(zip(DISPATCH, list(out)))


def plan_dispatch(lib, plan, B) -> Dict[str, int]:
    """hint_plan_dispatch: the launch decision of a device plan"""
    out = (C.c_int32 * len(DISPATCH))()
    st = lib.hint_plan_dispatch(plan, B, out, len(DISPATCH))
    assert st == 0, lib.hint_last_error().decode()
    return dict(zip(DISPATCH, list(out)))


def ragged(disp) -> bool:
    return disp["groups"] % disp["grid"] != 0


def mismatch(case: Case, disp: Dict[str, int]) -> Optional[str]:
    """None when the decision is what the case declares; else what differs"""
    got = instances_of(disp, case.entry)
    if got != case.expect:
        return f"{case.name}: runs {got}, declared {case.expect}"
    if case.multi and not (disp["passes"] >= 2 and ragged(disp)):
        return (f"{case.name}: declared multi-pass with a ragged last pass, runs {disp['passes']} pass(es) "
                f"({disp['groups']} tile groups on {disp['grid']} workgroups)")
    return None


def knob_env(monkeypatch, lib, knobs):
    """set a case's knobs (or none) and make the library re-read its environment"""
    for k in ("HINT_WL_NR", "HINT_NO_BWD_FLY", "HINT_FUSE_DW1", "HINT_DW_SMALL", "HINT_DW_SPLITS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    lib.hint_debug_reload_knobs()
