"""The geometry ledger of part B without a GPU (tests/wgrad_geometry.py): every target resolves to a batch size at 256 CUs and again
at 128, hint_plan_check_dispatch shows what each declares, and the union over the trees reaches every batch-split geometry of
hint_wgrad_kernel / hint_wreduce_kernel that the GPU test (tests/test_gpu_wgrad_geometry.py) is meant to compare with the float64
oracle.  When a threshold of wgrad_splits (hint_abi.cpp) moves, the assertions name the geometry that lost its case."""
import os
import re

import pytest

from hint_amd import _lib
import wgrad_geometry as wg
from instance_cases import KNOBS_EXCLUDED

CUS = (256, 128)
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hint_amd", "csrc", "hint_wgrad.hip")


@pytest.fixture(scope="module")
def ledgers():
    """CU count -> every resolved geometry of every tree"""
    lib = _lib.load()
    try:
        return {cu: [g for t in wg.TREES for g in wg.Resolver(lib, t, cu).all()] for cu in CUS}
    finally:
        lib.hint_debug_reload_knobs()


def test_print_ledger(ledgers, capsys):
    with capsys.disabled():         # (the table is the point of this test: shown under -q too)
        for cu in CUS:
            print(f"\npart-B geometry ledger at {cu} CUs: {len(ledgers[cu])} batches")
            # (the 49 tiny sizes of a tree but the first of each split count, and the many split changes of the wave-local tree
            #  past 1000 rows, are left out of the table: the tests below go through all of them)
            seen = set()
            shown = []
            for g in ledgers[cu]:
                key = (g.tree.name, g.family, g.splits) if g.family == "tiny" else \
                      (g.tree.name, g.family, g.splits, g.label) if g.family == "splits" and g.B > 1000 else id(g)
                if key not in seen:
                    seen.add(key)
                    shown.append(g)
            print("\n".join(wg.table_lines(shown)))


def test_constants_mirror_the_kernel_source():
    text = open(SRC).read()
    for name, pattern in wg.SOURCE_LINES.items():
        m = re.search(pattern, text)
        assert m, f"hint_wgrad.hip no longer has the line {pattern!r} that wgrad_geometry.{name} mirrors"
        assert int(m.group(1)) == getattr(wg, name), (name, m.group(1))
    assert wg.SOLO8_ROWS == 128
    assert "HINT_DW_SPLITS" not in " ".join(KNOBS_EXCLUDED), "HINT_DW_SPLITS has cases now: the `forced` targets"


def test_trees_are_the_instance_ledgers(ledgers):
    assert sorted({t.dw for t in wg.TREES}) == sorted(f"hint_wgrad_kernel<{s}, {w}>" for s in ("false", "true") for w in ("false", "true"))
    assert [t.name for t in wg.TREES if t.solo] == ["subtree_d43", "lean_d100", "split_root"]
    for t in wg.TREES:
        assert set(wg.families_of(t)) == {g.family for g in ledgers[256] if g.tree is t}, t.name


@pytest.mark.parametrize("cu", CUS)
def test_every_target_shows_what_it_declares(ledgers, cu):
    lib = _lib.load()
    disp = {t.name: wg.Dispatcher(lib, t) for t in wg.TREES}
    bad = [m for g in ledgers[cu] for m in [wg.check(lib, g, cu, disp[g.tree.name])] if m]
    assert not bad, "\n".join(bad)
    # the split follows the padded batch alone: the sizes that share one share the geometry
    for g in ledgers[cu]:
        if g.family == "steps":
            assert g.B % 16 == 1 and wg.check(lib, wg.Geo(g.tree, g.family, g.label, g.B + 15, g.splits, g.rows, g.grid), cu,
                                              disp[g.tree.name]) is None


@pytest.mark.parametrize("cu", CUS)
def test_tiny_targets(ledgers, cu):
    for t in wg.TREES:
        tiny = [g for g in ledgers[cu] if g.tree is t and g.family == "tiny"]
        assert [g.B for g in tiny] == list(range(1, 50)), t.name
        assert {g.splits for g in tiny} == {1, 2, 3, 4}, (t.name, "tiny: split counts")
        assert {g.last_valid for g in tiny} == set(range(1, 17)), (t.name, "tiny: residues of the last block")
        # rows_per_wg = 16: wavefront 1 has nothing and returns in front of the LDS combine
        assert all(g.rows == 16 and g.steps == ((1, 0), (1, 0)) and g.map == "plain" for g in tiny), t.name


@pytest.mark.parametrize("cu", CUS)
def test_steps_targets(ledgers, cu):
    for t in wg.TREES:
        steps = [g for g in ledgers[cu] if g.tree is t and g.family == "steps"]
        full, short = steps[0::2], steps[1::2]
        # every split full, one valid row in the last block: the per-wavefront step counts (1,0), (1,1), (2,1) .. (5,5) - both
        # exits of dw_gen's ping-pong (last1: odd, last2: even counts) and ring fills of 1, 2, 3 and 4+ steps
        assert [g.rows for g in full] == list(wg.STEP_ROWS), t.name
        for g, pair in zip(full, wg.STEP_PAIRS):
            assert set(g.split_rows) == {g.rows} and g.last_valid == 1, (g.id, g.split_rows, g.last_valid)
            assert g.steps == (pair, pair), (g.id, g.steps, "declared", pair)
        lost = set(wg.STEP_PAIRS) - {g.steps[0] for g in full}
        assert not lost, f"{t.name}: per-wavefront step pairs without a case: {sorted(lost)}"
        assert {min(w0, 4) for g in full for w0, _ in [g.steps[0]]} == {1, 2, 3, 4}, (t.name, "ring fills")
        # the shortest last split the dispatch allows: all splits but the last full, and for most R a last split of one row (one step
        # of wavefront 0, none of wavefront 1) at B = (S - 1) R + 1; not where S splits of fewer rows would do (R >= 144 at 8 splits)
        for g in short:
            assert g.last_valid == 1 and set(g.split_rows[:-1]) == {g.rows}, g.id
            assert (g.steps[1] == (1, 0)) == (g.B == (g.splits - 1) * g.rows + 1), (g.id, g.B, g.steps)
        assert sum(g.steps[1] == (1, 0) for g in short) >= 7, (t.name, [g.steps[1] for g in short])


@pytest.mark.parametrize("cu", CUS)
def test_solo8_targets(ledgers, cu):
    for t in wg.TREES:
        s8 = [g for g in ledgers[cu] if g.tree is t and g.family == "solo8"]
        if not t.solo:
            assert not s8
            continue
        assert [g.rows for g in s8] == list(wg.SOLO8_TARGET_ROWS), t.name
        # dw_solo8 with 0, 1 and 2 iterations, with and without a remainder for dw_gen (no iteration and no remainder is no split)
        got = [(it, rem > 0) for g in s8 for it, rem in [wg.solo8(g.rows)]]
        assert got == [(0, True), (1, False), (1, True), (2, False), (2, True)], (t.name, got)
        for g in s8:
            assert set(g.split_rows) == {g.rows} and g.last_valid == 1, g.id       # (row indices clamped to rows - 1 in the last iteration)


@pytest.mark.parametrize("cu", CUS)
def test_splits_targets(ledgers, cu):
    lib = _lib.load()
    for t in wg.TREES:
        sp = [g for g in ledgers[cu] if g.tree is t and g.family == "splits"]
        assert len(sp) >= 2 * 20 and all(a.B + 1 == b.B and a.splits != b.splits for a, b in zip(sp[0::2], sp[1::2])), t.name
        # nothing between two listed changes changes: the batch sizes half way keep the split count of the change before them
        d = wg.Dispatcher(lib, t)
        firsts = [b for b in sp[1::2]]
        for a, b in zip(firsts, firsts[1:]):
            assert d((a.B + b.B) // 2, cu)["dw_splits"] == a.splits, (t.name, a.B, b.B)
        assert firsts[-1].B <= 4 * 16 * cu and firsts[0].B == 17


def test_union_reaches_every_geometry(ledgers):
    for cu in CUS:
        geos = ledgers[cu]
        counts = {g.splits for g in geos}
        lost = (set(range(1, 9)) - counts)
        assert not lost, f"{cu} CUs: split counts without a case: {sorted(lost)}"
        assert any(s >= 16 for s in counts), f"{cu} CUs: no case with 16 or more splits (thresholds of wgrad_splits moved?)"
        maps = {g.map for g in geos}
        assert maps == {"plain", "xcd", "interleaved"}, f"{cu} CUs: block mappings reached: {sorted(maps)}"
        # the interleaved mapping needs a chain of a wave-local tree at a multiple of 8 splits; below 8 splits the chain is not interleaved
        for n in wg.CHAIN_BLOCKS:
            ch = [g for g in geos if g.family == f"chain{n}"]
            assert {g.tree.name for g in ch} == {"production", "subtree_d43"} and all(g.n_chain == n for g in ch)
            assert any(g.map == "interleaved" for g in ch if g.tree.name == "production"), (cu, n)
            assert any(g.map == "plain" and g.splits < 8 for g in ch if g.tree.name == "production"), (cu, n)
            assert any(g.map == "xcd" for g in ch if g.tree.name == "subtree_d43"), (cu, n)
        forced = [g for g in geos if g.family == "forced"]
        assert sorted((g.tree.name, g.splits) for g in forced) == sorted((t, f) for t in wg.FORCED_TREES for f in wg.FORCED)
        assert all(900 <= g.B <= 1200 and g.last_valid == 7 for g in forced), [(g.id, g.B) for g in forced]
        assert {g.map for g in forced if g.splits in (3, 12)} == {"plain"}
        thin = [g for g in geos if g.family == "thin"]
        assert {g.tree.name for g in thin} == {"lean_d100"}
        assert sorted((g.grid, g.last_valid) for g in thin) == sorted((n, v) for n in wg.THIN_GRIDS for v in (1, 16))
        assert all(g.B in (16 * g.grid, 16 * g.grid - 15) for g in thin)


def test_resolver_follows_the_cu_count(ledgers):
    """fewer CUs, fewer splits for the trees with few jobs: the same target resolves to another batch size"""
    at = {cu: {g.id: g for g in ledgers[cu] if g.tree.name == "wl_24_12" and g.family == "steps"} for cu in CUS}
    g256, g128 = at[256]["wl_24_12/steps/R=160 full, last block 1 row"], at[128]["wl_24_12/steps/R=160 full, last block 1 row"]
    assert g256.splits > g128.splits and g256.B > g128.B and g256.rows == g128.rows == 160
    assert max(g.splits for g in ledgers[256] if not g.knobs) > max(g.splits for g in ledgers[128] if not g.knobs)


def test_a_wrong_declaration_is_named():
    """the check the ledger rests on: a target that declares one 16-row step too many does not pass"""
    lib = _lib.load()
    g = wg.Resolver(lib, wg.TREE["production"], 256).steps()[4]
    assert wg.check(lib, g, 256) is None
    g.rows += 16
    assert "production/steps/R=48" in wg.check(lib, g, 256)


@pytest.mark.parametrize("tree_name", ["general_d40", "subtree_d43", "lean_d100"])
def test_one_step_is_far_over_the_bound(tree_name):
    """what the GPU comparison rests on, with the oracle alone: at the tree's LARGEST batch, where it weighs least, one 16-row step -
    what a loop of part B can drop or count twice - moves EVERY weight-gradient tensor by more than ten times what check_grads
    allows, and check_grads refuses the gradients of B - 16 rows as those of B.  Seen at 256 CUs: the least moved tensor 24.6 (d = 100),
    25.0 (d = 43), 28.5 (d = 40) times its bound - these three trees are the lowest - and 96 .. 261 times on the other five; the median
    tensor 190 .. 830 times.  (A single row moves the median tensor 28 .. 190 times its bound, but not every tensor: a few first-layer
    tensors of deep nodes get next to nothing from a row whose hidden units there are off.)"""
    import test_gpu_wgrad_geometry as T
    lib = _lib.load()
    tree = wg.TREE[tree_name]
    B = wg.pool_rows(lib, tree, 256)
    rows = T.pool(tree_name, 0, B)[:4]
    _, _, refs = T.oracle_prefixes(tree, 0, rows, [B - 16, B])
    less, ref = refs[B - 16], refs[B]
    gmax = max(float(v.abs().max()) for v in ref["gw"].values())
    for k, r in ref["gw"].items():
        moved = float((less["gw"][k] - r).abs().max())
        assert moved > 10 * (T.TOL_GW * float(r.abs().max()) + 1e-7 * gmax), (tree_name, B, k, moved, float(r.abs().max()))
    with pytest.raises(AssertionError):
        T.check_grads(tree_name, ref["gx"], ref["gc"], {k: v.float() for k, v in less["gw"].items()}, ref)
    T.check_grads(tree_name, ref["gx"], ref["gc"], {k: v.float() for k, v in ref["gw"].items()}, ref)
