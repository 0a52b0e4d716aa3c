"""The thin widths the shape-specialised wave-local instances fold into their per-tile epilogues (hint_amd/csrc/hint_wl.hpp
wl_row: the forward's thin product behind the h x h layer has r outputs, the backward's cin), without a GPU.  No table field
carries a group's r for the forward: `thin_K` of a group is cin in the forward's schedule and r in the backward's, and the forward
instance reads r of group gi from the BACKWARD schedule's group gi.  That holds only while both schedules list the same groups
at the same indices, and while the schedules' widths are the tree's own - checked here through hint_plan_check_wl_shape for
both table entries (cfg 2: leaves 1 / 2, root 3 / 3; GAS: 1 / 1, 2 / 2, 4 / 4)."""
import os
import sys

import pytest

from hint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wl_shape_table as gen  # noqa: E402
from instance_cases import descs_for  # noqa: E402

CU = 256
# name -> (d, widths, batch, (cin, r) per group in the plan's order: deepest level first, the root last)
SHAPES = {"cfg2": (6, (140, 70, 35, 17), 4096, [(1, 2), (3, 3)]),
          "gas": (8, (128, 64, 32, 16), 8192, [(1, 1), (2, 2), (4, 4)])}
# what says WHICH group an index holds (thin_K is the one field that differs by direction on purpose)
IDENTITY = ("ent_begin", "ent_cnt", "level", "level_last", "n1", "ntt_min", "ntt_max", "cin", "kcp", "hw", "sl")


@pytest.fixture()
def lib(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("HINT_WL_STATIC", raising=False)
    monkeypatch.delenv("HINT_WL_NR", raising=False)
    lib.hint_debug_reload_knobs()
    yield lib
    monkeypatch.undo()
    lib.hint_debug_reload_knobs()


def schedules(lib, name):
    d, widths, B, _ = SHAPES[name]
    n_groups = gen.shape_fields(lib, d, widths, B, CU, 0)[1][gen.fold_fields().index("a_n_groups")]
    assert n_groups == gen.shape_fields(lib, d, widths, B, CU, 1)[1][gen.fold_fields().index("a_n_groups")]
    fwd, _ = gen.sched_fields(lib, d, widths, B, CU, 0)
    bwd, _ = gen.sched_fields(lib, d, widths, B, CU, 1)
    return n_groups, fwd, bwd


@pytest.mark.parametrize("name", list(SHAPES))
def test_thin_widths_of_every_group_are_the_trees(lib, name):
    d, widths, B, expect = SHAPES[name]
    n_groups, fwd, bwd = schedules(lib, name)
    assert n_groups == len(expect)
    descs, n = descs_for(d, 0, widths)
    deepest = max(descs[i].depth for i in range(n))
    assert deepest + 1 == n_groups
    for g in range(n_groups):
        nodes = [descs[i] for i in range(n) if descs[i].depth == deepest - g]       # group g = level g, the deepest first
        assert nodes and fwd[g]["level"] == g and bwd[g]["level"] == g
        cin, r = expect[g]
        assert {nd.k for nd in nodes} == {cin} and {nd.r for nd in nodes} == {r}, (name, g)
        assert fwd[g]["thin_K"] == cin, (name, g, fwd[g])        # forward: the inputs of the first layer in front of the rows
        assert fwd[g]["cin"] == cin and bwd[g]["cin"] == cin, (name, g)
        assert bwd[g]["thin_K"] == r, (name, g, bwd[g])          # backward: g_s | g_t of the r transformed lanes
        assert 1 <= cin <= 4 and 1 <= r <= 4


@pytest.mark.parametrize("name", list(SHAPES))
def test_both_directions_list_the_same_groups_at_the_same_indices(lib, name):
    n_groups, fwd, bwd = schedules(lib, name)
    for g in range(gen.MAX_G):
        for f in IDENTITY:
            assert fwd[g][f] == bwd[g][f], (name, g, f, fwd[g][f], bwd[g][f])
    for g in range(n_groups, gen.MAX_G):
        assert not any(fwd[g].values()) and not any(bwd[g].values())


@pytest.mark.parametrize("name", list(SHAPES))
def test_committed_table_holds_these_schedules(lib, name):
    """the instances read the committed table, not the planner: its text is what the generator prints for these schedules"""
    d, widths, B, _ = SHAPES[name]
    table = open(os.path.join(ROOT, "hint_amd", "csrc", "hint_wl_shape_table.hpp")).read()
    for backward in (0, 1):
        assert gen.sched_text(*gen.sched_fields(lib, d, widths, B, CU, backward)) in table
