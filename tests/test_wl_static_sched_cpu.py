"""The level schedule of the shape-specialised wave-local instances without a GPU (hint_amd/csrc/hint_wl_shape.hpp WlSched): the
planner derives it by walking every row record, unit and coupling entry of a group; the generator refuses an entry with a field
that is not uniform over its group; and a launch whose plan's schedule is not the table entry's takes the dynamic instance -
cfg 2's tree with widths [140, 72] (the leaves' k-block count matches cfg 2's, their hidden width does not), a tree whose leaf
group mixes two hidden widths, and a tree with a condition."""
import os
import sys

import pytest

from hint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wl_shape_table as gen  # noqa: E402
from instance_cases import descs_for  # noqa: E402

CU = 256
CFG2 = (6, (140, 70, 35, 17), 4096)
GAS = (8, (128, 64, 32, 16), 8192)


@pytest.fixture()
def lib(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("HINT_WL_STATIC", raising=False)
    monkeypatch.delenv("HINT_WL_NR", raising=False)
    lib.hint_debug_reload_knobs()
    yield lib
    monkeypatch.undo()
    lib.hint_debug_reload_knobs()


def test_header_and_generator_agree_on_the_schedule_layout():
    hdr = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    names = gen.group_fields()
    assert f"#define HINT_WL_SCHED_FIELD0 {gen.SCHED_FIELD0}\n" in hdr
    assert f"#define HINT_WL_SCHED_FIELDS {gen.MAX_G * len(names) + 1}\n" in hdr
    for must in ("ent_begin", "ent_cnt", "level", "level_last", "slots", "n1", "ntt_min", "ntt_max", "thin_K", "cin", "kcp", "hw", "sl"):
        assert must in names


@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_schedules_of_the_two_shapes(lib, backward):
    """what the kernels rely on: at most four entries / slots per group (one coupling pass), at most four slabs per net (no
    `more` loop), two or three tiles per row (no one-tile MFMA group), k-blocks by hidden width"""
    for d, widths, B in (CFG2, GAS):
        groups, tail = gen.sched_fields(lib, d, widths, B, CU, backward)
        n_groups = gen.shape_fields(lib, d, widths, B, CU, backward)[1][gen.fold_fields().index("a_n_groups")]
        assert 0 <= tail <= 4
        for g in groups[:n_groups]:
            assert 1 <= g["ent_cnt"] <= 4 and 1 <= g["slots"] <= 4 and 1 <= g["sl"] <= 4
            assert 2 <= g["ntt_min"] <= g["ntt_max"] <= 3
            assert g["n1"] == (g["hw"] + 15) // 16 and g["kcp"] == (4 if g["cin"] < 4 else 8)
        for g in groups[n_groups:]:
            assert not any(g.values())
        # deepest level first; the last group is the root with the widest subnets
        assert [g["level"] for g in groups[:n_groups]] == list(range(n_groups))
        assert groups[n_groups - 1]["hw"] == widths[0]


@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_other_hidden_width_with_the_same_k_blocks_stays_dynamic(lib, backward):
    d, widths, B = CFG2
    other = (140, 72) + tuple(widths[2:])
    assert gen.shape_fields(lib, d, other, B, CU, backward)[0] == -1
    mine, _ = gen.sched_fields(lib, d, widths, B, CU, backward)
    theirs, _ = gen.sched_fields(lib, d, other, B, CU, backward)
    diff = {(i, k) for i, (p, q) in enumerate(zip(mine, theirs)) for k in p if p[k] != q[k]}
    assert diff == {(0, "hw")}, diff            # n1 = 5 either way: only a comparison of hw tells them apart


@pytest.mark.parametrize("h_other", [72, 90], ids=["same-n1", "other-n1"])
@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_generator_refuses_a_field_that_is_not_uniform(lib, backward, h_other):
    d, widths, B = CFG2
    descs, n = descs_for(d, 0, widths)
    leaves = [i for i in range(n) if descs[i].depth == max(descs[j].depth for j in range(n))]
    assert len(leaves) == 2
    descs[leaves[1]].h = h_other                # the leaf group now mixes two hidden widths
    with pytest.raises(ValueError, match="not uniform"):
        gen.sched_fields(lib, d, None, B, CU, backward, descs=(descs, n))
    assert lib.hint_plan_check_wl_shape(descs, n, d, 0, 4.0, B, CU, backward, 1, -1) == -1
    # the planner marks the field, it does not report one unit's value
    names = gen.group_fields()
    hw = lib.hint_plan_check_wl_shape(descs, n, d, 0, 4.0, B, CU, backward, 1, gen.SCHED_FIELD0 + names.index("hw"))
    assert hw == -1


@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_tree_with_a_condition_stays_dynamic(lib, backward):
    d, widths, B = CFG2
    assert gen.shape_fields(lib, d, widths, B, CU, backward, dc=3)[0] == -1
    with pytest.raises(ValueError):
        gen.sched_fields(lib, d, widths, B, CU, backward, dc=3)


def test_schedule_fields_outside_the_range_are_refused(lib):
    d, widths, B = CFG2
    descs, n = descs_for(d, 0, widths)
    n_sched = gen.MAX_G * len(gen.group_fields()) + 1
    for field in (36, gen.SCHED_FIELD0 - 1, gen.SCHED_FIELD0 + n_sched):
        assert lib.hint_plan_check_wl_shape(descs, n, d, 0, 4.0, B, CU, 0, 1, field) == -2 ** 63
