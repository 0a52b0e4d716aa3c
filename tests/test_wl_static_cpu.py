"""The shape-specialised wave-local instances without a GPU (hint_amd/csrc/hint_wl_shape.hpp): the committed table is what the
generator prints from the planner today, the launch site's field-by-field comparison takes the table's entries for exactly
the two shapes they were made for (BASELINE cfg 2 at 4096 rows, GAS at 8192, on 256 CUs, chained, permutations in LDS) and the
dynamic instance for everything else, HINT_WL_STATIC=0 switches them off, and the library holds one forward and one backward
instance per entry - the instance ledger (tests/instance_cases.py) does not list them: its pattern stops at the nested template
argument, and the GPU cases that reach them are tests/test_gpu_wl_static.py's."""
import os
import re
import subprocess
import sys

import pytest

from hint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wl_shape_table as gen  # noqa: E402

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


def test_committed_table_is_what_the_generator_prints(lib):
    committed = open(os.path.join(ROOT, "hint_amd", "csrc", "hint_wl_shape_table.hpp")).read()
    assert committed == gen.table_text(lib, gen.OFF)
    assert gen.FOLD_FIELDS == len(gen.fold_fields())
    hdr = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    assert f"#define HINT_WL_FOLD_FIELDS {gen.FOLD_FIELDS}\n" in hdr


def taken(lib, d, widths, B, backward, with_perm=1, dc=0, cu=CU):
    return gen.shape_fields(lib, d, widths, B, cu, backward, with_perm, dc)[0]


@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_selection_takes_the_entries_for_their_shapes(lib, backward):
    want = {name: (-1 if name in gen.OFF else i) for i, (name, *_) in enumerate(gen.SHAPES)}
    assert taken(lib, *CFG2, backward) == want["cfg2"]
    assert taken(lib, *GAS, backward) == want["gas"]
    # the fields do not move with the batch while plan variant and row tiles per workgroup stay: one tile per workgroup up to
    # one per CU (cfg 2), row pairs beyond (GAS)
    for B in (1, 17, 272, 4096):
        assert taken(lib, CFG2[0], CFG2[1], B, backward) == want["cfg2"], B
    assert taken(lib, GAS[0], GAS[1], 16 * CU + 1, backward) == want["gas"]


@pytest.mark.parametrize("backward", [0, 1], ids=["forward", "backward"])
def test_selection_leaves_every_other_launch_dynamic(lib, backward):
    assert taken(lib, 6, (64, 16), 4096, backward) == -1
    assert taken(lib, 6, (200, 100, 50, 25), 512, backward) == -1          # cfg 1
    assert taken(lib, 6, (200, 100, 50, 25), 4096, backward) == -1
    assert taken(lib, 6, CFG2[1], 4096, backward, dc=3) == -1              # cfg 2's tree with a condition
    assert taken(lib, *CFG2, backward, with_perm=0) == -1                  # no matrices in LDS: perm_lds and off_perm differ
    assert taken(lib, CFG2[0], CFG2[1], 8192, backward) == -1              # cfg 2 on row pairs
    assert taken(lib, GAS[0], GAS[1], 4096, backward) == -1                # GAS on single row tiles
    assert taken(lib, 8, (140, 70, 35, 17), 8192, backward) == -1


def test_one_changed_field_is_enough(lib):
    """every folded field takes part in the comparison: the two directions of a shape differ in a few LDS offsets only, and
    neither matches the other's entry"""
    for d, widths, B in (CFG2, GAS):
        f = gen.shape_fields(lib, d, widths, B, CU, 0)[1]
        b = gen.shape_fields(lib, d, widths, B, CU, 1)[1]
        assert f != b and sum(x != y for x, y in zip(f, b)) <= 10


def test_knob_switches_the_static_instances_off(lib, monkeypatch):
    monkeypatch.setenv("HINT_WL_STATIC", "0")
    lib.hint_debug_reload_knobs()
    assert taken(lib, *CFG2, 0) == -1 and taken(lib, *GAS, 1) == -1
    assert b"HINT_WL_STATIC=0" in lib.hint_build_info()
    monkeypatch.delenv("HINT_WL_STATIC")
    lib.hint_debug_reload_knobs()
    assert b"HINT_WL_STATIC" not in lib.hint_build_info()
    assert lib.hint_debug_last_wl_shape(0) in (-1, 0, 1)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "HINT_WL_STATIC" in doc


def test_library_holds_one_instance_pair_per_entry():
    out = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    have = sorted(set(re.findall(r"\b(hint_wl_(?:apply|bwd)_kernel<[^()]*WlStatic<\d+> ?>)\(", out)))
    norm = [h.replace("> >", ">>") for h in have]
    assert norm == ["hint_wl_apply_kernel<false, 1, true, hint::WlStatic<0>>", "hint_wl_apply_kernel<false, 2, true, hint::WlStatic<1>>",
                    "hint_wl_bwd_kernel<1, true, hint::WlStatic<0>>", "hint_wl_bwd_kernel<2, true, hint::WlStatic<1>>"], have
