"""The instance ledger without a GPU (tests/instance_cases.py): every row and part-B kernel instance in the built library's
symbol table is reached by a GPU case of tests/test_gpu_instances.py, each case lands on the instances it declares at 256 CUs
(hint_plan_check_dispatch: the launch decision hint_abi.cpp's dispatch() takes for every entry point), and every row-kernel
family has a case that runs two or more passes of its tile loop with a ragged last one."""
import pytest

from hint_amd import _lib
from instance_cases import (CASES, KNOBS_EXCLUDED, ROW_FAMILIES, check_dispatch, compiled_instances, families,
                            instances_of, knob_env, mismatch, ragged)

CU = 256


@pytest.fixture(scope="module")
def ledger():
    lib = _lib.load()
    mp = pytest.MonkeyPatch()
    rows = []
    try:
        for c in CASES:
            knob_env(mp, lib, c.knobs)
            rows.append((c, check_dispatch(lib, c.d, c.dc, c.widths, c.B(CU), CU)))
    finally:
        mp.undo()
        lib.hint_debug_reload_knobs()
    return rows


def test_print_ledger(ledger, capsys):
    with capsys.disabled():         # (the table is the point of this test: shown under -q too)
        _print_ledger(ledger)


def _print_ledger(ledger):
    print()
    print(f"{'case':32s} {'B':>7s} {'nw':>2s} {'nr':>2s} {'grid':>5s} {'pass':>4s} {'rag':>3s}  forward / inverse / backward / part B")
    for c, d in ledger:
        fwd, inv, bwd, dw = instances_of(d, c.entry)
        knobs = " " + " ".join(f"{k}={v}" for k, v in c.knobs.items()) if c.knobs else ""
        print(f"{c.name:32s} {c.B(CU):7d} {d['nw']:2d} {d['nr']:2d} {d['grid']:5d} {d['passes']:4d} {'y' if ragged(d) else '':>3s}  "
              f"{fwd} / {inv} / {bwd} / {dw}{knobs}")
    compiled = compiled_instances(_lib.LIB_PATH)
    reached = {i for c, d in ledger for i in instances_of(d, c.entry)}
    print(f"{len(compiled)} compiled instances, {len(reached & set(compiled))} reached:")
    for i in compiled:
        by = [c.name for c, d in ledger if i in instances_of(d, c.entry)]
        print(f"  {i:40s} {', '.join(by) if by else 'NOT REACHED'}")
    for k, why in KNOBS_EXCLUDED.items():
        print(f"  (no case: {k}: {why})")


def test_ledger_lists_every_compiled_instance():
    compiled = compiled_instances(_lib.LIB_PATH)
    # 4 general forward / inverse, 8 wave-local forward / inverse, 4 wave-local backward, 3 general backward, 4 part B
    assert len(compiled) == 23, compiled
    declared = {i for c in CASES for i in c.expect}
    assert declared <= set(compiled), declared - set(compiled)
    assert set(compiled) <= declared, f"compiled instances no case reaches: {sorted(set(compiled) - declared)}"


def test_every_case_lands_on_its_declared_instances(ledger):
    bad = [m for c, d in ledger for m in [mismatch(c, d)] if m]
    assert not bad, "\n".join(bad)


def test_default_cases_reach_every_instance_and_family_multi_pass(ledger):
    default = [(c, d) for c, d in ledger if not c.knobs]
    reached = {i for c, d in default for i in instances_of(d, c.entry)}
    missing = set(compiled_instances(_lib.LIB_PATH)) - reached
    assert not missing, f"instances the default knobs can reach but no default case does: {sorted(missing)}"
    multi = set()
    for c, d in default:
        if d["passes"] >= 2 and ragged(d):
            multi |= families(d)
    assert multi >= ROW_FAMILIES, f"row-kernel families without a ragged multi-pass case: {sorted(ROW_FAMILIES - multi)}"
    # (and the cases that say so really are: a grid cap or a threshold that moves takes their second pass away)
    lost = [c.name for c, d in ledger if c.multi and not (d["passes"] >= 2 and ragged(d))]
    assert not lost, f"multi-pass cases that lost their second pass: {lost}"


def test_each_backward_family_has_a_big_s_case(ledger):
    have = set()
    for c, d in ledger:
        if c.big_s:
            have |= families(d) & {"wl backward", "bwd", "n3", "fly", "subtree"}
    assert have >= {"wl backward", "bwd", "n3", "fly", "subtree"}, have


def test_dispatch_follows_the_cu_count():
    """a device with fewer CUs caps the grid lower: the same batch goes round the tile loop more often"""
    lib = _lib.load()
    c = next(c for c in CASES if c.name == "fly_block_multi")
    full = check_dispatch(lib, c.d, c.dc, c.widths, c.B(256), 256)
    part = check_dispatch(lib, c.d, c.dc, c.widths, c.B(256), 128)
    assert full["num_cu"] == 256 and part["num_cu"] == 128
    assert part["grid"] == 8 * 128 and part["passes"] > full["passes"]
    assert check_dispatch(lib, c.d, c.dc, c.widths, c.B(128), 128)["passes"] == full["passes"]


def test_dispatch_rejects_bad_arguments():
    lib = _lib.load()
    from instance_cases import DISPATCH, descs_for
    import ctypes as C
    descs, n = descs_for(6, 0, (24, 12))
    out = (C.c_int32 * len(DISPATCH))()
    assert lib.hint_plan_check_dispatch(descs, n, 6, 0, 4.0, 0, 256, out, len(DISPATCH)) != 0
    assert lib.hint_plan_check_dispatch(descs, n, 6, 0, 4.0, 100, 0, out, len(DISPATCH)) != 0
    assert lib.hint_plan_dispatch(None, 100, out, len(DISPATCH)) != 0
    # a short output array takes the leading fields only
    short = (C.c_int32 * 3)(-1, -1, -1)
    assert lib.hint_plan_check_dispatch(descs, n, 6, 0, 4.0, 100, 256, short, 2) == 0
    assert list(short) == [1, 1, -1]
