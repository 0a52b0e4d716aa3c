"""The path ledger without a GPU (tests/plan_path_cases.py): every case reaches the path tuple and the wavefront variant it declares
at 256 CUs (hint_plan_check_paths / hint_plan_check_dispatch), the ledger as a whole reaches every step of the planner's ladder, every
staging mode and the kernels' size limits, each limit has an accepted and a refused neighbour, every case finds its rows in its pool
with |z| and |J| bounded, and the float32 oracle stays within a quarter of the GPU test's tolerances on those rows - so the
tolerances are achievable in fp32 for these inputs before a GPU sees them."""
import ctypes as C

import pytest
import torch

from hint_amd import _lib
from instance_cases import descs_for
from plan_path_cases import (CASES, PATHS, THIN_GROUP, THIN_L2, THIN_WHOLE, Z_MAX, check_paths, check_variant, descs_of,
                             fwd_shares, grad_shares, inv_grad_shares, prepared)

CU = 256
IDS = [c.name for c in CASES]


def named(paths):
    return dict(zip(PATHS, paths))


@pytest.fixture(scope="module")
def ledger():
    lib = _lib.load()
    return [(c, named(check_paths(lib, c, CU)), check_variant(lib, c, CU)) for c in CASES]


def test_print_ledger(ledger, capsys):
    with capsys.disabled():         # (the table is the point of this test: shown under -q too)
        print()
        print(f"{'case':24s} {'entry':8s} {'B':>5s} nw  " + " ".join(f"{p:>10s}" for p in PATHS))
        for c, p, (nw, alt4) in ledger:
            print(f"{c.name:24s} {c.entry:8s} {c.B(CU):5d} {nw:2d}  " + " ".join(f"{p[k]:10d}" for k in PATHS))


def test_every_case_reaches_its_declared_paths(ledger):
    bad = [f"{c.name}: reaches {tuple(p.values())} on {nw} wavefronts (variant {alt4}), declared {c.paths} on {c.nw}"
           for c, p, (nw, alt4) in ledger if tuple(p.values()) != tuple(c.paths) or nw != c.nw or alt4 != (1 if c.nw == 4 else 0)]
    assert not bad, "\n".join(bad)
    assert len(set(IDS)) == len(IDS)


def test_batch_sizes():
    """37 rows (three row tiles, the last ragged) unless a case asks for more row tiles than CUs: 16 x CUs + 5"""
    for c in CASES:
        assert c.B(CU) == (16 * CU + 5 if c.many else 37) and c.B(304) == (16 * 304 + 5 if c.many else 37)
        assert c.nw == 8 or c.many, f"{c.name}: the 4-wavefront variant runs batches of more row tiles than CUs only"
        assert c.pool(CU) == 256 or c.many


def test_ledger_reaches_the_ladder_the_staging_modes_and_the_limits(ledger):
    nw8 = [(c, p) for c, p, (nw, _) in ledger if nw == 8]
    nw4 = [(c, p) for c, p, (nw, _) in ledger if nw == 4]
    assert {p["tile_cap"] for _, p in nw8} == {64, 48, 32, 16}
    assert {p["unit_waves"] for _, p in nw8} == {8, 4, 2, 1}
    # the 4-wavefront variant: it exists only for plans of the ladder's first step (test_no_variant_below_the_first_step), so what
    # it can reach is tile_cap 64 with its own 4 wavefronts per unit
    assert nw4 and {(p["tile_cap"], p["unit_waves"]) for _, p in nw4} == {(64, 4)}
    # ... and the d = 56 (tile_cap 16) and d = 64 (tile_cap 48) trees run 16 x CUs + 5 rows on the plan that takes that batch
    many = {(c.d, p["tile_cap"]) for c, p, _ in ledger if c.many}
    assert {(56, 16), (64, 48)} <= many
    for mode in (THIN_L2, THIN_WHOLE, THIN_GROUP):
        assert any(p["thin_fwd"] == mode for _, p, _ in ledger), f"thin forward mode {mode}"
        assert any(p["thin_bwd"] == mode for _, p, _ in ledger), f"thin backward mode {mode}"
    assert any(p["spill_fwd"] for _, p, _ in ledger) and any(p["spill_bwd"] for _, p, _ in ledger)
    assert all(p["thin_fwd"] == THIN_GROUP or not p["spill_fwd"] for _, p, _ in ledger)
    assert all(p["thin_bwd"] == THIN_GROUP or not p["spill_bwd"] for _, p, _ in ledger)
    assert {p["slots_lds"] for _, p, _ in ledger} == {0, 1}
    assert {p["rowdw"] for _, p, _ in ledger} == {0, 1}
    # every level cut to one group per node
    lib = _lib.load()
    stats = (C.c_int64 * 16)()

    def nodes_of(c):
        return descs_of(c)[1]
    assert any(p["groups"] == nodes_of(c) > 60 for c, p, _ in ledger)
    # cin = 128 (eight tail tiles) at d = 128 and on a plan that has the 4-wavefront variant; r = 128 on a coupling with k = 0
    assert any(p["cin_tiles"] == 8 and c.d == 128 for c, p, _ in ledger)
    assert any(p["cin_tiles"] == 8 for c, p in nw4)
    assert any(p["r_tiles"] == 8 and c.entry == "coupling" and c.d == 128 and c.dc <= 8 for c, p, _ in ledger)
    assert max(p["r_tiles"] for _, p, _ in ledger) == 8 and max(p["cin_tiles"] for _, p, _ in ledger) == 8      # MAX_TAIL
    assert sum(c.d == 128 for c in CASES) >= 4
    # a chain of two blocks at d = 128: 2 x 128 x 128 floats of permutation matrices exceed PERM_LDS_MAX (16 KiB)
    chains = [c for c in CASES if c.entry == "chain"]
    assert any(c.d == 128 and c.n_blocks == 2 and c.n_blocks * c.d * c.d * 4 > 16 * 1024 for c in chains)
    # the accepted attempts' LDS: within the limit, the tightest within a KiB of it
    tight = 0
    for c in CASES:
        descs, n, clamp = descs_of(c)
        assert lib.hint_plan_check(descs, n, c.d, c.dc, clamp, stats) == 0, lib.hint_last_error().decode()
        assert max(stats[4], stats[5]) <= 160 * 1024
        tight = max(tight, stats[4], stats[5])
    assert tight > 160 * 1024 - 1024


def test_no_variant_below_the_first_step():
    """the d = 56 and d = 64 trees (tile_cap 16 and 48) have no 4-wavefront variant, and the planner keeps none for any plan below the
    ladder's first step: the variant must fit the LDS twice (80 KiB), a later step is tried only after the one before needed more
    than 160 KiB, and a step at best halves the per-group region (32 -> 16 tiles, or half the slabs) and leaves the fixed part.  HINT_NW=4 shows the 4-wavefront plan of those trees on its
    own: the same tile_cap, far over 80 KiB"""
    lib = _lib.load()
    mp = pytest.MonkeyPatch()
    stats = (C.c_int64 * 16)()
    out = (C.c_int32 * len(PATHS))()
    try:
        mp.setenv("HINT_NW", "4")
        lib.hint_debug_reload_knobs()
        for d, dc, widths, cap in ((56, 100, (32,), 16), (64, 30, (64, 32), 48)):
            descs, n = descs_for(d, dc, widths)
            assert lib.hint_plan_check(descs, n, d, dc, 4.0, stats) == 0, lib.hint_last_error().decode()
            assert stats[6] == 4 and max(stats[4], stats[5]) > 80 * 1024
            assert lib.hint_plan_check_paths(descs, n, d, dc, 4.0, 16 * CU + 5, CU, out, len(PATHS)) == 0
            assert named(out)["tile_cap"] == cap and named(out)["unit_waves"] == 4
    finally:
        mp.undo()
        lib.hint_debug_reload_knobs()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_finds_its_rows_and_stays_bounded(case):
    """every case finds its B rows in its pool (at most half of it discarded next to a ReLU kink), and the float64 oracle's |z|, |J|
    of both directions stay below 50"""
    m, rows, ref, fig = prepared(case, CU)
    print(f"{case.name}: {fig}")
    assert fig["pool"] <= 256 or case.many
    assert fig["found"] == fig["B"] == case.B(CU), fig
    assert 2 * fig["discarded"] <= fig["pool"], fig
    assert fig["z_max"] < Z_MAX and fig["J_max"] < Z_MAX, fig
    assert all(v.shape[0] == fig["B"] for v in rows.values())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_oracle_within_a_quarter_of_the_tolerances(case):
    """the float32 oracle against the float64 one on the case's rows with the GPU test's metrics: forward, inverse, d/dx, d/dc and
    every weight tensor at or below a quarter of what the GPU test allows"""
    m, rows, ref, fig = prepared(case, CU)
    assert ref is not None, fig
    r32 = m.reference(rows, torch.float32)
    shares = dict(fwd_shares(r32, ref))
    shares.update(grad_shares(r32, ref))
    if "inv" in ref:
        shares.update(inv_grad_shares(r32["inv"], ref["inv"]))
    worst = max(shares, key=shares.get)
    print(f"{case.name}: float32 oracle's worst share of a tolerance: {worst} {shares[worst]:.3f}")
    over = {k: round(v, 3) for k, v in shares.items() if not v <= 0.25}
    assert not over, over


# ---- the limits: an accepted and a refused neighbour at each ----
def plan_check(d, dc, widths):
    """(status, message, stats) of hint_plan_check, which builds the plan and lets the planner verify its own schedule"""
    lib = _lib.load()
    descs, n = descs_for(d, dc, widths)
    stats = (C.c_int64 * 16)()
    st = lib.hint_plan_check(descs, n, d, dc, 4.0, stats)
    return st, lib.hint_last_error().decode(), list(stats)


def test_limit_d_128():
    st, msg, stats = plan_check(128, 0, (16,))
    assert st == 0, msg
    st, msg, _ = plan_check(129, 0, (16,))
    assert st != 0 and msg == "hint_plan_create: d = 129 lanes exceeds the supported maximum 128"


@pytest.mark.parametrize("d,dc,widths,r", [(128, 64, (64, 32), 64), (100, 78, (48,), 50)])
def test_limit_cin_128(d, dc, widths, r):
    st, msg, stats = plan_check(d, dc, widths)
    assert st == 0, msg
    assert max(stats[4], stats[5]) <= 160 * 1024
    st, msg, _ = plan_check(d, dc + 1, widths)
    assert st != 0 and msg == f"hint_plan_create: a node with r={r} outputs / cin=129 inputs exceeds the kernels' limit of 128"


def test_limit_r_128():
    """r = 128 needs k = 0 over all 128 lanes (the ledger's r128_coupling) and is accepted; r = 129 would need d >= 129, which the
    lane limit refuses first (test_limit_d_128)"""
    lib = _lib.load()
    c = next(c for c in CASES if c.entry == "coupling")
    descs, n, clamp = descs_of(c)
    stats = (C.c_int64 * 16)()
    assert lib.hint_plan_check(descs, n, c.d, c.dc, clamp, stats) == 0, lib.hint_last_error().decode()
    assert descs[0].k == 0 and descs[0].r == 128


def test_limit_h_4080():
    st, msg, _ = plan_check(6, 0, (4081,))
    assert st != 0 and msg == "hint_plan_create: a node is too wide for the row records (h <= 4080, cin <= 255)"


def test_limit_lds():
    """d = 128 with one hidden width for every node: 27 tiles per subnet (h = 432) fit with 1472 bytes to spare, 28 do not at any
    step of the ladder"""
    st, msg, stats = plan_check(128, 0, (432,))
    assert st == 0, msg
    assert 160 * 1024 - 2048 < max(stats[4], stats[5]) <= 160 * 1024
    st, msg, _ = plan_check(128, 0, (433,))
    assert st != 0 and msg == "hint_plan_create: block needs 164416 bytes of LDS (> 163840); d/dc/h too large"


def test_paths_reject_bad_arguments():
    lib = _lib.load()
    descs, n = descs_for(6, 0, (24, 12))
    out = (C.c_int32 * len(PATHS))()
    assert lib.hint_plan_check_paths(descs, n, 6, 0, 4.0, 0, 256, out, len(PATHS)) != 0
    assert lib.hint_plan_check_paths(descs, n, 6, 0, 4.0, 100, 0, out, len(PATHS)) != 0
    assert lib.hint_plan_check_paths(descs, n, 6, 0, 4.0, 100, 256, None, len(PATHS)) != 0
    assert lib.hint_plan_paths(None, 100, out, len(PATHS)) != 0
    # a short output array takes the leading fields only
    short = (C.c_int32 * 3)(-1, -1, -1)
    assert lib.hint_plan_check_paths(descs, n, 6, 0, 4.0, 100, 256, short, 2) == 0
    assert list(short) == [64, 8, -1]
