"""The table of the large-index tests (tests/large_cases.py) checked without a GPU: every case is admissible for its entry point,
its named array holds more than 2^31 elements at the smallest ragged N, the probe rows bracket the three crossings, the declared
memory covers the arrays and stays under the cap, and the oracle-side caps hold on the seeded probe rows."""
import numpy as np
import pytest

from hint_amd import _lib
import large_cases as lc
import shapegen_oracle as so

CASES = list(lc.ROW_CASES.values())
IDS = [c["name"] for c in CASES]


def tiles(case):
    """(rows a workgroup has in flight, workgroups) from the entry point's geometry query; (64, 256) where it has none"""
    lib = _lib.load()
    if case["geometry"] is None:
        return 64, 256
    fn, args = case["geometry"]
    f = getattr(lib, fn)
    wgs, tile = int(f(*args, 0)), int(f(*args, 1))
    assert wgs > 0 and tile > 0, (lib.hint_last_error() or b"").decode()
    return tile, wgs


def test_probe_rows_bracket_every_crossing():
    for width, N in ((100, 21474842), (256, 8388614), (3, 1 << 30), (2048, 1048582), (7, 400000000)):
        rows = lc.probe_rows(N, width)
        assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == N - 1
        assert set(range(lc.HEAD)) <= set(rows) and set(range(N - lc.TAIL, N)) <= set(rows)
        for k, r in zip(lc.CROSSINGS, lc.crossing_rows(width)):
            assert (r - 1) * width < (1 << k) <= r * width                # row r - 1 begins below 2^k, row r at or past it
            assert 4 * (r - 1) * width < (1 << (k + 2)) <= 4 * r * width  # ... and the byte offsets below / past 2^(k + 2)
            assert {r - 1, r} <= set(rows), (width, k)
        stride = lc.picket_stride(N)
        assert lc.is_prime(stride) and lc.PICKET // 2 <= N // stride <= lc.PICKET + 1
        assert set(range(0, N, stride)) <= set(rows)
    assert lc.runs_of([0, 1, 2, 5, 7, 8]) == [(0, 3), (5, 1), (7, 2)]
    assert lc.probe_rows(10, 3) == list(range(10))                        # a small batch: every row, no crossing inside


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_admissible_smallest_and_ragged(case):
    N, w = case["N"], case["width"]
    assert 1 <= N <= case["limit"]
    named = dict((a, n) for a, n, _ in case["arrays"])[case["named"]]
    assert named > lc.EDGE and 4 * named > 1 << 32
    if w is not None:
        assert named == N * w                                             # the named array is the one N was computed from
    if case["fixed_n"]:
        assert N == case["limit"]                                         # the documented maximum itself
    else:
        tile, wgs = tiles(case)
        assert N % 64 and (tile == 1 or N % tile), (N, tile)
        assert N % wgs and N % (tile * wgs), (N, tile, wgs)
        first = lc.rows_past(w) if w is not None else case["crossings"][-1]
        assert 0 <= N - first <= max(64, tile) + 5                        # the smallest such N, up to the ragged remainder
    rows = lc.probe_rows(N, w, crossings=case["crossings"])
    for r in case["crossings"]:
        assert 0 < r < N and {r - 1, r} <= set(rows)                      # every crossing lies inside the batch and is probed
    total = sum(n * b for _, n, b in case["arrays"])
    assert case["bytes"] == total and total + lc.SLACK <= case["peak"] <= lc.CAP
    assert lc.CHUNK_ELEMS * 8 <= lc.SLACK                                 # a float64 temporary of one chunk stays within 2 GiB


def test_ragged_templates_cross_where_the_table_says():
    case = lc.ROW_CASES["hausdorff_ragged"]
    N, T = case["N"], case["params"]["T"]
    assert lc.ragged_offset(0) == 0 and lc.ragged_offset(N) == T and T > 1 << 30 and T <= 4096 * N
    assert {lc.ragged_offset(n + 1) - lc.ragged_offset(n) for n in range(0, 50)} == {3, 4}
    for k, r in zip(lc.CROSSINGS, case["crossings"]):
        assert 2 * lc.ragged_offset(r - 1) < (1 << k) <= 2 * lc.ragged_offset(r)


def test_parameters_are_within_the_entry_points_limits():
    lib = _lib.load()
    c = lc.ROW_CASES["curve"]
    for P in c["params"]["P"]:
        assert lib.hint_curve_workspace_bytes(c["N"], c["params"]["K"], P) > 0
    c = lc.ROW_CASES["hausdorff_points"]
    lib.hint_hausdorff_workspace_bytes(c["N"], c["params"]["K"], c["params"]["P"], c["params"]["M"])
    assert not lib.hint_last_error()
    for name in ("hausdorff_ragged", "plus"):
        c = lc.ROW_CASES[name]
        fn, args = c["geometry"]
        assert getattr(lib, fn)(*args, 0) > 0
    assert lc.ROW_CASES["plus"]["params"]["max_dist"] > 0
    c = lc.ROW_CASES["lensgen"]
    assert lib.hint_lensgen_workspace_bytes(c["N"]) > 0
    off = c["params"]["offset"]
    assert off < 2 ** 32 < off + c["N"] < 2 ** 64                          # the row counter's high word changes inside the call
    c = lc.ROW_CASES["fcoef"]
    assert lib.hint_fcoef_workspace_bytes(c["N"], c["params"]["p_max"], c["params"]["K"]) > 0 and c["N"] >= 1 << 20
    assert lib.hint_fcoef_workspace_bytes(c["limit"] + 1, c["params"]["p_max"], c["params"]["K"]) == 0
    c = lc.ROW_CASES["abc"]
    assert lib.hint_abc_workspace_bytes(c["N"], c["params"]["ny"], c["params"]["k"]) > 0
    assert lib.hint_abc_workspace_bytes(c["N"] + 1, c["params"]["ny"], c["params"]["k"]) == 0
    c = lc.ROW_CASES["corr"]
    assert lib.hint_corr_workspace_bytes(c["N"], c["params"]["d"]) > 0
    assert lib.hint_corr_workspace_bytes(c["N"], c["params"]["d"] + 1) == 0


def test_abc_plants_its_rows_at_the_edges_and_the_crossings():
    case = lc.ROW_CASES["abc"]
    rows = lc.abc_plant_rows(case)
    assert len(rows) == len(set(rows)) == case["params"]["k"] and 0 in rows and case["N"] - 1 in rows
    for r in lc.crossing_rows(case["width"]):
        assert r - 1 in rows and r in rows
    assert max(rows) * case["width"] > lc.EDGE


def test_lensgen_probe_rows_stay_within_the_ambiguity_cap():
    """the oracle alone, on the Philox draws of the probe rows: the share of rows whose count the fp32 kernel may miss"""
    case = lc.ROW_CASES["lensgen"]
    seed, off, N = case["params"]["seed"], case["params"]["offset"], case["N"]
    flip = 2 ** 32 - off
    rows = lc.probe_rows(N, case["width"], extra=(flip - 2, flip - 1, flip, flip + 1))
    assert {flip - 1, flip} <= set(rows)
    d = np.concatenate([so.draws(seed, off + first, n, np.float32) for first, n in lc.runs_of(rows)])
    assert d.shape == (len(rows), 4)
    assert so.ambiguous(d).mean() <= so.MAX_AMBIGUOUS


def test_the_entry_points_left_out_are_written_down():
    assert set(lc.NOT_COVERED) == {"hint_mmd_run", "hint_adam_*"}
    covered = {c["entry"] for c in CASES}
    assert not covered & set(lc.NOT_COVERED) and all(e in _lib.exported_symbols() for e in covered)


# ---- the flow cases ----
def flow_plan(family, B=1 << 21, cu=256):
    import ctypes as C
    import instance_cases as ic
    lib = _lib.load()
    case = lc.ledger_case(family)
    descs, n = ic.descs_for(case.d, case.dc, case.widths)
    stats = (C.c_int64 * 16)()
    assert lib.hint_plan_check(descs, n, case.d, case.dc, 4.0, stats) == 0
    disp = ic.check_dispatch(lib, case.d, case.dc, case.widths, B, cu)
    return case, int(stats[1]), int(stats[2]), int(stats[3]), disp


@pytest.mark.parametrize("family", list(lc.FLOW_CASES))
def test_flow_batch_is_predicted_from_the_tape_layout(family):
    """B from the plan's stats (levels, WT), the lean field of the dispatch and the layout comment of hint_abi.cpp; the GPU test
    asserts that hint_plan_tape_floats of the device plan is this prediction at the B it bisects to"""
    import instance_cases as ic
    case, L, WT, ST, disp = flow_plan(family)
    nr, lean = disp["nr"], disp["lean"]
    tape = lambda B: lc.tape_floats_predicted(L, case.d, WT, lean, B)     # noqa: E731
    B, first = lc.flow_batch(tape, nr)
    assert tape(first) > lc.EDGE >= tape(first - 1) and 0 < B - first <= 16 * nr + 5 and B % (16 * nr) == 5 and B % 64
    _, _, _, _, at_b = flow_plan(family, B)
    assert at_b["nr"] == nr and at_b["lean"] == lean and at_b["passes"] >= 2
    want = tuple(s.replace(", true>", ", false>") for s in case.expect) if family == "wave_local" else case.expect
    assert ic.instances_of(at_b, "block") == want
    sections = lc.tape_sections(L, case.d, WT, lean, B)
    assert [b for b, _ in sections] == sorted(b for b, _ in sections) and sections[-1][0] + B * WT <= tape(B)
    cross = lc.flow_crossings(sections, B)
    assert set(cross) >= {29, 30}                                         # (2^31 is crossed in the tail's share of the last array)
    rows = lc.probe_rows(B, case.d, crossings=sorted(cross.values()))
    for r in cross.values():
        assert {r - 1, r} <= set(rows)
    Bp = -(-B // 16) * 16
    ws = (1 if lean else 2) * (Bp * WT + 64) + Bp * ST                    # g1 (, g2), g_st: the workspace without its slabs
    assert 4 * tape(B) + 4 * ws + 4 * B * (6 * case.d + 2 * case.dc + 4) + lc.SLACK <= lc.CAP - lc.GIB
    assert 2 * (4 * tape(B) + 4 * ws) + lc.SLACK > lc.CAP                 # why the wave-local family runs one block, not two


@pytest.mark.parametrize("family", list(lc.FLOW_CASES))
def test_flow_probe_rows_stay_within_the_kink_cap(family):
    """the float64 oracle alone on as many N(0, 1) rows as the GPU test probes (it draws its rows on the device, from the same
    distribution): the share next to a ReLU kink stays within the family's cap"""
    import torch
    from test_gpu_instances import block_params, oracle_block_rows
    case = lc.ledger_case(family)
    n = len(lc.probe_rows(1 << 20, case.d))
    g = torch.Generator().manual_seed(11)
    rows = (torch.randn(n, case.d, generator=g), torch.randn(n, case.dc, generator=g) if case.dc else None,
            torch.randn(n, case.d, generator=g), torch.randn(n, case.d, generator=g), torch.randn(n, generator=g))
    nodes, P = block_params(case)
    _, keep, _, _ = oracle_block_rows(case, nodes, P, rows)
    assert n - int(keep.sum()) <= case.kink_cap * n
