"""The table of the large-index tests (tests/large_cases.py) checked without a GPU: every case is admissible for its entry point,
its named array holds more than 2^31 elements at the smallest ragged N, the probe rows bracket the three crossings, the declared
memory covers the arrays and stays under the cap, and the oracle-side caps hold on the seeded probe rows.  The ledgers are held
against include/hint_amd.h: every function that takes a descriptor is the `entry` of a case, or in LIMITED (its documented limits
keep every offset below 2^31; the size query refuses one past them, and a named test runs it at them), or in NOT_COVERED; the
moduli of the cases that have no geometry query are the constants of the kernels' text."""
import ast
import fnmatch
import os
import re

import numpy as np
import pytest

from hint_amd import _lib
import large_cases as lc
import plusgen_oracle as pgo
import shapegen_oracle as so
from test_poison_table_cpu import ROOT, declarations

CASES = list(lc.ROW_CASES.values())
IDS = [c["name"] for c in CASES]


def tiles(case):
    """(rows a workgroup has in flight, workgroups) from the entry point's geometry query; where it has none, the case's `grid`
    (the kernel's constants, held against its text below), or (64, 256)"""
    lib = _lib.load()
    if case["geometry"] is None:
        if case["grid"] is not None:
            return case["grid"]
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


def test_plusgen_probe_rows_stay_within_the_ambiguity_cap():
    """the oracle alone, on the Philox draws of both plusgen cases' probe rows (the rows around the counter's high-word flip
    included): the share of rows whose ring or counts the fp32 kernel may miss"""
    for name in ("plusgen_outline", "plusgen_x"):
        case = lc.ROW_CASES[name]
        seed, off, N = case["params"]["seed"], case["params"]["offset"], case["N"]
        flip = 2 ** 32 - off
        rows = lc.probe_rows(N, case["width"], extra=(flip - 2, flip - 1, flip, flip + 1))
        assert {flip - 2, flip - 1, flip, flip + 1} <= set(rows) and off < 2 ** 32 < off + N
        d = np.concatenate([pgo.draws(seed, off + first, n) for first, n in lc.runs_of(rows)])
        assert d.shape == (len(rows), 9)
        share = float(pgo.ambiguous(d).mean())
        print(f"{name}: {share:.4f} of {len(rows)} probe rows are ambiguous")
        assert share <= pgo.MAX_AMBIGUOUS


def kernel_constants(source, names):
    """{name: value} of `constexpr int NAME = <integer expression of literals and earlier constants>;` in a kernel's text"""
    text = open(os.path.join(ROOT, "hint_amd", "csrc", source)).read()
    env = {}
    for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*([\w\s+\-*/()<]+);", text):
        try:
            env[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(env)))
        except (NameError, SyntaxError):
            pass
    return {n: env[n] for n in names}


def test_the_moduli_are_the_kernels_constants():
    pg = kernel_constants("hint_plusgen.hip", ("PG_WAVE_ROWS", "PG_WAVES", "PG_MAX_WG", "PG_ROW", "PG_PTS"))
    assert (pg["PG_WAVE_ROWS"], pg["PG_WAVES"], pg["PG_MAX_WG"]) == (lc.PG_WAVE_ROWS, lc.PG_WAVES, lc.PG_MAX_WG)
    assert pg["PG_ROW"] == lc.ROW_CASES["plusgen_x"]["width"] and 2 * pg["PG_PTS"] == lc.ROW_CASES["plusgen_outline"]["width"]
    ep = kernel_constants("hint_epoch.hip", ("EP_TILE", "EP_MAX_WG", "EP_MAX_SLABS"))
    assert (ep["EP_TILE"], ep["EP_MAX_WG"], ep["EP_MAX_SLABS"]) == (lc.EP_TILE, lc.EP_MAX_WG, lc.EP_MAX_SLABS)
    hh = kernel_constants("hint_householder.hip", ("HH_MAX_B", "HH_MAX_D", "HH_MAX_N", "HH_T", "HH_MAX_GRID"))
    assert (hh["HH_MAX_B"], hh["HH_MAX_D"], hh["HH_MAX_N"]) == (lc.HH_MAX_B, lc.HH_MAX_D, lc.HH_MAX_N)
    assert (hh["HH_T"], hh["HH_MAX_GRID"]) == (lc.HH_T, lc.HH_MAX_GRID) and lc.HH_TRIP == 16 * 4 * 1024
    text = open(os.path.join(ROOT, "hint_amd", "csrc", "hint_householder.hip")).read()
    assert f"t0 += {lc.HH_APPLY_WAVES} * (int)gridDim.x" in text and "cdiv(cdiv(B, HH_T), 4)" in text      # four tiles a workgroup
    lib = _lib.load()
    for name in ("plusgen_outline", "plusgen_x"):
        c = lc.ROW_CASES[name]
        N, off = c["N"], c["params"]["offset"]
        assert lib.hint_plusgen_workspace_bytes(N) == 4 * lc.PG_WAVES * lc.PG_MAX_WG        # the grid is at its cap
        assert lib.hint_plusgen_workspace_bytes(c["limit"] + 1) == 0
        assert N % lc.PG_WAVE_ROWS and N % (lc.PG_WAVE_ROWS * lc.PG_WAVES) and -(-N // lc.PG_WAVE_ROWS) % (lc.PG_WAVES * lc.PG_MAX_WG)
        assert off < 2 ** 32 < off + N < 2 ** 64                              # the row counter's high word changes inside the call
    c = lc.ROW_CASES["epoch"]
    N, d = c["N"], c["params"]["d"]
    for op in (_lib.EPOCH_GATHER, _lib.EPOCH_MOMENTS, _lib.EPOCH_STANDARDIZE):
        assert lib.hint_epoch_workspace_bytes(op, N, N, d) > 0 and lib.hint_epoch_workspace_bytes(op, N, N + 1, d) == 0
    assert lib.hint_epoch_workspace_bytes(_lib.EPOCH_GATHER, c["limit"] + 1, 1, d) == 0
    assert lib.hint_epoch_workspace_bytes(_lib.EPOCH_MOMENTS, N, N, d) == 8 * d * lc.EP_MAX_SLABS     # the slab cap is reached ...
    assert -(-N // lc.EP_MAX_SLABS) > lc.EP_TILE and -(-N // lc.EP_TILE) > 2 * lc.EP_MAX_WG             # ... and the tile loops go round


def descriptor_entry_points():
    """every function of include/hint_amd.h whose first parameter is the descriptor of a run, `const hint_*_desc* desc` (the
    planner's `const hint_node_desc* nodes` is an array of tree nodes, not a descriptor)"""
    return sorted(n for n, ps in declarations().items()
                  if ps and re.match(r"^const hint_\w+_desc ?\* ?desc$", " ".join(ps[0].split())))


def ledger_errors(cases, not_covered, limited):
    """what is wrong with the three ledgers against the header, as a list of sentences"""
    decls, need = declarations(), descriptor_entry_points()
    places = {"ROW_CASES": {c["entry"] for c in cases}, "NOT_COVERED": set(not_covered), "LIMITED": set(limited)}
    out = []
    missing = [e for e in need if not any(e in s for s in places.values())]
    if missing:
        out.append(f"descriptor entry points in none of ROW_CASES, LIMITED and NOT_COVERED of tests/large_cases.py: {missing}")
    for e in need:
        where = [k for k, s in places.items() if e in s]
        if len(where) > 1:
            out.append(f"{e} is in {where}: an entry point belongs to one ledger")
    for k, s in places.items():
        for e in sorted(s):
            if "*" in e:                                                    # a family that takes no descriptor, by pattern
                hit = fnmatch.filter(decls, e)
                if k != "NOT_COVERED" or not hit or set(hit) & set(need):
                    out.append(f"{k} names the pattern {e}, which matches {hit or 'nothing the header declares'}")
            elif e not in need:
                out.append(f"{k} names {e}, which is no descriptor entry point of the header")
    return out


def test_the_header_has_the_descriptor_entry_points():
    need = descriptor_entry_points()
    assert len(need) >= 14 and {"hint_curve_run", "hint_mmd_run", "hint_plusgen_run", "hint_householder_run", "hint_epoch_run"} <= set(need)
    assert not [e for e in need if "plan" in e]
    assert all(e in _lib.exported_symbols() for e in need)


def test_the_entry_points_left_out_are_written_down():
    """every descriptor entry point of the header is in exactly one of: a case's `entry`, LIMITED, NOT_COVERED; no ledger names
    what the header does not declare"""
    assert set(lc.NOT_COVERED) == {"hint_mmd_run", "hint_adam_*"}
    errors = ledger_errors(CASES, lc.NOT_COVERED, getattr(lc, "LIMITED", {}))
    assert not errors, "\n".join(errors)
    assert all(r.strip() for r in lc.NOT_COVERED.values()) and all(rec["reason"].strip() for rec in lc.LIMITED.values())


def test_the_ledger_check_notices_what_it_should():
    need = descriptor_entry_points()
    full = [dict(entry=e) for e in need]
    assert ledger_errors(full, {}, {}) == []
    e = ledger_errors(full[1:], {}, {})
    assert len(e) == 1 and need[0] in e[0]
    assert any("one ledger" in s for s in ledger_errors(full, {}, {need[0]: {}}))
    assert any("one ledger" in s for s in ledger_errors(full, {need[0]: ""}, {}))
    assert any("hint_gone_run" in s for s in ledger_errors(full, {"hint_gone_run": ""}, {}))
    assert any("hint_gone_run" in s for s in ledger_errors(full + [dict(entry="hint_gone_run")], {}, {}))
    assert any("hint_nothing_*" in s for s in ledger_errors(full, {"hint_nothing_*": ""}, {}))
    assert any("hint_*_run" in s for s in ledger_errors(full, {"hint_*_run": ""}, {}))      # a pattern may not swallow a descriptor run
    assert ledger_errors(full, {"hint_adam_*": ""}, {}) == []


def test_limited_entry_points_are_refused_past_their_limits_and_run_at_them():
    """LIMITED: the size query accepts the limit and refuses one past each of them, every element offset at the limit is below
    2^31, and the test that runs the entry point AT the limit exists"""
    lib = _lib.load()
    for entry, rec in lc.LIMITED.items():
        f = getattr(lib, rec["sizer"])
        assert f(*rec["at"]) > 0, (entry, (lib.hint_last_error() or b"").decode())
        for args in rec["over"]:
            assert args != rec["at"] and f(*args) == 0 and lib.hint_last_error(), (entry, args)
        assert 0 < rec["elements"] < lc.EDGE
        path, name = rec["test"].split("::")
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
        assert name in defined, f"{entry}: {rec['test']} does not exist"
    hh = lc.LIMITED["hint_householder_run"]
    assert hh["elements"] == hh["at"][1] * hh["at"][2] and hh["at"][1:] == (lc.HH_MAX_B, lc.HH_MAX_D, lc.HH_MAX_D)


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
