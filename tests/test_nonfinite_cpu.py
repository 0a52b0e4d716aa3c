"""tests/nonfinite_cases.py without a GPU: the optimizer's element table covers every class at every lane position and in a scalar
tail and keeps away from the fp32 overflow edge; every spoiled-row case lands on the row kernels it declares at 256 CUs
(hint_plan_check_dispatch) and all eight families are reached; the float64 oracle makes every spoiled row non-finite; and the
oracle's poisoned training step poisons its model."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
from hint_amd import _lib
from instance_cases import ROW_FAMILIES, check_dispatch, families, instances_of, knob_env
from oracle import hint_oracle as orc

CU = 256


# ---- the optimizer's element table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", sorted({s for _, s in nf.RUNS}))
def test_table_covers_every_class_at_every_lane_and_in_a_scalar_tail(scale):
    t = nf.table(scale)
    nc = len(t.names)
    body, tail = nf.coverage(t)
    assert body == {(c, lane) for c in range(nc) for lane in range(4)}
    assert tail == set(range(nc))
    assert set(nf.RAGGED) <= set(t.lengths) and sum(t.lengths) < 10000
    for p, m, v in zip(t.p, t.m, t.v):
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all() and (v >= 0).all()
    # the classes the issue lists are there, with the bits they are meant to have
    g = {n: nf._f32([val])[0] for n, val, _ in nf.classes(scale)}
    assert np.isnan(g["+nan"]) and np.isnan(g["-nan"]) and not np.signbit(g["+nan"]) and np.signbit(g["-nan"])
    assert g["+inf"] == np.inf and g["-inf"] == -np.inf and np.isfinite(g["+3.3e38"]) and g["+3.3e38"] > np.float32(3.0e38)
    assert g["+clamp"] * np.float32(scale) == np.float32(nf.CLAMP) and g["-clamp"] * np.float32(scale) == -np.float32(nf.CLAMP)
    assert g["+zero"] == 0 and not np.signbit(g["+zero"]) and np.signbit(g["-zero"])
    assert 0 < g["+subnormal"] < np.finfo(np.float32).tiny
    with np.errstate(over="ignore"):
        assert np.isinf(g["+1e30"] * g["+1e30"]) and np.isfinite(g["+1e15"] * g["+1e15"])
        assert np.isinf(g["+1e38"] * np.float32(4.0)) and np.isfinite(g["+1e38"] * np.float32(1.0))
    assert any(s == 4.0 for _, s in nf.RUNS)             # the run whose product g * grad_scale overflows


@pytest.mark.parametrize("clamp,scale", nf.RUNS)
def test_table_is_away_from_the_overflow_edge_and_the_reference_is_poisoned(clamp, scale):
    """both multiplication orders of (1 - b2) * g * g in fp32 give every element of p, m, v the same class on all three steps,
    and that class is torch's (clamp_ + torch.optim.Adam on the CPU); the NaN classes end up NaN in p, m and v"""
    t = nf.table(scale)
    ref = nf.torch_reference(t, clamp, scale)
    st = [[(p.copy(), m.copy(), v.copy()) for p, m, v in zip(t.p, t.m, t.v)] for _ in range(2)]
    for step in range(1, nf.STEPS + 1):
        for o in range(2):
            st[o] = [nf.adam_fp32(p, g, m, v, step, clamp, scale, o) for (p, m, v), g in zip(st[o], t.g)]
        for si, ci in enumerate(t.cls):
            for q, what in enumerate("pmv"):
                a, b, r = (nf.class_of(x) for x in (st[0][si][q], st[1][si][q], ref[step - 1][si][q]))
                assert (a == b).all(), (step, what, {t.names[i] for i in ci[a != b]})
                assert (a == r).all(), (step, what, {t.names[i] for i in ci[a != r]})
                fin = a == 0
                np.testing.assert_allclose(st[0][si][q][fin], ref[step - 1][si][q].numpy()[fin], rtol=1e-5, atol=1e-6)
    names = np.array(t.names)
    for si, ci in enumerate(t.cls):
        nan_in = np.isin(names[ci], ["+nan", "-nan"])
        for q in range(3):
            assert (nf.class_of(ref[-1][si][q])[nan_in] == 1).all()
        if clamp == 0:                                   # an unclamped inf: both moments inf, p NaN (then NaN everywhere)
            inf_in = np.isin(names[ci], ["+inf", "-inf"])
            assert (nf.class_of(ref[0][si][0])[inf_in] == 1).all()
            assert (np.isin(nf.class_of(ref[0][si][1])[inf_in], [2, 3])).all()
            assert (nf.class_of(ref[0][si][2])[inf_in] == 2).all()


# ---- spoiled rows -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ledger():
    lib = _lib.load()
    mp = pytest.MonkeyPatch()
    rows = []
    try:
        for c in nf.ROW_CASES + nf.CHAIN_CASES + [nf.KINK_CASE]:
            knob_env(mp, lib, c.knobs)
            rows.append((c, check_dispatch(lib, c.d, c.dc, c.widths, c.B, CU)))
    finally:
        mp.undo()
        lib.hint_debug_reload_knobs()
    return rows


def test_every_case_lands_on_its_family_and_all_eight_are_covered(ledger):
    for c, d in ledger:
        assert instances_of(d, c.entry) == c.expect, (c.name, instances_of(d, c.entry))
        assert d["nr"] == c.nr and d["groups"] == 3, (c.name, d["nr"], d["groups"])      # two full tiles and a ragged third
        assert c.B == 2 * 16 * c.nr + 5
    reached = set()
    for c, d in ledger:
        if c in nf.ROW_CASES:
            reached |= families(d)
    assert reached == ROW_FAMILIES, ROW_FAMILIES - reached
    assert {c.nr for c in nf.ROW_CASES if "wl" in c.name} == {1, 2}
    assert {d["fwd"] for c, d in ledger if c in nf.ROW_CASES} == {0, 1, 2}           # wl, general FLY off, general FLY on
    assert {c.entry for c in nf.CHAIN_CASES} == {"chain"} and {d["fwd"] for c, d in ledger if c in nf.CHAIN_CASES} == {0, 2}


@pytest.mark.parametrize("case", nf.ROW_CASES + nf.CHAIN_CASES, ids=lambda c: c.name)
def test_spoil_plan_has_every_position_and_the_oracle_makes_every_spoiled_row_non_finite(case):
    plan = nf.spoil_plan(case)
    tile, B = 16 * case.nr, case.B
    assert 0 in plan and B - 1 in plan and any(0 < r < tile - 1 for r in plan)
    assert all(r in plan for r in range(tile, 2 * tile))                                 # one whole tile
    assert any(r not in plan for r in range(0, tile)) and any(r not in plan for r in range(2 * tile, B))
    if case.nr == 2:
        pairs = [(r, r + 16) for r in range(16)]
        assert any(a in plan and b in plan for a, b in pairs) and any((a in plan) != (b in plan) for a, b in pairs)
    want = set(nf.CONTENTS) - (set() if case.dc else {"nan condition"})
    assert set(plan.values()) == want
    obj_bad, inv_bad, mask = nf.oracle_rows(case.name)
    assert int(mask.sum()) == len(plan)
    assert bool(obj_bad[mask].all()), "a spoiled row with a finite objective in the oracle: the case is vacuous"
    assert not bool(obj_bad[~mask].any()) and not bool(inv_bad[~mask].any())
    rows_in_z = torch.tensor([r for r, w in plan.items() if w != "nan condition"])
    assert bool(inv_bad[rows_in_z].all())
    if case.dc:
        assert bool(inv_bad[mask].all())                 # (a NaN condition spoils the inverse of its row as well)


def test_kink_rows_sit_exactly_on_the_kink():
    """on the all-zero rows the first layer of every node whose upper lanes no coupling below it has written (the nodes the
    forward visits first, and their ancestors along the untouched upper lanes) has pre-activations that are exactly 0 in float32
    and in float64 - products with 0 and a zero bias, in any order of the sum; every other hidden pre-activation of those rows
    lies far from a kink (KINK of test_gpu_instances.py), so relu'(0) = 0 is the only convention the comparison depends on"""
    case, nodes, P, x, c, gz, gJ = nf.kink_setup()
    rows = list(nf.KINK_ROWS)
    assert 0 in rows and case.B - 1 in rows and bool((gz[rows] != 0).any()) and bool((gJ[rows] != 0).all())
    keep = torch.zeros(case.B, dtype=torch.bool)
    keep[rows] = True
    assert not bool(gz[~keep].any()) and not bool(gJ[~keep].any())
    assert all(bool((v == 0).all()) for k, v in P.items() if k.endswith(".0.bias"))
    relu = torch.relu
    exact = {}
    for dt in (torch.float32, torch.float64):
        seen = []

        def spy(t):
            seen.append(t.detach()[rows].abs())
            return relu(t)
        torch.relu = spy
        try:
            orc.block_apply(nodes, {k: v.to(dt) for k, v in P.items()}, x.to(dt), [c.to(dt)], rev=False)
        finally:
            torch.relu = relu
        exact[dt] = [a == 0 for a in seen]
        for a in seen:
            rel = a / a.max(dim=1, keepdim=True).values.clamp(min=1e-3)
            assert bool(((a == 0) | (rel > 1e-5)).all()), "a hidden pre-activation next to (not on) a kink"
    assert all(torch.equal(a, b) for a, b in zip(exact[torch.float32], exact[torch.float64]))
    on_kink = [bool(e.all()) for e in exact[torch.float64]]
    n_leaves = sum(1 for n in nodes if n.leaf)
    assert sum(on_kink) >= 2 * n_leaves, (sum(on_kink), n_leaves)          # s and t of every leaf at the least
    assert sum(int(e.sum()) for e in exact[torch.float64]) == sum(e.numel() for e, k in zip(exact[torch.float64], on_kink) if k)


# ---- a poisoned step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow_name", list(nf.ss.FLOWS))
def test_oracle_poisoned_step_poisons_the_model(flow_name):
    ref = nf.poisoned_reference(flow_name)
    L = ref["losses"].sum(axis=1)
    assert np.isfinite(L[:2]).all(), L
    assert not np.isfinite(L[2]), "the spoiled step's loss is finite in the oracle"
    assert not np.isfinite(L[3]) and not np.isfinite(ref["nll"])
    assert ref["nan_params"] > 0
    print(f"{flow_name}: {ref['nan_params']} of {ref['n_params']} parameter tensors hold a NaN after the session")
