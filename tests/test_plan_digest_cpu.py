"""Everything the planner emits (hint_amd/csrc/hint_plan.cpp: the meta blob, slot table, thin and row records, bias map,
real-element map, weight-gradient jobs, first-layer-gradient map, pack segments and tiles, unit_w23, the plan's scalar fields;
the same for the 4-wavefront variant) equals, table by table, the digests recorded in tests/golden/plan_digests.json - for
the planner tests' shapes, the level forests of the inverse's backward pass, a shape that walks the whole retry loop, and the
knobs that change the plan.  No GPU.  A change that means to move a table regenerates the fixture (tools/plan_digests.py, which
owns the case list) and its diff shows what moved; a refactor moves nothing."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_digests as pd          # noqa: E402  (tools/plan_digests.py: the case list and the fixture's generator)
from hint_amd import _lib          # noqa: E402


def _fixture():
    with open(pd.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,kind,spec,env", pd.CASES, ids=[c[0].replace(" ", "_") for c in pd.CASES])
def test_planner_tables_match_the_recorded_digests(monkeypatch, cid, kind, spec, env):
    lib = _lib.load()
    want = _fixture()["cases"][cid]["digests"]
    got = pd.with_knobs(lib, env, lambda: pd.digests(lib, kind, spec), monkeypatch.setenv,
                        lambda k: monkeypatch.delenv(k, raising=False))
    assert sorted(got) == sorted(want), "case %r: the fixture's tables are not the library's" % cid
    moved = [t for t in got if got[t] != want[t]]
    assert not moved, "case %r: tables %s differ from tests/golden/plan_digests.json (planner of commit %s)" % (
        cid, ", ".join("%s (%s, recorded %s)" % (t, got[t], want[t]) for t in moved), _fixture()["planner_commit"])


def test_fixture_covers_the_case_list_and_the_retry_loop():
    cases = _fixture()["cases"]
    assert sorted(cases) == sorted(c[0] for c in pd.CASES)
    assert len({c[0] for c in pd.CASES}) == len(pd.CASES)
    # plans that fit at the first attempt never reach the planner's smaller-groups / fewer-slabs descents
    assert max(c.get("attempts", 1) for c in cases.values()) >= 13
    assert sum(1 for c in cases.values() if c.get("attempts", 1) > 1) >= 3
    # a plan with a 4-wavefront variant and one without are both pinned
    assert any(int(c["digests"]["alt4.meta"], 16) != 0 for c in cases.values())
    assert any(int(c["digests"]["alt4.meta"], 16) == 0 for c in cases.values())
