"""The refusals of the descriptor entry points are behaviour: tests/golden/desc_faults.json holds, for every refused call that
tests/golden/make_desc_faults.py builds - each fault alone, and each together with the next one in the entry point's checking
order - the status and the hint_last_error() text, and the built library answers each of them the same, character for character
(no GPU: every case is refused before any device call).  The fail( sites the table does not reach are listed in it with the
reason; that list does not change either."""
import json

import pytest

import make_desc_faults as gen

TABLE = json.load(open(gen.OUT))


@pytest.fixture(scope="module")
def replayed():
    return gen.record()


def test_the_table_holds_every_entry_point_and_every_kind_of_case():
    assert set(TABLE) == {"cases", "calls", "unreached"}
    assert set(TABLE["cases"]) == {"mmd", "abc", "curve", "hausdorff", "plus", "lensfit", "plusfit", "overlap", "corr", "lensgen",
                                   "fcoef", "plusgen", "householder build", "householder apply", "householder grad"}
    for op, cases in TABLE["cases"].items():
        assert "desc null" in cases and any(" + " in name for name in cases) and any("misaligned" in name for name in cases), op
        assert all(st == 1 and text.startswith("hint_") for st, text in cases.values()), op
    for op in ("mmd", "abc", "curve", "corr", "lensgen", "fcoef", "plusgen", "householder grad"):
        assert {"workspace null", "workspace misaligned", "workspace one byte short"} <= set(TABLE["cases"][op]), op
    called = {call.split("(")[0] for call in TABLE["calls"]}
    assert called == {name for name, _ in gen.CALLS} and len(called) == 23


def test_every_descriptor_case_is_refused_with_the_recorded_status_and_text(replayed):
    for op, cases in TABLE["cases"].items():
        assert sorted(replayed["cases"][op]) == sorted(cases), op
        for name, want in cases.items():
            assert replayed["cases"][op][name] == want, (op, name)


def test_every_size_call_is_refused_with_the_recorded_value_and_text(replayed):
    assert sorted(replayed["calls"]) == sorted(TABLE["calls"])
    for call, want in TABLE["calls"].items():
        assert replayed["calls"][call] == want, call


def test_the_unreached_fail_sites_are_the_recorded_ones(replayed):
    assert replayed["unreached"] == TABLE["unreached"] == gen.UNREACHED_WHY
