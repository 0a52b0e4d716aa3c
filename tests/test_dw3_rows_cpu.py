"""Part B's launch list without a GPU (hint_plan_check_wjob): with HINT_DW3_ROWS on, the weight-gradient jobs table minus the dW3
jobs of the units with at most four outputs, plus the row jobs (hint_wgrad.hip dw_rows), covers every real element of W3 and b3 of
every such unit exactly once and every other tensor as before; with the knob off the list is the table; the planner's digested
tables do not move with the knob."""
import ctypes as C

import numpy as np
import pytest

import hint_amd
from hint_amd import _lib
from hint_amd.hint import node_descs

FIELDS = ["psrc", "pcol", "M", "mw", "qsrc", "qcol", "N", "nw", "ldo", "wofs", "bofs", "r_r", "r_gcol", "r_h", "r_wcol"]
WSRC_GST, WSRC_A2, WSRC_GSTR = 2, 4, 9          # hint_dev.h
DW3R_COLS = 256
KNOB = "HINT_DW3_ROWS"
INT64_MIN = -2 ** 63

# (name, d, dc, widths): cfg 2's block, r = 1, r = 4, a conditional tree (every subnet of these trees has r <= 4)
TREES = [
    ("cfg2_block", 6, 0, (140, 70, 35, 17)),
    ("d2_r1", 2, 0, (17,)),
    ("d8_r4", 8, 0, (64, 16)),
    ("conditional", 6, 4, (140, 70)),
]


class Plan:
    def __init__(self, d, dc, widths):
        self.d, self.dc = d, dc
        blk = hint_amd.HierarchicalAffineCouplingBlock([(d,)], dims_c=[(dc,)] if dc else [], c_internal=list(widths))
        self.nodes = blk.tree._flat_nodes()
        self.descs, self.params, self.offsets, self.total = node_descs(self.nodes)
        self.lib = _lib.load()

    def wjob(self, variant, j, field):
        v = self.lib.hint_plan_check_wjob(self.descs, len(self.nodes), self.d, self.dc, 4.0, variant, j, field)
        assert v != INT64_MIN, self.lib.hint_last_error().decode()
        return v

    def counts(self, variant=0):
        return dict(zip(["list", "small", "rows", "table", "table_small"], (self.wjob(variant, -1, f) for f in range(5))))

    def jobs(self, variant=0):
        n = self.wjob(variant, -1, 0)
        return [dict(zip(FIELDS, (self.wjob(variant, j, f) for f in range(len(FIELDS))))) for j in range(n)]

    def has_variant(self):
        return self.lib.hint_plan_check_wjob(self.descs, len(self.nodes), self.d, self.dc, 4.0, 1, -1, 0) != INT64_MIN

    def digests(self):
        out = (C.c_uint64 * 24)()
        assert self.lib.hint_plan_check_digest(self.descs, len(self.nodes), self.d, self.dc, 4.0, out, 24) == 0
        return list(out)

    def units(self):
        """(r, h, offset of W3, offset of b3) of every subnet, from the node table"""
        out = []
        for dsc in self.descs:
            for net in range(2):
                out.append((dsc.r, dsc.h, dsc.p_off[net * 6 + 4], dsc.p_off[net * 6 + 5]))
        return out


def coverage(jobs, total):
    """how often every element of the flat gradient is written by the jobs of a list"""
    cov = np.zeros(total, dtype=np.int32)
    for j in jobs:
        for m in range(j["M"]):
            if j["N"] > 0:
                cov[j["wofs"] + m * j["ldo"]:j["wofs"] + m * j["ldo"] + j["N"]] += 1
        if j["bofs"] >= 0:
            cov[j["bofs"]:j["bofs"] + j["M"]] += 1
    return cov


@pytest.fixture
def knob(monkeypatch):
    lib = _lib.load()

    def set_(value):
        if value is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, value)
        lib.hint_debug_reload_knobs()
    yield set_
    monkeypatch.undo()
    lib.hint_debug_reload_knobs()


@pytest.mark.parametrize("name,d,dc,widths", TREES, ids=[t[0] for t in TREES])
def test_rows_cover_w3_b3_exactly_once(name, d, dc, widths, knob):
    p = Plan(d, dc, widths)
    variants = [0, 1] if p.has_variant() else [0]
    for variant in variants:
        knob("0")
        off_counts, off_jobs = p.counts(variant), p.jobs(variant)
        assert off_counts["rows"] == 0 and off_counts["list"] == off_counts["table"] and off_counts["small"] == off_counts["table_small"]
        cov_off = coverage(off_jobs, p.total)
        knob("1")
        cnt, jobs = p.counts(variant), p.jobs(variant)
        assert (cnt["table"], cnt["table_small"]) == (off_counts["table"], off_counts["table_small"])     # the table is the planner's
        small_units = [u for u in p.units() if u[0] <= 4]
        assert small_units, name
        # the list: [the table's jobs in order, minus the covered dW3 jobs | the row jobs]
        rows = jobs[cnt["list"] - cnt["rows"]:]
        kept = jobs[:cnt["list"] - cnt["rows"]]
        assert kept == [j for j in off_jobs if not (j["psrc"] == WSRC_GST and j["qsrc"] == WSRC_A2 and j["r_r"] <= 4)]
        assert all(j["psrc"] == WSRC_GSTR and j["qsrc"] == WSRC_A2 for j in rows)
        assert not any(j["psrc"] == WSRC_GSTR for j in kept)
        assert cnt["rows"] == sum(-(-h // DW3R_COLS) for r, h, _, _ in small_units)
        for j in rows:
            assert 1 <= j["M"] == j["r_r"] <= 4 and 1 <= j["N"] <= DW3R_COLS and j["nw"] == -(-j["N"] // 64) and j["ldo"] == j["r_h"]
            assert j["pcol"] == j["r_gcol"] and j["r_wcol"] <= j["qcol"] and j["qcol"] + j["N"] <= j["r_wcol"] + j["r_h"]
        cov = coverage(jobs, p.total)
        for r, h, w3, b3 in small_units:
            assert (cov[w3:w3 + r * h] == 1).all(), (name, variant, "W3", r, h)
            assert (cov[b3:b3 + r] == 1).all(), (name, variant, "b3", r, h)
        assert (cov == cov_off).all(), "some other element's coverage changed with the knob"
        print(f"{name} variant {variant}: {off_counts['table']} jobs in the table, {cnt['list'] - cnt['rows']} kept + {cnt['rows']} row jobs")


def test_cfg2_census(knob):
    """the issue's census of cfg 2's block: 14 dW3 jobs of 48 leave, 6 row jobs (one per subnet) come"""
    p = Plan(6, 0, (140, 70, 35, 17))
    knob("0")
    off = p.jobs()
    dw3 = [j for j in off if j["psrc"] == WSRC_GST and j["qsrc"] == WSRC_A2]
    assert (len(off), len(dw3)) == (48, 14)
    knob("1")
    c = p.counts()
    assert (c["list"], c["rows"], c["small"]) == (40, 6, 0)
    assert sorted(j["nw"] for j in p.jobs()[-6:]) == [2, 2, 2, 2, 3, 3]


def test_default_is_on_for_plans_without_subtree_groups(knob):
    knob(None)
    assert Plan(6, 0, (140, 70, 35, 17)).counts()["rows"] == 6          # wave-local
    assert Plan(2, 0, (17,)).counts()["rows"] == 2
    assert Plan(6, 4, (140, 70)).counts()["rows"] == 6                  # a condition: general kernels
    assert Plan(100, 0, (224, 112, 56)).counts()["rows"] > 0            # plus_hint_4's tree: general kernels, no subtree groups
    assert Plan(43, 0, (67, 33, 16, 8)).counts()["rows"] == 0           # MINIBOONE's tree: subtree groups
    assert Plan(100, 0, (32, 16, 8)).counts()["rows"] == 0              # a narrow d = 100 tree with a subtree level


@pytest.mark.parametrize("name,d,dc,widths", TREES, ids=[t[0] for t in TREES])
def test_digests_do_not_move_with_the_knob(name, d, dc, widths, knob):
    p = Plan(d, dc, widths)
    knob(None)
    ref = p.digests()
    assert any(ref)
    for v in ("0", "1"):
        knob(v)
        assert p.digests() == ref, v


def test_knob_is_reported_when_set(knob):
    lib = _lib.load()
    knob(None)
    assert KNOB not in lib.hint_build_info().decode()
    knob("0")
    assert f"{KNOB}=0" in lib.hint_build_info().decode()


def test_bad_job_index_fails_loudly(knob):
    p = Plan(2, 0, (17,))
    lib = p.lib
    n = p.wjob(0, -1, 0)
    for j, f in ((n, 0), (0, len(FIELDS)), (-2, 0), (-1, 5)):
        assert lib.hint_plan_check_wjob(p.descs, len(p.nodes), 2, 0, 4.0, 0, j, f) == INT64_MIN
        assert b"hint_plan_check_wjob" in lib.hint_last_error()
