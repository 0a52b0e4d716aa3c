"""The planner's emitted tables, pinned by digest (hint_plan_check_digest; no GPU needed).

CASES is the one list of planner inputs: tests/test_plan_digest_cpu.py imports it and compares every case with
tests/golden/plan_digests.json, table by table.  A pull request that means to change a table regenerates the fixture and
shows in its diff which tables of which cases moved:

    python tools/plan_digests.py <commit the planner was built from>

writes the fixture from the library in the tree; run twice, it must write the same bytes.
"""
import ctypes as C
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
# per plan, in hint_plan_check_digest's order (include/hint_amd.h); the 4-wavefront variant's follow as "alt4.<table>"
TABLES = ["meta", "slots", "thins", "recs", "bmap", "real", "wjobs", "twmap", "segs", "ptiles", "unit_w23", "scalars"]
CLAMP = 4.0

# (d, dc, widths): the shapes of tests/test_plan_cpu.py and one that walks both descents of the planner's retry loop
BLOCKS = [
    (6, 0, [200, 100, 50, 25]), (6, 0, [140, 70, 35, 17]), (8, 0, [128, 64, 32, 16]), (100, 0, [224, 112, 56]),
    (100, 4, [224, 112, 56]), (43, 0, [67, 33, 16, 8]), (42, 0, [67, 33, 16, 8]), (6, 0, [512, 256, 128]),
    (100, 0, [512, 256, 128, 64]), (5, 0, [385]), (1, 0, [8]), (2, 3, [7, 5]), (128, 0, [32, 16]), (9, 2, [19, 11, 3]),
    (100, 0, [48, 24, 20, 12, 8, 8]), (26, 0, [16, 16, 8, 8, 8]),     # subtree shapes
    (128, 8, [512, 256, 128]),                                        # 13 plan attempts: tile_cap and unit_waves descents
]
# the modules of ConditionalHintFlow(10, 3, 1, 24): (attribute, d, dc)
COND = [("ac_y_to_x", 10, 3), ("ac_y", 3, 0), ("hac_x", 10, 0)]
# level forests as hint_block_inverse_backward plans them: the nodes of one depth of a tree, as depth 0
LEVELS = [(43, [67, 33, 16, 8], 2), (6, [140, 70, 35, 17], 0)]
# every knob that changes what the planner emits, on the shapes of the benchmark configs
KNOB_BLOCKS = [(6, 0, [140, 70, 35, 17]), (8, 0, [128, 64, 32, 16]), (100, 0, [224, 112, 56]), (100, 4, [224, 112, 56]),
               (43, 0, [67, 33, 16, 8]), (6, 0, [512, 256, 128])]
KNOBS = [("HINT_SUB", "0"), ("HINT_LEAN", "0"), ("HINT_WL", "0"), ("HINT_FUSE_DW1", "0"), ("HINT_NW", "4"), ("HINT_LEANW", "0"),
         ("HINT_DW_SMALL", "0"), ("HINT_DW_SMALL", "1")]
KNOB_NAMES = sorted({k for k, _ in KNOBS} | {"HINT_LEANW_MAX"})      # what a case clears before it sets its own


def _wname(widths):
    return "-".join(str(w) for w in widths)


def _cases():
    """[(id, kind, spec, env)]"""
    out = [("block d%d dc%d %s" % (d, dc, _wname(w)), "block", (d, dc, w), {}) for d, dc, w in BLOCKS]
    out += [("cond10-3-1-24 %s" % a, "cond", (a, d, dc), {}) for a, d, dc in COND]
    out += [("level d%d %s depth%d" % (d, _wname(w), dep), "level", (d, w, dep), {}) for d, w, dep in LEVELS]
    out += [("block d%d dc%d %s %s=%s" % (d, dc, _wname(w), k, v), "block", (d, dc, w), {k: v})
            for d, dc, w in KNOB_BLOCKS for k, v in KNOBS]
    return out


CASES = _cases()


def case_descs(kind, spec):
    """(descs, n_nodes, d, dc) of a case: what the planner's entry points take"""
    import hint_amd
    from hint_amd._lib import NodeDesc
    from hint_amd.hint import node_descs
    if kind == "cond":
        attr, d, dc = spec
        tree = getattr(hint_amd.ConditionalHintFlow(10, 3, 1, 24), attr)[0].tree
    else:
        d, dc = (spec[0], spec[1]) if kind == "block" else (spec[0], 0)
        widths = spec[2] if kind == "block" else spec[1]
        tree = hint_amd.HierarchicalAffineCouplingBlock([(d,)], dims_c=[(dc,)] if dc else [], c_internal=widths).tree
    nodes = tree._flat_nodes()
    descs = node_descs(nodes)[0]
    if kind == "level":
        sel = [n for n in descs if n.depth == spec[2]]
        lvl = (NodeDesc * len(sel))()
        for i, n in enumerate(sel):
            C.memmove(C.byref(lvl[i]), C.byref(n), C.sizeof(NodeDesc))
            lvl[i].depth = 0
        descs = lvl
    return descs, len(descs), d, dc


def digests(lib, kind, spec):
    """{table: "0x..."} of a case under the knobs the library has loaded"""
    descs, n, d, dc = case_descs(kind, spec)
    out = (C.c_uint64 * (2 * len(TABLES)))()
    st = lib.hint_plan_check_digest(descs, n, d, dc, CLAMP, out, len(out))
    assert st == 0, lib.hint_last_error().decode()
    names = TABLES + ["alt4." + t for t in TABLES]
    return {t: "0x%016x" % v for t, v in zip(names, out)}


def with_knobs(lib, env, fn, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """fn() with the planner's knobs set to exactly `env` (the library reads its environment once: re-read, and restored)"""
    for k in KNOB_NAMES:
        delenv(k)
    try:
        for k, v in env.items():
            setenv(k, v)
        lib.hint_debug_reload_knobs()
        return fn()
    finally:
        for k in env:
            delenv(k)
        lib.hint_debug_reload_knobs()


def attempts(lib, kind, spec):
    """plans the planner builds before it accepts one (HINT_PLAN_DUMP prints one "nw N: wave-local" line per attempt; the
    4-wavefront variant's attempts print another N)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            with_knobs(lib, {"HINT_PLAN_DUMP": "1"}, lambda: digests(lib, kind, spec))
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        nws = re.findall(r"nw (\d+): wave-local", f.read().decode())
    return sum(1 for n in nws if n == nws[0])


def main():
    from hint_amd import _lib
    lib = _lib.load()
    cases = {}
    for cid, kind, spec, env in CASES:
        entry = {"digests": with_knobs(lib, env, lambda: digests(lib, kind, spec))}
        if not env:
            entry["attempts"] = attempts(lib, kind, spec)
        cases[cid] = entry
    doc = {"planner_commit": sys.argv[1] if len(sys.argv) > 1 else "unknown",
           "note": "digests of hint_plan_check_digest, clamp 4.0; attempts: plans built before one fits "
                   "(cases with more than one walk the planner's retry loop); regenerate with tools/plan_digests.py",
           "cases": cases}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), FIXTURE))


if __name__ == "__main__":
    main()
