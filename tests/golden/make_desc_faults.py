"""Records tests/golden/desc_faults.json: what every descriptor entry point (hint_{mmd,abc,curve,hausdorff,plus,lensfit,plusfit,
overlap,corr,lensgen,fcoef,plusgen,householder}_run and their _workspace_bytes / _geometry / _job companions) answers to refused
arguments - the status and the hint_last_error() text, character for character.  tests/test_desc_faults_cpu.py replays it.

Every case is refused before any device call, so no GPU is needed: pointers are made-up integers of the right or the wrong
alignment that nothing dereferences.  record() refuses to write a case that was accepted or that got as far as a device call.

Per entry point there is a valid descriptor (`base`) and a `chain` of faults in the order the entry point checks them.  Recorded
are the null descriptor, every fault of the chain and of `extra` (further values of the same checks) alone, and every fault of
the chain together with the next one it can be combined with - which pins the fault that is reported first.  Two faults are not
combined when they set the same field or belong to the same group (two ways of spoiling one rule may cancel each other).

"unreached" lists the fail( sites of the descriptor ops' sources whose message no case produces, with the reason.

    python tests/golden/make_desc_faults.py            # rewrites the table from the built library
"""
import ctypes as C
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hint_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "desc_faults.json")
CSRC = os.path.join(ROOT, "hint_amd", "csrc")
OP_SOURCES = ("mmd", "abc", "curve", "hausdorff", "plus", "lensfit", "plusfit", "overlap", "corr", "shapegen", "plusgen", "householder")
BASE = 0x7F0000000000           # made-up addresses: a rejected call never dereferences them
NAN, INF = float("nan"), float("inf")


def ptr(i, off=0):
    return BASE + (i << 28) + off


class Fault:
    def __init__(self, name, group=None, **fields):
        self.name, self.group, self.fields = name, group, fields


def bad(field, i, align, group=None, **more):
    """the pointer `field` half an alignment unit off"""
    return Fault(f"{field} misaligned", group, **{field: ptr(i, align // 2)}, **more)


class Op:
    def __init__(self, name, desc_cls, entry, base, chain, extra=(), stream_arg=True, ws=None):
        self.name, self.desc_cls, self.entry, self.base, self.chain, self.extra = name, desc_cls, entry, base, chain, extra
        self.stream_arg, self.ws = stream_arg, ws            # ws: (the workspace function, the fields it is called on)


def sizes(field, *values):
    return [Fault(f"{field} = {v}", **{field: v}) for v in values]


def rates(field):
    return [Fault(f"{field} = {v}", **{field: v}) for v in (NAN, -1.0, INF)]


def aligns(table, first=20):
    return [bad(f, first + i, a) for i, (f, a) in enumerate(table)]


def ops():
    o = []
    # ---- hint_mmd_run ----
    base = dict(x=ptr(0), y=ptr(1), out=ptr(2), workspace=ptr(3), n_x=100, n_y=120, d=4, n_kernels=3)
    base.update({"width[0]": 0.5, "width[1]": 0.2, "width[2]": 0.2, "exponent[0]": 1.0, "exponent[1]": 1.0, "exponent[2]": 0.5})
    chain = [Fault("x null", x=None), Fault("y null", y=None), Fault("out null", out=None), Fault("workspace null", workspace=None),
             *sizes("n_x", 0), *sizes("n_y", 0), *sizes("d", 0), *sizes("n_x", (1 << 20) + 1), *sizes("n_y", (1 << 20) + 1),
             *sizes("d", 4097), *sizes("n_kernels", 0), Fault("width[0] = nan", **{"width[0]": NAN}),
             Fault("exponent[0] = nan", **{"exponent[0]": NAN}), *aligns([("x", 4), ("y", 4), ("yy", 4), ("out", 4), ("workspace", 16)]),
             Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_x", -5), *sizes("n_y", -5), *sizes("d", -5), *sizes("n_kernels", 9, -1),
             *[Fault(f"{f} = {v}", **{f: v}) for f in ("width[0]", "width[2]", "exponent[1]") for v in (0.0, -1.0, INF)]]
    o.append(Op("mmd", _lib.MmdDesc, "hint_mmd_run", base, chain, extra, ws=("hint_mmd_workspace_bytes", ("n_x", "n_y", "d"))))
    # ---- hint_abc_run ----
    base = dict(y=ptr(0), target=ptr(1), idx=ptr(2), dist=ptr(3), workspace=ptr(4), n_rows=5000, ny=2, k=100)
    chain = [Fault("y null", y=None), Fault("target null", target=None), Fault("idx null", idx=None), Fault("dist null", dist=None),
             Fault("workspace null", workspace=None), *sizes("n_rows", 0), *sizes("ny", 0), *sizes("k", 0),
             *aligns([("y", 4), ("target", 4), ("idx", 4), ("dist", 4), ("workspace", 16)]),
             Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_rows", -1, (1 << 30) + 1), *sizes("ny", 33, -1), *sizes("k", 8193, -1), Fault("k above n_rows", n_rows=10, k=11)]
    o.append(Op("abc", _lib.AbcDesc, "hint_abc_run", base, chain, extra, ws=("hint_abc_workspace_bytes", ("n_rows", "ny", "k"))))
    # ---- hint_curve_run ----
    base = dict(x=ptr(0), y=ptr(1), eps=ptr(2), target=ptr(3), dist=ptr(4), mean=ptr(5), workspace=ptr(6), noise=0.05, n_rows=300,
                n_coeffs=5, n_points=100)
    chain = [Fault("x null", x=None), Fault("y null", y=None), *sizes("n_rows", 0), *sizes("n_coeffs", 0), *sizes("n_points", 1),
             Fault("dist without target", "target", target=None), Fault("mean without target", "target", target=None, dist=None),
             *sizes("max_groups", -1), Fault("noise = nan", noise=NAN),
             *aligns([("x", 4), ("eps", 4), ("target", 4), ("y", 4), ("dist", 4), ("mean", 4)]),
             Fault("workspace null", workspace=None), bad("workspace", 30, 16), Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_rows", -1, (1 << 30) + 1), *sizes("n_coeffs", 27, 4, -1), *sizes("n_points", 129, 0), Fault("noise = inf", noise=INF),
             Fault("noise = -inf", noise=-INF)]
    o.append(Op("curve", _lib.CurveDesc, "hint_curve_run", base, chain, extra, ws=("hint_curve_workspace_bytes", ("n_rows", "n_coeffs", "n_points"))))
    # ---- hint_hausdorff_run ----
    base = dict(x=ptr(0), a_points=ptr(1), a_params=ptr(2), max_h=ptr(3), avg_h=ptr(4), chamfer=ptr(5), points=ptr(6), n_rows=64,
                n_coeffs=5, n_points=100, n_template=16)
    curve_sizes = [*sizes("n_rows", 0), *sizes("n_coeffs", 0), *sizes("n_points", 1)]
    curve_extra = [*sizes("n_rows", -1, (1 << 30) + 1), *sizes("n_coeffs", 27, 4, -1), *sizes("n_points", 1025, 0)]
    source = [Fault("x and b_points both given", "source", b_points=ptr(9)), Fault("x and b_points both null", "source", x=None)]
    chain = [Fault("a_points null", a_points=None), *source,
             Fault("points beside b_points", "source", x=None, b_points=ptr(9)),
             Fault("no output", max_h=None, avg_h=None, chamfer=None, points=None), *sizes("n_template", 0), *curve_sizes,
             Fault("template above a row's limit", "template", n_template=4097),
             Fault("ragged template above the rows' limit", "template", a_offsets=ptr(10), n_template=64 * 4096 + 1),
             *sizes("max_groups", -1),
             bad("x", 20, 4, "source"), bad("b_points", 21, 4, "source", x=None, points=None), *aligns([("a_points", 4), ("a_offsets", 8), ("a_params", 4),
                                                                                   ("max_h", 4), ("avg_h", 4), ("chamfer", 4), ("points", 4)], 22)]
    o.append(Op("hausdorff", _lib.HausdorffDesc, "hint_hausdorff_run", base, chain, [*curve_extra, *sizes("n_template", -1)]))
    # ---- hint_plus_run ----
    base = dict(x=ptr(0), params=ptr(1), segments=ptr(2), keep=ptr(3), counts=ptr(4), loss=ptr(5), max_h=ptr(6), avg_h=ptr(7), n_rows=64,
                n_coeffs=5, n_points=100, max_dist=0.02)
    chain = [Fault("params null", params=None), Fault("no output", segments=None, keep=None, counts=None, loss=None, max_h=None, avg_h=None),
             *source, *curve_sizes, Fault("max_dist = 0", max_dist=0.0), *sizes("max_groups", -1),
             bad("x", 20, 4, "source"), bad("b_points", 21, 4, "source", x=None), *aligns([("params", 4), ("segments", 4), ("keep", 4), ("counts", 4), ("loss", 4),
                                                                      ("max_h", 4), ("avg_h", 4)], 22)]
    extra = [*curve_extra, *[Fault(f"max_dist = {v}", max_dist=v) for v in (NAN, INF, -1.0)],
             Fault("n_rows = 0 without a curve", x=None, loss=None, max_h=None, avg_h=None, n_rows=0)]
    o.append(Op("plus", _lib.PlusDesc, "hint_plus_run", base, chain, extra))
    # ---- hint_lensfit_run / hint_plusfit_run ----
    sched = [*sizes("n_starts", 0), *sizes("n_steps", -1), Fault("trace without steps", n_steps=0), *rates("lr")[:1], *rates("angle_lr")[:1],
             *rates("gamma")[:1], *rates("momentum")[:1]]
    sched_extra = [*sizes("n_starts", 17, -1), *sizes("n_steps", 1025), *rates("lr")[1:], *rates("angle_lr")[1:], *rates("gamma")[1:],
                   *rates("momentum")[1:]]
    outs = [("params", 4), ("loss", 4), ("best", 4), ("all_params", 4), ("all_loss", 4), ("grad", 4), ("trace", 4)]
    base = dict(x=ptr(0), a_points=ptr(1), starts=ptr(2), n_rows=8, n_coeffs=5, n_points=100, n_template=100, n_starts=2, n_steps=10,
                lr=0.1, angle_lr=0.01, gamma=0.98, momentum=0.2, weight=1.0, **{f: ptr(3 + i) for i, (f, _) in enumerate(outs)})
    chain = [Fault("a_points null", a_points=None), Fault("starts null", starts=None), *source,
             Fault("no output", **{f: None for f, _ in outs}), *curve_sizes, *sizes("n_template", 0), *sched,
             Fault("weight = nan", weight=NAN), *sizes("max_groups", -1), bad("x", 20, 4, "source"), bad("b_points", 21, 4, "source", x=None),
             *aligns([("a_points", 4), ("starts", 4), *outs], 22)]
    extra = [*curve_extra, *sizes("n_template", 1025, -1), *sched_extra, Fault("weight = inf", weight=INF)]
    o.append(Op("lensfit", _lib.LensFitDesc, "hint_lensfit_run", base, chain, extra))
    outs = [("params", 4), ("loss", 4), ("best", 4), ("n_run", 4), ("all_params", 4), ("all_loss", 4), ("grad", 4), ("trace", 4)]
    base = dict(x=ptr(0), starts=ptr(2), n_rows=8, n_coeffs=5, n_points=100, n_starts=9, n_steps=10, lr=0.1, angle_lr=0.01, gamma=0.98,
                momentum=0.2, corner_weight=1.0, stop_loss=0.005, corner_decay=1, **{f: ptr(3 + i) for i, (f, _) in enumerate(outs)})
    chain = [Fault("starts null", starts=None), *source, Fault("no output", **{f: None for f, _ in outs}), *curve_sizes, *sched,
             Fault("corner_weight = nan", corner_weight=NAN), *sizes("max_groups", -1), bad("x", 20, 4, "source"), bad("b_points", 21, 4, "source", x=None),
             *aligns([("starts", 4), *outs], 22)]
    extra = [*curve_extra, *sched_extra, Fault("corner_weight = -inf", corner_weight=-INF)]
    o.append(Op("plusfit", _lib.PlusFitDesc, "hint_plusfit_run", base, chain, extra))
    # ---- hint_overlap_run ----
    base = dict(x=ptr(0), a_points=ptr(1), a_params=ptr(2), areas=ptr(3), iou=ptr(4), dice=ptr(5), crossings=ptr(6), n_rows=64, n_coeffs=5,
                n_points=100, n_template=16)
    chain = [Fault("no output", areas=None, iou=None, dice=None, crossings=None),
             Fault("a_points and plus_params both given", "template", plus_params=ptr(9)),
             Fault("a_points and plus_params both null", "template", a_points=None),
             Fault("a_offsets without a_points", "template", a_points=None, plus_params=ptr(9), a_offsets=ptr(10), a_params=None),
             Fault("a_params without a_points", "template", a_points=None, plus_params=ptr(9)), *source,
             Fault("n_template = 2", "template", n_template=2), *curve_sizes,
             Fault("template above a row's limit", "template", n_template=4097),
             Fault("ragged template above the rows' limit", "template", a_offsets=ptr(10), n_template=64 * 4096 + 1),
             *sizes("max_groups", -1), bad("x", 20, 4, "source"), bad("b_points", 21, 4, "source", x=None),
             *aligns([("a_points", 4), ("a_offsets", 8), ("a_params", 4)], 22),
             Fault("plus_params misaligned", "template", a_points=None, a_params=None, plus_params=ptr(25, 2)),
             *aligns([("areas", 4), ("iou", 4), ("dice", 4), ("crossings", 4)], 26)]
    extra = [*curve_extra, *sizes("n_points", 2), Fault("n_template = 0", "template", n_template=0)]
    o.append(Op("overlap", _lib.OverlapDesc, "hint_overlap_run", base, chain, extra))
    # ---- hint_corr_run ----
    base = dict(x=ptr(0), target=ptr(1), corr=ptr(2), out=ptr(3), workspace=ptr(4), n=333, d=20)
    chain = [Fault("x null", x=None), Fault("out null", out=None), Fault("workspace null", workspace=None),
             Fault("nothing to compute", target=None, corr=None), *sizes("n", 0), *sizes("d", 0), *sizes("n", (1 << 24) + 1), *sizes("d", 513),
             *aligns([("x", 4), ("target", 8), ("corr", 8), ("out", 8), ("workspace", 16)]),
             Fault("workspace one byte short", workspace_bytes=-1)]
    o.append(Op("corr", _lib.CorrDesc, "hint_corr_run", base, chain, [*sizes("n", -1), *sizes("d", -1)],
                ws=("hint_corr_workspace_bytes", ("n", "d"))))
    # ---- hint_lensgen_run ----
    base = dict(x=ptr(0), ring=ptr(1), counts=ptr(2), eps=ptr(3), draws_out=ptr(4), workspace=ptr(5), n_rows=1000, seed=7, offset=0)
    chain = [Fault("x null", x=None), Fault("workspace null", workspace=None), *sizes("n_rows", 0),
             Fault("offset + n_rows overflows", offset=2 ** 64 - 1000), *sizes("max_groups", -1),
             *aligns([("draws", 16), ("x", 16), ("ring", 8), ("counts", 4), ("eps", 8), ("draws_out", 16), ("workspace", 16)]),
             Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_rows", -3, (1 << 30) + 1), Fault("workspace one byte short at the largest n_rows", n_rows=1 << 30, workspace_bytes=-1)]
    o.append(Op("lensgen", _lib.LensGenDesc, "hint_lensgen_run", base, chain, extra, ws=("hint_lensgen_workspace_bytes", ("n_rows",))))
    # ---- hint_fcoef_run ----
    base = dict(points=ptr(0), counts=ptr(1), x=ptr(2), workspace=ptr(3), n_rows=100, p_max=32, n_coeffs=5)
    chain = [Fault("points null", points=None), Fault("x null", x=None), Fault("workspace null", workspace=None), *sizes("n_rows", 0),
             *sizes("n_coeffs", 0), *sizes("p_max", 4), *sizes("max_groups", -1),
             *aligns([("points", 8), ("counts", 4), ("x", 4), ("workspace", 16)]), Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_rows", -1, (1 << 24) + 1), *sizes("n_coeffs", 27, 4, -1), *sizes("p_max", 1025, 0)]
    o.append(Op("fcoef", _lib.FcoefDesc, "hint_fcoef_run", base, chain, extra, ws=("hint_fcoef_workspace_bytes", ("n_rows", "p_max", "n_coeffs"))))
    # ---- hint_plusgen_run (the stream is a field) ----
    base = dict(x=ptr(0), y=ptr(1), outline=ptr(2), counts=ptr(3), corners=ptr(4), draws_out=ptr(5), workspace=ptr(6), n_rows=1000, seed=7,
                offset=0)
    chain = [Fault("x and y both null", x=None, y=None), Fault("workspace null", workspace=None), *sizes("n_rows", 0),
             Fault("rows and draws both given", "rows", rows=ptr(8), draws=ptr(9)), Fault("offset + n_rows overflows", offset=2 ** 64 - 1000),
             *sizes("max_groups", -1), Fault("target[1] = inf", target=(0.1, INF, 0.3, 1.0)), Fault("ratio = 4.001", target=(0.1, 0.2, 0.3, 4.001)),
             bad("rows", 20, 8, "rows"), bad("draws", 21, 4, "rows"), *aligns([("x", 16), ("y", 16), ("outline", 8), ("counts", 4), ("corners", 4),
                                                              ("draws_out", 4), ("workspace", 16)], 22),
             Fault("workspace one byte short", workspace_bytes=-1)]
    extra = [*sizes("n_rows", -3, (1 << 30) + 1), Fault("target[0] = nan", target=(NAN, 0.2, 0.3, 1.0)),
             Fault("target[2] = -inf", target=(0.1, 0.2, -INF, 1.0)), Fault("target[3] = nan", target=(0.1, 0.2, 0.3, NAN)),
             *[Fault(f"ratio = {v}", target=(0.1, 0.2, 0.3, v)) for v in (0.2499, -1.0, 0.0)],
             Fault("workspace one byte short at the largest n_rows", n_rows=1 << 30, workspace_bytes=-1)]
    o.append(Op("plusgen", _lib.PlusGenDesc, "hint_plusgen_run", base, chain, extra, stream_arg=False,
                ws=("hint_plusgen_workspace_bytes", ("n_rows",))))
    # ---- hint_householder_run (the stream is a field): build, apply, grad ----
    hh = [("Vs", 4), ("W", 4), ("x", 4), ("y", 4), ("g_y", 4), ("g_x", 4), ("g_W", 4), ("g_V", 4), ("workspace", 16)]
    base = dict(op=0, B=1, d=8, n=8, Vs=ptr(0), W=ptr(1))
    chain = [*sizes("op", -1), *sizes("d", 0), *sizes("n", 0), *aligns(hh), Fault("Vs null", Vs=None), Fault("W null", W=None)]
    o.append(Op("householder build", _lib.HouseholderDesc, "hint_householder_run", base, chain,
                [*sizes("op", 3), *sizes("d", 129, -1), *sizes("n", 257, -1)], stream_arg=False))
    base = dict(op=1, B=64, d=8, n=0, W=ptr(1), x=ptr(2), y=ptr(3))
    chain = [*sizes("d", 0), *sizes("B", 0), *aligns(hh), Fault("x null", x=None), Fault("W null", W=None), Fault("y null", y=None),
             Fault("y aliases x", "alias", y=ptr(2, 64))]
    o.append(Op("householder apply", _lib.HouseholderDesc, "hint_householder_run", base, chain,
                [*sizes("d", 129), *sizes("B", (1 << 22) + 1, -1)], stream_arg=False))
    base = dict(op=2, B=64, d=8, n=8, Vs=ptr(0), W=ptr(1), x=ptr(2), g_y=ptr(4), g_x=ptr(5), g_W=ptr(6), g_V=ptr(7), workspace=ptr(8))
    chain = [*sizes("d", 0), *sizes("n", 0), *sizes("B", 0), *aligns(hh), Fault("g_y null", g_y=None), Fault("W null", W=None),
             Fault("nothing to compute", g_x=None, g_W=None, g_V=None), Fault("x null", x=None), Fault("Vs null", Vs=None),
             Fault("g_x aliases g_y", "alias", g_x=ptr(4, 64)), Fault("workspace null", workspace=None),
             Fault("workspace one byte short", workspace_bytes=-1)]
    o.append(Op("householder grad", _lib.HouseholderDesc, "hint_householder_run", base, chain,
                [*sizes("d", 129), *sizes("n", 257), *sizes("B", (1 << 22) + 1)], stream_arg=False,
                ws=("hint_householder_workspace_bytes", ("op", "B", "d", "n"))))
    return o


# the refused calls of the functions that take sizes, not a descriptor
CALLS = [
    ("hint_mmd_workspace_bytes", [(0, 120, 4), (100, 0, 4), (100, 120, 0), (-1, 120, 4), ((1 << 20) + 1, 120, 4), (100, (1 << 20) + 1, 4),
                                  (100, 120, 4097), (0, 0, 0)]),
    ("hint_mmd_job", [(0, 120, 0, 0, 0), (100, 0, 0, 0, 0), (100, 120, 0, -2, 0), (100, 120, 0, 10 ** 9, 0), (100, 120, 0, 0, 4),
                      (100, 120, 0, 0, -1), (100, 120, 1, -1, 2)]),
    ("hint_abc_workspace_bytes", [(0, 2, 100), ((1 << 30) + 1, 2, 100), (5000, 0, 100), (5000, 33, 100), (5000, 2, 0), (5000, 2, 8193),
                                  (10, 2, 11), (0, 0, 0)]),
    ("hint_abc_geometry", [(0, 2, 0), ((1 << 30) + 1, 2, 0), (5000, 0, 0), (5000, 33, 0), (5000, 2, -1), (5000, 2, 3), (0, 2, 3)]),
    ("hint_curve_workspace_bytes", [(0, 5, 100), ((1 << 30) + 1, 5, 100), (300, 0, 100), (300, 4, 100), (300, 27, 100), (300, 5, 1),
                                    (300, 5, 129), (0, 0, 0)]),
    ("hint_curve_geometry", [(0, 5, 100, 0), (300, 4, 100, 0), (300, 5, 129, 0), (300, 5, 100, -1), (300, 5, 100, 4), (0, 5, 100, 4)]),
    ("hint_hausdorff_workspace_bytes", [(0, 5, 100, 16), ((1 << 30) + 1, 5, 100, 16), (64, 4, 100, 16), (64, 27, 100, 16), (64, 5, 1, 16),
                                        (64, 5, 1025, 16), (64, 0, 1, 16), (64, 5, 100, 0), (64, 5, 100, 4097), (0, 4, 1, 0)]),
    ("hint_hausdorff_geometry", [(0, 100, 16, 0), (64, 1, 16, 0), (64, 1025, 16, 0), (64, 100, 0, 0), (64, 100, 4097, 0), (64, 100, 16, -1),
                                 (64, 100, 16, 5), (0, 100, 16, 5)]),
    ("hint_plus_workspace_bytes", [(0, 5, 100), ((1 << 30) + 1, 5, 100), (64, 4, 100), (64, 27, 100), (64, 5, 1), (64, 5, 1025), (64, 0, 1)]),
    ("hint_plus_geometry", [(0, 100, 0), (64, 1, 0), (64, 1025, 0), (64, 100, -1), (64, 100, 5), (0, 100, 5)]),
    ("hint_lensfit_workspace_bytes", [(0, 5, 100, 100, 2, 10), (8, 4, 100, 100, 2, 10), (8, 5, 1, 100, 2, 10), (8, 5, 100, 0, 2, 10),
                                      (8, 5, 100, 1025, 2, 10), (8, 5, 100, 100, 0, 10), (8, 5, 100, 100, 17, 10), (8, 5, 100, 100, 2, -1),
                                      (8, 5, 100, 100, 2, 1025), (8, 5, 100, 0, 0, -1)]),
    ("hint_lensfit_geometry", [(0, 100, 0), (8, 1, 0), (8, 1025, 0), (8, 100, -1), (8, 100, 5), (0, 100, 5)]),
    ("hint_plusfit_workspace_bytes", [(0, 5, 100, 9, 10), (8, 4, 100, 9, 10), (8, 5, 1, 9, 10), (8, 5, 100, 0, 10), (8, 5, 100, 17, 10),
                                      (8, 5, 100, 9, -1), (8, 5, 100, 9, 1025), (8, 5, 1, 0, -1)]),
    ("hint_plusfit_geometry", [(0, 100, 0), (8, 1, 0), (8, 1025, 0), (8, 100, -1), (8, 100, 5), (0, 100, 5)]),
    ("hint_overlap_workspace_bytes", [(0, 5, 100, 16), (64, 4, 100, 16), (64, 5, 1, 16), (64, 5, 2, 16), (64, 5, 1025, 16), (64, 5, 100, 2),
                                      (64, 5, 100, 4097), (64, 5, 2, 2)]),
    ("hint_overlap_geometry", [(0, 100, 16, 0), (64, 2, 16, 0), (64, 1025, 16, 0), (64, 100, 2, 0), (64, 100, 4097, 0), (64, 100, 16, -1),
                               (64, 100, 16, 5), (0, 100, 16, 5)]),
    ("hint_corr_workspace_bytes", [(0, 20), (333, 0), ((1 << 24) + 1, 20), (333, 513), (-1, 20), (0, 0)]),
    ("hint_corr_job", [(0, 20, 0, 0), (333, 0, 0, 0), (333, 20, -2, 0), (333, 20, 10 ** 9, 0), (333, 20, 0, 5), (333, 20, 0, -1),
                       (333, 20, -1, 4)]),
    ("hint_lensgen_workspace_bytes", [(0,), (-1,), ((1 << 30) + 1,)]),
    ("hint_fcoef_workspace_bytes", [(0, 32, 5), ((1 << 24) + 1, 32, 5), (100, 32, 0), (100, 32, 4), (100, 32, 27), (100, 4, 5), (100, 1025, 5),
                                    (0, 4, 4)]),
    ("hint_plusgen_workspace_bytes", [(0,), (-1,), ((1 << 30) + 1,)]),
    ("hint_householder_workspace_bytes", [(-1, 64, 8, 8), (3, 64, 8, 8), (2, 64, 0, 8), (2, 64, 129, 8), (2, 64, 8, 0), (2, 64, 8, 257),
                                          (2, 0, 8, 8), (2, (1 << 22) + 1, 8, 8), (0, 0, 8, 0), (1, 0, 8, 0), (3, 0, 0, 0)]),
    ("hint_householder_geometry", [(0, 8, 0), ((1 << 22) + 1, 8, 0), (64, 0, 0), (64, 129, 0), (64, 8, -1), (64, 8, 3), (0, 8, 3)]),
]

# fail( sites no case reaches: format -> why
UNREACHED_WHY = {
    "%s: %s": "HIP_TRY: a device call has to fail",
}


def _fill(op, lib, faults):
    """the op's valid descriptor with `faults` applied; keep: what the descriptor points to.  workspace_bytes is what the op's
    workspace function says of the descriptor's sizes, plus the fault's difference"""
    desc, keep = op.desc_cls(), []
    fields = dict(op.base)
    for f in faults:
        fields.update(f.fields)
    if op.ws:
        need = getattr(lib, op.ws[0])(*[fields[k] for k in op.ws[1]])
        assert need > 0 or len(faults) > 0, op.name
        fields["workspace_bytes"] = max(0, need + fields.get("workspace_bytes", 0))
    for k, v in fields.items():
        m = re.fullmatch(r"(\w+)\[(\d+)\]", k)
        if m:
            getattr(desc, m.group(1))[int(m.group(2))] = v
        elif k == "target" and isinstance(v, tuple):
            keep.append((C.c_float * 4)(*v))
            desc.target = keep[-1]
        else:
            setattr(desc, k, v)
    return desc, keep


def _run(op, lib, faults):
    desc, keep = _fill(op, lib, faults)
    fn = getattr(lib, op.entry)
    st = fn(C.byref(desc), None) if op.stream_arg else fn(C.byref(desc))
    return [st, (lib.hint_last_error() or b"").decode()]


def combinable(a, b):
    return not (set(a.fields) & set(b.fields)) and (a.group is None or a.group != b.group)


def fail_sites():
    """the format of every fail( call in the descriptor ops' sources and the headers beside them"""
    files = [os.path.join(CSRC, f"hint_{n}.hip") for n in OP_SOURCES] + sorted(glob.glob(os.path.join(CSRC, "*.hpp")))
    formats = set()
    for path in files:
        src = open(path).read()
        for m in re.finditer(r"\bfail\(\s*((?:\"(?:[^\"\\]|\\.)*\"\s*)+)", src):
            formats.add("".join(re.findall(r"\"((?:[^\"\\]|\\.)*)\"", m.group(1))).replace('\\"', '"'))
    return sorted(formats)


def unreached(messages):
    """the formats no message is an instance of; a message counts for the matching format with the most literal text"""
    formats = fail_sites()
    spec = re.compile(r"%(?:lld|zu|[sdg])")
    rx = {f: re.compile(".*".join(re.escape(p) for p in spec.split(f)), re.S) for f in formats}
    lit = {f: len(spec.sub("", f)) for f in formats}
    hit = set()
    for msg in messages:
        match = [f for f in formats if rx[f].fullmatch(msg)]
        assert match, f"no fail( site words {msg!r}"
        hit.add(max(match, key=lambda f: lit[f]))
    return [f for f in formats if f not in hit]


def record():
    """the whole table from the loaded library: {"cases": {op: {case: [status, text]}}, "calls": {call: [value, text]},
    "unreached": {format: why}}"""
    lib = _lib.load()
    cases, calls, messages = {}, {}, []

    def refused(where, st, text):
        assert st != 0 and text.startswith("hint_"), f"{where}: not refused before the device ({st}, {text!r})"
        messages.append(text)

    for op in ops():
        table = cases[op.name] = {}
        fn = getattr(lib, op.entry)
        st = fn(None, None) if op.stream_arg else fn(None)
        table["desc null"] = [st, (lib.hint_last_error() or b"").decode()]
        for f in [*op.chain, *op.extra]:
            assert f.name not in table, (op.name, f.name)
            table[f.name] = _run(op, lib, [f])
        for i, a in enumerate(op.chain):
            b = next((b for b in op.chain[i + 1:] if combinable(a, b)), None)
            if b is not None:
                table[f"{a.name} + {b.name}"] = _run(op, lib, [a, b])
        for name, (st, text) in table.items():
            refused(f"{op.name}: {name}", st, text)
    for fname, arglists in CALLS:
        for args in arglists:
            v = getattr(lib, fname)(*args)
            text = (lib.hint_last_error() or b"").decode()
            assert v in (0, -1), (fname, args, v)
            refused(f"{fname}{args}", 1, text)
            calls[f"{fname}{args}"] = [v, text]
    left = unreached(messages)
    assert set(left) == set(UNREACHED_WHY), (left, sorted(UNREACHED_WHY))
    return {"cases": cases, "calls": calls, "unreached": {f: UNREACHED_WHY[f] for f in left}}


if __name__ == "__main__":
    table = record()
    with open(OUT, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{OUT}: {sum(len(v) for v in table['cases'].values())} descriptor cases, {len(table['calls'])} calls, "
          f"{len(table['unreached'])} unreached fail( sites")
