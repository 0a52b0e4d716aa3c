"""CPU tests of hint_householder_many_run, the entry point of the m trainable permutations of one flow: both symbols, the
struct's layout against the header, every rejection (they come before any device call), the workspace query, and what the three
header ledgers (stream table, poison table, large-index cases) see of the new declarations."""
import ctypes as C
import os
import re

import pytest

from hint_amd import _lib
from test_large_cases_cpu import descriptor_entry_points
from test_poison_table_cpu import declarations, writable_device_pointers
from test_stream_table_cpu import takes_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD, ROWS, FINISH = 0, 1, 2
GRAD = 2
RUN, SIZER = "hint_householder_many_run", "hint_householder_many_workspace_bytes"
WHO = RUN + ": "


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    decls = declarations()
    for name in (RUN, SIZER):
        assert name in _lib.exported_symbols() and name in decls and getattr(lib, name) is not None
    assert decls[RUN] == ["const hint_householder_many* job"]
    assert [" ".join(p.split()) for p in decls[SIZER]] == ["int32_t op", "int32_t m", "int32_t B", "int32_t d", "int32_t n"]
    assert (_lib.HOUSEHOLDER_MANY_BUILD, _lib.HOUSEHOLDER_MANY_ROWS, _lib.HOUSEHOLDER_MANY_FINISH) == (BUILD, ROWS, FINISH)
    src = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    for name, v in (("BUILD", 0), ("ROWS", 1), ("FINISH", 2)):
        assert re.search(r"#define HINT_HOUSEHOLDER_MANY_%s %d\b" % (name, v), src)
    assert lib.hint_abi_version() == 8                       # additive: the version stays


def test_the_frozen_ledgers_do_not_see_the_new_functions():
    """the stream is a field, the struct is no `_desc` and the parameter no `desc`, and no parameter is a writable pointer: what
    the three ledgers would have demanded is tested in tests/test_gpu_householder_many.py instead"""
    decls = declarations()
    for name in (RUN, SIZER):
        assert not takes_stream(decls[name])
        assert writable_device_pointers(decls[name]) == []
        assert name not in descriptor_entry_points()
    assert "hint_householder_run" in descriptor_entry_points()


# ---- the struct ----
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t}


def header_fields():
    src = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    body = re.search(r"typedef struct hint_householder_many \{(.*?)\} hint_householder_many;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        base, star, names = m.group(1), m.group(2), m.group(3)
        for name in names.split(","):
            fields.append((name.strip(), C.c_void_p if star else _CTYPES[base]))
    return fields


def test_struct_mirrors_the_header():
    fields = header_fields()
    assert [f for f, _ in fields] == [f for f, _ in _lib.HouseholderMany._fields_]
    assert fields[-1][0] == "stream"                          # the stream is a field, as in hint_householder_desc
    twin = type("Twin", (C.Structure,), {"_fields_": fields})
    assert C.sizeof(twin) == C.sizeof(_lib.HouseholderMany)
    for (name, _), (_, ct) in zip(fields, _lib.HouseholderMany._fields_):
        assert getattr(twin, name).offset == getattr(_lib.HouseholderMany, name).offset, name
        assert C.sizeof(ct) == getattr(twin, name).size, name


# ---- rejections ----
P = 0x10000                      # a plausible, aligned device address: no rejected run ever reads it
WS = 0x4000000
M, B, D, N = 3, 32, 8, 8


def slot_bytes(B=B, d=D, n=N):
    return _lib.load().hint_householder_workspace_bytes(GRAD, B, d, n)


def job_of(kind, **kw):
    j = _lib.HouseholderMany()
    op = kind
    j.op, j.m, j.j, j.B, j.d, j.n = op, M, 1, B, D, N
    j.Vs, j.vs_stride, j.W, j.w_stride = P, N * D, 2 * P, D * D
    if op == ROWS:
        j.x, j.g_y, j.g_x = 3 * P, 4 * P, 5 * P
    if op == FINISH:
        j.g_W, j.gw_stride, j.g_V, j.gv_stride = 6 * P, D * D, 7 * P, N * D
    if op != BUILD:
        j.workspace, j.workspace_bytes, j.ws_stride = WS, M * slot_bytes(), slot_bytes() // 4
    for k, v in kw.items():
        setattr(j, k, v)
    return j


REJECT = [
    # an unknown op
    ("op", job_of(BUILD, op=3)), ("op", job_of(BUILD, op=-1)),
    # m, d, n, B, j outside their limits
    ("m", job_of(BUILD, m=0)), ("m", job_of(FINISH, m=65)),
    ("d", job_of(BUILD, d=0)), ("d", job_of(ROWS, d=129)), ("n", job_of(BUILD, n=0)), ("n", job_of(FINISH, n=257)),
    ("B", job_of(ROWS, B=0)), ("B", job_of(FINISH, B=(1 << 22) + 1)),
    ("j", job_of(ROWS, j=-1)), ("j", job_of(ROWS, j=M)),
    # a required pointer that is NULL
    ("Vs", job_of(BUILD, Vs=None)), ("W", job_of(BUILD, W=None)),
    ("x", job_of(ROWS, x=None)), ("g_y", job_of(ROWS, g_y=None)), ("W", job_of(ROWS, W=None)),
    ("Vs", job_of(FINISH, Vs=None)), ("W", job_of(FINISH, W=None)), ("g_V", job_of(FINISH, g_V=None)),
    ("workspace", job_of(ROWS, workspace=None)), ("workspace", job_of(FINISH, workspace=None)),
    # ... misaligned by 4, the workspace by 16
    ("Vs", job_of(BUILD, Vs=P + 2)), ("W", job_of(BUILD, W=2 * P + 1)), ("x", job_of(ROWS, x=3 * P + 2)),
    ("g_y", job_of(ROWS, g_y=4 * P + 2)), ("g_x", job_of(ROWS, g_x=5 * P + 2)), ("g_W", job_of(FINISH, g_W=6 * P + 2)),
    ("g_V", job_of(FINISH, g_V=7 * P + 2)), ("workspace", job_of(ROWS, workspace=WS + 8)),
    # strides smaller than one item
    ("vs_stride", job_of(BUILD, vs_stride=N * D - 1)), ("w_stride", job_of(BUILD, w_stride=D * D - 1)),
    ("w_stride", job_of(ROWS, w_stride=0)), ("gv_stride", job_of(FINISH, gv_stride=N * D - 1)),
    ("gw_stride", job_of(FINISH, gw_stride=D * D - 1)), ("ws_stride", job_of(ROWS, ws_stride=slot_bytes() // 4 - 4)),
    ("ws_stride", job_of(FINISH, ws_stride=slot_bytes() // 4 + 1)), ("vs_stride", job_of(BUILD, vs_stride=(1 << 30) + 1)),
    # a workspace smaller than workspace_bytes says
    ("workspace_bytes", job_of(ROWS, workspace_bytes=M * slot_bytes() - 1)),
    ("workspace_bytes", job_of(FINISH, workspace_bytes=M * slot_bytes() - 1)),
    ("workspace_bytes", job_of(FINISH, ws_stride=slot_bytes() // 4 + 4)),           # wider slots need a larger workspace
    # g_x aliasing g_y
    ("g_x aliases g_y", job_of(ROWS, g_x=4 * P)), ("g_x aliases g_y", job_of(ROWS, g_x=4 * P + B * D * 4 - 4)),
]


@pytest.mark.parametrize("i", range(len(REJECT)))
def test_run_rejects_before_any_device_call(i):
    lib = _lib.load()
    field, job = REJECT[i]
    assert lib.hint_householder_many_run(C.byref(job)) != 0
    msg = lib.hint_last_error().decode()
    assert msg.startswith(WHO) and re.search(r"\b%s\b" % re.escape(field), msg[len(WHO):]), msg


def test_null_job():
    lib = _lib.load()
    assert lib.hint_householder_many_run(None) != 0
    msg = lib.hint_last_error().decode()
    assert msg.startswith(WHO) and re.search(r"\bjob\b", msg[len(WHO):]), msg


def test_workspace_bytes_is_monotone_and_zero_on_refused_sizes():
    lib = _lib.load()
    size = lib.hint_householder_many_workspace_bytes
    for args, field in (((ROWS, 0, 32, 8, 8), "m"), ((ROWS, 65, 32, 8, 8), "m"), ((FINISH, 3, 0, 8, 8), "B"),
                        ((ROWS, 3, (1 << 22) + 1, 8, 8), "B"), ((ROWS, 3, 32, 129, 8), "d"), ((ROWS, 3, 32, 0, 8), "d"),
                        ((FINISH, 3, 32, 8, 0), "n"), ((FINISH, 3, 32, 8, 257), "n"), ((7, 3, 32, 8, 8), "op"),
                        ((BUILD, 65, 1, 8, 8), "m")):
        assert size(*args) == 0
        msg = lib.hint_last_error().decode()
        assert msg.startswith(SIZER + ": ") and re.search(r"\b%s\b" % field, msg), msg
    assert size(BUILD, 3, 1, 8, 8) == 0                       # build uses none
    for d in (2, 20, 128):
        slab = lib.hint_householder_geometry(1, d, 0)
        prev = 0
        for m in (1, 2, 3, 64):
            prev_b = 0
            for Bq in (1, 16, slab, slab + 1, 2 * slab + 5, 1 << 22):
                ws = size(ROWS, m, Bq, d, d)
                assert ws == size(FINISH, m, Bq, d, d) == m * lib.hint_householder_workspace_bytes(GRAD, Bq, d, d)
                assert ws >= prev_b and ws % 16 == 0 and (ws // m) % 16 == 0
                prev_b = ws
            assert prev_b >= prev                             # (at the largest B: never decreases with m)
            prev = prev_b
