"""Every C entry point that takes a non-const device pointer is run on poisoned, guard-banded memory by a named test
(tests/poison_cases.py ENTRY_TESTS), or is excluded there with a reason.  A new entry point with an output buffer fails here,
by name, until it has a poison test."""
import ast
import os
import re

from poison_cases import ENTRY_TESTS, EXCLUDED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hint_amd.h")
# pointer parameters that are not device buffers: the stream, and the library's opaque handles
NOT_BUFFERS = re.compile(r"^(void\s*\*\s*stream|(const\s+)?hint_(plan|chain|pack_group)\b.*)$")


def declarations():
    """{function name: [parameter declarations]} of every hint_* function the header declares"""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"#[^\n]*", " ", src)
    out = {}
    for m in re.finditer(r"\b[\w\s\*]*?\b(hint_\w+)\s*\(([^;{]*?)\)\s*;", src):
        out[m.group(1)] = [p.strip() for p in m.group(2).replace("\n", " ").split(",") if p.strip() and p.strip() != "void"]
    return out


def writable_device_pointers(params):
    """the parameters that are non-const pointers to data (not a stream, not a handle)"""
    out = []
    for p in params:
        p = " ".join(p.split())
        if "*" not in p or NOT_BUFFERS.match(p):
            continue
        # const T* (pointee const) is an input; T* const* and T* are writable
        if re.match(r"^const\b", p) and p.count("*") == 1:
            continue
        out.append(p)
    return out


def test_header_parses():
    decls = declarations()
    assert len(decls) >= 40, sorted(decls)
    assert "hint_chain_backward_adam" in decls and len(decls["hint_chain_backward_adam"]) == 21


def test_every_writing_entry_point_has_a_poison_test():
    decls = declarations()
    need = sorted(n for n, ps in decls.items() if writable_device_pointers(ps))
    missing = [n for n in need if n not in ENTRY_TESTS and n not in EXCLUDED]
    assert not missing, f"entry points with a non-const device pointer and no poison test in tests/poison_cases.py: {missing}"
    stale = sorted(n for n in list(ENTRY_TESTS) + list(EXCLUDED) if n not in decls)
    assert not stale, f"tests/poison_cases.py names functions the header does not declare: {stale}"
    both = sorted(set(ENTRY_TESTS) & set(EXCLUDED))
    assert not both, f"both tested and excluded: {both}"
    assert all(r.strip() for r in EXCLUDED.values())


def test_named_tests_exist():
    """every ENTRY_TESTS target is a test function of tests/test_gpu_poison.py"""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_poison.py")).read())
    defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for fn, test in ENTRY_TESTS.items():
        path, name = test.split("::")
        assert path == "tests/test_gpu_poison.py" and name in defined, f"{fn}: {test} does not exist"
