"""Every C entry point that takes `void* stream` is run on a gated non-default stream by a named test of
tests/test_gpu_streams.py (tests/stream_cases.py STREAM_TESTS), every Python route listed there names its test, and at most a
quarter of the routes may skip the still_closed() assertion (`host_sync`, with the line that synchronises).  A new entry point
with a stream parameter fails here, by name, until it has a stream test."""
import ast
import os
import re

from stream_cases import MAX_EXEMPT_SHARE, ROUTES, STREAM_TESTS
from test_poison_table_cpu import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_gpu_streams.py"


def takes_stream(params):
    return any(re.match(r"^void\s*\*\s*stream$", " ".join(p.split())) for p in params)


def defined_tests():
    tree = ast.parse(open(os.path.join(ROOT, FILE)).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_entry_point_with_a_stream_has_a_stream_test():
    decls = declarations()
    need = sorted(n for n, ps in decls.items() if takes_stream(ps))
    assert len(need) >= 35, need
    missing = [n for n in need if n not in STREAM_TESTS]
    assert not missing, f"entry points with a stream parameter and no stream test in tests/stream_cases.py: {missing}"
    stale = sorted(n for n in STREAM_TESTS if n not in decls)
    assert not stale, f"tests/stream_cases.py names functions the header does not declare: {stale}"
    no_stream = sorted(n for n in STREAM_TESTS if n in decls and not takes_stream(decls[n]))
    assert not no_stream, f"tests/stream_cases.py names functions without a stream parameter: {no_stream}"


def test_named_tests_exist():
    defined = defined_tests()
    for what, test in list(STREAM_TESTS.items()) + [(r, t) for r, (t, _) in ROUTES.items()]:
        path, name = test.split("::")
        assert path == FILE and name in defined, f"{what}: {test} does not exist"


def test_the_self_tests_come_first():
    """pytest runs a file's tests in the order of their definition: the canary and the seeded mistake are the first two"""
    tree = ast.parse(open(os.path.join(ROOT, FILE)).read())
    names = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")]
    assert names[0].startswith("test_00_canary") and names[1].startswith("test_01_seeded_mistake"), names[:2]


def test_exemptions_stay_within_the_cap_and_name_their_line():
    exempt = {r: why for r, (_, why) in ROUTES.items() if why is not None}
    assert len(exempt) <= MAX_EXEMPT_SHARE * len(ROUTES), f"{len(exempt)} of {len(ROUTES)} routes are exempt: {sorted(exempt)}"
    for r, why in exempt.items():
        m = re.search(r"(hint_amd/\w+\.py):(\d+)", why)
        assert m, f"{r}: host_sync must name the source line that synchronises ({why!r})"
        lines = open(os.path.join(ROOT, m.group(1))).read().split("\n")
        assert int(m.group(2)) <= len(lines), f"{r}: {m.group(0)} is past the end of the file"
        line = lines[int(m.group(2)) - 1]
        assert "synchronize()" in line or ".item()" in line, f"{r}: {m.group(0)} does not synchronise: {line.strip()!r}"
