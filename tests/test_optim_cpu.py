"""CPU-side checks of hint_amd.ClampAdam and the hint_adam_multi_* entry points (no GPU): header, exports and binding agree,
the argument checks of hint_adam_multi_create come before any device call, the class refuses what it cannot run, and the
host's coalescing / chunking of segments tiles every float exactly once."""
import ctypes as C
import os
import re

import pytest
import torch

import hint_amd
from hint_amd import _lib, optim
from hint_amd._lib import HintAmdError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hint_adam_multi_create", "hint_adam_multi_step", "hint_adam_multi_destroy")
BASE = 0x7F0000000000           # made-up addresses: the checks and the chunking never dereference a segment's pointers


def seg_array(segs):
    arr = (_lib.AdamSeg * max(len(segs), 1))()
    for i, (p, g, m, v, n) in enumerate(segs):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n = p, g, m, v, n
    return arr


def create(segs, n=None):
    lib = _lib.load()
    h = C.c_void_p()
    st = lib.hint_adam_multi_create(seg_array(segs), len(segs) if n is None else n, C.byref(h))
    return st, h, (lib.hint_last_error() or b"").decode()


def test_new_symbols_declared_exported_and_bound_abi_still_8():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    declared = set(re.findall(r"\b(hint_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert "#define HINT_AMD_ABI_VERSION 8" in header
    assert lib.hint_abi_version() == _lib.ABI_VERSION == 8
    assert C.sizeof(_lib.AdamSeg) == 4 * 8 + 8
    assert hint_amd.ClampAdam is optim.ClampAdam
    assert issubclass(hint_amd.ClampAdam, torch.optim.Optimizer)


def test_create_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    ok = (BASE, BASE + (1 << 20), BASE + (2 << 20), BASE + (3 << 20), 100)
    st = lib.hint_adam_multi_create(seg_array([ok]), 1, None)
    assert st != 0 and "null" in lib.hint_last_error().decode()
    st = lib.hint_adam_multi_create(None, 1, C.byref(C.c_void_p()))
    assert st != 0 and "null" in lib.hint_last_error().decode()
    for k in range(4):                                  # each of p, g, m, v null
        bad = list(ok)
        bad[k] = 0
        st, h, msg = create([ok[:4] + (0,), tuple(bad)])
        assert st != 0 and not h.value and "segment 1" in msg and "null" in msg, msg
    st, h, msg = create([ok[:4] + (-1,)])
    assert st != 0 and not h.value and "negative" in msg, msg
    st, h, msg = create([(BASE + 2,) + ok[1:]])
    assert st != 0 and "aligned" in msg, msg
    # p ranges [BASE, BASE + 400) and [BASE + 396, ...) share one float; g, m, v are apart
    other = (BASE + 396, BASE + (5 << 20), BASE + (6 << 20), BASE + (7 << 20), 10)
    st, h, msg = create([ok, other])
    assert st != 0 and not h.value and "overlap" in msg and "0" in msg and "1" in msg, msg
    st, h, msg = create([other, ok])                    # ... in either order
    assert st != 0 and "overlap" in msg, msg
    st, h, msg = create([ok], n=-1)
    assert st != 0 and "n_segs" in msg, msg
    assert lib.hint_adam_multi_step(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0, 0, None) != 0
    assert "null" in lib.hint_last_error().decode()
    lib.hint_adam_multi_destroy(None)                   # a no-op


def test_empty_table_is_a_valid_handle_whose_step_does_nothing():
    lib = _lib.load()
    for segs in ([], [(BASE, BASE + 64, BASE + 128, BASE + 192, 0)]):      # no segment; one of no floats
        st, h, msg = create(segs)
        assert st == 0 and h.value, msg
        assert lib.hint_adam_multi_step(h, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0, 0, None) == 0
        assert lib.hint_adam_multi_step(h, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0, 0, None) != 0      # steps are 1-based
        lib.hint_adam_multi_destroy(h)


def test_clampadam_refuses_what_it_cannot_run():
    w = torch.nn.Parameter(torch.zeros(3, 4))
    with pytest.raises(HintAmdError, match=r"parameter 0 of param group 0 \(shape \(3, 4\)\).*cpu"):
        hint_amd.ClampAdam([w])
    w64 = torch.nn.Parameter(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(HintAmdError, match=r"parameter 0 of param group 1 \(shape \(5,\)\)"):
        hint_amd.ClampAdam([{"params": []}, {"params": [w64]}])
    for kw in ("amsgrad", "capturable", "maximize"):
        with pytest.raises(HintAmdError, match=kw):
            hint_amd.ClampAdam([w], **{kw: True})
    with pytest.raises(ValueError):
        hint_amd.ClampAdam([w], lr=-1.0)


def test_coalescing_merges_adjacent_runs_and_splits_on_gap_or_misalignment():
    P, G, M, V = BASE, BASE + (1 << 20), BASE + (2 << 20), BASE + (3 << 20)
    run = [(P, G, M, V, 8), (P + 32, G + 32, M + 32, V + 32, 5), (P + 52, G + 52, M + 52, V + 52, 3)]
    assert optim.coalesce_segments(run) == [(P, G, M, V, 16)]
    assert optim.coalesce_segments([]) == []
    gap = [(P, G, M, V, 8), (P + 48, G + 48, M + 48, V + 48, 4)]                    # 4 floats of padding in all four
    assert optim.coalesce_segments(gap) == gap
    for k in range(4):                                                              # one array does not continue
        nxt = [P + 32, G + 32, M + 32, V + 32]
        nxt[k] += 4
        segs = [(P, G, M, V, 8), tuple(nxt) + (4,)]
        assert optim.coalesce_segments(segs) == segs, k
    # empty parameters vanish and do not break a run
    assert optim.coalesce_segments([(P, G, M, V, 8), (P + 32, G + 32, M + 32, V + 32, 0),
                                    (P + 32, G + 32, M + 32, V + 32, 8)]) == [(P, G, M, V, 16)]
    # a later run may continue an earlier one's addresses only if it follows it directly
    back = [(P + 32, G + 32, M + 32, V + 32, 8), (P, G, M, V, 8)]
    assert optim.coalesce_segments(back) == back


def test_moment_layout_keeps_alignment_and_distance():
    ptrs = [BASE, BASE + 4 * 20, BASE + 4 * 37, BASE + 4 * 40, BASE + (1 << 20) + 8, BASE + 4 * 1000]
    numels = [17, 17, 3, 100, 9, 6]
    offs, total = optim.layout_moments(ptrs, numels)
    assert offs[:4] == [0, 20, 37, 40]                          # an arena's tensors keep their distances (padding mirrored)
    spans = sorted((o, o + n) for o, n in zip(offs, numels))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    for ptr, off in zip(ptrs, offs):
        assert (4 * off) % 16 == ptr % 16                       # same address modulo 16 as the parameter (buffer base: 256)
    assert optim.layout_moments([], []) == ([], 0)


def test_chunks_tile_every_segment_exactly_once():
    P, G, M, V = BASE, BASE + (1 << 24), BASE + (2 << 24), BASE + (3 << 24)
    assert optim.chunk_segments([]) == []
    segs, cur = [], 0
    for n, off in [(0, 0), (1, 1), (3, 2), (4, 3), (5, 0), (1023, 1), (1024, 0), (1027, 3), (1028, 2), (70001, 1), (4099, 0)]:
        cur = (cur + 3) // 4 * 4 + 64 + off
        segs.append((P + 4 * cur, G + 4 * cur, M + 4 * cur, V + 4 * cur, n))
        cur += n
    # ... and two whose pointers disagree modulo 16
    cur = (cur + 3) // 4 * 4 + 64
    segs.append((P + 4 * cur, G + 4 * cur + 4, M + 4 * cur, V + 4 * cur + 8, 5000))
    cur += 5008
    segs.append((P + 4 * cur + 12, G + 4 * cur, M + 4 * cur, V + 4 * cur, 2))
    chunks = optim.chunk_segments(segs)
    assert sum(c[2] for c in chunks) == sum(s[4] for s in segs)
    for si, s in enumerate(segs):
        mine = sorted((off, ln) for sg, off, ln in chunks if sg == si)
        pos = 0
        for off, ln in mine:                                    # consecutive: no hole, no overlap
            assert off == pos and 0 < ln <= 1024 + 3, (si, off, ln)
            pos += ln
        assert pos == s[4], si
        same = len({a % 16 for a in s[:4]}) == 1
        for off, ln in mine[1:]:                                # with a common alignment every later chunk starts on 16 bytes
            assert not same or (s[0] + 4 * off) % 16 == 0, (si, off)
        assert all(ln <= 1024 for off, ln in mine) or same
    assert all(0 <= sg < len(segs) for sg, _, _ in chunks)
    # the checks of create hold here too
    with pytest.raises(HintAmdError, match="overlap"):
        optim.chunk_segments([(P, G, M, V, 8), (P + 16, G + 64, M + 64, V + 64, 8)])
