"""A deterministic gate for stream tests (tests/test_gpu_streams.py): every call sequence runs on a side stream S while the
device side of one stream is held shut, so that "a dependency is missing" or "this went to another stream" becomes a wrong
result, and "this call blocks the host" a failed assertion, whatever the timing.

Gate(stream, ms).open() enqueues a bounded device-side delay on `stream` (torch.cuda._sleep, calibrated once per process; a
chain of matmuls where that helper is missing or does not delay) and records the event `released` behind it;
still_closed() is `not released.query()`.

run_case(name, make, S) runs one case.  make(fill, role) builds the case on the default stream (role "ref": for the default-
stream reference, e.g. on a twin module; "S": for the runs on S) - buffers filled with `fill`, the inputs' final contents in staging tensors, the live input buffers holding NAN_BITS - and returns a Seq.  The same Seq.call is
then run
  reference   on the default stream, un-gated, once per fill ("nan", "junk");
  warm-up     on S, un-gated (plans, level plans, pools, S's allocator blocks; its host time sets the gate's length: gate_ms);
  S-gated     gate on S, the live inputs refilled from staging on S behind it, the calls issued with S current, still_closed()
              asserted, S synchronised, every output compared bit for bit with the reference, guards checked.  Work that went to
              any other stream ran before the inputs existed or before its predecessors: it consumed the NaN pattern or a poisoned
              workspace, or its output was overwritten late;
  null-gated  gate on the default (null) stream, inputs in place, the calls issued with S current, S synchronised (never the
              device), still_closed() asserted, compare.  Work that went to the null stream, or to a stream that waits for it, runs
              after its successors or after S.synchronize(); a call that blocks on the null stream, or on the device, returns only
              when the gate has ended.
What neither variant sees: two streams running one object at the same time, and dependencies between streams none of which is
S or the null stream when both happen to be idle.

A Python route that synchronises by contract names the line in `host_sync`; it keeps every comparison and skips only the
still_closed() assertion.  C entry points never do."""
import time
from types import SimpleNamespace

import torch

from guarded import NAN_BITS

FACTOR, MIN_MS, MAX_MS, SPLIT_MS = 4.0, 20.0, 250.0, 60.0
FILLS = ("nan", "junk")                 # S-gated runs on the first, null-gated on the second
_delay = None                           # ("sleep", cycles per ms) | ("matmul", matmuls per ms, a, b)
RECORDS = []                            # (case, host_ms, device_ms, gate_ms, host_sync) of every case run in this process


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate():
    global _delay
    if _delay is not None:
        return _delay
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        n = 2_000_000
        sleep(1000)
        ms = min(_timed(lambda: sleep(n)) for _ in range(2))
        if ms >= 0.5:                                    # the helper delays: n cycles took ms
            _delay = ("sleep", n / ms)
            return _delay
    a = torch.randn(2048, 2048, device="cuda")
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    k = 20
    ms = min(_timed(lambda: [torch.mm(a, a, out=b) for _ in range(k)]) for _ in range(2))
    _delay = ("matmul", k / ms, a, b)
    return _delay


def delay(ms):
    """enqueue about `ms` milliseconds of device-side delay on the current stream; the host does not wait"""
    d = _calibrate()
    if d[0] == "sleep":
        torch.cuda._sleep(int(d[1] * ms))
    else:
        for _ in range(max(1, int(d[1] * ms))):
            torch.mm(d[2], d[2], out=d[3])


def gate_ms(host_ms, device_ms=0.0):
    """clamp(4 x host_ms, 20 ms, 250 ms), host_ms the wall time of the calls in the un-gated warm-up run.  The null-gated variant
    looks at the gate after S.synchronize(), that is after the sequence's own device time, so where that is the longer of the two
    (a fit of 400 serial steps is one launch of tens of milliseconds) it takes host_ms's place: a gate shorter than the work it
    has to outlast would fail a correct library.  The factor covers jitter; it is a harness parameter, not a tolerance"""
    return min(max(FACTOR * max(host_ms, device_ms), MIN_MS), MAX_MS)


class Gate:
    def __init__(self, stream, ms):
        _calibrate()
        self.stream, self.ms = stream, ms
        self.released = torch.cuda.Event()

    def open(self):
        with torch.cuda.stream(self.stream):
            delay(self.ms)
            self.released.record(self.stream)
        return self

    def still_closed(self):
        return not self.released.query()


class Seq(SimpleNamespace):
    """one built case.  call() -> {name: device tensor} issues the calls on the current stream and must not touch the host side of
    the device (no .cpu(), no .item()); late = [(live tensor, staging tensor)]; guards = [(name, Guarded)]; loose = names of
    outputs that are atomically accumulated sums (compared within 1e-6 relative, as the tests of those sums do); close()"""

    def __init__(self, call, late=(), guards=(), loose=(), close=None):
        super().__init__(call=call, late=list(late), guards=list(guards), loose=tuple(loose), close=close or (lambda: None))


def late_inputs(bufs):
    """bufs: [(Guarded or contiguous 4- or 8-byte tensor, values or None)] -> [(live, staging)]: the values wait in a staging tensor on the device, the live
    buffer (whose pointer the library gets) holds NAN_BITS until refill()"""
    out = []
    for g, values in bufs:
        live = g.words if hasattr(g, "words") else g.view(-1).view(torch.int32)
        if values is None:                               # what the buffer holds now
            values = live
        v = values.reshape(-1).to(live.device).contiguous().view(torch.int32)
        staging = v.clone()
        live[:v.numel()].fill_(NAN_BITS)
        out.append((live[:v.numel()], staging))
    return out


def refill(seq):
    """device-to-device copies on the current stream"""
    for live, staging in seq.late:
        live.copy_(staging, non_blocking=True)


def host(out):
    return {k: v.detach().cpu() for k, v in out.items() if v is not None}


def compare(name, got, ref, loose=()):
    """the harness's compare: every output bit for bit (atomically accumulated sums within 1e-6)"""
    assert got.keys() == ref.keys(), f"{name}: outputs {sorted(got)} != {sorted(ref)}"
    for k, r in ref.items():
        g = got[k]
        assert g.shape == r.shape and g.dtype == r.dtype, f"{name}: {k}: {g.shape} {g.dtype} != {r.shape} {r.dtype}"
        if k in loose:
            gd, rd = g.double(), r.double()
            assert bool(torch.isfinite(gd).all()) and float((gd - rd).abs().max()) <= 1e-6 * max(float(rd.abs().max()), 1e-30), \
                f"{name}: {k} (an accumulated sum) differs from the default-stream run"
            continue
        w = g.contiguous().reshape(-1).view(torch.uint8) != r.contiguous().reshape(-1).view(torch.uint8)
        bad = int(w.sum())
        assert bad == 0, f"{name}: {k} differs from the default-stream run in {bad} of {w.numel()} bytes"


def check_guards(name, seq):
    for k, g in seq.guards:
        g.check_guards(f"{name}: {k}")


def reference(name, make, fill):
    """the sequence on the default stream, un-gated"""
    seq = make(fill, "ref")
    refill(seq)
    out = seq.call()
    torch.cuda.synchronize()
    check_guards(f"{name} reference {fill}", seq)
    res = host(out)
    seq.close()
    return res


def warm_up(name, make, S):
    """the sequence on S, un-gated: -> (host milliseconds of its calls, device milliseconds from the first to the last, outputs)"""
    seq = make(FILLS[0], "S")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        refill(seq)
        e0.record(S)
        t0 = time.perf_counter()
        out = seq.call()
        host_ms = 1e3 * (time.perf_counter() - t0)
        e1.record(S)
    S.synchronize()
    res = host(out)
    torch.cuda.synchronize()
    seq.close()
    return host_ms, e0.elapsed_time(e1), res, seq.loose


def s_gated(name, make, S, ms, ref, host_sync=None):
    seq = make(FILLS[0], "S")
    torch.cuda.synchronize()
    gate = Gate(S, ms).open()
    with torch.cuda.stream(S):
        refill(seq)
        out = seq.call()
    closed = gate.still_closed()
    S.synchronize()
    torch.cuda.synchronize()
    try:
        compare(f"{name} S-gated", host(out), ref, seq.loose)
        check_guards(f"{name} S-gated", seq)
    finally:
        seq.close()
    assert closed or host_sync, (f"{name} S-gated: the gate ({ms:.0f} ms) had ended when the calls returned: a call blocked the host "
                                 "on the stream it was given")


def null_gated(name, make, S, ms, ref, host_sync=None):
    seq = make(FILLS[1], "S")
    refill(seq)
    torch.cuda.synchronize()
    gate = Gate(torch.cuda.default_stream(), ms).open()
    with torch.cuda.stream(S):
        out = seq.call()
    S.synchronize()
    closed = gate.still_closed()
    torch.cuda.synchronize()
    try:
        compare(f"{name} null-gated", host(out), ref, seq.loose)
        check_guards(f"{name} null-gated", seq)
    finally:
        seq.close()
    assert closed or host_sync, (f"{name} null-gated: the gate on the null stream ({ms:.0f} ms) had ended when S was synchronised: a "
                                 "call blocked on the null stream or on the device")


def run_case(name, make, S, host_sync=None, finite=True):
    """reference, warm-up, S-gated and null-gated runs of one case (see the module's docstring)"""
    refs = {fill: reference(name, make, fill) for fill in FILLS}
    for k, v in refs[FILLS[0]].items():
        if finite and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"{name}: reference output {k} is not finite"
    host_ms, device_ms, warm, loose = warm_up(name, make, S)
    compare(f"{name} un-gated on S", warm, refs[FILLS[0]], loose)
    assert host_ms <= SPLIT_MS or host_sync, f"{name}: {host_ms:.1f} ms of host time: split the case"
    ms = gate_ms(host_ms, device_ms)
    RECORDS.append((name, host_ms, device_ms, ms, host_sync))
    print(f"stream case {name}: host_ms {host_ms:.2f} device_ms {device_ms:.2f} gate_ms {ms:.0f}" + (f" host_sync: {host_sync}" if host_sync else ""))
    s_gated(name, make, S, ms, refs[FILLS[0]], host_sync=host_sync)
    null_gated(name, make, S, ms, refs[FILLS[1]], host_sync=host_sync)
