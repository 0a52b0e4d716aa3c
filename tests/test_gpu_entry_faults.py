"""Calls the host refuses before any launch: every chain entry point and the block entry points with checks of their own, each with
the message hint_last_error() gave when tests/golden/launch_bits.json was recorded ("faults"; tests/golden/make_launch_bits.py).
The entry points share one check routine (hint_amd/csrc/hint_chain.cpp); the table pins each one's own name inside the message,
which fault a call with two of them reports, and where the entry points differ.  Every call returns non-zero and leaves the buffers
it was handed as they were.

Two rigs of tests/test_gpu_call_forms.py at B = 37: three blocks of the smallest wave-local family (wl1) and of a family with a
condition (n3c).  Per rig: a committed training chain (`ok`), the same never committed (`raw`), one whose blocks have inputs of
their own (`gathered`) and an inference chain - no tape, no workspace (`infer`)."""
import ctypes as C
import json

import pytest
import torch

from hint_amd import _lib
import call_forms as cf
from poison_cases import check, stream
from test_gpu_call_forms import BITS_PATH, DEV, NB, Rig

pytestmark = pytest.mark.gpu
B = 37
ADAM = (0.9, 0.95, 1e-4, 0.0, 1.0, 0.0)        # beta1, beta2, eps, weight_decay, grad_scale, grad_clamp


class Faults:
    def __init__(self, lib, fam_name):
        self.lib, self.fam = lib, cf.FAMILY[fam_name]
        rig = self.rig = Rig(self.fam, lib, B)
        d, dc, n = self.fam.d, self.fam.dc, NB * rig.total
        g = torch.Generator().manual_seed(1)
        R = lambda *s: torch.randn(*s, generator=g).to(DEV)                            # noqa: E731
        self.x, self.gz, self.c = R(B, d), R(B, d), (R(B, dc) if dc else None)
        # what a launch would write: checked after every refused call
        self.outs = dict(z=R(B, d), J=R(B), gx=R(B, d), gc=R(B, max(dc, 1)), x_noisy=R(B, d), M=R(n + 4), V=R(n + 4))
        rig.G.copy_(R(n))
        self.outs.update(G=rig.G, arena=rig.arena)
        self.snap = {k: v.clone() for k, v in self.outs.items()}
        self.state = torch.tensor([0.0, 0.0, 0.95, 0.0, 1.0], device=DEV)
        none = [(None, None, None)] * NB
        self.chains = dict(ok=rig.chain([None] * NB, none), raw=self.chain(commit=False), infer=self.chain(train=False),
                           gathered=rig.chain([None] * NB, [(self.x, self.c, None)] * NB))

    def chain(self, commit=True, train=True):
        rig, lib, h = self.rig, self.lib, C.c_void_p()
        check(lib.hint_chain_create(rig.plan, NB, B, C.byref(h)), "hint_chain_create")
        for i in range(NB):
            t = (rig.tapes[i].data_ptr(), rig.wss[i].data_ptr(), rig.ws_bytes, rig.gps[i].data_ptr()) if train else (None, None, 0, None)
            check(lib.hint_chain_set_block(h, i, rig.params[i].data_ptr(), rig.packed[i].data_ptr(), None, *t), "hint_chain_set_block")
        if commit:
            check(lib.hint_chain_commit(h), "hint_chain_commit")
        return h

    def close(self):
        for h in self.chains.values():
            self.lib.hint_chain_destroy(h)

    def call(self, name):
        """the table's call `name`: its status and the message"""
        entry, chain, kw = CALLS[name][1:]
        st = getattr(self, entry)(self.chains[chain], **kw)
        msg = self.lib.hint_last_error().decode()
        torch.cuda.synchronize()
        for k, v in self.outs.items():
            assert torch.equal(v, self.snap[k]), f"{name}: refused, but {k} was written"
        return st, msg

    # ---- the entry points, every argument valid unless a call of the table says otherwise
    def p(self, t, kw, key):
        """the pointer of t, NULL where the call asks for it (`key=None`), or moved by `key` bytes"""
        v = kw.get(key, 0)
        return None if v is None or t is None else t.data_ptr() + v

    def forward(self, h, **kw):
        o = self.outs
        return self.lib.hint_chain_forward(h, self.p(self.x, kw, "x"), self.p(self.c, kw, "c"), o["z"].data_ptr(), o["J"].data_ptr(), None, None,
                                           stream())

    def inverse(self, h, **kw):
        o = self.outs
        return self.lib.hint_chain_inverse(h, self.p(self.x, kw, "x"), self.p(self.c, kw, "c"), o["z"].data_ptr(), o["J"].data_ptr(), None, stream())

    def rows(self, kw):
        o = self.outs
        return (self.p(self.x, kw, "x"), self.p(self.c, kw, "c"), self.p(self.gz, kw, "gz"), None, o["gx"].data_ptr(),
                o["gc"].data_ptr() if self.fam.dc else None, 1.0, 0.0)

    def arenas(self, kw):
        o, n = self.outs, NB * self.rig.total
        return (self.p(o["arena"], kw, "arena"), self.p(o["M"], kw, "M"), o["V"].data_ptr(), n - kw.get("short", 0), self.state.data_ptr(), *ADAM)

    def parts(self, h, parts=3, **kw):
        return self.lib.hint_chain_backward_parts(h, *self.rows(kw), 0, parts, stream())

    def wgrad_range(self, h, begin=0, end=NB, **kw):
        return self.lib.hint_chain_wgrad_range(h, self.p(self.x, kw, "x"), self.p(self.c, kw, "c"), 0, begin, end, stream())

    def backward_adam(self, h, **kw):
        return self.lib.hint_chain_backward_adam(h, *self.rows(kw), *self.arenas(kw), stream())

    def wgrad_adam(self, h, **kw):
        return self.lib.hint_chain_wgrad_adam(h, self.p(self.x, kw, "x"), self.p(self.c, kw, "c"), *self.arenas(kw), stream())

    def block_backward_ex(self, h, ws=0, less=0, **kw):
        rig, o = self.rig, self.outs
        return self.lib.hint_block_backward_ex(rig.plan, rig.params[0].data_ptr(), rig.packed[0].data_ptr(), self.x.data_ptr(), rig.tapes[0].data_ptr(),
                                               self.p(self.c, kw, "c"), self.gz.data_ptr(), None, o["gx"].data_ptr(), None, rig.gps[0].data_ptr(), 0,
                                               rig.wss[0].data_ptr() + ws, rig.ws_bytes - less, None, 1.0, 0.0, B, stream())

    def block_forward_noisy(self, h, **kw):
        rig, o = self.rig, self.outs
        return self.lib.hint_block_forward_noisy(rig.plan, rig.params[0].data_ptr(), rig.packed[0].data_ptr(), self.x.data_ptr(), self.p(self.c, kw, "c"),
                                                 o["z"].data_ptr(), o["J"].data_ptr(), None, None, None, None, 0.1, None, o["x_noisy"].data_ptr(), B,
                                                 stream())


# name -> (rig, entry point, chain, what differs from a valid call).  `x=None`: NULL; `arena=4`: the pointer moved by 4 bytes;
# `short=4`: n four floats short of the arena
W, CND = "wl1", "n3c"
CALLS = {}
for _e in ("forward", "inverse", "parts", "wgrad_range", "backward_adam", "wgrad_adam"):
    CALLS[f"{_e}: not committed"] = (W, _e, "raw", {})
    CALLS[f"{_e}: dc > 0 and no c"] = (CND, _e, "ok", dict(c=None))
for _e in ("forward", "inverse"):
    CALLS[f"{_e}: gathered chain"] = (W, _e, "gathered", {})
for _e in ("parts", "wgrad_range", "backward_adam", "wgrad_adam"):
    CALLS[f"{_e}: blocks without workspace"] = (W, _e, "infer", {})
    CALLS[f"{_e}: x NULL without a permutation"] = (W, _e, "ok", dict(x=None))
for _e in ("backward_adam", "wgrad_adam"):
    CALLS[f"{_e}: misaligned arena"] = (W, _e, "ok", dict(arena=4))
    CALLS[f"{_e}: misaligned exp_avg"] = (W, _e, "ok", dict(M=4))
    CALLS[f"{_e}: arena ends inside the last block"] = (W, _e, "ok", dict(short=4))
    CALLS[f"{_e}: arena begins behind block 0"] = (W, _e, "ok", dict(arena=16))
CALLS.update({
    "parts: gathered chain, parts 1": (W, "parts", "gathered", dict(parts=1)),
    "parts: parts 0": (W, "parts", "ok", dict(parts=0)),
    "parts: parts 4": (W, "parts", "ok", dict(parts=4)),
    "parts: g_z NULL": (W, "parts", "ok", dict(gz=None)),
    "backward_adam: g_z NULL": (W, "backward_adam", "ok", dict(gz=None)),
    "backward_adam: gathered chain": (CND, "backward_adam", "gathered", dict(c=None)),     # (reads neither x_in nor c_in: c is what it misses)
    "wgrad_range: empty range": (W, "wgrad_range", "ok", dict(begin=1, end=1)),
    "wgrad_range: end past the chain": (W, "wgrad_range", "ok", dict(begin=0, end=NB + 1)),
    "wgrad_range: negative begin": (W, "wgrad_range", "ok", dict(begin=-1, end=2)),
    "block_backward_ex: workspace too small": (CND, "block_backward_ex", "ok", dict(less=4)),
    "block_backward_ex: workspace misaligned": (CND, "block_backward_ex", "ok", dict(ws=4)),
    "block_forward_noisy: noise without rng_state": (W, "block_forward_noisy", "ok", {}),
    # two faults in one call: which one is reported
    "two: parts 0 on a chain not committed": (W, "parts", "raw", dict(parts=0)),
    "two: parts, x NULL and blocks without workspace": (W, "parts", "infer", dict(x=None)),
    "two: wgrad_range, x NULL and blocks without workspace": (W, "wgrad_range", "infer", dict(x=None)),
    "two: backward_adam, x NULL and a misaligned arena": (W, "backward_adam", "ok", dict(x=None, arena=4)),
    "two: wgrad_adam, x NULL and a misaligned arena": (W, "wgrad_adam", "ok", dict(x=None, arena=4)),
    "two: wgrad_adam, no c and a misaligned arena": (CND, "wgrad_adam", "ok", dict(c=None, arena=4)),
    "two: backward_adam, no c and x NULL": (CND, "backward_adam", "ok", dict(c=None, x=None)),
})


@pytest.fixture(scope="module")
def rigs():
    r = {name: Faults(_lib.load(), name) for name in (W, CND)}
    yield r
    for f in r.values():
        f.close()


def record(lib):
    """{call: message} of the library in use (tests/golden/make_launch_bits.py)"""
    r = {name: Faults(lib, name) for name in (W, CND)}
    out = {}
    for name, (fam, _, _, _) in CALLS.items():
        st, msg = r[fam].call(name)
        assert st != 0 and msg, (name, st, msg)
        out[name] = msg
    for f in r.values():
        f.close()
    return out


@pytest.mark.parametrize("name", list(CALLS))
def test_a_refused_call_says_what_it_said_before(rigs, name):
    with open(BITS_PATH) as f:
        want = json.load(f)["faults"]
    assert set(want) == set(CALLS)
    st, msg = rigs[CALLS[name][0]].call(name)
    print(f"{name}: {st} {msg!r}")
    assert st != 0, name
    assert msg == want[name], (name, msg, want[name])
