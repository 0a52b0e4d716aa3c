"""CPU tests of the Householder permutation: the test-side statement against itself (tests/householder_oracle.py), the
descriptor's layout, every rejection of hint_householder_run (they come before any device call), the slab geometry, and the
module contract of hint_amd.HouseholderPerm and the flows' learned_perms switch."""
import ctypes as C
import os
import re

import pytest
import torch

import hint_amd
from hint_amd import _lib
from hint_amd._lib import HintAmdError
import householder_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD, APPLY, GRAD = 0, 1, 2


# ---- the statement ----
@pytest.mark.parametrize("n,d", [(3, 7), (7, 7), (10, 7), (1, 1), (2, 20)])
def test_statement_is_orthogonal_and_the_recurrence_equals_autograd(n, d):
    torch.manual_seed(n * 100 + d)
    Vs = ho.init_Vs(n, d, seed=n + d).double() + 0.1 * torch.randn(n, d, dtype=torch.float64)
    Wm = ho.W(Vs)
    assert float((Wm @ Wm.t() - torch.eye(d, dtype=torch.float64)).abs().max()) < 1e-12
    G = torch.randn(d, d, dtype=torch.float64)
    want = ho.g_V_from_g_W(Vs, G)
    got = ho.g_V_recurrence(Vs, G)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
    # the three gradients of one product, against the chain rule through g_W
    x, gy = torch.randn(5, d, dtype=torch.float64), torch.randn(5, d, dtype=torch.float64)
    for rev in (False, True):
        gx, gW, gV = ho.grads(x, Vs, gy, rev)
        assert torch.allclose(gW, (gy.t() @ x) if rev else (x.t() @ gy), rtol=0, atol=1e-12)
        assert torch.allclose(gx, gy @ (Wm if rev else Wm.t()), rtol=0, atol=1e-12)
        assert float((ho.g_V_recurrence(Vs, gW) - gV).abs().max()) <= 1e-10 * float(gV.abs().max())


def test_abs_products():
    a, b = torch.tensor([[1.0, -2.0]]), torch.tensor([[-3.0], [4.0]])
    assert ho.abs_products(a, b).item() == 11.0 and ho.abs_products(a, b).dtype == torch.float64


# ---- the descriptor ----
_CTYPES = {"int32_t": C.c_int32, "size_t": C.c_size_t}


def header_fields():
    src = open(os.path.join(ROOT, "include", "hint_amd.h")).read()
    body = re.search(r"typedef struct hint_householder_desc \{(.*?)\} hint_householder_desc;", src, re.S).group(1)
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


def test_descriptor_mirrors_the_header():
    fields = header_fields()
    assert [f for f, _ in fields] == [f for f, _ in _lib.HouseholderDesc._fields_]
    twin = type("Twin", (C.Structure,), {"_fields_": fields})
    assert C.sizeof(twin) == C.sizeof(_lib.HouseholderDesc)
    for (name, _), (_, ct) in zip(fields, _lib.HouseholderDesc._fields_):
        assert getattr(twin, name).offset == getattr(_lib.HouseholderDesc, name).offset, name
        assert C.sizeof(ct) == getattr(twin, name).size, name


# ---- rejections ----
P = 0x10000                      # a plausible, aligned device address: no rejected run ever reads it
WS = 0x200000


def desc_of(kind, **kw):
    d = _lib.HouseholderDesc()
    op = kind
    d.op, d.transpose, d.B, d.d, d.n = op, 0, 32, 8, 8
    if op == BUILD:
        d.Vs, d.W = P, 2 * P
    elif op == APPLY:
        d.x, d.W, d.y = P, 2 * P, 3 * P
    else:
        d.x, d.W, d.g_y, d.Vs = P, 2 * P, 3 * P, 4 * P
        d.g_x, d.g_W, d.g_V = 5 * P, 6 * P, 7 * P
        d.workspace = WS
        d.workspace_bytes = _lib.load().hint_householder_workspace_bytes(GRAD, 32, 8, 8)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECT = [
    ("op", desc_of(BUILD, op=3)), ("op", desc_of(BUILD, op=-1)),
    ("d", desc_of(BUILD, d=0)), ("d", desc_of(APPLY, d=129)), ("n", desc_of(BUILD, n=0)), ("n", desc_of(GRAD, n=257)),
    ("B", desc_of(APPLY, B=0)), ("B", desc_of(GRAD, B=(1 << 22) + 1)),
    ("Vs", desc_of(BUILD, Vs=None)), ("W", desc_of(BUILD, W=None)),
    ("x", desc_of(APPLY, x=None)), ("W", desc_of(APPLY, W=None)), ("y", desc_of(APPLY, y=None)),
    ("g_y", desc_of(GRAD, g_y=None)), ("W", desc_of(GRAD, W=None)),
    ("x", desc_of(GRAD, x=None, g_x=None, g_V=None)), ("x", desc_of(GRAD, x=None, g_x=None, g_W=None)),
    ("Vs", desc_of(GRAD, Vs=None)),
    ("g_x", desc_of(GRAD, g_x=None, g_W=None, g_V=None)),
    ("Vs", desc_of(BUILD, Vs=P + 2)), ("W", desc_of(BUILD, W=P + 1)), ("x", desc_of(APPLY, x=P + 2)), ("y", desc_of(APPLY, y=3 * P + 2)),
    ("g_y", desc_of(GRAD, g_y=3 * P + 2)), ("g_x", desc_of(GRAD, g_x=5 * P + 2)), ("g_W", desc_of(GRAD, g_W=6 * P + 2)),
    ("g_V", desc_of(GRAD, g_V=7 * P + 2)),
    ("workspace", desc_of(GRAD, workspace=WS + 8)), ("workspace", desc_of(GRAD, workspace=None)),
    ("workspace_bytes", desc_of(GRAD, workspace_bytes=desc_of(GRAD).workspace_bytes - 1)),
    ("y aliases x", desc_of(APPLY, y=P)), ("y aliases x", desc_of(APPLY, y=P + 32 * 8 * 4 - 4)),
]


@pytest.mark.parametrize("i", range(len(REJECT)))
def test_run_rejects_before_any_device_call(i):
    lib = _lib.load()
    field, d = REJECT[i]
    assert lib.hint_householder_run(C.byref(d)) != 0
    msg = lib.hint_last_error().decode()
    assert msg.startswith("hint_householder_run: ") and re.search(r"\b%s\b" % re.escape(field), msg[22:]), msg


def test_null_desc_and_bad_workspace_sizes():
    lib = _lib.load()
    assert lib.hint_householder_run(None) != 0
    assert "desc" in lib.hint_last_error().decode()
    for args, field in (((GRAD, 0, 8, 8), "B"), ((GRAD, 32, 129, 8), "d"), ((GRAD, 32, 8, 0), "n"), ((7, 32, 8, 8), "op")):
        assert lib.hint_householder_workspace_bytes(*args) == 0
        assert field in lib.hint_last_error().decode()
    assert lib.hint_householder_workspace_bytes(GRAD, 1, 1, 1) > 0
    assert lib.hint_householder_geometry(0, 8, 0) == -1 and lib.hint_householder_geometry(16, 8, 9) == -1


@pytest.mark.parametrize("d", [2, 20, 128])
def test_geometry_covers_every_row_once(d):
    lib = _lib.load()
    slab = lib.hint_householder_geometry(1, d, 0)
    prev_slabs, prev_ws = 0, 0
    for B in (1, 16, slab, slab + 1, 2 * slab + 5, 1 << 22):
        R, slabs, nt = (lib.hint_householder_geometry(B, d, f) for f in (0, 1, 2))
        assert R >= 16 and R % 16 == 0 and nt == (d + 15) // 16
        # slab s holds rows [s R, min((s + 1) R, B)): together every row exactly once, none empty
        assert (slabs - 1) * R < B <= slabs * R
        assert slabs >= prev_slabs
        ws = lib.hint_householder_workspace_bytes(GRAD, B, d, d)
        assert ws >= prev_ws and ws >= 4 * slabs * nt * nt * 256 + 16 * d * d
        prev_slabs, prev_ws = slabs, ws
    assert lib.hint_householder_geometry(slab, d, 1) == 1 and lib.hint_householder_geometry(slab + 1, d, 1) == 2


# ---- the module ----
def test_module_contract():
    m = hint_amd.HouseholderPerm([(7,)], n_reflections=3, seed=5)
    assert list(m.state_dict().keys()) == ["Vs"] and m.state_dict()["Vs"].shape == (3, 7)
    assert m.Vs.requires_grad and m.Vs.dtype == torch.float32
    assert torch.equal(m.Vs.detach(), ho.init_Vs(3, 7, 5))
    f = hint_amd.HouseholderPerm([(7,)], fixed=True, seed=5)
    assert not f.Vs.requires_grad and list(f.state_dict().keys()) == ["Vs"] and f.Vs.shape == (7, 7)
    assert m.jacobian(None) == 0.0 and m.output_dims([(7,)]) == [(7,)]
    torch.manual_seed(3)
    a = hint_amd.HouseholderPerm([(4,)]).Vs.detach().clone()
    torch.manual_seed(3)
    assert torch.equal(a, 0.2 * torch.randn(4, 4) + torch.eye(4, 4))       # seed=None: the global generator
    for bad in (dict(dims_in=[(0,)]), dict(dims_in=[(129,)]), dict(dims_in=[(8,)], n_reflections=0),
                dict(dims_in=[(8,)], n_reflections=257), dict(dims_in=[(8,)], dims_c=[(2,)])):
        with pytest.raises(HintAmdError):
            hint_amd.HouseholderPerm(**bad)
    with pytest.raises(HintAmdError):
        m([torch.randn(4, 7)])                       # CPU input: there is no fallback
    with pytest.raises(HintAmdError):
        m.matrix()
    with pytest.raises(HintAmdError):
        m([torch.randn(4, 7)], c=[torch.randn(4, 2)])


def test_flows_take_learned_perms_and_defaults_are_unchanged():
    flow = hint_amd.HintFlow(20, 2, [32, 16], learned_perms=True)
    assert isinstance(flow.perms[1], hint_amd.HouseholderPerm) and isinstance(flow.perms[0], torch.nn.Identity)
    assert flow.perms[1].Vs.shape == (20, 20) and flow.perms[1].Vs.requires_grad
    assert flow.has_perm(1) and not flow.has_perm(0)
    assert "perms.1.Vs" in flow.state_dict() and "perms.1.Vs" in dict(flow.named_parameters())
    first = hint_amd.HintFlow(6, 2, [16], learned_perms=True, perm_first=True)
    assert all(isinstance(p, hint_amd.HouseholderPerm) for p in first.perms)
    plain = hint_amd.HintFlow(20, 2, [32, 16])
    assert isinstance(plain.perms[1], hint_amd.FixedOrthogonal) and isinstance(plain.perms[0], torch.nn.Identity)
    assert torch.equal(plain.perms[1].W, hint_amd.flow.random_orthogonal(20, 2))
    assert sorted(k for k in plain.state_dict() if k.startswith("perms")) == ["perms.1.W"]
    cond = hint_amd.ConditionalHintFlow(20, 2, 2, 32, learned_perms=True)
    assert isinstance(cond.perm_x[1], hint_amd.HouseholderPerm) and cond.perm_x[1].Vs.shape == (20, 20)
    assert isinstance(cond.perm_y[1], hint_amd.HouseholderPerm) and cond.perm_y[1].Vs.shape == (2, 2)
    assert isinstance(cond.perm_x[0], torch.nn.Identity) and isinstance(cond.perm_y[0], torch.nn.Identity)
    cplain = hint_amd.ConditionalHintFlow(20, 2, 2, 32)
    assert isinstance(cplain.perm_x[1], hint_amd.FixedOrthogonal) and isinstance(cplain.perm_y[1], hint_amd.FixedOrthogonal)
    assert torch.equal(cplain.perm_y[1].W, hint_amd.flow.random_orthogonal(2, 3))
    assert torch.equal(cplain.perm_x[1].W, hint_amd.flow.random_orthogonal(20, 4))
