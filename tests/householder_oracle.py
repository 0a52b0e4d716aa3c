"""The test-side statement of the Householder permutation (hint_amd.HouseholderPerm, hint_householder_run), in float64 torch.

    Vs [n, d], row i the vector v_i;   H_i = I - 2 v_i v_i^T / (v_i . v_i);   W = H_0 H_1 .. H_(n-1);   y = x W  (rev: y = x W^T)

FrEIA is not available, so this is the library's own definition written a second time, as plainly as possible: the matrices H_i
are formed and multiplied.  Gradients come from torch autograd on that statement; `g_V_recurrence` is the closed form the
kernel's header states, kept here so that a CPU test holds it against autograd before any kernel is trusted with it.
"""
import torch

F64 = torch.float64


def W(Vs):
    """W(V) by the definition: the product of the n reflection matrices, in float64 (differentiable)"""
    V = Vs.to(F64)
    n, d = V.shape
    out = torch.eye(d, dtype=F64, device=V.device)
    for i in range(n):
        v = V[i]
        out = out @ (torch.eye(d, dtype=F64, device=V.device) - 2.0 * torch.outer(v, v) / torch.dot(v, v))
    return out


def apply(x, Vs, rev=False, W_=None):
    M = W(Vs) if W_ is None else W_.to(F64)
    return x.to(F64) @ (M.t() if rev else M)


def grads(x, Vs, g_y, rev=False):
    """-> (g_x, g_W, g_V) of L = sum(g_y * y), y = x W(V) or x W(V)^T, by autograd in float64"""
    x64 = x.detach().to(F64).clone().requires_grad_(True)
    V64 = Vs.detach().to(F64).clone().requires_grad_(True)
    M = W(V64)
    M.retain_grad()
    y = x64 @ (M.t() if rev else M)
    (y * g_y.to(F64)).sum().backward()
    return x64.grad, M.grad, V64.grad


def g_V_from_g_W(Vs, G):
    """the chain rule dL/dW -> dL/dVs by autograd in float64"""
    V64 = Vs.detach().to(F64).clone().requires_grad_(True)
    (W(V64) * G.to(F64)).sum().backward()
    return V64.grad


def g_V_recurrence(Vs, G):
    """dL/dVs from G = dL/dW by the closed form: walking i = n-1 .. 0 with P = H_0 .. H_(i-1) and Gs = G (H_(i+1) .. H_(n-1))^T,
    a = P v_i, b = Gs v_i, q = P^T b, qt = Gs^T a, s = v_i . v_i,  g_(v_i) = -(2 / s)(q + qt) + (4 (a . b) / s^2) v_i"""
    V = Vs.detach().to(F64)
    n, d = V.shape
    eye = torch.eye(d, dtype=F64)
    H = lambda i: eye - 2.0 * torch.outer(V[i], V[i]) / torch.dot(V[i], V[i])
    P = W(V) @ H(n - 1)
    Gs = G.to(F64).clone()
    out = torch.empty_like(V)
    for i in range(n - 1, -1, -1):
        v = V[i]
        s = torch.dot(v, v)
        a, b = P @ v, Gs @ v
        q, qt = P.t() @ b, Gs.t() @ a
        out[i] = -(2.0 / s) * (q + qt) + (4.0 * torch.dot(a, b) / (s * s)) * v
        Gs = Gs @ H(i)
        if i > 0:
            P = P @ H(i - 1)
    return out


def abs_products(a, b):
    """|a| . |b| in float64: the magnitude a rounding-error bound of the product a . b is stated in"""
    return a.to(F64).abs() @ b.to(F64).abs()


def init_Vs(n, d, seed):
    """the module's initialisation: 0.2 randn(n, d) + eye(n, d) from a generator seeded by `seed`"""
    g = torch.Generator().manual_seed(seed)
    return (0.2 * torch.randn(n, d, generator=g) + torch.eye(n, d)).to(torch.float32)
