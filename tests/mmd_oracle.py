"""Test-side evaluations of the multi-kernel MMD (hint_amd.multi_mmd), written from the definition:

    k(D) = sum_k C_k^a_k ((C_k + D) / a_k)^(-a_k),   D = |u - v|^2
    MMD  = mean_ij k(D(x_i, x_j)) + mean_ij k(D(y_i, y_j)) - 2 mean_ij k(D(x_i, y_j))       (all pairs, the diagonal included)

mmd_terms64   float64, squared distances from explicit differences sum (u - v)^2: no Gram trick, nothing to cancel
gram_terms32  the formulation whose error sets the tolerance of the GPU tests: Gram products, norms from the Gram's diagonal,
              r_i + r_j - 2 g_ij clamped at 0, fp32 torch ops throughout
gram_terms64  the same in float64, for sizes where the explicit differences do not fit (N = 4000: the GPU test)
The fixtures' inputs (tests/golden/mmd_*.npz) are regenerated from their seeds by golden_inputs.
"""
import numpy as np
import torch

DEFAULT = ((0.5, 1), (0.2, 1), (0.2, 0.5))
OTHER = ((1, .5), (.2, .8), (.2, .4))
GOLDEN_CASES = [dict(name=f"n{n}_d{d}_{kn}", n=n, d=d, kernels=ks, seed=1000 + 37 * n + d)
                for n in (33, 133) for d in (5, 20) for kn, ks in (("default", DEFAULT), ("other", OTHER))]


def golden_inputs(case):
    """x ~ N(0, 1), y ~ 0.3 + 1.2 N(0, 1) (fp32), from the case's seed"""
    rs = np.random.RandomState(case["seed"])
    x = rs.standard_normal((case["n"], case["d"])).astype(np.float32)
    y = (0.3 + 1.2 * rs.standard_normal((case["n"], case["d"]))).astype(np.float32)
    return x, y


def checksum(arrays):
    return float(sum(np.abs(a.astype(np.float64)).sum() + (a.astype(np.float64) * np.arange(1, a.size + 1).reshape(a.shape)
                                                           ).sum() / a.size for a in arrays))


def kernel_sum(D, kernels):
    out = torch.zeros_like(D)
    for C, a in kernels:
        out = out + C ** a * ((C + D) / a) ** (-a)
    return out


def _mean_k_explicit(u, v, kernels, rows=256):
    total = 0.0
    for i in range(0, u.shape[0], rows):
        diff = u[i:i + rows, None, :] - v[None, :, :]
        total += float(kernel_sum((diff * diff).sum(-1), kernels).sum())
    return total / (u.shape[0] * v.shape[0])


def mmd_terms64(x, y, kernels=DEFAULT):
    """(MMD, mean XX, mean YY, mean XY) as Python floats; x, y: tensors or arrays of any float dtype, on any device"""
    x = torch.as_tensor(x).to(torch.float64)
    y = torch.as_tensor(y).to(torch.float64)
    xx, yy, xy = _mean_k_explicit(x, x, kernels), _mean_k_explicit(y, y, kernels), _mean_k_explicit(x, y, kernels)
    return xx + yy - 2.0 * xy, xx, yy, xy


def _gram_terms(x, y, kernels):
    gxx, gyy, gxy = x @ x.t(), y @ y.t(), x @ y.t()
    rx, ry = gxx.diag(), gyy.diag()
    dxx = (rx[:, None] + rx[None, :] - 2. * gxx).clamp(min=0)
    dyy = (ry[:, None] + ry[None, :] - 2. * gyy).clamp(min=0)
    dxy = (rx[:, None] + ry[None, :] - 2. * gxy).clamp(min=0)
    kxx, kyy, kxy = kernel_sum(dxx, kernels), kernel_sum(dyy, kernels), kernel_sum(dxy, kernels)
    xx, yy, xy = float(kxx.mean()), float(kyy.mean()), float(kxy.mean())
    # equal sizes: one mean over the combined matrix, as the formulation being measured takes it
    mmd = float((kxx + kyy - 2. * kxy).mean()) if x.shape[0] == y.shape[0] else xx + yy - 2.0 * xy
    return mmd, xx, yy, xy


def gram_terms32(x, y, kernels=DEFAULT):
    return _gram_terms(torch.as_tensor(x).to(torch.float32), torch.as_tensor(y).to(torch.float32), kernels)


def gram_terms64(x, y, kernels=DEFAULT):
    return _gram_terms(torch.as_tensor(x).to(torch.float64), torch.as_tensor(y).to(torch.float64), kernels)


def gram32_error_bound(x, y, kernels=DEFAULT):
    """a first-order worst-case bound, in float64 from the inputs alone, on |fp32 Gram formulation - exact| for the MMD:
    with u = 2^-24, a d-term fp32 dot product is off by at most (d + 1) u sum_k |a_k b_k|, so r_i + r_j - 2 g_ij is off by at most
    dD_ij = (d + 4) u (r_i + r_j + 2 sum_k |u_ik v_jk|) (three more roundings for the two additions and the doubling); a kernel
    term moves by at most |dk/dD| dD = a k_q(D) / (C + D) dD; evaluating a term (an addition, a division, a power, a scaling) and
    the fp32 means add 16 u relative to each term's size.  The terms enter with weights 1, 1 and 2.  On the diagonal of XX and
    YY that formulation is exact: the norms are the Gram's own diagonal, and r + r - 2 r rounds nowhere."""
    x = torch.as_tensor(x).to(torch.float64)
    y = torch.as_tensor(y).to(torch.float64)
    u, d = 2.0 ** -24, x.shape[1]

    def term(a, b, same=False):
        diff = a[:, None, :] - b[None, :, :]
        D = (diff * diff).sum(-1)
        dD = (d + 4) * u * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * a.abs() @ b.abs().t())
        if same:
            dD.fill_diagonal_(0.0)
        slope = sum(al * C ** al * ((C + D) / al) ** (-al) / (C + D) for C, al in kernels)
        return float((slope * dD).mean()) + 16 * u * float(kernel_sum(D, kernels).mean())

    return term(x, x, True) + term(y, y, True) + 2.0 * term(x, y)


def bounds(x, y, kernels=DEFAULT, want=None):
    """-> (want, e32, bound): the float64 values (MMD and the three terms), the fp32 Gram formulation's error on each, and
    max(4 e32, 2^-22 S) with S = mean XX + mean YY + 2 mean XY"""
    want = mmd_terms64(x, y, kernels) if want is None else want
    ref = gram_terms32(x, y, kernels)
    e32 = [abs(r - w) for r, w in zip(ref, want)]
    S = want[1] + want[2] + 2.0 * want[3]
    return list(want), e32, [max(4.0 * e, 2.0 ** -22 * S) for e in e32]
