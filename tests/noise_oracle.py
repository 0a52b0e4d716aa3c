"""The training noise as a specification: Philox4x32-10 (Salmon et al., SC'11; the Random123 library) + Box-Muller, in numpy.
TEST INFRASTRUCTURE - nothing here is imported by the library.

The forward kernels (philox_normal4 in hint_amd/csrc/hint_device.hpp) perturb a training batch x [B, d] in LDS:
    x_noisy.flat[f] = x.flat[f] + noise * N[f],     N[4 g + k] = output k of one Philox + Box-Muller call with
    counter = {g, step & 0xffffffff, step >> 32, 0x48494e54},   key = {seed & 0xffffffff, seed >> 32}
`normals(seed, step, n, dtype)` is N[:n].  The four 32-bit outputs c0..c3 of the call become
    u0 = ((float)c0 + 1) * 2^-32, u2 likewise: in (0, 1] (fp32 arithmetic: c = 2^32 - 1 rounds to 2^32, + 1 leaves it, clipped at 1)
    u1 = (float)c1 * 2^-32, u3 likewise: an angle in turns
    N = sqrt(-2 ln u0) * (cos 2 pi u1, sin 2 pi u1),  sqrt(-2 ln u2) * (cos 2 pi u3, sin 2 pi u3)
The uniforms are rounded to fp32 exactly as the kernel rounds them (they are the kernel's inputs to its transcendentals, part
of the definition); what follows is evaluated in float64 (the reference) or, the same formulas, in numpy float32 (the fp32 floor:
what any fp32 evaluation may differ from the reference by)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TAG = 0x48494E54            # counter word 3: "HINT"
RANK_STRIDE = 0x9E3779B97F4A7C15


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint64 arrays holding the 32-bit outputs"""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    k = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in key]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = k
    s32 = np.uint64(32)
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                         # 32 x 32 -> 64 bit: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK, (p0 >> s32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def uniforms(seed: int, step: int, n_groups: int):
    """the kernel's four fp32 uniforms of the first n_groups element groups: (u0, u1, u2, u3), each [n_groups]"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    g = np.arange(n_groups, dtype=np.uint64) & MASK
    c = philox4x32_10((g, step & 0xFFFFFFFF, step >> 32, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    f = [w.astype(np.float32) for w in c]                 # (float)c: round to nearest even, as v_cvt_f32_u32
    one, scale = np.float32(1.0), np.float32(2.0 ** -32)
    return (np.minimum((f[0] + one) * scale, one), f[1] * scale, np.minimum((f[2] + one) * scale, one), f[3] * scale)


def normals(seed: int, step: int, n: int, dtype=np.float64):
    """the first n draws of the stream of (seed, step), in `dtype` (float64: the reference; float32: the same formulas in fp32)"""
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(np.float64), np.dtype(np.float32))
    u0, u1, u2, u3 = (u.astype(dtype) for u in uniforms(seed, step, (n + 3) // 4))
    two, tau = dtype.type(2.0), dtype.type(2.0 * np.pi)
    r0, r1 = np.sqrt(-two * np.log(u0)), np.sqrt(-two * np.log(u2))
    a0, a1 = tau * u1, tau * u3
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    assert out.dtype == dtype
    return out.reshape(-1)[:n]


def rank_seed(seed: int, rank: int) -> int:
    """the seed a data-parallel rank keys its stream with (hint_amd/train.py, hint_amd/conditional.py)"""
    return (int(seed) + RANK_STRIDE * int(rank)) & (2 ** 63 - 1)


def fp32_floor(seed: int, step: int, n: int) -> float:
    """e32: the largest distance of the float32 evaluation from the float64 one over the first n draws"""
    return float(np.max(np.abs(normals(seed, step, n, np.float32).astype(np.float64) - normals(seed, step, n, np.float64))))
