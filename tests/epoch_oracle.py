"""The test-side definition of the epoch permutation (include/hint_amd.h, hint_epoch_desc), restated in numpy from the header's
text, the positions a rank takes of an epoch, and the error bounds of the column statistics.

    N = rows, 1 <= N <= 2^40; h = max(1, ceil(bitlength(N-1) / 2)); the domain is M = 4^h; v = L << h | R
    four rounds (L, R) -> (R, L ^ F_r(R)); F_r(R) = the low h bits of word 0 of Philox4x32-10 on counter {R, r, epoch, 0x45504F43},
    key {seed lo, seed hi}; cycle walking v = p; do v = feistel(v); while (v >= N); capped at 256 applications (-1)

MOMENTS.  u = 2^-53.  The data are fp32 values, exact in double.  A sum of N doubles in ANY fixed order differs from the exact sum
by at most (N - 1) u sum|x| to first order (every partial sum is rounded once and no partial sum exceeds sum|x|); the division by N
adds one rounding.  So the computed mean m^ has |m^ - m| <= E_m = (N + 1) u mean|x|.
The second pass sums fl((x - m^)^2).  Exactly, sum (x - m^)^2 = sum (x - m)^2 + N (m^ - m)^2 (the cross term vanishes), so the
quantity under the root is V + delta^2 with |delta| <= E_m, times (1 + theta), |theta| <= (N + 4) u: the subtraction (1 rounding),
the square (the subtraction's twice, its own once), the sum of N non-negative terms ((N - 1) u relative) and the division (1).
sqrt(V + delta^2) - sqrt(V) <= |delta|, sqrt((1 + theta)) - 1 <= theta / 2, and the root is rounded once.  So
|std^ - std| <= E_s = ((N + 4) / 2 + 1) u (std + E_m) + E_m.
The GPU tests compare against numpy's float64 mean and std, themselves fixed-order double sums of the same data, to which the same
bounds apply: the device and numpy may differ by 2 E_m and 2 E_s.  Nothing here is tuned to a device's output."""
import numpy as np

import noise_oracle as no

TAG = 0x45504F43
ROUNDS = 4
WALK_CAP = 256
MAX_ROWS = 1 << 40
U = 2.0 ** -53


def half_bits(n: int) -> int:
    return max(1, (int(n - 1).bit_length() + 1) // 2)


def feistel(v, h: int, seed: int, epoch: int):
    """one application of the network to an array of uint64 values of the domain 4^h"""
    v = np.asarray(v, dtype=np.uint64)
    mask = np.uint64((1 << h) - 1)
    L, R = v >> np.uint64(h), v & mask
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for r in range(ROUNDS):
        F = no.philox4x32_10((R, r, epoch & 0xFFFFFFFF, TAG), key)[0] & mask
        L, R = R, L ^ F
    return (L << np.uint64(h)) | R


def source_rows(n, seed: int, epoch: int, positions, shuffle: bool = True, with_steps: bool = False):
    """the source row of every position (int64; -1 where the walk reached the cap) [and the applications each took].  n: the
    table's rows, or one value per position (tables of one h, walked together)"""
    p = np.atleast_1d(np.asarray(positions, dtype=np.uint64))
    nn = np.broadcast_to(np.asarray(n, dtype=np.uint64), p.shape)
    assert 1 <= int(nn.min()) and int(nn.max()) <= MAX_ROWS and (p < nn).all()
    if not shuffle:
        return (p.astype(np.int64), np.zeros(len(p), dtype=np.int64)) if with_steps else p.astype(np.int64)
    h = half_bits(int(nn.max()))
    assert half_bits(int(nn.min())) == h
    out = np.full(len(p), -1, dtype=np.int64)
    steps = np.full(len(p), WALK_CAP, dtype=np.int64)
    live, v = np.arange(len(p)), p.copy()
    for i in range(1, WALK_CAP + 1):
        if len(live) == 0:
            break
        v = feistel(v, h, seed, epoch)
        done = v < nn[live]
        out[live[done]], steps[live[done]] = v[done].astype(np.int64), i
        live, v = live[~done], v[~done]
    return (out, steps) if with_steps else out


def epoch_order(n: int, seed: int, epoch: int):
    return source_rows(n, seed, epoch, np.arange(n, dtype=np.uint64))


def rank_positions(first_batch: int, n_batches: int, batch_size: int, rank: int = 0, world: int = 1):
    """the positions of an epoch rank `rank` of `world` takes for global batches first_batch .. first_batch + n_batches - 1:
    global batch g covers [g B world, (g + 1) B world), the rank the rank-th B of them"""
    g = np.arange(first_batch, first_batch + n_batches, dtype=np.int64)[:, None]
    return (g * batch_size * world + rank * batch_size + np.arange(batch_size, dtype=np.int64)[None, :]).reshape(-1)


def moment_bounds(x64: np.ndarray):
    """(E_m [d], E_s [d]) of the module docstring for the float64 copy of the fp32 data [N, d]"""
    N = x64.shape[0]
    a = np.abs(x64).mean(axis=0)
    std = x64.std(axis=0)
    e_m = (N + 1) * U * a
    e_s = ((N + 4) / 2 + 1) * U * (std + e_m) + e_m
    return e_m, e_s
