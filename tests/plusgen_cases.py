"""What tests/test_plusgen_cpu.py and tests/test_gpu_plusgen.py share: the seeds and sizes of the GPU tests (the CPU file
establishes, by the oracle alone, that their ambiguous share is within the cap), the hand-built draws, and the CPU sweeps the
moment test compares the device with.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import plusgen_oracle as po

SEED = 0x5EED0123456789AB
MOMENT_SEED = SEED + 7
N_BIG = 4099
HIGH = 2 ** 32 - 5                 # with n = 10 the row counter's high word changes inside the call
TARGETS = ((0.3, -0.2, 0.7, 0.25), (0.0, 0.0, 0.0, 1.0), (-0.4, 0.1, 1.3, 4.0), (0.2, 0.2, 0.4, 2.5), (0.2, 0.2, 1.1, 0.6))
# (target, radius, n, seed, candidates the CPU draws): a loose radius, so that a few hundred candidates suffice
CONDITIONAL = ((0.2, -0.1, 0.6, 1.5), 0.5, 64, 991, 1000)
SWEEP_SEED, SWEEP_ROWS = 20250, 400000
# the shares of a numpy sweep of 4e5 prior rows: full plus, one arm missing, two adjacent arms missing
SHARES = {15: 0.730, 14: 0.062, 13: 0.062, 11: 0.062, 7: 0.062, 10: 0.0054, 9: 0.0054, 6: 0.0054, 5: 0.0054}


def pattern_draws(per=6, seed=4):
    """draws [9 per, 9] with `per` rows of each of the nine patterns, and their arms masks.  A bar whose shift is extreme and whose
    length is short ends before the other bar's side: with u_s = 1 - 0.02 r and u_l = 0.02 r, r in [0, 1], xleft = -0.08 r, inside
    the narrowest y bar (0.25 either side)"""
    rng = np.random.RandomState(seed)
    rows, masks = [], []
    for xs in ("both", "low", "high"):
        for ys in ("both", "low", "high"):
            for _ in range(per):
                d = rng.rand(9)
                d[7:] = rng.randn(2)
                mask = 15
                for state, i_len, i_shift, lo_bit, hi_bit in ((xs, 0, 4, 1, 2), (ys, 1, 5, 8, 4)):
                    r = rng.rand()
                    if state == "both":
                        d[i_shift] = 0.35 + 0.3 * r
                    elif state == "low":                     # the bar ends before the other's low side: the low arm is missing
                        d[i_shift], d[i_len], mask = 1 - 0.02 * r, 0.02 * rng.rand(), mask & ~lo_bit
                    else:
                        d[i_shift], d[i_len], mask = 0.02 * r, 0.02 * rng.rand(), mask & ~hi_bit
                rows.append(d)
                masks.append(mask)
    return np.array(rows, dtype=np.float32), np.array(masks)


def corner_case_draws():
    """dyadic draws at the corners of the parameter box: all-zero and all-one uniforms, the longest bars with the narrowest widths
    and the shortest with the widest at every extreme and middle shift, and a row with an edge of exactly 0.5 (len / 0.2 = 2.5)"""
    rows = [np.zeros(9), np.concatenate([np.ones(7), [0.5, -0.25]])]
    for ul, uw in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)):
        for sx in (0.0, 0.5, 1.0):
            for sy in (0.0, 0.5, 1.0):
                rows.append(np.array([ul, ul, uw, uw, sx, sy, 0.5 * sx + 0.25 * sy, 0.5, -0.25]))
    rows.append(np.array([0.0, 0.0, 0.0, 0.5, 0.5, 0.25, 0.25, 0.0, 0.0]))       # ytop - xtop = 0.75 - 0.25 = 0.5
    return np.array(rows, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def sweep_arms():
    """the arms masks of the CPU sweep's SWEEP_ROWS prior rows"""
    d = po.draws(SWEEP_SEED, 0, SWEEP_ROWS)[:, :7].astype(np.float32)
    return po.arms(po.local_coords(np.concatenate([d, np.zeros((len(d), 2), np.float32)], axis=1)))


def corner_share():
    """(the share of 8-corner rows in the CPU sweep, its rows)"""
    return float((sweep_arms() != 15).mean()), SWEEP_ROWS


@functools.lru_cache(maxsize=None)
def geometry_moments(rows=40000):
    """(mean [2], variance [2], fourth central moment [2], rows) of (-mean) R over a CPU sweep: the part of center the normals do
    not touch"""
    g = np.concatenate([po.geometry_center(po.draws(SWEEP_SEED + 1, o, 10000).astype(np.float32)) for o in range(0, rows, 10000)])
    m = g.mean(axis=0)
    return m, g.var(axis=0), ((g - m) ** 4).mean(axis=0), rows
