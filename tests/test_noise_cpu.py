"""CPU tests of the noise oracle (tests/noise_oracle.py): Philox4x32-10 against the Random123 known answers, the fp32 floor of
the Box-Muller evaluation, and the per-rank seed rule of the trainers."""
import inspect

import numpy as np
import pytest

import noise_oracle as no

KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(w[0]) for w in no.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_philox_is_vectorised_over_the_counter():
    """an array of counters gives what the counters give one at a time (the three known answers in one call)"""
    cs = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    for j, (counter, key, want) in enumerate(KAT):
        got = no.philox4x32_10(cs, key)
        assert tuple(int(w[j]) for w in got) == want


def test_uniform_ranges_and_edges():
    u0, u1, u2, u3 = no.uniforms(1234, 1, 1 << 16)
    for u in (u0, u2):
        assert u.dtype == np.float32 and u.min() > 0.0 and u.max() <= 1.0
    for u in (u1, u3):
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() <= 1.0
    # the conversion at the ends of the range, as the kernel's fp32 arithmetic gives it
    f = np.array([0, 1, 2 ** 32 - 1], dtype=np.uint64).astype(np.float32)
    u = np.minimum((f + np.float32(1)) * np.float32(2.0 ** -32), np.float32(1))
    assert u[0] == np.float32(2.0 ** -32) and u[1] == np.float32(2.0 ** -31) and u[2] == np.float32(1.0)


def test_float32_path_against_float64_path():
    """e32, the fp32 floor of the draws: computed, not hard-coded.  The angle 2 pi v rounds to fp32 (half an ulp of up to 6.28:
    2.4e-7) and scales by the radius (up to 6.7 at u = 2^-32), log and sqrt add a few ulp of the radius: some 1e-6"""
    n = 1 << 20
    a, b = no.normals(1234, 1, n, np.float32), no.normals(1234, 1, n, np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == (n,)
    e32 = float(np.max(np.abs(a.astype(np.float64) - b)))
    print(f"\nfp32 floor e32 over 2^20 draws at seed 1234, step 1: {e32:.2e}")
    assert e32 == no.fp32_floor(1234, 1, n)
    assert 0.0 < e32 < 2.0 ** -16            # well under the element-wise GPU bound 2^-13 (tests/test_gpu_noise.py)
    # and the draws are standard normal: five-sigma bands of the first four moments over 2^20 draws
    s = 1.0 / np.sqrt(n)
    assert abs(b.mean()) < 5 * s and abs(b.var() - 1.0) < 5 * np.sqrt(2.0) * s
    assert abs((b ** 3).mean()) < 5 * np.sqrt(15.0) * s and abs((b ** 4).mean() - 3.0) < 5 * np.sqrt(96.0) * s
    assert np.abs(b).max() <= np.sqrt(-2.0 * np.log(2.0 ** -32)) + 1e-12


def test_the_gpu_bound_tells_draws_apart():
    """2^-13, the element-wise bound of tests/test_gpu_noise.py, is a discrimination threshold: of two independent draws (another
    step, another seed, the neighbouring element) fewer than 1 in 5000 lie that close, so a misplaced or repeated draw cannot
    pass on a batch of more than a few elements - and the fp32 floor lies far under it"""
    n = 1 << 20
    a = no.normals(1234, 1, n)
    for b in (no.normals(1234, 2, n), no.normals(1235, 1, n), np.roll(a, 1), np.roll(a, 4), np.roll(a, 16 * 6)):
        close = float(np.mean(np.abs(a - b) <= 2.0 ** -13))
        assert close < 2e-4, close
    assert no.fp32_floor(1234, 1, n) * 50 < 2.0 ** -13


def test_prefix_and_words():
    """normals(.., n) is a prefix of normals(.., m > n) for every n % 4; each key and counter word changes the stream"""
    full = no.normals(77, 5, 64)
    for n in (1, 2, 3, 4, 5, 6, 7, 61, 62, 63):
        assert np.array_equal(no.normals(77, 5, n), full[:n])
    base = no.normals(1234, 0, 64)
    for seed, step in ((1234 + 2 ** 32, 0), (1234, 2 ** 32), (1234, 1), (1235, 0)):
        other = no.normals(seed, step, 64)
        assert np.abs(other - base).min() > 0.0, (seed, step)


def test_rank_seeds_are_distinct_streams():
    """(seed + 0x9E3779B97F4A7C15 * rank) & (2^63 - 1), as hint_amd/train.py and hint_amd/conditional.py key the ranks: eight ranks,
    eight seeds, and no rank's first 2^16 draws equal another's in any element"""
    import hint_amd.conditional
    import hint_amd.train
    rule = "(seed + 0x9E3779B97F4A7C15 * rank) & (2 ** 63 - 1)"
    for mod in (hint_amd.train, hint_amd.conditional):       # (the oracle's rule is the trainers')
        assert rule in inspect.getsource(mod), mod.__name__
    for seed in (1234, 2 ** 62 + 12345, 2 ** 63 - 1):
        seeds = [no.rank_seed(seed, r) for r in range(8)]
        assert seeds[0] == seed and len(set(seeds)) == 8 and all(0 <= s < 2 ** 63 for s in seeds)
        draws = [no.normals(s, 1, 1 << 16) for s in seeds]
        for i in range(8):
            for j in range(i + 1, 8):
                assert not np.any(draws[i] == draws[j]), (seed, i, j)
