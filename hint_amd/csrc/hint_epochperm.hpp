// The epoch permutation: position p of epoch e -> source row, a function of (n_rows, seed, epoch, p) alone.  One text for the host
// (hint_epoch_index, tools/epochperm_check.cpp) and the device (hint_epoch.hip): no HIP intrinsics, 64-bit products where
// row_philox (hint_rowdraws.hpp) uses __umulhi.  The definition, word for word in include/hint_amd.h (hint_epoch_desc):
//   h = max(1, ceil(bitlength(N - 1) / 2)); the domain is M = 4^h, N <= M < 4 N for N >= 2; v = L << h | R
//   four rounds (L, R) -> (R, L ^ F_r(R)), F_r(R) = the low h bits of word 0 of Philox4x32-10 on counter {R, r, epoch, 0x45504F43},
//   key {seed lo, seed hi};  cycle walking: v = p; do v = feistel(v); while (v >= N);  at most 256 applications, then -1
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HINT_EP_HD __host__ __device__ inline
#else
#define HINT_EP_HD inline
#endif

namespace hint {

constexpr int EP_ROUNDS = 4;
constexpr int EP_WALK_CAP = 256;                    // applications of the network a row may take; a row that needs more is flagged
constexpr uint32_t EP_TAG = 0x45504F43u;            // counter word 3: "EPOC"
constexpr int64_t EP_MAX_ROWS = (int64_t)1 << 40;

// h: bits of a half
HINT_EP_HD int ep_half_bits(uint64_t n) {
    int bits = 0;
    for (uint64_t m = n - 1; m != 0; m >>= 1) ++bits;
    const int h = (bits + 1) / 2;
    return h < 1 ? 1 : h;
}

// word 0 of Philox4x32-10
HINT_EP_HD uint32_t ep_philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// one application of the network on the domain 4^h
HINT_EP_HD uint64_t ep_feistel(uint64_t v, int h, uint64_t seed, uint32_t epoch) {
    const uint32_t mask = (1u << h) - 1u;           // h <= 20
    uint32_t L = (uint32_t)(v >> h), R = (uint32_t)v & mask;
    for (uint32_t r = 0; r < (uint32_t)EP_ROUNDS; ++r) {
        const uint32_t F = ep_philox_word0(R, r, epoch, EP_TAG, (uint32_t)seed, (uint32_t)(seed >> 32)) & mask;
        const uint32_t t = L ^ F;
        L = R;
        R = t;
    }
    return ((uint64_t)L << h) | R;
}

// the source row of position p < n (h = ep_half_bits(n)); -1: the walk reached its cap.  steps (may be null): applications taken
HINT_EP_HD int64_t ep_source_row(uint64_t n, int h, uint64_t seed, uint32_t epoch, int shuffle, uint64_t p, int* steps = nullptr) {
    if (steps) *steps = 0;
    if (!shuffle) return (int64_t)p;
    uint64_t v = p;
    for (int i = 1; i <= EP_WALK_CAP; ++i) {
        v = ep_feistel(v, h, seed, epoch);
        if (v < n) {
            if (steps) *steps = i;
            return (int64_t)v;
        }
    }
    if (steps) *steps = EP_WALK_CAP;
    return -1;
}

}  // namespace hint
