// hint_amd/csrc/hint_epochperm.hpp on the host alone, for a run under AddressSanitizer + UBSan (host code only; nothing of it
// touches a GPU or is loaded into Python):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/epochperm_check.cpp -o epochperm_check
// For every N of 1..300 and of the large list it walks the positions tests/test_epoch_cpu.py compares with the oracle, over the
// same epochs and seeds, checks range, cap and (N <= 300) bijectivity, and prints one line per N: N, a sum of the source rows
// (mod 2^64) and the longest walk.  tests/test_epoch_cpu.py compares the lines with tests/epoch_oracle.py.  Exit status 1 on a
// violated property.
#include <cstdio>
#include <vector>

#include "../hint_amd/csrc/hint_epochperm.hpp"

using namespace hint;

static const uint32_t EPOCHS[3] = {0u, 1u, 0xFFFFFFFFu};
static const uint64_t SEEDS[3] = {0ull, 1ull, ~0ull};

// the positions of the large cases: 0, 1, N / 2, N - 2, N - 1 and 64 others, (k * 0x9E3779B97F4A7C15 >> 11) % N for k = 1..64
static std::vector<uint64_t> positions(uint64_t n) {
    std::vector<uint64_t> p = {0, 1 % n, n / 2, n >= 2 ? n - 2 : 0, n - 1};
    for (uint64_t k = 1; k <= 64; ++k) p.push_back(((k * 0x9E3779B97F4A7C15ull) >> 11) % n);
    return p;
}

static int run(uint64_t n, bool all) {
    const int h = ep_half_bits(n);
    uint64_t sum = 0;
    int longest = 0;
    std::vector<uint64_t> pos;
    if (all)
        for (uint64_t p = 0; p < n; ++p) pos.push_back(p);
    else
        pos = positions(n);
    for (uint32_t epoch : EPOCHS)
        for (uint64_t seed : SEEDS) {
            std::vector<char> seen(all ? n : 0, 0);
            for (uint64_t p : pos) {
                int steps = 0;
                const int64_t v = ep_source_row(n, h, seed, epoch, 1, p, &steps);
                if (v < 0 || (uint64_t)v >= n || steps < 1 || steps > EP_WALK_CAP) {
                    std::printf("N %llu position %llu: source row %lld after %d applications\n", (unsigned long long)n,
                                (unsigned long long)p, (long long)v, steps);
                    return 1;
                }
                if (all) {
                    if (seen[(size_t)v]) {
                        std::printf("N %llu: source row %lld taken twice\n", (unsigned long long)n, (long long)v);
                        return 1;
                    }
                    seen[(size_t)v] = 1;
                }
                if (ep_source_row(n, h, seed, epoch, 0, p) != (int64_t)p) return 1;
                sum += (uint64_t)v * (p + 1);
                longest = steps > longest ? steps : longest;
            }
        }
    std::printf("%llu %llu %d\n", (unsigned long long)n, (unsigned long long)sum, longest);
    return 0;
}

int main() {
    for (uint64_t n = 1; n <= 300; ++n)
        if (run(n, true)) return 1;
    const uint64_t big[6] = {1024, 1025, 4096, 4097, 65537, (uint64_t)1 << 40};
    for (uint64_t n : big)
        if (run(n, false)) return 1;
    return 0;
}
