// The draws of a sampled row, shared by the shape samplers (hint_shapegen.hip, hint_plusgen.hip), and, at the end, the host side
// their entry points share: the grid, the workspace of rejected-row counts and the checks around them.  Internal.
// Everything here is part of the contract of include/hint_amd.h (hint_lensgen_desc, hint_plusgen_desc): a row's draws are a
// function of (seed, row, stream, tag) alone.
#pragma once
#include <hip/hip_runtime.h>

#include "hint_host.hpp"

// (hint_curve.hip's: LDS writes of some lanes, reads of others, within one wavefront)
__device__ __forceinline__ void shapegen_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Philox4x32-10 on counter = {row lo, row hi, stream, tag}, key = {seed lo, seed hi} (include/hint_amd.h)
__device__ __forceinline__ void row_philox(unsigned long long seed, unsigned long long row, unsigned stream, unsigned tag, unsigned (&c)[4]) {
    unsigned c0 = (unsigned)row, c1 = (unsigned)(row >> 32), c2 = stream, c3 = tag;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
}
// one Box-Muller pair, as philox_normal4 (hint_device.hpp) takes it: v_log_f32 is log2, v_sin / v_cos take turns
__device__ __forceinline__ float2 row_box_muller(unsigned a, unsigned b) {
    const float u0 = fminf(((float)a + 1.0f) * 2.3283064365386963e-10f, 1.0f);
    const float u1 = (float)b * 2.3283064365386963e-10f;
    const float r = __builtin_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0));
    return float2{r * __builtin_amdgcn_cosf(u1), r * __builtin_amdgcn_sinf(u1)};
}

// ---- the host side of hint_lensgen_run, hint_fcoef_run and hint_plusgen_run ----
namespace hint {

// a sampler's launch: per_wave items (rows; hint_fcoef_run: rows x harmonics) a wavefront, `waves` wavefronts a workgroup, at
// most max_wg workgroups, at most max_n rows.  Every wavefront of the grid ends by writing the rows it rejected to its int32
// of the workspace
struct RowGrid {
    int per_wave, waves, max_wg;
    long long max_n;
    int groups(long long items, int max_groups) const {
        const long long g = ((items + per_wave - 1) / per_wave + waves - 1) / waves;
        const long long cap = max_groups > 0 && max_groups < max_wg ? max_groups : max_wg;
        return (int)(g > cap ? cap : g);
    }
    // the workspace: one int32 per wavefront of the default grid, whatever max_groups a run passes
    size_t ws_bytes(long long items) const { return (size_t)groups(items, 0) * waves * sizeof(int32_t); }
    int check_rows(const char* who, int64_t n_rows) const {
        if (n_rows < 1 || n_rows > max_n) return fail("%s: n_rows must be 1..%lld (got %lld)", who, max_n, (long long)n_rows);
        return 0;
    }
    // a smaller grid than the default one leaves the workspace's tail unwritten: the words of wavefronts that do not exist hold 0
    template <class Desc>
    int clear_tail(int wgs, const Desc* desc, size_t need, hipStream_t s) const {
        if ((size_t)wgs * waves * sizeof(int32_t) < need) HIP_TRY(hipMemsetAsync(desc->workspace, 0, need, s));
        return 0;
    }
};

// rows offset .. offset + n_rows - 1 of a Philox stream
inline int check_row_offset(const char* who, uint64_t offset, int64_t n_rows) {
    if (offset > ~0ull - (uint64_t)n_rows) return fail("%s: offset + n_rows must stay below 2^64", who);
    return 0;
}

}  // namespace hint
