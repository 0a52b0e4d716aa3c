// The draws of a sampled row, shared by the shape samplers (hint_shapegen.hip, hint_plusgen.hip).  Internal.
// Everything here is part of the contract of include/hint_amd.h (hint_lensgen_desc, hint_plusgen_desc): a row's draws are a
// function of (seed, row, stream, tag) alone.
#pragma once
#include <hip/hip_runtime.h>

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
