// Coefficients of an ExternalAffineCoupling (gfx950 / CDNA4 only): a one-node block whose upper half is empty, so that its s and t
// nets see the condition only (conditional_hint_4_full.py:76-82) and the coupling is a fixed element-wise affine map per condition row.
//
// Arithmetic reproduced (reference, read-only): hint.py:10-13 (Linear-ReLU-Linear-ReLU-Linear), hint.py:56-60 (soft clamp)
//   v = c;  s = mlp_s(v), t = mlp_t(v);  coef[row] = [ alpha * atan(s) | t ],  alpha = clamp * 0.636
//
// One workgroup takes 16 condition rows and ONE of the two nets (blockIdx.y: 0 = s, 1 = t).  The thin first layer (K = dc) runs on
// the vector ALU from the flat parameters; the h x h layer and the h -> r layer run transposed on the matrix pipe
// (v_mfma_f32_16x16x4_f32), out^T[features x 16 rows] = W * act^T, with the weights as the A operand straight from the plan's
// packed fragment tiles (hint_dev.h, layout 0: one float4 per lane per 16 x 16 tile) and the activations as the B operand from LDS
// in the same k order (component i of a lane's float4 feeds MFMA i of the k-block).
#include "hint_device.hpp"

using namespace hint;

constexpr int EXT_NW = 4;

// acc = one 16 x 16 tile of W * act^T: wt = the tile row's first packed tile, NT k-blocks; act: [16][ld] in LDS, zero beyond h
__device__ __forceinline__ void ext_gemm(f32x4& acc, const GLOBAL_AS float* wt, int NT, const float* act, int ld, int lane) {
    acc = zero4();
    const int m = lane & 15, kq = lane >> 4;
    for (int kb = 0; kb < NT; ++kb) {
        const f32x4 w = *(const GLOBAL_AS f32x4*)(wt + (size_t)kb * 256 + lane * 4);
        const f32x4 v = *(const f32x4*)(act + m * ld + kb * 16 + 4 * kq);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = mfma4(w[i], v[i], acc);
    }
}

__global__ __launch_bounds__(64 * EXT_NW) void hint_ext_coeff_kernel(ExtArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);
    const int net = blockIdx.y;
    const int row0 = blockIdx.x * ROWS;
    const int hp = 16 * a.NT, ld = hp + 4;       // (+4: the B-operand reads of 16 rows land on different banks)
    float* cs = lds;                             // [16][dc]
    float* a1 = cs + ((ROWS * a.dc + 3) & ~3);   // [16][ld]
    float* a2 = a1 + ROWS * ld;                  // [16][ld]
    const GLOBAL_AS float* P = (const GLOBAL_AS float*)a.params;
    const GLOBAL_AS float* W1 = P + a.w1[net];
    const GLOBAL_AS float* B1 = P + a.b1[net];
    const GLOBAL_AS float* B2 = P + a.b2[net];
    const GLOBAL_AS float* B3 = P + a.b3[net];
    const int nvalid = a.R - row0 < ROWS ? a.R - row0 : ROWS;
    for (int i = tid; i < ROWS * a.dc; i += blockDim.x) {
        const int r = i / a.dc;
        cs[i] = r < nvalid ? ((const GLOBAL_AS float*)a.c)[(size_t)row0 * a.dc + i] : 0.f;
    }
    __syncthreads();
    // first layer on the vector ALU: a1[row][j] = relu(b1[j] + sum_k W1[j][k] c[row][k]), zero up to hp
    for (int i = tid; i < ROWS * hp; i += blockDim.x) {
        const int r = i / hp, j = i - r * hp;
        float v = 0.f;
        if (j < a.h) {
            v = B1[j];
            for (int k = 0; k < a.dc; ++k) v = fmaf(W1[(size_t)j * a.dc + k], cs[r * a.dc + k], v);
            v = fmaxf(v, 0.f);
        }
        a1[r * ld + j] = v;
    }
    __syncthreads();
    const int m = lane & 15, fq = 4 * (lane >> 4);     // accumulator: features nt * 16 + fq + i of row m
    // second layer (h x h) on the matrix pipe
    for (int nt = wave; nt < a.NT; nt += EXT_NW) {
        f32x4 acc;
        ext_gemm(acc, (const GLOBAL_AS float*)a.packed + (size_t)(a.f2[net] + nt * a.NT) * 256, a.NT, a1, ld, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = nt * 16 + fq + i;
            a2[m * ld + f] = f < a.h ? fmaxf(acc[i] + B2[f], 0.f) : 0.f;
        }
    }
    __syncthreads();
    // third layer (h -> r) on the matrix pipe, then the clamp of the s net (hint.py:56-60).  The ReLUs above return 0 for a NaN
    // pre-activation, so a NaN or inf in a condition row would leave finite coefficients where the reference has NaN: pz is +0
    // for a finite row and NaN for any other (hint_fwd.hip poisons its rows the same way)
    float pz = 0.f;
    for (int k = 0; k < a.dc; ++k) pz += cs[m * a.dc + k];
    pz = pz - pz;
    for (int nt = wave; nt < a.RT; nt += EXT_NW) {
        f32x4 acc;
        ext_gemm(acc, (const GLOBAL_AS float*)a.packed + (size_t)(a.f3[net] + nt * a.NT) * 256, a.NT, a2, ld, lane);
        if (m < nvalid) {
            float* out = a.coef + (size_t)(row0 + m) * 2 * a.r + (size_t)net * a.r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = nt * 16 + fq + i;
                if (f < a.r) {
                    const float v = (acc[i] + B3[f]) + pz;
                    out[f] = net == 0 ? a.alpha * atanf(v) : v;
                }
            }
        }
    }
}

namespace hint {

int ext_lds_bytes(const ExtArgs& a) { return 4 * (((ROWS * a.dc + 3) & ~3) + 2 * ROWS * (16 * a.NT + 4)); }

hipError_t launch_ext_coeff(const ExtArgs& a, hipStream_t stream) {
    const int lds = ext_lds_bytes(a);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)hint_ext_coeff_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hint_ext_coeff_kernel, dim3((a.R + ROWS - 1) / ROWS, 2), dim3(64 * EXT_NW), lds, stream, a);
    return hipGetLastError();
}

}  // namespace hint
