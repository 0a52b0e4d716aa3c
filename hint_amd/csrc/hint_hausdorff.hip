// Dense curve tracing and the two-sided nearest-point distances of a curve to a template (gfx950): max / avg Hausdorff and chamfer.
//
// Reference being replaced (read-only): run_experiments.py:147-159 and eval_shapes.py:82-95 trace every sampled curve at 100 and at
// 1000 points (data.py:51-57 trace_fourier_curves) and call, per row in a Python loop, max_and_avg_hausdorff_distance
// (best_shape_fit.py:143-149: a [P, M, 2] numpy difference tensor and minima along both axes) on a template that is
// lens_points_from_params (best_shape_fit.py:195-199, via :275-277) or a densified plus outline (:153-156);
// points_to_lens_loss (best_shape_fit.py:203-209) is the same two-sided minimum over squared distances.
// The contract - point sets, the fp32 order of every operation, the outputs and the association of the double sums - is stated in
// include/hint_amd.h (hint_hausdorff_desc).  In short, per row: B = the curve (P points, traced by hint_curve.hip's rule or given),
// A = the template (M points, optionally rotated, scaled and moved), D(i, j) = fma(dy, dy, dx dx) of A_i - B_j,
// mA_i = min_j D, mB_j = min_i D; max_h = sqrt(max of all minima), avg_h = mean of their roots, chamfer = (mean mB, mean mA).
//
// hint_hausdorff_kernel: a persistent grid of G workgroups of 256 threads; workgroup w takes rows w, w + G, ... one at a time.
//   - once per workgroup: the P - 1 twiddles (cos, sin)(2 pi r / (P - 1)) in LDS, sincospi in double as hint_curve.hip does; every
//     frequency indexes them by r = (|m| t) mod (P - 1), which a thread steps from one k to the next by adding or subtracting
//     t mod (P - 1) (one integer modulo per point, none per term);
//   - per row: the 4K coefficients and the five transform constants go to LDS; thread t traces (or loads) points t, t + 256, ... of
//     B and writes them to LDS (8 KiB) and, if asked, to `points`;
//   - the template passes through LDS in tiles of 1024 points (8 KiB).  Per tile, pass 1: thread t holds A points t, t + 256, ...
//     of the tile in registers and walks all of B; pass 2: it walks the tile with its B points, whose minima live in registers
//     across the tiles.  Every LDS read of a walk has one address for the whole wavefront (a broadcast, no bank conflict) and
//     feeds up to four pairs of five vector operations each (two subtractions, a product, an fma, a minimum).  A fused single
//     pass would need a minimum across lanes per point; two passes need none;
//   - the maximum and the four double sums: per thread over its own points in ascending order, six xor-shuffles within the
//     wavefront, then thread 0 adds the four wavefronts in order through LDS and writes the row's outputs.
// Nothing is carried from row to row and nothing is read back from global memory, so a row's bits do not depend on the batch, the
// grid or what any buffer held.  No float atomics, no counters, no workspace.
// Why a workgroup per row: at P = M = 1000 a row is 2 x 10^6 pairs, ~40 000 vector operations per thread, against ~100 for the
// trace and the reductions and three barriers; 88 VGPRs and 24.6 KiB of LDS leave room for five workgroups a CU, which hide each
// other's barriers and loads.  A wavefront per row (as in hint_curve_kernel) would pay only for P, M <~ 128.  Untuned: DESIGN section 14.
#include "hint_host.hpp"

namespace hint {

constexpr int HD_MAX_K = 25, HD_MIN_P = 2, HD_MAX_P = 1024;
constexpr int HD_MAX_M = 4096;                  // template points of a row
constexpr int HD_TILE = 1024;                   // template points in LDS at a time
constexpr int HD_THREADS = 256, HD_PER = 4;     // HD_PER = HD_MAX_P / HD_THREADS = HD_TILE / HD_THREADS points per thread
constexpr int HD_MAX_WG = 1280;                 // the grid cap: 256 CUs x 5 workgroups (88 VGPRs: 5 wavefronts a SIMD)
constexpr long long HD_MAX_N = 1LL << 30;

inline int hd_grid(long long n, int max_groups) {
    const long long cap = max_groups > 0 && max_groups < HD_MAX_WG ? max_groups : HD_MAX_WG;
    return (int)(n < cap ? n : cap);
}

}  // namespace hint

// the walk of both passes: NC points of this thread against n points in LDS.  (D is written for A_i - B_j; pass 2 holds B and
// walks A, and the differences there are the exact negatives, so the squares - and D - are the same bits.)
template <int NC>
__device__ __forceinline__ void hd_scan(const float2* src, int n, const float (&px)[hint::HD_PER], const float (&py)[hint::HD_PER],
                                        float (&m)[hint::HD_PER]) {
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float2 q = src[j];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float dx = __fsub_rn(px[c], q.x), dy = __fsub_rn(py[c], q.y);
            m[c] = fminf(m[c], __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
        }
    }
}

__device__ __forceinline__ void hd_scan_n(int nc, const float2* src, int n, const float (&px)[hint::HD_PER],
                                          const float (&py)[hint::HD_PER], float (&m)[hint::HD_PER]) {
    switch (nc) {                                            // (nc is the same for the whole workgroup)
        case 1: hd_scan<1>(src, n, px, py, m); break;
        case 2: hd_scan<2>(src, n, px, py, m); break;
        case 3: hd_scan<3>(src, n, px, py, m); break;
        default: hd_scan<4>(src, n, px, py, m); break;
    }
}

__device__ __forceinline__ double hd_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);             // (a + b = b + a: every lane ends with the same bits)
    return v;
}

// the row's transform constants (cs, sn, scale, x, y) to LDS, by one thread.  Not inlined: the double-precision sincos holds some
// thirty registers of constants, which would otherwise stay live across the whole row loop
__device__ __noinline__ void hd_stage_params(const float* pr, float* prm) {
    double sn, cs;
    sincos((double)pr[3], &sn, &cs);
    prm[0] = (float)cs;
    prm[1] = (float)sn;
    prm[2] = pr[2];
    prm[3] = pr[0];
    prm[4] = pr[1];
}

__global__ __launch_bounds__(256) void hint_hausdorff_kernel(const float* __restrict__ x, const float* __restrict__ b_points,
                                                             int n, int K, int P, const float* __restrict__ a_points,
                                                             const long long* __restrict__ a_offsets,
                                                             const float* __restrict__ a_params, long long T,
                                                             float* __restrict__ max_h, float* __restrict__ avg_h,
                                                             float* __restrict__ chamfer, float* __restrict__ points) {
    using namespace hint;
    __shared__ float2 tw[HD_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[HD_MAX_P];
    __shared__ float2 Ap[HD_TILE];
    __shared__ float coef[4 * HD_MAX_K + 4];
    __shared__ float prm[8];                                 // cs, sn, scale, x, y
    __shared__ double red[HD_THREADS / 64][4];
    __shared__ float redm[HD_THREADS / 64];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int Pm1 = P - 1, H = K / 2, C = 4 * K;
    const bool traced = x != nullptr, with_prm = a_params != nullptr, with_dist = max_h || avg_h || chamfer;
    const int ncB = (P + HD_THREADS - 1) / HD_THREADS;
    if (traced) {
        for (int r = t; r < Pm1; r += HD_THREADS) {
            double sn, cs;
            sincospi(2.0 * (double)r / (double)(P - 1), &sn, &cs);
            tw[r] = make_float2((float)cs, (float)sn);
        }
    }
    const float qnan = __int_as_float(0x7fc00000);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        // ---- the row's template range; a ragged row whose range is not 1..4096 points inside a_points is a bad row ----
        long long o0 = 0, o1 = T;
        if (a_offsets) {
            o0 = a_offsets[row];
            o1 = a_offsets[row + 1];
        }
        const bool bad = o0 < 0 || o1 > T || o1 - o0 < 1 || o1 - o0 > HD_MAX_M;
        const int M = bad ? 0 : (int)(o1 - o0);
        if (traced && t < C) coef[t] = x[(size_t)row * C + t];
        if (with_prm && with_dist && t == 0) hd_stage_params(a_params + 4 * (size_t)row, prm);
        __syncthreads();
        // ---- B: points t, t + 256, ... to LDS (a rolled loop: one copy of the trace) ----
#pragma unroll 1
        for (int tt = t; tt < P; tt += HD_THREADS) {
            float ax = 0.f, ay = 0.f;
            if (traced) {
                const int t0 = tt == Pm1 ? 0 : tt;                           // t mod (P - 1)
                int r = (H * t0) % Pm1;
                for (int k = 0; k < K; ++k) {
                    const int m = k - H;
                    float2 w = tw[r];
                    if (m < 0) w.y = -w.y;
                    ax = __fmaf_rn(coef[k], w.x, ax);
                    ax = __fmaf_rn(-coef[2 * K + k], w.y, ax);
                    ay = __fmaf_rn(coef[K + k], w.x, ay);
                    ay = __fmaf_rn(-coef[3 * K + k], w.y, ay);
                    if (m < 0) {                                             // r of the next k: |m| goes down to 0, then up
                        r -= t0;
                        if (r < 0) r += Pm1;
                    } else {
                        r += t0;
                        if (r >= Pm1) r -= Pm1;
                    }
                }
                if (points) {
                    float* pp = points + 2 * ((size_t)row * P + tt);
                    pp[0] = ax;
                    pp[1] = ay;
                }
            } else {
                const float* bp = b_points + 2 * ((size_t)row * P + tt);
                ax = bp[0];
                ay = bp[1];
            }
            Bp[tt] = make_float2(ax, ay);
        }
        if (!with_dist) {                                    // points alone: the template is not read
            __syncthreads();                                 // the next row overwrites coef
            continue;
        }
        if (bad) {
            if (t == 0) {
                if (max_h) max_h[row] = qnan;
                if (avg_h) avg_h[row] = qnan;
                if (chamfer) chamfer[2 * (size_t)row] = chamfer[2 * (size_t)row + 1] = qnan;
            }
            __syncthreads();                                 // the next row overwrites coef
            continue;
        }
        float mx = 0.f;                                      // the largest minimum (every D is >= 0 or NaN)
        double sa_rt = 0.0, sa_sq = 0.0, sb_rt = 0.0, sb_sq = 0.0;
        float mb[HD_PER];
#pragma unroll
        for (int c = 0; c < HD_PER; ++c) mb[c] = INFINITY;
        for (int a0 = 0; a0 < M; a0 += HD_TILE) {
            const int cnt = M - a0 < HD_TILE ? M - a0 : HD_TILE;
            const int ncA = (cnt + HD_THREADS - 1) / HD_THREADS;
            if (a0) __syncthreads();                         // the walks of the tile before are done with Ap
#pragma unroll 1
            for (int i = t; i < cnt; i += HD_THREADS) {
                float2 a;                                    // (4-byte aligned: one 8-byte load all the same)
                __builtin_memcpy(&a, a_points + 2 * (size_t)(o0 + a0 + i), sizeof(a));
                float ax = a.x, ay = a.y;
                if (with_prm) {
                    const float cs = prm[0], sn = prm[1];
                    const float qx = __fmaf_rn(-ay, sn, __fmul_rn(ax, cs)), qy = __fmaf_rn(ay, cs, __fmul_rn(ax, sn));
                    ax = __fmaf_rn(qx, prm[2], prm[3]);
                    ay = __fmaf_rn(qy, prm[2], prm[4]);
                }
                Ap[i] = make_float2(ax, ay);
            }
            __syncthreads();
            // this thread's points of both sets, from LDS; a slot past the end repeats the last point and is not counted below
            float px[HD_PER], py[HD_PER], ma[HD_PER], bx[HD_PER], by[HD_PER];
#pragma unroll
            for (int c = 0; c < HD_PER; ++c) {
                const int i = t + HD_THREADS * c, j = t + HD_THREADS * c;
                const float2 pa = Ap[i < cnt ? i : cnt - 1], pb = Bp[j < P ? j : P - 1];
                px[c] = pa.x;
                py[c] = pa.y;
                bx[c] = pb.x;
                by[c] = pb.y;
                ma[c] = INFINITY;
            }
            hd_scan_n(ncA, Bp, P, px, py, ma);               // pass 1: mA of this thread's points of the tile
            hd_scan_n(ncB, Ap, cnt, bx, by, mb);             // pass 2: mB so far
#pragma unroll
            for (int c = 0; c < HD_PER; ++c) {
                if (t + HD_THREADS * c < cnt) {              // (then c < ncA)
                    mx = fmaxf(mx, ma[c]);
                    sa_sq += (double)ma[c];
                    sa_rt += (double)__fsqrt_rn(ma[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < HD_PER; ++c) {
            if (t + HD_THREADS * c < P) {                    // (then c < ncB)
                mx = fmaxf(mx, mb[c]);
                sb_sq += (double)mb[c];
                sb_rt += (double)__fsqrt_rn(mb[c]);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        sa_rt = hd_wave_sum(sa_rt);
        sa_sq = hd_wave_sum(sa_sq);
        sb_rt = hd_wave_sum(sb_rt);
        sb_sq = hd_wave_sum(sb_sq);
        if (l == 0) {
            red[wv][0] = sa_rt;
            red[wv][1] = sa_sq;
            red[wv][2] = sb_rt;
            red[wv][3] = sb_sq;
            redm[wv] = mx;
        }
        __syncthreads();                                     // (and every walk is done: the next row may overwrite Bp, Ap, coef, prm)
        if (t == 0) {
            double s[4];
            float v = redm[0];
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = red[0][q];
            for (int w = 1; w < HD_THREADS / 64; ++w) {
                v = fmaxf(v, redm[w]);
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] += red[w][q];
            }
            if (max_h) max_h[row] = __fsqrt_rn(v);
            if (avg_h) avg_h[row] = (float)((s[0] + s[2]) / (double)(M + P));
            if (chamfer) {
                chamfer[2 * (size_t)row] = (float)(s[3] / (double)P);
                chamfer[2 * (size_t)row + 1] = (float)(s[1] / (double)M);
            }
        }
    }
}

// ---- the C ABI ----
using namespace hint;

static int hd_check_sizes(const char* who, int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points,
                          bool traced) {
    if (n_rows < 1 || n_rows > HD_MAX_N) return fail("%s: n_rows must be 1..%lld (got %lld)", who, HD_MAX_N, (long long)n_rows);
    if (traced && (n_coeffs < 1 || n_coeffs > HD_MAX_K || (n_coeffs & 1) == 0))
        return fail("%s: n_coeffs must be odd and 1..%d (got %d)", who, HD_MAX_K, n_coeffs);
    if (n_points < HD_MIN_P || n_points > HD_MAX_P)
        return fail("%s: n_points must be %d..%d (got %d)", who, HD_MIN_P, HD_MAX_P, n_points);
    if (max_template_points < 1 || max_template_points > HD_MAX_M)
        return fail("%s: a row's template must hold 1..%d points (got %lld)", who, HD_MAX_M, (long long)max_template_points);
    return 0;
}

extern "C" {

size_t hint_hausdorff_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points) {
    // n_coeffs = 0 stands for the given-points source, which has no coefficients
    if (hd_check_sizes("hint_hausdorff_workspace_bytes", n_rows, n_coeffs, n_points, max_template_points, n_coeffs != 0)) return 0;
    last_error_ref().clear();
    return 0;                                                // the kernel needs none
}

int64_t hint_hausdorff_geometry(int64_t n_rows, int32_t n_points, int64_t max_template_points, int32_t field) {
    if (hd_check_sizes("hint_hausdorff_geometry", n_rows, 1, n_points, max_template_points, false)) return -1;
    if (field < 0 || field > 4) {
        fail("hint_hausdorff_geometry: no field %d (0 workgroups, 1 rows per workgroup at a time, 2 template points per LDS tile, "
             "3 the grid cap, 4 tiles of the largest template)", field);
        return -1;
    }
    const int64_t out[5] = {hd_grid(n_rows, 0), 1, HD_TILE, HD_MAX_WG, (max_template_points + HD_TILE - 1) / HD_TILE};
    return out[field];
}

int hint_hausdorff_run(const hint_hausdorff_desc* desc, void* stream) {
    const char* who = "hint_hausdorff_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->a_points) return fail("%s: a_points is null", who);
    if (desc->x && desc->b_points) return fail("%s: both x and b_points are given (the curve has one source)", who);
    if (!desc->x && !desc->b_points) return fail("%s: x and b_points are both null (the curve needs a source)", who);
    if (desc->points && desc->b_points) return fail("%s: points is an output of the traced source only (b_points is given)", who);
    if (!desc->max_h && !desc->avg_h && !desc->chamfer && !desc->points)
        return fail("%s: no output requested (max_h, avg_h, chamfer and points are all null)", who);
    if (desc->n_template < 1) return fail("%s: n_template must be >= 1 (got %lld)", who, (long long)desc->n_template);
    // a shared template is a row's template; ragged rows are checked by the kernel, their total here
    const int64_t row_max = desc->a_offsets ? 1 : desc->n_template;
    if (hd_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, row_max, desc->x != nullptr)) return 1;
    if (desc->a_offsets && desc->n_template > desc->n_rows * (int64_t)HD_MAX_M)
        return fail("%s: n_template = %lld is more than n_rows x %d points", who, (long long)desc->n_template, HD_MAX_M);
    if (desc->max_groups < 0) return fail("%s: max_groups must be >= 0 (got %d)", who, desc->max_groups);
    if (((uintptr_t)desc->x & 3) != 0) return fail("%s: x must be 4-byte aligned", who);
    if (((uintptr_t)desc->b_points & 3) != 0) return fail("%s: b_points must be 4-byte aligned", who);
    if (((uintptr_t)desc->a_points & 3) != 0) return fail("%s: a_points must be 4-byte aligned", who);
    if (((uintptr_t)desc->a_offsets & 7) != 0) return fail("%s: a_offsets must be 8-byte aligned", who);
    if (((uintptr_t)desc->a_params & 3) != 0) return fail("%s: a_params must be 4-byte aligned", who);
    if (((uintptr_t)desc->max_h & 3) != 0) return fail("%s: max_h must be 4-byte aligned", who);
    if (((uintptr_t)desc->avg_h & 3) != 0) return fail("%s: avg_h must be 4-byte aligned", who);
    if (((uintptr_t)desc->chamfer & 3) != 0) return fail("%s: chamfer must be 4-byte aligned", who);
    if (((uintptr_t)desc->points & 3) != 0) return fail("%s: points must be 4-byte aligned", who);
    const int grid = hd_grid(desc->n_rows, desc->max_groups);
    hipLaunchKernelGGL(hint_hausdorff_kernel, dim3(grid), dim3(HD_THREADS), 0, (hipStream_t)stream, desc->x, desc->b_points,
                       (int)desc->n_rows, desc->x ? desc->n_coeffs : 1, desc->n_points, desc->a_points,
                       (const long long*)desc->a_offsets, desc->a_params, (long long)desc->n_template, desc->max_h, desc->avg_h,
                       desc->chamfer, desc->points);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
