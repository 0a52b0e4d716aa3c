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
// hint_hausdorff_kernel: a persistent grid of G workgroups of 256 threads; workgroup w takes rows w, w + G, ... one at a time.  The
// curve's trace, the placement, the two-pass walk over LDS tiles of the other point set and the reductions are
// hint_pointset.hpp's, shared with hint_plus.hip and hint_lensfit.hip; this file adds where the template comes from:
//   - once per workgroup: the P - 1 twiddles in LDS (ps_twiddles);
//   - per row: the 4K coefficients and the row's pose (ps_stage_pose) go to LDS; B is traced or loaded into LDS (8 KiB) and, if
//     asked, written to `points` (ps_stage_curve);
//   - the template passes through LDS in tiles of 1024 points (8 KiB), loaded from a_points and placed by the row's pose
//     (ps_place) on the way in - the tile filler this kernel hands to ps_two_sided;
//   - the maximum and the four double sums by ps_block_reduce; thread 0 writes the row's outputs.
// Nothing is carried from row to row and nothing is read back from global memory, so a row's bits do not depend on the batch, the
// grid or what any buffer held.  No float atomics, no counters, no workspace.
// Why a workgroup per row: at P = M = 1000 a row is 2 x 10^6 pairs, ~40 000 vector operations per thread, against ~100 for the
// trace and the reductions and four barriers; 88 VGPRs and 24.6 KiB of LDS leave room for five workgroups a CU, which hide each
// other's barriers and loads.  A wavefront per row (as in hint_curve_kernel) would pay only for P, M <~ 128.  Untuned: DESIGN section 14.
#include "hint_pointset.hpp"

namespace hint {
constexpr int HD_MAX_WG = 1280;                 // the grid cap: 256 CUs x 5 workgroups (88 VGPRs: 5 wavefronts a SIMD)
}

__global__ __launch_bounds__(256) void hint_hausdorff_kernel(const float* __restrict__ x, const float* __restrict__ b_points,
                                                             int n, int K, int P, const float* __restrict__ a_points,
                                                             const long long* __restrict__ a_offsets,
                                                             const float* __restrict__ a_params, long long T,
                                                             float* __restrict__ max_h, float* __restrict__ avg_h,
                                                             float* __restrict__ chamfer, float* __restrict__ points) {
    using namespace hint;
    __shared__ float2 tw[PS_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[PS_MAX_P];
    __shared__ float2 Ap[PS_TILE];
    __shared__ float coef[4 * PS_MAX_K + 4];
    __shared__ ps_pose pose;
    __shared__ double red[PS_WAVES][4];
    __shared__ float redm[PS_WAVES];
    const int t = threadIdx.x, C = 4 * K;
    const bool traced = x != nullptr, with_prm = a_params != nullptr, with_dist = max_h || avg_h || chamfer;
    if (traced) ps_twiddles(tw, P, t);
    const float qnan = __int_as_float(0x7fc00000);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        // ---- the row's template range; a ragged row whose range is not 1..4096 points inside a_points is a bad row ----
        long long o0 = 0, o1 = T;
        if (a_offsets) {
            o0 = a_offsets[row];
            o1 = a_offsets[row + 1];
        }
        const bool bad = o0 < 0 || o1 > T || o1 - o0 < 1 || o1 - o0 > PS_MAX_M;
        const int M = bad ? 0 : (int)(o1 - o0);
        if (traced && t < C) coef[t] = x[(size_t)row * C + t];
        if (with_prm && with_dist && t == 0) ps_stage_pose(a_params + 4 * (size_t)row, &pose);
        __syncthreads();
        ps_stage_curve(Bp, tw, coef, traced, b_points, points, (size_t)row, K, P, t);
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
        __syncthreads();                                     // Bp is whole
        float bx[PS_PER], by[PS_PER];
        ps_own_points(Bp, P, t, bx, by);
        ps_part part = ps_two_sided(Ap, Bp, M, P, t, bx, by, [&](int g) {
            float2 a;
            ps_load_point(a, a_points + 2 * (size_t)(o0 + g));
            if (with_prm) a = ps_place(a, pose);
            return a;
        });
        double s[4] = {part.a_rt, part.a_sq, part.b_rt, part.b_sq};
        ps_block_reduce(s, part.mx, red, redm, t);           // (past its barrier the next row may overwrite Bp, Ap, pose)
        if (t == 0) {
            if (max_h) max_h[row] = __fsqrt_rn(part.mx);
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
    if (ps_check_sizes(who, n_rows, n_coeffs, n_points, traced)) return 1;
    if (max_template_points < 1 || max_template_points > PS_MAX_M)
        return fail("%s: a row's template must hold 1..%d points (got %lld)", who, PS_MAX_M, (long long)max_template_points);
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
    const int64_t out[5] = {capped_grid(n_rows, 0, HD_MAX_WG), 1, PS_TILE, HD_MAX_WG, (max_template_points + PS_TILE - 1) / PS_TILE};
    return out[field];
}

int hint_hausdorff_run(const hint_hausdorff_desc* desc, void* stream) {
    const char* who = "hint_hausdorff_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->a_points) return fail("%s: a_points is null", who);
    if (ps_check_source(who, desc->x, desc->b_points, "the curve needs a source")) return 1;
    if (desc->points && desc->b_points) return fail("%s: points is an output of the traced source only (b_points is given)", who);
    if (!desc->max_h && !desc->avg_h && !desc->chamfer && !desc->points)
        return fail("%s: no output requested (max_h, avg_h, chamfer and points are all null)", who);
    if (desc->n_template < 1) return fail("%s: n_template must be >= 1 (got %lld)", who, (long long)desc->n_template);
    // a shared template is a row's template; ragged rows are checked by the kernel, their total here
    const int64_t row_max = desc->a_offsets ? 1 : desc->n_template;
    if (hd_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, row_max, desc->x != nullptr)) return 1;
    if (desc->a_offsets && desc->n_template > desc->n_rows * (int64_t)PS_MAX_M)
        return fail("%s: n_template = %lld is more than n_rows x %d points", who, (long long)desc->n_template, PS_MAX_M);
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"x", desc->x, 3}, {"b_points", desc->b_points, 3}, {"a_points", desc->a_points, 3},
                               {"a_offsets", desc->a_offsets, 7}, {"a_params", desc->a_params, 3}, {"max_h", desc->max_h, 3},
                               {"avg_h", desc->avg_h, 3}, {"chamfer", desc->chamfer, 3}, {"points", desc->points, 3}}))
        return 1;
    const int grid = capped_grid(desc->n_rows, desc->max_groups, HD_MAX_WG);
    hipLaunchKernelGGL(hint_hausdorff_kernel, dim3(grid), dim3(PS_THREADS), 0, (hipStream_t)stream, desc->x, desc->b_points,
                       (int)desc->n_rows, desc->x ? desc->n_coeffs : 1, desc->n_points, desc->a_points,
                       (const long long*)desc->a_offsets, desc->a_params, (long long)desc->n_template, desc->max_h, desc->avg_h,
                       desc->chamfer, desc->points);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
