// The lens-shape fit of a curve (gfx950): the fit loss, its gradient and the whole SGD loop over several starts in one launch.
//
// Reference being replaced (read-only): run_experiments.py:150-159 calls, per row in a Python loop, fit_lens_shape_to_points
// (best_shape_fit.py:230-261): two starts of 100 autograd steps of torch's SGD (momentum 0.2, StepLR) on points_to_lens_loss
// (best_shape_fit.py:203-209) over lens_points_from_params (best_shape_fit.py:195-199), a [P, M] distance matrix per step.
// The contract - placement, the fp32 order of every operation, the selected pairs, the association of the double sums, the
// update rule and what a start and a row return - is stated in include/hint_amd.h (hint_lensfit_desc).
//
// hint_lensfit_kernel: the shape of hint_hausdorff_kernel - a persistent grid of G workgroups of 256 threads; workgroup w takes
// rows w, w + G, ... one at a time and runs the row's S starts one after the other, so the selection needs no second launch and
// no traffic between workgroups.  Built on hint_pointset.hpp: the trace, the own points, the placement, the walk in its form
// that keeps the index of the minimum, the reduction; and on hint_fit.hpp: the driver around an evaluation (the state, the trace
// record, the update rule, the selection over the starts).  This file adds the evaluation - the gradient's terms:
//   - once per workgroup: the P - 1 twiddles and the untransformed prototype (M <= 1024: one tile) to LDS;
//   - per row: the coefficients; B traced or loaded into LDS; each thread holds its <= 4 B points in registers;
//   - per step: thread 0 stages the pose of the parameters (ps_stage_pose); every thread places its <= 4 prototype points
//     (ps_place) and writes them to LDS; pass 1 walks B for them, pass 2 walks the placed prototype for the thread's B
//     points, both keeping the index of the minimum; the selected pairs' terms are recomputed in fp32 (q by ps_rotate from the
//     prototype in LDS: the same operations, the same bits) and added in double; ten double sums - the loss term and the four
//     gradient terms of either side, kept apart because the weights are applied after the sums - go through ps_block_reduce;
//     thread 0 forms the loss and the gradient, then records and takes the step (fit_step).  Three barriers a step.
// The state of a fit (parameters, momentum buffer, the two learning rates) lives in LDS and is set afresh for every start.
// Nothing is carried from row to row and no output is read back.  No float atomics, no counters, no workspace.
// Untuned defaults (a workgroup per row although at P = 100, M = 130 only 130 threads hold a point; starts in sequence): DESIGN
// section 16.
#include "hint_pointset.hpp"
#include "hint_fit.hpp"

namespace hint {
constexpr int LF_MAX_M = PS_TILE;
}

// a fit's state in LDS: p = x, y, scale, angle
struct lf_state : fit_state<4> {
    ps_pose pose;                                // of p, staged before every evaluation
};

// the terms of a selected pair (e = A_i - B_j, q = the rotated prototype point) onto five double sums
__device__ __forceinline__ void lf_add_pair(double (&s)[10], int o, float d, float ex, float ey, float2 q) {
    s[o] += (double)d;
    s[o + 1] += (double)ex;
    s[o + 2] += (double)ey;
    s[o + 3] += (double)__fmaf_rn(ey, q.y, __fmul_rn(ex, q.x));
    s[o + 4] += (double)__fmaf_rn(ey, q.x, -__fmul_rn(ex, q.y));
}

__global__ __launch_bounds__(256) void hint_lensfit_kernel(const float* __restrict__ x, const float* __restrict__ b_points, int n,
                                                           int K, int P, const float* __restrict__ a_points, int M,
                                                           const float* __restrict__ starts, int S, int n_steps, double lr0,
                                                           double alr0, double gamma, float momentum, double weight,
                                                           float* __restrict__ params, float* __restrict__ loss,
                                                           int* __restrict__ best, float* __restrict__ all_params,
                                                           float* __restrict__ all_loss, float* __restrict__ grad,
                                                           float* __restrict__ trace) {
    using namespace hint;
    __shared__ float2 tw[PS_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[PS_MAX_P];
    __shared__ float2 A0[LF_MAX_M];                          // the prototype as given
    __shared__ float2 Ap[LF_MAX_M];                          // ... placed by the step's parameters
    __shared__ float coef[4 * PS_MAX_K + 4];
    __shared__ lf_state st;
    __shared__ double red[PS_WAVES][10];
    __shared__ float redm[PS_WAVES];
    const int t = threadIdx.x, C = 4 * K;
    const bool traced = x != nullptr;
    const int ncA = (M + PS_THREADS - 1) / PS_THREADS, ncB = (P + PS_THREADS - 1) / PS_THREADS;
    const int evals = fit_evals(n_steps);
    if (traced) ps_twiddles(tw, P, t);
    for (int i = t; i < M; i += PS_THREADS) ps_load_point(A0[i], a_points + 2 * (size_t)i);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        if (traced && t < C) coef[t] = x[(size_t)row * C + t];
        __syncthreads();                                     // coef (and, the first time, tw and A0) are whole
        ps_stage_curve(Bp, tw, coef, traced, b_points, nullptr, (size_t)row, K, P, t);
        __syncthreads();                                     // Bp is whole
        float bx[PS_PER], by[PS_PER];
        ps_own_points(Bp, P, t, bx, by);
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            const size_t rs = (size_t)row * S + s;
            if (t == 0) {
                fit_begin(st, starts, rs, lr0, alr0);
                ps_stage_pose(st.p, &st.pose);
            }
            float L = 0.f, g[4] = {0.f, 0.f, 0.f, 0.f};      // of the last evaluation (thread 0)
#pragma unroll 1
            for (int it = 0; it < evals; ++it) {
                __syncthreads();                             // st is staged; the walks of the step before are done with Ap
                const ps_pose ps = st.pose;
                // ---- place: this thread's prototype points; a slot past the end repeats the last point and is not counted ----
                float ax[PS_PER], ay[PS_PER];
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    const int i = t + PS_THREADS * c;
                    const float2 a = ps_place(A0[i < M ? i : M - 1], ps);
                    ax[c] = a.x;
                    ay[c] = a.y;
                    if (i < M) Ap[i] = a;
                }
                __syncthreads();                             // Ap is whole
                double sm[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) sm[k] = 0.0;
                {   // ---- pass 1: mA of this thread's A points, and where ----
                    float m[PS_PER];
                    int at[PS_PER] = {0, 0, 0, 0};
                    ps_no_minima(m);
                    ps_scan_arg_n(ncA, Bp, P, ax, ay, m, at);
#pragma unroll
                    for (int c = 0; c < PS_PER; ++c) {
                        const int i = t + PS_THREADS * c;
                        if (i < M) {                         // (then c < ncA)
                            const float2 b = Bp[at[c]];
                            const float ex = __fsub_rn(ax[c], b.x), ey = __fsub_rn(ay[c], b.y);
                            lf_add_pair(sm, 5, __fmaf_rn(ey, ey, __fmul_rn(ex, ex)), ex, ey, ps_rotate(A0[i], ps.cs, ps.sn));
                        }
                    }
                }
                {   // ---- pass 2: mB of this thread's B points, and where ----
                    float m[PS_PER];
                    int at[PS_PER] = {0, 0, 0, 0};
                    ps_no_minima(m);
                    ps_scan_arg_n(ncB, Ap, M, bx, by, m, at);
#pragma unroll
                    for (int c = 0; c < PS_PER; ++c) {
                        if (t + PS_THREADS * c < P) {        // (then c < ncB)
                            const float2 a = Ap[at[c]];
                            const float ex = __fsub_rn(a.x, bx[c]), ey = __fsub_rn(a.y, by[c]);
                            lf_add_pair(sm, 0, __fmaf_rn(ey, ey, __fmul_rn(ex, ex)), ex, ey, ps_rotate(A0[at[c]], ps.cs, ps.sn));
                        }
                    }
                }
                float mx = 0.f;
                ps_block_reduce(sm, mx, red, redm, t);       // (its barrier ends the walks of this step)
                if (t == 0) {
                    // sm[0..4]: over the P pairs of B; sm[5..9]: over the M pairs of A - loss term, x, y, scale, angle terms
                    const double dP = (double)P, dM = (double)M;
                    L = (float)(sm[0] / dP + weight * (sm[5] / dM));
                    g[0] = (float)(2.0 * (sm[1] / dP + weight * (sm[6] / dM)));
                    g[1] = (float)(2.0 * (sm[2] / dP + weight * (sm[7] / dM)));
                    g[2] = (float)(2.0 * (sm[3] / dP + weight * (sm[8] / dM)));
                    g[3] = (float)(2.0 * (double)ps.scale * (sm[4] / dP + weight * (sm[9] / dM)));
                    if (n_steps > 0) {
                        fit_step(st, trace, rs * (size_t)n_steps + it, it, L, g, momentum, gamma);
                        if (it + 1 < evals) ps_stage_pose(st.p, &st.pose);
                    }
                }
            }
            if (t == 0) fit_close_start(st, s, rs, L, g, all_params, all_loss, grad);
        }
        if (t == 0) fit_close_row(st, (size_t)row, params, loss, best);
        // (the next row's first barrier comes before anything of this row in LDS is overwritten but coef, which no one reads now)
    }
}

// ---- the C ABI ----
using namespace hint;

// the sizes that come before the fit's own (fit_check, fit_check_sizes)
static int lf_check_sizes(const char* who, int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t n_template, bool traced) {
    if (ps_check_sizes(who, n_rows, n_coeffs, n_points, traced)) return 1;
    if (n_template < 1 || n_template > LF_MAX_M)
        return fail("%s: n_template must be 1..%d (got %lld)", who, LF_MAX_M, (long long)n_template);
    return 0;
}

extern "C" {

size_t hint_lensfit_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t n_template, int32_t n_starts,
                                    int32_t n_steps) {
    // n_coeffs = 0 stands for the given-points source, which has no coefficients
    const char* who = "hint_lensfit_workspace_bytes";
    if (lf_check_sizes(who, n_rows, n_coeffs, n_points, n_template, n_coeffs != 0)) return 0;
    if (fit_check_sizes(who, n_starts, n_steps)) return 0;
    last_error_ref().clear();
    return 0;                                                // the kernel needs none
}

int64_t hint_lensfit_geometry(int64_t n_rows, int32_t n_points, int32_t field) {
    if (ps_check_sizes("hint_lensfit_geometry", n_rows, 1, n_points, false, true)) return -1;
    if (field < 0 || field > 4) {
        fail("hint_lensfit_geometry: no field %d (0 workgroups, 1 rows per workgroup at a time, 2 prototype points per LDS tile, "
             "3 the grid cap, 4 the most prototype points)", field);
        return -1;
    }
    const int64_t out[5] = {capped_grid(n_rows, 0, FIT_MAX_WG), 1, PS_TILE, FIT_MAX_WG, LF_MAX_M};
    return out[field];
}

int hint_lensfit_run(const hint_lensfit_desc* desc, void* stream) {
    const char* who = "hint_lensfit_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->a_points) return fail("%s: a_points is null", who);
    if (!desc->starts) return fail("%s: starts is null", who);
    if (ps_check_source(who, desc->x, desc->b_points, "the curve needs a source")) return 1;
    if (!desc->params && !desc->loss && !desc->best && !desc->all_params && !desc->all_loss && !desc->grad && !desc->trace)
        return fail("%s: no output requested (params, loss, best, all_params, all_loss, grad and trace are all null)", who);
    if (lf_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, desc->n_template, desc->x != nullptr)) return 1;
    if (fit_check(who, desc->n_starts, desc->n_steps, desc->lr, desc->angle_lr, desc->gamma, desc->momentum, desc->trace)) return 1;
    if (!std::isfinite(desc->weight)) return fail("%s: weight must be finite (got %g)", who, desc->weight);
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"x", desc->x, 3}, {"b_points", desc->b_points, 3}, {"a_points", desc->a_points, 3},
                               {"starts", desc->starts, 3}, {"params", desc->params, 3}, {"loss", desc->loss, 3},
                               {"best", desc->best, 3}, {"all_params", desc->all_params, 3}, {"all_loss", desc->all_loss, 3},
                               {"grad", desc->grad, 3}, {"trace", desc->trace, 3}}))
        return 1;
    const int grid = capped_grid(desc->n_rows, desc->max_groups, FIT_MAX_WG);
    hipLaunchKernelGGL(hint_lensfit_kernel, dim3(grid), dim3(PS_THREADS), 0, (hipStream_t)stream, desc->x, desc->b_points,
                       (int)desc->n_rows, desc->x ? desc->n_coeffs : 1, desc->n_points, desc->a_points, (int)desc->n_template,
                       desc->starts, desc->n_starts, desc->n_steps, desc->lr, desc->angle_lr, desc->gamma, (float)desc->momentum,
                       desc->weight, desc->params, desc->loss, desc->best, desc->all_params, desc->all_loss, desc->grad,
                       desc->trace);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
