// IoU / DICE of a traced curve and a fitted shape (gfx950): the area of the intersection of two polygons without clipping, and
// the count of the curve's self-crossings.
//
// Reference being replaced (read-only): run_experiments.py:144-167 and eval_shapes.py:82-103 call, per row in a Python loop,
// iou_and_dice_lens_shape (best_shape_fit.py:265-271) or iou_and_dice_plus_shape (best_shape_fit.py:133-139): two shapely polygons,
// buffer(0), intersection.area and union.area on the host.
// The contract - the edges, the baseline, the fp32 order of a term, the crossing test, the outputs and the association of the
// double sums - is stated in include/hint_amd.h (hint_overlap_desc).  In short, per row: C = the curve's P points, closed; T = the
// template's M vertices, closed; y0 = the smallest y of both; every edge is (x0, h0, x1, h1) with h = y - y0 >= 0;
// I = | sum over the P x M pairs of edges of sign_e sign_f (the integral over the common x-interval of the smaller height) |.
//
// hint_overlap_kernel: the shape of hint_plus_kernel - a persistent grid of G workgroups of 256 threads; workgroup w takes rows
// w, w + G, ... one at a time; the twiddle table once per workgroup - on the core of hint_pointset.hpp (the trace, the staging of
// the curve, the placement, the reductions) and the plus geometry of hint_plusgeom.hpp:
//   - per row: the 4K coefficients and the pose (or the plus parameters) go to LDS; the curve is traced or loaded into LDS
//     (ps_stage_curve); with plus_params, lanes 0..11 place the twelve vertices (pl_segment);
//   - one pass over the thread's curve points and the template's vertices (loaded and placed, or read from LDS) gives the row's
//     minimum y and whether everything is finite: a workgroup minimum and a workgroup OR through LDS;
//   - each thread holds its <= 4 curve edges (point i and its successor from LDS, the reciprocal of the x-difference) in
//     registers;
//   - the template passes through LDS in tiles of 1024 edges: 1025 vertices (the seam vertex included, so the closing edge and
//     every seam edge belong to exactly one tile) and the 1024 reciprocals; the thread that fills an edge adds its area term;
//     then every thread walks the tile's edges (each read a wavefront broadcast) against its own;
//   - the crossing count: the thread's edges against every curve edge of higher index that shares no vertex index with it;
//   - ps_block_reduce over the two area sums, the pair sum and the count (a count below 2^53 is exact in a double).
// Nothing is carried from row to row and no output is read back.  No float atomics, no counters, no workspace.  Untuned defaults
// (tile size, edges per thread, grid cap, the idle threads of a short curve, the second placement of a vertex): DESIGN section 18.
#include "hint_plusgeom.hpp"

namespace hint {

constexpr int OV_MAX_WG = 768;                  // the grid cap: 256 CUs x 3 workgroups (155 VGPRs: 3 wavefronts a SIMD)
constexpr int OV_MIN_P = 3, OV_MIN_M = 3;       // a polygon has three vertices

}  // namespace hint

// the height of the edge (x0, h0) - (x1, h1), r = 1 / (x1 - x0), at xq inside the edge's x-range: both weights are quotients of
// differences that have the sign of x1 - x0, cut at 1, so the result is a sum of non-negative products; it is then cut to the
// edge's own heights, whatever the slope
__device__ __forceinline__ float ov_height(float x0, float h0, float x1, float h1, float r, float xq) {
    const float u1 = fminf(__fmul_rn(__fsub_rn(xq, x0), r), 1.f);
    const float u0 = fminf(__fmul_rn(__fsub_rn(x1, xq), r), 1.f);
    const float h = __fmaf_rn(u1, h1, __fmul_rn(u0, h0));
    return fmaxf(fminf(h0, h1), fminf(fmaxf(h0, h1), h));
}

// the signed term of the curve edge e and the template edge f
__device__ __forceinline__ float ov_term(float ex0, float eh0, float ex1, float eh1, float er, float fx0, float fh0, float fx1,
                                         float fh1, float fr) {
    const float a = fmaxf(fminf(ex0, ex1), fminf(fx0, fx1)), b = fminf(fmaxf(ex0, ex1), fmaxf(fx0, fx1));
    if (!(a < b)) return 0.f;                                // no common interval (an edge with x1 == x0 has none with anything)
    const float w = __fsub_rn(b, a);
    const float ea = ov_height(ex0, eh0, ex1, eh1, er, a), eb = ov_height(ex0, eh0, ex1, eh1, er, b);
    const float fa = ov_height(fx0, fh0, fx1, fh1, fr, a), fb = ov_height(fx0, fh0, fx1, fh1, fr, b);
    const float da = __fsub_rn(ea, fa), db = __fsub_rn(eb, fb);
    const float ma = fminf(ea, fa), mb = fminf(eb, fb);
    float sum;
    if ((da < 0.f && db > 0.f) || (da > 0.f && db < 0.f)) {  // the heights cross inside: split there
        const float den = __fsub_rn(da, db);
        const float ta = __fdiv_rn(da, den), tb = __fdiv_rn(-db, den);       // the crossing's share of w, and the rest
        const float hc = __fmaf_rn(ta, eb, __fmul_rn(tb, ea));
        sum = __fadd_rn(hc, __fmaf_rn(ta, ma, __fmul_rn(tb, mb)));
    } else {
        sum = __fadd_rn(ma, mb);
    }
    const float v = __fmul_rn(__fmul_rn(0.5f, w), sum);
    return ((ex1 < ex0) != (fx1 < fx0)) ? -v : v;
}

// the orientation determinant of (p, q, r)
__device__ __forceinline__ float ov_orient(const float2& p, const float2& q, const float2& r) {
    const float ux = __fsub_rn(q.x, p.x), uy = __fsub_rn(q.y, p.y), vx = __fsub_rn(r.x, p.x), vy = __fsub_rn(r.y, p.y);
    return __fmaf_rn(ux, vy, -__fmul_rn(uy, vx));
}

__device__ __forceinline__ bool ov_opposite(float a, float b) { return (a < 0.f && b > 0.f) || (a > 0.f && b < 0.f); }

// the thread's NC edges against the n edges of a tile: Ap[j], Ap[j + 1] the vertices and Ar[j] the reciprocal of edge j; the
// terms are added in double, edge j ascending and within it the thread's own edges ascending
template <int NC>
__device__ __forceinline__ void ov_walk(const float2* Ap, const float* Ar, int n, const float (&ex0)[hint::PS_PER],
                                        const float (&eh0)[hint::PS_PER], const float (&ex1)[hint::PS_PER],
                                        const float (&eh1)[hint::PS_PER], const float (&er)[hint::PS_PER], double& acc) {
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        const float2 f0 = Ap[j], f1 = Ap[j + 1];
        const float fr = Ar[j];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc += (double)ov_term(ex0[c], eh0[c], ex1[c], eh1[c], er[c], f0.x, f0.y, f1.x, f1.y, fr);
    }
}

__global__ __launch_bounds__(256) void hint_overlap_kernel(const float* __restrict__ x, const float* __restrict__ b_points, int n,
                                                           int K, int P, const float* __restrict__ a_points,
                                                           const long long* __restrict__ a_offsets,
                                                           const float* __restrict__ a_params, long long T,
                                                           const float* __restrict__ plus_params, float* __restrict__ areas,
                                                           float* __restrict__ iou, float* __restrict__ dice,
                                                           int* __restrict__ crossings) {
    using namespace hint;
    __shared__ float2 tw[PS_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[PS_MAX_P];
    __shared__ float2 Ap[PS_TILE + 1];                       // (x, h) of a tile's vertices, the seam vertex last
    __shared__ float Ar[PS_TILE];                            // 1 / (x1 - x0) of its edges
    __shared__ float coef[4 * PS_MAX_K + 4];
    __shared__ ps_pose pose;
    __shared__ pl_row rw;
    __shared__ double red[PS_WAVES][4];                      // area of T, area of C, the pair sum, the crossings
    __shared__ float redm[PS_WAVES];
    __shared__ float redy[PS_WAVES];                         // the minimum y
    __shared__ int redf[PS_WAVES];                           // something is not finite
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, C = 4 * K;
    const bool traced = x != nullptr, with_plus = plus_params != nullptr, with_prm = a_params != nullptr;
    const bool with_t = areas || iou || dice;                // without them the template is not read
    if (traced) ps_twiddles(tw, P, t);
    const float qnan = __int_as_float(0x7fc00000);
    const int nc = (P + PS_THREADS - 1) / PS_THREADS;
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        // ---- the row's template range; a ragged row whose range is not 3..4096 points inside a_points is a bad row ----
        long long o0 = 0, o1 = T;
        if (with_t && !with_plus && a_offsets) {
            o0 = a_offsets[row];
            o1 = a_offsets[row + 1];
        }
        const bool bad_range = with_t && !with_plus && (o0 < 0 || o1 > T || o1 - o0 < OV_MIN_M || o1 - o0 > PS_MAX_M);
        const int M = !with_t || bad_range ? 0 : with_plus ? 12 : (int)(o1 - o0);
        if (traced && t < C) coef[t] = x[(size_t)row * C + t];
        if (with_t && t == 0) {
            if (with_plus)
                pl_stage_params(plus_params + 9 * (size_t)row, &rw);
            else if (with_prm)
                ps_stage_pose(a_params + 4 * (size_t)row, &pose);
        }
        __syncthreads();
        ps_stage_curve(Bp, tw, coef, traced, b_points, nullptr, (size_t)row, K, P, t);
        if (with_t && with_plus && t < 12) {                 // the twelve placed vertices, one a lane
            float2 w0, w1;
            bool differ;
            pl_segment(rw, t, w0, w1, differ);
            rw.W[t] = w0;
            if (t == 11) rw.W[12] = w1;
        }
        __syncthreads();                                     // Bp and rw.W are whole
        // vertex g of the row's template, placed (0 <= g < M)
        auto vert = [&](int g) {
            float2 a;
            if (with_plus) {
                a = rw.W[g];
            } else {
                ps_load_point(a, a_points + 2 * (size_t)(o0 + g));
                if (with_prm) a = ps_place(a, pose);
            }
            return a;
        };
        // ---- the smallest y of both polygons, and whether every input is finite ----
        float ymin = INFINITY;
        int wild = bad_range ? 1 : 0;
#pragma unroll 1
        for (int i = t; i < P; i += PS_THREADS) {
            const float2 p = Bp[i];
            ymin = fminf(ymin, p.y);
            wild |= !(isfinite(p.x) && isfinite(p.y));
        }
        if (with_t && with_plus && t == 0) wild |= rw.finite == 0;
        if (with_t && !with_plus && with_prm && t < 4) wild |= !isfinite(a_params[4 * (size_t)row + t]);
#pragma unroll 1
        for (int g = t; g < M; g += PS_THREADS) {
            const float2 a = vert(g);
            ymin = fminf(ymin, a.y);
            wild |= !(isfinite(a.x) && isfinite(a.y));
        }
        ymin = ps_wave_min(ymin);
        wild = __any(wild) ? 1 : 0;
        if (l == 0) {
            redy[wv] = ymin;
            redf[wv] = wild;
        }
        __syncthreads();
        const float y0 = fminf(fminf(redy[0], redy[1]), fminf(redy[2], redy[3]));
        if (redf[0] | redf[1] | redf[2] | redf[3]) {         // (the same for every thread)
            if (t == 0) {
                if (areas) areas[3 * (size_t)row] = areas[3 * (size_t)row + 1] = areas[3 * (size_t)row + 2] = qnan;
                if (iou) iou[row] = qnan;
                if (dice) dice[row] = qnan;
                if (crossings) crossings[row] = -1;
            }
            __syncthreads();                                 // the next row overwrites coef, pose, rw, Bp
            continue;
        }
        // ---- this thread's curve edges: point i and its successor; a slot past the end is an edge of no length ----
        float ex0[PS_PER], eh0[PS_PER], ex1[PS_PER], eh1[PS_PER], er[PS_PER];
        double s_c = 0.0, s_t = 0.0, s_i = 0.0;
#pragma unroll
        for (int c = 0; c < PS_PER; ++c) {
            const int i = t + PS_THREADS * c;
            const int i0 = i < P ? i : P - 1;
            const float2 p = Bp[i0], q = Bp[i < P ? (i0 + 1 == P ? 0 : i0 + 1) : i0];
            ex0[c] = p.x;
            eh0[c] = __fsub_rn(p.y, y0);
            ex1[c] = q.x;
            eh1[c] = __fsub_rn(q.y, y0);
            const float dx = __fsub_rn(q.x, p.x);
            er[c] = __fdiv_rn(1.f, dx);
            if (i < P) s_c += (double)__fmul_rn(__fmul_rn(0.5f, dx), __fadd_rn(eh0[c], eh1[c]));
        }
        // ---- the template's edges, a tile at a time ----
        for (int a0 = 0; a0 < M; a0 += PS_TILE) {
            const int cnt = M - a0 < PS_TILE ? M - a0 : PS_TILE;
            if (a0) __syncthreads();                         // the walk of the tile before is done with Ap, Ar
#pragma unroll 1
            for (int i = t; i < cnt; i += PS_THREADS) {
                const int g = a0 + i;
                const float2 v0 = vert(g), v1 = vert(g + 1 == M ? 0 : g + 1);
                const float h0 = __fsub_rn(v0.y, y0), h1 = __fsub_rn(v1.y, y0), dx = __fsub_rn(v1.x, v0.x);
                Ap[i] = make_float2(v0.x, h0);
                if (i == cnt - 1) Ap[cnt] = make_float2(v1.x, h1);
                Ar[i] = __fdiv_rn(1.f, dx);
                s_t += (double)__fmul_rn(__fmul_rn(0.5f, dx), __fadd_rn(h0, h1));
            }
            __syncthreads();
            switch (nc) {                                    // (nc is the same for the whole workgroup)
                case 1: ov_walk<1>(Ap, Ar, cnt, ex0, eh0, ex1, eh1, er, s_i); break;
                case 2: ov_walk<2>(Ap, Ar, cnt, ex0, eh0, ex1, eh1, er, s_i); break;
                case 3: ov_walk<3>(Ap, Ar, cnt, ex0, eh0, ex1, eh1, er, s_i); break;
                default: ov_walk<4>(Ap, Ar, cnt, ex0, eh0, ex1, eh1, er, s_i); break;
            }
        }
        // ---- proper crossings of the curve with itself: edge i against the edges j > i + 1 (not the pair 0, P - 1) ----
        int cross = 0;
        if (crossings) {
            float2 a0p[PS_PER], a1p[PS_PER];
#pragma unroll
            for (int c = 0; c < PS_PER; ++c) {
                const int i = t + PS_THREADS * c;
                const int i0 = i < P ? i : P - 1;
                a0p[c] = Bp[i0];
                a1p[c] = Bp[i0 + 1 == P ? 0 : i0 + 1];
            }
#pragma unroll 1
            for (int j = 2; j < P; ++j) {
                const float2 b0 = Bp[j], b1 = Bp[j + 1 == P ? 0 : j + 1];
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    const int i = t + PS_THREADS * c;
                    if (i + 1 < j && !(i == 0 && j == P - 1)) {              // (then i < P)
                        const bool one = ov_opposite(ov_orient(a0p[c], a1p[c], b0), ov_orient(a0p[c], a1p[c], b1));
                        const bool two = ov_opposite(ov_orient(b0, b1, a0p[c]), ov_orient(b0, b1, a1p[c]));
                        cross += one && two ? 1 : 0;
                    }
                }
            }
        }
        double s[4] = {s_t, s_c, s_i, (double)cross};
        float mx = 0.f;
        ps_block_reduce(s, mx, red, redm, t);                // (past its barrier the next row may overwrite Bp, Ap, Ar, coef, rw)
        if (t == 0) {
            const double at = fabs(s[0]), ac = fabs(s[1]);
            const double cap = at < ac ? at : ac;
            double in = fabs(s[2]);
            in = in < cap ? in : cap;
            if (areas) {
                areas[3 * (size_t)row] = (float)at;
                areas[3 * (size_t)row + 1] = (float)ac;
                areas[3 * (size_t)row + 2] = (float)in;
            }
            if (iou) iou[row] = (float)(in / (at + ac - in));                // (0 / 0 = NaN)
            if (dice) dice[row] = (float)(2.0 * in / (at + ac));
            if (crossings) crossings[row] = (int)s[3];
        }
    }
}

// ---- the C ABI ----
using namespace hint;

static int ov_check_sizes(const char* who, int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points,
                          bool traced) {
    if (ps_check_sizes(who, n_rows, n_coeffs, n_points, traced)) return 1;
    if (n_points < OV_MIN_P) return fail("%s: n_points must be %d..%d (got %d)", who, OV_MIN_P, PS_MAX_P, n_points);
    if (max_template_points < OV_MIN_M || max_template_points > PS_MAX_M)
        return fail("%s: a row's template must hold %d..%d points (got %lld)", who, OV_MIN_M, PS_MAX_M,
                    (long long)max_template_points);
    return 0;
}

extern "C" {

size_t hint_overlap_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points) {
    // n_coeffs = 0 stands for the given-points source, which has no coefficients
    if (ov_check_sizes("hint_overlap_workspace_bytes", n_rows, n_coeffs, n_points, max_template_points, n_coeffs != 0)) return 0;
    last_error_ref().clear();
    return 0;                                                // the kernel needs none
}

int64_t hint_overlap_geometry(int64_t n_rows, int32_t n_points, int64_t max_template_points, int32_t field) {
    if (ov_check_sizes("hint_overlap_geometry", n_rows, 1, n_points, max_template_points, false)) return -1;
    if (field < 0 || field > 4) {
        fail("hint_overlap_geometry: no field %d (0 workgroups, 1 rows per workgroup at a time, 2 template edges per LDS tile, "
             "3 the grid cap, 4 tiles of the largest template)", field);
        return -1;
    }
    const int64_t out[5] = {capped_grid(n_rows, 0, OV_MAX_WG), 1, PS_TILE, OV_MAX_WG, (max_template_points + PS_TILE - 1) / PS_TILE};
    return out[field];
}

int hint_overlap_run(const hint_overlap_desc* desc, void* stream) {
    const char* who = "hint_overlap_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->areas && !desc->iou && !desc->dice && !desc->crossings)
        return fail("%s: no output requested (areas, iou, dice and crossings are all null)", who);
    const bool with_t = desc->areas || desc->iou || desc->dice;
    if (desc->a_points && desc->plus_params)
        return fail("%s: both a_points and plus_params are given (the template has one source)", who);
    if (with_t && !desc->a_points && !desc->plus_params)
        return fail("%s: a_points and plus_params are both null (areas, iou and dice need the template)", who);
    if (!desc->a_points && (desc->a_offsets || desc->a_params))
        return fail("%s: %s is given without a_points", who, desc->a_offsets ? "a_offsets" : "a_params");
    if (ps_check_source(who, desc->x, desc->b_points, "the curve needs a source")) return 1;
    // a shared template is a row's template; ragged rows are checked by the kernel, their total here
    const bool with_pts = with_t && desc->a_points;
    if (with_pts && desc->n_template < OV_MIN_M)
        return fail("%s: n_template must be >= %d (got %lld)", who, OV_MIN_M, (long long)desc->n_template);
    const int64_t row_max = with_pts && !desc->a_offsets ? desc->n_template : OV_MIN_M;
    if (ov_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, row_max, desc->x != nullptr)) return 1;
    if (with_pts && desc->a_offsets && desc->n_template > desc->n_rows * (int64_t)PS_MAX_M)
        return fail("%s: n_template = %lld is more than n_rows x %d points", who, (long long)desc->n_template, PS_MAX_M);
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"x", desc->x, 3}, {"b_points", desc->b_points, 3}, {"a_points", desc->a_points, 3},
                               {"a_offsets", desc->a_offsets, 7}, {"a_params", desc->a_params, 3},
                               {"plus_params", desc->plus_params, 3}, {"areas", desc->areas, 3}, {"iou", desc->iou, 3},
                               {"dice", desc->dice, 3}, {"crossings", desc->crossings, 3}}))
        return 1;
    const int grid = capped_grid(desc->n_rows, desc->max_groups, OV_MAX_WG);
    hipLaunchKernelGGL(hint_overlap_kernel, dim3(grid), dim3(PS_THREADS), 0, (hipStream_t)stream, desc->x, desc->b_points,
                       (int)desc->n_rows, desc->x ? desc->n_coeffs : 1, desc->n_points, with_t ? desc->a_points : nullptr,
                       with_t ? (const long long*)desc->a_offsets : nullptr, with_t ? desc->a_params : nullptr,
                       (long long)desc->n_template, with_t ? desc->plus_params : nullptr, desc->areas, desc->iou, desc->dice,
                       desc->crossings);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
