// The plus shape's fit loss and its max / avg Hausdorff distance to a curve (gfx950): the plus-shape counterpart of hint_hausdorff.hip.
//
// Reference being replaced (read-only): eval_shapes.py:82-95 calls, per row in a Python loop, points_to_plus_loss
// (best_shape_fit.py:54-65: plus_segments_from_params :26-50, squared_dists_points_to_line_segment :15-22 per segment, a cdist for
// the corner term) and max_and_avg_hausdorff_distance_plus_shape (best_shape_fit.py:153-156: densify_polyline, data.py:176-186, an
// np.linspace per edge, then the [P, M, 2] numpy tensor of :143-149).
// The contract - vertices, placement, the fp32 order of every operation, the outline's counts and points, the outputs and the
// association of the double sums - is stated in include/hint_amd.h (hint_plus_desc).
//
// hint_plus_kernel: the shape of hint_hausdorff_kernel - a persistent grid of G workgroups of 256 threads; workgroup w takes rows
// w, w + G, ... one at a time; the twiddle table once per workgroup - built from the same core (hint_pointset.hpp: the trace, the
// two-pass walk, the reductions), with a template that exists nowhere in memory:
//   - per row (the geometry: hint_plusgeom.hpp, shared with hint_plusfit.hip), thread 0 turns the 9 parameters into the 8 clamped
//     coordinates, cs, sn (double sincos, not inlined) and a finite flag in LDS; lanes 0..11 of wavefront 0 then each take one
//     segment: its two local vertices (picked from the 8 coordinates by two packed index tables), the keep bit, the two placed
//     vertices (written to `segments`), the loss's constants (a, n, L) and the outline's count (one double division); a ballot
//     gives `keep`, a 12-lane shuffle scan the prefix sums of the counts;
//   - B is traced or loaded into LDS (ps_stage_curve); each thread then holds its <= 4 B points in registers;
//   - loss: the thread walks the kept segments (constants from LDS, every read a wavefront broadcast) over its own B points and
//     keeps min_s d^2; the corner term is 12 workgroup-wide minima (thread, six xor-shuffles, four wavefronts through LDS);
//   - Hausdorff: ps_two_sided over LDS tiles of 1024 outline points, with a tile filler that generates them: the point's edge by
//     a 4-step search in the 16 padded prefix sums, one fp32 division for t, two products and two fmas;
//   - ps_block_reduce over the two root sums, the segment term and the maximum.
// Nothing is carried from row to row and no output is read back.  No float atomics, no counters, no workspace.  Untuned defaults
// (tile size, points per thread, grid cap, prefix search, the serial parameter stage): DESIGN section 15.
#include "hint_plusgeom.hpp"

namespace hint {

constexpr int PL_MAX_WG = 1024;                 // the grid cap: 256 CUs x 4 workgroups (113 VGPRs: 4 wavefronts a SIMD)
constexpr double PL_Q_CAP = 8192.0;             // a quotient is cut here before it becomes an integer (12 x 8192 fits an int)

}  // namespace hint

__global__ __launch_bounds__(256) void hint_plus_kernel(const float* __restrict__ x, const float* __restrict__ b_points, int n,
                                                        int K, int P, const float* __restrict__ params, float max_dist,
                                                        float* __restrict__ segments, int* __restrict__ keep,
                                                        int* __restrict__ counts, float* __restrict__ loss,
                                                        float* __restrict__ max_h, float* __restrict__ avg_h) {
    using namespace hint;
    __shared__ float2 tw[PS_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[PS_MAX_P];
    __shared__ float2 Ap[PS_TILE];
    __shared__ float coef[4 * PS_MAX_K + 4];
    __shared__ pl_row rw;
    __shared__ double red[PS_WAVES][3];                      // roots of mA, roots of mB, the segment term
    __shared__ float redm[PS_WAVES];
    __shared__ float redc[PS_WAVES][12];                     // the corner minima
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, C = 4 * K;
    const bool traced = x != nullptr, with_h = max_h || avg_h, with_curve = with_h || loss;
    if (traced && with_curve) ps_twiddles(tw, P, t);
    const float qnan = __int_as_float(0x7fc00000);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        if (traced && with_curve && t < C) coef[t] = x[(size_t)row * C + t];
        if (t == 0) pl_stage_params(params + 9 * (size_t)row, &rw);
        __syncthreads();
        // ---- the twelve segments, one a lane of wavefront 0 ----
        if (wv == 0) {
            float2 w0, w1;
            bool differ;
            pl_segment(rw, l < 12 ? l : 0, w0, w1, differ);
            const bool kept = l < 12 && differ;
            // the outline's count of this edge: the quotient in double, cut before it becomes an integer
            const double ex = fabs((double)w1.x - (double)w0.x), ey = fabs((double)w1.y - (double)w0.y);
            const double q = (ex > ey ? ex : ey) / (double)max_dist;
            const bool wild = l < 12 && !(isfinite(w0.x) && isfinite(w0.y) && isfinite(w1.x) && isfinite(w1.y) && isfinite(q));
            const double qc = q < PL_Q_CAP ? q : PL_Q_CAP;   // (a NaN goes to the cap as well)
            int cnt = (int)rint(qc);
            cnt = kept ? (cnt < 1 ? 1 : cnt) : 0;
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (l >= d) incl += up;
            }
            const unsigned long long kmask = __ballot(kept), wmask = __ballot(wild);
            const int M = __shfl(incl, 11, 64);
            const bool bad = wmask != 0 || rw.finite == 0 || M < 1 || M > PS_MAX_M;
            if (l < 12) {
                pl_store_segment(rw, l, w0, w1);
                rw.pre[l] = incl - cnt;
                if (segments) {
                    float* sp = segments + 4 * ((size_t)row * 12 + l);
                    sp[0] = w0.x;
                    sp[1] = w0.y;
                    sp[2] = w1.x;
                    sp[3] = w1.y;
                }
                if (counts) counts[(size_t)row * 12 + l] = bad ? -1 : cnt;
            } else if (l < 16) {
                rw.pre[l] = l == 12 ? M : 0x7fffffff;
            }
            if (l == 0) {
                rw.keep = (int)(kmask & 0xfff);
                rw.nk = __popcll(kmask & 0xfff);
                rw.M = M;
                rw.bad = bad ? 1 : 0;
                if (keep) keep[row] = (int)(kmask & 0xfff);
            }
        }
        if (!with_curve) {                                   // segments / keep / counts alone: the curve is not read
            __syncthreads();                                 // the next row overwrites rw
            continue;
        }
        ps_stage_curve(Bp, tw, coef, traced, b_points, nullptr, (size_t)row, K, P, t);
        __syncthreads();                                     // Bp and rw are whole
        float bx[PS_PER], by[PS_PER];
        ps_own_points(Bp, P, t, bx, by);
        const int kmask = rw.keep, M = rw.M;
        const bool bad = rw.bad != 0;
        double s_seg = 0.0;
        if (loss) {
            // ---- the segment term: min over the kept segments of the squared distance to the segment ----
            float ms[PS_PER];
            ps_no_minima(ms);
#pragma unroll 1
            for (int s = 0; s < 12; ++s) {
                if (!((kmask >> s) & 1)) continue;
                const float2 a = rw.a[s], nn = rw.n[s];
                const float L = rw.L[s];
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    const float apx = __fsub_rn(a.x, bx[c]), apy = __fsub_rn(a.y, by[c]);
                    const float len = fmaxf(0.f, fminf(L, -__fmaf_rn(apy, nn.y, __fmul_rn(apx, nn.x))));
                    const float vx = __fmaf_rn(len, nn.x, apx), vy = __fmaf_rn(len, nn.y, apy);
                    ms[c] = fminf(ms[c], __fmaf_rn(vy, vy, __fmul_rn(vx, vx)));
                }
            }
#pragma unroll
            for (int c = 0; c < PS_PER; ++c)
                if (t + PS_THREADS * c < P) s_seg += (double)ms[c];
            // ---- the corner term: for each vertex the nearest curve point (a repeated slot does not change a minimum) ----
#pragma unroll 1
            for (int s = 0; s < 12; ++s) {
                const float2 w = rw.W[s];
                float m = INFINITY;
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    const float dx = __fsub_rn(w.x, bx[c]), dy = __fsub_rn(w.y, by[c]);
                    m = fminf(m, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
                }
                m = ps_wave_min(m);
                if (l == 0) redc[wv][s] = m;
            }
        }
        ps_part part;
        if (with_h && !bad) {
            // outline point g lies on the edge s with pre[s] <= g < pre[s + 1]
            part = ps_two_sided(Ap, Bp, M, P, t, bx, by, [&](int g) {        // (M <= 4096 here)
                int s = 0;
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1)
                    if (rw.pre[s + d] <= g) s += d;          // (s + d <= 15; pre[12] = M > g, so s <= 11)
                const int first = rw.pre[s], ec = rw.pre[s + 1] - first;
                const float2 e = rw.W[s], nx = rw.W[s + 1];
                float2 a = e;
                if (ec > 1) {
                    const float tq = __fdiv_rn((float)(g - first), (float)(ec - 1)), om = __fsub_rn(1.f, tq);
                    a.x = __fmaf_rn(tq, nx.x, __fmul_rn(om, e.x));
                    a.y = __fmaf_rn(tq, nx.y, __fmul_rn(om, e.y));
                }
                return a;
            });
        }
        double s[3] = {part.a_rt, part.b_rt, s_seg};
        ps_block_reduce(s, part.mx, red, redm, t);           // (past its barrier the next row may overwrite Bp, Ap, coef, rw)
        if (t == 0) {
            if (max_h) max_h[row] = bad ? qnan : __fsqrt_rn(part.mx);
            if (avg_h) avg_h[row] = bad ? qnan : (float)((s[0] + s[1]) / (double)(M + P));
            if (loss) {
                double sc = 0.0;
                for (int k = 0; k < 12; ++k) {
                    if (!((kmask >> k) & 1)) continue;
                    float m = redc[0][k];
                    for (int w = 1; w < PS_WAVES; ++w) m = fminf(m, redc[w][k]);
                    sc += (double)m;
                }
                loss[2 * (size_t)row] = (float)(s[2] / (double)P);
                loss[2 * (size_t)row + 1] = (float)(sc / (double)rw.nk);
            }
        }
    }
}

// ---- the C ABI ----
using namespace hint;

extern "C" {

size_t hint_plus_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points) {
    // n_coeffs = 0 stands for the given-points source, which has no coefficients
    if (ps_check_sizes("hint_plus_workspace_bytes", n_rows, n_coeffs, n_points, n_coeffs != 0, true)) return 0;
    last_error_ref().clear();
    return 0;                                                // the kernel needs none
}

int64_t hint_plus_geometry(int64_t n_rows, int32_t n_points, int32_t field) {
    if (ps_check_sizes("hint_plus_geometry", n_rows, 1, n_points, false, true)) return -1;
    if (field < 0 || field > 4) {
        fail("hint_plus_geometry: no field %d (0 workgroups, 1 rows per workgroup at a time, 2 outline points per LDS tile, "
             "3 the grid cap, 4 the most outline points of a row)", field);
        return -1;
    }
    const int64_t out[5] = {capped_grid(n_rows, 0, PL_MAX_WG), 1, PS_TILE, PL_MAX_WG, PS_MAX_M};
    return out[field];
}

int hint_plus_run(const hint_plus_desc* desc, void* stream) {
    const char* who = "hint_plus_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->params) return fail("%s: params is null", who);
    if (!desc->segments && !desc->keep && !desc->counts && !desc->loss && !desc->max_h && !desc->avg_h)
        return fail("%s: no output requested (segments, keep, counts, loss, max_h and avg_h are all null)", who);
    const bool with_curve = desc->loss || desc->max_h || desc->avg_h;
    if (ps_check_source(who, desc->x, desc->b_points, with_curve ? "loss, max_h and avg_h need the curve" : nullptr)) return 1;
    if (ps_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, desc->x != nullptr,
                       with_curve || desc->x || desc->b_points))
        return 1;
    if (!(desc->max_dist > 0.f) || !std::isfinite(desc->max_dist))
        return fail("%s: max_dist must be finite and > 0 (got %g)", who, (double)desc->max_dist);
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"x", desc->x, 3}, {"b_points", desc->b_points, 3}, {"params", desc->params, 3},
                               {"segments", desc->segments, 3}, {"keep", desc->keep, 3}, {"counts", desc->counts, 3},
                               {"loss", desc->loss, 3}, {"max_h", desc->max_h, 3}, {"avg_h", desc->avg_h, 3}}))
        return 1;
    const int grid = capped_grid(desc->n_rows, desc->max_groups, PL_MAX_WG);
    // without a curve output the kernel reads no curve: P = 2 keeps its (unused) sizes in range
    hipLaunchKernelGGL(hint_plus_kernel, dim3(grid), dim3(PS_THREADS), 0, (hipStream_t)stream, with_curve ? desc->x : nullptr,
                       with_curve ? desc->b_points : nullptr, (int)desc->n_rows, with_curve && desc->x ? desc->n_coeffs : 1,
                       with_curve ? desc->n_points : 2, desc->params, desc->max_dist, desc->segments, desc->keep, desc->counts,
                       desc->loss, desc->max_h, desc->avg_h);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
