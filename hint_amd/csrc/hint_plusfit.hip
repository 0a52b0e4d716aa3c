// The plus-shape fit of a curve (gfx950): the fit loss, its gradient by the nine parameters and the whole SGD loop over several
// starts in one launch - the plus-shape counterpart of hint_lensfit.hip.
//
// Reference being replaced (read-only): eval_shapes.py:85-87 calls, per row in a Python loop, fit_plus_shape_to_points
// (best_shape_fit.py:93-129): up to nine starts of 400 autograd steps of torch's SGD (momentum 0.2, StepLR) on points_to_plus_loss
// (best_shape_fit.py:54-65) with a corner weight that decays to 0, stopping at the first start whose loss is below 0.005.
// The contract - the fp32 order of every operation, the selected segment and corner point, t, the association of the double sums,
// the clamp-tie rule, the schedule, the early stop, the selection and what a start that did not run holds - is stated in
// include/hint_amd.h (hint_plusfit_desc).
//
// hint_plusfit_kernel: the shape of hint_lensfit_kernel - a persistent grid of G workgroups of 256 threads; workgroup w takes rows
// w, w + G, ... one at a time and runs the row's S starts one after the other.  Built on hint_pointset.hpp (the trace, the own
// points, the reduction), hint_plusgeom.hpp (the row's geometry: the operations and the bits of hint_plus_kernel) and hint_fit.hpp
// (the driver the two fits share).  This file adds the evaluation, the weight schedule, the early stop and the not-run fill:
//   - once per workgroup: the P - 1 twiddles; per row: the coefficients; B traced or loaded into LDS; each thread holds its <= 4
//     B points in registers;
//   - per step: thread 0 has staged the parameters (pl_stage_params); lanes 0..11 of wavefront 0 stage the twelve segments;
//     every thread walks the kept segments over its points in hint_plus_kernel's order and keeps the first minimum, its segment,
//     len and v; the twelve corner minima are taken as 64-bit keys (the distance's bits above the point's index: the unsigned
//     minimum is the nearest point, the lowest index among equals); per point (v, t = len / L, the segment) goes to LDS, and
//     192 threads - 8 a sum - add the products v (1 - t), v t onto the 24 vertex sums in double, in index order (no indexed
//     register array, no scratch); the segment term goes through ps_block_reduce; thread 0 adds the corner term, chains the 24
//     vertex derivatives to the nine parameters through LDS, records and takes the step (fit_step) and stages the next parameters.
//     Four barriers a step.
// The state of a fit (parameters, momentum buffer, the two learning rates) lives in LDS and is set afresh for every start.
// Nothing is carried from row to row and no output is read back.  No float atomics, no counters, no workspace.
// Untuned defaults (a workgroup per row although at P = 100 only 100 threads hold a point; the serial chain by thread 0; starts in
// sequence): DESIGN section 17.
#include "hint_plusgeom.hpp"
#include "hint_fit.hpp"

namespace hint {
constexpr int PF_NP = 9, PF_REC = 19;           // parameters; floats of a trace record (p [9], L, g [9])
}

// a fit's state in LDS
struct pf_state : fit_state<hint::PF_NP> {
    int n_run, stop;
    double sm[25];                               // the workgroup's sums of a step: the segment term, 12 vertices x (x, y)
    double gw[24];                               // dL / dW: vertex k at [2 k], [2 k + 1]
    double gc[8];                                // dL / d the clamped coordinates, in the order of PL_VX / PL_VY
};

// the nearest point's key: the squared distance's bits (>= +0, so they order as unsigned integers; a NaN's lie above +inf's and
// are never the minimum against a number) above the point's index
__device__ __forceinline__ unsigned long long pf_key(float d, int i) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
}

__device__ __forceinline__ unsigned long long pf_wave_min_key(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

// thread 0: the loss (to g[9]) and the nine derivatives (to g[0..8]) from the workgroup's sums st->sm (segment term; vertex sums
// of v (1 - t) and v t), the corner keys and the staged row.  cw: the corner weight of this evaluation.  Everything it indexes
// lives in LDS: a register array indexed by a loop counter would go to scratch
__device__ __noinline__ void pf_chain(const unsigned long long (*redk)[12], const float2* Bp, int P, const pl_row* rw,
                                         pf_state* st, double cw, float* g) {
    using namespace hint;
    const double* sm = st->sm;
    const int kmask = rw->keep, nk = rw->nk;
    const double wP = 2.0 / (double)P, wC = 2.0 * cw / (double)nk;
    double sc = 0.0;
#pragma unroll 1
    for (int k = 0; k < 12; ++k) {
        double gx = wP * sm[1 + 2 * k], gy = wP * sm[2 + 2 * k];
        if ((kmask >> k) & 1) {
            unsigned long long key = redk[0][k];
#pragma unroll 1
            for (int w = 1; w < PS_WAVES; ++w) key = redk[w][k] < key ? redk[w][k] : key;
            sc += (double)__uint_as_float((unsigned)(key >> 32));
            int j = (int)(key & 0xffffffffu);
            j = j < P ? j : 0;                               // (always: every key holds the index of a point)
            const float2 b = Bp[j], w0 = rw->W[k];
            gx += wC * (double)__fsub_rn(w0.x, b.x);
            gy += wC * (double)__fsub_rn(w0.y, b.y);
        }
        st->gw[2 * k] = gx;
        st->gw[2 * k + 1] = gy;
    }
    g[PF_NP] = (float)(sm[0] / (double)P + cw * (sc / (double)nk));
    // W = V R + (xoffset, yoffset), R = [[cs, sn], [-sn, cs]]: gV = gW R^T; d W / d angle = (-q.y, q.x), q = V R
    const double cs = (double)rw->cs, sn = (double)rw->sn;
    double gxo = 0.0, gyo = 0.0, gan = 0.0;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) st->gc[i] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 12; ++k) {
        const double gx = st->gw[2 * k], gy = st->gw[2 * k + 1];
        const int ix = (int)((PL_VX >> (4 * k)) & 15), iy = (int)((PL_VY >> (4 * k)) & 15);
        const double vx = (double)rw->c[ix], vy = (double)rw->c[iy];
        const double qx = vx * cs - vy * sn, qy = vx * sn + vy * cs;
        gxo += gx;
        gyo += gy;
        gan += gy * qx - gx * qy;
        st->gc[ix] += gx * cs + gy * sn;
        st->gc[iy] += gy * cs - gx * sn;
    }
    // the clamps: the derivative of a clamped coordinate goes to the branch that was taken, on equality to the unclamped side
    const float* pr = st->p;
    const float hxl = __fmul_rn(0.5f, pr[0]), hyl = __fmul_rn(0.5f, pr[1]);
    const float xtop = __fmul_rn(0.5f, pr[2]), yright = __fmul_rn(0.5f, pr[3]), c = 0.01f;
    const bool free_l = __fsub_rn(pr[4], hxl) <= __fsub_rn(-yright, c), free_r = __fadd_rn(pr[4], hxl) >= __fadd_rn(yright, c);
    const bool free_t = __fadd_rn(pr[5], hyl) >= __fadd_rn(xtop, c), free_b = __fsub_rn(pr[5], hyl) <= __fsub_rn(-xtop, c);
    const double* gc = st->gc;
    double gxl = 0.0, gyl = 0.0, gxw = 0.5 * gc[4] - 0.5 * gc[6], gyw = 0.5 * gc[2] - 0.5 * gc[1], gxs = 0.0, gys = 0.0;
    if (free_l) {
        gxs += gc[0];
        gxl -= 0.5 * gc[0];
    } else {
        gyw -= 0.5 * gc[0];
    }
    if (free_r) {
        gxs += gc[3];
        gxl += 0.5 * gc[3];
    } else {
        gyw += 0.5 * gc[3];
    }
    if (free_t) {
        gys += gc[5];
        gyl += 0.5 * gc[5];
    } else {
        gxw += 0.5 * gc[5];
    }
    if (free_b) {
        gys += gc[7];
        gyl -= 0.5 * gc[7];
    } else {
        gxw -= 0.5 * gc[7];
    }
    g[0] = (float)gxl;
    g[1] = (float)gyl;
    g[2] = (float)gxw;
    g[3] = (float)gyw;
    g[4] = (float)gxs;
    g[5] = (float)gys;
    g[6] = (float)gxo;
    g[7] = (float)gyo;
    g[8] = (float)gan;
}

__global__ __launch_bounds__(256) void hint_plusfit_kernel(const float* __restrict__ x, const float* __restrict__ b_points, int n,
                                                           int K, int P, const float* __restrict__ starts, int S, int n_steps,
                                                           double lr0, double alr0, double gamma, float momentum,
                                                           double corner_weight, int corner_decay, double stop_loss,
                                                           float* __restrict__ params, float* __restrict__ loss,
                                                           int* __restrict__ best, int* __restrict__ n_run,
                                                           float* __restrict__ all_params, float* __restrict__ all_loss,
                                                           float* __restrict__ grad, float* __restrict__ trace) {
    using namespace hint;
    __shared__ float2 tw[PS_MAX_P];                          // [r], r < P - 1
    __shared__ float2 Bp[PS_MAX_P];
    __shared__ float coef[4 * PS_MAX_K + 4];
    __shared__ pl_row rw;
    __shared__ pf_state st;
    __shared__ float4 pt[PS_MAX_P];                          // per curve point: v.x, v.y, t, the segment
    __shared__ double red[PS_WAVES][1];
    __shared__ float redm[PS_WAVES];
    __shared__ unsigned long long redk[PS_WAVES][12];        // the corner keys
    __shared__ float gout[PF_NP + 1];                        // thread 0's loss and gradient of the last evaluation
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, C = 4 * K;
    const bool traced = x != nullptr;
    const int evals = fit_evals(n_steps);
    const float qnan = __int_as_float(0x7fc00000);
    if (traced) ps_twiddles(tw, P, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {                  // (n <= 2^30)
        if (traced && t < C) coef[t] = x[(size_t)row * C + t];
        __syncthreads();                                     // coef (and, the first time, tw) are whole; the row before is done
        if (t == 0) {
            st.stop = 0;
            st.n_run = 0;
        }
        ps_stage_curve(Bp, tw, coef, traced, b_points, nullptr, (size_t)row, K, P, t);
        __syncthreads();                                     // Bp is whole
        float bx[PS_PER], by[PS_PER];
        ps_own_points(Bp, P, t, bx, by);
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            const size_t rs = (size_t)row * S + s;
            if (st.stop) {                                   // (the same for the whole workgroup) a start that does not run
                if (t < PF_NP) {
                    if (all_params) all_params[PF_NP * rs + t] = starts[PF_NP * rs + t];
                    if (grad) grad[PF_NP * rs + t] = qnan;
                }
                if (t == 0 && all_loss) all_loss[rs] = INFINITY;
                if (trace)
                    for (int i = t; i < PF_REC * n_steps; i += PS_THREADS) trace[PF_REC * rs * (size_t)n_steps + i] = qnan;
                continue;
            }
            if (t == 0) {
                fit_begin(st, starts, rs, lr0, alr0);
                pl_stage_params(st.p, &rw);
            }
#pragma unroll 1
            for (int it = 0; it < evals; ++it) {
                __syncthreads();                             // the parameters are staged; the step before is done with rw
                // ---- the twelve segments, one a lane of wavefront 0: hint_plus_kernel's, without the outline's counts ----
                if (wv == 0) {
                    float2 w0, w1;
                    bool differ;
                    pl_segment(rw, l < 12 ? l : 0, w0, w1, differ);
                    const unsigned long long kmask = __ballot(l < 12 && differ);
                    if (l < 12) pl_store_segment(rw, l, w0, w1);
                    if (l == 0) {
                        rw.keep = (int)(kmask & 0xfff);
                        rw.nk = __popcll(kmask & 0xfff);
                    }
                }
                __syncthreads();                             // rw is whole
                const int kmask = rw.keep;
                // ---- the segment term: the first minimum over the kept segments, and which, with its len and v ----
                float ms[PS_PER], ln[PS_PER], vxs[PS_PER], vys[PS_PER];
                int sel[PS_PER];
                ps_no_minima(ms);
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    ln[c] = vxs[c] = vys[c] = 0.f;
                    sel[c] = 0;
                }
#pragma unroll 1
                for (int k = 0; k < 12; ++k) {
                    if (!((kmask >> k) & 1)) continue;
                    const float2 a = rw.a[k], nn = rw.n[k];
                    const float L = rw.L[k];
#pragma unroll
                    for (int c = 0; c < PS_PER; ++c) {
                        const float apx = __fsub_rn(a.x, bx[c]), apy = __fsub_rn(a.y, by[c]);
                        const float len = fmaxf(0.f, fminf(L, -__fmaf_rn(apy, nn.y, __fmul_rn(apx, nn.x))));
                        const float vx = __fmaf_rn(len, nn.x, apx), vy = __fmaf_rn(len, nn.y, apy);
                        const float d = __fmaf_rn(vy, vy, __fmul_rn(vx, vx));
                        const bool lt = d < ms[c];
                        ms[c] = lt ? d : ms[c];
                        sel[c] = lt ? k : sel[c];
                        ln[c] = lt ? len : ln[c];
                        vxs[c] = lt ? vx : vxs[c];
                        vys[c] = lt ? vy : vys[c];
                    }
                }
                // each point's record to LDS: v, t = len / L and the segment (the sums over the points are taken below)
                double sm[1] = {0.0};
#pragma unroll
                for (int c = 0; c < PS_PER; ++c) {
                    const int i = t + PS_THREADS * c;
                    if (i < P) {
                        sm[0] += (double)ms[c];
                        const float tt = __fdiv_rn(ln[c], rw.L[sel[c]]);                                   // (sel is 0..11)
                        pt[i] = make_float4(vxs[c], vys[c], tt, __int_as_float(sel[c]));
                    }
                }
                // ---- the corner term: for each vertex the nearest curve point and its index (a slot past the end repeats
                // point P - 1 under that point's index) ----
#pragma unroll 1
                for (int k = 0; k < 12; ++k) {
                    const float2 w = rw.W[k];
                    unsigned long long key = ~0ULL;
#pragma unroll
                    for (int c = 0; c < PS_PER; ++c) {
                        const int i = t + PS_THREADS * c;
                        const float dx = __fsub_rn(w.x, bx[c]), dy = __fsub_rn(w.y, by[c]);
                        const unsigned long long kc = pf_key(__fmaf_rn(dy, dy, __fmul_rn(dx, dx)), i < P ? i : P - 1);
                        key = kc < key ? kc : key;
                    }
                    key = pf_wave_min_key(key);
                    if (l == 0) redk[wv][k] = key;
                }
                __syncthreads();                             // pt is whole
                // ---- the 24 vertex sums: 8 lanes a sum, lane j over the points j, j + 8, ... in ascending order, then a
                // butterfly over the 8 lanes (distances 4, 2, 1) ----
                if (wv < 3) {
                    const int q = t >> 3, k = q >> 1, km = k == 0 ? 11 : k - 1, y = q & 1;
                    double acc = 0.0;
#pragma unroll 2
                    for (int i = t & 7; i < P; i += 8) {
                        const float4 r = pt[i];
                        const int sg = __float_as_int(r.w);
                        const float v = y ? r.y : r.x;
                        const float w = sg == k ? __fsub_rn(1.f, r.z) : r.z;
                        if (sg == k || sg == km) acc += (double)__fmul_rn(v, w);
                    }
#pragma unroll
                    for (int m = 4; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
                    if ((t & 7) == 0) st.sm[1 + q] = acc;
                }
                float mx = 0.f;
                ps_block_reduce(sm, mx, red, redm, t);       // (its barrier ends the walks of this step)
                if (t == 0) {
                    const double cw = corner_decay && n_steps > 0 ? corner_weight * (1.0 - (double)it / (double)n_steps)
                                                                  : corner_weight;
                    st.sm[0] = sm[0];
                    pf_chain(redk, Bp, P, &rw, &st, cw, gout);
                    if (n_steps > 0) {
                        fit_step(st, trace, rs * (size_t)n_steps + it, it, gout[PF_NP], gout, momentum, gamma);
                        if (it + 1 < evals) pl_stage_params(st.p, &rw);
                    }
                }
            }
            if (t == 0) {
                fit_close_start(st, s, rs, gout[PF_NP], gout, all_params, all_loss, grad);
                st.n_run = s + 1;
                if (stop_loss > 0.0 && (double)gout[PF_NP] < stop_loss) st.stop = 1;     // (a NaN on either side never stops)
            }
            __syncthreads();                                 // st.stop is the workgroup's
        }
        if (t == 0) {
            fit_close_row(st, (size_t)row, params, loss, best);
            if (n_run) n_run[row] = st.n_run;
        }
        // (the next row's first barrier comes before anything of this row in LDS is overwritten but coef, which no one reads now)
    }
}

// ---- the C ABI ----
using namespace hint;

extern "C" {

size_t hint_plusfit_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int32_t n_starts, int32_t n_steps) {
    // n_coeffs = 0 stands for the given-points source, which has no coefficients
    const char* who = "hint_plusfit_workspace_bytes";
    if (ps_check_sizes(who, n_rows, n_coeffs, n_points, n_coeffs != 0) || fit_check_sizes(who, n_starts, n_steps)) return 0;
    last_error_ref().clear();
    return 0;                                                // the kernel needs none
}

int64_t hint_plusfit_geometry(int64_t n_rows, int32_t n_points, int32_t field) {
    if (ps_check_sizes("hint_plusfit_geometry", n_rows, 1, n_points, false, true)) return -1;
    if (field < 0 || field > 4) {
        fail("hint_plusfit_geometry: no field %d (0 workgroups, 1 rows per workgroup at a time, 2 curve points a thread holds, "
             "3 the grid cap, 4 the most starts)", field);
        return -1;
    }
    const int64_t out[5] = {capped_grid(n_rows, 0, FIT_MAX_WG), 1, PS_PER, FIT_MAX_WG, FIT_MAX_S};
    return out[field];
}

int hint_plusfit_run(const hint_plusfit_desc* desc, void* stream) {
    const char* who = "hint_plusfit_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->starts) return fail("%s: starts is null", who);
    if (ps_check_source(who, desc->x, desc->b_points, "the curve needs a source")) return 1;
    if (!desc->params && !desc->loss && !desc->best && !desc->n_run && !desc->all_params && !desc->all_loss && !desc->grad &&
        !desc->trace)
        return fail("%s: no output requested (params, loss, best, n_run, all_params, all_loss, grad and trace are all null)", who);
    if (ps_check_sizes(who, desc->n_rows, desc->n_coeffs, desc->n_points, desc->x != nullptr)) return 1;
    if (fit_check(who, desc->n_starts, desc->n_steps, desc->lr, desc->angle_lr, desc->gamma, desc->momentum, desc->trace)) return 1;
    if (!std::isfinite(desc->corner_weight)) return fail("%s: corner_weight must be finite (got %g)", who, desc->corner_weight);
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"x", desc->x, 3}, {"b_points", desc->b_points, 3}, {"starts", desc->starts, 3},
                               {"params", desc->params, 3}, {"loss", desc->loss, 3}, {"best", desc->best, 3},
                               {"n_run", desc->n_run, 3}, {"all_params", desc->all_params, 3}, {"all_loss", desc->all_loss, 3},
                               {"grad", desc->grad, 3}, {"trace", desc->trace, 3}}))
        return 1;
    const int grid = capped_grid(desc->n_rows, desc->max_groups, FIT_MAX_WG);
    hipLaunchKernelGGL(hint_plusfit_kernel, dim3(grid), dim3(PS_THREADS), 0, (hipStream_t)stream, desc->x, desc->b_points,
                       (int)desc->n_rows, desc->x ? desc->n_coeffs : 1, desc->n_points, desc->starts, desc->n_starts,
                       desc->n_steps, desc->lr, desc->angle_lr, desc->gamma, (float)desc->momentum, desc->corner_weight,
                       desc->corner_decay ? 1 : 0, desc->stop_loss, desc->params, desc->loss, desc->best, desc->n_run,
                       desc->all_params, desc->all_loss, desc->grad, desc->trace);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
