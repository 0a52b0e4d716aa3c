// The driver of a fused shape fit, stated once for hint_lensfit.hip (NP = 4 parameters) and hint_plusfit.hip (NP = 9): what thread
// 0 does around an evaluation of the loss - start afresh, record the step, take it, close a start, close a row - and the host
// checks of the schedule.  Internal; DESIGN sections 16 and 17.  The update rule is the contract's (include/hint_amd.h,
// hint_lensfit_desc item 4): buf = g on step 0, else fma(momentum, buf, g); p = fma(-rate, buf, p) with the fp32 rounding of lr
// (of angle_lr for the angle, the last parameter); both rates times gamma in double after every step.  The loss L and the
// gradient g [NP] come by value and by pointer: the lens fit's stay in thread 0's registers, the plus fit's lie in LDS.
#pragma once
#include "hint_host.hpp"

namespace hint {
constexpr int FIT_MAX_WG = 1024;                // the grid cap: 256 CUs x 4 workgroups (at most 40 KiB of LDS each)
constexpr int FIT_MAX_S = 16, FIT_MAX_STEPS = 1024;

inline int fit_check_sizes(const char* who, int32_t n_starts, int32_t n_steps) {
    if (n_starts < 1 || n_starts > FIT_MAX_S) return fail("%s: n_starts must be 1..%d (got %d)", who, FIT_MAX_S, n_starts);
    if (n_steps < 0 || n_steps > FIT_MAX_STEPS) return fail("%s: n_steps must be 0..%d (got %d)", who, FIT_MAX_STEPS, n_steps);
    return 0;
}

// the schedule of a run, in the order its faults are reported in
inline int fit_check(const char* who, int32_t n_starts, int32_t n_steps, double lr, double angle_lr, double gamma, double momentum,
                     const void* trace) {
    if (fit_check_sizes(who, n_starts, n_steps)) return 1;
    if (trace && n_steps == 0) return fail("%s: trace holds a record per step, and n_steps is 0", who);
    const char* const names[4] = {"lr", "angle_lr", "gamma", "momentum"};
    const double rates[4] = {lr, angle_lr, gamma, momentum};
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(rates[k]) || rates[k] < 0.0)
            return fail("%s: %s must be finite and >= 0 (got %g)", who, names[k], rates[k]);
    return 0;
}
}  // namespace hint

// a fit's state in LDS, set afresh for every start; a kernel derives its own from it (the staged pose; the plus fit's sums)
template <int NP>
struct fit_state {
    float p[NP], buf[NP];                        // the parameters; the momentum buffer
    double lr, alr;                              // the learning rates before their fp32 rounding
    float best_p[NP], best_l;
    int best;
};

// n_steps = 0: one evaluation, no update
__device__ __forceinline__ int fit_evals(int n_steps) { return n_steps > 0 ? n_steps : 1; }

// thread 0: the fit starts afresh from start rs = row S + s
template <int NP>
__device__ __forceinline__ void fit_begin(fit_state<NP>& st, const float* starts, size_t rs, double lr0, double alr0) {
    for (int k = 0; k < NP; ++k) {
        st.p[k] = starts[NP * rs + k];
        st.buf[k] = 0.f;
    }
    st.lr = lr0;
    st.alr = alr0;
}

// thread 0, n_steps > 0: step `it` - its record p, L, g (2 NP + 1 floats, record rec = rs n_steps + it) and the update
template <int NP>
__device__ __forceinline__ void fit_step(fit_state<NP>& st, float* trace, size_t rec, int it, float L, const float* g,
                                         float momentum, double gamma) {
    if (trace) {
        float* tr = trace + (2 * NP + 1) * rec;
        for (int k = 0; k < NP; ++k) {
            tr[k] = st.p[k];
            tr[NP + 1 + k] = g[k];
        }
        tr[NP] = L;
    }
    const float lr = (float)st.lr, alr = (float)st.alr;
    for (int k = 0; k < NP; ++k) {
        const float b = it == 0 ? g[k] : __fmaf_rn(momentum, st.buf[k], g[k]);
        st.buf[k] = b;
        st.p[k] = __fmaf_rn(-(k == NP - 1 ? alr : lr), b, st.p[k]);
    }
    st.lr *= gamma;
    st.alr *= gamma;
}

// thread 0: start s's result, and the row's best so far - the first minimum
template <int NP>
__device__ __forceinline__ void fit_close_start(fit_state<NP>& st, int s, size_t rs, float L, const float* g, float* all_params,
                                                float* all_loss, float* grad) {
    if (all_params)
        for (int k = 0; k < NP; ++k) all_params[NP * rs + k] = st.p[k];
    if (all_loss) all_loss[rs] = L;
    if (grad)
        for (int k = 0; k < NP; ++k) grad[NP * rs + k] = g[k];
    if (s == 0 || L < st.best_l || (st.best_l != st.best_l && L == L)) {     // (a NaN compares as larger)
        for (int k = 0; k < NP; ++k) st.best_p[k] = st.p[k];
        st.best_l = L;
        st.best = s;
    }
}

// thread 0: the row's result
template <int NP>
__device__ __forceinline__ void fit_close_row(const fit_state<NP>& st, size_t row, float* params, float* loss, int* best) {
    if (params)
        for (int k = 0; k < NP; ++k) params[NP * row + k] = st.best_p[k];
    if (loss) loss[row] = st.best_l;
    if (best) best[row] = st.best;
}
