// hint_householder_many_run: the m trainable permutations of one flow (FlowTrainer(learned_perms=True)) - every matrix in one
// launch, the row work per permutation, every finish in one launch.  This file holds the entry points and their checks; the
// kernels and their launches are hint_householder.hip's (the single op's device code behind a grid index: the same bits).
#include "hint_host.hpp"
#include "hint_householder.hpp"

using namespace hint;

constexpr int HH_MAX_M = 64;                            // permutations of one job
constexpr int64_t HH_MAX_STRIDE = (int64_t)1 << 30;     // floats between two permutations' items (63 strides fit in 36 bits)

static bool hh_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

extern "C" {

static int hh_many_sizes(const char* who, int32_t op, int32_t m, int32_t B, int32_t d, int32_t n) {
    const HhLimits lim = hh_limits();
    if (op < HINT_HOUSEHOLDER_MANY_BUILD || op > HINT_HOUSEHOLDER_MANY_FINISH)
        return fail("%s: op = %d is not build (0), rows (1) or finish (2)", who, op);
    if (m < 1 || m > HH_MAX_M) return fail("%s: m = %d is outside 1..%d", who, m, HH_MAX_M);
    if (d < 1 || d > lim.max_d) return fail("%s: d = %d is outside 1..%d", who, d, lim.max_d);
    if (n < 1 || n > lim.max_n) return fail("%s: n = %d is outside 1..%d", who, n, lim.max_n);
    if (op != HINT_HOUSEHOLDER_MANY_BUILD && (B < 1 || B > lim.max_b)) return fail("%s: B = %d is outside 1..%d", who, B, lim.max_b);
    return 0;
}

static int hh_stride(const char* who, const char* name, int64_t stride, int64_t item) {
    if (stride < item || stride > HH_MAX_STRIDE)
        return fail("%s: %s = %lld is outside %lld (one item) .. %lld floats", who, name, (long long)stride, (long long)item, (long long)HH_MAX_STRIDE);
    return 0;
}

size_t hint_householder_many_workspace_bytes(int32_t op, int32_t m, int32_t B, int32_t d, int32_t n) {
    if (hh_many_sizes("hint_householder_many_workspace_bytes", op, m, B, d, n)) return 0;
    return op == HINT_HOUSEHOLDER_MANY_BUILD ? 0 : (size_t)m * hh_grad_workspace_bytes(B, d);
}

int hint_householder_many_run(const hint_householder_many* job) {
    const char* who = "hint_householder_many_run";
    if (!job) return fail("%s: job is null", who);
    if (hh_many_sizes(who, job->op, job->m, job->B, job->d, job->n)) return 1;
    const int op = job->op, m = job->m, B = job->B, d = job->d, n = job->n, j = job->j;
    if (op == HINT_HOUSEHOLDER_MANY_ROWS && (j < 0 || j >= m)) return fail("%s: j = %d is outside 0..%d (m - 1)", who, j, m - 1);
    if (check_aligned(who, {{"Vs", job->Vs, 3}, {"W", job->W, 3}, {"x", job->x, 3}, {"g_y", job->g_y, 3}, {"g_x", job->g_x, 3},
                            {"g_W", job->g_W, 3}, {"g_V", job->g_V, 3}, {"workspace", job->workspace, 15}}))
        return 1;
    if (!job->W) return fail("%s: W is null", who);
    if (hh_stride(who, "w_stride", job->w_stride, (int64_t)d * d)) return 1;
    hipStream_t s = (hipStream_t)job->stream;
    if (op != HINT_HOUSEHOLDER_MANY_ROWS) {
        if (!job->Vs) return fail("%s: Vs is null (%s)", who, op == HINT_HOUSEHOLDER_MANY_BUILD ? "build" : "finish");
        if (hh_stride(who, "vs_stride", job->vs_stride, (int64_t)n * d)) return 1;
    }
    if (op == HINT_HOUSEHOLDER_MANY_BUILD) {
        return hh_many_build(job->Vs, job->vs_stride, job->W, job->w_stride, m, d, n, s);
    }
    // rows, finish: slot j of the workspace is a single grad run's workspace, ws_stride floats from slot j - 1
    const size_t slot = hh_grad_workspace_bytes(B, d);
    if (workspace_null(who, job->workspace)) return 1;
    if (hh_stride(who, "ws_stride", job->ws_stride, (int64_t)(slot / 4))) return 1;
    if (job->ws_stride % 4 != 0) return fail("%s: ws_stride = %lld is no multiple of 4 floats (a slot is 16-byte aligned)", who, (long long)job->ws_stride);
    if (workspace_small(who, "householder_many", job->workspace_bytes, (size_t)(m - 1) * (size_t)job->ws_stride * 4 + slot)) return 1;
    char* ws = (char*)job->workspace;
    if (op == HINT_HOUSEHOLDER_MANY_ROWS) {
        if (!job->x) return fail("%s: x is null (rows)", who);
        if (!job->g_y) return fail("%s: g_y is null (rows)", who);
        if (job->g_x && hh_overlap(job->g_y, job->g_x, (size_t)B * d * 4)) return fail("%s: g_x aliases g_y", who);
        return hh_many_rows(job->x, job->g_y, job->W + (size_t)j * job->w_stride, job->g_x, ws + (size_t)j * (size_t)job->ws_stride * 4, B,
                            d, s);
    }
    if (!job->g_V) return fail("%s: g_V is null (finish)", who);
    if (hh_stride(who, "gv_stride", job->gv_stride, (int64_t)n * d)) return 1;
    if (job->g_W && hh_stride(who, "gw_stride", job->gw_stride, (int64_t)d * d)) return 1;
    return hh_many_finish(ws, job->ws_stride, job->W, job->w_stride, job->Vs, job->vs_stride, job->g_W, job->gw_stride, job->g_V,
                          job->gv_stride, m, B, d, n, s);
}

}  // extern "C"
