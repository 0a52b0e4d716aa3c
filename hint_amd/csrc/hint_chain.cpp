#include "hint_host.hpp"

using namespace hint;

extern "C" {

// ---------------------------------------------------------------------------------------
// chained launches: the blocks of a flow (same plan, own parameters) in one kernel each for the
// forward pass, backward part A and backward part B (+ its slab reduction)
// ---------------------------------------------------------------------------------------
struct hint_chain {
    const hint_plan* plan = nullptr;
    int n = 0, B = 0;
    bool committed = false;
    std::vector<ChainBlock> host;
    std::vector<char> set;
    ChainBlock* d_table = nullptr;
};

// blocks [b0, b1) of the chain as the block set of a launch
static BlockSet blocks_of(const hint_chain* C, int b0, int b1) {
    return {.one = &C->host[b0], .chain = C->d_table + b0, .host = C->host.data() + b0, .n_chain = b1 - b0, .cb0 = b0, .n_total = C->n};
}

int hint_chain_create(const hint_plan* P, int32_t n_blocks, int32_t B, hint_chain** out) {
    if (!P || !out) return fail("hint_chain_create: null argument");
    if (n_blocks < 1 || B < 1) return fail("hint_chain_create: n_blocks and B must be >= 1");
    hint_chain* C = new hint_chain();
    C->plan = variant(P, B); C->n = n_blocks; C->B = B;      // (the variant planned for this many row tiles)
    C->host.assign(n_blocks, ChainBlock{});
    C->set.assign(n_blocks, 0);
    if (hipMalloc((void**)&C->d_table, sizeof(ChainBlock) * (size_t)n_blocks) != hipSuccess) {
        delete C;
        return fail("hint_chain_create: hipMalloc failed");
    }
    *out = C;
    return 0;
}

int hint_chain_set_block(hint_chain* C, int32_t i, const float* params, const float* packed, const float* perm,
                         float* tape, void* workspace, size_t workspace_bytes, float* g_params) {
    if (!C || !params || !packed) return fail("hint_chain_set_block: null argument");
    if (i < 0 || i >= C->n) return fail("hint_chain_set_block: block %d out of range (chain has %d)", i, C->n);
    const hint_plan* P = C->plan;
    if (!tape && workspace)
        return fail("hint_chain_set_block: a trainable chain block needs a tape");
    ChainBlock b{};
    b.params = params; b.packed = packed; b.perm = perm; b.gparams = g_params;
    bind_tape(P, C->B, tape, &b);
    if (workspace) {
        if (!g_params) return fail("hint_chain_set_block: workspace without g_params");
        if (workspace_bytes < hint_plan_workspace_bytes(P, C->B))
            return fail("hint_chain_set_block: workspace too small (%zu < %zu)", workspace_bytes,
                        hint_plan_workspace_bytes(P, C->B));
        if (((uintptr_t)workspace & 15) != 0) return fail("hint_chain_set_block: workspace must be 16-byte aligned");
        if (((uintptr_t)g_params & 15) != 0) return fail("hint_chain_set_block: g_params must be 16-byte aligned");
        split_workspace(P, C->B, workspace, &b);
    }
    C->host[i] = b;
    C->set[i] = 1;
    C->committed = false;
    return 0;
}

int hint_chain_set_block_io(hint_chain* C, int32_t i, const float* x_in, const float* c_in, const float* g_add) {
    if (!C) return fail("hint_chain_set_block_io: null argument");
    if (i < 0 || i >= C->n) return fail("hint_chain_set_block_io: block %d out of range (chain has %d)", i, C->n);
    if (!C->set[i]) return fail("hint_chain_set_block_io: hint_chain_set_block(%d) comes first", i);
    if (c_in && C->plan->dc == 0) return fail("hint_chain_set_block_io: the plan has no condition");
    C->host[i].x_in = x_in; C->host[i].c_in = c_in; C->host[i].g_add = g_add;
    C->committed = false;
    return 0;
}

int hint_chain_set_block_affine(hint_chain* C, int32_t i, const float* coef, int64_t row_stride) {
    if (!C) return fail("hint_chain_set_block_affine: null argument");
    if (i < 0 || i >= C->n) return fail("hint_chain_set_block_affine: block %d out of range (chain has %d)", i, C->n);
    if (!C->set[i]) return fail("hint_chain_set_block_affine: hint_chain_set_block(%d) comes first", i);
    if (coef && C->host[i].tape)
        return fail("hint_chain_set_block_affine: block %d belongs to a training chain (it has a tape); the affine step is inference only", i);
    if (coef && row_stride != 0 && row_stride < 2 * (int64_t)C->plan->d)
        return fail("hint_chain_set_block_affine: row_stride %lld must be 0 (broadcast) or >= 2d = %d", (long long)row_stride, 2 * C->plan->d);
    if (coef && dispatch(C->plan, C->B).fwd == FWD_WL)
        return fail("hint_chain_set_block_affine: this plan runs B = %d on the wave-local kernels, which have no affine step", C->B);
    C->host[i].affine = coef;
    C->host[i].affine_stride = coef ? row_stride : 0;
    C->committed = false;
    return 0;
}

// blocks gathered for part B only (they ran as launches of their own): no chained forward / inverse / part A over them
static bool chain_gathered(const hint_chain* C) {
    for (const ChainBlock& b : C->host) if (b.x_in != nullptr || b.c_in != nullptr) return true;
    return false;
}

int hint_chain_commit(hint_chain* C) {
    if (!C) return fail("hint_chain_commit: null argument");
    for (int i = 0; i < C->n; ++i)
        if (!C->set[i]) return fail("hint_chain_commit: block %d was never set", i);
    HIP_TRY(hipMemcpy(C->d_table, C->host.data(), sizeof(ChainBlock) * (size_t)C->n, hipMemcpyHostToDevice));
    C->committed = true;
    return 0;
}

int hint_chain_forward(const hint_chain* C, const float* x, const float* c, float* z, float* J, const float* J_in,
                       float* loss_acc, void* stream) {
    return hint_chain_forward_noisy(C, x, c, z, J, J_in, loss_acc, 0.f, nullptr, nullptr, stream);
}

int hint_chain_forward_noisy(const hint_chain* C, const float* x, const float* c, float* z, float* J,
                             const float* J_in, float* loss_acc, float noise, const uint64_t* rng_state,
                             float* x_noisy, void* stream) {
    if (!C || !x || !z || !J) return fail("hint_chain_forward: null argument");
    if (!C->committed) return fail("hint_chain_forward: hint_chain_commit() has not been called");
    if (chain_gathered(C)) return fail("hint_chain_forward: the chain's blocks have inputs of their own (hint_chain_set_block_io): it serves part B only");
    const hint_plan* P = C->plan;
    if (P->dc > 0 && !c) return fail("hint_chain_forward: plan has dc=%d but c is NULL", P->dc);
    return launch_rows_fwd(P, C->B, false, blocks_of(C, 0, C->n),
                           {.x = x, .c = c, .z = z, .J = J, .J_in = J_in, .loss_acc = loss_acc, .noise = noise,
                            .rng_state = (const unsigned long long*)rng_state, .x_noisy = x_noisy}, (hipStream_t)stream);
}

int hint_chain_inverse(const hint_chain* C, const float* z, const float* c, float* x, float* J, const float* J_in,
                       void* stream) {
    if (!C || !z || !x || !J) return fail("hint_chain_inverse: null argument");
    if (!C->committed) return fail("hint_chain_inverse: hint_chain_commit() has not been called");
    if (chain_gathered(C)) return fail("hint_chain_inverse: the chain's blocks have inputs of their own (hint_chain_set_block_io): it serves part B only");
    const hint_plan* P = C->plan;
    if (P->dc > 0 && !c) return fail("hint_chain_inverse: plan has dc=%d but c is NULL", P->dc);
    return launch_rows_fwd(P, C->B, true, blocks_of(C, 0, C->n), {.x = z, .c = c, .z = x, .J = J, .J_in = J_in}, (hipStream_t)stream);
}

// What the chain's four backward entry points check before run_backward.  `who`: the name inside the messages; the flags hold the
// entry points' differences, the order of the checks included (each reports the fault it has always reported first).
enum : unsigned {
    CK_PART_A = 1, CK_PART_B = 2,      // the parts that run (the bits of `parts`)
    CK_RANGE = 4,                      // blocks [b0, b1) are the caller's and are checked; else the whole chain
    CK_ARENAS = 8,                     // `ad` and n: the arenas' alignment, and every block's parameters a slice of them
    CK_BLOCK_IO = 16,                  // a block's own x_in / c_in (hint_chain_set_block_io) count as inputs; part A refuses such a chain
    CK_X_FIRST = 32, CK_X_LAST = 64,   // a missing x is reported in front of the arenas' alignment / behind the blocks (neither: between them)
};
static int check_backward(const char* who, const hint_chain* C, unsigned f, bool null_arg, const BwdIO& io, int b0, int b1,
                          const AdamFuse* ad, int64_t n) {
    if (!C || null_arg || ((f & CK_ARENAS) && (!ad->p || !ad->m || !ad->v || !ad->st))) return fail("%s: null argument", who);
    if (!C->committed) return fail("%s: hint_chain_commit() has not been called", who);
    const hint_plan* P = C->plan;
    const bool own_io = (f & CK_BLOCK_IO) != 0;
    if (!(f & (CK_PART_A | CK_PART_B))) return fail("hint_chain_backward_parts: parts must select part A (1), part B (2) or both (3)");
    if (!(f & CK_RANGE)) { b0 = 0; b1 = C->n; }
    else if (b0 < 0 || b1 > C->n || b0 >= b1) return fail("%s: blocks [%d, %d) out of range (chain has %d)", who, b0, b1, C->n);
    if ((f & CK_PART_A) && own_io) {
        if (chain_gathered(C)) return fail("%s: the chain's blocks have inputs of their own (hint_chain_set_block_io): part B only", who);
        if (!io.g_z || !io.g_x) return fail("%s: null argument", who);
    }
    if (!own_io && P->dc > 0 && !io.c) return fail("%s: plan has dc=%d but c is NULL", who, P->dc);
    const bool no_x = !io.x && !C->host[0].perm && !(own_io && C->host[0].x_in);
    const char* no_x_msg = "%s: x is NULL but the first block has no fused permutation";
    if (no_x && (f & CK_X_FIRST)) return fail(no_x_msg, who);
    if ((f & CK_ARENAS) && (((uintptr_t)ad->p | (uintptr_t)ad->m | (uintptr_t)ad->v) & 15) != 0)
        return fail("%s: the arenas must be 16-byte aligned", who);
    if (no_x && !(f & CK_X_LAST)) return fail(no_x_msg, who);
    for (int i = b0; i < b1; ++i) {
        const ChainBlock& b = C->host[i];
        if (own_io && P->dc > 0 && !io.c && !b.c_in) return fail("%s: plan has dc=%d but block %d has no condition", who, P->dc, i);
        if (!b.wsG1 || !b.actA1 || !b.gparams) return fail("%s: block %d was set without workspace / g_params", who, i);
        const int64_t off = (f & CK_ARENAS) ? b.params - ad->p : 0;
        if ((f & CK_ARENAS) && (off < 0 || off + P->param_floats > n || (off & 3) != 0))
            return fail("%s: block %d's parameters are not a 16-byte aligned slice of the arena [params, params + n)", who, i);
    }
    if (no_x) return fail(no_x_msg, who);
    return 0;
}

static AdamFuse adam_fuse(float* params, float* exp_avg, float* exp_avg_sq, const float* opt_state, float beta1, float beta2, float eps,
                          float weight_decay, float grad_scale, float grad_clamp) {
    return {params, exp_avg, exp_avg_sq, opt_state, beta1, beta2, eps, weight_decay, grad_scale, grad_clamp > 0.f ? grad_clamp : HINT_NO_CLAMP};
}

int hint_chain_backward_parts(const hint_chain* C, const float* x, const float* c, const float* g_z, const float* g_J,
                              float* g_x, float* g_c, float gz_scale, float gJ_const, int32_t accumulate,
                              int32_t parts, void* stream) {
    const BwdIO io{.x = x, .c = c, .g_z = g_z, .g_J = g_J, .g_x = g_x, .g_c = g_c, .gz_scale = gz_scale, .gJ_const = gJ_const};
    if (check_backward("hint_chain_backward", C, (parts & 3) | CK_BLOCK_IO | CK_X_LAST, false, io, 0, 0, nullptr, 0)) return 1;
    return run_backward(C->plan, blocks_of(C, 0, C->n), io, C->B, accumulate ? 1 : 0, parts & 3, (hipStream_t)stream);
}

int hint_chain_wgrad_range(const hint_chain* C, const float* x, const float* c, int32_t accumulate, int32_t block_begin,
                           int32_t block_end, void* stream) {
    const BwdIO io{.x = x, .c = c};
    if (check_backward("hint_chain_wgrad_range", C, CK_PART_B | CK_RANGE | CK_BLOCK_IO, false, io, block_begin, block_end, nullptr, 0)) return 1;
    return run_backward(C->plan, blocks_of(C, block_begin, block_end), io, C->B, accumulate ? 1 : 0, 2, (hipStream_t)stream);
}

int hint_chain_backward(const hint_chain* C, const float* x, const float* c, const float* g_z, const float* g_J,
                        float* g_x, float* g_c, float gz_scale, float gJ_const, int32_t accumulate, void* stream) {
    return hint_chain_backward_parts(C, x, c, g_z, g_J, g_x, g_c, gz_scale, gJ_const, accumulate, 3, stream);
}

int hint_chain_backward_adam(const hint_chain* C, const float* x, const float* c, const float* g_z, const float* g_J,
                             float* g_x, float* g_c, float gz_scale, float gJ_const, float* params, float* exp_avg,
                             float* exp_avg_sq, int64_t n, const float* opt_state, float beta1, float beta2, float eps,
                             float weight_decay, float grad_scale, float grad_clamp, void* stream) {
    const BwdIO io{.x = x, .c = c, .g_z = g_z, .g_J = g_J, .g_x = g_x, .g_c = g_c, .gz_scale = gz_scale, .gJ_const = gJ_const};
    const AdamFuse ad = adam_fuse(params, exp_avg, exp_avg_sq, opt_state, beta1, beta2, eps, weight_decay, grad_scale, grad_clamp);
    // (no CK_BLOCK_IO: this entry point has never looked at x_in / c_in, nor refused a gathered chain as hint_chain_backward_parts does)
    if (check_backward("hint_chain_backward_adam", C, CK_PART_A | CK_PART_B | CK_ARENAS | CK_X_FIRST, !g_z || !g_x, io, 0, 0, &ad, n)) return 1;
    return run_backward(C->plan, blocks_of(C, 0, C->n), io, C->B, 1, 3, (hipStream_t)stream, &ad);
}

int hint_chain_wgrad_adam(const hint_chain* C, const float* x, const float* c, float* params, float* exp_avg, float* exp_avg_sq,
                          int64_t n, const float* opt_state, float beta1, float beta2, float eps, float weight_decay,
                          float grad_scale, float grad_clamp, void* stream) {
    const BwdIO io{.x = x, .c = c};
    const AdamFuse ad = adam_fuse(params, exp_avg, exp_avg_sq, opt_state, beta1, beta2, eps, weight_decay, grad_scale, grad_clamp);
    if (check_backward("hint_chain_wgrad_adam", C, CK_PART_B | CK_ARENAS | CK_BLOCK_IO, false, io, 0, 0, &ad, n)) return 1;
    return run_backward(C->plan, blocks_of(C, 0, C->n), io, C->B, 1, 2, (hipStream_t)stream, &ad);
}

void hint_chain_destroy(hint_chain* C) {
    if (!C) return;
    (void)hipFree(C->d_table);
    delete C;
}

}  // extern "C"
