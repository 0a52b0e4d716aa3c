// Sizes and layouts of a plan's buffers, the block-level entry points of the C ABI (include/hint_amd.h), the re-pack
// groups, the optimizer and the build information; launches the kernels of hint_fwd.hip / hint_bwd.hip /
// hint_wl_*.hip / hint_wgrad.hip / hint_pack.hip / hint_optim.hip.
#include "hint_host.hpp"

#include <atomic>

using namespace hint;

static thread_local std::string g_err;
static unsigned long long* g_stamp_buf = nullptr;  // diagnostic builds only (hint_debug_set_stamp_buffer)

namespace hint {

static Knobs read_knobs() {
    Knobs k;
    auto get = [&](const char* name, int* out) {
        const char* e = std::getenv(name);
        if (!e || !*e) return false;
        *out = std::atoi(e);
        k.non_default += (k.non_default.empty() ? "" : " ") + std::string(name) + "=" + e;
        return true;
    };
    int v;
    if (get("HINT_PLAN_DUMP", &v)) k.plan_dump = v != 0;
    if (get("HINT_WL", &v)) k.wl = v != 0;
    if (get("HINT_WL_NR", &v)) k.wl_nr = v;
    if (get("HINT_WL_STATIC", &v)) k.wl_static = v != 0;
    if (get("HINT_SUB", &v)) k.sub = v != 0;
    if (get("HINT_NW", &v)) k.nw = v;
    if (get("HINT_LEAN", &v)) k.lean = v != 0;
    if (get("HINT_LEANW", &v)) k.leanw = v != 0;
    if (get("HINT_LEANW_MAX", &v)) k.leanw_max = std::min(std::max(v, 4), LEANW_MAX);
    if (get("HINT_FUSE_DW1", &v)) k.fuse_dw1 = v != 0;
    if (get("HINT_PF", &v)) k.pf = v != 0 ? 1 : 0;
    if (get("HINT_NO_BWD_FLY", &v)) k.no_bwd_fly = v != 0;
    if (get("HINT_DW_SPLITS", &v)) k.dw_splits = v;
    if (get("HINT_DW_SMALL", &v)) k.dw_small = v != 0 ? 1 : 0;
    if (get("HINT_DW3_ROWS", &v)) k.dw3_rows = v != 0 ? 1 : 0;
    if (get("HINT_ABLATION_OK", &v)) k.ablation_ok = v != 0;
    return k;
}
static std::mutex g_knobs_mu;
static Knobs* g_knobs = nullptr;          // (replaced, never freed: a reader may hold the old one across hint_debug_reload_knobs)
const Knobs& knobs() {
    std::lock_guard<std::mutex> lk(g_knobs_mu);
    if (!g_knobs) g_knobs = new Knobs(read_knobs());
    return *g_knobs;
}

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}
std::string& last_error_ref() { return g_err; }

// the plan variant a batch of B rows runs on, and (wave-local plans) how many 16-row tiles a workgroup takes:
//   up to one row tile per CU                  the 8-wavefront plan, one tile per workgroup
//   more                                       wave-local plans: ROW PAIRS - two tiles on one weight stream (hint_wl.hpp) - on the
//                                              8-wavefront plan; beyond two pairs per CU on the 4-wavefront plan (two workgroups
//                                              per CU) when that fits the LDS twice
//                                              other plans: the 4-wavefront plan, one tile per workgroup
const hint_plan* variant(const hint_plan* P, int B) {
    if (!P || !P->alt4) return P;
    const int ntiles = (B + ROWS - 1) / ROWS;
    if (ntiles <= P->num_cu) return P;
    const int nr_forced = knobs().wl_nr;
    if (P->wl && P->wl_nr2 && nr_forced != 1) {
        const hint_plan* A = P->alt4;
        const bool alt_twice = A->wl && A->wl_nr2 && std::max(plan_lds(A, false, 2), plan_lds(A, true, 2)) + 4096 <= LDS_LIMIT / 2;
        return (alt_twice && ntiles > 4 * P->num_cu) ? A : P;
    }
    return P->alt4;
}
int wl_nr_for(const hint_plan* Pv, int B) {       // Pv: the variant already picked
    if (!Pv->wl || !Pv->wl_nr2) return 1;
    const int nr_forced = knobs().wl_nr;
    if (nr_forced == 1 || nr_forced == 2) return nr_forced;
    return (B + ROWS - 1) / ROWS > Pv->num_cu ? 2 : 1;
}

// Tape layout (floats): [lane tiles: L x B x d][s: L x B x d][pad to 4][a1: Bp x WT + slack][a2: same]
//                       [sign bytes of a1: Bp/16 x WT/16 x 64 bytes][of a2: same]
// (lean plans: no a1 array)
int64_t tape_act_off(const hint_plan* P, int B) {
    return (2 * (int64_t)P->n_levels * B * P->d + 3) / 4 * 4;
}
int64_t act_stride(const hint_plan* P, int B) { return (int64_t)rows_padded(B) * P->WT + WS_SLACK; }
int64_t bits_stride(const hint_plan* P, int B) { return (int64_t)rows_padded(B) / ROWS * (P->WT / 16) * 64; }   // bytes
// [Bp x WT + slack] arrays in front of the tape's sign bytes (a1, a2) and of the workspace's g_st (g1, g2): lean plans keep no a1 / g2
static int act_arrays(const hint_plan* P) { return P->lean ? 1 : 2; }
static int64_t tape_a2_off(const hint_plan* P, int B) { return (act_arrays(P) - 1) * act_stride(P, B); }      // floats from ChainBlock::actA1
static int64_t tape_bits_off(const hint_plan* P, int B) { return act_arrays(P) * act_stride(P, B); }          // .. of a1's sign bytes; a2's follow bits_stride bytes later

// batch split of part B: a multiple of 8 splits (one XCD each), enough workgroups to cover the chip,
// every workgroup reducing at least 128 rows
void wgrad_splits(const hint_plan* P, int B, int n_chain, int* splits_out, int* rows_out) {
    const long Bp = rows_padded(B);
    int splits = 8;
    while ((long)splits * P->n_wjobs * n_chain < (long)P->num_cu && Bp / (splits * 2) >= 128) splits *= 2;
    const int forced = knobs().dw_splits;          // (experiments)
    if (forced > 0 && Bp / forced >= 16) splits = forced;
    int rows_per_wg = (int)((Bp + splits - 1) / splits);
    rows_per_wg = (rows_per_wg + 15) / 16 * 16;
    if ((long)rows_per_wg * (splits - 1) >= Bp)   // tiny batches: fewer, non-empty splits
        splits = (int)((Bp + rows_per_wg - 1) / rows_per_wg);
    *splits_out = splits;
    *rows_out = rows_per_wg;
}

// Workspace layout (floats): [g1: Bp x WT + slack][g2: same][g_st: Bp x ST + slack, padded to 4][slabs: splits x param_floats]
int64_t ws_gst_off(const hint_plan* P, int B) { return act_arrays(P) * act_stride(P, B); }
int64_t ws_slab_off(const hint_plan* P, int B) {
    return ws_gst_off(P, B) + ((int64_t)rows_padded(B) * P->ST + WS_SLACK + 3) / 4 * 4;
}

// the backward kernel's first-layer gradient slabs (fuse_dw1) follow part B's slabs: [workgroup][tw_floats]
int64_t ws_thin_off(const hint_plan* P, int B) {        // floats from the part-B slabs' start
    int splits, rows;
    wgrad_splits(P, B, 1, &splits, &rows);        // (a chain never uses more splits than a single block)
    return (int64_t)splits * P->param_floats;
}

// The L2 warm-up has an explicit setter for the tests and A/B runs (hint_debug_set_prefetch): its initial value comes from
// HINT_PF (0 = off; hint_host.hpp Knobs).
static std::atomic<int> g_l2_prefetch{-1};
static std::atomic<int> g_last_lds[2] = {{0}, {0}};     // dynamic LDS bytes of the last row-kernel launch: [0] forward / inverse, [1] backward part A
static std::atomic<int> g_last_shape[2] = {{-1}, {-1}}; // .. and the WL_SHAPES entry whose instance it ran on (-1: a dynamic instance, or no wave-local kernel)
bool l2_prefetch_on() {
    int v = g_l2_prefetch.load(std::memory_order_relaxed);
    if (v < 0) {
        v = knobs().pf;
        g_l2_prefetch.store(v, std::memory_order_relaxed);
    }
    return v != 0;
}

// the 256-byte sink of the general kernels' L2 warm-up (hint_device.hpp prefetch_consumer) behind everything else of the launch
static int add_sink(const hint_plan* P, int total, KArgs* a) {
    a->sink_lds = 0;
    if (!P->wl && l2_prefetch_on() && total + 256 <= LDS_LIMIT) {
        a->sink_lds = total / (int)sizeof(float);
        total += 256;
    }
    return total;
}

// LDS bytes of the launch: the plan's, plus the chain's permutation matrices when they fit behind it
// (backward: which slot of hint_debug_last_lds_bytes the launch's size goes to)
static int lds_with_perms(const hint_plan* P, int lds_plan, int n_blocks, bool any_perm, KArgs* a, bool backward) {
    const long extra = (long)n_blocks * P->d * P->d * (long)sizeof(float);
    a->perm_lds = 0;
    const bool dump = knobs().plan_dump;
    if (dump) fprintf(stderr, "[hint plan] lds %d + perms %ld (cap %d)\n", lds_plan, extra, PERM_LDS_MAX);
    int total = lds_plan;
    if (any_perm && extra <= PERM_LDS_MAX && lds_plan + extra <= LDS_LIMIT) {
        a->perm_lds = lds_plan / (int)sizeof(float);
        total += (int)extra;
    }
    // the general kernels warm the L2 with the weights of what comes two phases later (hint_device.hpp prefetch_consumer): loads
    // straight into a 256-byte sink behind everything else (hint_debug_set_prefetch(0) / HINT_PF=0: never).  Not the wave-local
    // kernels: the same touch a block ahead is worth 6 us of 109 (forward) and 2 of 133 (backward) at cfg 2, but the call site -
    // wherever it was put - costs their register allocation 10 / 8 us (SGPR spills in the level loop), and from the block's top the
    // issuing wavefront's own loads wait for it (+14 / +9 us); as straight-line code - a `buffer_load ... lds` every wavefront
    // always issues, with an out-of-bound offset for the lanes that are not to touch anything - +2 / +6 us
    total = add_sink(P, total, a);
    if (dump) fprintf(stderr, "[hint plan] packed lines %d: sink at %d, lds %d\n", a->packed_lines, a->sink_lds, total);
    g_last_lds[backward ? 1 : 0].store(total, std::memory_order_relaxed);
    return total;
}
static KArgs make_args(const hint_plan* P, int B, bool backward) {
    KArgs a{};
    a.meta = P->d_meta; a.meta_bytes = P->meta_bytes; a.recs = P->d_recs; a.total_rows = P->total_rows; a.thins = P->d_thins; a.total_tiles = P->total_tiles;
    a.units_off = P->units_off; a.tmap_off = P->tmap_off; a.ents_off = P->ents_off; a.rng_off = P->rng_off;
    a.lops_off = P->lops_off; a.lopsc = P->d_lopsc; a.lop_cnt = P->lop_cnt;
    a.n_groups = P->n_groups; a.n_levels = P->n_levels; a.n_units = P->n_units; a.nw = P->nw;
    a.d = P->d; a.dc = P->dc; a.xld = P->xld; a.cld = P->cld;
    a.abuf_tiles = P->abuf_tiles; a.slab_floats = backward ? P->slab_bwd : P->slab_fwd; a.gld = P->gld;
    a.region_floats = backward ? P->region_bwd : P->region_fwd;
    a.WT = P->WT; a.ST = P->ST; a.perm_lds = 0; a.stage_out = P->stage_out;
    a.thin_off = backward ? P->thin_b_off : P->thin_f_off;
    a.thin_floats = backward ? P->thin_b_floats : P->thin_f_floats;
    a.thin_lds = backward ? P->thin_lds_b : P->thin_lds_f;
    a.thin_grp = backward ? P->thin_grp_b : P->thin_grp_f;
    a.act_stride = act_stride(P, B); a.bits_stride = bits_stride(P, B);
    a.fuse_dw1 = P->fuse_dw1; a.tw_floats = P->tw_floats; a.thin_slab_off = ws_thin_off(P, B);
    a.lean = P->lean; a.a2_off = tape_a2_off(P, B); a.bits_off = tape_bits_off(P, B);
    a.alpha = P->alpha; a.B = B; a.stamps = g_stamp_buf;
    a.rowdw_lds = backward ? P->rowdw_lds : 0;
    a.n_sub = P->n_sub;
    a.packed_tiles = (int)(P->packed_floats / 256);
    a.packed_lines = (int)(((P->packed_floats + P->n_bias) * 4 + 127) / 128);
    if (P->n_sub > 0) {
        const int* o = backward ? P->sub_lds_b : P->sub_lds_f;
        a.sub_slab = o[0]; a.sub_par = o[1]; a.sub_misc = o[2];
        a.sub_pf = P->sub_pf; a.sub_pb = P->sub_pb; a.sub_par_f4 = (P->sub_pf + P->sub_pb + P->sub_pbias) / 4;
        a.sub_bsrc = P->sub_bsrc; a.sub_bias_src = (int)P->packed_floats; a.sub_cols = P->sub_cols;
    }
    return a;
}

void split_workspace(const hint_plan* P, int B, void* workspace, ChainBlock* b) {
    b->wsG1 = (float*)workspace;
    b->wsGST = b->wsG1 + ws_gst_off(P, B);
    b->wsSlab = b->wsG1 + ws_slab_off(P, B);
}

// the hidden activations live inside the tape (the training forward writes them)
void bind_tape(const hint_plan* P, int B, float* tape, ChainBlock* b) {
    b->tape = tape;
    b->actA1 = tape ? tape + tape_act_off(P, B) : nullptr;
}

int grid_for(const hint_plan* P, int B) {
    const int ntiles = (B + ROWS - 1) / ROWS, nr = wl_nr_for(P, B);
    return std::min((ntiles + nr - 1) / nr, P->num_cu * 8);
}

// the row kernels loop over tile groups `for (tg = blockIdx.x; tg < groups; tg += gridDim.x)`: passes = ceil(groups / grid)
Dispatch dispatch(const hint_plan* P, int B, int n_chain) {
    Dispatch D;
    P = variant(P, B);
    D.P = P;
    D.ntiles = (B + ROWS - 1) / ROWS;
    D.nr = wl_nr_for(P, B);
    D.groups = (D.ntiles + D.nr - 1) / D.nr;
    D.grid = grid_for(P, B);
    D.passes = D.grid > 0 ? (D.groups + D.grid - 1) / D.grid : 0;
    D.fwd = P->wl ? FWD_WL : P->has_fly ? FWD_FLY : FWD_GEN;
    D.bwd = P->wl ? BWD_WL : P->has_fly && !knobs().no_bwd_fly ? BWD_FLY : P->row_ntt <= 3 && P->rowdw_lds == 0 ? BWD_N3 : BWD_GEN;
    D.dw_small = P->n_wsmall > 0;
    D.dw_wide = P->has_leanw != 0;
    if (B > 0) wgrad_splits(P, B, n_chain, &D.dw_splits, &D.dw_rows);
    return D;
}

int dispatch_out(const hint_plan* P, int B, int32_t* out, int32_t n_out) {
    const Dispatch D = dispatch(P, B);
    const hint_plan* V = D.P;
    const int32_t v[HINT_DISPATCH_FIELDS] = {V->wl, D.nr, V->nw, V != P ? 1 : 0, D.ntiles, D.groups, D.grid, D.passes, D.fwd, D.bwd,
                                             D.dw_small, D.dw_wide, D.dw_splits, D.dw_rows, V->n_sub, V->lean, V->has_leanw,
                                             V->rowdw_lds > 0 ? 1 : 0, V->fuse_dw1, V->num_cu};
    for (int i = 0; i < n_out && i < HINT_DISPATCH_FIELDS; ++i) out[i] = v[i];
    return 0;
}

// which of the planner's attempts the variant for B came from and how it stages its tables (the exports' layout: include/hint_amd.h)
int paths_out(const hint_plan* P, int B, int32_t* out, int32_t n_out) {
    const hint_plan* V = variant(P, B);
    auto thin_mode = [](int lds, int grp) { return lds <= 0 ? 0 : grp > 0 ? 2 : 1; };
    const int32_t v[HINT_PATH_FIELDS] = {V->tile_cap, V->unit_waves, V->n_groups, V->n_levels, thin_mode(V->thin_lds_f, V->thin_grp_f),
                                         thin_mode(V->thin_lds_b, V->thin_grp_b), V->thin_spill_f, V->thin_spill_b,
                                         V->lops_off >= 0 ? 1 : 0, V->rowdw_lds > 0 ? 1 : 0, cdiv(V->max_r, 16), cdiv(V->max_cin, 16)};
    for (int i = 0; i < n_out && i < HINT_PATH_FIELDS; ++i) out[i] = v[i];
    return 0;
}

// What a row kernel is launched with, forward / inverse or backward part A: the kernel arguments, the LDS size with the chain's
// permutation matrices behind the plan's when they fit, and the wave-local kernels' offsets with the place of those matrices.
// (The general backward kernels leave the matrices in global memory: one d x d product per block.  Their L2 warm-up has its sink like
//  the forward's - round 5: until then KArgs::sink_lds was 0 there and the block in hint_bwd.hip dead code.)
static RowLaunch row_launch(const Dispatch& D, int B, bool backward, const BlockSet& bs) {
    const hint_plan* P = D.P;
    RowLaunch L{make_args(P, B, backward), WlArgs{}, 0, D.grid};
    const bool perms_in_lds = any_perm(bs) && (P->wl || !backward);
    L.lds = lds_with_perms(P, plan_lds(P, backward, D.nr), bs.n_chain, perms_in_lds, &L.a, backward);
    if (P->wl) {
        L.w = (backward ? P->wl_b : P->wl_f)[D.nr - 1];
        L.w.off_perm = L.a.perm_lds;
        // the shape-specialised instances exist for chained launches only (the training forward and the backward)
        // (and only for a plan whose level schedule - every row record of every group walked by the planner - is the entry's)
        if (knobs().wl_static && bs.chain != nullptr) L.shape = wl_shape_match(L.a, L.w, backward ? P->wl_sb : P->wl_sf, backward);
    }
    return L;
}

// what hint_plan_check_wl_shape reads: the table entry a chained training launch of the variant for B would take, then the
// launch's own folded fields in list order (what tools/wl_shape_table.py prints the table from)
int wl_shape_out(const hint_plan* P, int B, bool backward, bool with_perm, int32_t* out, int32_t n_out, int32_t* sched) {
    const Dispatch D = dispatch(P, B);
    if (sched != nullptr) {
        const WlSched zero{};
        std::memcpy(sched, D.P->wl ? (backward ? &D.P->wl_sb : &D.P->wl_sf) : &zero, sizeof(WlSched));
    }
    if (!D.P->wl) {                  // (the general kernels: no entry, no fields)
        for (int i = 0; i < n_out && i < 1 + WL_FOLD_FIELDS; ++i) out[i] = i == 0 ? -1 : 0;
        return 0;
    }
    ChainBlock blk{};
    blk.perm = with_perm ? (const float*)&blk : nullptr;       // (never read: row_launch asks whether there is one)
    const RowLaunch L = row_launch(D, B, backward, {.one = &blk, .chain = &blk, .host = &blk});
    const WlFold f = wl_fold_of(L.a, L.w);
    if (n_out > 0) out[0] = L.shape;
    for (int i = 0; i < WL_FOLD_FIELDS && 1 + i < n_out; ++i) out[1 + i] = ((const int32_t*)&f)[i];
    return 0;
}

int launch_rows_fwd(const hint_plan* P, int B, bool rev, const BlockSet& bs, const FwdIO& io, hipStream_t s) {
    const Dispatch D = dispatch(P, B);
    RowLaunch L = row_launch(D, B, false, bs);
    if (rev) L.shape = -1;          // (the sampling direction stays dynamic)
    g_last_shape[0].store(L.shape, std::memory_order_relaxed);
    if (D.fwd == FWD_WL) HIP_TRY(launch_wl_apply(rev, L, bs, io, s));
    else HIP_TRY(launch_apply(rev, D.fwd == FWD_FLY, L, bs, io, s));
    return 0;
}

// part B's launch: the job list, the batch split, and where its kernels find the activations and their sign bytes
static WgradLaunch wgrad_launch(const Dispatch& D, int B) {
    const hint_plan* P = D.P;
    return {.jobs = P->d_wjobs, .n_jobs = P->n_ljobs, .n_small = P->n_lsmall, .n_rowj = P->n_rowj, .interleave = P->wsorted != 0,
            .splits = D.dw_splits, .rows_per_wg = D.dw_rows,     // (the whole chain's count: a bucketed launch sums in the same order)
            .WT = P->WT, .ST = P->ST, .d = P->d, .dc = P->dc, .n_levels = P->n_levels, .B = B, .Bp = rows_padded(B),
            .act_stride = act_stride(P, B), .a2_off = tape_a2_off(P, B), .bits_a2_off = tape_bits_off(P, B) * 4 + bits_stride(P, B),
            .param_floats = P->param_floats, .real = P->d_real, .twmap = P->fuse_dw1 ? P->d_twmap : nullptr, .tw_floats = P->tw_floats,
            .thin_slab_off = ws_thin_off(P, B), .thin_slabs = D.grid, .num_cu = P->num_cu, .small = D.dw_small, .wide = D.dw_wide};
}

static BwdLaunch* const BWD_LAUNCH[] = {launch_wl_bwd, launch_bwd, launch_bwd_n3, launch_bwd_fly};      // [Dispatch::bwd]

// part A (row-parallel, bit 0 of `parts`) and part B (weight gradients, bit 1) of the backward pass of
// one block or a chain
int run_backward(const hint_plan* P, const BlockSet& bs, const BwdIO& io, int B, int accumulate, int parts, hipStream_t s,
                 const AdamFuse* adam) {
#ifdef HINT_ABLATE_STORE
    // (a diagnostic build whose row kernels keep no activations cannot train: only with HINT_ABLATION_OK=1 in the environment -
    //  the timing scripts set it - does it launch a backward pass at all)
    if (!knobs().ablation_ok) return fail("this is an ablation build (HINT_ABLATE_STORE): its gradients are wrong; set HINT_ABLATION_OK=1 for timing runs");
#endif

    const Dispatch D = dispatch(P, B, bs.n_total);
    if (parts & 1) {
        const RowLaunch L = row_launch(D, B, true, bs);
        g_last_shape[1].store(L.shape, std::memory_order_relaxed);
        HIP_TRY(BWD_LAUNCH[D.bwd](L, bs, io, s));
    }
    if (parts & 2) HIP_TRY(launch_wgrad(wgrad_launch(D, B), bs, io.x, io.c, accumulate, adam, s));
    return 0;
}

}  // namespace hint

static int apply(const hint_plan* P, bool rev, const float* params, const float* packed, float* tape, const float* perm,
                 const FwdIO& io, int32_t B, void* stream) {
    const char* what = rev ? "inverse" : "forward";
    if (!P || !params || !packed || !io.x || !io.z || !io.J) return fail("hint_block_%s: null argument", what);
    if (P->dc > 0 && !io.c) return fail("hint_block_%s: plan has dc=%d but c is NULL", what, P->dc);
    if (B < 0) return fail("negative batch");
    if (B == 0) return 0;
    P = variant(P, B);
    ChainBlock one{};
    one.params = params; one.packed = packed; one.perm = perm;
    bind_tape(P, B, rev ? nullptr : tape, &one);
    return launch_rows_fwd(P, B, rev, {.one = &one}, io, (hipStream_t)stream);
}

extern "C" {

int hint_abi_version(void) { return HINT_AMD_ABI_VERSION; }

const char* hint_build_info(void) {
    // what the shipped binary was compiled with (the box that runs it may carry another HIP runtime: bench.py prints both), its
    // source stamp (-DHINT_SRC_STAMP: a hash of hint_amd/csrc + include, Makefile) and the HINT_* knobs set in this process
    static thread_local std::string info;
    info = std::string("libhint_amd abi ") + std::to_string(HINT_AMD_ABI_VERSION) +
#ifdef HINT_ABLATE_STORE
                                    " ABLATION BUILD (no activation / gradient stores: timing only, results are wrong)" +
#endif
                                    ", gfx950, HIP " +
                                    std::to_string(HIP_VERSION_MAJOR) + "." + std::to_string(HIP_VERSION_MINOR) + "." +
                                    std::to_string(HIP_VERSION_PATCH) + ", clang " + __clang_version__ +
#ifdef HINT_SRC_STAMP
                                    ", src " HINT_SRC_STAMP +
#endif
                                    (knobs().non_default.empty() ? std::string("") : ", knobs: " + knobs().non_default);
    return info.c_str();
}
const char* hint_last_error(void) { return g_err.c_str(); }

int hint_debug_reload_knobs(void) {
    std::lock_guard<std::mutex> lk(g_knobs_mu);
    g_knobs = new Knobs(read_knobs());
    g_l2_prefetch.store(g_knobs->pf, std::memory_order_relaxed);
    return 0;
}

int hint_debug_set_prefetch(int on) {
    hint::l2_prefetch_on();        // (so that the previous value is the environment's, not "unread")
    return g_l2_prefetch.exchange(on ? 1 : 0);
}
int32_t hint_debug_last_lds_bytes(int32_t backward) { return g_last_lds[backward ? 1 : 0].load(std::memory_order_relaxed); }
int32_t hint_debug_last_wl_shape(int32_t backward) { return g_last_shape[backward ? 1 : 0].load(std::memory_order_relaxed); }

int64_t hint_plan_param_floats(const hint_plan* P) { return P ? P->param_floats : -1; }
// + PACK_SLACK floats of zeros behind the bias region (a padded row's dummy steps load up to three tiles past its last)
int64_t hint_plan_packed_floats(const hint_plan* P) { return P ? P->packed_floats + P->n_bias + PACK_SLACK : -1; }

int64_t hint_plan_tape_floats(const hint_plan* P, int32_t B) {
    if (!P || B < 0) return -1;
    P = variant(P, B);
    return tape_act_off(P, B) + tape_bits_off(P, B) + 2 * bits_stride(P, B) / 4;
}

size_t hint_plan_workspace_bytes(const hint_plan* P, int32_t B) {
    if (!P || B <= 0) return 0;
    P = variant(P, B);
    const int64_t thin = P->fuse_dw1 ? (int64_t)grid_for(P, B) * P->tw_floats : 0;
    return (size_t)(ws_slab_off(P, B) + ws_thin_off(P, B) + thin) * sizeof(float);
}

int32_t hint_plan_lds_bytes(const hint_plan* P, int32_t backward) {
    return P ? plan_lds(P, backward != 0) : -1;
}

int hint_plan_describe(const hint_plan* P, int32_t B, int32_t* out) {
    if (!P || !out || B < 0) return fail("hint_plan_describe: bad arguments");
    P = variant(P, B);
    out[0] = P->wl; out[1] = wl_nr_for(P, B); out[2] = P->nw; out[3] = P->lean;
    out[4] = P->n_sub; out[5] = P->row_ntt; out[6] = P->rowdw_lds > 0 ? 1 : 0; out[7] = P->has_fly;
    return 0;
}

int hint_plan_dispatch(const hint_plan* P, int32_t B, int32_t* out, int32_t n_out) {
    if (!P || !out || B < 1 || n_out < 1) return fail("hint_plan_dispatch: bad arguments");
    return dispatch_out(P, B, out, n_out);
}

int hint_plan_paths(const hint_plan* P, int32_t B, int32_t* out, int32_t n_out) {
    if (!P || !out || B < 1 || n_out < 1) return fail("hint_plan_paths: bad arguments");
    return paths_out(P, B, out, n_out);
}

int hint_block_pack(const hint_plan* P, const float* params, float* packed, void* stream) {
    if (!P || !params || !packed) return fail("hint_block_pack: null argument");
    HIP_TRY(launch_pack(P->d_segs, P->d_ptiles, P->n_ptiles, P->d_bmap, P->n_bias, (long)P->packed_floats, params,
                        packed, (hipStream_t)stream));
    return 0;
}

int hint_block_ext_coeffs(const hint_plan* P, const float* params, const float* packed, const float* c, int32_t R,
                          float* coef_out, void* stream) {
    if (!P || !params || !packed || !c || !coef_out) return fail("hint_block_ext_coeffs: null argument");
    if (R < 0) return fail("hint_block_ext_coeffs: R = %d < 0", R);
    if (P->nodes.size() != 1 || P->nodes[0].k != 0 || P->dc == 0 || P->unit_w23.size() != 2)
        return fail("hint_block_ext_coeffs: the plan is not a one-node coupling with an empty upper half and a condition "
                    "(an ExternalAffineCoupling)");
    if (R == 0) return 0;
    const hint_node_desc& n = P->nodes[0];
    ExtArgs a{};
    a.params = params; a.packed = packed; a.c = c; a.coef = coef_out;
    a.R = R; a.dc = P->dc; a.h = n.h; a.r = n.r;
    a.NT = (n.h + 15) / 16; a.RT = (n.r + 15) / 16;
    for (int net = 0; net < 2; ++net) {
        a.f2[net] = P->unit_w23[net].x; a.f3[net] = P->unit_w23[net].y;
        a.w1[net] = n.p_off[net * 6 + HINT_W1]; a.b1[net] = n.p_off[net * 6 + HINT_B1];
        a.b2[net] = n.p_off[net * 6 + HINT_B2]; a.b3[net] = n.p_off[net * 6 + HINT_B3];
    }
    a.alpha = P->alpha;
    HIP_TRY(launch_ext_coeff(a, (hipStream_t)stream));
    return 0;
}

struct hint_pack_group {
    PackItem* d_items = nullptr;
    int n = 0, grid = 0;
};

int hint_pack_group_create(const hint_plan* const* plans, const float* const* params, float* const* packed,
                           int32_t n, hint_pack_group** out) {
    if (!plans || !params || !packed || n <= 0 || !out) return fail("hint_pack_group_create: bad arguments");
    std::vector<PackItem> items(n);
    int grid = 0;
    for (int i = 0; i < n; ++i) {
        const hint_plan* P = plans[i];
        if (!P || !params[i] || !packed[i]) return fail("hint_pack_group_create: null entry %d", i);
        PackItem& q = items[i];
        q.segs = P->d_segs; q.ptiles = P->d_ptiles; q.bmap = P->d_bmap; q.params = params[i]; q.packed = packed[i];
        q.bias_off = P->packed_floats; q.n_tiles = P->n_ptiles; q.n_bias = P->n_bias; q.grid_begin = grid; q.pad = 0;
        grid += P->n_ptiles + (P->n_bias + PACK_SLACK + 255) / 256;
    }
    hint_pack_group* G = new hint_pack_group();
    G->n = n; G->grid = grid;
    hipError_t e = hipMalloc((void**)&G->d_items, items.size() * sizeof(PackItem));
    if (e == hipSuccess) e = hipMemcpy(G->d_items, items.data(), items.size() * sizeof(PackItem), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(G->d_items); delete G; return fail("hint_pack_group_create: %s", hipGetErrorString(e)); }
    *out = G;
    return 0;
}

int hint_pack_group_run(const hint_pack_group* G, void* stream) {
    return hint_pack_group_run_ex(G, nullptr, 0, nullptr, nullptr, stream);
}

int hint_pack_group_run_ex(const hint_pack_group* G, float* zero_buf, int32_t zero_floats, uint64_t* rng_state,
                           float* opt_state, void* stream) {
    if (!G) return fail("hint_pack_group_run: null group");
    if (zero_floats < 0 || (zero_floats > 0 && !zero_buf)) return fail("hint_pack_group_run_ex: bad zero buffer");
    if (opt_state && !rng_state) return fail("hint_pack_group_run_ex: opt_state needs the step counter of rng_state");
    HIP_TRY(launch_pack_many(G->d_items, G->n, G->grid, zero_buf, zero_floats, (unsigned long long*)rng_state,
                             opt_state, (hipStream_t)stream));
    return 0;
}

void hint_pack_group_destroy(hint_pack_group* G) {
    if (!G) return;
    (void)hipFree(G->d_items);
    delete G;
}

int hint_block_forward(const hint_plan* P, const float* params, const float* packed, const float* x,
                       const float* c, float* z, float* J, float* tape, int32_t B, void* stream) {
    return apply(P, false, params, packed, tape, nullptr, {.x = x, .c = c, .z = z, .J = J}, B, stream);
}

int hint_block_forward_ex(const hint_plan* P, const float* params, const float* packed, const float* x,
                          const float* c, float* z, float* J, float* tape, const float* perm,
                          const float* J_in, float* loss_acc, int32_t B, void* stream) {
    return apply(P, false, params, packed, tape, perm, {.x = x, .c = c, .z = z, .J = J, .J_in = J_in, .loss_acc = loss_acc}, B, stream);
}

int hint_block_forward_noisy(const hint_plan* P, const float* params, const float* packed, const float* x,
                             const float* c, float* z, float* J, float* tape, const float* perm,
                             const float* J_in, float* loss_acc, float noise, const uint64_t* rng_state,
                             float* x_noisy, int32_t B, void* stream) {
    if (noise != 0.f && (!rng_state || !x_noisy)) return fail("hint_block_forward_noisy: noise needs rng_state and x_noisy");
    if (noise != 0.f && perm) return fail("hint_block_forward_noisy: the noise is added to the block's input, in front of no permutation");
    FwdIO io{.x = x, .c = c, .z = z, .J = J, .J_in = J_in, .loss_acc = loss_acc};
    if (noise != 0.f) { io.noise = noise; io.rng_state = (const unsigned long long*)rng_state; io.x_noisy = x_noisy; }
    return apply(P, false, params, packed, tape, perm, io, B, stream);
}

int hint_block_inverse(const hint_plan* P, const float* params, const float* packed, const float* z,
                       const float* c, float* x, float* J, int32_t B, void* stream) {
    return apply(P, true, params, packed, nullptr, nullptr, {.x = z, .c = c, .z = x, .J = J}, B, stream);
}

int hint_block_inverse_ex(const hint_plan* P, const float* params, const float* packed, const float* z,
                          const float* c, float* x, float* J, const float* perm, const float* J_in,
                          int32_t B, void* stream) {
    return apply(P, true, params, packed, nullptr, perm, {.x = z, .c = c, .z = x, .J = J, .J_in = J_in}, B, stream);
}

int hint_block_backward(const hint_plan* P, const float* params, const float* packed, const float* x,
                        const float* tape, const float* c, const float* g_z, const float* g_J, float* g_x,
                        float* g_c, float* g_params, int32_t accumulate, void* workspace,
                        size_t workspace_bytes, int32_t B, void* stream) {
    return hint_block_backward_ex(P, params, packed, x, tape, c, g_z, g_J, g_x, g_c, g_params, accumulate,
                                  workspace, workspace_bytes, nullptr, 1.0f, 0.0f, B, stream);
}

}  // extern "C"

namespace hint {
// parts: bit 0 the row-parallel kernel, bit 1 the weight gradients (run_backward)
int block_backward(const hint_plan* P, const float* params, const float* packed, const float* tape, float* g_params,
                   int32_t accumulate, void* workspace, size_t workspace_bytes, const float* perm, const BwdIO& io, int32_t B,
                   int parts, void* stream) {
    if (!P || !params || !packed || (!io.x && !perm) || !io.g_x || (!g_params && (parts & 2))) return fail("hint_block_backward: null argument");
    if (perm && !tape) return fail("hint_block_backward_ex: a fused permutation needs the tape of hint_block_forward_ex");
    if (P->dc > 0 && !io.c) return fail("hint_block_backward: plan has dc=%d but c is NULL", P->dc);
    if (!tape && B > 0) return fail("hint_block_backward: tape is NULL (the backward pass reads the forward's lane tiles, s values and activations from it)");
    if (B < 0) return fail("negative batch");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        if (!accumulate && g_params) HIP_TRY(launch_zero(g_params, (long)P->param_floats, P->num_cu, s));
        return 0;
    }
    P = variant(P, B);
    if (!workspace || workspace_bytes < hint_plan_workspace_bytes(P, B))
        return fail("hint_block_backward: workspace too small (%zu < %zu)", workspace_bytes,
                    hint_plan_workspace_bytes(P, B));
    if (((uintptr_t)workspace & 15) != 0) return fail("hint_block_backward: workspace must be 16-byte aligned");
    if (g_params && ((uintptr_t)g_params & 15) != 0) return fail("hint_block_backward: g_params must be 16-byte aligned");
    ChainBlock one{};
    one.params = params; one.packed = packed; one.perm = perm;
    bind_tape(P, B, const_cast<float*>(tape), &one);
    one.gparams = g_params;
    split_workspace(P, B, workspace, &one);
    return run_backward(P, {.one = &one}, io, B, accumulate ? 1 : 0, parts, s);
}
}  // namespace hint

extern "C" {

int hint_block_backward_ex(const hint_plan* P, const float* params, const float* packed, const float* x,
                           const float* tape, const float* c, const float* g_z, const float* g_J, float* g_x,
                           float* g_c, float* g_params, int32_t accumulate, void* workspace,
                           size_t workspace_bytes, const float* perm, float gz_scale, float gJ_const,
                           int32_t B, void* stream) {
    return block_backward(P, params, packed, tape, g_params, accumulate, workspace, workspace_bytes, perm,
                          {.x = x, .c = c, .g_z = g_z, .g_J = g_J, .g_x = g_x, .g_c = g_c, .gz_scale = gz_scale, .gJ_const = gJ_const}, B, 3, stream);
}

int hint_block_backward_rows(const hint_plan* P, const float* params, const float* packed, const float* x,
                             const float* tape, const float* c, const float* g_z, const float* g_J, float* g_x,
                             float* g_c, void* workspace, size_t workspace_bytes, const float* perm, float gz_scale,
                             float gJ_const, int32_t B, void* stream) {
    // part A alone: g_x, g_c and the per-row factors of the weight gradients (left in `workspace` for a later
    // hint_chain_wgrad_range / hint_chain_wgrad_adam over a chain that holds this block with the same tape and workspace)
    return block_backward(P, params, packed, tape, nullptr, 1, workspace, workspace_bytes, perm,
                          {.x = x, .c = c, .g_z = g_z, .g_J = g_J, .g_x = g_x, .g_c = g_c, .gz_scale = gz_scale, .gJ_const = gJ_const}, B, 1, stream);
}

#ifdef HINT_STAMPS
// diagnostic builds only (make stamps): device buffer of MAX_NW x 256 uint64 that workgroup 0 of the block
// kernels fills with shader-clock stamps of its phase boundaries; not part of the shipped ABI
int hint_debug_set_stamp_buffer(void* device_buffer) { g_stamp_buf = (unsigned long long*)device_buffer; return 0; }
// ... and one of [workgroups of a part-B launch][wavefronts][8] uint64 for hint_wgrad_kernel (tools/stamps_dw.py); NULL: off
int hint_debug_set_dw_stamp_buffer(void* device_buffer) { hint::set_dw_stamps((unsigned long long*)device_buffer); return 0; }
#endif

static int adam_num_cu() {
    static int num_cu = 0;
    if (num_cu == 0) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) num_cu = prop.multiProcessorCount;
        if (num_cu <= 0) num_cu = 256;
    }
    return num_cu;
}

int hint_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                   float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                   float grad_clamp, int32_t zero_grads, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq) return fail("hint_adam_step: null argument");
    if (n < 0 || step < 1) return fail("hint_adam_step: n must be >= 0 and step >= 1");
    if (n == 0) return 0;
    if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)
        return fail("hint_adam_step: buffers must be 16-byte aligned");
    // bias corrections in double like torch.optim.Adam's python scalars
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    HIP_TRY(launch_adam(params, grads, exp_avg, exp_avg_sq, (long)n, (float)((double)lr / bc1), beta1, beta2,
                        (float)(1.0 / std::sqrt(bc2)), eps, weight_decay, grad_scale,
                        grad_clamp > 0.f ? grad_clamp : HINT_NO_CLAMP, zero_grads ? 1 : 0, adam_num_cu(), nullptr,
                        (hipStream_t)stream));
    return 0;
}

int hint_adam_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const float* opt_state, float beta1, float beta2, float eps, float weight_decay,
                       float grad_scale, float grad_clamp, int32_t zero_grads, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !opt_state) return fail("hint_adam_step_dev: null argument");
    if (n < 0) return fail("hint_adam_step_dev: n must be >= 0");
    if (n == 0) return 0;
    if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)
        return fail("hint_adam_step_dev: buffers must be 16-byte aligned");
    HIP_TRY(launch_adam(params, grads, exp_avg, exp_avg_sq, (long)n, 0.f, beta1, beta2, 0.f, eps, weight_decay,
                        grad_scale, grad_clamp > 0.f ? grad_clamp : HINT_NO_CLAMP, zero_grads ? 1 : 0, adam_num_cu(),
                        opt_state, (hipStream_t)stream));
    return 0;
}

// ---- the step over a table of segments (hint_adam_multi_*) ----
struct hint_adam_multi {
    hint::AdamSeg* segs = nullptr;        // device
    hint::AdamChunk* chunks = nullptr;    // device
    int32_t n_segs = 0;
    int64_t n_chunks = 0;
    int device = -1, num_cu = 0;
};
static_assert(sizeof(hint::AdamSeg) == sizeof(hint_adam_seg), "AdamSeg mirrors hint_adam_seg");

// argument checks shared by hint_adam_multi_chunk and hint_adam_multi_create (no device call)
static int adam_multi_check(const char* who, const hint_adam_seg* segs, int32_t n_segs) {
    if (n_segs < 0) return fail("%s: n_segs must be >= 0", who);
    if (n_segs > 0 && !segs) return fail("%s: null segment table", who);
    for (int32_t i = 0; i < n_segs; ++i) {
        const hint_adam_seg& s = segs[i];
        if (s.n < 0) return fail("%s: segment %d has negative n (%lld)", who, i, (long long)s.n);
        if (!s.p || !s.g || !s.m || !s.v) return fail("%s: segment %d has a null pointer", who, i);
        if ((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 3) != 0)
            return fail("%s: segment %d has a pointer that is not 4-byte aligned", who, i);
    }
    // two segments whose p ranges overlap would take two steps (or race): sort by address, compare neighbours
    std::vector<int32_t> order;
    for (int32_t i = 0; i < n_segs; ++i)
        if (segs[i].n > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return (uintptr_t)segs[a].p < (uintptr_t)segs[b].p; });
    for (size_t k = 1; k < order.size(); ++k) {
        const hint_adam_seg& a = segs[order[k - 1]];
        if ((uintptr_t)a.p + 4 * (uintptr_t)a.n > (uintptr_t)segs[order[k]].p)
            return fail("%s: the p ranges of segments %d and %d overlap", who, order[k - 1], order[k]);
    }
    return 0;
}

// chunk c of the table: floats [off, off + len) of segment seg.  The first chunk of a segment whose four pointers agree
// modulo 16 also takes the floats in front of the first 16-byte boundary, so that every later chunk starts on one.
static void adam_multi_cut(const hint_adam_seg* segs, int32_t n_segs, std::vector<hint::AdamChunk>& out) {
    for (int32_t i = 0; i < n_segs; ++i) {
        const hint_adam_seg& s = segs[i];
        const uintptr_t mis = (uintptr_t)s.p & 15;
        const bool same = ((uintptr_t)s.g & 15) == mis && ((uintptr_t)s.m & 15) == mis && ((uintptr_t)s.v & 15) == mis;
        const int64_t head = same ? (int64_t)(((16 - mis) & 15) >> 2) : 0;
        for (int64_t off = 0; off < s.n;) {
            const int64_t len = std::min<int64_t>(s.n - off, hint::ADAM_CHUNK + (off == 0 ? head : 0));
            out.push_back(hint::AdamChunk{i, (int32_t)len, off});
            off += len;
        }
    }
}

int64_t hint_adam_multi_chunk(const hint_adam_seg* segs, int32_t n_segs, int64_t c, int32_t field) {
    if (adam_multi_check("hint_adam_multi_chunk", segs, n_segs)) return -1;
    std::vector<hint::AdamChunk> ch;
    adam_multi_cut(segs, n_segs, ch);
    if (c == -1) return (int64_t)ch.size();
    if (c < 0 || c >= (int64_t)ch.size() || field < 0 || field > 2) {
        fail("hint_adam_multi_chunk: no chunk %lld / field %d (%lld chunks)", (long long)c, field, (long long)ch.size());
        return -1;
    }
    return field == 0 ? ch[c].seg : field == 1 ? ch[c].off : ch[c].len;
}

int hint_adam_multi_create(const hint_adam_seg* segs, int32_t n_segs, hint_adam_multi_out out) {
    if (!out) return fail("hint_adam_multi_create: null argument");
    *out = nullptr;
    if (adam_multi_check("hint_adam_multi_create", segs, n_segs)) return 1;
    std::vector<hint::AdamChunk> ch;
    adam_multi_cut(segs, n_segs, ch);
    hint_adam_multi* h = new hint_adam_multi();
    h->n_segs = n_segs;
    h->n_chunks = (int64_t)ch.size();
    if (h->n_chunks > 0) {
        hipError_t e = hipGetDevice(&h->device);
        if (e == hipSuccess) e = hipMalloc((void**)&h->segs, sizeof(hint::AdamSeg) * (size_t)n_segs);
        if (e == hipSuccess) e = hipMalloc((void**)&h->chunks, sizeof(hint::AdamChunk) * ch.size());
        if (e == hipSuccess) e = hipMemcpy(h->segs, segs, sizeof(hint::AdamSeg) * (size_t)n_segs, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(h->chunks, ch.data(), sizeof(hint::AdamChunk) * ch.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hint_adam_multi_destroy(h);
            return fail("hint_adam_multi_create: %s", hipGetErrorString(e));
        }
        h->num_cu = adam_num_cu();
    }
    *out = h;
    return 0;
}

int hint_adam_multi_step(const hint_adam_multi* h, int32_t step, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float grad_scale, float grad_clamp, int32_t zero_grads, void* stream) {
    if (!h) return fail("hint_adam_multi_step: null argument");
    if (step < 1) return fail("hint_adam_multi_step: step must be >= 1");
    if (h->n_chunks == 0) return 0;
    // bias corrections in double like torch.optim.Adam's python scalars (hint_adam_step's expressions)
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    HIP_TRY(launch_adam_multi(h->segs, h->chunks, (long)h->n_chunks, (float)((double)lr / bc1), beta1, beta2,
                              (float)(1.0 / std::sqrt(bc2)), eps, weight_decay, grad_scale,
                              grad_clamp > 0.f ? grad_clamp : HINT_NO_CLAMP, zero_grads ? 1 : 0, h->num_cu, (hipStream_t)stream));
    return 0;
}

void hint_adam_multi_destroy(const hint_adam_multi* h) {
    if (!h) return;
    if (h->segs) (void)hipFree(h->segs);
    if (h->chunks) (void)hipFree(h->chunks);
    delete h;
}

}  // extern "C"
