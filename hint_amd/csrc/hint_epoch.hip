// Device-resident epochs (gfx950): the keyed shuffle-gather that feeds the training step, and the column statistics and the
// standardisation of a resident table.
//
// Reference being replaced (read-only): data.py:484-487 / :503-506 DataLoader(TensorDataset(...), shuffle=True, drop_last=True) - one
// __getitem__ per row and a collate on the host - and data.py:337-339, np.mean / np.std over train+val and the division.
//
// The order of an epoch is hint_epochperm.hpp's permutation (include/hint_amd.h hint_epoch_desc states it): a function of
// (n_rows, seed, epoch, position) alone, so chunks at any boundaries, rank shards and a resumed epoch have the bits of one call.
//   gather       a workgroup takes tiles of 256 output rows.  Phase 1: thread t walks the permutation for row t of the tile and
//       leaves the source row in LDS (and in indices_out).  Phase 2: the tile's rows x d floats are ONE contiguous piece of the
//       output; lanes run over its floats, e -> (row e / d, column e % d): the stores are fully coalesced, the loads are
//       dword-coalesced within a source row (d = 6: a 64-lane load touches eleven or twelve rows).  No load is wider than a dword: a row
//       of 24 bytes is never 16-byte aligned.  y likewise.  A rejected row (cap reached, cursor out of range) is written as NaN
//       and counted: every wavefront ends by writing its count to its int32 of the workspace.  No atomics.
//   moments      two passes over fixed slabs of rows, in double: a workgroup sums its slab per column (threads over (row, column),
//       each its rows ascending; the partial sums of a column added in ascending order), one thread per column adds the slabs in
//       ascending order.  Pass 1 gives the mean, pass 2 the sum of (x - mean)^2; std = sqrt(that / rows), ddof 0.
//   standardize  (float)(((double)x - mean) / std), elementwise, tiles as the gather's; in place or not.
#include "hint_host.hpp"
#include "hint_rowdraws.hpp"
#include "hint_epochperm.hpp"

namespace hint {

constexpr int EP_TILE = 256;                        // rows of a tile = threads of a workgroup
constexpr int EP_MAX_WG = 2048;                     // the grid cap: 256 CUs x 8
constexpr RowGrid EP_GRID{64, EP_TILE / 64, EP_MAX_WG, EP_MAX_ROWS};
constexpr int EP_MAX_D = 128;
constexpr int EP_MAX_SLABS = 1024;
constexpr long long EP_MAX_STRIDE = 1LL << 22;      // floats between rows: every element offset stays below 2^62

struct EpochGatherArgs {
    long long n, count, first, block, block_stride;
    unsigned long long seed;
    unsigned epoch;
    int shuffle, h, d, dy;
    const float* x;
    long long xs;
    const float* y;
    long long ys;
    const long long* cursor;
    float* ox;
    float* oy;
    long long* idx;
    int32_t* rejected;
};

struct EpochStatArgs {
    const float* x;
    long long xs, row0, rows, slab_rows;
    int d, cw, slabs;
    double* part;
    double* mean;
    double* std;
    float* out;
    long long os;
};

}  // namespace hint

// the tile's rows x d floats, contiguous in `out`: lanes over floats
__device__ __forceinline__ void ep_copy_tile(const float* __restrict__ src, long long stride, int d, const long long* rows_src,
                                             float* __restrict__ out, int floats, int tid) {
    const float qnan = __builtin_nanf("");
    for (int e = tid; e < floats; e += hint::EP_TILE) {
        const int r = (int)((unsigned)e / (unsigned)d), j = e - r * d;
        const long long s = rows_src[r];
        out[e] = s >= 0 ? src[s * stride + j] : qnan;
    }
}

__global__ __launch_bounds__(256) void hint_epoch_gather_kernel(const hint::EpochGatherArgs a) {
    using namespace hint;
    __shared__ long long src[EP_TILE];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    long long first = a.first;
    unsigned epoch = a.epoch;
    bool in_range = true;
    if (a.cursor) {                                 // {epoch, first} on the device: read only
        const long long e = a.cursor[0];
        first = a.cursor[1];
        in_range = e >= 0 && e <= 0xFFFFFFFFll && first >= 0 && first < a.n;
        epoch = (unsigned)e;
    }
    const long long tiles = (a.count + EP_TILE - 1) / EP_TILE;
    int rejected = 0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long base = t * EP_TILE, i = base + tid;
        const bool valid = i < a.count;
        long long s = -1;
        if (valid) {
            // (the host has checked the last offset against n: below 2^40, as first is)
            const long long p = first + (a.block > 0 ? (i / a.block) * a.block_stride + i % a.block : i);
            if (in_range && p < a.n) s = ep_source_row((uint64_t)a.n, a.h, a.seed, epoch, a.shuffle, (uint64_t)p);
            if (a.idx) a.idx[i] = s;
        }
        rejected += __popcll(__ballot(valid && s < 0));
        src[tid] = s;
        __syncthreads();
        const long long left = a.count - base;
        const int rows = (int)(left < EP_TILE ? left : EP_TILE);
        if (a.x) ep_copy_tile(a.x, a.xs, a.d, src, a.ox + base * a.d, rows * a.d, tid);
        if (a.y) ep_copy_tile(a.y, a.ys, a.dy, src, a.oy + base * a.dy, rows * a.dy, tid);
        __syncthreads();
    }
    if (l == 0) a.rejected[blockIdx.x * (EP_TILE / 64) + wv] = rejected;
}

// a slab's column sums: PASS 1 of x, PASS 2 of (x - mean)^2
template <int PASS>
__global__ __launch_bounds__(256) void hint_epoch_slab_kernel(const hint::EpochStatArgs a) {
    __shared__ double red[hint::EP_TILE];
    const int tid = threadIdx.x, j = tid % a.cw, r = tid / a.cw, nr = hint::EP_TILE / a.cw;
    const long long b = (long long)blockIdx.x * a.slab_rows;
    const long long e = b + a.slab_rows < a.rows ? b + a.slab_rows : a.rows;
    double s = 0.0;
    if (j < a.d) {
        const double m = PASS == 2 ? a.mean[j] : 0.0;
        for (long long i = b + r; i < e; i += nr) {
            double v = (double)a.x[(a.row0 + i) * a.xs + j];
            if (PASS == 2) {
                v -= m;
                v *= v;
            }
            s += v;
        }
    }
    red[tid] = s;
    __syncthreads();
    if (r == 0 && j < a.d) {
        double t = 0.0;
        for (int q = 0; q < nr; ++q) t += red[q * a.cw + j];
        a.part[(long long)blockIdx.x * a.d + j] = t;
    }
}

// the slabs of a column, ascending: PASS 1 -> mean, PASS 2 -> std
template <int PASS>
__global__ __launch_bounds__(128) void hint_epoch_finish_kernel(const hint::EpochStatArgs a) {
    const int j = threadIdx.x;
    if (j >= a.d) return;
    double t = 0.0;
    for (int s = 0; s < a.slabs; ++s) t += a.part[(long long)s * a.d + j];
    if (PASS == 1)
        a.mean[j] = t / (double)a.rows;
    else
        a.std[j] = sqrt(t / (double)a.rows);
}

__global__ __launch_bounds__(256) void hint_epoch_standardize_kernel(const hint::EpochStatArgs a) {
    using namespace hint;
    const int tid = threadIdx.x;
    const long long tiles = (a.rows + EP_TILE - 1) / EP_TILE;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long base = t * EP_TILE, left = a.rows - base;
        const int floats = (int)(left < EP_TILE ? left : EP_TILE) * a.d;
        for (int e = tid; e < floats; e += EP_TILE) {
            const int r = (int)((unsigned)e / (unsigned)a.d), j = e - r * a.d;
            const long long row = a.row0 + base + r;
            const double v = (double)a.x[row * a.xs + j];
            a.out[row * a.os + j] = (float)((v - a.mean[j]) / a.std[j]);        // (in place: the element's own thread)
        }
    }
}

// ---- the C ABI ----
using namespace hint;

static int epoch_slabs(int64_t rows) {
    const int64_t s = (rows + EP_TILE - 1) / EP_TILE;
    return (int)(s > EP_MAX_SLABS ? EP_MAX_SLABS : s);
}

// the sizes every op shares; count: positions (gather) or rows (moments, standardize)
static int epoch_check_sizes(const char* who, int32_t op, int64_t n_rows, int64_t count, int32_t d) {
    if (op < HINT_EPOCH_GATHER || op > HINT_EPOCH_STANDARDIZE) return fail("%s: op must be 0 (gather), 1 (moments) or 2 (standardize) (got %d)", who, op);
    if (n_rows < 1 || n_rows > EP_MAX_ROWS) return fail("%s: n_rows must be 1..%lld (got %lld)", who, (long long)EP_MAX_ROWS, (long long)n_rows);
    if (count < 1 || count > n_rows) return fail("%s: count must be 1..n_rows = %lld (got %lld)", who, (long long)n_rows, (long long)count);
    if (d < 1 || d > EP_MAX_D) return fail("%s: d must be 1..%d (got %d)", who, EP_MAX_D, d);
    return 0;
}

static size_t epoch_ws_bytes(int32_t op, int64_t count, int32_t d) {
    if (op == HINT_EPOCH_GATHER) return EP_GRID.ws_bytes(count);
    if (op == HINT_EPOCH_MOMENTS) return ((size_t)epoch_slabs(count) * d * sizeof(double) + 15) & ~(size_t)15;
    return 16;
}

static int epoch_check_stride(const char* who, const char* name, int64_t stride, int64_t least) {
    if (stride < least || stride > EP_MAX_STRIDE)
        return fail("%s: %s must be %lld..%lld floats (got %lld)", who, name, (long long)least, EP_MAX_STRIDE, (long long)stride);
    return 0;
}

extern "C" {

int64_t hint_epoch_index(int64_t n_rows, uint64_t seed, uint32_t epoch, int32_t shuffle, int64_t pos) {
    const char* who = "hint_epoch_index";
    if (n_rows < 1 || n_rows > EP_MAX_ROWS) {
        fail("%s: n_rows must be 1..%lld (got %lld)", who, (long long)EP_MAX_ROWS, (long long)n_rows);
        return -1;
    }
    if (pos < 0 || pos >= n_rows) {
        fail("%s: pos must be 0..n_rows - 1 = %lld (got %lld)", who, (long long)n_rows - 1, (long long)pos);
        return -1;
    }
    const int64_t v = ep_source_row((uint64_t)n_rows, ep_half_bits((uint64_t)n_rows), seed, epoch, shuffle, (uint64_t)pos);
    if (v < 0) fail("%s: the walk of position %lld reached its cap of %d applications", who, (long long)pos, EP_WALK_CAP);
    return v;
}

size_t hint_epoch_workspace_bytes(int32_t op, int64_t n_rows, int64_t count, int32_t d) {
    if (epoch_check_sizes("hint_epoch_workspace_bytes", op, n_rows, count, d)) return 0;
    return epoch_ws_bytes(op, count, d);
}

int hint_epoch_run(const hint_epoch_desc* desc) {
    const char* who = "hint_epoch_run";
    if (!desc) return fail("%s: desc is null", who);
    if (workspace_null(who, desc->workspace)) return 1;
    if (epoch_check_sizes(who, desc->op, desc->n_rows, desc->count, desc->d)) return 1;
    if (check_groups(who, desc->max_groups)) return 1;
    const bool gather = desc->op == HINT_EPOCH_GATHER;
    if (!desc->x && !(gather && desc->indices_out && !desc->y)) return fail("%s: x is null (a gather of indices_out alone may leave it out)", who);
    if (desc->x && epoch_check_stride(who, "x_stride", desc->x_stride, 0)) return 1;
    if (desc->first < 0) return fail("%s: first must be >= 0 (got %lld)", who, (long long)desc->first);
    int64_t last = desc->count - 1;                 // the last position's offset from first
    if (gather) {
        if (desc->dy < 0 || desc->dy > EP_MAX_D) return fail("%s: dy must be 0..%d (got %d)", who, EP_MAX_D, desc->dy);
        if (desc->x && !desc->out_x) return fail("%s: out_x is null", who);
        if ((desc->dy > 0) != (desc->y != nullptr)) return fail("%s: y and dy must be given together (dy = %d)", who, desc->dy);
        if (desc->y && !desc->out_y) return fail("%s: out_y is null", who);
        if (desc->y && epoch_check_stride(who, "y_stride", desc->y_stride, 0)) return 1;
        if (desc->block < 0 || desc->block_stride < 0 || (desc->block > 0 && desc->block_stride < desc->block))
            return fail("%s: block must be 0 (contiguous positions) or 1..block_stride (got block = %lld, block_stride = %lld)", who,
                        (long long)desc->block, (long long)desc->block_stride);
        if (desc->block > 0) {
            const int64_t q = last / desc->block;
            if (q > 0 && desc->block_stride > (EP_MAX_ROWS - 1) / q) last = EP_MAX_ROWS;      // (beyond any n_rows)
            else last = q * desc->block_stride + last % desc->block;
        }
    } else {
        if (!desc->mean || !desc->std) return fail("%s: mean and std must be given", who);
        if (desc->op == HINT_EPOCH_STANDARDIZE) {
            if (!desc->out_x) return fail("%s: out_x is null", who);
            if (epoch_check_stride(who, "out_stride", desc->out_stride, desc->d)) return 1;
        }
    }
    // (with a cursor the device holds `first`: a position at or past n_rows rejects its row there)
    if (last >= desc->n_rows - (gather && desc->cursor ? 0 : desc->first))
        return fail("%s: first + count must be <= n_rows (first = %lld, the last position's offset = %lld, n_rows = %lld)", who,
                    (long long)desc->first, (long long)last, (long long)desc->n_rows);
    if (check_aligned(who, {{"x", desc->x, 3}, {"y", desc->y, 3}, {"cursor", desc->cursor, 7}, {"out_x", desc->out_x, 3},
                            {"out_y", desc->out_y, 3}, {"indices_out", desc->indices_out, 7}, {"mean", desc->mean, 7},
                            {"std", desc->std, 7}}))
        return 1;
    const size_t need = epoch_ws_bytes(desc->op, desc->count, desc->d);
    if (workspace_fits(who, "epoch", desc->workspace, desc->workspace_bytes, need)) return 1;
    hipStream_t s = (hipStream_t)desc->stream;
    if (gather) {
        EpochGatherArgs a;
        a.n = desc->n_rows;
        a.count = desc->count;
        a.first = desc->first;
        a.block = desc->block;
        a.block_stride = desc->block_stride;
        a.seed = desc->seed;
        a.epoch = desc->epoch;
        a.shuffle = desc->shuffle != 0;
        a.h = ep_half_bits((uint64_t)desc->n_rows);
        a.d = desc->d;
        a.dy = desc->dy;
        a.x = desc->x;
        a.xs = desc->x_stride;
        a.y = desc->y;
        a.ys = desc->y_stride;
        a.cursor = (const long long*)desc->cursor;
        a.ox = desc->out_x;
        a.oy = desc->out_y;
        a.idx = (long long*)desc->indices_out;
        a.rejected = (int32_t*)desc->workspace;
        const int wgs = EP_GRID.groups(desc->count, desc->max_groups);
        if (EP_GRID.clear_tail(wgs, desc, need, s)) return 1;
        hipLaunchKernelGGL(hint_epoch_gather_kernel, dim3(wgs), dim3(EP_TILE), 0, s, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    EpochStatArgs a;
    a.x = desc->x;
    a.xs = desc->x_stride;
    a.row0 = desc->first;
    a.rows = desc->count;
    a.d = desc->d;
    a.cw = 1;
    while (a.cw < desc->d) a.cw *= 2;
    a.slabs = epoch_slabs(desc->count);
    a.slab_rows = (desc->count + a.slabs - 1) / a.slabs;
    a.part = (double*)desc->workspace;
    a.mean = desc->mean;
    a.std = desc->std;
    a.out = desc->out_x;
    a.os = desc->out_stride;
    if (desc->op == HINT_EPOCH_MOMENTS) {
        hipLaunchKernelGGL(hint_epoch_slab_kernel<1>, dim3(a.slabs), dim3(EP_TILE), 0, s, a);
        hipLaunchKernelGGL(hint_epoch_finish_kernel<1>, dim3(1), dim3(EP_MAX_D), 0, s, a);
        hipLaunchKernelGGL(hint_epoch_slab_kernel<2>, dim3(a.slabs), dim3(EP_TILE), 0, s, a);
        hipLaunchKernelGGL(hint_epoch_finish_kernel<2>, dim3(1), dim3(EP_MAX_D), 0, s, a);
    } else {
        const int wgs = EP_GRID.groups(desc->count, desc->max_groups);
        hipLaunchKernelGGL(hint_epoch_standardize_kernel, dim3(wgs), dim3(EP_TILE), 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
