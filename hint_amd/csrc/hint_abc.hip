// Fused ABC selection (gfx950): the k rows of y [N, ny] nearest to one target, exactly, in index order among ties.
//
// Reference being replaced (read-only): rejection_sampling.py:88-96 quantile_ABC, called at :188 by compare_conditional - a
// scipy distance_matrix of one target against 1e8 observations, a full np.argsort of 1e8 float64 values and a gather, on the CPU.
// Here, for y [N, ny], a target t [ny] and k:
//   D_i  = fma(d_j, d_j, ...) over j = 0, 1, .., ny - 1 in that order, d_j = y_ij - t_j, the first term a plain product (fp32,
//          every operation rounded once; written with the _rn intrinsics, so that no pass can contract or reorder it differently)
//   key  = the bit pattern of D_i (non-negative floats order as unsigned integers); anything that is not a finite number - inf, NaN -
//          becomes 0x7F800000 (+inf) and so sorts after every finite key
//   rows are ordered by (key, i); idx / dist = the first k rows of that order and sqrt of their D
// A radix select over the key, y re-read on every pass (nothing of size N is stored):
//   hint_abc_hist_kernel<MODE, PASS>   three passes over digits 30..20, 19..9, 8..0 of the key.  Workgroup w owns rows
//                            [w R, min(N, (w + 1) R)); it counts the digit of every row whose higher digits equal the prefix found
//                            so far in an LDS histogram (integer LDS adds; four interleaved copies keep lanes that hit one bin off
//                            one address) and writes it to its own slot of a slab.  The last pass also counts the rows whose
//                            higher digits are below the prefix.
//   hint_abc_sum_kernel      bin totals over the slab (integers: any order gives the same totals; the order is fixed all the same)
//   hint_abc_find_kernel     one workgroup: the bucket that holds the wanted rank; prefix and rank within the bucket for the next pass
//   hint_abc_count_kernel    per workgroup: rows with key < T*, rows with key == T* (from the last pass's slab, one wavefront each)
//   hint_abc_scan_kernel     one workgroup: exclusive prefix of those counts = every workgroup's output offsets
//   hint_abc_compact_kernel<MODE>   one more pass: rows with key < T* and the first k - count(key < T*) rows with key == T*,
//                            in index order, as (key, index) candidates
//   hint_abc_sort_kernel     one workgroup: bitonic sort of the k candidates by (key, index) in LDS; writes idx and dist
// No float atomics, no global counters: the result is exact and bit-reproducible, and every workspace word that is read was
// written earlier in the same call.
#include "hint_host.hpp"

namespace hint {

constexpr int ABC_BINS = 2048;              // bins of a workgroup's histogram (11-bit digits; the last digit has 9 bits)
constexpr int ABC_COPIES = 4;               // interleaved copies of the LDS histogram (lane & 3)
constexpr int ABC_MAX_WG = 1024;            // workgroups of the streaming passes, at most (four per CU)
constexpr int ABC_MIN_ROWS = 2048;          // rows per workgroup, at least
constexpr int ABC_HIST_U = 8;               // rows per thread in flight in the histogram passes
constexpr int ABC_TILE_U = 16;              // ... and in the compaction pass: a tile is 256 x 16 consecutive rows
constexpr int ABC_MAX_NY = 32, ABC_MAX_K = 8192;
constexpr long long ABC_MAX_N = 1LL << 30;
constexpr int ABC_SELECT_PASSES = 3;
constexpr uint32_t ABC_INF = 0x7F800000u;

__host__ __device__ constexpr int abc_shift(int pass) { return pass == 0 ? 20 : pass == 1 ? 9 : 0; }
__host__ __device__ constexpr int abc_bins(int pass) { return pass == 2 ? 512 : ABC_BINS; }

struct AbcGeom { int wgs, rows; };
inline AbcGeom abc_geom(long long n) {
    long long r = (n + ABC_MAX_WG - 1) / ABC_MAX_WG;
    r = (r + 255) / 256 * 256;
    if (r < ABC_MIN_ROWS) r = ABC_MIN_ROWS;
    AbcGeom g;
    g.rows = (int)r;
    g.wgs = (int)((n + r - 1) / r);
    return g;
}

// workspace layout (bytes; every offset a multiple of 256):
//   [state: 3 x {prefix, rank}][totals: 2048][below: wgs][count <: wgs][count ==: wgs][offset <: wgs][offset ==: wgs]
//   [candidate keys: k][candidate indices: k][slab: wgs x 2048]                                   (all 32-bit words)
struct AbcLayout { size_t state, totals, below, cnt_l, cnt_e, off_l, off_e, ckey, cidx, slab, total; };
inline size_t abc_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline AbcLayout abc_layout(long long n, int k) {
    const size_t G = (size_t)abc_geom(n).wgs;
    AbcLayout L;
    L.state = 0;
    L.totals = 256;
    L.below = L.totals + (size_t)ABC_BINS * 4;
    L.cnt_l = L.below + abc_up(G * 4);
    L.cnt_e = L.cnt_l + abc_up(G * 4);
    L.off_l = L.cnt_e + abc_up(G * 4);
    L.off_e = L.off_l + abc_up(G * 4);
    L.ckey = L.off_e + abc_up(G * 4);
    L.cidx = L.ckey + abc_up((size_t)k * 4);
    L.slab = L.cidx + abc_up((size_t)k * 4);
    L.total = L.slab + G * ABC_BINS * 4;
    return L;
}

}  // namespace hint

// ---- the key of one row ----
__device__ __forceinline__ uint32_t abc_key(float D) {
    const uint32_t u = __float_as_uint(D);          // D >= +0, +inf or a NaN of either sign
    return u < hint::ABC_INF ? u : hint::ABC_INF;
}
__device__ __forceinline__ float abc_first(float yv, float tv) {
    const float d = __fsub_rn(yv, tv);
    return __fmul_rn(d, d);
}
__device__ __forceinline__ float abc_next(float acc, float yv, float tv) {
    const float d = __fsub_rn(yv, tv);
    return __fmaf_rn(d, d, acc);
}
// MODE 0: any ny, any 4-byte aligned y;  2: ny == 2 and y 8-byte aligned (one 8-byte load);  4: ny == 4 and y 16-byte aligned
template <int MODE>
__device__ __forceinline__ uint32_t abc_row_key(const float* __restrict__ y, long long r, int ny, const float* ts) {
    float D;
    if (MODE == 2) {
        const float2 v = *((const float2*)y + r);
        D = abc_next(abc_first(v.x, ts[0]), v.y, ts[1]);
    } else if (MODE == 4) {
        const float4 v = *((const float4*)y + r);
        D = abc_next(abc_next(abc_next(abc_first(v.x, ts[0]), v.y, ts[1]), v.z, ts[2]), v.w, ts[3]);
    } else {
        const float* p = y + (size_t)r * ny;
        D = abc_first(p[0], ts[0]);
        for (int j = 1; j < ny; ++j) D = abc_next(D, p[j], ts[j]);
    }
    return abc_key(D);
}

// ---- one digit's histogram of the rows workgroup w owns ----
template <int MODE, int PASS>
__global__ __launch_bounds__(256) void hint_abc_hist_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                            long long n, int ny, int rows_per_wg,
                                                            const uint32_t* __restrict__ st_in, uint32_t* __restrict__ slab,
                                                            uint32_t* __restrict__ below) {
    constexpr int NB = hint::abc_bins(PASS), SHIFT = hint::abc_shift(PASS), U = hint::ABC_HIST_U;
    constexpr int HS = PASS == 0 ? 31 : hint::abc_shift(PASS - 1);        // the digits above this one start here
    __shared__ uint32_t hist[NB * hint::ABC_COPIES];
    __shared__ float ts[hint::ABC_MAX_NY];
    __shared__ uint32_t red[4];
    const int t = threadIdx.x;
    for (int i = t; i < NB * hint::ABC_COPIES; i += 256) hist[i] = 0u;
    if (t < ny) ts[t] = target[t];
    __syncthreads();
    float tr[4];                                    // MODE 2 / 4: the target in registers
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[j] = MODE != 0 && j < MODE ? ts[j] : 0.f;
    const float* tp = MODE != 0 ? tr : ts;
    const uint32_t want = PASS == 0 ? 0u : (st_in[0] >> HS);
    const long long r0 = (long long)blockIdx.x * rows_per_wg;
    const long long r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
    const int copy = t & (hint::ABC_COPIES - 1);
    uint32_t nbelow = 0u;
    for (long long base = r0; base < r1; base += 256 * U) {
        uint32_t key[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = base + u * 256 + t;
            key[u] = abc_row_key<MODE>(y, r < r1 ? r : r1 - 1, ny, tp);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = base + u * 256 + t;
            if (r < r1) {
                const uint32_t hi = PASS == 0 ? 0u : (key[u] >> HS);
                if (hi == want) atomicAdd(&hist[((key[u] >> SHIFT) & (NB - 1)) * hint::ABC_COPIES + copy], 1u);
                if (PASS == 2 && hi < want) ++nbelow;
            }
        }
    }
    __syncthreads();
    for (int b = t; b < NB; b += 256) {
        uint32_t s = 0u;
#pragma unroll
        for (int c = 0; c < hint::ABC_COPIES; ++c) s += hist[b * hint::ABC_COPIES + c];
        slab[(size_t)blockIdx.x * hint::ABC_BINS + b] = s;
    }
    if (PASS == 2) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nbelow += __shfl_xor(nbelow, m, 64);
        if ((t & 63) == 0) red[t >> 6] = nbelow;
        __syncthreads();
        if (t == 0) below[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// ---- bin totals: block b adds bins 32 b .. 32 b + 31 over the slab's slots; thread (g, bin) takes slots g, g + 8, .. ----
__global__ __launch_bounds__(256) void hint_abc_sum_kernel(const uint32_t* __restrict__ slab, int wgs,
                                                           uint32_t* __restrict__ totals) {
    __shared__ uint32_t red[8][32];
    const int b = threadIdx.x & 31, g = threadIdx.x >> 5, bin = 32 * blockIdx.x + b;
    uint32_t s = 0u;
    for (int w = g; w < wgs; w += 8) s += slab[(size_t)w * hint::ABC_BINS + bin];
    red[g][b] = s;
    __syncthreads();
    if (threadIdx.x < 32) {
        uint32_t v = 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += red[q][threadIdx.x];
        totals[bin] = v;
    }
}

// ---- the bucket that holds the wanted rank: st_out = {prefix with this digit, rank within the bucket} ----
__global__ __launch_bounds__(256) void hint_abc_find_kernel(const uint32_t* __restrict__ totals, int nb, int shift,
                                                            const uint32_t* __restrict__ st_in, uint32_t rank0,
                                                            uint32_t* __restrict__ st_out) {
    __shared__ uint32_t part[256];
    const int t = threadIdx.x, per = nb / 256;          // 8 or 2 consecutive bins per thread
    const uint32_t prefix = st_in ? st_in[0] : 0u, rank = st_in ? st_in[1] : rank0;
    uint32_t c[8], s = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c[i] = i < per ? totals[t * per + i] : 0u;
        s += c[i];
    }
    part[t] = s;
    __syncthreads();
    for (int m = 1; m < 256; m <<= 1) {                 // inclusive scan
        const uint32_t v = t >= m ? part[t - m] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t before = part[t] - s;
    if (rank >= before && rank < part[t]) {             // exactly one thread: the bucket is among its bins
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < per && rank >= before && rank < before + c[i]) {
                st_out[0] = prefix | ((uint32_t)(t * per + i) << shift);
                st_out[1] = rank - before;
            }
            before += c[i];
        }
    }
}

// ---- per workgroup of the passes: rows below T*, rows equal to it (one wavefront each) ----
__global__ __launch_bounds__(256) void hint_abc_count_kernel(const uint32_t* __restrict__ slab, const uint32_t* __restrict__ below,
                                                             const uint32_t* __restrict__ st, int wgs,
                                                             uint32_t* __restrict__ cnt_l, uint32_t* __restrict__ cnt_e) {
    const int l = threadIdx.x & 63, w = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (w >= wgs) return;
    const int last = (int)(st[0] & (hint::abc_bins(2) - 1));
    uint32_t s = 0u;
    for (int b = l; b < last; b += 64) s += slab[(size_t)w * hint::ABC_BINS + b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (l == 0) {
        cnt_l[w] = below[w] + s;
        cnt_e[w] = slab[(size_t)w * hint::ABC_BINS + last];
    }
}

// ---- output offsets: rows below T* first, in workgroup order, then the rows equal to it ----
__global__ __launch_bounds__(1024) void hint_abc_scan_kernel(const uint32_t* __restrict__ cnt_l, const uint32_t* __restrict__ cnt_e,
                                                             int wgs, uint32_t* __restrict__ off_l, uint32_t* __restrict__ off_e) {
    __shared__ uint32_t sl[1024], se[1024];
    const int t = threadIdx.x;
    const uint32_t cl = t < wgs ? cnt_l[t] : 0u, ce = t < wgs ? cnt_e[t] : 0u;
    sl[t] = cl;
    se[t] = ce;
    __syncthreads();
    for (int m = 1; m < 1024; m <<= 1) {
        const uint32_t a = t >= m ? sl[t - m] : 0u, b = t >= m ? se[t - m] : 0u;
        __syncthreads();
        sl[t] += a;
        se[t] += b;
        __syncthreads();
    }
    if (t < wgs) {
        off_l[t] = sl[t] - cl;
        off_e[t] = sl[1023] + (se[t] - ce);
    }
}

// ---- the ordered compaction pass ----
template <int MODE>
__global__ __launch_bounds__(256) void hint_abc_compact_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                               long long n, int ny, int rows_per_wg, int k,
                                                               const uint32_t* __restrict__ st, const uint32_t* __restrict__ off_l,
                                                               const uint32_t* __restrict__ off_e, uint32_t* __restrict__ ckey,
                                                               int32_t* __restrict__ cidx) {
    constexpr int U = hint::ABC_TILE_U;
    __shared__ float ts[hint::ABC_MAX_NY];
    __shared__ uint32_t cl[4 * U], ce[4 * U], tot[2];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    if (t < ny) ts[t] = target[t];
    __syncthreads();
    float tr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tr[j] = MODE != 0 && j < MODE ? ts[j] : 0.f;
    const float* tp = MODE != 0 ? tr : ts;
    const uint32_t T = st[0];
    uint32_t base_l = off_l[blockIdx.x], base_e = off_e[blockIdx.x];
    const long long r0 = (long long)blockIdx.x * rows_per_wg;
    const long long r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
    const unsigned long long lt = (1ull << l) - 1ull;
    for (long long base = r0; base < r1; base += 256 * U) {
        uint32_t key[U], ml = 0u, me = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = base + u * 256 + t;
            key[u] = abc_row_key<MODE>(y, r < r1 ? r : r1 - 1, ny, tp);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = base + u * 256 + t;
            if (r < r1) {
                ml |= (uint32_t)(key[u] < T) << u;
                me |= (uint32_t)(key[u] == T) << u;
            }
        }
        if (!__syncthreads_or((int)(ml | me))) continue;          // (most tiles hold no candidate)
        // rows of a tile are ordered by (u, wavefront, lane): counts per (u, wavefront), their exclusive prefix by wavefront 0
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned long long bl = __ballot((ml >> u) & 1u), be = __ballot((me >> u) & 1u);
            if (l == 0) {
                cl[4 * u + wv] = (uint32_t)__popcll(bl);
                ce[4 * u + wv] = (uint32_t)__popcll(be);
            }
        }
        __syncthreads();
        if (wv == 0) {
            const uint32_t a0 = cl[l], b0 = ce[l];
            uint32_t a = a0, b = b0;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const uint32_t ua = __shfl_up(a, m, 64), ub = __shfl_up(b, m, 64);
                if (l >= m) {
                    a += ua;
                    b += ub;
                }
            }
            cl[l] = a - a0;
            ce[l] = b - b0;
            if (l == 63) {
                tot[0] = a;
                tot[1] = b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned long long bl = __ballot((ml >> u) & 1u), be = __ballot((me >> u) & 1u);
            const long long r = base + u * 256 + t;
            if ((ml >> u) & 1u) {
                const uint32_t pos = base_l + cl[4 * u + wv] + (uint32_t)__popcll(bl & lt);
                if (pos < (uint32_t)k) {
                    ckey[pos] = key[u];
                    cidx[pos] = (int32_t)r;
                }
            }
            if ((me >> u) & 1u) {
                const uint32_t pos = base_e + ce[4 * u + wv] + (uint32_t)__popcll(be & lt);
                if (pos < (uint32_t)k) {                           // only the first k - count(key < T*) of them are wanted
                    ckey[pos] = key[u];
                    cidx[pos] = (int32_t)r;
                }
            }
        }
        base_l += tot[0];
        base_e += tot[1];
    }
}

// ---- k candidates sorted by (key, index) in LDS ----
__global__ __launch_bounds__(1024) void hint_abc_sort_kernel(const uint32_t* __restrict__ ckey, const int32_t* __restrict__ cidx,
                                                             int k, int P, int32_t* __restrict__ idx, float* __restrict__ dist) {
    extern __shared__ unsigned long long abc_sort_lds[];
    unsigned long long* s = abc_sort_lds;
    const int t = threadIdx.x;
    for (int i = t; i < P; i += 1024)
        s[i] = i < k ? ((unsigned long long)ckey[i] << 32) | (unsigned long long)(uint32_t)cidx[i] : ~0ull;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = t; i < P / 2; i += 1024) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const unsigned long long a = s[lo], b = s[hi];
                const bool up = (lo & size) == 0;
                if ((a > b) == up) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < k; i += 1024) {
        const unsigned long long v = s[i];
        idx[i] = (int32_t)(uint32_t)v;
        dist[i] = sqrtf(__uint_as_float((uint32_t)(v >> 32)));
    }
}

// ---- the C ABI ----
using namespace hint;

static int abc_check_sizes(const char* who, int64_t n_rows, int32_t ny, int32_t k, bool with_k) {
    if (n_rows < 1 || n_rows > ABC_MAX_N)
        return fail("%s: n_rows must be 1..%lld (got %lld)", who, ABC_MAX_N, (long long)n_rows);
    if (ny < 1 || ny > ABC_MAX_NY) return fail("%s: ny must be 1..%d (got %d)", who, ABC_MAX_NY, ny);
    if (with_k && (k < 1 || k > ABC_MAX_K || (int64_t)k > n_rows))
        return fail("%s: k must be 1..min(n_rows, %d) (got %d with n_rows = %lld)", who, ABC_MAX_K, k, (long long)n_rows);
    return 0;
}

template <int MODE>
static int abc_launch(const hint_abc_desc* d, const AbcGeom g, const AbcLayout& L, hipStream_t s) {
    char* ws = (char*)d->workspace;
    uint32_t* state = (uint32_t*)(ws + L.state);
    uint32_t* totals = (uint32_t*)(ws + L.totals);
    uint32_t* below = (uint32_t*)(ws + L.below);
    uint32_t* cnt_l = (uint32_t*)(ws + L.cnt_l);
    uint32_t* cnt_e = (uint32_t*)(ws + L.cnt_e);
    uint32_t* off_l = (uint32_t*)(ws + L.off_l);
    uint32_t* off_e = (uint32_t*)(ws + L.off_e);
    uint32_t* ckey = (uint32_t*)(ws + L.ckey);
    int32_t* cidx = (int32_t*)(ws + L.cidx);
    uint32_t* slab = (uint32_t*)(ws + L.slab);
    const long long n = d->n_rows;
    const int ny = d->ny, k = d->k;
    for (int p = 0; p < ABC_SELECT_PASSES; ++p) {
        const uint32_t* st_in = p ? state + 2 * (p - 1) : nullptr;
        if (p == 0)
            hipLaunchKernelGGL((hint_abc_hist_kernel<MODE, 0>), dim3(g.wgs), dim3(256), 0, s, d->y, d->target, n, ny, g.rows, st_in, slab, below);
        else if (p == 1)
            hipLaunchKernelGGL((hint_abc_hist_kernel<MODE, 1>), dim3(g.wgs), dim3(256), 0, s, d->y, d->target, n, ny, g.rows, st_in, slab, below);
        else
            hipLaunchKernelGGL((hint_abc_hist_kernel<MODE, 2>), dim3(g.wgs), dim3(256), 0, s, d->y, d->target, n, ny, g.rows, st_in, slab, below);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hint_abc_sum_kernel, dim3(abc_bins(p) / 32), dim3(256), 0, s, (const uint32_t*)slab, g.wgs, totals);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hint_abc_find_kernel, dim3(1), dim3(256), 0, s, (const uint32_t*)totals, abc_bins(p), abc_shift(p), st_in,
                           (uint32_t)(k - 1), state + 2 * p);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t* st = state + 2 * (ABC_SELECT_PASSES - 1);
    hipLaunchKernelGGL(hint_abc_count_kernel, dim3((g.wgs + 3) / 4), dim3(256), 0, s, (const uint32_t*)slab, (const uint32_t*)below, st,
                       g.wgs, cnt_l, cnt_e);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_abc_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)cnt_l, (const uint32_t*)cnt_e, g.wgs, off_l,
                       off_e);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((hint_abc_compact_kernel<MODE>), dim3(g.wgs), dim3(256), 0, s, d->y, d->target, n, ny, g.rows, k, st,
                       (const uint32_t*)off_l, (const uint32_t*)off_e, ckey, cidx);
    HIP_TRY(hipGetLastError());
    int P = 2;
    while (P < k) P <<= 1;
    hipLaunchKernelGGL(hint_abc_sort_kernel, dim3(1), dim3(1024), (size_t)P * 8, s, (const uint32_t*)ckey, (const int32_t*)cidx, k, P,
                       d->idx, d->dist);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

size_t hint_abc_workspace_bytes(int64_t n_rows, int32_t ny, int32_t k) {
    if (abc_check_sizes("hint_abc_workspace_bytes", n_rows, ny, k, true)) return 0;
    return abc_layout(n_rows, k).total;
}

int64_t hint_abc_geometry(int64_t n_rows, int32_t ny, int32_t field) {
    if (abc_check_sizes("hint_abc_geometry", n_rows, ny, 1, false)) return -1;
    if (field < 0 || field > 2) {
        fail("hint_abc_geometry: no field %d (0 workgroups, 1 rows per workgroup, 2 passes over y)", field);
        return -1;
    }
    const AbcGeom g = abc_geom(n_rows);
    return field == 0 ? g.wgs : field == 1 ? g.rows : ABC_SELECT_PASSES + 1;
}

int hint_abc_run(const hint_abc_desc* desc, void* stream) {
    if (!desc) return fail("hint_abc_run: desc is null");
    if (!desc->y) return fail("hint_abc_run: y is null");
    if (!desc->target) return fail("hint_abc_run: target is null");
    if (!desc->idx) return fail("hint_abc_run: idx is null");
    if (!desc->dist) return fail("hint_abc_run: dist is null");
    if (workspace_null("hint_abc_run", desc->workspace)) return 1;
    if (abc_check_sizes("hint_abc_run", desc->n_rows, desc->ny, desc->k, true)) return 1;
    if (check_aligned("hint_abc_run", {{"y", desc->y, 3}, {"target", desc->target, 3}, {"idx", desc->idx, 3}, {"dist", desc->dist, 3}}))
        return 1;
    const AbcLayout L = abc_layout(desc->n_rows, desc->k);
    if (workspace_fits("hint_abc_run", "abc", desc->workspace, desc->workspace_bytes, L.total)) return 1;
    const AbcGeom g = abc_geom(desc->n_rows);
    hipStream_t s = (hipStream_t)stream;
    if (desc->ny == 2 && ((uintptr_t)desc->y & 7) == 0) return abc_launch<2>(desc, g, L, s);
    if (desc->ny == 4 && ((uintptr_t)desc->y & 15) == 0) return abc_launch<4>(desc, g, L, s);
    return abc_launch<0>(desc, g, L, s);
}

}  // extern "C"
