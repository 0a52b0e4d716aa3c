// Fused multi-kernel MMD (gfx950): the sample-quality metric of the reference's evaluation loop in four small launches.
//
// Reference being replaced (read-only): rejection_sampling.py:56-73 multi_mmd - three N x N torch.mm, about
// thirty element-wise passes over N x N temporaries, one mean.  Here, for x [n_x, d], y [n_y, d] and kernels (C_k, a_k):
//   k(D) = sum_k C_k^a_k ((C_k + D) / a_k)^(-a_k),  D = max(|u - v|^2, 0)
//   MMD  = mean_ij k(D(x_i, x_j)) + mean_ij k(D(y_i, y_j)) - 2 mean_ij k(D(x_i, y_j))          (all pairs, the diagonal included)
//
//   hint_mmd_colsum_kernel   column sums of y over 16 row slices, in double (the common centre is y's mean: the metric is
//                            translation invariant, and the Gram form r_i + r_j - 2 g_ij loses eps (r_i + r_j) in D)
//   hint_mmd_prep_kernel     x - mean(y), y - mean(y) into the workspace as [pad64(rows)][pad16(d)], zero-filled, and the row norms -
//                            taken from the diagonal of the same MFMA sequence the pair kernel runs, so that g_ii == r_i bit for bit
//   hint_mmd_pair_kernel     one workgroup per 64 x 64 tile of a pair matrix (XX and YY: tiles tj >= ti only, off-diagonal ones
//                            with weight 2); Gram sub-tiles on v_mfma_f32_16x16x4_f32 with both operands straight from L2 (a lane's
//                            float4 of row l & 15, columns 16 kb + 4 (l >> 4) + i, is the A operand of MFMA i for x and the B
//                            operand for y: no transpose, no LDS staging); the kernels applied in the accumulator layout; one
//                            double per workgroup into its slot of a slab
//   hint_mmd_reduce_kernel   one workgroup adds the slab in a fixed order, in double, and writes out[4]
// No atomics, no counters: the result is bit-reproducible.
#include "hint_host.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace hint {

constexpr int MMD_T = 64;                   // tile edge of the pair kernel (4 wavefronts x 16 rows, 4 column sub-tiles)
constexpr int MMD_MAX_D = 4096;             // columns: the centre vector rides in 16 KiB of LDS
constexpr int MMD_MAX_N = 1 << 20;          // rows per set: at most 2^29 + 2^28 jobs (the grid's x dimension), row * pad16(d) in 64 bits
constexpr int MMD_MAX_KERNELS = 8;
constexpr int MMD_SLICES = 16;              // row slices of the column sums

struct MmdKernels {                         // k(D) = sum_q scale[q] (C[q] + D)^(-a[q]),  scale = C^a a^a
    int32_t n;
    int32_t type[MMD_MAX_KERNELS];          // 1: a == 1 (a division), 2: a == 0.5 (a division by the square root), 0: exp2(-a log2(.))
    float C[MMD_MAX_KERNELS], a[MMD_MAX_KERNELS], scale[MMD_MAX_KERNELS];
};

struct MmdJob { int32_t kind, ti, tj, weight; };         // kind 0 XX, 1 YY, 2 XY

__host__ __device__ inline long long mmd_tri(long long nt) { return nt * (nt + 1) / 2; }
__host__ __device__ inline long long mmd_job_count(int ntx, int nty, int with_yy) {
    return mmd_tri(ntx) + (with_yy ? 0 : mmd_tri(nty)) + (long long)ntx * nty;
}
// entry j of the upper triangle (tj >= ti) of nt x nt tiles, rows first
__host__ __device__ inline void mmd_tri_decode(int nt, long long j, int32_t* ti_out, int32_t* tj_out) {
    const double b = 2.0 * nt + 1.0;
    long long ti = (long long)((b - sqrt(b * b - 8.0 * (double)j)) * 0.5);
    if (ti < 0) ti = 0;
    if (ti > nt - 1) ti = nt - 1;
    // first entry of row t: t nt - t (t - 1) / 2  (the estimate is off by one at most; these settle it)
    while (ti > 0 && ti * nt - ti * (ti - 1) / 2 > j) --ti;
    while (ti + 1 < nt && (ti + 1) * nt - (ti + 1) * ti / 2 <= j) ++ti;
    *ti_out = (int32_t)ti;
    *tj_out = (int32_t)(ti + (j - (ti * nt - ti * (ti - 1) / 2)));
}
// job j of a run: [XX: upper triangle of ntx][YY: of nty, unless a mean YY was given][XY: ntx x nty]
__host__ __device__ inline MmdJob mmd_job(int ntx, int nty, int with_yy, long long j) {
    MmdJob o;
    const long long cxx = mmd_tri(ntx), cyy = with_yy ? 0 : mmd_tri(nty);
    if (j < cxx) {
        o.kind = 0;
        mmd_tri_decode(ntx, j, &o.ti, &o.tj);
    } else if (j < cxx + cyy) {
        o.kind = 1;
        mmd_tri_decode(nty, j - cxx, &o.ti, &o.tj);
    } else {
        const long long q = j - cxx - cyy;
        o.kind = 2;
        o.ti = (int32_t)(q / nty);
        o.tj = (int32_t)(q % nty);
    }
    o.weight = (o.kind != 2 && o.tj != o.ti) ? 2 : 1;
    return o;
}

inline int mmd_pad16(int d) { return (d + 15) & ~15; }
inline int mmd_tiles(int n) { return (n + MMD_T - 1) / MMD_T; }

// workspace layout (bytes; every offset a multiple of 256):
//   [xp: pad64(n_x) x pad16(d) floats][yp: pad64(n_y) x pad16(d)][rx: pad64(n_x)][ry: pad64(n_y)][column sums: 16 x pad16(d) doubles]
//   [slab: one double per job of a run without a given mean YY]
struct MmdLayout { size_t xp, yp, rx, ry, col, slab, total; };
inline MmdLayout mmd_layout(int n_x, int n_y, int d) {
    const size_t Kp = (size_t)mmd_pad16(d), nxp = (size_t)mmd_tiles(n_x) * MMD_T, nyp = (size_t)mmd_tiles(n_y) * MMD_T;
    MmdLayout L;
    L.xp = 0;
    L.yp = L.xp + nxp * Kp * 4;
    L.rx = L.yp + nyp * Kp * 4;
    L.ry = L.rx + nxp * 4;
    L.col = L.ry + nyp * 4;
    L.slab = L.col + (size_t)MMD_SLICES * Kp * 8;
    L.total = L.slab + (size_t)mmd_job_count(mmd_tiles(n_x), mmd_tiles(n_y), 0) * 8;
    L.total = (L.total + 255) & ~(size_t)255;
    return L;
}

}  // namespace hint

// ---- column sums of y: block (cb, s) adds rows 16 s + g + 256 i, g = thread >> 4, of columns 16 cb .. 16 cb + 15 ----
__global__ __launch_bounds__(256) void hint_mmd_colsum_kernel(const float* __restrict__ y, int n_y, int d, int Kp,
                                                              double* __restrict__ col) {
    __shared__ double red[16][16];
    const int c = 16 * blockIdx.x + (threadIdx.x & 15), g = threadIdx.x >> 4;
    double s = 0.0;
    if (c < d)
        for (long r = 16 * (long)blockIdx.y + g; r < n_y; r += 256) s += (double)y[(size_t)r * d + c];
    red[g][threadIdx.x & 15] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
        col[(size_t)blockIdx.y * Kp + c] = t;
    }
}

// ---- centred, padded copies and the row norms: one workgroup per 64 rows, one wavefront per 16 ----
__global__ __launch_bounds__(256) void hint_mmd_prep_kernel(const float* __restrict__ x, const float* __restrict__ y, int n_x,
                                                            int n_y, int d, int Kp, int ntx, const double* __restrict__ col,
                                                            float* __restrict__ xp, float* __restrict__ yp,
                                                            float* __restrict__ rx, float* __restrict__ ry) {
    __shared__ float centre[hint::MMD_MAX_D];
    for (int c = threadIdx.x; c < Kp; c += 256) {
        double s = 0.0;
        for (int k = 0; k < hint::MMD_SLICES; ++k) s += col[(size_t)k * Kp + c];      // (columns >= d hold 0)
        centre[c] = (float)(s / (double)n_y);
    }
    __syncthreads();
    const bool is_x = (int)blockIdx.x < ntx;
    const float* src = is_x ? x : y;
    float* dst = is_x ? xp : yp;
    float* nrm = is_x ? rx : ry;
    const int n = is_x ? n_x : n_y;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long row0 = (long)(is_x ? blockIdx.x : blockIdx.x - ntx) * hint::MMD_T + 16 * w;
    const long row = row0 + (l & 15);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < Kp / 16; ++kb) {
        const int c0 = 16 * kb + 4 * (l >> 4);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (row < n && c0 + i < d) ? src[(size_t)row * d + c0 + i] - centre[c0 + i] : 0.f;
        *(f32x4*)(dst + (size_t)row * Kp + c0) = v;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[i], v[i], acc, 0, 0, 0);
    }
    // the accumulator holds rows 4 (l >> 4) + i of column l & 15 of the 16 x 16 Gram: its diagonal is the norms
    if (((l & 15) >> 2) == (l >> 4)) {
        const int i = l & 3;
        nrm[row] = i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3];
    }
}

__device__ __forceinline__ float mmd_kernel_sum(float D, const hint::MmdKernels& K) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < hint::MMD_MAX_KERNELS; ++q) {
        if (q < K.n) {
            const float t = K.C[q] + D;
            if (K.type[q] == 1) s += K.scale[q] / t;
            else if (K.type[q] == 2) s += K.scale[q] / sqrtf(t);
            else s += K.scale[q] * exp2f(-K.a[q] * log2f(t));
        }
    }
    return s;
}

// ---- one 64 x 64 tile of XX, YY or XY per workgroup ----
__global__ __launch_bounds__(256) void hint_mmd_pair_kernel(const float* __restrict__ xp, const float* __restrict__ yp,
                                                            const float* __restrict__ rx, const float* __restrict__ ry, int n_x,
                                                            int n_y, int Kp, int ntx, int nty, int with_yy, hint::MmdKernels K,
                                                            double* __restrict__ slab) {
    __shared__ double red[4];
    const hint::MmdJob job = hint::mmd_job(ntx, nty, with_yy, (long long)blockIdx.x);
    const float* A = job.kind == 1 ? yp : xp;
    const float* B = job.kind == 0 ? xp : yp;
    const float* rA = job.kind == 1 ? ry : rx;
    const float* rB = job.kind == 0 ? rx : ry;
    const int nA = job.kind == 1 ? n_y : n_x, nB = job.kind == 0 ? n_x : n_y;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long arow0 = (long)job.ti * hint::MMD_T + 16 * w, brow0 = (long)job.tj * hint::MMD_T;
    const float* ap = A + (size_t)(arow0 + (l & 15)) * Kp + 4 * (l >> 4);
    const float* bp = B + (size_t)(brow0 + (l & 15)) * Kp + 4 * (l >> 4);
    const size_t bstep = (size_t)16 * Kp;
    f32x4 acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) acc[cs] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < Kp / 16; ++kb) {
        const f32x4 a = *(const f32x4*)(ap + 16 * kb);
        f32x4 b[4];
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) b[cs] = *(const f32x4*)(bp + cs * bstep + 16 * kb);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cs = 0; cs < 4; ++cs) acc[cs] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[cs][i], acc[cs], 0, 0, 0);
    }
    // lane l holds rows 4 (l >> 4) + i of column l & 15 of each sub-tile
    const long grow0 = arow0 + 4 * (l >> 4);
    const f32x4 ra = *(const f32x4*)(rA + grow0);
    const bool sym = job.kind != 2;
    double sum = 0.0;
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) {
        const long gcol = brow0 + 16 * cs + (l & 15);
        const float rb = rB[gcol];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long grow = grow0 + i;
            float D = fmaxf(fmaf(-2.f, acc[cs][i], ra[i] + rb), 0.f);
            if (sym && grow == gcol) D = 0.f;               // a row against itself
            const float kv = mmd_kernel_sum(D, K);
            if (grow < nA && gcol < nB) sum += (double)kv;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (l == 0) red[w] = sum;
    __syncthreads();
    if (threadIdx.x == 0) slab[blockIdx.x] = (double)job.weight * (((red[0] + red[1]) + red[2]) + red[3]);
}

// ---- the slab's three ranges, each added in a fixed order; out = {MMD, mean XX, mean YY, mean XY} ----
__global__ __launch_bounds__(256) void hint_mmd_reduce_kernel(const double* __restrict__ slab, long long cxx, long long cyy,
                                                              long long cxy, int n_x, int n_y, const float* __restrict__ yy,
                                                              float* __restrict__ out) {
    __shared__ double red[3][256];
    const long long lo[3] = {0, cxx, cxx + cyy}, cnt[3] = {cxx, cyy, cxy};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        for (long long j = threadIdx.x; j < cnt[k]; j += 256) s += slab[lo[k] + j];
        red[k][threadIdx.x] = s;
    }
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m)
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // the MMD is taken from the three means as stored (fp32), so that a run that is given mean YY agrees bit for bit
        const float mxx = (float)(red[0][0] / ((double)n_x * (double)n_x));
        const float myy = yy ? yy[0] : (float)(red[1][0] / ((double)n_y * (double)n_y));
        const float mxy = (float)(red[2][0] / ((double)n_x * (double)n_y));
        out[0] = (float)(((double)mxx + (double)myy) - 2.0 * (double)mxy);
        out[1] = mxx;
        out[2] = myy;
        out[3] = mxy;
    }
}

// ---- the C ABI ----
using namespace hint;

static int mmd_check_sizes(const char* who, int32_t n_x, int32_t n_y, int32_t d) {
    if (n_x < 1) return fail("%s: n_x must be >= 1 (got %d)", who, n_x);
    if (n_y < 1) return fail("%s: n_y must be >= 1 (got %d)", who, n_y);
    if (d < 1) return fail("%s: d must be >= 1 (got %d)", who, d);
    if (n_x > MMD_MAX_N) return fail("%s: n_x = %d is above the limit of %d rows", who, n_x, MMD_MAX_N);
    if (n_y > MMD_MAX_N) return fail("%s: n_y = %d is above the limit of %d rows", who, n_y, MMD_MAX_N);
    if (d > MMD_MAX_D) return fail("%s: d = %d is above the limit of %d columns", who, d, MMD_MAX_D);
    return 0;
}

extern "C" {

size_t hint_mmd_workspace_bytes(int32_t n_x, int32_t n_y, int32_t d) {
    if (mmd_check_sizes("hint_mmd_workspace_bytes", n_x, n_y, d)) return 0;
    return mmd_layout(n_x, n_y, d).total;
}

int64_t hint_mmd_job(int32_t n_x, int32_t n_y, int32_t with_yy, int64_t j, int32_t field) {
    if (mmd_check_sizes("hint_mmd_job", n_x, n_y, 1)) return -1;
    const int ntx = mmd_tiles(n_x), nty = mmd_tiles(n_y);
    const long long count = mmd_job_count(ntx, nty, with_yy != 0);
    if (j == -1 && (field == 0 || field == 1)) return field == 0 ? count : MMD_T;
    if (j < 0 || j >= count || field < 0 || field > 3) {
        fail("hint_mmd_job: no job %lld / field %d (%lld jobs)", (long long)j, field, count);
        return -1;
    }
    const MmdJob o = mmd_job(ntx, nty, with_yy != 0, j);
    return field == 0 ? o.kind : field == 1 ? o.ti : field == 2 ? o.tj : o.weight;
}

int hint_mmd_run(const hint_mmd_desc* desc, void* stream) {
    if (!desc) return fail("hint_mmd_run: desc is null");
    if (!desc->x) return fail("hint_mmd_run: x is null");
    if (!desc->y) return fail("hint_mmd_run: y is null");
    if (!desc->out) return fail("hint_mmd_run: out is null");
    if (workspace_null("hint_mmd_run", desc->workspace)) return 1;
    if (mmd_check_sizes("hint_mmd_run", desc->n_x, desc->n_y, desc->d)) return 1;
    if (desc->n_kernels < 1 || desc->n_kernels > MMD_MAX_KERNELS)
        return fail("hint_mmd_run: n_kernels must be 1..%d (got %d)", MMD_MAX_KERNELS, desc->n_kernels);
    MmdKernels K;
    memset(&K, 0, sizeof K);
    K.n = desc->n_kernels;
    for (int k = 0; k < K.n; ++k) {
        const float C = desc->width[k], a = desc->exponent[k];
        if (!(C > 0.f) || !std::isfinite(C)) return fail("hint_mmd_run: width[%d] must be positive and finite (got %g)", k, (double)C);
        if (!(a > 0.f) || !std::isfinite(a)) return fail("hint_mmd_run: exponent[%d] must be positive and finite (got %g)", k, (double)a);
        K.C[k] = C;
        K.a[k] = a;
        K.scale[k] = (float)(std::pow((double)C, (double)a) * std::pow((double)a, (double)a));
        K.type[k] = a == 1.f ? 1 : a == 0.5f ? 2 : 0;
    }
    if ((((uintptr_t)desc->x | (uintptr_t)desc->y | (uintptr_t)desc->out | (uintptr_t)desc->yy) & 3) != 0)
        return fail("hint_mmd_run: x, y, yy and out must be 4-byte aligned");
    const MmdLayout L = mmd_layout(desc->n_x, desc->n_y, desc->d);
    if (workspace_fits("hint_mmd_run", "mmd", desc->workspace, desc->workspace_bytes, L.total)) return 1;

    char* ws = (char*)desc->workspace;
    float* xp = (float*)(ws + L.xp);
    float* yp = (float*)(ws + L.yp);
    float* rx = (float*)(ws + L.rx);
    float* ry = (float*)(ws + L.ry);
    double* col = (double*)(ws + L.col);
    double* slab = (double*)(ws + L.slab);
    const int n_x = desc->n_x, n_y = desc->n_y, d = desc->d, Kp = mmd_pad16(d);
    const int ntx = mmd_tiles(n_x), nty = mmd_tiles(n_y), with_yy = desc->yy != nullptr;
    const long long cxx = mmd_tri(ntx), cyy = with_yy ? 0 : mmd_tri(nty), cxy = (long long)ntx * nty;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hint_mmd_colsum_kernel, dim3(Kp / 16, MMD_SLICES), dim3(256), 0, s, desc->y, n_y, d, Kp, col);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_mmd_prep_kernel, dim3(ntx + nty), dim3(256), 0, s, desc->x, desc->y, n_x, n_y, d, Kp, ntx,
                       (const double*)col, xp, yp, rx, ry);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_mmd_pair_kernel, dim3((unsigned)(cxx + cyy + cxy)), dim3(256), 0, s, (const float*)xp,
                       (const float*)yp, (const float*)rx, (const float*)ry, n_x, n_y, Kp, ntx, nty, with_yy, K, slab);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_mmd_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)slab, cxx, cyy, cxy, n_x, n_y, desc->yy,
                       desc->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
