// Fused correlation matrix and correlation MSE (gfx950), in double: the second number of the reference's test_likelihood.
//
// Reference being replaced (read-only): run_experiments.py:212-221 - the sample goes to the host, np.corrcoef(x.T) and
// np.nanmean(np.square(corr - corr_true)) run there in float64; corr_true is rejection_sampling.py:105-132's np.corrcoef of a
// ground-truth sample.  Here, for x fp32 [n, d] (rows are samples), u = double(x) - mean:
//   S_ij = sum_rows u_i u_j,   r_ij = S_ij / (sqrt(S_ii) sqrt(S_jj)) clipped to [-1, 1],   mse = mean over non-NaN of (r - t)^2
//
//   hint_corr_colsum_kernel  column sums of x over 32 row slices, in double
//   hint_corr_gram_kernel    one workgroup per job (row slab, tile row ti, tile column tj >= ti) of 16 x 16 tiles: the centred
//                            operands are formed on load (no centred copy of x exists) and multiplied on
//                            v_mfma_f64_16x16x4_f64; a lane's A value for output row l & 15 and k = l >> 4 is
//                            u[row0 + 4 kb + (l >> 4)][16 ti + (l & 15)], so each k-row is one coalesced 64-byte read and nothing is
//                            transposed; on a diagonal tile A and B are one register.  The job's 16 x 16 doubles go to its own slot
//   hint_corr_sum_kernel     S = the slab slots of each entry added in slab order
//   hint_corr_finish_kernel  one workgroup: r from S, clipped and written to both triangles from one value (symmetric bit for bit),
//                            and sum (r - t)^2 / its count / the NaN count reduced in a fixed order; out[4]
// No atomics, no counters: the result is bit-reproducible.  NaN semantics are numpy's and fall out of the arithmetic: a column of
// zero variance, or one that holds a NaN or an inf, gives a NaN row and column and leaves every other entry alone (rows past n
// and columns past d enter as exact zeros in BOTH operands, so a NaN never meets them in an entry that is kept).
#include "hint_host.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace hint {

constexpr int CORR_T = 16;                  // tile edge (the MFMA's)
constexpr int CORR_MAX_D = 512;             // columns: 32 tile rows, 528 tiles, sqrt(S_ii) of every column in 4 KiB of LDS
constexpr int CORR_MAX_N = 1 << 24;         // rows
constexpr int CORR_MIN_R = 256;             // rows per slab, at least
constexpr int CORR_MAX_SLABS = 64;          // ... and as many more as keep the slab count at this
constexpr int CORR_SLICES = 32;             // row slices of the column sums
constexpr int CORR_FIN_THREADS = 1024;

struct CorrGeom { int nt, tri, R, slabs; };
__host__ __device__ inline CorrGeom corr_geom(int n, int d) {
    CorrGeom g;
    g.nt = (d + CORR_T - 1) / CORR_T;
    g.tri = g.nt * (g.nt + 1) / 2;
    int R = (n + CORR_MAX_SLABS - 1) / CORR_MAX_SLABS;
    R = (R + 3) & ~3;                                   // whole k-blocks of 4 rows
    g.R = R < CORR_MIN_R ? CORR_MIN_R : R;
    g.slabs = (n + g.R - 1) / g.R;
    return g;
}
// first entry of tile row t in the upper triangle (tj >= ti) of nt x nt tiles, rows first
__host__ __device__ inline int corr_tri_first(int nt, int t) { return t * nt - t * (t - 1) / 2; }
__host__ __device__ inline void corr_tri_decode(int nt, int e, int* ti_out, int* tj_out) {
    int ti = 0;
    while (ti + 1 < nt && corr_tri_first(nt, ti + 1) <= e) ++ti;           // (nt <= 32)
    *ti_out = ti;
    *tj_out = ti + (e - corr_tri_first(nt, ti));
}

inline int corr_pad16(int d) { return (d + 15) & ~15; }

// workspace layout (bytes; every offset a multiple of 256):
//   [column sums: 32 x pad16(d) doubles][slab: slabs x tri x 256 doubles][S: tri x 256 doubles]
struct CorrLayout { size_t col, slab, S, total; };
inline CorrLayout corr_layout(int n, int d) {
    const CorrGeom g = corr_geom(n, d);
    CorrLayout L;
    L.col = 0;
    L.slab = L.col + (size_t)CORR_SLICES * corr_pad16(d) * 8;
    L.S = L.slab + (size_t)g.slabs * g.tri * 256 * 8;
    L.total = L.S + (size_t)g.tri * 256 * 8;
    return L;
}

}  // namespace hint

// ---- column sums: block (cb, s) adds rows 16 s + g + 512 i, g = thread >> 4, of columns 16 cb .. 16 cb + 15 ----
__global__ __launch_bounds__(256) void hint_corr_colsum_kernel(const float* __restrict__ x, int n, int d, int Kp,
                                                               double* __restrict__ col) {
    __shared__ double red[16][16];
    const int c = 16 * blockIdx.x + (threadIdx.x & 15), g = threadIdx.x >> 4;
    double s = 0.0;
    if (c < d)
        for (long r = 16 * (long)blockIdx.y + g; r < n; r += 16 * hint::CORR_SLICES) s += (double)x[(size_t)r * d + c];
    red[g][threadIdx.x & 15] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
        col[(size_t)blockIdx.y * Kp + c] = t;              // (c < Kp: columns >= d hold 0)
    }
}

// ---- one (slab, ti, tj) per workgroup; wavefront w takes the slab's k-blocks kb = w, w + 4, ..; the four partial tiles are
// added in wavefront order ----
__global__ __launch_bounds__(256) void hint_corr_gram_kernel(const float* __restrict__ x, int n, int d, int Kp, int nt, int tri,
                                                             int R, const double* __restrict__ col, double* __restrict__ slab) {
    __shared__ double part[3][4][64];
    const int sl = (int)blockIdx.x / tri, e = (int)blockIdx.x % tri;
    int ti, tj;
    hint::corr_tri_decode(nt, e, &ti, &tj);
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ca = 16 * ti + (l & 15), cb = 16 * tj + (l & 15);
    const bool va = ca < d, vb = cb < d, diag = ti == tj;
    double ma = 0.0, mb = 0.0;
    for (int k = 0; k < hint::CORR_SLICES; ++k) {          // (ca, cb < Kp)
        ma += col[(size_t)k * Kp + ca];
        mb += col[(size_t)k * Kp + cb];
    }
    ma /= (double)n;
    mb /= (double)n;
    const long row0 = (long)sl * R;
    const long rend = row0 + R < (long)n ? row0 + R : (long)n;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nkb = (R / 4 - w + 3) / 4;                   // k-blocks of 4 rows of this wavefront (R is a multiple of 4)
    const long rl = row0 + 4 * w + (l >> 4);
    // every load is issued, at an address clamped into the slab's rows and x's columns (rend - 1 >= row0: no slab is empty), and
    // its value is replaced by an exact zero where the row or column does not exist: no branch in the loop, nothing read outside x
    const float* pa = x + (va ? ca : d - 1);
    const float* pb = x + (vb ? cb : d - 1);
    auto load = [&](int it, float& xa, float& xb) -> bool {
        const long r = rl + 16 * (long)it;
        const bool vr = r < rend;
        const size_t ro = (size_t)(vr ? r : rend - 1) * d;
        xa = pa[ro];
        xb = pb[ro];
        return vr;
    };
    auto mult = [&](bool vr, float xa, float xb) {
        const double a = (vr && va) ? (double)xa - ma : 0.0;
        const double b = diag ? a : (vr && vb) ? (double)xb - mb : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    };
#ifdef HINT_CORR_VALU
    // A/B build only (make EXTRA=-DHINT_CORR_VALU; NOTES.md): the same rows per wavefront and the same accumulator layout on
    // v_fma_f64 - a lane's four entries are rows (l >> 4) + 4 q of column l & 15, one chain of fused multiply-adds each
    double mq[4];
    const float* pq[4];
    bool vq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 16 * ti + (l >> 4) + 4 * q;
        vq[q] = c < d;
        pq[q] = x + (vq[q] ? c : d - 1);
        mq[q] = 0.0;
        for (int k = 0; k < hint::CORR_SLICES; ++k) mq[q] += col[(size_t)k * Kp + c];
        mq[q] /= (double)n;
    }
    for (int kb = 0; kb < nkb; ++kb) {
        float xq[4][4], xb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long r = row0 + 4 * w + 16 * (long)kb + k;
            const size_t ro = (size_t)(r < rend ? r : rend - 1) * d;
            xb[k] = pb[ro];
#pragma unroll
            for (int q = 0; q < 4; ++q) xq[k][q] = pq[q][ro];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool vr = row0 + 4 * w + 16 * (long)kb + k < rend;
            const double b = (vr && vb) ? (double)xb[k] - mb : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fma((vr && vq[q]) ? (double)xq[k][q] - mq[q] : 0.0, b, acc[q]);
        }
    }
    int it = nkb;
#else
    int it = 0;
#endif
    for (; it + 4 <= nkb; it += 4) {                       // four k-blocks' loads in flight (the k-blocks stay in order)
        float xa[4], xb[4];
        bool vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) vr[i] = load(it + i, xa[i], xb[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) mult(vr[i], xa[i], xb[i]);
    }
    for (; it < nkb; ++it) {
        float xa, xb;
        const bool vr = load(it, xa, xb);
        mult(vr, xa, xb);
    }
    // the f64 accumulator: lane l holds rows (l >> 4) + 4 q of column l & 15
    if (w > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) part[w - 1][q][l] = acc[q];
    }
    __syncthreads();
    if (w == 0) {
        double* dst = slab + ((size_t)sl * tri + e) * 256;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            dst[16 * ((l >> 4) + 4 * q) + (l & 15)] = ((acc[q] + part[0][q][l]) + part[1][q][l]) + part[2][q][l];
    }
}

// ---- S: entry k of tile e over the slabs, in slab order ----
__global__ __launch_bounds__(256) void hint_corr_sum_kernel(const double* __restrict__ slab, int tri, int slabs,
                                                            double* __restrict__ S) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    for (int sl = 0; sl < slabs; ++sl) s += slab[(size_t)sl * tri * 256 + k];
    S[k] = s;
}

// ---- r, both triangles from one value; the MSE's three sums in a fixed order ----
__global__ __launch_bounds__(hint::CORR_FIN_THREADS) void hint_corr_finish_kernel(const double* __restrict__ S, int d, int nt,
                                                                                  const double* __restrict__ target,
                                                                                  double* __restrict__ corr,
                                                                                  double* __restrict__ out) {
    __shared__ double sd[hint::CORR_MAX_D];
    __shared__ double red[3][hint::CORR_FIN_THREADS];
    for (int c = threadIdx.x; c < d; c += hint::CORR_FIN_THREADS) {
        const int t = c >> 4, k = c & 15;
        sd[c] = sqrt(S[(size_t)hint::corr_tri_first(nt, t) * 256 + 17 * k]);
    }
    __syncthreads();
    double sum = 0.0, cnt = 0.0, nans = 0.0;
    for (int idx = threadIdx.x; idx < d * d; idx += hint::CORR_FIN_THREADS) {
        const int i = idx / d, j = idx - i * d;
        const int a = i < j ? i : j, b = i < j ? j : i;
        const int ti = a >> 4, tj = b >> 4;
        const double s = S[(size_t)(hint::corr_tri_first(nt, ti) + (tj - ti)) * 256 + 16 * (a & 15) + (b & 15)];
        double r = s / (sd[a] * sd[b]);
        r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;           // (a NaN stays)
        if (corr) corr[idx] = r;
        if (r != r) nans += 1.0;
        if (target) {
            const double df = r - target[idx];
            if (df == df) {
                sum += df * df;
                cnt += 1.0;
            }
        }
    }
    red[0][threadIdx.x] = sum;
    red[1][threadIdx.x] = cnt;
    red[2][threadIdx.x] = nans;
    __syncthreads();
    for (int m = hint::CORR_FIN_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m)
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0][0] / red[1][0];                    // 0 / 0 = NaN when nothing was compared: np.nanmean's value
        out[1] = red[0][0];
        out[2] = red[1][0];
        out[3] = red[2][0];
    }
}

// ---- the C ABI ----
using namespace hint;

static int corr_check_sizes(const char* who, int32_t n, int32_t d) {
    if (n < 1) return fail("%s: n must be >= 1 (got %d)", who, n);
    if (d < 1) return fail("%s: d must be >= 1 (got %d)", who, d);
    if (n > CORR_MAX_N) return fail("%s: n = %d is above the limit of %d rows", who, n, CORR_MAX_N);
    if (d > CORR_MAX_D) return fail("%s: d = %d is above the limit of %d columns", who, d, CORR_MAX_D);
    return 0;
}

extern "C" {

size_t hint_corr_workspace_bytes(int32_t n, int32_t d) {
    if (corr_check_sizes("hint_corr_workspace_bytes", n, d)) return 0;
    return corr_layout(n, d).total;
}

int64_t hint_corr_job(int32_t n, int32_t d, int64_t j, int32_t field) {
    if (corr_check_sizes("hint_corr_job", n, d)) return -1;
    const CorrGeom g = corr_geom(n, d);
    const long long count = (long long)g.slabs * g.tri;
    if (j == -1 && field >= 0 && field <= 3) return field == 0 ? count : field == 1 ? CORR_T : field == 2 ? g.R : g.slabs;
    if (j < 0 || j >= count || field < 0 || field > 4) {
        fail("hint_corr_job: no job %lld / field %d (%lld jobs)", (long long)j, field, count);
        return -1;
    }
    const int sl = (int)(j / g.tri);
    int ti, tj;
    corr_tri_decode(g.nt, (int)(j % g.tri), &ti, &tj);
    const long long row0 = (long long)sl * g.R;
    const long long rows = std::min<long long>(g.R, (long long)n - row0);
    return field == 0 ? sl : field == 1 ? ti : field == 2 ? tj : field == 3 ? row0 : rows;
}

int hint_corr_run(const hint_corr_desc* desc, void* stream) {
    if (!desc) return fail("hint_corr_run: desc is null");
    if (!desc->x) return fail("hint_corr_run: x is null");
    if (!desc->out) return fail("hint_corr_run: out is null");
    if (workspace_null("hint_corr_run", desc->workspace)) return 1;
    if (!desc->target && !desc->corr) return fail("hint_corr_run: target and corr are both null: nothing to compute");
    if (corr_check_sizes("hint_corr_run", desc->n, desc->d)) return 1;
    if (check_aligned("hint_corr_run", {{"x", desc->x, 3}, {"target", desc->target, 7}, {"corr", desc->corr, 7}, {"out", desc->out, 7}}))
        return 1;
    const int n = desc->n, d = desc->d, Kp = corr_pad16(d);
    const CorrLayout L = corr_layout(n, d);
    if (workspace_fits("hint_corr_run", "corr", desc->workspace, desc->workspace_bytes, L.total)) return 1;

    const CorrGeom g = corr_geom(n, d);
    char* ws = (char*)desc->workspace;
    double* col = (double*)(ws + L.col);
    double* slab = (double*)(ws + L.slab);
    double* S = (double*)(ws + L.S);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hint_corr_colsum_kernel, dim3(Kp / 16, CORR_SLICES), dim3(256), 0, s, desc->x, n, d, Kp, col);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_corr_gram_kernel, dim3((unsigned)(g.slabs * g.tri)), dim3(256), 0, s, desc->x, n, d, Kp, g.nt, g.tri, g.R,
                       (const double*)col, slab);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_corr_sum_kernel, dim3(g.tri), dim3(256), 0, s, (const double*)slab, g.tri, g.slabs, S);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hint_corr_finish_kernel, dim3(1), dim3(CORR_FIN_THREADS), 0, s, (const double*)S, d, g.nt, desc->target,
                       desc->corr, desc->out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
