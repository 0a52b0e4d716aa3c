// Trainable Householder permutation between blocks (gfx950): the matrix of n reflections, its product with a batch of rows,
// and the gradients of both.
//
// Reference being replaced (read-only): configs/lens_shape/unconditional_hint_2_full.py:62-65 and its siblings put FrEIA's
// HouseholderPerm(fixed=False, n_reflections=ndim) between their blocks; FrEIA is neither vendored there nor installed here, so
// the parameterisation is THIS LIBRARY'S DEFINITION (FrEIA parity unpinned).  For Vs fp32 [n, d], row i the vector v_i:
//   H_i = I - 2 v_i v_i^T / (v_i . v_i),   W = H_0 H_1 .. H_(n-1)  [d, d] row-major,   y = x W  (transpose: y = x W^T),  log-det 0
//
//   hint_hh_build_kernel   one wavefront per row r of W: w = e_r, then w <- w - (2 (w . v_i) / (v_i . v_i)) v_i for i = 0 .. n-1, all
//                          in double; lane l keeps entries l and l + 64; a dot product is the lane's two terms added in that order,
//                          then a butterfly over the lanes (xor 32, 16, 8, 4, 2, 1: every lane ends with the same bits); each entry is
//                          rounded to fp32 once, at the store
//   hint_hh_apply_kernel   y = x M, M = W or W^T staged once per workgroup in LDS as M[k][j] with k padded to a multiple of 4 by
//                          zeros; a wavefront takes 16 rows at a time, stages them in LDS (coalesced, zeros past B and d) and
//                          runs v_mfma_f32_16x16x4_f32 over the k-blocks in ascending order for each 16-column tile.  A row's
//                          result depends on that row and W only.  Rows past B and columns past d are neither read nor written
//   hint_hh_gram_kernel    g_W = x^T g_y (transpose: g_y^T x): one workgroup per (row slab, tile row, tile column); wavefront w
//                          takes the slab's k-blocks w, w + 4, ..; the four partial tiles are added in wavefront order and go to the
//                          job's own slot of the workspace
//   hint_hh_finish_kernel  the slab slots of each entry added in slab order, in double -> g_W; then (one workgroup, g_V asked)
//                          g_V from that sum and Vs, in double, walking i = n-1 .. 0 with P = H_0 .. H_(i-1) and
//                          Gs = G (H_(i+1) .. H_(n-1))^T kept in the workspace (the header states the recurrence)
// hint_householder_many_run (the m permutations of one flow, trained by FlowTrainer(learned_perms=True)) runs the same device
// functions: hint_hh_build_many_kernel makes every matrix in one launch (grid y = the permutation), the row work of permutation j
// is the apply and gram kernels on slot j of the workspace, and hint_hh_finish_many_kernel gives every permutation's finish a
// workgroup of its own, so the m serial walks over the reflections run side by side - with Gs and P in LDS where they fit (d <= 94).
// No atomics, no counters: the same bits on every run.  Nothing special happens for a zero or non-finite v_i: the division gives NaN.
#include "hint_host.hpp"
#include "hint_device.hpp"
#include "hint_householder.hpp"

namespace hint {

constexpr int HH_T = 16;                    // tile edge (the MFMA's)
constexpr int HH_MAX_D = 128;
constexpr int HH_MAX_N = 256;
constexpr int HH_MAX_B = 1 << 22;
constexpr int HH_MIN_R = 256;               // rows per slab of the Gram, at least
constexpr int HH_MAX_SLABS = 64;            // ... and as many more as keep the slab count at this
constexpr int HH_MAX_GRID = 1024;           // workgroups of an apply launch, at most (each stages W once)
constexpr int HH_FIN_THREADS = 1024;
constexpr int HH_FIN_LDS_D = 94;            // the batched finish keeps Gs and P in LDS up to this d
// (2 d^2 doubles beside hh_finish's own 19 KiB of vectors and partial sums: 157.1 KiB at d = 94, 16 bytes too many at d = 95)
static_assert(2 * HH_FIN_LDS_D * HH_FIN_LDS_D * 8 + (3 + 2 * 8) * HH_MAX_D * 8 <= 160 * 1024, "the finish's matrices and vectors fit in LDS");
static_assert(2 * (HH_FIN_LDS_D + 1) * (HH_FIN_LDS_D + 1) * 8 + (3 + 2 * 8) * HH_MAX_D * 8 > 160 * 1024, "... and HH_FIN_LDS_D is the last d that does");

struct HhGeom { int nt, R, slabs; };
__host__ __device__ inline HhGeom hh_geom(int B, int d) {
    HhGeom g;
    g.nt = (d + HH_T - 1) / HH_T;
    int R = (B + HH_MAX_SLABS - 1) / HH_MAX_SLABS;
    R = (R + 15) & ~15;                                   // whole k-blocks of 4 rows for each of the four wavefronts
    g.R = R < HH_MIN_R ? HH_MIN_R : R;
    g.slabs = (B + g.R - 1) / g.R;
    return g;
}
// LDS of the apply kernel: M[kp][ld] (ld = 16 or 48 mod 64: the four k-rows of a B operand fall on four different groups of 16
// banks) and one [16][ldx] row tile per wavefront (ldx = 4 mod 64: a lane's A value (l & 15) ldx + (l >> 4) falls on its own bank)
struct HhLds { int kp, ld, ldx, bytes; };
__host__ __device__ inline HhLds hh_lds(int d) {
    HhLds s;
    s.kp = (d + 3) & ~3;
    s.ld = (d + 15) & ~15;
    if (s.ld % 32 == 0) s.ld += 16;
    s.ldx = s.kp <= 64 ? 68 : 132;
    s.bytes = 4 * (s.kp * s.ld + 4 * HH_T * s.ldx);
    return s;
}
// workspace of a grad run (bytes; every offset a multiple of 256):
//   [slab slots: slabs x nt x nt x 256 floats][Gs: d x d doubles][P: d x d doubles]
struct HhLayout { size_t part, Gs, P, total; };
inline HhLayout hh_layout(int B, int d) {
    const HhGeom g = hh_geom(B, d);
    HhLayout L;
    L.part = 0;
    L.Gs = L.part + (size_t)g.slabs * g.nt * g.nt * 256 * 4;
    const size_t mat = ((size_t)d * d * 8 + 255) & ~(size_t)255;
    L.P = L.Gs + mat;
    L.total = L.P + mat;
    return L;
}

}  // namespace hint

__device__ __forceinline__ double hh_wave_sum(double v) {      // every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- BUILD: wavefront w of block b makes row 4 b + w ----
__device__ __forceinline__ void hh_build_row(const float* __restrict__ Vs, int d, int n, float* __restrict__ W, int r, int l) {
    if (r >= d) return;                                     // (whole wavefronts: no barrier follows)
    const int c0 = l, c1 = l + 64;
    const bool ok0 = c0 < d, ok1 = c1 < d;
    double w0 = c0 == r ? 1.0 : 0.0, w1 = c1 == r ? 1.0 : 0.0;
    for (int i = 0; i < n; ++i) {
        const float* v = Vs + (size_t)i * d;
        const double v0 = ok0 ? (double)v[c0] : 0.0, v1 = ok1 ? (double)v[c1] : 0.0;
        const double dot = hh_wave_sum(w0 * v0 + w1 * v1);
        const double s = hh_wave_sum(v0 * v0 + v1 * v1);
        const double f = 2.0 * dot / s;
        w0 -= f * v0;
        w1 -= f * v1;
    }
    if (ok0) W[(size_t)r * d + c0] = (float)w0;
    if (ok1) W[(size_t)r * d + c1] = (float)w1;
}
__global__ __launch_bounds__(256) void hint_hh_build_kernel(const float* __restrict__ Vs, int d, int n, float* __restrict__ W) {
    hh_build_row(Vs, d, n, W, 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6), threadIdx.x & 63);
}
// ... of permutation blockIdx.y of m: the same rows from the same arithmetic, all permutations in one launch
__global__ __launch_bounds__(256) void hint_hh_build_many_kernel(const float* __restrict__ Vs, long vs_stride, int d, int n,
                                                                 float* __restrict__ W, long w_stride) {
    const long j = blockIdx.y;
    hh_build_row(Vs + j * vs_stride, d, n, W + j * w_stride, 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6), threadIdx.x & 63);
}

// ---- APPLY: y = x M, M[k][j] = W[k][j] (T = 0) or W[j][k] (T = 1) ----
__global__ __launch_bounds__(256) void hint_hh_apply_kernel(const float* __restrict__ x, const float* __restrict__ W, int B, int d,
                                                            int transpose, int kp, int ld, int ldx, float* __restrict__ y) {
    extern __shared__ float hh_smem[];
    float* Ml = hh_smem;                                   // [kp][ld]
    const int l = threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    float* Xl = hh_smem + kp * ld + w * 16 * ldx;        // [16][ldx], this wavefront's
    const int nt = (d + 15) >> 4;
    for (int idx = threadIdx.x; idx < kp * ld; idx += 256) {
        const int k = idx / ld, j = idx - k * ld;
        Ml[idx] = (k < d && j < d) ? (transpose ? W[(size_t)j * d + k] : W[(size_t)k * d + j]) : 0.f;
    }
    const int ntiles = (B + 15) >> 4;
    for (int t0 = 4 * (int)blockIdx.x; t0 < ntiles; t0 += 4 * (int)gridDim.x) {       // (uniform over the workgroup)
        const int tile = t0 + w;
        const long row0 = 16 * (long)tile;
        __syncthreads();                                    // M is staged; the previous tile's rows are read
        if (tile < ntiles)
            for (int idx = l; idx < 16 * kp; idx += 64) {
                const int r = idx / kp, c = idx - r * kp;
                Xl[r * ldx + c] = (row0 + r < B && c < d) ? x[(size_t)(row0 + r) * d + c] : 0.f;
            }
        __syncthreads();
        if (tile >= ntiles) continue;
        const float* ap = Xl + (l & 15) * ldx + (l >> 4);
        for (int jt = 0; jt < nt; ++jt) {
            const float* bp = Ml + (l >> 4) * ld + 16 * jt + (l & 15);
            hint::f32x4 acc = hint::zero4();
            for (int k = 0; k < kp; k += 4) acc = hint::mfma4(ap[k], bp[k * ld], acc);
            // lane l holds rows 4 (l >> 4) + q of column l & 15
            const int c = 16 * jt + (l & 15);
            if (c < d) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long r = row0 + 4 * (l >> 4) + q;
                    if (r < B) y[(size_t)r * d + c] = acc[q];
                }
            }
        }
    }
}

// ---- GRAM: one (slab, ti, tj) per workgroup; S[i][j] = sum_rows a[row][16 ti + i] b[row][16 tj + j] ----
__global__ __launch_bounds__(256) void hint_hh_gram_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int d,
                                                           int nt, int R, float* __restrict__ part) {
    __shared__ float red[3][4][64];
    const int tiles = nt * nt;
    const int sl = (int)blockIdx.x / tiles, e = (int)blockIdx.x % tiles;
    const int ti = e / nt, tj = e - ti * nt;
    const int l = threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int ca = 16 * ti + (l & 15), cb = 16 * tj + (l & 15);
    const bool va = ca < d, vb = cb < d;
    const long row0 = (long)sl * R;
    const long rend = row0 + R < (long)B ? row0 + R : (long)B;
    // every load is issued at an address clamped into the slab's rows and the matrix's columns (rend - 1 >= row0: no slab is
    // empty), and its value is replaced by an exact zero where the row or column does not exist
    const float* pa = a + (va ? ca : d - 1);
    const float* pb = b + (vb ? cb : d - 1);
    hint::f32x4 acc = hint::zero4();
    const int nkb = R / 16;                                // k-blocks of 4 rows of this wavefront (R is a multiple of 16)
    const long rl = row0 + 4 * w + (l >> 4);
    for (int it = 0; it < nkb; ++it) {
        const long r = rl + 16 * (long)it;
        const bool vr = r < rend;
        const size_t ro = (size_t)(vr ? r : rend - 1) * d;
        const float xa = pa[ro], xb = pb[ro];
        acc = hint::mfma4((vr && va) ? xa : 0.f, (vr && vb) ? xb : 0.f, acc);
    }
    if (w > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w - 1][q][l] = acc[q];
    }
    __syncthreads();
    if (w == 0) {
        float* dst = part + ((size_t)sl * tiles + e) * 256;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            dst[16 * (4 * (l >> 4) + q) + (l & 15)] = ((acc[q] + red[0][q][l]) + red[1][q][l]) + red[2][q][l];
    }
}

// ---- FINISH: the slab sum (workgroup wg of nwg a share of the entries), then g_V by the one workgroup of a run that asks for it ----
__device__ __forceinline__ void hh_finish(const float* __restrict__ part, int slabs, int nt, int d, int n, const float* __restrict__ W,
                                          const float* __restrict__ Vs, float* __restrict__ g_W, float* __restrict__ g_V,
                                          double* __restrict__ Gs, double* __restrict__ P, int wg, int nwg) {
    __shared__ double vs[hint::HH_MAX_D], av[hint::HH_MAX_D], bv[hint::HH_MAX_D];
    __shared__ double red[2][8][hint::HH_MAX_D];
    const int t = threadIdx.x;
    const size_t tiles = (size_t)nt * nt;
    for (int idx = wg * hint::HH_FIN_THREADS + t; idx < d * d; idx += nwg * hint::HH_FIN_THREADS) {
        const int i = idx / d, j = idx - i * d;
        const size_t off = ((size_t)(i >> 4) * nt + (j >> 4)) * 256 + 16 * (i & 15) + (j & 15);
        double s = 0.0;
        for (int sl = 0; sl < slabs; ++sl) s += (double)part[(size_t)sl * tiles * 256 + off];
        if (g_W) g_W[idx] = (float)s;
        if (g_V) {
            Gs[idx] = s;
            P[idx] = (double)W[idx];
        }
    }
    if (!g_V) return;                                       // (g_V: the grid is one workgroup)
    const int r2 = t >> 3, sub = t & 7;                     // mat-vec: eight lanes per row
    const int c3 = t & 127, part3 = t >> 7;                 // update and transposed mat-vec: eight threads per column
    for (int i = n - 1; i >= 0; --i) {
        __syncthreads();                                    // P, Gs of the previous step are in memory; its LDS values are read
        if (t < d) vs[t] = (double)Vs[(size_t)i * d + t];
        __syncthreads();
        double s = 0.0;
        for (int c = 0; c < d; ++c) s += vs[c] * vs[c];     // (every thread, the same order)
        // P holds H_0 .. H_i here: tv = P v_i = -(H_0 .. H_(i-1)) v_i
        double tp = 0.0, tb = 0.0;
        if (r2 < d)
            for (int c = sub; c < d; c += 8) {
                tp += P[(size_t)r2 * d + c] * vs[c];
                tb += Gs[(size_t)r2 * d + c] * vs[c];
            }
#pragma unroll
        for (int m = 4; m >= 1; m >>= 1) {
            tp += __shfl_xor(tp, m, 64);
            tb += __shfl_xor(tb, m, 64);
        }
        if (r2 < d && sub == 0) {
            av[r2] = -tp;
            bv[r2] = tb;
        }
        __syncthreads();
        const double f = 2.0 / s;
        double q = 0.0, qt = 0.0;
        if (c3 < d)
            for (int r = part3; r < d; r += 8) {
                const size_t o = (size_t)r * d + c3;
                const double p = P[o] + f * av[r] * vs[c3];            // P <- P H_i: H_0 .. H_(i-1)
                const double g = Gs[o];
                P[o] = p;
                q += p * bv[r];
                qt += g * av[r];
                Gs[o] = g - f * bv[r] * vs[c3];                         // Gs <- Gs H_i
            }
        red[0][part3][c3] = q;
        red[1][part3][c3] = qt;
        __syncthreads();
        if (t < d) {
            double qs = 0.0, ab = 0.0;
            for (int k = 0; k < 8; ++k) qs += red[0][k][t] + red[1][k][t];
            for (int r = 0; r < d; ++r) ab += av[r] * bv[r];
            g_V[(size_t)i * d + t] = (float)(-f * qs + (4.0 * ab / (s * s)) * vs[t]);
        }
    }
}
__global__ __launch_bounds__(hint::HH_FIN_THREADS) void hint_hh_finish_kernel(const float* __restrict__ part, int slabs, int nt,
                                                                              int d, int n, const float* __restrict__ W,
                                                                              const float* __restrict__ Vs, float* __restrict__ g_W,
                                                                              float* __restrict__ g_V, double* __restrict__ Gs,
                                                                              double* __restrict__ P) {
    hh_finish(part, slabs, nt, d, n, W, Vs, g_W, g_V, Gs, P, (int)blockIdx.x, (int)gridDim.x);
}
// ... of m permutations at once: workgroup j is the one workgroup of permutation j's finish, on slot j of the workspace (the
// serial walks over the reflections overlap on m compute units instead of following each other).  IN_LDS (d <= HH_FIN_LDS_D): Gs and
// P, the two d x d double matrices every reflection reads and rewrites, live in LDS instead of the slot - the same values through
// the same operations in the same order, so the same bits; the slot then holds the slab tiles alone
template <bool IN_LDS>
__global__ __launch_bounds__(hint::HH_FIN_THREADS) void hint_hh_finish_many_kernel(char* __restrict__ ws, long ws_stride, size_t off_Gs,
                                                                                   size_t off_P, int slabs, int nt, int d, int n,
                                                                                   const float* __restrict__ W, long w_stride,
                                                                                   const float* __restrict__ Vs, long vs_stride,
                                                                                   float* __restrict__ g_W, long gw_stride,
                                                                                   float* __restrict__ g_V, long gv_stride) {
    extern __shared__ double hh_fin_mats[];                 // IN_LDS: [Gs: d x d][P: d x d]
    const long j = blockIdx.x;
    char* slot = ws + j * ws_stride * 4;
    double* Gs = IN_LDS ? hh_fin_mats : (double*)(slot + off_Gs);
    double* P = IN_LDS ? hh_fin_mats + d * d : (double*)(slot + off_P);
    hh_finish((const float*)slot, slabs, nt, d, n, W + j * w_stride, Vs + j * vs_stride, g_W ? g_W + j * gw_stride : nullptr,
              g_V + j * gv_stride, Gs, P, 0, 1);
}

// ---- the C ABI ----
using namespace hint;

static int hh_check_sizes(const char* who, int32_t op, int32_t B, int32_t d, int32_t n) {
    if (op < HINT_HOUSEHOLDER_BUILD || op > HINT_HOUSEHOLDER_GRAD) return fail("%s: op = %d is not build (0), apply (1) or grad (2)", who, op);
    if (d < 1 || d > HH_MAX_D) return fail("%s: d = %d is outside 1..%d", who, d, HH_MAX_D);
    if (op != HINT_HOUSEHOLDER_APPLY && (n < 1 || n > HH_MAX_N)) return fail("%s: n = %d is outside 1..%d", who, n, HH_MAX_N);
    if (op != HINT_HOUSEHOLDER_BUILD && (B < 1 || B > HH_MAX_B)) return fail("%s: B = %d is outside 1..%d", who, B, HH_MAX_B);
    return 0;
}

static bool hh_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

static int hh_launch_apply(const float* x, const float* W, int B, int d, int transpose, float* y, hipStream_t s) {
    const HhLds L = hh_lds(d);
    if (L.bytes > 64 * 1024) {
        // once per device, for the largest d: no launch after the first sets an attribute (a captured run is preceded by a plain one)
        static std::mutex mu;
        static bool done[64] = {};
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 0 || dev >= 64 || !done[dev]) {
            HIP_TRY(hipFuncSetAttribute((const void*)hint_hh_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        hh_lds(HH_MAX_D).bytes));
            if (dev >= 0 && dev < 64) done[dev] = true;
        }
    }
    const int groups = cdiv(cdiv(B, HH_T), 4);
    hipLaunchKernelGGL(hint_hh_apply_kernel, dim3(std::min(groups, HH_MAX_GRID)), dim3(256), L.bytes, s, x, W, B, d, transpose, L.kp,
                       L.ld, L.ldx, y);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

size_t hint_householder_workspace_bytes(int32_t op, int32_t B, int32_t d, int32_t n) {
    if (hh_check_sizes("hint_householder_workspace_bytes", op, B, d, n)) return 0;
    return op == HINT_HOUSEHOLDER_GRAD ? hh_layout(B, d).total : 0;
}

int64_t hint_householder_geometry(int32_t B, int32_t d, int32_t field) {
    if (hh_check_sizes("hint_householder_geometry", HINT_HOUSEHOLDER_APPLY, B, d, 1)) return -1;
    if (field < 0 || field > 2) {
        fail("hint_householder_geometry: no field %d", field);
        return -1;
    }
    const HhGeom g = hh_geom(B, d);
    return field == 0 ? g.R : field == 1 ? g.slabs : g.nt;
}

int hint_householder_run(const hint_householder_desc* desc) {
    const char* who = "hint_householder_run";
    if (!desc) return fail("%s: desc is null", who);
    if (hh_check_sizes(who, desc->op, desc->B, desc->d, desc->n)) return 1;
    const int op = desc->op, B = desc->B, d = desc->d, n = desc->n, T = desc->transpose != 0;
    if (check_aligned(who, {{"Vs", desc->Vs, 3}, {"W", desc->W, 3}, {"x", desc->x, 3}, {"y", desc->y, 3}, {"g_y", desc->g_y, 3},
                            {"g_x", desc->g_x, 3}, {"g_W", desc->g_W, 3}, {"g_V", desc->g_V, 3}, {"workspace", desc->workspace, 15}}))
        return 1;
    hipStream_t s = (hipStream_t)desc->stream;
    if (op == HINT_HOUSEHOLDER_BUILD) {
        if (!desc->Vs) return fail("%s: Vs is null (build)", who);
        if (!desc->W) return fail("%s: W is null (build)", who);
        hipLaunchKernelGGL(hint_hh_build_kernel, dim3(cdiv(d, 4)), dim3(256), 0, s, desc->Vs, d, n, desc->W);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const size_t row_bytes = (size_t)B * d * 4;
    if (op == HINT_HOUSEHOLDER_APPLY) {
        if (!desc->x) return fail("%s: x is null (apply)", who);
        if (!desc->W) return fail("%s: W is null (apply)", who);
        if (!desc->y) return fail("%s: y is null (apply)", who);
        if (hh_overlap(desc->x, desc->y, row_bytes)) return fail("%s: y aliases x", who);
        return hh_launch_apply(desc->x, desc->W, B, d, T, desc->y, s);
    }
    const bool want_w = desc->g_W != nullptr, want_v = desc->g_V != nullptr;
    if (!desc->g_y) return fail("%s: g_y is null (grad)", who);
    if (!desc->W) return fail("%s: W is null (grad)", who);
    if (!desc->g_x && !want_w && !want_v) return fail("%s: g_x, g_W and g_V are all null: nothing to compute", who);
    if ((want_w || want_v) && !desc->x) return fail("%s: x is null (grad with g_W or g_V)", who);
    if (want_v && !desc->Vs) return fail("%s: Vs is null (grad with g_V)", who);
    if (desc->g_x && hh_overlap(desc->g_y, desc->g_x, row_bytes)) return fail("%s: g_x aliases g_y", who);
    const HhLayout L = hh_layout(B, d);
    if ((want_w || want_v) && (workspace_null(who, desc->workspace, "grad with g_W or g_V") ||
                               workspace_small(who, "householder", desc->workspace_bytes, L.total)))
        return 1;
    if (desc->g_x && hh_launch_apply(desc->g_y, desc->W, B, d, !T, desc->g_x, s)) return 1;
    if (want_w || want_v) {
        const HhGeom g = hh_geom(B, d);
        char* ws = (char*)desc->workspace;
        float* part = (float*)(ws + L.part);
        // forward: g_W = x^T g_y; transpose: g_W = g_y^T x
        hipLaunchKernelGGL(hint_hh_gram_kernel, dim3((unsigned)(g.slabs * g.nt * g.nt)), dim3(256), 0, s, T ? desc->g_y : desc->x,
                           T ? desc->x : desc->g_y, B, d, g.nt, g.R, part);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hint_hh_finish_kernel, dim3(want_v ? 1 : cdiv(d * d, HH_FIN_THREADS)), dim3(HH_FIN_THREADS), 0, s,
                           (const float*)part, g.slabs, g.nt, d, n, desc->W, desc->Vs, desc->g_W, desc->g_V, (double*)(ws + L.Gs),
                           (double*)(ws + L.P));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"

// ---- the launches of hint_householder_many_run (hint_householder_many.hip holds its checks): m permutations a stride apart ----
namespace hint {

HhLimits hh_limits() { return {HH_MAX_D, HH_MAX_N, HH_MAX_B}; }

size_t hh_grad_workspace_bytes(int B, int d) { return hh_layout(B, d).total; }

int hh_many_build(const float* Vs, int64_t vs_stride, float* W, int64_t w_stride, int m, int d, int n, hipStream_t s) {
    hipLaunchKernelGGL(hint_hh_build_many_kernel, dim3(cdiv(d, 4), m), dim3(256), 0, s, Vs, (long)vs_stride, d, n, W, (long)w_stride);
    HIP_TRY(hipGetLastError());
    return 0;
}

// g_x = g_y W^T (g_x may be null) and the slab partial tiles of x^T g_y into `slot`, a single grad run's workspace
int hh_many_rows(const float* x, const float* g_y, const float* W, float* g_x, void* slot, int B, int d, hipStream_t s) {
    const HhLayout L = hh_layout(B, d);
    const HhGeom g = hh_geom(B, d);
    if (g_x && hh_launch_apply(g_y, W, B, d, 1, g_x, s)) return 1;
    hipLaunchKernelGGL(hint_hh_gram_kernel, dim3((unsigned)(g.slabs * g.nt * g.nt)), dim3(256), 0, s, x, g_y, B, d, g.nt, g.R,
                       (float*)((char*)slot + L.part));
    HIP_TRY(hipGetLastError());
    return 0;
}

int hh_many_finish(void* ws, int64_t ws_stride, const float* W, int64_t w_stride, const float* Vs, int64_t vs_stride, float* g_W,
                   int64_t gw_stride, float* g_V, int64_t gv_stride, int m, int B, int d, int n, hipStream_t s) {
    const HhLayout L = hh_layout(B, d);
    const HhGeom g = hh_geom(B, d);
    if (d <= HH_FIN_LDS_D) {
        const int lds = 2 * d * d * 8;
        if (lds > 32 * 1024) {
            // once per device: no launch after the first sets an attribute (a captured run is preceded by a plain one)
            static std::mutex mu;
            static bool done[64] = {};
            int dev = 0;
            HIP_TRY(hipGetDevice(&dev));
            std::lock_guard<std::mutex> lock(mu);
            if (dev < 0 || dev >= 64 || !done[dev]) {
                HIP_TRY(hipFuncSetAttribute((const void*)hint_hh_finish_many_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            2 * HH_FIN_LDS_D * HH_FIN_LDS_D * 8));
                if (dev >= 0 && dev < 64) done[dev] = true;
            }
        }
        hipLaunchKernelGGL(hint_hh_finish_many_kernel<true>, dim3(m), dim3(HH_FIN_THREADS), lds, s, (char*)ws, (long)ws_stride, L.Gs, L.P,
                           g.slabs, g.nt, d, n, W, (long)w_stride, Vs, (long)vs_stride, g_W,
                           (long)gw_stride, g_V, (long)gv_stride);
    } else {
        hipLaunchKernelGGL(hint_hh_finish_many_kernel<false>, dim3(m), dim3(HH_FIN_THREADS), 0, s, (char*)ws, (long)ws_stride, L.Gs, L.P,
                           g.slabs, g.nt, d, n, W, (long)w_stride, Vs, (long)vs_stride, g_W,
                           (long)gw_stride, g_V, (long)gv_stride);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace hint
