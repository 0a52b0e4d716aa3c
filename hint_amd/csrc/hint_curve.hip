// Lens-shape simulator (gfx950): Fourier curve -> largest diameter -> the two observed features, and their distance to a target.
//
// Reference being replaced (read-only): data.py:127-139 LensShapeModel.forward_process - a Python loop over rows around
// trace_fourier_curves (data.py:51-57), a 100 x 100 pdist / squareform matrix and its argmax, on the CPU - and
// rejection_sampling.py:99-102 mean_target_distance, called at :204 once per model and run on 4000 posterior samples;
// prepare_samples (rejection_sampling.py:76-85) runs the same simulator over the 1e8 prior rows.
// For x [N, 4K] (K odd; x[:, :2K] the real parts as [2 axes, K], x[:, 2K:] the imaginary parts; coefficient k of an axis belongs
// to frequency m = k - K/2) and P points:
//   twiddle  (c, s)(m, t) = (cos, sin)(2 pi r / (P - 1)), r = (|m| t) mod (P - 1) in integers, evaluated as sincospi(2 r / (P - 1))
//            in double and rounded to fp32; s changes sign for m < 0.  Point P - 1 therefore repeats point 0 bit for bit.
//   curve    p[t, axis] = acc after  acc = 0;  for k = 0 .. K - 1:  acc = fma(re[axis, k], c, acc);  acc = fma(-im[axis, k], s, acc)
//   D(i, j)  = fma(dy, dy, dx dx), dx = p_i.x - p_j.x, dy = p_i.y - p_j.y, for i < j; the chosen pair is the first maximum in
//            row-major (i, j) order; a NaN D never wins and the start value is pair (0, 1)
//   y[row]   = (p_j.y - p_i.y, p_j.x - p_i.x), each fma(noise, eps, .) when eps is given
//   dist     = sqrt(fma(d1, d1, d0 d0)), d = y[row] - target;  mean = (sum of dist in double, in a fixed order) / N as fp32
// (fp32, every operation rounded once; written with the _rn intrinsics, so that no pass can contract or reorder it differently.)
//
// hint_curve_kernel: a persistent grid of G workgroups of four wavefronts.  Each workgroup builds the twiddle table once in LDS,
// (K/2 + 1) x P pairs by parity; after that its wavefronts never meet again.  Wavefront q = 4 w + v owns the consecutive rows
// [q R, min(N, (q + 1) R)), R = ceil(N / 4G), one row per turn:
//   - the row's 4K coefficients go from global memory (one coalesced read, issued a turn ahead) to the wavefront's LDS slot;
//   - lane l traces points l and l + 64 into the wavefront's LDS slot of P float2;
//   - lane l <= (P - 1) / 2 scans the pairs of i = l and then of i' = P - 1 - l: P - 1 - l + l = P - 1 pairs for every lane, so the
//     triangle is balanced without a table; p_i, p_i' stay in registers and step s reads p_j at consecutive LDS addresses across
//     the lanes.  A lane meets its pairs in ascending (i, j) order and keeps (D, i P + j) under a strict >;
//   - six xor-shuffles reduce the lanes by (larger D, then lower index), which makes the tie rule independent of the lane mapping;
//   - lane 0 writes y and dist once and adds dist to the wavefront's double partial.
// The partials of all 4G wavefronts (empty ones write 0) are written to the workspace in row order; hint_curve_mean_kernel adds
// them in that order (256 consecutive chunks, then the chunk sums in order).  No float atomics, no counters, nothing carried
// between rows but the partial: a row's y and dist are the same bits wherever it stands and whatever G is.
// Why a wavefront per row and not a narrower lane group with several p_i per lane: with i and P - 1 - i on one lane every lane has
// the same trip count and each step is one conflict-free 8-byte LDS read for ~12 vector operations, so LDS is not the limit
// (4 SIMDs x 1 read per ~12 operations against one LDS port), no lane sits idle beyond 2 l > P - 1, and no workgroup barrier
// stands in the row loop.  Untuned: see DESIGN section 12.
#include "hint_host.hpp"

namespace hint {

constexpr int CURVE_MAX_K = 25, CURVE_MAX_P = 128, CURVE_MIN_P = 2;
constexpr int CURVE_WAVES = 4;                  // wavefronts of a workgroup = rows a workgroup has in flight (a tile)
constexpr int CURVE_MAX_WG = 2048;              // the grid cap: 256 CUs x 8 workgroups (32 wavefronts a CU, ~20 KB LDS each)
constexpr long long CURVE_MAX_N = 1LL << 30;
constexpr int CURVE_MAX_H = CURVE_MAX_K / 2 + 1;

struct CurveGeom { int wgs; long long rows; };          // workgroups, rows per wavefront
inline CurveGeom curve_geom(long long n, int max_groups) {
    long long g = (n + CURVE_WAVES - 1) / CURVE_WAVES;
    const long long cap = max_groups > 0 && max_groups < CURVE_MAX_WG ? max_groups : CURVE_MAX_WG;
    if (g > cap) g = cap;
    CurveGeom G;
    G.wgs = (int)g;
    G.rows = (n + g * CURVE_WAVES - 1) / (g * CURVE_WAVES);
    return G;
}
inline size_t curve_ws_bytes() { return (size_t)CURVE_MAX_WG * CURVE_WAVES * sizeof(double); }

}  // namespace hint

// LDS writes of some lanes, reads of others, within one wavefront: DS operations of a wavefront execute in order, so all that is
// needed is that the compiler keeps them in order too
__device__ __forceinline__ void curve_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void hint_curve_kernel(const float* __restrict__ x, long long n, int K, int P, long long rows_per_wave,
                                                         const float* __restrict__ eps, float noise,
                                                         const float* __restrict__ target, float* __restrict__ y,
                                                         float* __restrict__ dist, double* __restrict__ partial) {
    __shared__ float2 tw[hint::CURVE_MAX_H * hint::CURVE_MAX_P];                    // [|m|][t]
    __shared__ float coef[hint::CURVE_WAVES][4 * hint::CURVE_MAX_K + 4];
    __shared__ float2 pts[hint::CURVE_WAVES][hint::CURVE_MAX_P];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int H = K / 2 + 1, C = 4 * K;
    for (int e = t; e < H * P; e += 256) {
        const int m = e / P, tt = e - m * P;
        const int r = (m * tt) % (P - 1);
        double sn, cs;
        sincospi(2.0 * (double)r / (double)(P - 1), &sn, &cs);
        tw[e] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
    const long long q = (long long)blockIdx.x * hint::CURVE_WAVES + wv;
    const long long r0 = q * rows_per_wave < n ? q * rows_per_wave : n;
    const long long r1 = r0 + rows_per_wave < n ? r0 + rows_per_wave : n;
    float* cf = coef[wv];
    float2* pt = pts[wv];
    const bool with_t = target != nullptr;
    const float t0 = with_t ? target[0] : 0.f, t1 = with_t ? target[1] : 0.f;
    // the pairs of this lane: i = l (P - 1 - l of them), then i2 = P - 1 - l (l of them; none when i2 == i)
    const int i2 = P - 1 - l;
    const bool scans = l <= i2;
    const int n1 = scans ? i2 : 0;
    const int steps = !scans ? 0 : i2 > l ? P - 1 : n1;
    double acc = 0.0;
    float nx0 = 0.f, nx1 = 0.f;
    if (r0 < r1) {
        const float* xr = x + (size_t)r0 * C;
        if (l < C) nx0 = xr[l];
        if (l + 64 < C) nx1 = xr[l + 64];
    }
    for (long long row = r0; row < r1; ++row) {
        if (l < C) cf[l] = nx0;
        if (l + 64 < C) cf[l + 64] = nx1;
        if (row + 1 < r1) {                                  // the next row's coefficients, a turn ahead
            const float* xr = x + (size_t)(row + 1) * C;
            if (l < C) nx0 = xr[l];
            if (l + 64 < C) nx1 = xr[l + 64];
        }
        curve_wave_sync();
        // ---- the curve: points l and l + 64 ----
        float2 pa = make_float2(0.f, 0.f), pb = pa;          // p_i and p_i2 of the scan
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int tt = l + 64 * half;
            if (tt < P) {
                float ax = 0.f, ay = 0.f;
                for (int k = 0; k < K; ++k) {
                    const int m = k - K / 2;
                    float2 w = tw[(m < 0 ? -m : m) * P + tt];
                    if (m < 0) w.y = -w.y;
                    ax = __fmaf_rn(cf[k], w.x, ax);
                    ax = __fmaf_rn(-cf[2 * K + k], w.y, ax);
                    ay = __fmaf_rn(cf[K + k], w.x, ay);
                    ay = __fmaf_rn(-cf[3 * K + k], w.y, ay);
                }
                pt[tt] = make_float2(ax, ay);
                if (half == 0) pa = make_float2(ax, ay);
            }
        }
        curve_wave_sync();
        if (scans) pb = pt[i2];
        // ---- the diameter ----
        float bestD = -1.f;
        int bestI = 1;                                       // pair (0, 1)
        for (int s = 0; s < steps; ++s) {
            const bool first = s < n1;
            const int j = first ? l + 1 + s : i2 + 1 + (s - n1);
            const float2 a = first ? pa : pb;
            const float2 b = pt[j];
            const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y);
            const float D = __fmaf_rn(dy, dy, __fmul_rn(dx, dx));
            const int idx = (first ? l : i2) * P + j;
            if (D > bestD) {                                 // (false for a NaN D)
                bestD = D;
                bestI = idx;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float oD = __shfl_xor(bestD, m, 64);
            const int oI = __shfl_xor(bestI, m, 64);
            if (oD > bestD || (oD == bestD && oI < bestI)) {
                bestD = oD;
                bestI = oI;
            }
        }
        if (l == 0) {
            const int bi = bestI / P, bj = bestI - bi * P;
            const float2 p0 = pt[bi], p1 = pt[bj];
            float y0 = __fsub_rn(p1.y, p0.y), y1 = __fsub_rn(p1.x, p0.x);
            if (eps) {
                y0 = __fmaf_rn(noise, eps[2 * (size_t)row], y0);
                y1 = __fmaf_rn(noise, eps[2 * (size_t)row + 1], y1);
            }
            y[2 * (size_t)row] = y0;
            y[2 * (size_t)row + 1] = y1;
            if (with_t) {
                const float d0 = __fsub_rn(y0, t0), d1 = __fsub_rn(y1, t1);
                const float ds = sqrtf(__fmaf_rn(d1, d1, __fmul_rn(d0, d0)));
                if (dist) dist[row] = ds;
                acc += (double)ds;
            }
        }
        curve_wave_sync();                                   // the next turn overwrites cf and pt
    }
    if (partial && l == 0) partial[q] = acc;
}

// ---- the mean: n_part partials in order - thread t its consecutive chunk, then thread 0 the 256 chunk sums ----
__global__ __launch_bounds__(256) void hint_curve_mean_kernel(const double* __restrict__ partial, int n_part, long long n,
                                                              float* __restrict__ mean) {
    __shared__ double part[256];
    const int t = threadIdx.x, per = (n_part + 255) / 256;
    double s = 0.0;
    for (int i = t * per; i < (t + 1) * per && i < n_part; ++i) s += partial[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int i = 0; i < 256; ++i) v += part[i];
        mean[0] = (float)(v / (double)n);
    }
}

// ---- the C ABI ----
using namespace hint;

static int curve_check_sizes(const char* who, int64_t n_rows, int32_t n_coeffs, int32_t n_points) {
    if (n_rows < 1 || n_rows > CURVE_MAX_N)
        return fail("%s: n_rows must be 1..%lld (got %lld)", who, CURVE_MAX_N, (long long)n_rows);
    if (n_coeffs < 1 || n_coeffs > CURVE_MAX_K || (n_coeffs & 1) == 0)
        return fail("%s: n_coeffs must be odd and 1..%d (got %d)", who, CURVE_MAX_K, n_coeffs);
    if (n_points < CURVE_MIN_P || n_points > CURVE_MAX_P)
        return fail("%s: n_points must be %d..%d (got %d)", who, CURVE_MIN_P, CURVE_MAX_P, n_points);
    return 0;
}

extern "C" {

size_t hint_curve_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points) {
    if (curve_check_sizes("hint_curve_workspace_bytes", n_rows, n_coeffs, n_points)) return 0;
    return curve_ws_bytes();
}

int64_t hint_curve_geometry(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int32_t field) {
    if (curve_check_sizes("hint_curve_geometry", n_rows, n_coeffs, n_points)) return -1;
    if (field < 0 || field > 3) {
        fail("hint_curve_geometry: no field %d (0 workgroups, 1 rows per tile, 2 rows per wavefront, 3 the grid cap)", field);
        return -1;
    }
    const CurveGeom g = curve_geom(n_rows, 0);
    return field == 0 ? g.wgs : field == 1 ? CURVE_WAVES : field == 2 ? g.rows : CURVE_MAX_WG;
}

int hint_curve_run(const hint_curve_desc* desc, void* stream) {
    if (!desc) return fail("hint_curve_run: desc is null");
    if (!desc->x) return fail("hint_curve_run: x is null");
    if (!desc->y) return fail("hint_curve_run: y is null");
    if (curve_check_sizes("hint_curve_run", desc->n_rows, desc->n_coeffs, desc->n_points)) return 1;
    if (desc->dist && !desc->target) return fail("hint_curve_run: dist needs a target (target is null)");
    if (desc->mean && !desc->target) return fail("hint_curve_run: mean needs a target (target is null)");
    const char* who = "hint_curve_run";
    if (check_groups(who, desc->max_groups)) return 1;
    if (!std::isfinite(desc->noise)) return fail("hint_curve_run: noise must be finite");
    if (check_aligned(who, {{"x", desc->x, 3}, {"eps", desc->eps, 3}, {"target", desc->target, 3}, {"y", desc->y, 3},
                               {"dist", desc->dist, 3}, {"mean", desc->mean, 3}}))
        return 1;
    if (desc->mean && (workspace_null(who, desc->workspace, "mean needs one") ||
                       workspace_fits(who, "curve", desc->workspace, desc->workspace_bytes, curve_ws_bytes())))
        return 1;
    const CurveGeom g = curve_geom(desc->n_rows, desc->max_groups);
    hipStream_t s = (hipStream_t)stream;
    double* partial = desc->mean ? (double*)desc->workspace : nullptr;
    hipLaunchKernelGGL(hint_curve_kernel, dim3(g.wgs), dim3(256), 0, s, desc->x, (long long)desc->n_rows, desc->n_coeffs,
                       desc->n_points, g.rows, desc->eps, desc->noise, desc->target, desc->y, desc->dist, partial);
    HIP_TRY(hipGetLastError());
    if (desc->mean) {
        hipLaunchKernelGGL(hint_curve_mean_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, g.wgs * CURVE_WAVES,
                           (long long)desc->n_rows, desc->mean);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
