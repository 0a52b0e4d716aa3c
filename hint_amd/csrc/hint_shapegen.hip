// The lens-shape prior sampler and points -> Fourier coefficients (gfx950): what feeds the evaluation pipeline.
//
// Reference being replaced (read-only): data.py:85-125 LensShapeModel.generate_lens_shape / sample_prior / sample_joint - one
// polygon-library intersection and one DFT per row in a Python loop, called for 1e8 prior rows by rejection_sampling.py:76-85
// prepare_samples and for the training and test sets by data.py:466-489 - and data.py:42-49 fourier_coeffs.
//
// The lens needs no polygon library.  With r0 = 1 + u_r and theta = 2 pi u_t the figure is r0 times a UNIT figure that depends on
// theta alone: A, the clockwise regular 64-gon e_j = (cos(2 pi j / 64), -sin(2 pi j / 64)) on the unit circle, and B = c + 2 e_j,
// c = 2.4 (sin theta, cos theta).  The closed clockwise ring of A n B is
//     P, the A_j strictly inside B (one run jlo..jhi), Q, the B_k strictly inside A (one run klo..khi), P
// where P is the crossing of A's edge (jlo - 1, jlo) with B's edge (khi, khi + 1) and Q that of (jhi, jhi + 1) with (klo - 1, klo).
// (The order of the ring's vertices is this project's definition; include/hint_amd.h states it, DESIGN section 21 the error bounds.)
//   classification  a point is inside a regular polygon when it is inside the half-plane whose normal is nearest its direction.
//       The centre of A's run, in vertex indices, is j* = 64 u_t - 16 - plain arithmetic on the draw, no inverse function - and
//       the circles cross 9.7598 indices either side of it; seen from B the run is centred at j* + 32 and ends 4.2937 either side.
//       Each end of each run is settled among the four vertices around the circles' crossing (the polygons' own crossing lies
//       within 0.05 of an index of it), each tested against the half-plane the crossing points at and its neighbours: one either
//       side for A's vertices (a step of A turns the direction seen from B by 0.1 of an index), two for B's (0.38).  No branch
//       depends on the rounding of a transcendental: sin and cos of theta enter the tests as values only.
//   a row            pass 1 sums the closed ring in ring order, pass 2 centres each point, q = fma(r0, p - mean, -n / 2), and adds it
//       to the accumulators of hint_fourier.hpp with twiddles from two tables (N = 31, 32: made in double on the host, rounded
//       once).  The ring is regenerated from the 64-entry table, never held in registers.  Every sum runs in ring order in one
//       lane: the bits do not depend on the grid, on n_rows or on where a row stands.
//   one row per lane, no workgroup barrier in the row loop: a wavefront stages its 64 rows of 80 bytes in its own LDS slice and
//       stores them as 320 contiguous 16-byte pieces (whole lines).
// hint_fcoef_kernel: one thread per (row, |m|), the same accumulators in the same order, twiddles by sincospi in double of the
// integer-reduced angle.
#include "hint_host.hpp"
#include "hint_fourier.hpp"
#include "hint_rowdraws.hpp"

namespace hint {

constexpr int LENS_SIDES = 64;
constexpr int LENS_WAVES = 4;                       // wavefronts of a workgroup, 64 rows each
constexpr int LENS_MAX_WG = 2048;                   // the grid cap: 256 CUs x 8
constexpr long long LENS_MAX_N = 1LL << 30;
constexpr int LENS_K = 5;                           // coefficients per axis (LensShapeModel.n_parameters / 4)
constexpr int LENS_ROW = 4 * LENS_K;
constexpr int LENS_RING = 32;                       // points of the ring output: the closed ring has 31 or 32
constexpr int LENS_MIN_OPEN = 30, LENS_MAX_OPEN = 31;
constexpr unsigned LENS_TAG = 0x4C454E53u;          // counter word 3: "LENS"
constexpr float LENS_HALF_A = 9.7598f;              // acos(0.575) in vertex indices: where the circles cross, seen from A ..
constexpr float LENS_HALF_B = 4.2937f;              // .. acos(0.9125), seen from B

constexpr int FCOEF_MAX_P = 1024;
constexpr long long FCOEF_MAX_N = 1LL << 24;
constexpr int FCOEF_MAX_WG = 8192;
constexpr RowGrid LENS_GRID{64, LENS_WAVES, LENS_MAX_WG, LENS_MAX_N};
constexpr RowGrid FCOEF_GRID{64, 4, FCOEF_MAX_WG, FCOEF_MAX_N};    // an item: a row's harmonic |m|, K / 2 + 1 of them a row

struct LensTables {
    float2 h[2 * LENS_SIDES];                       // (cos, -sin) of 2 pi i / 128: e_j = h[2 j], the outward normal of edge (j, j + 1) = h[2 j + 1]
    float2 tw[64];                                  // (cos, sin) of 2 pi r / N: N = 31 at [0, 31), N = 32 at [32, 64)
    float apo;                                      // cos(pi / 64), the unit polygon's apothem
};

struct LensArgs {
    long long n;
    unsigned long long seed, offset;
    const float4* draws;
    float4* x4;
    float2* ring;
    int32_t* counts;
    float2* eps;
    float4* draws_out;
    int32_t* rejected;
};

inline long long fcoef_items(long long n, int K) { return n * (K / 2 + 1); }

static const LensTables& lens_tables() {
    static const LensTables T = [] {
        LensTables t;
        for (int i = 0; i < 2 * LENS_SIDES; ++i) {
            const float2 w = fourier_twiddle(i, 2 * LENS_SIDES);
            t.h[i] = float2{w.x, -w.y};
        }
        for (int r = 0; r < 64; ++r) t.tw[r] = float2{0.f, 0.f};
        for (int r = 0; r < 31; ++r) t.tw[r] = fourier_twiddle(r, 31);
        for (int r = 0; r < 32; ++r) t.tw[32 + r] = fourier_twiddle(r, 32);
        t.apo = (float)std::cos(3.14159265358979323846 / LENS_SIDES);
        return t;
    }();
    return T;
}

}  // namespace hint

// max over the W edges around e0 of n_k . v, less R apothem: negative when v (relative to the polygon's centre) is strictly inside
template <int W>
__device__ __forceinline__ float lens_slack(const float2* hs, float vx, float vy, int e0, float r_apo) {
    float m = -INFINITY;
#pragma unroll
    for (int i = -(W / 2); i <= W / 2; ++i) {
        const float2 nk = hs[2 * ((e0 + i) & 63) + 1];
        m = fmaxf(m, fmaf(nk.y, vy, nk.x * vx));
    }
    return m - r_apo;
}

__global__ __launch_bounds__(256) void hint_lensgen_kernel(const hint::LensArgs a, const hint::LensTables T) {
    using namespace hint;
    __shared__ float2 hs[2 * LENS_SIDES];
    __shared__ float2 tw[64];
    __shared__ float4 stage[LENS_WAVES][64 * LENS_ROW / 4];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    if (tid < 2 * LENS_SIDES) hs[tid] = T.h[tid];
    else if (tid < 2 * LENS_SIDES + 64) tw[tid - 2 * LENS_SIDES] = T.tw[tid - 2 * LENS_SIDES];
    __syncthreads();
    const float apo = T.apo, apo2 = 2.f * T.apo;
    float* srow = (float*)&stage[wv][0] + l * LENS_ROW;
    const long long tiles = (a.n + 63) / 64, wave = (long long)blockIdx.x * LENS_WAVES + wv, nwaves = (long long)gridDim.x * LENS_WAVES;
    int rejected = 0;
    for (long long t = wave; t < tiles; t += nwaves) {
        const long long row = t * 64 + l;
        const bool valid = row < a.n;
        const long long rr = valid ? row : a.n - 1;            // (lanes past the end repeat the last row and store nothing)
        float4 d;
        if (a.draws) {
            d = a.draws[rr];
        } else {
            unsigned c[4];
            row_philox(a.seed, a.offset + (unsigned long long)rr, 0u, LENS_TAG, c);
            const float2 nm = row_box_muller(c[2], c[3]);
            d = float4{(float)c[0] * 2.3283064365386963e-10f, (float)c[1] * 2.3283064365386963e-10f, nm.x, nm.y};
        }
        if (a.draws_out && valid) a.draws_out[row] = d;
        if (a.eps && valid) {
            unsigned c[4];
            row_philox(a.seed, a.offset + (unsigned long long)row, 1u, LENS_TAG, c);
            a.eps[row] = row_box_muller(c[0], c[1]);
        }
        // ---- the unit figure ----
        const float r0 = 1.f + d.x;
        float st, ct;
        sincospif(2.f * d.y, &st, &ct);
        const float cx = 2.4f * st, cy = 2.4f * ct;
        const float js = fmaf(64.f, d.y, -16.f), ks = js + 32.f;
        const int fa_lo = (int)floorf(js - LENS_HALF_A), fa_hi = (int)floorf(js + LENS_HALF_A);
        const int fb_lo = (int)floorf(ks - LENS_HALF_B), fb_hi = (int)floorf(ks + LENS_HALF_B);
        int a_out = 0, a_in = 0, b_out = 0, b_in = 0;          // of the four candidates of each run's end
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 e0 = hs[2 * ((fa_lo - 1 + i) & 63)], e1 = hs[2 * ((fa_hi - 1 + i) & 63)];
            a_out += lens_slack<3>(hs, e0.x - cx, e0.y - cy, fb_hi, apo2) < 0.f ? 0 : 1;
            a_in += lens_slack<3>(hs, e1.x - cx, e1.y - cy, fb_lo, apo2) < 0.f ? 1 : 0;
            const float2 g0 = hs[2 * ((fb_lo - 1 + i) & 63)], g1 = hs[2 * ((fb_hi - 1 + i) & 63)];
            b_out += lens_slack<5>(hs, fmaf(2.f, g0.x, cx), fmaf(2.f, g0.y, cy), fa_hi, apo) < 0.f ? 0 : 1;
            b_in += lens_slack<5>(hs, fmaf(2.f, g1.x, cx), fmaf(2.f, g1.y, cy), fa_lo, apo) < 0.f ? 1 : 0;
        }
        const int jlo = fa_lo - 1 + a_out, jhi = fa_hi - 2 + a_in, klo = fb_lo - 1 + b_out, khi = fb_hi - 2 + b_in;
        int nA = jhi - jlo + 1, nB = khi - klo + 1;
        // the draws are what the definition takes (the figure is periodic in u_t: a value outside [0, 1] would pass for its
        // fraction), each end has an outside and an inside candidate, and the count is one the definition knows: anything else
        // is a rejected row - x = NaN, count 0, ring 0 - counted in the workspace
        const bool in_range = d.x >= 0.f && d.x <= 1.f && d.y >= 0.f && d.y <= 1.f && fabsf(d.z) < INFINITY && fabsf(d.w) < INFINITY;
        const bool ok = in_range && a_out >= 1 && a_out <= 3 && a_in >= 1 && a_in <= 3 && b_out >= 1 && b_out <= 3 && b_in >= 1 && b_in <= 3 &&
                        nA + nB + 2 >= LENS_MIN_OPEN && nA + nB + 2 <= LENS_MAX_OPEN;
        rejected += __popcll(__ballot(valid && !ok));
        if (!ok) nA = nB = 0;
        const int N = nA + nB + 3;
        const float fN = (float)N;
        auto cross = [&](int j0, int k) -> float2 {             // A's edge (j0, j0 + 1) with the line of B's edge (k, k + 1)
            const float2 v0 = hs[2 * (j0 & 63)], v1 = hs[2 * ((j0 + 1) & 63)], nk = hs[2 * (k & 63) + 1];
            const float s0 = fmaf(nk.y, v0.y - cy, nk.x * (v0.x - cx)) - apo2;
            const float s1 = fmaf(nk.y, v1.y - cy, nk.x * (v1.x - cx)) - apo2;
            const float tt = s0 / (s0 - s1);
            return float2{fmaf(tt, v1.x - v0.x, v0.x), fmaf(tt, v1.y - v0.y, v0.y)};
        };
        const float2 P = cross(jlo - 1, khi), Q = cross(jhi, klo - 1);
        // ---- pass 1: the mean of the closed ring ----
        float sx = P.x, sy = P.y;
        for (int i = 0; i < nA; ++i) {
            const float2 e = hs[2 * ((jlo + i) & 63)];
            sx += e.x;
            sy += e.y;
        }
        sx += Q.x;
        sy += Q.y;
        for (int i = 0; i < nB; ++i) {
            const float2 e = hs[2 * ((klo + i) & 63)];
            sx += fmaf(2.f, e.x, cx);
            sy += fmaf(2.f, e.y, cy);
        }
        sx += P.x;
        sy += P.y;
        const float mx = sx / fN, my = sy / fN, hx = -0.5f * d.z, hy = -0.5f * d.w;
        // ---- pass 2: centre, scale, add the noise; the coefficients ----
        DftAcc a0, a1, a2;
        int n = 0, r2 = 0;
        const int base = N == 32 ? 32 : 0;
        float2* ring = a.ring && valid ? a.ring + row * LENS_RING : nullptr;
        auto visit = [&](float px, float py) {
            const float qx = fmaf(r0, px - mx, hx), qy = fmaf(r0, py - my, hy);
            const float2 t1 = tw[base + n], t2 = tw[base + r2];
            dft_term(a0, qx, qy, 1.f, 0.f);
            dft_term(a1, qx, qy, t1.x, t1.y);
            dft_term(a2, qx, qy, t2.x, t2.y);
            if (ring) ring[n] = float2{qx, qy};
            ++n;
            r2 += 2;
            if (r2 >= N) r2 -= N;
        };
        if (ok) {
            visit(P.x, P.y);
            for (int i = 0; i < nA; ++i) {
                const float2 e = hs[2 * ((jlo + i) & 63)];
                visit(e.x, e.y);
            }
            visit(Q.x, Q.y);
            for (int i = 0; i < nB; ++i) {
                const float2 e = hs[2 * ((klo + i) & 63)];
                visit(fmaf(2.f, e.x, cx), fmaf(2.f, e.y, cy));
            }
            visit(P.x, P.y);
        }
        if (ring)
            for (int i = n; i < LENS_RING; ++i) ring[i] = float2{0.f, 0.f};
        if (a.counts && valid) a.counts[row] = n;
        if (ok) {
            dft_store(srow, LENS_K, 0, a0, fN);
            dft_store(srow, LENS_K, 1, a1, fN);
            dft_store(srow, LENS_K, 2, a2, fN);
        } else {
#pragma unroll
            for (int i = 0; i < LENS_ROW; ++i) srow[i] = __builtin_nanf("");
        }
        // ---- the tile's rows, LDS -> x as contiguous 16-byte pieces ----
        shapegen_wave_sync();
        const long long left = a.n - t * 64;
        const int pieces = (int)(left < 64 ? left : 64) * (LENS_ROW / 4);
        float4* dst = a.x4 + t * (64 * LENS_ROW / 4);
#pragma unroll
        for (int i = 0; i < LENS_ROW / 4; ++i)
            if (l + 64 * i < pieces) dst[l + 64 * i] = stage[wv][l + 64 * i];
        shapegen_wave_sync();
    }
    if (l == 0) a.rejected[wave] = rejected;
}

__global__ __launch_bounds__(256) void hint_fcoef_kernel(const float2* __restrict__ pts, const int32_t* __restrict__ counts, long long n,
                                                         int P, int K, float* __restrict__ x, int32_t* __restrict__ rejected) {
    using namespace hint;
    const int H = K / 2 + 1;
    const long long total = n * H;
    int rej = 0;
    for (long long i0 = (long long)blockIdx.x * 256; i0 < total; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + threadIdx.x;
        const bool valid = i < total;
        const long long row = valid ? i / H : 0;
        const int h = valid ? (int)(i - row * H) : 0;
        const int cnt = counts ? counts[row] : P;
        const bool ok = cnt >= K && cnt <= P;                  // (so h <= K / 2 < cnt, and the output's width never depends on a row)
        DftAcc acc;
        if (valid && ok) {
            const float2* p = pts + row * P;
            int r = 0;
            for (int k = 0; k < cnt; ++k) {
                const float2 q = p[k], w = fourier_twiddle(r, cnt);
                dft_term(acc, q.x, q.y, w.x, w.y);
                r += h;
                if (r >= cnt) r -= cnt;
            }
        } else {
            acc.c0 = acc.s0 = acc.c1 = acc.s1 = __builtin_nanf("");
        }
        if (valid) dft_store(x + row * 4 * K, K, h, acc, (float)cnt);
        rej += __popcll(__ballot(valid && !ok && h == 0));
    }
    if ((threadIdx.x & 63) == 0) rejected[blockIdx.x * 4 + (threadIdx.x >> 6)] = rej;
}

// ---- the C ABI ----
using namespace hint;

static int fcoef_check_sizes(const char* who, int64_t n_rows, int32_t p_max, int32_t n_coeffs) {
    if (FCOEF_GRID.check_rows(who, n_rows)) return 1;
    if (n_coeffs < 1 || n_coeffs > FOURIER_MAX_K || n_coeffs % 2 == 0)
        return fail("%s: n_coeffs must be odd, 1..%d (got %d)", who, FOURIER_MAX_K, n_coeffs);
    if (p_max < n_coeffs || p_max > FCOEF_MAX_P) return fail("%s: p_max must be n_coeffs..%d (got %d)", who, FCOEF_MAX_P, p_max);
    return 0;
}

extern "C" {

size_t hint_lensgen_workspace_bytes(int64_t n_rows) {
    if (LENS_GRID.check_rows("hint_lensgen_workspace_bytes", n_rows)) return 0;
    return LENS_GRID.ws_bytes(n_rows);
}

int hint_lensgen_run(const hint_lensgen_desc* desc, void* stream) {
    const char* who = "hint_lensgen_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->x) return fail("%s: x is null", who);
    if (workspace_null(who, desc->workspace)) return 1;
    if (LENS_GRID.check_rows(who, desc->n_rows)) return 1;
    if (check_row_offset(who, desc->offset, desc->n_rows)) return 1;
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"draws", desc->draws, 15}, {"x", desc->x, 15}, {"ring", desc->ring, 7}, {"counts", desc->counts, 3},
                            {"eps", desc->eps, 7}, {"draws_out", desc->draws_out, 15}}))
        return 1;
    const int wgs = LENS_GRID.groups(desc->n_rows, desc->max_groups);
    const size_t need = LENS_GRID.ws_bytes(desc->n_rows);
    if (workspace_fits(who, "lensgen", desc->workspace, desc->workspace_bytes, need)) return 1;
    LensArgs a;
    a.n = desc->n_rows;
    a.seed = desc->seed;
    a.offset = desc->offset;
    a.draws = (const float4*)desc->draws;
    a.x4 = (float4*)desc->x;
    a.ring = (float2*)desc->ring;
    a.counts = desc->counts;
    a.eps = (float2*)desc->eps;
    a.draws_out = (float4*)desc->draws_out;
    a.rejected = (int32_t*)desc->workspace;
    hipStream_t s = (hipStream_t)stream;
    if (LENS_GRID.clear_tail(wgs, desc, need, s)) return 1;
    hipLaunchKernelGGL(hint_lensgen_kernel, dim3(wgs), dim3(256), 0, s, a, lens_tables());
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t hint_fcoef_workspace_bytes(int64_t n_rows, int32_t p_max, int32_t n_coeffs) {
    if (fcoef_check_sizes("hint_fcoef_workspace_bytes", n_rows, p_max, n_coeffs)) return 0;
    return FCOEF_GRID.ws_bytes(fcoef_items(n_rows, n_coeffs));
}

int hint_fcoef_run(const hint_fcoef_desc* desc, void* stream) {
    const char* who = "hint_fcoef_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->points) return fail("%s: points is null", who);
    if (!desc->x) return fail("%s: x is null", who);
    if (workspace_null(who, desc->workspace)) return 1;
    if (fcoef_check_sizes(who, desc->n_rows, desc->p_max, desc->n_coeffs)) return 1;
    if (check_groups(who, desc->max_groups)) return 1;
    if (check_aligned(who, {{"points", desc->points, 7}, {"counts", desc->counts, 3}, {"x", desc->x, 3}})) return 1;
    const long long items = fcoef_items(desc->n_rows, desc->n_coeffs);
    const int wgs = FCOEF_GRID.groups(items, desc->max_groups);
    const size_t need = FCOEF_GRID.ws_bytes(items);
    if (workspace_fits(who, "fcoef", desc->workspace, desc->workspace_bytes, need)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (FCOEF_GRID.clear_tail(wgs, desc, need, s)) return 1;
    hipLaunchKernelGGL(hint_fcoef_kernel, dim3(wgs), dim3(256), 0, s, (const float2*)desc->points, desc->counts, (long long)desc->n_rows,
                       desc->p_max, desc->n_coeffs, desc->x, (int32_t*)desc->workspace);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
