// The core that the kernels measuring a traced curve against a point set are built from (hint_hausdorff.hip: a template in
// memory; hint_plus.hip: a plus shape's outline, generated on the fly; hint_lensfit.hip: a prototype placed anew every step of a
// fit).  Internal; described in DESIGN section 14.
// Everything here is part of the contract of include/hint_amd.h - the fp32 order of every operation and the association of the
// double sums - stated once, so that the kernels give the same bits on the same point sets (tests/test_gpu_plus.py
// test_the_generated_outline_is_the_host_built_template_bit_for_bit) and keep the ones tests/golden/pointset_bits.npz recorded.
// The size and source checks of these kernels' entry points are here as well, their message texts part of the behaviour (the
// checks every descriptor entry point shares are hint_host.hpp's).
//   B = the curve: P <= 1024 points in LDS, traced by hint_curve.hip's rule from P - 1 twiddles or given; thread t owns points
//       t, t + 256, ... (at most PS_PER = 4) and holds them in registers
//   A = the other set: M <= 4096 points that pass through LDS in tiles of 1024, made by the kernel's `fill`; thread t owns points
//       t, t + 256, ... of a tile
//   D(i, j) = fma(dy, dy, dx dx) of A_i - B_j;  mA_i = min_j D,  mB_j = min_i D
#pragma once
#include "hint_host.hpp"

namespace hint {

constexpr int PS_MAX_K = 25, PS_MIN_P = 2, PS_MAX_P = 1024;
constexpr int PS_MAX_M = 4096;                  // points of a row's set A
constexpr int PS_TILE = 1024;                   // of them in LDS at a time
constexpr int PS_THREADS = 256, PS_PER = 4;     // PS_PER = PS_MAX_P / PS_THREADS = PS_TILE / PS_THREADS points per thread
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr long long PS_MAX_N = 1LL << 30;

// the size checks of the entry points (with_curve false: the call reads no curve, and only the rows are checked)
inline int ps_check_sizes(const char* who, int64_t n_rows, int32_t n_coeffs, int32_t n_points, bool traced, bool with_curve = true) {
    if (n_rows < 1 || n_rows > PS_MAX_N) return fail("%s: n_rows must be 1..%lld (got %lld)", who, PS_MAX_N, (long long)n_rows);
    if (!with_curve) return 0;
    if (traced && (n_coeffs < 1 || n_coeffs > PS_MAX_K || (n_coeffs & 1) == 0))
        return fail("%s: n_coeffs must be odd and 1..%d (got %d)", who, PS_MAX_K, n_coeffs);
    if (n_points < PS_MIN_P || n_points > PS_MAX_P)
        return fail("%s: n_points must be %d..%d (got %d)", who, PS_MIN_P, PS_MAX_P, n_points);
    return 0;
}

// the curve has one source, x or b_points; needs: what the message says of a call that has neither, null when the call reads
// no curve
inline int ps_check_source(const char* who, const void* x, const void* b_points, const char* needs) {
    if (x && b_points) return fail("%s: both x and b_points are given (the curve has one source)", who);
    if (needs && !x && !b_points) return fail("%s: x and b_points are both null (%s)", who, needs);
    return 0;
}

}  // namespace hint

// the walk of both passes: NC points of this thread against n points in LDS.  Every read has one address for the whole wavefront
// (a broadcast, no bank conflict) and feeds NC times five vector operations.  (D is written for A_i - B_j; pass 2 holds B and
// walks A, and the differences there are the exact negatives, so the squares - and D - are the same bits.)
// ARG: the walk also says where - the minimum is replaced only by a strictly smaller D, so among equal D the lowest index of src
// stays (and a NaN never enters); at[c] starts at 0 and is always an index of src.  (hint_lensfit.hip recomputes the selected
// pair's difference from it for the gradient.)  Without ARG at is not looked at
template <int NC, bool ARG>
__device__ __forceinline__ void ps_walk(const float2* src, int n, const float (&px)[hint::PS_PER], const float (&py)[hint::PS_PER],
                                        float (&m)[hint::PS_PER], int* at) {
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float2 q = src[j];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float dx = __fsub_rn(px[c], q.x), dy = __fsub_rn(py[c], q.y);
            const float d = __fmaf_rn(dy, dy, __fmul_rn(dx, dx));
            if constexpr (ARG) {
                const bool lt = d < m[c];
                m[c] = lt ? d : m[c];
                at[c] = lt ? j : at[c];
            } else {
                m[c] = fminf(m[c], d);
            }
        }
    }
}

template <bool ARG>
__device__ __forceinline__ void ps_walk_n(int nc, const float2* src, int n, const float (&px)[hint::PS_PER],
                                          const float (&py)[hint::PS_PER], float (&m)[hint::PS_PER], int* at) {
    switch (nc) {                                            // (nc is the same for the whole workgroup)
        case 1: ps_walk<1, ARG>(src, n, px, py, m, at); break;
        case 2: ps_walk<2, ARG>(src, n, px, py, m, at); break;
        case 3: ps_walk<3, ARG>(src, n, px, py, m, at); break;
        default: ps_walk<4, ARG>(src, n, px, py, m, at); break;
    }
}

__device__ __forceinline__ void ps_scan_n(int nc, const float2* src, int n, const float (&px)[hint::PS_PER],
                                          const float (&py)[hint::PS_PER], float (&m)[hint::PS_PER]) {
    ps_walk_n<false>(nc, src, n, px, py, m, nullptr);
}

__device__ __forceinline__ void ps_scan_arg_n(int nc, const float2* src, int n, const float (&px)[hint::PS_PER],
                                              const float (&py)[hint::PS_PER], float (&m)[hint::PS_PER], int (&at)[hint::PS_PER]) {
    ps_walk_n<true>(nc, src, n, px, py, m, at);
}

// minima before a walk
__device__ __forceinline__ void ps_no_minima(float (&m)[hint::PS_PER]) {
#pragma unroll
    for (int c = 0; c < hint::PS_PER; ++c) m[c] = INFINITY;
}

// a point at a 4-byte aligned address: one 8-byte load all the same
__device__ __forceinline__ void ps_load_point(float2& a, const float* p) { __builtin_memcpy(&a, p, sizeof(a)); }

// where the parameters (x, y, scale, angle) put a point a: q = a R (the angle), then q scale + (x, y) - lens_points_from_params
struct ps_pose {
    float cs, sn, scale, x, y;
};

// the pose of pr = (x, y, scale, angle) to LDS, by one thread.  Not inlined: the double-precision sincos holds some thirty
// registers of constants, which would otherwise stay live across the whole row loop
inline __device__ __noinline__ void ps_stage_pose(const float* pr, ps_pose* ps) {
    double sn, cs;
    sincos((double)pr[3], &sn, &cs);
    ps->cs = (float)cs;
    ps->sn = (float)sn;
    ps->scale = pr[2];
    ps->x = pr[0];
    ps->y = pr[1];
}

// (the point by reference: handed over by value, the tile filler of hint_hausdorff.hip compiles to a branch a point where it is
// two selects now)
__device__ __forceinline__ float2 ps_rotate(const float2& a, float cs, float sn) {
    return make_float2(__fmaf_rn(-a.y, sn, __fmul_rn(a.x, cs)), __fmaf_rn(a.y, cs, __fmul_rn(a.x, sn)));
}

__device__ __forceinline__ float2 ps_place(const float2& a, const ps_pose& ps) {
    const float2 q = ps_rotate(a, ps.cs, ps.sn);
    return make_float2(__fmaf_rn(q.x, ps.scale, ps.x), __fmaf_rn(q.y, ps.scale, ps.y));
}

__device__ __forceinline__ double ps_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);             // (a + b = b + a: every lane ends with the same bits)
    return v;
}

__device__ __forceinline__ float ps_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ float ps_wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}

// once per workgroup: the P - 1 twiddles (cos, sin)(2 pi r / (P - 1)) to LDS, sincospi in double as hint_curve.hip does
__device__ __forceinline__ void ps_twiddles(float2* tw, int P, int t) {
    for (int r = t; r < P - 1; r += hint::PS_THREADS) {
        double sn, cs;
        sincospi(2.0 * (double)r / (double)(P - 1), &sn, &cs);
        tw[r] = make_float2((float)cs, (float)sn);
    }
}

// point tt of the curve with the coefficients coef[4K]: fmas over k ascending, real term then imaginary term.  Frequency m = k - K/2
// reads twiddle r = (|m| tt) mod (P - 1), stepped from one k to the next by adding or subtracting tt mod (P - 1): one integer
// modulo per point, none per term
__device__ __forceinline__ float2 ps_trace_point(const float2* tw, const float* coef, int K, int P, int tt) {
    const int Pm1 = P - 1, H = K / 2;
    const int t0 = tt == Pm1 ? 0 : tt;                                       // tt mod (P - 1)
    int r = (H * t0) % Pm1;
    float ax = 0.f, ay = 0.f;
    for (int k = 0; k < K; ++k) {
        const int m = k - H;
        float2 w = tw[r];
        if (m < 0) w.y = -w.y;
        ax = __fmaf_rn(coef[k], w.x, ax);
        ax = __fmaf_rn(-coef[2 * K + k], w.y, ax);
        ay = __fmaf_rn(coef[K + k], w.x, ay);
        ay = __fmaf_rn(-coef[3 * K + k], w.y, ay);
        if (m < 0) {                                                         // r of the next k: |m| goes down to 0, then up
            r -= t0;
            if (r < 0) r += Pm1;
        } else {
            r += t0;
            if (r >= Pm1) r -= Pm1;
        }
    }
    return make_float2(ax, ay);
}

// B of a row: points t, t + 256, ... to LDS (a rolled loop: one copy of the trace) - traced from coef (x != nullptr), and then
// also written to `points` if that is given, or loaded from b_points.  The caller's barrier makes Bp whole
__device__ __forceinline__ void ps_stage_curve(float2* Bp, const float2* tw, const float* coef, bool traced, const float* b_points,
                                               float* points, size_t row, int K, int P, int t) {
#pragma unroll 1
    for (int tt = t; tt < P; tt += hint::PS_THREADS) {
        float2 b;
        if (traced) {
            b = ps_trace_point(tw, coef, K, P, tt);
            if (points) {
                float* pp = points + 2 * (row * P + tt);
                pp[0] = b.x;
                pp[1] = b.y;
            }
        } else {
            const float* bp = b_points + 2 * (row * P + tt);
            b = make_float2(bp[0], bp[1]);
        }
        Bp[tt] = b;
    }
}

// this thread's points of a set of n in LDS; a slot past the end repeats the last point and is not counted by anything below
__device__ __forceinline__ void ps_own_points(const float2* src, int n, int t, float (&px)[hint::PS_PER], float (&py)[hint::PS_PER]) {
#pragma unroll
    for (int c = 0; c < hint::PS_PER; ++c) {
        const int i = t + hint::PS_THREADS * c;
        const float2 p = src[i < n ? i : n - 1];
        px[c] = p.x;
        py[c] = p.y;
    }
}

// a thread's part of a row's distances: the largest of its minima and, over its own points in ascending order, the double sums
// of the minima's roots and of the minima (squared distances) on both sides
struct ps_part {
    float mx = 0.f;                                          // (every D is >= 0 or NaN)
    double a_rt = 0.0, a_sq = 0.0, b_rt = 0.0, b_sq = 0.0;
};

// the two-sided minima of a row, 1 <= M <= 4096.  Bp is whole and bx, by are ps_own_points of it; Ap takes the tiles, whose
// point g (0 <= g < M) is fill(g).  Per tile, pass 1: the thread's A points of the tile walk all of B; pass 2: its B points walk
// the tile, their minima living in registers across the tiles.  (A fused single pass would need a minimum across lanes per
// point; two passes need none.)  Barriers: one before a tile is overwritten, one after it is filled; the caller's next barrier
// ends the last walk
template <class Fill>
__device__ __forceinline__ ps_part ps_two_sided(float2* Ap, const float2* Bp, int M, int P, int t, const float (&bx)[hint::PS_PER],
                                                const float (&by)[hint::PS_PER], Fill fill) {
    using namespace hint;
    ps_part s;
    const int ncB = (P + PS_THREADS - 1) / PS_THREADS;
    float mb[PS_PER];
    ps_no_minima(mb);
    for (int a0 = 0; a0 < M; a0 += PS_TILE) {
        const int cnt = M - a0 < PS_TILE ? M - a0 : PS_TILE;
        const int ncA = (cnt + PS_THREADS - 1) / PS_THREADS;
        if (a0) __syncthreads();                             // the walks of the tile before are done with Ap
#pragma unroll 1
        for (int i = t; i < cnt; i += PS_THREADS) Ap[i] = fill(a0 + i);
        __syncthreads();
        float px[PS_PER], py[PS_PER], ma[PS_PER];
        ps_own_points(Ap, cnt, t, px, py);
        ps_no_minima(ma);
        ps_scan_n(ncA, Bp, P, px, py, ma);                   // pass 1: mA of this thread's points of the tile
        ps_scan_n(ncB, Ap, cnt, bx, by, mb);                 // pass 2: mB so far
#pragma unroll
        for (int c = 0; c < PS_PER; ++c) {
            if (t + PS_THREADS * c < cnt) {                  // (then c < ncA)
                s.mx = fmaxf(s.mx, ma[c]);
                s.a_sq += (double)ma[c];
                s.a_rt += (double)__fsqrt_rn(ma[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < PS_PER; ++c) {
        if (t + PS_THREADS * c < P) {                        // (then c < ncB)
            s.mx = fmaxf(s.mx, mb[c]);
            s.b_sq += (double)mb[c];
            s.b_rt += (double)__fsqrt_rn(mb[c]);
        }
    }
    return s;
}

// the workgroup's maximum and NS double sums of the threads' values: six xor-shuffles within the wavefront, one LDS row per
// wavefront, then thread 0 adds the wavefronts in order - on return s and mx are the workgroup's in thread 0 (only).  Its barrier
// is also the one after which every walk of the row is done
template <int NS>
__device__ __forceinline__ void ps_block_reduce(double (&s)[NS], float& mx, double (*red)[NS], float* redm, int t) {
    mx = ps_wave_max(mx);
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = ps_wave_sum(s[q]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) red[t >> 6][q] = s[q];
        redm[t >> 6] = mx;
    }
    __syncthreads();
    if (t == 0) {
        mx = redm[0];
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] = red[0][q];
        for (int w = 1; w < hint::PS_WAVES; ++w) {
            mx = fmaxf(mx, redm[w]);
#pragma unroll
            for (int q = 0; q < NS; ++q) s[q] += red[w][q];
        }
    }
}
