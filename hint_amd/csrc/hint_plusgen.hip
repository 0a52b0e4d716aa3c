// The plus-shape sampler (gfx950): prior, joint and targeted rows, what feeds the plus shape's evaluation pipeline.
//
// Reference being replaced (read-only): data.py:176-252 PlusShapeModel.densify_polyline / generate_plus_shape / sample_prior /
// sample_joint - one polygon-library union, one densify_polyline and one 25-coefficient DFT per row in a Python loop, called for
// the training and test sets (data.py:466-489), for the 1e8-row prior (rejection_sampling.py:76-85) and by the rejection loop of
// the ground-truth conditional sample (rejection_sampling.py:113-127).
//
// The union needs no polygon library: two axis-aligned bars that both contain the origin.  Four comparisons say which arms
// stand out; a 16-entry table (9 entries can occur) gives the clockwise ring of 8 or 12 corners as coordinate indices, in the
// manner of PL_VX / PL_VY (include/hint_amd.h hint_plusgen_desc states the ring; THE ORDER OF ITS VERTICES IS THIS PROJECT'S
// DEFINITION).
//   a row      16 lanes (a quarter wavefront); a wavefront holds 4 rows, a workgroup 16.  All 16 lanes compute the row's draws,
//       parameters and sincos (lock-step: it costs what one lane would).  Lane e < corners owns edge e: its count, then its dense
//       points to LDS.  The dense outline lives in LDS (1 KiB a row), never in registers.
//   the mean   lane k adds the points k, k + 16, .. in ascending order; the 16 partial sums are added in ascending lane order: a
//       fixed tree, the same bits in every lane, whatever the grid, n_rows or the row's place.
//   labels only (x and outline NULL): the row ends here - no second pass, no twiddles, no DFT.
//   pass 2     lanes over points: centre, rotate, offset (hint_plusgeom.hpp's pl_place: one definition of the placement), in place
//       in LDS and to `outline`.  Twiddles: N takes some fifty values, so there is a per-row table in LDS of the N values
//       sincospi(2 r / N) in double, rounded once - r <= N / 2 evaluated, the rest mirrored (cos, -sin), exact for the true values -
//       about N / 2 evaluations a row instead of 13 N.  DFT: lane m <= 12 runs the accumulators of hint_fourier.hpp over n
//       ascending, reading point n and twiddle (m n) mod N from LDS.
//   output     a wavefront's 4 rows of 400 bytes leave through LDS as 100 contiguous 16-byte pieces.
// One launch, no atomics, no workgroup barrier in the row loop (a row never leaves its wavefront).
#include "hint_host.hpp"
#include "hint_fourier.hpp"
#include "hint_rowdraws.hpp"
#include "hint_plusgeom.hpp"

namespace hint {

constexpr int PG_LANES = 16;                        // lanes of a row
constexpr int PG_WAVE_ROWS = 64 / PG_LANES;
constexpr int PG_WAVES = 4;                         // wavefronts of a workgroup
constexpr int PG_MAX_WG = 2048;                     // the grid cap: 256 CUs x 8
constexpr long long PG_MAX_N = 1LL << 30;
constexpr RowGrid PG_GRID{PG_WAVE_ROWS, PG_WAVES, PG_MAX_WG, PG_MAX_N};
constexpr int PG_K = 25;                            // coefficients per axis (PlusShapeModel.n_parameters / 4)
constexpr int PG_ROW = 4 * PG_K;
constexpr int PG_PTS = 128;                         // storage of a dense outline: 54 <= N <= 106 (include/hint_amd.h)
constexpr int PG_DRAWS = 9;
constexpr unsigned PG_TAG = 0x504C5553u;            // counter word 3: "PLUS"
constexpr float PG_U = 2.3283064365386963e-10f;     // 2^-32

// the clockwise ring of an arms mask (bit 0 left, 1 right, 2 top, 3 bottom) as coordinate indices in the order of PL_VX / PL_VY:
// 0 xleft, 1 yleft, 2 yright, 3 xright; 4 xtop, 5 ytop, 6 xbottom, 7 ybottom.  nc = 0: a mask no pair of bars produces
struct PlusGenTables {
    unsigned long long vx[16], vy[16];
    int nc[16];
};

struct PlusGenArgs {
    long long n;
    unsigned long long seed, offset;
    const unsigned long long* rows;
    const float* draws;
    int has_target;
    float t_angle, t_ratio;
    float4* x4;
    float4* y4;
    float2* outline;
    int32_t* counts;
    int32_t* corners;
    float* draws_out;
    int32_t* rejected;
};


// per quadrant, clockwise (upper-left, upper-right, lower-right, lower-left): X the x bar's corner, I the inner corner, Y the y
// bar's corner, F the reflex corner of the notch.  In the upper-left and lower-right quadrants the x bar's arm comes first
static const PlusGenTables& plusgen_tables() {
    static const PlusGenTables T = [] {
        PlusGenTables t;
        const int ax[4] = {0, 3, 3, 0}, bx[4] = {4, 4, 6, 6}, cx[4] = {1, 2, 2, 1}, dy[4] = {5, 5, 7, 7};
        const int xarm[4] = {0, 1, 1, 0}, yarm[4] = {2, 2, 3, 3};
        for (int mask = 0; mask < 16; ++mask) {
            unsigned long long vx = 0, vy = 0;
            int nc = 0;
            auto put = [&](int ix, int iy) {
                vx |= (unsigned long long)ix << (4 * nc);
                vy |= (unsigned long long)iy << (4 * nc);
                ++nc;
            };
            for (int q = 0; q < 4; ++q) {
                const bool xa = (mask >> xarm[q]) & 1, ya = (mask >> yarm[q]) & 1, xfirst = (q & 1) == 0;
                if (xa && ya) {
                    put(xfirst ? ax[q] : cx[q], xfirst ? bx[q] : dy[q]);
                    put(cx[q], bx[q]);
                    put(xfirst ? cx[q] : ax[q], xfirst ? dy[q] : bx[q]);
                } else if (xa) {
                    put(ax[q], bx[q]);
                } else if (ya) {
                    put(cx[q], dy[q]);
                } else {
                    put(xfirst ? cx[q] : ax[q], xfirst ? dy[q] : bx[q]);
                    put(ax[q], dy[q]);
                    put(xfirst ? ax[q] : cx[q], xfirst ? bx[q] : dy[q]);
                }
            }
            const bool opposite = (mask & 3) == 0 || (mask & 12) == 0;     // both arms of a bar missing: lengths exceed widths
            t.vx[mask] = vx;
            t.vy[mask] = vy;
            t.nc[mask] = (nc == 8 || nc == 12) && !opposite ? nc : 0;
        }
        return t;
    }();
    return T;
}

}  // namespace hint

// a row's state in LDS
struct pg_row {
    float2 pts[hint::PG_PTS];                       // the dense outline: local, then placed
    float2 tw[hint::PG_PTS];                        // (cos, sin) of 2 pi r / N
    float2 V[13];                                   // the ring's corners, V[corners] = V[0]
    int cnt[12];                                    // points of edge e
    float2 part[hint::PG_LANES];                    // the lanes' partial sums
};

// sincos in double of the fp32 angle, rounded once, as pl_stage_params; not inlined, for its reason
static __device__ __noinline__ float2 pg_sincos(float angle) {
    double sn, cs;
    sincos((double)angle, &sn, &cs);
    return float2{(float)cs, (float)sn};
}

__device__ __forceinline__ float pg_pick(const float (&c)[8], int i) {
    float v = c[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) v = i == j ? c[j] : v;
    return v;
}

__global__ __launch_bounds__(256) void hint_plusgen_kernel(const hint::PlusGenArgs a, const hint::PlusGenTables T) {
    using namespace hint;
    __shared__ pg_row rws[PG_WAVES * PG_WAVE_ROWS];
    __shared__ float4 stage[PG_WAVES][PG_WAVE_ROWS * PG_ROW / 4];
    __shared__ unsigned long long tvx[16], tvy[16];
    __shared__ int tnc[16];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, g = l / PG_LANES, k = l % PG_LANES;
    if (tid < 16) {
        tvx[tid] = T.vx[tid];
        tvy[tid] = T.vy[tid];
        tnc[tid] = T.nc[tid];
    }
    __syncthreads();
    pg_row& rw = rws[wv * PG_WAVE_ROWS + g];
    float* srow = (float*)&stage[wv][0] + g * PG_ROW;
    const bool want_x = a.x4 != nullptr, want_pts = want_x || a.outline != nullptr;
    const long long tiles = (a.n + PG_WAVE_ROWS - 1) / PG_WAVE_ROWS;
    const long long wave = (long long)blockIdx.x * PG_WAVES + wv, nwaves = (long long)gridDim.x * PG_WAVES;
    const float qnan = __builtin_nanf("");
    int rejected = 0;
    for (long long t = wave; t < tiles; t += nwaves) {
        const long long row = t * PG_WAVE_ROWS + g;
        const bool valid = row < a.n;
        const long long rr = valid ? row : a.n - 1;            // (lanes past the end repeat the last row and store nothing)
        // ---- the nine draws ----
        float dr[PG_DRAWS];
        if (a.draws) {
#pragma unroll
            for (int i = 0; i < PG_DRAWS; ++i) dr[i] = a.draws[rr * PG_DRAWS + i];
        } else {
            const unsigned long long prow = a.rows ? a.rows[rr] : a.offset + (unsigned long long)rr;
            unsigned c[4];
            row_philox(a.seed, prow, 0u, PG_TAG, c);
#pragma unroll
            for (int i = 0; i < 4; ++i) dr[i] = (float)c[i] * PG_U;
            row_philox(a.seed, prow, 1u, PG_TAG, c);
#pragma unroll
            for (int i = 0; i < 3; ++i) dr[4 + i] = (float)c[i] * PG_U;
            row_philox(a.seed, prow, 2u, PG_TAG, c);
            const float2 nm = row_box_muller(c[0], c[1]);
            dr[7] = nm.x;
            dr[8] = nm.y;
        }
        if (a.draws_out && valid && k < PG_DRAWS) {
            float v = dr[0];
#pragma unroll
            for (int i = 1; i < PG_DRAWS; ++i) v = k == i ? dr[i] : v;
            a.draws_out[row * PG_DRAWS + k] = v;
        }
        bool ok = fabsf(dr[7]) < INFINITY && fabsf(dr[8]) < INFINITY;
#pragma unroll
        for (int i = 0; i < 7; ++i) ok = ok && dr[i] >= 0.f && dr[i] <= 1.f;
        // ---- parameters, local coordinates, the arms ----
        const float xlength = fmaf(2.f, dr[0], 3.f), ylength = fmaf(2.f, dr[1], 3.f);
        const float xshift = fmaf(3.f, dr[4], -1.5f), yshift = fmaf(3.f, dr[5], -1.5f);
        float xwidth, ywidth, angle;
        if (a.has_target) {
            const float ratio = a.t_ratio, h = __fmul_rn(0.5f, ratio);
            xwidth = ratio >= 1.f ? fmaf(__fsub_rn(2.f, h), dr[2], h) : fmaf(__fsub_rn(__fmul_rn(2.f, ratio), 0.5f), dr[2], 0.5f);
            ywidth = __fdiv_rn(xwidth, ratio);
            angle = a.t_angle;
        } else {
            xwidth = fmaf(1.5f, dr[2], 0.5f);
            ywidth = fmaf(1.5f, dr[3], 0.5f);
            angle = __fmul_rn(1.57079637f, dr[6]);
        }
        float c[8];
        {
            const float hxl = __fmul_rn(0.5f, xlength), hyl = __fmul_rn(0.5f, ylength);
            const float xtop = __fmul_rn(0.5f, xwidth), yright = __fmul_rn(0.5f, ywidth);
            c[0] = __fsub_rn(xshift, hxl);      // xleft
            c[1] = -yright;                     // yleft
            c[2] = yright;
            c[3] = __fadd_rn(xshift, hxl);      // xright
            c[4] = xtop;
            c[5] = __fadd_rn(yshift, hyl);      // ytop
            c[6] = -xtop;                       // xbottom
            c[7] = __fsub_rn(yshift, hyl);      // ybottom
        }
        // (equality: the arm is absent)
        const int mask = (c[0] < c[1] ? 1 : 0) | (c[3] > c[2] ? 2 : 0) | (c[5] > c[4] ? 4 : 0) | (c[7] < c[6] ? 8 : 0);
        int nc = tnc[mask];
        ok = ok && nc != 0;
        if (!ok) nc = 0;
        if (k < nc) {
            const float2 v = float2{pg_pick(c, (int)((tvx[mask] >> (4 * k)) & 15)), pg_pick(c, (int)((tvy[mask] >> (4 * k)) & 15))};
            rw.V[k] = v;
            if (k == 0) rw.V[nc] = v;
        }
        shapegen_wave_sync();
        // ---- densify_polyline(coords, 0.2): edge e from E = V[e] to S = V[e + 1] ----
        float2 E = float2{0.f, 0.f}, S = E;
        int cnt = 0;
        if (k < nc) {
            E = rw.V[k];
            S = rw.V[k + 1];
            const float len = fmaxf(fabsf(__fsub_rn(S.x, E.x)), fabsf(__fsub_rn(S.y, E.y)));
            const double q = rint((double)len / 0.2);            // round half to even
            cnt = q < 1.0 ? 1 : (q > (double)PG_PTS ? PG_PTS : (int)q);
            rw.cnt[k] = cnt;
        }
        shapegen_wave_sync();
        int pre = 0, N = 0;
        for (int i = 0; i < nc; ++i) {
            const int ci = rw.cnt[i];
            pre += i < k ? ci : 0;
            N += ci;
        }
        // a count the storage or the transform cannot take (no draws in [0, 1] give one: 54 <= N <= 106) is a rejected row
        ok = ok && N >= PG_K && N <= PG_PTS;
        rejected += __popcll(__ballot(valid && !ok && k == 0));
        if (!ok) N = nc = cnt = 0;
        if (k < nc) {
            const float den = (float)(cnt - 1);
            for (int j = 0; j < cnt; ++j) {
                float2 p = E;
                if (cnt > 1) {
                    const float tt = __fdiv_rn((float)j, den), ot = __fsub_rn(1.f, tt);
                    p = float2{fmaf(tt, S.x, __fmul_rn(ot, E.x)), fmaf(tt, S.y, __fmul_rn(ot, E.y))};
                }
                rw.pts[pre + j] = p;                             // pre + j < N <= PG_PTS
            }
        }
        shapegen_wave_sync();
        // ---- pass 1: the mean, a fixed tree ----
        float sx = 0.f, sy = 0.f;
        for (int n = k; n < N; n += PG_LANES) {
            const float2 p = rw.pts[n];
            sx = __fadd_rn(sx, p.x);
            sy = __fadd_rn(sy, p.y);
        }
        rw.part[k] = float2{sx, sy};
        shapegen_wave_sync();
        sx = sy = 0.f;
#pragma unroll
        for (int i = 0; i < PG_LANES; ++i) {
            const float2 p = rw.part[i];
            sx = __fadd_rn(sx, p.x);
            sy = __fadd_rn(sy, p.y);
        }
        const float fN = (float)N;
        const float mx = __fdiv_rn(sx, fN), my = __fdiv_rn(sy, fN), hx = __fmul_rn(0.5f, dr[7]), hy = __fmul_rn(0.5f, dr[8]);
        const float2 rot = pg_sincos(angle);
        // ---- the label ----
        if (valid && k == 0) {
            if (a.y4) {
                const float2 ctr = pl_place(-mx, -my, rot.x, rot.y, hx, hy);
                a.y4[row] = ok ? float4{ctr.x, ctr.y, angle, __fdiv_rn(xwidth, ywidth)} : float4{qnan, qnan, qnan, qnan};
            }
            if (a.counts) a.counts[row] = N;
            if (a.corners) a.corners[row] = ok ? nc + 16 * mask : 0;
        }
        if (!want_pts) {                                         // (uniform: labels only)
            shapegen_wave_sync();
            continue;
        }
        // ---- pass 2: centre, rotate, offset; the twiddles of this N ----
        float2* outl = a.outline && valid ? a.outline + row * PG_PTS : nullptr;
        for (int n = k; n < PG_PTS; n += PG_LANES) {
            float2 q = float2{0.f, 0.f};
            if (n < N) {
                const float2 p = rw.pts[n];
                q = pl_place(__fsub_rn(p.x, mx), __fsub_rn(p.y, my), rot.x, rot.y, hx, hy);
                rw.pts[n] = q;
            }
            if (outl) outl[n] = q;
        }
        if (want_x) {
            for (int r = k; 2 * r <= N && ok; r += PG_LANES) {
                const float2 w = fourier_twiddle(r, N);
                rw.tw[r] = w;
                if (r > 0 && 2 * r < N) rw.tw[N - r] = float2{w.x, -w.y};
            }
            shapegen_wave_sync();
            if (k <= PG_K / 2) {
                DftAcc acc;
                if (ok) {
                    int r = 0;
                    for (int n = 0; n < N; ++n) {
                        const float2 q = rw.pts[n], w = rw.tw[r];
                        dft_term(acc, q.x, q.y, w.x, w.y);
                        r += k;
                        if (r >= N) r -= N;
                    }
                } else {
                    acc.c0 = acc.s0 = acc.c1 = acc.s1 = qnan;
                }
                dft_store(srow, PG_K, k, acc, ok ? fN : 1.f);
            }
            // ---- the wavefront's rows, LDS -> x as contiguous 16-byte pieces ----
            shapegen_wave_sync();
            const long long left = a.n - t * PG_WAVE_ROWS;
            const int pieces = (int)(left < PG_WAVE_ROWS ? left : PG_WAVE_ROWS) * (PG_ROW / 4);
            float4* dst = a.x4 + t * (PG_WAVE_ROWS * PG_ROW / 4);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (l + 64 * i < pieces) dst[l + 64 * i] = stage[wv][l + 64 * i];
        }
        shapegen_wave_sync();
    }
    if (l == 0) a.rejected[wave] = rejected;
}

// ---- the C ABI ----
using namespace hint;

extern "C" {

size_t hint_plusgen_workspace_bytes(int64_t n_rows) {
    if (PG_GRID.check_rows("hint_plusgen_workspace_bytes", n_rows)) return 0;
    return PG_GRID.ws_bytes(n_rows);
}

int hint_plusgen_run(const hint_plusgen_desc* desc) {
    const char* who = "hint_plusgen_run";
    if (!desc) return fail("%s: desc is null", who);
    if (!desc->x && !desc->y) return fail("%s: x and y are both null", who);
    if (workspace_null(who, desc->workspace)) return 1;
    if (PG_GRID.check_rows(who, desc->n_rows)) return 1;
    if (desc->rows && desc->draws) return fail("%s: rows and draws are both given (rows name Philox rows)", who);
    if (!desc->rows && !desc->draws && check_row_offset(who, desc->offset, desc->n_rows)) return 1;
    if (check_groups(who, desc->max_groups)) return 1;
    if (desc->target) {
        const float* t = desc->target;
        for (int i = 0; i < 4; ++i)
            if (!std::isfinite(t[i])) return fail("%s: target[%d] is not finite", who, i);
        if (t[3] < 0.25f || t[3] > 4.f) return fail("%s: target[3], the ratio, must be 0.25..4 (got %g)", who, (double)t[3]);
    }
    if (check_aligned(who, {{"rows", desc->rows, 7}, {"draws", desc->draws, 3}, {"x", desc->x, 15}, {"y", desc->y, 15},
                            {"outline", desc->outline, 7}, {"counts", desc->counts, 3}, {"corners", desc->corners, 3},
                            {"draws_out", desc->draws_out, 3}}))
        return 1;
    const int wgs = PG_GRID.groups(desc->n_rows, desc->max_groups);
    const size_t need = PG_GRID.ws_bytes(desc->n_rows);
    if (workspace_fits(who, "plusgen", desc->workspace, desc->workspace_bytes, need)) return 1;
    PlusGenArgs a;
    a.n = desc->n_rows;
    a.seed = desc->seed;
    a.offset = desc->offset;
    a.rows = (const unsigned long long*)desc->rows;
    a.draws = desc->draws;
    a.has_target = desc->target ? 1 : 0;
    a.t_angle = desc->target ? desc->target[2] : 0.f;
    a.t_ratio = desc->target ? desc->target[3] : 1.f;
    a.x4 = (float4*)desc->x;
    a.y4 = (float4*)desc->y;
    a.outline = (float2*)desc->outline;
    a.counts = desc->counts;
    a.corners = desc->corners;
    a.draws_out = desc->draws_out;
    a.rejected = (int32_t*)desc->workspace;
    hipStream_t s = (hipStream_t)desc->stream;
    if (PG_GRID.clear_tail(wgs, desc, need, s)) return 1;
    hipLaunchKernelGGL(hint_plusgen_kernel, dim3(wgs), dim3(256), 0, s, a, plusgen_tables());
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
