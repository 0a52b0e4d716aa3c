// The plus shape's geometry of a row, shared by the two plus kernels (hint_plus.hip: the fit loss and the Hausdorff distances of
// given parameters; hint_plusfit.hip: the fit itself, which stages a row's geometry anew at every step).  Internal.
// Everything here is part of the contract of include/hint_amd.h (hint_plus_desc items 1 - 4): the local vertices, the keep bit,
// the placement and the segment constants are the same operations in both kernels, so a fit step's vertices, keep bits and
// segment constants are the bits hint_plus_kernel computes for the same parameters.
#pragma once
#include "hint_pointset.hpp"

namespace hint {

// which of the 8 coordinates (0 xleft, 1 yleft, 2 yright, 3 xright; 4 xtop, 5 ytop, 6 xbottom, 7 ybottom) vertex s takes, 4 bits
// a vertex
constexpr unsigned long long PL_VX = 0x011223322110ULL;   // s = 0 is the lowest nibble: 0 1 1 2 2 3 3 2 2 1 1 0
constexpr unsigned long long PL_VY = 0x667766445544ULL;   // 4 4 5 5 4 4 6 6 7 7 6 6

}  // namespace hint

// a row's state in LDS
struct pl_row {
    float c[8];                                  // the clamped coordinates, in the order of PL_VX / PL_VY
    float cs, sn, xo, yo;
    int finite;                                  // all 9 parameters are
    float2 W[13];                                // placed vertices, W[12] = W[0]
    float2 a[12], n[12];                         // per segment: first vertex, unit direction
    float L[12];
    int pre[16];                                 // exclusive prefix sums of the counts; pre[12] = M, pre[13..15] = INT_MAX
    int keep, nk, M, bad;
};

// the row's 8 coordinates, cs, sn and the offsets to LDS, by one thread.  Not inlined, as ps_stage_pose and for the same
// reason: the double-precision sincos holds some thirty registers of constants
inline __device__ __noinline__ void pl_stage_params(const float* pr, pl_row* rw) {
    const float xlength = pr[0], ylength = pr[1], xwidth = pr[2], ywidth = pr[3], xshift = pr[4], yshift = pr[5];
    const float hxl = __fmul_rn(0.5f, xlength), hyl = __fmul_rn(0.5f, ylength);
    const float xtop = __fmul_rn(0.5f, xwidth), xbottom = -xtop, yright = __fmul_rn(0.5f, ywidth), yleft = -yright;
    float xleft = __fsub_rn(xshift, hxl), xright = __fadd_rn(xshift, hxl);
    float ybottom = __fsub_rn(yshift, hyl), ytop = __fadd_rn(yshift, hyl);
    const float c = 0.01f;
    xleft = fminf(xleft, __fsub_rn(yleft, c));
    xright = fmaxf(xright, __fadd_rn(yright, c));
    ytop = fmaxf(ytop, __fadd_rn(xtop, c));
    ybottom = fminf(ybottom, __fsub_rn(xbottom, c));
    rw->c[0] = xleft;
    rw->c[1] = yleft;
    rw->c[2] = yright;
    rw->c[3] = xright;
    rw->c[4] = xtop;
    rw->c[5] = ytop;
    rw->c[6] = xbottom;
    rw->c[7] = ybottom;
    double sn, cs;
    sincos((double)pr[8], &sn, &cs);
    rw->cs = (float)cs;
    rw->sn = (float)sn;
    rw->xo = pr[6];
    rw->yo = pr[7];
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(pr[i]);
    rw->finite = fin ? 1 : 0;
}

__device__ __forceinline__ float2 pl_place(float vx, float vy, float cs, float sn, float xo, float yo) {
    const float qx = __fmaf_rn(-vy, sn, __fmul_rn(vx, cs)), qy = __fmaf_rn(vy, cs, __fmul_rn(vx, sn));
    return make_float2(__fadd_rn(qx, xo), __fadd_rn(qy, yo));
}

// segment s of the staged row: its two placed vertices, and whether its two local vertices differ (the keep bit of a lane that
// holds a segment).  (The row by reference, as ps_rotate's point and for the same reason.)
__device__ __forceinline__ void pl_segment(const pl_row& rw, int s, float2& w0, float2& w1, bool& differ) {
    using namespace hint;
    const int s1 = s == 11 ? 0 : s + 1;
    const float cs = rw.cs, sn = rw.sn, xo = rw.xo, yo = rw.yo;
    const float v0x = rw.c[(PL_VX >> (4 * s)) & 15], v0y = rw.c[(PL_VY >> (4 * s)) & 15];
    const float v1x = rw.c[(PL_VX >> (4 * s1)) & 15], v1y = rw.c[(PL_VY >> (4 * s1)) & 15];
    differ = v0x != v1x || v0y != v1y;
    w0 = pl_place(v0x, v0y, cs, sn, xo, yo);
    w1 = pl_place(v1x, v1y, cs, sn, xo, yo);
}

// lane l < 12: the placed vertices and the loss's constants (a, n, L) of its segment to LDS
__device__ __forceinline__ void pl_store_segment(pl_row& rw, int l, const float2& w0, const float2& w1) {
    const float nx = __fsub_rn(w1.x, w0.x), ny = __fsub_rn(w1.y, w0.y);
    const float L = __fsqrt_rn(__fmaf_rn(ny, ny, __fmul_rn(nx, nx)));
    rw.W[l] = w0;
    if (l == 11) rw.W[12] = w1;
    rw.a[l] = w0;
    rw.n[l] = make_float2(__fdiv_rn(nx, L), __fdiv_rn(ny, L));
    rw.L[l] = L;
}
