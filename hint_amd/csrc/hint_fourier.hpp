// Points -> Fourier coefficients, the one definition the shape generators and hint_fcoef_run share (data.py:42-49 fourier_coeffs and
// data.py:30-33 flatten_coeffs of the reference):
//   a[c, m] = (1 / N) sum_n p[n, c] exp(-2 pi i m n / N),  m = -K/2 .. K/2,  N = the number of points
//   row = [Re a[0, :], Re a[1, :], Im a[0, :], Im a[1, :]], 4 K floats: the layout every kernel of hint_curve.hip reads
// One DftAcc holds frequency |m| of both axes: C = sum p cos(phi), S = sum p sin(phi), phi = 2 pi ((|m| n) mod N) / N, each an fp32
// fused multiply-add onto the sum, n ascending from 0.  Re a[+-m] = C / N, Im a[m] = -S / N, Im a[-m] = S / N (correctly rounded
// divisions by (float)N).  A twiddle is the true value rounded to fp32 once, its angle reduced in integers first.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hint {

constexpr int FOURIER_MAX_K = 25;

struct DftAcc { float c0 = 0.f, s0 = 0.f, c1 = 0.f, s1 = 0.f; };

__device__ __forceinline__ void dft_term(DftAcc& a, float px, float py, float cs, float sn) {
    a.c0 = fmaf(px, cs, a.c0);
    a.s0 = fmaf(px, sn, a.s0);
    a.c1 = fmaf(py, cs, a.c1);
    a.s1 = fmaf(py, sn, a.s1);
}

// frequency m >= 0 and its mirror into a row of 4 K floats
template <typename RowPtr>
__device__ __forceinline__ void dft_store(RowPtr row, int K, int m, const DftAcc& a, float fN) {
    const int h = K / 2;
    const float re0 = a.c0 / fN, re1 = a.c1 / fN, im0 = a.s0 / fN, im1 = a.s1 / fN;
    row[h + m] = re0;
    row[K + h + m] = re1;
    row[2 * K + h + m] = 0.f - im0;
    row[3 * K + h + m] = 0.f - im1;
    if (m) {
        row[h - m] = re0;
        row[K + h - m] = re1;
        row[2 * K + h - m] = im0;
        row[3 * K + h - m] = im1;
    }
}

// (cos, sin) of 2 pi r / count, 0 <= r < count, in double, rounded to fp32
__host__ __device__ inline float2 fourier_twiddle(int r, int count) {
    double s, c;
#ifdef __HIP_DEVICE_COMPILE__
    sincospi(2.0 * (double)r / (double)count, &s, &c);
#else
    const double a = 2.0 * 3.14159265358979323846 * (double)r / (double)count;
    s = std::sin(a);
    c = std::cos(a);
#endif
    return float2{(float)c, (float)s};
}

}  // namespace hint
