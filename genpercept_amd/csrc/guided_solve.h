// The per-pixel arithmetic of the guided upsampling (gp_guided_upsample; definition in include/genpercept_hip.h), written once for the device
// kernels of guided.hip and for a CPU program (tests/guided_check.cpp): the 16-bit quantisation, the solve of the local linear model from the
// integer window sums, the bilinear index rule, the four-tap blend and the apply.  No HIP header is needed: GS_HD is `__host__ __device__`
// under hipcc and nothing elsewhere.  Everything after the quantisation is float64, the operations are + - * / in the order written, and
// nothing may be contracted into a fused multiply-add (genpercept_amd/guided.py is numpy).
#pragma once

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD inline
#endif

constexpr int GS_MAX_DIM = 16384;  // 1 <= h, w, H, W <= 16384: (2 Y + 1) * h stays below 2^31
constexpr int GS_MAX_R = 32;       // 1 <= r <= 32: every product of the solve, at most 4225^2 * 255 * 65535, stays below 2^53

// the 16-bit rule of gp_postprocess: (uint16)(clamp(x, 0, 1) * 65535.0f), truncated, NaN -> 0
GS_HD unsigned gs_quant16(float x) {
    const float c = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
    return (unsigned)(unsigned short)(c * 65535.0f);
}

// The model q = a . I + b of one window for one prediction channel from its exact sums: n pixels, sI[c] = sum I_c, sII = sums of I_c I_d in the
// order 00 01 02 11 12 22, sp = sum p, sIp[c] = sum I_c p; e = eps * 65025.0.  Every product below that has two integer factors is exact.
GS_HD void gs_solve(unsigned n, const unsigned long long (&sI)[3], const unsigned long long (&sII)[6], unsigned long long sp,
                    const unsigned long long (&sIp)[3], double e, double (&a)[3], double& b) {
    const double N = (double)n, NN = N * N, P = (double)sp;
    const double I0 = (double)sI[0], I1 = (double)sI[1], I2 = (double)sI[2];
    const double cov0 = (N * (double)sIp[0] - I0 * P) / NN;
    const double cov1 = (N * (double)sIp[1] - I1 * P) / NN;
    const double cov2 = (N * (double)sIp[2] - I2 * P) / NN;
    const double s00 = (N * (double)sII[0] - I0 * I0) / NN + e;
    const double s01 = (N * (double)sII[1] - I0 * I1) / NN;
    const double s02 = (N * (double)sII[2] - I0 * I2) / NN;
    const double s11 = (N * (double)sII[3] - I1 * I1) / NN + e;
    const double s12 = (N * (double)sII[4] - I1 * I2) / NN;
    const double s22 = (N * (double)sII[5] - I2 * I2) / NN + e;
    // the cofactors of the symmetric matrix
    const double c00 = s11 * s22 - s12 * s12;
    const double c01 = s02 * s12 - s01 * s22;
    const double c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02;
    const double c12 = s01 * s02 - s00 * s12;
    const double c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    a[0] = ((c00 * cov0 + c01 * cov1) + c02 * cov2) / det;
    a[1] = ((c01 * cov0 + c11 * cov1) + c12 * cov2) / det;
    a[2] = ((c02 * cov0 + c12 * cov1) + c22 * cov2) / det;
    b = P / N - ((a[0] * (I0 / N) + a[1] * (I1 / N)) + a[2] * (I2 / N));
}

// Output index Y of an extent `to` in an extent `from`: s = max(0, ((2 Y + 1) from - to) / (2 to)), i0 = floor(s), i1 = min(i0 + 1, from - 1),
// f = s - i0.  (s < from - 1/2, so i0 <= from - 1.)
GS_HD void gs_index(int Y, int from, int to, int& i0, int& i1, double& f) {
    const double q = (double)((2LL * Y + 1) * from - to) / (double)(2LL * to);
    const double s = q > 0.0 ? q : 0.0;
    i0 = (int)s;  // (s >= 0: truncation is floor)
    i1 = i0 + 1 < from ? i0 + 1 : from - 1;
    f = s - (double)i0;
}

// the four taps (row i0: v00 at j0, v01 at j1; row i1: v10, v11): columns first, then rows; a constant stays that constant
GS_HD double gs_blend(double v00, double v01, double v10, double v11, double fx, double fy) {
    const double t0 = v00 + fx * (v01 - v00);
    const double t1 = v10 + fx * (v11 - v10);
    return t0 + fy * (t1 - t0);
}

// q = (((A0 g0 + A1 g1) + A2 g2) + B) / 65535, clamped to [0, 1] by comparisons (NaN -> 0), rounded once to float32
GS_HD float gs_apply(const double (&A)[3], double B, const unsigned char (&g)[3]) {
    const double v = (((A[0] * (double)g[0] + A[1] * (double)g[1]) + A[2] * (double)g[2]) + B) / 65535.0;
    return (float)(v > 0.0 ? (v < 1.0 ? v : 1.0) : 0.0);
}
