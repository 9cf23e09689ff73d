// The per-pixel arithmetic of the multi-level foreground estimation (gp_foreground; definition in include/genpercept_hip.h), written once for
// the device kernels of foreground.hip and for a CPU program (tests/foreground_check.cpp runs the whole multi-level loop over this text).
// No HIP header is needed: FG_HD is `__host__ __device__` under hipcc and nothing elsewhere.  Everything is float32, the operations are
// + - * / abs min max in the order written, and nothing may be contracted into a fused multiply-add (genpercept_amd/foreground.py is numpy).
#pragma once

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD inline
#endif

constexpr int FG_MAX_DIM = 16384;  // 1 <= H, W <= 16384: (y * H) of an index map stays below 2^31
constexpr int FG_SMALL = 32;       // a level of at most 32 x 32 takes n_small iterations, every other level n_big

// L = ceil(log2(max(H, W))), 0 for a 1 x 1 image
FG_HD int fg_num_levels(int H, int W) {
    const int m = H > W ? H : W;
    int L = 0;
    while ((1 << L) < m) ++L;
    return L;
}

// the extent of level l = 0 .. L of an extent n of the image: 1 at level 0, n at level L
FG_HD int fg_level_size(int n, int L, int l) { return (n + (1 << (L - l)) - 1) >> (L - l); }

// nearest: the index in an extent `from` that index i of an extent `to` samples
FG_HD int fg_src(int i, int from, int to) { return (i * from) / to; }

FG_HD float fg_unit(unsigned byte) { return (float)byte / 255.0f; }

// max(v, 0) and min(v, 1) as comparisons, so that -0 and +0 cannot differ between the routes: min(max(v, 0), 1)
FG_HD float fg_clamp01(float v) {
    v = v > 0.0f ? v : 0.0f;
    return v < 1.0f ? v : 1.0f;
}

// One Jacobi update of a pixel: alpha a and colour I of the pixel, alpha an and the previous iterates Fn, Bn of its four neighbours in the
// order left, right, up, down (coordinates clamped to the level, so a neighbour may be the pixel itself).  Returns det.
FG_HD float fg_update(float a, const float (&I)[3], const float (&an)[4], const float (&Fn)[4][3], const float (&Bn)[4][3], float reg, float gw,
                      float (&F)[3], float (&B)[3]) {
    const float a1 = 1.0f - a;
    float a00 = a * a;
    const float a01 = a * a1;
    float a11 = a1 * a1;
    float b0[3], b1[3];
    for (int c = 0; c < 3; ++c) {
        b0[c] = a * I[c];
        b1[c] = a1 * I[c];
    }
    for (int n = 0; n < 4; ++n) {
        const float d = a - an[n];
        const float da = reg + gw * (d < 0.0f ? -d : d);
        a00 = a00 + da;
        a11 = a11 + da;
        for (int c = 0; c < 3; ++c) {
            b0[c] = b0[c] + da * Fn[n][c];
            b1[c] = b1[c] + da * Bn[n][c];
        }
    }
    const float det = a00 * a11 - a01 * a01;
    const float inv = 1.0f / det;
    for (int c = 0; c < 3; ++c) {
        F[c] = fg_clamp01(inv * (a11 * b0[c] - a01 * b1[c]));
        B[c] = fg_clamp01(inv * (a00 * b1[c] - a01 * b0[c]));
    }
    return det;
}

// a value in [0, 1] as a byte: min(255, (int)(v * 255 + 0.5))
FG_HD unsigned char fg_byte(float v) {
    const int q = (int)(v * 255.0f + 0.5f);
    return (unsigned char)(q < 255 ? q : 255);
}

// the foreground over a new background N: (a F) + ((1 - a) N)
FG_HD float fg_composite(float a, float F, float N) { return (a * F) + ((1.0f - a) * N); }
