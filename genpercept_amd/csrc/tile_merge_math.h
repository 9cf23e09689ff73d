// The arithmetic of the tile merge (gp_tile_merge; definition in include/genpercept_hip.h), written once for the device kernels of
// tile_merge.hip and for a CPU program (tests/tile_check.cpp): the grid rule, the per-tile solve from the exact integer sums, and the
// per-pixel weight, accumulate and finish steps.  No HIP header is needed.  The quantisation is gs_quant16 of guided_solve.h.  Everything
// after the integer sums is float64, the operations are + - * / in the order written, and nothing may be contracted into a fused multiply-add
// (genpercept_amd/tiled.py is numpy).
#pragma once

#include "guided_solve.h"

#pragma clang fp contract(off)

#define TM_HD GS_HD

constexpr int TM_MAX_DIM = 16384;   // 1 <= H, W <= 16384: the five sums stay below 2^63 (3 * 2^28 values of at most 65535^2 < 2^32)
constexpr int TM_MAX_TILES = 1024;  // ny * nx <= 1024: the origin tables and the (s, t) table fit the LDS of a workgroup
enum { TM_ALIGN_LEAST_SQUARE = 0, TM_ALIGN_NONE = 1 };

// an axis of length L, window w = min(T, L), overlap o: 1 <= o <= w / 2
TM_HD bool tm_axis_ok(int L, int w, int o) { return L >= 1 && L <= TM_MAX_DIM && w >= 1 && w <= L && o >= 1 && 2 * o <= w; }

// the tile count of an axis: 1 if L <= w, else ceil((L - o) / (w - o))
TM_HD int tm_count(int L, int w, int o) { return L <= w ? 1 : (L - o + (w - o) - 1) / (w - o); }

// origin k of n: (k * (L - w)) // (n - 1), 0 for n = 1 (k * (L - w) < 2^24)
TM_HD int tm_origin(int k, int L, int w, int n) { return n > 1 ? (k * (L - w)) / (n - 1) : 0; }

// The fit of one tile from its exact sums: n values, sP = sum P, sG = sum G, sPP = sum P^2, sPG = sum P G.  Each sum is converted to float64
// once (round to nearest).
TM_HD void tm_solve(unsigned long long n, unsigned long long sP, unsigned long long sG, unsigned long long sPP, unsigned long long sPG, double& s,
                    double& t) {
    const double N = (double)n;
    const double mp = (double)sP / N;
    const double mg = (double)sG / N;
    const double var = (double)sPP / N - mp * mp;
    const double cov = (double)sPG / N - mp * mg;
    s = cov / var;
    if (!(var >= 1.0) || !(s > 0.0)) s = 1.0;  // flat to within one 16-bit step, or anti-correlated with the base: shifted only (NaN too)
    t = (mg - s * mp) / 65535.0;
}

// the weight of index y along an axis inside the window [y0, y0 + w): min(y - y0 + 1, y0 + w - y, o) >= 1
TM_HD int tm_weight(int y, int y0, int w, int o) {
    const int a = y - y0 + 1, b = y0 + w - y;
    const int m = a < b ? a : b;
    return m < o ? m : o;
}

// acc += wgt * (s * p + t): product, sum, product, sum
TM_HD double tm_accumulate(double acc, int wgt, double s, double t, float p) { return acc + (double)wgt * (s * (double)p + t); }

// q = acc / (sum of weights), clamped to [0, 1] by comparisons (NaN -> 0), rounded once to float32
TM_HD float tm_finish(double acc, long long wsum) {
    const double q = acc / (double)wsum;
    return (float)(q > 0.0 ? (q < 1.0 ? q : 1.0) : 0.0);
}
