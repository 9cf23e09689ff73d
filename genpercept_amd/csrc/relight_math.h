// The arithmetic of the relighting (gp_relight; definition in include/genpercept_hip.h), written once for the device kernel of relight.hip
// and for a CPU program (tests/relight_check.cpp): the integer normal of a pixel and its exact length, the diffuse and specular terms of a
// light, the shadow march over the nearness map, the combination in linear light and the blend with the image, and the checks of the light
// table.  No HIP header is needed.  The quantisation is gs_quant16 of guided_solve.h.  Everything after it is integer arithmetic, so a sum
// or a maximum does not depend on its order.
//
// Definition, per image.  image uint8 [3][H][W]; normal float32 [3][H][W]; pred float32 [H][W] or none; weight uint8 [H][W] or none; the
// table of L light rows and one ambient row; to_lin uint16 [256]; from_lin uint8 [4096].
//   1. N_k = 2 gs_quant16(v_k) - 65535 (encoded) or (int)(clamp(v_k, -1, 1) * 65535.0f) (raw), negated where the flip bit k is set;
//      m = floor(sqrt(N.N)); a NaN channel or m < 256: N = (0, 0, -65535), m = 65535.
//   2. cos12 = clamp(floor(N.L / (4 m)), 0, 4096); s = clamp(floor(N.H / (4 m)), 0, 4096), then k times s = (s s + 2048) >> 12; a light
//      with cos12 = 0 contributes nothing and its march is not walked.
//   3. D = the nearness (gs_quant16(pred), mirrored in depth space; 0 and no shadow at all for a NaN pixel).  For t = 1 .. reach,
//      q_t = (x + ((t ux + 128) >> 8), y + ((t uy + 128) >> 8)), inside the image: e_t = D(q_t) - D(p) - bias - t rise; E = max(0, max e_t);
//      dark = soft ? min(256, (E soft + 128) >> 8) : (E > 0 ? 256 : 0); shade = (dark strength) >> 8; vis = 256 - shade.
//   4. G_k = amb_k + ((sum_j col_jk cos12_j vis_j) >> 16); S_k = (sum_j spc_jk s_j vis_j) >> 16;
//      lin'_k = min(4095, ((to_lin[image_k] G_k + 2048) >> 12) + min(S_k, 4095)); relit_k = from_lin[lin'_k];
//      out_k = (w relit_k + (255 - w) image_k + 127) / 255; shadow = min(255, max_j shade_j).
#pragma once

#include "guided_solve.h"

#pragma clang fp contract(off)

#define RL_HD GS_HD

typedef unsigned long long rl_u64;

constexpr int RL_MAX_DIM = 16384;    // 1 <= H, W <= 16384
constexpr int RL_MAX_LIGHTS = 8;     // 1 <= L <= 8: the table travels as a kernel argument
constexpr int RL_MAX_REACH = 64;     // a shadow is at most 64 steps long: the tile and its apron are 160 x 144 16-bit words of LDS
constexpr int RL_ROW = 20;           // the integers of a table row
constexpr int RL_UNIT = 16384;       // a unit vector's length in the table
constexpr int RL_MAX_GAIN = 4096;    // col, spc: Q8, at most 16.0
constexpr int RL_MAX_AMB = 65536;    // amb: Q12, at most 16.0
constexpr int RL_MIN_LEN = 256;      // a normal shorter than this (of 65535) is no normal
constexpr int RL_N_ONE = 65535;
constexpr unsigned RL_LIN_MAX = 4095;
enum { RL_SPACE_DEPTH = 0, RL_SPACE_DISPARITY = 1 };
// a light row: L (3), H (3), col (3), spc (3), k, ux, uy, rise, bias, soft, strength, reach; the ambient row: amb (3), the rest unread
enum { RL_LX = 0, RL_HX = 3, RL_COL = 6, RL_SPC = 9, RL_K = 12, RL_UX = 13, RL_UY = 14, RL_RISE = 15, RL_BIAS = 16, RL_SOFT = 17, RL_STRENGTH = 18,
       RL_REACH = 19 };

// The light table as the kernel takes it: L light rows, then the ambient row.
struct RlTable {
    int v[RL_MAX_LIGHTS + 1][RL_ROW];
};

RL_HD int rl_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor(sqrt(s)) for s < 2^53: the float64 root is an estimate that the integer comparison sets right, so the result is exact whatever the
// root rounds to.
RL_HD unsigned rl_isqrt(rl_u64 s) {
    rl_u64 r = (rl_u64)__builtin_sqrt((double)s);
    while (r * r > s) --r;
    while ((r + 1) * (r + 1) <= s) ++r;
    return (unsigned)r;
}

// clamp(floor(num / den), 0, 4096) for den > 0.  Below the clamp the quotient is small, so a float estimate of it -- three roundings of
// 2^-24 on a value below 4096, far less than 1 off -- is set right by the integer remainder, as lb_resolve of lens_blur_math.h does.
RL_HD int rl_ratio12(long long num, long long den) {
    if (num <= 0) return 0;
    if (num >= 4096 * den) return 4096;
    long long q = (long long)((float)num / (float)den);
    if (q * den > num)
        --q;
    else if ((q + 1) * den <= num)
        ++q;
    return (int)q;
}

// Step 1.  The integer normal of one pixel; m is its length.
struct RlNormal {
    int n[3], m;
};

RL_HD int rl_component(float v, int encoded) {
    if (encoded) return 2 * (int)gs_quant16(v) - RL_N_ONE;
    const float c = v > -1.0f ? (v < 1.0f ? v : 1.0f) : -1.0f;
    return (int)(c * 65535.0f);
}

RL_HD RlNormal rl_normal(float vx, float vy, float vz, int encoded, int flip) {
    RlNormal a;
    a.n[0] = rl_component(vx, encoded);
    a.n[1] = rl_component(vy, encoded);
    a.n[2] = rl_component(vz, encoded);
    if (flip & 1) a.n[0] = -a.n[0];
    if (flip & 2) a.n[1] = -a.n[1];
    if (flip & 4) a.n[2] = -a.n[2];
    a.m = (int)rl_isqrt((rl_u64)((long long)a.n[0] * a.n[0]) + (rl_u64)((long long)a.n[1] * a.n[1]) + (rl_u64)((long long)a.n[2] * a.n[2]));
    if (!(vx == vx) || !(vy == vy) || !(vz == vz) || a.m < RL_MIN_LEN) {
        a.n[0] = a.n[1] = 0;
        a.n[2] = -RL_N_ONE;
        a.m = RL_N_ONE;
    }
    return a;
}

// Step 2.  v: the three integers of L or H in a row.
RL_HD int rl_cos12(const RlNormal& a, const int* v) {
    const long long d = (long long)a.n[0] * v[0] + (long long)a.n[1] * v[1] + (long long)a.n[2] * v[2];
    return rl_ratio12(d, 4LL * a.m);
}

RL_HD int rl_specular(const RlNormal& a, const int* row) {
    int s = rl_cos12(a, row + RL_HX);
    for (int i = 0; i < row[RL_K]; ++i) s = (s * s + 2048) >> 12;
    return s;
}

// Step 3
RL_HD int rl_nearness(float pred, int space) {
    if (!(pred == pred)) return 0;
    const int q = (int)gs_quant16(pred);
    return space == RL_SPACE_DISPARITY ? q : 65535 - q;
}

// the offset of step t along one axis, in pixels (a floor)
RL_HD int rl_step(int t, int u) { return (t * u + 128) >> 8; }

// what is taken from every D(q_t): e_t = D(q_t) - rl_floor(Dp, row, t).  It grows with t.
RL_HD int rl_floor(int Dp, const int* row, int t) { return Dp + row[RL_BIAS] + t * row[RL_RISE]; }

// (dark * strength) >> 8 of the excess E >= 0
RL_HD int rl_shade(int E, const int* row) {
    const int soft = row[RL_SOFT];
    int dark = soft ? (E * soft + 128) >> 8 : (E > 0 ? 256 : 0);  // (at most 65535 * 256 + 128)
    dark = dark < 256 ? dark : 256;
    return (dark * row[RL_STRENGTH]) >> 8;
}

// Step 4.  The sums of one pixel over its lights.
struct RlSums {
    rl_u64 g[3], s[3];
    int shade;
};

RL_HD void rl_sums_clear(RlSums& a) {
    a.g[0] = a.g[1] = a.g[2] = a.s[0] = a.s[1] = a.s[2] = 0;
    a.shade = 0;
}

// one light with cos12 > 0, its specular term s and its shade
RL_HD void rl_sums_add(RlSums& a, const int* row, int cos12, int s, int shade) {
    const rl_u64 cv = (rl_u64)(unsigned)(cos12 * (256 - shade)), sv = (rl_u64)(unsigned)(s * (256 - shade));  // (at most 2^20)
    for (int k = 0; k < 3; ++k) {
        a.g[k] += cv * (unsigned)row[RL_COL + k];
        a.s[k] += sv * (unsigned)row[RL_SPC + k];
    }
    a.shade = shade > a.shade ? shade : a.shade;
}

// the index into from_lin of channel k: lin = to_lin[image_k], amb = the ambient row
RL_HD unsigned rl_lin(const RlSums& a, const int* amb, int k, unsigned lin) {
    const unsigned G = (unsigned)amb[k] + (unsigned)(a.g[k] >> 16);  // (at most 65536 + 8 * 65536: lin * G stays below 2^32)
    const unsigned S = (unsigned)(a.s[k] >> 16);
    const unsigned v = (((lin & RL_LIN_MAX) * G + 2048u) >> 12) + (S < RL_LIN_MAX ? S : RL_LIN_MAX);
    return v < RL_LIN_MAX ? v : RL_LIN_MAX;
}

RL_HD unsigned char rl_blend(unsigned relit, unsigned image, unsigned w) { return (unsigned char)((w * relit + (255u - w) * image + 127u) / 255u); }

RL_HD unsigned char rl_shadow_byte(int shade) { return (unsigned char)(shade < 255 ? shade : 255); }

// the ranges of the call
RL_HD bool rl_dims_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= RL_MAX_DIM && W <= RL_MAX_DIM && (long long)B * H * W <= 0x7fffffffLL;
}
RL_HD bool rl_options_ok(int L, int encoded, int flip, int space, int max_reach) {
    return L >= 1 && L <= RL_MAX_LIGHTS && (encoded == 0 || encoded == 1) && flip >= 0 && flip <= 7 &&
           (space == RL_SPACE_DEPTH || space == RL_SPACE_DISPARITY) && max_reach >= 0 && max_reach <= RL_MAX_REACH;
}
RL_HD bool rl_in(int v, int lo, int hi) { return v >= lo && v <= hi; }
RL_HD bool rl_row_ok(const int* r, int max_reach) {
    for (int k = 0; k < 6; ++k)
        if (!rl_in(r[k], -RL_UNIT, RL_UNIT)) return false;
    for (int k = RL_COL; k < RL_K; ++k)
        if (!rl_in(r[k], 0, RL_MAX_GAIN)) return false;
    const int ax = r[RL_UX] < 0 ? -r[RL_UX] : r[RL_UX], ay = r[RL_UY] < 0 ? -r[RL_UY] : r[RL_UY];
    return rl_in(r[RL_K], 0, 7) && ax <= 256 && ay <= 256 && rl_in(r[RL_RISE], 0, 65535) && rl_in(r[RL_BIAS], 0, 65535) && rl_in(r[RL_SOFT], 0, 256) &&
           rl_in(r[RL_STRENGTH], 0, 256) && rl_in(r[RL_REACH], 0, max_reach) && (r[RL_REACH] == 0 || (ax > ay ? ax : ay) == 256);
}
// the table of L light rows and the ambient row (the options are in range)
RL_HD bool rl_table_ok(const int* lights, int L, int max_reach) {
    for (int j = 0; j < L; ++j)
        if (!rl_row_ok(lights + j * RL_ROW, max_reach)) return false;
    for (int k = 0; k < 3; ++k)
        if (!rl_in(lights[L * RL_ROW + k], 0, RL_MAX_AMB)) return false;
    return true;
}
