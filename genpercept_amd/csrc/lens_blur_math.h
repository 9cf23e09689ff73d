// The arithmetic of the synthetic depth of field (gp_lens_blur; definition in include/genpercept_hip.h), written once for the device kernel of
// lens_blur.hip and for a CPU program (tests/lens_blur_check.cpp): the nearness and the circle of confusion of a pixel, the disc sizes and
// weights, the reach of a source towards an output pixel, the 64-bit word a pixel is staged as, and the output byte.  No HIP header is needed.
// The quantisation is gs_quant16 of guided_solve.h.  Everything after it is integer arithmetic, so a sum does not depend on its order.
//
// Definition, per image.  image uint8 [3][H][W]; pred float32 [1][H][W]; sharp uint8 [H][W] or none; the row F, gain, cmax8, dz of the
// parameter table; to_lin uint16 [256]; from_lin uint8 [4096].
//   1. Q = gs_quant16(pred); D = Q (disparity) or 65535 - Q (depth): larger is nearer.  D = 0 for a NaN pixel.
//   2. e = max(0, |D - F| - dz); c = min(cmax8, (e * gain + 32768) >> 16), in eighths of a pixel; c = 0 where pred is NaN or sharp != 0.
//   3. n(c) = the number of integer offsets with 64 (dx^2 + dy^2) <= (c + 4)^2; w(c) = floor(2^20 / n(c)).
//   4. For the output pixel p, a source q inside the image at offset (dx, dy) has the reach r = c_q if D_q >= D_p, min(c_q, c_p) otherwise; it
//      contributes iff 64 (dx^2 + dy^2) <= (r + 4)^2, with the weight w(r): Sw = sum w, S_k = sum w * to_lin[image_k(q)].
//   5. out_k(p) = from_lin[(2 S_k + Sw) / (2 Sw)]; coc(p) = c_p.
#pragma once

#include "guided_solve.h"

#define LB_HD GS_HD

typedef unsigned long long lb_u64;

constexpr int LB_MAX_DIM = 16384;    // 1 <= H, W <= 16384
constexpr int LB_MAX_C8 = 256;       // 0 <= cmax8 <= 256: a blur radius of at most 32 pixels
constexpr int LB_MAX_R = 32;         // the largest offset that can contribute: (256 + 4) / 8
constexpr int LB_MAX_GAIN = 32768;   // 0 <= gain <= 32768: e * gain + 32768 stays below 2^31
constexpr int LB_PARAMS = 4;         // F, gain, cmax8, dz
constexpr unsigned LB_ONE = 1u << 20;
constexpr unsigned LB_LIN_MAX = 4095;
enum { LB_SPACE_DEPTH = 0, LB_SPACE_DISPARITY = 1 };

struct LbParams {
    int F, gain, cmax8, dz;
};

LB_HD int lb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A row of the parameter table with every value brought into its range; cmax8 also below the call's largest, max_c8.
LB_HD LbParams lb_params(const int* row, int max_c8) {
    return {lb_clamp(row[0], 0, 65535), lb_clamp(row[1], 0, LB_MAX_GAIN), lb_clamp(row[2], 0, max_c8), lb_clamp(row[3], 0, 65535)};
}

// Step 1
LB_HD int lb_nearness(float pred, int space) {
    if (!(pred == pred)) return 0;
    const int q = (int)gs_quant16(pred);
    return space == LB_SPACE_DISPARITY ? q : 65535 - q;
}

// Step 2.  still: pred is NaN or the pixel is pinned sharp.
LB_HD int lb_coc(int D, bool still, const LbParams& a) {
    if (still) return 0;
    const int d = D > a.F ? D - a.F : a.F - D;
    const int e = d > a.dz ? d - a.dz : 0;
    const int c = (int)(((unsigned)e * (unsigned)a.gain + 32768u) >> 16);  // (at most 65535 * 32768 + 32768 < 2^31)
    return c < a.cmax8 ? c : a.cmax8;
}

// the largest offset along an axis that reach c can span: floor((c + 4) / 8)
LB_HD int lb_reach_pixels(int c) { return (c + 4) >> 3; }

// Step 3: the offsets (dx, dy) with 64 (dx^2 + dy^2) <= (c + 4)^2, counted row by row; the widest dx falls as |dy| grows.
LB_HD unsigned lb_disc_count(int c) {
    const int k = ((c + 4) * (c + 4)) >> 6;  // dx^2 + dy^2 <= k
    int dx = 0;
    while ((dx + 1) * (dx + 1) <= k) ++dx;
    unsigned n = 0;
    for (int dy = 0; dy * dy <= k; ++dy) {
        while (dx * dx + dy * dy > k) --dx;
        n += (dy == 0 ? 1u : 2u) * (unsigned)(2 * dx + 1);
    }
    return n;
}

LB_HD unsigned lb_disc_weight(int c) { return LB_ONE / lb_disc_count(c); }

// Step 4: the reach of source q towards output pixel p
LB_HD int lb_reach(int Dq, int cq, int Dp, int cp) { return Dq >= Dp ? cq : (cq < cp ? cq : cp); }

// whether the offset with d2 = dx^2 + dy^2 lies inside reach r
LB_HD bool lb_inside(int d2, int r) { return 64 * d2 <= (r + 4) * (r + 4); }

// A pixel as one 64-bit word: D in bits 0 .. 15, c in 16 .. 24, the three linear colours in 28 .. 39, 40 .. 51, 52 .. 63.  A pixel outside the
// image is the word 0: with c = 0 its reach is 0 from every side and it contributes to no other pixel.
LB_HD lb_u64 lb_pack(int D, int c, unsigned l0, unsigned l1, unsigned l2) {
    return (lb_u64)(unsigned)D | (lb_u64)(unsigned)c << 16 | (lb_u64)(l0 & LB_LIN_MAX) << 28 | (lb_u64)(l1 & LB_LIN_MAX) << 40 |
           (lb_u64)(l2 & LB_LIN_MAX) << 52;
}
LB_HD int lb_word_D(lb_u64 w) { return (int)((unsigned)w & 0xffffu); }
LB_HD int lb_word_c(lb_u64 w) { return (int)(((unsigned)w >> 16) & 0x1ffu); }
LB_HD unsigned lb_word_lin(lb_u64 w, int k) { return (unsigned)(w >> (28 + 12 * k)) & LB_LIN_MAX; }

// The sums of one output pixel
struct LbSums {
    lb_u64 sw, s[3];
};

LB_HD void lb_sums_clear(LbSums& a) { a.sw = a.s[0] = a.s[1] = a.s[2] = 0; }

// one contributing source with the weight wt = w(r)
LB_HD void lb_sums_add(LbSums& a, unsigned wt, lb_u64 word) {
    a.sw += wt;
    a.s[0] += (lb_u64)wt * lb_word_lin(word, 0);
    a.s[1] += (lb_u64)wt * lb_word_lin(word, 1);
    a.s[2] += (lb_u64)wt * lb_word_lin(word, 2);
}

// Step 5: the index into from_lin, floor((2 s + sw) / (2 sw)), at most 4095 since every to_lin value is.  A 64-bit division costs the device
// some two hundred instructions; the quotient is small, so a float estimate of it -- three roundings of 2^-24 on a value below 4096, far
// less than 1 off -- is set right by the integer remainder.  The result is the exact quotient whatever the float division rounds to.
LB_HD unsigned lb_resolve(lb_u64 s, lb_u64 sw) {
    const lb_u64 num = 2 * s + sw, den = 2 * sw;
    unsigned q = (unsigned)((float)num / (float)den);
    if ((lb_u64)q * den > num)
        --q;
    else if ((lb_u64)(q + 1) * den <= num)
        ++q;
    return q;
}

// the ranges of the call
LB_HD bool lb_dims_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= LB_MAX_DIM && W <= LB_MAX_DIM && (long long)B * H * W <= 0x7fffffffLL;
}
LB_HD bool lb_options_ok(int space, int max_c8) {
    return (space == LB_SPACE_DEPTH || space == LB_SPACE_DISPARITY) && max_c8 >= 0 && max_c8 <= LB_MAX_C8;
}
