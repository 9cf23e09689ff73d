// The arithmetic of the stereo and parallax views (gp_stereo_views; definition in include/genpercept_hip.h), written once for the device
// kernels of stereo.hip and for a CPU program (tests/stereo_check.cpp): the nearness of a pixel, the shift of a source column for a view, the
// three pieces a source can cover an output column with, the comparison that picks the visible one, and the choice between the two
// neighbours of a hole.  No HIP header is needed.  The quantisation is gs_quant16 of guided_solve.h.  Everything after it is integer
// arithmetic, so the result does not depend on the order the pieces are looked at.
//
// Definition, per image, row and view (g, ox, oy, cmask).  D, c: the nearness and the three colour bytes of a source column.
//   1. Q = gs_quant16(pred); D = Q (disparity) or 65535 - Q (depth): larger is nearer.  D = 0 for a NaN pixel.
//   2. s = ((int64)(D - F) * g + 2^23) >> 24 (a floor), clamped to -max_s8 .. max_s8; t_x = 8 x + s, in eighths of a pixel.
//   3. x and x + 1 are connected iff |D_x - D_{x+1}| <= edge.  Output column p, at P = 8 p, is covered by
//        the span of a connected pair with L = t_{x+1} - t_x > 0 and t_x <= P < t_{x+1}: with a = P - t_x the nearness
//          (D_x (L - a) + D_{x+1} a + (L >> 1)) / L and the colours likewise;
//        the left cap of x, t_x - 4 <= P < t_x, iff x = 0 or (x - 1, x) is not connected; the right cap of x, t_x <= P < t_x + 4, iff
//          x = W - 1 or (x, x + 1) is not connected; both with D_x and c_x.
//   4. The piece with the largest nearness wins; ties go to the smallest x (no two pieces of one x cover the same P).
//   5. A column nothing covers takes the colour and nearness of the nearest covered column within R = max_s8 / 4 + 1 columns to its left or
//      to its right, the one with the SMALLER nearness, the left one on a tie; colour 0 and nearness 0 where neither exists.
#pragma once

#include "guided_solve.h"

#pragma clang fp contract(off)

#define ST_HD GS_HD

constexpr int ST_MAX_DIM = 16384;   // 1 <= H, W, CH, CW <= 16384
constexpr int ST_MAX_VIEWS = 64;    // 1 <= V <= 64: the table travels as a kernel argument
constexpr int ST_MAX_S8 = 512;      // 0 <= max_s8 <= 512: a shift of at most 64 pixels
constexpr int ST_MAX_G = 131072;    // |g| <= 2^17: (D - F) * g stays below 2^34, and 65535 * 2^17 >> 24 is just over max_s8's range
constexpr int ST_CAP = 4;           // half a pixel, in eighths
enum { ST_SPACE_DEPTH = 0, ST_SPACE_DISPARITY = 1 };

ST_HD int st_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Step 1
ST_HD int st_nearness(float pred, int space) {
    if (!(pred == pred)) return 0;
    const int q = (int)gs_quant16(pred);
    return space == ST_SPACE_DISPARITY ? q : 65535 - q;
}

// Step 2: the shift of a source of nearness D, in eighths of a pixel
ST_HD int st_shift(int D, int F, int g, int max_s8) {
    const long long v = ((long long)(D - F) * (long long)g + (1LL << 23)) >> 24;  // (arithmetic shift: a floor)
    return v < -max_s8 ? -max_s8 : (v > max_s8 ? max_s8 : (int)v);
}

// no source whose |s| is at most smax covers an output column more than this many columns away from its own
ST_HD int st_reach_pixels(int smax) { return (smax + 7) >> 3; }

// the hole search of step 5 looks this many columns to either side
ST_HD int st_fill_reach(int max_s8) { return max_s8 / 4 + 1; }

ST_HD bool st_connected(int Da, int Db, int edge) { return (Da > Db ? Da - Db : Db - Da) <= edge; }

// Step 3: one value of a span at a, 0 <= a < L: (v0 (L - a) + v1 a + (L >> 1)) / L, at most 65535 * 1032 + 516 < 2^27
ST_HD unsigned st_span(unsigned v0, unsigned v1, unsigned L, unsigned a) { return (v0 * (L - a) + v1 * a + (L >> 1)) / L; }

// the three colour bytes of a pixel as one word: channel k in bits 8 k .. 8 k + 7
ST_HD unsigned st_rgb(unsigned c0, unsigned c1, unsigned c2) { return c0 | c1 << 8 | c2 << 16; }
ST_HD unsigned st_span_rgb(unsigned c0, unsigned c1, unsigned L, unsigned a) {
    return st_rgb(st_span(c0 & 255u, c1 & 255u, L, a), st_span((c0 >> 8) & 255u, (c1 >> 8) & 255u, L, a),
                  st_span((c0 >> 16) & 255u, (c1 >> 16) & 255u, L, a));
}

// What covers an output column best so far: near < 0 while nothing does.
struct StBest {
    int near, x;
    unsigned rgb;
};

ST_HD void st_best_clear(StBest& b) {
    b.near = -1;
    b.x = 0;
    b.rgb = 0;
}

// Step 4: whether a piece of source x with this nearness beats the best so far -- nearer, or as near from a smaller x
ST_HD bool st_better(int near, int x, const StBest& b) { return near > b.near || (near == b.near && x < b.x); }

ST_HD void st_offer(StBest& b, int near, int x, unsigned rgb) {
    if (st_better(near, x, b)) {
        b.near = near;
        b.x = x;
        b.rgb = rgb;
    }
}

// Step 3 for source x and the output position P: its span towards x + 1 or its right cap, and its left cap.  left / right: whether x is
// connected to x - 1 / x + 1 (false at the borders); D1, c1, t1 are read only with right.  Returns the number of its pieces that cover P.
ST_HD int st_pieces(StBest& b, int P, int x, int D0, unsigned c0, int t0, bool left, bool right, int D1, unsigned c1, int t1) {
    int n = 0;
    if (right) {
        const int L = t1 - t0;
        if (L > 0 && t0 <= P && P < t1) {
            const unsigned a = (unsigned)(P - t0);
            st_offer(b, (int)st_span((unsigned)D0, (unsigned)D1, (unsigned)L, a), x, st_span_rgb(c0, c1, (unsigned)L, a));
            ++n;
        }
    } else if (t0 <= P && P < t0 + ST_CAP) {
        st_offer(b, D0, x, c0);
        ++n;
    }
    if (!left && t0 - ST_CAP <= P && P < t0) {
        st_offer(b, D0, x, c0);
        ++n;
    }
    return n;
}

// Step 5: whether a hole takes its left neighbour (it exists, and the right one does not or is nearer or as near)
ST_HD bool st_fill_from_left(bool has_l, int near_l, bool has_r, int near_r) { return has_l && (!has_r || near_l <= near_r); }

// The plane between the two passes: one word per output pixel, the nearness with bit 16 set where a piece covers it.
constexpr unsigned ST_COVERED = 1u << 16;

// the ranges of the call
ST_HD bool st_dims_ok(int B, int V, int H, int W) {
    return B >= 1 && B <= 65535 && V >= 1 && V <= ST_MAX_VIEWS && H >= 1 && W >= 1 && H <= ST_MAX_DIM && W <= ST_MAX_DIM &&
           (long long)B * V * H * W <= 0x7fffffffLL;
}
ST_HD bool st_options_ok(int space, int edge, int max_s8) {
    return (space == ST_SPACE_DEPTH || space == ST_SPACE_DISPARITY) && edge >= 0 && edge <= 65535 && max_s8 >= 0 && max_s8 <= ST_MAX_S8;
}
// one row g, ox, oy, cmask of the view table against the image and the canvas
ST_HD bool st_view_ok(const int* row, int H, int W, int CH, int CW) {
    return row[0] >= -ST_MAX_G && row[0] <= ST_MAX_G && row[3] >= 1 && row[3] <= 7 && row[1] >= 0 && row[2] >= 0 && row[1] <= CW - W &&
           row[2] <= CH - H;
}
// two views whose rectangles overlap and who write a common channel would race
ST_HD bool st_views_clash(const int* a, const int* b, int H, int W) {
    const int dx = a[1] > b[1] ? a[1] - b[1] : b[1] - a[1], dy = a[2] > b[2] ? a[2] - b[2] : b[2] - a[2];
    return (a[3] & b[3]) != 0 && dx < W && dy < H;
}
