// The arithmetic of the camera moves from one photograph (gp_parallax_frames; definition in include/genpercept_hip.h), written once for the
// device kernels of parallax.hip and for a CPU program (tests/parallax_check.cpp): where a source pixel lands in a frame, the cap and the two
// triangles a source covers output pixels with, the comparison that picks the visible piece, the packed key the device keeps it in, the
// choice among the four neighbours of a hole, and the bounds the device stages its sources by.  No HIP header is needed.  The nearness, the
// connection test and the colour word are those of stereo_math.h.  Everything after the quantiser is integer arithmetic, so the result does
// not depend on the order the pieces are looked at.
//
// Definition, per image and frame (gx, gy, gz, Z).  D, c: the nearness and the three colour bytes of a source pixel (x, y).
//   1. D = st_nearness(pred, space): larger is nearer, 0 for a NaN pixel.
//   2. Cx = 4 (W - 1), Cy = 4 (H - 1); rx = 8 x - Cx, ry = 8 y - Cy; e = D - F; dz = (e gz + 2^23) >> 24;
//      dx = ((e gx + 2^23) >> 24) + ((rx dz + 2^15) >> 16), clamped to -max_s8 .. max_s8, dy likewise with gy and ry;
//      tx = Cx + ((rx Z + 2^15) >> 16) + dx, ty likewise: eighths of a pixel, every shift a floor, 64-bit intermediates.
//   3. Two pixels are connected iff |D_a - D_b| <= edge.  Output pixel (p, q) sits at P = (8 p, 8 q).
//        The cap of a source, id 3 (y W + x): tx - h <= Px < tx + h and ty - h <= Py < ty + h with h = (4 Z + 65535) >> 16; D and c.
//        T0 = (x, y), (x+1, y), (x, y+1), id 3 (y W + x) + 1, and T1 = (x+1, y), (x+1, y+1), (x, y+1), id 3 (y W + x) + 2, where x + 1 < W and
//        y + 1 < H and the three vertex pairs are all connected.  Vertices a, b, c in that order: A = (b - a) x (c - a); A <= 0 covers nothing;
//        wa = (c - b) x (P - b), wb = (a - c) x (P - c), wc = A - wa - wb; it covers P iff all three are >= 0, with the nearness
//        (wa D_a + wb D_b + wc D_c + (A >> 1)) / A and each colour channel likewise.
//   4. The piece with the largest nearness wins, the smallest id on a tie.
//   5. A pixel nothing covers takes the nearest covered pixel to its left, to its right, above and below within R = max_s8 / 4 + 1: of those the
//      one with the smallest nearness, ties in that order; colour 0 and nearness 0 where none exists.
#pragma once

#include "stereo_math.h"

#pragma clang fp contract(off)

#define PV_HD ST_HD

constexpr int PV_MAX_DIM = 16384;      // 1 <= H, W <= 16384
constexpr int PV_MAX_FRAMES = 64;      // 1 <= V <= 64: the table travels as a kernel argument
constexpr int PV_MAX_S8 = 256;         // 0 <= max_s8 <= 256: a displacement of at most 32 pixels
constexpr int PV_MAX_G = 131072;       // |gx|, |gy| <= 2^17
constexpr int PV_MAX_GZ = 1 << 24;     // |gz| <= 2^24: |dz| <= 65535
constexpr int PV_Z_MIN = 65536;        // a zoom of 1 x ...
constexpr int PV_Z_MAX = 131072;       // ... to 2 x, in units of 1 / 65536
constexpr int PV_TILE = 32;            // the device's output tile, PV_TILE x PV_TILE pixels

struct PvFrame {
    int gx, gy, gz, Z;
};

// ---- step 2 ----
PV_HD int pv_centre(int n) { return 4 * (n - 1); }

// where the source at r = 8 x - C lands before its displacement, relative to C: (r Z + 2^15) >> 16
PV_HD int pv_scaled(int r, int Z) { return (int)(((long long)r * Z + (1LL << 15)) >> 16); }

// the source coordinate x of an axis of n pixels in the frame's eighths, without its displacement
PV_HD int pv_base(int x, int n, int Z) { return pv_centre(n) + pv_scaled(8 * x - pv_centre(n), Z); }

PV_HD int pv_dz(int e, int gz) { return (int)(((long long)e * gz + (1LL << 23)) >> 24); }

// the displacement along one axis before the clamp (64-bit: |r dz| reaches 2^32)
PV_HD long long pv_displacement_raw(int e, int g, int r, int dz) {
    return (((long long)e * g + (1LL << 23)) >> 24) + (((long long)r * dz + (1LL << 15)) >> 16);
}

PV_HD int pv_displacement(int e, int g, int r, int dz, int max_s8) {
    const long long v = pv_displacement_raw(e, g, r, dz);
    return v < -max_s8 ? -max_s8 : (v > max_s8 ? max_s8 : (int)v);
}

PV_HD void pv_position(int x, int y, int W, int H, int D, int F, const PvFrame& f, int max_s8, int& tx, int& ty) {
    const int rx = 8 * x - pv_centre(W), ry = 8 * y - pv_centre(H), e = D - F, dz = pv_dz(e, f.gz);
    tx = pv_centre(W) + pv_scaled(rx, f.Z) + pv_displacement(e, f.gx, rx, dz, max_s8);
    ty = pv_centre(H) + pv_scaled(ry, f.Z) + pv_displacement(e, f.gy, ry, dz, max_s8);
}

// ---- step 3 ----
PV_HD int pv_cap_half(int Z) { return (4 * Z + 65535) >> 16; }  // 4 .. 8 eighths

PV_HD bool pv_cap_covers(int tx, int ty, int h, int Px, int Py) { return tx - h <= Px && Px < tx + h && ty - h <= Py && Py < ty + h; }

struct PvVertex {
    int tx, ty, D;
    unsigned c;
};

PV_HD long long pv_cross(long long ax, long long ay, long long bx, long long by) { return ax * by - ay * bx; }

PV_HD long long pv_area(const PvVertex& a, const PvVertex& b, const PvVertex& c) { return pv_cross(b.tx - a.tx, b.ty - a.ty, c.tx - a.tx, c.ty - a.ty); }

// num / A for 0 <= num < 2^53 and 0 < A < 2^31, exactly: the float64 quotient is within one of the floor, the remainder sets it right
PV_HD long long pv_div(long long num, long long A) {
    long long q = (long long)((double)num / (double)A);
    const long long r = num - q * A;
    if (r < 0) --q;
    if (r >= A) ++q;
    return q;
}

// Whether the triangle a, b, c (in that order; A = pv_area > 0) covers P, and then its nearness and colours there.
PV_HD bool pv_triangle(const PvVertex& a, const PvVertex& b, const PvVertex& c, long long A, int Px, int Py, int& near, unsigned& rgb) {
    const long long wa = pv_cross(c.tx - b.tx, c.ty - b.ty, Px - b.tx, Py - b.ty);
    const long long wb = pv_cross(a.tx - c.tx, a.ty - c.ty, Px - c.tx, Py - c.ty);
    const long long wc = A - wa - wb;
    if (wa < 0 || wb < 0 || wc < 0) return false;
    const long long half = A >> 1;
    near = (int)pv_div(wa * a.D + wb * b.D + wc * c.D + half, A);
    unsigned ch[3];
    for (int k = 0; k < 3; ++k)
        ch[k] = (unsigned)pv_div(wa * (long long)((a.c >> (8 * k)) & 255u) + wb * (long long)((b.c >> (8 * k)) & 255u) +
                                     wc * (long long)((c.c >> (8 * k)) & 255u) + half,
                                 A);
    rgb = st_rgb(ch[0], ch[1], ch[2]);
    return true;
}

// whether the three vertex pairs of a triangle are all connected
PV_HD bool pv_triangle_exists(int Da, int Db, int Dc, int edge) { return st_connected(Da, Db, edge) && st_connected(Db, Dc, edge) && st_connected(Da, Dc, edge); }

// ---- step 4 ----
// What covers an output pixel best so far: near < 0 while nothing does.
struct PvBest {
    int near;
    long long id;
    unsigned rgb;
};

PV_HD void pv_best_clear(PvBest& b) {
    b.near = -1;
    b.id = 0;
    b.rgb = 0;
}

PV_HD void pv_offer(PvBest& b, int near, long long id, unsigned rgb) {
    if (near > b.near || (near == b.near && id < b.id)) {
        b.near = near;
        b.id = id;
        b.rgb = rgb;
    }
}

// The same order as one number, for a maximum: the nearness in the top 16 bits, the inverted id of the piece (below 2^24, and monotone in
// the id of the definition) in the next 24, the colours in the low 24.  No key is 0.
PV_HD unsigned long long pv_key(int near, unsigned local_id, unsigned rgb) {
    return (unsigned long long)(unsigned)near << 48 | (unsigned long long)(0xffffffu - local_id) << 24 | (unsigned long long)(rgb & 0xffffffu);
}
PV_HD int pv_key_near(unsigned long long key) { return (int)(key >> 48); }
PV_HD unsigned pv_key_rgb(unsigned long long key) { return (unsigned)(key & 0xffffffu); }

// ---- step 5 ----
PV_HD int pv_fill_reach(int max_s8) { return max_s8 / 4 + 1; }

// Which of the four neighbours (left, right, up, down; has[k]: it exists) a hole takes: the smallest nearness, the first on a tie; -1: none.
PV_HD int pv_fill_pick(const bool (&has)[4], const int (&near)[4]) {
    int pick = -1;
    for (int k = 0; k < 4; ++k)
        if (has[k] && (pick < 0 || near[k] < near[pick])) pick = k;
    return pick;
}

// The plane between the two passes: one word per output pixel, the nearness with bit 16 set where a piece covers it.
constexpr unsigned PV_COVERED = 1u << 16;

// ---- what the device stages its sources by (never part of the result) ----
// No source of a frame is displaced further than this along an axis whose centre is C: |(e g + 2^23) >> 24| <= (65535 |g| + 2^23) >> 24
// for |e| <= 65535, the same for dz, and |r| <= C.
PV_HD int pv_frame_reach(int g, int gz, int C, int max_s8) {
    const long long ag = g < 0 ? -(long long)g : g, az = gz < 0 ? -(long long)gz : gz;
    const long long shift = (65535LL * ag + (1LL << 23)) >> 24, dz = (65535LL * az + (1LL << 23)) >> 24;
    const long long v = shift + (((long long)C * dz + (1LL << 15)) >> 16);
    return v > max_s8 ? max_s8 : (int)v;
}

// neighbouring sources lie at most this far apart before their displacements; a cap is no wider than half of it on either side
PV_HD int pv_pitch_max(int Z) { return (8 * Z + 65535) >> 16; }  // 8 .. 16 eighths

// the smallest x in 0 .. n with pv_base(x) >= lo (n: none); pv_base does not decrease with x
PV_HD int pv_first_at_least(int lo, int n, int Z) {
    const int C = pv_centre(n);
    long long x = (((long long)(lo - C) * 65536) / Z + C) / 8;  // an estimate, set right below
    x = x < 0 ? 0 : (x > n ? n : x);
    int i = (int)x;
    while (i > 0 && pv_base(i - 1, n, Z) >= lo) --i;
    while (i < n && pv_base(i, n, Z) < lo) ++i;
    return i;
}

// The sources x0 .. x1 of an axis of n pixels that a piece covering one of the output pixels p0 .. p1 can have a vertex at, under
// displacements of at most `reach`: a piece that covers P has a vertex at or before P and one at or after it, and its vertices lie within
// pv_pitch_max of one another before their displacements.  x1 < x0: none.
PV_HD void pv_source_range(int p0, int p1, int n, int Z, int reach, int& x0, int& x1) {
    const int m = pv_pitch_max(Z);
    x0 = pv_first_at_least(8 * p0 - reach - m, n, Z);
    x1 = pv_first_at_least(8 * p1 + reach + m + 1, n, Z) - 1;
}

// pv_source_range gives at most this many sources for a tile of PV_TILE pixels: they are at least 8 eighths apart over a stretch of
// 8 (PV_TILE - 1) + 2 max_s8 + 2 * 16
PV_HD int pv_staged_side(int max_s8) { return PV_TILE + (max_s8 + 16 + 3) / 4; }

// ---- the ranges of the call ----
PV_HD bool pv_dims_ok(int B, int V, int H, int W) {
    return B >= 1 && B <= 65535 && V >= 1 && V <= PV_MAX_FRAMES && H >= 1 && W >= 1 && H <= PV_MAX_DIM && W <= PV_MAX_DIM &&
           (long long)B * V * H * W <= 0x7fffffffLL;
}
PV_HD bool pv_options_ok(int space, int edge, int max_s8) {
    return (space == ST_SPACE_DEPTH || space == ST_SPACE_DISPARITY) && edge >= 0 && edge <= 65535 && max_s8 >= 0 && max_s8 <= PV_MAX_S8;
}
// one row gx, gy, gz, Z of the frame table
PV_HD bool pv_frame_ok(const int* row) {
    return row[0] >= -PV_MAX_G && row[0] <= PV_MAX_G && row[1] >= -PV_MAX_G && row[1] <= PV_MAX_G && row[2] >= -PV_MAX_GZ && row[2] <= PV_MAX_GZ &&
           row[3] >= PV_Z_MIN && row[3] <= PV_Z_MAX;
}
