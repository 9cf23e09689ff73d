// Host-side number conversion and weight packing (pure host code): fp32 <-> the library's 16-bit element, and the packed weight layouts the
// conv / GEMM kernels read.  Shared by the engine (engine.hip) and the per-kernel entry points (kernel_abi.hip).
#pragma once
#include <cstring>
#include <vector>

#include "kernels.h"

namespace {

// fp32 -> the library's 16-bit element (common.h), round-to-nearest-even
inline h16_t f_to_h16_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
#if GP_F16
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (h16_t)(sign | 0x7e00u);                    // NaN
    if (a >= 0x477ff000u) return (h16_t)(sign | 0x7bffu);                   // >= 65520 rounds past the largest finite value: saturate
    if (a < 0x33000001u) return (h16_t)sign;                                // <= 2^-25: rounds to zero
    if (a < 0x38800000u) {                                                  // subnormal result: value = m * 2^-24
        const int e = (int)(a >> 23);                                       // biased fp32 exponent, 102 .. 112
        const uint32_t m = (a & 0x7fffffu) | 0x800000u;
        const int sh = 126 - e;                                             // 14 .. 24: bits dropped from the 24-bit significand
        const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
        return (h16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = a + 0xfffu + ((a >> 13) & 1u);                       // round the 13 dropped bits to nearest even
    return (h16_t)(sign | ((r - 0x38000000u) >> 13));
#else
    if ((u & 0x7fffffffu) > 0x7f800000u) return (h16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (h16_t)(u >> 16);
#endif
}
inline float half_to_float(uint16_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s;
        else {
            int sh = 0;
            uint32_t mm = m;
            while (!(mm & 0x400)) { mm <<= 1; ++sh; }
            u = s | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ff) << 13);
        }
    } else if (e == 31) u = s | 0x7f800000u | (m << 13);
    else u = s | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

inline float h16_to_float_host(h16_t h) {
#if GP_F16
    return half_to_float(h);
#else
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// GEGLU projection rows [value(0..C4) ; gate(0..C4)] -> packed order: every 32-row block holds 16 outputs, value j at
// 8*(j%16/4) + j%4 and its gate 4 rows further, which is where the igemm epilogue finds them in one lane.
inline int geglu_row(int n, int cout) {
    const int half = cout / 2;
    const bool gate = n >= half;
    const int r = gate ? n - half : n;
    return (r / 16) * 32 + ((r % 16) / 4) * 8 + (gate ? 4 : 0) + (r % 4);
}
// Pack [cout][cin][ks][ks] fp32 -> [n_rows][taps][cin_pad] bf16 (+ optional GEGLU row interleave).
// split: cin_pad is the logical padded width, the row holds 3 cin_pad elements per tap in B order [hi | hi | lo] (contract precision)
inline void pack_rows(const float* w, int cout, int cin, int ks, int cin_pad, bool geglu, std::vector<h16_t>& out, int row0, int n_rows_total,
                      bool split = false) {
    const int taps = ks * ks;
    (void)n_rows_total;
    const size_t kw = split ? (size_t)3 * cin_pad : (size_t)cin_pad;  // elements per tap
    for (int n = 0; n < cout; ++n) {
        int dst = n;
        if (geglu) {
            dst = geglu_row(n, cout);
        }
        h16_t* o = out.data() + (size_t)(row0 + dst) * taps * kw;
        const float* wi = w + (size_t)n * cin * taps;
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < taps; ++t) {
                const float x = wi[(size_t)c * taps + t];
                const h16_t hi = f_to_h16_host(x);
                o[(size_t)t * kw + c] = hi;
                if (split) {
                    o[(size_t)t * kw + cin_pad + c] = hi;
                    o[(size_t)t * kw + 2 * cin_pad + c] = f_to_h16_host(x - h16_to_float_host(hi));
                }
            }
    }
}
// The x2-nearest-upsample 3x3 conv as four 2 x 2-tap phase convolutions on the source map (conv_halo.hip, PH): output pixel (2y + a, 2x + b) reads
// source rows {y - 1 + a, y + a} with the kernel rows that fall onto the same source row summed -- a = 0: {w[0]}, {w[1] + w[2]}; a = 1: {w[0] + w[1]},
// {w[2]} -- and the same along x.  Sums in fp32, ONE rounding to the element type.  Layout [n_rows][phase = 2 a + b][tap = 2 ty + tx][cin_pad].
// split (contract precision): 3 cin_pad elements per tap in B order [hi | hi | lo] of the fp32 sum, like pack_rows
inline void pack_phase_rows(const float* w, int cout, int cin, int cin_pad, std::vector<h16_t>& out, bool split = false) {
    static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};  // [phase][tap]: kernel index range [lo, hi]
    const size_t kw = split ? (size_t)3 * cin_pad : (size_t)cin_pad;
    for (int n = 0; n < cout; ++n)
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b)
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        h16_t* o = out.data() + (((size_t)n * 4 + (2 * a + b)) * 4 + (2 * ty + tx)) * kw;
                        for (int c = 0; c < cin; ++c) {
                            const float* wi = w + ((size_t)n * cin + c) * 9;
                            float acc = 0.f;
                            for (int ky = lo[a][ty]; ky <= hi[a][ty]; ++ky)
                                for (int kx = lo[b][tx]; kx <= hi[b][tx]; ++kx) acc += wi[ky * 3 + kx];
                            const h16_t h = f_to_h16_host(acc);
                            o[c] = h;
                            if (split) {
                                o[cin_pad + c] = h;
                                o[2 * cin_pad + c] = f_to_h16_host(acc - h16_to_float_host(h));
                            }
                        }
                    }
}

}  // namespace
