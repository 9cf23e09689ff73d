// The relighting on the CPU over the very text the device kernel uses (genpercept_amd/csrc/relight_math.h): a stand-alone program for
// tests/test_relight_host.py, which compares its bytes with genpercept_amd/relight.py.  One image: every pixel, every light and every step of
// every march with plain loops, samples outside the image skipped, no early exit.
//   relight_check IN OUT
// IN:  int32 H, W, L, encoded, flip, space, has_pred, has_weight; int32 rows [L + 1][20]; uint16 to_lin [256]; uint8 from_lin [4096];
//      float32 normal [3][H][W]; uint8 image [3][H][W]; float32 pred [H][W] (has_pred); uint8 weight [H][W] (has_weight).
// OUT: uint8 out [3][H][W]; uint8 shadow [H][W].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/relight_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[8];
    if (!get(hd, 4, 8, f)) return 4;
    const int H = hd[0], W = hd[1], L = hd[2], encoded = hd[3], flip = hd[4], space = hd[5], has_pred = hd[6], has_weight = hd[7];
    if (!rl_dims_ok(1, H, W) || !rl_options_ok(L, encoded, flip, space, RL_MAX_REACH)) return 5;
    std::vector<int> rows((size_t)(L + 1) * RL_ROW);
    if (!get(rows.data(), 4, rows.size(), f) || !rl_table_ok(rows.data(), L, RL_MAX_REACH)) return 5;
    const size_t HW = (size_t)H * W;
    std::vector<unsigned short> to_lin(256);
    std::vector<unsigned char> from_lin(RL_LIN_MAX + 1), image(3 * HW), weight(has_weight ? HW : 0);
    std::vector<float> normal(3 * HW), pred(has_pred ? HW : 0);
    if (!get(to_lin.data(), 2, 256, f) || !get(from_lin.data(), 1, from_lin.size(), f) || !get(normal.data(), 4, normal.size(), f) ||
        !get(image.data(), 1, image.size(), f) || !get(pred.data(), 4, pred.size(), f) || !get(weight.data(), 1, weight.size(), f))
        return 6;
    std::fclose(f);

    // rl_isqrt is the exact root just below, at and just above a square, for roots around the shortest normal, the longest axis and the
    // longest normal
    const rl_u64 roots[] = {1, 2, 255, 256, 257, 65534, 65535, 65536, 113509, 113510, 113511, 113512, 131071};
    for (rl_u64 k : roots) {
        if (rl_isqrt(k * k - 1) != k - 1 || rl_isqrt(k * k) != k || rl_isqrt(k * k + 1) != k || rl_isqrt(k * k + 2 * k) != k) return 7;
    }
    const rl_u64 longest = (rl_u64)3 * 65535 * 65535, r3 = rl_isqrt(longest);  // the longest normal: floor(sqrt(3) * 65535) = 113509
    if (rl_isqrt(0) != 0 || r3 != 113509 || r3 * r3 > longest || (r3 + 1) * (r3 + 1) <= longest) return 7;
    // rl_ratio12 is the plain quotient, clamped, also where the numerator stands just below, at and just above a multiple of the divisor
    const long long dens[] = {1024, 1028, 4 * 65535LL, 4 * 113510LL, 4 * 40000LL};
    for (long long den : dens)
        for (long long q = 0; q <= 4097; ++q)
            for (int d = -2; d <= 2; ++d) {
                const long long num = q * den + d, want = num <= 0 ? 0 : (num / den > 4096 ? 4096 : num / den);
                if (rl_ratio12(num, den) != (int)want) return 8;
            }
    if (rl_ratio12(3LL * 65535 * 16384, 1024) != 4096 || rl_ratio12(-3LL * 65535 * 16384, 1024) != 0) return 8;

    std::vector<int> D(HW, 0);
    for (size_t i = 0; i < pred.size(); ++i) D[i] = rl_nearness(pred[i], space);
    std::vector<unsigned char> out(3 * HW), shadow(HW);
    const int* amb = rows.data() + (size_t)L * RL_ROW;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            const RlNormal nrm = rl_normal(normal[p], normal[HW + p], normal[2 * HW + p], encoded, flip);
            const bool lit = has_pred && pred[p] == pred[p];
            RlSums s;
            rl_sums_clear(s);
            for (int j = 0; j < L; ++j) {
                const int* row = rows.data() + (size_t)j * RL_ROW;
                const int cos12 = rl_cos12(nrm, row + RL_LX);
                if (cos12 == 0) continue;
                int E = 0;
                for (int t = 1; lit && t <= row[RL_REACH]; ++t) {
                    const int qx = x + rl_step(t, row[RL_UX]), qy = y + rl_step(t, row[RL_UY]);
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const int e = D[(size_t)qy * W + qx] - rl_floor(D[p], row, t);
                    E = e > E ? e : E;
                }
                rl_sums_add(s, row, cos12, rl_specular(nrm, row), rl_shade(E, row));
            }
            const unsigned w = has_weight ? weight[p] : 255u;
            for (int k = 0; k < 3; ++k) {
                const unsigned byte = image[k * HW + p];
                out[k * HW + p] = rl_blend(from_lin[rl_lin(s, amb, k, to_lin[byte])], byte, w);
            }
            shadow[p] = rl_shadow_byte(s.shade);
        }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(out.data(), 1, out.size(), f) || !put(shadow.data(), 1, shadow.size(), f)) return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
