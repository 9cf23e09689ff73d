// The synthetic depth of field on the CPU over the very text the device kernel uses (genpercept_amd/csrc/lens_blur_math.h): a stand-alone
// program for tests/test_lens_blur_host.py, which compares its bytes with genpercept_amd/lens_blur.py.  One image: the word of every pixel,
// then for every output pixel the whole 65 x 65 window walked with plain loops, clipped to the image.
//   lens_blur_check IN OUT
// IN:  int32 H, W, space, has_sharp, F, gain, cmax8, dz; uint16 to_lin [256]; uint8 from_lin [4096]; float32 pred [H][W]; uint8 image [3][H][W];
//      uint8 sharp [H][W] (has_sharp).
// OUT: uint8 out [3][H][W]; uint16 coc [H][W]; uint32 w [257].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/lens_blur_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[8];
    if (!get(hd, 4, 8, f)) return 4;
    const int H = hd[0], W = hd[1], space = hd[2], has_sharp = hd[3];
    if (!lb_dims_ok(1, H, W) || !lb_options_ok(space, LB_MAX_C8)) return 5;
    const LbParams prm = lb_params(hd + 4, LB_MAX_C8);
    if (prm.F != hd[4] || prm.gain != hd[5] || prm.cmax8 != hd[6] || prm.dz != hd[7]) return 5;  // (the test sends values inside their ranges)
    const size_t HW = (size_t)H * W;
    std::vector<unsigned short> to_lin(256);
    std::vector<unsigned char> from_lin(LB_LIN_MAX + 1), image(3 * HW), sharp(has_sharp ? HW : 0);
    std::vector<float> pred(HW);
    if (!get(to_lin.data(), 2, 256, f) || !get(from_lin.data(), 1, from_lin.size(), f) || !get(pred.data(), 4, HW, f) ||
        !get(image.data(), 1, image.size(), f) || !get(sharp.data(), 1, sharp.size(), f))
        return 6;
    std::fclose(f);

    // lb_resolve is the plain quotient, also where 2 s + sw stands just below, at and just above a multiple of 2 sw
    const lb_u64 sws[] = {1, 3, 316, 4097, LB_ONE, (lb_u64)9 << 20, ((lb_u64)1 << 32) - 1};
    for (lb_u64 sw : sws)
        for (lb_u64 k = 0; k <= LB_LIN_MAX; ++k)
            for (int d = -2; d <= 2; ++d) {
                const long long s = (long long)(sw * k + sw / 2) + d;  // (the quotient steps from k to k + 1 at s = sw k + sw / 2)
                if (s < 0 || (lb_u64)s > LB_LIN_MAX * sw) continue;
                if (lb_resolve((lb_u64)s, sw) != (unsigned)((2 * (lb_u64)s + sw) / (2 * sw))) return 7;
            }
    std::vector<unsigned> w(LB_MAX_C8 + 1);
    for (int c = 0; c <= LB_MAX_C8; ++c) w[c] = lb_disc_weight(c);
    std::vector<lb_u64> word(HW);
    std::vector<unsigned short> coc(HW);
    for (size_t i = 0; i < HW; ++i) {
        const int D = lb_nearness(pred[i], space);
        const int c = lb_coc(D, !(pred[i] == pred[i]) || (has_sharp && sharp[i] != 0), prm);
        word[i] = lb_pack(D, c, to_lin[image[i]], to_lin[image[HW + i]], to_lin[image[2 * HW + i]]);
        coc[i] = (unsigned short)c;
    }
    std::vector<unsigned char> out(3 * HW);
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const size_t p = (size_t)v * W + u;
            const int Dp = lb_word_D(word[p]), cp = lb_word_c(word[p]);
            LbSums s;
            lb_sums_clear(s);
            for (int dy = -LB_MAX_R; dy <= LB_MAX_R; ++dy)
                for (int dx = -LB_MAX_R; dx <= LB_MAX_R; ++dx) {
                    const int y = v + dy, x = u + dx;
                    if (y < 0 || y >= H || x < 0 || x >= W) continue;
                    const lb_u64 q = word[(size_t)y * W + x];
                    const int r = lb_reach(lb_word_D(q), lb_word_c(q), Dp, cp);
                    if (lb_inside(dx * dx + dy * dy, r)) lb_sums_add(s, w[r], q);
                }
            for (int k = 0; k < 3; ++k) out[k * HW + p] = from_lin[lb_resolve(s.s[k], s.sw)];
        }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(out.data(), 1, out.size(), f) || !put(coc.data(), 2, coc.size(), f) || !put(w.data(), 4, w.size(), f)) return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
