// The multi-level foreground estimation on the CPU over the very text the device kernels use (genpercept_amd/csrc/foreground_update.h): a
// stand-alone program for tests/test_foreground_host.py, which compares its F and B bit for bit with genpercept_amd/foreground.py.
//   foreground_check IN OUT
// IN:  int32 H, W, n_small, n_big; float32 reg, gw; uint8 image [3][H][W]; uint8 alpha [H][W].   OUT: float32 F [3][H][W], B [3][H][W].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/foreground_update.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[4];
    float rg[2];
    if (!get(hd, 4, 4, f) || !get(rg, 4, 2, f)) return 4;
    const int H = hd[0], W = hd[1], n_small = hd[2], n_big = hd[3];
    if (H < 1 || W < 1 || H > FG_MAX_DIM || W > FG_MAX_DIM) return 5;
    const size_t HW = (size_t)H * W;
    std::vector<unsigned char> img(3 * HW), alpha(HW);
    if (!get(img.data(), 1, 3 * HW, f) || !get(alpha.data(), 1, HW, f)) return 6;
    std::fclose(f);

    const int L = fg_num_levels(H, W);
    std::vector<float> cur, nxt, prev;  // planes [6][h * w]
    int hp = 1, wp = 1;
    for (int l = 0; l <= L; ++l) {
        const int hl = fg_level_size(H, L, l), wl = fg_level_size(W, L, l);
        const size_t n = (size_t)hl * wl;
        std::vector<float> a(n), I(3 * n);
        cur.assign(6 * n, 0.f);
        nxt.assign(6 * n, 0.f);
        for (int y = 0; y < hl; ++y)
            for (int x = 0; x < wl; ++x) {
                const size_t p = (size_t)y * wl + x, sp = (size_t)fg_src(y, H, hl) * W + fg_src(x, W, wl);
                a[p] = fg_unit(alpha[sp]);
                for (int c = 0; c < 3; ++c) I[c * n + p] = fg_unit(img[c * HW + sp]);
                const size_t pp = (size_t)fg_src(y, hp, hl) * wp + fg_src(x, wp, wl), np = (size_t)hp * wp;
                for (int c = 0; c < 3; ++c) {
                    cur[c * n + p] = l == 0 ? I[c * n + p] : prev[c * np + pp];
                    cur[(3 + c) * n + p] = l == 0 ? I[c * n + p] : prev[(3 + c) * np + pp];
                }
            }
        const int iters = hl <= FG_SMALL && wl <= FG_SMALL ? n_small : n_big;
        for (int k = 0; k < iters; ++k) {
            for (int y = 0; y < hl; ++y)
                for (int x = 0; x < wl; ++x) {
                    const size_t p = (size_t)y * wl + x;
                    const size_t nb[4] = {(size_t)y * wl + (x > 0 ? x - 1 : 0), (size_t)y * wl + (x + 1 < wl ? x + 1 : wl - 1),
                                          (size_t)(y > 0 ? y - 1 : 0) * wl + x, (size_t)(y + 1 < hl ? y + 1 : hl - 1) * wl + x};
                    float an[4], Fn[4][3], Bn[4][3], F[3], B[3];
                    for (int q = 0; q < 4; ++q) {
                        an[q] = a[nb[q]];
                        for (int c = 0; c < 3; ++c) Fn[q][c] = cur[c * n + nb[q]], Bn[q][c] = cur[(3 + c) * n + nb[q]];
                    }
                    const float Ip[3] = {I[p], I[n + p], I[2 * n + p]};
                    const float det = fg_update(a[p], Ip, an, Fn, Bn, rg[0], rg[1], F, B);
                    if (!(det > 0.f)) return 7;
                    for (int c = 0; c < 3; ++c) nxt[c * n + p] = F[c], nxt[(3 + c) * n + p] = B[c];
                }
            cur.swap(nxt);
        }
        prev = cur;
        hp = hl, wp = wl;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 8;
    if (!put(prev.data(), 4, 6 * HW, f)) return 9;
    std::fclose(f);
    // the byte rules, for the test to compare with foreground.to_bytes
    std::printf("%d %d %d %d\n", (int)fg_byte(0.0f), (int)fg_byte(0.5f), (int)fg_byte(1.0f), (int)fg_byte(fg_composite(0.25f, 1.0f, 0.2f)));
    std::printf("ok\n");
    return 0;
}
