// The guided upsampling on the CPU over the very text the device kernels use (genpercept_amd/csrc/guided_solve.h): a stand-alone program for
// tests/test_guided_host.py, which compares its models and outputs bit for bit with genpercept_amd/guided.py.  From the integer window sums
// it solves the local models, smooths them with plain loops in the order of the definition, and upsamples and applies them.
//   guided_check IN OUT
// IN:  int32 h, w, H, W, r, C; float64 eps; int64 N [h][w], S_I [3][h][w], S_II [6][h][w], S_p [C][h][w], S_Ip [C][3][h][w];
//      uint8 guide [3][H][W].   OUT: float64 a0, a1, a2, b [C][4][h][w]; float32 q [C][H][W].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/guided_solve.h"
#include "check_io.h"

typedef unsigned long long u64;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[6];
    double eps;
    if (!get(hd, 4, 6, f) || !get(&eps, 8, 1, f)) return 4;
    const int h = hd[0], w = hd[1], H = hd[2], W = hd[3], r = hd[4], C = hd[5];
    if (h < 1 || w < 1 || H < 1 || W < 1 || h > GS_MAX_DIM || w > GS_MAX_DIM || H > GS_MAX_DIM || W > GS_MAX_DIM) return 5;
    if (r < 1 || r > GS_MAX_R || (C != 1 && C != 3) || !(eps > 0.0 && eps <= 1.0)) return 5;
    const size_t hw = (size_t)h * w, HW = (size_t)H * W;
    std::vector<u64> N(hw), sI(3 * hw), sII(6 * hw), sp(C * hw), sIp(3 * C * hw);
    std::vector<unsigned char> guide(3 * HW);
    if (!get(N.data(), 8, hw, f) || !get(sI.data(), 8, 3 * hw, f) || !get(sII.data(), 8, 6 * hw, f) || !get(sp.data(), 8, C * hw, f) ||
        !get(sIp.data(), 8, 3 * C * hw, f) || !get(guide.data(), 1, 3 * HW, f))
        return 6;
    std::fclose(f);

    std::vector<double> ab(4 * C * hw), mean(4 * C * hw);
    for (int c = 0; c < C; ++c)
        for (size_t p = 0; p < hw; ++p) {
            const u64 vI[3] = {sI[p], sI[hw + p], sI[2 * hw + p]};
            const u64 vII[6] = {sII[p], sII[hw + p], sII[2 * hw + p], sII[3 * hw + p], sII[4 * hw + p], sII[5 * hw + p]};
            const u64 vIp[3] = {sIp[(3 * c) * hw + p], sIp[(3 * c + 1) * hw + p], sIp[(3 * c + 2) * hw + p]};
            double a[3], b;
            gs_solve((unsigned)N[p], vI, vII, sp[c * hw + p], vIp, eps * 65025.0, a, b);
            for (int k = 0; k < 3; ++k) ab[(4 * c + k) * hw + p] = a[k];
            ab[(4 * c + 3) * hw + p] = b;
        }
    for (int pl = 0; pl < 4 * C; ++pl)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int y0 = y - r > 0 ? y - r : 0, y1 = y + r < h - 1 ? y + r : h - 1, x0 = x - r > 0 ? x - r : 0, x1 = x + r < w - 1 ? x + r : w - 1;
                double col = 0.0;
                for (int yy = y0; yy <= y1; ++yy) {
                    double row = 0.0;
                    for (int xx = x0; xx <= x1; ++xx) row = row + ab[pl * hw + (size_t)yy * w + xx];
                    col = col + row;
                }
                if ((u64)(y1 - y0 + 1) * (u64)(x1 - x0 + 1) != N[(size_t)y * w + x]) return 7;
                mean[pl * hw + (size_t)y * w + x] = col / (double)((y1 - y0 + 1) * (x1 - x0 + 1));
            }
    std::vector<float> q(C * HW);
    for (int Y = 0; Y < H; ++Y) {
        int i0, i1;
        double fy;
        gs_index(Y, h, H, i0, i1, fy);
        if (i0 < 0 || i1 >= h || i0 > i1 || !(fy >= 0.0 && fy < 1.0)) return 8;
        for (int X = 0; X < W; ++X) {
            int j0, j1;
            double fx;
            gs_index(X, w, W, j0, j1, fx);
            if (j0 < 0 || j1 >= w || j0 > j1 || !(fx >= 0.0 && fx < 1.0)) return 8;
            const size_t P = (size_t)Y * W + X;
            const unsigned char g[3] = {guide[P], guide[HW + P], guide[2 * HW + P]};
            for (int c = 0; c < C; ++c) {
                double v[4];
                for (int k = 0; k < 4; ++k) {
                    const double* m = mean.data() + (4 * c + k) * hw;
                    v[k] = gs_blend(m[(size_t)i0 * w + j0], m[(size_t)i0 * w + j1], m[(size_t)i1 * w + j0], m[(size_t)i1 * w + j1], fx, fy);
                }
                const double A[3] = {v[0], v[1], v[2]};
                q[c * HW + P] = gs_apply(A, v[3], g);
            }
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(ab.data(), 8, ab.size(), f) || !put(q.data(), 4, q.size(), f)) return 10;
    std::fclose(f);
    // the 16-bit rule, for the test to compare with guided.quantize16: 0, 1, NaN, -0.25, 1.5, 0.5
    std::printf("%u %u %u %u %u %u\n", gs_quant16(0.0f), gs_quant16(1.0f), gs_quant16(0.0f / 1.0f * __builtin_nanf("")), gs_quant16(-0.25f),
                gs_quant16(1.5f), gs_quant16(0.5f));
    std::printf("ok\n");
    return 0;
}
