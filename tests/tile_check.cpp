// The tile merge on the CPU over the very text the device kernels use (genpercept_amd/csrc/tile_merge_math.h): a stand-alone program for
// tests/test_tiled_host.py, which compares its grid, fits and outputs bit for bit with genpercept_amd/tiled.py.  It makes the grid from the
// rule, takes the five integer sums of every tile with plain loops, solves, and blends pixel by pixel in the order of the definition.
//   tile_check IN OUT
// IN:  int32 C, H, W, T, o, align; float32 base [C][H][W]; float32 tiles [N][C][wh][ww] (N, wh, ww follow from the rule).
// OUT: int32 ny, nx, wh, ww; int32 ys [ny], xs [nx]; float64 fit [N][2]; float32 q [C][H][W].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/tile_merge_math.h"
#include "check_io.h"

typedef unsigned long long u64;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[6];
    if (!get(hd, 4, 6, f)) return 4;
    const int C = hd[0], H = hd[1], W = hd[2], T = hd[3], o = hd[4], align = hd[5];
    if ((C != 1 && C != 3) || H < 1 || W < 1 || H > TM_MAX_DIM || W > TM_MAX_DIM || T < 1) return 5;
    const int wh = T < H ? T : H, ww = T < W ? T : W;
    if (!tm_axis_ok(H, wh, o) || !tm_axis_ok(W, ww, o) || (align != TM_ALIGN_LEAST_SQUARE && align != TM_ALIGN_NONE)) return 5;
    const int ny = tm_count(H, wh, o), nx = tm_count(W, ww, o), N = ny * nx;
    if (N > TM_MAX_TILES) return 5;
    std::vector<int> ys(ny), xs(nx);
    for (int k = 0; k < ny; ++k) ys[k] = tm_origin(k, H, wh, ny);
    for (int k = 0; k < nx; ++k) xs[k] = tm_origin(k, W, ww, nx);
    const size_t HW = (size_t)H * W, tsz = (size_t)wh * ww;
    std::vector<float> base(C * HW), tiles((size_t)N * C * tsz);
    if (!get(base.data(), 4, base.size(), f) || !get(tiles.data(), 4, tiles.size(), f)) return 6;
    std::fclose(f);

    std::vector<double> fit(2 * (size_t)N);
    for (int k = 0; k < N; ++k) {
        double s = 1.0, t = 0.0;
        if (align == TM_ALIGN_LEAST_SQUARE) {
            const int y0 = ys[k / nx], x0 = xs[k % nx];
            u64 n = 0, sP = 0, sG = 0, sPP = 0, sPG = 0;
            for (int c = 0; c < C; ++c)
                for (int y = 0; y < wh; ++y)
                    for (int x = 0; x < ww; ++x) {
                        const u64 P = gs_quant16(tiles[((size_t)k * C + c) * tsz + (size_t)y * ww + x]);
                        const u64 G = gs_quant16(base[c * HW + (size_t)(y0 + y) * W + (x0 + x)]);
                        n += 1, sP += P, sG += G, sPP += P * P, sPG += P * G;
                    }
            tm_solve(n, sP, sG, sPP, sPG, s, t);
        }
        fit[2 * k] = s, fit[2 * k + 1] = t;
    }
    std::vector<float> q(C * HW);
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double acc = 0.0;
                long long wsum = 0;
                for (int iy = 0; iy < ny; ++iy) {
                    if (y < ys[iy] || y >= ys[iy] + wh) continue;
                    for (int ix = 0; ix < nx; ++ix) {
                        if (x < xs[ix] || x >= xs[ix] + ww) continue;
                        const int k = iy * nx + ix, wgt = tm_weight(y, ys[iy], wh, o) * tm_weight(x, xs[ix], ww, o);
                        if (wgt < 1) return 7;
                        acc = tm_accumulate(acc, wgt, fit[2 * k], fit[2 * k + 1], tiles[((size_t)k * C + c) * tsz + (size_t)(y - ys[iy]) * ww + (x - xs[ix])]);
                        wsum += wgt;
                    }
                }
                if (wsum < 1) return 8;  // the grid covers the image
                q[c * HW + (size_t)y * W + x] = tm_finish(acc, wsum);
            }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    const int out_hd[4] = {ny, nx, wh, ww};
    if (!put(out_hd, 4, 4, f) || !put(ys.data(), 4, ys.size(), f) || !put(xs.data(), 4, xs.size(), f) || !put(fit.data(), 8, fit.size(), f) ||
        !put(q.data(), 4, q.size(), f))
        return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
