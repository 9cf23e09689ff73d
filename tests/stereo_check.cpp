// The stereo and parallax views on the CPU over the very text the device kernels use (genpercept_amd/csrc/stereo_math.h): a stand-alone
// program for tests/test_stereo_host.py, which compares its bytes with genpercept_amd/stereo.py.  One image: for every view, row and output
// column EVERY source column of the row is offered with plain loops (no bound on the search), then the holes are filled.
//   stereo_check IN OUT
// IN:  int32 H, W, space, edge, max_s8, V, F, CH, CW, fill; int32 views [V][4]; float32 pred [H][W]; uint8 image [3][H][W].
// OUT: uint8 canvas [3][CH][CW] (it starts as `fill` everywhere); uint8 holes [V][H][W]; uint16 near [V][H][W]; int32 cover [V][H][W], the
//      number of pieces that cover each column.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/stereo_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[10];
    if (!get(hd, 4, 10, f)) return 4;
    const int H = hd[0], W = hd[1], space = hd[2], edge = hd[3], max_s8 = hd[4], V = hd[5], F = st_clamp(hd[6], 0, 65535), CH = hd[7], CW = hd[8];
    if (!st_dims_ok(1, V, H, W) || !st_options_ok(space, edge, max_s8) || CH < 1 || CW < 1 || CH > ST_MAX_DIM || CW > ST_MAX_DIM) return 5;
    std::vector<int> views(4 * (size_t)V);
    if (!get(views.data(), 4, views.size(), f)) return 6;
    for (int k = 0; k < V; ++k) {
        if (!st_view_ok(&views[4 * k], H, W, CH, CW)) return 7;
        for (int j = 0; j < k; ++j)
            if (st_views_clash(&views[4 * j], &views[4 * k], H, W)) return 7;
    }
    const size_t HW = (size_t)H * W, plane_c = (size_t)CH * CW;
    std::vector<float> pred(HW);
    std::vector<unsigned char> image(3 * HW);
    if (!get(pred.data(), 4, HW, f) || !get(image.data(), 1, image.size(), f)) return 6;
    std::fclose(f);

    std::vector<unsigned char> canvas(3 * plane_c, (unsigned char)hd[9]), holes(V * HW);
    std::vector<unsigned short> near(V * HW);
    std::vector<int> cover(V * HW), D(W), t(W), best_near(W);
    std::vector<unsigned> c(W), best_rgb(W);
    const int R = st_fill_reach(max_s8);
    for (int k = 0; k < V; ++k) {
        const int g = views[4 * k], ox = views[4 * k + 1], oy = views[4 * k + 2], cmask = views[4 * k + 3];
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x) {
                const size_t q = (size_t)y * W + x;
                D[x] = st_nearness(pred[q], space);
                c[x] = st_rgb(image[q], image[HW + q], image[2 * HW + q]);
                t[x] = 8 * x + st_shift(D[x], F, g, max_s8);
            }
            for (int p = 0; p < W; ++p) {
                StBest best;
                st_best_clear(best);
                int n = 0;
                for (int x = W - 1; x >= 0; --x) {  // (backwards: the comparison does not lean on the order)
                    const bool left = x > 0 && st_connected(D[x - 1], D[x], edge), right = x + 1 < W && st_connected(D[x], D[x + 1], edge);
                    n += st_pieces(best, 8 * p, x, D[x], c[x], t[x], left, right, right ? D[x + 1] : 0, right ? c[x + 1] : 0u, right ? t[x + 1] : 0);
                }
                best_near[p] = best.near;
                best_rgb[p] = best.rgb;
                cover[(k * (size_t)H + y) * W + p] = n;
            }
            for (int p = 0; p < W; ++p) {
                int value = best_near[p];
                unsigned rgb = best_rgb[p];
                const bool hole = value < 0;
                if (hole) {
                    int dl = 0, dr = 0;
                    for (int d = 1; d <= R && !dl && p - d >= 0; ++d)
                        if (best_near[p - d] >= 0) dl = d;
                    for (int d = 1; d <= R && !dr && p + d < W; ++d)
                        if (best_near[p + d] >= 0) dr = d;
                    value = 0;
                    rgb = 0;
                    if (dl || dr) {
                        const int src = st_fill_from_left(dl != 0, dl ? best_near[p - dl] : 0, dr != 0, dr ? best_near[p + dr] : 0) ? p - dl : p + dr;
                        value = best_near[src];
                        rgb = best_rgb[src];
                    }
                }
                const size_t o = (size_t)(oy + y) * CW + ox + p, q = (k * (size_t)H + y) * W + p;
                for (int ch = 0; ch < 3; ++ch)
                    if (cmask >> ch & 1) canvas[ch * plane_c + o] = (unsigned char)(rgb >> (8 * ch) & 255u);
                holes[q] = hole ? 1 : 0;
                near[q] = (unsigned short)value;
            }
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(canvas.data(), 1, canvas.size(), f) || !put(holes.data(), 1, holes.size(), f) || !put(near.data(), 2, near.size(), f) ||
        !put(cover.data(), 4, cover.size(), f))
        return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
