// The depth geometry on the CPU over the very text the device kernels use (genpercept_amd/csrc/depth_geometry_math.h): a stand-alone program
// for tests/test_geometry_host.py, which compares its planes and points bit for bit with genpercept_amd/geometry.py.  One image: the depth of
// every pixel, the window of every pixel walked in row-major order with plain loops, the per-pixel tail, the compaction in row-major order.
//   geometry_check IN OUT
// IN:  int32 H, W, space, r, min_count, stride, has_mask, has_image; float64 tau, min_cos, camera [8]; float32 pred [H][W]; uint8 mask [H][W]
//      (has_mask); uint8 image [3][H][W] (has_image).
// OUT: float32 xyz [3][H][W], normal [3][H][W]; uint8 keep [H][W]; int64 n; float32 points [n][3], point_normals [n][3]; uint8 point_rgb [n][3];
//      int32 point_index [n].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/depth_geometry_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[8];
    double opt[2 + DG_CAMERA];
    if (!get(hd, 4, 8, f) || !get(opt, 8, 2 + DG_CAMERA, f)) return 4;
    const int H = hd[0], W = hd[1], space = hd[2], r = hd[3], min_count = hd[4], stride = hd[5], has_mask = hd[6], has_image = hd[7];
    const double tau = opt[0], min_cos = opt[1];
    if (H < 1 || W < 1 || H > DG_MAX_DIM || W > DG_MAX_DIM || !dg_options_ok(space, r, tau, min_count, min_cos, stride) || !dg_camera_ok(opt + 2)) return 5;
    const DgCamera cam = {opt[2], opt[3], opt[4], opt[5], opt[6], opt[7], opt[8], opt[9]};
    const size_t HW = (size_t)H * W;
    std::vector<float> pred(HW);
    std::vector<unsigned char> mask(has_mask ? HW : 0), image(has_image ? 3 * HW : 0);
    if (!get(pred.data(), 4, HW, f) || !get(mask.data(), 1, mask.size(), f) || !get(image.data(), 1, image.size(), f)) return 6;
    std::fclose(f);

    std::vector<double> z(HW), w(HW);
    std::vector<unsigned char> valid(HW);
    for (size_t i = 0; i < HW; ++i) valid[i] = dg_depth(pred[i], !has_mask || mask[i] != 0, cam, space, z[i], w[i]) ? 1 : 0;
    std::vector<float> xyz(3 * HW), normal(3 * HW);
    std::vector<unsigned char> keep(HW);
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const size_t i = (size_t)v * W + u;
            DgSums s;
            dg_sums_clear(s);
            if (valid[i]) {
                const double lim = tau * z[i];
                for (int dv = -r; dv <= r; ++dv)
                    for (int du = -r; du <= r; ++du) {
                        const int y = v + dv, x = u + du;
                        if (y < 0 || y >= H || x < 0 || x >= W) continue;
                        const size_t j = (size_t)y * W + x;
                        if (valid[j] && dg_member(z[j], z[i], lim)) dg_sums_add(s, du, dv, w[j]);
                    }
            }
            float P[3], N[3];
            keep[i] = dg_pixel(u, v, valid[i] != 0, z[i], s, cam, min_count, min_cos, P, N) ? 1 : 0;
            for (int k = 0; k < 3; ++k) xyz[k * HW + i] = P[k], normal[k * HW + i] = N[k];
        }
    std::vector<float> points, point_normals;
    std::vector<unsigned char> point_rgb;
    std::vector<int> point_index;
    for (int v = 0; v < H; v += stride)
        for (int u = 0; u < W; u += stride) {
            const size_t i = (size_t)v * W + u;
            if (!keep[i]) continue;
            for (int k = 0; k < 3; ++k) {
                points.push_back(xyz[k * HW + i]);
                point_normals.push_back(normal[k * HW + i]);
                point_rgb.push_back(has_image ? image[k * HW + i] : 255);
            }
            point_index.push_back((int)i);
        }
    const long long n = (long long)point_index.size();
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(xyz.data(), 4, xyz.size(), f) || !put(normal.data(), 4, normal.size(), f) || !put(keep.data(), 1, keep.size(), f) || !put(&n, 8, 1, f) ||
        !put(points.data(), 4, points.size(), f) || !put(point_normals.data(), 4, point_normals.size(), f) ||
        !put(point_rgb.data(), 1, point_rgb.size(), f) || !put(point_index.data(), 4, point_index.size(), f))
        return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
