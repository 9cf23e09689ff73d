// The triangle mesh from depth on the CPU over the very text the device kernels use (genpercept_amd/csrc/depth_mesh_math.h): a stand-alone
// program for tests/test_mesh_host.py, which compares its codes, vertices and faces bit for bit with genpercept_amd/mesh.py.  One image: the
// code of every cell with plain loops, the used nodes in row-major order as vertices, the triangles of the cells in row-major order as faces.
//   mesh_check IN OUT
// IN:  int32 H, W, stride, has_normal, has_image, 0; float64 cut; float32 xyz [3][H][W]; float32 normal [3][H][W] (has_normal); uint8 keep
//      [H][W]; uint8 image [3][H][W] (has_image).
// OUT: uint8 codes [gh][gw]; int64 n, m; float32 vertices [n][3]; float32 vertex_normals [n][3] (has_normal); uint8 vertex_rgb [n][3];
//      float32 vertex_uv [n][2]; int32 vertex_index [n]; int32 faces [m][3].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/depth_mesh_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[6];
    double cut;
    if (!get(hd, 4, 6, f) || !get(&cut, 8, 1, f)) return 4;
    const int H = hd[0], W = hd[1], stride = hd[2], has_normal = hd[3], has_image = hd[4];
    if (H < 1 || W < 1 || H > DG_MAX_DIM || W > DG_MAX_DIM || stride < 1 || stride > DG_MAX_STRIDE || !dm_cut_ok(cut)) return 5;
    const size_t HW = (size_t)H * W;
    std::vector<float> xyz(3 * HW), normal(has_normal ? 3 * HW : 0);
    std::vector<unsigned char> keep(HW), image(has_image ? 3 * HW : 0);
    if (!get(xyz.data(), 4, xyz.size(), f) || !get(normal.data(), 4, normal.size(), f) || !get(keep.data(), 1, HW, f) ||
        !get(image.data(), 1, image.size(), f))
        return 6;
    std::fclose(f);

    const int gh = (H + stride - 1) / stride, gw = (W + stride - 1) / stride;
    const auto pixel = [&](int gy, int gx) { return (size_t)gy * stride * W + (size_t)gx * stride; };
    const auto kept = [&](int gy, int gx) { return keep[pixel(gy, gx)] != 0; };
    const auto depth = [&](int gy, int gx) { return (double)xyz[2 * HW + pixel(gy, gx)]; };
    std::vector<unsigned char> codes((size_t)gh * gw, 0);
    for (int cy = 0; cy + 1 < gh; ++cy)
        for (int cx = 0; cx + 1 < gw; ++cx)
            codes[(size_t)cy * gw + cx] = (unsigned char)dm_cell_code(kept(cy, cx), depth(cy, cx), kept(cy, cx + 1), depth(cy, cx + 1), kept(cy + 1, cx),
                                                                      depth(cy + 1, cx), kept(cy + 1, cx + 1), depth(cy + 1, cx + 1), cut);
    const auto code_at = [&](int gy, int gx) { return gy >= 0 && gx >= 0 ? (unsigned)codes[(size_t)gy * gw + gx] : 0u; };
    std::vector<int> place((size_t)gh * gw, -1), vertex_index;
    std::vector<float> vertices, vertex_normals, vertex_uv;
    std::vector<unsigned char> vertex_rgb;
    for (int gy = 0; gy < gh; ++gy)
        for (int gx = 0; gx < gw; ++gx) {
            if (!dm_node_used(code_at(gy, gx), code_at(gy, gx - 1), code_at(gy - 1, gx), code_at(gy - 1, gx - 1))) continue;
            const size_t i = pixel(gy, gx);
            place[(size_t)gy * gw + gx] = (int)vertex_index.size();
            vertex_index.push_back((int)i);
            for (int k = 0; k < 3; ++k) {
                vertices.push_back(xyz[k * HW + i]);
                if (has_normal) vertex_normals.push_back(normal[k * HW + i]);
                vertex_rgb.push_back(has_image ? image[k * HW + i] : 255);
            }
            vertex_uv.push_back(dm_uv(gx * stride, W));
            vertex_uv.push_back(dm_uv(gy * stride, H));
        }
    std::vector<int> faces;
    for (int cy = 0; cy + 1 < gh; ++cy)
        for (int cx = 0; cx + 1 < gw; ++cx) {
            const unsigned code = codes[(size_t)cy * gw + cx];
            const size_t a = (size_t)cy * gw + cx;
            for (int slot = 0; slot < 2; ++slot) {
                int t[3];
                if (!dm_triangle(code, slot, place[a], place[a + 1], place[a + gw], place[a + gw + 1], t)) continue;
                for (int k = 0; k < 3; ++k) {
                    if (t[k] < 0) return 7;   // a triangle names a node that is no vertex
                    faces.push_back(t[k]);
                }
            }
        }
    const long long nm[2] = {(long long)vertex_index.size(), (long long)(faces.size() / 3)};
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(codes.data(), 1, codes.size(), f) || !put(nm, 8, 2, f) || !put(vertices.data(), 4, vertices.size(), f) ||
        !put(vertex_normals.data(), 4, vertex_normals.size(), f) || !put(vertex_rgb.data(), 1, vertex_rgb.size(), f) ||
        !put(vertex_uv.data(), 4, vertex_uv.size(), f) || !put(vertex_index.data(), 4, vertex_index.size(), f) || !put(faces.data(), 4, faces.size(), f))
        return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
