// The camera moves from one photograph on the CPU over the very text the device kernels use (genpercept_amd/csrc/parallax_math.h): a
// stand-alone program for tests/test_parallax_host.py, which compares its bytes with genpercept_amd/parallax.py.  One image: for every frame
// and output pixel EVERY cap and triangle of the image is offered with plain loops, in reverse order (no bound on the search), then the
// holes are filled.  What the device stages its sources by is held to that search on the way: every vertex of every piece that covers a
// pixel lies inside the source rectangle pv_source_range gives for the pixel's 32 x 32 tile under pv_frame_reach, and no rectangle has more
// than pv_staged_side sources on a side; the packed key orders two pieces as pv_offer does.
//   parallax_check IN OUT
// IN:  int32 H, W, space, edge, max_s8, V, F; int32 frames [V][4]; float32 pred [H][W]; uint8 image [3][H][W].
// OUT: uint8 out [V][3][H][W]; uint8 holes [V][H][W]; uint16 near [V][H][W]; int32 cover [V][H][W], the number of pieces that cover each
//      pixel; int32 piece [V][H][W], the id of the winning piece, -1 in a hole.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genpercept_amd/csrc/parallax_math.h"
#include "check_io.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int hd[7];
    if (!get(hd, 4, 7, f)) return 4;
    const int H = hd[0], W = hd[1], space = hd[2], edge = hd[3], max_s8 = hd[4], V = hd[5], F = st_clamp(hd[6], 0, 65535);
    if (!pv_dims_ok(1, V, H, W) || !pv_options_ok(space, edge, max_s8)) return 5;
    std::vector<int> frames(4 * (size_t)V);
    if (!get(frames.data(), 4, frames.size(), f)) return 6;
    for (int k = 0; k < V; ++k)
        if (!pv_frame_ok(&frames[4 * k])) return 7;
    const size_t HW = (size_t)H * W;
    std::vector<float> pred(HW);
    std::vector<unsigned char> image(3 * HW);
    if (!get(pred.data(), 4, HW, f) || !get(image.data(), 1, image.size(), f)) return 6;
    std::fclose(f);

    std::vector<unsigned char> out(V * 3 * HW), holes(V * HW);
    std::vector<unsigned short> near(V * HW);
    std::vector<int> cover(V * HW), piece(V * HW), best_near(HW);
    std::vector<unsigned> best_rgb(HW);
    std::vector<PvVertex> v(HW);
    const int R = pv_fill_reach(max_s8), side = pv_staged_side(max_s8);
    const int tiles_x = (W + PV_TILE - 1) / PV_TILE, tiles_y = (H + PV_TILE - 1) / PV_TILE;
    std::vector<int> rx0(tiles_x), rx1(tiles_x), ry0(tiles_y), ry1(tiles_y);
    for (int k = 0; k < V; ++k) {
        PvFrame fr;
        fr.gx = frames[4 * k], fr.gy = frames[4 * k + 1], fr.gz = frames[4 * k + 2], fr.Z = frames[4 * k + 3];
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t q = (size_t)y * W + x;
                v[q].D = st_nearness(pred[q], space);
                v[q].c = st_rgb(image[q], image[HW + q], image[2 * HW + q]);
                pv_position(x, y, W, H, v[q].D, F, fr, max_s8, v[q].tx, v[q].ty);
            }
        for (int t = 0; t < tiles_x; ++t) {
            const int p1 = t * PV_TILE + PV_TILE - 1 < W ? t * PV_TILE + PV_TILE - 1 : W - 1;
            pv_source_range(t * PV_TILE, p1, W, fr.Z, pv_frame_reach(fr.gx, fr.gz, pv_centre(W), max_s8), rx0[t], rx1[t]);
            if (rx0[t] < 0 || rx1[t] >= W || rx1[t] - rx0[t] + 1 > side) return 20;
        }
        for (int t = 0; t < tiles_y; ++t) {
            const int q1 = t * PV_TILE + PV_TILE - 1 < H ? t * PV_TILE + PV_TILE - 1 : H - 1;
            pv_source_range(t * PV_TILE, q1, H, fr.Z, pv_frame_reach(fr.gy, fr.gz, pv_centre(H), max_s8), ry0[t], ry1[t]);
            if (ry0[t] < 0 || ry1[t] >= H || ry1[t] - ry0[t] + 1 > side) return 20;
        }
        const int h = pv_cap_half(fr.Z);
        for (int q = 0; q < H; ++q)
            for (int p = 0; p < W; ++p) {
                PvBest best;
                pv_best_clear(best);
                unsigned long long best_key = 0;
                int n = 0;
                const int Px = 8 * p, Py = 8 * q, tx_ = p / PV_TILE, ty_ = q / PV_TILE;
                for (int y = H - 1; y >= 0; --y)
                    for (int x = W - 1; x >= 0; --x) {  // (backwards: the comparison does not lean on the order)
                        const size_t s = (size_t)y * W + x;
                        const long long id = 3LL * (long long)s;
                        // the id the device would use inside its staged rectangle: row-major there, so in the same order
                        const unsigned local = 3u * (unsigned)((y - ry0[ty_]) * (rx1[tx_] - rx0[tx_] + 1) + (x - rx0[tx_]));
                        const bool staged = x >= rx0[tx_] && x <= rx1[tx_] && y >= ry0[ty_] && y <= ry1[ty_];
                        if (pv_cap_covers(v[s].tx, v[s].ty, h, Px, Py)) {
                            if (!staged) return 21;
                            pv_offer(best, v[s].D, id, v[s].c);
                            const unsigned long long key = pv_key(v[s].D, local, v[s].c);
                            best_key = key > best_key ? key : best_key;
                            ++n;
                        }
                        if (x + 1 >= W || y + 1 >= H) continue;
                        const PvVertex &a = v[s], &b = v[s + 1], &c = v[s + W], &d = v[s + W + 1];
                        for (int t = 0; t < 2; ++t) {
                            const PvVertex &ta = t ? b : a, &tb = t ? d : b, &tc = c;
                            if (!pv_triangle_exists(ta.D, tb.D, tc.D, edge)) continue;
                            const long long A = pv_area(ta, tb, tc);
                            int value;
                            unsigned rgb;
                            if (A <= 0 || !pv_triangle(ta, tb, tc, A, Px, Py, value, rgb)) continue;
                            if (!staged || x + 1 > rx1[tx_] || y + 1 > ry1[ty_]) return 22;
                            pv_offer(best, value, id + 1 + t, rgb);
                            const unsigned long long key = pv_key(value, local + 1u + (unsigned)t, rgb);
                            best_key = key > best_key ? key : best_key;
                            ++n;
                        }
                    }
                const size_t o = (size_t)q * W + p;
                if ((best.near < 0) != (best_key == 0)) return 23;
                if (best.near >= 0 && (pv_key_near(best_key) != best.near || pv_key_rgb(best_key) != best.rgb)) return 23;
                best_near[o] = best.near;
                best_rgb[o] = best.rgb;
                cover[k * HW + o] = n;
                piece[k * HW + o] = best.near < 0 ? -1 : (int)best.id;
            }
        for (int q = 0; q < H; ++q)
            for (int p = 0; p < W; ++p) {
                const size_t o = (size_t)q * W + p;
                int value = best_near[o];
                unsigned rgb = best_rgb[o];
                const bool hole = value < 0;
                if (hole) {
                    const int sx[4] = {-1, 1, 0, 0}, sy[4] = {0, 0, -1, 1};
                    bool has[4] = {false, false, false, false};
                    int val[4] = {0, 0, 0, 0};
                    size_t at[4] = {0, 0, 0, 0};
                    for (int dir = 0; dir < 4; ++dir)
                        for (int d = 1; d <= R && !has[dir]; ++d) {
                            const int x = p + d * sx[dir], y = q + d * sy[dir];
                            if (x < 0 || x >= W || y < 0 || y >= H) break;
                            if (best_near[(size_t)y * W + x] >= 0) has[dir] = true, val[dir] = best_near[(size_t)y * W + x], at[dir] = (size_t)y * W + x;
                        }
                    const int pick = pv_fill_pick(has, val);
                    value = pick < 0 ? 0 : val[pick];
                    rgb = pick < 0 ? 0u : best_rgb[at[pick]];
                }
                for (int ch = 0; ch < 3; ++ch) out[(k * 3 + ch) * HW + o] = (unsigned char)(rgb >> (8 * ch) & 255u);
                holes[k * HW + o] = hole ? 1 : 0;
                near[k * HW + o] = (unsigned short)value;
            }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 9;
    if (!put(out.data(), 1, out.size(), f) || !put(holes.data(), 1, holes.size(), f) || !put(near.data(), 2, near.size(), f) ||
        !put(cover.data(), 4, cover.size(), f) || !put(piece.data(), 4, piece.size(), f))
        return 10;
    std::fclose(f);
    std::printf("ok\n");
    return 0;
}
