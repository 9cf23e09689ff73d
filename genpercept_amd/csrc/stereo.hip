// Stereo and parallax views on the device (gp_stereo_views): the photograph re-rendered from viewpoints shifted sideways under its depth or
// disparity prediction, a forward warp.  Every row is a 1-D surface that is cut at depth edges and rasterised; the nearest surface wins, and
// the holes a new viewpoint opens are filled from the background side.  The definition is stated in include/genpercept_hip.h;
// genpercept_amd/stereo.py restates it on the host and gives the same bits; the arithmetic is stereo_math.h, which tests/stereo_check.cpp
// also runs on the CPU.
//   Two launches for any batch and any number of views.
//   warp     one workgroup of 256 threads per 256 output columns of one row of one image; it serves every view in turn.  The tile's source
//            columns plus an apron of A = ceil(max_s8 / 8) columns, the reach of the call's largest shift, and one more column on either
//            side (the neighbours the connections of the outermost sources are read from) are staged in LDS once: the nearness and one word
//            of colours per column.  For a view the positions t_x of the staged columns go to LDS; the shift is monotone in the nearness,
//            so the largest |s| of the STAGED REGION is that of its smallest or largest nearness, and a thread looks only at the sources
//            within ceil(smax / 8) columns of its own: one source where the region lies in the zero-parallax plane.  A thread keeps the best
//            piece of its column (stereo_math.h: nearer, or as near from a smaller x -- an order-free comparison), writes the view's
//            channels of the canvas where something covers the column, and the nearness with the covered bit to the plane.
//   fill     one workgroup per 256 output columns of one row of one view: the plane's words of the tile and of R = max_s8 / 4 + 1 columns on
//            either side go to LDS; a thread whose column nothing covers walks outwards to the nearest covered column on each side, takes
//            the one with the smaller nearness and copies its canvas bytes (a covered column, which this pass never writes).  holes and
//            near are written here for every column.
// No atomics, nothing read back; which thread computes which column depends on the sizes only and all arithmetic is integer, so an image's
// bytes are the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "stereo_math.h"

namespace {

constexpr int ST_TW = 256;                                   // output columns of a workgroup, one thread each
constexpr int ST_WAVES = ST_TW / 64;
constexpr int ST_MAX_A = (ST_MAX_S8 + 7) / 8;                // 64: the widest apron of the warp pass
constexpr int ST_STAGED = ST_TW + 2 * ST_MAX_A + 2;          // 386 source columns at most
constexpr int ST_MAX_FILL = ST_MAX_S8 / 4 + 1;               // 129: the widest apron of the fill pass
constexpr unsigned ST_EXISTS = 1u << 24;                     // in a staged colour word: the column lies inside the image

struct StViews {
    int v[ST_MAX_VIEWS][4];  // g, ox, oy, cmask
};

struct StCall {
    int H, W, CH, CW, V, space, edge, max_s8;
};

// grid (ceil(W / 256), H, B).  image: [B][3][H][W]; pred: [B][H][W]; conv: [B]; canvas: [B][3][CH][CW]; plane: [B][V][H][W].
__global__ __launch_bounds__(ST_TW) void st_warp_kernel(const unsigned char* __restrict__ image, const float* __restrict__ pred,
                                                       const int* __restrict__ conv, StViews views, StCall a, unsigned char* __restrict__ canvas,
                                                       unsigned* __restrict__ plane) {
    __shared__ int s_D[ST_STAGED];
    __shared__ unsigned s_c[ST_STAGED];
    __shared__ int s_t[ST_STAGED];
    __shared__ int s_lo[ST_WAVES], s_hi[ST_WAVES];
    const int tid = threadIdx.x, y = blockIdx.y;
    const long long b = blockIdx.z, HW = (long long)a.H * a.W;
    const int A = st_reach_pixels(a.max_s8), n = ST_TW + 2 * A + 2;  // (n <= ST_STAGED)
    const int x0 = blockIdx.x * ST_TW - A - 1;                        // the image column of staged column 0
    const int F = st_clamp(conv[b], 0, 65535);

    int lo = 65535, hi = 0;
    for (int i = tid; i < n; i += ST_TW) {
        const int x = x0 + i;
        int D = 0;
        unsigned c = 0;
        if (x >= 0 && x < a.W) {
            const long long q = (long long)y * a.W + x;
            D = st_nearness(pred[b * HW + q], a.space);
            const unsigned char* px = image + b * 3 * HW + q;
            c = st_rgb(px[0], px[HW], px[2 * HW]) | ST_EXISTS;
            lo = D < lo ? D : lo;
            hi = D > hi ? D : hi;
        }
        s_D[i] = D;
        s_c[i] = c;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((tid & 63) == 0) {
        s_lo[tid >> 6] = lo;
        s_hi[tid >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ST_WAVES; ++k) {
        lo = s_lo[k] < lo ? s_lo[k] : lo;
        hi = s_hi[k] > hi ? s_hi[k] : hi;
    }
    // (the tile's first column lies inside the image, so lo <= hi)

    const int p = blockIdx.x * ST_TW + tid, P = 8 * p, ci = tid + A + 1;
    for (int k = 0; k < a.V; ++k) {
        const int g = views.v[k][0], ox = views.v[k][1], oy = views.v[k][2], cmask = views.v[k][3];
        for (int i = tid; i < n; i += ST_TW) s_t[i] = 8 * (x0 + i) + st_shift(s_D[i], F, g, a.max_s8);
        __syncthreads();
        if (p < a.W) {
            const int s_a = st_shift(lo, F, g, a.max_s8), s_b = st_shift(hi, F, g, a.max_s8);
            const int smax = (s_a < 0 ? -s_a : s_a) > (s_b < 0 ? -s_b : s_b) ? (s_a < 0 ? -s_a : s_a) : (s_b < 0 ? -s_b : s_b);
            const int Rs = st_reach_pixels(smax);  // <= A: ci - Rs >= 1 and ci + Rs + 1 <= n - 1
            StBest best;
            st_best_clear(best);
            for (int i = ci - Rs; i <= ci + Rs; ++i) {
                const unsigned c0 = s_c[i];
                if (!(c0 & ST_EXISTS)) continue;
                const int D0 = s_D[i], D1 = s_D[i + 1];
                const unsigned c1 = s_c[i + 1];
                const bool left = (s_c[i - 1] & ST_EXISTS) && st_connected(s_D[i - 1], D0, a.edge);
                const bool right = (c1 & ST_EXISTS) && st_connected(D0, D1, a.edge);
                st_pieces(best, P, x0 + i, D0, c0 & 0xffffffu, s_t[i], left, right, D1, c1 & 0xffffffu, s_t[i + 1]);
            }
            plane[((b * a.V + k) * a.H + y) * a.W + p] = best.near < 0 ? 0u : ((unsigned)best.near | ST_COVERED);
            if (best.near >= 0) {
                const long long plane_c = (long long)a.CH * a.CW;
                unsigned char* o = canvas + b * 3 * plane_c + (long long)(oy + y) * a.CW + ox + p;
                if (cmask & 1) o[0] = (unsigned char)(best.rgb & 255u);
                if (cmask & 2) o[plane_c] = (unsigned char)((best.rgb >> 8) & 255u);
                if (cmask & 4) o[2 * plane_c] = (unsigned char)((best.rgb >> 16) & 255u);
            }
        }
        __syncthreads();  // (the next view overwrites s_t)
    }
}

// grid (ceil(W / 256) * V, H, B).  plane: [B][V][H][W]; canvas: [B][3][CH][CW]; holes, near: [B][V][H][W] or NULL.
__global__ __launch_bounds__(ST_TW) void st_fill_kernel(const unsigned* __restrict__ plane, StViews views, StCall a, int tiles_x,
                                                       unsigned char* canvas, unsigned char* __restrict__ holes,
                                                       unsigned short* __restrict__ near) {
    __shared__ unsigned s_p[ST_TW + 2 * ST_MAX_FILL];
    const int tid = threadIdx.x, y = blockIdx.y, k = blockIdx.x / tiles_x, tile = blockIdx.x - k * tiles_x;
    const long long b = blockIdx.z;
    const int R = st_fill_reach(a.max_s8), n = ST_TW + 2 * R;  // (R <= ST_MAX_FILL)
    const long long row = ((b * a.V + k) * a.H + y) * a.W;
    const int x0 = tile * ST_TW - R;
    for (int i = tid; i < n; i += ST_TW) {
        const int x = x0 + i;
        s_p[i] = x >= 0 && x < a.W ? plane[row + x] : 0u;  // (outside the image nothing is covered)
    }
    __syncthreads();
    const int p = tile * ST_TW + tid;
    if (p >= a.W) return;
    const int ci = tid + R;
    const unsigned me = s_p[ci];
    int value = (int)(me & 0xffffu);
    const bool hole = !(me & ST_COVERED);
    if (hole) {
        int dl = 0, dr = 0;  // the distance of the nearest covered column on either side, 0: none within R
        for (int d = 1; d <= R && !dl; ++d)
            if (s_p[ci - d] & ST_COVERED) dl = d;
        for (int d = 1; d <= R && !dr; ++d)
            if (s_p[ci + d] & ST_COVERED) dr = d;
        const int near_l = (int)(s_p[ci - dl] & 0xffffu), near_r = (int)(s_p[ci + dr] & 0xffffu);
        const int ox = views.v[k][1], oy = views.v[k][2], cmask = views.v[k][3];
        const long long plane_c = (long long)a.CH * a.CW;
        unsigned char* o = canvas + b * 3 * plane_c + (long long)(oy + y) * a.CW + ox + p;
        unsigned char c[3] = {0, 0, 0};
        value = 0;
        if (dl || dr) {
            const bool from_left = st_fill_from_left(dl != 0, near_l, dr != 0, near_r);
            const int d = from_left ? -dl : dr;  // (that column is covered: the warp pass wrote its bytes, this pass leaves them)
            value = from_left ? near_l : near_r;
            for (int ch = 0; ch < 3; ++ch)
                if (cmask >> ch & 1) c[ch] = o[ch * plane_c + d];
        }
        for (int ch = 0; ch < 3; ++ch)
            if (cmask >> ch & 1) o[ch * plane_c] = c[ch];
    }
    if (holes) holes[row + p] = hole ? 1 : 0;
    if (near) near[row + p] = (unsigned short)value;
}

}  // namespace

extern "C" {

long long gp_stereo_views_workspace(int B, int V, int H, int W) {
    if (!st_dims_ok(B, V, H, W)) return 0;
    return (4LL * B * V * H * W + 7) / 8 * 8;  // the plane between the two passes, one word per output pixel
}

gp_status gp_stereo_views(const unsigned char* image, const float* pred, const int* conv, const int* views, int B, int V, int H, int W, int CH,
                          int CW, int space, int edge, int max_s8, unsigned char* canvas, unsigned char* holes, unsigned short* near,
                          void* workspace, long long workspace_bytes, void* stream) {
    if (!image || !pred || !conv || !views || !canvas || !workspace) return GP_ERR_INVALID;
    if (!st_dims_ok(B, V, H, W) || !st_options_ok(space, edge, max_s8)) return GP_ERR_INVALID;
    if (CH < 1 || CW < 1 || CH > ST_MAX_DIM || CW > ST_MAX_DIM) return GP_ERR_INVALID;
    StViews table;
    for (int k = 0; k < V; ++k) {
        if (!st_view_ok(views + 4 * k, H, W, CH, CW)) return GP_ERR_INVALID;
        for (int j = 0; j < k; ++j)
            if (st_views_clash(views + 4 * j, views + 4 * k, H, W)) return GP_ERR_INVALID;
        for (int f = 0; f < 4; ++f) table.v[k][f] = views[4 * k + f];
    }
    for (int k = V; k < ST_MAX_VIEWS; ++k)
        for (int f = 0; f < 4; ++f) table.v[k][f] = 0;
    if ((((uintptr_t)pred | (uintptr_t)conv) & 3) != 0 || ((uintptr_t)near & 1) != 0 || ((uintptr_t)workspace & 7) != 0) return GP_ERR_INVALID;
    if (workspace_bytes < gp_stereo_views_workspace(B, V, H, W)) return GP_ERR_INVALID;
    if (canvas == image) return GP_ERR_INVALID;  // a view would overwrite the sources of the next
    const StCall a = {H, W, CH, CW, V, space, edge, max_s8};
    const int tiles_x = (W + ST_TW - 1) / ST_TW;
    unsigned* plane = (unsigned*)workspace;
    hipLaunchKernelGGL(st_warp_kernel, dim3(tiles_x, H, B), dim3(ST_TW), 0, (hipStream_t)stream, image, pred, conv, table, a, canvas, plane);
    hipLaunchKernelGGL(st_fill_kernel, dim3(tiles_x * V, H, B), dim3(ST_TW), 0, (hipStream_t)stream, plane, table, a, tiles_x, canvas, holes, near);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
