// Camera moves from one photograph on the device (gp_parallax_frames): the frames of a short clip in which the camera orbits, swings or
// pushes into a still under its depth or disparity prediction, a forward warp in two dimensions.  The picture is a triangle mesh over the
// pixel grid, cut at depth edges and rasterised with a z-test; the holes a move opens are filled from the background side.  The definition
// is stated in include/genpercept_hip.h; genpercept_amd/parallax.py restates it on the host and gives the same bits; the arithmetic is
// parallax_math.h, which tests/parallax_check.cpp also runs on the CPU.
//   Two launches for any batch and any number of frames.
//   warp     one workgroup of 256 threads per 32 x 32 output pixels of one frame of one image.  The frame's own largest displacement
//            (pv_frame_reach: from its row of the table alone, at most max_s8) bounds the rectangle of sources that can have a vertex of a
//            piece covering the tile (pv_source_range: the tile mapped back through Z, widened by the reach and the pitch); a frame that
//            does not move stages 34 x 34 sources, the widest call 100 x 100.  Per staged source the nearness, one word of colours and the
//            tile-relative position as two int16 go to dynamic LDS, sized by the call's max_s8 (8 KiB + 12 B per source, 125 KiB at most).
//            Then every staged cap and every triangle whose three vertices are staged is rasterised over the tile pixels of its bounding box
//            into a z-buffer of 32 x 32 64-bit keys in LDS by an LDS atomic maximum (pv_key: the nearness, the inverted row-major id of
//            the piece within the staged rectangle -- monotone in the id of the definition --, the colours).  The maximum is step 4 whatever
//            the order.  A triangle with a vertex outside the rectangle cannot cover a pixel of the tile.  The tile's bytes and its
//            nearness | covered words of the plane are written from the keys.
//   fill     one thread per output pixel: a pixel nothing covers walks the plane outwards along its row and its column, at most
//            R = max_s8 / 4 + 1 pixels each way, and copies the frame bytes of the neighbour pv_fill_pick chooses (a covered pixel, which
//            this pass never writes).  holes and near are written here for every pixel.
// No global atomics, nothing read back; which workgroup computes which tile depends on the sizes only and all arithmetic is integer, so an
// image's bytes are the same in every batch and from call to call.  The pre-pass over the map's smallest and largest nearness that would
// tighten the reach further is not built: the frame's row bounds it without reading the map.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "kernels.h"
#include "parallax_math.h"

namespace {

constexpr int PV_THREADS = 256;
constexpr int PV_ZBUF_BYTES = PV_TILE * PV_TILE * 8;
typedef unsigned long long pv_u64;

struct PvFrames {
    int v[PV_MAX_FRAMES][4];  // gx, gy, gz, Z
};

struct PvCall {
    int H, W, V, space, edge, max_s8, tiles_x, side;
};

__host__ __device__ inline int pv_lds_bytes(int side) { return PV_ZBUF_BYTES + 12 * side * side; }

__device__ __forceinline__ unsigned pv_pack(int tx, int ty) { return ((unsigned)tx & 0xffffu) | ((unsigned)ty << 16); }
__device__ __forceinline__ PvVertex pv_vertex(const int* s_D, const unsigned* s_c, const unsigned* s_t, int i) {
    const unsigned t = s_t[i];
    PvVertex v;
    v.tx = (int)(short)(t & 0xffffu);
    v.ty = (int)(short)(t >> 16);
    v.D = s_D[i];
    v.c = s_c[i];
    return v;
}

// One triangle over the tile pixels of its bounding box (tw x th pixels; positions are relative to the tile's first pixel).
__device__ __forceinline__ void pv_raster(pv_u64* s_z, const PvVertex& a, const PvVertex& b, const PvVertex& c, unsigned id, int tw, int th) {
    const long long A = pv_area(a, b, c);
    if (A <= 0) return;
    const int min_x = min(a.tx, min(b.tx, c.tx)), max_x = max(a.tx, max(b.tx, c.tx));
    const int min_y = min(a.ty, min(b.ty, c.ty)), max_y = max(a.ty, max(b.ty, c.ty));
    const int x0 = max(0, (min_x + 7) >> 3), x1 = min(tw - 1, max_x >> 3), y0 = max(0, (min_y + 7) >> 3), y1 = min(th - 1, max_y >> 3);
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            int near;
            unsigned rgb;
            if (pv_triangle(a, b, c, A, 8 * x, 8 * y, near, rgb)) atomicMax(&s_z[y * PV_TILE + x], pv_key(near, id, rgb));
        }
}

// grid (tiles_x * tiles_y, V, B).  image: [B][3][H][W]; pred: [B][H][W]; focus: [B]; out: [B][V][3][H][W]; plane: [B][V][H][W].
__global__ __launch_bounds__(PV_THREADS) void pv_warp_kernel(const unsigned char* __restrict__ image, const float* __restrict__ pred,
                                                            const int* __restrict__ focus, PvFrames frames, PvCall a,
                                                            unsigned char* __restrict__ out, unsigned* __restrict__ plane) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_pv[];
    pv_u64* s_z = (pv_u64*)s_pv;
    int* s_D = (int*)(s_pv + PV_ZBUF_BYTES);
    unsigned* s_c = (unsigned*)(s_D + a.side * a.side);
    unsigned* s_t = s_c + a.side * a.side;
    const int tid = threadIdx.x, k = blockIdx.y, tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const long long b = blockIdx.z, HW = (long long)a.H * a.W;
    const int p0 = tile_x * PV_TILE, q0 = tile_y * PV_TILE;
    const int tw = min(PV_TILE, a.W - p0), th = min(PV_TILE, a.H - q0);
    const int F = st_clamp(focus[b], 0, 65535);
    PvFrame f;
    f.gx = frames.v[k][0], f.gy = frames.v[k][1], f.gz = frames.v[k][2], f.Z = frames.v[k][3];

    int x0, x1, y0, y1;
    pv_source_range(p0, p0 + tw - 1, a.W, f.Z, pv_frame_reach(f.gx, f.gz, pv_centre(a.W), a.max_s8), x0, x1);
    pv_source_range(q0, q0 + th - 1, a.H, f.Z, pv_frame_reach(f.gy, f.gz, pv_centre(a.H), a.max_s8), y0, y1);
    const int nx = min(max(x1 - x0 + 1, 0), a.side), ny = min(max(y1 - y0 + 1, 0), a.side);  // (pv_staged_side: never more than side)
    const int n = nx * ny;

    for (int i = tid; i < PV_TILE * PV_TILE; i += PV_THREADS) s_z[i] = 0;
    for (int i = tid; i < n; i += PV_THREADS) {
        const int ly = i / nx, lx = i - ly * nx, x = x0 + lx, y = y0 + ly;
        const long long q = (long long)y * a.W + x;
        const int D = st_nearness(pred[b * HW + q], a.space);
        const unsigned char* px = image + b * 3 * HW + q;
        int tx, ty;
        pv_position(x, y, a.W, a.H, D, F, f, a.max_s8, tx, ty);
        s_D[i] = D;
        s_c[i] = st_rgb(px[0], px[HW], px[2 * HW]);
        s_t[i] = pv_pack(tx - 8 * p0, ty - 8 * q0);  // (within -2 max_s8 - 16 .. 248 + 2 max_s8 + 16)
    }
    __syncthreads();

    const int h = pv_cap_half(f.Z);
    for (int i = tid; i < n; i += PV_THREADS) {
        const int ly = i / nx, lx = i - ly * nx;
        const PvVertex v00 = pv_vertex(s_D, s_c, s_t, i);
        {
            const int cx0 = max(0, (v00.tx - h + 7) >> 3), cx1 = min(tw - 1, ((v00.tx + h + 7) >> 3) - 1);
            const int cy0 = max(0, (v00.ty - h + 7) >> 3), cy1 = min(th - 1, ((v00.ty + h + 7) >> 3) - 1);
            const pv_u64 key = pv_key(v00.D, 3u * (unsigned)i, v00.c);
            for (int y = cy0; y <= cy1; ++y)
                for (int x = cx0; x <= cx1; ++x) atomicMax(&s_z[y * PV_TILE + x], key);
        }
        if (lx + 1 < nx && ly + 1 < ny) {
            const PvVertex v01 = pv_vertex(s_D, s_c, s_t, i + 1), v10 = pv_vertex(s_D, s_c, s_t, i + nx), v11 = pv_vertex(s_D, s_c, s_t, i + nx + 1);
            if (pv_triangle_exists(v00.D, v01.D, v10.D, a.edge)) pv_raster(s_z, v00, v01, v10, 3u * (unsigned)i + 1u, tw, th);
            if (pv_triangle_exists(v01.D, v11.D, v10.D, a.edge)) pv_raster(s_z, v01, v11, v10, 3u * (unsigned)i + 2u, tw, th);
        }
    }
    __syncthreads();

    const long long frame = (b * a.V + k) * HW;
    for (int i = tid; i < PV_TILE * PV_TILE; i += PV_THREADS) {
        const int y = i / PV_TILE, x = i - y * PV_TILE;
        if (x >= tw || y >= th) continue;
        const pv_u64 key = s_z[i];
        const long long q = (long long)(q0 + y) * a.W + p0 + x;
        plane[frame + q] = key ? ((unsigned)pv_key_near(key) | PV_COVERED) : 0u;
        if (key) {
            const unsigned rgb = pv_key_rgb(key);
            unsigned char* o = out + 3 * frame + q;
            o[0] = (unsigned char)(rgb & 255u);
            o[HW] = (unsigned char)((rgb >> 8) & 255u);
            o[2 * HW] = (unsigned char)((rgb >> 16) & 255u);
        }
    }
}

// grid (ceil(B V H W / 256)).  plane: [B][V][H][W]; out: [B][V][3][H][W]; holes, near: [B][V][H][W] or NULL.
__global__ __launch_bounds__(PV_THREADS) void pv_fill_kernel(const unsigned* __restrict__ plane, PvCall a, long long total, unsigned char* out,
                                                            unsigned char* __restrict__ holes, unsigned short* __restrict__ near) {
    const long long i = (long long)blockIdx.x * PV_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long HW = (long long)a.H * a.W, bv = i / HW;
    const int rem = (int)(i - bv * HW), y = rem / a.W, x = rem - y * a.W;
    const unsigned me = plane[i];
    int value = (int)(me & 0xffffu);
    const bool hole = !(me & PV_COVERED);
    if (hole) {
        const unsigned* pl = plane + bv * HW;
        const int R = pv_fill_reach(a.max_s8);
        // left, right, up, down: the step in x and y, and how far the image goes that way
        const int sx[4] = {-1, 1, 0, 0}, sy[4] = {0, 0, -1, 1}, room[4] = {x, a.W - 1 - x, y, a.H - 1 - y};
        bool has[4];
        int val[4], at[4];
        for (int k = 0; k < 4; ++k) {
            has[k] = false;
            val[k] = 0;
            at[k] = 0;
            const int far = room[k] < R ? room[k] : R;
            for (int d = 1; d <= far; ++d) {
                const int q = (y + d * sy[k]) * a.W + x + d * sx[k];
                const unsigned w = pl[q];
                if (w & PV_COVERED) {
                    has[k] = true;
                    val[k] = (int)(w & 0xffffu);
                    at[k] = q;
                    break;
                }
            }
        }
        const int pick = pv_fill_pick(has, val);
        unsigned char* o = out + 3 * bv * HW;
        value = pick < 0 ? 0 : val[pick];
        for (int ch = 0; ch < 3; ++ch) o[ch * HW + rem] = pick < 0 ? (unsigned char)0 : o[ch * HW + at[pick]];  // (a covered pixel: the warp pass wrote it)
    }
    if (holes) holes[i] = hole ? 1 : 0;
    if (near) near[i] = (unsigned short)value;
}

}  // namespace

extern "C" {

long long gp_parallax_frames_workspace(int B, int V, int H, int W) {
    if (!pv_dims_ok(B, V, H, W)) return 0;
    return (4LL * B * V * H * W + 7) / 8 * 8;  // the plane between the two passes, one word per output pixel
}

gp_status gp_parallax_frames(const unsigned char* image, const float* pred, const int* focus, const int* frames, int B, int V, int H, int W,
                             int space, int edge, int max_s8, unsigned char* out, unsigned char* holes, unsigned short* near, void* workspace,
                             long long workspace_bytes, void* stream) {
    if (!image || !pred || !focus || !frames || !out || !workspace) return GP_ERR_INVALID;
    if (!pv_dims_ok(B, V, H, W) || !pv_options_ok(space, edge, max_s8)) return GP_ERR_INVALID;
    PvFrames table;
    for (int k = 0; k < V; ++k) {
        if (!pv_frame_ok(frames + 4 * k)) return GP_ERR_INVALID;
        for (int f = 0; f < 4; ++f) table.v[k][f] = frames[4 * k + f];
    }
    for (int k = V; k < PV_MAX_FRAMES; ++k)
        for (int f = 0; f < 4; ++f) table.v[k][f] = 0;
    if ((((uintptr_t)pred | (uintptr_t)focus) & 3) != 0 || ((uintptr_t)near & 1) != 0 || ((uintptr_t)workspace & 7) != 0) return GP_ERR_INVALID;
    if (workspace_bytes < gp_parallax_frames_workspace(B, V, H, W)) return GP_ERR_INVALID;
    if (out == image) return GP_ERR_INVALID;  // a frame would overwrite the sources of the next
    const int tiles_x = (W + PV_TILE - 1) / PV_TILE, tiles_y = (H + PV_TILE - 1) / PV_TILE;  // tiles_x * tiles_y <= 512 * 512
    const PvCall a = {H, W, V, space, edge, max_s8, tiles_x, pv_staged_side(max_s8)};
    static unsigned long long attr_mask = 0;
    gp_once_per_device(&attr_mask, [&] {
        (void)hipFuncSetAttribute((const void*)pv_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, pv_lds_bytes(pv_staged_side(PV_MAX_S8)));
    });
    unsigned* plane = (unsigned*)workspace;
    const long long total = (long long)B * V * H * W;
    hipLaunchKernelGGL(pv_warp_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, V, B), dim3(PV_THREADS), (size_t)pv_lds_bytes(a.side), (hipStream_t)stream,
                       image, pred, focus, table, a, out, plane);
    hipLaunchKernelGGL(pv_fill_kernel, dim3((unsigned)((total + PV_THREADS - 1) / PV_THREADS)), dim3(PV_THREADS), 0, (hipStream_t)stream,
                       (const unsigned*)plane, a, total, out, holes, near);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
