// The merge of tiled high-resolution inference on the device (gp_tile_merge): every tile's prediction is fitted onto its window of the base map
// by least squares (scale and shift) and the fitted tiles are blended with integer weights that fall off towards their borders.  The
// definition is stated in include/genpercept_hip.h; genpercept_amd/tiled.py restates it on the host and gives the same bits; the grid rule,
// the per-tile solve and the per-pixel steps are tile_merge_math.h, which tests/tile_check.cpp also runs on the CPU.
//   fit      workgroups over (slab, tile, image).  A slab is a run of the C * wh rows of a tile; its four waves take rows in turn, a wave's lanes
//            consecutive columns, so the tile (contiguous) and the base window (rows W apart) are read in 256-byte pieces.  Values are quantised
//            on reading; five 64-bit integer sums (n, P, G, P P, P G; the products fit 32 bits) go through block_sum into the slab of the
//            workgroup.  Integer sums: the order is immaterial and the result exact.  Skipped for the alignment `none`.
//   solve    one thread per (image, tile) adds the tile's slabs and runs tm_solve in float64; (s, t) goes to the workspace and, if asked for,
//            to fit_out.  `none` writes (1, 0).
//   blend    one workgroup of 256 threads per 256 columns x 4 rows of the output, a thread one column of it.  The origin tables (made from the grid rule, 4 (ny + nx)
//            bytes) and the image's (s, t) table (16 N bytes) are staged in LDS: at most 24 KiB, usually under 2 KiB.  The origins increase
//            strictly, so the tiles that cover a row or a column are a run of the table, found by two binary searches: per thread once for
//            its column and once for its four rows together.  A thread walks the covering tiles in ascending iy, then ix, and takes its four
//            rows side by side: the four (twelve for C = 3) loads of a tile are issued before their arithmetic, so that enough bytes are in
//            flight per thread (with one load at a time the pass is bound by the latency of its loads, not by bandwidth).  A row that a tile does not cover skips it, which leaves
//            every pixel its own tiles in their order.  Neighbouring threads read neighbouring floats of the same tile row, and read the same
//            (s, t) from LDS (a broadcast) except across a tile border.
// Three launches for any batch (two for `none`), stream-ordered, no atomics, nothing read back.  Which thread computes which pixel depends on
// the sizes only and the only sums that cross threads are integers, so an image's result is the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"
#include "tile_merge_math.h"

namespace {

constexpr int TM_ROWS = 4;  // output rows per blend workgroup: every thread takes one column of them, the rows side by side
constexpr int TM_NSUM = 5;  // n, sum P, sum G, sum P P, sum P G

struct TmGrid {
    int H, W, wh, ww, ny, nx, o;
};

// slabs per tile: at least 4096 values each, at most 512, and no more than there are rows
inline int tm_slabs(int C, int wh, int ww) {
    const int g = eval_blocks((long long)C * wh * ww);
    return g < C * wh ? g : C * wh;
}

// grid (ns, N, B).  slabs: [B][N][ns][TM_NSUM].
__global__ __launch_bounds__(EV_THREADS) void tm_fit_kernel(const float* __restrict__ base, const float* __restrict__ tiles, TmGrid g, int C,
                                                           u64* __restrict__ slabs) {
    const int tile = blockIdx.y, ns = gridDim.x, rows = C * g.wh;
    const long long bt = (long long)blockIdx.z * gridDim.y + tile;
    const int y0 = tm_origin(tile / g.nx, g.H, g.wh, g.ny), x0 = tm_origin(tile % g.nx, g.W, g.ww, g.nx);
    const int r0 = (int)((long long)blockIdx.x * rows / ns), r1 = (int)((long long)(blockIdx.x + 1) * rows / ns);
    const float* tp = tiles + bt * rows * g.ww;
    const float* bp = base + (long long)blockIdx.z * C * g.H * g.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 v[TM_NSUM] = {0, 0, 0, 0, 0};
    for (int r = r0 + wave; r < r1; r += EV_WAVES) {
        const int c = r / g.wh, y = r - c * g.wh;
        const float* trow = tp + (long long)r * g.ww;
        const float* brow = bp + ((long long)c * g.H + (y0 + y)) * g.W + x0;
#pragma unroll 4
        for (int x = lane; x < g.ww; x += 64) {
            const unsigned P = gs_quant16(trow[x]), G = gs_quant16(brow[x]);
            v[0] += 1, v[1] += P, v[2] += G, v[3] += P * P, v[4] += P * G;  // (65535^2 < 2^32)
        }
    }
    const u64 a = block_sum(v);
    if (threadIdx.x < TM_NSUM) slabs[(bt * ns + blockIdx.x) * TM_NSUM + threadIdx.x] = a;
}

// one thread per (image, tile).  st: [B][N][2] = s, t.
__global__ __launch_bounds__(EV_THREADS) void tm_solve_kernel(const u64* __restrict__ slabs, int total, int ns, int align, double* __restrict__ st,
                                                             double* __restrict__ fit_out) {
    const int i = blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= total) return;
    double s = 1.0, t = 0.0;
    if (align == TM_ALIGN_LEAST_SQUARE) {
        u64 a[TM_NSUM] = {0, 0, 0, 0, 0};
        const u64* sl = slabs + (long long)i * ns * TM_NSUM;
        for (int j = 0; j < ns; ++j) {
#pragma unroll
            for (int k = 0; k < TM_NSUM; ++k) a[k] += sl[j * TM_NSUM + k];
        }
        tm_solve(a[0], a[1], a[2], a[3], a[4], s, t);
    }
    st[2 * i] = s, st[2 * i + 1] = t;
    if (fit_out) fit_out[2 * i] = s, fit_out[2 * i + 1] = t;
}

// the first k of 0 .. n with tab[k] > v (n if none); tab increases
__device__ __forceinline__ int tm_first_above(const int* tab, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// grid (ceil(W / 256), ceil(H / TM_ROWS), B).  Dynamic LDS: 16 N + 4 (ny + nx) bytes.
template <int C>
__global__ __launch_bounds__(EV_THREADS) void tm_blend_kernel(const float* __restrict__ tiles, const double* __restrict__ st, TmGrid g, float* __restrict__ out) {
    extern __shared__ double s_tm[];
    const int N = g.ny * g.nx;
    const long long b = blockIdx.z;
    double* s_st = s_tm;                                  // [N][2]
    int* s_ys = reinterpret_cast<int*>(s_tm + 2 * N);     // [ny]
    int* s_xs = s_ys + g.ny;                              // [nx]
    for (int i = threadIdx.x; i < 2 * N; i += EV_THREADS) s_st[i] = st[b * 2 * N + i];
    for (int i = threadIdx.x; i < g.ny; i += EV_THREADS) s_ys[i] = tm_origin(i, g.H, g.wh, g.ny);
    for (int i = threadIdx.x; i < g.nx; i += EV_THREADS) s_xs[i] = tm_origin(i, g.W, g.ww, g.nx);
    __syncthreads();
    const int x = blockIdx.x * EV_THREADS + threadIdx.x;
    if (x >= g.W) return;
    // tile column ix covers x when xs[ix] <= x < xs[ix] + ww: a run of the table, never empty; rows likewise, for the TM_ROWS rows together
    const int ix0 = tm_first_above(s_xs, g.nx, x - g.ww), ix1 = tm_first_above(s_xs, g.nx, x) - 1;
    const int ya = blockIdx.y * TM_ROWS, yb = ya + TM_ROWS < g.H ? ya + TM_ROWS : g.H;
    const int iy0 = tm_first_above(s_ys, g.ny, ya - g.wh), iy1 = tm_first_above(s_ys, g.ny, yb - 1) - 1;
    const long long tsz = (long long)g.wh * g.ww;
    double acc[TM_ROWS][C];
    long long wsum[TM_ROWS];
#pragma unroll
    for (int r = 0; r < TM_ROWS; ++r) {
        wsum[r] = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[r][c] = 0.0;
    }
    for (int iy = iy0; iy <= iy1; ++iy) {
        const int y0 = s_ys[iy];
        for (int ix = ix0; ix <= ix1; ++ix) {
            const int x0 = s_xs[ix], wx = tm_weight(x, x0, g.ww, g.o), k = iy * g.nx + ix;
            const double s = s_st[2 * k], t = s_st[2 * k + 1];
            const float* p = tiles + (b * N + k) * C * tsz + (x - x0);
            // the loads of the rows first, then their arithmetic: TM_ROWS * C values in flight per thread
            float v[TM_ROWS][C];
            bool in[TM_ROWS];
#pragma unroll
            for (int r = 0; r < TM_ROWS; ++r) {
                const int y = ya + r;
                in[r] = y < yb && y >= y0 && y < y0 + g.wh;
#pragma unroll
                for (int c = 0; c < C; ++c) v[r][c] = in[r] ? p[c * tsz + (long long)(y - y0) * g.ww] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < TM_ROWS; ++r) {
                if (in[r]) {
                    const int wgt = tm_weight(ya + r, y0, g.wh, g.o) * wx;
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[r][c] = tm_accumulate(acc[r][c], wgt, s, t, v[r][c]);
                    wsum[r] += wgt;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TM_ROWS; ++r)
        if (ya + r < yb) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[((b * C + c) * g.H + (ya + r)) * g.W + x] = tm_finish(acc[r][c], wsum[r]);
        }
}

inline bool tm_dims_ok(int B, int C, int H, int W, int ny, int nx, int wh, int ww) {
    return B >= 1 && B <= 65535 && (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= TM_MAX_DIM && W <= TM_MAX_DIM && wh >= 1 && ww >= 1 && wh <= H && ww <= W &&
           ny >= 1 && nx >= 1 && ny <= TM_MAX_TILES && nx <= TM_MAX_TILES && ny * nx <= TM_MAX_TILES;
}

// the (s, t) table [B][N][2] of doubles, then the slabs [B][N][ns][TM_NSUM] of 64-bit sums
inline long long tm_workspace_bytes(int B, int C, int ny, int nx, int wh, int ww) {
    return (long long)B * ny * nx * (2 + (long long)tm_slabs(C, wh, ww) * TM_NSUM) * 8;
}

}  // namespace

extern "C" {

long long gp_tile_merge_workspace(int B, int C, int H, int W, int ny, int nx, int wh, int ww) {
    return tm_dims_ok(B, C, H, W, ny, nx, wh, ww) ? tm_workspace_bytes(B, C, ny, nx, wh, ww) : 0;
}

gp_status gp_tile_merge(const float* base, const float* tiles, int B, int C, int H, int W, const int* ys, int ny, const int* xs, int nx, int wh, int ww,
                        int overlap, int align, double* fit_out, float* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!base || !tiles || !ys || !xs || !out || !workspace) return GP_ERR_INVALID;
    if (!tm_dims_ok(B, C, H, W, ny, nx, wh, ww) || !tm_axis_ok(H, wh, overlap) || !tm_axis_ok(W, ww, overlap)) return GP_ERR_INVALID;
    if (align != TM_ALIGN_LEAST_SQUARE && align != TM_ALIGN_NONE) return GP_ERR_INVALID;
    // the grid is the rule's: the kernels make the origins from it, ys and xs (host memory) only have to agree
    if (ny != tm_count(H, wh, overlap) || nx != tm_count(W, ww, overlap)) return GP_ERR_INVALID;
    for (int k = 0; k < ny; ++k)
        if (ys[k] != tm_origin(k, H, wh, ny)) return GP_ERR_INVALID;
    for (int k = 0; k < nx; ++k)
        if (xs[k] != tm_origin(k, W, ww, nx)) return GP_ERR_INVALID;
    if ((((uintptr_t)base | (uintptr_t)tiles | (uintptr_t)out) & 3) != 0 || !eval_aligned8(fit_out, (const char*)workspace)) return GP_ERR_INVALID;
    if (workspace_bytes < tm_workspace_bytes(B, C, ny, nx, wh, ww)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int N = ny * nx, ns = tm_slabs(C, wh, ww);
    const TmGrid g = {H, W, wh, ww, ny, nx, overlap};
    double* st = (double*)workspace;
    u64* slabs = (u64*)(st + (long long)B * N * 2);
    if (align == TM_ALIGN_LEAST_SQUARE) hipLaunchKernelGGL(tm_fit_kernel, dim3(ns, N, B), dim3(EV_THREADS), 0, s, base, tiles, g, C, slabs);
    hipLaunchKernelGGL(tm_solve_kernel, dim3((B * N + EV_THREADS - 1) / EV_THREADS), dim3(EV_THREADS), 0, s, (const u64*)slabs, B * N, ns, align, st, fit_out);
    const auto blend = C == 1 ? tm_blend_kernel<1> : tm_blend_kernel<3>;
    hipLaunchKernelGGL(blend, dim3((W + EV_THREADS - 1) / EV_THREADS, (H + TM_ROWS - 1) / TM_ROWS, B), dim3(EV_THREADS), (size_t)16 * N + 4 * (size_t)(ny + nx), s,
                       tiles, (const double*)st, g, out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
