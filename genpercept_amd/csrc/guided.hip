// Edge-aware upsampling of a prediction on the device (gp_guided_upsample): the guided filter of He, Sun and Tang in its fast form, the image as
// guide.  A local linear model q = a . I + b is fitted at the processing size, a and b are smoothed there, upsampled and applied to the
// full-resolution image.  The definition is stated in include/genpercept_hip.h; genpercept_amd/guided.py restates it on the host and gives the
// same bits; the per-pixel arithmetic is guided_solve.h, which tests/guided_check.cpp also runs on the CPU.
//   model    one workgroup of 256 threads per 32 x 16 tile, two pixels per thread.  The tile and an apron of r pixels, cut at the image border,
//            are staged in LDS once: the three image bytes and the C predictions as 16-bit values (5 or 9 bytes per pixel).  The 9 + 4 C window
//            sums are box sums, so they are separable: a pass of row sums over the tile's columns and the region's rows (32-bit: at most
//            65 * 255 * 65535 < 2^31) into LDS, then each pixel adds its column of them in 64 bits in registers.  The sums go through in groups
//            of three or four (I; II 00 01 02; II 11 12 22; then p, I0 p, I1 p, I2 p of each channel), so only four row-sum planes are live:
//            LDS = 16 * 32 * (16 + 2 r) + (3 + 2 C)(32 + 2 r)(16 + 2 r) bytes, 17 KiB at r = 4 (no limit on occupancy: the eight workgroups
//            that the wave slots of a CU admit fit) and 78 / 108 KiB for C = 1 / 3 at r = 32 (two / one workgroups per CU: the region is
//            fifteen times the tile there, the cap of r is a cap of the cost too).  All thirteen planes at once would need 130 KiB at r = 32
//            on top of the staging, more than the 160 KiB of a CU.  The solve runs per pixel and channel in float64 and writes four planes
//            (a0, a1, a2, b) per channel.
//   smooth   a row launch and a column launch.  One launch would stage (32 + 2 r)^2 doubles per plane and tile, 72 KiB at r = 32, and read
//            every value (1 + 2 r / 32)^2 times from L2; the two launches stage 2.5 KiB and at most 48 KiB and read every value 1 + 2 r / 256
//            and 1 + 2 r / 32 times.  Rows: 256 pixels of a row and r either side in LDS, each thread adds its 2 r + 1 values left to right.
//            Columns: a 64 x 32 tile and r rows either side, each thread adds top to bottom and divides by the window's pixel count.
//            Values outside the image are staged as +0.0: a sum that starts at +0.0 never holds -0.0, so adding +0.0 changes nothing and the
//            sum is that of the clipped window in its order.
//   apply    one thread per output pixel, 256 consecutive pixels of a row per workgroup: three coalesced byte loads of the guide, the sixteen
//            float64 taps per channel from the smoothed planes (neighbouring pixels share them: they come from L2 / L1), one float store.
// Four launches for any batch, stream-ordered, no atomics, nothing read back.  Which thread computes which pixel depends on the sizes and r only
// and no sum crosses a thread, so an image's result is the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "kernels.h"
#include "guided_solve.h"

namespace {

typedef unsigned long long u64;

constexpr int GD_THREADS = 256;
constexpr int GD_TW = 32, GD_TH = 16;  // the tile of a model workgroup: two pixels per thread, rows t / 32 and t / 32 + 8
constexpr int GD_NQ = 4;               // row-sum planes live at once
constexpr int GD_CW = 64, GD_CH = 32;  // the tile of a column-smoothing workgroup
static_assert(GD_THREADS == GD_TW * GD_TH / 2 && GD_THREADS % GD_CW == 0, "pixel-to-thread assignment");

inline size_t gd_model_lds(int C, int r) {
    return (size_t)GD_NQ * GD_TW * (GD_TH + 2 * r) * 4 + (size_t)(3 + 2 * C) * (GD_TW + 2 * r) * (GD_TH + 2 * r);
}
constexpr int GD_MODEL_LDS_MAX = GD_NQ * GD_TW * (GD_TH + 2 * GS_MAX_R) * 4 + 9 * (GD_TW + 2 * GS_MAX_R) * (GD_TH + 2 * GS_MAX_R);
static_assert(GD_MODEL_LDS_MAX <= 160 * 1024, "the model pass has to fit the LDS of a CU");

// the tile of a model workgroup and its staged region inside an h x w image
struct GdTile {
    int h, w, r;
    int tx0, ty0, tx1, ty1;  // the tile, cut at the image
    int rx0, ry0, rw, rh;    // the tile and r rings, cut at the image
};

// NQ box sums of every pixel of the tile: f(i, v) gives the NQ values of the staged pixel i = ly * rw + lx.  out[k][q]: sum q of the thread's
// pixel k (row t / 32 + 8 k, column t % 32 of the tile); untouched where that pixel lies outside the tile.  Two barriers; s_row may be reused
// after it.
template <int NQ, typename F>
__device__ __forceinline__ void gd_box(const GdTile& g, unsigned* s_row, F f, u64 (&out)[2][NQ]) {
    static_assert(NQ <= GD_NQ, "row-sum planes");
    const int plane = GD_TW * (GD_TH + 2 * g.r);
    for (int e = threadIdx.x; e < GD_TW * g.rh; e += GD_THREADS) {
        const int ly = e / GD_TW, x = g.tx0 + e % GD_TW;
        if (x < g.tx1) {
            const int l0 = (x - g.r > 0 ? x - g.r : 0) - g.rx0, l1 = (x + g.r < g.w - 1 ? x + g.r : g.w - 1) - g.rx0;
            unsigned acc[NQ], v[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0;
            for (int lx = l0; lx <= l1; ++lx) {
                f(ly * g.rw + lx, v);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += v[q];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) s_row[q * plane + e] = acc[q];
        }
    }
    __syncthreads();
    const int x = g.tx0 + (threadIdx.x & (GD_TW - 1));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int y = g.ty0 + (threadIdx.x >> 5) + 8 * k;
        if (x < g.tx1 && y < g.ty1) {
            const int l0 = (y - g.r > 0 ? y - g.r : 0) - g.ry0, l1 = (y + g.r < g.h - 1 ? y + g.r : g.h - 1) - g.ry0;
            u64 acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0;
            for (int ly = l0; ly <= l1; ++ly) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += s_row[q * plane + ly * GD_TW + (threadIdx.x & (GD_TW - 1))];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) out[k][q] = acc[q];
        }
    }
    __syncthreads();
}

// grid (ntx * nty, 1, B): blockIdx.x = tile row * ntx + tile column.  ab: planes [B][C][4][h * w] = a0, a1, a2, b.  Dynamic LDS: gd_model_lds.
template <int C>
__global__ __launch_bounds__(GD_THREADS) void gd_model_kernel(const unsigned char* __restrict__ guide_lo, const float* __restrict__ pred, int h, int w, int r,
                                                              double e, int ntx, double* __restrict__ ab) {
    extern __shared__ unsigned s_gd[];
    const int pitch = (GD_TW + 2 * r) * (GD_TH + 2 * r);
    unsigned* s_row = s_gd;                                                                      // [GD_NQ][GD_TW * (GD_TH + 2 r)]
    unsigned short* s_p = reinterpret_cast<unsigned short*>(s_row + GD_NQ * GD_TW * (GD_TH + 2 * r));  // [C][pitch]
    unsigned char* s_i = reinterpret_cast<unsigned char*>(s_p + C * pitch);                      // [3][pitch]
    const long long b = blockIdx.z, hw = (long long)h * w;
    GdTile g;
    g.h = h, g.w = w, g.r = r;
    g.tx0 = (blockIdx.x % ntx) * GD_TW, g.ty0 = (blockIdx.x / ntx) * GD_TH;
    g.tx1 = g.tx0 + GD_TW < w ? g.tx0 + GD_TW : w, g.ty1 = g.ty0 + GD_TH < h ? g.ty0 + GD_TH : h;
    g.rx0 = g.tx0 - r > 0 ? g.tx0 - r : 0, g.ry0 = g.ty0 - r > 0 ? g.ty0 - r : 0;
    g.rw = (g.tx1 + r < w ? g.tx1 + r : w) - g.rx0, g.rh = (g.ty1 + r < h ? g.ty1 + r : h) - g.ry0;  // rw * rh <= pitch
    const unsigned char* img = guide_lo + b * 3 * hw;
    const float* prd = pred + b * C * hw;
    for (int i = threadIdx.x; i < g.rw * g.rh; i += GD_THREADS) {
        const int ly = i / g.rw, lx = i - ly * g.rw;
        const long long sp = (long long)(g.ry0 + ly) * w + (g.rx0 + lx);
#pragma unroll
        for (int c = 0; c < 3; ++c) s_i[c * pitch + i] = img[c * hw + sp];
#pragma unroll
        for (int c = 0; c < C; ++c) s_p[c * pitch + i] = (unsigned short)gs_quant16(prd[c * hw + sp]);
    }
    __syncthreads();
    u64 sI[2][3], sA[2][3], sB[2][3];  // sums of I, of I0 I0, I0 I1, I0 I2 and of I1 I1, I1 I2, I2 I2
    gd_box<3>(g, s_row, [&](int i, unsigned (&v)[3]) { v[0] = s_i[i], v[1] = s_i[pitch + i], v[2] = s_i[2 * pitch + i]; }, sI);
    gd_box<3>(g, s_row, [&](int i, unsigned (&v)[3]) {
        const unsigned i0 = s_i[i], i1 = s_i[pitch + i], i2 = s_i[2 * pitch + i];
        v[0] = i0 * i0, v[1] = i0 * i1, v[2] = i0 * i2;
    }, sA);
    gd_box<3>(g, s_row, [&](int i, unsigned (&v)[3]) {
        const unsigned i1 = s_i[pitch + i], i2 = s_i[2 * pitch + i];
        v[0] = i1 * i1, v[1] = i1 * i2, v[2] = i2 * i2;
    }, sB);
    const int x = g.tx0 + (threadIdx.x & (GD_TW - 1));
    for (int c = 0; c < C; ++c) {
        u64 sP[2][4];  // sums of p, I0 p, I1 p, I2 p
        const unsigned short* pc = s_p + c * pitch;
        gd_box<4>(g, s_row, [&](int i, unsigned (&v)[4]) {
            const unsigned p = pc[i];
            v[0] = p, v[1] = s_i[i] * p, v[2] = s_i[pitch + i] * p, v[3] = s_i[2 * pitch + i] * p;
        }, sP);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int y = g.ty0 + (threadIdx.x >> 5) + 8 * k;
            if (x < g.tx1 && y < g.ty1) {
                const int nx = (x + r < w - 1 ? x + r : w - 1) - (x - r > 0 ? x - r : 0) + 1;
                const int ny = (y + r < h - 1 ? y + r : h - 1) - (y - r > 0 ? y - r : 0) + 1;
                const u64 vI[3] = {sI[k][0], sI[k][1], sI[k][2]};
                const u64 vII[6] = {sA[k][0], sA[k][1], sA[k][2], sB[k][0], sB[k][1], sB[k][2]};
                const u64 vIp[3] = {sP[k][1], sP[k][2], sP[k][3]};
                double a[3], bb;
                gs_solve((unsigned)(nx * ny), vI, vII, sP[k][0], vIp, e, a, bb);
                double* o = ab + (b * C + c) * 4 * hw + (long long)y * w + x;
                o[0] = a[0], o[hw] = a[1], o[2 * hw] = a[2], o[3 * hw] = bb;
            }
        }
    }
}

// grid (nseg * h, planes, B): blockIdx.x = row * nseg + segment of 256 pixels.  dst = the sums over x - r .. x + r, clipped, left to right.
__global__ __launch_bounds__(GD_THREADS) void gd_smooth_rows_kernel(const double* __restrict__ src, double* __restrict__ dst, int h, int w, int r, int nseg) {
    __shared__ double s_v[GD_THREADS + 2 * GS_MAX_R];
    const long long hw = (long long)h * w, row = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * hw + (long long)(blockIdx.x / nseg) * w;
    const int x0 = (blockIdx.x % nseg) * GD_THREADS;
    for (int i = threadIdx.x; i < GD_THREADS + 2 * r; i += GD_THREADS) {
        const int x = x0 - r + i;
        s_v[i] = x >= 0 && x < w ? src[row + x] : 0.0;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x < w) {
        double acc = 0.0;
        for (int d = 0; d <= 2 * r; ++d) acc = acc + s_v[threadIdx.x + d];
        dst[row + x] = acc;
    }
}

// grid (ntx * nty, planes, B).  dst = (the sums of the row sums over y - r .. y + r, clipped, top to bottom) / N.  Dynamic LDS:
// (GD_CH + 2 r) * GD_CW doubles.
__global__ __launch_bounds__(GD_THREADS) void gd_smooth_cols_kernel(const double* __restrict__ src, double* __restrict__ dst, int h, int w, int r, int ntx) {
    extern __shared__ double s_c[];
    const long long hw = (long long)h * w, plane = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * hw;
    const int tx = threadIdx.x & (GD_CW - 1), tq = threadIdx.x / GD_CW;
    const int x = (blockIdx.x % ntx) * GD_CW + tx, ty0 = (blockIdx.x / ntx) * GD_CH;
    for (int ly = tq; ly < GD_CH + 2 * r; ly += GD_THREADS / GD_CW) {
        const int y = ty0 - r + ly;
        s_c[ly * GD_CW + tx] = x < w && y >= 0 && y < h ? src[plane + (long long)y * w + x] : 0.0;
    }
    __syncthreads();
    if (x >= w) return;
    const int nx = (x + r < w - 1 ? x + r : w - 1) - (x - r > 0 ? x - r : 0) + 1;
    for (int ly = tq; ly < GD_CH; ly += GD_THREADS / GD_CW) {
        const int y = ty0 + ly;
        if (y >= h) break;
        const int ny = (y + r < h - 1 ? y + r : h - 1) - (y - r > 0 ? y - r : 0) + 1;
        double acc = 0.0;
        for (int d = 0; d <= 2 * r; ++d) acc = acc + s_c[(ly + d) * GD_CW + tx];
        dst[plane + (long long)y * w + x] = acc / (double)(nx * ny);
    }
}

// grid (ceil(W / 256), H, B).  ab: the smoothed planes [B][C][4][h * w].
template <int C>
__global__ __launch_bounds__(GD_THREADS) void gd_apply_kernel(const double* __restrict__ ab, const unsigned char* __restrict__ guide, int h, int w, int H, int W,
                                                              float* __restrict__ out) {
    const int X = blockIdx.x * GD_THREADS + threadIdx.x, Y = blockIdx.y;
    if (X >= W) return;
    const long long b = blockIdx.z, hw = (long long)h * w, HW = (long long)H * W, P = (long long)Y * W + X;
    int i0, i1, j0, j1;
    double fy, fx;
    gs_index(Y, h, H, i0, i1, fy);
    gs_index(X, w, W, j0, j1, fx);
    const unsigned char* gp = guide + b * 3 * HW + P;
    const unsigned char gv[3] = {gp[0], gp[HW], gp[2 * HW]};
    const long long t00 = (long long)i0 * w + j0, t01 = (long long)i0 * w + j1, t10 = (long long)i1 * w + j0, t11 = (long long)i1 * w + j1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double* p = ab + (b * C + c) * 4 * hw;
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gs_blend(p[k * hw + t00], p[k * hw + t01], p[k * hw + t10], p[k * hw + t11], fx, fy);
        const double A[3] = {v[0], v[1], v[2]};
        out[(b * C + c) * HW + P] = gs_apply(A, v[3], gv);
    }
}

inline bool gd_dims_ok(int B, int C, int h, int w) {
    return B >= 1 && B <= 65535 && (C == 1 || C == 3) && h >= 1 && w >= 1 && h <= GS_MAX_DIM && w <= GS_MAX_DIM;
}

// two buffers of the planes [B][C][4][h * w] of doubles: the model and the smoothed model; the row sums
inline long long gd_workspace_bytes(int B, int C, int h, int w) { return 2LL * B * C * 4 * ((long long)h * w) * 8; }

}  // namespace

extern "C" {

long long gp_guided_upsample_workspace(int B, int C, int h, int w) { return gd_dims_ok(B, C, h, w) ? gd_workspace_bytes(B, C, h, w) : 0; }

gp_status gp_guided_upsample(const unsigned char* guide_lo, const float* pred, int C, const unsigned char* guide, int B, int h, int w, int H, int W, int r,
                             double eps, float* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!guide_lo || !pred || !guide || !out || !workspace) return GP_ERR_INVALID;
    if (!gd_dims_ok(B, C, h, w) || H < 1 || W < 1 || H > GS_MAX_DIM || W > GS_MAX_DIM) return GP_ERR_INVALID;
    if (r < 1 || r > GS_MAX_R || !(eps > 0.0 && eps <= 1.0)) return GP_ERR_INVALID;  // (NaN fails)
    if ((((uintptr_t)pred | (uintptr_t)out) & 3) != 0 || ((uintptr_t)workspace & 7) != 0) return GP_ERR_INVALID;
    if (workspace_bytes < gd_workspace_bytes(B, C, h, w)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    double* ab = (double*)workspace;
    double* rows = ab + (long long)B * C * 4 * ((long long)h * w);
    const int ntx = (w + GD_TW - 1) / GD_TW, nty = (h + GD_TH - 1) / GD_TH;  // ntx * nty <= 512 * 1024
    const auto model = C == 1 ? gd_model_kernel<1> : gd_model_kernel<3>;
    static unsigned long long attr_mask = 0;
    gp_once_per_device(&attr_mask, [&] {
        (void)hipFuncSetAttribute((const void*)gd_model_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, GD_MODEL_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)gd_model_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, GD_MODEL_LDS_MAX);
    });
    hipLaunchKernelGGL(model, dim3((unsigned)ntx * (unsigned)nty, 1, B), dim3(GD_THREADS), gd_model_lds(C, r), s, guide_lo, pred, h, w, r, eps * 65025.0, ntx,
                       ab);
    const int nseg = (w + GD_THREADS - 1) / GD_THREADS;  // nseg * h <= 64 * 16384
    hipLaunchKernelGGL(gd_smooth_rows_kernel, dim3((unsigned)nseg * (unsigned)h, 4 * C, B), dim3(GD_THREADS), 0, s, (const double*)ab, rows, h, w, r, nseg);
    const int ctx = (w + GD_CW - 1) / GD_CW, cty = (h + GD_CH - 1) / GD_CH;
    hipLaunchKernelGGL(gd_smooth_cols_kernel, dim3((unsigned)ctx * (unsigned)cty, 4 * C, B), dim3(GD_THREADS), (size_t)(GD_CH + 2 * r) * GD_CW * 8, s,
                       (const double*)rows, ab, h, w, r, ctx);
    const auto apply = C == 1 ? gd_apply_kernel<1> : gd_apply_kernel<3>;
    hipLaunchKernelGGL(apply, dim3((W + GD_THREADS - 1) / GD_THREADS, H, B), dim3(GD_THREADS), 0, s, (const double*)ab, guide, h, w, H, W, out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
