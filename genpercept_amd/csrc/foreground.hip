// Matting cutouts on the device (gp_foreground): foreground and background colours F, B of an image under an 8-bit alpha by the multi-level
// method of Germer et al. 2020 (pymatting's estimate_foreground_ml), the RGBA cutout and the composite over a new background.  The definition
// is stated in include/genpercept_hip.h; genpercept_amd/foreground.py restates it on the host and gives the same bits; the per-pixel update
// is foreground_update.h, which tests/foreground_check.cpp also runs on the CPU.
//   coarse   every level up to 32 x 32 in ONE launch, one workgroup of 1024 threads per image, one thread per pixel.  The alpha plane and the
//            two F / B iterates are resident in LDS (13 planes of 1024 floats, 52 KiB); the pixel's own I and a stay in registers.  One barrier
//            per iteration and one per level (the nearest upsample of the level below goes from one iterate buffer into the other).
//   level    every larger level is ONE launch, one workgroup of 256 threads per 32 x 16 tile.  The tile and an apron of n_big pixels, cut at
//            the level's border, are staged in LDS as 16 planes (a, I, two F / B iterates): F and B come from the coarser level's buffer
//            through the index map (no separate upsample pass), I and a from the full-resolution bytes (byte / 255 from a table of the 256
//            quotients and the index maps of the region's rows and columns, both built once per workgroup).  The n_big Jacobi iterations run in
//            LDS on shrinking rings: iteration k = 1 .. n_big is computed on the tile + (n_big - k) rings, which needs iteration k - 1 on one
//            ring more; neighbours are clamped at the true border of the level only, so every value is the one a whole-level pass computes.
//            Only the last iterate of the tile itself leaves the workgroup.  LDS: (32 + 2 n)(16 + 2 n) pixels x 64 bytes, 45 KiB for
//            n_big = 2 (three workgroups per CU), 60 KiB for n_big = 4.
//   outputs  the last level (whichever kernel runs it) writes fg / bg / rgba / comp directly, so the float planes are written only when asked
//            for.  The levels below it go to two buffers in the workspace, used alternately: planes [6][h_l * w_l] per image.
// 1 + (levels above 32 x 32) launches for any batch, stream-ordered, no atomics, nothing read back.  The fused level kernel is bit-equal to
// n_big whole-level passes by construction (Jacobi: a pixel's iterate k depends on iterates k - 1 of its clamped neighbours alone).  The plain
// form (n_big launches per level) was not built; a level launch with n_big = 1, the least one of its launches could cost, measured more than
// half of the fused launch with n_big = 2 at 480 x 640 and at 2048 x 2048, so the fused form ships.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"
#include "foreground_update.h"

namespace {

constexpr int FG_COARSE_THREADS = FG_SMALL * FG_SMALL;  // one thread per pixel of the largest coarse level
constexpr int FG_THREADS = 256;
constexpr int FG_TW = 32, FG_TH = 16;  // the tile of a level workgroup
constexpr int FG_PLANES = 16;          // a, I[3], two iterates of F[3] B[3]
static_assert(FG_THREADS == 256, "the level kernel fills its table of byte / 255 with one thread per byte");

struct FgIn {
    const unsigned char* image;  // [B][3][H][W]
    const void* alpha;           // [B][H][W] bytes or floats
    int H, W, L;
    float reg, gw;
};

struct FgOut {                   // of the last level
    float *fg, *bg;              // [B][3][H][W] or null
    unsigned char* rgba;         // [B][H][W][4] or null
    unsigned char* comp;         // [B][3][H][W] or null
    const unsigned char* new_bg; // [B][3][H][W] or null: new_rgb
    unsigned new_rgb;            // 0xRRGGBB
};

// the result of pixel (y, x) of image b: into the level buffer `lvl` (planes [6][hw] of this image), or, lvl == null, into the outputs
__device__ __forceinline__ void fg_store(float* lvl, long long hw, const FgOut& o, long long b, int H, int W, int y, int x, unsigned a8,
                                         const float (&F)[3], const float (&B)[3]) {
    const long long p = (long long)y * W + x;
    if (lvl) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lvl[c * hw + p] = F[c], lvl[(3 + c) * hw + p] = B[c];
        return;
    }
    const long long HW = (long long)H * W, q = b * 3 * HW + p;
    if (o.fg) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.fg[q + c * HW] = F[c];
    }
    if (o.bg) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.bg[q + c * HW] = B[c];
    }
    if (o.rgba) {
        const unsigned v = (unsigned)fg_byte(F[0]) | (unsigned)fg_byte(F[1]) << 8 | (unsigned)fg_byte(F[2]) << 16 | a8 << 24;
        reinterpret_cast<unsigned*>(o.rgba)[b * HW + p] = v;  // (4-byte aligned: checked by the entry)
    }
    if (o.comp) {
        const float a = fg_unit(a8);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned n8 = o.new_bg ? (unsigned)o.new_bg[q + c * HW] : (o.new_rgb >> (16 - 8 * c)) & 0xffu;
            o.comp[q + c * HW] = fg_byte(fg_composite(a, F[c], fg_unit(n8)));
        }
    }
}

// grid (B).  Levels 0 .. lc; the result of level lc into `lvl` (planes [6][h * w] per image), or, lc == L, into the outputs.
template <bool U8>
__global__ __launch_bounds__(FG_COARSE_THREADS) void fg_coarse_kernel(FgIn in, int lc, int n_small, float* lvl, FgOut out) {
    __shared__ float s_a[FG_COARSE_THREADS];
    __shared__ float s_fb[2][6][FG_COARSE_THREADS];
    const int H = in.H, W = in.W, L = in.L, t = threadIdx.x;
    const long long b = blockIdx.x, HW = (long long)H * W;
    const unsigned char* img = in.image + b * 3 * HW;
    const Pred8<U8> alpha(in.alpha, b * HW);
    int cur = 0, hp = 1, wp = 1;
    float F[3] = {0.f, 0.f, 0.f}, B[3] = {0.f, 0.f, 0.f};
    unsigned a8 = 0;
    int y = 0, x = 0;
    bool on = false;
    for (int l = 0; l <= lc; ++l) {
        const int hl = fg_level_size(H, L, l), wl = fg_level_size(W, L, l);
        on = t < hl * wl;
        y = t / wl, x = t % wl;
        float I[3] = {0.f, 0.f, 0.f}, a = 0.f;
        if (on) {
            const long long sp = (long long)fg_src(y, H, hl) * W + fg_src(x, W, wl);
            a8 = alpha[sp];
            a = fg_unit(a8);
#pragma unroll
            for (int c = 0; c < 3; ++c) I[c] = fg_unit(img[c * HW + sp]);
            if (l == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) F[c] = B[c] = I[c];
            } else {
                const int pp = fg_src(y, hp, hl) * wp + fg_src(x, wp, wl);
#pragma unroll
                for (int c = 0; c < 3; ++c) F[c] = s_fb[cur][c][pp], B[c] = s_fb[cur][3 + c][pp];
            }
            s_a[t] = a;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_fb[cur ^ 1][c][t] = F[c], s_fb[cur ^ 1][3 + c][t] = B[c];
        }
        __syncthreads();
        cur ^= 1;
        const int nb[4] = {y * wl + (x > 0 ? x - 1 : 0), y * wl + (x + 1 < wl ? x + 1 : wl - 1), (y > 0 ? y - 1 : 0) * wl + x,
                           (y + 1 < hl ? y + 1 : hl - 1) * wl + x};
        for (int k = 0; k < n_small; ++k) {
            if (on) {
                float an[4], Fn[4][3], Bn[4][3];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    an[n] = s_a[nb[n]];
#pragma unroll
                    for (int c = 0; c < 3; ++c) Fn[n][c] = s_fb[cur][c][nb[n]], Bn[n][c] = s_fb[cur][3 + c][nb[n]];
                }
                fg_update(a, I, an, Fn, Bn, in.reg, in.gw, F, B);
#pragma unroll
                for (int c = 0; c < 3; ++c) s_fb[cur ^ 1][c][t] = F[c], s_fb[cur ^ 1][3 + c][t] = B[c];
            }
            __syncthreads();
            cur ^= 1;
        }
        hp = hl, wp = wl;
    }
    if (on) fg_store(lvl ? lvl + b * 6 * ((long long)hp * wp) : nullptr, (long long)hp * wp, out, b, hp, wp, y, x, a8, F, B);
}

// floor(i / d) for 0 <= i < 2^16 and a divisor 1 <= d <= 64 given as inv = 1.0f / d: (i + 0.5) / d lies at least 0.5 / d from every integer, far
// more than the rounding of the two float operations, so the truncation is exact.  (Index arithmetic: not part of the definition.)
__device__ __forceinline__ int fg_div_small(int i, float inv) { return (int)(((float)i + 0.5f) * inv); }

// grid (ntx * nty, B): blockIdx.x = tile row * ntx + tile column.  Level l of extent hl x wl from the level below (hp x wp, planes
// [6][hp * wp] per image in `prev`); the result into `lvl` (planes [6][hl * wl] per image) or, l == L, into the outputs.  Dynamic LDS:
// FG_PLANES planes of `pitch` = (FG_TW + 2 n)(FG_TH + 2 n) floats.
template <bool U8>
__global__ __launch_bounds__(FG_THREADS) void fg_level_kernel(FgIn in, int hl, int wl, int hp, int wp, const float* __restrict__ prev, int n, int ntx,
                                                              int pitch, float* lvl, FgOut out) {
    extern __shared__ float s_fg[];
    float* s_a = s_fg;
    float* s_i = s_fg + pitch;       // [3][pitch]
    float* s_fb = s_fg + 4 * pitch;  // [2][6][pitch]
    const int H = in.H, W = in.W;
    const long long b = blockIdx.y, HW = (long long)H * W, hwp = (long long)hp * wp;
    const int tx0 = (blockIdx.x % ntx) * FG_TW, ty0 = (blockIdx.x / ntx) * FG_TH;
    const int tx1 = tx0 + FG_TW < wl ? tx0 + FG_TW : wl, ty1 = ty0 + FG_TH < hl ? ty0 + FG_TH : hl;
    // the staged region: the tile and n rings, cut at the level's border
    const int rx0 = tx0 - n > 0 ? tx0 - n : 0, ry0 = ty0 - n > 0 ? ty0 - n : 0;
    const int rx1 = tx1 + n < wl ? tx1 + n : wl, ry1 = ty1 + n < hl ? ty1 + n : hl;
    const int rw = rx1 - rx0, np = rw * (ry1 - ry0);  // np <= pitch
    const unsigned char* img = in.image + b * 3 * HW;
    const Pred8<U8> alpha(in.alpha, b * HW);
    prev += b * 6 * hwp;
    // once per workgroup instead of once per pixel: byte / 255 for every byte, and the two index maps of the region's rows and columns
    __shared__ float s_unit[256];
    __shared__ int s_sy[FG_TH + 8], s_py[FG_TH + 8], s_sx[FG_TW + 8], s_px[FG_TW + 8];
    s_unit[threadIdx.x] = fg_unit(threadIdx.x);  // (FG_THREADS == 256)
    if ((int)threadIdx.x < ry1 - ry0) {
        const int y = ry0 + threadIdx.x;
        s_sy[threadIdx.x] = fg_src(y, H, hl), s_py[threadIdx.x] = fg_src(y, hp, hl);
    } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < rw) {
        const int x = rx0 + threadIdx.x - 64;
        s_sx[threadIdx.x - 64] = fg_src(x, W, wl), s_px[threadIdx.x - 64] = fg_src(x, wp, wl);
    }
    __syncthreads();
    const float inv_rw = 1.0f / (float)rw;
    for (int i = threadIdx.x; i < np; i += FG_THREADS) {
        const int ly = fg_div_small(i, inv_rw), lx = i - ly * rw;
        const long long sp = (long long)s_sy[ly] * W + s_sx[lx];
        const long long pp = (long long)s_py[ly] * wp + s_px[lx];
        s_a[i] = s_unit[alpha[sp]];
#pragma unroll
        for (int c = 0; c < 3; ++c) s_i[c * pitch + i] = s_unit[img[c * HW + sp]];
#pragma unroll
        for (int c = 0; c < 6; ++c) s_fb[c * pitch + i] = prev[c * hwp + pp];
    }
    __syncthreads();
    int cur = 0;
    for (int k = 1; k <= n; ++k) {
        const int m = n - k;  // rings around the tile that this iteration still computes
        const int ex0 = tx0 - m > 0 ? tx0 - m : 0, ey0 = ty0 - m > 0 ? ty0 - m : 0;
        const int ex1 = tx1 + m < wl ? tx1 + m : wl, ey1 = ty1 + m < hl ? ty1 + m : hl;
        const int ew = ex1 - ex0, ne = ew * (ey1 - ey0);
        const float inv_ew = 1.0f / (float)ew;
        const float* src = s_fb + cur * 6 * pitch;
        float* dst = s_fb + (cur ^ 1) * 6 * pitch;
        for (int j = threadIdx.x; j < ne; j += FG_THREADS) {
            const int ey = fg_div_small(j, inv_ew);
            const int y = ey0 + ey, x = ex0 + (j - ey * ew);
            const int ly = y - ry0, lx = x - rx0, i = ly * rw + lx;
            // neighbours clamped to the LEVEL; inside it they lie in the region of iteration k - 1
            const int nb[4] = {ly * rw + (x > 0 ? lx - 1 : lx), ly * rw + (x + 1 < wl ? lx + 1 : lx), (y > 0 ? ly - 1 : ly) * rw + lx,
                               (y + 1 < hl ? ly + 1 : ly) * rw + lx};
            float an[4], Fn[4][3], Bn[4][3], F[3], B[3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                an[q] = s_a[nb[q]];
#pragma unroll
                for (int c = 0; c < 3; ++c) Fn[q][c] = src[c * pitch + nb[q]], Bn[q][c] = src[(3 + c) * pitch + nb[q]];
            }
            const float a = s_a[i];
            const float I[3] = {s_i[i], s_i[pitch + i], s_i[2 * pitch + i]};
            fg_update(a, I, an, Fn, Bn, in.reg, in.gw, F, B);
            if (k < n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * pitch + i] = F[c], dst[(3 + c) * pitch + i] = B[c];
            } else {  // the tile itself: the alpha byte once more for the cutout (the same load as the staged one)
                const unsigned a8 = lvl ? 0u : alpha[(long long)s_sy[ly] * W + s_sx[lx]];
                fg_store(lvl ? lvl + b * 6 * ((long long)hl * wl) : nullptr, (long long)hl * wl, out, b, hl, wl, y, x, a8, F, B);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

// the floats of the two level buffers of one image: level L - 1 (and L - 3, ...) and level L - 2 (and L - 4, ...)
inline void fg_buffers(int H, int W, long long& n0, long long& n1) {
    const int L = fg_num_levels(H, W);
    n0 = L >= 1 ? 6LL * fg_level_size(H, L, L - 1) * fg_level_size(W, L, L - 1) : 0;
    n1 = L >= 2 ? 6LL * fg_level_size(H, L, L - 2) * fg_level_size(W, L, L - 2) : 0;
}

inline long long fg_workspace_bytes(int B, int H, int W) {
    long long n0, n1;
    fg_buffers(H, W, n0, n1);
    const long long per = (n0 + n1) * 4;
    return (long long)B * (per > 8 ? per : 8);  // (6 floats per pixel: a multiple of 8)
}

}  // namespace

extern "C" {

long long gp_foreground_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || H > FG_MAX_DIM || W > FG_MAX_DIM) return 0;
    return fg_workspace_bytes(B, H, W);
}

gp_status gp_foreground(const unsigned char* image, const void* alpha, int alpha_is_u8, int B, int H, int W, float reg, float gw, int n_small,
                        int n_big, const unsigned char* new_bg, int new_rgb, float* fg_out, float* bg_out, unsigned char* rgba_out,
                        unsigned char* comp_out, void* workspace, long long workspace_bytes, void* stream) {
    if (!image || !alpha || !workspace || !(fg_out || bg_out || rgba_out || comp_out)) return GP_ERR_INVALID;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > FG_MAX_DIM || W > FG_MAX_DIM) return GP_ERR_INVALID;
    if (!(reg >= 1e-6f && reg <= 1.0f) || !(gw >= 0.0f && gw <= 100.0f)) return GP_ERR_INVALID;  // (NaN fails both)
    if (n_small < 0 || n_small > 64 || n_big < 1 || n_big > 4) return GP_ERR_INVALID;
    if (new_rgb < 0 || new_rgb > 0xffffff) return GP_ERR_INVALID;
    if (!eval_pred_ok(alpha, alpha_is_u8) || !eval_aligned8(workspace)) return GP_ERR_INVALID;
    if ((((uintptr_t)fg_out | (uintptr_t)bg_out | (uintptr_t)rgba_out) & 3) != 0) return GP_ERR_INVALID;
    if (workspace_bytes < fg_workspace_bytes(B, H, W)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int L = fg_num_levels(H, W);
    long long n0, n1;
    fg_buffers(H, W, n0, n1);
    float* buf[2] = {(float*)workspace, (float*)workspace + (long long)B * n0};  // level l < L lives in buf[(L - 1 - l) & 1]
    int lc = 0;
    while (lc < L && fg_level_size(H, L, lc + 1) <= FG_SMALL && fg_level_size(W, L, lc + 1) <= FG_SMALL) ++lc;
    const FgIn in = {image, alpha, H, W, L, reg, gw};
    const FgOut out = {fg_out, bg_out, rgba_out, comp_out, new_bg, (unsigned)new_rgb};
    const auto coarse = alpha_is_u8 ? fg_coarse_kernel<true> : fg_coarse_kernel<false>;
    const auto level = alpha_is_u8 ? fg_level_kernel<true> : fg_level_kernel<false>;
    hipLaunchKernelGGL(coarse, dim3(B), dim3(FG_COARSE_THREADS), 0, s, in, lc, n_small, lc < L ? buf[(L - 1 - lc) & 1] : nullptr, out);
    const int pitch = (FG_TW + 2 * n_big) * (FG_TH + 2 * n_big);
    for (int l = lc + 1; l <= L; ++l) {
        const int hl = fg_level_size(H, L, l), wl = fg_level_size(W, L, l), hp = fg_level_size(H, L, l - 1), wp = fg_level_size(W, L, l - 1);
        const int ntx = (wl + FG_TW - 1) / FG_TW, nty = (hl + FG_TH - 1) / FG_TH;  // ntx * nty <= 512 * 1024
        hipLaunchKernelGGL(level, dim3((unsigned)ntx * (unsigned)nty, B), dim3(FG_THREADS), (size_t)FG_PLANES * pitch * 4, s, in, hl, wl, hp, wp,
                           (const float*)buf[(L - l) & 1], n_big, ntx, pitch, l < L ? buf[(L - 1 - l) & 1] : nullptr, out);
    }
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
