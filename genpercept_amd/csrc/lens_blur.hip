// Synthetic depth of field on the device (gp_lens_blur): the photograph refocused under its depth or disparity prediction, every output pixel
// a variable-radius, occlusion-aware gather over the discs of its neighbours.  The definition is stated in include/genpercept_hip.h;
// genpercept_amd/lens_blur.py restates it on the host and gives the same bits; the arithmetic is lens_blur_math.h, which
// tests/lens_blur_check.cpp also runs on the CPU.
//   One launch for any batch; one workgroup of 512 threads per 32 x 16 output pixels of an image.
//   stage    the tile plus an apron of R = (max_c8 + 4) / 8 pixels, the reach of the call's largest radius, is computed once from the image, the
//            prediction, the mask and the image's parameter row and staged in LDS as one 64-bit word per pixel (D 16 bits, c 9 bits, three
//            12-bit linear colours; 60 KiB at R = 32).  A pixel outside the image is the word 0, which reaches nobody.  Adjacent lanes write and
//            later read adjacent words.  to_lin goes through LDS as well.
//   bound    cm = the largest c of the STAGED REGION, tile and apron together (shuffles inside a wave, LDS across the waves): no source the
//            tile can see reaches further than (cm + 4) / 8 pixels, so the gather walks the disc of cm only -- one pixel where the region is in
//            focus.  The tile's own largest c would be wrong: a blurred source in the apron spreads into a sharp tile.  The weights w(0 .. cm)
//            and the widest dx of every row of that disc are computed by the first threads into LDS.
//   gather   a thread walks the disc of its pixel row by row; the sums are 64-bit integers, so their order is free.
// No atomics, no workspace, nothing read back; which thread computes which pixel depends on the sizes only and every sum is an integer sum, so
// an image's bytes are the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "lens_blur_math.h"

namespace {

constexpr int LB_TW = 32, LB_TH = 16;      // the output tile
constexpr int LB_THREADS = LB_TW * LB_TH;  // 512: one thread per pixel of the tile
constexpr int LB_WAVES = LB_THREADS / 64;
constexpr int LB_W_SLOTS = 260;            // w(0 .. 256), padded to a multiple of 4 words
constexpr int LB_DX_SLOTS = 36;            // the widest dx of the rows dy = 0 .. 32, padded

struct LbCall {
    int H, W, space, max_c8, R;
};

// the dynamic LDS of a launch with the apron R: the words, w, to_lin, the row widths, the waves' maxima
inline size_t lb_lds_bytes(int R) {
    return (size_t)8 * (LB_TW + 2 * R) * (LB_TH + 2 * R) + 4 * LB_W_SLOTS + 2 * 256 + 4 * LB_DX_SLOTS + 4 * LB_WAVES;
}

// grid (ceil(W / 32), ceil(H / 16), B).  image, out: [B][3][H][W]; pred: [B][H][W]; sharp, coc: [B][H][W] or NULL; params: [B][4].
__global__ __launch_bounds__(LB_THREADS) void lb_gather_kernel(const unsigned char* __restrict__ image, const float* __restrict__ pred,
                                                              const unsigned char* __restrict__ sharp, const int* __restrict__ params,
                                                              const unsigned short* __restrict__ to_lin, const unsigned char* __restrict__ from_lin,
                                                              LbCall a, unsigned char* __restrict__ out, unsigned short* __restrict__ coc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lb[];
    const int R = a.R, pw = LB_TW + 2 * R, ph = LB_TH + 2 * R, np = pw * ph;
    lb_u64* s_px = (lb_u64*)s_lb;                            // [ph][pw]
    unsigned* s_w = (unsigned*)(s_px + np);                  // [LB_W_SLOTS]
    unsigned short* s_lin = (unsigned short*)(s_w + LB_W_SLOTS);  // [256]
    int* s_dx = (int*)(s_lin + 256);                         // [LB_DX_SLOTS]
    int* s_max = s_dx + LB_DX_SLOTS;                         // [LB_WAVES]
    const int tid = threadIdx.x;
    const long long b = blockIdx.z, HW = (long long)a.H * a.W;
    const LbParams prm = lb_params(params + b * LB_PARAMS, a.max_c8);
    if (tid < 256) s_lin[tid] = to_lin[tid];
    __syncthreads();

    const int x0 = blockIdx.x * LB_TW - R, y0 = blockIdx.y * LB_TH - R;
    int cm = 0;
    for (int i = tid; i < np; i += LB_THREADS) {
        const int py = i / pw, px = i - py * pw, y = y0 + py, x = x0 + px;
        lb_u64 word = 0;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const long long q = (long long)y * a.W + x;
            const float v = pred[b * HW + q];
            const int D = lb_nearness(v, a.space);
            const int c = lb_coc(D, !(v == v) || (sharp && sharp[b * HW + q] != 0), prm);
            const unsigned char* g = image + b * 3 * HW + q;
            word = lb_pack(D, c, s_lin[g[0]], s_lin[g[HW]], s_lin[g[2 * HW]]);
            cm = c > cm ? c : cm;
        }
        s_px[i] = word;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int other = __shfl_xor(cm, off, 64);
        cm = other > cm ? other : cm;
    }
    if ((tid & 63) == 0) s_max[tid >> 6] = cm;
    __syncthreads();
    cm = s_max[0];
#pragma unroll
    for (int k = 1; k < LB_WAVES; ++k) cm = s_max[k] > cm ? s_max[k] : cm;
    // (cm <= max_c8 <= 256 < LB_THREADS - LB_DX_SLOTS: the two tables have threads of their own)
    const int Rs = lb_reach_pixels(cm);  // <= R
    if (tid <= cm) s_w[tid] = lb_disc_weight(tid);
    if (tid >= LB_THREADS - 1 - Rs) {
        const int dy = LB_THREADS - 1 - tid, k = (((cm + 4) * (cm + 4)) >> 6) - dy * dy;  // dx^2 <= k, k >= 0
        int dx = 0;
        while ((dx + 1) * (dx + 1) <= k) ++dx;
        s_dx[dy] = dx;
    }
    __syncthreads();

    const int tx = tid % LB_TW, ty = tid / LB_TW;
    const int u = blockIdx.x * LB_TW + tx, v = blockIdx.y * LB_TH + ty;
    if (u >= a.W || v >= a.H) return;
    const int centre = (ty + R) * pw + (tx + R);
    const lb_u64 me = s_px[centre];
    const int Dp = lb_word_D(me), cp = lb_word_c(me);
    LbSums f;
    lb_sums_clear(f);
    for (int dy = -Rs; dy <= Rs; ++dy) {
        const int dxm = s_dx[dy < 0 ? -dy : dy], dy2 = dy * dy;
        const lb_u64* row = s_px + centre + dy * pw;
#pragma unroll 4
        for (int dx = -dxm; dx <= dxm; ++dx) {
            const lb_u64 word = row[dx];
            const int r = lb_reach(lb_word_D(word), lb_word_c(word), Dp, cp);
            const unsigned wt = s_w[r];  // (r <= cm: the entry is there)
            lb_sums_add(f, lb_inside(dx * dx + dy2, r) ? wt : 0u, word);
        }
    }
    const long long p = (long long)v * a.W + u;
    unsigned char* o = out + b * 3 * HW + p;
    o[0] = from_lin[lb_resolve(f.s[0], f.sw)];
    o[HW] = from_lin[lb_resolve(f.s[1], f.sw)];
    o[2 * HW] = from_lin[lb_resolve(f.s[2], f.sw)];
    if (coc) coc[b * HW + p] = (unsigned short)cp;
}

}  // namespace

extern "C" {

gp_status gp_lens_blur(const unsigned char* image, const float* pred, const unsigned char* sharp, const int* params, const unsigned short* to_lin,
                       const unsigned char* from_lin, int B, int H, int W, int space, int max_c8, unsigned char* out, unsigned short* coc,
                       void* stream) {
    if (!image || !pred || !params || !to_lin || !from_lin || !out) return GP_ERR_INVALID;
    if (!lb_dims_ok(B, H, W) || !lb_options_ok(space, max_c8)) return GP_ERR_INVALID;
    if ((((uintptr_t)pred | (uintptr_t)params) & 3) != 0 || (((uintptr_t)to_lin | (uintptr_t)coc) & 1) != 0) return GP_ERR_INVALID;
    if (out == image) return GP_ERR_INVALID;  // a gather cannot run in place
    const int R = lb_reach_pixels(max_c8);
    const LbCall a = {H, W, space, max_c8, R};
    hipLaunchKernelGGL(lb_gather_kernel, dim3((W + LB_TW - 1) / LB_TW, (H + LB_TH - 1) / LB_TH, B), dim3(LB_THREADS), lb_lds_bytes(R),
                       (hipStream_t)stream, image, pred, sharp, params, to_lin, from_lin, a, out, coc);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
