// Relighting on the device (gp_relight): the photograph under up to eight new directional lights and an ambient term, shaded by its normal
// map -- diffuse and specular -- with screen-space cast shadows marched over its depth or disparity map, blended with the image under an
// optional weight.  The definition is stated in include/genpercept_hip.h; genpercept_amd/relight.py restates it on the host and gives the
// same bits; the arithmetic is relight_math.h, which tests/relight_check.cpp also runs on the CPU.
//   One launch for any batch and any number of lights; one workgroup of 256 threads per 32 x 16 output pixels of an image, two pixels (rows
//   ty and ty + 8) per thread.  The light table, host memory, travels as a kernel argument.
//   stage    (shadows only) the nearness D of the tile plus an apron of R pixels, the longest reach of the table's rows, is computed once
//            from the prediction and staged in LDS as one 16-bit word per pixel (45 KiB at R = 64: three workgroups per CU).  A pixel
//            outside the image is the word 0, which shadows nobody.  Adjacent lanes write and later read adjacent words; a 32-lane half
//            of a wave is one row of the tile, so along any march direction its lanes read 32 adjacent words: 16 or 17 banks, no conflict.
//   bound    Dmax = the largest D of the STAGED REGION (shuffles inside a wave, LDS across the waves): e_t = D(q_t) - floor_t with floor_t
//            growing in t, so a march ends at the first t with floor_t >= Dmax -- a flat background costs one step per light, not 64.
//   shade    per pixel and light the two ratios of relight_math.h, the march where the light reaches the pixel, integer sums.
// The shading-only form (no pred, or no row with a reach) stages nothing: a streaming kernel over three float planes and three byte planes.
// No atomics, no workspace, nothing read back; which thread computes which pixel depends on the sizes only and every sum is an integer sum,
// so an image's bytes are the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "relight_math.h"

namespace {

constexpr int RL_TW = 32, RL_TH = 16;  // the output tile
constexpr int RL_THREADS = 256;        // two pixels of the tile per thread
constexpr int RL_WAVES = RL_THREADS / 64;

struct RlCall {
    int H, W, L, encoded, flip, space, R;
};

// the dynamic LDS of a launch with the apron R: the 16-bit words, rounded up to whole dwords
inline size_t rl_lds_bytes(int R) { return (((size_t)2 * (RL_TW + 2 * R) * (RL_TH + 2 * R)) + 3) & ~(size_t)3; }

// grid (ceil(W / 32), ceil(H / 16), B).  image, out: [B][3][H][W]; normal: [B][3][H][W]; pred, weight, shadow: [B][H][W] or NULL.
template <bool SHADOWS>
__global__ __launch_bounds__(RL_THREADS) void rl_relight_kernel(const unsigned char* __restrict__ image, const float* __restrict__ normal,
                                                                const float* __restrict__ pred, const unsigned char* __restrict__ weight,
                                                                const unsigned short* __restrict__ to_lin,
                                                                const unsigned char* __restrict__ from_lin, const RlTable tab, RlCall a,
                                                                unsigned char* __restrict__ out, unsigned char* __restrict__ shadow) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_rl[];
    __shared__ int s_max[RL_WAVES];
    unsigned short* s_D = (unsigned short*)s_rl;  // [ph][pw]
    const int R = a.R, pw = RL_TW + 2 * R, ph = RL_TH + 2 * R;
    const int tid = threadIdx.x;
    const long long b = blockIdx.z, HW = (long long)a.H * a.W;
    int Dmax = 0;
    if (SHADOWS) {
        const int x0 = blockIdx.x * RL_TW - R, y0 = blockIdx.y * RL_TH - R, np = pw * ph;
        for (int i = tid; i < np; i += RL_THREADS) {
            const int py = i / pw, px = i - py * pw, y = y0 + py, x = x0 + px;
            int D = 0;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) D = rl_nearness(pred[b * HW + (long long)y * a.W + x], a.space);
            s_D[i] = (unsigned short)D;
            Dmax = D > Dmax ? D : Dmax;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int other = __shfl_xor(Dmax, off, 64);
            Dmax = other > Dmax ? other : Dmax;
        }
        if ((tid & 63) == 0) s_max[tid >> 6] = Dmax;
        __syncthreads();
        Dmax = s_max[0];
#pragma unroll
        for (int k = 1; k < RL_WAVES; ++k) Dmax = s_max[k] > Dmax ? s_max[k] : Dmax;
    }

    const int tx = tid % RL_TW, u = blockIdx.x * RL_TW + tx;
    if (u >= a.W) return;
    const int* amb = tab.v[a.L];
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int ty = tid / RL_TW + half * (RL_TH / 2), v = blockIdx.y * RL_TH + ty;
        if (v >= a.H) return;
        const long long p = (long long)v * a.W + u;
        const float* nv = normal + b * 3 * HW + p;
        const RlNormal nrm = rl_normal(nv[0], nv[HW], nv[2 * HW], a.encoded, a.flip);
        bool lit = false;  // whether this pixel can receive a shadow
        int Dp = 0, centre = 0;
        if (SHADOWS) {
            const float pv = pred[b * HW + p];
            lit = pv == pv;
            centre = (ty + R) * pw + (tx + R);
            Dp = s_D[centre];
        }
        RlSums f;
        rl_sums_clear(f);
#pragma unroll 1
        for (int j = 0; j < a.L; ++j) {
            const int* row = tab.v[j];
            const int cos12 = rl_cos12(nrm, row + RL_LX);
            if (cos12 == 0) continue;
            int E = 0;
            if (SHADOWS && lit) {
                const int reach = row[RL_REACH], ux = row[RL_UX], uy = row[RL_UY];
                for (int t = 1; t <= reach; ++t) {
                    const int fl = rl_floor(Dp, row, t);
                    if (fl >= Dmax) break;
                    // (|offset| <= t <= reach <= R: inside the staged region; outside the image the word is 0)
                    const int e = (int)s_D[centre + rl_step(t, uy) * pw + rl_step(t, ux)] - fl;
                    E = e > E ? e : E;
                }
            }
            rl_sums_add(f, row, cos12, rl_specular(nrm, row), rl_shade(E, row));
        }
        const unsigned char* g = image + b * 3 * HW + p;
        unsigned char* o = out + b * 3 * HW + p;
        const unsigned w = weight ? weight[b * HW + p] : 255u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned byte = g[k * HW];
            o[k * HW] = rl_blend(from_lin[rl_lin(f, amb, k, to_lin[byte])], byte, w);
        }
        if (shadow) shadow[b * HW + p] = rl_shadow_byte(f.shade);
    }
}

}  // namespace

extern "C" {

gp_status gp_relight(const unsigned char* image, const float* normal, const float* pred, const unsigned char* weight, const int* lights,
                     const unsigned short* to_lin, const unsigned char* from_lin, int B, int H, int W, int L, int encoded, int flip, int space,
                     int max_reach, unsigned char* out, unsigned char* shadow, void* stream) {
    if (!image || !normal || !lights || !to_lin || !from_lin || !out) return GP_ERR_INVALID;
    if (!rl_dims_ok(B, H, W) || !rl_options_ok(L, encoded, flip, space, max_reach)) return GP_ERR_INVALID;
    if ((((uintptr_t)normal | (uintptr_t)pred | (uintptr_t)lights) & 3) != 0 || ((uintptr_t)to_lin & 1) != 0) return GP_ERR_INVALID;
    if (out == image) return GP_ERR_INVALID;  // the image is read after neighbours may have been written
    if (!rl_table_ok(lights, L, max_reach)) return GP_ERR_INVALID;  // (host memory: read here)
    RlTable tab = {};
    int R = 0;
    for (int j = 0; j <= L; ++j)
        for (int k = 0; k < RL_ROW; ++k) tab.v[j][k] = lights[j * RL_ROW + k];
    for (int j = 0; j < L; ++j) R = tab.v[j][RL_REACH] > R ? tab.v[j][RL_REACH] : R;
    const RlCall a = {H, W, L, encoded, flip, space, pred ? R : 0};
    const dim3 grid((W + RL_TW - 1) / RL_TW, (H + RL_TH - 1) / RL_TH, B);
    if (pred && R > 0)
        hipLaunchKernelGGL(rl_relight_kernel<true>, grid, dim3(RL_THREADS), rl_lds_bytes(R), (hipStream_t)stream, image, normal, pred, weight, to_lin,
                           from_lin, tab, a, out, shadow);
    else
        hipLaunchKernelGGL(rl_relight_kernel<false>, grid, dim3(RL_THREADS), 0, (hipStream_t)stream, image, normal, pred, weight, to_lin, from_lin, tab,
                           a, out, shadow);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
