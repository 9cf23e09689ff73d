// Test-time ensembling on the device (gp_ensemble_gather, gp_ensemble_reduce): the tensor half of genpercept/util/ensemble.py:43-205 for the E
// members of every image of a batch that are already on the GPU.  The host restatement is genpercept_amd/ensemble.py; the BFGS optimiser over
// E x (<= max_res^2) numbers stays on the host between the two entries.
//   gather   the nearest-exact reduction the optimiser works on (image_util.resize_max_res, the source index of prepost.hip) and each
//            reduced member's min / max, from which the optimiser's initial guess is built;
//   reduce   per pixel in float32: a_e = d_e * s_e + t_e (two roundings, no FMA), then the element of rank (E - 1) / 2 of the members
//            (torch.median: the LOWER middle for even E) with the same rank of |a_e - median| as uncertainty, or the mean (summed in member
//            order, divided by E) with the unbiased standard deviation; then per image pred = (pred - d_min) / rng and uncertainty / rng with
//            rng = max(d_max - d_min, 1e-6), d_min = 0 for scale-only alignment.
// One streaming pass over the members (4 E bytes per pixel) that writes the un-normalised maps and leaves one (min, max) slab per workgroup in
// the workspace, a one-workgroup-per-image finaliser, an in-place normalise pass.  Stream-ordered, no host synchronisation, no atomics.  The
// number of workgroups per image and the pixel -> thread assignment depend on H * W alone -- never on B, on the image's position in the batch
// or on pointer alignment (which only selects 16-byte or scalar accesses of the same four pixels) -- so an image's result is bitwise the same
// alone and inside any batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "resize_index.h"

// The framework ops this replaces have no fused multiply-adds (eval.hip explains why the pragma and not the __f*_rn wrappers); float division
// and square root are correctly rounded by default.
#pragma clang fp contract(off)

namespace {

constexpr int EN_THREADS = 256;
constexpr long long EN_PIX_PER_WG = 4 * EN_THREADS;  // at least one quad per thread ...
constexpr int EN_MAX_WG = 1024;                      // ... and at most this many workgroups (= slabs) per image
constexpr int EN_REG_E = 16;                         // E <= 16: members in registers, fully unrolled; above: members re-read from cache
constexpr int EN_MAX_E = 64;
constexpr int GA_THREADS = 1024;                     // the gather: one workgroup per reduced member

int ens_blocks(long long hw) {
    long long g = (hw + EN_PIX_PER_WG - 1) / EN_PIX_PER_WG;
    return (int)(g < 1 ? 1 : (g > EN_MAX_WG ? EN_MAX_WG : g));
}

// (lo, hi) of every thread -> min / max over the workgroup, valid in thread 0.  min and max are exact, so the order cannot change the result.
template <int WAVES>
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
    __shared__ float s_lo[WAVES], s_hi[WAVES];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) lo = fminf(lo, s_lo[w]), hi = fmaxf(hi, s_hi[w]);
    }
}

// one workgroup per plane (b, e): small[plane] = depth[plane][iy(oy)][ix(ox)], minmax[plane] = (min, max) of the reduced member
__global__ __launch_bounds__(GA_THREADS) void ens_gather_kernel(const float* __restrict__ depth, int H, int W, int h, int w, float sy, float sx,
                                                                float* __restrict__ small, float* __restrict__ minmax) {
    const long long plane = blockIdx.x;
    const float* src = depth + plane * H * W;
    float* dst = small + plane * h * w;
    const long long n = (long long)h * w;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long long idx = threadIdx.x; idx < n; idx += GA_THREADS) {
        const int ox = (int)(idx % w), oy = (int)(idx / w);
        const int iy = nearest_exact_src(oy, sy, H), ix = nearest_exact_src(ox, sx, W);
        const float v = src[(long long)iy * W + ix];
        dst[idx] = v;
        lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    block_minmax<GA_THREADS / 64>(lo, hi);
    if (threadIdx.x == 0) minmax[plane * 2] = lo, minmax[plane * 2 + 1] = hi;
}

struct Quad { float v[4]; };  // four consecutive pixels of one map (0 beyond the image)

// pixels i0 .. i0 + 3: one 16-byte load when the map's base address allows it (vec) and the quad is whole, scalar loads otherwise
__device__ __forceinline__ Quad load_quad(const float* __restrict__ p, long long i0, long long hw, bool vec) {
    Quad r;
    if (vec && i0 + 4 <= hw) {
        const float4 t = *reinterpret_cast<const float4*>(p + i0);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[j] = i0 + j < hw ? p[i0 + j] : 0.f;
    }
    return r;
}
__device__ __forceinline__ void store_quad(float* __restrict__ p, long long i0, long long hw, bool vec, const float (&v)[4]) {
    if (vec && i0 + 4 <= hw) {
        *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < hw) p[i0 + j] = v[j];
    }
}

// member e of four pixels, aligned: d * s + t in two roundings (t == nullptr: d * s)
__device__ __forceinline__ Quad aligned_quad(const float* __restrict__ d, const float* __restrict__ sc, const float* __restrict__ sh, int e, long long i0,
                                             long long hw, bool vec) {
    Quad q = load_quad(d + (long long)e * hw, i0, hw, vec);
    const float s = sc[e];
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = q.v[j] * s;
    if (sh) {
        const float t = sh[e];
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = q.v[j] + t;
    }
    return q;
}

// The element of rank (E - 1) / 2: rank_i = #{j : a_j < a_i or (a_j == a_i and j < i)} is a permutation of 0 .. E - 1, so exactly one i matches.
template <int E>
__device__ __forceinline__ float select_median(const float (&a)[E]) {
    constexpr int K = (E - 1) / 2;
    float r = a[0];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (j < i) rank += a[j] <= a[i] ? 1 : 0;
            if (j > i) rank += a[j] < a[i] ? 1 : 0;
        }
        r = rank == K ? a[i] : r;
    }
    return r;
}

// E members of one pixel in registers -> (pred, uncertainty) before the rescale.  RED 0: median, 1: mean.
template <int E, int RED>
__device__ __forceinline__ void reduce_regs(const float (&a)[E], bool want_unc, float& pred, float& unc) {
    unc = 0.f;
    if constexpr (RED == 0) {
        pred = select_median<E>(a);
        if (want_unc) {
            float d[E];
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = fabsf(a[e] - pred);
            unc = select_median<E>(d);
        }
    } else {
        float s = a[0];
#pragma unroll
        for (int e = 1; e < E; ++e) s = s + a[e];
        pred = s / (float)E;
        if (want_unc) {  // two passes over the values the thread holds, divisor E - 1 (E = 1: 0 / 0 = NaN, as torch.std)
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float d = a[e] - pred;
                ss = ss + d * d;
            }
            unc = sqrtf(ss / (float)(E - 1));
        }
    }
}

// The same for a runtime E (17 .. 64): the members of the quad are re-read (they are cache-resident) in the inner loops.
template <int RED>
__device__ __forceinline__ void reduce_mem(const float* __restrict__ d, const float* __restrict__ sc, const float* __restrict__ sh, int E, long long i0,
                                           long long hw, bool vec, bool want_unc, float (&pred)[4], float (&unc)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) pred[p] = 0.f, unc[p] = 0.f;
    if constexpr (RED == 0) {
        const int K = (E - 1) / 2;
        for (int pass = 0; pass < (want_unc ? 2 : 1); ++pass) {  // pass 0: rank of a_e; pass 1: rank of |a_e - median|
            float med[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) med[p] = pred[p];
            for (int i = 0; i < E; ++i) {
                Quad ai = aligned_quad(d, sc, sh, i, i0, hw, vec);
                if (pass) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) ai.v[p] = fabsf(ai.v[p] - med[p]);
                }
                int rank[4] = {0, 0, 0, 0};
                for (int j = 0; j < E; ++j) {
                    Quad aj = aligned_quad(d, sc, sh, j, i0, hw, vec);
                    if (pass) {
#pragma unroll
                        for (int p = 0; p < 4; ++p) aj.v[p] = fabsf(aj.v[p] - med[p]);
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) rank[p] += (aj.v[p] < ai.v[p] || (aj.v[p] == ai.v[p] && j < i)) ? 1 : 0;
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (rank[p] == K) (pass ? unc[p] : pred[p]) = ai.v[p];
                }
            }
        }
    } else {
        float s[4];
        for (int e = 0; e < E; ++e) {
            const Quad a = aligned_quad(d, sc, sh, e, i0, hw, vec);
#pragma unroll
            for (int p = 0; p < 4; ++p) s[p] = e == 0 ? a.v[p] : s[p] + a.v[p];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) pred[p] = s[p] / (float)E;
        if (want_unc) {
            float ss[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e = 0; e < E; ++e) {
                const Quad a = aligned_quad(d, sc, sh, e, i0, hw, vec);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float x = a.v[p] - pred[p];
                    ss[p] = ss[p] + x * x;
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) unc[p] = sqrtf(ss[p] / (float)(E - 1));
        }
    }
}

// pass 1: align + reduce, un-normalised pred / uncertainty out, one (min, max) of pred per workgroup.  grid (ens_blocks(H * W), B).
// EC > 0: E == EC at compile time, members in registers; EC == 0: runtime E.
template <int EC, int RED>
__global__ __launch_bounds__(EN_THREADS) void ens_reduce_kernel(const float* __restrict__ depth, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int E, long long hw, float* __restrict__ pred,
                                                                float* __restrict__ unc, float* __restrict__ ws) {
    const long long b = blockIdx.y;
    const float* d = depth + b * E * hw;
    const float* sc = scale + b * E;
    const float* sh = shift ? shift + b * E : nullptr;
    float* po = pred + b * hw;
    float* uo = unc ? unc + b * hw : nullptr;
    // every member's base address is 16-byte aligned when the image's is and the member stride is a whole number of quads
    const bool vld = ((uintptr_t)d & 15) == 0 && ((hw & 3) == 0 || E == 1);
    const bool vst = ((uintptr_t)po & 15) == 0 && ((uintptr_t)uo & 15) == 0;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const long long nq = (hw + 3) / 4;
    for (long long q = (long long)blockIdx.x * EN_THREADS + threadIdx.x; q < nq; q += (long long)gridDim.x * EN_THREADS) {
        const long long i0 = q * 4;
        float p4[4], u4[4];
        if constexpr (EC > 0) {
            float a[4][EC];
#pragma unroll
            for (int e = 0; e < EC; ++e) {
                const Quad v = aligned_quad(d, sc, sh, e, i0, hw, vld);
#pragma unroll
                for (int p = 0; p < 4; ++p) a[p][e] = v.v[p];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) reduce_regs<EC, RED>(a[p], uo != nullptr, p4[p], u4[p]);
        } else {
            reduce_mem<RED>(d, sc, sh, E, i0, hw, vld, uo != nullptr, p4, u4);
        }
        store_quad(po, i0, hw, vst, p4);
        if (uo) store_quad(uo, i0, hw, vst, u4);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (i0 + p < hw) lo = fminf(lo, p4[p]), hi = fmaxf(hi, p4[p]);
        }
    }
    block_minmax<EN_THREADS / 64>(lo, hi);
    if (threadIdx.x == 0) {
        float* slab = ws + (b * gridDim.x + blockIdx.x) * 2;
        slab[0] = lo, slab[1] = hi;
    }
}

// after pass 1: the slabs of one image -> fin[b] = (d_min, rng).  One wave per image.
__global__ __launch_bounds__(64) void ens_finalise_kernel(const float* __restrict__ ws, int nblk, int has_shift, float* __restrict__ fin) {
    const long long b = blockIdx.x;
    const float* slabs = ws + b * nblk * 2;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int j = threadIdx.x; j < nblk; j += 64) lo = fminf(lo, slabs[2 * j]), hi = fmaxf(hi, slabs[2 * j + 1]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
    }
    if (threadIdx.x == 0) {
        const float d_min = has_shift ? lo : 0.f;
        fin[b * 2] = d_min;
        fin[b * 2 + 1] = fmaxf(hi - d_min, 1e-6f);
    }
}

// pass 2, in place: pred = (pred - d_min) / rng, uncertainty = uncertainty / rng.  Same grid as pass 1.
__global__ __launch_bounds__(EN_THREADS) void ens_normalise_kernel(float* __restrict__ pred, float* __restrict__ unc, long long hw, const float* __restrict__ fin) {
    const long long b = blockIdx.y;
    float* po = pred + b * hw;
    float* uo = unc ? unc + b * hw : nullptr;
    const float d_min = fin[b * 2], rng = fin[b * 2 + 1];
    const bool vec = ((uintptr_t)po & 15) == 0 && ((uintptr_t)uo & 15) == 0;
    const long long nq = (hw + 3) / 4;
    for (long long q = (long long)blockIdx.x * EN_THREADS + threadIdx.x; q < nq; q += (long long)gridDim.x * EN_THREADS) {
        const long long i0 = q * 4;
        Quad v = load_quad(po, i0, hw, vec);
#pragma unroll
        for (int p = 0; p < 4; ++p) v.v[p] = (v.v[p] - d_min) / rng;
        store_quad(po, i0, hw, vec, v.v);
        if (uo) {
            Quad u = load_quad(uo, i0, hw, vec);
#pragma unroll
            for (int p = 0; p < 4; ++p) u.v[p] = u.v[p] / rng;
            store_quad(uo, i0, hw, vec, u.v);
        }
    }
}

template <int RED>
void launch_reduce(int E, dim3 grid, hipStream_t s, const float* depth, const float* scale, const float* shift, long long hw, float* pred, float* unc,
                   float* ws) {
    switch (E) {
#define EN_CASE(n)                                                                                                                         \
    case n:                                                                                                                                \
        hipLaunchKernelGGL((ens_reduce_kernel<n, RED>), grid, dim3(EN_THREADS), 0, s, depth, scale, shift, E, hw, pred, unc, ws);          \
        break;
        EN_CASE(1) EN_CASE(2) EN_CASE(3) EN_CASE(4) EN_CASE(5) EN_CASE(6) EN_CASE(7) EN_CASE(8)
        EN_CASE(9) EN_CASE(10) EN_CASE(11) EN_CASE(12) EN_CASE(13) EN_CASE(14) EN_CASE(15) EN_CASE(16)
#undef EN_CASE
        default:
            hipLaunchKernelGGL((ens_reduce_kernel<0, RED>), grid, dim3(EN_THREADS), 0, s, depth, scale, shift, E, hw, pred, unc, ws);
    }
}
static_assert(EN_REG_E == 16, "launch_reduce lists the compile-time member counts");

}  // namespace

extern "C" {

gp_status gp_ensemble_gather(const float* depth, int B, int E, int H, int W, int h, int w, float* small, float* minmax, void* stream) {
    if (!depth || !small || !minmax) return GP_ERR_INVALID;
    if (B < 1 || E < 1 || H < 1 || W < 1 || h < 1 || w < 1) return GP_ERR_INVALID;
    if ((long long)H * W > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL || (long long)B * E > 0x7fffffffLL) return GP_ERR_INVALID;
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;  // area_pixel_compute_scale, align_corners = false (prepost.hip)
    hipLaunchKernelGGL(ens_gather_kernel, dim3((unsigned)(B * E)), dim3(GA_THREADS), 0, (hipStream_t)stream, depth, H, W, h, w, sy, sx, small, minmax);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

long long gp_ensemble_workspace(int B, int E, int H, int W) {
    if (B < 1 || E < 1 || H < 1 || W < 1) return 0;
    return (long long)B * (ens_blocks((long long)H * W) + 1) * 2 * (long long)sizeof(float);  // the slabs, then (d_min, rng) per image
}

gp_status gp_ensemble_reduce(const float* depth, const float* scale, const float* shift, int B, int E, int H, int W, int reduction, float* pred,
                             float* uncertainty, void* workspace, long long workspace_bytes, void* stream) {
    if (E < 1 || E > EN_MAX_E || reduction < 0 || reduction > 1) return GP_ERR_INVALID;
    if (!depth || !scale || !pred || !workspace) return GP_ERR_INVALID;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return GP_ERR_INVALID;
    if (workspace_bytes < gp_ensemble_workspace(B, E, H, W) || ((uintptr_t)workspace & 7) != 0) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W;
    const int nblk = ens_blocks(hw);
    float* ws = (float*)workspace;
    float* fin = ws + (long long)B * nblk * 2;
    if (reduction == 0) launch_reduce<0>(E, dim3(nblk, B), s, depth, scale, shift, hw, pred, uncertainty, ws);
    else launch_reduce<1>(E, dim3(nblk, B), s, depth, scale, shift, hw, pred, uncertainty, ws);
    hipLaunchKernelGGL(ens_finalise_kernel, dim3(B), dim3(64), 0, s, (const float*)ws, nblk, shift ? 1 : 0, fin);
    hipLaunchKernelGGL(ens_normalise_kernel, dim3(nblk, B), dim3(EN_THREADS), 0, s, pred, uncertainty, hw, (const float*)fin);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
