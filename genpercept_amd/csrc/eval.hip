// Depth evaluation on the device (gp_eval_depth): the per-image protocol of eval.py:168-215 -- least-squares alignment
// (src/util/alignment.py:29-94), clip to the dataset range, the ten metrics of src/util/metric.py:34-158 -- for predictions that are
// already on the GPU.  The host restatement is genpercept_amd/eval_metrics.py (evaluate_depth); this file reproduces what that code computes
// for float32 `pred` / `gt`:
//   fit      np.linalg.lstsq works in float64 and returns float32: here float64 sums n, Sp, Sg, Spp, Spg over the fit mask, the 2 x 2 normal
//            equations in float64, (s, t) rounded to float32;
//   apply    aligned = pred * s + t in float32, two roundings, no FMA; disparity space: gt_disp = 1 / gt (float32, 0 where gt <= 0), fit mask
//            valid & gt > 0 & pred > 0, disp clipped at 1e-3, aligned = 1 / disp in float32;
//   clip     to [min_depth, max_depth], then to >= 1e-6, in float32;
//   metrics  float64 from here on: masked means over valid_mask, terms evaluated at masked pixels only (the host's np.where discards the
//            inf / nan of the others);
//   max_res  the fit samples columns only, ix = min(floor(dst * float32(1 / scale)), W - 1) for dst < fit_cols, every row
//            (eval_metrics._nearest_downscale); the metrics run at full resolution.
// Two memory-bound passes (9 bytes per pixel each) and two one-workgroup-per-image finalisers, stream-ordered, no host synchronisation, no
// atomics: every workgroup leaves one slab of float64 partial sums in the workspace and the finaliser adds the slabs in index order.  The
// number of workgroups per image and the pixel -> thread assignment depend on H * W alone -- never on B, on the image's position in the
// batch or on pointer alignment (which only selects 16-byte or scalar loads of the same four pixels) -- so an image's result is bitwise the
// same alone and inside any batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"

// The host's numpy code has no fused multiply-adds, so nothing below may be contracted into one.  The float32 recipe is written as plain
// `*`, `+`, `/` under this pragma: the __fmul_rn / __fadd_rn wrappers are plain operators compiled under the header's own (contracting)
// setting and fuse after inlining; float and double division are correctly rounded by default.
#pragma clang fp contract(off)

namespace {

constexpr int EV_NFIT = 5;                 // n, Sp, Sg, Spp, Spg
constexpr int EV_NMET = 11;                // n_valid, abs_rel, sq_rel, sq, dlog^2, |dlog10|, inv^2, dlog, delta1..3 counts
constexpr int EV_OUT = 14;                 // s, t, n_valid, n_fit, ten metrics

struct Quad { float p[4], g[4]; unsigned m; };  // four consecutive pixels; m: one mask byte per pixel (0 beyond the image)

// pixels 4q .. 4q + 3 of one image: one 16-byte load each of pred and gt and one 4-byte load of the mask when the image's three base
// addresses allow it (vec) and the quad is whole, scalar loads otherwise.  Same values, same order either way.
__device__ __forceinline__ Quad load_quad(const float* __restrict__ pred, const float* __restrict__ gt, const unsigned char* __restrict__ mask, long long q,
                                          long long hw, bool vec) {
    Quad r;
    const long long i0 = q * 4;
    if (vec && i0 + 4 <= hw) {
        const float4 p = *reinterpret_cast<const float4*>(pred + i0);
        const float4 g = *reinterpret_cast<const float4*>(gt + i0);
        r.m = *reinterpret_cast<const unsigned*>(mask + i0);
        r.p[0] = p.x, r.p[1] = p.y, r.p[2] = p.z, r.p[3] = p.w;
        r.g[0] = g.x, r.g[1] = g.y, r.g[2] = g.z, r.g[3] = g.w;
    } else {
        r.m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < hw;
            r.p[j] = in ? pred[i0 + j] : 0.f;
            r.g[j] = in ? gt[i0 + j] : 0.f;
            r.m |= in ? (unsigned)mask[i0 + j] << (8 * j) : 0u;
        }
    }
    return r;
}

struct FitAcc {
    unsigned n = 0;
    double sp = 0.0, sg = 0.0, spp = 0.0, spg = 0.0;
    __device__ __forceinline__ void add(float pf, float gf, bool valid, bool disparity) {
        if (!valid) return;
        if (disparity) {  // depth2disparity(gt) and the fit mask of eval.py:181-200
            if (!(gf > 0.f) || !(pf > 0.f)) return;
            gf = 1.0f / gf;
        }
        const double p = (double)pf, g = (double)gf;
        n += 1;
        sp += p;
        sg += g;
        spp += p * p;
        spg += p * g;
    }
};

// pass 1: the five sums of the normal equations over the fit mask.  grid (eval_blocks(H * W), B).  fit_cols > 0: column-subsampled fit.
__global__ __launch_bounds__(EV_THREADS) void eval_fit_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const unsigned char* __restrict__ mask, int H, int W, int disparity, int fit_cols,
                                                              float fit_inv_scale, double* __restrict__ ws) {
    const long long hw = (long long)H * W;
    const long long base = (long long)blockIdx.y * hw;
    pred += base, gt += base, mask += base;
    FitAcc acc;
    const long long tid = (long long)blockIdx.x * EV_THREADS + threadIdx.x, stride = (long long)gridDim.x * EV_THREADS;
    if (fit_cols > 0) {
        const long long n = (long long)H * fit_cols;
        const double inv = (double)fit_inv_scale;
        for (long long k = tid; k < n; k += stride) {
            const long long row = k / fit_cols;
            const int dst = (int)(k - row * fit_cols);
            long long ix = (long long)floor((double)dst * inv);
            ix = ix < 0 ? 0 : (ix > W - 1 ? W - 1 : ix);
            const long long i = row * W + ix;
            acc.add(pred[i], gt[i], mask[i] != 0, disparity != 0);
        }
    } else {
        const bool vec = (((uintptr_t)pred | (uintptr_t)gt) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
        const long long nq = (hw + 3) / 4;
        for (long long q = tid; q < nq; q += stride) {
            const Quad v = load_quad(pred, gt, mask, q, hw, vec);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc.add(v.p[j], v.g[j], ((v.m >> (8 * j)) & 0xffu) != 0, disparity != 0);
        }
    }
    double v[EV_NFIT] = {(double)acc.n, acc.sp, acc.sg, acc.spp, acc.spg};
    block_reduce_store<EV_NFIT>(v, ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * EV_NFIT);
}

// after pass 1: slabs in index order, 2 x 2 normal equations in float64, (s, t) rounded to float32 into out[b][0..1] (where pass 2 reads
// them), n_fit into out[b][3].  Fewer than two fit pixels or a singular system: s = t = NaN.  nblk = 0 (no alignment): s = 1, t = 0.
__global__ __launch_bounds__(64) void eval_fit_finalise_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ out) {
    __shared__ double s_sum[EV_NFIT];
    const int b = blockIdx.x;
    if (nblk == 0) {
        if (threadIdx.x == 0) out[(long long)b * EV_OUT] = 1.0, out[(long long)b * EV_OUT + 1] = 0.0, out[(long long)b * EV_OUT + 3] = 0.0;
        return;
    }
    if (threadIdx.x < EV_NFIT) s_sum[threadIdx.x] = sum_slabs<EV_NFIT>(ws + (long long)b * nblk * EV_NFIT, nblk, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = s_sum[0], sp = s_sum[1], sg = s_sum[2], spp = s_sum[3], spg = s_sum[4];
        const double det = n * spp - sp * sp;
        float s = __builtin_nanf(""), t = __builtin_nanf("");
        if (n >= 2.0 && det > 0.0) {
            s = (float)((n * spg - sp * sg) / det);
            t = (float)((spp * sg - sp * spg) / det);
        }
        out[(long long)b * EV_OUT] = (double)s;
        out[(long long)b * EV_OUT + 1] = (double)t;
        out[(long long)b * EV_OUT + 3] = n;
    }
}

struct MetAcc {
    unsigned n = 0, d1 = 0, d2 = 0, d3 = 0;
    double abs_rel = 0.0, sq_rel = 0.0, sq = 0.0, dlog2 = 0.0, dlog10 = 0.0, inv2 = 0.0, dlog = 0.0;
    // alignment.py:57-76 / eval.py:181-215 on one pixel in float32, then the terms of metric.py in float64
    __device__ __forceinline__ void add(float pf, float gf, bool valid, int alignment, float s, float t, float lo, float hi) {
        if (!valid) return;
        float al = pf;
        if (alignment != 0) {
            const float scaled = pf * s;  // two roundings
            al = scaled + t;
            if (alignment == 2) al = 1.0f / fmaxf(al, 1e-3f);  // clip the disparity at 1e-3, disparity2depth
        }
        al = fmaxf(fminf(fmaxf(al, lo), hi), 1e-6f);
        const double a = (double)al, g = (double)gf;
        const double diff = a - g, ad = fabs(diff);
        const double dl = log(a) - log(g);
        const double ia = 1.0 / a - 1.0 / g;
        const double r = fmax(a / g, g / a);
        n += 1;
        abs_rel += ad / g;
        sq_rel += ad * ad / g;
        sq += diff * diff;
        dlog2 += dl * dl;
        dlog10 += fabs(log10(a) - log10(g));
        inv2 += ia * ia;
        dlog += dl;
        d1 += r < 1.25 ? 1u : 0u;
        d2 += r < 1.25 * 1.25 ? 1u : 0u;
        d3 += r < 1.25 * 1.25 * 1.25 ? 1u : 0u;
    }
};

// pass 2: the metric sums over valid_mask with the (s, t) the fit finaliser left in out[b][0..1]
__global__ __launch_bounds__(EV_THREADS) void eval_metric_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const unsigned char* __restrict__ mask, int H, int W, int alignment, float lo, float hi,
                                                                 const double* __restrict__ out, double* __restrict__ ws) {
    const long long hw = (long long)H * W;
    const long long base = (long long)blockIdx.y * hw;
    pred += base, gt += base, mask += base;
    const float s = (float)out[(long long)blockIdx.y * EV_OUT], t = (float)out[(long long)blockIdx.y * EV_OUT + 1];
    MetAcc acc;
    const bool vec = (((uintptr_t)pred | (uintptr_t)gt) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const long long nq = (hw + 3) / 4;
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < nq; q += (long long)gridDim.x * EV_THREADS) {
        const Quad v = load_quad(pred, gt, mask, q, hw, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc.add(v.p[j], v.g[j], ((v.m >> (8 * j)) & 0xffu) != 0, alignment, s, t, lo, hi);
    }
    double v[EV_NMET] = {(double)acc.n, acc.abs_rel, acc.sq_rel, acc.sq, acc.dlog2, acc.dlog10, acc.inv2, acc.dlog,
                         (double)acc.d1, (double)acc.d2, (double)acc.d3};
    block_reduce_store<EV_NMET>(v, ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * EV_NMET);
}

// after pass 2: slabs in index order, then the ten values with the host's formulas, in eval_metrics.METRICS order
__global__ __launch_bounds__(64) void eval_metric_finalise_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ out) {
    __shared__ double s_sum[EV_NMET];
    const int b = blockIdx.x;
    if (threadIdx.x < EV_NMET) s_sum[threadIdx.x] = sum_slabs<EV_NMET>(ws + (long long)b * nblk * EV_NMET, nblk, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = out + (long long)b * EV_OUT;
        const double n = s_sum[0];
        o[2] = n;
        o[4] = s_sum[1] / n;                                         // abs_relative_difference
        o[5] = s_sum[2] / n;                                         // squared_relative_difference
        o[6] = sqrt(s_sum[3] / n);                                   // rmse_linear
        o[7] = sqrt(s_sum[4] / n);                                   // rmse_log
        o[8] = s_sum[5] / n;                                         // log10
        o[9] = s_sum[8] / n;                                         // delta1_acc
        o[10] = s_sum[9] / n;                                        // delta2_acc
        o[11] = s_sum[10] / n;                                       // delta3_acc
        o[12] = sqrt(s_sum[6] / n);                                  // i_rmse
        o[13] = sqrt(s_sum[4] / n - s_sum[7] * s_sum[7] / (n * n)) * 100.0;  // silog_rmse: sqrt(first - second) * 100
    }
}

// ---- surface normals (gp_eval_normal) ------------------------------------------------------------------------------------------------------
// The per-image quantity of eval_metrics.normal_angular_error -- the reference's angular_loss (genpercept/losses/geometry_losses.py:550-590)
// in float64, operation by operation -- for maps that are on the GPU, plus the exact median of the device's own angles:
//   angle    p, g = double(x) (decoded: double(x) * 2 - 1, eval_metrics.decode_normals); num = (p0 g0 + p1 g1) + p2 g2; |x| = sqrt((x0 x0 + x1 x1)
//            + x2 x2); den = max(|p|, 1e-8) max(|g|, 1e-8); ang = acos(min(max(num / den, -1 + 1e-4), 1 - 1e-4)); deg = ang * (180 / pi).
//            Products, sums, division and sqrt are correctly rounded on both sides, so acos sees the host's argument bit for bit.
//   sums     n, sum ang, sum deg, sum deg^2 and the three counts over the valid pixels, slabs as above.
//   median   the angle pass stores each angle's bit pattern (positive doubles order like their patterns; invalid pixels: all ones, never
//            counted) and a radix select walks the key from the top: six digits (five of 11 bits, one of 9), per digit one histogram pass
//            (integer LDS atomics, one slab of counts per workgroup) and one pick kernel per image that adds the slabs, finds the bucket of
//            rank (n - 1) / 2 and of rank n / 2 and extends their prefixes.  The two prefixes may diverge at any digit; from then on each has
//            its own histogram.  Integer sums do not depend on their order, so the result is bitwise reproducible and batch-independent.
// 14 launches for every B; nothing is read back.
constexpr int EN_NSUM = 7;        // n, sum ang, sum deg, sum deg^2, counts < 11.25, < 22.5, < 30
constexpr int EN_OUT = 8;         // n_valid, mean_rad, mean_deg, median_deg, rmse_deg, within_11.25, within_22.5, within_30
constexpr int EN_BINS = 2048;     // 11-bit digits
constexpr int EN_PASSES = 6;      // 5 x 11 + 9 = 64 key bits
constexpr int EN_STATE = 4;       // per image: prefix of rank (n-1)/2, prefix of rank n/2, the two remaining ranks (low | high 32 bits), active
constexpr int EN_PICK_THREADS = 1024;
constexpr int EN_PICK_GROUPS = EN_PICK_THREADS / 256;
constexpr unsigned long long EN_INVALID_KEY = ~0ull;

__host__ __device__ constexpr int en_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
__host__ __device__ constexpr int en_width(int pass) { return pass < 5 ? 11 : 9; }

struct NormalWs {  // carving of the workspace: every part a multiple of 8 bytes and proportional to B
    long long keys, slabs, hist, state, total;  // byte offsets
};
NormalWs normal_ws(long long B, long long hw) {
    const long long nblk = eval_blocks(hw);
    NormalWs w;
    w.keys = 0;
    w.slabs = w.keys + B * hw * 8;
    w.hist = w.slabs + B * nblk * EN_NSUM * 8;
    w.state = w.hist + B * nblk * 2 * EN_BINS * 4;
    w.total = w.state + B * EN_STATE * 8;
    return w;
}

// four consecutive values of one channel plane (0 beyond the image): one 16-byte load when the plane's base allows it and the quad is whole
__device__ __forceinline__ void load_plane_quad(const float* __restrict__ plane, long long i0, long long hw, float (&v)[4]) {
    if (((uintptr_t)plane & 15) == 0 && i0 + 4 <= hw) {
        const float4 x = *reinterpret_cast<const float4*>(plane + i0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < hw ? plane[i0 + j] : 0.f;
    }
}

// angle pass: grid (eval_blocks(H * W), B).  keys: [B][H * W] bit patterns; angles_out: optional [B][H * W] radians, NaN where invalid.
__global__ __launch_bounds__(EV_THREADS) void normal_angle_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  const unsigned char* __restrict__ mask, long long hw, int decode,
                                                                  unsigned long long* __restrict__ keys, double* __restrict__ angles_out,
                                                                  double* __restrict__ ws) {
    const long long b = blockIdx.y;
    pred += b * 3 * hw, gt += b * 3 * hw, keys += b * hw;
    if (mask) mask += b * hw;
    if (angles_out) angles_out += b * hw;
    const bool mvec = mask && ((uintptr_t)mask & 3) == 0;
    const bool dp = (decode & 1) != 0, dg = (decode & 2) != 0;
    const double lo = -1.0 + 1e-4, hi = 1.0 - 1e-4, to_deg = 180.0 / 3.141592653589793;
    unsigned n = 0, c11 = 0, c22 = 0, c30 = 0;
    double sa = 0.0, sd = 0.0, sdd = 0.0;
    const long long nq = (hw + 3) / 4;
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < nq; q += (long long)gridDim.x * EV_THREADS) {
        const long long i0 = q * 4;
        float pf[3][4], gf[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            load_plane_quad(pred + c * hw, i0, hw, pf[c]);
            load_plane_quad(gt + c * hw, i0, hw, gf[c]);
        }
        unsigned m = 0;
        if (mask) {
            if (mvec && i0 + 4 <= hw) {
                m = *reinterpret_cast<const unsigned*>(mask + i0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) m |= i0 + j < hw ? (unsigned)mask[i0 + j] << (8 * j) : 0u;
            }
        } else {  // base_dataset.py:416-418: (normal != 0).any(dim=0) on the stored ground truth
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= (i0 + j < hw && (gf[0][j] != 0.f || gf[1][j] != 0.f || gf[2][j] != 0.f)) ? 1u << (8 * j) : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= hw) break;
            const bool valid = ((m >> (8 * j)) & 0xffu) != 0;
            double ang = __builtin_nan("");
            if (valid) {
                double p[3], g[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[c] = (double)pf[c][j], g[c] = (double)gf[c][j];
                    if (dp) p[c] = p[c] * 2.0 - 1.0;
                    if (dg) g[c] = g[c] * 2.0 - 1.0;
                }
                const double num = (p[0] * g[0] + p[1] * g[1]) + p[2] * g[2];
                const double np_ = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
                const double ng_ = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
                const double den = fmax(np_, 1e-8) * fmax(ng_, 1e-8);
                ang = acos(fmin(fmax(num / den, lo), hi));
                const double deg = ang * to_deg;
                n += 1;
                sa += ang;
                sd += deg;
                sdd += deg * deg;
                c11 += deg < 11.25 ? 1u : 0u;
                c22 += deg < 22.5 ? 1u : 0u;
                c30 += deg < 30.0 ? 1u : 0u;
            }
            keys[i0 + j] = valid ? (unsigned long long)__double_as_longlong(ang) : EN_INVALID_KEY;
            if (angles_out) angles_out[i0 + j] = ang;
        }
    }
    double v[EN_NSUM] = {(double)n, sa, sd, sdd, (double)c11, (double)c22, (double)c30};
    block_reduce_store<EN_NSUM>(v, ws + (b * gridDim.x + blockIdx.x) * EN_NSUM);
}

// after the angle pass: slabs in index order, the seven values that need no order statistic, and the state the selection starts from.
// n = 0: seven NaN and an inactive state -- the selection kernels then do nothing for this image.
__global__ __launch_bounds__(64) void normal_finalise_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ out,
                                                             unsigned long long* __restrict__ state) {
    __shared__ double s_sum[EN_NSUM];
    const int b = blockIdx.x;
    if (threadIdx.x < EN_NSUM) s_sum[threadIdx.x] = sum_slabs<EN_NSUM>(ws + (long long)b * nblk * EN_NSUM, nblk, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = out + (long long)b * EN_OUT;
        unsigned long long* st = state + (long long)b * EN_STATE;
        const double n = s_sum[0];
        o[0] = n;
        st[0] = 0, st[1] = 0;
        if (n > 0.0) {
            o[1] = s_sum[1] / n;
            o[2] = s_sum[2] / n;
            o[3] = __builtin_nan("");  // the last pick kernel writes the median
            o[4] = sqrt(s_sum[3] / n);
            o[5] = s_sum[4] / n;
            o[6] = s_sum[5] / n;
            o[7] = s_sum[6] / n;
            const unsigned long long cnt = (unsigned long long)n;
            st[2] = ((cnt - 1) / 2) | ((cnt / 2) << 32);
            st[3] = 1;
        } else {
            for (int k = 1; k < EN_OUT; ++k) o[k] = __builtin_nan("");
            st[2] = 0, st[3] = 0;
        }
    }
}

// one digit of the selection: per workgroup the counts of the digit among the keys that carry the prefix of rank (n-1)/2 (histogram 0) and,
// once the prefixes differ, of rank n/2 (histogram 1).  grid (eval_blocks(H * W), B); slabs: [B][nblk][2][EN_BINS].
__global__ __launch_bounds__(EV_THREADS) void normal_hist_kernel(const unsigned long long* __restrict__ keys, long long hw, int pass,
                                                                 const unsigned long long* __restrict__ state, unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[2][EN_BINS];
    const long long b = blockIdx.y;
    const unsigned long long* st = state + b * EN_STATE;
    if (st[3] == 0) return;  // no valid pixel: no rank
    const unsigned long long p0 = st[0], p1 = st[1];
    const bool two = p0 != p1;
    for (int k = threadIdx.x; k < 2 * EN_BINS; k += EV_THREADS) (&s_h[0][0])[k] = 0;
    __syncthreads();
    keys += b * hw;
    const int shift = en_shift(pass), width = en_width(pass);
    const unsigned dmask = (1u << width) - 1u;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < hw; i += 4 * stride) {
        unsigned long long k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = i + u * stride < hw ? keys[i + u * stride] : EN_INVALID_KEY;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (k[u] == EN_INVALID_KEY) continue;
            const unsigned long long top = pass == 0 ? 0ull : k[u] >> (shift + width);
            const unsigned d = (unsigned)(k[u] >> shift) & dmask;
            if (top == p0) atomicAdd(&s_h[0][d], 1u);
            if (two && top == p1) atomicAdd(&s_h[1][d], 1u);
        }
    }
    __syncthreads();
    unsigned* slab = hist + (b * gridDim.x + blockIdx.x) * (2 * EN_BINS);
    const int nwrite = two ? 2 * EN_BINS : EN_BINS;
    for (int k = threadIdx.x; k < nwrite; k += EV_THREADS) slab[k] = (&s_h[0][0])[k];
}

// after a histogram pass, one workgroup per image: add the slabs (thread t of each of the four groups owns bins 8t .. 8t + 7 of every fourth
// slab), find for each rank the bucket that holds it, extend the prefix and make the rank relative to the bucket.  The last digit completes the
// two keys: median = (lo * (180 / pi) + hi * (180 / pi)) / 2, np.median's rule for the degrees.
__global__ __launch_bounds__(EN_PICK_THREADS) void normal_pick_kernel(const unsigned* __restrict__ hist, int nblk, int pass,
                                                                      unsigned long long* __restrict__ state, double* __restrict__ out) {
    __shared__ unsigned s_cnt[EN_PICK_GROUPS][EN_BINS];
    __shared__ unsigned s_bin[2], s_rank[2];
    const long long b = blockIdx.x;
    unsigned long long* st = state + b * EN_STATE;
    if (st[3] == 0) return;
    const unsigned long long p[2] = {st[0], st[1]};
    const unsigned rank[2] = {(unsigned)(st[2] & 0xffffffffull), (unsigned)(st[2] >> 32)};
    const bool two = p[0] != p[1];
    const int t = threadIdx.x & 255, grp = threadIdx.x >> 8;
    const int width = en_width(pass), nbins = 1 << width;
    if (threadIdx.x < 2) s_bin[threadIdx.x] = 0, s_rank[threadIdx.x] = 0;
    for (int h = 0; h < (two ? 2 : 1); ++h) {
        unsigned c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 8  // (independent loads, integer sums)
        for (int j = grp; j < nblk; j += EN_PICK_GROUPS) {
            const uint2* s = reinterpret_cast<const uint2*>(hist + ((b * nblk + j) * 2 + h) * EN_BINS + 8 * t);  // (the workspace is 8-byte aligned)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint2 a = s[k];
                c[2 * k] += a.x, c[2 * k + 1] += a.y;
            }
        }
        __syncthreads();  // (second histogram: the scan below has finished with s_cnt)
#pragma unroll
        for (int k = 0; k < 8; ++k) s_cnt[grp][8 * t + k] = c[k];
        __syncthreads();
        for (int k = threadIdx.x; k < EN_BINS; k += EN_PICK_THREADS) {
            unsigned a = s_cnt[0][k];
#pragma unroll
            for (int g = 1; g < EN_PICK_GROUPS; ++g) a += s_cnt[g][k];
            s_cnt[0][k] = a;
        }
        __syncthreads();
        if (threadIdx.x < 64) {  // wave 0: lane l owns bins [l * per, (l + 1) * per), an inclusive scan of the lane totals, then a walk
            const int per = nbins / 64, lane = threadIdx.x;
            unsigned mine = 0;
            for (int k = 0; k < per; ++k) mine += s_cnt[0][lane * per + k];
            unsigned incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            const unsigned excl = incl - mine;
            for (int r = 0; r < 2; ++r) {
                if (two ? r != h : false) continue;
                const unsigned want = rank[r];
                if (want >= excl && want < incl) {
                    unsigned before = excl;
                    int k = 0;
                    for (; k < per - 1; ++k) {
                        const unsigned cb = s_cnt[0][lane * per + k];
                        if (want < before + cb) break;
                        before += cb;
                    }
                    s_bin[r] = (unsigned)(lane * per + k);
                    s_rank[r] = want - before;
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long k0 = (p[0] << width) | s_bin[0], k1 = (p[1] << width) | s_bin[1];
        st[0] = k0, st[1] = k1;
        st[2] = (unsigned long long)s_rank[0] | ((unsigned long long)s_rank[1] << 32);
        if (pass == EN_PASSES - 1) {
            const double to_deg = 180.0 / 3.141592653589793;
            const double lo = __longlong_as_double((long long)k0) * to_deg, hi = __longlong_as_double((long long)k1) * to_deg;
            out[b * EN_OUT + 3] = (lo + hi) / 2.0;
        }
    }
}

// ---- dis / matting (gp_eval_mask) -----------------------------------------------------------------------------------------------------------
// The reference has no metric for these modes; the header defines them and eval_metrics.mask_counts / mask_metrics_from_counts restate them on
// the host.  Everything is a function of integer counts over the 8-bit prediction q = (unsigned char)(clamp(x, 0, 1) * 255.0f) (the byte
// quantize_kernel writes, run.py:449-455) and the 8-bit ground truth g:
//   counts   n, sum q, sum |q - g|, sum (q - g)^2 and two 256-bin histograms of q, one per class of g (g <= 128, g > 128), over the region.
//            One pass: per-lane integer sums, histograms by integer LDS atomics into one copy per wave.  Real masks are almost all 0 and 255, and
//            64 lanes adding to one LDS word serialise, so those two bins are counted per class with a ballot and a population count -- a
//            wave-uniform register, one LDS add per wave and bin at the end -- and only the other lanes issue atomics.  One slab per workgroup,
//            no global atomics.  Integer sums do not depend on their order: the pixel -> thread assignment may depend on pointer alignment here.
//   values   one workgroup per image adds the slabs, turns the histograms into suffix sums with one LDS scan (TP_t, P_t for the 256 thresholds
//            "q >= t"), thread t evaluates F_t, thread 0 does the left-to-right sum, the first-maximum search and the scalar values.  Each value
//            is one fixed sequence of correctly rounded float64 *, /, + on the integers (this file contracts nothing), so the host's float64
//            restatement is bit-equal.
// Two launches for every B; nothing is read back.
constexpr int EM_BINS = EV_BINS;
constexpr int EM_NSUM = 4;                        // n, sum_q, sad, sse
constexpr int EM_COUNTS = EM_NSUM + 2 * EM_BINS;  // a row of counts_out: the four sums, hist_bg, hist_fg
constexpr int EM_OUT = 10;                        // n, n_fg, mae, mse, sad, max_f, mean_f, adp_f, iou, t_max
constexpr int EM_UNROLL = 2;                      // quads in flight per lane (4: the ballot masks of an iteration no longer fit the SGPRs)
// a slab: the four sums as 64-bit, the 512 bins as 32-bit (an image has fewer than 2^31 pixels)
constexpr long long EM_SLAB_BYTES = class_slab_bytes(EM_NSUM);

struct MaskAcc {
    unsigned n = 0, q4 = 0, ad4 = 0, sq4 = 0;  // per lane; q4, ad4, sq4: the sums of at most four pixels, flushed into the 64-bit ones
    u64 sum_q = 0, sad = 0, sse = 0;           // per lane
    // one pixel; every lane of the wave calls this together (`in`: the pixel exists and is inside the region)
    __device__ __forceinline__ void add(unsigned q, unsigned g, bool in, ClassHist& hist) {
        const unsigned d = in ? max(q, g) - min(q, g) : 0u;
        n += in ? 1u : 0u;
        q4 += in ? q : 0u;
        ad4 += d;
        sq4 += d * d;
        hist.add(q, g > 128u, in);
    }
    __device__ __forceinline__ void flush() {
        sum_q += q4, sad += ad4, sse += sq4;
        q4 = ad4 = sq4 = 0;
    }
};

// grid (eval_blocks(H * W), B).  pred: float (quantised here) or, U8, bytes.  Pixels [head, head + 4 nq) of an image go as quads -- one 16-byte
// load of pred (4 bytes for U8), 4 bytes of gt and of region per lane --, the up to three before and after them one by one; head is the
// distance of the gt plane from a 4-byte boundary, and the quads are taken only when the same head aligns pred and region too (it does for
// the planes of one allocation each: plane i starts i * H * W elements in), otherwise every pixel goes the scalar way.
template <bool U8>
__global__ __launch_bounds__(EV_THREADS) void mask_count_kernel(const void* __restrict__ pred_v, const unsigned char* __restrict__ gt,
                                                                const unsigned char* __restrict__ region, long long hw, char* __restrict__ ws) {
    const long long b = blockIdx.y;
    const Pred8<U8> pred(pred_v, b * hw);
    gt += b * hw;
    if (region) region += b * hw;
    ClassHist hist;

    const long long head = (long long)((4 - ((uintptr_t)gt & 3)) & 3);
    const bool vec = head <= hw && pred.quad_aligned(head) && (!region || ((uintptr_t)(region + head) & 3) == 0);
    const QuadSplit sp(hw, vec ? head : hw);
    const long long stride = (long long)gridDim.x * EV_THREADS;
    MaskAcc acc;
    // (both loops have workgroup-uniform bounds: the ballots inside add() see whole waves)
    for (long long q0 = (long long)blockIdx.x * EV_THREADS; q0 < sp.nq; q0 += EM_UNROLL * stride) {
        float4 pf[EM_UNROLL];
        unsigned pb[EM_UNROLL], g4[EM_UNROLL], r4[EM_UNROLL];
        bool act[EM_UNROLL];
#pragma unroll
        for (int u = 0; u < EM_UNROLL; ++u) {
            const long long q = q0 + u * stride + threadIdx.x;
            act[u] = q < sp.nq;
            pf[u] = make_float4(0.f, 0.f, 0.f, 0.f), pb[u] = 0, g4[u] = 0, r4[u] = 0x01010101u;
            if (act[u]) {
                const long long i0 = sp.quad(q);
                if (U8) pb[u] = *reinterpret_cast<const unsigned*>(pred.u + i0);
                else pf[u] = *reinterpret_cast<const float4*>(pred.f + i0);
                g4[u] = *reinterpret_cast<const unsigned*>(gt + i0);
                if (region) r4[u] = *reinterpret_cast<const unsigned*>(region + i0);
            }
        }
#pragma unroll
        for (int u = 0; u < EM_UNROLL; ++u) {
            const float f[4] = {pf[u].x, pf[u].y, pf[u].z, pf[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned q = U8 ? (pb[u] >> (8 * j)) & 0xffu : quantise8(f[j]);
                acc.add(q, (g4[u] >> (8 * j)) & 0xffu, act[u] && ((r4[u] >> (8 * j)) & 0xffu) != 0, hist);
            }
            acc.flush();
        }
    }
    for (long long k0 = (long long)blockIdx.x * EV_THREADS; k0 < sp.ns; k0 += stride) {
        const long long k = k0 + threadIdx.x;
        const bool act = k < sp.ns;
        unsigned q = 0, g = 0;
        bool in = false;
        if (act) {
            const long long i = sp.scalar(k);
            q = pred[i];
            g = gt[i];
            in = region ? region[i] != 0 : true;
        }
        acc.add(q, g, in, hist);
        acc.flush();
    }
    hist.flush();
    u64 v[EM_NSUM] = {acc.n, acc.sum_q, acc.sad, acc.sse};
    const u64 a = block_sum(v);  // (its barrier: every wave's histogram is complete)
    char* slab = ws + (b * gridDim.x + blockIdx.x) * EM_SLAB_BYTES;
    if (threadIdx.x < EM_NSUM) reinterpret_cast<u64*>(slab)[threadIdx.x] = a;
    hist.store(reinterpret_cast<unsigned*>(slab + EM_NSUM * 8));
}

// one workgroup per image: sum_class_slabs, then thread i < 512 owns bin i, and thread t < 256 threshold t.
__global__ __launch_bounds__(EV_FIN_THREADS) void mask_finalise_kernel(const char* __restrict__ ws, int nblk, double* __restrict__ out,
                                                                       u64* __restrict__ counts_out) {
    __shared__ u64 s_cnt[EV_FIN_GROUPS][2 * EM_BINS], s_sum[EM_NSUM];
    __shared__ double s_f[EM_BINS];
    u64* s_bg = s_cnt[0];
    u64* s_fg = s_cnt[0] + EM_BINS;
    const long long b = blockIdx.x;
    const int t = threadIdx.x & (EM_BINS - 1);
    const bool first = threadIdx.x < EM_BINS, owner = threadIdx.x < 2 * EM_BINS;
    const u64 bin = sum_class_slabs<EM_NSUM>(ws + b * nblk * EM_SLAB_BYTES, nblk, s_cnt, s_sum);
    if (counts_out && threadIdx.x < EM_NSUM) counts_out[b * EM_COUNTS + threadIdx.x] = s_sum[threadIdx.x];
    if (owner) {  // bin threadIdx.x of [hist_bg | hist_fg]
        if (counts_out) counts_out[b * EM_COUNTS + EM_NSUM + threadIdx.x] = bin;
        s_cnt[0][threadIdx.x] = bin;  // (its own column)
    }
    __syncthreads();
    for (int off = 1; off < EM_BINS; off <<= 1) {  // inclusive suffix sums inside each histogram: s_x[t] = sum_{v >= t} hist_x[v]
        unsigned long long a = 0;
        if (owner && t + off < EM_BINS) a = s_cnt[0][threadIdx.x + off];
        __syncthreads();
        if (owner) s_cnt[0][threadIdx.x] += a;
        __syncthreads();
    }
    const unsigned long long n = s_sum[0], n_fg = s_fg[0];
    if (first) {
        const unsigned long long tp = s_fg[t], p = tp + s_bg[t];
        const double prec = (double)tp / (double)(p > 1 ? p : 1ull), rec = (double)tp / (double)(n_fg > 1 ? n_fg : 1ull);
        const double den = 0.3 * prec + rec;
        s_f[t] = den == 0.0 ? 0.0 : ((1.3 * prec) * rec) / den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = out + b * EM_OUT;
        o[0] = (double)n, o[1] = (double)n_fg;
        if (n == 0) {
            for (int k = 2; k < EM_OUT; ++k) o[k] = __builtin_nan("");
            return;
        }
        const unsigned long long sum_q = s_sum[1], sad = s_sum[2], sse = s_sum[3];
        const double dn = (double)n;
        o[2] = (double)sad / (255.0 * dn);
        o[3] = (double)sse / (65025.0 * dn);
        o[4] = (double)sad / 255000.0;
        double sum = s_f[0], best = s_f[0];
        int t_best = 0;
        for (int k = 1; k < EM_BINS; ++k) {
            const double f = s_f[k];
            sum += f;
            if (f > best) best = f, t_best = k;
        }
        o[5] = best;
        o[6] = sum / 256.0;
        const unsigned long long cap = 255ull * n, twice = 2ull * sum_q;
        const unsigned long long t_a = ((twice < cap ? twice : cap) + n - 1) / n;  // the smallest t with t * n >= min(2 sum_q, 255 n)
        o[7] = s_f[t_a];
        const unsigned long long tp = s_fg[128], p = tp + s_bg[128], uni = p + n_fg - tp;
        o[8] = uni == 0 ? 0.0 : (double)tp / (double)uni;
        o[9] = (double)t_best;
    }
}

}  // namespace

extern "C" {

long long gp_eval_depth_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return (long long)B * eval_blocks((long long)H * W) * EV_NMET * (long long)sizeof(double);
}

gp_status gp_eval_depth(const float* pred, const float* gt, const unsigned char* mask, int B, int H, int W, int alignment, int fit_cols,
                        float fit_inv_scale, float min_depth, float max_depth, double* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!pred || !gt || !mask || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W)) return GP_ERR_INVALID;
    if (alignment < 0 || alignment > 2 || fit_cols < 0 || fit_cols > W || (fit_cols > 0 && !(fit_inv_scale > 0.f))) return GP_ERR_INVALID;
    if (workspace_bytes < gp_eval_depth_workspace(B, H, W) || !eval_aligned8(workspace, out)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    double* ws = (double*)workspace;
    const int nblk = eval_blocks((long long)H * W);
    if (alignment != 0)
        hipLaunchKernelGGL(eval_fit_kernel, dim3(nblk, B), dim3(EV_THREADS), 0, s, pred, gt, mask, H, W, alignment == 2 ? 1 : 0, fit_cols, fit_inv_scale, ws);
    hipLaunchKernelGGL(eval_fit_finalise_kernel, dim3(B), dim3(64), 0, s, (const double*)ws, alignment != 0 ? nblk : 0, out);
    hipLaunchKernelGGL(eval_metric_kernel, dim3(nblk, B), dim3(EV_THREADS), 0, s, pred, gt, mask, H, W, alignment, min_depth, max_depth, (const double*)out, ws);
    hipLaunchKernelGGL(eval_metric_finalise_kernel, dim3(B), dim3(64), 0, s, (const double*)ws, nblk, out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

long long gp_eval_normal_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return normal_ws(B, (long long)H * W).total;
}

gp_status gp_eval_normal(const float* pred, const float* gt, const unsigned char* mask, int B, int H, int W, int decode, double* out,
                         double* angles_out, void* workspace, long long workspace_bytes, void* stream) {
    if (!pred || !gt || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W)) return GP_ERR_INVALID;
    if (decode < 0 || decode > 3 || (!mask && (decode & 2) != 0)) return GP_ERR_INVALID;
    if (!eval_aligned8(workspace, out, angles_out)) return GP_ERR_INVALID;
    const long long hw = (long long)H * W;
    const NormalWs w = normal_ws(B, hw);
    if (workspace_bytes < w.total) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)workspace;
    unsigned long long* keys = (unsigned long long*)(base + w.keys);
    double* slabs = (double*)(base + w.slabs);
    unsigned* hist = (unsigned*)(base + w.hist);
    unsigned long long* state = (unsigned long long*)(base + w.state);
    const int nblk = eval_blocks(hw);
    hipLaunchKernelGGL(normal_angle_kernel, dim3(nblk, B), dim3(EV_THREADS), 0, s, pred, gt, mask, hw, decode, keys, angles_out, slabs);
    hipLaunchKernelGGL(normal_finalise_kernel, dim3(B), dim3(64), 0, s, (const double*)slabs, nblk, out, state);
    for (int pass = 0; pass < EN_PASSES; ++pass) {
        hipLaunchKernelGGL(normal_hist_kernel, dim3(nblk, B), dim3(EV_THREADS), 0, s, (const unsigned long long*)keys, hw, pass,
                           (const unsigned long long*)state, hist);
        hipLaunchKernelGGL(normal_pick_kernel, dim3(B), dim3(EN_PICK_THREADS), 0, s, (const unsigned*)hist, nblk, pass, state, out);
    }
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

long long gp_eval_mask_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return (long long)B * eval_blocks((long long)H * W) * EM_SLAB_BYTES;
}

gp_status gp_eval_mask(const void* pred, int pred_is_u8, const unsigned char* gt, const unsigned char* region, int B, int H, int W, double* out,
                       unsigned long long* counts_out, void* workspace, long long workspace_bytes, void* stream) {
    if (!pred || !gt || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W)) return GP_ERR_INVALID;
    if (!eval_pred_ok(pred, pred_is_u8) || !eval_aligned8(workspace, out, counts_out)) return GP_ERR_INVALID;
    if (workspace_bytes < gp_eval_mask_workspace(B, H, W)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W;
    const int nblk = eval_blocks(hw);
    char* ws = (char*)workspace;
    const auto count = pred_is_u8 ? mask_count_kernel<true> : mask_count_kernel<false>;
    hipLaunchKernelGGL(count, dim3(nblk, B), dim3(EV_THREADS), 0, s, pred, gt, region, hw, ws);
    hipLaunchKernelGGL(mask_finalise_kernel, dim3(B), dim3(EV_FIN_THREADS), 0, s, (const char*)ws, nblk, out, counts_out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
