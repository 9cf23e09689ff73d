// Contract-precision mode (gp_set_precision(e, GP_PREC_CONTRACT); the Python pipeline selects it for torch_dtype=float32, the reference's
// default: run.py:273-281): the build that meets north_star's "within 1e-3 rel of the reference" under BOTH readings.
//
//   * every activation that is STORED (residual trunk, skip stack, GroupNorm / LayerNorm inputs, attention logits, GEMM outputs) is fp32;
//   * every matrix product runs on the bf16 matrix cores with SPLIT operands:  x = x_hi + x_lo,  x_hi = bf16(x),  x_lo = bf16(x - x_hi)
//     (2^-17 relative), and  x.w ~= x_hi w_hi + x_lo w_hi + x_hi w_lo  (the dropped x_lo w_lo term is 2^-18 relative), fp32 accumulation.
//     The three products are ONE launch of the ordinary MFMA kernels over a tripled K: the A operand is laid out as channel blocks
//     [hi | lo | hi] ("A order"), the B operand (weights, keys, values) as [hi | hi | lo] ("B order"), so the kernels' inner loops, rings
//     and swizzles are untouched and the accumulator never leaves fp32.
//
// This file holds the kernels that sit BETWEEN the matrix products in that mode and exist in no other: fp32 in, split-bf16 (or statistics) out.
// They are written for exactness and simplicity (all HBM-bound, one read and one write of their tensor), not for the last 10 %.  The layout and
// pointwise kernels with fp32 in AND out (concat, add, bilinear, the layout changes, ddim, decode epilogue, ...) are the float instantiations of
// elementwise.hip's templates.
// Reference call sites: genpercept_pipeline.py:399-526 (single_infer / encode_rgb / decode_pred), custom_unet.py:305-415, dpt_head.py:213-335.
#include "common.h"
#include "kernels.h"

static inline unsigned cgrid(long long n, int per_block = 256) {
    long long g = (n + per_block - 1) / per_block;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// 8 fp32 values -> 8 hi elements + 8 lo elements (round-to-nearest-even both times)
GP_DEV void split8(const float (&v)[8], uint4& hi, uint4& lo) {
    unsigned h[4], l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = pack_h16x2(v[2 * k], v[2 * k + 1]);
        l[k] = pack_h16x2(v[2 * k] - h16_lo(h[k]), v[2 * k + 1] - h16_hi(h[k]));
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}
// store one 8-channel group of a split row: A order [hi | lo | hi], B order [hi | hi | lo]; blk = elements per block (the logical width)
GP_DEV void store_split8(h16_t* row, int col, int blk, int b_order, const float (&v)[8]) {
    uint4 hi, lo;
    split8(v, hi, lo);
    *(uint4*)(row + col) = hi;
    *(uint4*)(row + blk + col) = b_order ? hi : lo;
    *(uint4*)(row + 2 * blk + col) = b_order ? lo : hi;
}
GP_DEV void load8(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
GP_DEV void store8(float* p, const float (&v)[8]) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- plain split: out[r] = split(act(x[r][0..C) * scale)) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void c_split3_kernel(const float* __restrict__ x, int ldx, h16_t* __restrict__ out, long long rows, int C,
                                                        int b_order, int act, float scale) {
    const int nv = C >> 3;
    const long long n = rows * nv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / nv;
        const int c = (int)(i - r * nv) * 8;
        float v[8];
        load8(x + r * ldx + c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] *= scale;
            if (act == GP_ACT_RELU) v[e] = fmaxf(v[e], 0.f);
            else if (act == GP_ACT_SILU) v[e] = silu_f(v[e]);
        }
        store_split8(out + r * 3 * C, c, C, b_order, v);
    }
}
void launch_c_split3(const float* x, int ldx, h16_t* out, long long rows, int C, int b_order, int act, float scale, hipStream_t s) {
    hipLaunchKernelGGL(c_split3_kernel, dim3(cgrid(rows * (C / 8))), dim3(256), 0, s, x, ldx, out, rows, C, b_order, act, scale);
}

// ---- RGB [B][3][H][W] (uint8, or float already in [-1, 1]) -> split NHWC with 64 logical channels (3 real), A order ---------------------
// (x / 255 * 2 - 1 in that operation order: genpercept_pipeline.py:245)
__global__ __launch_bounds__(256) void c_rgb_split_kernel(const void* __restrict__ rgb, int is_u8, h16_t* __restrict__ out, int B, long long HW) {
    const long long n = (long long)B * HW * 8;  // 8 groups of 8 channels per pixel
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long px = i >> 3;
        const int g = (int)(i & 7);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (g == 0) {
            const long long b = px / HW, p = px - b * HW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long src = (b * 3 + c) * HW + p;
                v[c] = is_u8 ? ((float)((const unsigned char*)rgb)[src] / 255.0f * 2.0f - 1.0f) : ((const float*)rgb)[src];
            }
        }
        store_split8(out + px * 192, g * 8, 64, 0, v);
    }
}
void launch_c_rgb_split(const void* rgb, int is_u8, h16_t* out, int B, int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(c_rgb_split_kernel, dim3(cgrid((long long)B * H * W * 8)), dim3(256), 0, s, rgb, is_u8, out, B, (long long)H * W);
}

// ---- GroupNorm statistics of an fp32 NHWC tensor: per (row of `bm` consecutive pixels, channel) {sum, M2}, M2 = sum (x - row mean)^2 the
// CENTRED second moment, in the "mode 3" layout of gn_finalize_tiles_kernel (norm.hip): [B][R][C][2] partials followed by [B][R] pixel counts
// (the last row of an image may be short).  Two passes over the row (the second one is L2-hot): a single-pass {sum, sum of squares} loses
// eps * (mean / std)^2 of the variance to cancellation (2e-4 relative at mean / std = 100), the centred form does not.  A thread owns one
// 4-channel vector and every TY-th pixel of the row; the TY partials meet in LDS in a fixed order: deterministic. ---------------------------
__global__ __launch_bounds__(256) void c_gn_stats_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int C, int bm, int R, int TX) {
    __shared__ float red[256 * 4];
    __shared__ float mu[256 * 4];
    const int r = blockIdx.x, b = blockIdx.y, vb = blockIdx.z;
    const int TY = 256 / TX, tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int nv = C >> 2, v = vb * TX + tx;
    const int p0 = r * bm, cnt = min(bm, HW - p0);
    const float* xp = x + ((long long)b * HW + p0) * C + v * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
    if (v < nv) {
        for (int p = ty; p < cnt; p += TY) {
            const float4 a = *(const float4*)(xp + (long long)p * C);
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[threadIdx.x * 4 + e] = s[e];
    __syncthreads();
    if (ty == 0 && v < nv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            for (int k = 0; k < TY; ++k) ss[e] += red[(k * TX + tx) * 4 + e];
            mu[tx * 4 + e] = ss[e] / (float)cnt;
        }
    }
    __syncthreads();
    if (v < nv) {
        const float m[4] = {mu[tx * 4], mu[tx * 4 + 1], mu[tx * 4 + 2], mu[tx * 4 + 3]};
        for (int p = ty; p < cnt; p += TY) {
            const float4 a = *(const float4*)(xp + (long long)p * C);
            const float d[4] = {a.x - m[0], a.y - m[1], a.z - m[2], a.w - m[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] += d[e] * d[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[threadIdx.x * 4 + e] = q[e];
    __syncthreads();
    if (ty == 0 && v < nv) {
        float* o = part + (((long long)b * R + r) * C + v * 4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float qq = 0.f;
            for (int k = 0; k < TY; ++k) qq += red[(k * TX + tx) * 4 + e];
            o[2 * e] = ss[e];
            o[2 * e + 1] = qq;
        }
    }
    if (threadIdx.x == 0 && vb == 0) part[(long long)gridDim.y * R * C * 2 + (long long)b * R + r] = (float)cnt;
}
// rows per image launch_c_gn_stats writes (the caller allocates B * R * (2 C + 1) floats)
int c_gn_stat_rows(int HW, int C, int* bm_out) {
    // ~16 K elements per workgroup pass, at least 8 and at most 1024 pixels per row
    int bm = 16384 / (C > 0 ? C : 1) * 4;
    if (bm < 8) bm = 8;
    if (bm > 1024) bm = 1024;
    if (bm > HW) bm = HW;
    if (bm_out) *bm_out = bm;
    return (HW + bm - 1) / bm;
}
void launch_c_gn_stats(const float* x, float* part, int B, int HW, int C, hipStream_t s) {
    int bm = 0;
    const int R = c_gn_stat_rows(HW, C, &bm);
    const int nv = C >> 2;
    int TX = 16;
    while (TX < nv && TX < 256) TX <<= 1;
    hipLaunchKernelGGL(c_gn_stats_kernel, dim3(R, B, (nv + TX - 1) / TX), dim3(256), 0, s, x, part, HW, C, bm, R, TX);
}

// the contract precision's GroupNorm statistics: the centred per-row partials above, Chan-combined across rows by the finaliser (mode 3) into
// scale[b][c] / shift[b][c] of y = x * scale + shift.  part: B * c_gn_stat_rows(HW, C) * (2 C + 1) floats of scratch.
void launch_c_groupnorm_scale_shift(const float* x, float* part, int B, int H, int W, int C, int G, float eps, const float* gamma, const float* beta,
                                    float* scale, float* shift, hipStream_t s) {
    const int R = c_gn_stat_rows(H * W, C, nullptr);
    launch_c_gn_stats(x, part, B, H * W, C, s);
    launch_groupnorm_from_partials(part, 3, R, B, H, W, C, G, eps, gamma, beta, scale, shift, s);
}

// ---- GroupNorm apply (+ SiLU) of an fp32 tensor, written as a split A-order operand: y = act(x * scale[b][c] + shift[b][c]) --------------
__global__ __launch_bounds__(256) void c_gn_apply_split_kernel(const float* __restrict__ x, h16_t* __restrict__ out, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, long long HW, int C, long long n, int silu) {
    const int nv = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long px = i / nv;
        const int c = (int)(i - px * nv) * 8;
        const long long b = px / HW;
        float v[8], sc[8], sh[8];
        load8(x + px * C + c, v);
        load8(scale + b * C + c, sc);
        load8(shift + b * C + c, sh);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = __builtin_fmaf(v[e], sc[e], sh[e]);
            if (silu) v[e] = silu_f(v[e]);
        }
        store_split8(out + px * 3 * C, c, C, 0, v);
    }
}
void launch_c_gn_apply_split(const float* x, h16_t* out, const float* scale, const float* shift, int B, int HW, int C, int silu, hipStream_t s) {
    const long long n = (long long)B * HW * (C / 8);
    hipLaunchKernelGGL(c_gn_apply_split_kernel, dim3(cgrid(n)), dim3(256), 0, s, x, out, scale, shift, (long long)HW, C, n, silu);
}

// ---- LayerNorm over the last dim of fp32 [rows][C] -> split A-order operand.  One wave per row, exact two-pass statistics (the row is
// re-read from L1 / L2), C % 8 == 0. ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void c_layernorm_split_kernel(const float* __restrict__ x, h16_t* __restrict__ out, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (long long)row * C;
    const int nv = C >> 3;
    float s = 0.f;
    for (int v = lane; v < nv; v += 64) {
        float a[8];
        load8(xr + v * 8, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += a[e];
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int v = lane; v < nv; v += 64) {
        float a[8];
        load8(xr + v * 8, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) q += (a[e] - mean) * (a[e] - mean);
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    h16_t* orow = out + (long long)row * 3 * C;
    for (int v = lane; v < nv; v += 64) {
        float a[8], g[8], b[8];
        load8(xr + v * 8, a);
        load8(gamma + v * 8, g);
        load8(beta + v * 8, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (a[e] - mean) * rstd * g[e] + b[e];
        store_split8(orow, v * 8, C, 0, a);
    }
}
void launch_c_layernorm_split(const float* x, h16_t* out, const float* gamma, const float* beta, int rows, int C, float eps, hipStream_t s) {
    hipLaunchKernelGGL(c_layernorm_split_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, out, gamma, beta, rows, C, eps);
}

// ---- attention, unfused: head split -> batched logits GEMM (fp32) -> row softmax -> batched P.V GEMM -> head merge --------------------------
// qkv fp32 [B*T][ld] with q | k | v at columns 0 | C | 2C, C = heads * hd  ->
//   Qs [B*heads][T][3 hd] A order,  Ks [B*heads][T][3 hd] B order,  Vts [B*heads][hd][3 Tpad] B order, V TRANSPOSED, zero beyond T.
__global__ __launch_bounds__(256) void c_heads_split_qk_kernel(const float* __restrict__ qkv, int ld, h16_t* __restrict__ Qs, h16_t* __restrict__ Ks,
                                                                int B, int T, int heads, int hd) {
    const int nv = hd >> 3;
    const long long n = (long long)B * T * heads * nv * 2;
    const int C = heads * hd;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        long long t = i;
        const int v = (int)(t % nv); t /= nv;
        const int h = (int)(t % heads); t /= heads;
        const int which = (int)(t & 1); t >>= 1;  // 0: q, 1: k
        const long long bt = t, b = bt / T, tok = bt - b * T;
        float a[8];
        load8(qkv + bt * ld + which * C + h * hd + v * 8, a);
        h16_t* dst = (which ? Ks : Qs) + ((b * heads + h) * T + tok) * 3 * hd;
        store_split8(dst, v * 8, hd, which, a);
    }
}
// V^T: one workgroup per (64-token block, 64-channel block of one head, b * heads + h); tile through LDS
__global__ __launch_bounds__(256) void c_heads_split_vt_kernel(const float* __restrict__ qkv, int ld, h16_t* __restrict__ Vts, int T, int Tpad,
                                                                int heads, int hd) {
    __shared__ float tile[64][65];
    const int t0 = blockIdx.x * 64, d0 = blockIdx.y * 64, z = blockIdx.z, b = z / heads, h = z - b * heads;
    const int C = heads * hd;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int tt = i >> 6, d = i & 63;
        tile[tt][d] = (t0 + tt < T) ? qkv[((long long)b * T + t0 + tt) * ld + 2 * C + h * hd + d0 + d] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int d = i >> 3, g = i & 7;
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = tile[g * 8 + e][d];
        store_split8(Vts + ((long long)z * hd + d0 + d) * 3 * Tpad, t0 + g * 8, Tpad, 1, a);
    }
}
void launch_c_heads_split(const float* qkv, int ld, h16_t* Qs, h16_t* Ks, h16_t* Vts, int B, int T, int Tpad, int heads, int hd, hipStream_t s) {
    hipLaunchKernelGGL(c_heads_split_qk_kernel, dim3(cgrid((long long)B * T * heads * (hd / 8) * 2)), dim3(256), 0, s, qkv, ld, Qs, Ks, B, T, heads, hd);
    hipLaunchKernelGGL(c_heads_split_vt_kernel, dim3(Tpad / 64, hd / 64, B * heads), dim3(256), 0, s, qkv, ld, Vts, T, Tpad, heads, hd);
}

// The same head split for flash_attn64_split_kernel (attention.hip): PLANES instead of interleaved blocks -- QKhi / QKlo [B*T][2C] (q | k row-major),
// Vthi / Vtlo [B * heads][hd][Tpad] (V transposed, zero beyond T).
__global__ __launch_bounds__(256) void c_qk_planes_kernel(const float* __restrict__ qkv, int ld, h16_t* __restrict__ hi, h16_t* __restrict__ lo, long long rows,
                                                           int C2) {
    const int nv = C2 >> 3;
    const long long n = rows * nv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long r = i / nv;
        const int c = (int)(i - r * nv) * 8;
        float a[8];
        load8(qkv + r * ld + c, a);
        uint4 h4, l4;
        split8(a, h4, l4);
        *(uint4*)(hi + r * C2 + c) = h4;
        *(uint4*)(lo + r * C2 + c) = l4;
    }
}
__global__ __launch_bounds__(256) void c_vt_planes_kernel(const float* __restrict__ qkv, int ld, h16_t* __restrict__ hi, h16_t* __restrict__ lo, int T, int Tpad,
                                                           int heads, int hd) {
    __shared__ float tile[64][65];
    const int t0 = blockIdx.x * 64, d0 = blockIdx.y * 64, z = blockIdx.z, b = z / heads, h = z - b * heads;
    const int C = heads * hd;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int tt = i >> 6, d = i & 63;
        tile[tt][d] = (t0 + tt < T) ? qkv[((long long)b * T + t0 + tt) * ld + 2 * C + h * hd + d0 + d] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 8; i += 256) {
        const int d = i >> 3, g = i & 7;
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = tile[g * 8 + e][d];
        uint4 h4, l4;
        split8(a, h4, l4);
        const long long o = ((long long)z * hd + d0 + d) * Tpad + t0 + g * 8;
        *(uint4*)(hi + o) = h4;
        *(uint4*)(lo + o) = l4;
    }
}
void launch_c_qkv_planes(const float* qkv, int ld, h16_t* qk_hi, h16_t* qk_lo, h16_t* vt_hi, h16_t* vt_lo, int B, int T, int Tpad, int heads, int hd,
                         hipStream_t s) {
    const int C = heads * hd;
    hipLaunchKernelGGL(c_qk_planes_kernel, dim3(cgrid((long long)B * T * (2 * C / 8))), dim3(256), 0, s, qkv, ld, qk_hi, qk_lo, (long long)B * T, 2 * C);
    hipLaunchKernelGGL(c_vt_planes_kernel, dim3(Tpad / 64, hd / 64, B * heads), dim3(256), 0, s, qkv, ld, vt_hi, vt_lo, T, Tpad, heads, hd);
}

// row softmax of fp32 logits [rows][ld] (first T valid) -> split A-order probabilities [rows][3 ld], zero beyond T.  One workgroup per row,
// the row kept in registers (ld <= 256 * 4 * CS_MAXV).
constexpr int CS_MAXV = 16;
__global__ __launch_bounds__(256) void c_softmax_split_kernel(const float* __restrict__ in, h16_t* __restrict__ out, int T, int ld, float scale) {
    __shared__ float red[8];
    const long long row = blockIdx.x;
    const float* x = in + row * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4 v[CS_MAXV];
    float m = -3.0e38f;
#pragma unroll
    for (int k = 0; k < CS_MAXV; ++k) {
        const int c = (k * 256 + tid) * 4;
        if (c < ld) {
            v[k] = *(const float4*)(x + c);
            v[k].x = c < T ? v[k].x * scale : -3.0e38f;
            v[k].y = c + 1 < T ? v[k].y * scale : -3.0e38f;
            v[k].z = c + 2 < T ? v[k].z * scale : -3.0e38f;
            v[k].w = c + 3 < T ? v[k].w * scale : -3.0e38f;
            m = fmaxf(m, fmaxf(fmaxf(v[k].x, v[k].y), fmaxf(v[k].z, v[k].w)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CS_MAXV; ++k) {
        const int c = (k * 256 + tid) * 4;
        if (c < ld) {
            v[k].x = c < T ? __expf(v[k].x - m) : 0.f;
            v[k].y = c + 1 < T ? __expf(v[k].y - m) : 0.f;
            v[k].z = c + 2 < T ? __expf(v[k].z - m) : 0.f;
            v[k].w = c + 3 < T ? __expf(v[k].w - m) : 0.f;
            sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.f / ((red[4] + red[5]) + (red[6] + red[7]));
    h16_t* orow = out + row * 3 * ld;
#pragma unroll
    for (int k = 0; k < CS_MAXV; ++k) {
        const int c = (k * 256 + tid) * 4;
        if (c < ld) {
            const float p[4] = {v[k].x * inv, v[k].y * inv, v[k].z * inv, v[k].w * inv};
            const unsigned h0 = pack_h16x2(p[0], p[1]), h1 = pack_h16x2(p[2], p[3]);
            const unsigned l0 = pack_h16x2(p[0] - h16_lo(h0), p[1] - h16_hi(h0)), l1 = pack_h16x2(p[2] - h16_lo(h1), p[3] - h16_hi(h1));
            *(uint2*)(orow + c) = make_uint2(h0, h1);
            *(uint2*)(orow + ld + c) = make_uint2(l0, l1);
            *(uint2*)(orow + 2 * ld + c) = make_uint2(h0, h1);
        }
    }
}
// the same for rows too long for the register-resident form (maps beyond 128 x 128 latents): three passes over the row (L2-hot), same arithmetic
__global__ __launch_bounds__(256) void c_softmax_split_long_kernel(const float* __restrict__ in, h16_t* __restrict__ out, int T, int ld, float scale) {
    __shared__ float red[8];
    const long long row = blockIdx.x;
    const float* x = in + row * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -3.0e38f;
    for (int c = tid; c < T; c += 256) m = fmaxf(m, x[c] * scale);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int c = tid; c < T; c += 256) sum += __expf(x[c] * scale - m);
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.f / ((red[4] + red[5]) + (red[6] + red[7]));
    h16_t* orow = out + row * 3 * ld;
    for (int c = tid * 2; c < ld; c += 512) {
        const float p0 = c < T ? __expf(x[c] * scale - m) * inv : 0.f, p1 = c + 1 < T ? __expf(x[c + 1] * scale - m) * inv : 0.f;
        const unsigned h = pack_h16x2(p0, p1), l = pack_h16x2(p0 - h16_lo(h), p1 - h16_hi(h));
        *(unsigned*)(orow + c) = h;
        *(unsigned*)(orow + ld + c) = l;
        *(unsigned*)(orow + 2 * ld + c) = h;
    }
}
bool c_softmax_split_supported(int ld) { return (ld & 3) == 0; }
// the attention core's way and its transient bytes (kernels.h); the plane sizes are the ones launch_c_qkv_planes writes
int c_attention_plan(int B, int T, int heads, int hd, long long* workspace_bytes) {
    const GpSwitches& sw = gp_sw();
    const long long Tpad = ((long long)T + 63) / 64 * 64, Z = (long long)B * heads, C = (long long)heads * hd;
    const long long unfused = 10 * Z * T * Tpad;                        // fp32 logits + split probabilities, both live across the softmax
    const long long planes = 8 * (long long)B * T * C + 4 * Z * hd * Tpad;  // q | k hi + lo [B*T][2C], V^T hi + lo [Z][hd][Tpad]: 16-bit
    int path = C_ATTN_UNFUSED;
    if (hd == 64 && !sw.c_no_flash && (long long)T * 3 * C * 2 < 0x7fffffffll) path = C_ATTN_FLASH64;
    else if (hd == 512 && heads == 1 && !GP_F16 && flash_attn512_split_supported(T) &&
             (sw.c_flash512 > 0 || (sw.c_flash512 < 0 && unfused > C_FLASH512_ABOVE_BYTES)))
        path = C_ATTN_FLASH512;
    if (workspace_bytes) *workspace_bytes = path == C_ATTN_UNFUSED ? unfused : planes;
    return path;
}
void launch_c_softmax_split(const float* in, h16_t* out, long long rows, int T, int ld, float scale, hipStream_t s) {
    if (ld <= 256 * 4 * CS_MAXV) hipLaunchKernelGGL(c_softmax_split_kernel, dim3((unsigned)rows), dim3(256), 0, s, in, out, T, ld, scale);
    else hipLaunchKernelGGL(c_softmax_split_long_kernel, dim3((unsigned)rows), dim3(256), 0, s, in, out, T, ld, scale);
}

// O fp32 [B*heads][T][hd] -> split A-order [B*T][3 C] (C = heads * hd): the input of to_out
__global__ __launch_bounds__(256) void c_heads_merge_split_kernel(const float* __restrict__ O, h16_t* __restrict__ out, int B, int T, int heads, int hd) {
    const int nv = hd >> 3, C = heads * hd;
    const long long n = (long long)B * T * heads * nv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        long long t = i;
        const int v = (int)(t % nv); t /= nv;
        const int h = (int)(t % heads); t /= heads;
        const long long bt = t, b = bt / T, tok = bt - b * T;
        float a[8];
        load8(O + ((b * heads + h) * T + tok) * hd + v * 8, a);
        store_split8(out + bt * 3 * C, h * hd + v * 8, C, 0, a);
    }
}
void launch_c_heads_merge_split(const float* O, h16_t* out, int B, int T, int heads, int hd, hipStream_t s) {
    hipLaunchKernelGGL(c_heads_merge_split_kernel, dim3(cgrid((long long)B * T * heads * (hd / 8))), dim3(256), 0, s, O, out, B, T, heads, hd);
}

// ---- cross-attention against the folded two-token context (norm.hip states the algebra):
//   y_out = y + c0 + sum_h sigmoid(LNhat(y) . U[h] + u0[h]) G[h];   n3 = split(LayerNorm(y_out; g3, b3)).  fp32 rows, one wave per row. ------------
__global__ __launch_bounds__(256) void c_cross_fold_kernel(const float* __restrict__ y, float* __restrict__ y_out, h16_t* __restrict__ n3_out,
                                                            const float* __restrict__ U, const float* __restrict__ u0, const float* __restrict__ G,
                                                            const float* __restrict__ c0, const float* __restrict__ g3, const float* __restrict__ b3,
                                                            int rows, int C, int heads, float eps) {
    constexpr int MAXV = 4;  // C <= 64 * 8 * MAXV = 2048
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nv = C >> 3;
    const float invC = 1.f / (float)C;
    float x[MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int v = lane + 64 * u;
        if (v < nv) {
            load8(y + (long long)row * C + v * 8, x[u]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[u][e];
        }
    }
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < MAXV; ++u)
        if (lane + 64 * u < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) q += (x[u][e] - mean) * (x[u][e] - mean);
        }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
    float acc[MAXV][8];
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int v = lane + 64 * u;
        if (v < nv) {
            float c[8];
            load8(c0 + v * 8, c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[u][e] = x[u][e] + c[e];
        }
    }
    for (int h = 0; h < heads; ++h) {
        float d = 0.f;
#pragma unroll
        for (int u = 0; u < MAXV; ++u) {
            const int v = lane + 64 * u;
            if (v < nv) {
                float w[8];
                load8(U + (long long)h * C + v * 8, w);
#pragma unroll
                for (int e = 0; e < 8; ++e) d += (x[u][e] - mean) * rstd * w[e];
            }
        }
        d = wave_sum(d) + u0[h];
        const float sg = 1.f / (1.f + __expf(-d));
#pragma unroll
        for (int u = 0; u < MAXV; ++u) {
            const int v = lane + 64 * u;
            if (v < nv) {
                float g[8];
                load8(G + (long long)h * C + v * 8, g);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[u][e] = __builtin_fmaf(sg, g[e], acc[u][e]);
            }
        }
    }
    float s2 = 0.f;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int v = lane + 64 * u;
        if (v < nv) {
            store8(y_out + (long long)row * C + v * 8, acc[u]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s2 += acc[u][e];
        }
    }
    if (!n3_out) return;
    const float mean2 = wave_sum(s2) * invC;
    float q2 = 0.f;
#pragma unroll
    for (int u = 0; u < MAXV; ++u)
        if (lane + 64 * u < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) q2 += (acc[u][e] - mean2) * (acc[u][e] - mean2);
        }
    const float rstd2 = rsqrtf(wave_sum(q2) * invC + eps);
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int v = lane + 64 * u;
        if (v < nv) {
            float g[8], b[8], o[8];
            load8(g3 + v * 8, g);
            load8(b3 + v * 8, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (acc[u][e] - mean2) * rstd2 * g[e] + b[e];
            store_split8(n3_out + (long long)row * 3 * C, v * 8, C, 0, o);
        }
    }
}
bool c_cross_fold_supported(int C) { return (C & 7) == 0 && C <= 2048; }
void launch_c_cross_fold(const float* y, float* y_out, h16_t* n3_out, const float* U, const float* u0, const float* G, const float* c0, const float* g3,
                         const float* b3, int rows, int C, int heads, float eps, hipStream_t s) {
    hipLaunchKernelGGL(c_cross_fold_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, y, y_out, n3_out, U, u0, G, c0, g3, b3, rows, C, heads, eps);
}

// ---- cross-attention against a small constant context of any length (attention.hip: cross_attn_small_kernel), fp32 q -> split A-order output
__global__ __launch_bounds__(256) void c_cross_attn_small_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                                  h16_t* __restrict__ out, long long nrh, int C, int heads, int L) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nrh) return;
    const long long row = idx / heads;
    const int h = (int)(idx - row * heads);
    float qv[64], o[64];
    const float* qp = q + row * C + h * 64;
#pragma unroll
    for (int i = 0; i < 64; i += 4) {
        const float4 a = *(const float4*)(qp + i);
        qv[i] = a.x; qv[i + 1] = a.y; qv[i + 2] = a.z; qv[i + 3] = a.w;
    }
#pragma unroll
    for (int d = 0; d < 64; ++d) o[d] = 0.f;
    float m = -1e30f, l = 0.f;
    for (int j = 0; j < L; ++j) {
        const float* kp = kc + (long long)j * C + h * 64;
        float sc = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) sc += qv[d] * kp[d];
        sc *= 0.125f;
        const float mn = fmaxf(m, sc);
        const float a = __expf(m - mn), pj = __expf(sc - mn);
        m = mn;
        l = l * a + pj;
        const float* vp = vc + (long long)j * C + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) o[d] = o[d] * a + pj * vp[d];
    }
    const float inv = 1.f / l;
    h16_t* orow = out + row * 3 * C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = o[i * 8 + e] * inv;
        store_split8(orow, h * 64 + i * 8, C, 0, v);
    }
}
void launch_c_cross_attn_small(const float* q, const float* kc, const float* vc, h16_t* out, int rows, int C, int L, hipStream_t s) {
    const int heads = C / 64;
    const long long nrh = (long long)rows * heads;
    hipLaunchKernelGGL(c_cross_attn_small_kernel, dim3((unsigned)((nrh + 255) / 256)), dim3(256), 0, s, q, kc, vc, out, nrh, C, heads, L);
}
