// Seg evaluation on the device (gp_seg_decode, gp_eval_seg): the three-channel colour output of mode seg snapped to the classes of a user-supplied
// palette and scored against a colour or label ground truth, per image.  The definitions are stated once in include/genpercept_hip.h;
// eval_metrics.palette_labels / seg_counts / seg_metrics_from_counts restate them on the host.  Everything is a function of integers over the
// 8-bit prediction (quantise8 per channel, the byte run.py:449-455 saves):
//   decode   d_k = (r - pr_k)^2 + (g - pg_k)^2 + (b - pb_k)^2 in integers, the smallest k of the minimum: `<` in increasing k.  The palette is
//            staged once per workgroup as one packed word per colour in LDS; the K-loop runs over a wave-uniform index (every lane reads the
//            same LDS word: a broadcast) for the four pixels of a lane's quad at once.
//   zero     the per-image matrices [3 + K * K] of 64-bit words (in counts_out, or in the workspace when it is NULL) are cleared.
//   count    grid (eval_blocks(H * W), B).  The K x K confusion matrix of a workgroup is 32-bit counters in dynamic LDS (K * K * 4 bytes: 147456
//            at K = 192, one workgroup per CU; a small K keeps many per CU), filled by LDS integer atomics -- 64 lanes on one word serialise
//            for about 64 clocks, against about 8 K integer operations per decode: the K-loop, not the atomics, is the long part.  A workgroup sees at most
//            2^31 / 512 pixels: 32 bits cannot overflow.  At the end the NON-ZERO entries are added to the image's 64-bit matrix by integer
//            atomicAdd; n, n_void and sum_d by per-lane sums, a shuffle tree, LDS, one 64-bit atomicAdd per value and workgroup.  Integer adds
//            do not depend on their order, so the pixel -> thread assignment may depend on pointer alignment: pixels [head, head + 4 nq) go as
//            quads (head: the distance of the ground truth from a 4-byte boundary), every stream of a quad by one vector access where that
//            stream is aligned there and by its four scalars where it is not (planes H * W apart need not share an alignment); the up to three
//            pixels before and after them one by one.
//   values   one workgroup per image: row and column sums by 64-bit LDS integer atomics over one coalesced sweep of the matrix, thread i the
//            quotients of class i, thread 0 the float64 sums in increasing class index.  Each value is one fixed sequence of correctly rounded
//            float64 + * / sqrt on the integers (this file contracts nothing), so the host's restatement is bit-equal.
// gp_eval_seg: three launches for every B (zero, count, values); gp_seg_decode: one.  Nothing is read back; no float is ever added atomically.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "kernels.h"
#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SG_MAX_K = 192;   // K * K * 4 bytes of LDS counters: 147456 of the CU's 163840
constexpr int SG_NSUM = 3;      // n, n_void, sum_d in front of the matrix
constexpr int SG_OUT = 8;       // n, n_void, pixel_acc, mean_acc, miou, fwiou, colour_rmse, n_classes in front of iou[K]
constexpr int SG_LDS_MAX = SG_MAX_K * SG_MAX_K * 4;

inline long long seg_words(int K) { return SG_NSUM + (long long)K * K; }

// one packed word per palette colour: r | g << 8 | b << 16 (threads k < K; the caller synchronises)
__device__ __forceinline__ void seg_stage_palette(const unsigned char* __restrict__ pal, int K, unsigned* s_pal) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) s_pal[k] = (unsigned)pal[3 * k] | (unsigned)pal[3 * k + 1] << 8 | (unsigned)pal[3 * k + 2] << 16;
}

// N packed colours against the palette: cls = the smallest k of the minimum distance, dist = that minimum (<= 3 * 255^2)
template <int N>
__device__ __forceinline__ void seg_nearest(const unsigned* s_pal, int K, const unsigned (&rgb)[N], unsigned (&cls)[N], int (&dist)[N]) {
    int r[N], g[N], b[N];
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = (int)(rgb[j] & 0xffu), g[j] = (int)((rgb[j] >> 8) & 0xffu), b[j] = (int)((rgb[j] >> 16) & 0xffu), cls[j] = 0, dist[j] = 0x7fffffff;
    for (int k = 0; k < K; ++k) {
        const unsigned p = s_pal[k];
        const int pr = (int)(p & 0xffu), pg = (int)((p >> 8) & 0xffu), pb = (int)(p >> 16);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int dr = r[j] - pr, dg = g[j] - pg, db = b[j] - pb;
            const int d = dr * dr + dg * dg + db * db;
            if (d < dist[j]) dist[j] = d, cls[j] = (unsigned)k;
        }
    }
}

// four consecutive bytes as one word (little endian), by one load where p is 4-byte aligned
__device__ __forceinline__ unsigned seg_ld4(const unsigned char* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const unsigned*>(p);
    return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
}

__device__ __forceinline__ void seg_st4(unsigned char* p, bool aligned, unsigned v) {
    if (aligned) {
        *reinterpret_cast<unsigned*>(p) = v;
        return;
    }
    p[0] = (unsigned char)v, p[1] = (unsigned char)(v >> 8), p[2] = (unsigned char)(v >> 16), p[3] = (unsigned char)(v >> 24);
}

// The prediction of one image: three planes hw apart, floats (quantised here) or bytes.
template <bool U8>
struct SegPred {
    Pred8<U8> p;  // plane c, pixel i: element c * hw + i
    long long hw;
    bool al[3];   // plane c is vector-aligned at pixel `head`
    __device__ __forceinline__ SegPred(const void* pred, long long b, long long hw_, long long head) : p(pred, b * 3 * hw_), hw(hw_) {
#pragma unroll
        for (int c = 0; c < 3; ++c) al[c] = p.quad_aligned(c * hw_ + head);
    }
    // pixel i as a packed colour
    __device__ __forceinline__ unsigned one(long long i) const { return p[i] | p[hw + i] << 8 | p[2 * hw + i] << 16; }
    // the four quantised bytes of plane c at pixels i0 .. i0 + 3
    __device__ __forceinline__ unsigned plane4(int c, long long i0) const {
        if (U8) return seg_ld4(p.u + c * hw + i0, al[c]);
        const float* f = p.f + c * hw + i0;
        float4 v;
        if (al[c]) v = *reinterpret_cast<const float4*>(f);
        else v = make_float4(f[0], f[1], f[2], f[3]);
        return quantise8(v.x) | quantise8(v.y) << 8 | quantise8(v.z) << 16 | quantise8(v.w) << 24;
    }
    // pixels i0 .. i0 + 3 as packed colours
    __device__ __forceinline__ void quad(long long i0, unsigned (&rgb)[4]) const {
        const unsigned r4 = plane4(0, i0), g4 = plane4(1, i0), b4 = plane4(2, i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) rgb[j] = ((r4 >> (8 * j)) & 0xffu) | ((g4 >> (8 * j)) & 0xffu) << 8 | ((b4 >> (8 * j)) & 0xffu) << 16;
    }
};

// ---- decode -----------------------------------------------------------------------------------------------------------------------------------
// grid (eval_blocks(H * W), B); head aligns labels_out
template <bool U8>
__global__ __launch_bounds__(EV_THREADS) void seg_decode_kernel(const void* __restrict__ pred_v, const unsigned char* __restrict__ pal, int K, long long hw,
                                                                unsigned char* __restrict__ labels_out, int* __restrict__ dist_out) {
    __shared__ unsigned s_pal[SG_MAX_K];
    const long long b = blockIdx.y;
    seg_stage_palette(pal, K, s_pal);
    __syncthreads();
    labels_out += b * hw;
    if (dist_out) dist_out += b * hw;
    const QuadSplit sp(hw, (long long)((4 - ((uintptr_t)labels_out & 3)) & 3));
    const SegPred<U8> pred(pred_v, b, hw, sp.head);
    const bool d_al = dist_out && ((uintptr_t)(dist_out + sp.head) & 15) == 0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < sp.nq; q += stride) {
        const long long i0 = sp.quad(q);
        unsigned rgb[4], cls[4];
        int dist[4];
        pred.quad(i0, rgb);
        seg_nearest<4>(s_pal, K, rgb, cls, dist);
        seg_st4(labels_out + i0, true, cls[0] | cls[1] << 8 | cls[2] << 16 | cls[3] << 24);
        if (dist_out) {
            if (d_al) *reinterpret_cast<int4*>(dist_out + i0) = make_int4(dist[0], dist[1], dist[2], dist[3]);
            else dist_out[i0] = dist[0], dist_out[i0 + 1] = dist[1], dist_out[i0 + 2] = dist[2], dist_out[i0 + 3] = dist[3];
        }
    }
    for (long long k = (long long)blockIdx.x * EV_THREADS + threadIdx.x; k < sp.ns; k += stride) {
        const long long i = sp.scalar(k);
        const unsigned rgb[1] = {pred.one(i)};
        unsigned cls[1];
        int dist[1];
        seg_nearest<1>(s_pal, K, rgb, cls, dist);
        labels_out[i] = (unsigned char)cls[0];
        if (dist_out) dist_out[i] = dist[0];
    }
}

// ---- zero -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EV_THREADS) void seg_zero_kernel(u64* __restrict__ mat, long long words) {
    const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < words) mat[i] = 0;
}

// ---- count ------------------------------------------------------------------------------------------------------------------------------------
struct SegAcc {
    unsigned n = 0, n_void = 0;  // per lane
    u64 sum_d = 0;
    // one pixel: prediction class c at distance d, ground-truth class g (>= K: void), `in`: inside the region
    __device__ __forceinline__ void add(unsigned c, int d, unsigned g, bool in, unsigned K, unsigned* conf) {
        if (!in) return;
        if (g >= K) {
            n_void += 1;
            return;
        }
        n += 1, sum_d += (u64)(unsigned)d;
        atomicAdd(&conf[g * K + c], 1u);
    }
};

// grid (eval_blocks(H * W), B), dynamic LDS K * K * 4.  gt: LABELS ? uint8 [B][H][W] : uint8 [B][H][W][3]
template <bool U8, bool LABELS>
__global__ __launch_bounds__(EV_THREADS) void seg_count_kernel(const void* __restrict__ pred_v, const unsigned char* __restrict__ gt, int gt_tol,
                                                               const unsigned char* __restrict__ region, const unsigned char* __restrict__ pal, int K,
                                                               long long hw, u64* __restrict__ mat, unsigned char* __restrict__ labels_out) {
    extern __shared__ unsigned s_conf[];
    __shared__ unsigned s_pal[SG_MAX_K];
    const long long b = blockIdx.y;
    const int kk = K * K;
    for (int k = threadIdx.x; k < kk; k += EV_THREADS) s_conf[k] = 0;
    seg_stage_palette(pal, K, s_pal);
    __syncthreads();
    gt += b * hw * (LABELS ? 1 : 3);
    if (region) region += b * hw;
    if (labels_out) labels_out += b * hw;
    mat += b * (SG_NSUM + (long long)kk);
    // head: pixel `head` of the ground truth sits on a 4-byte boundary (3 * head = -address mod 4 for the interleaved form)
    const QuadSplit sp(hw, LABELS ? (long long)((4 - ((uintptr_t)gt & 3)) & 3) : (long long)((uintptr_t)gt & 3));
    const SegPred<U8> pred(pred_v, b, hw, sp.head);
    const bool r_al = region && ((uintptr_t)(region + sp.head) & 3) == 0, l_al = labels_out && ((uintptr_t)(labels_out + sp.head) & 3) == 0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    SegAcc acc;
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < sp.nq; q += stride) {
        const long long i0 = sp.quad(q);
        unsigned rgb[4], cls[4], gcl[4];
        int dist[4];
        pred.quad(i0, rgb);
        const unsigned r4 = region ? seg_ld4(region + i0, r_al) : 0x01010101u;
        if (LABELS) {
            const unsigned g4 = seg_ld4(gt + i0, true);
#pragma unroll
            for (int j = 0; j < 4; ++j) gcl[j] = (g4 >> (8 * j)) & 0xffu;
            seg_nearest<4>(s_pal, K, rgb, cls, dist);
        } else {
            const unsigned* g = reinterpret_cast<const unsigned*>(gt + 3 * i0);  // 12 bytes: (r g b) x 4
            const unsigned w0 = g[0], w1 = g[1], w2 = g[2];
            unsigned both[8] = {rgb[0], rgb[1], rgb[2], rgb[3], w0 & 0xffffffu, (w0 >> 24) | (w1 & 0xffffu) << 8, (w1 >> 16) | (w2 & 0xffu) << 16, w2 >> 8};
            unsigned c8[8];
            int d8[8];
            seg_nearest<8>(s_pal, K, both, c8, d8);
#pragma unroll
            for (int j = 0; j < 4; ++j) cls[j] = c8[j], dist[j] = d8[j], gcl[j] = d8[4 + j] > gt_tol ? 0xffu : c8[4 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc.add(cls[j], dist[j], gcl[j], ((r4 >> (8 * j)) & 0xffu) != 0, (unsigned)K, s_conf);
        if (labels_out) seg_st4(labels_out + i0, l_al, cls[0] | cls[1] << 8 | cls[2] << 16 | cls[3] << 24);
    }
    for (long long k = (long long)blockIdx.x * EV_THREADS + threadIdx.x; k < sp.ns; k += stride) {
        const long long i = sp.scalar(k);
        unsigned c, g;
        int d;
        if (LABELS) {
            const unsigned rgb[1] = {pred.one(i)};
            unsigned c1[1];
            int d1[1];
            seg_nearest<1>(s_pal, K, rgb, c1, d1);
            c = c1[0], d = d1[0], g = gt[i];
        } else {
            const unsigned both[2] = {pred.one(i), (unsigned)gt[3 * i] | (unsigned)gt[3 * i + 1] << 8 | (unsigned)gt[3 * i + 2] << 16};
            unsigned c2[2];
            int d2[2];
            seg_nearest<2>(s_pal, K, both, c2, d2);
            c = c2[0], d = d2[0], g = d2[1] > gt_tol ? 0xffu : c2[1];
        }
        acc.add(c, d, g, region ? region[i] != 0 : true, (unsigned)K, s_conf);
        if (labels_out) labels_out[i] = (unsigned char)c;
    }
    u64 v[SG_NSUM] = {acc.n, acc.n_void, acc.sum_d};
    const u64 a = block_sum(v);  // (its barrier also: every LDS atomic of the workgroup has landed)
    if (threadIdx.x < SG_NSUM && a != 0) atomicAdd(mat + threadIdx.x, a);
    for (int k = threadIdx.x; k < kk; k += EV_THREADS) {
        const unsigned a = s_conf[k];
        if (a != 0) atomicAdd(mat + SG_NSUM + k, (u64)a);
    }
}

// ---- values -----------------------------------------------------------------------------------------------------------------------------------
// one workgroup per image
__global__ __launch_bounds__(EV_THREADS) void seg_finalise_kernel(const u64* __restrict__ mat, int K, double* __restrict__ out) {
    __shared__ u64 s_row[SG_MAX_K], s_col[SG_MAX_K], s_tp[SG_MAX_K];
    __shared__ double s_acc[SG_MAX_K], s_iou[SG_MAX_K];
    const long long b = blockIdx.x;
    const int kk = K * K;
    mat += b * (SG_NSUM + (long long)kk);
    double* o = out + b * (SG_OUT + K);
    for (int k = threadIdx.x; k < K; k += EV_THREADS) s_row[k] = 0, s_col[k] = 0, s_tp[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < kk; k += EV_THREADS) {
        const u64 a = mat[SG_NSUM + k];
        if (a == 0) continue;
        const int g = k / K, c = k - g * K;
        atomicAdd(&s_row[g], a);
        atomicAdd(&s_col[c], a);
        if (g == c) s_tp[g] = a;
    }
    __syncthreads();
    const u64 n = mat[0], n_void = mat[1], sum_d = mat[2];
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < K; i += EV_THREADS) {
        const u64 row = s_row[i], tp = s_tp[i], uni = row + s_col[i] - tp;
        const double iou = uni != 0 ? (double)tp / (double)uni : nan;
        s_acc[i] = row != 0 ? (double)tp / (double)row : nan;
        s_iou[i] = iou;
        o[SG_OUT + i] = n != 0 ? iou : nan;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    o[0] = (double)n, o[1] = (double)n_void;
    if (n == 0) {
        for (int k = 2; k < SG_OUT; ++k) o[k] = nan;
        return;
    }
    u64 sum_tp = 0, n_rows = 0, n_cls = 0;
    double acc = 0.0, iou = 0.0, fw = 0.0;
    for (int i = 0; i < K; ++i) {
        sum_tp += s_tp[i];
        if (s_row[i] != 0) {
            acc = acc + s_acc[i];
            fw = fw + (double)s_row[i] * s_iou[i];
            n_rows += 1;
        }
        if (s_row[i] + s_col[i] - s_tp[i] != 0) {  // iou_i is defined
            iou = iou + s_iou[i];
            n_cls += 1;
        }
    }
    const double dn = (double)n;
    o[2] = (double)sum_tp / dn;
    o[3] = acc / (double)n_rows;
    o[4] = iou / (double)n_cls;
    o[5] = fw / dn;
    o[6] = __dsqrt_rn((double)sum_d / (3.0 * dn)) / 255.0;
    o[7] = (double)n_cls;
}

template <bool U8, bool LABELS>
void seg_launch_count(dim3 grid, int lds, hipStream_t s, const void* pred, const unsigned char* gt, int gt_tol, const unsigned char* region,
                      const unsigned char* pal, int K, long long hw, u64* mat, unsigned char* labels_out) {
    static unsigned long long attr_mask = 0;  // one per instantiation
    gp_once_per_device(&attr_mask, [&] {
        (void)hipFuncSetAttribute((const void*)seg_count_kernel<U8, LABELS>, hipFuncAttributeMaxDynamicSharedMemorySize, SG_LDS_MAX);
    });
    hipLaunchKernelGGL((seg_count_kernel<U8, LABELS>), grid, dim3(EV_THREADS), lds, s, pred, gt, gt_tol, region, pal, K, hw, mat, labels_out);
}

}  // namespace

extern "C" {

gp_status gp_seg_decode(const void* pred, int pred_is_u8, const unsigned char* palette, int K, int B, int H, int W, unsigned char* labels_out,
                        int* dist_out, void* stream) {
    if (!pred || !palette || !labels_out) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W) || K < 1 || K > SG_MAX_K) return GP_ERR_INVALID;
    if (!eval_pred_ok(pred, pred_is_u8) || ((uintptr_t)dist_out & 3) != 0) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W;
    const dim3 grid(eval_blocks(hw), B);
    const auto decode = pred_is_u8 ? seg_decode_kernel<true> : seg_decode_kernel<false>;
    hipLaunchKernelGGL(decode, grid, dim3(EV_THREADS), 0, s, pred, palette, K, hw, labels_out, dist_out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

long long gp_eval_seg_workspace(int B, int H, int W, int K) {
    if (B < 1 || H < 1 || W < 1 || K < 1 || K > SG_MAX_K) return 0;
    return (long long)B * seg_words(K) * 8;
}

gp_status gp_eval_seg(const void* pred, int pred_is_u8, const unsigned char* gt, int gt_is_labels, int gt_tol, const unsigned char* region,
                      const unsigned char* palette, int K, int B, int H, int W, double* out, unsigned long long* counts_out,
                      unsigned char* labels_out, void* workspace, long long workspace_bytes, void* stream) {
    if (!pred || !gt || !palette || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W) || K < 1 || K > SG_MAX_K) return GP_ERR_INVALID;
    if (!eval_pred_ok(pred, pred_is_u8) || gt_is_labels < 0 || gt_is_labels > 1 || gt_tol < 0) return GP_ERR_INVALID;
    if (!eval_aligned8(workspace, out, counts_out)) return GP_ERR_INVALID;
    if (workspace_bytes < gp_eval_seg_workspace(B, H, W, K)) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W, words = (long long)B * seg_words(K);
    u64* mat = counts_out ? counts_out : (u64*)workspace;
    hipLaunchKernelGGL(seg_zero_kernel, dim3((unsigned)((words + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, s, mat, words);
    const dim3 grid(eval_blocks(hw), B);
    const int lds = K * K * 4;
    if (pred_is_u8) {
        if (gt_is_labels) seg_launch_count<true, true>(grid, lds, s, pred, gt, gt_tol, region, palette, K, hw, mat, labels_out);
        else seg_launch_count<true, false>(grid, lds, s, pred, gt, gt_tol, region, palette, K, hw, mat, labels_out);
    } else {
        if (gt_is_labels) seg_launch_count<false, true>(grid, lds, s, pred, gt, gt_tol, region, palette, K, hw, mat, labels_out);
        else seg_launch_count<false, false>(grid, lds, s, pred, gt, gt_tol, region, palette, K, hw, mat, labels_out);
    }
    hipLaunchKernelGGL(seg_finalise_kernel, dim3(B), dim3(EV_THREADS), 0, s, (const u64*)mat, K, out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
