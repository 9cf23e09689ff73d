// What the evaluation kernels (eval.hip, eval_structure.hip, eval_matting.hip, eval_seg.hip, mask_band.hip) share: the workgroup shape, the
// slab count rule, the fixed-order block sums, the two-class histogram of an 8-bit prediction and the summing of its slabs, the reading of a
// prediction that is floats or bytes, the head / quads / tail split of an image and the argument checks of the host entries.  Include after
// <hip/hip_runtime.h>.
#pragma once

#include <stdint.h>

// The host's numpy code has no fused multiply-adds: nothing here, and nothing in the files that include this one, may be contracted into one.
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr long long EV_PIX_PER_WG = 4096;  // at least this many pixels per workgroup ...
constexpr int EV_MAX_WG = 512;             // ... and at most this many workgroups (= slabs) per image

inline int eval_blocks(long long hw) {
    long long g = (hw + EV_PIX_PER_WG - 1) / EV_PIX_PER_WG;
    return (int)(g < 1 ? 1 : (g > EV_MAX_WG ? EV_MAX_WG : g));
}

// ---- host: the argument checks every entry point makes ---------------------------------------------------------------------------------------
inline bool eval_dims_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL; }

// `pred` may be read as is_u8 says: bytes, or floats on a 4-byte boundary
inline bool eval_pred_ok(const void* pred, int is_u8) { return is_u8 == 1 || (is_u8 == 0 && ((uintptr_t)pred & 3) == 0); }

// every pointer (NULL included) is 8-byte aligned
template <typename... P>
inline bool eval_aligned8(const P*... p) {
    return ((... | (uintptr_t)p) & 7) == 0;
}

// ---- block sums --------------------------------------------------------------------------------------------------------------------------------
// one 64-lane wave: lane 0 ends with the sum of the wave's v, by a shuffle tree 32 down to 1 (the shuffle moves the two halves of a 64-bit value)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// v[0..N) of every thread of an EV_THREADS workgroup -> thread k < N returns the workgroup's sum k (T: double or u64).  Fixed order:
// wave_sum inside each wave, then the waves in index order through LDS.  One barrier; every thread of the workgroup calls it.
template <typename T, int N>
__device__ __forceinline__ T block_sum(T (&v)[N]) {
    __shared__ T s_part[EV_WAVES][N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_part[wave][k] = v[k];
    }
    __syncthreads();
    T a = 0;
    if (threadIdx.x < N) {
        a = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EV_WAVES; ++w) a += s_part[w][threadIdx.x];
    }
    return a;
}

// block_sum, then slab[0..N) = the sums
template <int N>
__device__ __forceinline__ void block_reduce_store(double (&v)[N], double* __restrict__ slab) {
    const double a = block_sum(v);
    if (threadIdx.x < N) slab[threadIdx.x] = a;
}

// the slabs of one image, summed in index order by thread k < N (loads batched 16 deep: they are independent, the additions are not)
template <int N>
__device__ __forceinline__ double sum_slabs(const double* __restrict__ ws, int nblk, int k) {
    double a = 0.0;
    int j = 0;
    for (; j + 16 <= nblk; j += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = ws[(long long)(j + u) * N + k];
#pragma unroll
        for (int u = 0; u < 16; ++u) a += v[u];
    }
    for (; j < nblk; ++j) a += ws[(long long)j * N + k];
    return a;
}

// ---- reading an 8-bit prediction -----------------------------------------------------------------------------------------------------------------
// run.py:449-455 on one value: clip to [0, 1] (NaN -> 0), * 255 in fp32, truncate
__device__ __forceinline__ unsigned quantise8(float x) {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
    return (unsigned)(unsigned char)(c * 255.0f);
}

// A prediction from element `first` on: floats in [0, 1] (quantised on reading) or, U8, the bytes themselves.
template <bool U8>
struct Pred8 {
    const float* f;          // !U8
    const unsigned char* u;  // U8
    __device__ __forceinline__ Pred8(const void* pred, long long first)
        : f(U8 ? nullptr : (const float*)pred + first), u(U8 ? (const unsigned char*)pred + first : nullptr) {}
    // pixel i as its 8-bit value
    __device__ __forceinline__ unsigned operator[](long long i) const { return U8 ? (unsigned)u[i] : quantise8(f[i]); }
    // pixels i .. i + 3 may go as one load (16 bytes of floats, 4 bytes)
    __device__ __forceinline__ bool quad_aligned(long long i) const { return U8 ? ((uintptr_t)(u + i) & 3) == 0 : ((uintptr_t)(f + i) & 15) == 0; }
};

// ---- head / quads / tail ---------------------------------------------------------------------------------------------------------------------------
// The hw pixels of an image for a kernel that takes four at a time: pixels [head, head + 4 nq) are quad q = pixels quad(q) .. quad(q) + 3, the
// up to three before and the up to three after them are the ns scalar pixels scalar(0) .. scalar(ns - 1).  head (clamped to hw; hw: no quads)
// is the caller's choice, usually the distance of one of its streams from a 4-byte boundary.
struct QuadSplit {
    long long head, nq, tail0, ns;
    __device__ __forceinline__ QuadSplit(long long hw, long long head_)
        : head(head_ < hw ? head_ : hw), nq((hw - head) / 4), tail0(head + 4 * nq), ns(head + (hw - tail0)) {}
    __device__ __forceinline__ long long quad(long long q) const { return head + 4 * q; }
    __device__ __forceinline__ long long scalar(long long k) const { return k < head ? k : tail0 + (k - head); }
};

// ---- the two-class histogram -------------------------------------------------------------------------------------------------------------------------
// 256 bins of an 8-bit value q for each class (bg, fg) of its pixel, per workgroup: integer LDS atomics into one copy per wave.  Real masks are
// almost all 0 and 255, and 64 lanes adding to one LDS word serialise, so those two bins are counted per class with a ballot and a population
// count -- a wave-uniform register, one LDS add per wave and bin at the end -- and only the other lanes issue atomics.
constexpr int EV_BINS = 256;
constexpr long long class_slab_bytes(int nsum) { return nsum * 8 + 2 * EV_BINS * 4; }  // a count slab: nsum 64-bit sums, [bg | fg] 32-bit bins

struct ClassHist {
    unsigned* all;   // the EV_WAVES copies [2][EV_BINS] in LDS
    unsigned sat[4] = {0, 0, 0, 0};  // per WAVE (uniform): q == 0 & bg, q == 0 & fg, q == 255 & bg, q == 255 & fg
    // every thread of the EV_THREADS workgroup: the copies zeroed, one barrier
    __device__ __forceinline__ ClassHist() {
        __shared__ unsigned s_h[EV_WAVES][2 * EV_BINS];
        all = &s_h[0][0];
        for (int k = threadIdx.x; k < EV_WAVES * 2 * EV_BINS; k += EV_THREADS) all[k] = 0;
        __syncthreads();
    }
    // one pixel; every lane of the wave calls this together (`in`: the pixel exists and is counted)
    __device__ __forceinline__ void add(unsigned q, bool fg, bool in) {
        const bool lo = in && q == 0u, hi = in && q == 255u;
        sat[0] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(lo && !fg));
        sat[1] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(lo && fg));
        sat[2] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(hi && !fg));
        sat[3] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(hi && fg));
        if (in && !lo && !hi) atomicAdd(&all[(threadIdx.x >> 6) * 2 * EV_BINS + (fg ? EV_BINS : 0) + q], 1u);
    }
    // after the last add: the saturated bins into the wave's copy.  A barrier has to follow before store().
    __device__ __forceinline__ void flush() {
        unsigned* hist = all + (threadIdx.x >> 6) * 2 * EV_BINS;
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&hist[0], sat[0]);
            atomicAdd(&hist[EV_BINS], sat[1]);
            atomicAdd(&hist[EV_BINS - 1], sat[2]);
            atomicAdd(&hist[2 * EV_BINS - 1], sat[3]);
        }
    }
    // the copies of the waves added into slab_h[0 .. 2 * EV_BINS)
    __device__ __forceinline__ void store(unsigned* __restrict__ slab_h) const {
        for (int k = threadIdx.x; k < 2 * EV_BINS; k += EV_THREADS) {
            unsigned a = all[k];
#pragma unroll
            for (int w = 1; w < EV_WAVES; ++w) a += all[w * 2 * EV_BINS + k];
            slab_h[k] = a;
        }
    }
};

// One workgroup of EV_FIN_THREADS threads adds the count slabs of one image (NSUM 64-bit sums, then the 512 bins; `base`: the first slab,
// 8-byte aligned).  That is the long part of a finaliser (512 slabs of 2 KB for a 24-megapixel image, pulled by one CU), so the loads are
// batched: EV_FIN_LANES threads cover the 512 bins of a slab, four bins each, EV_FIN_GROUPS slabs at a time, eight such loads in flight per
// thread; wave 0 adds the sums.  Returns bin threadIdx.x of [bg | fg] to thread threadIdx.x < 512 and leaves the sums in s_sum.  s_cnt is
// staging: afterwards column i has been read by thread i alone, which may reuse it without another barrier.  One barrier.  Integer sums: the
// order does not matter.
constexpr int EV_FIN_THREADS = 1024;
constexpr int EV_FIN_LANES = 2 * EV_BINS / 4;
constexpr int EV_FIN_GROUPS = EV_FIN_THREADS / EV_FIN_LANES;

template <int NSUM>
__device__ __forceinline__ u64 sum_class_slabs(const char* __restrict__ base, int nblk, u64 (&s_cnt)[EV_FIN_GROUPS][2 * EV_BINS], u64 (&s_sum)[NSUM]) {
    constexpr long long SLAB = class_slab_bytes(NSUM);
    {
        const int l = threadIdx.x % EV_FIN_LANES, grp = threadIdx.x / EV_FIN_LANES;
        const char* mine = base + NSUM * 8 + 16 * l;  // bins 4 l .. 4 l + 3 of a slab
        u64 c[4] = {0, 0, 0, 0};
        int j = grp;
        for (; j + 7 * EV_FIN_GROUPS < nblk; j += 8 * EV_FIN_GROUPS) {
            uint2 lo[8], hi[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint2* h = reinterpret_cast<const uint2*>(mine + (long long)(j + u * EV_FIN_GROUPS) * SLAB);
                lo[u] = h[0], hi[u] = h[1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) c[0] += lo[u].x, c[1] += lo[u].y, c[2] += hi[u].x, c[3] += hi[u].y;
        }
        for (; j < nblk; j += EV_FIN_GROUPS) {
            const uint2* h = reinterpret_cast<const uint2*>(mine + (long long)j * SLAB);
            const uint2 lo = h[0], hi = h[1];
            c[0] += lo.x, c[1] += lo.y, c[2] += hi.x, c[3] += hi.y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_cnt[grp][4 * l + k] = c[k];
    }
    if (threadIdx.x < 64) {
        u64 a[NSUM];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) a[k] = 0;
        for (int j = threadIdx.x; j < nblk; j += 64) {
            const u64* sl = reinterpret_cast<const u64*>(base + (long long)j * SLAB);
#pragma unroll
            for (int k = 0; k < NSUM; ++k) a[k] += sl[k];
        }
#pragma unroll
        for (int k = 0; k < NSUM; ++k) a[k] = wave_sum(a[k]);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) s_sum[k] = a[k];
        }
    }
    __syncthreads();
    u64 a = 0;
    if (threadIdx.x < 2 * EV_BINS) {
        a = s_cnt[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < EV_FIN_GROUPS; ++g) a += s_cnt[g][threadIdx.x];
    }
    return a;
}

}  // namespace
