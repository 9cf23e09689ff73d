// What the evaluation kernels of eval.hip and eval_structure.hip share: the workgroup shape, the slab count rule, the fixed-order float64
// reductions and the 8-bit quantisation of a mask prediction.  Include after <hip/hip_runtime.h>.
#pragma once

// The host's numpy code has no fused multiply-adds: nothing here, and nothing in the files that include this one, may be contracted into one.
#pragma clang fp contract(off)

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr long long EV_PIX_PER_WG = 4096;  // at least this many pixels per workgroup ...
constexpr int EV_MAX_WG = 512;             // ... and at most this many workgroups (= slabs) per image

inline int eval_blocks(long long hw) {
    long long g = (hw + EV_PIX_PER_WG - 1) / EV_PIX_PER_WG;
    return (int)(g < 1 ? 1 : (g > EV_MAX_WG ? EV_MAX_WG : g));
}

// v[0..N) of every thread -> their sums over the workgroup, in slab[0..N).  Fixed order: a 64-lane shuffle tree inside each wave (the
// shuffle moves the two halves of a double), then the waves in index order through LDS.
template <int N>
__device__ __forceinline__ void block_reduce_store(double (&v)[N], double* __restrict__ slab) {
    __shared__ double s_part[EV_WAVES][N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_part[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double a = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EV_WAVES; ++w) a += s_part[w][threadIdx.x];
        slab[threadIdx.x] = a;
    }
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

// run.py:449-455 on one value: clip to [0, 1] (NaN -> 0), * 255 in fp32, truncate
__device__ __forceinline__ unsigned quantise8(float x) {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
    return (unsigned)(unsigned char)(c * 255.0f);
}

}  // namespace
