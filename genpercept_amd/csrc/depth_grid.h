// What the two ops that compact the stride grid of an image share (depth_geometry.hip: the kept pixels as a point cloud; depth_mesh.hip: the
// used nodes as vertices and the cells' triangles as faces): the grid and its rows in segments of 64 nodes, a wave per segment; which node a
// lane of a segment is; the one-workgroup scan that turns per-segment counts into exclusive offsets and the per-image offsets array; the
// size checks and the rounding of a workspace part.  Include after <hip/hip_runtime.h> and eval_common.h.
#pragma once

#include <stdint.h>

#include "depth_geometry_math.h"   // DG_MAX_DIM, DG_MAX_STRIDE

namespace {

constexpr int DG_SCAN_THREADS = 1024;
constexpr int DG_SCAN_WAVES = DG_SCAN_THREADS / 64;
constexpr int DG_SCAN_PER = 4;               // counts per thread and step of the scan

// the stride grid: gh x gw pixels, a row of it in nseg segments of 64
struct DgGrid {
    int H, W, stride, gh, gw, nseg;
};

inline DgGrid dg_grid(int H, int W, int stride) {
    const int gh = (H + stride - 1) / stride, gw = (W + stride - 1) / stride;
    return {H, W, stride, gh, gw, (gw + 63) / 64};
}

inline bool dg_dims_ok(int B, int H, int W, int stride) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= DG_MAX_DIM && W <= DG_MAX_DIM && (long long)B * H * W <= 0x7fffffffLL && stride >= 1 &&
           stride <= DG_MAX_STRIDE;
}

inline long long dg_round8(long long n) { return (n + 7) / 8 * 8; }

// Lane `lane` of segment `seg` of B gh nseg: its image, its node (gy, gx) of the stride grid, its segment's place sx in the row, the node's
// pixel and whether the node exists (the last segment of a row may be partial).
struct DgNode {
    long long b;
    int gy, gx, sx;
    int pix;    // v W + u
    bool exists;
    __device__ __forceinline__ DgNode(const DgGrid& g, int seg, int lane) {
        const int t = seg / g.nseg;
        sx = seg % g.nseg, gy = t % g.gh, gx = sx * 64 + lane;
        b = t / g.gh;
        pix = gy * g.stride * g.W + gx * g.stride;   // (gy stride < H; gx stride < W where gx < gw)
        exists = gx < g.gw;
    }
};

// One workgroup per array of counts: array k = blockIdx.x (0 or 1) is counts + k * second and writes offsets0 or offsets1.  counts [total]
// become their exclusive prefix sums (below 2^31); offsets[k] = the prefix of image k's first segment, offsets[B] = the sum.
__global__ __launch_bounds__(DG_SCAN_THREADS) void dg_scan_kernel(unsigned* __restrict__ counts, long long second, int total, int per_image, int B,
                                                                  long long* __restrict__ offsets0, long long* __restrict__ offsets1) {
    __shared__ unsigned s_wave[DG_SCAN_WAVES];
    counts += blockIdx.x * second;
    long long* __restrict__ offsets = blockIdx.x ? offsets1 : offsets0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;
    for (long long base = 0; base < total; base += DG_SCAN_THREADS * DG_SCAN_PER) {
        const long long i0 = base + (long long)threadIdx.x * DG_SCAN_PER;
        unsigned v[DG_SCAN_PER], mine = 0;
#pragma unroll
        for (int k = 0; k < DG_SCAN_PER; ++k) {
            v[k] = i0 + k < total ? counts[i0 + k] : 0u;
            mine += v[k];
        }
        unsigned incl = mine;  // the inclusive sum of the wave's lanes up to this one
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < DG_SCAN_WAVES; ++k) {
            const unsigned t = s_wave[k];
            before += k < wave ? t : 0u;
            all += t;
        }
        unsigned run = carry + before + (incl - mine);
#pragma unroll
        for (int k = 0; k < DG_SCAN_PER; ++k) {
            if (i0 + k < total) counts[i0 + k] = run;
            run += v[k];
        }
        carry += all;
        __syncthreads();  // s_wave is written again in the next step
    }
    // (the barrier above orders this workgroup's own stores before these loads)
    for (int k = threadIdx.x; k < B; k += DG_SCAN_THREADS) offsets[k] = (long long)counts[(long long)k * per_image];
    if (threadIdx.x == 0) offsets[B] = (long long)carry;
}

}  // namespace
