// Triangle meshes from the point map of a depth prediction on the device (gp_depth_mesh): the nodes of the stride grid are joined to their
// neighbours wherever both are kept and their depths are close, every cell of four nodes gives up to two triangles on the diagonal that
// crosses the smaller depth difference, the nodes that a triangle uses are compacted into vertices and the triangles into faces.  The
// definition is stated in include/genpercept_hip.h; genpercept_amd/mesh.py restates it on the host and gives the same bits; the per-cell
// arithmetic is depth_mesh_math.h, which tests/mesh_check.cpp also runs on the CPU.  The grid, its segments and the scan are depth_grid.h,
// shared with depth_geometry.hip.
//   codes     one thread per node: the four-bit code of the cell whose corner a the node is (0 in the last row and column) into a byte plane
//             of the workspace.  A cell reads z and keep of two adjacent nodes in two grid rows; the neighbours' reads are served by the cache.
//   count     one wave per segment of 64 nodes of a grid row.  A node is a vertex iff a triangle of one of its four cells uses it: the
//             ballot of that is the segment's used mask, kept as a 64-bit word, and its population count the vertex count; the face count is
//             the population count of the ballots "the cell emits a triangle" and "the cell emits two".
//   scan      one launch, a workgroup for each of the two count arrays: exclusive offsets in place and the two offsets[B + 1] arrays.
//   scatter   a wave per segment again.  A vertex's place is its segment's offset plus its rank in the used mask; a face's place is its
//             segment's face offset plus the triangles of the lanes below.  The index of a corner in the next segment or the next row is that
//             segment's offset plus the population count of its stored mask below the corner's lane: no index plane.
// Four launches for any batch, stream-ordered, no atomics, nothing read back.  Which thread handles which node depends on the sizes only and
// the counts are integers, so an image's mesh is the same in every batch and from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"
#include "depth_mesh_math.h"
#include "depth_grid.h"

namespace {

// one thread per node of B gh gw (below 2^30).  xyz: [B][3][H][W]; keep: [B][H][W]; codes: [B][gh][gw].
__global__ __launch_bounds__(EV_THREADS) void dm_codes_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ keep, DgGrid g, int nodes,
                                                             double cut, unsigned char* __restrict__ codes) {
    const int i = (int)(blockIdx.x * (unsigned)EV_THREADS + threadIdx.x);
    if (i >= nodes) return;
    const int gx = i % g.gw, t = i / g.gw, gy = t % g.gh;
    const long long b = t / g.gh, HW = (long long)g.H * g.W;
    unsigned code = 0;
    if (gx + 1 < g.gw && gy + 1 < g.gh) {
        // (the nodes right of and below this one exist, so their pixels lie inside the image)
        const long long pa = (long long)gy * g.stride * g.W + (long long)gx * g.stride, pb = pa + g.stride, pc = pa + (long long)g.stride * g.W, pd = pc + g.stride;
        const float* z = xyz + b * 3 * HW + 2 * HW;
        const unsigned char* k = keep + b * HW;
        code = dm_cell_code(k[pa] != 0, (double)z[pa], k[pb] != 0, (double)z[pb], k[pc] != 0, (double)z[pc], k[pd] != 0, (double)z[pd], cut);
    }
    codes[i] = (unsigned char)code;
}

// What a lane of a segment knows of its node from the code plane: the code of its own cell and whether the node is a vertex.
struct DmLane {
    unsigned code;
    bool used;
    __device__ __forceinline__ DmLane(const unsigned char* __restrict__ codes, const DgGrid& g, const DgNode& n) {
        code = 0, used = false;
        if (!n.exists) return;
        const unsigned char* c = codes + ((n.b * g.gh + n.gy) * g.gw + n.gx);
        code = c[0];
        const unsigned left = n.gx > 0 ? c[-1] : 0u, up = n.gy > 0 ? c[-g.gw] : 0u, up_left = n.gx > 0 && n.gy > 0 ? c[-g.gw - 1] : 0u;
        used = dm_node_used(code, left, up, up_left);
    }
};

__device__ __forceinline__ u64 dm_below(int lane) { return (1ull << lane) - 1ull; }

// one wave per segment.  vcount, fcount: [total]; used: [total], the segments' masks.
__global__ __launch_bounds__(EV_THREADS) void dm_count_kernel(const unsigned char* __restrict__ codes, DgGrid g, int total, unsigned* __restrict__ vcount,
                                                             unsigned* __restrict__ fcount, u64* __restrict__ used) {
    const long long seg = (long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);  // (wave-uniform)
    if (seg >= total) return;
    const int lane = threadIdx.x & 63;
    const DgNode n(g, (int)seg, lane);
    const DmLane l(codes, g, n);
    const u64 m = __builtin_amdgcn_ballot_w64(l.used);
    const u64 one = __builtin_amdgcn_ballot_w64(dm_code_count(l.code) >= 1), two = __builtin_amdgcn_ballot_w64(dm_code_count(l.code) == 2);
    if (lane == 0) {
        vcount[seg] = (unsigned)__popcll(m);
        fcount[seg] = (unsigned)(__popcll(one) + __popcll(two));
        used[seg] = m;
    }
}

// one wave per segment.  vfirst, ffirst: [total], the exclusive prefix sums; used: [total].  xyz, normal: the planes [B][3][H][W].
__global__ __launch_bounds__(EV_THREADS) void dm_scatter_kernel(const unsigned char* __restrict__ codes, const unsigned* __restrict__ vfirst,
                                                               const unsigned* __restrict__ ffirst, const u64* __restrict__ used, DgGrid g, int total,
                                                               const float* __restrict__ xyz, const float* __restrict__ normal,
                                                               const unsigned char* __restrict__ image, float* __restrict__ vertices,
                                                               float* __restrict__ vertex_normals, unsigned char* __restrict__ vertex_rgb,
                                                               float* __restrict__ vertex_uv, int* __restrict__ vertex_index, int* __restrict__ faces) {
    const int seg = (int)((long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6));  // (wave-uniform)
    if (seg >= total) return;
    const int lane = threadIdx.x & 63;
    const DgNode n(g, seg, lane);
    if (!n.exists) return;
    const u64 m = used[seg];
    const unsigned v0 = vfirst[seg];
    if ((m >> lane) & 1ull) {
        const long long dst = (long long)v0 + __popcll(m & dm_below(lane)), HW = (long long)g.H * g.W, src = n.b * 3 * HW + n.pix;
        if (vertices) {
            float* o = vertices + 3 * dst;
            o[0] = xyz[src], o[1] = xyz[src + HW], o[2] = xyz[src + 2 * HW];
        }
        if (vertex_normals) {
            float* o = vertex_normals + 3 * dst;
            o[0] = normal[src], o[1] = normal[src + HW], o[2] = normal[src + 2 * HW];
        }
        if (vertex_rgb) {
            unsigned char* o = vertex_rgb + 3 * dst;
            o[0] = image ? image[src] : 255, o[1] = image ? image[src + HW] : 255, o[2] = image ? image[src + 2 * HW] : 255;
        }
        if (vertex_uv) {
            const int v = n.gy * g.stride, u = n.gx * g.stride;
            vertex_uv[2 * dst] = dm_uv(u, g.W), vertex_uv[2 * dst + 1] = dm_uv(v, g.H);
        }
        if (vertex_index) vertex_index[dst] = n.pix;
    }
    if (!faces) return;
    const unsigned code = codes[(n.b * g.gh + n.gy) * g.gw + n.gx];
    // the triangles of the lanes below, from the codes of the whole segment: every lane that exists is still here
    const u64 one = __builtin_amdgcn_ballot_w64(dm_code_count(code) >= 1), two = __builtin_amdgcn_ballot_w64(dm_code_count(code) == 2);
    if (code == 0) return;
    // A cell exists only where the node right of it and the row below do: their segments are inside this image, and every corner a
    // triangle names is a vertex, so its rank in its segment's mask is its place.
    const int below_row = seg + g.nseg;
    const bool last_lane = lane == 63;
    const int seg_b = last_lane ? seg + 1 : seg, seg_d = last_lane ? below_row + 1 : below_row, lane_r = last_lane ? 0 : lane + 1;
    const unsigned base = vfirst[(int)(n.b * g.gh * g.nseg)];   // the image's first vertex: face indices are local to the image
    const int a = (int)(v0 - base) + __popcll(m & dm_below(lane));
    const int b = (int)(vfirst[seg_b] - base) + __popcll(used[seg_b] & dm_below(lane_r));
    const int c = (int)(vfirst[below_row] - base) + __popcll(used[below_row] & dm_below(lane));
    const int d = (int)(vfirst[seg_d] - base) + __popcll(used[seg_d] & dm_below(lane_r));
    long long dst = (long long)ffirst[seg] + __popcll(one & dm_below(lane)) + __popcll(two & dm_below(lane));
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        int t[3];
        if (dm_triangle(code, slot, a, b, c, d, t)) {
            int* o = faces + 3 * dst;
            o[0] = t[0], o[1] = t[1], o[2] = t[2];
            ++dst;
        }
    }
}

inline bool dm_dims_ok(int B, int H, int W, int stride) {
    if (!dg_dims_ok(B, H, W, stride)) return false;
    const DgGrid g = dg_grid(H, W, stride);
    return (long long)B * g.gh * g.gw < DM_MAX_NODES;
}

// Per image: the codes of its nodes, the vertex counts and the face counts of its segments, their used masks; every part a multiple of 8
// bytes.  The parts of all images stand together: the two count arrays first and side by side, which the scan relies on.
struct DmWorkspace {
    long long vcount, fcount, used, codes, bytes;  // offsets of the parts; the size
    DmWorkspace(int B, int H, int W, int stride) {
        const DgGrid g = dg_grid(H, W, stride);
        const long long per_image = (long long)g.gh * g.nseg;
        vcount = 0;
        fcount = vcount + B * dg_round8(4 * per_image);
        used = fcount + B * dg_round8(4 * per_image);
        codes = used + B * 8 * per_image;
        bytes = codes + B * dg_round8((long long)g.gh * g.gw);
    }
};

}  // namespace

extern "C" {

long long gp_depth_mesh_workspace(int B, int H, int W, int stride) { return dm_dims_ok(B, H, W, stride) ? DmWorkspace(B, H, W, stride).bytes : 0; }

gp_status gp_depth_mesh(const float* xyz, const float* normal, const unsigned char* keep, const unsigned char* image, int B, int H, int W, int stride,
                        double cut, float* vertices, float* vertex_normals, unsigned char* vertex_rgb, float* vertex_uv, int* vertex_index, int* faces,
                        long long* vertex_offsets, long long* face_offsets, void* workspace, long long workspace_bytes, void* stream) {
    if (!xyz || !keep || !vertex_offsets || !face_offsets || !workspace) return GP_ERR_INVALID;
    if (!dm_dims_ok(B, H, W, stride) || !dm_cut_ok(cut)) return GP_ERR_INVALID;
    if (vertex_normals && !normal) return GP_ERR_INVALID;
    if ((((uintptr_t)xyz | (uintptr_t)normal | (uintptr_t)vertices | (uintptr_t)vertex_normals | (uintptr_t)vertex_uv | (uintptr_t)vertex_index |
          (uintptr_t)faces) & 3) != 0 ||
        !eval_aligned8(vertex_offsets, face_offsets, (const char*)workspace))
        return GP_ERR_INVALID;
    const DmWorkspace ws(B, H, W, stride);
    if (workspace_bytes < ws.bytes) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    char* wp = (char*)workspace;
    unsigned* vcount = (unsigned*)(wp + ws.vcount);
    unsigned* fcount = (unsigned*)(wp + ws.fcount);
    u64* used = (u64*)(wp + ws.used);
    unsigned char* codes = (unsigned char*)(wp + ws.codes);
    const DgGrid g = dg_grid(H, W, stride);
    const int per_image = g.gh * g.nseg, total = B * per_image, nodes = B * g.gh * g.gw;  // (nodes < 2^30)
    const unsigned nblk = (unsigned)((total + EV_WAVES - 1) / EV_WAVES);
    hipLaunchKernelGGL(dm_codes_kernel, dim3((unsigned)((nodes + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, s, xyz, keep, g, nodes, cut, codes);
    hipLaunchKernelGGL(dm_count_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, (const unsigned char*)codes, g, total, vcount, fcount, used);
    hipLaunchKernelGGL(dg_scan_kernel, dim3(2), dim3(DG_SCAN_THREADS), 0, s, vcount, (long long)(fcount - vcount), total, per_image, B, vertex_offsets,
                       face_offsets);
    if (vertices || vertex_normals || vertex_rgb || vertex_uv || vertex_index || faces)
        hipLaunchKernelGGL(dm_scatter_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, (const unsigned char*)codes, (const unsigned*)vcount, (const unsigned*)fcount,
                           (const u64*)used, g, total, xyz, normal, image, vertices, vertex_normals, vertex_rgb, vertex_uv, vertex_index, faces);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
