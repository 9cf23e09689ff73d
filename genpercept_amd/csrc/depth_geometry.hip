// Point maps, surface normals and point clouds from a depth prediction on the device (gp_depth_geometry): every pixel is unprojected through
// its image's pinhole camera, gets the normal of a plane fitted in inverse depth to the neighbours on its own side of every depth edge, and is
// kept or dropped as a flying pixel; the kept pixels of the stride grid are compacted into a point cloud.  The definition is stated in
// include/genpercept_hip.h; genpercept_amd/geometry.py restates it on the host and gives the same bits; the per-pixel arithmetic is
// depth_geometry_math.h, which tests/geometry_check.cpp also runs on the CPU.
//   geometry  one workgroup of 512 threads per 32 x 16 pixels of an image.  z and w = 1 / z of the tile plus an apron of r pixels are computed
//             once from the prediction and staged in LDS (16 bytes per pixel, 24 KiB at r = 8); an invalid pixel, and one outside the image,
//             is a NaN z, which fails the membership test by itself.  A thread walks the window of its pixel from LDS in row-major order --
//             a wave's lanes read two runs of 32 consecutive doubles -- and writes the point, the normal and the keep byte.
//   count     one wave per segment: 64 consecutive columns of one row of the stride grid.  The kept pixels of a segment are counted by a
//             ballot and a population count.
//   scan      one workgroup turns the counts of all segments of all images into exclusive offsets, in place (four per thread and step,
//             shuffles inside a wave, LDS across the waves), and writes offsets[B + 1] from them (depth_grid.h, shared with depth_mesh.hip,
//             as are the grid and the addressing of its segments).
//   scatter   a wave per segment again: a kept pixel's place is its segment's offset plus its rank inside the ballot, so the points stand
//             in row-major order, image after image.
// Four launches for any batch after one copy of the cameras (HOST memory) into the workspace, stream-ordered, no atomics, nothing read back.
// Which thread computes which pixel depends on the sizes only, no float sum crosses threads and the counts are integers, so an image's
// planes are the same in every batch and from call to call, and so are its points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"
#include "depth_geometry_math.h"
#include "depth_grid.h"

namespace {

constexpr int DG_TW = 32, DG_TH = 16;        // the tile of the geometry pass
constexpr int DG_THREADS = DG_TW * DG_TH;    // 512: one thread per pixel of the tile

struct DgCall {
    int H, W, space, r, min_count;
    double tau, min_cos;
};

// grid (ceil(W / 32), ceil(H / 16), B).  Dynamic LDS: 16 (32 + 2 r) (16 + 2 r) bytes.  xyz, normal: [B][3][H][W] or NULL; keep_a, keep_b: [B][H][W] or NULL.
__global__ __launch_bounds__(DG_THREADS) void dg_geometry_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ mask,
                                                                const double* __restrict__ cams, DgCall a, float* __restrict__ xyz,
                                                                float* __restrict__ normal, unsigned char* __restrict__ keep_a,
                                                                unsigned char* __restrict__ keep_b) {
    extern __shared__ double s_dg[];
    const int r = a.r, pw = DG_TW + 2 * r, ph = DG_TH + 2 * r, np = pw * ph;
    double* s_z = s_dg;       // [ph][pw]
    double* s_w = s_dg + np;  // [ph][pw]
    const long long b = blockIdx.z, HW = (long long)a.H * a.W;
    const double* cp = cams + b * DG_CAMERA;
    const DgCamera cam = {cp[0], cp[1], cp[2], cp[3], cp[4], cp[5], cp[6], cp[7]};
    const double qnan = __builtin_nan("");
    const int x0 = blockIdx.x * DG_TW - r, y0 = blockIdx.y * DG_TH - r;
    for (int i = threadIdx.x; i < np; i += DG_THREADS) {
        const int py = i / pw, px = i - py * pw, y = y0 + py, x = x0 + px;
        double z = qnan, w = 0.0;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const long long p = b * HW + (long long)y * a.W + x;
            const bool usable = !mask || mask[p] != 0;
            if (!dg_depth(pred[p], usable, cam, a.space, z, w)) z = qnan;
        }
        s_z[i] = z, s_w[i] = w;
    }
    __syncthreads();
    const int tx = threadIdx.x % DG_TW, ty = threadIdx.x / DG_TW;
    const int u = blockIdx.x * DG_TW + tx, v = blockIdx.y * DG_TH + ty;
    if (u >= a.W || v >= a.H) return;
    const int c = (ty + r) * pw + (tx + r);
    const double zi = s_z[c];
    const bool valid = zi == zi;
    DgSums f;
    dg_sums_clear(f);
    if (valid) {
        const double lim = a.tau * zi;
        for (int dv = -r; dv <= r; ++dv) {
            const int row = c + dv * pw;
            for (int du = -r; du <= r; ++du)
                if (dg_member(s_z[row + du], zi, lim)) dg_sums_add(f, du, dv, s_w[row + du]);
        }
    }
    float P[3], N[3];
    const bool kept = dg_pixel(u, v, valid, zi, f, cam, a.min_count, a.min_cos, P, N);
    const long long q = (long long)v * a.W + u;
    if (xyz) {
        float* o = xyz + b * 3 * HW + q;
        o[0] = P[0], o[HW] = P[1], o[2 * HW] = P[2];
    }
    if (normal) {
        float* o = normal + b * 3 * HW + q;
        o[0] = N[0], o[HW] = N[1], o[2 * HW] = N[2];
    }
    if (keep_a) keep_a[b * HW + q] = kept ? 1 : 0;
    if (keep_b) keep_b[b * HW + q] = kept ? 1 : 0;
}

// Segment `seg` of `total` = B gh nseg: its image, the pixel of its lane on the stride grid, and whether that pixel exists and is kept.
struct DgLane {
    long long b;
    int pix;    // v W + u
    bool kept;
    __device__ __forceinline__ DgLane(const unsigned char* __restrict__ keep, const DgGrid& g, int seg, int lane) {
        const DgNode n(g, seg, lane);
        b = n.b, pix = n.pix;
        kept = n.exists && keep[b * g.H * g.W + pix] != 0;
    }
};

// one wave per segment.  counts: [total].
__global__ __launch_bounds__(EV_THREADS) void dg_count_kernel(const unsigned char* __restrict__ keep, DgGrid g, int total, unsigned* __restrict__ counts) {
    const long long seg = (long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);  // (wave-uniform)
    if (seg >= total) return;
    const int lane = threadIdx.x & 63;
    const DgLane l(keep, g, (int)seg, lane);
    const u64 m = __builtin_amdgcn_ballot_w64(l.kept);
    if (lane == 0) counts[seg] = (unsigned)__popcll(m);
}

// one wave per segment.  first: [total], the exclusive prefix sums.  xyz, normal: the planes [B][3][H][W].
__global__ __launch_bounds__(EV_THREADS) void dg_scatter_kernel(const unsigned char* __restrict__ keep, const unsigned* __restrict__ first, DgGrid g, int total,
                                                               const float* __restrict__ xyz, const float* __restrict__ normal,
                                                               const unsigned char* __restrict__ image, float* __restrict__ points,
                                                               float* __restrict__ point_normals, unsigned char* __restrict__ point_rgb,
                                                               int* __restrict__ point_index) {
    const long long seg = (long long)blockIdx.x * EV_WAVES + (threadIdx.x >> 6);  // (wave-uniform)
    if (seg >= total) return;
    const int lane = threadIdx.x & 63;
    const DgLane l(keep, g, (int)seg, lane);
    const u64 m = __builtin_amdgcn_ballot_w64(l.kept);
    if (!l.kept) return;
    const long long dst = (long long)first[seg] + __popcll(m & ((1ull << lane) - 1ull)), HW = (long long)g.H * g.W, src = l.b * 3 * HW + l.pix;
    if (points) {
        float* o = points + 3 * dst;
        o[0] = xyz[src], o[1] = xyz[src + HW], o[2] = xyz[src + 2 * HW];
    }
    if (point_normals) {
        float* o = point_normals + 3 * dst;
        o[0] = normal[src], o[1] = normal[src + HW], o[2] = normal[src + 2 * HW];
    }
    if (point_rgb) {
        unsigned char* o = point_rgb + 3 * dst;
        o[0] = image ? image[src] : 255, o[1] = image ? image[src + HW] : 255, o[2] = image ? image[src + 2 * HW] : 255;
    }
    if (point_index) point_index[dst] = l.pix;
}

// Per image: its camera (64 bytes), the counts of its segments, its keep bytes, its two sets of three float planes; every part a multiple of
// 8 bytes.  The parts of all images stand together: cameras, counts, keep, xyz planes, normal planes.
struct DgWorkspace {
    long long cams, counts, keep, xyz, normal, bytes;  // offsets of the parts; the size
    DgWorkspace(int B, int H, int W, int stride) {
        const DgGrid g = dg_grid(H, W, stride);
        const long long HW = (long long)H * W;
        cams = 0;
        counts = cams + (long long)B * DG_CAMERA * 8;
        keep = counts + B * dg_round8(4LL * g.gh * g.nseg);
        xyz = keep + B * dg_round8(HW);
        normal = xyz + B * 12 * HW;
        bytes = normal + B * 12 * HW;
    }
};

}  // namespace

extern "C" {

long long gp_depth_geometry_workspace(int B, int H, int W, int stride) { return dg_dims_ok(B, H, W, stride) ? DgWorkspace(B, H, W, stride).bytes : 0; }

gp_status gp_depth_geometry(const float* pred, const unsigned char* mask, const unsigned char* image, const double* cameras, int B, int H, int W, int space,
                            int r, double tau, int min_count, double min_cos, int stride, float* xyz, float* normal, unsigned char* keep, float* points,
                            float* point_normals, unsigned char* point_rgb, int* point_index, long long* offsets, void* workspace,
                            long long workspace_bytes, void* stream) {
    if (!pred || !cameras || !workspace) return GP_ERR_INVALID;
    if (!dg_dims_ok(B, H, W, stride) || !dg_options_ok(space, r, tau, min_count, min_cos, stride)) return GP_ERR_INVALID;
    for (int k = 0; k < B; ++k)
        if (!dg_camera_ok(cameras + (long long)k * DG_CAMERA)) return GP_ERR_INVALID;
    const bool any_points = points || point_normals || point_rgb || point_index;
    if (any_points && !offsets) return GP_ERR_INVALID;          // the caller cannot tell how many points there are
    if (!xyz && !normal && !keep && !offsets) return GP_ERR_INVALID;  // nothing to do
    if ((((uintptr_t)pred | (uintptr_t)xyz | (uintptr_t)normal | (uintptr_t)points | (uintptr_t)point_normals | (uintptr_t)point_index) & 3) != 0 ||
        !eval_aligned8(offsets, (const char*)workspace))
        return GP_ERR_INVALID;
    const DgWorkspace ws(B, H, W, stride);
    if (workspace_bytes < ws.bytes) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    char* wp = (char*)workspace;
    double* cams_d = (double*)(wp + ws.cams);
    unsigned* counts = (unsigned*)(wp + ws.counts);
    unsigned char* keep_w = offsets ? (unsigned char*)(wp + ws.keep) : nullptr;
    // the scatter reads the planes: the caller's where given, the workspace's otherwise
    float* xyz_w = xyz ? xyz : (points ? (float*)(wp + ws.xyz) : nullptr);
    float* normal_w = normal ? normal : (point_normals ? (float*)(wp + ws.normal) : nullptr);
    if (hipMemcpyAsync(cams_d, cameras, (size_t)B * DG_CAMERA * 8, hipMemcpyHostToDevice, s) != hipSuccess) return GP_ERR_HIP;
    const DgCall a = {H, W, space, r, min_count, tau, min_cos};
    const size_t lds = (size_t)16 * (DG_TW + 2 * r) * (DG_TH + 2 * r);
    hipLaunchKernelGGL(dg_geometry_kernel, dim3((W + DG_TW - 1) / DG_TW, (H + DG_TH - 1) / DG_TH, B), dim3(DG_THREADS), lds, s, pred, mask,
                       (const double*)cams_d, a, xyz_w, normal_w, keep, keep_w);
    if (offsets) {
        const DgGrid g = dg_grid(H, W, stride);
        const int per_image = g.gh * g.nseg, total = B * per_image;  // (at most B H W < 2^31)
        const unsigned nblk = (unsigned)((total + EV_WAVES - 1) / EV_WAVES);
        hipLaunchKernelGGL(dg_count_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, (const unsigned char*)keep_w, g, total, counts);
        hipLaunchKernelGGL(dg_scan_kernel, dim3(1), dim3(DG_SCAN_THREADS), 0, s, counts, 0LL, total, per_image, B, offsets, (long long*)nullptr);
        if (any_points)
            hipLaunchKernelGGL(dg_scatter_kernel, dim3(nblk), dim3(EV_THREADS), 0, s, (const unsigned char*)keep_w, (const unsigned*)counts, g, total,
                               (const float*)xyz_w, (const float*)normal_w, image, points, point_normals, point_rgb, point_index);
    }
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
