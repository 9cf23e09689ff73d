// Dis structure scores on the device (gp_eval_structure): S-measure (Fan 2017), E-measure (Fan 2018) and the weighted F-measure (Margolin
// 2014) of an 8-bit prediction q against a binary ground truth G = g > 128, per image.  The definitions are stated once in
// include/genpercept_hip.h; eval_metrics.structure_counts / structure_from_counts / edt_keys / weighted_f restate them on the host.
//   counts    one pass like eval.hip's mask count pass: q (quantised here and kept as bytes for the later passes), the two class histograms
//             (integer LDS atomics, one copy per wave, bins 0 and 255 by ballot + population count), n_fg, sum_fg x, sum_fg y; one slab per
//             workgroup.  A one-workgroup-per-image finaliser adds the slabs and leaves the 64-bit histograms and n_fg, sums, cx, cy.
//   quadrants the 4 x 4 integer sums a, a2, b, c of the blocks the centroid cuts, one slab per workgroup.
//   EDT       exact, two passes.  Columns: one lane per column, a down scan and an up scan (in separate workgroups) leave (du, dd), the distances to the nearest
//             foreground pixel at-or-above and at-or-below (0xffff: none), two 16-bit halves of one word per pixel.  Rows: one workgroup per
//             row turns each column's pair into its better candidate key (d2 << 32 | index) in LDS (a row wider than ES_ROW_LDS reads the
//             pairs from global memory instead); pixel x minimises key(x') + ((x - x')^2 << 32) outwards from x and stops once dx^2 exceeds
//             the best d2 (four offsets at a time).  The 64-bit minimum is the tie rule: smallest d2, then smallest row-major index.
//   weights   32 x 8 tiles: Et = (255 - q[idx]) / 255.0 gathered through the keys into LDS with a 3-pixel apron, the 49 taps in row-major
//             order in float64, Ew per pixel, two float64 sums per tile in block_reduce_store's fixed order.
//   values    one workgroup per image: thread t the E-measure at threshold t, thread 0 the rest, each value one fixed sequence of correctly
//             rounded float64 operations (this file contracts nothing), so the host's restatement of S and E is bit-equal.
// Seven launches for every B, stream-ordered, no global atomics, nothing read back.  Every workgroup count and every pixel -> thread
// assignment depends on H and W alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ES_BINS = EV_BINS;
constexpr int ES_OUT = 15;                          // n, n_fg, s_alpha, s_object, s_region, max_e, mean_e, adp_e, wf, wf_precision, wf_recall, sums, cx, cy
constexpr int ES_HEAD = 5;                          // counts_out: n_fg, sum x, sum y, cx, cy ...
constexpr int ES_NQUAD = 16;                        // ... 4 x (a, a2, b, c) in the slabs, 4 x (N, a, a2, b, c) in counts_out ...
constexpr int ES_COUNTS = ES_HEAD + 20 + 2 * ES_BINS;  // ... hist_bg, hist_fg
constexpr int ES_NSUM = 3;                          // n_fg, sum x, sum y
constexpr long long ES_CSLAB = class_slab_bytes(ES_NSUM);  // a count slab: three 64-bit sums, 512 32-bit bins
constexpr int ES_INFO = 8;                          // 64-bit words per image: n_fg, sum x, sum y, cx, cy, 3 spare
constexpr int ES_TW = 32, ES_TH = 8, ES_AP = 3;     // the weighting tile and its apron
constexpr int ES_COL_THREADS = 64;
constexpr int ES_COL_BATCH = 16;                    // rows of a column scan whose loads are in flight together
constexpr int ES_ROW_GROUP = 4;                     // offsets of the row search examined together
constexpr int ES_ROW_LDS = 8192;                    // columns of a row whose candidate keys are staged in LDS (64 KiB)
constexpr unsigned ES_NONE16 = 0xffffu;
constexpr u64 ES_NOKEY = ~0ull;                     // the key of every pixel of an image without foreground
constexpr u64 ES_FAR = (0x7fffffffull << 32) | 0xffffffffull;  // a column without foreground: above every real key, room for + (dx^2 << 32)

// the normalised 7 x 7 Gaussian, sigma = 5 (the same literals as eval_metrics.WF_K)
__constant__ double ES_K[49] = {
    0x1.1075d7f1e0af6p-6, 0x1.2d1d7fa535fb0p-6, 0x1.3fbc331b753f8p-6, 0x1.4631b947fa56fp-6, 0x1.3fbc331b753f8p-6, 0x1.2d1d7fa535fb0p-6, 0x1.1075d7f1e0af6p-6,
    0x1.2d1d7fa535fb0p-6, 0x1.4cc8a6b9e9761p-6, 0x1.615cabadc2e2fp-6, 0x1.688018ee505f7p-6, 0x1.615cabadc2e2fp-6, 0x1.4cc8a6b9e9761p-6, 0x1.2d1d7fa535fb0p-6,
    0x1.3fbc331b753f8p-6, 0x1.615cabadc2e2fp-6, 0x1.77367232eb477p-6, 0x1.7ecadfe6d5847p-6, 0x1.77367232eb477p-6, 0x1.615cabadc2e2fp-6, 0x1.3fbc331b753f8p-6,
    0x1.4631b947fa56fp-6, 0x1.688018ee505f7p-6, 0x1.7ecadfe6d5847p-6, 0x1.8686809d3875ep-6, 0x1.7ecadfe6d5847p-6, 0x1.688018ee505f7p-6, 0x1.4631b947fa56fp-6,
    0x1.3fbc331b753f8p-6, 0x1.615cabadc2e2fp-6, 0x1.77367232eb477p-6, 0x1.7ecadfe6d5847p-6, 0x1.77367232eb477p-6, 0x1.615cabadc2e2fp-6, 0x1.3fbc331b753f8p-6,
    0x1.2d1d7fa535fb0p-6, 0x1.4cc8a6b9e9761p-6, 0x1.615cabadc2e2fp-6, 0x1.688018ee505f7p-6, 0x1.615cabadc2e2fp-6, 0x1.4cc8a6b9e9761p-6, 0x1.2d1d7fa535fb0p-6,
    0x1.1075d7f1e0af6p-6, 0x1.2d1d7fa535fb0p-6, 0x1.3fbc331b753f8p-6, 0x1.4631b947fa56fp-6, 0x1.3fbc331b753f8p-6, 0x1.2d1d7fa535fb0p-6, 0x1.1075d7f1e0af6p-6};
constexpr double ES_WF_C = -0x1.1be9bff2e94bfp-3;   // log(0.5) / 5

// the workspace of a batch: byte offsets of its parts (each a multiple of 8 and proportional to B)
struct StructWs {
    long long cslab, hist, info, qslab, wslab, dudd, keys, qbuf, total, hwp;
    int nblk, tx, ty;
};

StructWs struct_ws(long long B, int H, int W) {
    StructWs w;
    const long long hw = (long long)H * W;
    w.hwp = (hw + 7) / 8 * 8;
    w.nblk = eval_blocks(hw);
    w.tx = (W + ES_TW - 1) / ES_TW, w.ty = (H + ES_TH - 1) / ES_TH;
    long long o = 0;
    w.cslab = o, o += B * w.nblk * ES_CSLAB;
    w.hist = o, o += B * 2 * ES_BINS * 8;
    w.info = o, o += B * ES_INFO * 8;
    w.qslab = o, o += B * w.nblk * ES_NQUAD * 8;
    w.wslab = o, o += B * w.tx * w.ty * 2 * 8;
    w.dudd = o, o += B * w.hwp * 4;
    w.keys = o, o += B * hw * 8;
    w.qbuf = o, o += B * w.hwp;
    w.total = o;
    return w;
}

// ---- counts -------------------------------------------------------------------------------------------------------------------------------
// grid (eval_blocks(H * W), B).  Integer sums do not depend on their order.
template <bool U8>
__global__ __launch_bounds__(EV_THREADS) void st_count_kernel(const void* __restrict__ pred_v, const unsigned char* __restrict__ gt, unsigned W,
                                                              long long hw, long long hwp, char* __restrict__ cslab,
                                                              unsigned char* __restrict__ qbuf) {
    const long long b = blockIdx.y;
    const Pred8<U8> pred(pred_v, b * hw);
    gt += b * hw, qbuf += b * hwp;
    ClassHist hist;
    u64 v[ES_NSUM] = {0, 0, 0};
    const long long stride = (long long)gridDim.x * EV_THREADS;
    // (workgroup-uniform bounds: the ballots see whole waves)
    for (long long i0 = (long long)blockIdx.x * EV_THREADS; i0 < hw; i0 += stride) {
        const long long i = i0 + threadIdx.x;
        const bool in = i < hw;
        unsigned q = 0, g = 0;
        if (in) {
            q = pred[i];
            g = gt[i];
            qbuf[i] = (unsigned char)q;
        }
        const bool fg = g > 128u;
        if (in && fg) {
            const unsigned y = (unsigned)i / W;
            v[0] += 1, v[1] += (unsigned)i - y * W, v[2] += y;
        }
        hist.add(q, fg, in);
    }
    hist.flush();
    const u64 a = block_sum(v);  // (its barrier: every wave's histogram is complete)
    char* slab = cslab + (b * gridDim.x + blockIdx.x) * ES_CSLAB;
    if (threadIdx.x < ES_NSUM) reinterpret_cast<u64*>(slab)[threadIdx.x] = a;
    hist.store(reinterpret_cast<unsigned*>(slab + ES_NSUM * 8));
}

// one workgroup per image: the slabs added (sum_class_slabs), the centroid (halves rounded up; 0, 0 without foreground)
__global__ __launch_bounds__(EV_FIN_THREADS) void st_centroid_kernel(const char* __restrict__ cslab, int nblk, u64* __restrict__ hist,
                                                                     u64* __restrict__ info) {
    __shared__ u64 s_cnt[EV_FIN_GROUPS][2 * ES_BINS], s_sum[ES_NSUM];
    const long long b = blockIdx.x;
    const u64 bin = sum_class_slabs<ES_NSUM>(cslab + b * nblk * ES_CSLAB, nblk, s_cnt, s_sum);
    if (threadIdx.x < 2 * ES_BINS) hist[b * 2 * ES_BINS + threadIdx.x] = bin;
    if (threadIdx.x == 0) {
        const u64 n_fg = s_sum[0], sx = s_sum[1], sy = s_sum[2];
        u64* o = info + b * ES_INFO;
        o[0] = n_fg, o[1] = sx, o[2] = sy;
        o[3] = n_fg ? (2 * sx + n_fg) / (2 * n_fg) : 0;
        o[4] = n_fg ? (2 * sy + n_fg) / (2 * n_fg) : 0;
        o[5] = o[6] = o[7] = 0;
    }
}

// ---- quadrants ----------------------------------------------------------------------------------------------------------------------------
// grid (eval_blocks(H * W), B).  Block k = 2 (y > cy) + (x > cx): LT, RT, LB, RB; per block a = sum q, a2 = sum q^2, b = sum G, c = sum q G.
__global__ __launch_bounds__(EV_THREADS) void st_quad_kernel(const unsigned char* __restrict__ qbuf, const unsigned char* __restrict__ gt,
                                                             const u64* __restrict__ info, unsigned W, long long hw, long long hwp,
                                                             u64* __restrict__ qslab) {
    const long long b = blockIdx.y;
    qbuf += b * hwp, gt += b * hw;
    const unsigned cx = (unsigned)info[b * ES_INFO + 3], cy = (unsigned)info[b * ES_INFO + 4];
    u64 acc[ES_NQUAD];
#pragma unroll
    for (int k = 0; k < ES_NQUAD; ++k) acc[k] = 0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < hw; i += stride) {
        const unsigned q = qbuf[i], fg = gt[i] > 128 ? 1u : 0u;
        const unsigned y = (unsigned)i / W, x = (unsigned)i - y * W;
        const int kk = (y > cy ? 2 : 0) | (x > cx ? 1 : 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned m = k == kk ? 1u : 0u;
            acc[4 * k + 0] += m * q, acc[4 * k + 1] += m * q * q, acc[4 * k + 2] += m * fg, acc[4 * k + 3] += m * fg * q;
        }
    }
    const u64 a = block_sum(acc);
    if (threadIdx.x < ES_NQUAD) qslab[(b * gridDim.x + blockIdx.x) * ES_NQUAD + threadIdx.x] = a;
}

// ---- exact Euclidean distance transform -----------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), B, 2): lane = column, coalesced along x; blockIdx.z = 0 the down scan (du, the low half of dudd[y][x]), 1 the up scan
// (dd, the high half).  The scans only read gt, ES_COL_BATCH rows at a time, so that the loads of a batch are in flight together; the chain
// through `last` is register arithmetic.
__global__ __launch_bounds__(ES_COL_THREADS) void st_edt_col_kernel(const unsigned char* __restrict__ gt, int H, int W, long long hwp,
                                                                    unsigned short* __restrict__ dudd) {
    const int x = blockIdx.x * ES_COL_THREADS + threadIdx.x;
    if (x >= W) return;
    const long long b = blockIdx.y;
    const int up = blockIdx.z;
    gt += b * ((long long)H * W) + x;
    dudd += 2 * (b * hwp + x) + up;
    int last = -1;  // rows since the start of the scan, -1: no foreground yet
    for (int s0 = 0; s0 < H; s0 += ES_COL_BATCH) {
        unsigned char g[ES_COL_BATCH];
#pragma unroll
        for (int u = 0; u < ES_COL_BATCH; ++u) {
            const int s = s0 + u < H ? s0 + u : H - 1;  // (past the end: the last row again, not used)
            g[u] = gt[(long long)(up ? H - 1 - s : s) * W];
        }
#pragma unroll
        for (int u = 0; u < ES_COL_BATCH; ++u) {
            const int s = s0 + u;
            if (s < H) {
                if (g[u] > 128) last = s;
                dudd[2 * ((long long)(up ? H - 1 - s : s) * W)] = (unsigned short)(last < 0 ? ES_NONE16 : (unsigned)(s - last));
            }
        }
    }
}

// the better of a column's two candidates for row y, as a key; ES_FAR when the column has no foreground
__device__ __forceinline__ u64 column_key(unsigned v, int y, int x, int W) {
    const unsigned du = v & 0xffffu, dd = v >> 16;
    const u64 ku = du == ES_NONE16 ? ES_FAR : (u64)(du * du) << 32 | (unsigned)((y - (int)du) * W + x);
    const u64 kd = dd == ES_NONE16 ? ES_FAR : (u64)(dd * dd) << 32 | (unsigned)((y + (int)dd) * W + x);
    return ku < kd ? ku : kd;
}

// grid (H, B).  STAGED (W <= ES_ROW_LDS): dynamic LDS of W keys; wider rows: no LDS, the pairs come from global memory
template <bool STAGED>
__global__ __launch_bounds__(EV_THREADS) void st_edt_row_kernel(const unsigned* __restrict__ dudd, const u64* __restrict__ info, int H, int W,
                                                                long long hwp, u64* __restrict__ keys) {
    extern __shared__ u64 s_key[];
    const int y = blockIdx.x;
    const long long b = blockIdx.y;
    keys += b * ((long long)H * W) + (long long)y * W;
    if (info[b * ES_INFO] == 0) {  // (workgroup-uniform)
        for (int x = threadIdx.x; x < W; x += EV_THREADS) keys[x] = ES_NOKEY;
        return;
    }
    const unsigned* row = dudd + b * hwp + (long long)y * W;
    if (STAGED) {
        for (int x = threadIdx.x; x < W; x += EV_THREADS) s_key[x] = column_key(row[x], y, x, W);
        __syncthreads();
    }
    for (int x = threadIdx.x; x < W; x += EV_THREADS) {
        u64 best = STAGED ? s_key[x] : column_key(row[x], y, x, W);
        const int rmax = x > W - 1 - x ? x : W - 1 - x;
        // four offsets at a time: eight independent reads (a column outside the row: the clamped index, the result discarded), then the
        // minima.  The stop is tested once per group: an offset past the stopping point has d2 >= dx^2 > best d2 and cannot win.
        for (int r = 1; r <= rmax; r += ES_ROW_GROUP) {
            if ((u64)((unsigned)r * (unsigned)r) > (best >> 32)) break;  // r <= 32766
            u64 k[2 * ES_ROW_GROUP];
#pragma unroll
            for (int u = 0; u < ES_ROW_GROUP; ++u) {
                const int rr = r + u, xl = x - rr, xr = x + rr;
                const int il = xl < 0 ? 0 : xl, ir = xr >= W ? W - 1 : xr;
                const u64 add = (u64)((unsigned)rr * (unsigned)rr) << 32;
                const u64 kl = (STAGED ? s_key[il] : column_key(row[il], y, il, W)) + add;
                const u64 kr = (STAGED ? s_key[ir] : column_key(row[ir], y, ir, W)) + add;
                k[2 * u] = xl < 0 ? ES_NOKEY : kl, k[2 * u + 1] = xr >= W ? ES_NOKEY : kr;
            }
#pragma unroll
            for (int u = 0; u < 2 * ES_ROW_GROUP; ++u) best = k[u] < best ? k[u] : best;
        }
        keys[x] = best;  // n_fg > 0: some column has foreground, and the search reaches it before dx^2 passes ES_FAR's d2
    }
}

// ---- weighted F: the weighting pass ----------------------------------------------------------------------------------------------------------
// grid (ceil(W / 32), ceil(H / 8), B); slab = (sum_fg Ew, sum_bg Ew) of the tile
__global__ __launch_bounds__(EV_THREADS) void st_weight_kernel(const unsigned char* __restrict__ qbuf, const unsigned char* __restrict__ gt,
                                                               const u64* __restrict__ keys, const u64* __restrict__ info, int H, int W,
                                                               long long hwp, double* __restrict__ wslab) {
    __shared__ double s_et[ES_TH + 2 * ES_AP][ES_TW + 2 * ES_AP];
    const long long b = blockIdx.z;
    const long long hw = (long long)H * W;
    double* slab = wslab + ((b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    if (info[b * ES_INFO] == 0) {  // no foreground: no keys to gather through; wf = 0 by definition
        if (threadIdx.x < 2) slab[threadIdx.x] = 0.0;
        return;
    }
    qbuf += b * hwp, gt += b * hw, keys += b * hw;
    const int x0 = blockIdx.x * ES_TW, y0 = blockIdx.y * ES_TH;
    constexpr int AW = ES_TW + 2 * ES_AP, AH = ES_TH + 2 * ES_AP;
    for (int k = threadIdx.x; k < AW * AH; k += EV_THREADS) {
        const int ly = k / AW, lx = k - ly * AW;
        const int yy = y0 + ly - ES_AP, xx = x0 + lx - ES_AP;
        double et = 0.0;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const unsigned idx = (unsigned)keys[(long long)yy * W + xx];  // < H * W: the row pass wrote a real key
            et = (double)(255u - qbuf[idx]) / 255.0;
        }
        s_et[ly][lx] = et;
    }
    __syncthreads();
    const int lx = threadIdx.x & (ES_TW - 1), ly = threadIdx.x / ES_TW;
    const int x = x0 + lx, y = y0 + ly;
    double v[2] = {0.0, 0.0};
    if (x < W && y < H) {
        const long long i = (long long)y * W + x;
        if (gt[i] > 128) {
            const double e = s_et[ly + ES_AP][lx + ES_AP];
            double ea = 0.0;  // (a tap outside the image adds K * 0.0 = +0.0 to a non-negative sum: bitwise the same as skipping it)
#pragma unroll
            for (int a = 0; a < 7; ++a) {
#pragma unroll
                for (int c = 0; c < 7; ++c) ea += ES_K[7 * a + c] * s_et[ly + a][lx + c];
            }
            v[0] = ea < e ? ea : e;
        } else {
            const double e = (double)qbuf[i] / 255.0;
            const double d2 = (double)(unsigned)(keys[i] >> 32);
            v[1] = e * (2.0 - exp(ES_WF_C * __dsqrt_rn(d2)));
        }
    }
    block_reduce_store<2>(v, slab);
}

// ---- values ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double st_e_term(double p, double g, double mp, double mg) {
    const double ap = p - mp, ag = g - mg;
    const double phi = ((2.0 * ap) * ag) / (ap * ap + ag * ag);
    return ((phi + 1.0) * (phi + 1.0)) / 4.0;
}

__device__ __forceinline__ double st_object(u64 N, u64 a, u64 a2) {
    const double dn = (double)N;
    const double xb = (double)a / (255.0 * dn), m2 = (double)a2 / (65025.0 * dn);
    double d = m2 - xb * xb;
    if (d < 0.0) d = 0.0;
    const double var = N == 1 ? 0.0 : (d * dn) / (double)(N - 1);
    return (2.0 * xb) / ((xb * xb + 1.0) + __dsqrt_rn(var));
}

__device__ __forceinline__ double st_block(u64 N, u64 a, u64 a2, u64 b, u64 c) {
    const double dn = (double)N;
    const double xb = (double)a / (255.0 * dn), yb = (double)b / dn;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    if (N > 1) {
        const double dm = (double)(N - 1);
        sxx = ((double)a2 / 65025.0 - (xb * xb) * dn) / dm;
        syy = ((double)b - (yb * yb) * dn) / dm;
        sxy = ((double)c / 255.0 - (xb * yb) * dn) / dm;
    }
    const double A = ((4.0 * xb) * yb) * sxy, Bq = (xb * xb + yb * yb) * (sxx + syy);
    if (A != 0.0 && Bq != 0.0) return A / Bq;
    return A == 0.0 && Bq == 0.0 ? 1.0 : 0.0;
}

// one workgroup per image
__global__ __launch_bounds__(EV_THREADS) void st_finalise_kernel(const u64* __restrict__ hist, const u64* __restrict__ info,
                                                                 const u64* __restrict__ qslab, int nblk, const double* __restrict__ wslab,
                                                                 int ntile, int H, int W, double* __restrict__ out,
                                                                 u64* __restrict__ counts_out) {
    __shared__ u64 s_bg[ES_BINS], s_fg[ES_BINS], s_quad[ES_NQUAD], s_qpart[EV_THREADS / ES_NQUAD][ES_NQUAD];
    __shared__ double s_e[ES_BINS], s_w[EV_THREADS][2];
    const long long b = blockIdx.x;
    const int t = threadIdx.x;
    s_bg[t] = hist[b * 2 * ES_BINS + t];
    s_fg[t] = hist[b * 2 * ES_BINS + ES_BINS + t];
    {  // the quadrant slabs: thread (g, k) adds value k of slabs g, g + 16, ... (integers: any order)
        const int k = t % ES_NQUAD, grp = t / ES_NQUAD;
        u64 a = 0;
#pragma unroll 4
        for (int j = grp; j < nblk; j += EV_THREADS / ES_NQUAD) a += qslab[(b * nblk + j) * ES_NQUAD + k];
        s_qpart[grp][k] = a;
    }
    {  // the tile sums: thread t adds tiles t, t + 256, ... in that order (loads batched 8 deep, the additions in order), thread 0 then adds
       // the 256 partial sums in index order
        const double2* tiles = reinterpret_cast<const double2*>(wslab) + b * ntile;
        double f = 0.0, g = 0.0;
        int j = t;
        for (; j + 7 * EV_THREADS < ntile; j += 8 * EV_THREADS) {
            double2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = tiles[j + u * EV_THREADS];
#pragma unroll
            for (int u = 0; u < 8; ++u) f += v[u].x, g += v[u].y;
        }
        for (; j < ntile; j += EV_THREADS) f += tiles[j].x, g += tiles[j].y;
        s_w[t][0] = f, s_w[t][1] = g;
    }
    __syncthreads();
    if (t < ES_NQUAD) {
        u64 a = 0;
        for (int g = 0; g < EV_THREADS / ES_NQUAD; ++g) a += s_qpart[g][t];
        s_quad[t] = a;
    }
    const u64 n = (u64)H * (u64)W, n_fg = info[b * ES_INFO];
    const double dn = (double)n, dm1 = (double)(n > 1 ? n - 1 : 1ull);
    {  // threshold t: positive where q >= t
        u64 tp = 0, bp = 0;
        for (int k = t; k < ES_BINS; ++k) tp += s_fg[k], bp += s_bg[k];
        const u64 p = tp + bp, fp = bp, fn = n_fg - tp, tn = n - n_fg - bp;
        double e;
        if (n_fg == 0) e = (double)(n - p) / dm1;
        else if (n_fg == n) e = (double)p / dm1;
        else {
            const double mp = (double)p / dn, mg = (double)n_fg / dn;
            double s = (double)tp * st_e_term(1.0, 1.0, mp, mg);
            s += (double)fp * st_e_term(1.0, 0.0, mp, mg);
            s += (double)fn * st_e_term(0.0, 1.0, mp, mg);
            s += (double)tn * st_e_term(0.0, 0.0, mp, mg);
            e = s / dm1;
        }
        s_e[t] = e;
    }
    __syncthreads();
    const u64 cx = info[b * ES_INFO + 3], cy = info[b * ES_INFO + 4];
    const u64 qn[4] = {(cy + 1) * (cx + 1), (cy + 1) * ((u64)W - cx - 1), ((u64)H - cy - 1) * (cx + 1), ((u64)H - cy - 1) * ((u64)W - cx - 1)};
    if (counts_out) {
        u64* c = counts_out + b * ES_COUNTS;
        if (t < ES_HEAD) c[t] = info[b * ES_INFO + t];
        if (t < 4) {
            c[ES_HEAD + 5 * t] = qn[t];
            for (int k = 0; k < 4; ++k) c[ES_HEAD + 5 * t + 1 + k] = s_quad[4 * t + k];
        }
        c[ES_HEAD + 20 + t] = s_bg[t];
        c[ES_HEAD + 20 + ES_BINS + t] = s_fg[t];
    }
    if (t != 0) return;
    double* o = out + b * ES_OUT;
    const double nan = __builtin_nan("");
    o[0] = dn, o[1] = (double)n_fg, o[13] = (double)cx, o[14] = (double)cy;
    // E-measure
    u64 sum_q = 0, a_fg = 0, a2_fg = 0, a_bg = 0, a2_bg = 0;
    double best = s_e[0], sum = s_e[0];
    for (int k = 0; k < ES_BINS; ++k) {
        const u64 v = (u64)k, w = 255ull - v;
        sum_q += v * (s_bg[k] + s_fg[k]);
        a_fg += v * s_fg[k], a2_fg += v * v * s_fg[k];
        a_bg += w * s_bg[k], a2_bg += w * w * s_bg[k];
        if (k > 0) {
            sum += s_e[k];
            if (s_e[k] > best) best = s_e[k];
        }
    }
    const u64 cap = 255ull * n, twice = 2ull * sum_q;
    const u64 t_a = ((twice < cap ? twice : cap) + n - 1) / n;
    o[5] = best, o[6] = sum / 256.0, o[7] = s_e[t_a];
    // S-measure
    if (n_fg == 0) {
        o[2] = 1.0 - (double)sum_q / (255.0 * dn), o[3] = nan, o[4] = nan;
    } else if (n_fg == n) {
        o[2] = (double)sum_q / (255.0 * dn), o[3] = nan, o[4] = nan;
    } else {
        const double u = (double)n_fg / dn;
        const double so = u * st_object(n_fg, a_fg, a2_fg) + (1.0 - u) * st_object(n - n_fg, a_bg, a2_bg);
        double sr = 0.0;
        for (int k = 0; k < 4; ++k)
            if (qn[k] != 0) sr += ((double)qn[k] / dn) * st_block(qn[k], s_quad[4 * k], s_quad[4 * k + 1], s_quad[4 * k + 2], s_quad[4 * k + 3]);
        const double s = 0.5 * so + 0.5 * sr;
        o[2] = s < 0.0 ? 0.0 : s, o[3] = so, o[4] = sr;
    }
    // weighted F
    double s_fgw = 0.0, s_bgw = 0.0;
    for (int k = 0; k < EV_THREADS; ++k) s_fgw += s_w[k][0], s_bgw += s_w[k][1];
    double wf = 0.0, prec = 0.0, rec = 0.0;
    if (n_fg != 0) {
        const double tpw = (double)n_fg - s_fgw, den = tpw + s_bgw;
        rec = 1.0 - s_fgw / (double)n_fg;
        prec = den == 0.0 ? 0.0 : tpw / den;
        wf = rec + prec == 0.0 ? 0.0 : ((2.0 * rec) * prec) / (rec + prec);
    }
    o[8] = wf, o[9] = prec, o[10] = rec, o[11] = s_fgw, o[12] = s_bgw;
}

}  // namespace

extern "C" {

long long gp_eval_structure_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return struct_ws(B, H, W).total;
}

gp_status gp_eval_structure(const void* pred, int pred_is_u8, const unsigned char* gt, int B, int H, int W, double* out,
                            unsigned long long* counts_out, unsigned long long* edt_out, void* workspace, long long workspace_bytes, void* stream) {
    if (!pred || !gt || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W) || H > 32767 || W > 32767) return GP_ERR_INVALID;
    if (!eval_pred_ok(pred, pred_is_u8) || !eval_aligned8(workspace, out, counts_out, edt_out)) return GP_ERR_INVALID;
    const StructWs w = struct_ws(B, H, W);
    if (workspace_bytes < w.total) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W;
    char* base = (char*)workspace;
    char* cslab = base + w.cslab;
    u64* hist = (u64*)(base + w.hist);
    u64* info = (u64*)(base + w.info);
    u64* qslab = (u64*)(base + w.qslab);
    double* wslab = (double*)(base + w.wslab);
    unsigned* dudd = (unsigned*)(base + w.dudd);
    u64* keys = edt_out ? edt_out : (u64*)(base + w.keys);
    unsigned char* qbuf = (unsigned char*)(base + w.qbuf);
    const auto count = pred_is_u8 ? st_count_kernel<true> : st_count_kernel<false>;
    hipLaunchKernelGGL(count, dim3(w.nblk, B), dim3(EV_THREADS), 0, s, pred, gt, (unsigned)W, hw, w.hwp, cslab, qbuf);
    hipLaunchKernelGGL(st_centroid_kernel, dim3(B), dim3(EV_FIN_THREADS), 0, s, (const char*)cslab, w.nblk, hist, info);
    hipLaunchKernelGGL(st_quad_kernel, dim3(w.nblk, B), dim3(EV_THREADS), 0, s, (const unsigned char*)qbuf, gt, (const u64*)info, (unsigned)W, hw, w.hwp,
                       qslab);
    hipLaunchKernelGGL(st_edt_col_kernel, dim3((W + ES_COL_THREADS - 1) / ES_COL_THREADS, B, 2), dim3(ES_COL_THREADS), 0, s, gt, H, W, w.hwp,
                       (unsigned short*)dudd);
    if (W <= ES_ROW_LDS)
        hipLaunchKernelGGL(st_edt_row_kernel<true>, dim3(H, B), dim3(EV_THREADS), (size_t)W * 8, s, (const unsigned*)dudd, (const u64*)info, H, W, w.hwp, keys);
    else
        hipLaunchKernelGGL(st_edt_row_kernel<false>, dim3(H, B), dim3(EV_THREADS), 0, s, (const unsigned*)dudd, (const u64*)info, H, W, w.hwp, keys);
    hipLaunchKernelGGL(st_weight_kernel, dim3(w.tx, w.ty, B), dim3(EV_THREADS), 0, s, (const unsigned char*)qbuf, gt, (const u64*)keys,
                       (const u64*)info, H, W, w.hwp, wslab);
    hipLaunchKernelGGL(st_finalise_kernel, dim3(B), dim3(EV_THREADS), 0, s, (const u64*)hist, (const u64*)info, (const u64*)qslab, w.nblk,
                       (const double*)wslab, w.tx * w.ty, H, W, out, counts_out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
