// Trimap and boundary bands on the device (gp_mask_band): which pixels of an 8-bit map lie within `reach` of A = {a > lo} and within `reach` of
// Bc = {a < hi}, exactly, for the squared Euclidean and the Chebyshev metric.  The definitions are stated once in include/genpercept_hip.h;
// eval_metrics.mask_band restates them on the host.
//   columns  one lane per column, one workgroup per 64 columns x one segment of rows.  A down scan and an up scan, each started `rv` rows
//            (the vertical reach) outside the segment, count the rows since the last pixel of A and of Bc, capped at rv + 1.  The down scan
//            leaves its two counts in the pixel's scratch word; the up scan of the same lane reads them back, takes the minima (and, with
//            border = 1, the distance to the image's top and bottom edge for Bc) and replaces each vertical distance d by the HORIZONTAL reach
//            it leaves: the largest |dx| with d^2 + dx^2 <= reach (metric 0) or reach itself (metric 1), from a table of rv + 2 entries built
//            in LDS by an integer square root; stored + 1, 0 = the column is out of reach.  Bit 15 of the low half says that the pixel is in A.
//   rows     one workgroup per row x 1024 columns.  The words of the tile and an apron of the horizontal reach on either side are staged in
//            LDS (columns outside the image: out of reach for A; for Bc in reach everywhere with border = 1, out of reach with border = 0);
//            a ballot per 64 staged words notes whether any of them is within reach of A, of Bc, at all.  Pixel x looks outwards, four offsets
//            at a time, until both sets are found, |dx| passes the horizontal reach, or its window's notes say the missing set is nowhere.  An apron above
//            MB_APRON columns is not staged: the same search reads the words from global memory.  No barrier inside the search.
// Two launches for every B, stream-ordered, integers only, no atomics, nothing read back.  Every workgroup count and every pixel -> thread
// assignment depends on H, W and reach alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"

namespace {

constexpr int MB_COL_THREADS = 64;
constexpr int MB_COL_BATCH = 32;          // rows of a column scan whose loads are in flight together
constexpr int MB_SEG = 32;                // rows of a column segment: the multiple of this that is at least the vertical reach (a scan is a
                                          // chain of load batches, so short segments and many workgroups finish sooner than long ones)
constexpr int MB_MAX_RV = 4096;           // the largest vertical / horizontal reach (reach <= 4096 or reach <= 4096^2)
constexpr int MB_TILE = 1024;             // columns of a row workgroup
constexpr int MB_APRON = 1024;            // the widest apron that is staged in LDS (about 12 KiB with the tile)
constexpr int MB_ROW_GROUP = 4;           // offsets of the row search examined together
constexpr unsigned MB_IN_A = 0x8000u;     // bit 15 of the low half: the pixel itself is in A

// floor(sqrt(v)), v < 2^26, in integers
__host__ __device__ inline int mb_isqrt(unsigned v) {
    unsigned r = 0;
    for (unsigned bit = 1u << 12; bit != 0; bit >>= 1) {
        const unsigned t = r | bit;
        if (t * t <= v) r = t;
    }
    return (int)r;
}

inline int mb_vertical_reach(int metric, int reach) { return metric ? reach : mb_isqrt((unsigned)reach); }
inline int mb_segment(int rv) { return rv <= MB_SEG ? MB_SEG : (rv + MB_SEG - 1) / MB_SEG * MB_SEG; }

// grid (ceil(W / 64) * ceil(H / seg), B): blockIdx.x = segment * column blocks + column block.
template <bool U8>
__global__ __launch_bounds__(MB_COL_THREADS) void mb_col_kernel(const void* __restrict__ a_v, int H, int W, long long hwp, int lo, int hi,
                                                                int metric, int reach, int rv, int seg, int border, int ncb, unsigned* ws) {
    __shared__ short s_tab[MB_MAX_RV + 2];  // vertical distance d -> the horizontal reach it leaves, -1: none (d = rv + 1 always)
    for (int d = threadIdx.x; d <= rv + 1; d += MB_COL_THREADS) {
        int h = -1;
        if (d <= rv) h = metric ? reach : mb_isqrt((unsigned)reach - (unsigned)d * (unsigned)d);
        s_tab[d] = (short)h;
    }
    __syncthreads();
    const int cb = blockIdx.x % ncb, sg = blockIdx.x / ncb;
    const int x = cb * MB_COL_THREADS + threadIdx.x;
    if (x >= W) return;
    const long long b = blockIdx.y;
    const Pred8<U8> a(a_v, b * ((long long)H * W) + x);  // this lane's column
    ws += b * hwp + x;
    const int cap = rv + 1;
    const int y0 = sg * seg, y1 = y0 + seg < H ? y0 + seg : H;  // (seg <= 4096: no overflow)
    {  // down: rows ys .. y1 - 1, stored from y0 on
        const int ys = y0 - rv > 0 ? y0 - rv : 0;
        int dA = cap, dB = cap;
        for (int s0 = ys; s0 < y1; s0 += MB_COL_BATCH) {
            int v[MB_COL_BATCH];
#pragma unroll
            for (int u = 0; u < MB_COL_BATCH; ++u) {
                const int y = s0 + u < y1 ? s0 + u : y1 - 1;  // (past the end: the last row again, not used)
                v[u] = (int)a[(long long)y * W];
            }
#pragma unroll
            for (int u = 0; u < MB_COL_BATCH; ++u) {
                const int y = s0 + u;
                if (y < y1) {
                    dA = v[u] > lo ? 0 : (dA < cap ? dA + 1 : cap);
                    dB = v[u] < hi ? 0 : (dB < cap ? dB + 1 : cap);
                    if (y >= y0) ws[(long long)y * W] = (unsigned)dA | (unsigned)dB << 16;
                }
            }
        }
    }
    {  // up: rows ye - 1 .. y0, finished from y1 - 1 on (this lane's own words of the down scan come back)
        const int ye = (long long)y1 + rv < H ? y1 + rv : H;
        int dA = cap, dB = cap;
        for (int s0 = ye - 1; s0 >= y0; s0 -= MB_COL_BATCH) {
            int v[MB_COL_BATCH];
            unsigned w[MB_COL_BATCH];
#pragma unroll
            for (int u = 0; u < MB_COL_BATCH; ++u) {
                const int y = s0 - u > y0 ? s0 - u : y0;
                v[u] = (int)a[(long long)y * W];
                w[u] = y < y1 ? ws[(long long)y * W] : 0u;
            }
#pragma unroll
            for (int u = 0; u < MB_COL_BATCH; ++u) {
                const int y = s0 - u;
                if (y >= y0) {
                    const bool inA = v[u] > lo;
                    dA = inA ? 0 : (dA < cap ? dA + 1 : cap);
                    dB = v[u] < hi ? 0 : (dB < cap ? dB + 1 : cap);
                    if (y < y1) {
                        int fA = (int)(w[u] & 0xffffu), fB = (int)(w[u] >> 16);
                        fA = dA < fA ? dA : fA, fB = dB < fB ? dB : fB;
                        if (border) {
                            const int e = y + 1 < H - y ? y + 1 : H - y;
                            fB = e < fB ? e : fB;
                        }
                        const unsigned hA = (unsigned)(s_tab[fA] + 1), hB = (unsigned)(s_tab[fB] + 1);
                        ws[(long long)y * W] = hA | (inA ? MB_IN_A : 0u) | hB << 16;
                    }
                }
            }
        }
    }
}

struct MbOut {
    unsigned char *band, *fg, *bg, *inner, *trimap;
};

// grid (H * ceil(W / 1024), B): blockIdx.x = row * tiles + tile.  STAGED: dynamic LDS of mb_row_lds(rh) bytes.  rh: the horizontal reach, at most W.  edge: the word of a
// column outside the image.
template <bool STAGED>
__global__ __launch_bounds__(EV_THREADS) void mb_row_kernel(const unsigned* __restrict__ ws, int H, int W, long long hwp, int rh, unsigned edge,
                                                            int ntx, MbOut out) {
    extern __shared__ unsigned s_w[];
    const int y = blockIdx.x / ntx, x0 = (blockIdx.x % ntx) * MB_TILE;
    const long long b = blockIdx.y;
    const unsigned* row = ws + b * hwp + (long long)y * W;
    const int x1 = x0 + MB_TILE < W ? x0 + MB_TILE : W;
    unsigned* s_any = s_w + MB_TILE + 2 * rh;  // per 64 staged words: bit 0 some column is within reach of A at all, bit 1 of Bc
    if (STAGED) {
        const int n = x1 - x0 + 2 * rh;
        for (int k0 = 0; k0 < n; k0 += EV_THREADS) {  // (workgroup-uniform bounds: the ballots see whole waves)
            const int k = k0 + threadIdx.x, xx = x0 - rh + k;
            unsigned w = 0;
            if (k < n) {
                w = xx >= 0 && xx < W ? row[xx] : edge;
                s_w[k] = w;
            }
            const bool anyA = __builtin_amdgcn_ballot_w64((w & 0x7fffu) != 0) != 0, anyB = __builtin_amdgcn_ballot_w64((w >> 16) != 0) != 0;
            if ((threadIdx.x & 63) == 0) s_any[k >> 6] = (anyA ? 1u : 0u) | (anyB ? 2u : 0u);
        }
        __syncthreads();
    }
    const long long o = b * ((long long)H * W) + (long long)y * W;
    for (int x = x0 + threadIdx.x; x < x1; x += EV_THREADS) {
        const int c = x - x0 + rh;  // this pixel in s_w
        const unsigned w0 = STAGED ? s_w[c] : row[x];
        const bool inA = (w0 & MB_IN_A) != 0;
        bool hitA = (w0 & 0x7fffu) != 0, hitB = (w0 >> 16) != 0;
        unsigned can = 3u;  // which of the two sets has a column within reach anywhere in this pixel's window: the other one needs no search
        if (STAGED) {
            can = 0u;
            for (int j = (c - rh) >> 6; j <= (c + rh) >> 6; ++j) can |= s_any[j];
        }
        // four offsets at a time: eight independent reads, then the tests.  Column x + dx is within reach of the pixel when the horizontal
        // reach it stores (+ 1) exceeds |dx|; an offset past rh fails every test, so the stop is tested once per group.
        for (int r = 1; r <= rh && ((!hitA && (can & 1u)) || (!hitB && (can & 2u))); r += MB_ROW_GROUP) {
            unsigned wl[MB_ROW_GROUP], wr[MB_ROW_GROUP];
#pragma unroll
            for (int u = 0; u < MB_ROW_GROUP; ++u) {
                const int d = r + u <= rh ? r + u : rh;  // (past rh: rh again)
                if (STAGED) {
                    wl[u] = s_w[c - d], wr[u] = s_w[c + d];
                } else {
                    const int xl = x - d, xr = x + d;
                    const unsigned vl = row[xl < 0 ? 0 : xl], vr = row[xr >= W ? W - 1 : xr];
                    wl[u] = xl < 0 ? edge : vl, wr[u] = xr >= W ? edge : vr;
                }
            }
#pragma unroll
            for (int u = 0; u < MB_ROW_GROUP; ++u) {
                const unsigned d = (unsigned)(r + u <= rh ? r + u : rh);
                hitA = hitA || (wl[u] & 0x7fffu) > d || (wr[u] & 0x7fffu) > d;
                hitB = hitB || (wl[u] >> 16) > d || (wr[u] >> 16) > d;
            }
        }
        // (every pixel is in A or in Bc, so at least one of the two is found at dx = 0)
        const bool band = hitA && hitB;
        if (out.band) out.band[o + x] = band ? 255 : 0;
        if (out.fg) out.fg[o + x] = hitB ? 0 : 255;
        if (out.bg) out.bg[o + x] = hitA ? 0 : 255;
        if (out.inner) out.inner[o + x] = inA && hitB ? 255 : 0;
        if (out.trimap) out.trimap[o + x] = band ? 128 : (hitA ? 255 : 0);
    }
}

// the staged words of a tile with its aprons, then one summary word per 64 of them (the last wave of the staging loop may write past the row's end)
inline size_t mb_row_lds(int rh) { return (size_t)(MB_TILE + 2 * rh + (MB_TILE + 2 * rh) / 64 + 5) * 4; }
inline long long mb_hwp(int H, int W) { return ((long long)H * W + 1) / 2 * 2; }

}  // namespace

extern "C" {

long long gp_mask_band_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return (long long)B * mb_hwp(H, W) * 4;
}

gp_status gp_mask_band(const void* a, int a_is_u8, int B, int H, int W, int lo, int hi, int metric, int reach, int border,
                       unsigned char* band_out, unsigned char* fg_out, unsigned char* bg_out, unsigned char* inner_out, unsigned char* trimap_out,
                       void* workspace, long long workspace_bytes, void* stream) {
    if (!a || !workspace || !(band_out || fg_out || bg_out || inner_out || trimap_out)) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W)) return GP_ERR_INVALID;
    if (metric < 0 || metric > 1 || border < 0 || border > 1) return GP_ERR_INVALID;
    if (lo < -1 || hi > 256 || lo >= hi) return GP_ERR_INVALID;
    if (reach < 0 || reach > (metric ? MB_MAX_RV : MB_MAX_RV * MB_MAX_RV)) return GP_ERR_INVALID;
    if (!eval_pred_ok(a, a_is_u8) || !eval_aligned8(workspace)) return GP_ERR_INVALID;
    const long long hwp = mb_hwp(H, W);
    if (workspace_bytes < (long long)B * hwp * 4) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    unsigned* ws = (unsigned*)workspace;
    const int rv = mb_vertical_reach(metric, reach);  // the horizontal reach of a column at vertical distance 0 is the same number
    const int seg = mb_segment(rv);
    const int ncb = (W + MB_COL_THREADS - 1) / MB_COL_THREADS, nseg = (H + seg - 1) / seg;  // ncb * nseg <= H * W / 64 + H + W
    const dim3 cgrid((unsigned)ncb * (unsigned)nseg, B);
    const auto col = a_is_u8 ? mb_col_kernel<true> : mb_col_kernel<false>;
    hipLaunchKernelGGL(col, cgrid, dim3(MB_COL_THREADS), 0, s, a, H, W, hwp, lo, hi, metric, reach, rv, seg, border, ncb, ws);
    // a column outside the image: never A; with border = 1 all of it is Bc (vertical distance 0), with border = 0 nothing is there.  No pixel
    // is more than W columns away from the outside, so a horizontal reach above W searches nothing new.
    const int rh = rv < W ? rv : W;
    const unsigned edge = border ? (unsigned)(rv + 1) << 16 : 0u;
    const MbOut out = {band_out, fg_out, bg_out, inner_out, trimap_out};
    const int ntx = (W + MB_TILE - 1) / MB_TILE;
    const dim3 rgrid((unsigned)H * (unsigned)ntx, B);
    if (rh <= MB_APRON)
        hipLaunchKernelGGL(mb_row_kernel<true>, rgrid, dim3(EV_THREADS), mb_row_lds(rh), s, (const unsigned*)ws, H, W, hwp, rh, edge, ntx, out);
    else
        hipLaunchKernelGGL(mb_row_kernel<false>, rgrid, dim3(EV_THREADS), 0, s, (const unsigned*)ws, H, W, hwp, rh, edge, ntx, out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
