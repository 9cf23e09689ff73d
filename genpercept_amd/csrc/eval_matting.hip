// Matting gradient and connectivity errors on the device (gp_eval_matting): Grad and Conn (Rhemann et al. 2009) of an 8-bit prediction q against an
// 8-bit alpha g, per image.  The definitions are stated once in include/genpercept_hip.h; eval_metrics.conn_levels / conn_error /
// grad_error_map / grad_error restate them on the host.
//   prep      one pass like eval.hip's count pass: q (quantised here and kept as bytes), m = min(q, g), level[i] = 10, parent[i] = the start of
//             i's run of I_10 inside its wave's 64 pixels (i itself elsewhere), the minima and maxima of q and g, one slab per workgroup; a
//             one-workgroup-per-image kernel folds the slabs.
//   labelling ONE union-find over the row-major pixel indices, grown from k = 10 down to 1 (the superlevel sets are nested): the root of a
//             tree is the smallest index of its component, a link always points to a smaller index.  Stage k, two launches:
//               union  one thread per pixel adds the edges to its right and lower neighbour whose smaller end lies in [T_k, T_{k+1}) -- the
//                      edges that are new at this stage -- by the lock-free find / atomicMin loop below (32-bit labels in global memory; no
//                      LDS-local phase: see DESIGN.md).  The same launch first settles stage k + 1: membership in Omega_{k+1} from the roots
//                      and the arg-max that the count pass of stage k + 1 left, level[i] = k where the pixel is outside, and size[i] = 0.
//               count  root = find(i) for every pixel of I_k, kept (a flatten: parent[i] = root) and counted by integer atomicAdds on
//                      size[root], one per wave and root and, for each wave's first root, one per workgroup; every add offers (count so far << 32 | ~root), the workgroup's maximum goes into
//                      the image's word by one 64-bit atomicMax.  The maximum over all offers is (size of the largest component, ~ its smallest root): the tie rule.
//             Integer min, add and max do not depend on their order: roots, sizes and arg-max are the same bits for every schedule.
//   conn      stage 1 settled, the level (optionally written out), the eleven level counts (ballot + population count), n and conn_num over the
//             region: per-workgroup integer sums, one 64-bit atomicAdd per value and workgroup.
//   grad      rows: one workgroup per 256 pixels of a row, both normalised maps staged in LDS with a 4-pixel apron (the clamp happens at the
//             staging, so a row of any width takes the same path), four 9-tap sums per pixel.  Columns: 32 x 8 tiles, the nine rows clamped,
//             amp, err, one float64 sum per tile in block_reduce_store's fixed order.
//   values    one workgroup per image adds the tile sums in a fixed order and writes out / counts_out.
// 26 launches for every B, stream-ordered, nothing read back.  Every workgroup count and every pixel -> thread assignment depends on H and W
// alone; the only global atomics are integer min, add and max.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/genpercept_hip.h"
#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MT_OUT = 4;                            // n, grad, conn, grad_sum
constexpr int MT_LEVELS = 10;
constexpr int MT_COUNTS = 2 + MT_LEVELS + 1;         // counts_out: n, conn_num, the counts of the levels 0..10
constexpr int MT_INFO = 32;                          // 64-bit words per image: best[k - 1] for k = 1..10, then ...
constexpr int MT_I_COUNTS = 10;                      // ... the 13 words of counts_out, then ...
constexpr int MT_I_RANGE = 24;                       // ... min q, max q, min g, max g
constexpr int MT_HALF = 4;                           // the filters' half size
constexpr int MT_TAPS = 2 * MT_HALF + 1;
constexpr int MT_TW = 32, MT_TH = 8;                 // the tile of the column pass
constexpr int MT_CNT_THREADS = 1024;                 // the count pass: 16 waves share one add per root
constexpr int MT_CNT_WAVES = MT_CNT_THREADS / 64;
const unsigned MT_T[MT_LEVELS + 1] = {26, 51, 77, 102, 128, 153, 179, 204, 230, 255, 256};  // T_1..T_10 = ceil(255 k / 10); 256: above every byte

// the Gaussian (sigma = 1.4) and its derivative, each divided by its L2 norm (the same literals as eval_metrics.GRAD_G, GRAD_D)
__constant__ double MT_G[MT_TAPS] = {0x1.5f2161173037cp-7, 0x1.05c2b72947cf6p-4, 0x1.d49edcea5016bp-3, 0x1.f7af85f5976d7p-2, 0x1.4506d2f73739dp-1,
                                     0x1.f7af85f5976d7p-2, 0x1.d49edcea5016bp-3, 0x1.05c2b72947cf6p-4, 0x1.5f2161173037cp-7};
__constant__ double MT_D[MT_TAPS] = {0x1.62b49a56df053p-5,  0x1.8ca37e89855ffp-3,  0x1.d9645351e6fcbp-2,  0x1.fcd0621654797p-2, 0x0.0p+0,
                                     -0x1.fcd0621654797p-2, -0x1.d9645351e6fcbp-2, -0x1.8ca37e89855ffp-3, -0x1.62b49a56df053p-5};

// the workspace of a batch: byte offsets of its parts (each a multiple of 8 and proportional to B)
struct MatWs {
    long long info, range, tslab, qbuf, mbuf, level, parent, size, root, rows, total, hwp;
    int nblk, tx, ty;
};

MatWs mat_ws(long long B, int H, int W) {
    MatWs w;
    const long long hw = (long long)H * W;
    w.hwp = (hw + 7) / 8 * 8;
    w.nblk = eval_blocks(hw);
    w.tx = (W + MT_TW - 1) / MT_TW, w.ty = (H + MT_TH - 1) / MT_TH;
    long long o = 0;
    w.rows = o, o += B * hw * 32;  // (first: as aligned as the workspace itself)
    w.info = o, o += B * MT_INFO * 8;
    w.range = o, o += B * w.nblk * 4 * 4;
    w.tslab = o, o += B * w.tx * w.ty * 8;
    w.qbuf = o, o += B * w.hwp;
    w.mbuf = o, o += B * w.hwp;
    w.level = o, o += B * w.hwp;
    w.parent = o, o += B * w.hwp * 4;
    w.size = o, o += B * w.hwp * 4;
    w.root = o, o += B * w.hwp * 4;
    w.total = o;
    return w;
}

// ---- prep ---------------------------------------------------------------------------------------------------------------------------------
// grid (eval_blocks(H * W), B)
template <bool U8>
__global__ __launch_bounds__(EV_THREADS) void mt_prep_kernel(const void* __restrict__ pred_v, const unsigned char* __restrict__ gt, unsigned W,
                                                             long long hw, long long hwp, unsigned char* __restrict__ qbuf, unsigned char* __restrict__ mbuf,
                                                             unsigned char* __restrict__ level, unsigned* __restrict__ parent,
                                                             unsigned* __restrict__ range, u64* __restrict__ info) {
    __shared__ unsigned s_r[EV_WAVES][4];
    const long long b = blockIdx.y;
    const Pred8<U8> pred(pred_v, b * hw);
    gt += b * hw, qbuf += b * hwp, mbuf += b * hwp, level += b * hwp, parent += b * hwp;
    if (blockIdx.x == 0 && threadIdx.x < MT_INFO) info[b * MT_INFO + threadIdx.x] = 0;
    unsigned r[4] = {255u, 0u, 255u, 0u};  // min q, max q, min g, max g
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    // (workgroup-uniform bounds: the ballot sees whole waves)
    for (long long i0 = (long long)blockIdx.x * EV_THREADS; i0 < hw; i0 += stride) {
        const long long i = i0 + threadIdx.x;
        const bool in = i < hw;
        unsigned m = 0;
        if (in) {
            const unsigned q = pred[i];
            const unsigned g = gt[i];
            m = q < g ? q : g;
            qbuf[i] = (unsigned char)q;
            mbuf[i] = (unsigned char)m;
            level[i] = (unsigned char)MT_LEVELS;
            r[0] = q < r[0] ? q : r[0], r[1] = q > r[1] ? q : r[1], r[2] = g < r[2] ? g : r[2], r[3] = g > r[3] ? g : r[3];
        }
        // parent[i] = the first pixel of the run of I_10 that holds i inside this wave's 64 consecutive pixels of one row (i itself outside
        // I_10): the horizontal edges of stage 10 inside a wave, linked without an atomic.  `joined`: linked to the pixel on its left.
        const unsigned left = __shfl_up(m, 1, 64);
        const bool joined = in && lane > 0 && m >= 255u && left >= 255u && (unsigned)i % W != 0u;
        const u64 starts = ~__builtin_amdgcn_ballot_w64(joined) & (~0ull >> (63 - lane));  // the lanes up to this one that begin a run: lane 0 is one
        const int first = 63 - __clzll((long long)starts);
        if (in) parent[i] = (unsigned)i - (unsigned)(lane - first);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o0 = __shfl_down(r[0], off, 64), o1 = __shfl_down(r[1], off, 64), o2 = __shfl_down(r[2], off, 64), o3 = __shfl_down(r[3], off, 64);
        r[0] = o0 < r[0] ? o0 : r[0], r[1] = o1 > r[1] ? o1 : r[1], r[2] = o2 < r[2] ? o2 : r[2], r[3] = o3 > r[3] ? o3 : r[3];
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_r[wave][k] = r[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const bool mx = threadIdx.x & 1;
        unsigned a = s_r[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EV_WAVES; ++w) {
            const unsigned o = s_r[w][threadIdx.x];
            a = mx ? (o > a ? o : a) : (o < a ? o : a);
        }
        range[(b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = a;
    }
}

// one workgroup of 64 threads per image: the slabs folded into info[MT_I_RANGE ..]
__global__ __launch_bounds__(64) void mt_range_kernel(const unsigned* __restrict__ range, int nblk, u64* __restrict__ info) {
    const long long b = blockIdx.x;
    unsigned r[4] = {255u, 0u, 255u, 0u};
    for (int j = threadIdx.x; j < nblk; j += 64) {
        const unsigned* s = range + (b * nblk + j) * 4;
        r[0] = s[0] < r[0] ? s[0] : r[0], r[1] = s[1] > r[1] ? s[1] : r[1], r[2] = s[2] < r[2] ? s[2] : r[2], r[3] = s[3] > r[3] ? s[3] : r[3];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o0 = __shfl_down(r[0], off, 64), o1 = __shfl_down(r[1], off, 64), o2 = __shfl_down(r[2], off, 64), o3 = __shfl_down(r[3], off, 64);
        r[0] = o0 < r[0] ? o0 : r[0], r[1] = o1 > r[1] ? o1 : r[1], r[2] = o2 < r[2] ? o2 : r[2], r[3] = o3 > r[3] ? o3 : r[3];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) info[b * MT_INFO + MT_I_RANGE + k] = r[k];
    }
}

// ---- labelling ------------------------------------------------------------------------------------------------------------------------------
// Invariant: parent[i] <= i, and only atomicMin and the flatten (which stores an ancestor) ever write it, so a chain of parents strictly
// decreases and ends at a root.  A load that returns an older value returns an older ancestor: still in the same component, still <= i.
__device__ __forceinline__ unsigned mt_find(const unsigned* parent, unsigned i) {
    unsigned p;
    while ((p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != i) i = p;
    return i;
}

// The standard lock-free union.  A turn either returns or goes on with a pair whose larger member is smaller than before (atomicMin returned
// b itself: linked, done; otherwise b already had a parent old < b, which now has to be joined with a): it never waits for another thread.
__device__ __forceinline__ void mt_unite(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = mt_find(parent, a), b = mt_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const unsigned t = a;
            a = b, b = t;
        }
        const unsigned old = atomicMin(parent + b, a);
        if (old == b) return;
        b = old;
    }
}

// membership in Omega_k from what the count pass of stage k left: the root of the pixel and the image's arg-max word (0: I_k is empty)
__device__ __forceinline__ bool mt_member(u64 best, unsigned m, unsigned t_k, unsigned root) {
    return best != 0 && m >= t_k && root == 0xffffffffu - (unsigned)best;
}

// grid (ceil(H * W / 256), B).  Edges of stage k: both ends >= t_lo = T_k, the smaller end < t_hi = T_{k+1} (256 for k = 10).  settle = k + 1
// (0 for k = 10): the stage whose membership is turned into levels first; its threshold is t_hi.
__global__ __launch_bounds__(EV_THREADS) void mt_union_kernel(const unsigned char* __restrict__ mbuf, unsigned* parent, unsigned* __restrict__ size,
                                                              const unsigned* __restrict__ root, unsigned char* __restrict__ level,
                                                              const u64* __restrict__ info, unsigned W, long long hw, long long hwp, unsigned t_lo,
                                                              unsigned t_hi, int settle) {
    const long long b = blockIdx.y;
    const long long il = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (il >= hw) return;
    const unsigned i = (unsigned)il;
    mbuf += b * hwp, parent += b * hwp, size += b * hwp, root += b * hwp, level += b * hwp;
    const unsigned m = mbuf[i];
    if (settle) {
        const u64 best = info[b * MT_INFO + settle - 1];
        if (!mt_member(best, m, t_hi, m >= t_hi ? root[i] : 0u)) level[i] = (unsigned char)(settle - 1);
    }
    size[i] = 0;
    if (m < t_lo) return;
    const unsigned x = i % W;
    if (x + 1 < W) {
        const unsigned o = mbuf[i + 1];
        if (o >= t_lo && (m < o ? m : o) < t_hi) mt_unite(parent, i, i + 1);
    }
    if ((long long)i + W < hw) {
        const unsigned o = mbuf[i + W];
        if (o >= t_lo && (m < o ? m : o) < t_hi) mt_unite(parent, i, i + W);
    }
}

// grid (ceil(H * W / 1024), B), after the union pass of stage k: no link changes here, find is exact
__global__ __launch_bounds__(MT_CNT_THREADS) void mt_count_kernel(const unsigned char* __restrict__ mbuf, unsigned* parent, unsigned* size,
                                                                  unsigned* __restrict__ root, u64* info, long long hw, long long hwp, unsigned t_k,
                                                                  int k) {
    __shared__ u64 s_key[MT_CNT_WAVES];
    __shared__ unsigned s_root[MT_CNT_WAVES], s_cnt[MT_CNT_WAVES];
    const long long b = blockIdx.y;
    const long long il = (long long)blockIdx.x * MT_CNT_THREADS + threadIdx.x;
    mbuf += b * hwp, parent += b * hwp, size += b * hwp, root += b * hwp;
    u64 key = 0;
    unsigned r = 0;
    bool open = il < hw && mbuf[il] >= t_k;  // this lane's pixel is in I_k and not counted yet
    if (open) {
        const unsigned i = (unsigned)il;
        r = mt_find(parent, i);
        if (r != i) parent[i] = r;
        root[i] = r;
    }
    // One atomicAdd per root and wave instead of one per pixel (the pixels of a large component would queue on one word): the first open
    // lane's root is taken, its lanes are counted by a ballot and closed.  The first such group of every wave goes through LDS, where the
    // first wave that holds a root adds for all the waves of the workgroup that hold it (large components span whole workgroups); the
    // other groups of a wave are added one by one until no lane is open.  Every turn of that loop closes at least its first lane.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const u64 todo = __builtin_amdgcn_ballot_w64(open);
        const int first = todo ? __ffsll((long long)todo) - 1 : 0;
        const unsigned fr = __shfl(r, first, 64);
        const bool mine = open && r == fr;
        const unsigned c = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(mine));  // 0: the wave has no open lane
        if (lane == 0) s_root[wave] = fr, s_cnt[wave] = c;
        open = open && !mine;
        __syncthreads();
        if (lane == 0 && c != 0) {
            bool head = true;
            unsigned total = 0;
            for (int w = 0; w < MT_CNT_WAVES; ++w) {
                const bool same = s_cnt[w] != 0 && s_root[w] == fr;
                head = head && !(same && w < wave);
                total += same && w >= wave ? s_cnt[w] : 0u;
            }
            if (head) {
                const unsigned before = atomicAdd(size + fr, total);
                key = (u64)(before + total) << 32 | (0xffffffffu - fr);
            }
        }
    }
    for (;;) {
        const u64 todo = __builtin_amdgcn_ballot_w64(open);
        if (todo == 0) break;
        const int first = __ffsll((long long)todo) - 1;
        const unsigned fr = __shfl(r, first, 64);
        const bool mine = open && r == fr;
        const unsigned c = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(mine));
        if (lane == first) {
            const unsigned before = atomicAdd(size + fr, c);
            const u64 offer = (u64)(before + c) << 32 | (0xffffffffu - fr);
            key = offer > key ? offer : key;
        }
        open = open && !mine;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = s_key[0];
        for (int w = 1; w < MT_CNT_WAVES; ++w) a = s_key[w] > a ? s_key[w] : a;
        if (a != 0) atomicMax(info + b * MT_INFO + (k - 1), a);
    }
}

// ---- conn -----------------------------------------------------------------------------------------------------------------------------------
// grid (eval_blocks(H * W), B): stage 1 settled, then the level counts over the image and n, conn_num over the region
__global__ __launch_bounds__(EV_THREADS) void mt_conn_kernel(const unsigned char* __restrict__ qbuf, const unsigned char* __restrict__ gt,
                                                             const unsigned char* __restrict__ region, const unsigned char* __restrict__ mbuf,
                                                             const unsigned* __restrict__ root, const unsigned char* __restrict__ level, u64* info,
                                                             long long hw, long long hwp, unsigned t_1, unsigned char* __restrict__ level_out) {
    __shared__ u64 s_part[EV_WAVES][MT_COUNTS];
    const long long b = blockIdx.y;
    qbuf += b * hwp, mbuf += b * hwp, root += b * hwp, level += b * hwp, gt += b * hw;
    if (region) region += b * hw;
    if (level_out) level_out += b * hw;
    const u64 best = info[b * MT_INFO];
    u64 n = 0, num = 0;
    unsigned cnt[MT_LEVELS + 1];  // per wave (uniform)
#pragma unroll
    for (int l = 0; l <= MT_LEVELS; ++l) cnt[l] = 0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    // (workgroup-uniform bounds: the ballots see whole waves)
    for (long long i0 = (long long)blockIdx.x * EV_THREADS; i0 < hw; i0 += stride) {
        const long long i = i0 + threadIdx.x;
        const bool in = i < hw;
        int lev = -1;
        if (in) {
            const unsigned m = mbuf[i];
            lev = mt_member(best, m, t_1, m >= t_1 ? root[i] : 0u) ? (int)level[i] : 0;
            if (level_out) level_out[i] = (unsigned char)lev;
            if (!region || region[i] != 0) {
                const int base = 255 * lev;
                int dg = 10 * (int)gt[i] - base, dq = 10 * (int)qbuf[i] - base;
                dg = dg >= 383 ? dg : 0, dq = dq >= 383 ? dq : 0;
                n += 1, num += (u64)(dg > dq ? dg - dq : dq - dg);
            }
        }
#pragma unroll
        for (int l = 0; l <= MT_LEVELS; ++l) cnt[l] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(lev == l));
    }
    n = wave_sum(n), num = wave_sum(num);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = n, s_part[wave][1] = num;
#pragma unroll
        for (int l = 0; l <= MT_LEVELS; ++l) s_part[wave][2 + l] = cnt[l];
    }
    __syncthreads();
    if (threadIdx.x < MT_COUNTS) {
        u64 a = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EV_WAVES; ++w) a += s_part[w][threadIdx.x];
        if (a != 0) atomicAdd(info + b * MT_INFO + MT_I_COUNTS + threadIdx.x, a);
    }
}

// ---- grad -----------------------------------------------------------------------------------------------------------------------------------
// grid (H * ceil(W / 256), B): one workgroup per 256 pixels of one row.  rows[pixel] = (sum_j D[j] qn, sum_j G[j] qn, sum_j D[j] gn, sum_j G[j] gn)
// over the columns clamp(x + j - 4), taps in index order from 0.0.
__global__ __launch_bounds__(EV_THREADS) void mt_grad_row_kernel(const unsigned char* __restrict__ qbuf, const unsigned char* __restrict__ gt,
                                                                 const u64* __restrict__ info, int W, int segs, long long hw, long long hwp,
                                                                 double4* __restrict__ rows) {
    __shared__ double s_q[EV_THREADS + 2 * MT_HALF], s_g[EV_THREADS + 2 * MT_HALF];
    const long long b = blockIdx.y;
    const int y = blockIdx.x / segs, x0 = (blockIdx.x - y * segs) * EV_THREADS;
    const unsigned char* qrow = qbuf + b * hwp + (long long)y * W;
    const unsigned char* grow = gt + b * hw + (long long)y * W;
    const u64* rg = info + b * MT_INFO + MT_I_RANGE;
    const unsigned q_lo = (unsigned)rg[0], q_hi = (unsigned)rg[1], g_lo = (unsigned)rg[2], g_hi = (unsigned)rg[3];
    const double q_den = (double)(q_hi - q_lo), g_den = (double)(g_hi - g_lo);
    for (int k = threadIdx.x; k < EV_THREADS + 2 * MT_HALF; k += EV_THREADS) {
        int xx = x0 + k - MT_HALF;
        xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
        s_q[k] = q_hi > q_lo ? (double)((unsigned)qrow[xx] - q_lo) / q_den : 0.0;
        s_g[k] = g_hi > g_lo ? (double)((unsigned)grow[xx] - g_lo) / g_den : 0.0;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    double dq = 0.0, sq = 0.0, dg = 0.0, sg = 0.0;
#pragma unroll
    for (int j = 0; j < MT_TAPS; ++j) {
        const double vq = s_q[threadIdx.x + j], vg = s_g[threadIdx.x + j];
        dq = dq + MT_D[j] * vq, sq = sq + MT_G[j] * vq;
        dg = dg + MT_D[j] * vg, sg = sg + MT_G[j] * vg;
    }
    rows[b * hw + (long long)y * W + x] = make_double4(dq, sq, dg, sg);
}

// grid (tx * ty, B): 32 x 8 tiles; slab = the tile's sum of err over the region
__global__ __launch_bounds__(EV_THREADS) void mt_grad_col_kernel(const double4* __restrict__ rows, const unsigned char* __restrict__ region, int H, int W,
                                                                 int tx, double* __restrict__ tslab, double* __restrict__ grad_map_out) {
    const long long b = blockIdx.y;
    const long long hw = (long long)H * W;
    const int by = blockIdx.x / tx, bx = blockIdx.x - by * tx;
    const int lx = threadIdx.x & (MT_TW - 1), ly = threadIdx.x / MT_TW;
    const int x = bx * MT_TW + lx, y = by * MT_TH + ly;
    rows += b * hw;
    double v[1] = {0.0};
    if (x < W && y < H) {
        double4 r[MT_TAPS];
#pragma unroll
        for (int i = 0; i < MT_TAPS; ++i) {
            int yy = y + i - MT_HALF;
            yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
            r[i] = rows[(long long)yy * W + x];
        }
        double gxq = 0.0, gyq = 0.0, gxg = 0.0, gyg = 0.0;
#pragma unroll
        for (int i = 0; i < MT_TAPS; ++i) {
            gxq = gxq + MT_G[i] * r[i].x, gyq = gyq + MT_D[i] * r[i].y;
            gxg = gxg + MT_G[i] * r[i].z, gyg = gyg + MT_D[i] * r[i].w;
        }
        const double aq = __dsqrt_rn(gxq * gxq + gyq * gyq), ag = __dsqrt_rn(gxg * gxg + gyg * gyg);
        const double d = aq - ag;
        const double err = d * d;
        const long long i = (long long)y * W + x;
        if (grad_map_out) grad_map_out[b * hw + i] = err;
        if (!region || region[b * hw + i] != 0) v[0] = err;
    }
    block_reduce_store<1>(v, tslab + b * gridDim.x + blockIdx.x);
}

// ---- values ---------------------------------------------------------------------------------------------------------------------------------
// one workgroup per image: thread t adds tiles t, t + 256, ... in that order, thread 0 the 256 partial sums in index order (the rule of
// eval_structure.hip's weighted F)
__global__ __launch_bounds__(EV_THREADS) void mt_finalise_kernel(const u64* __restrict__ info, const double* __restrict__ tslab, int ntile,
                                                                 double* __restrict__ out, u64* __restrict__ counts_out) {
    __shared__ double s_w[EV_THREADS];
    const long long b = blockIdx.x;
    const int t = threadIdx.x;
    const double* tiles = tslab + b * ntile;
    double f = 0.0;
    int j = t;
    for (; j + 7 * EV_THREADS < ntile; j += 8 * EV_THREADS) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = tiles[j + u * EV_THREADS];
#pragma unroll
        for (int u = 0; u < 8; ++u) f += v[u];
    }
    for (; j < ntile; j += EV_THREADS) f += tiles[j];
    s_w[t] = f;
    __syncthreads();
    const u64* c = info + b * MT_INFO + MT_I_COUNTS;
    if (counts_out && t < MT_COUNTS) counts_out[b * MT_COUNTS + t] = c[t];
    if (t != 0) return;
    double sum = 0.0;
    for (int k = 0; k < EV_THREADS; ++k) sum += s_w[k];
    double* o = out + b * MT_OUT;
    const u64 n = c[0];
    const double nan = __builtin_nan("");
    o[0] = (double)n;
    o[1] = n ? sum / 1000.0 : nan;
    o[2] = n ? (double)c[1] / 2550000.0 : nan;
    o[3] = n ? sum : nan;
}

}  // namespace

extern "C" {

long long gp_eval_matting_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return mat_ws(B, H, W).total;
}

gp_status gp_eval_matting(const void* pred, int pred_is_u8, const unsigned char* gt, const unsigned char* region, int B, int H, int W, double* out,
                          unsigned long long* counts_out, unsigned char* level_out, double* grad_map_out, void* workspace, long long workspace_bytes,
                          void* stream) {
    if (!pred || !gt || !out || !workspace) return GP_ERR_INVALID;
    if (!eval_dims_ok(B, H, W) || !eval_pred_ok(pred, pred_is_u8)) return GP_ERR_INVALID;
    if (!eval_aligned8(workspace, out, counts_out, grad_map_out)) return GP_ERR_INVALID;
    const MatWs w = mat_ws(B, H, W);
    if (workspace_bytes < w.total) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long hw = (long long)H * W;
    char* base = (char*)workspace;
    u64* info = (u64*)(base + w.info);
    unsigned* range = (unsigned*)(base + w.range);
    double* tslab = (double*)(base + w.tslab);
    unsigned char* qbuf = (unsigned char*)(base + w.qbuf);
    unsigned char* mbuf = (unsigned char*)(base + w.mbuf);
    unsigned char* level = (unsigned char*)(base + w.level);
    unsigned* parent = (unsigned*)(base + w.parent);
    unsigned* size = (unsigned*)(base + w.size);
    unsigned* root = (unsigned*)(base + w.root);
    double4* rows = (double4*)(base + w.rows);
    const dim3 pix((unsigned)((hw + EV_THREADS - 1) / EV_THREADS), B), cnt((unsigned)((hw + MT_CNT_THREADS - 1) / MT_CNT_THREADS), B);
    const auto prep = pred_is_u8 ? mt_prep_kernel<true> : mt_prep_kernel<false>;
    hipLaunchKernelGGL(prep, dim3(w.nblk, B), dim3(EV_THREADS), 0, s, pred, gt, (unsigned)W, hw, w.hwp, qbuf, mbuf, level, parent, range, info);
    hipLaunchKernelGGL(mt_range_kernel, dim3(B), dim3(64), 0, s, (const unsigned*)range, w.nblk, info);
    for (int k = MT_LEVELS; k >= 1; --k) {
        hipLaunchKernelGGL(mt_union_kernel, pix, dim3(EV_THREADS), 0, s, (const unsigned char*)mbuf, parent, size, (const unsigned*)root, level,
                           (const u64*)info, (unsigned)W, hw, w.hwp, MT_T[k - 1], MT_T[k], k == MT_LEVELS ? 0 : k + 1);
        hipLaunchKernelGGL(mt_count_kernel, cnt, dim3(MT_CNT_THREADS), 0, s, (const unsigned char*)mbuf, parent, size, root, info, hw, w.hwp, MT_T[k - 1], k);
    }
    hipLaunchKernelGGL(mt_conn_kernel, dim3(w.nblk, B), dim3(EV_THREADS), 0, s, (const unsigned char*)qbuf, gt, region, (const unsigned char*)mbuf,
                       (const unsigned*)root, (const unsigned char*)level, info, hw, w.hwp, MT_T[0], level_out);
    const int segs = (W + EV_THREADS - 1) / EV_THREADS;
    hipLaunchKernelGGL(mt_grad_row_kernel, dim3((unsigned)((long long)H * segs), B), dim3(EV_THREADS), 0, s, (const unsigned char*)qbuf, gt,
                       (const u64*)info, W, segs, hw, w.hwp, rows);
    hipLaunchKernelGGL(mt_grad_col_kernel, dim3((unsigned)((long long)w.tx * w.ty), B), dim3(EV_THREADS), 0, s, (const double4*)rows, region, H, W, w.tx,
                       tslab, grad_map_out);
    hipLaunchKernelGGL(mt_finalise_kernel, dim3(B), dim3(EV_THREADS), 0, s, (const u64*)info, (const double*)tslab, w.tx * w.ty, out, counts_out);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

}  // extern "C"
