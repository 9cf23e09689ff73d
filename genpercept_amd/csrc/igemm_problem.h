// The launch forms of launch_igemm (kernels.h): one builder of IGemmParams per form, shared by the engine's layer ops (engine.hip) and the per-kernel
// entry points the tests and tools drive (kernel_abi.hip), so that "what the tests launch" and "what the engine launches" are the same code.
// Host-only; plain pointers and ints in, a value-initialised IGemmParams with the form's fields out.  What is a caller's policy is set by the caller
// after the builder call: dbg, stats_out, the split-K workspace, in_scale / in_shift / in_silu.
#pragma once
#include <stdexcept>
#include <string>

#include "kernels.h"

#define HIPCHK(x)                                                                                         \
    do {                                                                                                  \
        hipError_t _e = (x);                                                                              \
        if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #x); \
    } while (0)

namespace {  // (internal linkage: both translation units that include this keep their own copies, nothing reaches the dynamic symbol table)

struct PackedW {
    h16_t* w = nullptr;   // [n_rows][taps][cin_pad]
    h16_t* w_ph = nullptr;  // x2-upsample convs only: [n_rows][4 phases][2 x 2 taps][cin_pad], kernel rows / columns on the same source pixel summed (pack_phases)
    float* bias = nullptr; // [cout] or null
    int cout = 0, cin_pad = 0, ks = 1, n_rows = 0;
};
struct Nhwc {  // an NHWC tensor, or B * H * W matrix rows of stride C
    const h16_t* p;
    int B, H, W, C;  // C = allocated channels (row stride)
};
struct ConvForm {
    int stride = 1, pad_t = 1, pad_l = 1;
    int Ho = 0, Wo = 0;     // 0: same as input (or upsampled size)
    int ups_h = 0, ups_w = 0;
    const h16_t* res = nullptr;
    int act = GP_ACT_NONE;
    int n_store = 0;        // 0: the output width
};
struct GemmMat {  // one operand of a batched plain GEMM: rows of stride ld elements, batch stride bs elements
    const void* p;
    int ld;
    long long bs;
};

// columns a layer of `cout` weight rows stores: GEGLU multiplies the value half by the gated half
inline int igemm_out_width(int cout, int act) { return act == GP_ACT_GEGLU ? cout / 2 : cout; }

// conv: NHWC input x, packed weight (1x1 or 3x3), geometry / residual / act / n_store from `o`, phase weights on an upsample conv
inline IGemmParams igemm_conv(const Nhwc& x, const PackedW& w, const ConvForm& o, void* out, const h16_t* zero) {
    if (x.C != w.cin_pad) throw std::logic_error("conv: channel mismatch (" + std::to_string(x.C) + " vs " + std::to_string(w.cin_pad) + ")");
    const int Hin = o.ups_h ? o.ups_h : x.H, Win = o.ups_w ? o.ups_w : x.W;
    const int Ho = o.Ho ? o.Ho : Hin, Wo = o.Wo ? o.Wo : Win;
    const int nst = o.n_store ? o.n_store : igemm_out_width(w.cout, o.act);
    IGemmParams p{};
    p.in = x.p; p.wt = w.w; p.bias = w.bias; p.res = o.res; p.out = out; p.zero = zero;
    p.M = x.B * Ho * Wo; p.N = w.cout; p.Cin = w.cin_pad; p.n_rows = w.n_rows; p.ks = w.ks;
    p.B = x.B; p.Hi = x.H; p.Wi = x.W; p.Ho = Ho; p.Wo = Wo;
    p.stride = o.stride; p.pad_t = w.ks == 3 ? o.pad_t : 0; p.pad_l = w.ks == 3 ? o.pad_l : 0;
    p.ups = o.ups_h ? 1 : 0; p.Hu = o.ups_h; p.Wu = o.ups_w;
    p.wt_ph = o.ups_h ? w.w_ph : nullptr;  // (used where the size is exactly x2: conv_halo_uses_phases)
    p.lda = x.C; p.ldo = nst; p.ldres = nst; p.ldw = (w.ks == 3 ? 9 : 1) * w.cin_pad;
    p.n_store = nst; p.out_fp32 = 0; p.act = o.act; p.bias_mode = w.bias ? GP_BIAS_COL : GP_BIAS_NONE;
    p.batch = 1;
    return p;
}

// linear: y[M][N] = x[M][K] W^T (+ column bias) (+ res), M = the rows of x, N = w.cout (GEGLU halves the stored width).  The image geometry is
// kept: igemm_tile_info needs B to keep a statistics tile inside one image.
inline IGemmParams igemm_linear(const Nhwc& x, const PackedW& w, const h16_t* res, int act, void* out, const h16_t* zero) {
    if (x.C != w.cin_pad) throw std::logic_error("linear: channel mismatch");
    const int nout = igemm_out_width(w.cout, act);
    IGemmParams p{};
    p.in = x.p; p.wt = w.w; p.bias = w.bias; p.res = res; p.out = out; p.zero = zero;
    p.M = (int)((long long)x.B * x.H * x.W); p.N = w.cout; p.Cin = w.cin_pad; p.n_rows = w.n_rows; p.ks = 1;
    p.B = x.B; p.Hi = x.H; p.Wi = x.W; p.Ho = x.H; p.Wo = x.W; p.stride = 1;
    p.lda = x.C; p.ldo = nout; p.ldres = nout; p.ldw = w.cin_pad; p.n_store = nout; p.act = act;
    p.bias_mode = w.bias ? GP_BIAS_COL : GP_BIAS_NONE; p.batch = 1;
    return p;
}

// contract precision (contract.hip), on top of igemm_conv / igemm_linear over a split operand: fp32 rows out, fp32 residual
inline void igemm_contract(IGemmParams& p, const float* res_f) {
    p.out_fp32 = 1;
    p.res = (const h16_t*)res_f; p.res_f32 = res_f ? 1 : 0;
}

// batched plain GEMM: out[z][M][n_store] = a[z][M][K] bt[z][N][K]^T (+ bias by column or by row), z < batch; n_rows = rows of bt that may be read
inline IGemmParams igemm_bgemm(const GemmMat& a, const GemmMat& bt, const GemmMat& out, int M, int N, int K, int n_rows, int n_store, int batch,
                               const float* bias, int bias_mode, int out_fp32, const h16_t* zero) {
    IGemmParams p{};
    p.in = (const h16_t*)a.p; p.wt = (const h16_t*)bt.p; p.bias = bias; p.out = (void*)out.p; p.zero = zero;
    p.M = M; p.N = N; p.Cin = K; p.n_rows = n_rows; p.ks = 1; p.stride = 1;
    p.lda = a.ld; p.ldw = bt.ld; p.ldo = out.ld; p.n_store = n_store; p.out_fp32 = out_fp32;
    p.bias_mode = bias ? bias_mode : GP_BIAS_NONE;
    p.batch = batch; p.in_bs = a.bs; p.wt_bs = bt.bs; p.out_bs = out.bs;
    return p;
}

// fused q | k | V^T projection of a self-attention over C channels (pgemm.hip only): the rows of x times the stacked [3C][K] weight; columns [0, 2C)
// go to qk_out row-major, the V third transposed to vt_out [B][C][Tpad] with T = x.H * x.W tokens per image (IGemmParams::vt_out)
inline IGemmParams igemm_qkv(const Nhwc& x, const h16_t* w, int ldw, int n_rows, int K, int C, int Tpad, void* qk_out, h16_t* vt_out, const h16_t* zero) {
    IGemmParams p{};
    p.in = x.p; p.wt = w; p.out = qk_out; p.zero = zero;
    p.M = (int)((long long)x.B * x.H * x.W); p.N = 3 * C; p.Cin = K; p.n_rows = n_rows; p.ks = 1;
    p.B = x.B; p.Hi = x.H; p.Wi = x.W; p.Ho = x.H; p.Wo = x.W; p.stride = 1;
    p.lda = x.C; p.ldo = 2 * C; p.ldres = 2 * C; p.ldw = ldw; p.n_store = 2 * C; p.act = GP_ACT_NONE;
    p.bias_mode = GP_BIAS_NONE; p.batch = 1;
    p.vt_out = vt_out; p.vt_col0 = 2 * C; p.vt_T = x.H * x.W; p.vt_Tpad = Tpad;
    return p;
}
// ... whose launch writes V^T up to T only: keys beyond T must read as zero
inline void igemm_qkv_clear_pad(const IGemmParams& p, hipStream_t s) {
    if (p.vt_Tpad != p.vt_T) HIPCHK(hipMemsetAsync(p.vt_out, 0, (size_t)p.B * (p.N - p.vt_col0) * p.vt_Tpad * sizeof(h16_t), s));
}

}  // namespace
