// Per-kernel entry points of the C-ABI (include/genpercept_hip.h): the stateless interface the parity tests and tools/kbench drive, one kernel
// (or one short launch sequence) per call on the caller's stream.  None of them takes a gp_engine; the conv / GEMM entries build their launch
// parameters with the builders the engine's layer ops use (igemm_problem.h) and pack weights with the engine's packers (host_pack.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "../../include/genpercept_hip.h"
#include "host_pack.h"
#include "igemm_problem.h"

// Scratch of the per-kernel entry points (the parity-test interface below; engines use their own pool): one set per DEVICE, and the
// entry points that use it hold g_scratch_mu for the duration of their enqueue, so two host threads cannot resize it under each other.
struct DevScratch {
    h16_t* zero = nullptr;
    float* bufs[3] = {nullptr, nullptr, nullptr};  // 0: GroupNorm workspace, 1: statistics partials, 2: split-K partial sums
    size_t floats[3] = {0, 0, 0};
};
static std::mutex g_scratch_mu;
static std::map<int, DevScratch> g_scratch;
static DevScratch& dev_scratch() {  // call with g_scratch_mu held
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    return g_scratch[dev];
}
static h16_t* zero_page() {
    DevScratch& d = dev_scratch();
    if (!d.zero) {
        HIPCHK(hipMalloc((void**)&d.zero, 4096));
        HIPCHK(hipMemset(d.zero, 0, 4096));
    }
    return d.zero;
}
static float* scratch_floats(int which, size_t need) {
    DevScratch& d = dev_scratch();
    if (need > d.floats[which]) {
        if (d.bufs[which]) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(d.bufs[which])); d.bufs[which] = nullptr; d.floats[which] = 0; }
        HIPCHK(hipMalloc((void**)&d.bufs[which], need * sizeof(float)));
        d.floats[which] = need;
    }
    return d.bufs[which];
}
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }  // (nullptr passes: optional arguments are checked for presence separately)
// split-K workspace for a per-kernel call (engines take theirs from the pool)
static void attach_splitk_scratch(IGemmParams& p, int tile_hint) {
    const int S = igemm_ksplit(p, tile_hint);
    if (S > 1) {
        p.splitk_ws_floats = (long long)S * p.M * p.n_store;
        p.splitk_ws = scratch_floats(2, (size_t)p.splitk_ws_floats);
    }
}
// What every per-kernel entry point that uses the scratch runs its body in: the scratch lock, the A/B switches as the environment has them NOW,
// the launch error check after a body that returned GP_OK (any other status is returned as it is), every exception as GP_ERR_HIP.
// Argument validation stays in front of it, in the entry point.
template <typename F>
static gp_status kernel_entry(F&& f) {
    try {
        std::lock_guard<std::mutex> g(g_scratch_mu);
        gp_switches_reload();
        const gp_status st = f();
        if (st != GP_OK) return st;
        HIPCHK(hipGetLastError());
        return GP_OK;
    } catch (...) { return GP_ERR_HIP; }
}
static PackedW packed_w(const void* w, const void* w_phases, const float* bias, int cout, int cin_pad, int ks) {
    PackedW pw;
    pw.w = (h16_t*)w; pw.w_ph = (h16_t*)w_phases; pw.bias = (float*)bias; pw.cout = cout; pw.cin_pad = cin_pad; pw.ks = ks; pw.n_rows = gp_packed_rows(cout);
    return pw;
}
// optional tail of a conv entry point: GroupNorm scale / shift of the conv's output from the statistics its epilogue leaves (gamma null: none)
struct GnTail {
    const float *gamma = nullptr, *beta = nullptr;
    int groups = 0;
    float eps = 0.f;
    float *scale_out = nullptr, *shift_out = nullptr;
};
// gp_conv2d_up2 / gp_conv2d_up2_stats / gp_conv2d_stats: a stride-1 "same" conv, optionally behind the x2 nearest upsample (+ GnTail).
// need_phases: refuse anything but the phase kernel.
static gp_status conv_same(const Nhwc& x, const PackedW& w, const void* residual, void* out, bool ups, int tile_hint, bool need_phases, const GnTail& gn,
                           hipStream_t stream) {
    ConvForm o;
    if (ups) { o.ups_h = 2 * x.H; o.ups_w = 2 * x.W; }
    o.res = (const h16_t*)residual;
    IGemmParams p = igemm_conv(x, w, o, out, zero_page());
    p.dbg = gp_sw().igemm_dbg;
    if (need_phases && (!conv_uses_halo(p, tile_hint) || !conv_halo_uses_phases(p))) return GP_ERR_INVALID;
    int mode = 0, bm = 0;
    if (gn.gamma) {
        const int nt = igemm_tile_info(p, tile_hint, &mode, &bm);
        if (nt <= 0) return GP_ERR_INVALID;  // this kernel path leaves no statistics
        p.stats_out = scratch_floats(1, (size_t)nt * (w.cout * 2 + 1));
    }
    launch_igemm(p, tile_hint, stream);
    if (gn.gamma)
        launch_groupnorm_from_partials(p.stats_out, mode, bm, x.B, p.Ho, p.Wo, w.cout, gn.groups, gn.eps, gn.gamma, gn.beta, gn.scale_out, gn.shift_out, stream);
    return GP_OK;
}

// gp_pack_weight(_split) / gp_pack_weight_phases(_split): host_pack.h's layouts into a device buffer of the caller; split = contract precision
// (ks == 0: the x2-upsample conv's phase weights)
static gp_status pack_weight(const float* w, int cout, int cin, int ks, int cin_pad, int geglu, bool split, void* dev_out) {
    if (!w || !dev_out || cout < 1 || cin < 1 || (ks != 0 && ks != 1 && ks != 3) || cin_pad < cin || (cin_pad % 64)) return GP_ERR_INVALID;
    try {
        const int n_rows = gp_packed_rows(cout);
        std::vector<h16_t> buf((size_t)n_rows * (ks ? ks * ks : 16) * (split ? 3 : 1) * cin_pad, 0);
        if (ks) pack_rows(w, cout, cin, ks, cin_pad, geglu != 0, buf, 0, n_rows, split);
        else pack_phase_rows(w, cout, cin, cin_pad, buf, split);
        HIPCHK(hipMemcpy(dev_out, buf.data(), buf.size() * 2, hipMemcpyHostToDevice));
        return GP_OK;
    } catch (...) { return GP_ERR_HIP; }
}

extern "C" {

// ---- per-kernel entry points --------------------------------------------------------------------------------------
int gp_packed_rows(int cout) { return (cout + 255) / 256 * 256; }
int gp_last_igemm_path(int* pgemm_rows) { return igemm_last_path(pgemm_rows); }
int gp_latent_size(int x) { for (int i = 0; i < 3; ++i) x = (x - 2) / 2 + 1; return x; }
int gp_dpt_out_size(int latent) { for (int i = 0; i < 2; ++i) latent = (latent - 1) / 2 + 1; return 32 * latent; }

gp_status gp_pack_weight(const float* w, int cout, int cin, int ks, int cin_pad, int geglu, void* dev_out) {
    return ks ? pack_weight(w, cout, cin, ks, cin_pad, geglu, false, dev_out) : GP_ERR_INVALID;
}
gp_status gp_pack_weight_phases(const float* w, int cout, int cin, int cin_pad, void* dev_out) { return pack_weight(w, cout, cin, 0, cin_pad, 0, false, dev_out); }
gp_status gp_pack_weight_split(const float* w, int cout, int cin, int ks, int cin_pad, int geglu, void* dev_out) {
    return ks && !GP_F16 ? pack_weight(w, cout, cin, ks, cin_pad, geglu, true, dev_out) : GP_ERR_INVALID;
}
gp_status gp_pack_weight_phases_split(const float* w, int cout, int cin, int cin_pad, void* dev_out) {
    return GP_F16 ? GP_ERR_INVALID : pack_weight(w, cout, cin, 0, cin_pad, 0, true, dev_out);
}

gp_status gp_conv2d(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int Hi, int Wi, int Cin,
                    int Cout, int ks, int stride, int pad_t, int pad_l, int Ho, int Wo, int ups_h, int ups_w, int act, int n_store,
                    int out_fp32, int tile_hint, void* stream) {
    if (!in || !w_packed || !out || (Cin % 64) || (ks != 1 && ks != 3)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        ConvForm o;
        o.stride = stride; o.pad_t = pad_t; o.pad_l = pad_l; o.Ho = Ho; o.Wo = Wo; o.ups_h = ups_h; o.ups_w = ups_w;
        o.res = (const h16_t*)residual; o.act = act; o.n_store = n_store > 0 ? n_store : 0;
        IGemmParams p = igemm_conv({(const h16_t*)in, B, Hi, Wi, Cin}, packed_w(w_packed, nullptr, bias, Cout, Cin, ks), o, out, zero_page());
        p.out_fp32 = out_fp32;
        p.dbg = gp_sw().igemm_dbg;  // profiling ablations (tools/conv_bench.py)
        attach_splitk_scratch(p, tile_hint);
        launch_igemm(p, tile_hint, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_conv2d_up2(const void* in, const void* w_packed, const void* w_phases, const float* bias, const void* residual, void* out, int B, int Hi, int Wi,
                        int Cin, int Cout, void* stream) {
    if (!in || !w_packed || !w_phases || !out || (Cin % 64) || (Cout % 8)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {  // (this entry point exists to test the phase kernel)
        return conv_same({(const h16_t*)in, B, Hi, Wi, Cin}, packed_w(w_packed, w_phases, bias, Cout, Cin, 3), residual, out, true, 5, true, GnTail{}, (hipStream_t)stream);
    });
}

gp_status gp_conv2d_up2_stats(const void* in, const void* w_packed, const void* w_phases, const float* bias, const void* residual, void* out, int B, int Hi,
                              int Wi, int Cin, int Cout, const float* gamma, const float* beta, int groups, float eps, float* scale_out, float* shift_out,
                              void* stream) {
    if (!in || !w_packed || !w_phases || !out || !gamma || !beta || !scale_out || !shift_out || (Cin % 64) || (Cout % 8) || groups < 1 || (Cout % groups))
        return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        return conv_same({(const h16_t*)in, B, Hi, Wi, Cin}, packed_w(w_packed, w_phases, bias, Cout, Cin, 3), residual, out, true, 5, true,
                         GnTail{gamma, beta, groups, eps, scale_out, shift_out}, (hipStream_t)stream);
    });
}

gp_status gp_conv2d_gn(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int H, int W, int Cin,
                       int Cout, int ups, int act, const float* gamma, const float* beta, int groups, float eps, int silu, void* stream) {
    if (!in || !w_packed || !out || !gamma || !beta || (Cin % 64) || (Cin % groups)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        ConvForm o;
        if (ups) { o.ups_h = 2 * H; o.ups_w = 2 * W; }
        o.res = (const h16_t*)residual; o.act = act;
        IGemmParams p = igemm_conv({(const h16_t*)in, B, H, W, Cin}, packed_w(w_packed, nullptr, bias, Cout, Cin, 3), o, out, zero_page());
        p.dbg = gp_sw().igemm_dbg;
        float* ws = scratch_floats(0, groupnorm_ws_layout(B, H * W, Cin, groups));
        float *scale, *shift;
        groupnorm_ws_layout(B, H * W, Cin, groups, ws, &scale, &shift);
        launch_groupnorm_stats((const h16_t*)in, gamma, beta, B, H * W, Cin, groups, eps, ws, scale, shift, (hipStream_t)stream);
        p.in_scale = scale; p.in_shift = shift; p.in_silu = silu;
        if (!conv_uses_halo(p, 5)) return GP_ERR_INVALID;
        launch_igemm(p, 5, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_rgb_conv_in(const void* rgb, int is_u8, const void* w_packed, const float* bias, void* out, int B, int H, int W, int Cout, void* stream) {
    if (!rgb || !w_packed || !out || B < 1 || H < 1 || W < 1 || (Cout % 32)) return GP_ERR_INVALID;
    h16_t* w27 = nullptr;
    if (hipMalloc((void**)&w27, (size_t)Cout * 32 * sizeof(h16_t)) != hipSuccess) return GP_ERR_HIP;
    launch_pack_k27((const h16_t*)w_packed, 9 * 64, Cout, w27, (hipStream_t)stream);
    launch_rgb_conv_in(rgb, is_u8, w27, bias, (h16_t*)out, nullptr, B, H, W, Cout, (hipStream_t)stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(w27);
    return (e == hipSuccess && hipGetLastError() == hipSuccess) ? GP_OK : GP_ERR_HIP;
}

gp_status gp_conv2d_stats(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int H, int W, int Cin,
                          int Cout, int ks, int ups, int tile_hint, const float* gamma, const float* beta, int groups, float eps,
                          float* scale_out, float* shift_out, void* stream) {
    if (!in || !w_packed || !out || !gamma || !beta || !scale_out || !shift_out || (Cin % 64) || (ks != 1 && ks != 3) || groups < 1 || (Cout % groups))
        return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        return conv_same({(const h16_t*)in, B, H, W, Cin}, packed_w(w_packed, nullptr, bias, Cout, Cin, ks), residual, out, ups != 0, tile_hint, false,
                         GnTail{gamma, beta, groups, eps, scale_out, shift_out}, (hipStream_t)stream);
    });
}

gp_status gp_gemm(const void* a, int lda, const void* bt, int ldb, const float* bias, int bias_mode, const void* residual, int ldres, void* out,
                  int ldo, int M, int N, int K, int n_rows_bt, int n_store, int act, int out_fp32, int batch, long long a_bs, long long bt_bs,
                  long long out_bs, int tile_hint, void* stream) {
    if (!a || !bt || !out || (K % 64)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        IGemmParams p = igemm_bgemm({a, lda, a_bs}, {bt, ldb, bt_bs}, {out, ldo, out_bs}, M, N, K, n_rows_bt, n_store > 0 ? n_store : N, batch > 0 ? batch : 1, bias,
                                    bias_mode, out_fp32, zero_page());
        p.res = (const h16_t*)residual; p.ldres = ldres; p.act = act;  // (beyond the engine's batched GEMMs: tests reach residual and GEGLU epilogues here)
        p.dbg = gp_sw().igemm_dbg;  // profiling ablations (tools/kbench)
        attach_splitk_scratch(p, tile_hint);
        launch_igemm(p, tile_hint, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_decoder_tail(const void* in, const void* w_packed, const float* bias, const float* gamma, const float* beta, int groups, float eps,
                          int B, int H, int W, int Cin, int mean3, int raw, float* out, void* stream) {
    if (!in || !w_packed || !gamma || !beta || !out || B < 1 || !conv_few_applicable(Cin, 3, H, W) || (Cin % groups)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        float* ws = scratch_floats(0, groupnorm_ws_layout(B, H * W, Cin, groups));
        float *scale, *shift;
        groupnorm_ws_layout(B, H * W, Cin, groups, ws, &scale, &shift);
        launch_groupnorm_stats((const h16_t*)in, gamma, beta, B, H * W, Cin, groups, eps, ws, scale, shift, (hipStream_t)stream);
        launch_conv_few((const h16_t*)in, (const h16_t*)w_packed, bias, scale, shift, zero_page(), out, B, H, W, 1, mean3, raw, 0, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_gemm_qkv(const void* a, int lda, const void* w_packed, int ldw, int n_rows_w, int K, void* qk_out, void* vt_out, int B, int T, int C,
                      int Tpad, void* stream) {
    if (!a || !w_packed || !qk_out || !vt_out || (K % 64) || B < 1 || T < 1 || C < 1 || Tpad < T) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        IGemmParams p = igemm_qkv({(const h16_t*)a, B, T, 1, lda}, (const h16_t*)w_packed, ldw, n_rows_w, K, C, Tpad, qk_out, (h16_t*)vt_out, zero_page());
        p.dbg = gp_sw().igemm_dbg;
        if (!igemm_uses_pgemm(p, 0)) return GP_ERR_INVALID;  // only the persistent GEMM has the transposed epilogue
        igemm_qkv_clear_pad(p, (hipStream_t)stream);
        launch_igemm(p, 0, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int silu, void* stream) {
    if (!x || !y || !gamma || !beta || (C % 8) || (C % G)) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        float* g_gn_ws = scratch_floats(0, groupnorm_ws_layout(B, HW, C, G));
        if (groupnorm_small_applicable(B, HW, C, G)) launch_groupnorm_small((const h16_t*)x, (h16_t*)y, gamma, beta, B, HW, C, G, eps, silu, (hipStream_t)stream);
        else launch_groupnorm((const h16_t*)x, (h16_t*)y, gamma, beta, B, HW, C, G, eps, silu, g_gn_ws, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_layernorm(const void* x, void* y, const float* gamma, const float* beta, int rows, int C, float eps, void* stream) {
    if (!x || !y || (C % 8) || C > 4096) return GP_ERR_INVALID;
    launch_layernorm((const h16_t*)x, (h16_t*)y, gamma, beta, rows, C, eps, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_flash_attention(const void* q, const void* k, const void* vt, void* out, int B, int T, int heads, int ldq, int ldk, int Tpad, int ldo,
                             void* stream) {
    if (!q || !k || !vt || !out || (Tpad % 64) || Tpad < T) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        launch_flash_attn64((const h16_t*)q, (const h16_t*)k, (const h16_t*)vt, (h16_t*)out, B, T, heads, ldq, ldk, Tpad, ldo,
                            (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_flash_attention_split(const float* qkv, int ld, void* out_split, int B, int T, int heads, void* stream) {
    if (!qkv || !out_split || B < 1 || T < 1 || heads < 1 || ld < 3 * heads * 64 || (ld % 4) || !al16(qkv) || !al16(out_split) || GP_F16)
        return GP_ERR_INVALID;  // (c_qk_planes_kernel reads float4 pairs: 16-byte aligned rows)
    return kernel_entry([&]() -> gp_status {
        const int C = heads * 64, Tpad = (T + 63) / 64 * 64;
        const size_t n_qk = (size_t)B * T * 2 * C, n_vt = (size_t)B * heads * 64 * Tpad;
        h16_t* buf = nullptr;
        HIPCHK(hipMalloc((void**)&buf, (2 * n_qk + 2 * n_vt) * sizeof(h16_t)));
        h16_t *qk_hi = buf, *qk_lo = buf + n_qk, *vt_hi = buf + 2 * n_qk, *vt_lo = vt_hi + n_vt;
        launch_c_qkv_planes(qkv, ld, qk_hi, qk_lo, vt_hi, vt_lo, B, T, Tpad, heads, 64, (hipStream_t)stream);
        launch_flash_attn64_split(qk_hi, qk_lo, vt_hi, vt_lo, (h16_t*)out_split, B, T, heads, 2 * C, Tpad, (hipStream_t)stream);
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        (void)hipFree(buf);
        if (e != hipSuccess) return GP_ERR_HIP;
        return GP_OK;
    });
}

gp_status gp_flash_attention_hd512_split(const float* qkv, int ld, void* out_split, int B, int T, float scale, void* stream) {
    if (!qkv || !out_split || B < 1 || T < 1 || ld < 1536 || (ld % 4) || !al16(qkv) || !al16(out_split) || GP_F16 || !flash_attn512_split_supported(T))
        return GP_ERR_INVALID;  // (c_qk_planes_kernel reads float4 pairs: 16-byte aligned rows)
    return kernel_entry([&]() -> gp_status {
        const int Tpad = (T + 63) / 64 * 64;
        const size_t n_qk = (size_t)B * T * 1024, n_vt = (size_t)B * 512 * Tpad;
        h16_t* buf = nullptr;
        HIPCHK(hipMalloc((void**)&buf, (2 * n_qk + 2 * n_vt) * sizeof(h16_t)));
        h16_t *qk_hi = buf, *qk_lo = buf + n_qk, *vt_hi = buf + 2 * n_qk, *vt_lo = vt_hi + n_vt;
        launch_c_qkv_planes(qkv, ld, qk_hi, qk_lo, vt_hi, vt_lo, B, T, Tpad, 1, 512, (hipStream_t)stream);
        launch_flash_attn512_split(qk_hi, qk_lo, vt_hi, vt_lo, (h16_t*)out_split, B, T, Tpad, scale, (hipStream_t)stream);
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        (void)hipFree(buf);
        if (e != hipSuccess) return GP_ERR_HIP;
        return GP_OK;
    });
}

gp_status gp_c_attention_plan(int B, int T, int heads, int hd, int* path, long long* workspace_bytes) {
    if (B < 1 || T < 1 || heads < 1 || hd < 64 || (hd % 64) || !path || !workspace_bytes) return GP_ERR_INVALID;
    gp_switches_reload();
    *path = c_attention_plan(B, T, heads, hd, workspace_bytes);
    return GP_OK;
}

// ---- contract-precision test entry points (bf16 library only): the launchers the engine's conv_c / linear_c / groupnorm use ---------------
gp_status gp_c_split3(const float* x, int ldx, void* out, long long rows, int C, int b_order, int act, float scale, void* stream) {
    if (GP_F16 || !x || !out || rows < 1 || C < 8 || (C % 8) || ldx < C || (ldx % 4) || !al16(x) || !al16(out) || (b_order != 0 && b_order != 1) ||
        (act != GP_ACT_NONE && act != GP_ACT_RELU))  // (the acts the engine splits with: split_operand)
        return GP_ERR_INVALID;
    launch_c_split3(x, ldx, (h16_t*)out, rows, C, b_order, act, scale, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_c_groupnorm_split(const float* x, void* out, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int silu,
                               float* scale_out, float* shift_out, void* stream) {
    if (GP_F16 || !x || !out || !gamma || !beta || !scale_out || !shift_out || B < 1 || HW < 1 || C < 8 || (C % 8) || G < 1 || (C % G) || !al16(x) ||
        !al16(out) || !al16(scale_out) || !al16(shift_out))
        return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        float* part = scratch_floats(1, (size_t)B * c_gn_stat_rows(HW, C, nullptr) * (2 * C + 1));
        launch_c_groupnorm_scale_shift(x, part, B, HW, 1, C, G, eps, gamma, beta, scale_out, shift_out, (hipStream_t)stream);
        launch_c_gn_apply_split(x, (h16_t*)out, scale_out, shift_out, B, HW, C, silu ? 1 : 0, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_c_conv2d(const void* in_split, const void* w_packed, const void* w_phases, const float* bias, const float* residual, float* out, int B,
                      int Hi, int Wi, int Cin, int Cout, int ks, int stride, int pad_t, int pad_l, int Ho, int Wo, int ups, int act, int tile_hint,
                      const float* gamma, const float* beta, int groups, float eps, float* scale_out, float* shift_out, int* path_out, void* stream) {
    const int nout = act == GP_ACT_GEGLU ? Cout / 2 : Cout;
    if (GP_F16 || !in_split || !w_packed || !out || B < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Cin < 64 || (Cin % 64) || Cout < 8 || (nout % 8) ||
        (ks != 1 && ks != 3) || (stride != 1 && stride != 2) || (ups && (ks != 3 || stride != 1)) || (act == GP_ACT_GEGLU && (ks != 1 || (Cout % 16))) ||
        (act != GP_ACT_NONE && act != GP_ACT_GEGLU && act != GP_ACT_SILU && act != GP_ACT_RELU) || !al16(in_split) || !al16(w_packed) || !al16(out) ||
        !al16(residual) || !al16(bias) || !al16(w_phases))
        return GP_ERR_INVALID;
    const bool stats = gamma != nullptr;
    if (stats && (!beta || !scale_out || !shift_out || groups < 1 || (nout % groups) || act == GP_ACT_GEGLU || !al16(scale_out) || !al16(shift_out)))
        return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        // the engine's own parameter setup (gp_engine::conv_c / linear_c): the same builders over the split operand and its tripled width
        const Nhwc xs{(const h16_t*)in_split, B, Hi, Wi, 3 * Cin};
        const PackedW pw = packed_w(w_packed, w_phases, bias, Cout, 3 * Cin, ks);
        ConvForm o;
        o.stride = stride; o.pad_t = pad_t; o.pad_l = pad_l; o.Ho = Ho; o.Wo = Wo; o.ups_h = ups ? 2 * Hi : 0; o.ups_w = ups ? 2 * Wi : 0;
        o.act = act;
        const bool is_linear = ks == 1 && stride == 1 && !ups && Ho == Hi && Wo == Wi;  // a linear layer (linear_c)
        IGemmParams p = is_linear ? igemm_linear(xs, pw, nullptr, act, out, zero_page()) : igemm_conv(xs, pw, o, out, zero_page());
        igemm_contract(p, residual);
        p.dbg = gp_sw().igemm_dbg;
        attach_splitk_scratch(p, tile_hint);
        if (path_out) *path_out = igemm_path(p, tile_hint);
        launch_igemm(p, tile_hint, (hipStream_t)stream);
        if (stats) {
            float* part = scratch_floats(1, (size_t)B * c_gn_stat_rows(Ho * Wo, nout, nullptr) * (2 * nout + 1));
            launch_c_groupnorm_scale_shift(out, part, B, Ho, Wo, nout, groups, eps, gamma, beta, scale_out, shift_out, (hipStream_t)stream);
        }
        return GP_OK;
    });
}

gp_status gp_c_layernorm_split(const float* x, void* out, const float* gamma, const float* beta, int rows, int C, float eps, void* stream) {
    if (GP_F16 || !x || !out || !gamma || !beta || rows < 1 || C < 8 || (C % 8) || !al16(x) || !al16(out) || !al16(gamma) || !al16(beta))
        return GP_ERR_INVALID;
    launch_c_layernorm_split(x, (h16_t*)out, gamma, beta, rows, C, eps, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_c_softmax_split(const float* in, void* out, int rows, int T, int ld, float scale, void* stream) {
    if (GP_F16 || !in || !out || rows < 1 || T < 1 || ld < T || !c_softmax_split_supported(ld) || !al16(in) || !al16(out)) return GP_ERR_INVALID;
    launch_c_softmax_split(in, (h16_t*)out, rows, T, ld, scale, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_flash_attention_hd512(const void* q, const void* k, const void* vt, void* out, int B, int T, int ldq, int ldk, int Tpad, int ldo,
                                   float scale, int ncu, void* stream) {
    if (!q || !k || !vt || !out || (Tpad % 64) || Tpad < T || B < 1 || T < 1 || ncu < 0) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        if (ncu == 0) {
            int dev = 0;
            hipDeviceProp_t pr;
            HIPCHK(hipGetDevice(&dev));
            HIPCHK(hipGetDeviceProperties(&pr, dev));
            ncu = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
        }
        const long long wsf = flash_attn512_workspace_floats(B, T, ncu);
        float* ws = wsf ? scratch_floats(2, (size_t)wsf) : nullptr;
        launch_flash_attn512((const h16_t*)q, (const h16_t*)k, (const h16_t*)vt, (h16_t*)out, ws, B, T, ldq, ldk, Tpad, ldo, scale,
                             ncu, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_cross_attention(const void* q, const float* kc, const float* vc, void* out, int rows, int C, int L, void* stream) {
    if (!q || !kc || !vc || !out || (C % 64)) return GP_ERR_INVALID;
    launch_cross_attn_small((const h16_t*)q, kc, vc, (h16_t*)out, rows, C, L, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_cross_attention_fold(const void* y, void* y_out, void* n3_out, const float* U, const float* u0, const float* G, const float* c0,
                                  const float* g3, const float* b3, int rows, int C, int heads, float eps, void* stream) {
    if (!y || !y_out || !U || !u0 || !G || !c0 || !cross_attn_fold_supported(C, heads) || (n3_out && (!g3 || !b3))) return GP_ERR_INVALID;
    gp_switches_reload();
    launch_cross_attn_fold((const h16_t*)y, (h16_t*)y_out, (h16_t*)n3_out, U, u0, G, c0, g3, b3, rows, C, heads, eps, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

void gp_resize_max_res_size(int H0, int W0, int max_edge, int* h, int* w) {
    // image_util.py:95-101: downscale_factor = min(max / W, max / H) in double, new size by int() truncation
    const double f = std::min((double)max_edge / (double)W0, (double)max_edge / (double)H0);
    if (h) *h = (int)((double)H0 * f);
    if (w) *w = (int)((double)W0 * f);
}

gp_status gp_preprocess(const void* rgb_u8, int B, int H0, int W0, void* out_u8, int h, int w, int resample, float* tmp, void* stream) {
    if (!rgb_u8 || !out_u8 || B < 1 || H0 < 1 || W0 < 1 || h < 1 || w < 1 || resample < 0 || resample > 2 || (resample != 1 && !tmp)) return GP_ERR_INVALID;
    launch_resize(rgb_u8, out_u8, tmp, (long long)B * 3, H0, W0, h, w, resample, 1, 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_preprocess_f32(const float* rgb, int B, int C, int H0, int W0, float* out, int h, int w, int resample, int normalize, float* tmp, void* stream) {
    if (!rgb || !out || B < 1 || C < 1 || H0 < 1 || W0 < 1 || h < 1 || w < 1 || resample < 0 || resample > 2) return GP_ERR_INVALID;
    const bool same = h == H0 && w == W0;
    if (!same && resample != 1 && !tmp) return GP_ERR_INVALID;
    if (same && !normalize && rgb != out) return GP_ERR_INVALID;  // nothing to do but a copy: the caller keeps its tensor
    hipStream_t s = (hipStream_t)stream;
    if (!same) launch_resize(rgb, out, tmp, (long long)B * C, H0, W0, h, w, resample, 0, 0, s);
    if (normalize) launch_normalize_rgb(same ? rgb : out, out, (long long)B * C * h * w, s);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_postprocess(const float* pred, int B, int C, int h, int w, float* pred_out, int Ho, int Wo, int resample, float* tmp,
                         const unsigned char* lut_dev, void* colored_out, void* q_out, int q_bits, void* stream) {
    if (!pred || !pred_out || B < 1 || C < 1 || h < 1 || w < 1 || Ho < 1 || Wo < 1 || resample < 0 || resample > 2) return GP_ERR_INVALID;
    if (colored_out && (!lut_dev || C != 1)) return GP_ERR_INVALID;
    if (q_out && q_bits != 16 && q_bits != 8) return GP_ERR_INVALID;
    const bool same = h == Ho && w == Wo;
    if (!same && resample != 1 && !tmp) return GP_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)B * C * Ho * Wo;
    if (same) launch_clip01(pred, pred_out, n, s);
    else launch_resize(pred, pred_out, tmp, (long long)B * C, h, w, Ho, Wo, resample, 0, 1, s);
    if (colored_out) launch_colorize_lut(pred_out, lut_dev, (unsigned char*)colored_out, n, s);
    if (q_out) launch_quantize(pred_out, q_out, n, q_bits, s);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

double gp_mfma_peak_tflops(int device, void* stream) {
    if (hipSetDevice(device) != hipSuccess) return -1.0;
    return mfma_peak_tflops(20, (hipStream_t)stream);
}
double gp_mfma_peak_tflops_shape(int device, int shape, void* stream) {
    if (hipSetDevice(device) != hipSuccess || (shape != 0 && shape != 1)) return -1.0;
    return mfma_peak_tflops(20, (hipStream_t)stream, shape);
}

double gp_mfma_lds_probe(int device, int reads_per_16_mfma, int waves_per_simd, int mode, void* stream) {
    if (hipSetDevice(device) != hipSuccess) return -1.0;
    return mfma_lds_probe_tflops(reads_per_16_mfma, waves_per_simd, mode, (hipStream_t)stream);
}

gp_status gp_softmax_rows(const float* in, void* out, int rows, int T, int ld, float scale, void* stream) {
    if (!in || !out || ld < T) return GP_ERR_INVALID;
    launch_softmax_rows(in, (h16_t*)out, rows, T, ld, scale, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_softmax_rows_f16(const void* in_f16, void* out, int rows, int T, int ld, float scale, void* stream) {
    if (!in_f16 || !out || ld < T || !softmax_rows_f16_supported(ld) || scale <= 0.f) return GP_ERR_INVALID;
    launch_softmax_rows_f16(in_f16, (h16_t*)out, rows, T, ld, scale, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

gp_status gp_bilinear(const void* in, void* out, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream) {
    if (!in || !out || (C % 8)) return GP_ERR_INVALID;
    launch_bilinear((const h16_t*)in, (h16_t*)out, B, Hi, Wi, Ho, Wo, C, align_corners, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP;
}

// ---- the elementwise / layout kernels between the matrix products (elementwise.hip), and with contract != 0 their fp32 forms (the same templates
// over float; contract.hip for the split outputs; bf16 library only).  Everything a kernel would fault on is refused here, before any HIP call. -----
#define GP_LAUNCHED() (hipGetLastError() == hipSuccess ? GP_OK : GP_ERR_HIP)
static bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

gp_status gp_rgb_prologue(const void* rgb, int is_u8, void* out, int B, int H, int W, int Cpad, int contract, void* stream) {
    if (!rgb || !out || B < 1 || H < 1 || W < 1 || !al16(out) || (!is_u8 && ((uintptr_t)rgb & 3))) return GP_ERR_INVALID;
    if (contract) {
        if (GP_F16 || Cpad != 64) return GP_ERR_INVALID;  // (c_rgb_split_kernel writes 64 logical channels: 192 elements per pixel)
        launch_c_rgb_split(rgb, is_u8, (h16_t*)out, B, H, W, (hipStream_t)stream);
    } else {
        if (Cpad < 8 || (Cpad % 8)) return GP_ERR_INVALID;
        launch_rgb_prologue(rgb, is_u8, (h16_t*)out, B, H, W, Cpad, (hipStream_t)stream);
    }
    return GP_LAUNCHED();
}

gp_status gp_concat(const void* a, int Ca, const void* b, int Cb, void* out, long long pixels, int contract, void* stream) {
    const int v = contract ? 4 : 8;
    if ((contract && GP_F16) || !a || !b || !out || pixels < 1 || Ca < v || Cb < v || (Ca % v) || (Cb % v) || !al16(a) || !al16(b) || !al16(out))
        return GP_ERR_INVALID;
    if (contract) launch_concat((const float*)a, Ca, (const float*)b, Cb, (float*)out, pixels, (hipStream_t)stream);
    else launch_concat((const h16_t*)a, Ca, (const h16_t*)b, Cb, (h16_t*)out, pixels, (hipStream_t)stream);
    return GP_LAUNCHED();
}

int gp_concat_stats_bm(long long hw, long long pixels, int channels) { return (hw < 1 || pixels < 1 || channels < 8) ? 0 : concat_stats_bm(hw, pixels, channels); }

gp_status gp_concat_stats(const void* a, int Ca, const void* b, int Cb, void* out, int B, int HW, int bm, int* bm_used, const float* gamma, const float* beta,
                          int groups, float eps, float* scale_out, float* shift_out, void* stream) {
    if (!a || !b || !out || B < 1 || HW < 1 || Ca < 8 || Cb < 8 || (Ca % 8) || (Cb % 8) || !al16(a) || !al16(b) || !al16(out) || bm < 0) return GP_ERR_INVALID;
    const int C = Ca + Cb;
    if (gamma && (!beta || !scale_out || !shift_out || groups < 1 || (C % groups))) return GP_ERR_INVALID;
    const long long pixels = (long long)B * HW;
    if (!bm) bm = concat_stats_bm(HW, pixels, C);
    if (bm < 1 || (HW % bm)) return GP_ERR_INVALID;  // (a statistics tile never spans two images)
    if (bm_used) *bm_used = bm;
    return kernel_entry([&]() -> gp_status {
        float* part = scratch_floats(1, (size_t)(pixels / bm) * C * 2);
        launch_concat_stats((const h16_t*)a, Ca, (const h16_t*)b, Cb, (h16_t*)out, pixels, bm, part, (hipStream_t)stream);
        if (gamma)  // the engine's consumer (gp_engine::gn_scale_shift with the Act::st_mode gp_engine::concat sets)
            launch_groupnorm_from_partials(part, CONCAT_STATS_MODE, bm, B, HW, 1, C, groups, eps, gamma, beta, scale_out, shift_out, (hipStream_t)stream);
        return GP_OK;
    });
}

gp_status gp_rgb_conv_in_stats(const void* rgb, int is_u8, const void* w_packed, const float* bias, void* out, int B, int H, int W, int Cout, const float* gamma,
                               const float* beta, int groups, float eps, float* scale_out, float* shift_out, void* stream) {
    if (!rgb || !w_packed || !out || B < 1 || H < 1 || W < 1 || Cout < 32 || (Cout % 32) || !gamma || !beta || !scale_out || !shift_out || groups < 1 ||
        (Cout % groups) || !al16(w_packed) || !al16(out) || (!is_u8 && ((uintptr_t)rgb & 3)))
        return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        const int J = rgb_conv_in_rows(B, H, W);
        float* st = scratch_floats(1, (size_t)B * J * (2 * Cout + 1));
        h16_t* w27 = nullptr;
        HIPCHK(hipMalloc((void**)&w27, (size_t)Cout * 32 * sizeof(h16_t)));
        launch_pack_k27((const h16_t*)w_packed, 9 * 64, Cout, w27, (hipStream_t)stream);
        launch_rgb_conv_in(rgb, is_u8, w27, bias, (h16_t*)out, st, B, H, W, Cout, (hipStream_t)stream);
        launch_groupnorm_from_partials(st, RGB_CONV_IN_STATS_MODE, J, B, H, W, Cout, groups, eps, gamma, beta, scale_out, shift_out, (hipStream_t)stream);
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        (void)hipFree(w27);
        return e == hipSuccess ? GP_OK : GP_ERR_HIP;
    });
}

gp_status gp_nchw_to_nhwc(const float* in, void* out, int B, int C, int H, int W, int Cpad, int contract, void* stream) {
    if ((contract && GP_F16) || !in || !out || B < 1 || C < 1 || H < 1 || W < 1 || Cpad < C) return GP_ERR_INVALID;
    if (contract) launch_nchw_f32_to_nhwc(in, (float*)out, B, C, H, W, Cpad, (hipStream_t)stream);
    else launch_nchw_f32_to_nhwc(in, (h16_t*)out, B, C, H, W, Cpad, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_nhwc_to_nchw(const void* in, float* out, int B, int C, int H, int W, int ld, int contract, void* stream) {
    if ((contract && GP_F16) || !in || !out || B < 1 || C < 1 || H < 1 || W < 1 || ld < C) return GP_ERR_INVALID;
    if (contract) launch_nhwc_to_nchw_f32((const float*)in, out, B, C, H, W, ld, (hipStream_t)stream);
    else launch_nhwc_to_nchw_f32((const h16_t*)in, out, B, C, H, W, ld, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_ddim_init(const float* noise_nchw, void* lat, float* sample, int B, int H, int W, int L, int ld, int off, int contract, void* stream) {
    if ((contract && GP_F16) || !lat || !sample || B < 1 || H < 1 || W < 1 || L < 1 || off < 0 || (long long)off + L > ld) return GP_ERR_INVALID;
    if (contract) launch_ddim_init(noise_nchw, (float*)lat, sample, B, H, W, L, ld, off, (hipStream_t)stream);
    else launch_ddim_init(noise_nchw, (h16_t*)lat, sample, B, H, W, L, ld, off, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_ddim_update(const void* model, int ldm, float* sample, void* uin, int ldu, int off, void* x0_out, int ldx, long long pixels, int L,
                         const float* coef7_host, int contract, void* stream) {
    if ((contract && GP_F16) || !model || !sample || !uin || !coef7_host || pixels < 1 || L < 1 || ldm < L || off < 0 || (long long)off + L > ldu ||
        (x0_out && ldx < L))
        return GP_ERR_INVALID;
    const DdimCoef k{coef7_host[0], coef7_host[1], coef7_host[2], coef7_host[3], coef7_host[4], coef7_host[5], coef7_host[6]};
    if (contract) launch_ddim_step((const float*)model, ldm, sample, (float*)uin, ldu, off, (float*)x0_out, ldx, pixels, L, k, (hipStream_t)stream);
    else launch_ddim_step((const h16_t*)model, ldm, sample, (h16_t*)uin, ldu, off, (h16_t*)x0_out, ldx, pixels, L, k, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_decode_epilogue(const void* in, float* out, int B, int H, int W, int ld, int mean3, int raw, int contract, void* stream) {
    if ((contract && GP_F16) || !in || !out || B < 1 || H < 1 || W < 1 || ld < 3) return GP_ERR_INVALID;
    if (contract) {
        launch_decode_epilogue((const float*)in, out, B, H, W, ld, mean3, raw, (hipStream_t)stream);
    } else {
        if ((ld % 4) || !al8(in)) return GP_ERR_INVALID;  // (decode_epilogue_kernel reads a pixel's three channels as one uint2)
        launch_decode_epilogue((const h16_t*)in, out, B, H, W, ld, mean3, raw, (hipStream_t)stream);
    }
    return GP_LAUNCHED();
}

gp_status gp_scale_pad(const void* in, void* out, long long pixels, int C, int ldi, int ldo, float scale, void* stream) {
    if (!in || !out || pixels < 1 || C < 1 || ldi < C || ldo < C) return GP_ERR_INVALID;
    launch_scale_pad((const h16_t*)in, (h16_t*)out, pixels, C, ldi, ldo, scale, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_pointwise_small(const void* in, void* out, const float* w, const float* bias, long long pixels, int Cin, int Cout, int ldi, int ldo, float in_scale,
                             int contract, void* stream) {
    if ((contract && GP_F16) || !in || !out || !w || pixels < 1 || Cin < 1 || Cin > 8 || Cout < 1 || Cout > 8 || ldi < Cin || ldo < Cout) return GP_ERR_INVALID;
    if (contract) launch_pointwise_small((const float*)in, (float*)out, w, bias, pixels, Cin, Cout, ldi, ldo, in_scale, (hipStream_t)stream);
    else launch_pointwise_small((const h16_t*)in, (h16_t*)out, w, bias, pixels, Cin, Cout, ldi, ldo, in_scale, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_relu(const void* in, void* out, long long n, void* stream) {
    if (!in || !out || n < 8 || (n % 8) || !al16(in) || !al16(out)) return GP_ERR_INVALID;
    launch_relu((const h16_t*)in, (h16_t*)out, n, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_add(const void* a, const void* b, void* out, long long n, int contract, void* stream) {
    const int v = contract ? 4 : 8;
    if ((contract && GP_F16) || !a || !b || !out || n < v || (n % v) || !al16(a) || !al16(b) || !al16(out)) return GP_ERR_INVALID;
    if (contract) launch_add((const float*)a, (const float*)b, (float*)out, n, (hipStream_t)stream);
    else launch_add((const h16_t*)a, (const h16_t*)b, (h16_t*)out, n, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_dpt_final(const void* in, const float* w, float bias, float* out, int B, int HW, int Cin, int contract, void* stream) {
    const int v = contract ? 4 : 8;
    if ((contract && GP_F16) || !in || !w || !out || B < 1 || HW < 1 || Cin < v || (Cin % v) || !al16(in)) return GP_ERR_INVALID;
    if (contract) launch_dpt_final((const float*)in, w, bias, out, B, HW, Cin, (hipStream_t)stream);
    else launch_dpt_final((const h16_t*)in, w, bias, out, B, HW, Cin, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_minmax_norm(float* x, int B, long long n, void* stream) {
    if (!x || B < 1 || B > 65535 || n < 1) return GP_ERR_INVALID;
    return kernel_entry([&]() -> gp_status {
        launch_minmax_norm(x, B, n, scratch_floats(1, (size_t)B * 64 * 2), (hipStream_t)stream);  // (64 partial {min, max} per image)
        return GP_OK;
    });
}

// ---- contract-only glue (contract.hip) -----------------------------------------------------------------------------------------------------------
gp_status gp_c_heads_split(const float* qkv, int ld, void* Qs, void* Ks, void* Vts, int B, int T, int Tpad, int heads, int hd, void* stream) {
    if (GP_F16 || !qkv || !Qs || !Ks || !Vts || B < 1 || T < 1 || heads < 1 || hd < 64 || (hd % 64) || (Tpad % 64) || Tpad < T || (long long)B * heads > 65535 ||
        ld < 3 * heads * hd || (ld % 4) || !al16(qkv) || !al16(Qs) || !al16(Ks) || !al16(Vts))
        return GP_ERR_INVALID;
    launch_c_heads_split(qkv, ld, (h16_t*)Qs, (h16_t*)Ks, (h16_t*)Vts, B, T, Tpad, heads, hd, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_c_heads_merge_split(const float* O, void* out, int B, int T, int heads, int hd, void* stream) {
    if (GP_F16 || !O || !out || B < 1 || T < 1 || heads < 1 || hd < 8 || (hd % 8) || !al16(O) || !al16(out)) return GP_ERR_INVALID;
    launch_c_heads_merge_split(O, (h16_t*)out, B, T, heads, hd, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_c_cross_fold(const float* y, float* y_out, void* n3_out, const float* U, const float* u0, const float* G, const float* c0, const float* g3,
                          const float* b3, int rows, int C, int heads, float eps, void* stream) {
    if (GP_F16 || !y || !y_out || !U || !u0 || !G || !c0 || rows < 1 || C < 8 || !c_cross_fold_supported(C) || heads < 1 || (n3_out && (!g3 || !b3)) ||
        !al16(y) || !al16(y_out) || !al16(n3_out) || !al16(U) || !al16(G) || !al16(c0) || !al16(g3) || !al16(b3))
        return GP_ERR_INVALID;
    launch_c_cross_fold(y, y_out, (h16_t*)n3_out, U, u0, G, c0, g3, b3, rows, C, heads, eps, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_c_cross_attention(const float* q, const float* kc, const float* vc, void* out, int rows, int C, int L, void* stream) {
    if (GP_F16 || !q || !kc || !vc || !out || rows < 1 || C < 64 || (C % 64) || L < 1 || !al16(q) || !al16(out)) return GP_ERR_INVALID;
    launch_c_cross_attn_small(q, kc, vc, (h16_t*)out, rows, C, L, (hipStream_t)stream);
    return GP_LAUNCHED();
}

gp_status gp_c_bilinear(const float* in, float* out, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream) {
    if (GP_F16 || !in || !out || B < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || C < 4 || (C % 4) || !al16(in) || !al16(out)) return GP_ERR_INVALID;
    launch_bilinear(in, out, B, Hi, Wi, Ho, Wo, C, align_corners, (hipStream_t)stream);
    return GP_LAUNCHED();
}

}  // extern "C"
