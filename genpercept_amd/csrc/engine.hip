// Engine: weight ingestion / constant folding / bf16 packing, activation pool, and the static forward schedules of
// the SD2.1 VAE encoder, UNet single step (t fixed, context fixed), VAE decoder and DPT head, all enqueued on one
// HIP stream.  Exposed through the gp_engine* part of the C-ABI of include/genpercept_hip.h (the stateless per-kernel entry points are
// kernel_abi.hip); every conv / GEMM launch is filled by a builder of igemm_problem.h, the same one the matching entry point calls.
//
// Both precisions run ONE set of layer ops and schedules.  An `Act` is either a 16-bit tensor / split operand (`p`) or a stored fp32 tensor (`f`);
// new_stored / new_product_input allocate the form the precision uses, conv / linear pick `.p` or `.f` of their input, residual and in-place target,
// and each glue kernel's 16-bit or fp32 form is chosen in one small op.  Only attention_c, the split-operand attention, has no 16-bit twin.
//
// Lifetime: every activation and scratch buffer is a Pool::Buf (pool.h), a move-only owner that hands its buffer back to the pool when it ends; an
// `Act` owns its tensor and its statistics partials, and whatever only reads one takes `const Act&`.  The pool recycles a buffer as soon as it is
// back, so WHERE an owner ends relative to the allocations around it sets the pool's high-water mark: the schedules end an owner early with
// reset() or a nested block, and write `h = f(h)` for a layer that replaces its input (f(h) is evaluated first, then the old h released).
// A stage that throws returns its buffers by unwinding; every entry point ends with nothing outstanding (finish_call checks it).
//
// Control flow mirrors (never copies) the reference: genpercept/genpercept_pipeline.py:399-526 (single_infer,
// encode_rgb, decode_pred), genpercept/models/custom_unet.py:109-119,146-170,273,305-415 (UNet forward, skip order,
// upsample_size, multi_level_feats), genpercept/models/dpt_head.py:213-335,443-582 (DPT neck/head); module internals
// follow the public SD2.1 architecture.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <mutex>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/genpercept_hip.h"
#include "host_pack.h"
#include "igemm_problem.h"
#include "pool.h"

namespace {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// the pool's device allocator (pool.h takes it as two function pointers)
void* device_alloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    return p;
}
void device_free(void* p) { (void)hipFree(p); }

// An activation: move-only owner of its tensor and of the statistics partials that go with it; both go back to the pool when it ends or at reset().
struct Act {
    Pool::Buf mem;      // the tensor: 16-bit (p) or fp32 (f)
    bool fp32 = false;
    int B = 0, H = 0, W = 0, C = 0;  // C = allocated channels (row stride)
    // GroupNorm partial statistics written by the producing conv's epilogue ([pixel tile][C][2] fp32)
    Pool::Buf stats;
    int st_mode = 0, st_bm = 0;
    // contract precision (contract.hip): a STORED tensor is fp32 (`f`, C channels per pixel); a matrix-product operand is a split tensor (`p`, with
    // C = 3 x the logical width: [hi | lo | hi] blocks).  Exactly one of p / f is set; neither in an empty Act.
    h16_t* p() const { return fp32 ? nullptr : mem.get<h16_t>(); }
    float* f() const { return fp32 ? mem.get<float>() : nullptr; }
    void* data() const { return mem.get<void>(); }
    float* st() const { return stats.get<float>(); }
    long long pixels() const { return (long long)B * H * W; }
    void reset() { mem.reset(); stats.reset(); }
};

struct NormW {
    float* g = nullptr;
    float* b = nullptr;
    int C = 0;
};
struct ResW {
    NormW n1, n2;
    PackedW c1, c2, sc;
    bool has_sc = false;
    // time-embedding fold (UNet only)
    bool has_temb = false;
    std::vector<float> c1_bias_h, tw_h, tb_h;  // conv1.bias, time_emb_proj.{weight,bias}
    size_t temb_off = 0;                       // where c1.bias lives in the engine's time-embedding bias arena (floats)
};
struct TfW {
    NormW gn, ln1, ln2, ln3;
    PackedW proj_in, qkv, qk, v, o1, q2, o2, ff1, ff2, proj_out;  // qk / v: views of qkv's rows [0, 2C) / [2C, 3C)
    float* kc = nullptr;  // folded cross-attention keys / values [L][C] fp32
    float* vc = nullptr;
    std::vector<float> wk_h, wv_h;  // attn2.to_k / to_v [C][D]
    // two-token context: the whole attn2 branch folded into per-head vectors (norm.hip: cross_fold_kernel); null when L != 2
    float *fU = nullptr, *fu0 = nullptr, *fG = nullptr, *fc0 = nullptr;
    std::vector<float> wq2_h, wo2_h, bo2_h, ln2g_h, ln2b_h;  // attn2.to_q / to_out.0, norm2 (host copies for the fold)
    int C = 0, heads = 0;
};
struct VaeAttnW {
    NormW gn;
    PackedW qk, v, o;
    PackedW qkv;  // contract precision: to_q | to_k | to_v stacked, unscaled (the softmax kernel applies 1 / sqrt(C))
    int C = 0;
};

}  // namespace

struct SatFlags { unsigned* f[16]; int n; };
// one lane per translation unit: a set flag becomes one event of the engine's counter and is cleared for the next call
__global__ void collect_saturation_kernel(SatFlags fl, unsigned* counter) {
    const int i = threadIdx.x;
    if (i < fl.n) {
        const unsigned v = __hip_atomic_load(fl.f[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) {
            __hip_atomic_store(fl.f[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(counter, 1u);
        }
    }
}

struct gp_engine {
    gp_config cfg;
    std::string err;
    std::unordered_map<std::string, HostTensor> host;
    bool finalized = false;
    hipStream_t st = nullptr;
    Pool pool{device_alloc, device_free};
    std::vector<void*> weights_dev;  // everything hipMalloc'ed for weights
    h16_t* zero = nullptr;
    Pool::Buf gn_ws;  // GroupNorm workspace, kept across calls (declared after the pool: it goes back before the pool frees its buffers)
    size_t gn_ws_floats = 0;
    hipStream_t last_stream = nullptr;  // the pool recycles buffers in stream order: a change of stream is fenced (check_ready)
    bool stream_seen = false;
    h16_t* conv_in_w27 = nullptr;  // VAE encoder conv_in as a [Cout][32] (K = 27) matrix for rgb_conv_in_kernel
    bool fuse_gn = true;   // GENPERCEPT_NO_GN_FUSION=1 keeps the separate apply pass (A/B measurements)
    int gn_fuse_max_slices = 1;        // GENPERCEPT_GN_FUSE_MAX_SLICES: on large maps fuse the apply only into convs with at most this many 128-channel output slices
    int gn_fuse_always_below_px = 0;   // GENPERCEPT_GN_FUSE_BELOW_PX: maps with fewer pixels per image fuse whatever the slice count (r1: 16384; r2 in-box
                                       // A/B with the faster apply / one-launch small-map GroupNorm: 0 is 1.3 ms per pass faster)
    bool fuse_stats = true;  // GENPERCEPT_NO_STATS_FUSION=1 keeps the separate statistics pass
    // gp_set_precision(GP_PREC_CONTRACT): fp32 storage + split-bf16 operands (three MFMAs per product over a tripled K), see contract.hip.
    // Weights are packed [n_rows][taps][3 cin_pad] in B order [hi | hi | lo]; every PackedW::cin_pad below is then the TRIPLED width.
    bool contract = false;

    std::unordered_map<std::string, PackedW> convs;
    std::unordered_map<std::string, NormW> norms;
    std::unordered_map<std::string, ResW> resnets;
    std::unordered_map<std::string, TfW> tfs;
    std::unordered_map<std::string, VaeAttnW> vattn;
    std::vector<float> te_w1, te_b1, te_w2, te_b2;  // time_embedding MLP (host)
    std::vector<float> ctx;                          // [L][D]
    int ctx_L = 0, ctx_D = 0;
    float timestep = 1.f;
    int ncu = 256;                        // compute units of the device (persistent launches size their grids by it)
    float* temb_arena = nullptr;          // conv1 biases of all UNet resnets at the current timestep
    size_t temb_total = 0;
    std::map<float, float*> temb_cache;   // timestep -> device copy of the arena's contents
    std::vector<float> pq_w, pq_b;  // post_quant_conv
    float* pq_w_dev = nullptr;
    float* pq_b_dev = nullptr;
    float* dpt_w_dev = nullptr;  // head.head.4 weight [32]
    float dpt_b = 0.f;
    // fp16 build: saturating conversions that clipped (common.h: gp_sat_flag per translation unit), collected at the end of every call
    double flops_halo_exec = 0.0;   // executed (not algorithmic) flops of the halo-conv launches, see gp_halo_executed_flops
    SatFlags sat_flags{};
    unsigned* sat_dev = nullptr;          // [1] events since the last reset
    void collect_saturation() {
        if (sat_dev && sat_flags.n > 0) hipLaunchKernelGGL(collect_saturation_kernel, dim3(1), dim3(64), 0, st, sat_flags, sat_dev);
    }

    // profiling
    int prof = 0;
    gp_timings tm{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<int> ev_kind;
    size_t ev_used = 0;

    // ---------------------------------------------------------------------------------------------------------------
    const HostTensor& H(const std::string& n) const {
        auto it = host.find(n);
        if (it == host.end()) throw std::out_of_range("missing weight: " + n);
        return it->second;
    }
    bool has(const std::string& n) const { return host.find(n) != host.end(); }

    template <typename T>
    T* upload(const T* src, size_t n) {
        T* d = nullptr;
        HIPCHK(hipMalloc((void**)&d, n * sizeof(T) + 256));
        HIPCHK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
        weights_dev.push_back(d);
        return d;
    }

    void pack_phases(PackedW& pw, const std::string& name) {
        const HostTensor& w = H(name + ".weight");
        if (w.shape.size() != 4 || w.shape[2] != 3 || w.shape[3] != 3) throw std::invalid_argument(name + ": not a 3x3 conv");
        const int cout = (int)w.shape[0], cin = (int)w.shape[1];
        std::vector<h16_t> buf((size_t)pw.n_rows * 16 * pw.cin_pad, 0);  // (contract precision: pw.cin_pad is already the tripled width)
        pack_phase_rows(w.v.data(), cout, cin, contract ? pw.cin_pad / 3 : pw.cin_pad, buf, contract);
        pw.w_ph = upload(buf.data(), buf.size());
    }
    PackedW pack(const float* w, const float* bias, int cout, int cin, int ks, int cin_pad, bool geglu = false) {
        PackedW pw;
        pw.cout = cout; pw.cin_pad = contract ? 3 * cin_pad : cin_pad; pw.ks = ks; pw.n_rows = gp_packed_rows(cout);
        std::vector<h16_t> buf((size_t)pw.n_rows * ks * ks * pw.cin_pad, 0);
        pack_rows(w, cout, cin, ks, cin_pad, geglu, buf, 0, pw.n_rows, contract);
        pw.w = upload(buf.data(), buf.size());
        if (bias) {
            std::vector<float> b(bias, bias + cout);
            if (geglu) {
                for (int n = 0; n < cout; ++n) b[geglu_row(n, cout)] = bias[n];
            }
            pw.bias = upload(b.data(), b.size());
        }
        return pw;
    }
    PackedW pack_named(const std::string& name, int ks, int cin_pad_override = 0, bool geglu = false) {
        const HostTensor& w = H(name + ".weight");
        const int cout = (int)w.shape[0], cin = (int)w.shape[1];
        const float* b = has(name + ".bias") ? H(name + ".bias").v.data() : nullptr;
        const int cin_pad = cin_pad_override ? cin_pad_override : round_up(cin, 64);
        return pack(w.v.data(), b, cout, cin, ks, cin_pad, geglu);
    }
    // two linear layers stacked along the output dimension ([Wa; Wb]), optional biases
    // (scale_a multiplies the first layer's weight and bias: the softmax scale of an attention folded into its query projection)
    PackedW pack_stacked(const std::vector<std::string>& names, float scale_first = 1.f) {
        const int cin = (int)(H(names[0] + ".weight").numel() / H(names[0] + ".weight").shape[0]);
        int ctot = 0;
        for (auto& n : names) ctot += (int)H(n + ".weight").shape[0];
        std::vector<float> w((size_t)ctot * cin), bias;
        const bool with_bias = has(names[0] + ".bias");
        if (with_bias) bias.resize(ctot);
        int row = 0;
        for (size_t k = 0; k < names.size(); ++k) {
            const HostTensor& wk = H(names[k] + ".weight");
            const int ck = (int)wk.shape[0];
            if ((int)(wk.numel() / ck) != cin) throw std::invalid_argument("stacked projections must share their input width");
            memcpy(w.data() + (size_t)row * cin, wk.v.data(), (size_t)ck * cin * 4);
            if (with_bias) memcpy(bias.data() + row, H(names[k] + ".bias").v.data(), (size_t)ck * 4);
            if (k == 0 && scale_first != 1.f) {
                for (size_t i = 0; i < (size_t)ck * cin; ++i) w[i] *= scale_first;
                for (int i = 0; i < ck && with_bias; ++i) bias[i] *= scale_first;
            }
            row += ck;
        }
        return pack(w.data(), with_bias ? bias.data() : nullptr, ctot, cin, 1, round_up(cin, 64));
    }
    PackedW pack_stacked(const std::string& a, const std::string& b, float scale_a = 1.f) { return pack_stacked(std::vector<std::string>{a, b}, scale_a); }
    NormW norm_named(const std::string& name) {
        NormW n;
        const HostTensor& g = H(name + ".weight");
        n.C = (int)g.numel();
        n.g = upload(g.v.data(), g.v.size());
        n.b = upload(H(name + ".bias").v.data(), (size_t)n.C);
        return n;
    }

    void build_resnet(const std::string& p, bool temb) {
        ResW r;
        r.n1 = norm_named(p + ".norm1");
        r.n2 = norm_named(p + ".norm2");
        r.c1 = pack_named(p + ".conv1", 3);
        r.c2 = pack_named(p + ".conv2", 3);
        r.has_sc = has(p + ".conv_shortcut.weight");
        if (r.has_sc) r.sc = pack_named(p + ".conv_shortcut", 1);
        if (temb) {
            r.has_temb = true;
            r.c1_bias_h = H(p + ".conv1.bias").v;
            r.tw_h = H(p + ".time_emb_proj.weight").v;
            r.tb_h = H(p + ".time_emb_proj.bias").v;
        }
        resnets[p] = std::move(r);
    }
    void build_transformer(const std::string& p, int heads) {
        TfW t;
        const std::string b = p + ".transformer_blocks.0";
        t.gn = norm_named(p + ".norm");
        t.proj_in = pack_named(p + ".proj_in", 1);
        t.C = t.proj_in.cout;
        t.heads = heads;
        if (t.C != heads * 64) throw std::invalid_argument("self-attention head_dim must be 64 (" + p + ")");
        t.ln1 = norm_named(b + ".norm1");
        t.ln2 = norm_named(b + ".norm2");
        t.ln3 = norm_named(b + ".norm3");
        // to_q | to_k | to_v stacked along the output dimension: ONE projection launch writes q | k row-major and V transposed (pgemm.hip:
        // IGemmParams::vt_out); the two-launch form (q | k GEMM + transposed V GEMM) reads the same buffer through row views
        t.qkv = pack_stacked({b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"});
        t.qk = t.qkv; t.qk.cout = 2 * t.C;
        t.v = t.qkv; t.v.cout = t.C; t.v.w = t.qkv.w + (size_t)2 * t.C * t.qkv.cin_pad; t.v.n_rows = t.qkv.n_rows - 2 * t.C;
        if (t.qkv.bias) { t.v.bias = t.qkv.bias + 2 * t.C; }
        t.o1 = pack_named(b + ".attn1.to_out.0", 1);
        t.q2 = pack_named(b + ".attn2.to_q", 1);
        t.o2 = pack_named(b + ".attn2.to_out.0", 1);
        t.ff1 = pack_named(b + ".ff.net.0.proj", 1, 0, true);
        t.ff2 = pack_named(b + ".ff.net.2", 1);
        t.proj_out = pack_named(p + ".proj_out", 1);
        t.wk_h = H(b + ".attn2.to_k.weight").v;
        t.wv_h = H(b + ".attn2.to_v.weight").v;
        t.wq2_h = H(b + ".attn2.to_q.weight").v;
        t.wo2_h = H(b + ".attn2.to_out.0.weight").v;
        t.bo2_h = H(b + ".attn2.to_out.0.bias").v;
        t.ln2g_h = H(b + ".norm2.weight").v;
        t.ln2b_h = H(b + ".norm2.bias").v;
        tfs[p] = std::move(t);
    }
    void build_vae_attn(const std::string& p) {
        VaeAttnW a;
        const bool newn = has(p + ".to_q.weight");
        const std::string q = p + (newn ? ".to_q" : ".query"), k = p + (newn ? ".to_k" : ".key"), v = p + (newn ? ".to_v" : ".value"),
                          o = p + (newn ? ".to_out.0" : ".proj_attn");
        a.gn = norm_named(p + ".group_norm");
        a.C = a.gn.C;
        // softmax(q k^T / sqrt(C)): the scale goes into the query projection, so the logits the score GEMM writes are the SCALED ones
        // (what diffusers keeps in fp16 too); raw 512-term dot products of a real checkpoint can pass fp16's 65504
        if (contract) a.qkv = pack_stacked(std::vector<std::string>{q, k, v});
        else {
            a.qk = pack_stacked(q, k, 1.0f / std::sqrt((float)a.C));
            a.v = pack_named(v, 1);
        }
        a.o = pack_named(o, 1);
        vattn[p] = std::move(a);
    }

    // conv1 bias + time_emb_proj(SiLU(time_embedding(t))) of every UNet resnet at timestep t, concatenated in arena order; computed on
    // the host in double once per distinct t and kept on the device, so a change of timestep is one stream-ordered D2D copy
    // (the multi-step archs walk 10-50 timesteps per image; genpercept_pipeline.py:447-463).
    const float* timestep_biases(float t) {
        // an engine finalised without the UNet's time-embedding weights (a VAE-only engine) has nothing to fold and no arena to copy into
        if (te_w1.empty() || te_b1.empty() || !temb_arena) throw std::out_of_range("missing weight: unet.time_embedding.* (this engine holds no UNet)");
        auto it = temb_cache.find(t);
        if (it != temb_cache.end()) return it->second;
        const int c0 = cfg.unet_block_out[0], te = c0 * 4, half = c0 / 2;
        std::vector<double> temb(c0), e1(te), emb(te);
        for (int i = 0; i < half; ++i) {
            const double f = std::exp(-std::log(10000.0) * i / half);
            temb[i] = std::cos((double)t * f);
            temb[half + i] = std::sin((double)t * f);
        }
        for (int o = 0; o < te; ++o) {
            double a = te_b1[o];
            for (int i = 0; i < c0; ++i) a += (double)te_w1[(size_t)o * c0 + i] * temb[i];
            e1[o] = a / (1.0 + std::exp(-a));
        }
        for (int o = 0; o < te; ++o) {
            double a = te_b2[o];
            for (int i = 0; i < te; ++i) a += (double)te_w2[(size_t)o * te + i] * e1[i];
            emb[o] = a / (1.0 + std::exp(-a));  // SiLU(emb), the input of every time_emb_proj
        }
        std::vector<float> all(temb_total);
        std::vector<const ResW*> rs;
        for (auto& kv : resnets)
            if (kv.second.has_temb) rs.push_back(&kv.second);
        // 26 M multiply-adds in double: spread over a few host threads (a 50-step schedule folds 50 timesteps on its first image)
        const unsigned nthr = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool_thr;
        for (unsigned w = 0; w < nthr; ++w)
            pool_thr.emplace_back([&, w] {
                for (size_t k = w; k < rs.size(); k += nthr) {
                    const ResW& r = *rs[k];
                    for (int o = 0; o < r.c1.cout; ++o) {
                        double a = (double)r.c1_bias_h[o] + r.tb_h[o];
                        const float* wrow = &r.tw_h[(size_t)o * te];
                        for (int i = 0; i < te; ++i) a += (double)wrow[i] * emb[i];
                        all[r.temb_off + o] = (float)a;
                    }
                }
            });
        for (auto& t : pool_thr) t.join();
        float* d = nullptr;
        HIPCHK(hipMalloc((void**)&d, temb_total * sizeof(float)));
        weights_dev.push_back(d);
        HIPCHK(hipMemcpy(d, all.data(), temb_total * sizeof(float), hipMemcpyHostToDevice));
        temb_cache[t] = d;
        return d;
    }
    void fold_timestep() {  // synchronous form (gp_finalize / gp_set_timestep)
        if (te_w1.empty()) return;
        if (!temb_arena) {  // every temb resnet's conv1 bias re-pointed into one arena
            temb_total = 0;
            for (auto& kv : resnets)
                if (kv.second.has_temb) { kv.second.temb_off = temb_total; temb_total += (size_t)((kv.second.c1.cout + 63) / 64) * 64; }
            HIPCHK(hipMalloc((void**)&temb_arena, temb_total * sizeof(float)));
            weights_dev.push_back(temb_arena);
            for (auto& kv : resnets)
                if (kv.second.has_temb) kv.second.c1.bias = temb_arena + kv.second.temb_off;
        }
        HIPCHK(hipMemcpy(temb_arena, timestep_biases(timestep), temb_total * sizeof(float), hipMemcpyDeviceToDevice));
    }
    void set_timestep_on_stream(float t) {  // inside a pass: ordered after the launches that still read the previous biases
        const float* src = timestep_biases(t);
        timestep = t;
        HIPCHK(hipMemcpyAsync(temb_arena, src, temb_total * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    void fold_context() {
        if (ctx.empty()) return;
        for (auto& kv : tfs) {
            TfW& t = kv.second;
            const int C = t.C, D = ctx_D, L = ctx_L;
            if ((int)(t.wk_h.size() / C) != D) throw std::invalid_argument("context dim does not match attn2.to_k");
            std::vector<float> kc((size_t)L * C), vc((size_t)L * C);
            for (int l = 0; l < L; ++l)
                for (int c = 0; c < C; ++c) {
                    double ak = 0, av = 0;
                    for (int d = 0; d < D; ++d) {
                        ak += (double)t.wk_h[(size_t)c * D + d] * ctx[(size_t)l * D + d];
                        av += (double)t.wv_h[(size_t)c * D + d] * ctx[(size_t)l * D + d];
                    }
                    kc[(size_t)l * C + c] = (float)ak;
                    vc[(size_t)l * C + c] = (float)av;
                }
            t.kc = upload(kc.data(), kc.size());
            t.vc = upload(vc.data(), vc.size());
            t.fU = t.fu0 = t.fG = t.fc0 = nullptr;
            if (L == 2 && cross_attn_fold_supported(C, t.heads) && !gp_sw().no_cross_fold) {
                // softmax over two keys = sigmoid of the logit difference; see cross_fold_kernel (norm.hip) for the algebra
                const int hd = 64, nh = t.heads;
                std::vector<float> U((size_t)nh * C), u0(nh), G((size_t)nh * C), c0(C);
                for (int h = 0; h < nh; ++h) {
                    double b0 = 0;
                    for (int c = 0; c < C; ++c) {
                        double a = 0;
                        for (int j = h * hd; j < (h + 1) * hd; ++j) a += (double)t.wq2_h[(size_t)j * C + c] * ((double)kc[j] - (double)kc[(size_t)C + j]);
                        a *= 0.125;  // 1 / sqrt(head_dim)
                        U[(size_t)h * C + c] = (float)(a * t.ln2g_h[c]);
                        b0 += a * t.ln2b_h[c];
                    }
                    u0[h] = (float)b0;
                }
                for (int c = 0; c < C; ++c) {
                    double a = t.bo2_h[c];
                    for (int j = 0; j < C; ++j) a += (double)t.wo2_h[(size_t)c * C + j] * vc[(size_t)C + j];
                    c0[c] = (float)a;
                    for (int h = 0; h < nh; ++h) {
                        double g = 0;
                        for (int j = h * hd; j < (h + 1) * hd; ++j) g += (double)t.wo2_h[(size_t)c * C + j] * ((double)vc[j] - (double)vc[(size_t)C + j]);
                        G[(size_t)h * C + c] = (float)g;
                    }
                }
                t.fU = upload(U.data(), U.size());
                t.fu0 = upload(u0.data(), u0.size());
                t.fG = upload(G.data(), G.size());
                t.fc0 = upload(c0.data(), c0.size());
            }
        }
    }

    void finalize() {
        if (finalized) throw std::logic_error("gp_finalize called twice");
        HIPCHK(hipSetDevice(cfg.device));
        gp_switches_reload();  // the A/B switches of this process as of now (never read again on the launch path)
        fuse_gn = !gp_sw().no_gn_fusion;
        if (gp_sw().gn_fuse_max_slices >= 0) gn_fuse_max_slices = gp_sw().gn_fuse_max_slices;
        if (gp_sw().gn_fuse_below_px >= 0) gn_fuse_always_below_px = gp_sw().gn_fuse_below_px;
        fuse_stats = !gp_sw().no_stats_fusion;
        {
            std::vector<h16_t> z(2048, 0);
            zero = upload(z.data(), z.size());
        }
        const bool have_unet = has("unet.conv_in.weight");
        // ---------------- VAE ----------------
        if (has("vae.encoder.conv_in.weight")) {
            convs["vae.encoder.conv_in"] = pack_named("vae.encoder.conv_in", 3);
            for (int i = 0; i < 4; ++i) {
                for (int j = 0; j < cfg.vae_layers_per_block; ++j) build_resnet("vae.encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), false);
                if (i != 3) convs["vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv"] = pack_named("vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", 3);
            }
            build_resnet("vae.encoder.mid_block.resnets.0", false);
            build_vae_attn("vae.encoder.mid_block.attentions.0");
            build_resnet("vae.encoder.mid_block.resnets.1", false);
            norms["vae.encoder.conv_norm_out"] = norm_named("vae.encoder.conv_norm_out");
            // fold quant_conv (1x1) into encoder.conv_out and keep only the mean half, times scaling_factor
            const HostTensor& wc = H("vae.encoder.conv_out.weight");
            const HostTensor& bc = H("vae.encoder.conv_out.bias");
            const HostTensor& wq = H("vae.quant_conv.weight");
            const HostTensor& bq = H("vae.quant_conv.bias");
            const int L = cfg.vae_latent_channels, M2 = 2 * L, cin = (int)wc.shape[1];
            std::vector<float> wf((size_t)L * cin * 9), bf(L);
            for (int o = 0; o < L; ++o) {
                double bb = bq.v[o];
                for (int m = 0; m < M2; ++m) bb += (double)wq.v[(size_t)o * M2 + m] * bc.v[m];
                bf[o] = (float)(bb * cfg.vae_scaling_factor);
                for (size_t e = 0; e < (size_t)cin * 9; ++e) {
                    double a = 0;
                    for (int m = 0; m < M2; ++m) a += (double)wq.v[(size_t)o * M2 + m] * wc.v[(size_t)m * cin * 9 + e];
                    wf[(size_t)o * cin * 9 + e] = (float)(a * cfg.vae_scaling_factor);
                }
            }
            convs["vae.encoder.conv_out_folded"] = pack(wf.data(), bf.data(), L, cin, 3, round_up(cin, 64));
        }
        if (has("vae.decoder.conv_in.weight")) {
            pq_w = H("vae.post_quant_conv.weight").v;
            pq_b = H("vae.post_quant_conv.bias").v;
            pq_w_dev = upload(pq_w.data(), pq_w.size());
            pq_b_dev = upload(pq_b.data(), pq_b.size());
            convs["vae.decoder.conv_in"] = pack_named("vae.decoder.conv_in", 3);
            build_resnet("vae.decoder.mid_block.resnets.0", false);
            build_vae_attn("vae.decoder.mid_block.attentions.0");
            build_resnet("vae.decoder.mid_block.resnets.1", false);
            for (int i = 0; i < 4; ++i) {
                for (int j = 0; j < cfg.vae_layers_per_block + 1; ++j) build_resnet("vae.decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), false);
                if (i != 3) {
                    const std::string un = "vae.decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
                    convs[un] = pack_named(un, 3);
                    pack_phases(convs[un], un);
                }
            }
            norms["vae.decoder.conv_norm_out"] = norm_named("vae.decoder.conv_norm_out");
            convs["vae.decoder.conv_out"] = pack_named("vae.decoder.conv_out", 3);
        }
        // ---------------- UNet ----------------
        if (have_unet) {
            te_w1 = H("unet.time_embedding.linear_1.weight").v;
            te_b1 = H("unet.time_embedding.linear_1.bias").v;
            te_w2 = H("unet.time_embedding.linear_2.weight").v;
            te_b2 = H("unet.time_embedding.linear_2.bias").v;
            convs["unet.conv_in"] = pack_named("unet.conv_in", 3);
            for (int i = 0; i < 4; ++i) {
                const std::string bp = "unet.down_blocks." + std::to_string(i);
                for (int j = 0; j < cfg.unet_layers_per_block; ++j) {
                    build_resnet(bp + ".resnets." + std::to_string(j), true);
                    if (cfg.unet_down_attn[i]) build_transformer(bp + ".attentions." + std::to_string(j), cfg.unet_num_heads[i]);
                }
                if (i != 3) convs[bp + ".downsamplers.0.conv"] = pack_named(bp + ".downsamplers.0.conv", 3);
            }
            build_resnet("unet.mid_block.resnets.0", true);
            build_transformer("unet.mid_block.attentions.0", cfg.unet_num_heads[3]);
            build_resnet("unet.mid_block.resnets.1", true);
            for (int i = 0; i < 4; ++i) {
                const std::string bp = "unet.up_blocks." + std::to_string(i);
                const bool attn = cfg.unet_down_attn[3 - i];
                for (int j = 0; j < cfg.unet_layers_per_block + 1; ++j) {
                    build_resnet(bp + ".resnets." + std::to_string(j), true);
                    if (attn) build_transformer(bp + ".attentions." + std::to_string(j), cfg.unet_num_heads[3 - i]);
                }
                if (i != 3) {
                    convs[bp + ".upsamplers.0.conv"] = pack_named(bp + ".upsamplers.0.conv", 3);
                    pack_phases(convs[bp + ".upsamplers.0.conv"], bp + ".upsamplers.0.conv");
                }
            }
            if (cfg.unet_has_out) {
                norms["unet.conv_norm_out"] = norm_named("unet.conv_norm_out");
                convs["unet.conv_out"] = pack_named("unet.conv_out", 3);
            }
            fold_timestep();
            fold_context();
        }
        // ---------------- DPT head ----------------
        if (cfg.dpt_enabled && has("dpt.neck.convs.0.weight")) {
            convs["dpt.feature_upsample_0.conv"] = pack_named("dpt.feature_upsample_0.conv", 3);
            pack_phases(convs["dpt.feature_upsample_0.conv"], "dpt.feature_upsample_0.conv");  // (x2 nearest + 3x3: four phase convolutions, conv_halo.hip PH)
            for (int i = 0; i < 4; ++i) {
                convs["dpt.neck.convs." + std::to_string(i)] = pack_named("dpt.neck.convs." + std::to_string(i), 3);
                const std::string lp = "dpt.neck.fusion_stage.layers." + std::to_string(i);
                convs[lp + ".projection"] = pack_named(lp + ".projection", 1);
                if (i != 0) {
                    convs[lp + ".residual_layer1.convolution1"] = pack_named(lp + ".residual_layer1.convolution1", 3);
                    convs[lp + ".residual_layer1.convolution2"] = pack_named(lp + ".residual_layer1.convolution2", 3);
                }
                convs[lp + ".residual_layer2.convolution1"] = pack_named(lp + ".residual_layer2.convolution1", 3);
                convs[lp + ".residual_layer2.convolution2"] = pack_named(lp + ".residual_layer2.convolution2", 3);
            }
            convs["dpt.head.projection"] = pack_named("dpt.head.projection", 3);
            convs["dpt.head.head.0"] = pack_named("dpt.head.head.0", 3);
            convs["dpt.head.head.2"] = pack_named("dpt.head.head.2", 3);
            const HostTensor& w4 = H("dpt.head.head.4.weight");
            dpt_w_dev = upload(w4.v.data(), w4.v.size());
            dpt_b = H("dpt.head.head.4.bias").v[0];
        }
        host.clear();
        finalized = true;
    }

    // ---------------------------------------------------------------------------------------------------------------
    // run-time helpers (everything below only enqueues work on `st`)
    Act new_act(int B, int H, int W, int C) {
        Act a;
        a.B = B; a.H = H; a.W = W; a.C = C;
        a.mem = pool.alloc((size_t)B * H * W * C * sizeof(h16_t));
        return a;
    }
    // ---- contract precision: stored tensors (fp32) and split operands -----------------------------------------------------------------
    Act new_act_f(int B, int H, int W, int C) {
        Act a;
        a.B = B; a.H = H; a.W = W; a.C = C;
        a.fp32 = true;
        a.mem = pool.alloc((size_t)B * H * W * C * sizeof(float));
        return a;
    }
    Act new_operand(int B, int H, int W, int C_logical) { return new_act(B, H, W, 3 * C_logical); }
    // ---- the two allocation verbs of the layer ops and stages -----------------------------------------------------------------------------
    // a tensor this precision STORES: 16-bit `p`, or fp32 `f` in contract precision
    Act new_stored(int B, int H, int W, int C) {
        if (contract) return new_act_f(B, H, W, C);
        return new_act(B, H, W, C);
    }
    // the input of a matrix product over C channels: 16-bit `p` of width C, or the split operand of width 3 C
    Act new_product_input(int B, int H, int W, int C) {
        if (contract) return new_operand(B, H, W, C);
        return new_act(B, H, W, C);
    }
    // A-order split of a stored tensor (optionally through ReLU): the operand form a conv / linear layer reads
    Act split_operand(const Act& x, int act = GP_ACT_NONE) {
        if (!x.f()) throw std::logic_error("split_operand: not a stored fp32 tensor");
        Act y = new_operand(x.B, x.H, x.W, x.C);
        mark("split3 " + dims(x));
        launch_c_split3(x.f(), x.C, y.p(), x.pixels(), x.C, 0, act, 1.0f, st);
        return y;
    }
    // ask the kernel that is about to write `y` to leave per-tile channel statistics behind (next GroupNorm skips its read pass)
    // (not in contract precision: the epilogues' single-pass {sum, sum of squares} partials would lose eps * (mean / std)^2 of a group's variance
    // on fp32 data, igemm_tile_info refuses fp32 rows; the GroupNorm re-reads the tensor instead, contract.hip: c_gn_stats_kernel)
    void attach_stats(Act& y, IGemmParams& p) {
        if (!fuse_stats || contract) return;
        int mode = 0, bm = 0;
        const int nt = igemm_tile_info(p, 0, &mode, &bm);
        if (nt <= 0) return;
        y.stats = pool.alloc((size_t)nt * (p.N * 2 + 1) * sizeof(float));
        y.st_mode = mode;
        y.st_bm = bm;
        p.stats_out = y.st();
    }
    // profiling level 3: one event before every launch; a launch's cost is the time to the next mark (kernel + the gap behind it)
    struct Mark { hipEvent_t ev; std::string name; double flops; };
    std::vector<Mark> marks;
    size_t marks_used = 0;
    void mark(const std::string& name, double flops = 0.0, int n = 1) {
        tm.n_launches += n;
        if (prof < 3) return;
        if (marks_used == marks.size()) {
            Mark m;
            HIPCHK(hipEventCreate(&m.ev));
            marks.push_back(m);
        }
        marks[marks_used].name = name;
        marks[marks_used].flops = flops;
        HIPCHK(hipEventRecord(marks[marks_used].ev, st));
        ++marks_used;
    }
    static std::string dims(const Act& a) { return std::to_string(a.B) + "x" + std::to_string(a.H) + "x" + std::to_string(a.W) + "x" + std::to_string(a.C); }
    void prof_begin(int kind) {
        if (prof < 2) return;
        if (ev_used == ev_pool.size()) {
            hipEvent_t a, b;
            HIPCHK(hipEventCreate(&a));
            HIPCHK(hipEventCreate(&b));
            ev_pool.push_back({a, b});
            ev_kind.push_back(kind);
        }
        ev_kind[ev_used] = kind;
        HIPCHK(hipEventRecord(ev_pool[ev_used].first, st));
    }
    void prof_end() {
        if (prof < 2) return;
        HIPCHK(hipEventRecord(ev_pool[ev_used].second, st));
        ++ev_used;
    }
    void run_igemm(const IGemmParams& p, int hint = 0) {
        const int taps = p.ks == 3 ? 9 : 1;
        // (contract precision: K is tripled -- hi.hi + lo.hi + hi.lo -- and the ALGORITHMIC count is a third of what the kernel executes)
        const double fl = 2.0 * (double)p.M * (double)p.N * (double)p.Cin * taps * (p.batch > 0 ? p.batch : 1) / (contract ? 3.0 : 1.0);
        const bool halo = conv_uses_halo(p, hint);
        tm.flops_igemm += fl;
        tm.n_igemm++;
        if (halo) { tm.flops_halo += fl; tm.n_halo++; flops_halo_exec += (conv_halo_uses_phases(p) ? fl * (4.0 / 9.0) : fl) * (contract ? 3.0 : 1.0); }  // (executed: the tripled K counts)
        if (prof >= 3) {
            const char* path = conv_uses_halo(p, hint) ? (p.in_scale ? (p.in_silu ? "halo+gn+silu" : "halo+gn") : "halo") : igemm_uses_pgemm(p, hint) ? "pgemm" : "igemm";
            mark(std::string(p.ks == 3 ? (p.ups ? "conv3x3up " : (p.stride == 2 ? "conv3x3s2 " : "conv3x3 ")) : (p.batch > 1 ? "bgemm " : "gemm ")) + path + " M=" + std::to_string(p.M) +
                     " N=" + std::to_string(p.N) + " K=" + std::to_string(p.Cin * taps) + (p.batch > 1 ? " batch=" + std::to_string(p.batch) : "") + (p.res ? " +res" : "") +
                     (p.act == GP_ACT_GEGLU ? " geglu" : "") + (p.stats_out ? " +stats" : "") + (p.vt_out ? " q|k|vT" : ""),
                 fl);
        } else {
            tm.n_launches++;
        }
        IGemmParams q = p;
        Pool::Buf ws;
        const int S = halo ? 1 : igemm_ksplit(q, hint);
        if (S > 1) {  // split-K partial sums: from this engine's pool (stream-ordered reuse), never process-global
            q.splitk_ws_floats = (long long)S * q.M * q.n_store;
            ws = pool.alloc((size_t)q.splitk_ws_floats * sizeof(float));
            q.splitk_ws = ws.get<float>();
        }
        prof_begin(halo ? 2 : 0);
        launch_igemm(q, hint, st);
        prof_end();
    }

    struct ConvOpt : ConvForm {
        const Act* residual = nullptr;  // added to the output; conv fills ConvForm::res (16-bit) or the fp32 residual (contract precision) from it
        bool want_stats = false;        // the output feeds a GroupNorm
    };
    static Nhwc nhwc(const Act& a) { return {a.p(), a.B, a.H, a.W, a.C}; }
    ConvForm conv_form(const ConvOpt& o) const {
        ConvForm f = o;
        if (o.residual && !contract) f.res = o.residual->p();
        return f;
    }
    // Contract precision, in all three ops: the product reads a split operand (a stored input is split on entry into `xs`, which ends with the
    // op, after the launch), writes fp32 rows and adds an fp32 residual (igemm_contract).
    // in_scale / in_shift / in_silu: GroupNorm(+SiLU) applied to the staged input inside the halo conv kernel (16-bit only, see conv_gn)
    Act conv(const Act& x0, const PackedW& w, const ConvOpt& o, const float* in_scale = nullptr, const float* in_shift = nullptr, bool in_silu = false) {
        Act xs;
        if (contract && !x0.p()) xs = split_operand(x0);
        const Act& x = xs.data() ? xs : x0;
        IGemmParams p = igemm_conv(nhwc(x), w, conv_form(o), nullptr, zero);
        if (contract) igemm_contract(p, o.residual ? o.residual->f() : nullptr);
        Act y = new_stored(x.B, p.Ho, p.Wo, p.n_store);
        p.out = y.data();
        if (!contract) {
            p.in_scale = in_scale; p.in_shift = in_shift; p.in_silu = in_silu ? 1 : 0;
            if (in_scale && !conv_uses_halo(p, 0)) throw std::logic_error("fused GroupNorm input needs the halo conv kernel");
        }
        if (o.want_stats) attach_stats(y, p);
        run_igemm(p);
        return y;
    }
    // y[M][N] = x[M][K] W^T (+bias) (+res), N = w.cout (GEGLU halves it)
    Act linear(const Act& x0, const PackedW& w, const Act* res = nullptr, int act = GP_ACT_NONE, bool want_stats = false) {
        Act xs;
        if (contract && !x0.p()) xs = split_operand(x0);
        const Act& x = xs.data() ? xs : x0;
        IGemmParams p = igemm_linear(nhwc(x), w, res && !contract ? res->p() : nullptr, act, nullptr, zero);
        if (contract) igemm_contract(p, res ? res->f() : nullptr);
        Act y = new_stored(x.B, x.H, x.W, p.n_store);
        p.out = y.data();
        if (want_stats) attach_stats(y, p);
        run_igemm(p);
        return y;
    }
    // y += x W^T (+bias), in place: y is the residual and the output
    void linear_add_into(const Act& x0, const PackedW& w, const Act& y) {
        Act xs;
        if (contract && !x0.p()) xs = split_operand(x0);
        const Act& x = xs.data() ? xs : x0;
        IGemmParams p = igemm_linear(nhwc(x), w, contract ? nullptr : y.p(), GP_ACT_NONE, nullptr, zero);
        if (contract) igemm_contract(p, y.f());
        p.out = y.data();
        run_igemm(p);
    }
    // V^T[b][c][t] = sum_k Wv[c][k] x[b][t][k] (+ bias[c]); zero-filled up to Tpad
    Pool::Buf v_transposed(const Act& x, const PackedW& wv, int T, int Tpad) {
        const int C = wv.cout;
        Pool::Buf vt = pool.alloc((size_t)x.B * C * Tpad * sizeof(h16_t));
        const IGemmParams p = igemm_bgemm({wv.w, wv.cin_pad, 0}, {x.p(), x.C, (long long)T * x.C}, {vt.get<h16_t>(), Tpad, (long long)C * Tpad}, C, T, wv.cin_pad, T, Tpad, x.B,
                                          wv.bias, GP_BIAS_ROW, 0, zero);
        // rows = channels (320 ... 1280), columns = tokens: 64x64 tiles when there are few tokens or the channel count is not a multiple of 128
        // (320 rows leave a 128-row tile half empty), 128x64 tiles otherwise -- measured per shape with GENPERCEPT_VT_TILE (igemm.hip: tile_hint),
        // 0.77 -> 0.67 ms per pass over the 18 projections
        const int vt_tile = gp_sw().vt_tile;
        run_igemm(p, vt_tile >= 0 ? vt_tile : (T <= 1024 || (C % 128)) ? 2 : 6);
        return vt;
    }
    // statistics -> per-(image, channel) scale / shift in the GN workspace; from the producer's tile partials when it left some
    void gn_scale_shift(const Act& x, const NormW& n, float eps, float*& scale, float*& shift) {
        if (x.C != n.C) throw std::logic_error("groupnorm: channel mismatch");
        float* ws = gn_workspace(x);
        groupnorm_ws_layout(x.B, x.H * x.W, x.C, cfg.norm_groups, ws, &scale, &shift);
        if (contract) {  // statistics pass over the fp32 tensor: centred per-row partials, Chan-combined by the tile finaliser ("mode 3")
            const int R = c_gn_stat_rows(x.H * x.W, x.C, nullptr);
            Pool::Buf part = pool.alloc((size_t)x.B * R * (2 * x.C + 1) * sizeof(float));
            mark("c_gn_stats+finalize " + dims(x), 0.0, 2);
            launch_c_groupnorm_scale_shift(x.f(), part.get<float>(), x.B, x.H, x.W, x.C, cfg.norm_groups, eps, n.g, n.b, scale, shift, st);
            return;
        }
        if (x.st()) {
            mark("gn_finalize_tiles " + dims(x));
            launch_groupnorm_from_partials(x.st(), x.st_mode, x.st_bm, x.B, x.H, x.W, x.C, cfg.norm_groups, eps, n.g, n.b, scale, shift, st);
        } else {
            mark("gn_stats+finalize " + dims(x), 0.0, 2);
            launch_groupnorm_stats(x.p(), n.g, n.b, x.B, x.H * x.W, x.C, cfg.norm_groups, eps, ws, scale, shift, st);
        }
    }
    // one-launch GroupNorm for small maps whose producer left no statistics behind (split-K convs of the 12x12 level, ...)
    bool gn_small(const Act& x) const { return !contract && !x.st() && groupnorm_small_applicable(x.B, x.H * x.W, x.C, cfg.norm_groups) && !gp_sw().no_gn_small; }
    Act groupnorm_small(const Act& x, const NormW& n, float eps, bool silu) {
        if (x.C != n.C) throw std::logic_error("groupnorm: channel mismatch");
        Act y = new_act(x.B, x.H, x.W, x.C);
        mark("gn_small " + dims(x));
        launch_groupnorm_small(x.p(), y.p(), n.g, n.b, x.B, x.H * x.W, x.C, cfg.norm_groups, eps, silu ? 1 : 0, st);
        return y;
    }
    // x * scale + shift (+ SiLU); the normalised tensor only ever feeds a matrix product (contract precision: written as its split operand)
    Act gn_apply(const Act& x, const float* scale, const float* shift, bool silu) {
        Act y = new_product_input(x.B, x.H, x.W, x.C);
        mark((contract ? "c_gn_apply_split " : "gn_apply ") + dims(x));
        if (contract) launch_c_gn_apply_split(x.f(), y.p(), scale, shift, x.B, x.H * x.W, x.C, silu ? 1 : 0, st);
        else launch_groupnorm_apply(x.p(), y.p(), scale, shift, x.B, x.H * x.W, x.C, silu ? 1 : 0, st);
        return y;
    }
    Act groupnorm(const Act& x, const NormW& n, float eps, bool silu) {
        if (gn_small(x)) return groupnorm_small(x, n, eps, silu);
        float *scale, *shift;
        gn_scale_shift(x, n, eps, scale, shift);
        return gn_apply(x, scale, shift, silu);
    }
    float* gn_workspace(const Act& x) {  // partial statistics + per-(image, channel) scale / shift
        const size_t need = groupnorm_ws_layout(x.B, x.H * x.W, x.C, cfg.norm_groups);
        if (need > gn_ws_floats) {
            gn_ws.reset();
            gn_ws = pool.alloc_persistent(need * 4 * 2);
            gn_ws_floats = need * 2;
        }
        return gn_ws.get<float>();
    }
    // conv(act(GroupNorm(x))): statistics pass, then the normalisation is applied either inside the conv kernel on the staged
    // input halo (conv_halo.hip) or, when that kernel does not take the layer, by the separate apply pass.
    Act conv_gn(const Act& x, const NormW& n, float eps, bool silu, const PackedW& w, const ConvOpt& o) {
        // the separate GroupNorm (contract precision: it writes the split operand; small maps without statistics: one launch) unless a halo
        // conv would fuse the apply: keep the statistics path for that
        if (contract || (gn_small(x) && !conv_uses_halo(igemm_conv(nhwc(x), w, conv_form(o), nullptr, zero), 0))) {
            Act y = groupnorm(x, n, eps, silu);
            return conv(y, w, o);
        }
        float *scale, *shift;
        gn_scale_shift(x, n, eps, scale, shift);
        IGemmParams p = igemm_conv(nhwc(x), w, conv_form(o), nullptr, zero);
        p.in_scale = scale; p.in_shift = shift; p.in_silu = silu ? 1 : 0;
        // The fused transform is redone by every 128-channel slice of the output (each slice's workgroup stages its own halo) and it is
        // bound by the two quarter-rate transcendentals per element inside the conv.  One separate apply pass -- 2 x tensor bytes of HBM
        // traffic -- is cheaper than that redundant arithmetic as soon as there are two slices (measured r1: decoder -0.6 ms, encoder
        // -0.4 ms on the large VAE maps; r2: also on the 96x96 .. 24x24 maps, another -1.3 ms per pass), so only single-slice convs fuse.
        const int slices = (w.cout + 127) / 128;
        const bool fuse_here = slices <= gn_fuse_max_slices || x.H * x.W < gn_fuse_always_below_px;
        if (fuse_gn && fuse_here && conv_uses_halo(p, 0)) return conv(x, w, o, scale, shift, silu);
        Act y = gn_apply(x, scale, shift, silu);
        return conv(y, w, o);
    }
    Act layernorm(const Act& x, const NormW& n) {
        Act y = new_product_input(x.B, x.H, x.W, x.C);
        mark((contract ? "c_layernorm_split " : "layernorm ") + dims(x));
        if (contract) launch_c_layernorm_split(x.f(), y.p(), n.g, n.b, (int)x.pixels(), x.C, 1e-5f, st);
        else launch_layernorm(x.p(), y.p(), n.g, n.b, (int)x.pixels(), x.C, 1e-5f, st);
        return y;
    }

    Act resnet(const Act& x, const std::string& name, float eps) {
        const ResW& r = resnets.at(name);
        ConvOpt o1;
        o1.want_stats = true;
        Act h = conv_gn(x, r.n1, eps, true, r.c1, o1);
        Act sc;  // the shortcut's output where there is one; else x itself is the residual
        if (r.has_sc) sc = linear(x, r.sc);
        ConvOpt o;
        o.residual = r.has_sc ? &sc : &x;
        o.want_stats = true;
        return conv_gn(h, r.n2, eps, true, r.c2, o);
    }

    // GEMM -> scores in HBM -> row softmax -> GEMM (head dims other than 512, and the A/B switch GENPERCEPT_NO_FLASH512)
    void vae_attention_unfused(const Act& qk, const h16_t* vt, const Act& o, int B, int T, int Tpad, int C) {
        // logits as fp16 (11 significant bits: finer than the bf16 probabilities they turn into) halve the score traffic, the largest HBM
        // item of this path.  They are the SCALED logits (1/sqrt(C) is folded into the query projection, build_vae_attn) and the fp16
        // conversion saturates at +-65504 (epilogue.h), so an outlier row degrades to a one-hot softmax instead of inf - inf = NaN.
        // GENPERCEPT_FP32_SCORES=1 keeps fp32 (A/B)
        const bool f32_scores = gp_sw().fp32_scores;
        const bool half_scores = !f32_scores && softmax_rows_f16_supported(Tpad);
        Pool::Buf S = pool.alloc((size_t)B * T * Tpad * (half_scores ? 2 : 4));
        run_igemm(igemm_bgemm({qk.p(), 2 * C, (long long)T * 2 * C}, {qk.p() + C, 2 * C, (long long)T * 2 * C}, {S.get<float>(), Tpad, (long long)T * Tpad}, T, T, C,
                              T, T, B, nullptr, GP_BIAS_NONE, half_scores ? 2 : 1, zero));
        Pool::Buf P = pool.alloc((size_t)B * T * Tpad * sizeof(h16_t));
        mark("softmax_rows T=" + std::to_string(T));
        if (half_scores) launch_softmax_rows_f16(S.get<float>(), P.get<h16_t>(), B * T, T, Tpad, 1.0f, st);
        else launch_softmax_rows(S.get<float>(), P.get<h16_t>(), B * T, T, Tpad, 1.0f, st);
        S.reset();
        run_igemm(igemm_bgemm({P.get<h16_t>(), Tpad, (long long)T * Tpad}, {vt, Tpad, (long long)C * Tpad}, {o.p(), C, (long long)T * C}, T, C, Tpad, C, C, B,
                              nullptr, GP_BIAS_NONE, 0, zero));
    }

    // contract precision: softmax(scale q k^T) v per head with fp32 logits in HBM (head split -> batched logits GEMM -> row softmax -> batched
    // P.V GEMM -> head merge; every product over split operands), or fused where c_attention_plan (kernels.h) says so: flash_attn64_split for
    // head_dim 64, flash_attn512_split for the VAE's one head of 512 above 8 GiB of logits + probabilities or by GENPERCEPT_C_FLASH512.
    // qkv: stored [B*T][3C] with q | k | v at columns 0 | C | 2C; returns the A-order operand [B*T][3C] the output projection reads.
    Act attention_c(const Act& qkv, int heads, int hd, float scale) {
        const int B = qkv.B, T = qkv.H * qkv.W, Tpad = round_up(T, 64), Z = B * heads;
        if (hd % 64 || qkv.C != 3 * heads * hd) throw std::logic_error("attention_c: layout");
        const int path = c_attention_plan(B, T, heads, hd, nullptr);
        if (path == C_ATTN_FLASH512 || path == C_ATTN_FLASH64) {
            // fused over hi / lo planes of q | k and of V^T, no logits in HBM (attention.hip): flash_attn512_split for one head of 512 (the VAE,
            // 6 KiB of planes per token), flash_attn64_split for heads of 64
            const bool f512 = path == C_ATTN_FLASH512;
            if (!f512 && scale != 0.125f) throw std::logic_error("attention_c: the split flash kernel computes softmax(q k^T / 8), scale must be 0.125");
            const int C = heads * hd;
            Pool::Buf qk_hi = pool.alloc((size_t)B * T * 2 * C * sizeof(h16_t));
            Pool::Buf qk_lo = pool.alloc((size_t)B * T * 2 * C * sizeof(h16_t));
            Pool::Buf vt_hi = pool.alloc((size_t)Z * hd * Tpad * sizeof(h16_t));
            Pool::Buf vt_lo = pool.alloc((size_t)Z * hd * Tpad * sizeof(h16_t));
            mark("c_qkv_planes T=" + std::to_string(T) + " heads=" + std::to_string(heads), 0.0, 2);
            launch_c_qkv_planes(qkv.f(), qkv.C, qk_hi.get<h16_t>(), qk_lo.get<h16_t>(), vt_hi.get<h16_t>(), vt_lo.get<h16_t>(), B, T, Tpad, heads, hd, st);
            Act a = new_operand(qkv.B, qkv.H, qkv.W, C);
            const double fl = 4.0 * Z * (double)T * T * hd;
            tm.flops_attn += fl;
            tm.n_attn++;
            mark(f512 ? "flash_attn512_split T=" + std::to_string(T) : "flash_attn64_split T=" + std::to_string(T) + " heads=" + std::to_string(heads), fl);
            prof_begin(1);
            if (f512) launch_flash_attn512_split(qk_hi.get<h16_t>(), qk_lo.get<h16_t>(), vt_hi.get<h16_t>(), vt_lo.get<h16_t>(), a.p(), B, T, Tpad, scale, st);
            else launch_flash_attn64_split(qk_hi.get<h16_t>(), qk_lo.get<h16_t>(), vt_hi.get<h16_t>(), vt_lo.get<h16_t>(), a.p(), B, T, heads, 2 * C, Tpad, st);
            prof_end();
            return a;
        }
        if (!c_softmax_split_supported(Tpad)) throw std::logic_error("attention_c: Tpad");
        Pool::Buf Qs = pool.alloc((size_t)Z * T * 3 * hd * sizeof(h16_t));
        Pool::Buf Ks = pool.alloc((size_t)Z * T * 3 * hd * sizeof(h16_t));
        Pool::Buf Vts = pool.alloc((size_t)Z * hd * 3 * Tpad * sizeof(h16_t));
        mark("c_heads_split T=" + std::to_string(T) + " heads=" + std::to_string(heads), 0.0, 2);
        launch_c_heads_split(qkv.f(), qkv.C, Qs.get<h16_t>(), Ks.get<h16_t>(), Vts.get<h16_t>(), B, T, Tpad, heads, hd, st);
        Pool::Buf S = pool.alloc((size_t)Z * T * Tpad * sizeof(float));
        run_igemm(igemm_bgemm({Qs.get<h16_t>(), 3 * hd, (long long)T * 3 * hd}, {Ks.get<h16_t>(), 3 * hd, (long long)T * 3 * hd}, {S.get<float>(), Tpad, (long long)T * Tpad},
                              T, T, 3 * hd, T, T, Z, nullptr, GP_BIAS_NONE, 1, zero));
        Qs.reset();
        Ks.reset();
        Pool::Buf P = pool.alloc((size_t)Z * T * 3 * Tpad * sizeof(h16_t));
        mark("c_softmax_split T=" + std::to_string(T));
        launch_c_softmax_split(S.get<float>(), P.get<h16_t>(), (long long)Z * T, T, Tpad, scale, st);
        S.reset();
        Pool::Buf O = pool.alloc((size_t)Z * T * hd * sizeof(float));
        run_igemm(igemm_bgemm({P.get<h16_t>(), 3 * Tpad, (long long)T * 3 * Tpad}, {Vts.get<h16_t>(), 3 * Tpad, (long long)hd * 3 * Tpad}, {O.get<float>(), hd, (long long)T * hd},
                              T, hd, 3 * Tpad, hd, hd, Z, nullptr, GP_BIAS_NONE, 1, zero));
        P.reset();
        Vts.reset();
        Act a = new_operand(qkv.B, qkv.H, qkv.W, heads * hd);
        mark("c_heads_merge_split " + dims(a));
        launch_c_heads_merge_split(O.get<float>(), a.p(), B, T, heads, hd, st);
        tm.flops_attn += 4.0 * Z * (double)T * T * hd;
        tm.n_attn++;
        return a;
    }
    // VAE self-attention, head_dim 512 = C, one head: the GroupNorm output (consumed: released here, as soon as q, k and v are enqueued) -> the input of to_out
    Act vae_self_attention(Act n, const VaeAttnW& a) {
        if (contract) {  // stacked q | k | v, stored, then the split attention
            Act qkv = linear(n, a.qkv);
            n.reset();
            return attention_c(qkv, 1, a.C, 1.0f / std::sqrt((float)a.C));
        }
        const int T = n.H * n.W, C = a.C, Tpad = round_up(T, 64), B = n.B;
        Act qk = linear(n, a.qk);  // [B*T][2C]
        Pool::Buf vt = v_transposed(n, a.v, T, Tpad);
        n.reset();
        Act o = new_act(qk.B, qk.H, qk.W, C);
        if (flash_attn512_supported(C)) {
            // fused: scores and probabilities never leave the CU (attention.hip: flash_attn512_kernel).  The softmax scale 1/sqrt(C) is
            // folded into the query projection (build_vae_attn), logits exist in fp32 registers only.
            const long long wsf = flash_attn512_workspace_floats(B, T, ncu);
            Pool::Buf ws;
            if (wsf) ws = pool.alloc((size_t)wsf * sizeof(float));
            const double fl = 4.0 * B * (double)T * T * C;
            tm.flops_attn += fl;
            tm.n_attn++;
            mark("flash_attn512 T=" + std::to_string(T), fl);
            prof_begin(1);
            launch_flash_attn512(qk.p(), qk.p() + C, vt.get<h16_t>(), o.p(), ws.get<float>(), B, T, 2 * C, 2 * C, Tpad, C, 1.0f, ncu, st);
            prof_end();
        } else {
            vae_attention_unfused(qk, vt.get<h16_t>(), o, B, T, Tpad, C);
        }
        return o;
    }
    Act vae_attention(const Act& x, const std::string& name) {
        const VaeAttnW& a = vattn.at(name);
        Act o = vae_self_attention(groupnorm(x, a.gn, cfg.vae_norm_eps, false), a);
        return linear(o, a.o, &x, GP_ACT_NONE, true);
    }

    // UNet self-attention, head_dim 64: the LayerNorm output (consumed: released here, as soon as q, k and v are enqueued) -> the input of to_out
    Act self_attention64(Act l1, const TfW& t) {
        if (contract) {  // stacked q | k | v, stored, then the split attention
            Act qkv = linear(l1, t.qkv);
            l1.reset();
            return attention_c(qkv, t.heads, 64, 0.125f);
        }
        const int B = l1.B, T = l1.H * l1.W, C = t.C, Tpad = round_up(T, 64);
        Act qk;
        Pool::Buf vt;
        {   // q | k | V^T in ONE launch when the persistent GEMM takes it (T % 16 == 0 ...), else the q | k GEMM + the transposed V GEMM
            const bool no_fuse = gp_sw().no_qkv_fuse;  // A/B switch
            IGemmParams p = igemm_qkv(nhwc(l1), t.qkv.w, t.qkv.cin_pad, t.qkv.n_rows, t.qkv.cin_pad, C, Tpad, nullptr,
                                      (h16_t*)zero /* (non-null for the applicability test) */, zero);
            // measured (tools/kbench, weight-cold): 4 x 2304 tokens, C = 640: 43 us fused vs 25 + 25; 4 x 576, C = 1280: 46 vs 29 + 25; at
            // 4 x 9216 tokens, C = 320 the transposed stores of the V third (16 bytes per channel row and lane) eat the saving: 55 vs 29 + 25
            // (same-box pipeline A/B, tools/gpu_ab_r03.sh: fusing every level is 0.1-0.2 ms per pass ahead of fusing none, the 4 x 9216 level
            // included: one launch and one pass over the LayerNorm output less outweigh the slower V slices)
            const int fuse_max_rows = gp_sw().qkv_fuse_max_rows;
            if (!no_fuse && p.M <= fuse_max_rows && !t.qkv.bias && l1.C == t.qkv.cin_pad && igemm_uses_pgemm(p, 0)) {
                qk = new_act(l1.B, l1.H, l1.W, 2 * C);
                vt = pool.alloc((size_t)B * C * Tpad * sizeof(h16_t));
                p.out = qk.p(); p.vt_out = vt.get<h16_t>();
                igemm_qkv_clear_pad(p, st);
                run_igemm(p);
            } else {
                qk = linear(l1, t.qk);
                vt = v_transposed(l1, t.v, T, Tpad);
            }
        }
        l1.reset();
        Act a = new_act(qk.B, qk.H, qk.W, C);
        const double fl = 4.0 * B * t.heads * (double)T * T * 64;
        tm.flops_attn += fl;
        tm.n_attn++;
        mark("flash_attn64 T=" + std::to_string(T) + " heads=" + std::to_string(t.heads), fl);
        prof_begin(1);
        launch_flash_attn64(qk.p(), qk.p() + C, vt.get<h16_t>(), a.p(), B, T, t.heads, 2 * C, 2 * C, Tpad, C, st);
        prof_end();
        return a;
    }
    // cross-attention against the folded constant context: y += to_out(attn2(LN2(y))) in place; returns LN3(y), the feed-forward's input
    Act cross_attention(const Act& y, const TfW& t) {
        const int C = t.C, M = (int)y.pixels();
        // two context tokens: LayerNorm + to_q + attention + to_out + residual + the feed-forward's LayerNorm in ONE pass
        if (t.fU && (!contract || c_cross_fold_supported(C))) {
            Act l3 = new_product_input(y.B, y.H, y.W, C);
            mark((contract ? "c_cross_fold " : "cross_attn_fold ") + dims(y));
            if (contract) launch_c_cross_fold(y.f(), y.f(), l3.p(), t.fU, t.fu0, t.fG, t.fc0, t.ln3.g, t.ln3.b, M, C, t.heads, 1e-5f, st);
            else launch_cross_attn_fold(y.p(), y.p(), l3.p(), t.fU, t.fu0, t.fG, t.fc0, t.ln3.g, t.ln3.b, M, C, t.heads, 1e-5f, st);
            return l3;
        }
        Act q2 = linear(layernorm(y, t.ln2), t.q2);  // (the LayerNorm output ends with this statement)
        Act a2 = new_product_input(y.B, y.H, y.W, C);
        mark((contract ? "c_cross_attn_small " : "cross_attn_small ") + dims(q2));
        if (contract) launch_c_cross_attn_small(q2.f(), t.kc, t.vc, a2.p(), M, C, ctx_L, st);
        else launch_cross_attn_small(q2.p(), t.kc, t.vc, a2.p(), M, C, ctx_L, st);
        q2.reset();
        linear_add_into(a2, t.o2, y);
        a2.reset();
        return layernorm(y, t.ln3);
    }
    // BasicTransformerBlock inside Transformer2DModel (custom_unet.py call sites :305-327,341-352)
    Act transformer(const Act& x, const std::string& name) {
        const TfW& t = tfs.at(name);
        if (!t.kc) throw std::logic_error("gp_set_context has not been called");
        Act y = linear(groupnorm(x, t.gn, 1e-6f, false), t.proj_in);
        Act a = self_attention64(layernorm(y, t.ln1), t);
        linear_add_into(a, t.o1, y);  // y += to_out(attn), in place
        a.reset();
        // GEGLU feed-forward
        Act ff = linear(cross_attention(y, t), t.ff1, nullptr, GP_ACT_GEGLU);
        linear_add_into(ff, t.ff2, y);
        ff.reset();
        return linear(y, t.proj_out, &x, GP_ACT_NONE, true);
    }

    // ---- stages ---------------------------------------------------------------------------------------------------
    // rgb (device NCHW) -> latent NHWC, 64 allocated channels (cfg.vae_latent_channels real, scaled by scaling_factor)
    Act vae_encode(const void* rgb, int is_u8, int B, int Hh, int Ww) {
        const PackedW& win = convs.at("vae.encoder.conv_in");
        Act h;
        if (!contract && win.cout % 32 == 0 && win.cin_pad == 64 && !gp_sw().no_rgb_conv) {
            // u8 image -> conv_in output in one kernel (K = 27), statistics for the first resnet's norm1 included
            h = new_act(B, Hh, Ww, win.cout);
            if (fuse_stats) {
                const int rows = rgb_conv_in_rows(B, Hh, Ww);  // persistent conv_in: one row per workgroup + its pixel count (mode 2's layout, centred: "mode 3")
                h.stats = pool.alloc((size_t)B * rows * (2 * win.cout + 1) * sizeof(float));
                h.st_mode = RGB_CONV_IN_STATS_MODE;
                h.st_bm = rows;
            }
            tm.flops_igemm += 2.0 * (double)h.pixels() * win.cout * 27.0;
            mark("rgb_conv_in " + dims(h), 2.0 * (double)h.pixels() * win.cout * 27.0);
            prof_begin(0);
            if (!conv_in_w27) {  // compact K = 27 weight matrix, built once from the packed conv weight
                HIPCHK(hipMalloc((void**)&conv_in_w27, (size_t)win.cout * 32 * sizeof(h16_t)));
                weights_dev.push_back(conv_in_w27);
                launch_pack_k27(win.w, 9 * win.cin_pad, win.cout, conv_in_w27, st);
            }
            launch_rgb_conv_in(rgb, is_u8, conv_in_w27, win.bias, h.p(), h.st(), B, Hh, Ww, win.cout, st);
            prof_end();
        } else {
            Act x = new_product_input(B, Hh, Ww, 64);
            mark(contract ? "c_rgb_split" : "rgb_prologue");
            // (contract precision: x / 255 * 2 - 1 is not a bf16 number: the image itself enters as a split operand)
            if (contract) launch_c_rgb_split(rgb, is_u8, x.p(), B, Hh, Ww, st);
            else launch_rgb_prologue(rgb, is_u8, x.p(), B, Hh, Ww, 64, st);
            ConvOpt oin;
            oin.want_stats = true;
            h = conv(x, win, oin);
        }
        for (int i = 0; i < 4; ++i) {
            for (int j = 0; j < cfg.vae_layers_per_block; ++j) {
                h = resnet(h, "vae.encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.vae_norm_eps);
            }
            if (i != 3) {
                ConvOpt o;  // pad (0,1,0,1) then stride-2 conv without padding (Appendix B.6)
                o.stride = 2; o.pad_t = 0; o.pad_l = 0; o.want_stats = true;
                o.Ho = (h.H + 1 - 3) / 2 + 1; o.Wo = (h.W + 1 - 3) / 2 + 1;
                h = conv(h, convs.at("vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv"), o);
            }
        }
        h = resnet(h, "vae.encoder.mid_block.resnets.0", cfg.vae_norm_eps);
        h = vae_attention(h, "vae.encoder.mid_block.attentions.0");
        h = resnet(h, "vae.encoder.mid_block.resnets.1", cfg.vae_norm_eps);
        Act n = groupnorm(h, norms.at("vae.encoder.conv_norm_out"), cfg.vae_norm_eps, true);
        h.reset();
        ConvOpt o;
        o.n_store = 64;
        return conv(n, convs.at("vae.encoder.conv_out_folded"), o);
    }

    // [h | skip] along the channels
    Act concat(const Act& h, const Act& skip) {
        Act cat = new_stored(h.B, h.H, h.W, h.C + skip.C);
        const int cbm = (fuse_stats && !contract) ? concat_stats_bm((long long)h.H * h.W, h.pixels(), h.C + skip.C) : 0;
        mark("concat " + dims(cat));
        if (contract) {
            launch_concat(h.f(), h.C, skip.f(), skip.C, cat.f(), h.pixels(), st);
        } else if (cbm) {  // the copy also leaves the statistics the resnet's first GroupNorm needs
            cat.stats = pool.alloc((size_t)(h.pixels() / cbm) * cat.C * 2 * sizeof(float));
            cat.st_mode = CONCAT_STATS_MODE;
            cat.st_bm = cbm;
            launch_concat_stats(h.p(), h.C, skip.p(), skip.C, cat.p(), h.pixels(), cbm, cat.st(), st);
        } else {
            launch_concat(h.p(), h.C, skip.p(), skip.C, cat.p(), h.pixels(), st);
        }
        return cat;
    }
    // latent NHWC (64 allocated channels) -> sample NHWC (64 allocated, unet_out_channels real; empty unless wanted) and/or the 4 up-block features
    Act unet(const Act& latent, Act* feats /* [4] or null */, bool want_sample) {
        std::vector<Act> skips;  // owns every down-path output; the running tensor of the down path is skips.back()
        const int nup = 3;
        const bool fwd_size = (latent.H % (1 << nup)) != 0 || (latent.W % (1 << nup)) != 0;
        ConvOpt oin;
        oin.want_stats = true;
        skips.push_back(conv(latent, convs.at("unet.conv_in"), oin));
        for (int i = 0; i < 4; ++i) {
            const std::string bp = "unet.down_blocks." + std::to_string(i);
            for (int j = 0; j < cfg.unet_layers_per_block; ++j) {
                Act y = resnet(skips.back(), bp + ".resnets." + std::to_string(j), cfg.unet_norm_eps);
                if (cfg.unet_down_attn[i]) y = transformer(y, bp + ".attentions." + std::to_string(j));
                skips.push_back(std::move(y));
            }
            if (i != 3) {
                const Act& cur = skips.back();
                ConvOpt o;
                o.stride = 2; o.want_stats = true;
                o.Ho = (cur.H + 2 - 3) / 2 + 1; o.Wo = (cur.W + 2 - 3) / 2 + 1;
                Act y = conv(cur, convs.at(bp + ".downsamplers.0.conv"), o);
                skips.push_back(std::move(y));
            }
        }
        // mid
        Act own = resnet(skips.back(), "unet.mid_block.resnets.0", cfg.unet_norm_eps);
        own = transformer(own, "unet.mid_block.attentions.0");
        own = resnet(own, "unet.mid_block.resnets.1", cfg.unet_norm_eps);
        // up: the running tensor h is `own`, or the caller's feats[i] once an up block's output was moved there (multi_level_feats).  The caller
        // keeps a feature map's tensor; only its statistics partials go back here, where an owned h goes back whole.
        Act* h = &own;
        for (int i = 0; i < 4; ++i) {
            const std::string bp = "unet.up_blocks." + std::to_string(i);
            const bool attn = cfg.unet_down_attn[3 - i];
            const int nres = cfg.unet_layers_per_block + 1;
            for (int j = 0; j < nres; ++j) {
                Act cat = concat(*h, skips.back());
                h->stats.reset();
                own.reset();  // (already empty when h is a feature map)
                h = &own;
                skips.pop_back();
                own = resnet(cat, bp + ".resnets." + std::to_string(j), cfg.unet_norm_eps);
                cat.reset();
                if (attn) own = transformer(own, bp + ".attentions." + std::to_string(j));
            }
            if (i != 3) {
                ConvOpt o;
                if (fwd_size) { o.ups_h = skips.back().H; o.ups_w = skips.back().W; }
                else { o.ups_h = own.H * 2; o.ups_w = own.W * 2; }
                own = conv(own, convs.at(bp + ".upsamplers.0.conv"), o);
            }
            if (feats) {  // custom_unet.py:365,400: the output of every up block; retained, not copied (the buffer outlives its use here)
                feats[i] = std::move(own);
                h = &feats[i];
            }
        }
        Act out;
        if (want_sample && cfg.unet_has_out) {
            Act n = groupnorm(*h, norms.at("unet.conv_norm_out"), cfg.unet_norm_eps, true);
            ConvOpt o;
            o.n_store = 64;
            out = conv(n, convs.at("unet.conv_out"), o);
        }
        h->stats.reset();
        return out;
    }

    // post_quant_conv (1x1 over the latent channels) of in_scale * z_in
    Act post_quant(const Act& z_in, float in_scale) {
        const int L = cfg.vae_latent_channels;
        Act z = new_stored(z_in.B, z_in.H, z_in.W, 64);
        mark("post_quant_conv");
        if (contract) launch_pointwise_small(z_in.f(), z.f(), pq_w_dev, pq_b_dev, z_in.pixels(), L, L, z_in.C, 64, in_scale, st);
        else launch_pointwise_small(z_in.p(), z.p(), pq_w_dev, pq_b_dev, z_in.pixels(), L, L, z_in.C, 64, in_scale, st);
        return z;
    }
    // z_in: NHWC with 64 allocated channels holding the UNet output v (in_scale = -1/scaling) or a pred latent (1/scaling)
    // out_dev != nullptr: the caller wants the fp32 NCHW result of decode_pred (+ clip / shift unless raw); when the fused tail kernel takes
    // the last three layers (conv_few.hip) it is written directly and the returned Act is empty, else decode_to runs decode_epilogue
    Act vae_decode(const Act& z_in, float in_scale, float* out_dev = nullptr, int mean3 = 0, int raw = 0) {
        ConvOpt oin;
        oin.want_stats = true;
        Act h = conv(post_quant(z_in, in_scale), convs.at("vae.decoder.conv_in"), oin);
        h = resnet(h, "vae.decoder.mid_block.resnets.0", cfg.vae_norm_eps);
        h = vae_attention(h, "vae.decoder.mid_block.attentions.0");
        h = resnet(h, "vae.decoder.mid_block.resnets.1", cfg.vae_norm_eps);
        for (int i = 0; i < 4; ++i) {
            for (int j = 0; j < cfg.vae_layers_per_block + 1; ++j) {
                h = resnet(h, "vae.decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), cfg.vae_norm_eps);
            }
            if (i != 3) {
                ConvOpt o;
                o.ups_h = h.H * 2; o.ups_w = h.W * 2; o.want_stats = true;
                h = conv(h, convs.at("vae.decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv"), o);
            }
        }
        const PackedW& wout = convs.at("vae.decoder.conv_out");
        if (!contract && out_dev && conv_few_applicable(h.C, wout.cout, h.H, h.W) && wout.cin_pad == h.C) {
            float *scale, *shift;
            gn_scale_shift(h, norms.at("vae.decoder.conv_norm_out"), cfg.vae_norm_eps, scale, shift);
            const double fl = 2.0 * (double)h.pixels() * wout.cout * 9.0 * h.C;
            tm.flops_igemm += fl;
            tm.n_igemm++;
            mark("conv_few gn+silu+conv3x3+decode " + dims(h), fl);
            prof_begin(0);
            launch_conv_few(h.p(), wout.w, wout.bias, scale, shift, zero, out_dev, h.B, h.H, h.W, 1, mean3, raw, ncu, st);
            prof_end();
            return Act{};
        }
        Act n = groupnorm(h, norms.at("vae.decoder.conv_norm_out"), cfg.vae_norm_eps, true);
        h.reset();
        ConvOpt o;
        o.n_store = 4;  // 3 real channels + one zero: 8-byte pixels for the epilogue
        return conv(n, wout, o);
    }

    // decoder output NHWC (3 real channels) -> the caller's fp32 NCHW map: channel mean, clip / shift unless raw (genpercept_pipeline.py:523-525,469-472)
    void decode_epilogue(const Act& dec, float* out, int mean3, int raw) {
        mark("decode_epilogue");
        if (dec.f()) launch_decode_epilogue(dec.f(), out, dec.B, dec.H, dec.W, dec.C, mean3, raw, st);
        else launch_decode_epilogue(dec.p(), out, dec.B, dec.H, dec.W, dec.C, mean3, raw, st);
    }
    // the decode tail of an entry point: latent -> the caller's map (the fused tail kernel of vae_decode wrote `out` itself when no tensor comes back)
    void decode_to(const Act& z, float in_scale, float* out, int mean3, int raw) {
        Act dec = vae_decode(z, in_scale, out, mean3, raw);
        if (dec.data()) decode_epilogue(dec, out, mean3, raw);
    }

    Act bilinear(const Act& x, int Ho, int Wo, int align_corners) {
        Act y = new_stored(x.B, Ho, Wo, x.C);
        mark("bilinear " + dims(y));
        if (contract) launch_bilinear(x.f(), y.f(), x.B, x.H, x.W, Ho, Wo, x.C, align_corners, st);
        else launch_bilinear(x.p(), y.p(), x.B, x.H, x.W, Ho, Wo, x.C, align_corners, st);
        return y;
    }
    Act relu_input(const Act& x) {  // ReLU(x) as the input of a matrix product
        if (contract) return split_operand(x, GP_ACT_RELU);
        Act r = new_act(x.B, x.H, x.W, x.C);
        mark("relu " + dims(x));
        launch_relu(x.p(), r.p(), x.pixels() * x.C, st);
        return r;
    }
    Act add(const Act& a, const Act& b) {
        Act y = new_stored(a.B, a.H, a.W, a.C);
        mark("add " + dims(a));
        if (contract) launch_add(a.f(), b.f(), y.f(), a.pixels() * a.C, st);
        else launch_add(a.p(), b.p(), y.p(), a.pixels() * a.C, st);
        return y;
    }
    void dpt_final(const Act& z, float* out_dev) {  // head.head.4 (1x1 to one channel), fp32 [B][H * W]
        mark("dpt_final " + dims(z));
        if (contract) launch_dpt_final(z.f(), dpt_w_dev, dpt_b, out_dev, z.B, z.H * z.W, z.C, st);
        else launch_dpt_final(z.p(), dpt_w_dev, dpt_b, out_dev, z.B, z.H * z.W, z.C, st);
    }
    Act rcu(const Act& x, const std::string& p) {  // pre-activation residual unit (dpt_head.py:256-271)
        ConvOpt o1;
        o1.act = GP_ACT_RELU;
        Act h = conv(relu_input(x), convs.at(p + ".convolution1"), o1);
        ConvOpt o2;
        o2.residual = &x;
        return conv(h, convs.at(p + ".convolution2"), o2);
    }
    // feats: reversed multi_level_feats [c0@h, c1@h, c2@h/2, c3@h/4] -> fp32 [B][8h*8w] written to out_dev
    void dpt_head(const Act* const feats[4], float* out_dev) {
        ConvOpt ou;
        ou.ups_h = feats[0]->H * 2; ou.ups_w = feats[0]->W * 2;
        Act nk[4];
        nk[0] = conv(conv(*feats[0], convs.at("dpt.feature_upsample_0.conv"), ou), convs.at("dpt.neck.convs.0"), ConvOpt{});
        for (int i = 1; i < 4; ++i) nk[i] = conv(*feats[i], convs.at("dpt.neck.convs." + std::to_string(i)), ConvOpt{});
        Act fused;
        for (int i = 0; i < 4; ++i) {
            const std::string lp = "dpt.neck.fusion_stage.layers." + std::to_string(i);
            Act x = std::move(nk[3 - i]);
            if (i != 0) {
                if (x.H != fused.H || x.W != fused.W) x = bilinear(x, fused.H, fused.W, 0);
                Act rc = rcu(x, lp + ".residual_layer1");
                x.reset();
                x = add(fused, rc);
                fused.reset();
            }
            Act x2 = rcu(x, lp + ".residual_layer2");
            x.reset();
            // dpt_head.py:303-309 interpolates (bilinear x2, align_corners) and THEN applies the 1x1 projection.  The two commute -- the projection mixes
            // channels per pixel, the interpolation mixes pixels per channel with weights that sum to one, so the bias passes through as well --
            // and the projection on the SOURCE map is a quarter of the GEMM and of its HBM traffic (r5)
            Act pr = linear(x2, convs.at(lp + ".projection"));
            x2.reset();
            fused = bilinear(pr, pr.H * 2, pr.W * 2, 1);
        }
        ConvOpt op;
        op.act = GP_ACT_RELU;
        Act h = conv(fused, convs.at("dpt.head.projection"), op);
        fused.reset();
        h = conv(h, convs.at("dpt.head.head.0"), ConvOpt{});
        h = bilinear(h, h.H * 2, h.W * 2, 1);
        ConvOpt o32;
        o32.act = GP_ACT_RELU;
        h = conv(h, convs.at("dpt.head.head.2"), o32);
        dpt_final(h, out_dev);
    }

    Act from_nchw_f32(const float* src, int B, int C, int Hh, int Ww, int Cpad) {
        Act a = new_stored(B, Hh, Ww, Cpad);
        mark("nchw_f32_to_nhwc");
        if (contract) launch_nchw_f32_to_nhwc(src, a.f(), B, C, Hh, Ww, Cpad, st);
        else launch_nchw_f32_to_nhwc(src, a.p(), B, C, Hh, Ww, Cpad, st);
        return a;
    }
    void to_nchw_f32(const Act& a, int C, float* dst) {
        mark("nhwc_to_nchw_f32");
        if (a.f()) launch_nhwc_to_nchw_f32(a.f(), dst, a.B, C, a.H, a.W, a.C, st);
        else launch_nhwc_to_nchw_f32(a.p(), dst, a.B, C, a.H, a.W, a.C, st);
    }

    // multi-step archs: the fp32 denoising state `sample` and the UNet input `lat` (channels [off, off + L) hold the sample)
    void ddim_init(const float* noise_dev, const Act& lat, float* sample, int L, int off) {
        mark("ddim_init");
        if (contract) launch_ddim_init(noise_dev, lat.f(), sample, lat.B, lat.H, lat.W, L, lat.C, off, st);
        else launch_ddim_init(noise_dev, lat.p(), sample, lat.B, lat.H, lat.W, L, lat.C, off, st);
    }
    void ddim_step(const Act& v, float* sample, const Act& lat, int L, int off, const Act& x0, bool last /* pred_x0 goes to x0 */, const DdimCoef& k) {
        mark("ddim_step");
        if (contract) launch_ddim_step(v.f(), v.C, sample, lat.f(), lat.C, off, last ? x0.f() : nullptr, x0.C, lat.pixels(), L, k, st);
        else launch_ddim_step(v.p(), v.C, sample, lat.p(), lat.C, off, last ? x0.p() : nullptr, x0.C, lat.pixels(), L, k, st);
    }

    void collect_profile() {
        if (prof < 2 || ev_used == 0) return;
        HIPCHK(hipStreamSynchronize(st));
        for (size_t i = 0; i < ev_used; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
            if (ev_kind[i] == 1) tm.ms_attn += ms;
            else tm.ms_igemm += ms;                  // the whole conv / GEMM family ...
            if (ev_kind[i] == 2) tm.ms_halo += ms;   // ... and its dominant member, conv3x3_halo3_kernel, on its own
        }
        ev_used = 0;
    }
};

// =====================================================================================================================
// C-ABI
// =====================================================================================================================
template <typename F>
static gp_status guard(gp_engine* e, F&& f) {
    gp_status st = GP_OK;
    try {
        f();
        return GP_OK;
    } catch (const std::out_of_range& ex) {
        if (e) e->err = ex.what();
        st = GP_ERR_MISSING_WEIGHT;
    } catch (const std::invalid_argument& ex) {
        if (e) e->err = ex.what();
        st = GP_ERR_INVALID;
    } catch (const std::logic_error& ex) {
        if (e) e->err = ex.what();
        st = GP_ERR_STATE;
    } catch (const std::exception& ex) {
        if (e) e->err = ex.what();
        st = GP_ERR_HIP;
    }
    return st;
}

extern "C" {

const char* gp_version(void) { return GP_F16 ? "genpercept_hip 0.3 (gfx950, fp16 elements)" : "genpercept_hip 0.3 (gfx950, bf16 elements)"; }
int gp_abi_version(void) { return GP_ABI_VERSION; }
gp_dtype gp_element_dtype(void) { return GP_F16 ? GP_DT_F16 : GP_DT_BF16; }

void gp_default_config(gp_config* c) {
    memset(c, 0, sizeof(*c));
    c->device = 0;
    c->unet_in_channels = 4; c->unet_out_channels = 4;
    const int bo[4] = {320, 640, 1280, 1280}, nh[4] = {5, 10, 20, 20}, da[4] = {1, 1, 1, 0};
    const int vb[4] = {128, 256, 512, 512}, dn[4] = {320, 640, 1280, 1280};
    for (int i = 0; i < 4; ++i) { c->unet_block_out[i] = bo[i]; c->unet_num_heads[i] = nh[i]; c->unet_down_attn[i] = da[i]; c->vae_block_out[i] = vb[i]; c->dpt_neck[i] = dn[i]; }
    c->unet_layers_per_block = 2; c->unet_cross_dim = 1024; c->unet_has_out = 1; c->unet_norm_eps = 1e-5f;
    c->vae_layers_per_block = 2; c->vae_latent_channels = 4; c->vae_norm_eps = 1e-6f; c->vae_scaling_factor = 0.18215f;
    c->dpt_enabled = 0; c->dpt_fusion = 256; c->norm_groups = 32;
}

gp_status gp_create(const gp_config* cfg, gp_engine** out) {
    if (!cfg || !out) return GP_ERR_INVALID;
    gp_switches_reload();
    gp_engine* e = new gp_engine();
    e->cfg = *cfg;
    *out = e;
    return guard(e, [&] {
        int n = 0;
        HIPCHK(hipGetDeviceCount(&n));
        if (cfg->device < 0 || cfg->device >= n) throw std::invalid_argument("no such HIP device");
        HIPCHK(hipSetDevice(cfg->device));
        hipDeviceProp_t pr;
        HIPCHK(hipGetDeviceProperties(&pr, cfg->device));
        if (pr.multiProcessorCount > 0) e->ncu = pr.multiProcessorCount;
        {   // saturation flags of every translation unit on THIS device (nullptr in the bf16 build: nothing to collect)
            void* (*const tus[])() = GP_SAT_TUS;
            for (auto fn : tus) {
                void* a = fn();
                if (a && e->sat_flags.n < 16) e->sat_flags.f[e->sat_flags.n++] = (unsigned*)a;
            }
            if (e->sat_flags.n > 0) {
                HIPCHK(hipMalloc((void**)&e->sat_dev, 2 * sizeof(unsigned)));
                HIPCHK(hipMemset(e->sat_dev, 0, 2 * sizeof(unsigned)));
            }
        }
        for (int i = 0; i < 4; ++i) {
            if (cfg->unet_block_out[i] % 64 || cfg->vae_block_out[i] % 64) throw std::invalid_argument("block_out_channels must be multiples of 64");
            if (cfg->unet_down_attn[i] && cfg->unet_block_out[i] != 64 * cfg->unet_num_heads[i]) throw std::invalid_argument("attention head_dim must be 64");
        }
        if (cfg->vae_latent_channels > 8 || cfg->vae_latent_channels < 1) throw std::invalid_argument("latent_channels must be in 1..8");
    });
}

void gp_destroy(gp_engine* e) {
    if (!e) return;
    hipSetDevice(e->cfg.device);
    hipDeviceSynchronize();
    for (void* p : e->weights_dev) hipFree(p);
    if (e->sat_dev) hipFree(e->sat_dev);
    for (auto& pr : e->ev_pool) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto& m : e->marks) hipEventDestroy(m.ev);
    for (int i = 0; i < 4; ++i) if (e->ev[i]) hipEventDestroy(e->ev[i]);
    delete e;  // (the pool frees its buffers)
}

const char* gp_last_error(const gp_engine* e) { return e ? e->err.c_str() : "null engine"; }

gp_status gp_load_tensor(gp_engine* e, const char* name, const void* host_ptr, const int64_t* shape, int ndim, gp_dtype dtype) {
    if (!e || !name || !host_ptr || (ndim > 0 && !shape)) return GP_ERR_INVALID;
    return guard(e, [&] {
        if (e->finalized) throw std::logic_error("gp_load_tensor after gp_finalize");
        HostTensor t;
        t.shape.assign(shape, shape + ndim);
        const int64_t n = t.numel();
        t.v.resize((size_t)n);
        if (dtype == GP_DT_F32) memcpy(t.v.data(), host_ptr, (size_t)n * 4);
        else if (dtype == GP_DT_F16) { const uint16_t* s = (const uint16_t*)host_ptr; for (int64_t i = 0; i < n; ++i) t.v[i] = half_to_float(s[i]); }
        else if (dtype == GP_DT_BF16) { const uint16_t* s = (const uint16_t*)host_ptr; for (int64_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)s[i] << 16; memcpy(&t.v[i], &u, 4); } }
        else throw std::invalid_argument("unknown dtype");
        e->host[name] = std::move(t);
    });
}

gp_status gp_set_context(gp_engine* e, const float* embed, int L, int D) {
    if (!e || !embed || L < 1 || D < 1) return GP_ERR_INVALID;
    return guard(e, [&] {
        e->ctx.assign(embed, embed + (size_t)L * D);
        e->ctx_L = L;
        e->ctx_D = D;
        if (e->finalized) { HIPCHK(hipSetDevice(e->cfg.device)); HIPCHK(hipDeviceSynchronize()); e->fold_context(); }
    });
}

gp_status gp_set_timestep(gp_engine* e, float t) {
    if (!e) return GP_ERR_INVALID;
    return guard(e, [&] {
        e->timestep = t;
        if (e->finalized) { HIPCHK(hipSetDevice(e->cfg.device)); HIPCHK(hipDeviceSynchronize()); e->fold_timestep(); }
    });
}

gp_status gp_set_precision(gp_engine* e, gp_precision prec) {
    if (!e || (prec != GP_PREC_NATIVE && prec != GP_PREC_CONTRACT)) return GP_ERR_INVALID;
    return guard(e, [&] {
        if (e->finalized) throw std::logic_error("gp_set_precision after gp_finalize (the weights are packed per precision)");
        // the split is written for bf16 pieces (fp32 range: neither piece can saturate or flush); the fp16 library stays a 16-bit engine
        if (GP_F16 && prec == GP_PREC_CONTRACT) throw std::invalid_argument("contract precision lives in the bf16 library (libgenpercept_hip.so)");
        e->contract = prec == GP_PREC_CONTRACT;
    });
}
gp_precision gp_get_precision(const gp_engine* e) { return (e && e->contract) ? GP_PREC_CONTRACT : GP_PREC_NATIVE; }

gp_status gp_finalize(gp_engine* e) {
    if (!e) return GP_ERR_INVALID;
    return guard(e, [&] { e->finalize(); });
}

gp_status gp_set_profile(gp_engine* e, int level) {
    if (!e) return GP_ERR_INVALID;
    e->prof = level;
    return GP_OK;
}
gp_status gp_reset_timings(gp_engine* e) {
    if (!e) return GP_ERR_INVALID;
    e->tm = gp_timings{};
    e->flops_halo_exec = 0.0;
    e->ev_used = 0;
    return GP_OK;
}
/* MFMA flops the halo-conv launches EXECUTED since gp_reset_timings.  gp_timings.flops_halo counts algorithmic flops (2 M N 9 Cin, what a roofline
 * figure is quoted on); the two differ where a launch does less arithmetic than its algorithmic count: the x2-upsample convs run as four 2 x 2-tap phase
 * convolutions, 4/9 of the flops (conv_halo.hip, PH).  (A new entry point, not a new field: gp_timings is frozen.) */
gp_status gp_halo_executed_flops(gp_engine* e, double* flops) {
    if (!e || !flops) return GP_ERR_INVALID;
    *flops = e->flops_halo_exec;
    return GP_OK;
}
/* Bytes of device memory the activation pool holds (every buffer it ever allocated: the pool recycles, it never returns memory before
 * gp_destroy), i.e. the high-water mark of the engine's transient memory.  Host bookkeeping only. */
gp_status gp_pool_bytes(gp_engine* e, long long* bytes) {
    if (!e || !bytes) return GP_ERR_INVALID;
    *bytes = (long long)e->pool.total;
    return GP_OK;
}
gp_status gp_get_timings(gp_engine* e, gp_timings* out) {
    if (!e || !out) return GP_ERR_INVALID;
    return guard(e, [&] {
        e->collect_profile();
        *out = e->tm;
    });
}

/* fp16 library: number of (call, translation unit) pairs in which a saturating fp32 -> fp16 conversion actually clipped since the last reset
 * (0 = every stored activation was inside the fp16 range: the output is not silently clipped).  Always 0 in the bf16 library.  Synchronises
 * the engine's stream. */
gp_status gp_saturation_events(gp_engine* e, long long* events, int reset) {
    if (!e || !events) return GP_ERR_INVALID;
    return guard(e, [&] {
        *events = 0;
        if (!e->sat_dev) return;
        HIPCHK(hipSetDevice(e->cfg.device));
        unsigned n = 0;
        // the flag words are per translation unit, process and device: a per-kernel entry point (gp_conv2d, gp_gemm, ... never collect) or another
        // engine on this device may have left one set.  Collect before reading so that a reset really starts from clean flags.
        e->collect_saturation();
        HIPCHK(hipStreamSynchronize(e->st));
        HIPCHK(hipMemcpy(&n, e->sat_dev, sizeof(n), hipMemcpyDeviceToHost));
        *events = (long long)n;
        if (reset) HIPCHK(hipMemset(e->sat_dev, 0, sizeof(unsigned)));
    });
}

/* Per-launch log of the last gp_infer at profiling level 3: one line "ms<TAB>flops<TAB>name" per launch (ms = time to the next launch's
 * start: kernel + gap).  Returns the number of bytes the full log needs (incl. NUL); writes at most cap bytes. */
int gp_get_launch_log(gp_engine* e, char* buf, int cap) {
    if (!e) return -1;
    std::string out;
    try {
        if (e->marks_used > 1) {
            HIPCHK(hipEventSynchronize(e->marks[e->marks_used - 1].ev));
            for (size_t i = 0; i + 1 < e->marks_used; ++i) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, e->marks[i].ev, e->marks[i + 1].ev));
                char line[64];
                snprintf(line, sizeof line, "%.4f\t%.0f\t", ms, e->marks[i].flops);
                out += line;
                out += e->marks[i].name;
                out += "\n";
            }
        }
    } catch (const std::exception& ex) {
        e->err = ex.what();
        return -1;
    }
    if (buf && cap > 0) {
        const size_t n = std::min(out.size(), (size_t)cap - 1);
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int)out.size() + 1;
}

}  // extern "C"

static void check_ready(gp_engine* e, void* stream) {
    if (!e->finalized) throw std::logic_error("engine not finalized");
    HIPCHK(hipSetDevice(e->cfg.device));
    // the activation pool hands a buffer to its next user as soon as the last consumer is ENQUEUED, which is only safe within one
    // stream: when the caller switches streams, everything issued on the previous one is waited for first
    if (e->stream_seen && e->last_stream != (hipStream_t)stream) HIPCHK(hipStreamSynchronize(e->last_stream));
    e->last_stream = (hipStream_t)stream;
    e->stream_seen = true;
    e->st = (hipStream_t)stream;
}

// stage events of a whole pass (profiling level >= 1): 0 = start, 1 = encoded, 2 = UNet done, 3 = end
static void stage(gp_engine* e, int i) {
    if (e->prof < 1) return;
    if (!e->ev[i]) HIPCHK(hipEventCreate(&e->ev[i]));
    HIPCHK(hipEventRecord(e->ev[i], e->st));
}
static void begin_pass(gp_engine* e) {
    stage(e, 0);
    e->marks_used = 0;
}
static void end_pass(gp_engine* e) {
    e->mark("END", 0.0, 0);
    stage(e, 3);
    if (e->prof < 1) return;
    HIPCHK(hipEventSynchronize(e->ev[3]));
    HIPCHK(hipEventElapsedTime(&e->tm.ms_encode, e->ev[0], e->ev[1]));
    HIPCHK(hipEventElapsedTime(&e->tm.ms_unet, e->ev[1], e->ev[2]));
    HIPCHK(hipEventElapsedTime(&e->tm.ms_head, e->ev[2], e->ev[3]));
    HIPCHK(hipEventElapsedTime(&e->tm.ms_total, e->ev[0], e->ev[3]));
}
// the last thing every entry point that enqueues work does: every activation and scratch buffer of the call has gone back to the pool by now
static void finish_call(gp_engine* e) {
    e->collect_saturation();
    HIPCHK(hipGetLastError());
    if (e->pool.outstanding != 0) throw std::logic_error("pool buffers outstanding at the end of a call: " + std::to_string(e->pool.outstanding));
}
// An entry point that enqueues work on `stream`: f() runs between check_ready and finish_call.  A stage that throws has, by unwinding, already
// handed its buffers back to the pool while kernels that use them may still be queued: the failed call waits for the device before it returns,
// so the next call's kernels cannot meet them.
template <typename F>
static gp_status guard_call(gp_engine* e, void* stream, F&& f) {
    bool entered = false;
    const gp_status s = guard(e, [&] {
        check_ready(e, stream);
        entered = true;
        f();
        finish_call(e);
    });
    if (s != GP_OK && entered) {
        (void)hipSetDevice(e->cfg.device);
        (void)hipDeviceSynchronize();
    }
    return s;
}

extern "C" {

gp_status gp_infer(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, gp_mode mode, float* out_dev, void* stream) {
    if (!e || !rgb_dev || !out_dev) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        if (B < 1 || H < 8 || W < 8) throw std::invalid_argument("need B >= 1 and H, W >= 8");
        begin_pass(e);
        Act lat = e->vae_encode(rgb_dev, is_u8, B, H, W);
        stage(e, 1);
        if (!e->cfg.dpt_enabled) {
            Act v = e->unet(lat, nullptr, true);
            lat.reset();
            stage(e, 2);
            // scheduler step with beta == 1: pred_x0 = -v (F5); decode_pred divides by the scaling factor
            const int mean3 = !(mode == GP_MODE_NORMAL || mode == GP_MODE_SEG);
            e->decode_to(v, -1.0f / e->cfg.vae_scaling_factor, out_dev, mean3, 0);
        } else {
            Act feats[4];
            e->unet(lat, feats, false);
            lat.reset();
            stage(e, 2);
            const Act* rev[4] = {&feats[3], &feats[2], &feats[1], &feats[0]};
            const long long out_px = (long long)gp_dpt_out_size(rev[0]->H) * gp_dpt_out_size(rev[0]->W);
            e->dpt_head(rev, out_dev);
            for (Act& f : feats) f.reset();
            e->mark("minmax_norm", 0.0, 2);
            Pool::Buf mm_ws = e->pool.alloc((size_t)B * 64 * 2 * sizeof(float));  // [B][64 partials][min, max]
            launch_minmax_norm(out_dev, B, out_px, mm_ws.get<float>(), e->st);
        }
        end_pass(e);
    });
}

gp_status gp_infer_steps(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, gp_mode mode, const gp_ddim_step* steps,
                         int n_steps, const float* noise_dev, float* out_dev, void* stream) {
    if (!e || !rgb_dev || !out_dev || !steps) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        if (B < 1 || H < 8 || W < 8 || n_steps < 1) throw std::invalid_argument("need B >= 1, H, W >= 8 and at least one step");
        if (e->cfg.dpt_enabled || !e->cfg.unet_has_out) throw std::invalid_argument("the multi-step archs use the VAE-decoder head");
        const int L = e->cfg.vae_latent_channels;
        if (e->cfg.unet_in_channels != (noise_dev ? 2 * L : L))
            throw std::invalid_argument(noise_dev ? "an initial noise sample needs a UNet with 2 x latent input channels (marigold, run.py:59-78)"
                                                  : "without an initial noise sample the UNet takes the latent channels only (rgb_blending)");
        begin_pass(e);
        const float t_before = e->timestep;
        Act lat = e->vae_encode(rgb_dev, is_u8, B, H, W);  // channels 0..L-1 = rgb latent; the UNet input tensor from here on
        stage(e, 1);
        const int off = noise_dev ? L : 0;
        Pool::Buf sample = e->pool.alloc((size_t)lat.pixels() * L * sizeof(float));
        e->ddim_init(noise_dev, lat, sample.get<float>(), L, off);
        Act x0 = e->new_stored(B, lat.H, lat.W, 64);
        try {
            for (int i = 0; i < n_steps; ++i) {
                const gp_ddim_step& s = steps[i];
                if (s.timestep != e->timestep) e->set_timestep_on_stream(s.timestep);
                Act v = e->unet(lat, nullptr, true);
                const DdimCoef k{s.x0_sample, s.x0_model, s.eps_sample, s.eps_model, s.prev_x0, s.prev_eps, s.clip};
                e->ddim_step(v, sample.get<float>(), lat, L, off, x0, i == n_steps - 1, k);
            }
        } catch (...) {  // a failed step must not leave the loop's timestep behind as the engine's (gp_set_timestep) one
            if (e->timestep != t_before) {
                try { e->set_timestep_on_stream(t_before); } catch (...) {}
            }
            throw;
        }
        sample.reset();
        lat.reset();
        if (e->timestep != t_before) e->set_timestep_on_stream(t_before);
        stage(e, 2);
        const int mean3 = !(mode == GP_MODE_NORMAL || mode == GP_MODE_SEG);
        e->decode_to(x0, 1.0f / e->cfg.vae_scaling_factor, out_dev, mean3, 0);
        x0.reset();
        end_pass(e);
    });
}

gp_status gp_vae_encode(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, float* latent_out, void* stream) {
    if (!e || !rgb_dev || !latent_out) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        Act lat = e->vae_encode(rgb_dev, is_u8, B, H, W);
        e->to_nchw_f32(lat, e->cfg.vae_latent_channels, latent_out);
    });
}

gp_status gp_unet(gp_engine* e, const float* latent_in, int B, int h, int w, float* sample_out, float* const* feats_out, void* stream) {
    if (!e || !latent_in) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        Act lat = e->from_nchw_f32(latent_in, B, e->cfg.unet_in_channels, h, w, 64);
        Act feats[4];
        Act v = e->unet(lat, feats_out ? feats : nullptr, sample_out != nullptr);
        lat.reset();
        if (sample_out) {
            if (!v.data()) throw std::logic_error("this UNet has no conv_out (DPT variant)");
            e->to_nchw_f32(v, e->cfg.unet_out_channels, sample_out);
        }
        if (feats_out)
            for (int i = 0; i < 4; ++i)
                if (feats_out[i]) e->to_nchw_f32(feats[i], feats[i].C, feats_out[i]);
    });
}

gp_status gp_vae_decode(gp_engine* e, const float* pred_latent, int B, int h, int w, int mean3, float* out, void* stream) {
    if (!e || !pred_latent || !out) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        Act z = e->from_nchw_f32(pred_latent, B, e->cfg.vae_latent_channels, h, w, 64);
        // decode_pred (genpercept_pipeline.py:507-526): channel mean for 1-channel modes, no clip / shift
        e->decode_to(z, 1.0f / e->cfg.vae_scaling_factor, out, mean3, 1);
    });
}

gp_status gp_vae_mid_attention(gp_engine* e, int decoder, const float* x, int B, int h, int w, float* out, void* stream) {
    if (!e || !x || !out) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        const std::string name = decoder ? "vae.decoder.mid_block.attentions.0" : "vae.encoder.mid_block.attentions.0";
        const int C = e->vattn.at(name).C;
        Act a = e->from_nchw_f32(x, B, C, h, w, C);
        Act y = e->vae_attention(a, name);
        a.reset();
        e->to_nchw_f32(y, C, out);
    });
}

gp_status gp_dpt_head(gp_engine* e, const float* const* feats, int B, int h, int w, float* out, void* stream) {
    if (!e || !feats || !out) return GP_ERR_INVALID;
    return guard_call(e, stream, [&] {
        if (!e->dpt_w_dev) throw std::logic_error("DPT head weights were not loaded");
        const int h2 = (h - 1) / 2 + 1, w2 = (w - 1) / 2 + 1;  // UNet stride-2 pad-1 downsamples
        const int hs[4] = {h, h, h2, (h2 - 1) / 2 + 1}, ws[4] = {w, w, w2, (w2 - 1) / 2 + 1};
        Act f[4];
        for (int i = 0; i < 4; ++i) f[i] = e->from_nchw_f32(feats[i], B, e->cfg.dpt_neck[i], hs[i], ws[i], e->cfg.dpt_neck[i]);
        const Act* fp[4] = {&f[0], &f[1], &f[2], &f[3]};
        e->dpt_head(fp, out);
    });
}

}  // extern "C"
