/* genpercept_hip.h — C-ABI of libgenpercept_hip.so: the MI355X (gfx950) engine behind GenPercept's one-step
 * inference path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * What each entry point replaces in the reference (/root/reference, aim-uofa/GenPercept):
 *   gp_infer          GenPerceptPipeline.single_infer               genpercept/genpercept_pipeline.py:375-486
 *   gp_vae_encode     GenPerceptPipeline.encode_rgb                 genpercept/genpercept_pipeline.py:488-505
 *                       (diffusers AutoencoderKL.encoder + quant_conv, call site :500-501)
 *   gp_unet           self.unet(...) / CustomUNet2DConditionModel.forward
 *                                                                   genpercept_pipeline.py:455-457,476-479; models/custom_unet.py:34-427
 *                       (+ scheduler.step == "-model_output", genpercept_pipeline.py:460-465, ddim.py:166-204)
 *   gp_vae_decode     GenPerceptPipeline.decode_pred                genpercept/genpercept_pipeline.py:507-526
 *   gp_dpt_head       DPTNeckHeadForUnetAfterUpsampleIdentity.forward  genpercept/models/dpt_head.py:443-560,585-593
 *   gp_load_tensor    from_pretrained / load_state_dict of the diffusers-layout checkpoints   run.py:296-357
 *   gp_set_context    encode_text + text_embed cache                genpercept_pipeline.py:360-372,425-429
 *   gp_set_timestep   scheduler.set_timesteps / fix_timesteps       genpercept_pipeline.py:403-408
 *   gp_infer_steps    single_infer for archs marigold / rgb_blending: the denoising loop with the DDIM update
 *                                                                   genpercept_pipeline.py:413-422,447-465; ddim.py:144-217; run.py:361-368
 *   gp_eval_depth     eval.py's per-image alignment + metrics               eval.py:168-215; src/util/alignment.py:29-94; src/util/metric.py:34-158
 *   gp_eval_normal    the angular error of angular_loss per image + summary statistics   genpercept/losses/geometry_losses.py:550-590;
 *                       ground-truth column and validity rule                 src/dataset/base_dataset.py:362-363,416-418
 *   gp_eval_mask      (no reference code: genpercept_trainer.py:1169 is a TODO) dis / matting metrics on the saved 8-bit map   run.py:449-455
 *   gp_seg_decode, gp_eval_seg
 *                     (no reference code: the trainer's evaluation branch is a TODO) palette decode and confusion-matrix scores of the seg
 *                       colour output against the RGB label image of column 6   src/dataset/base_dataset.py:333-346,366; run.py:449-455
 *   gp_mask_band      (no reference code) the trimap of a ground-truth alpha (dilate(alpha != 0) - erode(alpha == 255)) and the inner boundary
 *                       band of Boundary IoU, as region planes for gp_eval_mask
 *   gp_foreground     (no reference code) what a user does with a matting / dis alpha: the foreground colours by multi-level foreground
 *                       estimation (Germer et al. 2020), the RGBA cutout and the composite over a new background
 *   gp_guided_upsample
 *                     (no reference code: genpercept_pipeline.py:301-307 resizes the map) the prediction brought to the input size
 *                       with the image as guide: the fast guided filter of He and Sun 2015
 *   gp_tile_merge     (no reference code) tiled high-resolution inference: each window's prediction at native resolution fitted onto the
 *                       whole-image prediction by least squares, the fitted windows blended across their overlaps
 *   gp_depth_geometry (no reference code: genpercept/losses/metric3d_losses/VNL.py transfer_xyz unprojects with x = (u - u0) z / f and that
 *                       is all) a depth or disparity prediction as a point map, edge-aware surface normals and a point cloud without the
 *                       flying pixels of depth edges
 *   gp_depth_mesh     (no reference code) that point map as a triangle mesh: the grid's nodes joined where the surface is continuous, cut at
 *                       depth edges, compacted into vertices and faces for .glb and .ply export
 *   gp_lens_blur      (no reference code) the photograph refocused under its depth or disparity prediction: a variable-radius,
 *                       occlusion-aware disc gather in integer arithmetic
 *   gp_stereo_views   (no reference code) stereo pairs, anaglyphs and quilts from a depth or disparity prediction: a forward warp of every
 *                       row, cut at depth edges, nearest surface first, disocclusions filled from the background side
 *   gp_parallax_frames (no reference code) the frames of a camera move -- orbit, swing, dolly -- from one photograph and its depth or
 *                       disparity prediction: a forward warp of a triangle mesh cut at depth edges, with a z-test
 *   gp_relight        (no reference code) the photograph under new directional lights: diffuse and specular shading from its normal map,
 *                       screen-space cast shadows marched over its depth or disparity map, in integer arithmetic
 *   gp_ensemble_gather, gp_ensemble_reduce
 *                     ensemble_depth's tensor half (the BFGS fit stays on the host)   genpercept/util/ensemble.py:43-205;
 *                                                                   genpercept_pipeline.py:289-298
 * The per-kernel entry points (gp_conv2d ... gp_bilinear) exist for the parity tests; they are the same launchers the
 * engine uses.
 *
 * Ownership: the engine owns weights, folded constants and its activation pool.  The caller owns every in/out DEVICE
 * buffer (e.g. PyTorch-ROCm tensors passed by data_ptr()) and keeps them alive until the stream has been synchronised.
 * Errors: every call returns gp_status; gp_last_error() gives the message.  Nothing throws across the ABI.
 * Threading: one engine per GPU; an engine is not re-entrant; different engines (same or different GPUs) may run on different host
 *   threads concurrently: every workspace an engine call touches (activation pool, split-K partial sums, GroupNorm statistics, min-max
 *   partials) belongs to that engine, and per-device kernel attributes are set per device.  An engine recycles activation buffers in
 *   stream order; if consecutive calls pass different streams, the engine synchronises the previous stream first.  A call that fails
 *   returns every buffer it had taken to the engine's pool.  The per-kernel entry points (parity-test interface) share one scratch
 *   set per device and serialise on a process-wide mutex while they enqueue.
 */
#ifndef GENPERCEPT_HIP_H
#define GENPERCEPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gp_engine gp_engine;

typedef enum { GP_OK = 0, GP_ERR_INVALID = 1, GP_ERR_HIP = 2, GP_ERR_MISSING_WEIGHT = 3, GP_ERR_STATE = 4 } gp_status;
typedef enum { GP_DT_F32 = 0, GP_DT_F16 = 1, GP_DT_BF16 = 2 } gp_dtype;
/* depth / matting / dis / disparity average the 3 decoder channels (genpercept_pipeline.py:523-525); normal / seg keep 3 */
typedef enum { GP_MODE_DEPTH = 0, GP_MODE_NORMAL = 1, GP_MODE_SEG = 2, GP_MODE_MATTING = 3, GP_MODE_DIS = 4, GP_MODE_DISPARITY = 5 } gp_mode;

typedef struct gp_config {
    int device;                 /* HIP device ordinal */
    /* UNet2DConditionModel (SD2.1 unet/config.json) */
    int unet_in_channels, unet_out_channels;
    int unet_block_out[4];
    int unet_num_heads[4];      /* `attention_head_dim` of the config = number of heads; head_dim must be 64 */
    int unet_down_attn[4];      /* 1 = CrossAttnDownBlock2D, 0 = DownBlock2D */
    int unet_layers_per_block;
    int unet_cross_dim;
    int unet_has_out;           /* 0 for DPT-head UNets (conv_norm_out / conv_out deleted, run.py:316-318) */
    float unet_norm_eps;
    /* AutoencoderKL (SD2.1 vae/config.json) */
    int vae_block_out[4];
    int vae_layers_per_block;
    int vae_latent_channels;
    float vae_norm_eps;
    float vae_scaling_factor;   /* GenPerceptPipeline.latent_scale_factor = 0.18215 */
    /* DPT neck+head (hf_configs/dpt-sd2.1-unet-after-upsample-general/config.json); dpt_enabled = 0 -> VAE-decoder head */
    int dpt_enabled;
    int dpt_neck[4];
    int dpt_fusion;
    int norm_groups;            /* 32 */
} gp_config;

typedef struct gp_timings {
    float ms_encode, ms_unet, ms_head, ms_total;   /* last gp_infer, valid when profiling level >= 1 */
    double flops_igemm, flops_attn;                /* algorithmic flops issued since gp_reset_timings */
    float ms_igemm, ms_attn;                       /* summed kernel time of those launches (profiling level 2) */
    int n_igemm, n_attn, n_launches;
    double flops_halo;                             /* the dominant kernel alone: conv3x3_halo3_kernel (a subset of the igemm figures) */
    float ms_halo;
    int n_halo;
} gp_timings;   /* (frozen layout: new counters get their own entry point, e.g. gp_saturation_events, never a field appended here) */

void gp_default_config(gp_config* cfg);                                  /* SD2.1 values */
gp_status gp_create(const gp_config* cfg, gp_engine** out);
void gp_destroy(gp_engine* e);
const char* gp_last_error(const gp_engine* e);
const char* gp_version(void);
/* Bumped whenever a struct layout or an existing signature changes (additions do not bump it).  3: gp_timings lost its trailing `sat_events`
 * field in round 5 (gp_saturation_events replaced it) -- a client built against the older header must be rebuilt; it can check this at load time. */
#define GP_ABI_VERSION 3
int gp_abi_version(void);
/* Storage / MFMA-operand element of THIS library: GP_DT_BF16 (libgenpercept_hip.so) or GP_DT_F16 (libgenpercept_hip_f16.so, the
 * reference's half precision: run.py --half_precision / torch_dtype=torch.float16).  Per-kernel entry points take and return
 * tensors of this element type; stage-level entry points are fp32 at the boundary in both libraries. */
gp_dtype gp_element_dtype(void);

/* Arithmetic of the engine (call before gp_finalize; the weights are packed per precision):
 *   GP_PREC_NATIVE    16-bit storage and MFMA operands in this library's element type (the default; BASELINE.json's bf16 when this is
 *                     libgenpercept_hip.so, the reference's --half_precision when it is libgenpercept_hip_f16.so).
 *   GP_PREC_CONTRACT  what torch_dtype=float32 -- the reference's default, run.py:273-281 -- asks for: every STORED activation is fp32 and
 *                     every matrix product runs on the bf16 matrix cores with split operands (x = hi + lo, three MFMAs per product: hi.hi +
 *                     lo.hi + hi.lo, fp32 accumulation; csrc/contract.hip).  About 2^-16 relative per product: final maps within 1e-3 of the
 *                     fp32 path under both the mean-absolute and the relative-RMS reading, at roughly a quarter of the native throughput.
 *                     bf16 library only (GP_ERR_INVALID in the fp16 library).
 *                     Memory of the VAE mid-block attention (one head of 512, T = h * w tokens per image) in this precision: the unfused path
 *                     keeps fp32 logits and split probabilities in device memory, 10 * B * T * Tpad bytes (Tpad = T rounded up to 64: 3.4 GB
 *                     for batch 4 at 768 x 768, 10.7 GB at 1024 x 1024), the fused one (flash_attn512_split_kernel) 6 KiB per token and
 *                     nothing quadratic in T.  Selection (gp_c_attention_plan): GENPERCEPT_C_FLASH512=1 always fused, =0 never, unset
 *                     fused only where the unfused workspace would exceed 8 GiB.  The two differ by summation order only. */
typedef enum { GP_PREC_NATIVE = 0, GP_PREC_CONTRACT = 1 } gp_precision;
gp_status gp_set_precision(gp_engine* e, gp_precision prec);
gp_precision gp_get_precision(const gp_engine* e);

/* One call per state-dict entry.  `name` = "<module>.<diffusers key>" with module in {vae, unet, dpt}.  The engine copies
 * (and converts to fp32); the caller keeps ownership of host_ptr. */
gp_status gp_load_tensor(gp_engine* e, const char* name, const void* host_ptr, const int64_t* shape, int ndim, gp_dtype dtype);
/* Text-encoder output for the prompt: embed is HOST fp32 [L][D] (L = 2 for the empty prompt). */
gp_status gp_set_context(gp_engine* e, const float* embed, int L, int D);
gp_status gp_set_timestep(gp_engine* e, float t);                        /* default 1 */
/* Fold constants (time embedding, cross-attention K/V, quant_conv), pack weights to bf16 device layouts, free host copies. */
gp_status gp_finalize(gp_engine* e);

/* rgb_dev: DEVICE [B][3][H][W], uint8 0..255 (is_u8 = 1) or fp32 already in [-1,1] (is_u8 = 0).
 * out_dev: DEVICE fp32 [B][C][8h][8w], C = 1 or 3 by mode, values in [0,1]; (h, w) = gp_latent_size(H), gp_latent_size(W)
 * (== H/8, W/8 when H, W are multiples of 8).  With the DPT head: [B][1][gp_dpt_out_size(h)][gp_dpt_out_size(w)].  stream: hipStream_t (NULL = default). */
int gp_latent_size(int pixels);   /* three VAE downsamples: x -> (x - 2) / 2 + 1 */
int gp_dpt_out_size(int latent);  /* DPT head output edge: 32 * (two UNet downsamples of the latent edge) == 8 * latent when latent % 4 == 0 */
gp_status gp_infer(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, gp_mode mode, float* out_dev, void* stream);

/* The multi-step archs (VAE-decoder head only).  One scheduler step in affine form (what diffusers' DDIMScheduler.step computes for
 * epsilon / sample / v_prediction with eta = 0; the host derives the numbers, genpercept_amd/scheduler.py):
 *   x0 = clip(x0_sample * s + x0_model * m, +-clip)   (clip <= 0: none),   eps = eps_sample * s + eps_model * m,
 *   s' = prev_x0 * x0 + prev_eps * eps,               m = UNet(input_t, timestep), s = current sample.
 * noise_dev != NULL (marigold): DEVICE fp32 [B][L][h][w] initial sample; the UNet reads [rgb_latent, sample] (unet_in_channels == 2L).
 * noise_dev == NULL (rgb_blending): the sample starts as the rgb latent and is itself the UNet input (unet_in_channels == L).
 * The result is the LAST step's x0 (pred_original_sample, :465), decoded / clipped / shifted exactly like gp_infer.  The engine's
 * timestep (gp_set_timestep) is restored on return; the first use of a new timestep value folds its time embedding on the host (tens
 * of ms, once per engine and value), later uses are one device copy. */
typedef struct gp_ddim_step {
    float timestep;
    float x0_sample, x0_model, eps_sample, eps_model, prev_x0, prev_eps, clip;
} gp_ddim_step;
gp_status gp_infer_steps(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, gp_mode mode, const gp_ddim_step* steps,
                         int n_steps, const float* noise_dev, float* out_dev, void* stream);

/* Stage-level entry points (DEVICE fp32 NCHW in/out). */
gp_status gp_vae_encode(gp_engine* e, const void* rgb_dev, int is_u8, int B, int H, int W, float* latent_out, void* stream);
gp_status gp_unet(gp_engine* e, const float* latent_in, int B, int h, int w, float* sample_out /* may be NULL */,
                  float* const* feats_out /* 4 pointers or NULL; multi_level_feats order */, void* stream);
gp_status gp_vae_decode(gp_engine* e, const float* pred_latent, int B, int h, int w, int mean3, float* out, void* stream);
/* The VAE mid-block attention alone (AutoencoderKL mid_block.attentions[0]: GroupNorm, 1 head x C, +residual; call sites
 * genpercept_pipeline.py:500-501 / :521-522); decoder = 0: the encoder's, 1: the decoder's.  x, out: DEVICE fp32 [B][C][h][w]. */
gp_status gp_vae_mid_attention(gp_engine* e, int decoder, const float* x, int B, int h, int w, float* out, void* stream);
gp_status gp_dpt_head(gp_engine* e, const float* const* feats /* reversed multi_level_feats: [c0@h, c1@h, c2@h/2, c3@h/4] */,
                      int B, int h, int w, float* out /* [B][gp_dpt_out_size(h)][gp_dpt_out_size(w)], not normalised */, void* stream);

/* Profiling: level 0 off, 1 per-stage hipEvents, 2 additionally per-launch events on the MFMA kernels. */
gp_status gp_set_profile(gp_engine* e, int level);
gp_status gp_get_timings(gp_engine* e, gp_timings* out);
/* Saturation is never silent in the fp16 library (libgenpercept_hip_f16.so; the reference's --half_precision, run.py:273-281, overflows to
 * inf / NaN on the same activations): conversions saturate at +-65504, and every call in which one actually clipped is counted here --
 * events = (call, kernel file) pairs since the last reset; 0 means no stored activation left the fp16 range.  The bf16 library (fp32
 * range) always reports 0.  Synchronises the engine's stream.  The Python pipeline logs a warning when a call raised events. */
gp_status gp_saturation_events(gp_engine* e, long long* events, int reset);
gp_status gp_reset_timings(gp_engine* e);
/* Bytes of device memory the engine's activation pool holds: everything it ever allocated (it recycles buffers and returns memory only in
 * gp_destroy), i.e. the high-water mark of the transient memory of the calls so far. */
gp_status gp_pool_bytes(gp_engine* e, long long* bytes);
/* executed (not algorithmic) MFMA flops of the halo-conv launches since gp_reset_timings: equals gp_timings.flops_halo except for launches that do
 * less arithmetic than their algorithmic count (the x2-upsample convs as four 2x2-tap phase convolutions: 4/9) */
gp_status gp_halo_executed_flops(gp_engine* e, double* flops);
/* Profiling level 3: text log of the last gp_infer, one line "ms<TAB>algorithmic flops<TAB>description" per kernel launch
 * (ms = start-to-next-start on the stream: kernel time plus the gap behind it).  Returns the bytes needed (incl. NUL). */
int gp_get_launch_log(gp_engine* e, char* buf, int cap);

/* ---- pre / post processing of GenPerceptPipeline.__call__ on the device (DEVICE pointers, NCHW) ---------------------------------
 * resample (genpercept/util/image_util.py:108-126): 0 = bilinear with antialias (torchvision resize(..., antialias=True): ATen's separable
 * triangle filter), 1 = nearest-exact, 2 = bicubic with antialias (the same index ranges, Keys cubic a = -0.5; uint8 results clamped).
 * tmp: DEVICE fp32 scratch for the separable passes, >= B * C * H_in * W_out floats (unused for nearest-exact). */
/* new size of resize_max_res (genpercept/util/image_util.py:75-105): longest edge -> max_edge, int() truncation */
void gp_resize_max_res_size(int H0, int W0, int max_edge, int* h, int* w);
/* resize_max_res on the uint8 RGB [B][3][H0][W0] -> [B][3][h][w] uint8 (fp32 interpolation, round half to even; genpercept_pipeline.py:236-242) */
gp_status gp_preprocess(const void* rgb_u8, int B, int H0, int W0, void* out_u8, int h, int w, int resample, float* tmp, void* stream);
/* The same for FLOAT images (a float `input_image` tensor, e.g. the trainer's `rgb_int`, genpercept_trainer.py:1151-1165): fp32 [B][C][H0][W0]
 * -> [B][C][h][w] fp32, no rounding and no clamp (torchvision's float path; skipped when the sizes are equal), then with normalize != 0
 * x / 255 * 2 - 1 in that operation order (genpercept_pipeline.py:245) -- the [-1, 1] image gp_infer takes with is_u8 = 0. */
gp_status gp_preprocess_f32(const float* rgb, int B, int C, int H0, int W0, float* out, int h, int w, int resample, int normalize, float* tmp,
                            void* stream);
/* genpercept_pipeline.py:301-329 + run.py:449-455: pred fp32 [B][C][h][w] -> resize to (Ho, Wo) (skipped when equal) -> clip to [0, 1]
 * -> pred_out fp32 [B][C][Ho][Wo]; optionally colored_out uint8 [B][Ho][Wo][3] through the 256 x 3 byte colour LUT lut_dev (C == 1), and
 * q_out = (pred_out * 65535).astype(uint16) (q_bits 16) or (pred_out * 255).astype(uint8) (q_bits 8), [B][C][Ho][Wo]. */
gp_status gp_postprocess(const float* pred, int B, int C, int h, int w, float* pred_out, int Ho, int Wo, int resample, float* tmp,
                         const unsigned char* lut_dev, void* colored_out, void* q_out, int q_bits, void* stream);

/* ---- depth evaluation on the device (DEVICE pointers; stateless like the pre / post entries; csrc/eval.hip) ----------------------
 * The per-image protocol of eval.py:168-215 for predictions that are already on the GPU: least-squares alignment in depth or disparity space
 * (src/util/alignment.py:29-94), clip to [min_depth, max_depth] and to >= 1e-6, the ten metrics of src/util/metric.py:34-158.
 * pred, gt: fp32 [B][H][W]; mask: uint8 [B][H][W] (non-zero = valid).  alignment: 0 none, 1 least squares on depth, 2 least squares on
 * disparity (gt_disp = 1 / gt where gt > 0; fit over valid & gt > 0 & pred > 0; aligned = 1 / max(s pred + t, 1e-3)).  fit_cols > 0: the fit
 * (not the metrics) reads columns min(floor(dst * fit_inv_scale), W - 1), dst < fit_cols, of every row -- alignment.py:43-55 with
 * fit_cols = floor(W * scale), fit_inv_scale = float32(1 / scale); 0: the fit reads every pixel.
 * out: double [B][14] = s, t, n_valid, n_fit, then abs_relative_difference, squared_relative_difference, rmse_linear, rmse_log, log10,
 * delta1_acc, delta2_acc, delta3_acc, i_rmse, silog_rmse.  s and t are float32 values (what np.linalg.lstsq returns for float32 data);
 * both are NaN when an image has fewer than two fit pixels or a singular system; alignment 0 gives s = 1, t = 0, n_fit = 0.
 * Sums are float64, reduced in a fixed order that depends on H * W alone: an image's 14 values are bitwise the same from call to call and
 * for every batch it is part of.  workspace: DEVICE scratch of at least the workspace entry's byte count (8-byte aligned), free again once
 * the stream has passed the call.  Four kernel launches on `stream` (three for alignment 0), no host synchronisation. */
long long gp_eval_depth_workspace(int B, int H, int W);   /* bytes; 0 for B, H or W < 1 */
gp_status gp_eval_depth(const float* pred, const float* gt, const unsigned char* mask, int B, int H, int W, int alignment, int fit_cols,
                        float fit_inv_scale, float min_depth, float max_depth, double* out, void* workspace, long long workspace_bytes, void* stream);

/* ---- surface-normal evaluation on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/eval.hip) ----
 * Per image the angle of the reference's angular_loss (genpercept/losses/geometry_losses.py:550-590) between prediction and ground truth at
 * every valid pixel, in float64 and operation by operation what eval_metrics.normal_angular_error computes, and its summary statistics; the
 * ground truth is column 3 of a filename-list line (src/dataset/base_dataset.py:362-363), valid where any channel is non-zero (:416-418);
 * the per-image-then-mean reduction is eval.py's and stays with the caller.
 * pred, gt: fp32 [B][3][H][W].  decode: bit 0 = pred is the pipeline's [0, 1] encoding, bit 1 = gt is; decoding is n = double(x) * 2 - 1.
 * mask: uint8 [B][H][W], non-zero = valid, or NULL: valid = any of the three stored gt channels != 0 (NULL with decode bit 1 is refused).
 * num = (p0 g0 + p1 g1) + p2 g2, |x| = sqrt((x0 x0 + x1 x1) + x2 x2), ang = acos(min(max(num / (max(|p|, 1e-8) max(|g|, 1e-8)), -1 + 1e-4),
 * 1 - 1e-4)), deg = ang * (180 / pi), no FMA: the argument of acos is bitwise the host's, only acos itself may differ in its last bits.
 * out: double [B][8] = n_valid, mean_rad, mean_deg, median_deg, rmse_deg, within_11.25, within_22.5, within_30 (the last seven NaN when
 * n_valid = 0).  median_deg is the EXACT order statistic of the device's own angles, (lo + hi) / 2 of ranks (n - 1) / 2 and n / 2 in degrees
 * (np.median): a radix select over the angles' bit patterns, six digits from the top, integer histograms in LDS, one slab per workgroup.
 * angles_out: optional double [B][H][W], the per-pixel angle in radians, NaN at invalid pixels.
 * Sums are float64 in a fixed order that depends on H * W alone, histogram counts are integers: an image's eight values are bitwise the
 * same from call to call and for every batch it is part of.  workspace: DEVICE scratch of at least the workspace entry's byte count
 * (8-byte aligned; 8 bytes per pixel for the keys plus the slabs), free again once the stream has passed the call.  Fourteen kernel launches
 * on `stream` for every B (angle pass, finaliser, 6 x (histogram, pick)), no global atomics, nothing read back.
 * GP_ERR_INVALID before any HIP call: null pred / gt / out / workspace, B, H or W < 1, B > 65535, H * W > 2^31 - 1, decode outside 0..3,
 * out / angles_out / workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_eval_normal_workspace(int B, int H, int W);      /* bytes; 0 for B, H or W < 1; proportional to B; multiple of 8 */
gp_status gp_eval_normal(const float* pred, const float* gt, const unsigned char* mask, int B, int H, int W, int decode,
                         double* out, double* angles_out, void* workspace, long long workspace_bytes, void* stream);

/* ---- dis / matting evaluation on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/eval.hip) ----
 * Scores the single-channel [0, 1] maps of mode dis and matting against an 8-bit ground truth (mask or alpha).  The reference has no metric for
 * them (genpercept_trainer.py:1169 is a TODO), so the definitions are this project's; eval_metrics.mask_counts / mask_metrics_from_counts are
 * the same definitions on the host.  Everything is computed on the 8-BIT prediction q = (unsigned char)(clamp(x, 0, 1) * 255.0f): the product
 * in fp32, truncated, NaN -> 0 -- on pipeline outputs the byte run.py:449-455 saves and gp_postprocess writes with q_bits = 8.
 * pred: fp32 [B][H][W] (pred_is_u8 = 0; quantised here) or uint8 [B][H][W] (pred_is_u8 = 1; q as it is).  gt: uint8 [B][H][W].
 * region: uint8 [B][H][W], non-zero = scored, or NULL = every pixel (e.g. a trimap's unknown region for matting).
 * Per image over the region R, unsigned 64-bit counts: n = |R|, sum_q = sum q, sad = sum |q - g|, sse = sum (q - g)^2, hist_bg[256] = counts of
 * q over the pixels with g <= 128, hist_fg[256] = counts of q over the pixels with g > 128, n_fg = sum hist_fg.  Integers: exact, order-free.
 * The values are float64, each one fixed sequence of correctly rounded *, /, + on those integers (no FMA):
 *   mae = sad / (255.0 * n);  mse = sse / (65025.0 * n);  sad = sad / 255000.0 (the matting "SAD", in thousands of pixels);
 *   for t = 0..255, prediction positive where q >= t: TP_t = sum_{v >= t} hist_fg[v], P_t = TP_t + sum_{v >= t} hist_bg[v],
 *     prec = TP_t / max(P_t, 1), rec = TP_t / max(n_fg, 1), F_t = ((1.3 * prec) * rec) / (0.3 * prec + rec), 0.0 when that denominator is 0
 *     (beta^2 = 0.3);
 *   max_f = max_t F_t, t_max the smallest t that attains it;  mean_f = (F_0 + F_1 + ... + F_255) / 256.0, summed left to right;
 *   adp_f = F_{t_a}, t_a the smallest integer with t_a * n >= min(2 * sum_q, 255 * n) (threshold = min(2 * mean, 1), in integers);
 *   iou at t = 128: TP / (P + n_fg - TP), 0.0 when that denominator is 0.
 * out: double [B][10] = n, n_fg, mae, mse, sad, max_f, mean_f, adp_f, iou, t_max; n = 0 gives n = n_fg = 0 and NaN for the other eight.
 * counts_out: optional unsigned 64-bit [B][516] = n, sum_q, sad, sse, hist_bg[256], hist_fg[256].
 * An image's values are bitwise the same from call to call, for every batch it is part of and for every pointer alignment.  workspace:
 * DEVICE scratch of at least the workspace entry's byte count (8-byte aligned; one slab of 4 + 512 counts per workgroup), free again once the
 * stream has passed the call.  Two kernel launches on `stream` for every B (count pass of 5 bytes per pixel, 6 with a region, 2 or 3 for
 * uint8 predictions; one finalising workgroup per image), no global atomics, no float sums, nothing read back.
 * GP_ERR_INVALID before any HIP call: null pred / gt / out / workspace, B, H or W < 1, B > 65535, H * W > 2^31 - 1, pred_is_u8 outside 0..1,
 * out / counts_out / workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_eval_mask_workspace(int B, int H, int W);        /* bytes; 0 for B, H or W < 1; proportional to B; multiple of 8 */
gp_status gp_eval_mask(const void* pred, int pred_is_u8, const unsigned char* gt, const unsigned char* region, int B, int H, int W,
                       double* out /* [B][10] */, unsigned long long* counts_out /* [B][516] or NULL */, void* workspace,
                       long long workspace_bytes, void* stream);

/* ---- dis structure scores on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/eval_structure.hip) ----
 * The other three columns of the DIS5K table beside max F and MAE: S-measure (Fan 2017, alpha = 0.5), E-measure (Fan 2018) and the weighted
 * F-measure (Margolin 2014, beta^2 = 1 as published).  The reference has no metric for dis (genpercept_trainer.py:1169 is a TODO), so the
 * definitions are this project's; they follow the published evaluation code wherever integers allow, and eval_metrics.structure_counts /
 * structure_from_counts / edt_keys / weighted_f are the same definitions on the host.  Deviations from the toolboxes: their `eps` terms are
 * dropped wherever the branch structure already keeps the denominator non-zero (the E-measure's alignment and its n - 1, the S-measure's
 * object and block quotients, the weighted F's precision and final quotient), the centroid is rounded in integers, and the weighted F works on
 * the 8-bit prediction like everything else.
 * pred, pred_is_u8, gt as for gp_eval_mask: everything is computed on the 8-bit prediction q; G = g > 128; no region (whole-image scores).
 * p = q / 255.0, n = H * W, n_fg = |G|.  All float64 arithmetic is a fixed sequence of correctly rounded + - * / sqrt, no FMA.
 * E-measure, from hist_bg / hist_fg alone.  Threshold t (positive where q >= t): class counts TP, FP, FN, TN, P_t = TP + FP, mp = P_t / n,
 *   mg = n_fg / n.  0 < n_fg < n: per class ap = p - mp, ag = g - mg with p, g in {0, 1}, phi = ((2 * ap) * ag) / (ap * ap + ag * ag),
 *   e = ((phi + 1) * (phi + 1)) / 4, E_t = (TP * e(TP) + FP * e(FP) + FN * e(FN) + TN * e(TN)) / max(n - 1, 1), summed in that order.
 *   n_fg == 0: E_t = (n - P_t) / max(n - 1, 1);  n_fg == n: E_t = P_t / max(n - 1, 1).
 *   max_e = max_t E_t;  mean_e = (E_0 + ... + E_255) / 256.0, left to right;  adp_e = E_{t_a} with gp_eval_mask's t_a.
 * S-measure.  n_fg == 0: S = 1 - sum q / (255.0 * n);  n_fg == n: S = sum q / (255.0 * n);  otherwise S = max(0.5 * S_o + 0.5 * S_r, 0).
 *   S_o = u * O(fg) + (1 - u) * O(bg), u = n_fg / n.  A class of N pixels with a = sum v, a2 = sum v^2 (v = q on the foreground, 255 - q on
 *   the background): xb = a / (255.0 * N), m2 = a2 / (65025.0 * N), var = (max(m2 - xb * xb, 0) * N) / (N - 1) (0 for N == 1),
 *   O = (2 * xb) / ((xb * xb + 1) + sqrt(var)).
 *   S_r: cx = (2 * sum_fg x + n_fg) div (2 * n_fg), cy likewise (0-based, halves up).  Blocks rows [0, cy] / (cy, H) x columns [0, cx] /
 *   (cx, W) in the order LT, RT, LB, RB, weight N_k / n.  Per block from N, a = sum q, a2 = sum q^2, b = sum G, c = sum q G:
 *   xb = a / (255.0 * N), yb = b / N, sxx = (a2 / 65025.0 - (xb * xb) * N) / (N - 1), syy = (b - (yb * yb) * N) / (N - 1),
 *   sxy = (c / 255.0 - (xb * yb) * N) / (N - 1) (all 0 for N == 1), A = ((4 * xb) * yb) * sxy, Bq = (xb * xb + yb * yb) * (sxx + syy),
 *   Q = A / Bq when both are non-zero, 1 when both are 0, else 0.  S_r = sum w_k * Q_k in block order; a block with N == 0 adds nothing.
 * Weighted F.  key(pixel) = min over foreground pixels of (d2 << 32 | idx): d2 the squared Euclidean distance, idx = y' * W + x'; among
 *   equidistant foreground pixels the smallest row-major index wins; a foreground pixel's key is (0, itself); an image without foreground
 *   has every key = 2^64 - 1.  Et = double(255 - q[idx]) / 255.0;  E = Et on the foreground, q / 255.0 on the background;  EA = the 49-tap
 *   sum K[i][j] * Et(y + i - 3, x + j - 3) in row-major tap order, taps outside the image skipped, K the normalised 7 x 7 Gaussian with
 *   sigma = 5 as a table of hex-float literals (eval_structure.hip ES_K == eval_metrics.WF_K);  Ew = min(EA, E) on the foreground,
 *   E * (2 - exp(c * sqrt(double(d2)))) on the background, c = log(0.5) / 5 as a literal.  S_fg = sum_fg Ew, S_bg = sum_bg Ew: float64 sums
 *   per 32 x 8 tile, tiles added in an order that depends on H and W alone.  TPw = n_fg - S_fg, R = 1 - S_fg / n_fg,
 *   P = TPw / (TPw + S_bg) (0 when that is 0), wf = ((2 * R) * P) / (R + P) (0 when R + P == 0);  n_fg == 0: wf = P = R = S_fg = S_bg = 0.
 *   Only exp may differ from the host in its last bits.
 * out: double [B][15] = n, n_fg, s_alpha, s_object, s_region, max_e, mean_e, adp_e, wf, wf_precision, wf_recall, wf_sum_fg, wf_sum_bg, cx, cy
 *   (s_object = s_region = NaN in the degenerate S branches; cx = cy = 0 without foreground).
 * counts_out: optional unsigned 64-bit [B][537] = n_fg, sum_fg x, sum_fg y, cx, cy, 4 x (N, a, a2, b, c), hist_bg[256], hist_fg[256].
 * edt_out: optional unsigned 64-bit [B][H][W], the keys.
 * An image's values are bitwise the same from call to call and for every batch it is part of.  workspace: DEVICE scratch of at least the
 * workspace entry's byte count (8-byte aligned; about 13 bytes per pixel), free again once the stream has passed the call.  Seven kernel
 * launches on `stream` for every B, no global atomics, nothing read back.
 * GP_ERR_INVALID before any HIP call: null pred / gt / out / workspace, B, H or W < 1, B > 65535, H or W > 32767 (d2 < 2^31),
 * H * W > 2^31 - 1, pred_is_u8 outside 0..1, out / counts_out / edt_out / workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_eval_structure_workspace(int B, int H, int W);   /* bytes; 0 for B, H or W < 1; proportional to B; multiple of 8 */
gp_status gp_eval_structure(const void* pred, int pred_is_u8, const unsigned char* gt, int B, int H, int W, double* out /* [B][15] */,
                            unsigned long long* counts_out /* [B][537] or NULL */, unsigned long long* edt_out /* [B][H][W] keys or NULL */,
                            void* workspace, long long workspace_bytes, void* stream);

/* ---- matting gradient and connectivity errors on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/eval_matting.hip) ----
 * The other two columns of the matting table beside SAD and MSE: Grad and Conn (Rhemann et al. 2009, as used by Deep Image Matting).  The
 * reference has no metric for matting (genpercept_trainer.py:1169 is a TODO), so the definitions are this project's; they follow the published
 * Matlab and Python evaluation code wherever integers allow, and eval_metrics.conn_levels / conn_error / grad_error_map / grad_error are the
 * same definitions on the host.  Deviation from the toolboxes: their Conn compares q / 255 >= k / 10 in floating point, which depends on how
 * k / 10 was produced (byte 153 against 0.6); here the thresholds are integers.
 * pred, pred_is_u8, gt, region as for gp_eval_mask: everything is computed on the 8-bit prediction q against the 8-bit alpha g.  The filters
 * and the labelling run over the whole image; region (non-zero = scored, e.g. a trimap's unknown band; NULL = every pixel) restricts only the
 * final sums.  n = |R|.
 * Conn.  T_k = ceil(255 k / 10), k = 1..10: 26, 51, 77, 102, 128, 153, 179, 204, 230, 255.  m = min(q, g), I_k = { m >= T_k } (nested).
 *   Omega_k = the largest 4-connected component of I_k; among components of equal size the one that holds the smallest row-major pixel index;
 *   empty when I_k is.  level(x) = (the smallest k in 1..10 with x outside Omega_k) - 1, 10 if x is in all ten.
 *   dg = 10 g - 255 level, dq = 10 q - 255 level; dg' = dg if dg >= 383 else 0, dq' likewise (the published >= 0.15 is >= 382.5 on this scale).
 *   conn_num = sum_R |dg' - dq'| (unsigned 64-bit; exact, order-free);  conn = conn_num / 2550000.0 (in thousands), one float64 division.
 * Grad.  Per map x (q, then g): xn = (x - min x) / double(max x - min x), min and max over the whole image; a constant map gives all zeros.
 *   G[9], D[9]: the Gaussian with sigma = 1.4 and its derivative at the taps -4..4 (D[0] > 0, D[4] = 0), each divided by its own L2 norm, as
 *   tables of hex-float literals (eval_matting.hip MT_G, MT_D == eval_metrics.GRAD_G, GRAD_D).
 *   gx(y, x) = sum_i G[i] * (sum_j D[j] * xn(clamp(y + i - 4), clamp(x + j - 4))), gy with the tables exchanged: the inner (row) sum first,
 *   every sum from 0.0 with the taps in index order 0..8, coordinates clamped to the image, float64, no FMA.
 *   amp = sqrt(gx * gx + gy * gy);  err = (amp_q - amp_g) * (amp_q - amp_g);  grad_sum = sum_R err: float64 sums per 32 x 8 tile, tiles added
 *   in an order that depends on H and W alone (the rule of the weighted F);  grad = grad_sum / 1000.0.
 * out: double [B][4] = n, grad, conn, grad_sum; n = 0 gives n = 0 and NaN for the other three.
 * counts_out: optional unsigned 64-bit [B][13] = n, conn_num, then the counts of the levels 0..10 over the WHOLE image (not the region).
 * level_out: optional uint8 [B][H][W], the levels.  grad_map_out: optional double [B][H][W], err (every pixel, whatever the region).
 * The labelling is one union-find over the row-major pixel indices (the root of a component is its smallest index), grown from k = 10 down
 * to 1.  Unlike the other evaluation entries this one USES global atomics, integers only: atomicMin on the 32-bit labels, atomicAdd on the
 * component sizes and the final counts, a 64-bit atomicMax for (size, ~root).  Integer min, add and max are order-free, so an image's values
 * are still bitwise the same from call to call and for every batch it is part of; no float is ever added atomically.  workspace: DEVICE
 * scratch of at least the workspace entry's byte count (8-byte aligned; about 47 bytes per pixel), free again once the stream has passed the
 * call.  26 kernel launches on `stream` for every B, nothing read back.
 * GP_ERR_INVALID before any HIP call: null pred / gt / out / workspace, B, H or W < 1, B > 65535, H * W > 2^31 - 1, pred_is_u8 outside 0..1,
 * a float pred not 4-byte aligned, out / counts_out / grad_map_out / workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_eval_matting_workspace(int B, int H, int W);     /* bytes; 0 for B, H or W < 1; proportional to B; multiple of 8 */
gp_status gp_eval_matting(const void* pred, int pred_is_u8, const unsigned char* gt, const unsigned char* region, int B, int H, int W,
                          double* out /* [B][4] */, unsigned long long* counts_out /* [B][13] or NULL */,
                          unsigned char* level_out /* [B][H][W] or NULL */, double* grad_map_out /* [B][H][W] err or NULL */, void* workspace,
                          long long workspace_bytes, void* stream);

/* ---- seg evaluation on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/eval_seg.hip) ----
 * Mode seg is colour regression: the reference trains it against an RGB label image, column 6 of the filename list
 * (src/dataset/base_dataset.py:333-346,366), and ships neither a palette nor a decode nor a metric (the trainer's evaluation branch is a TODO).
 * So the definitions are this project's and the USER supplies the palette; eval_metrics.palette_labels / seg_gt_labels / seg_counts /
 * seg_metrics_from_counts are the same definitions on the host.
 * palette: uint8 [K][3] (r, g, b), 1 <= K <= 192 (the count kernel keeps K * K 32-bit counters in LDS: 147456 of a CU's 163840 bytes at K = 192);
 *   duplicate colours are allowed; any alignment.
 * Quantised prediction: everything is computed on the 8-BIT prediction, quantise8 per channel = (unsigned char)(clamp(x, 0, 1) * 255.0f), the
 *   product in fp32, truncated, NaN -> 0 -- the byte run.py:449-455 saves and gp_postprocess writes with q_bits = 8.  A uint8 prediction is
 *   taken as it is.  pred: fp32 (pred_is_u8 = 0) or uint8 (pred_is_u8 = 1), [B][3][H][W] planar, planes at any offset (H * W need not be a
 *   multiple of 4).
 * Decode: for a pixel colour (r, g, b), d_k = (r - pr_k)^2 + (g - pg_k)^2 + (b - pb_k)^2 in integers; the class is the SMALLEST k attaining
 *   the minimum, d is that minimum.  Exact and order-free: host and device agree bit for bit, ties included.
 * Ground truth, one of two forms.  gt_is_labels = 0: a colour image, uint8 [B][H][W][3], interleaved as the image file decodes (3 bytes per
 *   pixel at any alignment), decoded by the same rule; a pixel whose minimum distance exceeds gt_tol is void (gt_tol: int >= 0, a squared
 *   distance; 0 = exact palette colour).  gt_is_labels = 1: a label map, uint8 [B][H][W]; values >= K are void (255: the usual ignore label);
 *   gt_tol is ignored.
 * region: uint8 [B][H][W], non-zero = scored, or NULL = every pixel, as in gp_eval_mask.
 * Per image, unsigned 64-bit counts: n = scored pixels (in the region and not void), n_void = pixels in the region but void, sum_d = the sum
 *   of the prediction's d over the scored pixels, conf[g][c] = scored pixels of ground-truth class g (row) predicted as class c (column).
 * The values are float64, each one fixed sequence of correctly rounded + * / sqrt on those integers (no FMA), classes in increasing index:
 *   row_i = sum_j conf[i][j], col_i = sum_j conf[j][i], tp_i = conf[i][i], union_i = row_i + col_i - tp_i, all in integers;
 *   pixel_acc = (sum_i tp_i) / n;  mean_acc = the mean of tp_i / row_i over the classes with row_i > 0;
 *   iou_i = tp_i / union_i where union_i > 0, NaN otherwise;  miou = the mean of the defined iou_i;
 *   fwiou = (sum_{row_i > 0} (double)row_i * iou_i) / n;  colour_rmse = sqrt(sum_d / (3.0 * n)) / 255.0 (how far the colour output sits from
 *   the palette);  n_classes = the number of classes with union_i > 0.
 * out: double [B][8 + K] = n, n_void, pixel_acc, mean_acc, miou, fwiou, colour_rmse, n_classes, iou[K]; n = 0 gives the two counts and NaN
 *   for everything else.
 * counts_out: optional unsigned 64-bit [B][3 + K * K] = n, n_void, sum_d, conf row-major.  labels_out: optional uint8 [B][H][W], the
 *   prediction's classes (every pixel, whatever the region).
 * gp_seg_decode is the decode alone: labels_out uint8 [B][H][W], dist_out optional int32 [B][H][W] = the minimum d.  One kernel launch.
 * gp_eval_seg: THREE kernel launches on `stream` for every B: the per-image matrices (in counts_out, or in the workspace when it is NULL) are
 * zeroed, one count pass (K x K 32-bit counters per workgroup in LDS, filled by LDS integer atomics; the non-zero entries added to the image's
 * matrix by 64-bit integer atomicAdd), one finalising workgroup per image.  Integer global atomics only, exact and order-free as in
 * gp_eval_matting; no float is ever added atomically, nothing is read back.  An image's counts_out, out and labels are bitwise the same from
 * call to call, for every batch it is part of and for every pointer alignment.  workspace: DEVICE scratch of at least the workspace entry's
 * byte count (8-byte aligned; one matrix per image), free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null pred / gt / palette / out / workspace (gp_seg_decode: null pred / palette / labels_out), B, H or
 * W < 1, B > 65535, H * W > 2^31 - 1, K < 1 or K > 192, gt_tol < 0, pred_is_u8 or gt_is_labels outside 0..1, a float pred (or dist_out) not
 * 4-byte aligned, out / counts_out / workspace not 8-byte aligned, workspace_bytes too small. */
gp_status gp_seg_decode(const void* pred, int pred_is_u8, const unsigned char* palette /* [K][3] */, int K, int B, int H, int W,
                        unsigned char* labels_out /* [B][H][W] */, int* dist_out /* [B][H][W] or NULL */, void* stream);
long long gp_eval_seg_workspace(int B, int H, int W, int K);  /* bytes; 0 for B, H or W < 1 or K outside 1..192; proportional to B; multiple of 8 */
gp_status gp_eval_seg(const void* pred, int pred_is_u8, const unsigned char* gt, int gt_is_labels, int gt_tol, const unsigned char* region,
                      const unsigned char* palette /* [K][3] */, int K, int B, int H, int W, double* out /* [B][8 + K] */,
                      unsigned long long* counts_out /* [B][3 + K * K] or NULL */, unsigned char* labels_out /* [B][H][W] or NULL */,
                      void* workspace, long long workspace_bytes, void* stream);

/* ---- trimap and boundary bands on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/mask_band.hip) ----
 * "Which pixels lie within reach of a set and within reach of its complement", exactly: the transition region of the trimap-free matting protocol
 * (P3M / AIM tables: trimap = dilate(alpha != 0) - erode(alpha == 255)) and the inner boundary band of Boundary IoU (Cheng et al. 2021), as 0 / 255
 * planes that gp_eval_mask / gp_eval_matting take as `region` or as maps.  eval_metrics.mask_band is the same definition on the host.
 * a: uint8 [B][H][W] (a_is_u8 = 1) or fp32 [B][H][W] (a_is_u8 = 0), quantised first by gp_eval_mask's rule,
 *   q = (unsigned char)(clamp(x, 0, 1) * 255.0f), NaN -> 0.
 * Thresholds -1 <= lo < hi <= 256:  A = { a > lo },  Bc = { a < hi };  every pixel is in A or in Bc.  The matting trimap is lo = 0, hi = 255; a
 *   binary ground truth g > 128 is lo = 128, hi = 129; a binarised prediction q >= 128 is lo = 127, hi = 128.
 * d(p, S), over the pixels of S INSIDE the image: metric 0 the squared Euclidean distance min (dy^2 + dx^2), metric 1 the Chebyshev distance
 *   min max(|dy|, |dx|); +inf when S is empty.
 * border = 1: the outside of the image counts as Bc, so d(p, Bc) is additionally at most the distance to the nearest outside pixel: with
 *   e = min(y + 1, x + 1, H - y, W - x), e^2 for metric 0 and e for metric 1.  border = 0: nothing lies outside (cv2's default for dilate and
 *   erode alike).
 * reach: an integer.  Metric 0: the squared radius R^2 (the disc dy^2 + dx^2 <= R^2; for a real radius pass floor(radius^2)); metric 1: the radius d.
 * Per pixel:  band = d(p, A) <= reach and d(p, Bc) <= reach;  fg side = d(p, Bc) > reach (implies a >= hi);  bg side = d(p, A) > reach (implies
 *   a <= lo);  inner = p in A and d(p, Bc) <= reach.  band, fg and bg partition the image.  Planes are 0 / 255; trimap is 0 / 128 / 255 for
 *   bg / band / fg.
 * band(metric 1, border 0) is cv2 dilate - erode with a MORPH_RECT kernel of size 2 d + 1, exactly; inner(metric 1, border 1) is Boundary IoU's
 *   "pad with 0, erode d times with 3 x 3, subtract".  cv2's MORPH_ELLIPSE is NOT the disc of metric 0, so numbers differ slightly from tables
 *   that were produced with an elliptical kernel.
 * band_out, fg_out, bg_out, inner_out, trimap_out: uint8 [B][H][W] each, or NULL; at least one is given.
 * Integers only, no atomics, nothing read back; two kernel launches on `stream` for every B (a column pass that leaves one 32-bit word per
 * pixel in the workspace, a row pass).  Every pixel -> thread assignment depends on H, W and reach alone: an image's planes are bitwise the
 * same from call to call and for every batch it is part of.  workspace: DEVICE scratch of at least the workspace entry's byte count (8-byte
 * aligned; 4 bytes per pixel), free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null a / workspace, all five outputs null, B, H or W < 1, B > 65535, H * W > 2^31 - 1, a_is_u8, metric or
 * border outside 0..1, lo < -1, hi > 256 or lo >= hi, reach < 0, reach > 2^24 (metric 0) or reach > 4096 (metric 1), a float `a` not 4-byte
 * aligned, workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_mask_band_workspace(int B, int H, int W);        /* bytes; 0 for B, H or W < 1; proportional to B; multiple of 8 */
gp_status gp_mask_band(const void* a, int a_is_u8, int B, int H, int W, int lo, int hi, int metric, int reach, int border,
                       unsigned char* band_out, unsigned char* fg_out, unsigned char* bg_out, unsigned char* inner_out,
                       unsigned char* trimap_out /* each [B][H][W] or NULL, at least one non-NULL */, void* workspace,
                       long long workspace_bytes, void* stream);

/* ---- matting cutouts on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/foreground.hip) ----
 * Multiplying the image by alpha is not a cutout: where 0 < a < 1 the pixel is a F + (1 - a) B and the old background bleeds in.  gp_foreground
 * estimates the foreground colour F (and the background colour B) by the multi-level method of Germer et al. 2020 ("Fast Multi-Level Foreground
 * Estimation", pymatting's estimate_foreground_ml).  genpercept_amd/foreground.py is the same definition on the host and gives the same bits.
 * Inputs per image: image uint8 [3][H][W]; alpha uint8 [H][W] (alpha_is_u8 = 1) or fp32 [H][W] (alpha_is_u8 = 0), quantised first by
 *   gp_eval_mask's rule, q = (unsigned char)(clamp(x, 0, 1) * 255.0f), NaN -> 0 (run.py:449-455).  I = byte / 255, a = byte / 255, one
 *   float32 division each.  1 <= H, W <= 16384.
 * Arithmetic: float32 throughout; the only operations are + - * / abs min max in exactly the order written below; no fused multiply-add;
 *   division is correctly rounded.  max(v, 0) is (v > 0 ? v : 0) and min(v, 1) is (v < 1 ? v : 1).
 * Levels: L = ceil(log2(max(H, W))), 0 for a 1 x 1 image.  Level l = 0 .. L has h_l = (H + 2^(L-l) - 1) >> (L-l) and w_l likewise (integers;
 *   level 0 is 1 x 1, level L is H x W; pymatting's round(w0 ** (l / L)) is deliberately not used: no size depends on a pow).  Every level
 *   samples image and alpha from the full-resolution bytes, nearest: src = ((y * H) / h_l, (x * W) / w_l).  F and B of level l start as the
 *   nearest upsample of level l-1's result, ((y * h_{l-1}) / h_l, (x * w_{l-1}) / w_l); at level 0, F = B = I.
 * Iterations: a level with h_l <= 32 and w_l <= 32 takes n_small (default 10, 0 .. 64), every other level n_big (default 2, 1 .. 4).  Jacobi:
 *   each reads only the previous iterate.  One iteration at a pixel, neighbours in the order left, right, up, down, coordinates clamped to
 *   the level:
 *     a1 = 1 - a;  a00 = a*a;  a01 = a*a1;  a11 = a1*a1;  b0[c] = a*I[c];  b1[c] = a1*I[c]
 *     for each neighbour n:  da = reg + gw*|a - a_n|;  a00 += da;  a11 += da;  b0[c] += da*F_n[c];  b1[c] += da*B_n[c]
 *     det = a00*a11 - a01*a01;  inv = 1/det
 *     F[c] = min(max(inv*(a11*b0[c] - a01*b1[c]), 0), 1);   B[c] = min(max(inv*(a00*b1[c] - a01*b0[c]), 0), 1)
 *   reg: default 1e-5, range [1e-6, 1] (below it det is no longer safely positive in float32); gw: default 1, range [0, 100].
 * Outputs, each optional, at least one given: fg_out, bg_out fp32 [B][3][H][W];  rgba_out uint8 [B][H][W][4], RGB = min(255, (int)(F*255 + 0.5f)),
 *   A = the alpha byte;  comp_out uint8 [B][3][H][W] = (a*F) + ((1-a)*N) quantised the same way, N = byte / 255 of new_bg uint8 [B][3][H][W]
 *   or, new_bg == NULL, of the one colour new_rgb = 0xRRGGBB.
 * 1 + (levels above 32 x 32) kernel launches on `stream` for every B, no atomics, nothing read back; an image's result is bitwise the same
 * from call to call and in every batch.  workspace: DEVICE scratch of at least the workspace entry's byte count (8-byte aligned), free again
 * once the stream has passed the call.  image, a uint8 alpha, new_bg and comp_out may start at any byte.
 * GP_ERR_INVALID before any HIP call: null image / alpha / workspace, all four outputs null, B < 1, B > 65535, H or W outside 1 .. 16384,
 * alpha_is_u8 outside 0..1, reg, gw, n_small or n_big outside their ranges (NaN included), new_rgb outside 0 .. 0xffffff, a float alpha or
 * fg_out / bg_out / rgba_out not 4-byte aligned, workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_foreground_workspace(int B, int H, int W);       /* bytes; 0 for B, H or W < 1 or H, W > 16384; proportional to B; multiple of 8 */
gp_status gp_foreground(const unsigned char* image, const void* alpha, int alpha_is_u8, int B, int H, int W, float reg, float gw, int n_small,
                        int n_big, const unsigned char* new_bg /* [B][3][H][W] or NULL */, int new_rgb, float* fg_out, float* bg_out,
                        unsigned char* rgba_out, unsigned char* comp_out /* at least one non-NULL */, void* workspace,
                        long long workspace_bytes, void* stream);

/* ---- edge-aware upsampling of a prediction (DEVICE pointers; stateless, stream-ordered, no host synchronisation; csrc/guided.hip) ----
 * A map computed at the processing size and resized bilinearly has edges as wide as the resize factor.  gp_guided_upsample brings it to the
 * input size with the image as guide: the guided filter of He, Sun and Tang (2010 / 2013) in its fast form (He and Sun 2015).  A local linear
 * model q = a . I + b between the low-resolution image and the low-resolution prediction is fitted in every window, a and b are smoothed,
 * upsampled and applied to the full-resolution image.  genpercept_amd/guided.py is the same definition on the host and gives the same bits;
 * the per-pixel arithmetic stands once more in csrc/guided_solve.h.
 * Inputs per image: guide_lo uint8 [3][h][w], the image at the processing size; pred fp32 [C][h][w], C = 1 or 3; guide uint8 [3][H][W], the
 *   image at the output size; r = 1 .. 32, the window radius; eps in (0, 1], the regulariser in units of [0, 1]^2.  1 <= h, w, H, W <= 16384.
 *   Output fp32 [C][H][W] in [0, 1].
 * Quantise: p = (uint16)(clamp(pred, 0, 1) * 65535.0f), a float32 product, truncated, NaN -> 0: the 16-bit rule of gp_postprocess.
 * Window sums: the window of pixel k is the (2 r + 1)^2 square around it clipped to the image, N its pixel count.  Over it S_I[c] (3 sums),
 *   S_II[c][d] (6, c <= d) and per prediction channel S_p and S_Ip[c].  They are exact integers, and with r <= 32 every product below stays
 *   under 2^53 (4225^2 * 255 * 65535 = 3.0e14), so any summation order in int64 or float64 gives the same bits.
 * Solve: float64, the operations + - * / in exactly this order, no fused multiply-add, division correctly rounded.
 *     cov[c] = (N * S_Ip[c] - S_I[c] * S_p) / (N * N)
 *     s[c][d] = (N * S_II[c][d] - S_I[c] * S_I[d]) / (N * N), and + e on the diagonal, e = eps * 65025.0
 *     c00 = s11 s22 - s12 s12;  c01 = s02 s12 - s01 s22;  c02 = s01 s12 - s02 s11
 *     c11 = s00 s22 - s02 s02;  c12 = s01 s02 - s00 s12;  c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02
 *     a[0] = ((c00 cov[0] + c01 cov[1]) + c02 cov[2]) / det;  a[1] = ((c01 cov[0] + c11 cov[1]) + c12 cov[2]) / det
 *     a[2] = ((c02 cov[0] + c12 cov[1]) + c22 cov[2]) / det
 *     b = S_p / N - ((a[0] * (S_I[0] / N) + a[1] * (S_I[1] / N)) + a[2] * (S_I[2] / N))
 * Smooth: the means of a[c] and b over the same clipped window.  These are float64 sums of non-integers, so the order is part of the
 *   definition: each row of the window is summed left to right starting from +0.0, the row sums are summed top to bottom starting from +0.0,
 *   then one division by N.  Every window is summed afresh; a running "add one, drop one" sum rounds differently and is not this definition.
 * Upsample and apply: for output row Y, s = max(0, ((2 Y + 1) h - H) / (2 H)), one float64 division of the two integers; i0 = floor(s),
 *   i1 = min(i0 + 1, h - 1), fy = s - i0; columns likewise (j0, j1, fx).  Each smoothed plane v of a[0], a[1], a[2], b is blended as
 *     t0 = v[i0][j0] + fx * (v[i0][j1] - v[i0][j0]);  t1 = v[i1][j0] + fx * (v[i1][j1] - v[i1][j0]);  V = t0 + fy * (t1 - t0)
 *   (a constant plane stays that constant), and q = (((A[0] * g[0] + A[1] * g[1]) + A[2] * g[2]) + B) / 65535.0 with g the three guide bytes
 *   of the output pixel, clamped by comparisons, q > 0 ? (q < 1 ? q : 1) : 0 (so NaN -> 0), and rounded once to fp32.  With h = H and w = W
 *   this is the plain guided filter; the formula holds for any pair of sizes, larger or smaller.
 * C = 3: the channels are filtered independently and share the image sums.  Normals are NOT renormalised: the caller does that if it wants
 *   unit vectors.  For eps near the lower end det is computed with cancellation (the eigenvalues of s are at least e, its entries reach
 *   16256); the result is still the one the operations above give.
 * Four kernel launches on `stream` for every B (model, row sums, column sums, apply), no atomics, nothing read back; an image's result is
 * bitwise the same from call to call and in every batch.  workspace: DEVICE scratch of at least the workspace entry's byte count (two sets of
 * 4 C float64 planes of h x w per image), 8-byte aligned, free again once the stream has passed the call.  guide_lo and guide may start at any
 * byte.
 * GP_ERR_INVALID before any HIP call: null guide_lo / pred / guide / out / workspace, B, h, w, H or W < 1, B > 65535, a side above 16384,
 * C not 1 or 3, r outside 1 .. 32, eps outside (0, 1] (NaN included), pred or out not 4-byte aligned, workspace not 8-byte aligned,
 * workspace_bytes too small. */
long long gp_guided_upsample_workspace(int B, int C, int h, int w);  /* bytes; 0 for invalid B, C, h, w; proportional to B; multiple of 8 */
gp_status gp_guided_upsample(const unsigned char* guide_lo, const float* pred, int C, const unsigned char* guide, int B, int h, int w, int H,
                             int W, int r, double eps, float* out, void* workspace, long long workspace_bytes, void* stream);

/* ---- the merge of tiled high-resolution inference (DEVICE pointers but ys / xs; stateless, stream-ordered, no host synchronisation; csrc/tile_merge.hip) ----
 * Every map is computed at the processing size; a guided upsample sharpens its edges but adds no detail.  Tiled inference runs the model once on
 * the whole image (the base, for the global layout) and again on overlapping windows at native resolution (the tiles).  gp_tile_merge puts
 * each tile's affine-invariant prediction onto the base and blends the seams.  genpercept_amd/tiled.py is the same definition on the host and
 * gives the same bits; the grid rule, the per-tile solve and the per-pixel steps stand once more in csrc/tile_merge_math.h.
 * Grid: along an axis of length L with tile size T and overlap o the window is w = min(T, L); the tile count is n = 1 if L <= w, else
 *   n = ceil((L - o) / (w - o)); the origins are y_k = (k * (L - w)) / (n - 1) in integers, rounded down (0 for n = 1).  Neighbours overlap by
 *   at least o, the first tile starts at 0, the last ends at L, the origins increase strictly.  Tiles are numbered iy * nx + ix.  Ranges:
 *   1 <= o <= w / 2 on both axes, ny * nx <= 1024, 1 <= H, W <= 16384, C = 1 or 3.  The kernels make the origins from this rule; ys [ny] and
 *   xs [nx] are int32 arrays in HOST memory that have to hold exactly these origins (the caller crops its windows by them), and are checked.
 * Inputs per image: base fp32 [C][H][W], the map of the whole image at the input size; tiles fp32 [N][C][wh][ww], N = ny * nx, the maps of the
 *   windows; the overlap o; align = 0 (least_square) or 1 (none).  Output fp32 [C][H][W] in [0, 1].
 * Fit, per image and tile, over all wh * ww * C values of the window (three channels share one fit):
 *   P = quantise(tile), G = quantise(base window): (uint16)(clamp(x, 0, 1) * 65535.0f), a float32 product, truncated, NaN -> 0: the 16-bit rule of
 *   gp_postprocess.  The sums n, S_P, S_G, S_PP = sum P^2, S_PG = sum P G are exact integers in 64 bits (at most 3 * 2^28 values of at most
 *   65535^2: below 2^63).  Each is converted to float64 once, round to nearest.  Then float64, the operations + - * / in exactly this order, no
 *   fused multiply-add, division correctly rounded:
 *     mp = S_P / n;  mg = S_G / n;  var = S_PP / n - mp * mp;  cov = S_PG / n - mp * mg;  s = cov / var
 *     if not (var >= 1.0) or not (s > 0):  s = 1     (a tile flat to within one 16-bit step, or anti-correlated with the base, is shifted only)
 *     t = (mg - s * mp) / 65535
 *   align = none: s = 1, t = 0 (matting, dis, seg and normal maps are not affine-invariant).
 * Blend, per output pixel and channel: the tiles that cover the pixel are visited in ascending iy, then ascending ix.  The integer weight is
 *   wgt = wy * wx with wy = min(y - y0 + 1, y0 + wh - y, o) and wx likewise, always >= 1.  acc starts at +0.0 and takes
 *   acc += (double)wgt * (s * (double)p + t) -- product, sum, product, sum -- with p the tile's fp32 value as it stands (not quantised).
 *   q = acc / (double)(sum of wgt), clamped by comparisons, q > 0 ? (q < 1 ? q : 1) : 0 (so NaN -> 0), and rounded once to fp32.
 * C = 3: one (s, t) per tile for the three channels.  Normals are NOT renormalised: the caller does that if it wants unit vectors.
 * fit_out (optional): fp64 [B][N][2] = (s, t) of every tile.
 * Three kernel launches on `stream` for every B (fit, solve, blend; two for align = none), no atomics, nothing read back; an image's result is
 * bitwise the same from call to call and in every batch.  workspace: DEVICE scratch of at least the workspace entry's byte count (the (s, t)
 * table and the 64-bit partial sums), 8-byte aligned, free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null base / tiles / ys / xs / out / workspace, B < 1, B > 65535, C not 1 or 3, H or W outside
 * 1 .. 16384, wh > H, ww > W, o outside 1 .. min(wh, ww) / 2, ny or nx not the rule's count, ny * nx > 1024, ys or xs not the rule's origins,
 * align outside 0 .. 1, base, tiles or out not 4-byte aligned, fit_out or workspace not 8-byte aligned, workspace_bytes too small. */
long long gp_tile_merge_workspace(int B, int C, int H, int W, int ny, int nx, int wh, int ww);  /* bytes; 0 for invalid sizes; proportional to B; multiple of 8 */
gp_status gp_tile_merge(const float* base, const float* tiles, int B, int C, int H, int W, const int* ys /* HOST [ny] */, int ny,
                        const int* xs /* HOST [nx] */, int nx, int wh, int ww, int overlap, int align, double* fit_out /* [B][N][2] or NULL */,
                        float* out, void* workspace, long long workspace_bytes, void* stream);

/* ---- point maps, normals and point clouds from a depth prediction (DEVICE pointers but cameras; stateless, stream-ordered, no host synchronisation; csrc/depth_geometry.hip) ----
 * The depth modes stop at a map; the scene in 3-D is a point per pixel, a surface normal per pixel and a point cloud.  Plain finite differences
 * smear normals across every depth edge, and a resized prediction has "flying pixels" between foreground and background; both are dealt with
 * here.  genpercept_amd/geometry.py is the same definition on the host and gives the same bits; the per-pixel arithmetic stands once more in
 * csrc/depth_geometry_math.h.
 * Inputs per image: pred fp32 [1][H][W]; mask uint8 [H][W] or NULL, non-zero means usable; image uint8 [3][H][W] or NULL; the camera, eight
 *   float64 values s, t, fx, fy, cx, cy, z_min, z_max, all finite with fx, fy > 0 and 0 < z_min < z_max.  Per call: space = 0 (depth) or 1
 *   (disparity); the window radius r = 1 .. 8; tau in (0, 1]; min_count in 3 .. (2 r + 1)^2; min_cos in [0, 1); stride = 1 .. 64.
 *   1 <= H, W <= 16384 and B * H * W < 2^31.  The camera is OpenCV's: x right, y down, z forward, and pixel (u, v) has its centre at integer
 *   (u, v).  Everything after the quantisation is float64, the operations + - * / sqrt in exactly the order written, no fused multiply-add,
 *   division and square root correctly rounded.
 * 1. Quantise: Q = (uint16)(clamp(pred, 0, 1) * 65535.0f), a float32 product, truncated: the 16-bit rule of gp_postprocess.
 *    lin = s * (Q / 65535) + t;  z = lin for depth, 1 / lin for disparity.  A pixel is valid iff pred is not NaN, the mask is not 0, z is
 *    finite and z_min <= z <= z_max.  w = 1 / z.
 * 2. Point map: X = ((u - cx) / fx) * z, Y = ((v - cy) / fy) * z, Z = z, each rounded once to fp32; NaN for an invalid pixel.
 * 3. Edge-aware plane fit in inverse depth.  A plane n . P = d seen by a pinhole camera has inverse depth affine in the pixel coordinates, so
 *    the fit is linear and the depth step it must not cross is easy to state.  The members of a valid pixel i are the valid pixels j of its
 *    (2 r + 1)^2 window, clipped to the image, with |z_j - z_i| <= tau * z_i.  They are visited in row-major order; with du = u_j - u_i and
 *    dv = v_j - v_i the integers n, Su, Sv, Suu, Suv, Svv are exact, and the float64 sums Sw, Suw = sum du * w, Svw = sum dv * w start from
 *    +0.0 and take one product and one add per member.  The symmetric system [[Suu, Suv, Su], [., Svv, Sv], [., ., n]] (a, b, c) =
 *    (Suw, Svw, Sw) is solved by cofactors in the order of gp_guided_upsample's solve, s00 .. s22 the matrix:
 *      c00 = s11 s22 - s12 s12;  c01 = s02 s12 - s01 s22;  c02 = s01 s12 - s02 s11;  c11 = s00 s22 - s02 s02;  c12 = s01 s02 - s00 s12
 *      c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02      (for r <= 8 every cofactor and det is an exact integer below 2^53)
 *      a = ((c00 Suw + c01 Svw) + c02 Sw) / det;  b = ((c01 Suw + c11 Svw) + c12 Sw) / det;  c = ((c02 Suw + c12 Svw) + c22 Sw) / det
 *    The fit is valid iff n >= min_count and det > 0.  m = (a * fx, b * fy, (c + a * (cx - u_i)) + b * (cy - v_i)).
 * 4. Normal: N_k = -m_k / sqrt((m0^2 + m1^2) + m2^2), so the normal faces the camera; rounded once to fp32; (0, 0, 0) where the fit is invalid
 *    or the norm is 0 or not finite.
 * 5. Keep, the flying-pixel filter: a pixel is kept iff it is valid, its fit is valid, and with the view ray p = ((u - cx) / fx,
 *    (v - cy) / fy, 1) and mp = (m0 p0 + m1 p1) + m2:  mp * mp >= ((min_cos * min_cos) * ((m0^2 + m1^2) + m2^2)) * ((p0^2 + p1^2) + 1)  and
 *    mp > 0.
 * 6. Compaction: the kept pixels with u % stride == 0 and v % stride == 0 in row-major order, image after image: points fp32 [n][3],
 *    point_normals fp32 [n][3], point_rgb uint8 [n][3] (all 255 without an image), point_index int32 [n] = v * W + u, offsets int64 [B + 1]
 *    (image k owns the points offsets[k] .. offsets[k + 1]; written on the device).  The caller sizes the four point arrays for the worst
 *    case, B * ceil(H / stride) * ceil(W / stride) points.
 * Outputs: xyz fp32 [B][3][H][W], normal fp32 [B][3][H][W], keep uint8 [B][H][W] and the arrays of step 6; each may be NULL, but at least one
 *   of xyz, normal, keep, offsets is given, and a point array needs offsets.  With offsets alone the points are counted only.
 * cameras: float64 [B][8] in HOST memory, checked before any HIP call and copied to the workspace on `stream`; it stays unchanged until the
 * stream has passed the call.  After that copy four kernel launches for every B (geometry; count, scan, scatter: only with offsets, the last
 * only with a point array), no atomics, nothing read back; an image's result is bitwise the same from call to call and in every batch.
 * workspace: DEVICE scratch of at least the workspace entry's byte count (the cameras, the segment counts, a keep plane and the six planes
 * the scatter reads when the caller gives none), 8-byte aligned, free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null pred / cameras / workspace, B < 1, B > 65535, H or W outside 1 .. 16384, B * H * W >= 2^31, space
 * outside 0 .. 1, r outside 1 .. 8, tau outside (0, 1] (NaN included), min_count outside 3 .. (2 r + 1)^2, min_cos outside [0, 1), stride
 * outside 1 .. 64, a camera with a non-finite value, fx or fy <= 0 or not 0 < z_min < z_max, no output at all, a point array without offsets,
 * pred, xyz, normal, points, point_normals or point_index not 4-byte aligned, offsets or workspace not 8-byte aligned, workspace_bytes too
 * small. */
long long gp_depth_geometry_workspace(int B, int H, int W, int stride);  /* bytes; 0 for invalid sizes; proportional to B; multiple of 8 */
gp_status gp_depth_geometry(const float* pred, const unsigned char* mask /* or NULL */, const unsigned char* image /* or NULL */,
                            const double* cameras /* HOST [B][8] */, int B, int H, int W, int space, int r, double tau, int min_count,
                            double min_cos, int stride, float* xyz, float* normal, unsigned char* keep, float* points, float* point_normals,
                            unsigned char* point_rgb, int* point_index, long long* offsets, void* workspace, long long workspace_bytes,
                            void* stream);

/* ---- triangle meshes from the point map of a depth prediction (DEVICE pointers only; stateless, stream-ordered, no host synchronisation, no atomics; csrc/depth_mesh.hip) ----
 * A point cloud has holes as soon as the camera moves and no viewer lights or textures it; joining every pixel to its neighbours draws a
 * "rubber sheet" across every depth edge.  Here the nodes of the stride grid are joined only where both are kept by gp_depth_geometry's
 * flying-pixel filter and their depths are close, so the surface is cut at depth edges.  genpercept_amd/mesh.py is the same definition on the
 * host and gives the same bits; the per-cell arithmetic stands once more in csrc/depth_mesh_math.h.
 * Inputs per image: xyz fp32 [3][H][W] as gp_depth_geometry writes them; normal fp32 [3][H][W] or NULL; keep uint8 [H][W]; image uint8
 *   [3][H][W] or NULL.  Per call: stride = 1 .. 64; cut, float64 in (0, 1] (a NaN is refused; the bindings' default 0.05 is a convention, not
 *   a measurement).  1 <= H, W <= 16384, 1 <= B <= 65535, B * H * W < 2^31 and B * gh * gw < 2^30, so the triangle count stays below 2^31.
 * Grid: gh = ceil(H / stride), gw = ceil(W / stride); node (gy, gx) is the pixel (v, u) = (gy * stride, gx * stride), its k is keep != 0 and
 *   its z is plane 2 of xyz, promoted to float64.
 * Link: two nodes p, q are linked iff both are kept and |z_p - z_q| <= cut * min(z_p, z_q), in float64 and in that order: one subtraction,
 *   fabs, one min, one product, one compare, no fused multiply-add.  A NaN fails the test.
 * Cell (cy, cx), for cy < gh - 1 and cx < gw - 1, has the corners a = (cy, cx), b = (cy, cx + 1), c = (cy + 1, cx), d = (cy + 1, cx + 1) and
 *   the candidate triangles T0 = (a, c, d), T1 = (a, d, b) on diagonal a-d and T2 = (a, c, b), T3 = (b, c, d) on diagonal b-c.  A triangle is
 *   sound iff each of its three edges is linked.  The cell uses diagonal a-d iff k_a and k_d hold and also one of these: k_b and k_c do not
 *   both hold, or |z_a - z_d| <= |z_b - z_c| (a tie goes to a-d); otherwise it uses b-c.  It emits the sound triangles of its diagonal and
 *   nothing from the other one; there is no fallback.  So one foreground corner over a background leaves the one background triangle, and
 *   a cell with three kept corners leaves at most that triangle.  The cell's code is T0 | T1 << 1 | T2 << 2 | T3 << 3: 0, 1, 2, 3, 4, 8 or 12.
 * Winding: the corner orders make (v1 - v0) x (v2 - v0) point to the camera: its dot product with v0 is negative, with the camera at the
 *   origin, x right, y down and z forward (the front face is counter-clockwise seen from the camera in a y-up viewer).
 * Vertices: a node is a vertex iff an emitted triangle uses it (kept pixels that end up in no triangle are not exported), in row-major node
 *   order, image after image: vertices fp32 [n][3] from xyz; vertex_normals fp32 [n][3] from normal (needs the normal input); vertex_rgb
 *   uint8 [n][3], all 255 without an image; vertex_uv fp32 [n][2] = ((u + 0.5) / W, (v + 0.5) / H), float64, each rounded once;
 *   vertex_index int32 [n] = v * W + u.
 * Faces: cells in row-major order, image after image, within a cell T0 before T1 or T2 before T3: faces int32 [m][3], indices local to the
 *   image (the global vertex index minus vertex_offsets[b]), so each image's mesh stands alone.
 * Offsets: vertex_offsets and face_offsets, int64 [B + 1], written on the device, both required.  Every other output may be NULL; with all
 *   of them NULL the call only counts.  The caller sizes the arrays for the worst case, B * gh * gw vertices and 2 * B * (gh - 1) * (gw - 1) faces.
 * Four kernel launches for every B (codes, count, one scan over both count arrays, scatter: the last only with an output array), nothing
 * read back; an image's mesh is bitwise the same from call to call and in every batch.
 * workspace: DEVICE scratch of at least the workspace entry's byte count (a code byte per node; two counts and a 64-bit used mask per
 * segment of 64 nodes), 8-byte aligned, free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null xyz / keep / vertex_offsets / face_offsets / workspace, B < 1, B > 65535, H or W outside
 * 1 .. 16384, B * H * W >= 2^31, B * gh * gw >= 2^30, stride outside 1 .. 64, cut outside (0, 1] (NaN included), vertex_normals without normal,
 * xyz, normal, vertices, vertex_normals, vertex_uv, vertex_index or faces not 4-byte aligned, the offsets or workspace not 8-byte aligned,
 * workspace_bytes too small. */
long long gp_depth_mesh_workspace(int B, int H, int W, int stride);  /* bytes; 0 for invalid sizes; proportional to B; multiple of 8 */
gp_status gp_depth_mesh(const float* xyz, const float* normal /* or NULL */, const unsigned char* keep, const unsigned char* image /* or NULL */,
                        int B, int H, int W, int stride, double cut, float* vertices, float* vertex_normals, unsigned char* vertex_rgb,
                        float* vertex_uv, int* vertex_index, int* faces, long long* vertex_offsets, long long* face_offsets, void* workspace,
                        long long workspace_bytes, void* stream);

/* ---- synthetic depth of field: the photograph refocused under its depth prediction (DEVICE pointers; stateless, stream-ordered, no host synchronisation, no atomics; csrc/lens_blur.hip) ----
 * The image-space use of a monocular depth map: the defocus blur of a wide aperture, driven by the map.  Framework ops give the two classic
 * defects -- blurred background bleeds over the sharp subject's outline, and a blurred foreground is cut off at its own silhouette instead of
 * spreading over what lies behind it.  Here every output pixel is a variable-radius, occlusion-aware gather.  The whole definition is integer
 * arithmetic, so the result does not depend on the order of the gather and the device equals the host route genpercept_amd/lens_blur.py bit
 * for bit; the arithmetic stands once more in csrc/lens_blur_math.h.
 * Inputs per image: image uint8 [3][H][W]; pred fp32 [1][H][W]; sharp uint8 [H][W] or NULL, non-zero pins the pixel sharp (a matting alpha,
 *   thresholded, keeps the subject in focus); a row of four int32 parameters F, gain, cmax8, dz.  Per call: space = 0 (depth) or 1 (disparity);
 *   to_lin uint16 [256], strictly increasing with values <= 4095, the bytes of the image as linear light; from_lin uint8 [4096], its inverse,
 *   from_lin[to_lin[v]] == v for every v.  1 <= H, W <= 16384 and B * H * W < 2^31; 0 <= F, dz <= 65535; 0 <= gain <= 32768;
 *   0 <= cmax8 <= max_c8 <= 256 (a blur radius of at most 32 pixels, in eighths of a pixel).
 * 1. Nearness: Q = (uint16)(clamp(pred, 0, 1) * 65535.0f), the 16-bit rule of gp_postprocess.  D = Q in disparity space and D = 65535 - Q in
 *    depth space, so a larger D is nearer.  A NaN pixel has D = 0.
 * 2. Circle of confusion in eighths of a pixel: e = max(0, |D - F| - dz); c = min(cmax8, (e * gain + 32768) >> 16); c = 0 where pred is NaN or
 *    sharp is non-zero.  F is the nearness in focus, dz the half-width of the sharp zone around it.  The radius is LINEAR IN THE MAP'S VALUE:
 *    for a disparity map that is the thin-lens law (the circle of confusion of a thin lens is proportional to |1 / z - 1 / z_focus|), whatever
 *    the unknown scale and shift of an affine-invariant disparity; for an affine-invariant depth map it is a stated convention, not optics.
 * 3. Disc sizes: n(c) = the number of integer offsets (dx, dy) with 64 (dx^2 + dy^2) <= (c + 4)^2, a disc of radius c / 8 + 1 / 2 pixels;
 *    w(c) = floor(2^20 / n(c)).  n(0) = n(3) = 1, n(4) = 5, n(8) = 9, n(16) = 21, n(64) = 225, n(256) = 3313, w(256) = 316.
 * 4. Gather: for the output pixel p, a source pixel q inside the image at offset (dx, dy) has the reach r = c_q if D_q >= D_p -- a nearer or
 *    equally near source spreads over p -- and r = min(c_q, c_p) otherwise: a source behind p is seen through p only as far as p itself is
 *    blurred.  q contributes iff 64 (dx^2 + dy^2) <= (r + 4)^2, with the weight w(r).  Sw = sum w, S_k = sum w * to_lin[image_k(q)]: exact
 *    integers that fit in 64 bits (at most 65^2 sources * 2^20 * 4095).  p always contributes to itself, so Sw > 0.  Pixels outside the image
 *    do not exist; nothing is replicated.
 * 5. Output: out_k(p) = from_lin[(2 S_k + Sw) / (2 Sw)], integer division.  coc(p) = c_p.
 * Outputs: out uint8 [B][3][H][W] (not the image itself); coc uint16 [B][H][W] or NULL.
 * params: int32 [B][4] in DEVICE memory, so that a focus picked from the map on the device needs no read-back; for the same reason its values
 * cannot be refused, and one outside its range is clamped into it (cmax8 into 0 .. max_c8).  max_c8, a host value, sizes the apron every
 * tile is staged with.  to_lin and from_lin are DEVICE tables; their monotonicity and round trip are the caller's to check
 * (genpercept_amd/lens_blur.py check_tables does); the kernel reads 12 bits of a to_lin value, so a wrong table gives wrong colours and no
 * wild access.  One kernel launch for every B: a workgroup stages its 32 x 16 tile and the apron in LDS as one 64-bit word per pixel and
 * bounds its search by the largest c of the staged region; no workspace, nothing read back; an image's bytes are the same from call to call
 * and in every batch.
 * GP_ERR_INVALID before any HIP call: null image / pred / params / to_lin / from_lin / out, B < 1, B > 65535, H or W outside 1 .. 16384,
 * B * H * W >= 2^31, space outside 0 .. 1, max_c8 outside 0 .. 256, pred or params not 4-byte aligned, to_lin or coc not 2-byte aligned,
 * out == image. */
gp_status gp_lens_blur(const unsigned char* image, const float* pred, const unsigned char* sharp /* or NULL */, const int* params /* [B][4] */,
                       const unsigned short* to_lin /* [256] */, const unsigned char* from_lin /* [4096] */, int B, int H, int W, int space,
                       int max_c8, unsigned char* out, unsigned short* coc /* or NULL */, void* stream);

/* ---- stereo and parallax views: the photograph re-rendered from viewpoints shifted sideways (DEVICE pointers but the view table; stateless, stream-ordered, no host synchronisation, no atomics; csrc/stereo.hip) ----
 * The second eye of a monocular depth map: side-by-side frames, anaglyphs, "wiggle" pairs and the 9 to 48 view quilts of lenticular and
 * light-field displays.  With framework ops this is a grid_sample by the disparity, a BACKWARD warp that smears the foreground across every
 * depth edge and cannot tell an occlusion from a disocclusion.  Here it is a forward warp (depth-image-based rendering): each row of the
 * picture is a 1-D surface that is cut at depth edges and rasterised, the nearest surface wins where two land on one pixel, and the holes a
 * new viewpoint opens are filled from the background side.  The whole definition is integer arithmetic, so the result does not depend on the
 * order of evaluation and the device equals the host route genpercept_amd/stereo.py bit for bit; the arithmetic stands once more in
 * csrc/stereo_math.h.
 * Inputs per image: image uint8 [3][H][W]; pred fp32 [1][H][W]; one int32 F of conv [B], the nearness of the zero-parallax plane.  Per call:
 *   space = 0 (depth) or 1 (disparity); edge 0 .. 65535; max_s8 0 .. 512, the largest shift in eighths of a pixel (at most 64 pixels), which
 *   sizes the apron; a HOST table views int32 [V][4] = (g, ox, oy, cmask) per view, 1 <= V <= 64, |g| <= 131072, (ox, oy) the origin of the
 *   view's H x W rectangle in the canvas, cmask in 1 .. 7 the channels the view writes (bit k: channel k).  1 <= H, W, CH, CW <= 16384 and
 *   B * V * H * W < 2^31.
 * 1. Nearness: Q = (uint16)(clamp(pred, 0, 1) * 65535.0f); D = Q in disparity space and D = 65535 - Q in depth space.  A NaN pixel has D = 0.
 *    This is step 1 of gp_lens_blur.
 * 2. Shift of source column x for view k in eighths of a pixel: s = ((int64)(D - F) * g + 2^23) >> 24, an arithmetic shift, that is a floor,
 *    then clamped to -max_s8 .. max_s8.  t_x = 8 x + s.  Rows are independent and shifts are horizontal only.
 * 3. Surface: neighbours x and x + 1 of a row are CONNECTED iff |D_x - D_{x+1}| <= edge.  The pieces that can cover output column p, at
 *    P = 8 p, are
 *      the span of a connected pair with L = t_{x+1} - t_x > 0 and t_x <= P < t_{x+1}: with a = P - t_x the nearness
 *        (D_x (L - a) + D_{x+1} a + (L >> 1)) / L and per channel the colour (c_x (L - a) + c_{x+1} a + (L >> 1)) / L, integer divisions,
 *        everything below 2^27;
 *      the left cap of x, t_x - 4 <= P < t_x, which exists iff x = 0 or (x - 1, x) is not connected;
 *      the right cap of x, t_x <= P < t_x + 4, which exists iff x = W - 1 or (x, x + 1) is not connected; both caps carry D_x and c_x.
 *    A connected pair with L <= 0 (a fold) covers nothing.  Pixels outside the image do not exist.
 * 4. Visibility: among the pieces that cover p the largest nearness wins; ties go to the smallest x (no two pieces of one x cover one P).
 * 5. Holes: a column that no piece covers is a disocclusion.  Let l and r be the nearest covered columns of the same output row to its left
 *    and to its right, looked for within R = max_s8 / 4 + 1 columns.  The hole takes the colour and nearness of the one with the SMALLER
 *    nearness -- the background continues behind the foreground --, l on a tie; the one that exists if only one does; colour 0 and nearness 0
 *    if neither does, as in a row with nothing covered.
 *    Why R: a hole opens where the surface is cut.  Between the right cap of source x, which ends at t_x + 4, and the left cap of source
 *    x + 1, which begins at t_{x+1} - 4, lie s_{x+1} - s_x <= 2 max_s8 eighths, that is at most max_s8 / 4 columns; the same holds between a
 *    border of the row and the cap of its first or last source, |s| <= max_s8 eighths away from where it came from.  Every connected stretch
 *    of sources that moves forwards covers all it passes over.  So on a surface of planar pieces -- piecewise-planar rows of W = 1 .. 89 with
 *    max_s8 0 .. 512 and every edge showed no exception -- each existing neighbour lies within R columns.  The bound is nevertheless part of
 *    the DEFINITION and not only of the search: a row that alternates folds and cuts at sub-pixel phases (a left cap, a fold back by more
 *    than a pixel, a right cap, each four eighths wide and between two sample positions) covers no column over any length, and there a
 *    column further than R from everything covered takes colour 0 and nearness 0, on the host route as on the device.
 * 6. Outputs: canvas uint8 [B][3][CH][CW] (not the image itself): view k writes the bytes of its cmask channels at (oy + y, ox + x); bytes no
 *    view writes keep what they held.  holes uint8 [B][V][H][W] or NULL: 1 marks a disocclusion, for a user's own inpainting.  near uint16
 *    [B][V][H][W] or NULL: the winning or copied nearness, the new view's own map (a disparity map for gp_lens_blur).
 * The table of rectangles and channel masks expresses a pair ([3][H][2 W]), side by side, over / under, an anaglyph (both views at (0, 0),
 * masks 1 and 6) and a quilt of ny x nx views in one call, with no copy afterwards.  F is DEVICE memory so that a convergence plane picked
 * from the map needs no read-back; for the same reason it cannot be refused, and a value outside 0 .. 65535 is clamped.
 * Two launches for any B and V: a warp pass (a workgroup stages 256 source columns of a row and the apron in LDS, bounds its search by the
 * largest |s| of the staged region and gathers every view's columns) and a fill pass.  No atomics, nothing read back; an image's bytes are
 * the same from call to call and in every batch.  workspace: DEVICE scratch of at least the workspace entry's byte count (the nearness-and-
 * covered plane between the two passes), 8-byte aligned, free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null image / pred / conv / views / canvas / workspace, B < 1, B > 65535, V outside 1 .. 64, H, W, CH or
 * CW outside 1 .. 16384, B * V * H * W >= 2^31, space outside 0 .. 1, edge outside 0 .. 65535, max_s8 outside 0 .. 512, |g| > 131072, cmask
 * outside 1 .. 7, a rectangle that leaves the canvas, two rectangles that overlap and share a channel (a race), pred or conv not 4-byte
 * aligned, near not 2-byte aligned, workspace not 8-byte aligned, workspace_bytes too small, canvas == image. */
long long gp_stereo_views_workspace(int B, int V, int H, int W);  /* bytes; 0 for invalid sizes; proportional to B; multiple of 8 */
gp_status gp_stereo_views(const unsigned char* image, const float* pred, const int* conv /* [B] */, const int* views /* HOST [V][4] */, int B,
                          int V, int H, int W, int CH, int CW, int space, int edge, int max_s8, unsigned char* canvas,
                          unsigned char* holes /* or NULL */, unsigned short* near /* or NULL */, void* workspace, long long workspace_bytes,
                          void* stream);

/* ---- camera moves from one photograph: the frames of a "3-D photo" (DEVICE pointers but the frame table; stateless, stream-ordered, no host synchronisation, no global atomics; csrc/parallax.hip) ----
 * The best-known use of a monocular depth map: a short clip in which the camera orbits, swings or pushes into a single still (the 3-D Ken
 * Burns effect).  gp_stereo_views stops at shifts along a row; this entry has parallax in both directions, a zoom per frame, a
 * depth-dependent magnification for the dolly, and a 2-D surface: a triangle mesh over the pixel grid, cut at depth edges, with a z-test.
 * With framework ops this is a grid_sample by the flow, a BACKWARD warp that smears the subject across every depth edge, which is where the
 * eye looks in a moving clip.  The whole definition is integer arithmetic, so the result does not depend on the order of evaluation and the
 * device equals the host route genpercept_amd/parallax.py bit for bit; the arithmetic stands once more in csrc/parallax_math.h.
 * Inputs per image: image uint8 [3][H][W]; pred fp32 [1][H][W]; one int32 F of focus [B], the nearness of the plane that stays put.  Per call:
 *   space = 0 (depth) or 1 (disparity); edge 0 .. 65535; max_s8 0 .. 256, a displacement of at most 32 pixels in eighths of a pixel, which
 *   sizes the staged sources; a HOST table frames int32 [V][4] = (gx, gy, gz, Z) per frame, 1 <= V <= 64, |gx|, |gy| <= 2^17, |gz| <= 2^24,
 *   Z in 65536 .. 131072, a zoom of 1 x to 2 x in units of 1 / 65536.  1 <= H, W <= 16384 and B * V * H * W < 2^31.
 *   Why 32 pixels: a 32 x 32 output tile under displacements of up to A pixels can be reached from (32 + 2 A + 4)^2 sources, 100 x 100 at
 *   A = 32; at 12 bytes each that is 117 KiB, and with the 8 KiB z-buffer it fits the 160 KiB of LDS of a compute unit.  A = 64 does not.
 * 1. Nearness: Q = (uint16)(clamp(pred, 0, 1) * 65535.0f); D = Q in disparity space and D = 65535 - Q in depth space.  A NaN pixel has D = 0.
 *    This is step 1 of gp_stereo_views.
 * 2. Position of source (x, y) in a frame, in eighths of a pixel, with 64-bit intermediates and arithmetic shifts, that is floors:
 *      Cx = 4 (W - 1), Cy = 4 (H - 1); rx = 8 x - Cx, ry = 8 y - Cy; e = D - F; dz = (e gz + 2^23) >> 24;
 *      dx = ((e gx + 2^23) >> 24) + ((rx dz + 2^15) >> 16), clamped to -max_s8 .. max_s8; dy likewise with gy and ry;
 *      tx = Cx + ((rx Z + 2^15) >> 16) + dx; ty = Cy + ((ry Z + 2^15) >> 16) + dy.
 *    Z + dz is the magnification of a pixel: a camera pushed forward magnifies near things more.
 * 3. Pieces.  Two pixels are CONNECTED iff |D_a - D_b| <= edge.  Output pixel (p, q) sits at P = (8 p, 8 q).
 *      Cap: every source has one, the square tx - h <= Px < tx + h, ty - h <= Py < ty + h with h = (4 Z + 65535) >> 16.  It carries D and c
 *        of the source and has the piece id 3 (y W + x).
 *      Triangles: each quad with x + 1 < W and y + 1 < H gives T0 = (x, y), (x + 1, y), (x, y + 1) with id 3 (y W + x) + 1 and
 *        T1 = (x + 1, y), (x + 1, y + 1), (x, y + 1) with id 3 (y W + x) + 2.  A triangle exists iff its three vertex pairs are all
 *        connected.  With the vertices a, b, c in that order A = (b - a) x (c - a); a triangle with A <= 0 covers nothing: it is folded.
 *        wa = (c - b) x (P - b), wb = (a - c) x (P - c), wc = A - wa - wb; the triangle covers P iff all three are >= 0.  The nearness there
 *        is (wa D_a + wb D_b + wc D_c + (A >> 1)) / A and each colour channel likewise, integer divisions.
 * 4. Visibility: the piece with the largest nearness wins; on a tie the smallest piece id.
 * 5. Holes: a pixel that nothing covers looks outwards along its row and its column and takes the nearest covered pixel in each of the four
 *    directions within R = max_s8 / 4 + 1.  Of those it takes the one with the SMALLEST nearness -- the background continues behind the
 *    subject --, ties in the order left, right, up, down, and copies that pixel's colour and nearness; colour 0 and nearness 0 where none
 *    exists.  R is part of the definition, as in gp_stereo_views.
 * 6. Outputs: out uint8 [B][V][3][H][W] (not the image itself); holes uint8 [B][V][H][W] or NULL: 1 marks a disocclusion; near uint16
 *    [B][V][H][W] or NULL: the winning or copied nearness, the frame's own map.
 * F is DEVICE memory so that a plane picked from the map needs no read-back; for the same reason it cannot be refused, and a value outside
 * 0 .. 65535 is clamped.  How a swing, an orbit or a dolly becomes rows of the table is the host's business (parallax.py: camera_path, plan).
 * Two launches for any B and V: a warp pass (a workgroup per 32 x 32 output pixels of a frame stages the sources that can reach the tile in
 * LDS and rasterises their caps and triangles into a z-buffer in LDS by a 64-bit LDS atomic maximum on a packed key -- nearness, inverted
 * piece id, colours --, which is step 4 whatever the order) and a fill pass.  No global atomics, nothing read back; an image's bytes are the
 * same from call to call and in every batch.  workspace: DEVICE scratch of at least the workspace entry's byte count (the
 * nearness-and-covered plane between the two passes), 8-byte aligned, free again once the stream has passed the call.
 * GP_ERR_INVALID before any HIP call: null image / pred / focus / frames / out / workspace, B < 1, B > 65535, V outside 1 .. 64, H or W
 * outside 1 .. 16384, B * V * H * W >= 2^31, space outside 0 .. 1, edge outside 0 .. 65535, max_s8 outside 0 .. 256, |gx| or |gy| > 2^17,
 * |gz| > 2^24, Z outside 65536 .. 131072, pred or focus not 4-byte aligned, near not 2-byte aligned, workspace not 8-byte aligned,
 * workspace_bytes too small, out == image. */
long long gp_parallax_frames_workspace(int B, int V, int H, int W);  /* bytes; 0 for invalid sizes; proportional to B; multiple of 8 */
gp_status gp_parallax_frames(const unsigned char* image, const float* pred, const int* focus /* [B] */, const int* frames /* HOST [V][4] */,
                             int B, int V, int H, int W, int space, int edge, int max_s8, unsigned char* out,
                             unsigned char* holes /* or NULL */, unsigned short* near /* or NULL */, void* workspace,
                             long long workspace_bytes, void* stream);

/* ---- relighting: the photograph under new lights, from its normal and depth maps (DEVICE pointers but the light table; stateless, stream-ordered, no host synchronisation, no atomics; csrc/relight.hip) ----
 * What surface normals are for in a photograph: "portrait lighting", "studio light".  Framework ops do the Lambert term; what makes a relit
 * image look right is that a light from the side is blocked by what stands in front of it -- a nose shadows a cheek, a person the wall --,
 * a march over the depth map per pixel and light.  Here the image is shaded under up to 8 directional lights and an ambient term, diffuse
 * and specular, with screen-space cast shadows, and blended with the original under an optional weight (a matting alpha relights the
 * subject only).  The whole definition is integer arithmetic, so the order of evaluation is free and the device equals the host route
 * genpercept_amd/relight.py bit for bit; the arithmetic stands once more in csrc/relight_math.h.
 * Axes: those of gp_depth_geometry (x right, y down, z away from the camera).  A camera-facing normal has N_z < 0; a light in front of the
 *   scene has L_z < 0.  The projection is orthographic and the view direction (0, 0, -1) at every pixel, a stated convention: an
 *   affine-invariant map has no camera.
 * Inputs per image: image uint8 [3][H][W]; normal fp32 [3][H][W]; pred fp32 [H][W] or NULL (no shadows without it); weight uint8 [H][W] or
 *   NULL.  Per call: encoded = 1 (values in [0, 1], as the pipeline's normal mode writes them) or 0 (values in [-1, 1], as
 *   gp_depth_geometry writes them); flip, 3 bits, bit k negates N_k (a checkpoint trained in another convention); space = 0 (depth) or 1
 *   (disparity); to_lin and from_lin, the DEVICE tables of gp_lens_blur under the same conditions; lights, a HOST table of L + 1 rows of
 *   20 int32 -- L light rows (1 <= L <= 8), then the ambient row; max_reach 0 .. 64, the longest march a row may ask for.  1 <= H, W <=
 *   16384, B <= 65535 and B * H * W < 2^31.
 * A light row: L_x, L_y, L_z, the unit vector TOWARDS the light * 16384; H_x, H_y, H_z, the unit half vector between L and the view
 *   direction * 16384; col_r, col_g, col_b and spc_r, spc_g, spc_b, the diffuse and specular gains in Q8 (256 = 1.0, at most 4096); k, the
 *   specular term is raised to the power 2^k (0 .. 7); ux, uy, the screen step towards the light in 1 / 256 pixel, max(|ux|, |uy|) = 256
 *   where the row has a reach; rise >= 0, the nearness the ray gains per step (at most 65535); bias 0 .. 65535; soft, strength 0 .. 256;
 *   reach 0 .. max_reach steps.  The ambient row: amb_r, amb_g, amb_b in Q12 (4096 = 1.0, at most 65536); its other entries are not read.
 * 1. Normal: N_k = 2 Q(v_k) - 65535 (encoded), Q the 16-bit rule of gp_postprocess, or N_k = (int)(clamp(v_k, -1, 1) * 65535.0f),
 *    truncated (raw); then the sign flips.  m = floor(sqrt(N_x^2 + N_y^2 + N_z^2)), exact (the argument is below 2^34).  A pixel with a NaN
 *    channel or m < 256 has no usable normal and is shaded as facing the camera, N = (0, 0, -65535), m = 65535: the smooth fallback for the
 *    pixels gp_depth_geometry leaves without a fit.
 * 2. Per light j: cos12 = clamp(floor(N . L_j / (4 m)), 0, 4096); s = clamp(floor(N . H_j / (4 m)), 0, 4096), then k_j times
 *    s = (s s + 2048) >> 12.  A light with cos12 = 0 contributes nothing, neither diffuse nor specular nor to the shadow plane.
 * 3. Shadow of light j, where pred is given, the row has a reach, cos12 > 0 and the pixel's pred is not NaN: D is the nearness of
 *    gp_lens_blur step 1 (a NaN pixel has D = 0 and neither casts nor receives a shadow).  For t = 1 .. reach the sample is
 *    q_t = (x + ((t ux + 128) >> 8), y + ((t uy + 128) >> 8)) (floor shifts); samples outside the image do not exist.
 *    e_t = D(q_t) - D(p) - bias - t rise; E = max(0, max_t e_t).  dark = min(256, (E soft + 128) >> 8), or with soft = 0 dark = 256 iff
 *    E > 0 (a hard shadow); shade_j = (dark strength) >> 8; vis_j = 256 - shade_j.  Everywhere else shade_j = 0.
 * 4. Combination in linear light, lin_k = to_lin[image_k]: G_k = amb_k + ((sum_j col_jk cos12_j vis_j) >> 16);
 *    S_k = (sum_j spc_jk s_j vis_j) >> 16; lin'_k = min(4095, ((lin_k G_k + 2048) >> 12) + min(S_k, 4095)); relit_k = from_lin[lin'_k];
 *    out_k = (w relit_k + (255 - w) image_k + 127) / 255 with w the weight, 255 without one.  The image is taken as albedo times its own
 *    light, a convention: ambient 1.0 keeps it and the lights add to it; one white light of gain 1.0 from the camera on a camera-facing
 *    surface with ambient 0 gives G = 4096 and returns the image.
 * Outputs: out uint8 [B][3][H][W] (not the image itself); shadow uint8 [B][H][W] or NULL: min(255, max_j shade_j).
 * One kernel launch for every B and L: a workgroup stages the nearness of its 32 x 16 tile and an apron of the rows' longest reach in LDS as
 * 16-bit words and ends a march where D(p) + bias + t rise reaches the largest D it staged; without pred, or with no row that has a reach,
 * nothing is staged.  No workspace, nothing read back; an image's bytes are the same from call to call and in every batch.
 * GP_ERR_INVALID before any HIP call: null image / normal / lights / to_lin / from_lin / out, B < 1, B > 65535, H or W outside 1 .. 16384,
 * B * H * W >= 2^31, L outside 1 .. 8, encoded outside 0 .. 1, flip outside 0 .. 7, space outside 0 .. 1, max_reach outside 0 .. 64, normal,
 * pred or lights not 4-byte aligned, to_lin not 2-byte aligned, out == image, a value of a light row or of amb outside its range (the table
 * is host memory, so it can be refused). */
gp_status gp_relight(const unsigned char* image, const float* normal, const float* pred /* or NULL */, const unsigned char* weight /* or NULL */,
                     const int* lights /* HOST [L + 1][20] */, const unsigned short* to_lin /* [256] */, const unsigned char* from_lin /* [4096] */,
                     int B, int H, int W, int L, int encoded, int flip, int space, int max_reach, unsigned char* out,
                     unsigned char* shadow /* or NULL */, void* stream);

/* ---- test-time ensembling on the device (DEVICE pointers; stateless, stream-ordered, no host synchronisation, no atomics; csrc/ensemble.hip) ----
 * The tensor half of ensemble_depth (genpercept/util/ensemble.py:43-205, called at genpercept_pipeline.py:289-298) for the E members of each of
 * B images; the optimiser that finds the per-member (scale, shift) runs on the host between the two entries, on what the gather produced.
 * gather: small [B][E][h][w] = the nearest-exact reduction of depth [B][E][H][W] (image_util.resize_max_res with (h, w) from the size rule of
 *   gp_resize_max_res_size; the source index of the nearest-exact resize of gp_preprocess; h == H and w == W: a copy), minmax [B][E][2] = each
 *   reduced member's (min, max).  One launch.
 * reduce, per pixel in float32 without fused multiply-adds: a_e = depth_e * scale_e + shift_e (shift == NULL: scale-only, a_e = depth_e * scale_e);
 *   reduction 0: pred = the element of rank (E - 1) / 2 of the sorted members (torch.median: the lower middle for even E), uncertainty = the
 *   same rank of |a_e - pred|; reduction 1: pred = (sum in member order) / E, uncertainty = the unbiased standard deviation (two passes, divisor
 *   E - 1; NaN for E = 1).  Then per image d_max = max(pred), d_min = min(pred) (0 when shift == NULL), rng = max(d_max - d_min, 1e-6),
 *   pred = (pred - d_min) / rng, uncertainty = uncertainty / rng.  pred, uncertainty: [B][H][W]; uncertainty may be NULL.  1 <= E <= 64,
 *   1 <= B <= 65535, H * W <= 0x7fffffff.  An image's result is bitwise the same alone and inside any batch.  An image with a NaN or an
 *   infinite member has an unspecified result.  workspace: DEVICE scratch of at least the workspace entry's byte count (8-byte aligned), free
 *   again once the stream has passed the call.  Three launches.  Arguments are validated before any HIP call (GP_ERR_INVALID). */
gp_status gp_ensemble_gather(const float* depth, int B, int E, int H, int W, int h, int w, float* small, float* minmax, void* stream);
long long gp_ensemble_workspace(int B, int E, int H, int W);   /* bytes; 0 for B, E, H or W < 1; proportional to B */
gp_status gp_ensemble_reduce(const float* depth, const float* scale, const float* shift, int B, int E, int H, int W, int reduction, float* pred,
                             float* uncertainty, void* workspace, long long workspace_bytes, void* stream);

/* Sustained TFLOP/s of back-to-back v_mfma_f32_32x32x16 (this library's element type) on every CU of `device`: the chip's own MFMA
 * peak under load, reported by bench.py beside the nominal 2.5 PFLOP/s.  < 0 on error. */
double gp_mfma_peak_tflops(int device, void* stream);
/* The same for one MFMA shape: 0 = v_mfma_f32_32x32x16 (the attention kernels), 1 = v_mfma_f32_16x16x32 (the conv / GEMM kernels; K = 32 per
 * instruction moves a quarter of the accumulator registers per flop).  The chip runs against its power budget, so the two sustain different
 * clocks on the same data. */
double gp_mfma_peak_tflops_shape(int device, int shape, void* stream);
/* Measurement probe (r4): TFLOP/s of the conv / GEMM inner loop in isolation -- per wave and iteration 16 independent
 * v_mfma_f32_16x16x32 plus `reads_per_16_mfma` (0, 2, 4, 8 or 16) conflict-free ds_read_b128 refilling the other fragment set -- at
 * `waves_per_simd` (1, 2 or 4) waves per SIMD on every CU.  mode 0: nothing else (how much of a fragment read's LDS -> register return overlaps
 * with matrix work on the same SIMD); mode bits (8 reads, 2 waves per SIMD only) add the real kernels' other ingredients per 32-MFMA step:
 * 1 = one s_barrier, 2 = the weight stream (16 KiB per workgroup by LDS-DMA into a 3-deep ring, counted vmcnt), 4 = weight fragments read from
 * that ring, 8 = the DMA as buffer_load ... lds, 16 = the halo stream (48 KiB per workgroup every ninth step from HBM).  < 0 on error or an
 * unsupported combination (csrc/microbench.hip lists them). */
double gp_mfma_lds_probe(int device, int reads_per_16_mfma, int waves_per_simd, int mode, void* stream);

/* ---- per-kernel entry points (DEVICE pointers, bf16 NHWC activations) -------------------------------------------- */
/* Pack an OIHW fp32 HOST weight into the device layout [n_rows][taps][cin_pad] bf16 (n_rows = gp_packed_rows(cout)). */
int gp_packed_rows(int cout);
gp_status gp_pack_weight(const float* w_oihw_host, int cout, int cin, int ks, int cin_pad, int geglu, void* dev_out);
/* x2-nearest-upsample 3x3 conv (Upsample2D, resnet.py of diffusers: F.interpolate(scale_factor=2, mode="nearest") then conv; call sites
 * custom_unet.py:372-400 up blocks, VAE decoder up blocks) as four 2 x 2-tap phase convolutions on the source map: gp_pack_weight_phases sums the kernel
 * rows / columns that fall onto the same source pixel ([rows][phase 2a+b][tap 2ty+tx][cin_pad], rows = gp_packed_rows(cout)); gp_conv2d_up2 runs
 * the phase kernel (w_packed = the ordinary 3x3 packing of the same weight, for the launcher's checks).  Test entry points. */
gp_status gp_pack_weight_phases(const float* w_oihw_host, int cout, int cin, int cin_pad, void* dev_out);
gp_status gp_conv2d_up2(const void* in, const void* w_packed, const void* w_phases, const float* bias, const void* residual, void* out, int B, int Hi,
                        int Wi, int Cin, int Cout, void* stream);
/* the same with the GroupNorm statistics of the tensor it writes (the phase kernel's per-(tile, phase) partial sums and pixel counts, what the VAE
 * decoder's upsampler convs leave for the next resnet's norm1), finalised to scale / shift like gp_conv2d_stats.  Test entry point. */
gp_status gp_conv2d_up2_stats(const void* in, const void* w_packed, const void* w_phases, const float* bias, const void* residual, void* out, int B, int Hi,
                              int Wi, int Cin, int Cout, const float* gamma, const float* beta, int groups, float eps, float* scale_out, float* shift_out,
                              void* stream);
gp_status gp_conv2d(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int Hi, int Wi, int Cin,
                    int Cout, int ks, int stride, int pad_t, int pad_l, int Ho, int Wo, int ups_h, int ups_w, int act, int n_store,
                    int out_fp32, int tile_hint, void* stream);
/* conv3x3(act(GroupNorm(in))) with the normalisation applied inside the conv kernel (statistics pass + fused apply);
 * stride 1, pad 1, optional nearest x2 upsample of the normalised input; H, W >= 16 (x2: >= 8). */
gp_status gp_conv2d_gn(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int H, int W, int Cin,
                       int Cout, int ups, int act, const float* gamma, const float* beta, int groups, float eps, int silu, void* stream);
/* VAE-encoder conv_in fused with the RGB prologue of GenPerceptPipeline.__call__ (genpercept_pipeline.py:245, x / 255 * 2 - 1) :
 * rgb [B][3][H][W] on the device (uint8 when is_u8, else float already in [-1,1]) -> conv3x3(pad 1, 3 -> Cout) + bias -> NHWC bf16.
 * w_packed: gp_pack_weight(.., cout, 3, 3, 64, 0, ..).  Cout % 32 == 0. */
gp_status gp_rgb_conv_in(const void* rgb, int is_u8, const void* w_packed, const float* bias, void* out, int B, int H, int W, int Cout, void* stream);
/* conv (3x3 pad 1 or 1x1, stride 1, optional nearest x2 upsample) whose epilogue also leaves the GroupNorm statistics of the tensor it
 * writes (per-tile channel sums), finalised to the affine form the next GroupNorm applies: scale[b][c] = gamma[c] * rstd[b][g(c)],
 * shift[b][c] = beta[c] - mean[b][g(c)] * scale[b][c].  This is how the engine skips the statistics read pass of
 * diffusers' ResnetBlock2D.norm2 / the following block's norm1 (resnet.py forward: norm -> nonlinearity -> conv).
 * Returns GP_ERR_INVALID when the selected kernel cannot produce statistics for this shape. */
gp_status gp_conv2d_stats(const void* in, const void* w_packed, const float* bias, const void* residual, void* out, int B, int H, int W, int Cin,
                          int Cout, int ks, int ups, int tile_hint, const float* gamma, const float* beta, int groups, float eps,
                          float* scale_out, float* shift_out, void* stream);
/* out[M][N] = A[M][K] * Bt[N][K]^T (+bias per column / per row), batched over `batch` with element strides. */
gp_status gp_gemm(const void* a, int lda, const void* bt, int ldb, const float* bias, int bias_mode, const void* residual, int ldres, void* out,
                  int ldo, int M, int N, int K, int n_rows_bt, int n_store, int act, int out_fp32 /* 0 bf16, 1 fp32, 2 fp16 */, int batch, long long a_bs, long long bt_bs,
                  long long out_bs, int tile_hint, void* stream);
/* Test entry point: the kernel the last conv / GEMM launcher call (gp_conv2d, gp_conv2d_up2, gp_conv2d_gn, gp_conv2d_stats, gp_gemm, gp_gemm_qkv,
 * gp_c_conv2d) of the CALLING host thread dispatched to, with the numbering of gp_c_conv2d's path_out; with the persistent GEMM (3) also its
 * row tile (128 or 256) in *pgemm_rows (0 otherwise).  Reading clears it: 0 = no such launch since the previous call. */
int gp_last_igemm_path(int* pgemm_rows);
/* The VAE decoder's tail in one kernel (diffusers AutoencoderKL.decoder conv_norm_out -> SiLU -> conv_out, call site
 * genpercept_pipeline.py:521-522; channel mean :523-525; clip / shift :469-472): in NHWC [B][H][W][128] (this library's element type),
 * w_packed = gp_pack_weight(conv_out.weight [3][128][3][3]), GroupNorm(groups, eps) statistics computed here, out fp32 NCHW
 * [B][mean3 ? 1 : 3][H][W]; raw = 1: no clip / shift (decode_pred alone).  Cin must be 128 (GP_ERR_INVALID otherwise). */
gp_status gp_decoder_tail(const void* in, const void* w_packed, const float* bias, const float* gamma, const float* beta, int groups, float eps,
                          int B, int H, int W, int Cin, int mean3, int raw, float* out, void* stream);
/* The self-attention input projections of a BasicTransformerBlock (attn1.to_q / to_k / to_v, bias-free in SD2.1; custom_unet.py's
 * Transformer2DModel blocks) as ONE GEMM over the stacked weight [3C][K] (gp_pack_weight of the concatenation): q | k go to qk_out
 * [B*T][2C] row-major, V goes to vt_out TRANSPOSED as [B][C][Tpad] (zero beyond T) -- the operand layout of gp_flash_attention.
 * Requirements: K % 64 == 0, (2C) % 128 == 0, T % 16 == 0, Tpad % 8 == 0, B*T >= 256; GP_ERR_INVALID otherwise (use gp_gemm twice). */
gp_status gp_gemm_qkv(const void* a, int lda, const void* w_packed, int ldw, int n_rows_w, int K, void* qk_out, void* vt_out, int B, int T, int C,
                      int Tpad, void* stream);
gp_status gp_groupnorm(const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int silu, void* stream);
gp_status gp_layernorm(const void* x, void* y, const float* gamma, const float* beta, int rows, int C, float eps, void* stream);
gp_status gp_flash_attention(const void* q, const void* k, const void* vt, void* out, int B, int T, int heads, int ldq, int ldk, int Tpad, int ldo,
                             void* stream);
/* Contract precision (gp_set_precision; csrc/contract.hip, attention.hip: flash_attn64_split_kernel): the UNet's self-attention core over SPLIT operands.
 * qkv: DEVICE fp32 [B*T][ld] with q | k | v at columns 0 | C | 2C (C = heads * 64; the output of the stacked attn1.to_q / to_k / to_v projection);
 * out_split: DEVICE 16-bit [B*T][3C] = the A-order split operand [hi | lo | hi] of softmax(q k^T / 8) v that the output projection reads (value = hi + lo).
 * ld % 4 == 0 and 16-byte aligned qkv / out_split (GP_ERR_INVALID otherwise).  bf16 library only.  Synchronises the stream (test entry point). */
gp_status gp_flash_attention_split(const float* qkv, int ld, void* out_split, int B, int T, int heads, void* stream);
/* The same for the VAE mid-block attention (one head, head_dim 512; attention.hip: flash_attn512_split_kernel): qkv DEVICE fp32 [B*T][ld] with
 * q | k | v at columns 0 | 512 | 1024, out_split 16-bit [B*T][1536] = [hi | lo | hi] of softmax(scale q k^T) v; scores and probabilities stay
 * on the CU, no workspace beyond the operand planes (6 KiB per token).  Any B >= 1, T >= 1 (T < 2^21); ld >= 1536, ld % 4 == 0, 16-byte aligned
 * qkv / out_split (GP_ERR_INVALID otherwise, before anything is launched).  bf16 library only.  Synchronises the stream (test entry point). */
gp_status gp_flash_attention_hd512_split(const float* qkv, int ld, void* out_split, int B, int T, float scale, void* stream);
/* Which way the contract precision's attention core goes for B images of T tokens, heads x hd, with the GENPERCEPT_* switches as the
 * environment has them now, and the transient workspace of that way in bytes.  path: 0 unfused (logits + probabilities in device memory,
 * 10 * B * heads * T * Tpad bytes), 1 flash_attn64_split (hd 64), 2 flash_attn512_split (one head of 512; see gp_set_precision); for 1 and 2
 * the workspace is the hi / lo operand planes, 8 * B * T * heads * hd + 4 * B * heads * hd * Tpad bytes.  Host arithmetic only. */
gp_status gp_c_attention_plan(int B, int T, int heads, int hd, int* path, long long* workspace_bytes);
/* ---- contract-precision test entry points (bf16 library only; GP_ERR_INVALID from the fp16 library) -------------------------------------------
 * The launchers the engine's contract path uses (csrc/contract.hip), with every argument checked on the host first: fp32 rows with ld % 4 == 0,
 * 16-byte aligned pointers.  A "split" operand is 16-bit [rows][3 C]: A order [hi | lo | hi], B order [hi | hi | lo], hi = bf16(x), lo = bf16(x - hi).
 * gp_c_split3: out = split(act(x * scale)) (act: none or ReLU, the engine's split_operand).
 * gp_c_groupnorm_split: GroupNorm(G, eps) (+ SiLU) of fp32 NHWC x [B][HW][C] -> A-order split out; the centred statistics pass and the finaliser
 *   also leave the affine form in scale_out / shift_out [B][C] (DEVICE fp32): y = x * scale + shift.
 * gp_pack_weight_split / gp_pack_weight_phases_split: gp_pack_weight / gp_pack_weight_phases in B order (3 cin_pad elements per tap).
 * gp_c_conv2d: conv (3x3 or 1x1, stride 1 or 2, optional nearest x2 upsample with the phase packing in w_phases) or linear (ks = 1; act may be
 *   GEGLU) on an A-order split input [B][Hi][Wi][3 Cin], fp32 out [B][Ho][Wo][Cout or Cout / 2] (+ bias, + fp32 residual; residual may be out);
 *   with gamma non-null also the GroupNorm scale / shift of the output as the engine computes them.  The launch parameters are the engine's own
 *   (conv_c; linear_c for ks = 1 without stride / upsample).  path_out (optional) reports the kernel launch_igemm dispatched to: 1 halo conv
 *   with 16-row tiles, 2 halo phase conv, 3 persistent GEMM, 4 conv_img + split-K reduce, 5 split-K igemm + reduce, 6 igemm, 7 halo conv with
 *   12-row tiles, 8 per-tile halo conv.
 * gp_c_layernorm_split: LayerNorm over the last dim of fp32 [rows][C] -> A-order split.
 * gp_c_softmax_split: row softmax of scale * x over the first T of ld columns -> A-order split probabilities [rows][3 ld] (zero beyond T). */
gp_status gp_c_split3(const float* x, int ldx, void* out, long long rows, int C, int b_order, int act, float scale, void* stream);
gp_status gp_c_groupnorm_split(const float* x, void* out, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int silu,
                               float* scale_out, float* shift_out, void* stream);
gp_status gp_pack_weight_split(const float* w_oihw_host, int cout, int cin, int ks, int cin_pad, int geglu, void* dev_out);
gp_status gp_pack_weight_phases_split(const float* w_oihw_host, int cout, int cin, int cin_pad, void* dev_out);
gp_status gp_c_conv2d(const void* in_split, const void* w_packed, const void* w_phases, const float* bias, const float* residual, float* out, int B,
                      int Hi, int Wi, int Cin, int Cout, int ks, int stride, int pad_t, int pad_l, int Ho, int Wo, int ups, int act, int tile_hint,
                      const float* gamma, const float* beta, int groups, float eps, float* scale_out, float* shift_out, int* path_out, void* stream);
gp_status gp_c_layernorm_split(const float* x, void* out, const float* gamma, const float* beta, int rows, int C, float eps, void* stream);
gp_status gp_c_softmax_split(const float* in, void* out, int rows, int T, int ld, float scale, void* stream);
/* The VAE mid-block attention's core (one head, head_dim 512; diffusers Attention inside AutoencoderKL, call sites
 * genpercept_pipeline.py:500-501,521-522), fused: softmax(scale * q k^T) v with scores and probabilities kept on the CU.  q, k: [B][T][ld]
 * (512 channels), vt: [B][512][Tpad] zero beyond T, out [B][T][ldo].  ncu: persistent workgroups to size the launch for (0 = the device's CU
 * count; the parity tests pass small values to exercise the key-split of the left-over query blocks). */
gp_status gp_flash_attention_hd512(const void* q, const void* k, const void* vt, void* out, int B, int T, int ldq, int ldk, int Tpad, int ldo,
                                   float scale, int ncu, void* stream);
gp_status gp_cross_attention(const void* q, const float* kc, const float* vc, void* out, int rows, int C, int L, void* stream);
/* BasicTransformerBlock.attn2 (+ norm2, + residual, + norm3 of the result) for a TWO-token context, folded into per-head vectors
 * (gp_set_context does the fold for the engine; csrc/norm.hip states the algebra): y_out = y + c0 + sum_h sigmoid(LNhat(y) . U[h] + u0[h]) G[h],
 * n3_out = LayerNorm(y_out; g3, b3) (optional).  U, G: [heads][C] fp32, u0 [heads], c0 / g3 / b3 [C]; y_out may alias y. */
gp_status gp_cross_attention_fold(const void* y, void* y_out, void* n3_out, const float* U, const float* u0, const float* G, const float* c0,
                                  const float* g3, const float* b3, int rows, int C, int heads, float eps, void* stream);
gp_status gp_softmax_rows(const float* in, void* out, int rows, int T, int ld, float scale, void* stream);
/* the same for fp16 logits (gp_gemm with out_fp32 = 2 writes them): ld % 4 == 0, ld <= 16384 */
gp_status gp_softmax_rows_f16(const void* in_f16, void* out, int rows, int T, int ld, float scale, void* stream);
gp_status gp_bilinear(const void* in, void* out, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);

/* ---- test entry points of the elementwise / layout kernels between the matrix products (csrc/elementwise.hip) and, with contract != 0, of their
 * fp32 twins of the contract precision (csrc/contract.hip; bf16 library only, GP_ERR_INVALID from the fp16 library).  Stateless, on the
 * caller's stream, DEVICE pointers; "16-bit" = this library's element type.  Whatever a kernel would fault on is refused with GP_ERR_INVALID
 * before any HIP call: null pointers, pointers that are not 16-byte aligned where the kernel moves 16-byte vectors, channel counts that are
 * no multiple of the vector (8 elements, fp32 twins 4), strides smaller than what is read or written.
 * gp_rgb_prologue: rgb [B][3][H][W] (uint8, or float in [-1, 1]) -> 16-bit NHWC [B*H*W][Cpad], x / 255 * 2 - 1 in fp32 in that order, channels
 *   3 .. Cpad-1 zero (Cpad % 8 == 0); contract: the A-order split operand [B*H*W][192] of 64 logical channels (Cpad must be 64).
 * gp_concat: out[p] = [a[p][0..Ca) | b[p][0..Cb)] (the UNet's [hidden, skip]).
 * gp_concat_stats: the same copy (16-bit only) that also leaves per-(bm pixels, channel) GroupNorm partials; bm = 0 takes gp_concat_stats_bm's
 *   choice, *bm_used (optional) reports it, HW % bm == 0 is required.  With gamma non-null the partials are finalised to scale / shift [B][C] as
 *   gp_conv2d_stats does.  gp_concat_stats_bm: host arithmetic, 0 = no tile size divides hw.
 * gp_rgb_conv_in_stats: gp_rgb_conv_in with the statistics rows its persistent workgroups leave, finalised to scale / shift [B][Cout].
 * gp_nchw_to_nhwc: fp32 NCHW -> NHWC [B*H*W][Cpad] (16-bit, or fp32 with contract), channels >= C zero.  gp_nhwc_to_nchw: NHWC rows of stride ld -> fp32 NCHW.
 * gp_ddim_init / gp_ddim_update: the state kernels of the multi-step archs.  init: sample [B*H*W][L] fp32 = noise (NCHW) and lat[p][off .. off+L) =
 *   its copy in the tensor's type, or with noise null sample = lat[p][0..L) widened; off + L <= ld.  update: one scheduler step in the affine form
 *   of gp_ddim_step, coef7_host = HOST {x0_sample, x0_model, eps_sample, eps_model, prev_x0, prev_eps, clip}; model rows of stride ldm, the new
 *   sample also into uin[p][off .. off+L) (stride ldu, off + L <= ldu) and x0 into x0_out[p][0..L) (optional, stride ldx).
 * gp_decode_epilogue: NHWC (3 real channels, stride ld; 16-bit: ld % 4 == 0 and an 8-byte aligned tensor) -> fp32 NCHW [B][mean3 ? 1 : 3][H][W],
 *   channel mean, then unless raw clip(-1, 1), + 1, * 0.5.
 * gp_scale_pad: out[p][0..ldo) = {in[p][0..C) * scale, 0 ...}.  gp_pointwise_small: out[p][0..ldo) = {W (in[p][0..Cin) * in_scale) + bias, 0 ...},
 *   W [Cout][Cin] fp32, 1 <= Cin, Cout <= 8, bias optional.  gp_relu, gp_add: n elements, n % 8 == 0 (fp32 gp_add: % 4).
 * gp_dpt_final: out[p] = sum_c w[c] in[p][c] + bias, fp32 out.  gp_minmax_norm: x[b][0..n) <- (x - min_b) / (max_b - min_b) in place, per image. */
gp_status gp_rgb_prologue(const void* rgb, int is_u8, void* out, int B, int H, int W, int Cpad, int contract, void* stream);
gp_status gp_concat(const void* a, int Ca, const void* b, int Cb, void* out, long long pixels, int contract, void* stream);
int gp_concat_stats_bm(long long hw, long long pixels, int channels);
gp_status gp_concat_stats(const void* a, int Ca, const void* b, int Cb, void* out, int B, int HW, int bm, int* bm_used, const float* gamma, const float* beta,
                          int groups, float eps, float* scale_out, float* shift_out, void* stream);
gp_status gp_rgb_conv_in_stats(const void* rgb, int is_u8, const void* w_packed, const float* bias, void* out, int B, int H, int W, int Cout, const float* gamma,
                               const float* beta, int groups, float eps, float* scale_out, float* shift_out, void* stream);
gp_status gp_nchw_to_nhwc(const float* in, void* out, int B, int C, int H, int W, int Cpad, int contract, void* stream);
gp_status gp_nhwc_to_nchw(const void* in, float* out, int B, int C, int H, int W, int ld, int contract, void* stream);
gp_status gp_ddim_init(const float* noise_nchw, void* lat, float* sample, int B, int H, int W, int L, int ld, int off, int contract, void* stream);
gp_status gp_ddim_update(const void* model, int ldm, float* sample, void* uin, int ldu, int off, void* x0_out, int ldx, long long pixels, int L,
                         const float* coef7_host, int contract, void* stream);
gp_status gp_decode_epilogue(const void* in, float* out, int B, int H, int W, int ld, int mean3, int raw, int contract, void* stream);
gp_status gp_scale_pad(const void* in, void* out, long long pixels, int C, int ldi, int ldo, float scale, void* stream);
gp_status gp_pointwise_small(const void* in, void* out, const float* w, const float* bias, long long pixels, int Cin, int Cout, int ldi, int ldo, float in_scale,
                             int contract, void* stream);
gp_status gp_relu(const void* in, void* out, long long n, void* stream);
gp_status gp_add(const void* a, const void* b, void* out, long long n, int contract, void* stream);
gp_status gp_dpt_final(const void* in, const float* w, float bias, float* out, int B, int HW, int Cin, int contract, void* stream);
gp_status gp_minmax_norm(float* x, int B, long long n, void* stream);
/* contract precision only (bf16 library).  gp_c_heads_split: qkv fp32 [B*T][ld] (q | k | v at columns 0 | C | 2C, C = heads * hd) -> Qs [B*heads][T][3 hd]
 * A order, Ks the same in B order, Vts [B*heads][hd][3 Tpad] B order, V TRANSPOSED, zero in [T, Tpad); hd % 64 == 0, Tpad % 64 == 0, Tpad >= T.
 * gp_c_heads_merge_split: O fp32 [B*heads][T][hd] -> A-order split [B*T][3 heads hd].  gp_c_cross_fold: gp_cross_attention_fold on fp32 rows (C % 8 == 0,
 * C <= 2048), n3_out the A-order split of LayerNorm(y_out).  gp_c_cross_attention: gp_cross_attention on fp32 q, A-order split out.  gp_c_bilinear:
 * gp_bilinear on fp32 NHWC (C % 4 == 0). */
gp_status gp_c_heads_split(const float* qkv, int ld, void* Qs, void* Ks, void* Vts, int B, int T, int Tpad, int heads, int hd, void* stream);
gp_status gp_c_heads_merge_split(const float* O, void* out, int B, int T, int heads, int hd, void* stream);
gp_status gp_c_cross_fold(const float* y, float* y_out, void* n3_out, const float* U, const float* u0, const float* G, const float* c0, const float* g3,
                          const float* b3, int rows, int C, int heads, float eps, void* stream);
gp_status gp_c_cross_attention(const float* q, const float* kc, const float* vc, void* out, int rows, int C, int L, void* stream);
gp_status gp_c_bilinear(const float* in, float* out, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENPERCEPT_HIP_H */
