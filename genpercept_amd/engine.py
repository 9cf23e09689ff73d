"""ctypes binding of libgenpercept_hip.so (include/genpercept_hip.h).  PyTorch-ROCm tensors are used for device memory
and streams only; every tensor operation of the hot path runs in the HIP library.  There is NO fallback: if the library
is missing or fails to load, importing the engine raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .eval_metrics import (BAND_METRIC, BAND_PLANES, BOUNDARY_METRICS, MASK_METRICS, MATTING_METRICS, SEG_MAX_K, SEG_METRICS,  # noqa: F401
                           STRUCTURE_METRICS, TRIMAP_METRICS)  # the names of the evaluators' values: one list each, stated in eval_metrics
from .post_common import F_DEFAULT, MAX_DIM, SPACES, _pixel_inside, _with_planes

_HERE = os.path.dirname(os.path.abspath(__file__))
# One library per 16-bit element type (csrc/common.h): identical C-ABI, bf16 or IEEE fp16 activations / weights / MFMA operands.
# "bf16" is the default (BASELINE.json's dtype); "fp16" is the reference's half precision (run.py --half_precision), 8x finer
# rounding at the same speed (inside north_star's 1e-3 under the mean-absolute reading on benign weights only); the build that meets the
# tolerance under both readings is the contract precision below.
LIB_PATHS = {"bf16": os.path.join(_HERE, "lib", "libgenpercept_hip.so"), "fp16": os.path.join(_HERE, "lib", "libgenpercept_hip_f16.so")}
LIB_PATH = LIB_PATHS["bf16"]
ELT_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
# Engine precisions: the two element-type libraries in their native arithmetic, and "fp32c" = the CONTRACT precision of the bf16 library
# (`gp_set_precision(GP_PREC_CONTRACT)`: fp32 storage, split-bf16 MFMA operands, csrc/contract.hip) -- what torch_dtype=float32 selects.
ENGINE_PRECISIONS = {"bf16": ("bf16", 0), "fp16": ("fp16", 0), "fp32c": ("bf16", 1)}
_default_precision = "bf16"


def set_default_precision(precision: str):
    """Element type used by the per-kernel wrappers below (tests); engines name theirs explicitly."""
    global _default_precision
    assert precision in LIB_PATHS
    _default_precision = precision


def act_dtype(precision: Optional[str] = None) -> torch.dtype:
    return ELT_DTYPE[precision or _default_precision]


def precision_of(dtype) -> str:
    """torch dtype a caller asks for (from_pretrained(torch_dtype=...), .to(dtype=...)) -> engine precision: bf16 -> "bf16", fp16 -> "fp16"
    (the reference's --half_precision), fp32 -> "fp32c" (the reference's default, run.py:273-281: fp32 storage + split-bf16 matrix products,
    inside north_star's 1e-3 under both readings)."""
    if dtype is None or dtype == torch.bfloat16:
        return "bf16"
    if dtype == torch.float16:
        return "fp16"
    if dtype == torch.float32:
        return "fp32c"
    raise ValueError(f"unsupported dtype {dtype}")

GP_OK = 0
GP_ERR_INVALID = 1
MODES = {"depth": 0, "normal": 1, "seg": 2, "matting": 3, "dis": 4, "disparity": 5}
ONE_CHANNEL_MODES = ("depth", "matting", "dis", "disparity")  # genpercept_pipeline.py:523
ACT = {"none": 0, "silu": 1, "relu": 2, "geglu": 3}
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


class GpConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int),
        ("unet_in_channels", C.c_int), ("unet_out_channels", C.c_int),
        ("unet_block_out", C.c_int * 4), ("unet_num_heads", C.c_int * 4), ("unet_down_attn", C.c_int * 4),
        ("unet_layers_per_block", C.c_int), ("unet_cross_dim", C.c_int), ("unet_has_out", C.c_int), ("unet_norm_eps", C.c_float),
        ("vae_block_out", C.c_int * 4), ("vae_layers_per_block", C.c_int), ("vae_latent_channels", C.c_int),
        ("vae_norm_eps", C.c_float), ("vae_scaling_factor", C.c_float),
        ("dpt_enabled", C.c_int), ("dpt_neck", C.c_int * 4), ("dpt_fusion", C.c_int),
        ("norm_groups", C.c_int),
    ]


class GpTimings(C.Structure):
    _fields_ = [
        ("ms_encode", C.c_float), ("ms_unet", C.c_float), ("ms_head", C.c_float), ("ms_total", C.c_float),
        ("flops_igemm", C.c_double), ("flops_attn", C.c_double),
        ("ms_igemm", C.c_float), ("ms_attn", C.c_float),
        ("n_igemm", C.c_int), ("n_attn", C.c_int), ("n_launches", C.c_int),
        ("flops_halo", C.c_double), ("ms_halo", C.c_float), ("n_halo", C.c_int),
    ]


_libs: Dict[str, C.CDLL] = {}

# (name, restype, argtypes) for every symbol include/genpercept_hip.h declares
_vp, _i, _f, _ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
class GpDdimStep(C.Structure):
    """`gp_ddim_step` (include/genpercept_hip.h)."""
    _fields_ = [(n, C.c_float) for n in ("timestep", "x0_sample", "x0_model", "eps_sample", "eps_model", "prev_x0", "prev_eps", "clip")]


SYMBOLS = {
    "gp_default_config": (None, [C.POINTER(GpConfig)]),
    "gp_create": (_i, [C.POINTER(GpConfig), C.POINTER(_vp)]),
    "gp_destroy": (None, [_vp]),
    "gp_last_error": (C.c_char_p, [_vp]),
    "gp_version": (C.c_char_p, []),
    "gp_abi_version": (_i, []),
    "gp_set_precision": (_i, [_vp, _i]),
    "gp_get_precision": (_i, [_vp]),
    "gp_element_dtype": (_i, []),
    "gp_load_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i, _i]),
    "gp_set_context": (_i, [_vp, _vp, _i, _i]),
    "gp_set_timestep": (_i, [_vp, _f]),
    "gp_finalize": (_i, [_vp]),
    "gp_infer": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "gp_infer_steps": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "gp_vae_encode": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "gp_unet": (_i, [_vp, _vp, _i, _i, _i, _vp, C.POINTER(_vp), _vp]),
    "gp_vae_decode": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "gp_dpt_head": (_i, [_vp, C.POINTER(_vp), _i, _i, _i, _vp, _vp]),
    "gp_vae_mid_attention": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "gp_set_profile": (_i, [_vp, _i]),
    "gp_get_timings": (_i, [_vp, C.POINTER(GpTimings)]),
    "gp_reset_timings": (_i, [_vp]),
    "gp_halo_executed_flops": (_i, [_vp, C.POINTER(C.c_double)]),
    "gp_saturation_events": (_i, [_vp, C.POINTER(C.c_longlong), _i]),
    "gp_pool_bytes": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "gp_get_launch_log": (_i, [_vp, C.c_char_p, _i]),
    "gp_packed_rows": (_i, [_i]),
    "gp_last_igemm_path": (_i, [C.POINTER(_i)]),
    "gp_latent_size": (_i, [_i]),
    "gp_dpt_out_size": (_i, [_i]),
    "gp_pack_weight": (_i, [_vp, _i, _i, _i, _i, _i, _vp]),
    "gp_pack_weight_phases": (_i, [_vp, _i, _i, _i, _vp]),
    "gp_conv2d_up2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gp_conv2d_up2_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "gp_conv2d": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 17 + [_vp]),
    "gp_conv2d_gn": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _vp, _i, _f, _i, _vp]),
    "gp_rgb_conv_in": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gp_conv2d_stats": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 8 + [_vp, _vp, _i, _f, _vp, _vp, _vp]),
    "gp_gemm": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _ll, _ll, _ll, _i, _vp]),
    "gp_decoder_tail": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _f, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "gp_gemm_qkv": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gp_groupnorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "gp_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "gp_flash_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_flash_attention_split": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "gp_flash_attention_hd512_split": (_i, [_vp, _i, _vp, _i, _i, _f, _vp]),
    "gp_c_attention_plan": (_i, [_i, _i, _i, _i, C.POINTER(_i), C.POINTER(C.c_longlong)]),
    "gp_c_split3": (_i, [_vp, _i, _vp, _ll, _i, _i, _i, _f, _vp]),
    "gp_c_groupnorm_split": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp]),
    "gp_pack_weight_split": (_i, [_vp, _i, _i, _i, _i, _i, _vp]),
    "gp_pack_weight_phases_split": (_i, [_vp, _i, _i, _i, _vp]),
    "gp_c_conv2d": (_i, [_vp] * 6 + [_i] * 14 + [_vp, _vp, _i, _f, _vp, _vp, C.POINTER(_i), _vp]),
    "gp_c_layernorm_split": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "gp_c_softmax_split": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "gp_flash_attention_hd512": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "gp_cross_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "gp_resize_max_res_size": (None, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "gp_preprocess": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "gp_preprocess_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "gp_postprocess": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "gp_eval_depth_workspace": (_ll, [_i, _i, _i]),
    "gp_eval_depth": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _ll, _vp]),
    "gp_eval_normal_workspace": (_ll, [_i, _i, _i]),
    "gp_eval_normal": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gp_eval_mask_workspace": (_ll, [_i, _i, _i]),
    "gp_eval_mask": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gp_eval_structure_workspace": (_ll, [_i, _i, _i]),
    "gp_eval_structure": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gp_eval_matting_workspace": (_ll, [_i, _i, _i]),
    "gp_eval_matting": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gp_seg_decode": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gp_eval_seg_workspace": (_ll, [_i, _i, _i, _i]),
    "gp_eval_seg": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gp_mask_band_workspace": (_ll, [_i, _i, _i]),
    "gp_mask_band": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gp_foreground_workspace": (_ll, [_i, _i, _i]),
    "gp_foreground": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "gp_guided_upsample_workspace": (_ll, [_i, _i, _i, _i]),
    "gp_guided_upsample": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, C.c_double, _vp, _vp, _ll, _vp]),
    "gp_tile_merge_workspace": (_ll, [_i] * 8),
    "gp_tile_merge": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gp_depth_geometry_workspace": (_ll, [_i] * 4),
    "gp_depth_geometry": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_double, _i, C.c_double, _i] + [_vp] * 9 + [_ll, _vp]),
    "gp_depth_mesh_workspace": (_ll, [_i] * 4),
    "gp_depth_mesh": (_i, [_vp] * 4 + [_i] * 4 + [C.c_double] + [_vp] * 9 + [_ll, _vp]),
    "gp_lens_blur": (_i, [_vp] * 6 + [_i] * 5 + [_vp] * 3),
    "gp_stereo_views_workspace": (_ll, [_i] * 4),
    "gp_stereo_views": (_i, [_vp] * 4 + [_i] * 9 + [_vp] * 4 + [_ll, _vp]),
    "gp_parallax_frames_workspace": (_ll, [_i] * 4),
    "gp_parallax_frames": (_i, [_vp] * 4 + [_i] * 7 + [_vp] * 4 + [_ll, _vp]),
    "gp_relight": (_i, [_vp] * 7 + [_i] * 8 + [_vp] * 3),
    "gp_ensemble_gather": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gp_ensemble_workspace": (_ll, [_i, _i, _i, _i]),
    "gp_ensemble_reduce": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp]),
    "gp_mfma_peak_tflops": (C.c_double, [_i, _vp]),
    "gp_mfma_peak_tflops_shape": (C.c_double, [_i, _i, _vp]),
    "gp_mfma_lds_probe": (C.c_double, [_i, _i, _i, _i, _vp]),
    "gp_cross_attention_fold": (_i, [_vp] * 9 + [_i, _i, _i, _f, _vp]),
    "gp_softmax_rows": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "gp_softmax_rows_f16": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "gp_bilinear": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_rgb_prologue": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "gp_concat": (_i, [_vp, _i, _vp, _i, _vp, _ll, _i, _vp]),
    "gp_concat_stats_bm": (_i, [_ll, _ll, _i]),
    "gp_concat_stats": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, C.POINTER(_i), _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "gp_rgb_conv_in_stats": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "gp_nchw_to_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_nhwc_to_nchw": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_ddim_init": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_ddim_update": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _i, _ll, _i, C.POINTER(_f), _i, _vp]),
    "gp_decode_epilogue": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "gp_scale_pad": (_i, [_vp, _vp, _ll, _i, _i, _i, _f, _vp]),
    "gp_pointwise_small": (_i, [_vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _f, _i, _vp]),
    "gp_relu": (_i, [_vp, _vp, _ll, _vp]),
    "gp_add": (_i, [_vp, _vp, _vp, _ll, _i, _vp]),
    "gp_dpt_final": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _vp]),
    "gp_minmax_norm": (_i, [_vp, _i, _ll, _vp]),
    "gp_c_heads_split": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gp_c_heads_merge_split": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "gp_c_cross_fold": (_i, [_vp] * 9 + [_i, _i, _i, _f, _vp]),
    "gp_c_cross_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "gp_c_bilinear": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
}


def load_library(precision: Optional[str] = None, path: Optional[str] = None):
    """dlopen the HIP library of the given element type and bind every C-ABI symbol.  Raises (never falls back) when it is missing."""
    precision = precision or _default_precision
    if precision in _libs and path is None:
        return _libs[precision]
    path = path or (os.environ.get("GENPERCEPT_HIP_LIB") if precision == "bf16" else None) or LIB_PATHS[precision]
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -m genpercept_amd.build` (hipcc, gfx950). "
                          "There is no CPU/PyTorch fallback for the inference path.")
    lib = C.CDLL(path)  # RTLD_LOCAL: the two libraries export the same symbol names
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.gp_element_dtype() != _DT[ELT_DTYPE[precision]]:
        raise ImportError(f"{path} is not the {precision} build")
    _libs[precision] = lib
    return lib


def _stream_ptr(device=None) -> int:
    """HIP stream handle of torch's current stream on `device` (an engine passes ITS device: with several GPUs in one process the
    calling thread's current device may be another one)."""
    return int(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class Engine:
    """One engine per GPU (not re-entrant).  Mirrors the reference's module handles: weights in, stages out."""

    def __init__(self, device: int = 0, unet_cfg=None, vae_cfg=None, dpt_cfg=None, precision: str = "bf16"):
        libname, contract = ENGINE_PRECISIONS[precision]
        lib = load_library(libname)
        self.precision = precision
        if not torch.cuda.is_available():
            raise RuntimeError("genpercept_amd needs a ROCm GPU (MI355X / gfx950); there is no CPU path")
        self.lib = lib
        cfg = GpConfig()
        lib.gp_default_config(C.byref(cfg))
        cfg.device = device
        if unet_cfg is not None:
            cfg.unet_in_channels, cfg.unet_out_channels = unet_cfg.in_channels, unet_cfg.out_channels
            for i in range(4):
                cfg.unet_block_out[i] = unet_cfg.block_out_channels[i]
                cfg.unet_num_heads[i] = unet_cfg.num_heads[i]
                cfg.unet_down_attn[i] = int(unet_cfg.down_has_attn[i])
            cfg.unet_layers_per_block = unet_cfg.layers_per_block
            cfg.unet_cross_dim = unet_cfg.cross_attention_dim
            cfg.unet_has_out = int(unet_cfg.has_out)
            cfg.unet_norm_eps = unet_cfg.norm_eps
        if vae_cfg is not None:
            for i in range(4):
                cfg.vae_block_out[i] = vae_cfg.block_out_channels[i]
            cfg.vae_layers_per_block = vae_cfg.layers_per_block
            cfg.vae_latent_channels = vae_cfg.latent_channels
            cfg.vae_norm_eps = vae_cfg.norm_eps
            cfg.vae_scaling_factor = vae_cfg.scaling_factor
        if dpt_cfg is not None:
            cfg.dpt_enabled = 1
            for i in range(4):
                cfg.dpt_neck[i] = dpt_cfg.neck_hidden_sizes[i]
            cfg.dpt_fusion = dpt_cfg.fusion_hidden_size
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self._h = C.c_void_p()
        st = lib.gp_create(C.byref(cfg), C.byref(self._h))
        if st != GP_OK:
            msg = lib.gp_last_error(self._h).decode() if self._h else "gp_create failed"
            raise RuntimeError(msg)
        if contract:
            self._check(lib.gp_set_precision(self._h, 1))
        self.finalized = False

    # -- error handling --------------------------------------------------------------------------------------------
    def _check(self, st: int):
        if st == GP_OK:
            return
        msg = self.lib.gp_last_error(self._h).decode()
        if st == 1:
            raise ValueError(msg)
        if st == 3:
            raise KeyError(msg)
        raise RuntimeError(f"genpercept_hip error {st}: {msg}")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -----------------------------------------------------------------------------------------------------
    def load_state_dict(self, module: str, sd: Dict[str, torch.Tensor]):
        """module in {'vae', 'unet', 'dpt'}; sd uses the diffusers key layout (any float dtype, CPU or GPU)."""
        for k, t in sd.items():
            t = t.detach()
            if t.dtype not in _DT:
                t = t.float()
            t = t.cpu().contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape) if t.dim() else (C.c_int64 * 1)(1)
            nd = t.dim()
            src = t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t
            self._check(self.lib.gp_load_tensor(self._h, f"{module}.{k}".encode(), src.data_ptr(), shape, nd, _DT[t.dtype]))

    def set_context(self, embed: torch.Tensor):
        e = embed.detach().float().cpu().reshape(-1, embed.shape[-1]).contiguous()
        self._check(self.lib.gp_set_context(self._h, e.data_ptr(), e.shape[0], e.shape[1]))

    def set_timestep(self, t: float):
        self._check(self.lib.gp_set_timestep(self._h, float(t)))

    def finalize(self):
        self._check(self.lib.gp_finalize(self._h))
        self.finalized = True

    # -- stages --------------------------------------------------------------------------------------------------------
    def infer(self, rgb: torch.Tensor, mode: str) -> torch.Tensor:
        """rgb: [B,3,H,W] uint8 (0..255) or float32 in [-1,1], on this engine's device.  Returns fp32 [B,C,H,W] in [0,1]."""
        assert rgb.is_cuda and rgb.dim() == 4 and rgb.shape[1] == 3
        is_u8 = rgb.dtype == torch.uint8
        if not is_u8:
            rgb = rgb.float()
        rgb = rgb.contiguous()
        b, _, h, w = rgb.shape
        c = 1 if (mode in ONE_CHANNEL_MODES or self.cfg.dpt_enabled) else 3
        lh, lw = self.lib.gp_latent_size(h), self.lib.gp_latent_size(w)
        oh, ow = (self.lib.gp_dpt_out_size(lh), self.lib.gp_dpt_out_size(lw)) if self.cfg.dpt_enabled else (8 * lh, 8 * lw)
        out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=rgb.device)
        self._check(self.lib.gp_infer(self._h, rgb.data_ptr(), int(is_u8), b, h, w, MODES[mode], out.data_ptr(), _stream_ptr(self.device)))
        return out

    def infer_steps(self, rgb: torch.Tensor, mode: str, steps, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The denoising loop of the multi-step archs (gp_infer_steps).  steps: the dicts of `DDIMSchedulerCustomized.plan()`;
        noise: fp32 [B,L,h,w] on this device (marigold) or None (rgb_blending: the sample starts as the rgb latent)."""
        assert rgb.is_cuda and rgb.dim() == 4 and rgb.shape[1] == 3
        is_u8 = rgb.dtype == torch.uint8
        rgb = (rgb if is_u8 else rgb.float()).contiguous()
        b, _, h, w = rgb.shape
        lh, lw = self.lib.gp_latent_size(h), self.lib.gp_latent_size(w)
        arr = (GpDdimStep * len(steps))()
        for a, s in zip(arr, steps):
            if s.get("std", 0.0) or s.get("eps_from_x0", False):
                raise ValueError("the engine's loop is the deterministic update (eta = 0, use_clipped_model_output = False)")
            for f, _t in GpDdimStep._fields_:
                setattr(a, f, float(s[f]))
        if noise is not None:
            if tuple(noise.shape) != (b, self.cfg.vae_latent_channels, lh, lw):
                raise ValueError(f"noise must be [{b},{self.cfg.vae_latent_channels},{lh},{lw}], got {tuple(noise.shape)}")
            noise = noise.to(device=rgb.device, dtype=torch.float32).contiguous()
        out = torch.empty((b, 1 if mode in ONE_CHANNEL_MODES else 3, 8 * lh, 8 * lw), dtype=torch.float32, device=rgb.device)
        self._check(self.lib.gp_infer_steps(self._h, rgb.data_ptr(), int(is_u8), b, h, w, MODES[mode], C.cast(arr, _vp), len(steps),
                                            _ptr(noise), out.data_ptr(), _stream_ptr(self.device)))
        return out

    def vae_encode(self, rgb: torch.Tensor) -> torch.Tensor:
        is_u8 = rgb.dtype == torch.uint8
        rgb = (rgb if is_u8 else rgb.float()).contiguous()
        b, _, h, w = rgb.shape
        out = torch.empty((b, self.cfg.vae_latent_channels, self.lib.gp_latent_size(h), self.lib.gp_latent_size(w)), dtype=torch.float32,
                          device=rgb.device)
        self._check(self.lib.gp_vae_encode(self._h, rgb.data_ptr(), int(is_u8), b, h, w, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def _feat_shapes(self, b, h, w):
        bo = list(self.cfg.unet_block_out)
        # multi_level_feats (custom_unet.py:365-400): each taken after that up block's upsampler
        return [(b, bo[3], _up(h, 3, 1), _up(w, 3, 1)), (b, bo[2], _up(h, 3, 2), _up(w, 3, 2)), (b, bo[1], h, w), (b, bo[0], h, w)]

    def unet(self, latent: torch.Tensor, want_sample: bool = True, want_feats: bool = False):
        latent = latent.float().contiguous()
        b, _, h, w = latent.shape
        sample = torch.empty((b, self.cfg.unet_out_channels, h, w), dtype=torch.float32, device=latent.device) if want_sample else None
        feats = None
        fp = None
        if want_feats:
            feats = [torch.empty(s, dtype=torch.float32, device=latent.device) for s in self._feat_shapes(b, h, w)]
            fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])
        self._check(self.lib.gp_unet(self._h, latent.data_ptr(), b, h, w, _ptr(sample), fp, _stream_ptr(self.device)))
        return sample, feats

    def vae_decode(self, pred_latent: torch.Tensor, mean3: bool) -> torch.Tensor:
        z = pred_latent.float().contiguous()
        b, _, h, w = z.shape
        out = torch.empty((b, 1 if mean3 else 3, h * 8, w * 8), dtype=torch.float32, device=z.device)
        self._check(self.lib.gp_vae_decode(self._h, z.data_ptr(), b, h, w, int(mean3), out.data_ptr(), _stream_ptr(self.device)))
        return out

    def vae_mid_attention(self, x: torch.Tensor, decoder: bool) -> torch.Tensor:
        x = x.float().contiguous()
        b, _, h, w = x.shape
        out = torch.empty_like(x)
        self._check(self.lib.gp_vae_mid_attention(self._h, int(decoder), x.data_ptr(), b, h, w, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def dpt_head(self, feats: Sequence[torch.Tensor]) -> torch.Tensor:
        feats = [f.float().contiguous() for f in feats]
        b, _, h, w = feats[0].shape
        out = torch.empty((b, self.lib.gp_dpt_out_size(h), self.lib.gp_dpt_out_size(w)), dtype=torch.float32, device=feats[0].device)
        fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])
        self._check(self.lib.gp_dpt_head(self._h, fp, b, h, w, out.data_ptr(), _stream_ptr(self.device)))
        return out

    # -- profiling -----------------------------------------------------------------------------------------------------
    def set_profile(self, level: int):
        self._check(self.lib.gp_set_profile(self._h, level))

    def reset_timings(self):
        self._check(self.lib.gp_reset_timings(self._h))

    def launch_log(self):
        """[(ms, flops, description)] of the last infer() at profiling level 3 (kernel time + the gap to the next launch)."""
        n = self.lib.gp_get_launch_log(self._h, None, 0)
        if n <= 1:
            return []
        buf = C.create_string_buffer(n)
        self.lib.gp_get_launch_log(self._h, buf, n)
        rows = []
        for line in buf.value.decode().splitlines():
            ms, fl, name = line.split("\t", 2)
            rows.append((float(ms), float(fl), name))
        return rows

    def timings(self) -> dict:
        t = GpTimings()
        self._check(self.lib.gp_get_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in GpTimings._fields_}

    def halo_executed_flops(self) -> float:
        """MFMA flops the halo-conv launches executed since reset_timings (`gp_halo_executed_flops`): below timings()["flops_halo"] (algorithmic)
        by the 5/9 the phase-decomposed x2-upsample convs do not execute."""
        v = C.c_double(0.0)
        self._check(self.lib.gp_halo_executed_flops(self._h, C.byref(v)))
        return float(v.value)

    def pool_bytes(self) -> int:
        """Bytes of device memory the engine's activation pool holds (`gp_pool_bytes`): the high-water mark of its transient memory."""
        n = C.c_longlong(0)
        self._check(self.lib.gp_pool_bytes(self._h, C.byref(n)))
        return int(n.value)

    def saturation_events(self, reset: bool = False) -> int:
        """fp16 library: (call, kernel file) pairs since the last reset in which a saturating fp32 -> fp16 conversion actually clipped
        (`gp_saturation_events`); 0 = nothing left the fp16 range.  Always 0 for the bf16 library.  Synchronises the engine's stream."""
        n = C.c_longlong(0)
        self._check(self.lib.gp_saturation_events(self._h, C.byref(n), 1 if reset else 0))
        return int(n.value)


def _up(x: int, levels: int, ups: int) -> int:
    """spatial size after `levels` stride-2 (pad 1) downsamples followed by `ups` upsample-to-skip-size steps."""
    sizes = [x]
    for _ in range(levels):
        sizes.append((sizes[-1] - 1) // 2 + 1)
    return sizes[levels - ups]


# ---- per-kernel wrappers (used by tests/) -----------------------------------------------------------------------------
def to_nhwc_h16(x: torch.Tensor, cpad: Optional[int] = None) -> torch.Tensor:
    """[B,C,H,W] float -> contiguous [B,H,W,Cpad] in the default library's element type (zero-padded channels)."""
    b, c, h, w = x.shape
    cp = cpad or c
    out = torch.zeros((b, h, w, cp), dtype=act_dtype(), device=x.device)
    out[..., :c] = x.permute(0, 2, 3, 1).to(act_dtype())
    return out.contiguous()


to_nhwc_bf16 = to_nhwc_h16  # (name kept for the bf16-era call sites)


def last_igemm_path():
    """(path, pgemm row tile) of the last conv / GEMM launch of this thread (`gp_last_igemm_path`; reading clears it): 1 halo 16-row tiles,
    2 halo phases, 3 persistent GEMM, 4 conv_img + split-K reduce, 5 split-K igemm + reduce, 6 igemm, 7 halo 12-row tiles, 8 per-tile halo."""
    rows = C.c_int(0)
    path = load_library().gp_last_igemm_path(C.byref(rows))
    return int(path), int(rows.value)


def pack_weight(w: torch.Tensor, cin_pad: Optional[int] = None, geglu: bool = False, device="cuda") -> torch.Tensor:
    lib = load_library()
    w = w.detach().float().cpu().contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, ks, _ = w.shape
    cp = cin_pad or ((cin + 63) // 64 * 64)
    rows = lib.gp_packed_rows(cout)
    out = torch.empty((rows, ks * ks, cp), dtype=act_dtype(), device=device)
    st = lib.gp_pack_weight(w.data_ptr(), cout, cin, ks, cp, int(geglu), out.data_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_pack_weight failed ({st})")
    return out


def conv2d(x_nhwc: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, ks: int, stride: int = 1, pad_t: int = 1,
           pad_l: int = 1, out_hw=None, ups_hw=None, residual: Optional[torch.Tensor] = None, act: str = "none", n_store: int = 0,
           out_fp32: bool = False, tile: int = 0) -> torch.Tensor:
    lib = load_library()
    b, hi, wi, cin = x_nhwc.shape
    uh, uw = ups_hw if ups_hw else (0, 0)
    hin, win = (uh, uw) if ups_hw else (hi, wi)
    ho, wo = out_hw if out_hw else (hin, win)
    nout = cout // 2 if act == "geglu" else cout
    nst = n_store or nout
    out = torch.empty((b, ho, wo, nst), dtype=torch.float32 if out_fp32 else act_dtype(), device=x_nhwc.device)
    st = lib.gp_conv2d(x_nhwc.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), b, hi, wi, cin, cout, ks, stride,
                       pad_t if ks == 3 else 0, pad_l if ks == 3 else 0, ho, wo, uh, uw, ACT[act], nst, int(out_fp32), tile, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_conv2d failed ({st})")
    return out


def pack_weight_phases(w: torch.Tensor, cin_pad: Optional[int] = None, device="cuda") -> torch.Tensor:
    """[cout][cin][3][3] -> the phase-summed packing of the x2-upsample conv (`gp_pack_weight_phases`): [rows][4][4][cin_pad]."""
    lib = load_library()
    w = w.detach().float().cpu().contiguous()
    cout, cin = w.shape[:2]
    cp = cin_pad or ((cin + 63) // 64 * 64)
    out = torch.empty((lib.gp_packed_rows(cout), 16, cp), dtype=act_dtype(), device=device)
    st = lib.gp_pack_weight_phases(w.data_ptr(), cout, cin, cp, out.data_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_pack_weight_phases failed ({st})")
    return out


def conv2d_up2(x_nhwc: torch.Tensor, w_packed: torch.Tensor, w_phases: torch.Tensor, bias, cout: int, residual=None) -> torch.Tensor:
    """conv3x3(nearest_upsample_x2(x)) through the four-phase kernel (`gp_conv2d_up2`)."""
    lib = load_library()
    b, hi, wi, cin = x_nhwc.shape
    out = torch.empty((b, 2 * hi, 2 * wi, cout), dtype=act_dtype(), device=x_nhwc.device)
    st = lib.gp_conv2d_up2(x_nhwc.data_ptr(), w_packed.data_ptr(), w_phases.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), b, hi, wi, cin, cout,
                           _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_conv2d_up2 failed ({st})")
    return out


def conv2d_up2_stats(x_nhwc: torch.Tensor, w_packed: torch.Tensor, w_phases: torch.Tensor, bias, cout: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                     eps: float, residual=None):
    """`gp_conv2d_up2_stats`: the phase kernel with its GroupNorm-statistics epilogue; returns (out, scale[b][c], shift[b][c])."""
    lib = load_library()
    b, hi, wi, cin = x_nhwc.shape
    out = torch.empty((b, 2 * hi, 2 * wi, cout), dtype=act_dtype(), device=x_nhwc.device)
    scale = torch.empty((b, cout), dtype=torch.float32, device=x_nhwc.device)
    shift = torch.empty((b, cout), dtype=torch.float32, device=x_nhwc.device)
    st = lib.gp_conv2d_up2_stats(x_nhwc.data_ptr(), w_packed.data_ptr(), w_phases.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), b, hi, wi, cin, cout,
                                 gamma.data_ptr(), beta.data_ptr(), groups, eps, scale.data_ptr(), shift.data_ptr(), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_conv2d_up2_stats failed ({st})")
    return out, scale, shift


def conv2d_gn(x_nhwc: torch.Tensor, w_packed: torch.Tensor, bias, cout: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
              silu: bool, ups: bool = False, residual=None, act: str = "none") -> torch.Tensor:
    """conv3x3(act(GroupNorm(x))) with the GroupNorm apply fused into the conv kernel's input staging."""
    lib = load_library()
    b, h, w, cin = x_nhwc.shape
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    out = torch.empty((b, ho, wo, cout), dtype=act_dtype(), device=x_nhwc.device)
    st = lib.gp_conv2d_gn(x_nhwc.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), b, h, w, cin, cout, int(ups), ACT[act],
                          gamma.data_ptr(), beta.data_ptr(), groups, eps, int(silu), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_conv2d_gn failed ({st})")
    return out


def rgb_conv_in(rgb: torch.Tensor, w_packed: torch.Tensor, bias, cout: int) -> torch.Tensor:
    """rgb: [B,3,H,W] uint8 (0..255) or float32 in [-1,1] on the device -> conv_in output NHWC bf16 (prologue fused)."""
    lib = load_library()
    b, _, h, w = rgb.shape
    rgb = rgb.contiguous()
    out = torch.empty((b, h, w, cout), dtype=act_dtype(), device=rgb.device)
    st = lib.gp_rgb_conv_in(rgb.data_ptr(), int(rgb.dtype == torch.uint8), w_packed.data_ptr(), _ptr(bias), out.data_ptr(), b, h, w, cout, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_rgb_conv_in failed ({st})")
    return out


def conv2d_stats(x_nhwc: torch.Tensor, w_packed: torch.Tensor, bias, cout: int, ks: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                 eps: float, ups: bool = False, residual=None, tile: int = 0):
    """conv whose epilogue leaves the GroupNorm statistics of its output; returns (out, scale[b][c], shift[b][c])."""
    lib = load_library()
    b, h, w, cin = x_nhwc.shape
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    out = torch.empty((b, ho, wo, cout), dtype=act_dtype(), device=x_nhwc.device)
    scale = torch.empty((b, cout), dtype=torch.float32, device=x_nhwc.device)
    shift = torch.empty((b, cout), dtype=torch.float32, device=x_nhwc.device)
    st = lib.gp_conv2d_stats(x_nhwc.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), b, h, w, cin, cout, ks, int(ups),
                             tile, gamma.data_ptr(), beta.data_ptr(), groups, eps, scale.data_ptr(), shift.data_ptr(), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_conv2d_stats failed ({st})")
    return out, scale, shift


def gemm(a: torch.Tensor, bt: torch.Tensor, bias=None, bias_mode: int = 1, residual=None, act: str = "none", out_fp32: bool = False,
         n_store: int = 0, tile: int = 0) -> torch.Tensor:
    """out = a @ bt^T for 2-D (or batched 3-D) bf16 tensors; K % 64 == 0."""
    lib = load_library()
    batched = a.dim() == 3
    if not batched:
        a, bt = a[None], bt[None]
    bsz, m, k = a.shape
    n = bt.shape[1]
    nout = n // 2 if act == "geglu" else n
    nst = n_store or nout
    out = torch.empty((bsz, m, nst), dtype=torch.float16 if int(out_fp32) == 2 else (torch.float32 if out_fp32 else act_dtype()), device=a.device)
    st = lib.gp_gemm(a.data_ptr(), a.stride(1), bt.data_ptr(), bt.stride(1), _ptr(bias), bias_mode, _ptr(residual), nst, out.data_ptr(), nst, m, n,
                     k, n, nst, ACT[act], int(out_fp32), bsz, a.stride(0), bt.stride(0), m * nst, tile, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_gemm failed ({st})")
    return out if batched else out[0]


def decoder_tail(x_nhwc: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                 mean3: bool, raw: bool = False) -> torch.Tensor:
    """GroupNorm + SiLU + conv3x3(128 -> 3) + [channel mean] + clip / shift, fp32 NCHW (gp_decoder_tail)."""
    lib = load_library()
    b, h, w, c = x_nhwc.shape
    out = torch.empty((b, 1 if mean3 else 3, h, w), dtype=torch.float32, device=x_nhwc.device)
    st = lib.gp_decoder_tail(x_nhwc.data_ptr(), w_packed.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), groups, eps, b, h, w, c, int(mean3),
                             int(raw), out.data_ptr(), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_decoder_tail failed ({st})")
    return out


def gemm_qkv(a: torch.Tensor, w_packed: torch.Tensor, batch: int, tokens: int, c: int):
    """a [B*T, K]; w_packed = pack_weight(cat(Wq, Wk, Wv)) [rows, 1, K]; returns (qk [B*T, 2C], vt [B, C, Tpad]).  gp_gemm_qkv."""
    lib = load_library()
    m, k = a.shape
    assert m == batch * tokens
    tpad = (tokens + 63) // 64 * 64
    qk = torch.empty((m, 2 * c), dtype=act_dtype(), device=a.device)
    vt = torch.full((batch, c, tpad), float("nan"), dtype=act_dtype(), device=a.device)
    st = lib.gp_gemm_qkv(a.data_ptr(), a.stride(0), w_packed.data_ptr(), w_packed.stride(0), w_packed.shape[0], k, qk.data_ptr(), vt.data_ptr(), batch, tokens, c,
                         tpad, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_gemm_qkv failed ({st})")
    return qk, vt


def groupnorm(x_nhwc: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool) -> torch.Tensor:
    lib = load_library()
    b, h, w, c = x_nhwc.shape
    y = torch.empty_like(x_nhwc)
    st = lib.gp_groupnorm(x_nhwc.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), b, h * w, c, groups, eps, int(silu), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_groupnorm failed ({st})")
    return y


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    lib = load_library()
    rows, c = x.shape
    y = torch.empty_like(x)
    st = lib.gp_layernorm(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, c, eps, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_layernorm failed ({st})")
    return y


def flash_attention_hd512(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, scale: float, ncu: int = 0) -> torch.Tensor:
    """q, k: [B,T,512] (row stride may exceed 512); vt: [B,512,Tpad], zero beyond T.  softmax(scale q k^T) v, one head."""
    lib = load_library()
    b, t, c = q.shape
    assert c == 512 and vt.shape[1] == 512
    out = torch.empty((b, t, c), dtype=act_dtype(), device=q.device)
    st = lib.gp_flash_attention_hd512(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), b, t, q.stride(1), k.stride(1), vt.shape[2], c,
                                      float(scale), int(ncu), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_flash_attention_hd512 failed ({st})")
    return out


def flash_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int) -> torch.Tensor:
    """q, k: [B,T,C] bf16 (row stride may exceed C); vt: [B,C,Tpad] bf16, zero beyond T."""
    lib = load_library()
    b, t, c = q.shape
    out = torch.empty((b, t, c), dtype=act_dtype(), device=q.device)
    st = lib.gp_flash_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), b, t, heads, q.stride(1), k.stride(1), vt.shape[2], c,
                                _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_flash_attention failed ({st})")
    return out


def flash_attention_split(qkv: torch.Tensor, batch: int, tokens: int, heads: int) -> torch.Tensor:
    """qkv fp32 [B*T, 3C] (q | k | v) -> the attention result as fp32 [B*T, C], reassembled (hi + lo) from the split operand gp_flash_attention_split writes
    (contract precision; bf16 library)."""
    lib = load_library("bf16")
    m, c3 = qkv.shape
    c = heads * 64
    assert m == batch * tokens and c3 >= 3 * c and qkv.dtype == torch.float32
    out = torch.empty((m, 3 * c), dtype=torch.bfloat16, device=qkv.device)
    st = lib.gp_flash_attention_split(qkv.data_ptr(), qkv.stride(0), out.data_ptr(), batch, tokens, heads, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_flash_attention_split failed ({st})")
    assert torch.equal(out[:, :c], out[:, 2 * c:])  # [hi | lo | hi]
    return out[:, :c].float() + out[:, c:2 * c].float()


def flash_attention_hd512_split(qkv: torch.Tensor, batch: int, tokens: int, scale: float, return_operand: bool = False):
    """qkv fp32 [B*T, >= 1536] (q | k | v at columns 0 | 512 | 1024) -> softmax(scale q k^T) v of the one-head, head_dim-512 attention as fp32
    [B*T, 512], reassembled (hi + lo) from the split operand gp_flash_attention_hd512_split writes (contract precision; bf16 library).
    return_operand: also the bf16 operand [B*T, 1536] itself ([hi | lo | hi])."""
    lib = load_library("bf16")
    m, c3 = qkv.shape
    assert m == batch * tokens and c3 >= 1536 and qkv.dtype == torch.float32
    out = torch.empty((m, 1536), dtype=torch.bfloat16, device=qkv.device)
    st = lib.gp_flash_attention_hd512_split(qkv.data_ptr(), qkv.stride(0), out.data_ptr(), batch, tokens, float(scale), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_flash_attention_hd512_split failed ({st})")
    val = out[:, :512].float() + out[:, 512:1024].float()
    return (val, out) if return_operand else val


def c_attention_plan(batch: int, tokens: int, heads: int, hd: int):
    """(path, workspace bytes) of the contract precision's attention core for this shape under the current GENPERCEPT_* switches
    (`gp_c_attention_plan`): 0 unfused, 1 flash_attn64_split, 2 flash_attn512_split.  Host arithmetic, no GPU."""
    lib = load_library("bf16")
    path, ws = C.c_int(-1), C.c_longlong(-1)
    _c_check(lib.gp_c_attention_plan(batch, tokens, heads, hd, C.byref(path), C.byref(ws)), "gp_c_attention_plan")
    return int(path.value), int(ws.value)


# ---- contract precision (bf16 library): split operands are bf16 [rows][3 C], A order [hi | lo | hi], B order [hi | hi | lo] ----------------------
def _c_check(st: int, name: str):
    if st != GP_OK:
        raise RuntimeError(f"{name} failed ({st})")


def c_split3(x: torch.Tensor, b_order: bool = False, act: str = "none", scale: float = 1.0) -> torch.Tensor:
    """fp32 [rows, C] (row stride may exceed C) -> split bf16 [rows, 3C] of act(x * scale) (gp_c_split3)."""
    lib = load_library("bf16")
    rows, c = x.shape
    out = torch.empty((rows, 3 * c), dtype=torch.bfloat16, device=x.device)
    _c_check(lib.gp_c_split3(x.data_ptr(), x.stride(0), out.data_ptr(), rows, c, int(b_order), ACT[act], float(scale), _stream_ptr(x.device)), "gp_c_split3")
    return out


def c_groupnorm_split(x_nhwc: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool = False):
    """fp32 NHWC [B,H,W,C] -> (split bf16 [B,H,W,3C] of act(GroupNorm(x)), scale [B,C], shift [B,C]) (gp_c_groupnorm_split)."""
    lib = load_library("bf16")
    b, h, w, c = x_nhwc.shape
    out = torch.empty((b, h, w, 3 * c), dtype=torch.bfloat16, device=x_nhwc.device)
    sc = torch.empty((b, c), dtype=torch.float32, device=x_nhwc.device)
    sh = torch.empty_like(sc)
    _c_check(lib.gp_c_groupnorm_split(x_nhwc.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), b, h * w, c, groups, float(eps), int(silu),
                                      sc.data_ptr(), sh.data_ptr(), _stream_ptr(x_nhwc.device)), "gp_c_groupnorm_split")
    return out, sc, sh


def pack_weight_split(w: torch.Tensor, geglu: bool = False, device="cuda") -> torch.Tensor:
    """OIHW (or [out, in]) fp32 -> B-order split packing [rows, taps, 3 cin_pad] (gp_pack_weight_split)."""
    lib = load_library("bf16")
    w = w.detach().float().cpu().contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, ks, _ = w.shape
    cp = (cin + 63) // 64 * 64
    out = torch.empty((lib.gp_packed_rows(cout), ks * ks, 3 * cp), dtype=torch.bfloat16, device=device)
    _c_check(lib.gp_pack_weight_split(w.data_ptr(), cout, cin, ks, cp, int(geglu), out.data_ptr()), "gp_pack_weight_split")
    return out


def pack_weight_phases_split(w: torch.Tensor, device="cuda") -> torch.Tensor:
    lib = load_library("bf16")
    w = w.detach().float().cpu().contiguous()
    cout, cin = w.shape[:2]
    cp = (cin + 63) // 64 * 64
    out = torch.empty((lib.gp_packed_rows(cout), 16, 3 * cp), dtype=torch.bfloat16, device=device)
    _c_check(lib.gp_pack_weight_phases_split(w.data_ptr(), cout, cin, cp, out.data_ptr()), "gp_pack_weight_phases_split")
    return out


def c_conv2d(x_split: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int, ks: int, stride: int = 1, pad=(1, 1), out_hw=None,
             ups: bool = False, w_phases: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: str = "none", tile: int = 0,
             out: Optional[torch.Tensor] = None, gn=None):
    """contract-precision conv / linear (gp_c_conv2d): split NHWC [B,Hi,Wi,3 Cin] -> fp32 [B,Ho,Wo,N].  `out` may be `residual` (in place).
    gn = (gamma, beta, groups, eps): also the GroupNorm scale / shift of the output.  Returns (y, path, scale, shift)."""
    lib = load_library("bf16")
    b, hi, wi, c3 = x_split.shape
    ho, wo = out_hw if out_hw else ((2 * hi, 2 * wi) if ups else (hi, wi))
    nout = cout // 2 if act == "geglu" else cout
    if out is None:
        out = torch.empty((b, ho, wo, nout), dtype=torch.float32, device=x_split.device)
    path = C.c_int(0)
    sc = sh = None
    g = (None, None, 0, 0.0)
    if gn is not None:
        sc = torch.empty((b, nout), dtype=torch.float32, device=x_split.device)
        sh = torch.empty_like(sc)
        g = gn
    _c_check(lib.gp_c_conv2d(x_split.data_ptr(), w_packed.data_ptr(), _ptr(w_phases), _ptr(bias), _ptr(residual), out.data_ptr(), b, hi, wi, c3 // 3, cout,
                             ks, stride, pad[0], pad[1], ho, wo, int(ups), ACT[act], tile, _ptr(g[0]), _ptr(g[1]), int(g[2]), float(g[3]), _ptr(sc), _ptr(sh),
                             C.byref(path), _stream_ptr(x_split.device)), "gp_c_conv2d")
    return out, path.value, sc, sh


def c_layernorm_split(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    lib = load_library("bf16")
    rows, c = x.shape
    out = torch.empty((rows, 3 * c), dtype=torch.bfloat16, device=x.device)
    _c_check(lib.gp_c_layernorm_split(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, c, float(eps), _stream_ptr(x.device)),
             "gp_c_layernorm_split")
    return out


def c_softmax_split(x: torch.Tensor, tokens: int, scale: float) -> torch.Tensor:
    """fp32 logits [rows, ld] (first `tokens` valid) -> split probabilities bf16 [rows, 3 ld] (gp_c_softmax_split)."""
    lib = load_library("bf16")
    rows, ld = x.shape
    out = torch.empty((rows, 3 * ld), dtype=torch.bfloat16, device=x.device)
    _c_check(lib.gp_c_softmax_split(x.data_ptr(), out.data_ptr(), rows, tokens, ld, float(scale), _stream_ptr(x.device)), "gp_c_softmax_split")
    return out


def cross_attention(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    rows, c = q.shape
    out = torch.empty_like(q)
    st = lib.gp_cross_attention(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), rows, c, kc.shape[0], _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_cross_attention failed ({st})")
    return out


RESAMPLE_CODE = {"bilinear": 0, "nearest-exact": 1, "bicubic": 2}  # image_util.py:108-126: everything get_tv_resample_method accepts


def resize_max_res_size(h0: int, w0: int, max_edge: int):
    lib = load_library()
    h, w = C.c_int(), C.c_int()
    lib.gp_resize_max_res_size(h0, w0, max_edge, C.byref(h), C.byref(w))
    return h.value, w.value


def preprocess(rgb: torch.Tensor, size, resample: str = "bilinear", normalize: bool = False) -> torch.Tensor:
    """resize_max_res of a [B,3,H0,W0] image ON THE DEVICE to size = (h, w) (image_util.py:75-105).  uint8 in -> uint8 out (fp32 interpolation,
    rounded: what the reference does to the PIL / uint8 input); float in -> fp32 out without rounding, and with `normalize` the
    x / 255 * 2 - 1 of genpercept_pipeline.py:245 on top (the [-1, 1] image the engine takes as fp32)."""
    lib = load_library()
    assert rgb.is_cuda and rgb.dim() == 4
    b, c, h0, w0 = rgb.shape
    h, w = int(size[0]), int(size[1])
    same = (h, w) == (h0, w0)
    need_tmp = not same and resample != "nearest-exact"
    if rgb.dtype == torch.uint8:
        assert c == 3 and not normalize
        rgb = rgb.contiguous()
        if same:
            return rgb
        out = torch.empty((b, 3, h, w), dtype=torch.uint8, device=rgb.device)
        tmp = torch.empty((b * 3 * h0 * w,), dtype=torch.float32, device=rgb.device) if need_tmp else None
        st = lib.gp_preprocess(rgb.data_ptr(), b, h0, w0, out.data_ptr(), h, w, RESAMPLE_CODE[resample], _ptr(tmp), _stream_ptr(rgb.device))
    else:
        rgb = rgb.to(torch.float32).contiguous()
        if same and not normalize:
            return rgb
        out = torch.empty((b, c, h, w), dtype=torch.float32, device=rgb.device)
        tmp = torch.empty((b * c * h0 * w,), dtype=torch.float32, device=rgb.device) if need_tmp else None
        st = lib.gp_preprocess_f32(rgb.data_ptr(), b, c, h0, w0, out.data_ptr(), h, w, RESAMPLE_CODE[resample], int(bool(normalize)), _ptr(tmp),
                                   _stream_ptr(rgb.device))
    if st != GP_OK:
        raise RuntimeError(f"gp_preprocess failed ({st})")
    return out


_lut_cache: Dict[tuple, torch.Tensor] = {}


def colormap_lut(cmap: str, device) -> torch.Tensor:
    """256 x 3 uint8 table of a matplotlib colour map, exactly the bytes (cm(i / 256...)[:3] * 255).astype(uint8) gives for LUT entry i."""
    key = (cmap, str(device))
    if key not in _lut_cache:
        import matplotlib
        import numpy as np
        cm = matplotlib.colormaps[cmap]
        table = cm(np.arange(256, dtype=np.int64), bytes=False)[:, :3]  # integer input: direct LUT lookup
        _lut_cache[key] = torch.from_numpy((table * 255).astype(np.uint8)).contiguous().to(device)
    return _lut_cache[key]


def postprocess(pred: torch.Tensor, size, resample: str = "bilinear", cmap: Optional[str] = None, q_bits: int = 0):
    """pred fp32 [B,C,h,w] on the device -> (pred_out [B,C,H,W] clipped to [0,1], colored uint8 [B,H,W,3] or None, quantised or None)."""
    lib = load_library()
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 4
    pred = pred.contiguous()
    b, c, h, w = pred.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=pred.device)
    tmp = torch.empty((b * c * h * wo,), dtype=torch.float32, device=pred.device) if (resample != "nearest-exact" and (h, w) != (ho, wo)) else None
    lut = colormap_lut(cmap, pred.device) if cmap is not None else None
    col = torch.empty((b, ho, wo, 3), dtype=torch.uint8, device=pred.device) if cmap is not None else None
    q = torch.empty((b, c, ho, wo), dtype=torch.uint16 if q_bits == 16 else torch.uint8, device=pred.device) if q_bits else None
    st = lib.gp_postprocess(pred.data_ptr(), b, c, h, w, out.data_ptr(), ho, wo, RESAMPLE_CODE[resample], _ptr(tmp), _ptr(lut), _ptr(col), _ptr(q), q_bits,
                            _stream_ptr(pred.device))
    if st != GP_OK:
        raise RuntimeError(f"gp_postprocess failed ({st})")
    return out, col, q


EVAL_ALIGNMENT = {None: 0, "": 0, "none": 0, "least_square": 1, "least_square_disparity": 2}  # eval.py:168-200


def _eval_maps(x: torch.Tensor, name: str) -> torch.Tensor:
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    elif x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError(f"{name}: expected [B, H, W] (or [B, 1, H, W], [H, W]), got {tuple(x.shape)}")
    return x


def _mask_u8(m: torch.Tensor, name: str, shape) -> torch.Tensor:
    """A validity mask or region as a contiguous uint8 plane [B, H, W] of `shape`: bool and uint8 as their bytes (every kernel tests the byte
    against zero, eval.hip's depth passes included), any other dtype through `!= 0`."""
    m = _eval_maps(m, name)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{name} {tuple(m.shape)} does not match the maps {tuple(shape)}")
    assert m.is_cuda
    return (m if m.dtype in (torch.bool, torch.uint8) else m != 0).contiguous().view(torch.uint8)


def _map8(x: torch.Tensor, name: str):
    """A float map in [0, 1] as contiguous fp32 (the kernel quantises it), or its uint8 quantisation as it is: (map, is_u8)."""
    is_u8 = x.dtype == torch.uint8
    if not is_u8 and not x.dtype.is_floating_point:
        raise ValueError(f"{name}: a float map in [0, 1] or its uint8 quantisation, got {x.dtype}")
    return (x if is_u8 else x.to(torch.float32)).contiguous(), is_u8


def _pred_gt8(pred: torch.Tensor, gt: torch.Tensor):
    """pred (`_map8`) and the 8-bit ground truth as contiguous [B, H, W] device maps of one shape: (pred, is_u8, gt, (b, h, w))."""
    pred, gt = _eval_maps(pred, "pred"), _eval_maps(gt, "gt")
    assert pred.is_cuda and gt.is_cuda
    if gt.dtype != torch.uint8:
        raise ValueError(f"gt: the ground truth is an 8-bit mask / alpha map (uint8), got {gt.dtype}")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have one shape")
    pred, is_u8 = _map8(pred, "pred")
    return pred, is_u8, gt.contiguous(), tuple(int(v) for v in pred.shape)


def _workspace(nbytes: int, device):
    """(an 8-byte aligned device buffer for the `nbytes` a gp_*_workspace call asks for, nbytes)"""
    nbytes = int(nbytes)
    return torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=device), nbytes


def _packed(b: int, n_out: int, n_cnt: int, device):
    """One int64 device buffer that holds the float64 values [b, n_out] and then the int64 counts [b, n_cnt] (n_cnt = 0: None), so that one
    copy brings both to the host: (buf, out, counts), the last two views of buf."""
    buf = torch.empty((b * (n_out + n_cnt),), dtype=torch.int64, device=device)
    return buf, buf[:b * n_out].view(torch.float64).view(b, n_out), buf[b * n_out:].view(b, n_cnt) if n_cnt else None


def _unpacked(buf: torch.Tensor, b: int, n_out: int):
    """The host copy of a `_packed` buffer with counts: (float64 numpy [b, n_out], int64 numpy [b, n_cnt])."""
    host = buf.cpu().numpy()
    return host[:b * n_out].view("float64").reshape(b, n_out), host[b * n_out:].reshape(b, -1)


# ---- what the post-processing ops (foreground, guided_upsample, tile_merge, depth_geometry, lens_blur) share -------------------------------
def _images_u8(x, name: str) -> torch.Tensor:
    """8-bit RGB images as a contiguous uint8 [B, 3, H, W] tensor (one image may come without the batch axis)."""
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-3] != 3:
        raise ValueError(f"{name}: uint8 [B, 3, H, W] or [3, H, W], got {x.dtype if torch.is_tensor(x) else type(x)} "
                         f"{tuple(x.shape) if torch.is_tensor(x) else ''}")
    return (x[None] if x.dim() == 3 else x).contiguous()


def _float32(x, name: str) -> torch.Tensor:
    """A prediction of any float dtype as float32 (the kernels read float32)."""
    if not torch.is_tensor(x) or not x.dtype.is_floating_point:
        raise ValueError(f"{name}: a float tensor, got {x.dtype if torch.is_tensor(x) else type(x)}")
    return x.to(torch.float32)


def _float_maps(x, name: str) -> torch.Tensor:
    """One-channel float maps as contiguous float32 [B, H, W] (`_eval_maps` shapes)."""
    return _eval_maps(_float32(x, name), name).contiguous()


def _same_batch(image: torch.Tensor, shape, device, name: str) -> torch.Tensor:
    """`image` ([B, 3, H, W], of `_images_u8`) goes with maps of `shape` = (B, H, W) on `device`: one map per image, same size, same device."""
    b, h, w = shape
    if tuple(image.shape) != (b, 3, h, w) or image.device != device:
        raise ValueError(f"{name} {tuple(image.shape)} on {image.device} and the maps {(b, h, w)} on {device}: one map per image, same size, same device")
    return image


def _post_dims(b: int, h: int, w: int, what: str, count_limit: bool = True) -> None:
    """The range every post-processing entry takes: 1 .. 65535 images, sides in 1 .. MAX_DIM and, where the kernels index the batch with
    32 bits (count_limit), B * H * W < 2^31."""
    if not (1 <= b <= 65535 and 1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM) or (count_limit and b * h * w >= 2 ** 31):
        raise ValueError(f"{what} takes 1 .. 65535 images with sides in 1 .. {MAX_DIM}{' and B * H * W < 2^31' if count_limit else ''}, got {(b, h, w)}")


def _op_workspace(name: str, device, *dims):
    """`_workspace` of what the entry `name` asks for through its `name`_workspace(*dims)."""
    return _workspace(getattr(load_library(), name + "_workspace")(*dims), device)


def _launch(name: str, describe: str, *args) -> None:
    """Call the entry `name`; the status of refused arguments is a ValueError that says what was passed, any other failure a RuntimeError."""
    st = getattr(load_library(), name)(*args)
    if st == GP_ERR_INVALID:
        raise ValueError(f"{name}: invalid arguments ({describe})")
    _c_check(st, name)


# ---- what the ops that render a photograph under one plane of its map (lens_blur, stereo_views, parallax_frames) share ---------------------------
def _image_and_maps(image, pred, space: str, what: str):
    """The opening of the three bindings: (image uint8 [B, 3, H, W], pred float32 [B, H, W], (B, H, W), their device), checked -- one map per
    image, same size, same device, a known space, the range of `_post_dims`."""
    image, pred = _images_u8(image, "image"), _float_maps(pred, "pred")
    shape = tuple(int(v) for v in pred.shape)
    _same_batch(image, shape, pred.device, "image")
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")
    _post_dims(*shape, what)
    return image, pred, shape, pred.device


def _nearness_plane(pred: torch.Tensor, value, at, space: str, default: Optional[int] = None) -> torch.Tensor:
    """The plane of every image as its nearness, int32 [B] on the maps' device: of `value` (host float32 [B]), of the pixels `at` (host
    int64 [B, 2] = (u, v)) of the maps pred [B, H, W], or `default` with neither.  The 16-bit rule in float32 (`post_common.nearness`):
    plumbing on the device, so that a plane picked from the map is not read back."""
    b, h, w = pred.shape
    if value is None and at is None:
        return torch.full((b,), default, dtype=torch.int32, device=pred.device)
    if value is not None:
        v = torch.from_numpy(value).to(pred.device, non_blocking=True)
    else:
        v = pred.view(b, h * w).gather(1, torch.from_numpy(at[:, 1] * w + at[:, 0]).to(pred.device, non_blocking=True)[:, None])[:, 0]
    q = (v.clamp(0.0, 1.0) * 65535.0).nan_to_num(0.0).to(torch.int32)
    return torch.where(v.isnan(), torch.zeros_like(q), q if space == "disparity" else 65535 - q).contiguous()


def _output_u8(out, name: str, shape, device) -> torch.Tensor:
    """The output a caller supplies, checked -- a contiguous uint8 tensor of `shape` on `device` --, or with None a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f"{name}: a contiguous uint8 {tuple(shape)} tensor on {device}, got {out.dtype if torch.is_tensor(out) else type(out)} "
                         f"{tuple(out.shape) if torch.is_tensor(out) else ''}")
    return out


def _warp_planes(out: torch.Tensor, shape, want_holes: bool, want_near: bool):
    """The planes a warp writes next to `out`, where wanted: (holes uint8 `shape` or None, near int16 `shape` or None, what the binding
    returns -- `out` alone or a tuple with the wanted planes after it)."""
    holes = torch.empty(shape, dtype=torch.uint8, device=out.device) if want_holes else None
    near = torch.empty(shape, dtype=torch.int16, device=out.device) if want_near else None
    return holes, near, _with_planes(out, holes, near, want_holes, want_near)


def eval_depth_raw(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, alignment: Optional[str] = "least_square",
                   alignment_max_res: Optional[int] = None, min_depth: float = 1e-3, max_depth: float = 10.0) -> torch.Tensor:
    """gp_eval_depth on device tensors: float64 [B, 14] ON THE DEVICE = s, t, n_valid, n_fit, then the ten metrics in eval_metrics.METRICS
    order.  Enqueued on the current stream, no synchronisation; the error checks of `eval_depth` are the caller's."""
    import numpy as np
    if alignment not in EVAL_ALIGNMENT:
        raise NotImplementedError(alignment)
    lib = load_library()
    pred, gt = _eval_maps(pred, "pred"), _eval_maps(gt, "gt")
    assert pred.is_cuda and gt.is_cuda
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have one shape")
    mask = _mask_u8(mask, "mask", pred.shape)
    pred, gt = pred.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    b, h, w = (int(v) for v in pred.shape)
    fit_cols, fit_inv = 0, 0.0
    if alignment_max_res is not None and EVAL_ALIGNMENT[alignment]:  # alignment.py:43-55 as eval_metrics.align_depth_least_square restates it
        scale = float(np.min(alignment_max_res / np.array([h, w])))
        if scale < 1:
            fit_cols, fit_inv = int(np.floor(w * scale)), float(np.float32(1.0 / scale))
            if fit_cols < 1:
                raise ValueError(f"alignment_max_res = {alignment_max_res} leaves no column of a {h} x {w} image to fit on")
    out = torch.empty((b, 14), dtype=torch.float64, device=pred.device)
    ws, nbytes = _workspace(lib.gp_eval_depth_workspace(b, h, w), pred.device)
    _c_check(lib.gp_eval_depth(pred.data_ptr(), gt.data_ptr(), mask.data_ptr(), b, h, w, EVAL_ALIGNMENT[alignment], fit_cols, fit_inv, float(min_depth),
                               float(max_depth), out.data_ptr(), ws.data_ptr(), nbytes, _stream_ptr(pred.device)), "gp_eval_depth")
    return out


def eval_depth(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, alignment: Optional[str] = "least_square",
               alignment_max_res: Optional[int] = None, min_depth: float = 1e-3, max_depth: float = 10.0):
    """eval_metrics.evaluate_depth (eval.py:168-215) for a batch of maps that are on the device: pred, gt fp32 [B, H, W], mask bool / uint8.
    Returns (one metric dict per image, (s, t, n_valid)) with s, t, n_valid as numpy arrays [B] (s = 1, t = 0 without alignment).  Raises
    ValueError when an image has fewer than 2 fit pixels or a singular system.  One device -> host copy of B x 14 doubles."""
    from .eval_metrics import METRICS
    raw = eval_depth_raw(pred, gt, mask, alignment, alignment_max_res, min_depth, max_depth).cpu().numpy()
    if EVAL_ALIGNMENT[alignment]:
        for i, row in enumerate(raw):
            if row[3] < 2 or not (row[0] == row[0] and row[1] == row[1]):
                raise ValueError(f"image {i}: least-squares alignment needs at least 2 fit pixels and a non-singular system (n_fit = {int(row[3])})")
    names = list(METRICS.keys())
    return [{k: float(row[4 + j]) for j, k in enumerate(names)} for row in raw], (raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2].astype("int64"))


NORMAL_METRICS = ("mean_rad", "mean_deg", "median_deg", "rmse_deg", "within_11.25", "within_22.5", "within_30")  # normal_angular_error's keys


def _normal_maps(x: torch.Tensor, name: str) -> torch.Tensor:
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{name}: expected [B, 3, H, W] (or [3, H, W]), got {tuple(x.shape)}")
    return x


def eval_normal_raw(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, pred_encoded: bool = True, gt_encoded: bool = False,
                    want_angles: bool = False):
    """gp_eval_normal on device tensors: float64 [B, 8] ON THE DEVICE = n_valid, then the seven values of eval_metrics.normal_angular_error in
    its order (NaN for an image without a valid pixel); with want_angles also the float64 [B, H, W] angles in radians (NaN where invalid).
    pred, gt: [B, 3, H, W] or [3, H, W]; *_encoded: the map is the pipeline's [0, 1] encoding (decode_normals); mask: [B, H, W], [B, 1, H, W] or
    [H, W], bool or integer, None = "any stored gt channel != 0" (not with gt_encoded).  Enqueued on the current stream, no synchronisation."""
    lib = load_library()
    pred, gt = _normal_maps(pred, "pred"), _normal_maps(gt, "gt")
    assert pred.is_cuda and gt.is_cuda
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have one shape")
    if mask is None and gt_encoded:
        raise ValueError("the derived validity rule (gt != 0) needs the signed ground truth: pass a mask with gt_encoded")
    pred, gt = pred.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    b, _, h, w = (int(v) for v in pred.shape)
    if mask is not None:
        mask = _mask_u8(mask, "mask", (b, h, w))
    out = torch.empty((b, 8), dtype=torch.float64, device=pred.device)
    angles = torch.empty((b, h, w), dtype=torch.float64, device=pred.device) if want_angles else None
    ws, nbytes = _workspace(lib.gp_eval_normal_workspace(b, h, w), pred.device)
    _c_check(lib.gp_eval_normal(pred.data_ptr(), gt.data_ptr(), _ptr(mask), b, h, w, int(bool(pred_encoded)) | int(bool(gt_encoded)) << 1, out.data_ptr(),
                                _ptr(angles), ws.data_ptr(), nbytes, _stream_ptr(pred.device)), "gp_eval_normal")
    return (out, angles) if want_angles else out


def eval_normal(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, pred_encoded: bool = True, gt_encoded: bool = False):
    """eval_metrics.normal_angular_error for a batch of maps that are on the device (arguments as `eval_normal_raw`).  Returns (one dict per
    image with normal_angular_error's seven names, n_valid as an int64 numpy array [B]).  Raises ValueError naming the image when it has no
    valid pixel.  One device -> host copy of B x 8 doubles."""
    raw = eval_normal_raw(pred, gt, mask, pred_encoded, gt_encoded).cpu().numpy()
    for i, row in enumerate(raw):
        if row[0] == 0:
            raise ValueError(f"image {i}: no valid pixel to evaluate normals on (n_valid = 0)")
    return [{k: float(row[1 + j]) for j, k in enumerate(NORMAL_METRICS)} for row in raw], raw[:, 0].astype("int64")


MASK_OUT = 10      # n, n_fg, MASK_METRICS (out[2 .. 8]), t_max
MASK_COUNTS = 516  # n, sum_q, sad, sse, hist_bg[256], hist_fg[256]


def _eval_mask_launch(pred: torch.Tensor, gt: torch.Tensor, region: Optional[torch.Tensor], want_counts: bool):
    """The checks and the call of `eval_mask_raw`.  Returns (buf, out, counts): out float64 [B, 10] and counts int64 [B, 516] (or None) are
    views of the one int64 device buffer `buf`, so that one copy brings both to the host."""
    lib = load_library()
    pred, is_u8, gt, (b, h, w) = _pred_gt8(pred, gt)
    if region is not None:
        region = _mask_u8(region, "region", (b, h, w))
    buf, out, counts = _packed(b, MASK_OUT, MASK_COUNTS if want_counts else 0, pred.device)
    ws, nbytes = _workspace(lib.gp_eval_mask_workspace(b, h, w), pred.device)
    _c_check(lib.gp_eval_mask(pred.data_ptr(), int(is_u8), gt.data_ptr(), _ptr(region), b, h, w, out.data_ptr(), _ptr(counts), ws.data_ptr(), nbytes,
                              _stream_ptr(pred.device)), "gp_eval_mask")
    return buf, out, counts


def eval_mask_raw(pred: torch.Tensor, gt: torch.Tensor, region: Optional[torch.Tensor] = None, want_counts: bool = False):
    """gp_eval_mask on device tensors: float64 [B, 10] ON THE DEVICE = n, n_fg, then MASK_METRICS, then t_max (NaN after n_fg for an image whose
    region is empty); with want_counts also the int64 [B, 516] counts n, sum_q, sad, sse, hist_bg[256], hist_fg[256] (eval_metrics.mask_counts).
    pred: [B, H, W], [B, 1, H, W] or [H, W], a float map in [0, 1] (quantised to 8 bits by the kernel as run.py:449-455 does) or uint8 (the
    bytes `postprocess(..., q_bits=8)` returns); gt: uint8, same shape; region: bool or integer, non-zero = scored, None = every pixel.
    Enqueued on the current stream, no synchronisation."""
    _, out, counts = _eval_mask_launch(pred, gt, region, want_counts)
    return (out, counts) if want_counts else out


def eval_mask(pred: torch.Tensor, gt: torch.Tensor, region: Optional[torch.Tensor] = None):
    """eval_metrics.mask_metrics for a batch of maps that are on the device (arguments as `eval_mask_raw`).  Returns one dict per image:
    MASK_METRICS, "n", "n_fg", "t_max" and "counts" (int64 numpy [516]).  Raises ValueError naming the image when its region is empty.  One
    device -> host copy of B x (10 + 516) words."""
    buf, out, _ = _eval_mask_launch(pred, gt, region, True)
    raw, counts = _unpacked(buf, out.shape[0], MASK_OUT)
    res = []
    for i, row in enumerate(raw):
        if row[0] == 0:
            raise ValueError(f"image {i}: no pixel to evaluate the mask on (n = 0)")
        d = {k: float(row[2 + j]) for j, k in enumerate(MASK_METRICS)}
        d.update(n=int(row[0]), n_fg=int(row[1]), t_max=int(row[9]), counts=counts[i].copy())
        res.append(d)
    return res


STRUCTURE_OUT_NAMES = ["n", "n_fg", "s_alpha", "s_object", "s_region", "max_e", "mean_e", "adp_e", "wf", "wf_precision", "wf_recall", "wf_sum_fg",
                       "wf_sum_bg", "cx", "cy"]
STRUCTURE_OUT = 15       # the names above (STRUCTURE_METRICS: out[2], [5 .. 8])
STRUCTURE_COUNTS = 537   # n_fg, sum_fg x, sum_fg y, cx, cy, 4 x (N, a, a2, b, c), hist_bg[256], hist_fg[256]


def eval_structure_raw(pred: torch.Tensor, gt: torch.Tensor, want_counts: bool = False, want_edt: bool = False):
    """gp_eval_structure on device tensors: float64 [B, 15] ON THE DEVICE = STRUCTURE_OUT_NAMES (S-measure, E-measure and weighted F of a dis
    prediction; definitions in include/genpercept_hip.h); with want_counts also the int64 [B, 537] counts (eval_metrics.structure_counts),
    with want_edt also the int64 [B, H, W] distance-transform keys (eval_metrics.edt_keys, the same bits), in that order.  pred: [B, H, W],
    [B, 1, H, W] or [H, W], a float map in [0, 1] (quantised to 8 bits by the kernel) or uint8; gt: uint8, same shape; H, W <= 32767.
    Enqueued on the current stream, no synchronisation."""
    lib = load_library()
    pred, is_u8, gt, (b, h, w) = _pred_gt8(pred, gt)
    if h > 32767 or w > 32767:
        raise ValueError(f"structure scores take maps of at most 32767 x 32767, got {h} x {w}")
    out = torch.empty((b, STRUCTURE_OUT), dtype=torch.float64, device=pred.device)
    counts = torch.empty((b, STRUCTURE_COUNTS), dtype=torch.int64, device=pred.device) if want_counts else None
    edt = torch.empty((b, h, w), dtype=torch.int64, device=pred.device) if want_edt else None
    ws, nbytes = _workspace(lib.gp_eval_structure_workspace(b, h, w), pred.device)
    _c_check(lib.gp_eval_structure(pred.data_ptr(), int(is_u8), gt.data_ptr(), b, h, w, out.data_ptr(), _ptr(counts), _ptr(edt), ws.data_ptr(), nbytes,
                                   _stream_ptr(pred.device)), "gp_eval_structure")
    res = (out,) + ((counts,) if want_counts else ()) + ((edt,) if want_edt else ())
    return res if len(res) > 1 else out


def eval_structure(pred: torch.Tensor, gt: torch.Tensor):
    """eval_metrics.structure_metrics for a batch of maps that are on the device (arguments as `eval_structure_raw`).  Returns one dict per
    image with STRUCTURE_OUT_NAMES (n, n_fg, cx, cy as ints).  One device -> host copy of B x 15 doubles."""
    raw = eval_structure_raw(pred, gt).cpu().numpy()
    ints = ("n", "n_fg", "cx", "cy")
    return [{k: (int(row[j]) if k in ints else float(row[j])) for j, k in enumerate(STRUCTURE_OUT_NAMES)} for row in raw]


MATTING_OUT_NAMES = ["n", "grad", "conn", "grad_sum"]  # MATTING_METRICS: out[1], [2]
MATTING_OUT = 4       # the names above
MATTING_COUNTS = 13   # n, conn_num, the counts of the levels 0..10 over the whole image


def eval_matting_raw(pred: torch.Tensor, gt: torch.Tensor, region: Optional[torch.Tensor] = None, want_counts: bool = False,
                     want_levels: bool = False, want_grad_map: bool = False):
    """gp_eval_matting on device tensors: float64 [B, 4] ON THE DEVICE = MATTING_OUT_NAMES (gradient and connectivity error of a matting
    prediction; definitions in include/genpercept_hip.h; NaN after n for an image whose region is empty); with want_counts also the int64
    [B, 13] counts (eval_metrics.conn_error's "counts"), with want_levels the uint8 [B, H, W] levels (eval_metrics.conn_levels), with
    want_grad_map the float64 [B, H, W] error map (eval_metrics.grad_error_map, the same bits), in that order.  pred: [B, H, W], [B, 1, H, W]
    or [H, W], a float map in [0, 1] (quantised to 8 bits by the kernel) or uint8; gt: uint8, same shape; region: bool or integer, non-zero =
    scored, None = every pixel (it restricts only the sums).  Enqueued on the current stream, no synchronisation."""
    lib = load_library()
    pred, is_u8, gt, (b, h, w) = _pred_gt8(pred, gt)
    if region is not None:
        region = _mask_u8(region, "region", (b, h, w))
    out = torch.empty((b, MATTING_OUT), dtype=torch.float64, device=pred.device)
    counts = torch.empty((b, MATTING_COUNTS), dtype=torch.int64, device=pred.device) if want_counts else None
    levels = torch.empty((b, h, w), dtype=torch.uint8, device=pred.device) if want_levels else None
    grad_map = torch.empty((b, h, w), dtype=torch.float64, device=pred.device) if want_grad_map else None
    ws, nbytes = _workspace(lib.gp_eval_matting_workspace(b, h, w), pred.device)
    _c_check(lib.gp_eval_matting(pred.data_ptr(), int(is_u8), gt.data_ptr(), _ptr(region), b, h, w, out.data_ptr(), _ptr(counts), _ptr(levels),
                                 _ptr(grad_map), ws.data_ptr(), nbytes, _stream_ptr(pred.device)), "gp_eval_matting")
    res = (out,) + ((counts,) if want_counts else ()) + ((levels,) if want_levels else ()) + ((grad_map,) if want_grad_map else ())
    return res if len(res) > 1 else out


def eval_matting(pred: torch.Tensor, gt: torch.Tensor, region: Optional[torch.Tensor] = None):
    """eval_metrics.matting_metrics for a batch of maps that are on the device (arguments as `eval_matting_raw`).  Returns one dict per image
    with MATTING_OUT_NAMES (n as an int).  Raises ValueError naming the image when its region is empty.  One device -> host copy of B x 4
    doubles."""
    raw = eval_matting_raw(pred, gt, region).cpu().numpy()
    for i, row in enumerate(raw):
        if row[0] == 0:
            raise ValueError(f"image {i}: no pixel to evaluate the alpha map on (n = 0)")
    return [{k: (int(row[j]) if k == "n" else float(row[j])) for j, k in enumerate(MATTING_OUT_NAMES)} for row in raw]


def mask_band(a: torch.Tensor, lo: int, hi: int, reach: int, metric="euclidean", border: bool = False, want: Sequence[str] = ("band",)):
    """gp_mask_band on a device tensor: a [B, H, W], [B, 1, H, W] or [H, W], a float map in [0, 1] (quantised to 8 bits by the kernel) or
    uint8.  A = {a > lo}, Bc = {a < hi} (-1 <= lo < hi <= 256).  Returns a dict of the uint8 [B, H, W] planes named in `want` (BAND_PLANES):
    band (within reach of A and of Bc), fg (out of Bc's reach), bg (out of A's reach), inner (in A, within Bc's reach), each 0 / 255, trimap
    (0 / 128 / 255).  metric "euclidean": reach is a squared radius (<= 2^24); "chebyshev": a radius (<= 4096).  border: the outside of the
    image counts as Bc.  Definitions in include/genpercept_hip.h; eval_metrics.mask_band gives the same bits.  Enqueued on the current
    stream, no synchronisation."""
    a = _eval_maps(a, "a")
    assert a.is_cuda
    if metric not in BAND_METRIC:
        raise ValueError(f"metric is 'euclidean' or 'chebyshev', got {metric!r}")
    want = list(want)
    if not want or any(k not in BAND_PLANES for k in want) or len(set(want)) != len(want):
        raise ValueError(f"want names one or more of {BAND_PLANES}, got {want}")
    a, is_u8 = _map8(a, "a")
    b, h, w = (int(v) for v in a.shape)
    planes = torch.empty((len(want), b, h, w), dtype=torch.uint8, device=a.device)
    outs = [_ptr(planes[want.index(k)]) if k in want else None for k in BAND_PLANES]
    ws, nbytes = _op_workspace("gp_mask_band", a.device, b, h, w)
    _launch("gp_mask_band", f"lo = {lo}, hi = {hi}, reach = {reach}, metric = {metric!r}, maps {(b, h, w)}", a.data_ptr(), int(is_u8), b, h, w, int(lo),
            int(hi), BAND_METRIC[metric], int(reach), int(bool(border)), *outs, ws.data_ptr(), nbytes, _stream_ptr(a.device))
    return {k: planes[j] for j, k in enumerate(want)}


def eval_trimap(pred: torch.Tensor, gt: torch.Tensor, radius: float, metric="euclidean"):
    """eval_metrics.trimap_metrics for a batch of maps that are on the device (pred, gt as `eval_mask_raw`): one gp_mask_band on the ground
    truth (lo = 0, hi = 255, nothing outside the image) gives the transition region and the two sides, three gp_eval_mask calls score the
    prediction over them.  Returns one dict per image: TRIMAP_METRICS, "n_t", "n_fg_side", "n_bg_side".  Raises ValueError naming the image
    when its transition region is empty.  One device -> host copy of 3 x B x 516 words."""
    from .eval_metrics import band_reach, trimap_from_counts
    gt = _eval_maps(gt, "gt")
    planes = mask_band(gt, 0, 255, band_reach(radius, metric), metric, False, want=("band", "fg", "bg"))
    counts = torch.stack([_eval_mask_launch(pred, gt, planes[k], True)[2] for k in ("band", "fg", "bg")]).cpu().numpy()
    res = []
    for i in range(counts.shape[1]):
        if counts[0, i, 0] == 0:
            raise ValueError(f"image {i}: no pixel in the transition region (n = 0)")
        res.append(trimap_from_counts(counts[0, i], counts[1, i], counts[2, i]))
    return res


def eval_boundary_iou(pred: torch.Tensor, gt: torch.Tensor, ratio: float = 0.02):
    """eval_metrics.boundary_iou for a batch of maps that are on the device (pred, gt as `eval_mask_raw`): the inner bands of G = gt > 128 and
    of P = q >= 128 (Chebyshev, d = boundary_reach(H, W, ratio), the outside of the image counts as the other side) from two gp_mask_band
    calls, their IoU from gp_eval_mask.  Returns one dict per image: "biou", "d", "n_gt_band", "n_pred_band".  One device -> host copy of
    B x (10 + 516) words."""
    from .eval_metrics import boundary_reach
    pred, _, gt, (b, h, w) = _pred_gt8(pred, gt)
    d = boundary_reach(h, w, ratio)
    g_d = mask_band(gt, 128, 129, d, "chebyshev", True, want=("inner",))["inner"]
    p_d = mask_band(pred, 127, 128, d, "chebyshev", True, want=("inner",))["inner"]
    raw, counts = _unpacked(_eval_mask_launch(p_d, g_d, None, True)[0], b, MASK_OUT)
    return [dict(biou=float(raw[i, 8]), d=d, n_gt_band=int(raw[i, 1]), n_pred_band=int(counts[i, 1]) // 255) for i in range(b)]


FOREGROUND_OUTPUTS = ["fg", "bg", "rgba", "comp"]


def foreground(image: torch.Tensor, alpha: torch.Tensor, background=None, want: Sequence[str] = ("rgba",), reg: float = 1e-5, gw: float = 1.0,
               n_small: int = 10, n_big: int = 2):
    """gp_foreground on device tensors: image uint8 [B, 3, H, W] ([3, H, W]: one image); alpha [B, H, W], [B, 1, H, W] or [H, W], a float map in [0, 1]
    (quantised to 8 bits by the kernel) or uint8.  Returns a dict of the outputs named in `want` (FOREGROUND_OUTPUTS): fg, bg float32
    [B, 3, H, W] (the estimated foreground and background colours), rgba uint8 [B, H, W, 4] (the cutout), comp uint8 [B, 3, H, W] (the
    foreground over `background`: a uint8 [B, 3, H, W] / [3, H, W] device image or one colour of three bytes).  Definition in
    include/genpercept_hip.h; genpercept_amd/foreground.py gives the same bits.  Enqueued on the current stream, no synchronisation."""
    from .foreground import check_options
    image = _images_u8(image, "image")
    alpha, is_u8 = _map8(_eval_maps(alpha, "alpha"), "alpha")
    b, h, w = (int(v) for v in alpha.shape)
    _same_batch(image, (b, h, w), alpha.device, "image")
    _post_dims(b, h, w, "a cutout", count_limit=False)
    reg, gw, n_small, n_big = check_options(reg, gw, n_small, n_big)
    want = list(want)
    if not want or any(k not in FOREGROUND_OUTPUTS for k in want) or len(set(want)) != len(want):
        raise ValueError(f"want names one or more of {FOREGROUND_OUTPUTS}, got {want}")
    new_bg, new_rgb = None, 0
    if "comp" in want:
        if background is None:
            raise ValueError("the composite needs a background: a uint8 image or one colour")
        if torch.is_tensor(background) and background.dim() >= 3:
            new_bg = _same_batch(_images_u8(background, "background"), (b, h, w), image.device, "background")
        else:
            rgb = [int(v) for v in (background.tolist() if hasattr(background, "tolist") else background)]
            if len(rgb) != 3 or any(not 0 <= v <= 255 for v in rgb):
                raise ValueError(f"background: one colour is three bytes, got {background!r}")
            new_rgb = rgb[0] << 16 | rgb[1] << 8 | rgb[2]
    assert image.is_cuda
    kinds = dict(fg=((b, 3, h, w), torch.float32), bg=((b, 3, h, w), torch.float32), rgba=((b, h, w, 4), torch.uint8), comp=((b, 3, h, w), torch.uint8))
    outs = {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=image.device) for k in want}
    ws, nbytes = _op_workspace("gp_foreground", image.device, b, h, w)
    _launch("gp_foreground", f"images {(b, h, w)}, reg = {reg}, gw = {gw}, n_small = {n_small}, n_big = {n_big}", image.data_ptr(), alpha.data_ptr(),
            int(is_u8), b, h, w, float(reg), float(gw), n_small, n_big, _ptr(new_bg), new_rgb, *[_ptr(outs.get(k)) for k in FOREGROUND_OUTPUTS],
            ws.data_ptr(), nbytes, _stream_ptr(image.device))
    return outs


def estimate_foreground(image: torch.Tensor, alpha: torch.Tensor, reg: float = 1e-5, gw: float = 1.0, n_small: int = 10, n_big: int = 2):
    """foreground.estimate_foreground for a batch on the device (arguments as `foreground`): (F, B), float32 [B, 3, H, W] each."""
    o = foreground(image, alpha, want=("fg", "bg"), reg=reg, gw=gw, n_small=n_small, n_big=n_big)
    return o["fg"], o["bg"]


def cutout(image: torch.Tensor, alpha: torch.Tensor, background=None, reg: float = 1e-5, gw: float = 1.0, n_small: int = 10, n_big: int = 2):
    """The cutout of a batch on the device (arguments as `foreground`): without a background the RGBA image uint8 [B, H, W, 4]
    (foreground.cutout_rgba), with one the composite over it, uint8 [B, 3, H, W] (foreground.composite).  The float planes are not written."""
    k = "rgba" if background is None else "comp"
    return foreground(image, alpha, background, want=(k,), reg=reg, gw=gw, n_small=n_small, n_big=n_big)[k]


def guided_upsample(guide_lo: torch.Tensor, pred: torch.Tensor, guide: torch.Tensor, radius: int = 4, eps: float = 1e-4) -> torch.Tensor:
    """gp_guided_upsample on device tensors: guide_lo uint8 [B, 3, h, w] (the image at the processing size), pred float [B, C, h, w], C = 1 or
    3 (the prediction at that size), guide uint8 [B, 3, H, W] (the image at the output size); a single image may come without the batch axis.
    Returns float32 [B, C, H, W] in [0, 1]: the prediction upsampled with the image as guide (guided filter, window radius 1 .. 32, eps in
    (0, 1]).  Definition in include/genpercept_hip.h; genpercept_amd/guided.py gives the same bits.  Allocates the workspace; enqueued on the
    current stream, no synchronisation."""
    from .guided import check_options
    guide_lo, guide, pred = _images_u8(guide_lo, "guide_lo"), _images_u8(guide, "guide"), _float32(pred, "pred")
    if pred.dim() not in (3, 4):
        raise ValueError(f"pred: float [B, C, h, w] or [C, h, w], got {tuple(pred.shape)}")
    pred = (pred[None] if pred.dim() == 3 else pred).contiguous()
    b, c, h, w = (int(v) for v in pred.shape)
    hh, ww = int(guide.shape[-2]), int(guide.shape[-1])
    if c not in (1, 3):
        raise ValueError(f"pred {tuple(pred.shape)} needs 1 or 3 channels")
    _same_batch(guide_lo, (b, h, w), pred.device, "guide_lo")
    _same_batch(guide, (b, hh, ww), pred.device, "guide")
    _post_dims(b, h, w, "guided upsampling", count_limit=False)
    _post_dims(b, hh, ww, "guided upsampling", count_limit=False)
    radius, eps = check_options(radius, eps)
    assert pred.is_cuda
    out = torch.empty((b, c, hh, ww), dtype=torch.float32, device=pred.device)
    ws, nbytes = _op_workspace("gp_guided_upsample", pred.device, b, c, h, w)
    _launch("gp_guided_upsample", f"{(b, c, h, w)} -> {(hh, ww)}, radius = {radius}, eps = {eps}", guide_lo.data_ptr(), pred.data_ptr(), c, guide.data_ptr(),
            b, h, w, hh, ww, radius, eps, out.data_ptr(), ws.data_ptr(), nbytes, _stream_ptr(pred.device))
    return out


def tile_merge(base: torch.Tensor, tiles: torch.Tensor, ys, xs, overlap: int, align: str = "least_square", want_fit: bool = False):
    """gp_tile_merge on device tensors: base float [B, C, H, W], C = 1 or 3 (the maps of the whole images at the input size), tiles float
    [B, N, C, wh, ww] (the maps of the windows, N = ny * nx, numbered iy * nx + ix); a single image may come without the batch axis.  ys [ny],
    xs [nx]: the origins of the grid as `tiled.tile_grid` gives them (host integers; they are checked against the grid rule); overlap: the
    grid's; align: "least_square" (every tile is fitted onto the base by scale and shift) or "none".  Returns float32 [B, C, H, W] in [0, 1],
    and with want_fit (out, fit) with fit float64 [B, N, 2] = (s, t) of every tile.  Definition in include/genpercept_hip.h;
    genpercept_amd/tiled.py gives the same bits.  Allocates the workspace; enqueued on the current stream, no synchronisation."""
    from .tiled import ALIGNMENTS
    base, tiles = _float32(base, "base"), _float32(tiles, "tiles")
    if base.dim() == 3 and tiles.dim() == 4:
        base, tiles = base[None], tiles[None]
    if base.dim() != 4 or tiles.dim() != 5 or tiles.shape[0] != base.shape[0] or tiles.shape[2] != base.shape[1] or base.shape[1] not in (1, 3):
        raise ValueError(f"base [B, C, H, W] with C = 1 or 3 and tiles [B, N, C, wh, ww], got {tuple(base.shape)} and {tuple(tiles.shape)}")
    if align not in ALIGNMENTS:
        raise ValueError(f"align is one of {ALIGNMENTS}, got {align!r}")
    base, tiles = base.contiguous(), tiles.contiguous()
    ys_c, xs_c = (np.ascontiguousarray(np.asarray(v.cpu() if torch.is_tensor(v) else v)) for v in (ys, xs))
    if any(v.ndim != 1 or v.dtype.kind not in "iu" or v.size < 1 for v in (ys_c, xs_c)):
        raise ValueError("ys and xs are one-dimensional integer arrays")
    ys_c, xs_c = ys_c.astype(np.int32), xs_c.astype(np.int32)
    b, c, h, w = (int(v) for v in base.shape)
    n, wh, ww = int(tiles.shape[1]), int(tiles.shape[3]), int(tiles.shape[4])
    ny, nx = int(ys_c.size), int(xs_c.size)
    if n != ny * nx:
        raise ValueError(f"{ny} x {nx} origins do not number the {n} tiles")
    assert base.is_cuda and tiles.is_cuda and base.device == tiles.device
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=base.device)
    fit = torch.empty((b, n, 2), dtype=torch.float64, device=base.device) if want_fit else None
    ws, nbytes = _op_workspace("gp_tile_merge", base.device, b, c, h, w, ny, nx, wh, ww)
    _launch("gp_tile_merge", f"base {(b, c, h, w)}, {ny} x {nx} tiles of {wh} x {ww}, overlap = {overlap}, ys = {ys_c.tolist()}, xs = {xs_c.tolist()}: "
            "not the grid of the rule, or outside its ranges", base.data_ptr(), tiles.data_ptr(), b, c, h, w, ys_c.ctypes.data, ny, xs_c.ctypes.data, nx,
            wh, ww, int(overlap), ALIGNMENTS.index(align), _ptr(fit), out.data_ptr(), ws.data_ptr(), nbytes, _stream_ptr(base.device))
    return (out, fit) if want_fit else out


def depth_geometry(pred: torch.Tensor, cameras=None, image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, space: str = "depth",
                   radius: int = 2, tau: float = 0.05, min_count: Optional[int] = None, min_cos: Optional[float] = None, stride: int = 1):
    """gp_depth_geometry on device tensors: pred float [B, 1, H, W] ([B, H, W] and [H, W] too), a depth or disparity map in [0, 1]; cameras None
    (`geometry.default_camera`, a viewing convention), eight values s, t, fx, fy, cx, cy, z_min, z_max for every image or a HOST [B, 8] array;
    image uint8 [B, 3, H, W] or None (the points' colours); mask [B, H, W] or None (non-zero: usable); space "depth" or "disparity"; radius
    1 .. 8, tau in (0, 1], min_count 3 .. (2 r + 1)^2 (default 2 r + 1), min_cos in [0, 1) (default cos 85 degrees), stride 1 .. 64.  Returns a
    dict of device tensors: xyz float32 [B, 3, H, W] (NaN where the pixel is invalid), normal float32 [B, 3, H, W] (camera-facing unit
    vectors, zero without a fit), keep uint8 [B, H, W], and the point cloud without flying pixels -- points float32 [n, 3],
    point_normals float32 [n, 3], point_rgb uint8 [n, 3], point_index int32 [n] (v * W + u) -- with offsets, a HOST int64 [B + 1] array
    (image k owns the points offsets[k] .. offsets[k + 1]): the point arrays are sliced by one read of it, the only synchronisation.
    Definition in include/genpercept_hip.h; genpercept_amd/geometry.py gives the same bits.  Allocates the workspace and, for the point
    arrays, the worst case B * ceil(H / stride) * ceil(W / stride)."""
    from .geometry import check_cameras, check_options
    pred = _float_maps(pred, "pred")
    b, h, w = (int(v) for v in pred.shape)
    dev = pred.device
    if image is not None:
        image = _same_batch(_images_u8(image, "image"), (b, h, w), dev, "image")
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")
    radius, tau, min_count, min_cos, stride = check_options(radius, tau, min_count, min_cos, stride)
    _post_dims(b, h, w, "depth geometry")
    cams = check_cameras(cameras.cpu().numpy() if torch.is_tensor(cameras) else cameras, b, h, w)
    assert pred.is_cuda
    if mask is not None:
        mask = _mask_u8(mask, "mask", (b, h, w))
    out = dict(xyz=torch.empty((b, 3, h, w), dtype=torch.float32, device=dev), normal=torch.empty((b, 3, h, w), dtype=torch.float32, device=dev),
               keep=torch.empty((b, h, w), dtype=torch.uint8, device=dev))
    cap = b * (-(-h // stride)) * (-(-w // stride))
    pts = dict(points=torch.empty((cap, 3), dtype=torch.float32, device=dev), point_normals=torch.empty((cap, 3), dtype=torch.float32, device=dev),
               point_rgb=torch.empty((cap, 3), dtype=torch.uint8, device=dev), point_index=torch.empty((cap,), dtype=torch.int32, device=dev),
               offsets=torch.empty((b + 1,), dtype=torch.int64, device=dev))
    ws, nbytes = _op_workspace("gp_depth_geometry", dev, b, h, w, stride)
    _launch("gp_depth_geometry", f"maps {(b, h, w)}, radius = {radius}, tau = {tau}, min_count = {min_count}, min_cos = {min_cos}, stride = {stride}",
            pred.data_ptr(), _ptr(mask), _ptr(image), cams.ctypes.data, b, h, w, SPACES.index(space), radius, tau, min_count, min_cos, stride,
            out["xyz"].data_ptr(), out["normal"].data_ptr(), out["keep"].data_ptr(),
            *[pts[k].data_ptr() for k in ("points", "point_normals", "point_rgb", "point_index", "offsets")], ws.data_ptr(), nbytes, _stream_ptr(dev))
    offsets = pts["offsets"].cpu().numpy()   # (synchronises: `cams`, host memory the call reads in stream order, has been read by now)
    n = int(offsets[-1])
    out.update({k: pts[k][:n] for k in ("points", "point_normals", "point_rgb", "point_index")}, offsets=offsets)
    return out


def depth_mesh(pred: torch.Tensor, cameras=None, image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, space: str = "depth",
               radius: int = 2, tau: float = 0.05, min_count: Optional[int] = None, min_cos: Optional[float] = None, stride: int = 1, cut: float = 0.05):
    """gp_depth_geometry for the three planes (no point arrays), then gp_depth_mesh on them, on one stream: the arguments of `depth_geometry`
    and cut in (0, 1] (0.05, a convention): grid nodes whose depths differ by more than cut times the nearer one are not joined.  Returns a
    dict of device tensors: xyz, normal float32 [B, 3, H, W], keep uint8 [B, H, W] and the triangle mesh cut at depth edges -- vertices,
    vertex_normals float32 [n, 3], vertex_rgb uint8 [n, 3] (255 without an image), vertex_uv float32 [n, 2], vertex_index int32 [n] (v * W + u),
    faces int32 [m, 3] (indices local to the image) -- with vertex_offsets and face_offsets, HOST int64 [B + 1] arrays (image k owns the
    vertices vertex_offsets[k] .. vertex_offsets[k + 1] and the faces likewise): the arrays are sliced by one read of the two, the only
    synchronisation.  Definition in include/genpercept_hip.h; genpercept_amd/mesh.py gives the same bits.  Allocates both workspaces and,
    for the arrays, the worst case B * gh * gw vertices and 2 * B * (gh - 1) * (gw - 1) faces."""
    from .geometry import check_cameras
    from .mesh import MAX_NODES, check_mesh_options
    pred = _float_maps(pred, "pred")
    b, h, w = (int(v) for v in pred.shape)
    dev = pred.device
    if image is not None:
        image = _same_batch(_images_u8(image, "image"), (b, h, w), dev, "image")
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")
    o = check_mesh_options(radius, tau, min_count, min_cos, stride, cut)
    _post_dims(b, h, w, "a depth mesh")
    gh, gw = -(-h // o["stride"]), -(-w // o["stride"])
    if b * gh * gw >= MAX_NODES:
        raise ValueError(f"a depth mesh takes B * gh * gw < 2^30 grid nodes, got {(b, gh, gw)}")
    cams = check_cameras(cameras.cpu().numpy() if torch.is_tensor(cameras) else cameras, b, h, w)
    assert pred.is_cuda
    if mask is not None:
        mask = _mask_u8(mask, "mask", (b, h, w))
    out = dict(xyz=torch.empty((b, 3, h, w), dtype=torch.float32, device=dev), normal=torch.empty((b, 3, h, w), dtype=torch.float32, device=dev),
               keep=torch.empty((b, h, w), dtype=torch.uint8, device=dev))
    n_cap, m_cap = b * gh * gw, 2 * b * (gh - 1) * (gw - 1)
    arrays = dict(vertices=torch.empty((n_cap, 3), dtype=torch.float32, device=dev), vertex_normals=torch.empty((n_cap, 3), dtype=torch.float32, device=dev),
                  vertex_rgb=torch.empty((n_cap, 3), dtype=torch.uint8, device=dev), vertex_uv=torch.empty((n_cap, 2), dtype=torch.float32, device=dev),
                  vertex_index=torch.empty((n_cap,), dtype=torch.int32, device=dev), faces=torch.empty((m_cap, 3), dtype=torch.int32, device=dev))
    both = torch.empty((2, b + 1), dtype=torch.int64, device=dev)    # vertex_offsets, face_offsets: one copy brings both to the host
    ws_g, nbytes_g = _op_workspace("gp_depth_geometry", dev, b, h, w, o["stride"])
    ws_m, nbytes_m = _op_workspace("gp_depth_mesh", dev, b, h, w, o["stride"])
    describe = f"maps {(b, h, w)}, " + ", ".join(f"{k} = {v}" for k, v in o.items())
    _launch("gp_depth_geometry", describe, pred.data_ptr(), _ptr(mask), _ptr(image), cams.ctypes.data, b, h, w, SPACES.index(space), o["radius"], o["tau"],
            o["min_count"], o["min_cos"], o["stride"], out["xyz"].data_ptr(), out["normal"].data_ptr(), out["keep"].data_ptr(), None, None, None, None, None,
            ws_g.data_ptr(), nbytes_g, _stream_ptr(dev))
    _launch("gp_depth_mesh", describe, out["xyz"].data_ptr(), out["normal"].data_ptr(), out["keep"].data_ptr(), _ptr(image), b, h, w, o["stride"], o["cut"],
            *[arrays[k].data_ptr() for k in ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "vertex_index", "faces")],
            both[0].data_ptr(), both[1].data_ptr(), ws_m.data_ptr(), nbytes_m, _stream_ptr(dev))
    offsets = both.cpu().numpy()   # (synchronises: `cams`, host memory the first call reads in stream order, has been read by now)
    n, m = int(offsets[0, -1]), int(offsets[1, -1])
    out.update({k: arrays[k][:m if k == "faces" else n] for k in arrays}, vertex_offsets=offsets[0].copy(), face_offsets=offsets[1].copy())
    return out


_LENS_TABLES: Dict = {}   # (device, the tables' bytes) -> (to_lin, from_lin) on that device


def _lens_tables(tables, device):
    from .lens_blur import check_tables
    to_lin, from_lin = check_tables(tables)
    key = (str(device), to_lin.tobytes(), from_lin.tobytes())
    if key not in _LENS_TABLES:
        if len(_LENS_TABLES) >= 16:
            _LENS_TABLES.clear()
        # (uint16 has no torch dtype everywhere: the table travels as int16 bits)
        _LENS_TABLES[key] = (torch.from_numpy(to_lin.view(np.int16).copy()).to(device), torch.from_numpy(from_lin.copy()).to(device))
    return _LENS_TABLES[key]


def lens_blur(image: torch.Tensor, pred: torch.Tensor, focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0, space: str = "depth",
              sharp: Optional[torch.Tensor] = None, tables=None, want_coc: bool = False):
    """gp_lens_blur on device tensors: the images refocused under their maps, synthetic depth of field.  image uint8 [B, 3, H, W] ([3, H, W]: one
    image); pred float [B, 1, H, W] ([B, H, W] and [H, W] too), a depth or disparity map in [0, 1]; exactly one of focus (a value of the map in
    [0, 1]) and focus_at (a pixel (u, v): the focus is that pixel's nearness, read on the device); aperture, the blur radius in pixels at the
    far end of the scale; max_radius <= 32 pixels; dof, the half-width of the sharp zone in map units -- each one value or one per image;
    space "depth" or "disparity"; sharp [B, H, W] or None (non-zero pins the pixel sharp); tables None (`lens_blur.srgb_tables`) or a HOST
    pair (to_lin uint16 [256], from_lin uint8 [4096]).  Returns uint8 [B, 3, H, W] on the device, and with want_coc (out, coc) with coc the
    circle of confusion in eighths of a pixel, int16 [B, H, W] (0 .. 256).  Definition in include/genpercept_hip.h;
    genpercept_amd/lens_blur.py gives the same bits.  Enqueued on the current stream, no synchronisation, nothing read back."""
    from .lens_blur import lens_blur_options
    image, pred, (b, h, w), dev = _image_and_maps(image, pred, space, "lens blur")
    o = lens_blur_options(b, focus, focus_at, aperture, max_radius, dof)
    _pixel_inside(o["focus_at"], "focus_at", h, w)
    assert pred.is_cuda
    if sharp is not None:
        sharp = _mask_u8(sharp, "sharp", (b, h, w))
    to_lin, from_lin = _lens_tables(tables, dev)
    host = np.stack([np.zeros(b, np.int64), o["gain"], o["cmax8"], o["dz"]], 1).astype(np.int32)
    near = _nearness_plane(pred, o["focus"], o["focus_at"], space)
    params = torch.from_numpy(host).to(dev, non_blocking=True)
    params[:, 0] = near
    out = torch.empty((b, 3, h, w), dtype=torch.uint8, device=dev)
    coc = torch.empty((b, h, w), dtype=torch.int16, device=dev) if want_coc else None
    max_c8 = int(o["cmax8"].max())
    _launch("gp_lens_blur", f"images {(b, h, w)}, space = {space}, max_c8 = {max_c8}", image.data_ptr(), pred.data_ptr(), _ptr(sharp), params.data_ptr(),
            to_lin.data_ptr(), from_lin.data_ptr(), b, h, w, SPACES.index(space), max_c8, out.data_ptr(), _ptr(coc), _stream_ptr(dev))
    return (out, coc) if want_coc else out


def stereo_views(image: torch.Tensor, pred: torch.Tensor, layout="sbs", views=2, separation=16.0, converge=None, converge_at=None, edge=0.04,
                 space: str = "depth", want_holes: bool = False, want_near: bool = False, canvas: Optional[torch.Tensor] = None):
    """gp_stereo_views on device tensors: the images re-rendered from viewpoints shifted sideways under their maps -- a stereo pair, an
    anaglyph, a quilt.  image uint8 [B, 3, H, W] ([3, H, W]: one image); pred float [B, 1, H, W] ([B, H, W] and [H, W] too), a depth or
    disparity map in [0, 1]; layout "pair", "sbs", "over_under", "anaglyph" or "quilt" with views a count or, for a quilt, (ny, nx);
    separation, the parallax in pixels between the outermost views at the two ends of the nearness scale; at most one of converge (a value of
    the map in [0, 1]) and converge_at (a pixel (u, v), read on the device) -- each one value or one per image --, the zero-parallax plane,
    the middle of the scale with neither; edge, the fraction of the map's range beyond which neighbours are cut apart (0.04: a convention);
    space "depth" or "disparity"; canvas None or a uint8 [B, 3, CH, CW] tensor of the layout's size to write into (bytes no view writes
    keep what they held).  Returns the canvas uint8 [B, 3, CH, CW] on the device, and with want_holes / want_near a tuple with holes uint8
    [B, V, H, W] (1: a disocclusion) and near int16 [B, V, H, W] (the bits of the uint16 nearness of the new view) after it.  Definition in
    include/genpercept_hip.h; genpercept_amd/stereo.py gives the same bits and states the rule from these terms to the call's integers.
    Allocates the workspace; enqueued on the current stream, no synchronisation, nothing read back."""
    from .stereo import plan
    image, pred, (b, h, w), dev = _image_and_maps(image, pred, space, "stereo views")
    o = plan(b, h, w, layout, views, separation, converge, converge_at, edge)
    table, (ch, cw), n_views = o["table"], o["size"], int(o["table"].shape[0])
    canvas = _output_u8(canvas, "canvas", (b, 3, ch, cw), dev)   # (a new one holds no bytes to keep: the views of every layout cover it)
    assert pred.is_cuda
    conv = _nearness_plane(pred, o["converge"], o["converge_at"], space, F_DEFAULT)
    holes, near, result = _warp_planes(canvas, (b, n_views, h, w), want_holes, want_near)
    ws, nbytes = _op_workspace("gp_stereo_views", dev, b, n_views, h, w)
    _launch("gp_stereo_views", f"images {(b, h, w)}, {n_views} views in a canvas of {(ch, cw)}, space = {space}, edge = {o['edge']}, max_s8 = {o['max_s8']}",
            image.data_ptr(), pred.data_ptr(), conv.data_ptr(), table.ctypes.data, b, n_views, h, w, ch, cw, SPACES.index(space), o["edge"], o["max_s8"],
            canvas.data_ptr(), _ptr(holes), _ptr(near), ws.data_ptr(), nbytes, _stream_ptr(dev))
    return result


def parallax_frames(image: torch.Tensor, pred: torch.Tensor, path="orbit", frames: int = 16, amount: float = 16.0, push: float = 0.0,
                    zoom: float = 1.0, pan: bool = False, focus=None, focus_at=None, edge=0.04, overscan: bool = True, frame_range=None,
                    space: str = "depth", want_holes: bool = False, want_near: bool = False, out: Optional[torch.Tensor] = None):
    """gp_parallax_frames on device tensors: the frames of a camera move from one photograph -- the "3-D photo".  image uint8 [B, 3, H, W]
    ([3, H, W]: one image); pred float [B, 1, H, W] ([B, H, W] and [H, W] too), a depth or disparity map in [0, 1]; path "swing", "orbit"
    or "dolly" with `frames` frames, `amount` (the parallax in pixels between the two ends of the nearness scale), and for the dolly `push`,
    `zoom` and `pan`, or an explicit [V, 4] array of (shift_x, shift_y, push, zoom) per frame; at most one of focus (a value of the map in
    [0, 1]) and focus_at (a pixel (u, v), read on the device) -- each one value or one per image --, the plane that stays put, the middle of
    the scale with neither; edge, the fraction of the map's range beyond which neighbours are cut apart; overscan, which zooms each frame in
    by its largest displacement so that no border shows; frame_range = (first, end), the frames of the path this call renders (at most 64;
    all of them without it); space "depth" or "disparity"; out None or a contiguous uint8 [B, V, 3, H, W] tensor to write into.  Returns the
    frames uint8 [B, V, 3, H, W] on the device, and with want_holes / want_near a tuple with holes uint8 [B, V, H, W] (1: a disocclusion)
    and near int16 [B, V, H, W] (the bits of the uint16 nearness of the frame) after it.  Definition in include/genpercept_hip.h;
    genpercept_amd/parallax.py gives the same bits and states the rule from these terms to the call's integers.  Allocates the workspace;
    enqueued on the current stream, no synchronisation, nothing read back."""
    from .parallax import plan
    image, pred, (b, h, w), dev = _image_and_maps(image, pred, space, "parallax frames")
    o = plan(b, h, w, path, frames, amount, push, zoom, pan, focus, focus_at, edge, overscan, frame_range)
    table, n_frames = o["table"], int(o["table"].shape[0])
    out = _output_u8(out, "out", (b, n_frames, 3, h, w), dev)   # (every byte is written)
    assert pred.is_cuda
    plane = _nearness_plane(pred, o["focus"], o["focus_at"], space, F_DEFAULT)
    holes, near, result = _warp_planes(out, (b, n_frames, h, w), want_holes, want_near)
    ws, nbytes = _op_workspace("gp_parallax_frames", dev, b, n_frames, h, w)
    _launch("gp_parallax_frames", f"images {(b, h, w)}, {n_frames} frames, space = {space}, edge = {o['edge']}, max_s8 = {o['max_s8']}",
            image.data_ptr(), pred.data_ptr(), plane.data_ptr(), table.ctypes.data, b, n_frames, h, w, SPACES.index(space), o["edge"], o["max_s8"],
            out.data_ptr(), _ptr(holes), _ptr(near), ws.data_ptr(), nbytes, _stream_ptr(dev))
    return result


def relight(image: torch.Tensor, normal: torch.Tensor, pred: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, lights=True,
            ambient=0.35, relief=64.0, encoded: bool = True, flip=(False, False, False), space: str = "depth", tables=None,
            want_shadow: bool = False):
    """gp_relight on device tensors: the images under new directional lights, shaded by their normal maps with cast shadows from their depth
    or disparity maps.  image uint8 [B, 3, H, W] ([3, H, W]: one image); normal float [B, 3, H, W], encoded in [0, 1] (the pipeline's normal
    mode) or raw in [-1, 1] (`depth_geometry`'s normals: encoded=False); pred float [B, 1, H, W] ([B, H, W] and [H, W] too) or None (no
    shadows); weight uint8 [B, H, W] or None (255: relit, 0: the image; a matting alpha as bytes relights the subject only); lights True
    (`relight.DEFAULT_LIGHT`), a dict over its keys or up to 8 of them, or a HOST integer table [L + 1, 20] (`relight.relight_lights`), with
    which ambient and relief are not read; ambient one value or three; relief, the height in pixels of the map's full range; flip, a sign
    per axis; space "depth" or "disparity"; tables None (`lens_blur.srgb_tables`) or a HOST pair (to_lin, from_lin).  Returns uint8
    [B, 3, H, W] on the device, and with want_shadow (out, shadow) with shadow uint8 [B, H, W], the darkest shade over the lights.
    Definition in include/genpercept_hip.h; genpercept_amd/relight.py gives the same bits.  Enqueued on the current stream, no
    synchronisation, nothing read back."""
    from .relight import REACH, check_flip, check_rows, check_tables, relight_lights
    image = _images_u8(image, "image")
    b, _, h, w = (int(v) for v in image.shape)
    dev = image.device
    normal = _float32(normal, "normal")
    normal = (normal[None] if normal.dim() == 3 else normal).contiguous()
    if tuple(normal.shape) != (b, 3, h, w) or normal.device != dev:
        raise ValueError(f"normal {tuple(normal.shape)} on {normal.device} and image {(b, 3, h, w)} on {dev}: three planes per image, same size, same device")
    if pred is not None:
        pred = _float_maps(pred, "pred")
        _same_batch(image, tuple(int(v) for v in pred.shape), pred.device, "image")
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")
    _post_dims(b, h, w, "relight")
    if weight is not None:
        if not torch.is_tensor(weight) or weight.dtype != torch.uint8 or weight.device != dev:
            raise ValueError(f"weight: a uint8 tensor on {dev}, got {weight.dtype if torch.is_tensor(weight) else type(weight)}")
        weight = _eval_maps(weight, "weight").contiguous()   # (its bytes are weights, not a mask: `_mask_u8` would take any dtype through != 0)
        if tuple(weight.shape) != (b, h, w):
            raise ValueError(f"weight {tuple(weight.shape)} does not match the images {(b, h, w)}")
    rows = check_rows(lights) if isinstance(lights, np.ndarray) else relight_lights(lights, ambient, relief)
    bits = check_flip(flip)
    check_tables(tables)   # (refused before the device is asked for)
    n_lights, max_reach = int(rows.shape[0]) - 1, int(rows[:-1, REACH].max())
    assert image.is_cuda
    to_lin, from_lin = _lens_tables(tables, dev)
    out = torch.empty((b, 3, h, w), dtype=torch.uint8, device=dev)
    shadow = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if want_shadow else None
    _launch("gp_relight", f"images {(b, h, w)}, {n_lights} lights, space = {space}, max_reach = {max_reach}", image.data_ptr(), normal.data_ptr(),
            _ptr(pred), _ptr(weight), rows.ctypes.data, to_lin.data_ptr(), from_lin.data_ptr(), b, h, w, n_lights, int(bool(encoded)), bits,
            SPACES.index(space), max_reach, out.data_ptr(), _ptr(shadow), _stream_ptr(dev))
    return (out, shadow) if want_shadow else out


SEG_OUT = 8       # n, n_void, SEG_METRICS (out[2 .. 6]), n_classes; iou[K] follows
SEG_NSUM = 3       # n, n_void, sum_d in front of the K x K matrix of counts_out


def _seg_pred(pred: torch.Tensor):
    """pred [B, 3, H, W] or [3, H, W], float or uint8 -> (contiguous fp32 / uint8 [B, 3, H, W], is_u8)"""
    if not torch.is_tensor(pred) or pred.dim() not in (3, 4) or pred.shape[-3] != 3:
        raise ValueError(f"pred: expected [B, 3, H, W] or [3, H, W], got {tuple(pred.shape) if torch.is_tensor(pred) else type(pred)}")
    if pred.dim() == 3:
        pred = pred[None]
    if min(pred.shape) < 1:
        raise ValueError(f"pred: empty map {tuple(pred.shape)}")
    return _map8(pred, "pred")


def _seg_palette(palette, device) -> torch.Tensor:
    pal = palette if torch.is_tensor(palette) else torch.from_numpy(np.array(palette))  # (a copy: the array may be read-only)
    if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= SEG_MAX_K:
        raise ValueError(f"palette: uint8 [K, 3] with 1 <= K <= {SEG_MAX_K}, got {pal.dtype} {tuple(pal.shape)}")
    return pal.to(device).contiguous()


def seg_decode(pred: torch.Tensor, palette, want_dist: bool = False):
    """gp_seg_decode on a device tensor: the classes of a seg colour map, uint8 [B, H, W] ON THE DEVICE -- per pixel the smallest index of the
    nearest palette colour (squared distance in integers on the 8-bit colour; eval_metrics.palette_labels, the same bits); with want_dist also
    the int32 [B, H, W] minimum distances.  pred: [B, 3, H, W] or [3, H, W], a float map in [0, 1] (quantised to 8 bits per channel by the
    kernel as run.py:449-455 does) or uint8 (the bytes `postprocess(..., q_bits=8)` returns); palette: uint8 [K, 3], tensor or array, K <= 192.
    Enqueued on the current stream, no synchronisation."""
    pred, is_u8 = _seg_pred(pred)
    pal = _seg_palette(palette, pred.device)
    assert pred.is_cuda
    b, _, h, w = (int(v) for v in pred.shape)
    labels = torch.empty((b, h, w), dtype=torch.uint8, device=pred.device)
    dist = torch.empty((b, h, w), dtype=torch.int32, device=pred.device) if want_dist else None
    _c_check(load_library().gp_seg_decode(pred.data_ptr(), int(is_u8), pal.data_ptr(), int(pal.shape[0]), b, h, w, labels.data_ptr(), _ptr(dist),
                                          _stream_ptr(pred.device)), "gp_seg_decode")
    return (labels, dist) if want_dist else labels


def _eval_seg_launch(pred, gt, palette, region, gt_tol, want_counts: bool, want_labels: bool):
    """The checks and the call of `eval_seg_raw`.  Returns (buf, out, counts, labels): out float64 [B, 8 + K] and counts int64 [B, 3 + K * K]
    (or None) are views of the one int64 device buffer `buf`, so that one copy brings both to the host."""
    pred_dim = pred.dim() if torch.is_tensor(pred) else 0
    pred, is_u8 = _seg_pred(pred)
    b, _, h, w = (int(v) for v in pred.shape)
    if not torch.is_tensor(gt) or gt.dtype != torch.uint8:
        raise ValueError(f"gt: a uint8 colour image [B, H, W, 3] or label map [B, H, W], got {gt.dtype if torch.is_tensor(gt) else type(gt)}")
    batch = (b,) if pred_dim == 4 else ()
    if gt.dim() == pred_dim and gt.shape[-1] == 3:
        labels_gt, want = False, batch + (h, w, 3)
    elif gt.dim() == pred_dim - 1:
        labels_gt, want = True, batch + (h, w)
    else:
        raise ValueError(f"gt {tuple(gt.shape)}: neither a colour image (last dimension 3, {pred_dim} dimensions) nor a label map ({pred_dim - 1})")
    if tuple(gt.shape) != want:
        raise ValueError(f"gt {tuple(gt.shape)} does not match pred {tuple(pred.shape)}: expected {want}")
    gt = gt.reshape((b, h, w) if labels_gt else (b, h, w, 3)).contiguous()
    pal = _seg_palette(palette, pred.device)
    k = int(pal.shape[0])
    gt_tol = int(gt_tol)
    if gt_tol < 0:
        raise ValueError(f"gt_tol: a squared distance >= 0, got {gt_tol}")
    if region is not None:
        region = _mask_u8(region, "region", (b, h, w))
    assert pred.is_cuda and gt.is_cuda
    lib = load_library()
    buf, out, counts = _packed(b, SEG_OUT + k, SEG_NSUM + k * k if want_counts else 0, pred.device)
    labels = torch.empty((b, h, w), dtype=torch.uint8, device=pred.device) if want_labels else None
    ws, nbytes = _workspace(lib.gp_eval_seg_workspace(b, h, w, k), pred.device)
    _c_check(lib.gp_eval_seg(pred.data_ptr(), int(is_u8), gt.data_ptr(), int(labels_gt), gt_tol, _ptr(region), pal.data_ptr(), k, b, h, w, out.data_ptr(),
                             _ptr(counts), _ptr(labels), ws.data_ptr(), nbytes, _stream_ptr(pred.device)), "gp_eval_seg")
    return buf, out, counts, labels


def eval_seg_raw(pred: torch.Tensor, gt: torch.Tensor, palette, region: Optional[torch.Tensor] = None, gt_tol: int = 0, want_counts: bool = False,
                 want_labels: bool = False):
    """gp_eval_seg on device tensors: float64 [B, 8 + K] ON THE DEVICE = n, n_void, then SEG_METRICS, n_classes and the K per-class IoUs (NaN
    after n_void for an image without a scored pixel; definitions in include/genpercept_hip.h); with want_counts also the int64
    [B, 3 + K * K] counts n, n_void, sum_d, conf[g][c] (eval_metrics.seg_counts), with want_labels the uint8 [B, H, W] classes of the prediction
    (`seg_decode`), in that order.  pred, palette as for `seg_decode`.  gt: uint8, the colour image [B, H, W, 3] (last dimension 3, as many
    dimensions as pred: decoded by the same rule, a pixel farther than the squared distance gt_tol from every palette colour is void) or the
    label map [B, H, W] (one dimension fewer: values >= K are void).  region: bool or integer [B, H, W], non-zero = scored, None = every pixel.
    Enqueued on the current stream, no synchronisation."""
    _, out, counts, labels = _eval_seg_launch(pred, gt, palette, region, gt_tol, want_counts, want_labels)
    res = (out,) + ((counts,) if want_counts else ()) + ((labels,) if want_labels else ())
    return res if len(res) > 1 else out


def eval_seg(pred: torch.Tensor, gt: torch.Tensor, palette, region: Optional[torch.Tensor] = None, gt_tol: int = 0):
    """eval_metrics.seg_metrics for a batch of maps that are on the device (arguments as `eval_seg_raw`).  Returns one dict per image:
    SEG_METRICS, "n", "n_void", "n_classes", "iou" (float64 numpy [K]) and "conf" (int64 numpy [K, K], row = ground truth).  Raises ValueError
    naming the image when it has no scored pixel.  One device -> host copy of B x (8 + K + 3 + K * K) words."""
    buf, out, _, _ = _eval_seg_launch(pred, gt, palette, region, gt_tol, True, False)
    k = out.shape[1] - SEG_OUT
    raw, cnt = _unpacked(buf, out.shape[0], out.shape[1])
    res = []
    for i, row in enumerate(raw):
        if row[0] == 0:
            raise ValueError(f"image {i}: no pixel to evaluate the segmentation on (n = 0)")
        d = {name: float(row[2 + j]) for j, name in enumerate(SEG_METRICS)}
        d.update(n=int(row[0]), n_void=int(row[1]), n_classes=int(row[7]), iou=row[SEG_OUT:].copy(), conf=cnt[i, SEG_NSUM:].reshape(k, k).copy())
        res.append(d)
    return res


ENSEMBLE_REDUCTION = {"median": 0, "mean": 1}


def ensemble_gather(depth: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None):
    """gp_ensemble_gather on the members depth fp32 [B, E, H, W] ON THE DEVICE: (small [B, E, h, w], minmax [B, E, 2]) = the nearest-exact
    reduction `image_util.resize_max_res(depth, max_res, "nearest-exact")` for (h, w) = `image_util.resize_max_res_size(H, W, max_res)` and each
    reduced member's (min, max).  `out`: an fp32 device buffer of B * E * (h * w + 2) elements to carve both results from (so that one copy
    brings them to the host).  Enqueued on the current stream, no synchronisation."""
    assert depth.is_cuda and depth.dim() == 4
    depth = depth.to(torch.float32).contiguous()
    b, e, hh, ww = (int(v) for v in depth.shape)
    n = b * e * int(h) * int(w)
    if out is None:
        out = torch.empty((n + b * e * 2,), dtype=torch.float32, device=depth.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n + b * e * 2
    small, minmax = out[:n].view(b, e, int(h), int(w)), out[n:].view(b, e, 2)
    st = load_library().gp_ensemble_gather(depth.data_ptr(), b, e, hh, ww, int(h), int(w), small.data_ptr(), minmax.data_ptr(), _stream_ptr(depth.device))
    if st != GP_OK:
        raise RuntimeError(f"gp_ensemble_gather failed ({st})")
    return small, minmax


def ensemble_reduce(depth: torch.Tensor, scale=None, shift=None, reduction: str = "median", output_uncertainty: bool = False):
    """gp_ensemble_reduce on the members depth fp32 [B, E, H, W] ON THE DEVICE: per pixel a_e = depth_e * scale_e + shift_e (fp32, no FMA),
    the median (torch.median: lower middle) or mean over the members, per-image rescale to [0, 1] -> (pred [B, H, W], uncertainty [B, H, W] or
    None).  scale, shift: [B, E] (any tensor / array; cast to fp32); scale None = ones (no alignment), shift None = scale-only (d_min = 0).
    Enqueued on the current stream, no synchronisation."""
    assert depth.is_cuda and depth.dim() == 4
    if reduction not in ENSEMBLE_REDUCTION:
        raise ValueError(f"Unrecognized reduction method: {reduction}.")
    depth = depth.to(torch.float32).contiguous()
    b, e, h, w = (int(v) for v in depth.shape)
    host = [torch.ones((b, e), dtype=torch.float32) if scale is None else torch.as_tensor(scale).to(torch.float32).reshape(b, e)]
    if shift is not None:
        host.append(torch.as_tensor(shift).to(torch.float32).reshape(b, e))
    if len({t.device for t in host}) > 1:
        host = [t.to(depth.device) for t in host]
    par = torch.stack(host).to(depth.device).contiguous()  # one upload when both come from the host
    lib = load_library()
    pred = torch.empty((b, h, w), dtype=torch.float32, device=depth.device)
    unc = torch.empty((b, h, w), dtype=torch.float32, device=depth.device) if output_uncertainty else None
    ws, nbytes = _workspace(lib.gp_ensemble_workspace(b, e, h, w), depth.device)
    st = lib.gp_ensemble_reduce(depth.data_ptr(), par[0].data_ptr(), par[1].data_ptr() if shift is not None else None, b, e, h, w,
                                ENSEMBLE_REDUCTION[reduction], pred.data_ptr(), _ptr(unc), ws.data_ptr(), nbytes, _stream_ptr(depth.device))
    if st != GP_OK:
        raise RuntimeError(f"gp_ensemble_reduce failed ({st})")
    return pred, unc


def mfma_peak_tflops(device: int = 0, precision: Optional[str] = None) -> float:
    """Measured MFMA peak of this chip (TFLOP/s, dense, the library's 16-bit element type)."""
    return float(load_library(precision).gp_mfma_peak_tflops(device, _stream_ptr()))


def mfma_peak_tflops_shape(device: int = 0, shape: int = 0, precision: Optional[str] = None) -> float:
    """the same for one MFMA shape: 0 = v_mfma_f32_32x32x16, 1 = v_mfma_f32_16x16x32 (the conv / GEMM kernels' instruction)"""
    return float(load_library(precision).gp_mfma_peak_tflops_shape(device, shape, _stream_ptr()))


def mfma_lds_probe(device: int = 0, reads_per_16_mfma: int = 8, waves_per_simd: int = 2, mode: int = 0, precision: Optional[str] = None) -> float:
    """TFLOP/s of 16 MFMAs + `reads_per_16_mfma` ds_read_b128 per wave and iteration (gp_mfma_lds_probe): the conv inner loop in isolation
    (mode 0) or with barrier / DMA ring / ring reads / halo stream added (mode bits 1 / 2 / 4 / 16; 8 = MUBUF DMA)"""
    return float(load_library(precision).gp_mfma_lds_probe(device, reads_per_16_mfma, waves_per_simd, mode, _stream_ptr()))


def cross_attention_fold(y: torch.Tensor, U: torch.Tensor, u0: torch.Tensor, G: torch.Tensor, c0: torch.Tensor, g3: torch.Tensor, b3: torch.Tensor,
                         eps: float = 1e-5):
    """y [rows, C] (16-bit elements); returns (y_out, LayerNorm(y_out)).  See gp_cross_attention_fold."""
    lib = load_library()
    rows, c = y.shape
    y_out, n3 = torch.empty_like(y), torch.empty_like(y)
    st = lib.gp_cross_attention_fold(y.data_ptr(), y_out.data_ptr(), n3.data_ptr(), U.data_ptr(), u0.data_ptr(), G.data_ptr(), c0.data_ptr(),
                                     g3.data_ptr(), b3.data_ptr(), rows, c, U.shape[0], eps, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_cross_attention_fold failed ({st})")
    return y_out, n3


def softmax_rows(x: torch.Tensor, t: int, scale: float) -> torch.Tensor:
    lib = load_library()
    rows, ld = x.shape
    out = torch.empty((rows, ld), dtype=act_dtype(), device=x.device)
    if x.dtype == torch.float16:
        st = lib.gp_softmax_rows_f16(x.data_ptr(), out.data_ptr(), rows, t, ld, scale, _stream_ptr())
    else:
        st = lib.gp_softmax_rows(x.data_ptr(), out.data_ptr(), rows, t, ld, scale, _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_softmax_rows failed ({st})")
    return out


def bilinear(x_nhwc: torch.Tensor, out_hw, align_corners: bool) -> torch.Tensor:
    lib = load_library()
    b, h, w, c = x_nhwc.shape
    out = torch.empty((b, out_hw[0], out_hw[1], c), dtype=act_dtype(), device=x_nhwc.device)
    st = lib.gp_bilinear(x_nhwc.data_ptr(), out.data_ptr(), b, h, w, out_hw[0], out_hw[1], c, int(align_corners), _stream_ptr())
    if st != GP_OK:
        raise RuntimeError(f"gp_bilinear failed ({st})")
    return out


# ---- the elementwise / layout kernels (tests/test_kernels_glue_*.py).  Thin: the caller owns every buffer, so that a test can prefill a
# destination and see what a kernel leaves alone.  contract=True runs the fp32 twin of the contract precision (bf16 library). -------------------
DDIM_COEF = ("x0_sample", "x0_model", "eps_sample", "eps_model", "prev_x0", "prev_eps", "clip")


def _glue(name: str, contract: bool = False):
    lib = load_library("bf16" if contract else None)
    fn = getattr(lib, name)

    def call(*args):
        st = fn(*args)
        if st != GP_OK:
            raise RuntimeError(f"{name} failed ({st})")
    return call


def rgb_prologue(rgb: torch.Tensor, out: torch.Tensor, cpad: int, contract: bool = False):
    b, _, h, w = rgb.shape
    _glue("gp_rgb_prologue", contract)(rgb.data_ptr(), int(rgb.dtype == torch.uint8), out.data_ptr(), b, h, w, cpad, int(contract), _stream_ptr(rgb.device))
    return out


def concat(a: torch.Tensor, b: torch.Tensor, contract: bool = False) -> torch.Tensor:
    """a [pixels, Ca], b [pixels, Cb] contiguous -> [pixels, Ca + Cb]"""
    out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]), dtype=a.dtype, device=a.device)
    _glue("gp_concat", contract)(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], out.data_ptr(), a.shape[0], int(contract), _stream_ptr(a.device))
    return out


def concat_stats_bm(hw: int, pixels: int, channels: int) -> int:
    return int(load_library().gp_concat_stats_bm(hw, pixels, channels))


def concat_stats(a: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, bm: int = 0):
    """a [B, HW, Ca], b [B, HW, Cb] -> (out [B, HW, Ca + Cb], scale [B, C], shift [B, C], bm used)"""
    bsz, hw, ca = a.shape
    c = ca + b.shape[2]
    out = torch.empty((bsz, hw, c), dtype=a.dtype, device=a.device)
    sc = torch.empty((bsz, c), dtype=torch.float32, device=a.device)
    sh = torch.empty_like(sc)
    used = C.c_int(0)
    _glue("gp_concat_stats")(a.data_ptr(), ca, b.data_ptr(), b.shape[2], out.data_ptr(), bsz, hw, bm, C.byref(used), gamma.data_ptr(), beta.data_ptr(), groups,
                             float(eps), sc.data_ptr(), sh.data_ptr(), _stream_ptr(a.device))
    return out, sc, sh, int(used.value)


def rgb_conv_in_stats(rgb: torch.Tensor, w_packed: torch.Tensor, bias, cout: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float):
    b, _, h, w = rgb.shape
    rgb = rgb.contiguous()
    out = torch.empty((b, h, w, cout), dtype=act_dtype(), device=rgb.device)
    sc = torch.empty((b, cout), dtype=torch.float32, device=rgb.device)
    sh = torch.empty_like(sc)
    _glue("gp_rgb_conv_in_stats")(rgb.data_ptr(), int(rgb.dtype == torch.uint8), w_packed.data_ptr(), _ptr(bias), out.data_ptr(), b, h, w, cout, gamma.data_ptr(),
                                  beta.data_ptr(), groups, float(eps), sc.data_ptr(), sh.data_ptr(), _stream_ptr(rgb.device))
    return out, sc, sh


def nchw_to_nhwc(x: torch.Tensor, out: torch.Tensor, cpad: int, contract: bool = False):
    b, c, h, w = x.shape
    _glue("gp_nchw_to_nhwc", contract)(x.data_ptr(), out.data_ptr(), b, c, h, w, cpad, int(contract), _stream_ptr(x.device))
    return out


def nhwc_to_nchw(x: torch.Tensor, b: int, c: int, h: int, w: int, ld: int, contract: bool = False) -> torch.Tensor:
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device)
    _glue("gp_nhwc_to_nchw", contract)(x.data_ptr(), out.data_ptr(), b, c, h, w, ld, int(contract), _stream_ptr(x.device))
    return out


def ddim_init(noise: Optional[torch.Tensor], lat: torch.Tensor, sample: torch.Tensor, b: int, h: int, w: int, L: int, ld: int, off: int, contract: bool = False):
    _glue("gp_ddim_init", contract)(_ptr(noise), lat.data_ptr(), sample.data_ptr(), b, h, w, L, ld, off, int(contract), _stream_ptr(lat.device))


def ddim_update(model: torch.Tensor, ldm: int, sample: torch.Tensor, uin: torch.Tensor, ldu: int, off: int, x0_out: Optional[torch.Tensor], ldx: int, pixels: int,
                L: int, coef: dict, contract: bool = False):
    k = (C.c_float * 7)(*[float(coef[n]) for n in DDIM_COEF])
    _glue("gp_ddim_update", contract)(model.data_ptr(), ldm, sample.data_ptr(), uin.data_ptr(), ldu, off, _ptr(x0_out), ldx, pixels, L, k, int(contract),
                                      _stream_ptr(model.device))


def decode_epilogue(x: torch.Tensor, b: int, h: int, w: int, ld: int, mean3: bool, raw: bool, out: torch.Tensor, contract: bool = False):
    _glue("gp_decode_epilogue", contract)(x.data_ptr(), out.data_ptr(), b, h, w, ld, int(mean3), int(raw), int(contract), _stream_ptr(x.device))
    return out


def scale_pad(x: torch.Tensor, out: torch.Tensor, pixels: int, c: int, ldi: int, ldo: int, scale: float):
    _glue("gp_scale_pad")(x.data_ptr(), out.data_ptr(), pixels, c, ldi, ldo, float(scale), _stream_ptr(x.device))
    return out


def pointwise_small(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], pixels: int, ldi: int, ldo: int, in_scale: float,
                    contract: bool = False):
    cout, cin = w.shape
    _glue("gp_pointwise_small", contract)(x.data_ptr(), out.data_ptr(), w.data_ptr(), _ptr(bias), pixels, cin, cout, ldi, ldo, float(in_scale), int(contract),
                                          _stream_ptr(x.device))
    return out


def relu(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(x)
    _glue("gp_relu")(x.data_ptr(), out.data_ptr(), x.numel(), _stream_ptr(x.device))
    return out


def add(a: torch.Tensor, b: torch.Tensor, contract: bool = False) -> torch.Tensor:
    out = torch.empty_like(a)
    _glue("gp_add", contract)(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), int(contract), _stream_ptr(a.device))
    return out


def dpt_final(x: torch.Tensor, w: torch.Tensor, bias: float, contract: bool = False) -> torch.Tensor:
    """x [B, HW, Cin] -> fp32 [B, HW]"""
    b, hw, cin = x.shape
    out = torch.empty((b, hw), dtype=torch.float32, device=x.device)
    _glue("gp_dpt_final", contract)(x.data_ptr(), w.data_ptr(), float(bias), out.data_ptr(), b, hw, cin, int(contract), _stream_ptr(x.device))
    return out


def minmax_norm(x: torch.Tensor) -> torch.Tensor:
    """x fp32 [B, n] -> per-image (x - min) / (max - min) (a copy; the kernel works in place)"""
    y = x.clone()
    _glue("gp_minmax_norm")(y.data_ptr(), y.shape[0], y.shape[1], _stream_ptr(x.device))
    return y


def c_heads_split(qkv: torch.Tensor, batch: int, tokens: int, heads: int, hd: int, vts: torch.Tensor):
    """qkv fp32 [B*T, ld]; vts = the caller's (prefilled) [B*heads, hd, 3 Tpad] -> (Qs, Ks [B*heads, T, 3 hd], vts)"""
    qs = torch.empty((batch * heads, tokens, 3 * hd), dtype=torch.bfloat16, device=qkv.device)
    ks = torch.empty_like(qs)
    _glue("gp_c_heads_split", True)(qkv.data_ptr(), qkv.stride(0), qs.data_ptr(), ks.data_ptr(), vts.data_ptr(), batch, tokens, vts.shape[2] // 3, heads, hd,
                                    _stream_ptr(qkv.device))
    return qs, ks, vts


def c_heads_merge_split(o: torch.Tensor, batch: int, heads: int) -> torch.Tensor:
    """O fp32 [B*heads, T, hd] -> A-order split [B*T, 3 heads hd]"""
    _, t, hd = o.shape
    out = torch.empty((batch * t, 3 * heads * hd), dtype=torch.bfloat16, device=o.device)
    _glue("gp_c_heads_merge_split", True)(o.data_ptr(), out.data_ptr(), batch, t, heads, hd, _stream_ptr(o.device))
    return out


def c_cross_fold(y: torch.Tensor, U: torch.Tensor, u0: torch.Tensor, G: torch.Tensor, c0: torch.Tensor, g3: torch.Tensor, b3: torch.Tensor, want_n3: bool = True,
                 eps: float = 1e-5):
    rows, c = y.shape
    y_out = torch.empty_like(y)
    n3 = torch.empty((rows, 3 * c), dtype=torch.bfloat16, device=y.device) if want_n3 else None
    _glue("gp_c_cross_fold", True)(y.data_ptr(), y_out.data_ptr(), _ptr(n3), U.data_ptr(), u0.data_ptr(), G.data_ptr(), c0.data_ptr(), g3.data_ptr(), b3.data_ptr(),
                                   rows, c, U.shape[0], float(eps), _stream_ptr(y.device))
    return y_out, n3


def c_cross_attention(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor) -> torch.Tensor:
    rows, c = q.shape
    out = torch.empty((rows, 3 * c), dtype=torch.bfloat16, device=q.device)
    _glue("gp_c_cross_attention", True)(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), rows, c, kc.shape[0], _stream_ptr(q.device))
    return out


def c_bilinear(x_nhwc: torch.Tensor, out_hw, align_corners: bool) -> torch.Tensor:
    b, h, w, c = x_nhwc.shape
    out = torch.empty((b, out_hw[0], out_hw[1], c), dtype=torch.float32, device=x_nhwc.device)
    _glue("gp_c_bilinear", True)(x_nhwc.data_ptr(), out.data_ptr(), b, h, w, out_hw[0], out_hw[1], c, int(align_corners), _stream_ptr(x_nhwc.device))
    return out
