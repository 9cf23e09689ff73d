"""Matting cutouts, the host route (numpy, no torch): foreground colours by the multi-level method of Germer et al. 2020 ("Fast Multi-Level
Foreground Estimation", pymatting's estimate_foreground_ml), an RGBA cutout and a composite over a new background.  This file is the
specification in executable form; csrc/foreground.hip (gp_foreground) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h and csrc/foreground.hip)
  Inputs per image: an 8-bit RGB image [3, H, W] and an 8-bit alpha [H, W] (a float map in [0, 1] is quantised first with
    eval_metrics.quantize_mask, the byte run.py:449-455 saves); I = byte / 255, a = byte / 255, one float32 division each; 1 <= H, W <= 16384.
  Arithmetic: float32 throughout, only + - * / abs min max in exactly the order written below, no fused multiply-add.  max(v, 0) is
    `v if v > 0 else 0` and min(v, 1) is `v if v < 1 else 1`, so that the sign of a zero cannot differ between routes.
  Levels: L = ceil(log2(max(H, W))) (0 for 1 x 1); level l = 0 .. L has h_l = (H + 2^(L-l) - 1) >> (L-l) and w_l likewise (level 0 is 1 x 1,
    level L is H x W; no pow anywhere).  Every level samples image and alpha from the full-resolution bytes, nearest:
    src = ((y * H) // h_l, (x * W) // w_l).  F and B of level l start as the nearest upsample of level l-1's result,
    ((y * h_{l-1}) // h_l, (x * w_{l-1}) // w_l); at level 0, F = B = I.
  Iterations: a level with h_l <= 32 and w_l <= 32 takes n_small (default 10, 0 .. 64), every other level n_big (default 2, 1 .. 4).
    Jacobi: each reads only the previous iterate.  One iteration at a pixel, neighbours in the order left, right, up, down with coordinates
    clamped to the level:
      a1 = 1 - a;  a00 = a*a;  a01 = a*a1;  a11 = a1*a1;  b0[c] = a*I[c];  b1[c] = a1*I[c]
      for each neighbour n:  da = reg + gw*|a - a_n|;  a00 += da;  a11 += da;  b0[c] += da*F_n[c];  b1[c] += da*B_n[c]
      det = a00*a11 - a01*a01;  inv = 1/det
      F[c] = min(max(inv*(a11*b0[c] - a01*b1[c]), 0), 1);   B[c] = min(max(inv*(a00*b1[c] - a01*b0[c]), 0), 1)
    reg: default 1e-5, range [1e-6, 1] (below it det is no longer safely positive in float32); gw: default 1, range [0, 100].
  Outputs: F, B float32 [3, H, W];  rgba uint8 [H, W, 4] with RGB = min(255, (int)(F*255 + 0.5)) and A = the alpha byte;  the composite
    uint8 [3, H, W] = (a*F) + ((1-a)*N) quantised the same way, N a uint8 [3, H, W] image or one [3] colour, as byte / 255.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .eval_metrics import quantize_mask
from .post_common import MAX_DIM

SMALL = 32
DEFAULTS = dict(reg=1e-5, gw=1.0, n_small=10, n_big=2)
f32 = np.float32


def level_sizes(h: int, w: int) -> List[Tuple[int, int]]:
    """[(h_l, w_l) for l = 0 .. L]: (1, 1) first, (h, w) last."""
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f"1 <= H, W <= {MAX_DIM}, got {h} x {w}")
    L = 0
    while (1 << L) < max(h, w):
        L += 1
    return [((h + (1 << (L - l)) - 1) >> (L - l), (w + (1 << (L - l)) - 1) >> (L - l)) for l in range(L + 1)]


def check_options(reg: float, gw: float, n_small: int, n_big: int) -> Tuple[np.float32, np.float32, int, int]:
    """The ranges of the definition (ValueError outside them); reg and gw as the float32 values the arithmetic uses."""
    reg32, gw32 = f32(reg), f32(gw)
    if not (f32(1e-6) <= reg32 <= f32(1.0)):
        raise ValueError(f"reg is in [1e-6, 1], got {reg}")
    if not (f32(0.0) <= gw32 <= f32(100.0)):
        raise ValueError(f"gw is in [0, 100], got {gw}")
    if int(n_small) != n_small or not 0 <= n_small <= 64:
        raise ValueError(f"n_small is in 0 .. 64, got {n_small}")
    if int(n_big) != n_big or not 1 <= n_big <= 4:
        raise ValueError(f"n_big is in 1 .. 4, got {n_big}")
    return reg32, gw32, int(n_small), int(n_big)


def _inputs(image_u8, alpha) -> Tuple[np.ndarray, np.ndarray]:
    image_u8 = np.asarray(image_u8)
    if image_u8.dtype != np.uint8 or image_u8.ndim != 3 or image_u8.shape[0] != 3:
        raise ValueError(f"image: uint8 [3, H, W], got {image_u8.dtype} {image_u8.shape}")
    a8 = quantize_mask(np.asarray(alpha))
    if a8.shape != image_u8.shape[1:]:
        raise ValueError(f"alpha {a8.shape} does not match the image {image_u8.shape}")
    return image_u8, a8


def _clamp01(v: np.ndarray) -> np.ndarray:
    v = np.where(v > f32(0.0), v, f32(0.0))
    return np.where(v < f32(1.0), v, f32(1.0))


def estimate_foreground(image_u8, alpha, reg: float = 1e-5, gw: float = 1.0, n_small: int = 10, n_big: int = 2,
                        stats: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(F, B), float32 [3, H, W] each, of one image by the definition above.  stats: a dict that receives "det_min", the smallest det of any
    pixel of any iteration (inf when no iteration ran)."""
    image_u8, a8 = _inputs(image_u8, alpha)
    reg, gw, n_small, n_big = check_options(reg, gw, n_small, n_big)
    H, W = a8.shape
    sizes = level_sizes(H, W)
    det_min = np.inf
    F = B = None
    for l, (hl, wl) in enumerate(sizes):
        ys, xs = (np.arange(hl) * H) // hl, (np.arange(wl) * W) // wl
        I = image_u8[:, ys[:, None], xs[None, :]].astype(f32) / f32(255.0)
        a = a8[ys[:, None], xs[None, :]].astype(f32) / f32(255.0)
        if l == 0:
            F, B = I.copy(), I.copy()
        else:
            hp, wp = sizes[l - 1]
            py, px = (np.arange(hl) * hp) // hl, (np.arange(wl) * wp) // wl
            F, B = F[:, py[:, None], px[None, :]], B[:, py[:, None], px[None, :]]
        yi, xi = np.arange(hl), np.arange(wl)
        # left, right, up, down, clamped to the level
        nb = [(yi, np.maximum(xi - 1, 0)), (yi, np.minimum(xi + 1, wl - 1)), (np.maximum(yi - 1, 0), xi), (np.minimum(yi + 1, hl - 1), xi)]
        a1 = f32(1.0) - a
        a01 = a * a1
        for _ in range(n_small if hl <= SMALL and wl <= SMALL else n_big):
            a00, a11 = a * a, a1 * a1
            b0, b1 = a * I, a1 * I
            for ny, nx in nb:
                sel = (ny[:, None], nx[None, :])
                da = reg + gw * np.abs(a - a[sel])
                a00, a11 = a00 + da, a11 + da
                b0 = b0 + da * F[(slice(None),) + sel]
                b1 = b1 + da * B[(slice(None),) + sel]
            det = a00 * a11 - a01 * a01
            inv = f32(1.0) / det
            det_min = min(det_min, float(det.min()))
            F, B = _clamp01(inv * (a11 * b0 - a01 * b1)), _clamp01(inv * (a00 * b1 - a01 * b0))
            assert F.dtype == np.float32 and B.dtype == np.float32
    if stats is not None:
        stats["det_min"] = det_min
    return np.ascontiguousarray(F, dtype=f32), np.ascontiguousarray(B, dtype=f32)


def to_bytes(v: np.ndarray) -> np.ndarray:
    """min(255, (int)(v * 255 + 0.5)) of float32 values in [0, 1]"""
    q = (v.astype(f32) * f32(255.0) + f32(0.5)).astype(np.int32)
    return np.minimum(q, 255).astype(np.uint8)


def cutout_rgba(image_u8, alpha, **options) -> np.ndarray:
    """The cutout of one image: uint8 [H, W, 4], RGB the bytes of the estimated foreground colour, A the alpha byte."""
    image_u8, a8 = _inputs(image_u8, alpha)
    F, _ = estimate_foreground(image_u8, a8, **options)
    return np.ascontiguousarray(np.concatenate([to_bytes(F), a8[None]], axis=0).transpose(1, 2, 0))


def composite(image_u8, alpha, background, **options) -> np.ndarray:
    """The estimated foreground over a new background: uint8 [3, H, W] of (a*F) + ((1-a)*N); background: a uint8 [3, H, W] image or one
    [3] colour."""
    image_u8, a8 = _inputs(image_u8, alpha)
    N = np.asarray(background)
    if N.dtype != np.uint8 or N.shape not in ((3,), image_u8.shape):
        raise ValueError(f"background: a uint8 [3, H, W] image of the image's size or one uint8 [3] colour, got {N.dtype} {N.shape}")
    N = np.broadcast_to(N.reshape(3, 1, 1) if N.ndim == 1 else N, image_u8.shape).astype(f32) / f32(255.0)
    F, _ = estimate_foreground(image_u8, a8, **options)
    a = a8.astype(f32) / f32(255.0)
    return to_bytes((a * F) + ((f32(1.0) - a) * N))
