"""Synthetic depth of field, the host route (numpy, no torch): a photograph refocused under its depth or disparity prediction, as "portrait
mode" does, with the defocus blur of a wide aperture driven by the map.  Every output pixel is a variable-radius, occlusion-aware gather: a
blurred background does not bleed over a sharp subject, and a blurred foreground spreads over what lies behind it.  This file is the
specification in executable form, one vectorised pass per offset; csrc/lens_blur.hip (gp_lens_blur) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the arithmetic once more in csrc/lens_blur_math.h)
  Per image: image uint8 [3, H, W]; pred float32 [1, H, W]; sharp [H, W], optional, non-zero pins the pixel sharp; four integers F, gain,
    cmax8, dz with 0 <= F, dz <= 65535, 0 <= gain <= 32768, 0 <= cmax8 <= 256.  Per call: space "depth" or "disparity"; to_lin uint16 [256],
    strictly increasing, values <= 4095; from_lin uint8 [4096] with from_lin[to_lin[v]] == v.  1 <= H, W <= 16384 and B * H * W < 2^31.
  1. Nearness: Q = quantize16(pred) = (uint16)(clamp(pred, 0, 1) * 65535.0f), the 16-bit rule of gp_postprocess.  D = Q in disparity space,
     D = 65535 - Q in depth space: a larger D is nearer.  A NaN pixel has D = 0.
  2. Circle of confusion in eighths of a pixel: e = max(0, |D - F| - dz); c = min(cmax8, (e * gain + 32768) >> 16); c = 0 where pred is NaN or
     sharp is non-zero.  The radius is linear in the map's value: the thin-lens law for a disparity map, whatever its unknown scale and shift,
     and a stated convention for an affine-invariant depth map.
  3. Disc sizes: n(c) = the number of integer offsets (dx, dy) with 64 (dx^2 + dy^2) <= (c + 4)^2; w(c) = floor(2^20 / n(c)).
  4. Gather: for the output pixel p, a source q inside the image at offset (dx, dy) has the reach r = c_q if D_q >= D_p and min(c_q, c_p)
     otherwise; it contributes iff 64 (dx^2 + dy^2) <= (r + 4)^2, with the weight w(r).  Sw = sum w, S_k = sum w * to_lin[image_k(q)], exact
     integers.  Pixels outside the image do not exist.
  5. out_k(p) = from_lin[(2 S_k + Sw) // (2 Sw)]; coc(p) = c_p, uint16.

The user's terms (`lens_params`): focus, a value of the map in [0, 1] (F is its nearness), or focus_at = (u, v), the pixel whose nearness is
F; aperture, the blur radius in pixels at the far end of the scale (gain = round(8 * aperture)); max_radius <= 32 pixels (cmax8 =
round(8 * max_radius)); dof, the half-width of the sharp zone in map units (dz = round(65535 * dof)).
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, Optional, Tuple

import numpy as np

from .post_common import MAX_DIM, SPACES, _check_space, _per_image, _pixel_inside, _plane, _plane_F, nearness, quantize16  # noqa: F401

MAX_C8 = 256
MAX_RADIUS = 32.0
MAX_GAIN = 32768
ONE = 1 << 20
LIN_MAX = 4095
PARAM_FIELDS = ("F", "gain", "cmax8", "dz")
PARAM_MAX = (65535, MAX_GAIN, MAX_C8, 65535)
DEFAULTS = dict(focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0)
i64 = np.int64


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------------
def inverse_table(to_lin) -> np.ndarray:
    """from_lin uint8 [4096] of a strictly increasing to_lin: the byte whose linear value is nearest, the smaller byte on a tie --
    from_lin[l] = the number of v in 1 .. 255 with to_lin[v - 1] + to_lin[v] < 2 l.  from_lin[to_lin[v]] == v."""
    t = np.asarray(to_lin, i64)
    return np.searchsorted(t[:-1] + t[1:], 2 * np.arange(LIN_MAX + 1, dtype=i64), side="left").astype(np.uint8)


@lru_cache(maxsize=None)
def _srgb() -> Tuple[np.ndarray, np.ndarray]:
    def to_linear(s):
        return s / 12.92 if s <= 0.04045 else ((s + 0.055) / 1.055) ** 2.4
    to_lin = np.array([int(math.floor(LIN_MAX * to_linear(v / 255.0) + 0.5)) for v in range(256)], np.uint16)
    return to_lin, inverse_table(to_lin)


def srgb_tables() -> Tuple[np.ndarray, np.ndarray]:
    """The default tables: to_lin[v] = round(4095 * srgb_to_linear(v / 255)), 12-bit linear light, and its inverse (`inverse_table`)."""
    return tuple(t.copy() for t in _srgb())


def identity_tables() -> Tuple[np.ndarray, np.ndarray]:
    """to_lin[v] = v and from_lin[l] = min(l, 255): the blur averages the bytes as they are."""
    to_lin = np.arange(256, dtype=np.uint16)
    return to_lin, inverse_table(to_lin)


def check_tables(tables) -> Tuple[np.ndarray, np.ndarray]:
    """(to_lin uint16 [256], from_lin uint8 [4096]) checked and contiguous; None: `srgb_tables`.  ValueError unless to_lin is strictly
    increasing with values <= 4095 and from_lin[to_lin[v]] == v for every v."""
    if tables is None:
        return _srgb()
    try:
        to_lin, from_lin = (np.asarray(t) for t in tables)
    except (TypeError, ValueError):
        raise ValueError("tables: a pair (to_lin, from_lin)") from None
    if to_lin.shape != (256,) or from_lin.shape != (LIN_MAX + 1,) or to_lin.dtype.kind not in "iu" or from_lin.dtype.kind not in "iu":
        raise ValueError(f"tables: integers to_lin [256] and from_lin [4096], got {to_lin.dtype} {to_lin.shape} and {from_lin.dtype} {from_lin.shape}")
    t, f = to_lin.astype(i64), from_lin.astype(i64)
    if t.min() < 0 or t.max() > LIN_MAX or (np.diff(t) <= 0).any():
        raise ValueError("tables: to_lin is strictly increasing with values in 0 .. 4095")
    if f.min() < 0 or f.max() > 255 or (f[t] != np.arange(256)).any():
        raise ValueError("tables: from_lin holds bytes and from_lin[to_lin[v]] == v for every v")
    return np.ascontiguousarray(to_lin.astype(np.uint16)), np.ascontiguousarray(from_lin.astype(np.uint8))


# ---- disc sizes -------------------------------------------------------------------------------------------------------------------------------------
def disc_count(c: int) -> int:
    """n(c): the integer offsets (dx, dy) with 64 (dx^2 + dy^2) <= (c + 4)^2."""
    r = (c + 4) >> 3
    d = np.arange(-r, r + 1, dtype=i64)
    return int((64 * (d[:, None] ** 2 + d[None, :] ** 2) <= (c + 4) ** 2).sum())


@lru_cache(maxsize=None)
def disc_weights() -> np.ndarray:
    """w(c) = floor(2^20 / n(c)) for c = 0 .. 256, int64 [257]."""
    return np.array([ONE // disc_count(c) for c in range(MAX_C8 + 1)], i64)


# ---- the user's terms ---------------------------------------------------------------------------------------------------------------------------------
def lens_blur_options(B: int, focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0) -> Dict:
    """The user's terms checked (ValueError outside their ranges) and spread over the B images: a dict of focus float32 [B] or None, focus_at
    int64 [B, 2] = (u, v) or None -- exactly one of the two is given --, and the integers gain, cmax8, dz, int64 [B] each."""
    out = dict(zip(("focus", "focus_at"), _plane(B, focus, focus_at, "focus", "focus_at", exactly_one=True)))
    a, m, d = _per_image(aperture, B, "aperture"), _per_image(max_radius, B, "max_radius"), _per_image(dof, B, "dof")
    if (a < 0.0).any() or (a > MAX_GAIN / 8.0).any():
        raise ValueError(f"aperture is a radius in pixels in [0, {MAX_GAIN // 8}], got {aperture!r}")
    if (m < 0.0).any() or (m > MAX_RADIUS).any():
        raise ValueError(f"max_radius is in [0, {MAX_RADIUS:g}] pixels, got {max_radius!r}")
    if (d < 0.0).any() or (d > 1.0).any():
        raise ValueError(f"dof is in [0, 1], in units of the map, got {dof!r}")
    out.update(gain=np.floor(8.0 * a + 0.5).astype(i64), cmax8=np.floor(8.0 * m + 0.5).astype(i64), dz=np.floor(65535.0 * d + 0.5).astype(i64))
    return out


def lens_params(pred, space: str, focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0) -> np.ndarray:
    """The four integers F, gain, cmax8, dz of every image, int32 [B, 4], from the user's terms and, for focus_at, the maps pred [B, 1, H, W]."""
    pred = np.asarray(pred)
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    o = lens_blur_options(B, focus, focus_at, aperture, max_radius, dof)
    _pixel_inside(o["focus_at"], "focus_at", H, W)
    F = _plane_F(pred.reshape(B, H, W), space, o["focus"], o["focus_at"])
    return np.stack([F, o["gain"], o["cmax8"], o["dz"]], 1).astype(np.int32)


def check_params(params, B: int) -> np.ndarray:
    """params as a checked contiguous int32 [B, 4] array of F, gain, cmax8, dz ([4]: the same row for every image)."""
    p = np.asarray(params)
    if p.dtype.kind not in "iu":
        raise ValueError(f"params: integers {PARAM_FIELDS}, got {p.dtype}")
    if p.ndim == 1:
        p = np.broadcast_to(p[None], (B,) + p.shape)
    if p.shape != (B, 4):
        raise ValueError(f"params: four integers {PARAM_FIELDS} per image, [4] or [{B}, 4], got {p.shape}")
    p = p.astype(i64)
    if (p < 0).any() or (p > np.array(PARAM_MAX, i64)[None]).any():
        raise ValueError(f"params: 0 <= {PARAM_FIELDS} <= {PARAM_MAX}, got {p.tolist()}")
    return np.ascontiguousarray(p.astype(np.int32))


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------
def circle_of_confusion(D, still, row) -> np.ndarray:
    """Step 2: c int64 from the nearness D, the pixels that stay sharp (NaN or pinned) and a parameter row F, gain, cmax8, dz."""
    F, gain, cmax8, dz = (int(v) for v in row)
    e = np.maximum(0, np.abs(D - F) - dz)
    return np.where(still, 0, np.minimum(cmax8, (e * gain + 32768) >> 16))


def gather(D, c, lin) -> Tuple[np.ndarray, np.ndarray]:
    """Step 4 for one image: D, c int64 [H, W], lin int64 [3, H, W] -> (S int64 [3, H, W], Sw int64 [H, W]).  One pass per offset of the disc of
    the image's largest c; beyond it nothing contributes."""
    H, W = D.shape
    cm = int(c.max())
    R = (cm + 4) >> 3
    w = disc_weights()
    Dp, cp, lp = np.zeros((H + 2 * R, W + 2 * R), i64), np.zeros((H + 2 * R, W + 2 * R), i64), np.zeros((3, H + 2 * R, W + 2 * R), i64)
    Dp[R:R + H, R:R + W], cp[R:R + H, R:R + W], lp[:, R:R + H, R:R + W] = D, c, lin  # (outside the image c = 0: the reach is 0 from every side)
    S, Sw = np.zeros((3, H, W), i64), np.zeros((H, W), i64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = 64 * (dx * dx + dy * dy)
            if d2 > (cm + 4) ** 2:
                continue
            ys, xs = slice(R + dy, R + dy + H), slice(R + dx, R + dx + W)
            Dq, cq = Dp[ys, xs], cp[ys, xs]
            r = np.where(Dq >= D, cq, np.minimum(cq, c))
            wt = np.where(d2 <= (r + 4) ** 2, w[r], 0)
            Sw += wt
            S += wt[None] * lp[:, ys, xs]
    return S, Sw


def lens_blur_params(image, pred, params, space: str = "depth", sharp=None, tables=None, want_coc: bool = False):
    """A batch by the definition above from the four integers of every image.  image uint8 [B, 3, H, W] ([3, H, W]: one image); pred float
    [B, 1, H, W] ([B, H, W] with B images, [H, W] with one); params integers [B, 4] or [4]; sharp [B, H, W] or None; tables (to_lin, from_lin)
    or None (`srgb_tables`).  Returns out uint8 [B, 3, H, W], and with want_coc (out, coc) with coc uint16 [B, H, W]."""
    _check_space(space)
    image = np.asarray(image)
    image = image[None] if image.ndim == 3 else image
    if image.dtype != np.uint8 or image.ndim != 4 or image.shape[1] != 3:
        raise ValueError(f"image: uint8 [B, 3, H, W] or [3, H, W], got {image.dtype} {image.shape}")
    B, _, H, W = image.shape
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or B < 1 or B * H * W >= 2 ** 31:
        raise ValueError(f"image: sides in 1 .. {MAX_DIM}, B * H * W < 2^31, got {image.shape}")
    pred = np.asarray(pred)
    if pred.dtype.kind != "f" or pred.size != B * H * W or tuple(pred.shape[-2:]) != (H, W):
        raise ValueError(f"pred: float {(B, 1, H, W)}, got {pred.dtype} {pred.shape}")
    pred = pred.reshape(B, H, W).astype(np.float32)
    params = check_params(params, B)
    if sharp is not None:
        sharp = np.asarray(sharp)
        sharp = sharp[None] if sharp.ndim == 2 else sharp
        if sharp.shape != (B, H, W) or sharp.dtype.kind not in "biu":
            raise ValueError(f"sharp: integers or booleans {(B, H, W)}, got {sharp.dtype} {sharp.shape}")
    to_lin, from_lin = check_tables(tables)
    out, coc = np.empty((B, 3, H, W), np.uint8), np.empty((B, H, W), np.uint16)
    for k in range(B):
        D = nearness(pred[k], space)
        still = np.isnan(pred[k]) if sharp is None else np.isnan(pred[k]) | (sharp[k] != 0)
        c = circle_of_confusion(D, still, params[k])
        S, Sw = gather(D, c, to_lin[image[k]].astype(i64))
        out[k], coc[k] = from_lin[(2 * S + Sw[None]) // (2 * Sw[None])], c
    return (out, coc) if want_coc else out


def lens_blur(image, pred, focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0, space: str = "depth", sharp=None, tables=None,
              want_coc: bool = False):
    """`lens_blur_params` from the user's terms (module docstring): exactly one of focus and focus_at; every term one value or one per image."""
    image = np.asarray(image)
    B = 1 if image.ndim == 3 else image.shape[0]
    _check_space(space)
    pred = np.asarray(pred)
    if image.ndim not in (3, 4) or pred.size != B * image.shape[-2] * image.shape[-1] or tuple(pred.shape[-2:]) != tuple(image.shape[-2:]):
        raise ValueError(f"image [B, 3, H, W] and pred [B, 1, H, W], got {image.shape} and {pred.shape}")
    params = lens_params(pred.reshape((B, 1) + pred.shape[-2:]), space, focus, focus_at, aperture, max_radius, dof)
    return lens_blur_params(image, pred, params, space, sharp, tables, want_coc)
