"""Edge-aware upsampling of a prediction, the host route (numpy, no torch): the guided filter of He, Sun and Tang ("Guided Image Filtering",
2010 / 2013) in its fast form (He and Sun, "Fast Guided Filter", 2015) with the image as guide.  This file is the specification in executable
form; csrc/guided.hip (gp_guided_upsample) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the per-pixel arithmetic once more in csrc/guided_solve.h)
  Inputs per image: guide_lo uint8 [3, h, w], the image at the processing size; pred float32 [C, h, w], C = 1 or 3; guide uint8 [3, H, W], the
    image at the input size; r = 1 .. 32; eps in (0, 1], in units of [0, 1]^2.  1 <= h, w, H, W <= 16384.  Output float32 [C, H, W] in [0, 1].
  Quantise: p = (uint16)(clamp(pred, 0, 1) * 65535.0f), a float32 product, truncated, NaN -> 0 (the 16-bit rule of gp_postprocess).
  Window sums: the window of pixel k is the (2 r + 1)^2 square around it clipped to the image, N its pixel count; over it S_I[c], S_II[c][d]
    (c <= d), and per prediction channel S_p, S_Ip[c].  Exact integers; with r <= 32 every product below stays under 2^53.
  Solve, float64, no fused multiply-add, in this order:
    cov[c] = (N * S_Ip[c] - S_I[c] * S_p) / (N * N);   s[c][d] = (N * S_II[c][d] - S_I[c] * S_I[d]) / (N * N), + e on the diagonal, e = eps * 65025
    c00 = s11 s22 - s12 s12;  c01 = s02 s12 - s01 s22;  c02 = s01 s12 - s02 s11;  c11 = s00 s22 - s02 s02;  c12 = s01 s02 - s00 s12;
    c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02
    a[0] = ((c00 cov0 + c01 cov1) + c02 cov2) / det;  a[1] = ((c01 cov0 + c11 cov1) + c12 cov2) / det;  a[2] = ((c02 cov0 + c12 cov1) + c22 cov2) / det
    b = S_p / N - ((a[0] * (S_I[0] / N) + a[1] * (S_I[1] / N)) + a[2] * (S_I[2] / N))
  Smooth: the means of a[c] and b over the same clipped window.  Each row of the window is summed left to right starting from +0.0, the row
    sums are summed top to bottom starting from +0.0, then one division by N.  Every window is summed afresh (no running sums).
  Upsample and apply: for output row Y, s = max(0, ((2 Y + 1) h - H) / (2 H)), one float64 division of the two integers; i0 = floor(s),
    i1 = min(i0 + 1, h - 1), fy = s - i0; columns likewise (j0, j1, fx).  Each of the four smoothed planes v is blended as
    t0 = v[i0][j0] + fx * (v[i0][j1] - v[i0][j0]);  t1 = v[i1][j0] + fx * (v[i1][j1] - v[i1][j0]);  V = t0 + fy * (t1 - t0)
    and q = (((A[0] * g[0] + A[1] * g[1]) + A[2] * g[2]) + B) / 65535 with g the three guide bytes, clamped by comparisons
    (q > 0 ? (q < 1 ? q : 1) : 0, so NaN -> 0), rounded once to float32.  With h = H and w = W this is the plain guided filter.
  C = 3: the channels are filtered independently and share the image sums.  Normals are NOT renormalised.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .post_common import MAX_DIM, options_from, quantize16  # noqa: F401  (quantize16: re-exported, the rule was first stated here)

MAX_R = 32
DEFAULTS = dict(radius=4, eps=1e-4)
f32, f64 = np.float32, np.float64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the order of the six S_II sums


def check_options(radius, eps) -> Tuple[int, float]:
    """The ranges of the definition (ValueError outside them)."""
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= radius <= MAX_R:
        raise ValueError(f"radius is in 1 .. {MAX_R}, got {radius}")
    eps = float(eps)
    if not (0.0 < eps <= 1.0):
        raise ValueError(f"eps is in (0, 1], got {eps}")
    return int(radius), eps


def refine_options(refine) -> Dict:
    """The `refine` argument of the pipeline entries -- True or dict(radius=..., eps=...) -- as the checked options of `guided_upsample`."""
    return options_from(refine, DEFAULTS, "refine", lambda o: dict(zip(("radius", "eps"), check_options(**o))))


def _window(n: int, r: int) -> Tuple[np.ndarray, np.ndarray]:
    i = np.arange(n)
    return np.maximum(i - r, 0), np.minimum(i + r, n - 1) + 1


def _box_int(v: np.ndarray, r: int) -> np.ndarray:
    """Exact sums of an int64 array [..., h, w] over the clipped (2 r + 1)^2 windows."""
    for axis in (-1, -2):
        lo, hi = _window(v.shape[axis], r)
        c = np.concatenate([np.zeros_like(np.take(v, [0], axis=axis)), np.cumsum(v, axis=axis, dtype=np.int64)], axis=axis)
        v = np.take(c, hi, axis=axis) - np.take(c, lo, axis=axis)
    return v


def _inputs(guide_lo, pred, guide):
    guide_lo, guide = np.asarray(guide_lo), np.asarray(guide)
    pred = np.asarray(pred)
    for name, g in (("guide_lo", guide_lo), ("guide", guide)):
        if g.dtype != np.uint8 or g.ndim != 3 or g.shape[0] != 3 or not all(1 <= n <= MAX_DIM for n in g.shape[1:]):
            raise ValueError(f"{name}: uint8 [3, H, W] with sides in 1 .. {MAX_DIM}, got {g.dtype} {g.shape}")
    if pred.ndim == 2:
        pred = pred[None]
    if pred.ndim != 3 or pred.shape[0] not in (1, 3) or pred.shape[1:] != guide_lo.shape[1:] or pred.dtype.kind != "f":
        raise ValueError(f"pred: float [C, h, w], C = 1 or 3, of guide_lo's size {guide_lo.shape[1:]}, got {pred.dtype} {pred.shape}")
    return guide_lo, pred.astype(f32), guide


def window_sums(guide_lo: np.ndarray, p16: np.ndarray, r: int) -> Dict[str, np.ndarray]:
    """The integer sums of the definition, int64: N [h, w], S_I [3, h, w], S_II [6, h, w] (PAIRS), S_p [C, h, w], S_Ip [C, 3, h, w]."""
    I = guide_lo.astype(np.int64)
    p = p16.astype(np.int64)
    h, w = I.shape[1:]
    (ylo, yhi), (xlo, xhi) = _window(h, r), _window(w, r)
    return dict(N=((yhi - ylo)[:, None] * (xhi - xlo)[None, :]).astype(np.int64), S_I=_box_int(I, r),
                S_II=_box_int(np.stack([I[c] * I[d] for c, d in PAIRS]), r), S_p=_box_int(p, r), S_Ip=_box_int(p[:, None] * I[None], r))


def solve(sums: Dict[str, np.ndarray], eps: float) -> np.ndarray:
    """The local linear models: float64 [C, 4, h, w] = a[0], a[1], a[2], b of every pixel and prediction channel."""
    N = sums["N"].astype(f64)
    NN = N * N
    e = f64(eps) * f64(65025.0)
    I0, I1, I2 = (sums["S_I"][c].astype(f64) for c in range(3))
    Im = (I0, I1, I2)
    s = {}
    for k, (c, d) in enumerate(PAIRS):
        v = (N * sums["S_II"][k].astype(f64) - Im[c] * Im[d]) / NN
        s[c, d] = v + e if c == d else v
    c00 = s[1, 1] * s[2, 2] - s[1, 2] * s[1, 2]
    c01 = s[0, 2] * s[1, 2] - s[0, 1] * s[2, 2]
    c02 = s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]
    c11 = s[0, 0] * s[2, 2] - s[0, 2] * s[0, 2]
    c12 = s[0, 1] * s[0, 2] - s[0, 0] * s[1, 2]
    c22 = s[0, 0] * s[1, 1] - s[0, 1] * s[0, 1]
    det = (s[0, 0] * c00 + s[0, 1] * c01) + s[0, 2] * c02
    out = []
    with np.errstate(all="ignore"):
        for ch in range(sums["S_p"].shape[0]):
            P = sums["S_p"][ch].astype(f64)
            cov0, cov1, cov2 = ((N * sums["S_Ip"][ch, c].astype(f64) - Im[c] * P) / NN for c in range(3))
            a0 = ((c00 * cov0 + c01 * cov1) + c02 * cov2) / det
            a1 = ((c01 * cov0 + c11 * cov1) + c12 * cov2) / det
            a2 = ((c02 * cov0 + c12 * cov1) + c22 * cov2) / det
            b = P / N - ((a0 * (I0 / N) + a1 * (I1 / N)) + a2 * (I2 / N))
            out.append(np.stack([a0, a1, a2, b]))
    return np.stack(out)


def _sum_in_order(v: np.ndarray, r: int, axis: int) -> np.ndarray:
    """Over the clipped window i - r .. i + r along `axis`, in index order, starting from +0.0 (what lies outside adds +0.0: no change)."""
    n = v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (r, r)
    z = np.pad(v, pad)
    acc = np.zeros_like(v)
    for d in range(2 * r + 1):
        acc = acc + np.take(z, np.arange(d, d + n), axis=axis)
    return acc


def smooth(ab: np.ndarray, r: int) -> np.ndarray:
    """The window means of float64 planes [..., h, w] in the order of the definition."""
    h, w = ab.shape[-2:]
    (ylo, yhi), (xlo, xhi) = _window(h, r), _window(w, r)
    N = ((yhi - ylo)[:, None] * (xhi - xlo)[None, :]).astype(f64)
    with np.errstate(all="ignore"):
        return _sum_in_order(_sum_in_order(ab.astype(f64), r, -1), r, -2) / N


def index_map(n_from: int, n_to: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(i0, i1, f) of every output index of an extent n_to in an extent n_from."""
    Y = np.arange(n_to, dtype=np.int64)
    q = ((2 * Y + 1) * n_from - n_to).astype(f64) / f64(2 * n_to)
    s = np.where(q > 0.0, q, 0.0)
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, n_from - 1), s - i0.astype(f64)


def resize_bilinear(v: np.ndarray, H: int, W: int) -> np.ndarray:
    """float64 planes [..., h, w] -> [..., H, W] by the index rule and the four-tap blend of the definition."""
    v = np.asarray(v, dtype=f64)
    (i0, i1, fy), (j0, j1, fx) = index_map(v.shape[-2], H), index_map(v.shape[-1], W)
    fy = fy[:, None]
    with np.errstate(all="ignore"):
        top, bot = v[..., i0, :], v[..., i1, :]
        t0 = top[..., j0] + fx * (top[..., j1] - top[..., j0])
        t1 = bot[..., j0] + fx * (bot[..., j1] - bot[..., j0])
        return t0 + fy * (t1 - t0)


def upsample_apply(ab_mean: np.ndarray, guide: np.ndarray) -> np.ndarray:
    """The smoothed models float64 [C, 4, h, w] applied to the image uint8 [3, H, W]: float32 [C, H, W]."""
    H, W = guide.shape[1:]
    V = resize_bilinear(ab_mean, H, W)
    g = guide.astype(f64)
    with np.errstate(all="ignore"):
        q = (((V[:, 0] * g[0] + V[:, 1] * g[1]) + V[:, 2] * g[2]) + V[:, 3]) / f64(65535.0)
    q = np.where(q > 0.0, np.where(q < 1.0, q, 1.0), 0.0)
    return np.ascontiguousarray(q.astype(f32))


def guided_upsample(guide_lo, pred, guide, radius: int = 4, eps: float = 1e-4) -> np.ndarray:
    """One image by the definition above: guide_lo uint8 [3, h, w], pred float [C, h, w] (or [h, w]), guide uint8 [3, H, W] -> float32
    [C, H, W] in [0, 1]."""
    guide_lo, pred, guide = _inputs(guide_lo, pred, guide)
    r, eps = check_options(radius, eps)
    return upsample_apply(smooth(solve(window_sums(guide_lo, quantize16(pred), r), eps), r), guide)
