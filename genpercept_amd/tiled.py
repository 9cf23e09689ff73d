"""Tiled high-resolution inference, the host route of the merge (numpy, no torch): a map computed once on the whole image (the base, for the
global layout) and once more on overlapping windows at native resolution (the tiles, for the detail) is put together -- each tile's
affine-invariant prediction is fitted onto the base by least squares, and the fitted tiles are blended with weights that fall off towards
their borders.  This file is the specification in executable form; csrc/tile_merge.hip (gp_tile_merge) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the per-tile solve and the per-pixel steps once more in csrc/tile_merge_math.h)
  Grid: along an axis of length L with tile size T and overlap o the window is w = min(T, L); the tile count is n = 1 if L <= w, else
    n = ceil((L - o) / (w - o)); the origins are y_k = (k * (L - w)) // (n - 1) in integers (0 for n = 1).  Neighbours overlap by at least o,
    the first tile starts at 0, the last ends at L, the origins increase strictly.  Tiles are numbered iy * nx + ix.  Ranges: 1 <= o <= w / 2
    on both axes, ny * nx <= 1024, 1 <= H, W <= 16384, C = 1 or 3.  `ys` and `xs` passed to the functions below ARE these origins: they are
    checked against the rule, not taken as they come.
  Inputs per image: base float32 [C, H, W], the map of the whole image at the input size; tiles float32 [N, C, wh, ww], the maps of the
    windows; the overlap; the alignment, "least_square" or "none".  Output float32 [C, H, W] in [0, 1].
  Fit, per tile, over all wh * ww * C values of the window (three channels share one fit):
    P = quantize16(tile), G = quantize16(base window): (uint16)(clamp(x, 0, 1) * 65535.0f), a float32 product, truncated, NaN -> 0 (the rule of
    guided.quantize16 / gp_postprocess).  The sums n, sum P, sum G, sum P^2, sum P G are exact integers (below 2^63 within the ranges); each is
    converted to float64 once, round to nearest; then in float64, no fused multiply-add, in this order:
      mp = SP / n;  mg = SG / n;  var = SPP / n - mp * mp;  cov = SPG / n - mp * mg;  s = cov / var
      if not (var >= 1.0) or not (s > 0): s = 1      (a tile flat to within one 16-bit step, or anti-correlated with the base: shifted only)
      t = (mg - s * mp) / 65535
    Alignment "none": s = 1, t = 0 (matting, dis, seg and normal maps are not affine-invariant).
  Blend, per output pixel and channel: the tiles that cover the pixel are visited in ascending iy, then ascending ix.  The integer weight is
    wgt = wy * wx, wy = min(y - y0 + 1, y0 + wh - y, o) and wx likewise (always >= 1).  acc starts at +0.0 and takes
    acc += (double)wgt * (s * (double)p + t) -- product, sum, product, sum -- with p the tile's float32 value as it is (not quantised).
    q = acc / (double)(sum of wgt), clamped by comparisons (q > 0 ? (q < 1 ? q : 1) : 0, so NaN -> 0), rounded once to float32.
  C = 3: one (s, t) per tile for the three channels.  Normals are NOT renormalised: the caller does that if it wants unit vectors.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .post_common import MAX_DIM, is_int, options_from, quantize16

MAX_TILES = 1024
ALIGNMENTS = ("least_square", "none")
AFFINE_INVARIANT_MODES = ("depth", "disparity")
OPTION_KEYS = ("size", "overlap", "align", "batch")
DEFAULT_BATCH = 4
f32, f64 = np.float32, np.float64


def axis_origins(L: int, size: int, overlap: int) -> Tuple[np.ndarray, int]:
    """One axis of the grid: (origins int32 [n], window w)."""
    if not (is_int(L) and is_int(size) and is_int(overlap)):
        raise ValueError(f"lengths, tile sizes and overlaps are integers, got {L!r}, {size!r}, {overlap!r}")
    L, size, o = int(L), int(size), int(overlap)
    if not 1 <= L <= MAX_DIM or size < 1:
        raise ValueError(f"an axis is 1 .. {MAX_DIM} long and a tile at least 1, got {L} and {size}")
    w = min(size, L)
    if not 1 <= o <= w // 2:
        raise ValueError(f"the overlap is in 1 .. w / 2 = {w // 2} for the window w = min({size}, {L}), got {o}")
    n = 1 if L <= w else -((o - L) // (w - o))
    k = np.arange(n, dtype=np.int64)
    return ((k * (L - w)) // max(n - 1, 1)).astype(np.int32), w


def tile_grid(H: int, W: int, size: int, overlap: int) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """The grid of the definition: (ys int32 [ny], xs int32 [nx], wh, ww).  ValueError outside the ranges."""
    ys, wh = axis_origins(H, size, overlap)
    xs, ww = axis_origins(W, size, overlap)
    if len(ys) * len(xs) > MAX_TILES:
        raise ValueError(f"at most {MAX_TILES} tiles, got {len(ys)} x {len(xs)}")
    return ys, xs, wh, ww


def tiles_options(tiles, processing_res=None, mode: str = "depth") -> Dict:
    """The `tiles` argument of the pipeline entries -- True or a dict with the keys size, overlap, align, batch -- as checked options.  The
    defaults: size = the processing resolution, overlap = size // 4, align = "least_square" for depth and disparity and "none" otherwise,
    batch = 4 tiles per model pass."""
    opts = options_from(tiles, dict(size=None, overlap=None, align=None, batch=DEFAULT_BATCH), "tiles")
    if opts["size"] is None:
        if not processing_res:
            raise ValueError("tiles: without a processing resolution (processing_res = 0) the tile size has to be given")
        opts["size"] = processing_res
    if not is_int(opts["size"]) or not 2 <= opts["size"] <= MAX_DIM:
        raise ValueError(f"tiles: size is an integer in 2 .. {MAX_DIM}, got {opts['size']!r}")
    if opts["overlap"] is None:
        opts["overlap"] = opts["size"] // 4
    if not is_int(opts["overlap"]) or not 1 <= opts["overlap"] <= opts["size"] // 2:
        raise ValueError(f"tiles: overlap is an integer in 1 .. size / 2 = {opts['size'] // 2}, got {opts['overlap']!r}")
    if opts["align"] is None:
        opts["align"] = "least_square" if mode in AFFINE_INVARIANT_MODES else "none"
    if opts["align"] not in ALIGNMENTS:
        raise ValueError(f"tiles: align is one of {ALIGNMENTS}, got {opts['align']!r}")
    if not is_int(opts["batch"]) or opts["batch"] < 1:
        raise ValueError(f"tiles: batch is a positive integer, got {opts['batch']!r}")
    return {k: (opts[k] if k == "align" else int(opts[k])) for k in OPTION_KEYS}


def _inputs(base, tiles, ys, xs, overlap, align):
    """The checked inputs: (base float32 [C, H, W], tiles float32 [N, C, wh, ww], ys, xs int32)."""
    base, tiles = np.asarray(base), np.asarray(tiles)
    if base.ndim == 2:
        base = base[None]
    if base.ndim != 3 or base.shape[0] not in (1, 3) or base.dtype.kind != "f":
        raise ValueError(f"base: float [C, H, W], C = 1 or 3, got {base.dtype} {base.shape}")
    if align not in ALIGNMENTS:
        raise ValueError(f"align is one of {ALIGNMENTS}, got {align!r}")
    if tiles.ndim != 4 or tiles.shape[1] != base.shape[0] or tiles.dtype.kind != "f":
        raise ValueError(f"tiles: float [N, {base.shape[0]}, wh, ww], got {tiles.dtype} {tiles.shape}")
    (C, H, W), (N, _, wh, ww) = base.shape, tiles.shape
    if wh > H or ww > W:
        raise ValueError(f"a {wh} x {ww} window does not fit a {H} x {W} image")
    want_ys, want_xs = axis_origins(H, wh, overlap)[0], axis_origins(W, ww, overlap)[0]  # (the window of an axis is its own tile size)
    if len(want_ys) * len(want_xs) > MAX_TILES:
        raise ValueError(f"at most {MAX_TILES} tiles, got {len(want_ys)} x {len(want_xs)}")
    ys, xs = np.asarray(ys), np.asarray(xs)
    if ys.dtype.kind not in "iu" or xs.dtype.kind not in "iu" or not np.array_equal(ys, want_ys) or not np.array_equal(xs, want_xs):
        raise ValueError(f"ys, xs are the origins of the grid rule, {want_ys.tolist()} and {want_xs.tolist()}, got {ys.tolist()} and {xs.tolist()}")
    if N != len(want_ys) * len(want_xs):
        raise ValueError(f"{len(want_ys)} x {len(want_xs)} tiles expected, got {N}")
    return base.astype(f32), tiles.astype(f32), want_ys, want_xs


def fit_sums(base: np.ndarray, tiles: np.ndarray, ys, xs) -> np.ndarray:
    """The integer sums of the definition, int64 [N, 5]: n, sum P, sum G, sum P^2, sum P G of every tile."""
    N, C, wh, ww = tiles.shape
    nx = len(xs)
    G16 = quantize16(base).astype(np.int64)
    out = np.zeros((N, 5), np.int64)
    for k in range(N):
        y0, x0 = int(ys[k // nx]), int(xs[k % nx])
        P = quantize16(tiles[k]).astype(np.int64)
        G = G16[:, y0:y0 + wh, x0:x0 + ww]
        out[k] = (P.size, P.sum(), G.sum(), (P * P).sum(), (P * G).sum())
    return out


def solve(sums: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(s, t) float64 [N] from the sums int64 [N, 5], in the order of the definition."""
    n, SP, SG, SPP, SPG = (sums[:, j].astype(f64) for j in range(5))
    with np.errstate(all="ignore"):
        mp = SP / n
        mg = SG / n
        var = SPP / n - mp * mp
        cov = SPG / n - mp * mg
        s = cov / var
        s = np.where((var >= 1.0) & (s > 0.0), s, f64(1.0))
        t = (mg - s * mp) / f64(65535.0)
    return s, t


def _fit(base, tiles, ys, xs, align):
    if align == "none":
        return np.ones(len(tiles), f64), np.zeros(len(tiles), f64)
    return solve(fit_sums(base, tiles, ys, xs))


def edge_weights(w: int, overlap: int) -> np.ndarray:
    """min(i + 1, w - i, o) of every index i of a window, int64 [w]."""
    i = np.arange(w, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, w - i), overlap)


def _blend(tiles, ys, xs, overlap, s, t, H, W) -> np.ndarray:
    N, C, wh, ww = tiles.shape
    nx = len(xs)
    wgt = edge_weights(wh, overlap)[:, None] * edge_weights(ww, overlap)[None, :]
    wf = wgt.astype(f64)
    acc, wsum = np.zeros((C, H, W), f64), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for k in range(N):  # ascending iy, then ascending ix
            y0, x0 = int(ys[k // nx]), int(xs[k % nx])
            acc[:, y0:y0 + wh, x0:x0 + ww] += wf * (s[k] * tiles[k].astype(f64) + t[k])
            wsum[y0:y0 + wh, x0:x0 + ww] += wgt
        q = acc / wsum.astype(f64)
    q = np.where(q > 0.0, np.where(q < 1.0, q, 1.0), 0.0)
    return np.ascontiguousarray(q.astype(f32))


def tile_fit(base, tiles, ys, xs, align: str = "least_square") -> Tuple[np.ndarray, np.ndarray]:
    """(s, t), float64 [N] each: every tile's fit onto its window of the base.  The fit does not depend on the overlap, so ys and xs are only
    held to lie inside the image here; `tile_merge` checks them against the grid rule."""
    base, tiles, ys, xs = np.asarray(base), np.asarray(tiles), np.asarray(ys), np.asarray(xs)
    if base.ndim == 2:
        base = base[None]
    if (base.ndim != 3 or tiles.ndim != 4 or base.shape[0] not in (1, 3) or tiles.shape[1] != base.shape[0] or align not in ALIGNMENTS
            or base.dtype.kind != "f" or tiles.dtype.kind != "f" or ys.ndim != 1 or xs.ndim != 1 or ys.dtype.kind not in "iu" or xs.dtype.kind not in "iu"
            or tiles.shape[0] != len(ys) * len(xs) or min(len(ys), len(xs), tiles.shape[2], tiles.shape[3]) < 1 or ys.min() < 0 or xs.min() < 0
            or ys.max() + tiles.shape[2] > base.shape[1] or xs.max() + tiles.shape[3] > base.shape[2]):
        raise ValueError(f"base float [C, H, W], C = 1 or 3; tiles float [ny * nx, C, wh, ww] with windows inside the image; align one of {ALIGNMENTS}")
    return _fit(base.astype(f32), tiles.astype(f32), ys, xs, align)


def tile_merge(base, tiles, ys, xs, overlap: int, align: str = "least_square") -> np.ndarray:
    """One image by the definition above: base float [C, H, W] (or [H, W]), tiles float [N, C, wh, ww], the grid's origins ys [ny] and xs [nx]
    (N = ny * nx, as `tile_grid` gives them) -> float32 [C, H, W] in [0, 1]."""
    base, tiles, ys, xs = _inputs(base, tiles, ys, xs, overlap, align)
    s, t = _fit(base, tiles, ys, xs, align)
    return _blend(tiles, ys, xs, int(overlap), s, t, base.shape[1], base.shape[2])
