"""Stereo and parallax views from depth, the host route (numpy, no torch): the photograph re-rendered from viewpoints shifted sideways under
its depth or disparity prediction -- side-by-side frames, red/cyan anaglyphs, "wiggle" pairs, the quilts of lenticular and light-field
displays.  A forward warp (depth-image-based rendering): every row is a 1-D surface that is cut at depth edges and rasterised, the nearest
surface wins where two land on one pixel, and the holes a new viewpoint opens are filled from the background side.  This file is the
specification in executable form, one vectorised pass per source offset; csrc/stereo.hip (gp_stereo_views) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the arithmetic once more in csrc/stereo_math.h)
  Per image: image uint8 [3, H, W]; pred float32 [1, H, W]; one integer F in 0 .. 65535, the nearness of the zero-parallax plane.  Per call:
    space "depth" or "disparity"; edge 0 .. 65535; max_s8 0 .. 512 (a shift of at most 64 pixels, in eighths); a table of V rows
    (g, ox, oy, cmask), 1 <= V <= 64, |g| <= 131072, (ox, oy) the origin of the view's H x W rectangle in the canvas, cmask in 1 .. 7 the
    channels it writes.  1 <= H, W <= 16384 and B * V * H * W < 2^31.
  1. Nearness: Q = quantize16(pred); D = Q in disparity space, D = 65535 - Q in depth space; a NaN pixel has D = 0 (`post_common.nearness`).
  2. Shift of source column x for a view, in eighths of a pixel: s = ((D - F) * g + 2^23) >> 24, a floor, clamped to -max_s8 .. max_s8;
     t_x = 8 x + s.
  3. x and x + 1 are connected iff |D_x - D_{x+1}| <= edge.  Output column p, at P = 8 p, is covered by the span of a connected pair with
     L = t_{x+1} - t_x > 0 and t_x <= P < t_{x+1} (with a = P - t_x: nearness (D_x (L - a) + D_{x+1} a + (L >> 1)) // L, the colours
     likewise), by the left cap of x, t_x - 4 <= P < t_x, iff x = 0 or (x - 1, x) is not connected, and by the right cap of x,
     t_x <= P < t_x + 4, iff x = W - 1 or (x, x + 1) is not connected (both caps: D_x, c_x).  A connected pair with L <= 0 covers nothing.
  4. The piece with the largest nearness wins, the smallest x on a tie.
  5. A column nothing covers is a hole: it takes the colour and nearness of the nearest covered column within R = max_s8 // 4 + 1 columns to
     its left or right, the one with the SMALLER nearness, the left one on a tie; colour 0 and nearness 0 where neither exists.
  6. canvas uint8 [B, 3, CH, CW]: view k writes its cmask channels at (oy + y, ox + x), other bytes keep what they held; holes uint8
     [B, V, H, W]; near uint16 [B, V, H, W], the new view's own map.

The user's terms (`view_table`, `stereo_options`).  `separation` is the parallax in pixels between the outermost views at the two ends of
the nearness scale.  View k of V sits at e_k = k / (V - 1) - 1/2 (e = -1/2, +1/2 for V = 2; 0 for V = 1), view 0 is the leftmost camera, and
g_k = -round(e_k * separation * 8 * 2^24 / 65535), halves rounded up: a camera moved to the right sees near things move left.  The largest
shift any pixel can get, (span * |g| + 2^23) >> 24 with span = 65535 (or max(F, 65535 - F) where F is known on the host), must not exceed 512
eighths.  `edge` is a fraction of the map's range, floor(65535 * edge + 1/2); its default EDGE_DEFAULT = 0.04 is a convention, not a
measurement.  `converge` is a value of the map in [0, 1] (F is its nearness) or `converge_at` = (u, v) the pixel whose nearness is F; at most
one may be given, and with neither F = 32768, the middle of the scale.  Layouts: "pair" (two views, canvas [3, H, 2 W], the left eye in the
left half), "sbs" (V views in a row), "over_under" (V views in a column, view 0 on top), "anaglyph" (two views at (0, 0); view 0, the left
eye, writes red, view 1 green and blue) and "quilt" (views = (ny, nx): view 0 at the BOTTOM left, then to the right and upwards -- the
order light-field displays read a quilt in, a convention).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .post_common import (EDGE_DEFAULT, F_DEFAULT, MAX_DIM, SPACES, _check_space, _count_limit, _edge16, _images_and_maps,  # noqa: F401
                          _pixel_inside, _plane, _plane_F, _plane_span, _warp_integers, _with_planes, is_int, nearness, quantize16)

MAX_VIEWS = 64
MAX_S8 = 512
MAX_G = 131072
CAP = 4
LAYOUTS = ("pair", "sbs", "over_under", "anaglyph", "quilt")
i64 = np.int64


# ---- the user's terms ---------------------------------------------------------------------------------------------------------------------------------
def view_gains(n_views: int, separation: float) -> np.ndarray:
    """g_k = -round(e_k * separation * 8 * 2^24 / 65535) for e_k = k / (V - 1) - 1/2, int64 [V]."""
    if not is_int(n_views) or not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"1 .. {MAX_VIEWS} views, got {n_views!r}")
    sep = float(separation)
    if not np.isfinite(sep):
        raise ValueError(f"separation is a finite number of pixels, got {separation!r}")
    e = np.arange(n_views, dtype=np.float64) / max(1, n_views - 1) - (0.5 if n_views > 1 else 0.0)
    g = -np.floor(e * sep * 8.0 * 16777216.0 / 65535.0 + 0.5).astype(i64)
    if (np.abs(g) > MAX_G).any():
        raise ValueError(f"separation {separation!r} needs a shift of more than 64 pixels")
    return g


def max_shift8(gains, span: int = 65535) -> int:
    """The largest |s| a pixel at most `span` away from F in nearness can get under these gains, in eighths of a pixel."""
    g = int(np.abs(np.asarray(gains, i64)).max())
    return (int(span) * g + (1 << 23)) >> 24


def view_table(layout: str, views, separation: float, H: int, W: int) -> Tuple[np.ndarray, Tuple[int, int]]:
    """The rows (g, ox, oy, cmask) of a layout, int32 [V, 4], and the canvas size (CH, CW).  views: the number of views (2 for "pair" and
    "anaglyph", the only count they take), or (ny, nx) for "quilt"."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout is one of {LAYOUTS}, got {layout!r}")
    if layout == "quilt":
        if not isinstance(views, (tuple, list)) or len(views) != 2 or not all(is_int(v) and v >= 1 for v in views):
            raise ValueError(f"a quilt takes views = (ny, nx), got {views!r}")
        ny, nx = (int(v) for v in views)
        n = ny * nx
    else:
        if not is_int(views) or views < 1:
            raise ValueError(f"views is a count, got {views!r}")
        n = int(views)
        if layout in ("pair", "anaglyph") and n != 2:
            raise ValueError(f"{layout} takes two views, got {n}")
    g = view_gains(n, separation)
    k = np.arange(n)
    zero, full = np.zeros(n, i64), np.full(n, 7, i64)
    if layout in ("pair", "sbs"):
        ox, oy, cmask, size = k * W, zero, full, (H, n * W)
    elif layout == "over_under":
        ox, oy, cmask, size = zero, k * H, full, (n * H, W)
    elif layout == "anaglyph":
        ox, oy, cmask, size = zero, zero, np.array([1, 6], i64), (H, W)
    else:
        ox, oy, cmask, size = (k % nx) * W, (ny - 1 - k // nx) * H, full, (ny * H, nx * W)
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or size[0] > MAX_DIM or size[1] > MAX_DIM:
        raise ValueError(f"images of {H} x {W} in a canvas of {size[0]} x {size[1]}: sides in 1 .. {MAX_DIM}")
    return np.stack([g, ox, oy, cmask], 1).astype(np.int32), size


def stereo_options(B: int, converge=None, converge_at=None, edge=EDGE_DEFAULT) -> Dict:
    """converge, converge_at and edge checked (ValueError outside their ranges) and spread over the B images: a dict of converge float32 [B]
    or None, converge_at int64 [B, 2] = (u, v) or None -- at most one of the two is given --, and the integer edge."""
    value, at = _plane(B, converge, converge_at, "converge", "converge_at", exactly_one=False)
    return dict(converge=value, converge_at=at, edge=_edge16(edge))


def plan(B: int, H: int, W: int, layout="sbs", views=2, separation=16.0, converge=None, converge_at=None, edge=EDGE_DEFAULT) -> Dict:
    """Everything of a call that needs no map: the options of `stereo_options`, the table and canvas size of `view_table`, and max_s8, the
    largest shift in eighths -- from the gains and, where `converge` fixes F on the host, from how far a nearness can lie from it.
    ValueError where that shift exceeds 64 pixels, or where converge_at lies outside the image."""
    o = stereo_options(B, converge, converge_at, edge)
    table, size = view_table(layout, views, separation, H, W)
    _pixel_inside(o["converge_at"], "converge_at", H, W)
    max_s8 = max_shift8(table[:, 0], _plane_span(B, o["converge"], o["converge_at"], F_DEFAULT))
    if max_s8 > MAX_S8:
        raise ValueError(f"separation {separation!r} needs a shift of {max_s8 / 8:g} pixels, more than 64")
    _count_limit(B, table.shape[0], H, W)
    o.update(table=table, size=size, max_s8=max_s8)
    return o


def convergence(pred, space: str, o: Dict) -> np.ndarray:
    """F int64 [B] of the options `o` and, for converge_at, the maps pred [B, H, W]."""
    return _plane_F(pred, space, o["converge"], o["converge_at"], F_DEFAULT)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------
def shifts(D, F: int, g: int, max_s8: int) -> np.ndarray:
    """Step 2: s int64 of the nearness D."""
    return np.clip(((np.asarray(D, i64) - int(F)) * int(g) + (1 << 23)) >> 24, -int(max_s8), int(max_s8))


def warp_rows(D, rgb, F: int, g: int, edge: int, max_s8: int):
    """Steps 2 to 4 for one image and one view: D int64 [H, W], rgb int64 [3, H, W] -> (near int64 [H, W], -1 where nothing covers the
    column; colours int64 [3, H, W]; the number of pieces that cover each column, int64 [H, W]).  One pass per source offset in increasing
    x, so that a later piece has to be strictly nearer to win."""
    H, W = D.shape
    s = shifts(D, F, g, max_s8)
    reach = (int(np.abs(s).max()) + 7) >> 3
    pad = reach + 1
    Wp = W + 2 * pad
    Dp, tp, ex = np.zeros((H, Wp), i64), np.zeros((H, Wp), i64), np.zeros((H, Wp), bool)
    cp = np.zeros((3, H, Wp), i64)
    Dp[:, pad:pad + W], tp[:, pad:pad + W], ex[:, pad:pad + W], cp[:, :, pad:pad + W] = D, 8 * np.arange(W, dtype=i64)[None] + s, True, rgb
    conn = np.zeros((H, Wp), bool)                      # conn[x]: x and x + 1 are connected
    conn[:, :-1] = ex[:, :-1] & ex[:, 1:] & (np.abs(Dp[:, :-1] - Dp[:, 1:]) <= edge)
    P = 8 * np.arange(W, dtype=i64)[None]
    best, out, count = np.full((H, W), -1, i64), np.zeros((3, H, W), i64), np.zeros((H, W), i64)
    for d in range(-reach, reach + 1):
        x0, x1, xm = slice(pad + d, pad + d + W), slice(pad + d + 1, pad + d + 1 + W), slice(pad + d - 1, pad + d - 1 + W)
        t0, t1, D0, D1, right, left, here = tp[:, x0], tp[:, x1], Dp[:, x0], Dp[:, x1], conn[:, x0], conn[:, xm], ex[:, x0]
        L = t1 - t0
        span = right & (L > 0) & (t0 <= P) & (P < t1)
        cap = here & ((~right & (t0 <= P) & (P < t0 + CAP)) | (~left & (t0 - CAP <= P) & (P < t0)))
        Ls, a = np.where(span, L, 1), np.where(span, P - t0, 0)
        value = np.where(span, (D0 * (Ls - a) + D1 * a + (Ls >> 1)) // Ls, np.where(cap, D0, -1))
        better = value > best
        if better.any():
            colour = np.where(span[None], (cp[:, :, x0] * (Ls - a)[None] + cp[:, :, x1] * a[None] + (Ls >> 1)[None]) // Ls[None], cp[:, :, x0])
            best = np.where(better, value, best)
            out = np.where(better[None], colour, out)
        count += span.astype(i64) + cap
    return best, out, count


def fill_holes(near, colours, max_s8: int):
    """Step 5 for one image and one view: near int64 [H, W] with -1 in the holes, colours int64 [3, H, W] -> (near, colours, holes bool)."""
    H, W = near.shape
    R = int(max_s8) // 4 + 1
    covered = near >= 0
    idx = np.arange(W, dtype=i64)[None]
    far = 4 * MAX_DIM
    left = np.maximum.accumulate(np.where(covered, idx, -far), axis=1)
    right = np.minimum.accumulate(np.where(covered, idx, far)[:, ::-1], axis=1)[:, ::-1]
    has_l, has_r = idx - left <= R, right - idx <= R
    near_l = np.take_along_axis(near, np.clip(left, 0, W - 1), 1)
    near_r = np.take_along_axis(near, np.clip(right, 0, W - 1), 1)
    from_left = has_l & (~has_r | (near_l <= near_r))
    src = np.clip(np.where(from_left, left, right), 0, W - 1)
    some = has_l | has_r
    holes = ~covered
    filled = np.where(holes, np.where(some, np.take_along_axis(near, src, 1), 0), near)
    taken = np.where(some[None], np.take_along_axis(colours, np.broadcast_to(src[None], colours.shape), 2), 0)
    return filled, np.where(holes[None], taken, colours), holes


def check_table(table, H: int, W: int, CH: int, CW: int) -> np.ndarray:
    """The view table as a checked contiguous int32 [V, 4] array: the ranges of the definition, every rectangle inside the canvas, and no
    two rectangles that overlap and share a channel."""
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[1] != 4 or not 1 <= t.shape[0] <= MAX_VIEWS:
        raise ValueError(f"table: integers (g, ox, oy, cmask) for 1 .. {MAX_VIEWS} views, got {t.dtype} {t.shape}")
    t = t.astype(i64)
    g, ox, oy, cmask = t.T
    if not (1 <= CH <= MAX_DIM and 1 <= CW <= MAX_DIM):
        raise ValueError(f"canvas sides in 1 .. {MAX_DIM}, got {(CH, CW)}")
    if (np.abs(g) > MAX_G).any() or (cmask < 1).any() or (cmask > 7).any():
        raise ValueError(f"table: |g| <= {MAX_G} and cmask in 1 .. 7, got {t.tolist()}")
    if (ox < 0).any() or (oy < 0).any() or (ox + W > CW).any() or (oy + H > CH).any():
        raise ValueError(f"table: a {H} x {W} rectangle leaves the {CH} x {CW} canvas, got {t.tolist()}")
    for j in range(len(t)):
        for k in range(j):
            if cmask[j] & cmask[k] and abs(ox[j] - ox[k]) < W and abs(oy[j] - oy[k]) < H:
                raise ValueError(f"table: views {k} and {j} overlap and share a channel")
    return np.ascontiguousarray(t.astype(np.int32))


def stereo_views_table(image, pred, F, table, canvas, space: str = "depth", edge: int = 0, max_s8: int = MAX_S8, want_cover: bool = False):
    """A batch by the definition above from its integers.  image uint8 [B, 3, H, W] ([3, H, W]: one image); pred float [B, 1, H, W]
    ([B, H, W] with B images, [H, W] with one); F integers [B] or one; table integers [V, 4]; canvas: uint8 [B, 3, CH, CW], written IN PLACE,
    or its size (CH, CW), a canvas of zeros.  Returns (canvas, holes uint8 [B, V, H, W], near uint16 [B, V, H, W]), and with want_cover also
    the number of pieces that cover each column, int64 [B, V, H, W]."""
    _check_space(space)
    image, pred = _images_and_maps(image, pred)
    B, _, H, W = image.shape
    F = _warp_integers(F, B, edge, max_s8, MAX_S8)
    if not isinstance(canvas, np.ndarray):
        canvas = np.zeros((B, 3) + tuple(int(v) for v in canvas), np.uint8)
    if canvas.dtype != np.uint8 or canvas.ndim != 4 or canvas.shape[:2] != (B, 3):
        raise ValueError(f"canvas: uint8 {(B, 3, 'CH', 'CW')}, got {canvas.dtype} {canvas.shape}")
    table = check_table(table, H, W, canvas.shape[2], canvas.shape[3])
    V = table.shape[0]
    _count_limit(B, V, H, W)
    holes, near, cover = np.empty((B, V, H, W), np.uint8), np.empty((B, V, H, W), np.uint16), np.empty((B, V, H, W), i64)
    for b in range(B):
        D, rgb = nearness(pred[b], space), image[b].astype(i64)
        for k, (g, ox, oy, cmask) in enumerate(table.tolist()):
            best, colours, cover[b, k] = warp_rows(D, rgb, int(F[b]), g, int(edge), int(max_s8))
            filled, colours, hole = fill_holes(best, colours, int(max_s8))
            holes[b, k], near[b, k] = hole, filled
            for ch in range(3):
                if cmask >> ch & 1:
                    canvas[b, ch, oy:oy + H, ox:ox + W] = colours[ch]
    return (canvas, holes, near, cover) if want_cover else (canvas, holes, near)


def stereo_views(image, pred, layout="sbs", views=2, separation=16.0, converge=None, converge_at=None, edge=EDGE_DEFAULT, space: str = "depth",
                 want_holes: bool = False, want_near: bool = False):
    """`stereo_views_table` from the user's terms (module docstring).  Returns the canvas uint8 [B, 3, CH, CW], and with want_holes /
    want_near a tuple with those planes after it."""
    _check_space(space)
    image, pred = _images_and_maps(image, pred)
    B, _, H, W = image.shape
    o = plan(B, H, W, layout, views, separation, converge, converge_at, edge)
    canvas, holes, near = stereo_views_table(image, pred, convergence(pred, space, o), o["table"], o["size"], space, o["edge"], o["max_s8"])
    return _with_planes(canvas, holes, near, want_holes, want_near)
