"""Camera moves from one photograph, the host route (numpy, no torch): the "3-D photo", a short clip in which the camera orbits, swings or
pushes into a single still under its depth or disparity prediction.  A forward warp in two dimensions: the picture is a triangle mesh over the
pixel grid that is cut at depth edges and rasterised with a z-test, so the subject keeps its outline where a `grid_sample` by the flow smears
it, and the holes a move opens are filled from the background side.  This file is the specification in executable form, every piece scattered
over the pixels of its bounding box in one vectorised pass; csrc/parallax.hip (gp_parallax_frames) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the arithmetic once more in csrc/parallax_math.h)
  Per image: image uint8 [3, H, W]; pred float32 [1, H, W]; one integer F in 0 .. 65535, the nearness of the plane that stays put.  Per call:
    space "depth" or "disparity"; edge 0 .. 65535; max_s8 0 .. 256 (a displacement of at most 32 pixels, in eighths); a table of V rows
    (gx, gy, gz, Z), 1 <= V <= 64, |gx|, |gy| <= 2^17, |gz| <= 2^24, Z in 65536 .. 131072 (a zoom of 1 x to 2 x in units of 1 / 65536).
    1 <= H, W <= 16384 and B * V * H * W < 2^31.
  1. Nearness: D = `post_common.nearness`(pred, space), larger is nearer, 0 for a NaN pixel.
  2. Position of source (x, y) in a frame, in eighths of a pixel: Cx = 4 (W - 1), Cy = 4 (H - 1); rx = 8 x - Cx, ry = 8 y - Cy; e = D - F;
     dz = (e gz + 2^23) >> 24; dx = ((e gx + 2^23) >> 24) + ((rx dz + 2^15) >> 16), clamped to -max_s8 .. max_s8, dy likewise with gy and ry;
     tx = Cx + ((rx Z + 2^15) >> 16) + dx, ty likewise.  Every shift is a floor.  Z + dz is the magnification of a pixel: a camera pushed
     forward magnifies near things more.
  3. Pieces.  Two pixels are connected iff |D_a - D_b| <= edge.  Output pixel (p, q) sits at P = (8 p, 8 q).
     Cap: every source has one, the square tx - h <= Px < tx + h, ty - h <= Py < ty + h with h = (4 Z + 65535) >> 16; D and c of the source;
       piece id 3 (y W + x).
     Triangles: each quad with x + 1 < W and y + 1 < H gives T0 = (x, y), (x + 1, y), (x, y + 1), id 3 (y W + x) + 1, and
       T1 = (x + 1, y), (x + 1, y + 1), (x, y + 1), id 3 (y W + x) + 2; a triangle exists iff its three vertex pairs are all connected.  With
       the vertices a, b, c in that order A = (b - a) x (c - a); a triangle with A <= 0 covers nothing (it is folded);
       wa = (c - b) x (P - b), wb = (a - c) x (P - c), wc = A - wa - wb; it covers P iff all three are >= 0; its nearness there is
       (wa D_a + wb D_b + wc D_c + (A >> 1)) // A and each colour channel likewise.
  4. Visibility: the piece with the largest nearness wins, the smallest piece id on a tie.
  5. Holes: a pixel nothing covers takes the nearest covered pixel to its left, to its right, above and below, each within
     R = max_s8 // 4 + 1; of those the one with the smallest nearness, ties in the order left, right, up, down; it copies that pixel's colour
     and nearness; colour 0 and nearness 0 where none exists.
  6. frames uint8 [B, V, 3, H, W]; holes uint8 [B, V, H, W]; near uint16 [B, V, H, W], the frame's own map.

The user's terms (`camera_path`, `plan`).  `amount` is the parallax in pixels between the two ends of the nearness scale:
G = rnd(amount * 8 * 2^24 / 65535) with rnd(v) = floor(v + 1/2), halves rounded up as in `stereo.view_gains`.  With theta_k = 2 pi k / V:
"swing" has gx = -rnd(G / 2 * sin theta_k); "orbit" has gx = -rnd(G / 2 * cos theta_k), gy = -rnd(G / 2 * sin theta_k); "dolly", with
u_k = k / (V - 1) (0 for V = 1), has gz = rnd(u_k * push * 2^24) and Z = rnd(65536 (1 + u_k (zoom - 1))) and, with `pan`, gx = rnd((u_k - 1/2) G),
a linear pan from -G / 2 to +G / 2.  Alternatively the path is an explicit [V, 4] array of (shift_x, shift_y, push, zoom) per frame:
gx = rnd(shift_x * 8 * 2^24 / 65535), gy likewise, gz = rnd(push * 2^24), Z = rnd(65536 zoom).  The trigonometry runs in float64 here; only
integers reach the entry.  A frame's largest possible displacement along an axis with centre C is, in eighths,
  s8 = ((span |g| + 2^23) >> 24) + ((C dzmax + 2^15) >> 16), dzmax = (span |gz| + 2^23) >> 24,
with span = 65535, or max(F, 65535 - F) where F is known on the host; max_s8 is the largest over the axes and frames of the WHOLE path.
`overscan` (the default) raises each frame's Z to at least 65536 + ceil(16384 s8_k / (min(H, W) - 1)), that is a zoom of
1 + 2 S_k / (min(H, W) - 1) for the frame's largest displacement S_k = s8_k / 8 pixels, so that the borders a move would expose stay outside
the frame.  ValueError for a bound over 256 eighths, a zoom over 2 and a zoom under 1.  `focus` / `focus_at`, `edge` and their defaults follow the
rules of `converge` / `converge_at` / `edge` in `stereo.py`.  A path may be longer than one call's 64 frames: `frame_range` picks the rows
of a call, and max_s8 and the rows are those of the whole path whichever range is taken.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from .post_common import (EDGE_DEFAULT, F_DEFAULT, MAX_DIM, SPACES, _check_space, _count_limit, _edge16, _images_and_maps, _pixel_inside,  # noqa: F401
                          _plane, _plane_F, _plane_span, _warp_integers, _with_planes, is_int, nearness)

MAX_FRAMES = 64            # the rows of one call
MAX_PATH = 4096            # the frames of a path, taken MAX_FRAMES at a time
MAX_S8 = 256
MAX_G = 131072
MAX_GZ = 1 << 24
Z_MIN, Z_MAX = 65536, 131072
KINDS = ("swing", "orbit", "dolly")
PAIR_CHUNK = 1 << 21       # (piece, pixel) pairs evaluated at a time
i64 = np.int64


def _rnd(v) -> np.ndarray:
    return np.floor(np.asarray(v, np.float64) + 0.5).astype(i64)


# ---- the user's terms ---------------------------------------------------------------------------------------------------------------------------------
def amount_gain(amount: float) -> int:
    """G = rnd(amount * 8 * 2^24 / 65535)."""
    a = float(amount)
    if not np.isfinite(a):
        raise ValueError(f"amount is a finite number of pixels, got {amount!r}")
    return int(_rnd(a * 8.0 * 16777216.0 / 65535.0))


def camera_path(path="orbit", frames: int = 16, amount: float = 16.0, push: float = 0.0, zoom: float = 1.0, pan: bool = False) -> np.ndarray:
    """The rows (gx, gy, gz, Z) of a path before `overscan`, int64 [V, 4].  path: one of KINDS with `frames` frames, or an explicit [V, 4]
    array of (shift_x, shift_y, push, zoom) per frame (frames, amount, push, zoom and pan are then not used)."""
    if isinstance(path, str):
        if path not in KINDS:
            raise ValueError(f"path is one of {KINDS} or a [V, 4] array, got {path!r}")
        if not is_int(frames) or not 1 <= frames <= MAX_PATH:
            raise ValueError(f"1 .. {MAX_PATH} frames, got {frames!r}")
        V, G = int(frames), amount_gain(amount)
        k = np.arange(V, dtype=np.float64)
        theta = 2.0 * np.pi * k / V
        rows = np.zeros((V, 4), i64)
        rows[:, 3] = Z_MIN
        if path == "swing":
            rows[:, 0] = -_rnd(G / 2.0 * np.sin(theta))
        elif path == "orbit":
            rows[:, 0], rows[:, 1] = -_rnd(G / 2.0 * np.cos(theta)), -_rnd(G / 2.0 * np.sin(theta))
        else:
            if not np.isfinite(float(push)) or not np.isfinite(float(zoom)):
                raise ValueError(f"push and zoom are finite, got {push!r} and {zoom!r}")
            u = k / max(1, V - 1)
            rows[:, 2], rows[:, 3] = _rnd(u * float(push) * 16777216.0), _rnd(65536.0 * (1.0 + u * (float(zoom) - 1.0)))
            if pan:
                rows[:, 0] = _rnd((u - 0.5) * G)
    else:
        a = np.asarray(path, np.float64)
        if a.ndim != 2 or a.shape[1] != 4 or not 1 <= a.shape[0] <= MAX_PATH or not np.isfinite(a).all():
            raise ValueError(f"an explicit path is finite (shift_x, shift_y, push, zoom) for 1 .. {MAX_PATH} frames, got {a.shape}")
        rows = np.stack([_rnd(a[:, 0] * 8.0 * 16777216.0 / 65535.0), _rnd(a[:, 1] * 8.0 * 16777216.0 / 65535.0), _rnd(a[:, 2] * 16777216.0),
                         _rnd(65536.0 * a[:, 3])], 1)
    if (rows[:, 3] < Z_MIN).any():
        raise ValueError(f"a zoom under 1 would show the borders of the image, got {rows[:, 3].min() / 65536.0:g}")
    if (rows[:, 3] > Z_MAX).any():
        raise ValueError(f"a zoom of at most 2, got {rows[:, 3].max() / 65536.0:g}")
    if (np.abs(rows[:, :2]) > MAX_G).any() or (np.abs(rows[:, 2]) > MAX_GZ).any():
        raise ValueError("the path needs a displacement of more than 32 pixels (|gx|, |gy| <= 2^17, |gz| <= 2^24)")
    return rows


def frame_bounds8(rows, H: int, W: int, span: int = 65535) -> np.ndarray:
    """The largest displacement a pixel at most `span` away from F in nearness can get in each frame, in eighths of a pixel: int64 [V]."""
    rows = np.asarray(rows, i64).reshape(-1, 4)
    span = int(span)
    dz = (span * np.abs(rows[:, 2]) + (1 << 23)) >> 24
    sx = ((span * np.abs(rows[:, 0]) + (1 << 23)) >> 24) + ((4 * (W - 1) * dz + (1 << 15)) >> 16)
    sy = ((span * np.abs(rows[:, 1]) + (1 << 23)) >> 24) + ((4 * (H - 1) * dz + (1 << 15)) >> 16)
    return np.maximum(sx, sy)


def plan(B: int, H: int, W: int, path="orbit", frames: int = 16, amount: float = 16.0, push: float = 0.0, zoom: float = 1.0, pan: bool = False,
         focus=None, focus_at=None, edge=EDGE_DEFAULT, overscan: bool = True, frame_range: Optional[Tuple[int, int]] = None) -> Dict:
    """Everything of a call that needs no map: focus float32 [B] or None, focus_at int64 [B, 2] or None, the integer edge, the table int32
    [V, 4] of the frames `frame_range` = (first, end) picks from the path (all of them without it), n_path, the length of the whole path, and
    max_s8, the largest displacement bound over the whole path.  ValueError for a bound over 32 pixels, a zoom outside 1 .. 2 (after
    `overscan`), a focus_at outside the image, more than 64 frames in one call, B * V * H * W >= 2^31."""
    value, at = _plane(B, focus, focus_at, "focus", "focus_at", exactly_one=False)
    o = dict(focus=value, focus_at=at, edge=_edge16(edge))
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or B < 1:
        raise ValueError(f"images with sides in 1 .. {MAX_DIM}, got {(B, H, W)}")
    _pixel_inside(at, "focus_at", H, W)
    rows = camera_path(path, frames, amount, push, zoom, pan)
    s8 = frame_bounds8(rows, H, W, _plane_span(B, value, at, F_DEFAULT))
    max_s8 = int(s8.max())
    if max_s8 > MAX_S8:
        raise ValueError(f"the path needs a displacement of {max_s8 / 8:g} pixels, more than {MAX_S8 // 8}")
    if overscan:
        rows[:, 3] = np.maximum(rows[:, 3], Z_MIN + -((-16384 * s8) // max(1, min(H, W) - 1)))
        if (rows[:, 3] > Z_MAX).any():
            raise ValueError(f"overscan needs a zoom of {rows[:, 3].max() / 65536.0:g}, more than 2: a smaller move, or overscan=False")
    n_path = rows.shape[0]
    first, end = (0, n_path) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
    if not 0 <= first < end <= n_path:
        raise ValueError(f"frame_range = (first, end) within the {n_path} frames of the path, got {frame_range!r}")
    if end - first > MAX_FRAMES:
        raise ValueError(f"at most {MAX_FRAMES} frames in one call, got {end - first}: take the path in parts with frame_range")
    _count_limit(B, end - first, H, W)
    o.update(table=np.ascontiguousarray(rows[first:end].astype(np.int32)), n_path=n_path, max_s8=max_s8)
    return o


def focus_plane(pred, space: str, o: Dict) -> np.ndarray:
    """F int64 [B] of the options `o` and, for focus_at, the maps pred [B, H, W]."""
    return _plane_F(pred, space, o["focus"], o["focus_at"], F_DEFAULT)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------
def positions(D, F: int, frame, max_s8: int):
    """Step 2: (tx, ty) int64 [H, W] of the nearness D, and whether any displacement met the clamp."""
    H, W = D.shape
    gx, gy, gz, Z = (int(v) for v in frame)
    Cx, Cy = 4 * (W - 1), 4 * (H - 1)
    rx, ry = (8 * np.arange(W, dtype=i64) - Cx)[None], (8 * np.arange(H, dtype=i64) - Cy)[:, None]
    e = np.asarray(D, i64) - int(F)
    dz = (e * gz + (1 << 23)) >> 24
    raw_x = ((e * gx + (1 << 23)) >> 24) + ((rx * dz + (1 << 15)) >> 16)
    raw_y = ((e * gy + (1 << 23)) >> 24) + ((ry * dz + (1 << 15)) >> 16)
    tx = Cx + ((rx * Z + (1 << 15)) >> 16) + np.clip(raw_x, -max_s8, max_s8)
    ty = Cy + ((ry * Z + (1 << 15)) >> 16) + np.clip(raw_y, -max_s8, max_s8)
    return tx, ty, bool((np.abs(raw_x) > max_s8).any() or (np.abs(raw_y) > max_s8).any())


def _pairs(lo_x, hi_x, lo_y, hi_y):
    """Every pixel of every bounding box lo .. hi (inclusive; empty where hi < lo): (index of the box, px, py), flat."""
    w, h = np.maximum(hi_x - lo_x + 1, 0), np.maximum(hi_y - lo_y + 1, 0)
    n = w * h
    which = np.repeat(np.arange(n.size, dtype=i64), n)
    off = np.arange(int(n.sum()), dtype=i64) - (np.cumsum(n) - n)[which]
    ww = w[which]
    return which, lo_x[which] + off % ww, lo_y[which] + off // ww


def _chunks(n_pixels):
    """Runs of boxes with about PAIR_CHUNK pixels each."""
    total = np.cumsum(n_pixels)
    start = 0
    while start < n_pixels.size:
        base = int(total[start - 1]) if start else 0
        end = max(start + 1, int(np.searchsorted(total, base + PAIR_CHUNK, side="right")))
        yield slice(start, end)
        start = end


def _barycentric(v, Px, Py):
    """Step 3 for triangles with the vertices v = (tx [3, n], ty [3, n]) and A > 0 at the points P: (covers, wa, wb, wc, A)."""
    tx, ty = v
    A = (tx[1] - tx[0]) * (ty[2] - ty[0]) - (ty[1] - ty[0]) * (tx[2] - tx[0])
    wa = (tx[2] - tx[1]) * (Py - ty[1]) - (ty[2] - ty[1]) * (Px - tx[1])
    wb = (tx[0] - tx[2]) * (Py - ty[2]) - (ty[0] - ty[2]) * (Px - tx[2])
    wc = A - wa - wb
    return (wa >= 0) & (wb >= 0) & (wc >= 0), wa, wb, wc, A


TRIANGLES = (((0, 0), (0, 1), (1, 0)), ((0, 1), (1, 1), (1, 0)))      # (dy, dx) of the vertices a, b, c of T0 and T1


def warp_frame(D, rgb, F: int, frame, edge: int, max_s8: int, want_stats: bool = False):
    """Steps 2 to 4 for one image and one frame: D int64 [H, W], rgb int64 [3, H, W] -> (near int64 [H, W], -1 where nothing covers the
    pixel; colours int64 [3, H, W]), and with want_stats a dict after them: piece int64 [H, W], the id of the winning piece (-1: none);
    cover int64 [H, W], the pieces that cover each pixel; triangles int64 [H, W], the triangles among them; ties int64 [H, W], those of them with the winning nearness; folded, the number of
    existing triangles with A <= 0; clamped, whether a displacement met the clamp."""
    H, W = D.shape
    Z = int(frame[3])
    tx, ty, clamped = positions(D, F, frame, max_s8)
    h = (4 * Z + 65535) >> 16
    ids = 3 * np.arange(H * W, dtype=i64).reshape(H, W)
    ceil8 = lambda v: -((-v) // 8)  # noqa: E731

    def boxes(lo_x, hi_x, lo_y, hi_y):
        return np.maximum(lo_x, 0), np.minimum(hi_x, W - 1), np.maximum(lo_y, 0), np.minimum(hi_y, H - 1)

    # the pieces: their ids, the boxes of output pixels they can cover, and for the triangles the positions, nearness and colours of a, b, c
    pieces = [dict(id=ids.ravel(), box=boxes(*(a.ravel() for a in (ceil8(tx - h), ceil8(tx + h) - 1, ceil8(ty - h), ceil8(ty + h) - 1))), src=np.arange(H * W))]
    folded = 0
    if H > 1 and W > 1:
        for t, corners in enumerate(TRIANGLES):
            sl = [(slice(dy, H - 1 + dy), slice(dx, W - 1 + dx)) for dy, dx in corners]
            Dv = np.stack([D[s] for s in sl])
            exists = (np.abs(Dv[0] - Dv[1]) <= edge) & (np.abs(Dv[1] - Dv[2]) <= edge) & (np.abs(Dv[0] - Dv[2]) <= edge)
            vx, vy = np.stack([tx[s] for s in sl]), np.stack([ty[s] for s in sl])
            A = (vx[1] - vx[0]) * (vy[2] - vy[0]) - (vy[1] - vy[0]) * (vx[2] - vx[0])
            folded += int((exists & (A <= 0)).sum())
            keep = exists & (A > 0)
            vx, vy, Dv = vx[:, keep], vy[:, keep], Dv[:, keep]
            cv = np.stack([rgb[(slice(None),) + s][:, keep] for s in sl])              # [3 vertices, 3 channels, n]
            pieces.append(dict(id=ids[:-1, :-1][keep] + t + 1, box=boxes(ceil8(vx.min(0)), vx.max(0) // 8, ceil8(vy.min(0)), vy.max(0) // 8), v=(vx, vy), D=Dv,
                               c=cv))

    def scatter(visit):
        """visit(piece set, chunk of its pieces, index of the piece within the chunk, pixel, covers, nearness, wa, wb, wc, A)"""
        for ps in pieces:
            lo_x, hi_x, lo_y, hi_y = ps["box"]
            n = np.maximum(hi_x - lo_x + 1, 0) * np.maximum(hi_y - lo_y + 1, 0)
            for ch in _chunks(n):
                which, px, py = _pairs(lo_x[ch], hi_x[ch], lo_y[ch], hi_y[ch])
                if which.size == 0:
                    continue
                if "v" not in ps:
                    src = ps["src"][ch][which]
                    sx, sy = tx.ravel()[src], ty.ravel()[src]
                    covers = (sx - h <= 8 * px) & (8 * px < sx + h) & (sy - h <= 8 * py) & (8 * py < sy + h)
                    visit(ps, ch, which, py * W + px, covers, D.ravel()[src], None)
                else:
                    v = (ps["v"][0][:, ch][:, which], ps["v"][1][:, ch][:, which])
                    covers, wa, wb, wc, A = _barycentric(v, 8 * px, 8 * py)
                    Dv = ps["D"][:, ch][:, which]
                    near = (wa * Dv[0] + wb * Dv[1] + wc * Dv[2] + (A >> 1)) // A
                    visit(ps, ch, which, py * W + px, covers, near, (wa, wb, wc, A))

    # step 4 as one maximum: the nearness above the inverted piece id (below 3 * 2^28 < 2^30)
    best = np.full(H * W, -1, i64)
    cover, triangles = np.zeros(H * W, i64), np.zeros(H * W, i64)

    def offer(ps, ch, which, pix, covers, near, w):
        np.maximum.at(best, pix[covers], (near[covers] << 30) + ((1 << 30) - 1 - ps["id"][ch][which][covers]))
        if want_stats:
            np.add.at(cover, pix[covers], 1)
            if w is not None:
                np.add.at(triangles, pix[covers], 1)

    scatter(offer)
    near_out = np.where(best >= 0, best >> 30, -1)
    piece = np.where(best >= 0, (1 << 30) - 1 - (best & ((1 << 30) - 1)), -1)
    out = np.zeros((3, H * W), i64)
    ties = np.zeros(H * W, i64)

    def colours(ps, ch, which, pix, covers, near, w):
        won = covers & (ps["id"][ch][which] == piece[pix])
        if want_stats:
            np.add.at(ties, pix[covers & (near == near_out[pix])], 1)
        if not won.any():
            return
        if w is None:
            out[:, pix[won]] = rgb.reshape(3, -1)[:, ps["src"][ch][which][won]]
        else:
            wa, wb, wc, A = (a[won] for a in w)
            cv = ps["c"][:, :, ch][:, :, which][:, :, won]
            out[:, pix[won]] = (wa * cv[0] + wb * cv[1] + wc * cv[2] + (A >> 1)) // A

    scatter(colours)
    res = (near_out.reshape(H, W), out.reshape(3, H, W))
    if want_stats:
        res += (dict(piece=piece.reshape(H, W), cover=cover.reshape(H, W), triangles=triangles.reshape(H, W), ties=ties.reshape(H, W),
                     folded=folded, clamped=clamped),)
    return res


def fill_holes(near, colours, max_s8: int):
    """Step 5 for one image and one frame: near int64 [H, W] with -1 in the holes, colours int64 [3, H, W] -> (near, colours, holes bool,
    the direction each hole was filled from: 0 left, 1 right, 2 up, 3 down, -1 none or no hole)."""
    H, W = near.shape
    R = int(max_s8) // 4 + 1
    covered = near >= 0
    far = 4 * MAX_DIM
    yy, xx = np.broadcast_to(np.arange(H, dtype=i64)[:, None], (H, W)), np.broadcast_to(np.arange(W, dtype=i64)[None], (H, W))
    pick, pick_near, pick_y, pick_x = np.full((H, W), -1, i64), np.zeros((H, W), i64), np.zeros((H, W), i64), np.zeros((H, W), i64)
    for k, (axis, forward) in enumerate(((1, True), (1, False), (0, True), (0, False))):       # left, right, up, down
        idx = xx if axis == 1 else yy
        if forward:
            src = np.maximum.accumulate(np.where(covered, idx, -far), axis=axis)
            has = idx - src <= R
        else:
            src = np.flip(np.minimum.accumulate(np.flip(np.where(covered, idx, far), axis), axis=axis), axis)
            has = src - idx <= R
        src = np.clip(src, 0, (W if axis == 1 else H) - 1)
        sy, sx = (yy, src) if axis == 1 else (src, xx)
        value = near[sy, sx]
        take = has & ((pick < 0) | (value < pick_near))
        pick, pick_near, pick_y, pick_x = np.where(take, k, pick), np.where(take, value, pick_near), np.where(take, sy, pick_y), np.where(take, sx, pick_x)
    holes = ~covered
    some = pick >= 0
    filled = np.where(holes, np.where(some, pick_near, 0), near)
    taken = np.where(some[None], colours[:, pick_y, pick_x], 0)
    return filled, np.where(holes[None], taken, colours), holes, np.where(holes, pick, -1)


def check_table(table) -> np.ndarray:
    """The frame table as a checked contiguous int32 [V, 4] array: the ranges of the definition."""
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[1] != 4 or not 1 <= t.shape[0] <= MAX_FRAMES:
        raise ValueError(f"table: integers (gx, gy, gz, Z) for 1 .. {MAX_FRAMES} frames, got {t.dtype} {t.shape}")
    t = t.astype(i64)
    if (np.abs(t[:, :2]) > MAX_G).any() or (np.abs(t[:, 2]) > MAX_GZ).any() or (t[:, 3] < Z_MIN).any() or (t[:, 3] > Z_MAX).any():
        raise ValueError(f"table: |gx|, |gy| <= {MAX_G}, |gz| <= {MAX_GZ} and Z in {Z_MIN} .. {Z_MAX}, got {t.tolist()}")
    return np.ascontiguousarray(t.astype(np.int32))


def parallax_frames_table(image, pred, F, table, space: str = "depth", edge: int = 0, max_s8: int = MAX_S8, want_stats: bool = False):
    """A batch by the definition above from its integers.  image uint8 [B, 3, H, W] ([3, H, W]: one image); pred float [B, 1, H, W]
    ([B, H, W] with B images, [H, W] with one); F integers [B] or one; table integers [V, 4].  Returns (frames uint8 [B, V, 3, H, W], holes
    uint8 [B, V, H, W], near uint16 [B, V, H, W]), and with want_stats also a list [B][V] of the dicts of `warp_frame` with `filled_from`
    int64 [H, W] of `fill_holes` added."""
    _check_space(space)
    image, pred = _images_and_maps(image, pred)
    B, _, H, W = image.shape
    F = _warp_integers(F, B, edge, max_s8, MAX_S8)
    table = check_table(table)
    V = table.shape[0]
    _count_limit(B, V, H, W)
    frames, holes, near = np.empty((B, V, 3, H, W), np.uint8), np.empty((B, V, H, W), np.uint8), np.empty((B, V, H, W), np.uint16)
    stats = [[None] * V for _ in range(B)]
    for b in range(B):
        D, rgb = nearness(pred[b], space), image[b].astype(i64)
        for k, frame in enumerate(table.tolist()):
            res = warp_frame(D, rgb, int(F[b]), frame, int(edge), int(max_s8), want_stats)
            filled, colours, hole, direction = fill_holes(res[0], res[1], int(max_s8))
            frames[b, k], holes[b, k], near[b, k] = colours, hole, filled
            if want_stats:
                stats[b][k] = dict(res[2], filled_from=direction)
    return (frames, holes, near, stats) if want_stats else (frames, holes, near)


def parallax_frames(image, pred, path="orbit", frames: int = 16, amount: float = 16.0, push: float = 0.0, zoom: float = 1.0, pan: bool = False,
                    focus=None, focus_at=None, edge=EDGE_DEFAULT, overscan: bool = True, frame_range=None, space: str = "depth",
                    want_holes: bool = False, want_near: bool = False):
    """`parallax_frames_table` from the user's terms (module docstring).  Returns the frames uint8 [B, V, 3, H, W], and with want_holes /
    want_near a tuple with those planes after them."""
    _check_space(space)
    image, pred = _images_and_maps(image, pred)
    B, _, H, W = image.shape
    o = plan(B, H, W, path, frames, amount, push, zoom, pan, focus, focus_at, edge, overscan, frame_range)
    out, holes, near = parallax_frames_table(image, pred, focus_plane(pred, space, o), o["table"], space, o["edge"], o["max_s8"])
    return _with_planes(out, holes, near, want_holes, want_near)
