"""Relighting, the host route (numpy, no torch): a photograph under up to eight new directional lights and an ambient term, shaded by its
normal map -- diffuse and specular --, with screen-space cast shadows marched over its depth or disparity map and an optional per-pixel
weight, as "portrait lighting" does.  This file is the specification in executable form, vectorised over the pixels with a loop over the
lights and the steps of a march; csrc/relight.hip (gp_relight) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h, the normative text; the arithmetic once more in csrc/relight_math.h)
  Axes: x right, y down, z away from the camera (those of geometry.py).  A camera-facing normal has N_z < 0, a light in front of the scene
    L_z < 0.  The projection is orthographic, the view direction (0, 0, -1): a stated convention, an affine-invariant map has no camera.
  Per image: image uint8 [3, H, W]; normal float32 [3, H, W]; pred float32 [H, W], optional (no shadows without it); weight uint8 [H, W],
    optional.  Per call: encoded (values in [0, 1]) or raw (values in [-1, 1]); flip, a sign per axis; space; the tables of lens_blur.py;
    L + 1 rows of 20 integers (`ROW_FIELDS`): L light rows, 1 <= L <= 8, and the ambient row.
  1. N_k = 2 quantize16(v_k) - 65535 (encoded) or trunc(clamp(v_k, -1, 1) * 65535.0f) (raw), then the flips; m = floor(sqrt(N . N)), exact.
     A NaN channel or m < 256: N = (0, 0, -65535), m = 65535.
  2. Per light: cos12 = clamp(N . L // (4 m), 0, 4096); s = clamp(N . H // (4 m), 0, 4096), k times s = (s s + 2048) >> 12.  A light with
     cos12 = 0 contributes nothing.
  3. Shadow, where pred is given and not NaN at the pixel, the row has a reach and cos12 > 0: D = nearness(pred); for t = 1 .. reach,
     q_t = (x + ((t ux + 128) >> 8), y + ((t uy + 128) >> 8)) inside the image; e_t = D(q_t) - D(p) - bias - t rise; E = max(0, max e_t);
     dark = min(256, (E soft + 128) >> 8), with soft = 0: 256 iff E > 0; shade = (dark strength) >> 8; vis = 256 - shade.
  4. lin_k = to_lin[image_k]; G_k = amb_k + ((sum_j col_jk cos12_j vis_j) >> 16); S_k = (sum_j spc_jk s_j vis_j) >> 16;
     lin'_k = min(4095, ((lin_k G_k + 2048) >> 12) + min(S_k, 4095)); relit_k = from_lin[lin'_k];
     out_k = (w relit_k + (255 - w) image_k + 127) // 255, w = 255 without a weight; shadow = min(255, max_j shade_j).
  The image is taken as albedo times its own light, a convention: ambient 1.0 keeps it and the lights add to it.

The user's terms per light (`relight_lights`, `DEFAULT_LIGHT`), all float64 on the host, floor(x + 1/2) for every rounding:
  azimuth, elevation in degrees: L = (cos e cos a, -cos e sin a, -sin e) -- azimuth 0 lights from the right, 90 from above, 180 from the
    left; elevation 90 is the camera's own direction; the row holds floor(16384 L + 1/2) and, for H, the same of (L + (0, 0, -1)) / |.|.
  intensity, colour (three values in [0, 1]), specular: col_k = floor(256 intensity colour_k + 1/2), spc_k = floor(256 intensity specular
    colour_k + 1/2), at most 4096 each.  shininess = 2^k, k = 0 .. 7.
  shadows (False: reach = 0), reach in pixels along the longer axis of the step, 0 .. 64.  (ux, uy) = floor(256 (L_x, L_y) / max(|L_x|,
    |L_y|) + 1/2) from the row's integers L_x, L_y; a light with L_x = L_y = 0 has no step and no reach.
  softness, the part of the map's range over which a shadow grows to full: soft = 0 (hard) for 0, else clamp(floor(1 / softness + 1/2), 1,
    256).  strength in [0, 1]: floor(256 strength + 1/2).  bias in [0, 1], in units of the map: floor(65535 bias + 1/2).
Per call: ambient, one value or three, amb_k = floor(4096 ambient_k + 1/2); relief, the height in pixels of the map's full range:
  rise = min(65535, floor(max(0, tan e) * (sqrt(ux^2 + uy^2) / 256) * (65535 / relief) + 1/2)), in that order.
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np

from .lens_blur import check_tables, srgb_tables  # noqa: F401
from .post_common import MAX_DIM, SPACES, _check_space, _images_and_maps, is_int, nearness, options_from, quantize16

MAX_LIGHTS = 8
MAX_REACH = 64
UNIT = 16384
MAX_GAIN = 4096
MAX_AMB = 65536
MIN_LEN = 256
N_ONE = 65535
LIN_MAX = 4095
ROW_FIELDS = ("Lx", "Ly", "Lz", "Hx", "Hy", "Hz", "col_r", "col_g", "col_b", "spc_r", "spc_g", "spc_b", "k", "ux", "uy", "rise", "bias", "soft",
              "strength", "reach")
ROW = len(ROW_FIELDS)
LX, HX, COL, SPC, K, UX, UY, RISE, BIAS, SOFT, STRENGTH, REACH = 0, 3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19
DEFAULT_LIGHT = dict(azimuth=135.0, elevation=40.0, intensity=1.0, colour=(1.0, 1.0, 1.0), specular=0.0, shininess=16, shadows=True, reach=32,
                     softness=0.0, strength=1.0, bias=0.002)
DEFAULT_AMBIENT = 0.35
DEFAULT_RELIEF = 64.0
i64 = np.int64


# ---- the user's terms ---------------------------------------------------------------------------------------------------------------------------------
def _rnd(x: float) -> int:
    return int(math.floor(x + 0.5))


def _number(v, name: str, lo: float, hi: float) -> float:
    if isinstance(v, bool) or np.ndim(v) != 0 or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
            or not lo <= float(v) <= hi:
        raise ValueError(f"{name} is one number in [{lo:g}, {hi:g}], got {v!r}")
    return float(v)


def _colour(v, name: str, hi: float) -> np.ndarray:
    a = np.asarray(v)
    if a.dtype.kind not in "iuf" or a.shape not in ((), (3,)) or not np.isfinite(a.astype(np.float64)).all() or (a < 0).any() or (a > hi).any():
        raise ValueError(f"{name} is one value or three in [0, {hi:g}], got {v!r}")
    return np.broadcast_to(a.astype(np.float64), (3,))


def _check_light(o: Dict) -> Dict:
    """One light's terms checked (ValueError outside their ranges); the dict comes back with plain floats, ints and bools."""
    out = dict(azimuth=_number(o["azimuth"], "azimuth", -3600.0, 3600.0), elevation=_number(o["elevation"], "elevation", -90.0, 90.0),
               intensity=_number(o["intensity"], "intensity", 0.0, 16.0), colour=tuple(float(c) for c in _colour(o["colour"], "colour", 1.0)),
               specular=_number(o["specular"], "specular", 0.0, 16.0), softness=_number(o["softness"], "softness", 0.0, 1.0),
               strength=_number(o["strength"], "strength", 0.0, 1.0), bias=_number(o["bias"], "bias", 0.0, 1.0))
    if out["intensity"] * max(1.0, out["specular"]) > 16.0:
        raise ValueError(f"intensity and intensity * specular are gains of at most 16, got {o['intensity']!r} and {o['specular']!r}")
    if not is_int(o["shininess"]) or o["shininess"] not in tuple(1 << k for k in range(8)):
        raise ValueError(f"shininess is a power of two in 1 .. 128, got {o['shininess']!r}")
    if not isinstance(o["shadows"], (bool, np.bool_)):
        raise ValueError(f"shadows is True or False, got {o['shadows']!r}")
    if not is_int(o["reach"]) or not 0 <= o["reach"] <= MAX_REACH:
        raise ValueError(f"reach is a whole number of pixels in 0 .. {MAX_REACH}, got {o['reach']!r}")
    out.update(shininess=int(o["shininess"]), shadows=bool(o["shadows"]), reach=int(o["reach"]))
    return out


def relight_options(lights=True) -> List[Dict]:
    """The `lights` argument of the pipeline's entries -- True (`DEFAULT_LIGHT`), a dict over its keys or a sequence of 1 .. 8 of either --
    as a list of checked, filled-in dicts, one per light.  ValueError for an unknown key or a term outside its range."""
    seq = list(lights) if isinstance(lights, (list, tuple)) else [lights]
    if not 1 <= len(seq) <= MAX_LIGHTS:
        raise ValueError(f"lights: 1 .. {MAX_LIGHTS} lights, got {len(seq)}")
    return [options_from(one, DEFAULT_LIGHT, "a light", _check_light) for one in seq]


def light_row(o: Dict, relief: float) -> List[int]:
    """The 20 integers of one light (module docstring) from its checked terms."""
    a, e = math.radians(o["azimuth"]), math.radians(o["elevation"])
    L = (math.cos(e) * math.cos(a), -(math.cos(e) * math.sin(a)), -math.sin(e))
    Li = [_rnd(UNIT * v) for v in L]
    h = (L[0], L[1], L[2] - 1.0)
    n = math.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
    Hi = [_rnd(UNIT * (v / n)) for v in h] if n > 0.0 else [0, 0, 0]   # (n = 0: the light shines from behind, straight at the camera)
    col = [_rnd(256.0 * o["intensity"] * c) for c in o["colour"]]
    spc = [_rnd(256.0 * o["intensity"] * o["specular"] * c) for c in o["colour"]]
    k = int(o["shininess"]).bit_length() - 1
    big = max(abs(Li[0]), abs(Li[1]))
    ux = uy = rise = reach = 0
    if big > 0 and o["shadows"] and o["reach"] > 0:
        ux, uy, reach = _rnd(256.0 * Li[0] / big), _rnd(256.0 * Li[1] / big), o["reach"]
        rise = min(65535, _rnd(max(0.0, math.tan(e)) * (math.sqrt(float(ux * ux + uy * uy)) / 256.0) * (65535.0 / relief)))
    soft = 0 if o["softness"] == 0.0 else min(256, max(1, _rnd(1.0 / o["softness"])))
    return Li + Hi + col + spc + [k, ux, uy, rise, _rnd(65535.0 * o["bias"]), soft, _rnd(256.0 * o["strength"]), reach]


def relight_lights(lights=True, ambient=DEFAULT_AMBIENT, relief=DEFAULT_RELIEF) -> np.ndarray:
    """The table of a call, int32 [L + 1, 20], from the user's terms: `lights` as `relight_options` takes it, ambient one value or three in
    [0, 16], relief > 0 the height in pixels of the map's full range."""
    opts = relight_options(lights)
    amb = _colour(ambient, "ambient", 16.0)
    relief = _number(relief, "relief", 1e-3, 1e9)
    rows = [light_row(o, relief) for o in opts] + [[_rnd(4096.0 * float(v)) for v in amb] + [0] * (ROW - 3)]
    return check_rows(np.array(rows, np.int32))


def check_rows(rows) -> np.ndarray:
    """The table as a checked contiguous int32 [L + 1, 20] array: every value inside the range gp_relight takes."""
    r = np.asarray(rows)
    if r.dtype.kind not in "iu" or r.ndim != 2 or r.shape[1] != ROW or not 2 <= r.shape[0] <= MAX_LIGHTS + 1:
        raise ValueError(f"rows: integers [L + 1, {ROW}] with 1 <= L <= {MAX_LIGHTS}, got {r.dtype} {r.shape}")
    r = r.astype(i64)
    li, amb = r[:-1], r[-1, :3]
    lo = np.array([-UNIT] * 6 + [0] * 6 + [0, -256, -256, 0, 0, 0, 0, 0], i64)
    hi = np.array([UNIT] * 6 + [MAX_GAIN] * 6 + [7, 256, 256, 65535, 65535, 256, 256, MAX_REACH], i64)
    stepless = (li[:, REACH] > 0) & (np.maximum(np.abs(li[:, UX]), np.abs(li[:, UY])) != 256)
    if (li < lo[None]).any() or (li > hi[None]).any() or stepless.any() or (amb < 0).any() or (amb > MAX_AMB).any():
        raise ValueError(f"rows: a light row {ROW_FIELDS} or the ambient row outside its range, got {r.tolist()}")
    return np.ascontiguousarray(r.astype(np.int32))


def check_flip(flip) -> int:
    """flip, three booleans (a sign per axis), as the 3 bits gp_relight takes."""
    f = np.asarray(flip)
    if f.shape != (3,) or f.dtype.kind != "b":
        raise ValueError(f"flip is three booleans, a sign per axis, got {flip!r}")
    return int(f[0]) | int(f[1]) << 1 | int(f[2]) << 2


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------
def isqrt(s) -> np.ndarray:
    """floor(sqrt(s)) of int64 s < 2^53, exact: the float64 root set right by the integer comparison."""
    s = np.asarray(s, i64)
    r = np.floor(np.sqrt(s.astype(np.float64))).astype(i64)
    r = r - (r * r > s)
    return r + ((r + 1) * (r + 1) <= s)


def integer_normals(normal, encoded: bool, flip: int):
    """Step 1 for one image: normal float32 [3, H, W] -> (N int64 [3, H, W], m int64 [H, W])."""
    v = np.asarray(normal, np.float32)
    if encoded:
        N = 2 * quantize16(v).astype(i64) - N_ONE
    else:
        c = np.where(v > np.float32(-1.0), np.where(v < np.float32(1.0), v, np.float32(1.0)), np.float32(-1.0)).astype(np.float32)
        N = np.where(np.isnan(v), 0, np.trunc(np.nan_to_num(c * np.float32(65535.0)))).astype(i64)
    for k in range(3):
        if flip >> k & 1:
            N[k] = -N[k]
    m = isqrt((N * N).sum(0))
    bad = np.isnan(v).any(0) | (m < MIN_LEN)
    N = np.where(bad[None], np.array([0, 0, -N_ONE], i64)[:, None, None], N)
    return N, np.where(bad, N_ONE, m)


def ratio12(N, m, vec) -> np.ndarray:
    """Step 2: clamp(N . vec // (4 m), 0, 4096)."""
    d = N[0] * int(vec[0]) + N[1] * int(vec[1]) + N[2] * int(vec[2])
    return np.clip(d // (4 * m), 0, 4096)


def march(D, row) -> np.ndarray:
    """Step 3 for one image and light: E int64 [H, W] of the nearness D int64 [H, W], one pass per step."""
    H, W = D.shape
    reach, ux, uy, rise, bias = (int(row[k]) for k in (REACH, UX, UY, RISE, BIAS))
    E = np.zeros((H, W), i64)
    if reach == 0:
        return E
    Dp = np.zeros((H + 2 * reach, W + 2 * reach), i64)   # (outside the image D = 0, which exceeds no floor: such samples do not exist)
    Dp[reach:reach + H, reach:reach + W] = D
    for t in range(1, reach + 1):
        dx, dy = (t * ux + 128) >> 8, (t * uy + 128) >> 8
        E = np.maximum(E, Dp[reach + dy:reach + dy + H, reach + dx:reach + dx + W] - D - bias - t * rise)
    return E


def shade_of(E, row) -> np.ndarray:
    soft, strength = int(row[SOFT]), int(row[STRENGTH])
    dark = np.minimum(256, (E * soft + 128) >> 8) if soft else np.where(E > 0, 256, 0)
    return (dark * strength) >> 8


def relight_rows(image, normal, pred=None, weight=None, rows=None, encoded: bool = True, flip=(False, False, False), space: str = "depth",
                 tables=None, want_shadow: bool = False):
    """A batch by the definition above from the integer table.  image uint8 [B, 3, H, W] ([3, H, W]: one image); normal float [B, 3, H, W];
    pred float [B, 1, H, W] ([B, H, W] too) or None; weight uint8 [B, H, W] or None; rows integers [L + 1, 20]; tables (to_lin, from_lin) or
    None (`srgb_tables`).  Returns out uint8 [B, 3, H, W], and with want_shadow (out, shadow) with shadow uint8 [B, H, W]."""
    _check_space(space)
    image = np.asarray(image)
    image = image[None] if image.ndim == 3 else image
    normal = np.asarray(normal)
    normal = normal[None] if normal.ndim == 3 else normal
    if image.dtype != np.uint8 or image.ndim != 4 or image.shape[1] != 3:
        raise ValueError(f"image: uint8 [B, 3, H, W] or [3, H, W], got {image.dtype} {image.shape}")
    B, _, H, W = image.shape
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or B < 1 or B * H * W >= 2 ** 31:
        raise ValueError(f"image: sides in 1 .. {MAX_DIM}, B * H * W < 2^31, got {image.shape}")
    if normal.dtype.kind != "f" or normal.shape != image.shape:
        raise ValueError(f"normal: float {image.shape}, got {normal.dtype} {normal.shape}")
    normal = normal.astype(np.float32)
    if pred is not None:
        image, pred = _images_and_maps(image, pred)
    if weight is not None:
        weight = np.asarray(weight)
        weight = weight[None] if weight.ndim == 2 else weight
        if weight.shape != (B, H, W) or weight.dtype != np.uint8:
            raise ValueError(f"weight: uint8 {(B, H, W)}, got {weight.dtype} {weight.shape}")
    rows, bits = check_rows(rows).astype(i64), check_flip(flip)
    to_lin, from_lin = check_tables(tables)
    lights, amb = rows[:-1], rows[-1]
    out, shadow = np.empty((B, 3, H, W), np.uint8), np.zeros((B, H, W), np.uint8)
    for b in range(B):
        N, m = integer_normals(normal[b], bool(encoded), bits)
        G, S, worst = np.zeros((3, H, W), i64), np.zeros((3, H, W), i64), np.zeros((H, W), i64)
        D = nearness(pred[b], space) if pred is not None else None
        for row in lights:
            cos12 = ratio12(N, m, row[LX:LX + 3])
            s = ratio12(N, m, row[HX:HX + 3])
            for _ in range(int(row[K])):
                s = (s * s + 2048) >> 12
            shade = np.zeros((H, W), i64)
            if D is not None:
                shade = np.where(np.isnan(pred[b]) | (cos12 == 0), 0, shade_of(march(D, row), row))
            vis = np.where(cos12 > 0, 256 - shade, 0)       # (a light with cos12 = 0 contributes nothing)
            G += row[COL:COL + 3, None, None] * (cos12 * vis)[None]
            S += row[SPC:SPC + 3, None, None] * (s * vis)[None]
            worst = np.maximum(worst, shade)
        lin = to_lin[image[b]].astype(i64)
        new = np.minimum(LIN_MAX, ((lin * (amb[:3, None, None] + (G >> 16)) + 2048) >> 12) + np.minimum(S >> 16, LIN_MAX))
        relit = from_lin[new].astype(i64)
        w = weight[b].astype(i64)[None] if weight is not None else 255
        out[b] = (w * relit + (255 - w) * image[b].astype(i64) + 127) // 255
        shadow[b] = np.minimum(255, worst)
    return (out, shadow) if want_shadow else out


def relight(image, normal, pred=None, weight=None, lights=True, ambient=DEFAULT_AMBIENT, relief=DEFAULT_RELIEF, encoded: bool = True,
            flip=(False, False, False), space: str = "depth", tables=None, want_shadow: bool = False):
    """`relight_rows` from the user's terms (module docstring): lights True, a dict or a sequence of up to 8 dicts over `DEFAULT_LIGHT`."""
    return relight_rows(image, normal, pred, weight, relight_lights(lights, ambient, relief), encoded, flip, space, tables, want_shadow)
