"""What the host routes of the post-processing ops (foreground, guided, tiled, geometry, lens_blur, stereo, parallax) share: the limit of an
image side, the two spaces a depth map is read in, the 16-bit quantisation rule and the parser of a `True or dict` pipeline argument; and,
for the three ops that render a photograph under one plane of its map (lens_blur, stereo, parallax), the 16-bit nearness, the parser of that
plane -- a value of the map or a pixel of it --, its integer F, how far a nearness can lie from it, and their shared input and range checks.
Limits whose reason belongs to one op (a window radius, a tile count, a stride) stay in that op's module."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import numpy as np

MAX_DIM = 16384                    # the longest image side an op takes (the C headers' *_MAX_DIM, each with its own reason)
SPACES = ("depth", "disparity")    # how a map in [0, 1] is read: far = 1 or near = 1
F_DEFAULT = 32768                  # the plane of stereo and parallax where none is given: the middle of the nearness scale
EDGE_DEFAULT = 0.04                # a convention: neighbours further apart than 4 % of the map's range are cut
i64 = np.int64


def is_int(v) -> bool:
    """A Python or numpy integer; a bool is not one."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def quantize16(pred) -> np.ndarray:
    """(uint16)(clamp(pred, 0, 1) * 65535.0f): a float32 product, truncated, NaN -> 0"""
    x = np.asarray(pred, dtype=np.float32)
    c = np.where(x > np.float32(0.0), np.where(x < np.float32(1.0), x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return (c * np.float32(65535.0)).astype(np.int64).astype(np.uint16)


def options_from(arg, defaults: Dict, name: str, check: Optional[Callable[[Dict], Dict]] = None) -> Dict:
    """The `name` argument of a pipeline entry -- True (the defaults) or a dict over the keys of `defaults`, an unknown key refused -- as
    the options `check` makes of the filled-in dict (ValueError outside the op's ranges)."""
    opts = dict(defaults)
    if arg is not True:
        if not isinstance(arg, dict) or any(k not in defaults for k in arg):
            raise ValueError(f"{name} is None, True or a dict with the keys {sorted(defaults)}, got {arg!r}")
        opts.update(arg)
    return opts if check is None else check(opts)


# ---- one plane of the map: lens_blur (focus), stereo (converge), parallax (focus) -----------------------------------------------------------------------
def _per_image(v, B: int, name: str, width: int = 0) -> np.ndarray:
    a = np.asarray(v, np.float64)
    shape = (B, width) if width else (B,)
    if a.ndim == len(shape) - 1:
        a = np.broadcast_to(a[None], (B,) + a.shape)
    if a.shape != shape or not np.isfinite(a).all():
        raise ValueError(f"{name}: finite, one value for every image or {list(shape)}, got {np.shape(v)}")
    return a


def nearness(pred, space: str) -> np.ndarray:
    """D int64 of pred float32 of any shape: Q = quantize16(pred) in disparity space, 65535 - Q in depth space, 0 for a NaN pixel."""
    pred = np.asarray(pred, np.float32)
    q = quantize16(pred).astype(i64)
    return np.where(np.isnan(pred), 0, q if space == "disparity" else 65535 - q)


def _check_space(space) -> None:
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")


def _plane(B: int, value, at, value_name: str, at_name: str, exactly_one: bool) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """The plane of a call in the user's terms, checked (ValueError outside the ranges) and spread over the B images: (`value_name`, a value
    of the map in [0, 1], as float32 [B] or None; `at_name`, a pixel (u, v), as int64 [B, 2] or None).  Exactly one of the two is given, or,
    for an op that has a default plane, at most one."""
    if value is not None and at is not None or (exactly_one and value is None and at is None):
        raise ValueError(f"{'exactly' if exactly_one else 'at most'} one of {value_name} (a value of the map) and {at_name} (a pixel (u, v)) is given")
    if value is not None:
        f = _per_image(value, B, value_name)
        if (f < 0.0).any() or (f > 1.0).any():
            raise ValueError(f"{value_name} is a value of the map in [0, 1], got {value!r}")
        return f.astype(np.float32), None
    if at is not None:
        p = _per_image(at, B, at_name, 2)
        if (p != np.floor(p)).any() or (p < 0).any() or (p >= MAX_DIM).any():
            raise ValueError(f"{at_name} is a pixel (u, v) of the image, got {at!r}")
        return None, p.astype(i64)
    return None, None


def _edge16(edge) -> int:
    """`edge`, a fraction of the map's range, as the integer floor(65535 * edge + 1/2)."""
    if isinstance(edge, bool) or np.ndim(edge) != 0 or not np.isfinite(float(edge)) or not 0.0 <= float(edge) <= 1.0:
        raise ValueError(f"edge is a fraction of the map's range in [0, 1], got {edge!r}")
    return int(np.floor(65535.0 * float(edge) + 0.5))


def _pixel_inside(at, at_name: str, H: int, W: int) -> None:
    """The pixels (u, v) int64 [B, 2] (or None) lie inside an H x W image."""
    if at is not None and ((at[:, 0] >= W).any() or (at[:, 1] >= H).any()):
        raise ValueError(f"{at_name} = (u, v) lies inside the {W} x {H} image, got {at.tolist()}")


def _plane_F(pred, space: str, value, at, default: Optional[int] = None) -> np.ndarray:
    """F int64 [B] of a plane of `_plane` and, for a pixel, the maps pred [B, H, W]; `default` for every image where neither is given."""
    B = pred.shape[0]
    if value is not None:
        return nearness(value, space)
    if at is not None:
        return nearness(pred[np.arange(B), at[:, 1], at[:, 0]], space)
    return np.full(B, default, i64)


def _plane_span(B: int, value, at, default: Optional[int] = None) -> int:
    """How far a nearness can lie from F where the host knows F, max(q, 65535 - q) over the batch (the same for both spaces: F is q or
    65535 - q); 65535 where the plane is a pixel, read on the device."""
    if at is not None:
        return 65535
    q = quantize16(value).astype(i64) if value is not None else np.full(B, default, i64)
    return int(np.maximum(q, 65535 - q).max())


def _images_and_maps(image, pred):
    image = np.asarray(image)
    image = image[None] if image.ndim == 3 else image
    if image.dtype != np.uint8 or image.ndim != 4 or image.shape[1] != 3:
        raise ValueError(f"image: uint8 [B, 3, H, W] or [3, H, W], got {image.dtype} {image.shape}")
    B, _, H, W = image.shape
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or B < 1:
        raise ValueError(f"image: sides in 1 .. {MAX_DIM}, got {image.shape}")
    pred = np.asarray(pred)
    if pred.dtype.kind != "f" or pred.size != B * H * W or tuple(pred.shape[-2:]) != (H, W):
        raise ValueError(f"pred: float {(B, 1, H, W)}, got {pred.dtype} {pred.shape}")
    return image, pred.reshape(B, H, W).astype(np.float32)


def _count_limit(B: int, V: int, H: int, W: int) -> None:
    if B * V * H * W >= 2 ** 31:
        raise ValueError(f"B * V * H * W < 2^31, got {(B, V, H, W)}")


def _warp_integers(F, B: int, edge, max_s8, max_s8_limit: int) -> np.ndarray:
    """The integers of a table entry of stereo or parallax checked: edge in 0 .. 65535, max_s8 in 0 .. `max_s8_limit`; F, one integer or
    [B], comes back as int64 [B] clipped to 0 .. 65535."""
    if not is_int(edge) or not 0 <= edge <= 65535 or not is_int(max_s8) or not 0 <= max_s8 <= max_s8_limit:
        raise ValueError(f"edge in 0 .. 65535 and max_s8 in 0 .. {max_s8_limit}, got {edge!r} and {max_s8!r}")
    F = np.asarray(F)
    if F.dtype.kind not in "iu" or F.shape not in ((), (B,)):
        raise ValueError(f"F: one integer or [{B}], got {F.dtype} {F.shape}")
    return np.clip(np.broadcast_to(F.astype(i64), (B,)), 0, 65535)


def _with_planes(out, holes, near, want_holes: bool, want_near: bool):
    """`out` alone, or a tuple of it and the planes that are wanted after it."""
    extra = ((holes,) if want_holes else ()) + ((near,) if want_near else ())
    return (out,) + extra if extra else out
