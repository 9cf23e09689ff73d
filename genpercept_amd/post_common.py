"""What the host routes of the post-processing ops (foreground, guided, tiled, geometry, lens_blur) share: the limit of an image side, the
two spaces a depth map is read in, the 16-bit quantisation rule and the parser of a `True or dict` pipeline argument.  Limits whose reason
belongs to one op (a window radius, a tile count, a stride) stay in that op's module."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np

MAX_DIM = 16384                    # the longest image side an op takes (the C headers' *_MAX_DIM, each with its own reason)
SPACES = ("depth", "disparity")    # how a map in [0, 1] is read: far = 1 or near = 1


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
