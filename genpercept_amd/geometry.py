"""Point maps, surface normals and point clouds from a depth prediction, the host route (numpy, no torch): the map is unprojected through a
pinhole camera, every pixel gets the normal of a plane fitted to its neighbours that lie on the same surface, the "flying pixels" between
foreground and background are dropped, and what is left is compacted into a point cloud.  This file is the specification in executable
form; csrc/depth_geometry.hip (gp_depth_geometry) gives the same bits on the device.

Definition (restated in include/genpercept_hip.h; the per-pixel arithmetic once more in csrc/depth_geometry_math.h)
  Per image: pred float32 [1, H, W]; mask uint8 [H, W], optional, non-zero means usable; image uint8 [3, H, W], optional; the camera, eight
    float64 values s, t, fx, fy, cx, cy, z_min, z_max (all finite, fx, fy > 0, 0 < z_min < z_max).  Per call: space "depth" or "disparity";
    radius r in 1 .. 8 (default 2); tau in (0, 1] (0.05); min_count in 3 .. (2 r + 1)^2 (2 r + 1); min_cos in [0, 1) (cos 85 degrees, computed
    in float64); stride in 1 .. 64 (1).  1 <= H, W <= 16384 and B * H * W < 2^31.  The camera is OpenCV's: x right, y down, z forward, and pixel
    (u, v) has its centre at integer (u, v).  Everything after the quantisation is float64, the operations + - * / sqrt in the order written,
    no fused multiply-add.
  1. Quantise: Q = quantize16(pred) = (uint16)(clamp(pred, 0, 1) * 65535.0f), the 16-bit rule of gp_postprocess.  lin = s * (Q / 65535) + t;
     z = lin for depth, 1 / lin for disparity.  A pixel is valid iff pred is not NaN, the mask is not 0, z is finite and z_min <= z <= z_max.
     w = 1 / z.
  2. Point map: X = ((u - cx) / fx) * z, Y = ((v - cy) / fy) * z, Z = z, each rounded once to float32; NaN for an invalid pixel.
  3. Edge-aware plane fit in inverse depth (a plane n . P = d seen by a pinhole camera has inverse depth affine in the pixel coordinates, so
     the fit is linear).  The members of a valid pixel i are the valid pixels j of its (2 r + 1)^2 window, clipped to the image, with
     |z_j - z_i| <= tau * z_i.  In row-major order, with du = u_j - u_i and dv = v_j - v_i: the integers n, Su, Sv, Suu, Suv, Svv (exact) and
     the float64 sums Sw, Suw = sum du * w, Svw = sum dv * w, each from +0.0 with one product and one add per member.  The symmetric system
     [[Suu, Suv, Su], [., Svv, Sv], [., ., n]] (a, b, c) = (Suw, Svw, Sw) is solved by cofactors in the order of the guided filter's solve:
       c00 = s11 s22 - s12 s12;  c01 = s02 s12 - s01 s22;  c02 = s01 s12 - s02 s11;  c11 = s00 s22 - s02 s02;  c12 = s01 s02 - s00 s12
       c22 = s00 s11 - s01 s01;  det = (s00 c00 + s01 c01) + s02 c02       (exact integers below 2^53 for r <= 8)
       a = ((c00 Suw + c01 Svw) + c02 Sw) / det;  b = ((c01 Suw + c11 Svw) + c12 Sw) / det;  c = ((c02 Suw + c12 Svw) + c22 Sw) / det
     The fit is valid iff n >= min_count and det > 0.  m = (a * fx, b * fy, (c + a * (cx - u_i)) + b * (cy - v_i)).
  4. Normal: N_k = -m_k / sqrt((m0^2 + m1^2) + m2^2), facing the camera, rounded once to float32; (0, 0, 0) where the fit is invalid or the norm
     is 0 or not finite.
  5. Keep (the flying-pixel filter): valid, the fit valid, and with the view ray p = ((u - cx) / fx, (v - cy) / fy, 1) and
     mp = (m0 p0 + m1 p1) + m2:  mp * mp >= ((min_cos * min_cos) * ((m0^2 + m1^2) + m2^2)) * ((p0^2 + p1^2) + 1)  and  mp > 0.
  6. Compaction: the kept pixels with u % stride == 0 and v % stride == 0 in row-major order, image after image: points float32 [n, 3],
     point_normals float32 [n, 3], point_rgb uint8 [n, 3] (all 255 without an image), point_index int32 [n] = v * W + u, offsets int64 [B + 1].

The default camera (`default_camera`) is a VIEWING CONVENTION, not a measurement: `intrinsics_from_fov` at 55 degrees with s = 1, t = 1,
z_min = 1e-3, z_max = 1e6, which puts z in [1, 2].  An affine-invariant map carries no metric scale until the caller supplies s and t.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

from .post_common import MAX_DIM, SPACES, is_int, options_from, quantize16  # noqa: F401

MAX_R = 8
MAX_STRIDE = 64
DEFAULTS = dict(radius=2, tau=0.05, min_count=None, min_cos=None, stride=1)
DEFAULT_MIN_COS = math.cos(math.radians(85.0))
CAMERA_FIELDS = ("s", "t", "fx", "fy", "cx", "cy", "z_min", "z_max")
f32, f64 = np.float32, np.float64


def check_options(radius=2, tau=0.05, min_count=None, min_cos=None, stride=1) -> Tuple[int, float, int, float, int]:
    """The ranges of the definition (ValueError outside them), with the defaults filled in: (radius, tau, min_count, min_cos, stride)."""
    if not is_int(radius) or not 1 <= radius <= MAX_R:
        raise ValueError(f"radius is an integer in 1 .. {MAX_R}, got {radius!r}")
    tau = float(tau)
    if not (0.0 < tau <= 1.0):
        raise ValueError(f"tau is in (0, 1], got {tau}")
    if min_count is None:
        min_count = 2 * radius + 1
    if not is_int(min_count) or not 3 <= min_count <= (2 * radius + 1) ** 2:
        raise ValueError(f"min_count is an integer in 3 .. (2 r + 1)^2 = {(2 * radius + 1) ** 2}, got {min_count!r}")
    min_cos = DEFAULT_MIN_COS if min_cos is None else float(min_cos)
    if not (0.0 <= min_cos < 1.0):
        raise ValueError(f"min_cos is in [0, 1), got {min_cos}")
    if not is_int(stride) or not 1 <= stride <= MAX_STRIDE:
        raise ValueError(f"stride is an integer in 1 .. {MAX_STRIDE}, got {stride!r}")
    return int(radius), tau, int(min_count), min_cos, int(stride)


def pointcloud_options(pointcloud) -> Dict:
    """The `pointcloud` argument of the pipeline entries -- True or a dict with the keys radius, tau, min_count, min_cos, stride -- as the
    checked options of `depth_geometry`."""
    return options_from(pointcloud, DEFAULTS, "pointcloud", lambda o: dict(zip(DEFAULTS, check_options(**o))))


def intrinsics_from_fov(H: int, W: int, fov_deg: float = 55.0) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of a pinhole camera with the horizontal field of view fov_deg and its principal point at the image centre:
    fx = fy = (W / 2) / tan(fov / 2), cx = (W - 1) / 2, cy = (H - 1) / 2."""
    if not (is_int(H) and is_int(W)) or H < 1 or W < 1 or not 0.0 < float(fov_deg) < 180.0:
        raise ValueError(f"sizes are positive integers and the field of view is in (0, 180) degrees, got {H!r}, {W!r}, {fov_deg!r}")
    f = (W / 2.0) / math.tan(math.radians(float(fov_deg)) / 2.0)
    return f, f, (W - 1) / 2.0, (H - 1) / 2.0


def default_camera(H: int, W: int, fov_deg: float = 55.0) -> np.ndarray:
    """The viewing convention of the module docstring as a camera, float64 [8]: s = 1, t = 1, `intrinsics_from_fov`, z_min = 1e-3, z_max = 1e6."""
    return np.array((1.0, 1.0) + intrinsics_from_fov(H, W, fov_deg) + (1e-3, 1e6), f64)


def check_cameras(cameras, B: int, H: int, W: int) -> np.ndarray:
    """cameras (None: the default camera; [8] for every image; [B, 8]) as a checked contiguous float64 [B, 8] array."""
    if cameras is None:
        cameras = default_camera(H, W)
    cams = np.asarray(cameras, f64)
    if cams.ndim == 1:
        cams = np.broadcast_to(cams[None], (B,) + cams.shape)
    if cams.shape != (B, 8):
        raise ValueError(f"cameras: eight values {CAMERA_FIELDS} per image, [8] or [{B}, 8], got {cams.shape}")
    ok = np.isfinite(cams).all(1) & (cams[:, 2] > 0) & (cams[:, 3] > 0) & (cams[:, 6] > 0) & (cams[:, 6] < cams[:, 7])
    if not ok.all():
        raise ValueError(f"cameras: finite values with fx, fy > 0 and 0 < z_min < z_max, got {cams[~ok][0].tolist()}")
    return np.ascontiguousarray(cams)


def depth_from_prediction(pred, mask, cam, space: str) -> np.ndarray:
    """Step 1 for one image: pred float32 [H, W], mask [H, W] or None -> z float64 [H, W], NaN where the pixel is invalid."""
    s, t, _, _, _, _, z_min, z_max = (f64(v) for v in cam)
    with np.errstate(all="ignore"):
        lin = s * (quantize16(pred).astype(f64) / f64(65535.0)) + t
        z = f64(1.0) / lin if space == "disparity" else lin
        valid = ~np.isnan(pred) & np.isfinite(z) & (z_min <= z) & (z <= z_max)
    if mask is not None:
        valid &= np.asarray(mask) != 0
    return np.where(valid, z, f64(np.nan))


def window_sums(z: np.ndarray, r: int, tau: float):
    """Step 3's sums for every pixel of z float64 [H, W] (NaN: invalid): (ints int64 [6, H, W] = n, Su, Sv, Suu, Suv, Svv; sums float64
    [3, H, W] = Sw, Suw, Svw).  The offsets are visited in row-major order, so every pixel's members are."""
    H, W = z.shape
    zp = np.full((H + 2 * r, W + 2 * r), np.nan, f64)
    zp[r:r + H, r:r + W] = z
    ints, sums = np.zeros((6, H, W), np.int64), np.zeros((3, H, W), f64)
    with np.errstate(all="ignore"):
        wp = f64(1.0) / zp
        lim = f64(tau) * z
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                zj, wj = zp[r + dv:r + dv + H, r + du:r + du + W], wp[r + dv:r + dv + H, r + du:r + du + W]
                member = np.abs(zj - z) <= lim          # (False for a NaN on either side)
                k = member.astype(np.int64)
                for j, c in enumerate((1, du, dv, du * du, du * dv, dv * dv)):
                    if c:
                        ints[j] += c * k
                sums[0] = np.where(member, sums[0] + wj, sums[0])
                sums[1] = np.where(member, sums[1] + f64(du) * wj, sums[1])
                sums[2] = np.where(member, sums[2] + f64(dv) * wj, sums[2])
    return ints, sums


def solve(ints: np.ndarray, sums: np.ndarray):
    """(a, b, c, det), float64 [H, W] each, from the sums in the order of the definition."""
    n, su, sv, suu, suv, svv = (ints[k].astype(f64) for k in range(6))
    sw, suw, svw = sums
    s00, s01, s02, s11, s12, s22 = suu, suv, su, svv, sv, n
    with np.errstate(all="ignore"):
        c00 = s11 * s22 - s12 * s12
        c01 = s02 * s12 - s01 * s22
        c02 = s01 * s12 - s02 * s11
        c11 = s00 * s22 - s02 * s02
        c12 = s01 * s02 - s00 * s12
        c22 = s00 * s11 - s01 * s01
        det = (s00 * c00 + s01 * c01) + s02 * c02
        a = ((c00 * suw + c01 * svw) + c02 * sw) / det
        b = ((c01 * suw + c11 * svw) + c12 * sw) / det
        c = ((c02 * suw + c12 * svw) + c22 * sw) / det
    return a, b, c, det


def geometry_from_depth(z, cam, radius=2, tau=0.05, min_count=None, min_cos=None, raw: bool = False):
    """Steps 2 to 5 for one image on float64 z [H, W] directly (NaN, or a value outside [z_min, z_max]: invalid) -- the definition without its
    quantisation.  Returns (xyz float32 [3, H, W], normal float32 [3, H, W], keep bool [H, W]) and, with raw, a dict of what stands before the
    rounding as a fourth value: n int64 [H, W] (the members), det and fit [H, W], m float64 [3, H, W], normal64 float64 [3, H, W]."""
    radius, tau, min_count, min_cos, _ = check_options(radius, tau, min_count, min_cos, 1)
    cam = check_cameras(cam, 1, *np.shape(z))[0]
    _, _, fx, fy, cx, cy, z_min, z_max = (f64(v) for v in cam)
    z = np.asarray(z, f64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(z) & (z_min <= z) & (z <= z_max)
    z = np.where(valid, z, f64(np.nan))
    H, W = z.shape
    u, v = np.arange(W, dtype=f64)[None, :], np.arange(H, dtype=f64)[:, None]
    ints, sums = window_sums(z, radius, tau)
    a, b, c, det = solve(ints, sums)
    with np.errstate(all="ignore"):
        p0 = np.broadcast_to((u - cx) / fx, (H, W))
        p1 = np.broadcast_to((v - cy) / fy, (H, W))
        xyz = np.where(valid, np.stack([p0 * z, p1 * z, z]), f64(np.nan)).astype(f32)
        fit = valid & (ints[0] >= min_count) & (det > 0.0)
        m0, m1, m2 = a * fx, b * fy, (c + a * (cx - u)) + b * (cy - v)
        mm = (m0 * m0 + m1 * m1) + m2 * m2
        length = np.sqrt(mm)
        ok = fit & (length > 0.0) & np.isfinite(length)
        normal64 = np.where(ok, np.stack([-m0 / length, -m1 / length, -m2 / length]), f64(0.0))
        mp = (m0 * p0 + m1 * p1) + m2
        pp = (p0 * p0 + p1 * p1) + f64(1.0)
        keep = fit & (mp * mp >= ((f64(min_cos) * f64(min_cos)) * mm) * pp) & (mp > 0.0)
    out = (np.ascontiguousarray(xyz), np.ascontiguousarray(normal64.astype(f32)), keep)
    return out + (dict(n=ints[0], det=det, fit=fit, m=np.stack([m0, m1, m2]), normal64=normal64),) if raw else out


def compact(xyz, normal, keep, image, stride: int):
    """Step 6 for one image: (points [n, 3], point_normals [n, 3], point_rgb uint8 [n, 3], point_index int32 [n])."""
    H, W = keep.shape
    sel = np.zeros((H, W), bool)
    sel[::stride, ::stride] = keep[::stride, ::stride]
    idx = np.flatnonzero(sel)
    rgb = np.full((len(idx), 3), 255, np.uint8) if image is None else np.ascontiguousarray(np.asarray(image).reshape(3, H * W)[:, idx].T)
    return (np.ascontiguousarray(xyz.reshape(3, H * W)[:, idx].T), np.ascontiguousarray(normal.reshape(3, H * W)[:, idx].T), rgb, idx.astype(np.int32))


def depth_geometry(pred, cameras=None, image=None, mask=None, space: str = "depth", radius=2, tau=0.05, min_count=None, min_cos=None, stride=1) -> Dict:
    """A batch by the definition above.  pred float [B, 1, H, W] ([1, H, W] and [H, W]: one image); cameras None (`default_camera`), [8] or
    [B, 8]; image uint8 [B, 3, H, W] or None; mask [B, H, W] or None.  Returns a dict: xyz float32 [B, 3, H, W], normal float32 [B, 3, H, W],
    keep uint8 [B, H, W], points float32 [n, 3], point_normals float32 [n, 3], point_rgb uint8 [n, 3], point_index int32 [n], offsets int64
    [B + 1] (image k owns the points offsets[k] .. offsets[k + 1])."""
    radius, tau, min_count, min_cos, stride = check_options(radius, tau, min_count, min_cos, stride)
    if space not in SPACES:
        raise ValueError(f"space is one of {SPACES}, got {space!r}")
    pred = np.asarray(pred)
    if pred.dtype.kind != "f" or pred.ndim not in (2, 3, 4):
        raise ValueError(f"pred: float [B, 1, H, W], [1, H, W] or [H, W], got {pred.dtype} {pred.shape}")
    pred = pred.reshape((1,) * (4 - pred.ndim) + pred.shape).astype(f32)
    B, C, H, W = pred.shape
    if C != 1 or not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM) or B < 1 or B * H * W >= 2 ** 31:
        raise ValueError(f"pred: one channel, sides in 1 .. {MAX_DIM}, B * H * W < 2^31, got {pred.shape}")
    cams = check_cameras(cameras, B, H, W)
    if image is not None:
        image = np.asarray(image)
        image = image[None] if image.ndim == 3 else image
        if image.dtype != np.uint8 or image.shape != (B, 3, H, W):
            raise ValueError(f"image: uint8 {(B, 3, H, W)}, got {image.dtype} {image.shape}")
    if mask is not None:
        mask = np.asarray(mask)
        mask = mask[None] if mask.ndim == 2 else mask
        if mask.shape != (B, H, W) or mask.dtype.kind not in "biu":
            raise ValueError(f"mask: integers or booleans {(B, H, W)}, got {mask.dtype} {mask.shape}")
    out = dict(xyz=np.empty((B, 3, H, W), f32), normal=np.empty((B, 3, H, W), f32), keep=np.empty((B, H, W), np.uint8))
    parts, offsets = [], [0]
    for k in range(B):
        z = depth_from_prediction(pred[k, 0], None if mask is None else mask[k], cams[k], space)
        xyz, normal, keep = geometry_from_depth(z, cams[k], radius, tau, min_count, min_cos)
        out["xyz"][k], out["normal"][k], out["keep"][k] = xyz, normal, keep
        parts.append(compact(xyz, normal, keep, None if image is None else image[k], stride))
        offsets.append(offsets[-1] + len(parts[-1][3]))
    for j, name in enumerate(("points", "point_normals", "point_rgb", "point_index")):
        out[name] = np.concatenate([p[j] for p in parts])
    out["offsets"] = np.array(offsets, np.int64)
    return out


PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(path: str, points, normals, rgb) -> None:
    """A point cloud as a binary little-endian PLY file: per vertex x y z nx ny nz (float) and red green blue (uchar), 27 bytes."""
    points, normals, rgb = np.asarray(points), np.asarray(normals), np.asarray(rgb)
    n = len(points)
    if points.shape != (n, 3) or normals.shape != (n, 3) or rgb.shape != (n, 3) or rgb.dtype != np.uint8:
        raise ValueError(f"points and normals float [n, 3] and rgb uint8 [n, 3], got {points.shape}, {normals.shape}, {rgb.dtype} {rgb.shape}")
    rec = np.empty(n, PLY_DTYPE)
    for j, k in enumerate("xyz"):
        rec[k], rec["n" + k] = points[:, j], normals[:, j]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n"
    header += "".join(f"property float {k}\n" for k in ("x", "y", "z", "nx", "ny", "nz"))
    header += "".join(f"property uchar {k}\n" for k in ("red", "green", "blue")) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + rec.tobytes())
