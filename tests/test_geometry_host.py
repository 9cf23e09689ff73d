"""Point maps, normals and point clouds from depth (gp_depth_geometry), the host half: genpercept_amd/geometry.py (vectorised numpy) bit-equal
to a plain scalar loop implementation written here from the definition; tests/geometry_check.cpp, a stand-alone CPU program over the kernels'
own arithmetic (csrc/depth_geometry_math.h, contraction off, under AddressSanitizer and UBSan), bit-equal to the host route; what the
definition is for -- an exact plane gives its normal, a quantised plane gives it better as the window grows, a depth step does not tilt the
normals beside it, the pixels of a ramp between two surfaces are dropped; the compaction and the PLY writer; the header, the two libraries
and the ctypes table carry the new entries; their argument checks (they come before the first HIP call, so they run without a GPU)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs, q16, same_bits  # noqa: E402,F401

NAMES = ("gp_depth_geometry_workspace", "gp_depth_geometry")
f32, f64 = np.float32, np.float64
# H, W, r
CASES = [(9, 13, 1), (17, 11, 2), (12, 12, 8), (5, 23, 4)]
PLANES = ("xyz", "normal", "keep")
POINTS = ("points", "point_normals", "point_rgb", "point_index")


def random_case(rng, h, w):
    """(pred float32 [h, w], mask uint8 [h, w], image uint8 [3, h, w], camera float64 [8]): a smooth map with noise and a depth step down a
    column, NaNs, values outside [0, 1], and a camera whose z_max leaves the map's far end (depth) or near end (disparity) invalid; the
    principal point is off-centre and fx != fy."""
    yy, xx = np.mgrid[0:h, 0:w]
    pred = (0.45 + 0.25 * np.sin(yy / 4.0) * np.cos(xx / 5.0) + 0.004 * rng.randn(h, w)).astype(f32)
    pred[:, w // 2:] += f32(0.3)
    for _ in range(3):
        pred[rng.randint(h), rng.randint(w)] = np.nan
    pred[rng.randint(h), rng.randint(w)], pred[rng.randint(h), rng.randint(w)] = 1.5, -0.25
    mask = (rng.rand(h, w) > 0.1).astype(np.uint8) * rng.randint(1, 256, (h, w)).astype(np.uint8)
    image = rng.randint(0, 256, (3, h, w)).astype(np.uint8)
    cam = np.array([1.7, 0.4, 21.5 + rng.rand(), 19.25 + rng.rand(), 0.45 * w + rng.rand(), 0.55 * h - rng.rand(), 0.5, 1.9], f64)
    return pred, mask, image, cam


# ---- the definition as plain loops ---------------------------------------------------------------------------------------------------------------
def div(a, b):
    """IEEE float64 a / b without Python's ZeroDivisionError"""
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def loops_planes(pred, mask, cam, space, r, tau, min_count, min_cos):
    """Steps 1 to 5, literally: Python integers for the integer sums and the cofactors, Python floats (IEEE float64, one operation at a time)
    for everything else."""
    H, W = pred.shape
    s, t, fx, fy, cx, cy, z_min, z_max = (float(v) for v in cam)
    z, wgt, valid = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), bool)
    for v in range(H):
        for u in range(W):
            lin = s * (q16(pred[v, u]) / 65535.0) + t
            zz = div(1.0, lin) if space == "disparity" else lin
            ok = not np.isnan(pred[v, u]) and (mask is None or mask[v, u] != 0) and math.isfinite(zz) and z_min <= zz <= z_max
            z[v, u], wgt[v, u], valid[v, u] = zz, div(1.0, zz), ok
    xyz, normal, keep = np.full((3, H, W), np.nan, f32), np.zeros((3, H, W), f32), np.zeros((H, W), bool)
    for v in range(H):
        for u in range(W):
            if not valid[v, u]:
                continue
            zi = float(z[v, u])
            p0, p1 = (float(u) - cx) / fx, (float(v) - cy) / fy
            xyz[:, v, u] = f32(p0 * zi), f32(p1 * zi), f32(zi)
            n = su = sv = suu = suv = svv = 0
            sw = suw = svw = 0.0
            lim = tau * zi
            for dv in range(-r, r + 1):
                for du in range(-r, r + 1):
                    y, x = v + dv, u + du
                    if not (0 <= y < H and 0 <= x < W) or not valid[y, x] or not abs(float(z[y, x]) - zi) <= lim:
                        continue
                    wj = float(wgt[y, x])
                    n, su, sv, suu, suv, svv = n + 1, su + du, sv + dv, suu + du * du, suv + du * dv, svv + dv * dv
                    sw = sw + wj
                    suw = suw + float(du) * wj
                    svw = svw + float(dv) * wj
            s00, s01, s02, s11, s12, s22 = suu, suv, su, svv, sv, n
            c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
            c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
            det = (s00 * c00 + s01 * c01) + s02 * c02
            assert max(abs(k) for k in (c00, c01, c02, c11, c12, c22, det)) < 2 ** 53
            if n < min_count or det <= 0:
                continue
            c00, c01, c02, c11, c12, c22, det = (float(k) for k in (c00, c01, c02, c11, c12, c22, det))
            a = ((c00 * suw + c01 * svw) + c02 * sw) / det
            b = ((c01 * suw + c11 * svw) + c12 * sw) / det
            c = ((c02 * suw + c12 * svw) + c22 * sw) / det
            m0, m1, m2 = a * fx, b * fy, (c + a * (cx - float(u))) + b * (cy - float(v))
            mm = (m0 * m0 + m1 * m1) + m2 * m2
            length = math.sqrt(mm)
            if length > 0.0 and math.isfinite(length):
                normal[:, v, u] = f32(-m0 / length), f32(-m1 / length), f32(-m2 / length)
            mp = (m0 * p0 + m1 * p1) + m2
            pp = (p0 * p0 + p1 * p1) + 1.0
            keep[v, u] = mp * mp >= ((min_cos * min_cos) * mm) * pp and mp > 0.0
    return xyz, normal, keep


def loops_compact(xyz, normal, keep, image, stride):
    H, W = keep.shape
    pts, nrm, rgb, idx = [], [], [], []
    for v in range(H):
        for u in range(W):
            if keep[v, u] and u % stride == 0 and v % stride == 0:
                pts.append(xyz[:, v, u]), nrm.append(normal[:, v, u]), idx.append(v * W + u)
                rgb.append(image[:, v, u] if image is not None else np.full(3, 255, np.uint8))
    return (np.array(pts, f32).reshape(-1, 3), np.array(nrm, f32).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3), np.array(idx, np.int32))


@pytest.mark.parametrize("space", ["depth", "disparity"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%d-r%d" % s)
def test_host_route_equals_plain_loops(case, space):
    from genpercept_amd import geometry as gm
    h, w, r = case
    pred, mask, image, cam = random_case(np.random.RandomState(100 * h + w), h, w)
    _, tau, min_count, min_cos, _ = gm.check_options(r)
    assert min_count == 2 * r + 1 and min_cos == math.cos(math.radians(85.0))
    kept = 0
    for use_mask in (False, True):
        m = mask if use_mask else None
        xyz, normal, keep = loops_planes(pred, m, cam, space, r, tau, min_count, min_cos)
        assert np.isnan(xyz[2]).any() and (keep.any() or r == 8)
        kept += int(keep.sum())
        for stride in (1, 3):
            im = image if stride == 1 else None
            got = gm.depth_geometry(pred[None, None], cam, None if im is None else im[None], None if m is None else m[None], space, r, stride=stride)
            assert same_bits(got["xyz"][0], xyz) and same_bits(got["normal"][0], normal), (case, space, use_mask)
            assert got["keep"].dtype == np.uint8 and np.array_equal(got["keep"][0], keep.astype(np.uint8))
            want = loops_compact(xyz, normal, keep, im, stride)
            for name, wv in zip(POINTS, want):
                assert same_bits(got[name], wv), (case, space, use_mask, stride, name)
            assert got["offsets"].dtype == np.int64 and got["offsets"].tolist() == [0, len(want[3])]
    assert kept > 0


# ---- the kernels' arithmetic on the CPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "geometry_check.cpp")


@pytest.mark.parametrize("case", CASES + [(40, 70, 2), (33, 100, 3)], ids=lambda s: "%dx%d-r%d" % s)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    from genpercept_amd import geometry as gm
    h, w, r = case
    pred, mask, image, cam = random_case(np.random.RandomState(7 * h + w), h, w)
    _, tau, min_count, min_cos, _ = gm.check_options(r)
    k = 0
    for sp, space in enumerate(gm.SPACES):
        for use_mask, stride in ((False, 1), (True, 3)):
            k += 1
            src, dst = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
            with open(src, "wb") as f:
                f.write(np.array([h, w, sp, r, min_count, stride, use_mask, not use_mask], np.int32).tobytes() + np.array([tau, min_cos], f64).tobytes()
                        + cam.tobytes() + pred.tobytes() + (mask.tobytes() if use_mask else image.tobytes()))
            raw, hw = ps.run_check(check_exe, src, dst)[1], h * w
            want = gm.depth_geometry(pred, cam, None if use_mask else image, mask if use_mask else None, space, r, stride=stride)
            assert same_bits(np.frombuffer(raw[:12 * hw], f32).reshape(3, h, w), want["xyz"][0]), (case, space)
            assert same_bits(np.frombuffer(raw[12 * hw:24 * hw], f32).reshape(3, h, w), want["normal"][0]), (case, space)
            assert same_bits(np.frombuffer(raw[24 * hw:25 * hw], np.uint8).reshape(h, w), want["keep"][0]), (case, space)
            n, pos = int(np.frombuffer(raw[25 * hw:25 * hw + 8], np.int64)[0]), 25 * hw + 8
            assert n == want["offsets"][1] and len(raw) == pos + 31 * n
            assert same_bits(np.frombuffer(raw[pos:pos + 12 * n], f32).reshape(n, 3), want["points"])
            assert same_bits(np.frombuffer(raw[pos + 12 * n:pos + 24 * n], f32).reshape(n, 3), want["point_normals"])
            assert same_bits(np.frombuffer(raw[pos + 24 * n:pos + 27 * n], np.uint8).reshape(n, 3), want["point_rgb"])
            assert same_bits(np.frombuffer(raw[pos + 27 * n:], np.int32), want["point_index"])


# ---- what the definition is for ----------------------------------------------------------------------------------------------------------------------
def plane_depth(h=24, w=32, f=40.0):
    """z float64 [h, w] of the plane n . P = d with n proportional to (0.3, -0.2, -0.93) at distance 1.5 |n_z| (z = 1.5 on the optical axis),
    seen by a camera with fx = fy = f and its principal point at the centre; (z, camera, the unit normal that faces the camera)."""
    n = np.array([0.3, -0.2, -0.93])
    n = n / np.sqrt((n * n).sum())
    d = 1.5 * n[2]
    cam = np.array([1.0, 0.0, f, f, (w - 1) / 2.0, (h - 1) / 2.0, 1e-3, 1e6])
    v, u = np.mgrid[0:h, 0:w].astype(f64)
    z = d / (n[0] * ((u - cam[4]) / f) + n[1] * ((v - cam[5]) / f) + n[2])
    assert z.min() > 1.0 and z.max() < 2.0 and n[2] < 0
    return z, cam, n


def sine_of_angle_to(normal, truth):
    """|N x truth| per pixel for unit vectors: the sine of the angle between them"""
    c = np.cross(np.moveaxis(normal.astype(f64), 0, -1), truth)
    return np.sqrt((c * c).sum(-1))


def test_an_exact_plane_gives_its_normal():
    """Float64 z through the entry without the quantisation: every pixel has a valid fit at r = 1, 2, 4 with tau = 0.05 (the smallest window has
    4, 9 and 21 members), and every component of every normal, as it stands before its one rounding to float32, is within 1e-9 of the truth
    (the system has an integer matrix and is well conditioned: many orders above float64 rounding).  The float32 output is that value
    rounded."""
    from genpercept_amd import geometry as gm
    z, cam, truth = plane_depth()
    for r, smallest in ((1, 4), (2, 9), (4, 21)):
        xyz, normal, keep, raw = gm.geometry_from_depth(z, cam, r, 0.05, raw=True)
        assert raw["n"].min() == smallest and raw["fit"].all() and (raw["det"] > 0).all() and keep.all()
        err = float(np.abs(raw["normal64"] - truth[:, None, None]).max())
        print(f"exact plane, r = {r}: smallest window {raw['n'].min()}, max component error {err:.3e}")
        assert err <= 1e-9
        assert same_bits(normal, raw["normal64"].astype(f32)) and same_bits(xyz[2], z.astype(f32))


def test_a_quantised_plane_gives_its_normal_better_as_the_window_grows():
    """The same plane through step 1 (s = z.max - z.min, t = z.min): the largest angle to the true normal falls as r grows and stays under 0.05
    degrees at r = 1.  Compared by the cross product's norm.  Measured here: 0.0132, 0.0038 and 0.00077 degrees at r = 1, 2, 4."""
    from genpercept_amd import geometry as gm
    z, cam, truth = plane_depth()
    cam[0], cam[1] = z.max() - z.min(), z.min()
    pred = ((z - z.min()) / (z.max() - z.min())).astype(f32)
    worst = []
    for r in (1, 2, 4):
        got = gm.depth_geometry(pred, cam, radius=r)
        assert got["keep"].all() and got["offsets"].tolist() == [0, pred.size]
        worst.append(float(np.degrees(np.arcsin(sine_of_angle_to(got["normal"][0], truth).max()))))
    print("quantised plane: largest angle to the truth in degrees at r = 1, 2, 4:", worst)
    assert worst[0] < 0.05 and worst[0] > worst[1] > worst[2]


def step_case(ramp: bool):
    from genpercept_amd import geometry as gm
    h, w = 24, 32
    pred = np.zeros((h, w), f32)
    pred[:, 16:] = 1.0
    if ramp:
        pred[:, 15], pred[:, 16], pred[:, 17] = 0.25, 0.5, 0.75
    cam = gm.default_camera(h, w)
    cam[0], cam[1] = 0.5, 1.0
    return pred, cam


def test_a_depth_step_does_not_tilt_the_normals_beside_it():
    """Columns < 16 at z = 1, the rest at z = 1.5, r = 2.  With tau = 0.05 no window crosses the step: every fit is valid and every normal is
    (x, y, -1) with |x|, |y| < 1e-12.  With tau = 0.6 the windows cross it and some normal tilts by more than 45 degrees -- what plain finite
    differences do."""
    from genpercept_amd import geometry as gm
    pred, cam = step_case(False)
    got = gm.depth_geometry(pred, cam, radius=2, tau=0.05)
    n = got["normal"][0].astype(f64)
    print(f"depth step, tau = 0.05: max |x|, |y| = {np.abs(n[:2]).max():.3e}")
    assert got["keep"].all() and np.abs(n[:2]).max() < 1e-12 and (n[2] == -1.0).all()
    loose = gm.depth_geometry(pred, cam, radius=2, tau=0.6)["normal"][0].astype(f64)
    tilt = np.degrees(np.arccos(np.clip(-loose[2], -1.0, 1.0)))
    print(f"depth step, tau = 0.6: largest tilt {tilt.max():.1f} degrees")
    assert tilt.max() > 45.0


def test_the_pixels_of_a_ramp_between_two_surfaces_are_dropped():
    """The step replaced by a 3-pixel linear ramp (columns 15, 16, 17), default options: the ramp's middle column is not kept, every pixel three
    or more columns from it is; the point cloud holds no point of the middle column."""
    from genpercept_amd import geometry as gm
    pred, cam = step_case(True)
    got = gm.depth_geometry(pred, cam)
    keep = got["keep"][0].astype(bool)
    cols = np.arange(pred.shape[1])
    assert not keep[:, 16].any() and keep[:, np.abs(cols - 16) >= 3].all()
    assert not (got["point_index"] % pred.shape[1] == 16).any()
    # min_cos is the cosine between the surface normal and the view ray: on the tilted plane, a bound of cos 15 degrees keeps exactly the pixels
    # whose ray meets the plane within 15 degrees of its normal (pixels within 1e-6 of the bound are left out of the comparison)
    z, pcam, truth = plane_depth()
    bound = math.cos(math.radians(15.0))
    v, u = np.mgrid[0:z.shape[0], 0:z.shape[1]].astype(f64)
    p = np.stack([(u - pcam[4]) / pcam[2], (v - pcam[5]) / pcam[3], np.ones_like(u)])
    cos = -(p * truth[:, None, None]).sum(0) / np.sqrt((p * p).sum(0))
    sure = np.abs(cos - bound) > 1e-6
    kept = gm.geometry_from_depth(z, pcam, 2, min_cos=bound)[2]
    assert gm.geometry_from_depth(z, pcam, 2)[2].all() and 0 < kept.sum() < kept.size and np.array_equal(kept[sure], (cos >= bound)[sure])


def test_compaction_and_ply(tmp_path):
    from genpercept_amd import geometry as gm
    rng = np.random.RandomState(11)
    h, w = 21, 30
    per = [random_case(rng, h, w) for _ in range(3)]
    pred, mask, image, cams = (np.stack([p[k] for p in per]) for k in range(4))
    mask[1] = 0                                                       # the middle image is entirely invalid
    for stride in (1, 3, 4):
        got = gm.depth_geometry(pred[:, None], cams, image, mask, "depth", 2, stride=stride)
        off = got["offsets"]
        assert off.dtype == np.int64 and off.shape == (4,) and off[0] == 0 and off[1] == off[2] and off[3] == len(got["points"]) > 0
        assert not got["keep"][1].any() and np.isnan(got["xyz"][1]).all() and not got["normal"][1].any()
        for k in range(3):
            sel = np.zeros((h, w), bool)
            sel[::stride, ::stride] = got["keep"][k, ::stride, ::stride] != 0
            idx = got["point_index"][off[k]:off[k + 1]]
            assert idx.dtype == np.int32 and off[k + 1] - off[k] == sel.sum() and (np.diff(idx) > 0).all() and np.array_equal(idx, np.flatnonzero(sel))
            assert same_bits(got["points"][off[k]:off[k + 1]], got["xyz"][k].reshape(3, -1)[:, idx].T)
            assert same_bits(got["point_normals"][off[k]:off[k + 1]], got["normal"][k].reshape(3, -1)[:, idx].T)
            assert same_bits(got["point_rgb"][off[k]:off[k + 1]], image[k].reshape(3, -1)[:, idx].T)
        assert (gm.depth_geometry(pred[:, None], cams, None, mask, stride=stride)["point_rgb"] == 255).all()
        assert np.isfinite(got["points"]).all() and np.allclose((got["point_normals"].astype(f64) ** 2).sum(1), 1.0, atol=1e-6)
    # the PLY file, read back by a parser of its own
    path = str(tmp_path / "cloud.ply")
    gm.write_ply(path, got["points"], got["point_normals"], got["point_rgb"])
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == f"element vertex {len(got['points'])}"
    assert lines[3:] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {k}" for k in ("red", "green", "blue")]
    want = b"".join(got["points"][i].astype("<f4").tobytes() + got["point_normals"][i].astype("<f4").tobytes() + got["point_rgb"][i].tobytes()
                    for i in range(len(got["points"])))
    assert body == want and len(body) == 27 * len(got["points"])
    gm.write_ply(path, got["points"][:0], got["point_normals"][:0], got["point_rgb"][:0])
    assert open(path, "rb").read().endswith(b"element vertex 0\n" + head.split(b"\n", 3)[3] + b"end_header\n")
    with pytest.raises(ValueError):
        gm.write_ply(path, got["points"], got["point_normals"][:-1], got["point_rgb"])


def test_options_cameras_and_shapes_are_checked():
    from genpercept_amd import geometry as gm
    cos85 = math.cos(math.radians(85.0))
    assert gm.pointcloud_options(True) == dict(radius=2, tau=0.05, min_count=5, min_cos=cos85, stride=1)
    assert gm.pointcloud_options(dict(radius=8, stride=64, tau=1.0, min_cos=0.0)) == dict(radius=8, tau=1.0, min_count=17, min_cos=0.0, stride=64)
    assert gm.pointcloud_options(dict(radius=1, min_count=9))["min_count"] == 9
    for bad in (False, None, 1, "yes", dict(r=2), dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(tau=0.0), dict(tau=1.5),
                dict(tau=float("nan")), dict(min_count=2), dict(min_count=26), dict(min_count=5.0), dict(min_cos=1.0), dict(min_cos=-0.1),
                dict(min_cos=float("nan")), dict(stride=0), dict(stride=65), dict(stride=2.0)):
        with pytest.raises(ValueError):
            gm.pointcloud_options(bad)
    fx, fy, cx, cy = gm.intrinsics_from_fov(480, 640)
    assert fx == fy == 320.0 / math.tan(math.radians(55.0) / 2.0) and (cx, cy) == (319.5, 239.5)
    assert gm.intrinsics_from_fov(10, 20, 90.0)[0] == 10.0 / math.tan(math.radians(90.0) / 2.0)
    assert gm.default_camera(480, 640).tolist() == [1.0, 1.0, fx, fy, cx, cy, 1e-3, 1e6]
    for bad in ((0, 5), (5, 0), (5, 5, 0.0), (5, 5, 180.0), (5.0, 5)):
        with pytest.raises(ValueError):
            gm.intrinsics_from_fov(*bad)
    pred = np.random.RandomState(5).rand(2, 1, 6, 7).astype(f32)
    got = gm.depth_geometry(pred)                                    # the default camera: z in [1, 2]
    assert got["xyz"].shape == (2, 3, 6, 7) and got["xyz"][:, 2].min() >= 1.0 and got["xyz"][:, 2].max() <= 2.0
    cam = gm.default_camera(6, 7)
    assert same_bits(gm.depth_geometry(pred, cam)["xyz"], got["xyz"]) and same_bits(gm.depth_geometry(pred, np.stack([cam, cam]))["normal"], got["normal"])
    assert same_bits(gm.depth_geometry(pred[0, 0])["xyz"], got["xyz"][:1]) and same_bits(gm.depth_geometry(pred[0])["keep"], got["keep"][:1])

    def with_field(k, v):
        c = cam.copy()
        c[k] = v
        return c

    for bad in (dict(cameras=cam[:7]), dict(cameras=np.stack([cam] * 3)), dict(cameras=with_field(2, 0.0)), dict(cameras=with_field(3, -1.0)),
                dict(cameras=with_field(6, 0.0)), dict(cameras=with_field(7, 1e-3)), dict(cameras=with_field(0, np.nan)), dict(cameras=with_field(4, np.inf)),
                dict(space="metric"), dict(image=np.zeros((2, 3, 6, 6), np.uint8)), dict(image=np.zeros((2, 3, 6, 7), f32)), dict(mask=np.ones((2, 7, 6), bool)),
                dict(mask=np.ones((2, 6, 7), f32)), dict(radius=9), dict(stride=0)):
        with pytest.raises(ValueError):
            gm.depth_geometry(pred, **bad)
    for bad in (pred[:, [0, 0]], (pred * 255).astype(np.uint8), pred[0, 0, 0]):
        with pytest.raises(ValueError):
            gm.depth_geometry(bad)


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    _, math_h = ps.assert_entries_bound(NAMES, "depth_geometry.hip", "depth_geometry_math.h")
    args = engine.SYMBOLS["gp_depth_geometry"][1]
    assert len(args) == 24 and args[9] is C.c_double and args[11] is C.c_double and engine.SYMBOLS["gp_depth_geometry_workspace"] == (C.c_longlong, [C.c_int] * 4)
    assert callable(engine.depth_geometry)
    assert "hip_runtime" not in math_h


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 64, 64, 1), (65536, 8, 8, 1), (1, 0, 64, 1), (1, 64, 16385, 1), (1, 64, 64, 0), (1, 64, 64, 65), (8, 16384, 16384, 1), (-1, 64, 64, 1)):
            assert lib.gp_depth_geometry_workspace(*bad) == 0, bad
        for h, w, stride in ((17, 23, 1), (33, 200, 3), (768, 768, 1), (2048, 3072, 2), (16384, 16384, 64)):
            one = lib.gp_depth_geometry_workspace(1, h, w, stride)
            assert one > 0 and one % 8 == 0 and one >= 64 + 25 * h * w
            for b in (2, 7):
                assert lib.gp_depth_geometry_workspace(b, h, w, stride) == b * one
        assert lib.gp_depth_geometry_workspace(7, 16384, 16384, 1) > 0


def geometry_args(lib, b, h, w, stride=1, **ptrs):
    """A valid argument set of gp_depth_geometry for these sizes (pointers as given, small integers by default), and the host camera array it
    points to."""
    from genpercept_amd import geometry as gm
    cams = np.ascontiguousarray(np.stack([gm.default_camera(h, w)] * b))
    ok = dict(pred=0x1000, mask=0x2001, image=0x3003, cams=cams.ctypes.data, B=b, H=h, W=w, space=0, r=2, tau=0.05, min_count=5, min_cos=0.1, stride=stride,
              xyz=0x4000, normal=0x5000, keep=0x6001, points=0x7000, point_normals=0x8000, point_rgb=0x9001, point_index=0xA000, offsets=0xB000, ws=0xC000,
              nbytes=int(lib.gp_depth_geometry_workspace(b, h, w, stride)))
    ok.update(ptrs)
    return ok, cams


def invalid_cases(ok, cams, keep):
    """The argument sets gp_depth_geometry refuses, as changes to a valid set `ok`; the host arrays the cases point to are appended to `keep`."""
    huge = 1 << 62

    def cam(k, v, image=-1):
        c = cams.copy()
        c[image, k] = v
        keep.append(c)
        return c.ctypes.data

    outs = dict(xyz=None, normal=None, keep=None, points=None, point_normals=None, point_rgb=None, point_index=None, offsets=None)
    return [dict(pred=None), dict(cams=None), dict(ws=None),
            dict(B=0), dict(B=-1), dict(B=65536, nbytes=huge), dict(H=0), dict(W=-5), dict(H=16385, nbytes=huge), dict(W=16385, nbytes=huge),
            dict(B=8, H=16384, W=16384, nbytes=huge),                                            # B H W = 2^31
            dict(space=2), dict(space=-1), dict(r=0), dict(r=9), dict(r=-1), dict(tau=0.0), dict(tau=-0.5), dict(tau=1.0000001), dict(tau=float("nan")),
            dict(min_count=2), dict(min_count=26), dict(min_count=0), dict(r=1, min_count=10), dict(min_cos=1.0), dict(min_cos=-1e-9),
            dict(min_cos=float("nan")), dict(stride=0), dict(stride=65), dict(stride=-1),
            dict(cams=cam(2, 0.0)), dict(cams=cam(3, -1.0)), dict(cams=cam(6, 0.0)), dict(cams=cam(7, 1e-3)), dict(cams=cam(6, 2e6)),
            dict(cams=cam(0, float("nan"))), dict(cams=cam(1, float("inf"))), dict(cams=cam(4, float("-inf"))), dict(cams=cam(5, float("nan"), 0)),
            dict(cams=cam(2, float("inf"))),
            outs, dict(outs, points=ok["points"]), dict(offsets=None), dict(outs, point_rgb=ok["point_rgb"], xyz=ok["xyz"]),
            dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1), dict(xyz=ok["xyz"] + 2), dict(normal=ok["normal"] + 1), dict(points=ok["points"] + 2),
            dict(point_normals=ok["point_normals"] + 3), dict(point_index=ok["point_index"] + 2), dict(offsets=ok["offsets"] + 4),
            dict(offsets=ok["offsets"] + 1), dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1),
            dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=ok["nbytes"] // 2)]


def call_geometry(lib, a):
    return lib.gp_depth_geometry(a["pred"], a["mask"], a["image"], a["cams"], a["B"], a["H"], a["W"], a["space"], a["r"], a["tau"], a["min_count"], a["min_cos"],
                                 a["stride"], a["xyz"], a["normal"], a["keep"], a["points"], a["point_normals"], a["point_rgb"], a["point_index"], a["offsets"],
                                 a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced (the cameras are a host array and are read)."""
    for lib in _libs():
        ok, cams = geometry_args(lib, 2, 40, 70)
        keep = [cams]
        assert ok["nbytes"] > 0
        ps.assert_all_refused(call_geometry, lib, ok, invalid_cases(ok, cams, keep))
