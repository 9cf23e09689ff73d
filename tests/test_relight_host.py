"""The relighting on the host (genpercept_amd/relight.py), without a GPU: the numpy route equals plain scalar loops written here from the
definition in include/genpercept_hip.h, and a stand-alone CPU build of the kernel's arithmetic (tests/relight_check.cpp over
csrc/relight_math.h, built with the ROCm clang++ under the address and undefined-behaviour sanitizers and run as a child process); the exact
square root; the properties the definition is for, with exact expectations; the light rows against hand-computed integers and the user's
terms; the entry declared, exported, bound, and its argument checks with NULL buffers.  There is no tolerance in this file."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import libs as _libs, same_bits  # noqa: E402,F401

SHAPES = [(7, 9), (16, 16), (33, 40)]
AZIMUTHS = (0.0, 90.0, 45.0, 135.0, 225.0, 315.0, 180.0, 270.0)      # straight on along x and y (uy = 0, ux = 0) and all four quadrants


def random_case(rng, h, w):
    """One image: (pred float32 [h, w], two noisy planes and a nearer box, values beyond [0, 1] and NaNs among them; image uint8 [3, h, w];
    normal float32 [3, h, w], ENCODED in [0, 1], a bumpy camera-facing surface with NaN, zero-length and out-of-range pixels; weight uint8
    [h, w])."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pred = 0.7 - 0.2 * xx / w + 0.1 * yy / h
    pred[h // 4: h // 4 + max(2, h // 3), w // 3: w // 3 + max(2, w // 4)] = 0.25
    pred += rng.uniform(-0.01, 0.01, (h, w))
    pred[rng.rand(h, w) < 0.02] = 1.2
    pred[rng.rand(h, w) < 0.02] = -0.1
    pred[rng.rand(h, w) < 0.04] = np.nan
    image = rng.randint(0, 256, (3, h, w)).astype(np.uint8)
    n = np.stack([0.6 * np.sin(xx / 2.0) + rng.uniform(-0.2, 0.2, (h, w)), 0.6 * np.cos(yy / 3.0) + rng.uniform(-0.2, 0.2, (h, w)), -np.ones((h, w))])
    n /= np.sqrt((n * n).sum(0))[None]
    normal = 0.5 * n + 0.5
    normal[:, rng.rand(h, w) < 0.04] = 0.5               # a zero normal: no fit
    normal[rng.randint(0, 3), rng.rand(h, w) < 0.04] = np.nan
    normal[rng.rand(3, h, w) < 0.02] = 1.3
    normal[rng.rand(3, h, w) < 0.02] = -0.2
    weight = rng.randint(0, 256, (h, w)).astype(np.uint8)
    weight[rng.rand(h, w) < 0.2] = 255
    weight[rng.rand(h, w) < 0.2] = 0
    return pred.astype(np.float32), image, normal.astype(np.float32), weight


def raw_of(normal):
    """The raw form of an encoded normal map, values in [-1.6, 1.6]."""
    return (np.float32(2.0) * normal - np.float32(1.0)).astype(np.float32)


def stored(normal, encoded, flip):
    """The encoded camera-facing map `normal` ([3, h, w] or a batch of them) as a checkpoint of another convention stores it: raw where not
    encoded, and the flipped axes negated, so that the call's flips bring it back."""
    out = normal.copy() if encoded else raw_of(normal)
    for k in range(3):
        if flip[k]:
            out[..., k, :, :] = (np.float32(1.0) - out[..., k, :, :]) if encoded else -out[..., k, :, :]
    return out


def light_terms(n, reach):
    """n lights of different directions, colours, specular lobes, softness, strength and bias; the longest march is `reach` steps."""
    out = []
    for j in range(n):
        out.append(dict(azimuth=AZIMUTHS[j], elevation=(25.0, 40.0, 55.0, 70.0)[j % 4], intensity=0.4 + 0.3 * j, colour=(1.0, 1.0 - 0.1 * j, 0.5 + 0.05 * j),
                        specular=(0.0, 0.8, 2.0)[j % 3], shininess=1 << (j % 8), shadows=j != 5, reach=max(0, reach - 3 * j) if j else reach,
                        softness=(0.0, 0.02, 0.3)[j % 3], strength=(1.0, 0.6)[j % 2], bias=(0.002, 0.0, 0.05)[j % 3]))
    return out


def all_tables():
    from genpercept_amd import lens_blur as lb
    return dict(srgb=lb.srgb_tables(), identity=lb.identity_tables())


# ---- the definition once more, in plain loops ---------------------------------------------------------------------------------------------------------
def loops_relight(image, normal, pred, weight, rows, encoded, flip, space, tables):
    """One image by the header's steps 1 .. 4, in Python integers: (out uint8 [3, h, w], shadow uint8 [h, w])."""
    to_lin, from_lin = tables
    rows = [[int(v) for v in r] for r in rows]
    lights, amb = rows[:-1], rows[-1]
    _, h, w = image.shape
    D = ps.loops_nearness(pred, space) if pred is not None else None
    out, shadow = np.zeros((3, h, w), np.uint8), np.zeros((h, w), np.uint8)
    one = np.float32(1.0)
    for y in range(h):
        for x in range(w):
            N, nan = [], False
            for k in range(3):
                v = np.float32(normal[k, y, x])
                if np.isnan(v):
                    nan = True
                    N.append(0)
                    continue
                if encoded:
                    n = 2 * ps.q16(v) - 65535
                else:
                    c = (v if v < one else one) if v > -one else -one
                    n = int(np.float32(c * np.float32(65535.0)))           # (int() truncates towards zero)
                N.append(-n if flip[k] else n)
            m = math.isqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2])
            if nan or m < 256:
                N, m = [0, 0, -65535], 65535
            G, S, worst = [0, 0, 0], [0, 0, 0], 0
            for r in lights:
                cos12 = min(4096, max(0, (N[0] * r[0] + N[1] * r[1] + N[2] * r[2]) // (4 * m)))
                if cos12 == 0:
                    continue
                s = min(4096, max(0, (N[0] * r[3] + N[1] * r[4] + N[2] * r[5]) // (4 * m)))
                for _ in range(r[12]):
                    s = (s * s + 2048) >> 12
                E = 0
                if D is not None and not np.isnan(pred[y, x]):
                    for t in range(1, r[19] + 1):
                        qx, qy = x + ((t * r[13] + 128) >> 8), y + ((t * r[14] + 128) >> 8)
                        if 0 <= qx < w and 0 <= qy < h:
                            E = max(E, D[qy][qx] - D[y][x] - r[16] - t * r[15])
                dark = min(256, (E * r[17] + 128) >> 8) if r[17] else (256 if E > 0 else 0)
                shade = (dark * r[18]) >> 8
                vis = 256 - shade
                for k in range(3):
                    G[k] += r[6 + k] * cos12 * vis
                    S[k] += r[9 + k] * s * vis
                worst = max(worst, shade)
            wt = 255 if weight is None else int(weight[y, x])
            for k in range(3):
                byte = int(image[k, y, x])
                lin = min(4095, ((int(to_lin[byte]) * (amb[k] + (G[k] >> 16)) + 2048) >> 12) + min(S[k] >> 16, 4095))
                out[k, y, x] = (wt * int(from_lin[lin]) + (255 - wt) * byte + 127) // 255
            shadow[y, x] = min(255, worst)
    return out, shadow


def variations():
    """Eight settings that between them hold 1 and 8 lights, both encodings, every flip, both spaces, with and without pred and weight."""
    for bits in range(8):
        yield dict(n_lights=8 if bits in (0, 3, 5, 6) else 1, encoded=bits % 2 == 0, flip=(bool(bits & 1), bool(bits & 2), bool(bits & 4)),
                   space=("depth", "disparity")[bits >> 1 & 1], use_pred=bits != 3, use_weight=bits % 3 != 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_route_equals_plain_loops(shape):
    from genpercept_amd import relight as rl
    h, w = shape
    pred, image, normal, weight = random_case(np.random.RandomState(13 * h + w), h, w)
    shaded = 0
    for k, v in enumerate(variations()):
        rows = rl.relight_lights(light_terms(v["n_lights"], min(64, 6 + 9 * k)), ambient=(0.2, 0.3, 0.25 + 0.1 * k), relief=24.0)
        nrm = stored(normal, v["encoded"], v["flip"])
        tables = list(all_tables().values())[k % 2]
        kw = dict(encoded=v["encoded"], flip=v["flip"], space=v["space"], tables=tables)
        got, got_sh = rl.relight_rows(image, nrm, pred if v["use_pred"] else None, weight if v["use_weight"] else None, rows, want_shadow=True, **kw)
        want, want_sh = loops_relight(image, nrm, pred if v["use_pred"] else None, weight if v["use_weight"] else None, rows, **kw)
        assert same_bits(got_sh[0], want_sh) and same_bits(got[0], want), (shape, v)
        assert not same_bits(want, image) and (want_sh.any() == v["use_pred"])
        shaded += int(want_sh.any())
    assert shaded >= 6


def test_host_route_equals_plain_loops_on_a_batch_whose_middle_map_is_nan():
    from genpercept_amd import relight as rl
    b, h, w = 3, 16, 16
    pred, image, normal, weight = ps.batch_case(random_case, 5, b, h, w, middle_nan=True)
    rows = rl.relight_lights(light_terms(8, 64), ambient=0.3, relief=16.0)
    got, got_sh = rl.relight_rows(image, normal, pred, weight, rows, want_shadow=True)
    for i in range(b):
        want, want_sh = loops_relight(image[i], normal[i], pred[i, 0], weight[i], rows, True, (False,) * 3, "depth", all_tables()["srgb"])
        assert same_bits(got[i], want) and same_bits(got_sh[i], want_sh), i
    assert not got_sh[1].any() and got_sh[0].any() and got_sh[2].any()
    assert same_bits(got[1], rl.relight_rows(image[1], normal[1], None, weight[1], rows)[0])       # a map of NaNs shadows nothing


# ---- the kernel's arithmetic on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "relight_check.cpp")


@pytest.mark.parametrize("shape", SHAPES + [(40, 70)], ids=lambda s: "%dx%d" % s)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, shape, tmp_path):
    from genpercept_amd import relight as rl
    h, w = shape
    pred, image, normal, weight = random_case(np.random.RandomState(7 * h + w), h, w)
    hw = h * w
    for k, v in enumerate(variations()):
        rows = rl.relight_lights(light_terms(v["n_lights"], min(64, 5 + 9 * k)), ambient=(0.2, 0.3, 0.25 + 0.1 * k), relief=24.0)
        nrm = stored(normal, v["encoded"], v["flip"])
        to_lin, from_lin = tables = list(all_tables().values())[k % 2]
        bits = sum(int(f) << i for i, f in enumerate(v["flip"]))
        src, dst = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
        with open(src, "wb") as f:
            f.write(np.array([h, w, len(rows) - 1, v["encoded"], bits, rl.SPACES.index(v["space"]), v["use_pred"], v["use_weight"]], np.int32).tobytes()
                    + rows.tobytes() + to_lin.astype(np.uint16).tobytes() + from_lin.tobytes() + nrm.tobytes() + image.tobytes()
                    + (pred.tobytes() if v["use_pred"] else b"") + (weight.tobytes() if v["use_weight"] else b""))
        raw = ps.run_check(check_exe, src, dst, timeout=120)[1]
        assert len(raw) == 4 * hw
        want, want_sh = rl.relight_rows(image, nrm, pred if v["use_pred"] else None, weight if v["use_weight"] else None, rows, v["encoded"], v["flip"],
                                        v["space"], tables, want_shadow=True)
        assert same_bits(np.frombuffer(raw[:3 * hw], np.uint8).reshape(3, h, w), want[0]), (shape, v)
        assert same_bits(np.frombuffer(raw[3 * hw:], np.uint8).reshape(h, w), want_sh[0]), (shape, v)


def test_the_square_root_is_exact():
    from genpercept_amd import relight as rl
    longest = int(math.floor(math.sqrt(3.0) * 65535.0))
    assert longest == 113509 == math.isqrt(3 * 65535 * 65535)
    ks = np.array([k + d for k in (256, 65535, longest) for d in range(-3, 4)], np.int64)
    for off in (-1, 0, 1):
        s = ks * ks + off
        assert rl.isqrt(s).tolist() == [math.isqrt(int(v)) for v in s] == (ks - (off < 0)).tolist()
    assert rl.isqrt(np.array([0, 1, 2, 3, 4, 3 * 65535 * 65535], np.int64)).tolist() == [0, 1, 1, 1, 2, longest]


# ---- what the definition is for -----------------------------------------------------------------------------------------------------------------------
def facing(h, w, encoded=True):
    """A camera-facing plane as a normal map [1, 3, h, w]."""
    n = np.zeros((1, 3, h, w), np.float32)
    n[:, 2] = -1.0
    return (np.float32(0.5) * n + np.float32(0.5)).astype(np.float32) if encoded else n


def test_one_white_light_from_the_camera_returns_the_image():
    from genpercept_amd import relight as rl
    image = np.random.RandomState(1).randint(0, 256, (1, 3, 12, 19)).astype(np.uint8)
    image[0, :, 0, :8] = np.array([0, 1, 2, 3, 252, 253, 254, 255], np.uint8)
    light = dict(azimuth=0.0, elevation=90.0, intensity=1.0, colour=(1.0, 1.0, 1.0), specular=0.0)
    rows = rl.relight_lights(light, ambient=0.0)
    assert rows[0, :6].tolist() == [0, 0, -16384, 0, 0, -16384] and rows[0, 6:9].tolist() == [256] * 3 and not rows[1].any() and rows[0, 19] == 0
    for tables in all_tables().values():
        for encoded in (True, False):
            # (the raw plane is exactly (0, 0, -65535); the encoded one (-1, -1, -65535), whose cosine is 4096 all the same)
            out = rl.relight(image, facing(12, 19, encoded), lights=light, ambient=0.0, encoded=encoded, tables=tables)
            assert same_bits(out, image)
    # pixels without a usable normal are that plane
    assert same_bits(rl.relight(image, np.full((1, 3, 12, 19), np.nan, np.float32), lights=light, ambient=0.0), image)
    assert same_bits(rl.relight(image, np.full((1, 3, 12, 19), 0.5, np.float32), lights=light, ambient=0.0), image)


def test_shading_and_weight():
    from genpercept_amd import relight as rl
    image = np.random.RandomState(2).randint(0, 256, (1, 3, 10, 14)).astype(np.uint8)
    to_lin, from_lin = rl.srgb_tables()
    behind = dict(azimuth=30.0, elevation=-20.0, intensity=3.0, specular=4.0)                # behind the surface: N . L < 0
    for amb in (0.0, 0.5, 1.0):
        out = rl.relight(image, facing(10, 14), lights=behind, ambient=amb)
        a12 = int(math.floor(4096.0 * amb + 0.5))
        want = from_lin[np.minimum(4095, (to_lin[image].astype(np.int64) * a12 + 2048) >> 12)]
        assert same_bits(out, want)                                                         # ambient only
    assert same_bits(rl.relight(image, facing(10, 14), lights=behind, ambient=1.0), image)
    side = dict(azimuth=180.0, elevation=30.0, intensity=0.8, specular=0.3, shininess=4)
    relit = rl.relight(image, facing(10, 14), lights=side, ambient=0.1)
    assert not same_bits(relit, image) and (relit < 255).any()
    assert same_bits(rl.relight(image, facing(10, 14), weight=np.zeros((1, 10, 14), np.uint8), lights=side, ambient=0.1), image)
    assert same_bits(rl.relight(image, facing(10, 14), weight=np.full((1, 10, 14), 255, np.uint8), lights=side, ambient=0.1), relit)
    half = rl.relight(image, facing(10, 14), weight=np.full((1, 10, 14), 128, np.uint8), lights=side, ambient=0.1)
    assert same_bits(half, ((128 * relit.astype(np.int64) + 127 * image.astype(np.int64) + 127) // 255).astype(np.uint8))
    # a colour per light, and the lights add up
    red = rl.relight(image, facing(10, 14), lights=dict(side, colour=(1.0, 0.0, 0.0), specular=0.0), ambient=0.0)
    assert not red[0, 1:].any() and red[0, 0].any()


@pytest.mark.parametrize("elevation,height", [(30.0, 0.3), (60.0, 0.5), (15.0, 0.05)])
def test_a_wall_lit_from_the_left_shadows_exactly_the_columns_the_march_reaches(elevation, height):
    """disparity space: the ground at 0.2, a wall 4 columns wide and `height` nearer.  Lit from the left with hard shadows, a ground pixel t
    columns right of the wall's last column is dark iff t <= reach and D_wall - D_ground - bias - t rise > 0 -- its nearest wall sample has
    the largest excess --, and nothing left of the wall or on it is."""
    from genpercept_amd import relight as rl
    h, w, c0, c1 = 6, 90, 20, 24
    pred = np.full((1, 1, h, w), 0.2, np.float32)
    pred[..., c0:c1] = 0.2 + height
    image = np.full((1, 3, h, w), 200, np.uint8)
    light = dict(azimuth=180.0, elevation=elevation, reach=40, softness=0.0, strength=1.0, bias=0.001)
    row = rl.relight_lights(light, relief=32.0)[0]
    ux, uy, rise, bias, soft, strength, reach = (int(v) for v in row[13:20])
    assert (ux, uy, soft, strength, reach) == (-256, 0, 0, 256, 40) and rise > 0
    step = ps.q16(pred[0, 0, 0, c0]) - ps.q16(pred[0, 0, 0, 0])
    dark = [c1 - 1 + t for t in range(1, w - c1 + 1) if t <= reach and step - bias - t * rise > 0]
    assert 0 < len(dark) < 40
    out, shadow = rl.relight(image, facing(h, w), pred, lights=light, relief=32.0, space="disparity", want_shadow=True)
    want = np.zeros((h, w), np.uint8)
    want[:, dark] = 255
    assert same_bits(shadow[0], want)
    lit = rl.relight(image, facing(h, w), None, lights=light, relief=32.0)
    assert same_bits(out[..., :c1], lit[..., :c1]) and (out[0][:, :, dark] < lit[0][:, :, dark]).all()
    # lit from the right the shadow falls to the left
    mirrored, msh = rl.relight(image, facing(h, w), pred[..., ::-1].copy(), lights=dict(light, azimuth=0.0), relief=32.0, space="disparity", want_shadow=True)
    assert same_bits(msh[0, :, ::-1], want)
    # in depth space the same scene is 1 - pred up to the quantiser's rounding: a wall again, one step of the scale lower at most
    assert rl.relight(image, facing(h, w), (1.0 - pred).astype(np.float32), lights=light, relief=32.0, want_shadow=True)[1].any()


def test_light_rows_are_these_integers():
    from genpercept_amd import relight as rl
    rows = rl.relight_lights(dict(azimuth=180.0, elevation=30.0, intensity=1.0, colour=(1.0, 0.5, 0.25), specular=0.5, shininess=16, reach=20, softness=0.0,
                                  strength=1.0, bias=0.002), ambient=0.35, relief=64.0)
    assert rows.dtype == np.int32 and rows.shape == (2, 20) and rl.ROW == 20 and len(rl.ROW_FIELDS) == 20
    # L = (-cos 30, 0, -sin 30); H = (L + (0, 0, -1)) / sqrt(3) = (-1/2, 0, -cos 30); rise = tan 30 * 1 * 65535 / 64 = 591.2
    assert rows[0].tolist() == [-14189, 0, -8192, -8192, 0, -14189, 256, 128, 64, 128, 64, 32, 4, -256, 0, 591, 131, 0, 256, 20]
    assert rows[1].tolist() == [1434, 1434, 1434] + [0] * 17
    # a diagonal light: azimuth 45 is up and to the right, the step (256, -256) is sqrt(2) pixels long
    up_right = rl.relight_lights(dict(azimuth=45.0, elevation=45.0, softness=0.01, strength=0.5, bias=0.0, reach=64), ambient=(0.0, 1.0, 16.0), relief=128.0)
    assert up_right[0, :3].tolist() == [8192, -8192, -11585] and up_right[0, 13:].tolist() == [256, -256, 724, 0, 100, 128, 64]
    assert up_right[1, :3].tolist() == [0, 4096, 65536]
    # from the camera: no step, no reach; shadows off: no reach; a steep light's rise is capped
    assert rl.relight_lights(dict(elevation=90.0))[0, 13:].tolist() == [0, 0, 0, 131, 0, 256, 0]
    assert rl.relight_lights(dict(shadows=False))[0, 13:16].tolist() == [0, 0, 0] and rl.relight_lights(dict(shadows=False))[0, 19] == 0
    assert rl.relight_lights(dict(azimuth=0.0, elevation=89.9), relief=1.0)[0, 13:16].tolist() == [256, 0, 65535]
    assert rl.relight_lights(dict(softness=0.001))[0, 17] == 256 and rl.relight_lights(dict(softness=1.0))[0, 17] == 1
    # the defaults, and up to 8 lights
    assert len(rl.relight_lights()) == 2 and len(rl.relight_lights([True] * 8)) == 9 and rl.relight_options(True) == [rl._check_light(rl.DEFAULT_LIGHT)]
    assert [r[12] for r in rl.relight_lights([dict(shininess=1 << k) for k in range(8)])[:-1].tolist()] == list(range(8))


def test_terms_and_rows_outside_their_ranges_are_refused():
    from genpercept_amd import relight as rl
    for bad in (dict(azimuth=float("nan")), dict(azimuth="left"), dict(elevation=91.0), dict(elevation=-91.0), dict(intensity=-0.1), dict(intensity=16.5),
                dict(colour=(1.0, 0.5)), dict(colour=(1.0, 0.5, 1.5)), dict(colour=(1.0, -0.5, 0.5)), dict(specular=-1.0), dict(specular=17.0),
                dict(intensity=8.0, specular=4.0), dict(shininess=3), dict(shininess=256), dict(shininess=0), dict(shininess=2.0), dict(shadows=1),
                dict(reach=65), dict(reach=-1), dict(reach=2.5), dict(softness=-0.1), dict(softness=1.5), dict(strength=1.1), dict(strength=-0.1),
                dict(bias=-0.1), dict(bias=1.1), dict(colour="red"), dict(tint=1.0), "sun", None, [], [True] * 9, [dict(reach=70)]):
        with pytest.raises(ValueError):
            rl.relight_lights(bad)
    for bad in (dict(ambient=-0.1), dict(ambient=17.0), dict(ambient=(1.0, 1.0)), dict(ambient=float("inf")), dict(relief=0.0), dict(relief=-4.0),
                dict(relief=float("nan")), dict(relief=[64.0])):
        with pytest.raises(ValueError):
            rl.relight_lights(True, **bad)
    ok = rl.relight_lights(dict(azimuth=0.0, reach=10))                                     # (ux, uy) = (256, 0)
    for col, value in ((0, 16385), (2, -16385), (5, 20000), (6, -1), (8, 4097), (11, 4097), (12, 8), (12, -1), (13, 257), (13, 255), (14, -257), (15, -1),
                       (15, 65536), (16, 65536), (17, 257), (18, 257), (18, -1), (19, 65), (19, -1)):
        bad = ok.copy()
        bad[0, col] = value
        with pytest.raises(ValueError):
            rl.check_rows(bad)
    for col, value in ((0, -1), (1, 65537)):
        bad = ok.copy()
        bad[1, col] = value
        with pytest.raises(ValueError):
            rl.check_rows(bad)
    for bad in (ok[:1], ok[0], ok.astype(np.float32), np.zeros((10, 20), np.int32), ok[:, :19]):
        with pytest.raises(ValueError):
            rl.check_rows(bad)
    pred, image, normal, weight = random_case(np.random.RandomState(8), 10, 12)
    for bad in (dict(image=image.astype(np.float32)), dict(image=image[:2]), dict(normal=normal[:2]), dict(normal=np.zeros_like(normal, np.uint8)),
                dict(normal=normal[:, :5]), dict(pred=pred[:5]), dict(pred=np.zeros_like(pred, np.uint8)), dict(weight=weight[:5]),
                dict(weight=weight.astype(np.float32)), dict(flip=(True, False)), dict(flip=(1, 0, 0)), dict(flip=True), dict(space="metric"),
                dict(tables=(np.zeros(256, np.uint16), np.zeros(4096, np.uint8))), dict(lights=dict(reach=99))):
        with pytest.raises(ValueError):
            rl.relight(**dict(dict(image=image, normal=normal, pred=pred, weight=weight), **bad))


@pytest.fixture
def library_calls(monkeypatch):
    return ps.library_calls(monkeypatch)


def test_the_binding_the_pipeline_and_the_loop_refuse_before_the_library_is_touched(library_calls, tmp_path):
    import torch
    from genpercept_amd import engine
    from genpercept_amd import infer_eval as ie
    from genpercept_amd.pipeline import GenPerceptPipeline
    image, normal, maps = torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.full((2, 3, 8, 8), 0.5), torch.full((2, 1, 8, 8), 0.5)
    weight = torch.zeros((2, 8, 8), dtype=torch.uint8)
    for bad in (dict(image=image.float()), dict(image=image[:1]), dict(normal=normal[:, :2]), dict(normal=normal[..., :7]), dict(normal=normal.numpy()),
                dict(normal=normal.to(torch.int32)), dict(pred=maps[..., :7]), dict(pred=maps.to(torch.int32)), dict(pred=maps[:1]), dict(weight=weight.float()),
                dict(weight=weight[:, :7]), dict(lights=dict(reach=65)), dict(lights=dict(elevation=100.0)), dict(lights=[True] * 9), dict(ambient=-1.0),
                dict(relief=0.0), dict(flip=(True, False)), dict(space="metric"), dict(tables=(np.zeros(256, np.uint16), np.zeros(4096, np.uint8))),
                dict(lights=np.zeros((2, 20), np.int32) + 70000)):
        with pytest.raises(ValueError):
            engine.relight(**dict(dict(image=image, normal=normal, pred=maps, weight=weight), **bad))
    for good in (dict(), dict(pred=None), dict(weight=None, want_shadow=True), dict(lights=[True, dict(azimuth=10.0)], encoded=False)):
        with pytest.raises(AssertionError):      # CPU tensors get as far as the assert that they are on the device
            engine.relight(**dict(dict(image=image, normal=normal, pred=maps, weight=weight), **good))
    pipe = GenPerceptPipeline(unet={}, vae={}, text_encoder=np.zeros((2, 1024), np.float32), torch_dtype=torch.float32)
    for bad in (dict(mode="matting"), dict(mode="seg"), dict(lights=dict(reach=65)), dict(lights=dict(glow=1.0)), dict(ambient=20.0), dict(relief=-1.0),
                dict(flip=(True,)), dict(match_input_res=False), dict(mode="depth", depth=maps)):
        with pytest.raises(ValueError):
            pipe.relight_batch_device(image, **bad)
    with pytest.raises(ValueError):
        pipe.relight_batch_device(image.float())
    samples = [["set0/im/0000.png"]]
    for bad in (dict(mode="matting"), dict(lights=dict(reach=65)), dict(sweep=0), dict(sweep=2.5), dict(animate="gif"), dict(sweep=3, animate="mp4"),
                dict(flip=(True,)), dict(ambient=-1.0), dict(relief=0.0)):
        with pytest.raises(ValueError):
            ie.run_relight(pipe, str(tmp_path), samples, str(tmp_path / "out"), ie.FileNameMode.id, **bad)
    assert library_calls == []


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    from genpercept_amd import engine, infer_eval
    from genpercept_amd.pipeline import GenPerceptPipeline
    hdr, math_h = ps.assert_entries_bound(["gp_relight"], "relight.hip", "relight_math.h")
    res, args = engine.SYMBOLS["gp_relight"]
    assert res is C.c_int and len(args) == 18 and args[7:15] == [C.c_int] * 8 and args[:7] == [C.c_void_p] * 7
    assert callable(engine.relight) and callable(infer_eval.run_relight)
    assert callable(GenPerceptPipeline.relight_batch_device) and callable(GenPerceptPipeline.relight)
    assert "hip_runtime" not in math_h and "orthographic" in hdr and "gp_relight        (no reference code)" in hdr
    for name in ("gs_quant16",):                                                                          # reused, not copied
        assert not any(line.lstrip().startswith(("RL_HD", "GS_HD")) and name + "(" in line.split("{")[0] for line in math_h.splitlines()), name


def lights_array(rows):
    """A host light table the C entry can read: the int32 array (keep it alive) and its address."""
    a = np.ascontiguousarray(np.asarray(rows, np.int32))
    return a, a.ctypes.data


def relight_args(b, h, w, rows, **ptrs):
    """A valid argument set of gp_relight for these sizes (pointers as given, small integers by default; lights is real host memory)."""
    ok = dict(image=0x1001, normal=0x2000, pred=0x3004, weight=0x4003, lights=rows, to_lin=0x5002, from_lin=0x6001, B=b, H=h, W=w, L=2, encoded=1, flip=0,
              space=0, max_reach=64, out=0x7003, shadow=0x8001)
    ok.update(ptrs)
    return ok


def valid_rows():
    from genpercept_amd import relight as rl
    return rl.relight_lights([dict(azimuth=0.0, reach=64), dict(azimuth=300.0, reach=5, specular=1.0)])    # steps (256, 0) and (148, 256)


def invalid_cases(ok, keep):
    """The argument sets gp_relight refuses, as changes to a valid set `ok` with two lights; the changed tables are appended to `keep`."""
    def table(row, col, value):
        a, ptr = lights_array(valid_rows())
        a[row, col] = value
        keep.append(a)
        return dict(lights=ptr)
    return [dict(image=None), dict(normal=None), dict(lights=None), dict(to_lin=None), dict(from_lin=None), dict(out=None),
            dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(W=-5), dict(H=16385), dict(W=16385), dict(B=8, H=16384, W=16384),   # B H W = 2^31
            dict(L=0), dict(L=9), dict(L=-1), dict(encoded=2), dict(encoded=-1), dict(flip=8), dict(flip=-1), dict(space=2), dict(space=-1),
            dict(max_reach=-1), dict(max_reach=65), dict(max_reach=63),                                                         # (a row asks for 64)
            dict(normal=ok["normal"] + 2), dict(normal=ok["normal"] + 1), dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1),
            dict(lights=ok["lights"] + 2), dict(to_lin=ok["to_lin"] + 1), dict(out=ok["image"]),
            table(0, 0, 16385), table(1, 2, -16385), table(0, 4, 16385), table(1, 6, -1), table(0, 8, 4097), table(1, 9, 4097), table(0, 12, 8),
            table(1, 12, -1), table(0, 13, 257), table(0, 13, 100), table(1, 14, -257), table(0, 15, -1), table(1, 15, 65536), table(0, 16, -1),
            table(1, 16, 65536), table(0, 17, 257), table(1, 18, 257), table(0, 18, -1), table(0, 19, 65), table(1, 19, -1), table(2, 0, -1),
            table(2, 2, 65537)]


def call_relight(lib, a):
    return lib.gp_relight(a["image"], a["normal"], a["pred"], a["weight"], a["lights"], a["to_lin"], a["from_lin"], a["B"], a["H"], a["W"], a["L"],
                          a["encoded"], a["flip"], a["space"], a["max_reach"], a["out"], a["shadow"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced; the light table, host memory, is read and refused by its values."""
    rows, ptr = lights_array(valid_rows())
    for lib in _libs():
        keep = []
        ok = relight_args(2, 40, 70, ptr)
        cases = invalid_cases(ok, keep)
        assert len(cases) == 55
        ps.assert_all_refused(call_relight, lib, ok, cases)
    assert rows.shape == (3, 20)
