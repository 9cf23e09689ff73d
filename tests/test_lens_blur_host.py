"""The synthetic depth of field on the host (genpercept_amd/lens_blur.py), without a GPU: the numpy route equals plain scalar loops written
here from the definition, and a stand-alone CPU build of the kernel's arithmetic (tests/lens_blur_check.cpp over csrc/lens_blur_math.h, built
with the ROCm clang++ under the address and undefined-behaviour sanitizers and run as a child process); the properties the definition is
for, with exact expectations; the tables and the user's terms; the entry declared, exported, bound, and its argument checks with NULL
buffers.  There is no tolerance in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs, same_bits  # noqa: E402,F401

# H, W, (F, gain, cmax8, dz)
CASES = [(9, 13, (30000, 2000, 24, 0)), (17, 11, (50000, 700, 40, 3000)), (7, 9, (0, 32768, 256, 0)), (5, 23, (65535, 300, 13, 100))]


def random_case(rng, h, w, nan=True):
    """One image: (pred float32 [h, w] of two or three noisy planes, values beyond [0, 1] and NaNs among them; image uint8 [3, h, w]; sharp
    uint8 [h, w])."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pred = 0.15 + 0.2 * xx / w + 0.1 * yy / h
    cut = rng.randint(1, max(2, w - 1))
    pred[:, cut:] = 0.8 - 0.3 * yy[:, cut:] / h
    if h > 4:
        pred[h // 2:, : max(1, cut // 2)] = 0.5
    pred += rng.uniform(-0.02, 0.02, (h, w))
    pred[rng.rand(h, w) < 0.03] = 1.2
    pred[rng.rand(h, w) < 0.03] = -0.1
    if nan:
        pred[rng.rand(h, w) < 0.04] = np.nan
    image = rng.randint(0, 256, (3, h, w)).astype(np.uint8)
    image[:, :, cut:] //= 3
    sharp = (rng.rand(h, w) < 0.15).astype(np.uint8) * rng.randint(1, 256, (h, w)).astype(np.uint8)
    return pred.astype(np.float32), image, sharp


def all_tables():
    from genpercept_amd import lens_blur as lb
    return dict(srgb=lb.srgb_tables(), identity=lb.identity_tables())


# ---- the definition once more, in plain loops ---------------------------------------------------------------------------------------------------------
def loops_disc_count(c):
    return sum(1 for dy in range(-33, 34) for dx in range(-33, 34) if 64 * (dx * dx + dy * dy) <= (c + 4) ** 2)


_COUNTS = {}


def loops_weight(c):
    if c not in _COUNTS:
        _COUNTS[c] = (1 << 20) // loops_disc_count(c)
    return _COUNTS[c]


def loops_lens_blur(image, pred, row, space, sharp, tables):
    to_lin, from_lin = tables
    F, gain, cmax8, dz = (int(v) for v in row)
    _, h, w = image.shape
    D, c = [[0] * w for _ in range(h)], [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            v = np.float32(pred[y, x])
            if np.isnan(v):
                continue
            cl = np.float32(1.0) if v >= np.float32(1.0) else (v if v > np.float32(0.0) else np.float32(0.0))
            q = int(np.float32(cl * np.float32(65535.0)))
            D[y][x] = q if space == "disparity" else 65535 - q
            if sharp is None or sharp[y, x] == 0:
                c[y][x] = min(cmax8, (max(0, abs(D[y][x] - F) - dz) * gain + 32768) >> 16)
    out = np.zeros((3, h, w), np.uint8)
    reach = (max(max(r) for r in c) + 4) // 8
    for y in range(h):
        for x in range(w):
            sw, s = 0, [0, 0, 0]
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < h and 0 <= xx < w):
                        continue
                    r = c[yy][xx] if D[yy][xx] >= D[y][x] else min(c[yy][xx], c[y][x])
                    if 64 * (dx * dx + dy * dy) <= (r + 4) ** 2:
                        wt = loops_weight(r)
                        sw += wt
                        for k in range(3):
                            s[k] += wt * int(to_lin[image[k, yy, xx]])
            for k in range(3):
                out[k, y, x] = from_lin[(2 * s[k] + sw) // (2 * sw)]
    return out, np.array(c, np.uint16)


@pytest.mark.parametrize("space", ["depth", "disparity"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%d" % s[:2])
def test_host_route_equals_plain_loops(case, space):
    from genpercept_amd import lens_blur as lb
    h, w, row = case
    pred, image, sharp = random_case(np.random.RandomState(11 * h + w), h, w)
    for name, tables in all_tables().items():
        for use_sharp in (False, True):
            got, coc = lb.lens_blur_params(image, pred[None], row, space, sharp[None] if use_sharp else None, tables, want_coc=True)
            want, want_coc = loops_lens_blur(image, pred, row, space, sharp if use_sharp else None, tables)
            assert same_bits(coc[0], want_coc) and same_bits(got[0], want), (case, space, name, use_sharp)
            assert coc.max() > 4 and not same_bits(got[0], image)


def test_disc_sizes():
    from genpercept_amd import lens_blur as lb
    for c, n in ((0, 1), (3, 1), (4, 5), (8, 9), (16, 21), (64, 225), (256, 3313)):
        assert lb.disc_count(c) == n == loops_disc_count(c)
    w = lb.disc_weights()
    assert w.shape == (257,) and w[256] == 316 and w[0] == 1 << 20 and all(w[c] == (1 << 20) // lb.disc_count(c) for c in range(257))
    assert (np.diff(w) <= 0).all()


# ---- the kernel's arithmetic on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "lens_blur_check.cpp", extra_flags=())   # (the one program built without -ffp-contract=off)


@pytest.mark.parametrize("case", CASES + [(40, 70, (20000, 4000, 64, 500)), (33, 50, (40000, 32768, 256, 0))], ids=lambda s: "%dx%d" % s[:2])
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    from genpercept_amd import lens_blur as lb
    h, w, row = case
    pred, image, sharp = random_case(np.random.RandomState(7 * h + w), h, w)
    tables = all_tables()
    k = 0
    for sp, space in enumerate(lb.SPACES):
        for use_sharp, name in ((False, "srgb"), (True, "identity")):
            k += 1
            src, dst = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
            to_lin, from_lin = tables[name]
            with open(src, "wb") as f:
                f.write(np.array([h, w, sp, use_sharp] + list(row), np.int32).tobytes() + to_lin.astype(np.uint16).tobytes() + from_lin.tobytes()
                        + pred.tobytes() + image.tobytes() + (sharp.tobytes() if use_sharp else b""))
            raw, hw = ps.run_check(check_exe, src, dst, timeout=120)[1], h * w
            assert len(raw) == 5 * hw + 4 * 257
            want, coc = lb.lens_blur_params(image, pred, row, space, sharp if use_sharp else None, tables[name], want_coc=True)
            assert same_bits(np.frombuffer(raw[:3 * hw], np.uint8).reshape(3, h, w), want[0]), (case, space, name)
            assert same_bits(np.frombuffer(raw[3 * hw:5 * hw], np.uint16).reshape(h, w), coc[0]), (case, space, name)
            assert same_bits(np.frombuffer(raw[5 * hw:], np.uint32).astype(np.int64), lb.disc_weights())


# ---- what the definition is for -----------------------------------------------------------------------------------------------------------------------
def two_planes(h=40, w=48, edge=21, near=0.2, far=0.9, seed=3):
    """depth space: a near plane left of column `edge`, a far plane right of it, a random image"""
    pred = np.full((1, 1, h, w), far, np.float32)
    pred[..., :edge] = near
    image = np.random.RandomState(seed).randint(0, 256, (1, 3, h, w)).astype(np.uint8)
    return pred, image


def test_everything_in_focus_returns_the_input_bytes():
    from genpercept_amd import lens_blur as lb
    pred, image, sharp = random_case(np.random.RandomState(1), 20, 30)
    for tables in all_tables().values():
        for kw in (dict(aperture=0.0, focus=0.3), dict(max_radius=0.0, focus=0.3), dict(dof=1.0, focus=0.5), dict(focus=0.3, sharp=np.ones((1, 20, 30), bool)),
                   dict(aperture=0.375, focus=0.0)):     # (gain 3: c <= 3 everywhere, a disc of one pixel)
            out, coc = lb.lens_blur(image, pred, tables=tables, want_coc=True, **kw)
            assert same_bits(out[0], image) and coc.max() <= 3, kw
    out, coc = lb.lens_blur(image, np.full((1, 1, 20, 30), np.nan, np.float32), focus=0.0, aperture=32.0, max_radius=32.0, want_coc=True)
    assert same_bits(out[0], image) and not coc.any()                                                 # a map of NaNs blurs nothing


def test_a_constant_colour_stays():
    from genpercept_amd import lens_blur as lb
    pred, _, sharp = random_case(np.random.RandomState(2), 24, 31)
    for tables in all_tables().values():
        for colour in ((0, 0, 0), (255, 255, 255), (17, 200, 93)):
            image = np.broadcast_to(np.array(colour, np.uint8)[:, None, None], (3, 24, 31)).copy()
            for space in lb.SPACES:
                out, coc = lb.lens_blur(image, pred, focus=0.3, aperture=40.0, max_radius=9.0, space=space, sharp=sharp, tables=tables, want_coc=True)
                assert same_bits(out[0], image) and coc.max() == 72


@pytest.mark.parametrize("c8", [0, 3, 4, 8, 16, 64, 100])
def test_one_bright_pixel_becomes_its_disc(c8):
    """All at one radius c away from the border: the byte-255 pixel spreads over exactly the n(c) pixels of its disc, at w(c) * 4095 each."""
    from genpercept_amd import lens_blur as lb
    h = w = 4 * ((c8 + 4) // 8) + 3
    image = np.zeros((1, 3, h, w), np.uint8)
    image[0, :, h // 2, w // 2] = 255
    pred = np.full((1, 1, h, w), 0.5, np.float32)
    n = lb.disc_count(c8)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = 64 * ((yy - h // 2) ** 2 + (xx - w // 2) ** 2) <= (c8 + 4) ** 2
    assert disc.sum() == n
    for tables in all_tables().values():
        to_lin, from_lin = tables
        top = int(to_lin[255])
        # a uniform radius: the focus at the far end, the largest gain, and cmax8 = c8 caps every pixel at c8; no disc the bright pixel lies in
        # is clipped by the border
        out, coc = lb.lens_blur_params(image, pred, (0, 32768, c8, 0), "disparity", tables=tables, want_coc=True)
        assert (coc == c8).all()
        wt = (1 << 20) // n
        value = from_lin[(2 * wt * top + n * wt) // (2 * n * wt)]
        assert value == from_lin[(2 * top + n) // (2 * n)]
        want = np.where(disc, value, from_lin[0]).astype(np.uint8)
        assert all(same_bits(out[0, k], want) for k in range(3)), c8


def test_a_sharp_near_plane_does_not_take_the_blurred_background():
    from genpercept_amd import lens_blur as lb
    pred, image = two_planes()
    edge, radius = 21, 6
    kw = dict(focus=0.2, aperture=64.0, max_radius=float(radius))
    out, coc = lb.lens_blur(image, pred, want_coc=True, **kw)
    assert not coc[0, :, :edge].any() and (coc[0, :, edge:] == 8 * radius).all()
    assert same_bits(out[0, :, :, :edge], image[0, :, :, :edge])                                       # no bleed: every near byte is untouched
    uniform = lb.lens_blur(image, np.full_like(pred, 0.9), **kw)                                      # the far plane alone, everywhere
    far = edge + radius + 1                                                                           # (the reach is (48 + 4) / 8 = 6 pixels)
    assert same_bits(out[0, :, :, far:], uniform[0, :, :, far:])
    assert not same_bits(out[0, :, :, edge:far], uniform[0, :, :, edge:far])                          # next to the edge the near plane occludes


def test_a_blurred_near_plane_spreads_over_the_sharp_background():
    from genpercept_amd import lens_blur as lb
    pred, image = two_planes()
    edge, radius = 21, 6
    out, coc = lb.lens_blur(image, pred, focus=0.9, aperture=64.0, max_radius=float(radius), want_coc=True)
    assert (coc[0, :, :edge] == 8 * radius).all() and not coc[0, :, edge:].any()
    assert same_bits(out[0, :, :, edge + radius:], image[0, :, :, edge + radius:])                    # beyond the reach the far plane is untouched
    changed = (out[0, :, :, edge:edge + radius] != image[0, :, :, edge:edge + radius]).any(0)
    assert changed.any(0).all()                                                                      # within it the foreground spreads: every column


def test_flipping_the_inputs_flips_the_output():
    from genpercept_amd import lens_blur as lb
    pred, image, sharp = random_case(np.random.RandomState(5), 21, 34)
    for space in lb.SPACES:
        kw = dict(focus=0.25, aperture=30.0, max_radius=5.5, dof=0.02, space=space, want_coc=True)
        out, coc = lb.lens_blur(image, pred, sharp=sharp, **kw)
        fout, fcoc = lb.lens_blur(image[:, ::-1, ::-1].copy(), pred[::-1, ::-1].copy(), sharp=sharp[::-1, ::-1].copy(), **kw)
        assert same_bits(fout[0, :, ::-1, ::-1], out[0]) and same_bits(fcoc[0, ::-1, ::-1], coc[0]) and coc.max() == 44


def test_sharp_dz_nan_and_spaces():
    from genpercept_amd import lens_blur as lb
    pred, image, sharp = random_case(np.random.RandomState(6), 18, 26)
    kw = dict(focus=0.2, aperture=20.0, max_radius=4.0)
    out, coc = lb.lens_blur(image, pred, want_coc=True, **kw)
    pinned, pcoc = lb.lens_blur(image, pred, sharp=sharp, want_coc=True, **kw)
    assert not pcoc[0][sharp != 0].any() and same_bits(pcoc[0][sharp == 0], coc[0][sharp == 0]) and not same_bits(pinned, out)
    assert not coc[0][np.isnan(pred)].any() and np.isnan(pred).any()
    # dof widens the sharp zone: c is the c of the distance less dz
    D = lb.nearness(pred, "depth")
    F, gain, cmax8, dz = lb.lens_params(pred[None, None], "depth", dof=0.1, **kw)[0]
    assert (F, gain, cmax8, dz) == (65535 - int(np.float32(0.2) * np.float32(65535.0)), 160, 32, 6554)
    _, wcoc = lb.lens_blur(image, pred, dof=0.1, want_coc=True, **kw)
    want = np.where(np.isnan(pred), 0, np.minimum(32, (np.maximum(0, np.abs(D - F) - 6554) * 160 + 32768) >> 16))
    assert same_bits(wcoc[0], want.astype(np.uint16)) and (wcoc <= coc).all() and (wcoc < coc).any()
    # the spaces read the map in opposite directions: 1 - pred in the other space has the same nearness up to the rounding of the quantiser
    assert same_bits(lb.nearness(np.float32([0.0, 1.0, 0.25, np.nan, 2.0, -1.0]), "depth"), np.array([65535, 0, 65535 - 16383, 0, 0, 65535]))
    assert same_bits(lb.nearness(np.float32([0.0, 1.0, 0.25, np.nan, 2.0, -1.0]), "disparity"), np.array([0, 65535, 16383, 0, 65535, 0]))
    other = lb.lens_blur(image, pred, space="disparity", **kw)
    assert not same_bits(other, out)
    # focus_at is the focus of that pixel's value; a NaN pixel has the nearness 0
    v, u = 3, 7
    assert not np.isnan(pred[v, u])
    for space in lb.SPACES:
        assert same_bits(lb.lens_blur(image, pred, focus_at=(u, v), aperture=20.0, space=space),
                         lb.lens_blur(image, pred, focus=float(pred[v, u].clip(0, 1)), aperture=20.0, space=space))
    holes = pred.copy()
    holes[v, u] = np.nan
    assert lb.lens_params(holes[None, None], "depth", focus_at=(u, v))[0, 0] == 0


def test_tables_and_terms_are_checked():
    from genpercept_amd import lens_blur as lb
    for to_lin, from_lin in all_tables().values():
        assert to_lin.dtype == np.uint16 and from_lin.dtype == np.uint8 and to_lin.shape == (256,) and from_lin.shape == (4096,)
        assert (np.diff(to_lin.astype(int)) > 0).all() and to_lin.max() <= 4095 and same_bits(from_lin[to_lin], np.arange(256, dtype=np.uint8))
        assert (np.diff(from_lin.astype(int)) >= 0).all()
        lb.check_tables((to_lin, from_lin))
    to_lin, from_lin = lb.srgb_tables()
    assert to_lin[0] == 0 and to_lin[255] == 4095 and to_lin[128] == round(4095 * ((128 / 255 + 0.055) / 1.055) ** 2.4)
    ident = lb.identity_tables()
    assert same_bits(ident[0], np.arange(256, dtype=np.uint16)) and same_bits(ident[1], np.minimum(np.arange(4096), 255).astype(np.uint8))
    flat, high, wrong = to_lin.copy(), to_lin.astype(np.int64), from_lin.copy()
    flat[10] = flat[9]
    high[255] = 4096
    wrong[to_lin[77]] = 78
    for bad in ((flat, from_lin), (high, from_lin), (to_lin, wrong), (to_lin[:255], from_lin), (to_lin, from_lin[:4095]), (to_lin.astype(float), from_lin),
                to_lin, (to_lin[::-1], from_lin)):
        with pytest.raises(ValueError):
            lb.check_tables(bad)
    pred, image, sharp = random_case(np.random.RandomState(8), 10, 12)
    ok = dict(focus=0.5)
    for bad in (dict(), dict(focus=0.5, focus_at=(1, 1)), dict(focus=1.5), dict(focus=-0.1), dict(focus=float("nan")), dict(focus=None, focus_at=(12, 0)),
                dict(focus=None, focus_at=(0, 10)), dict(focus=None, focus_at=(-1, 0)), dict(focus=None, focus_at=(0.5, 0)), dict(focus=None, focus_at=3),
                dict(aperture=-1.0), dict(aperture=4097.0), dict(max_radius=32.5), dict(max_radius=-0.1), dict(dof=-0.1), dict(dof=1.1), dict(space="metric"),
                dict(focus=[0.5, 0.5]), dict(sharp=sharp[:5]), dict(sharp=sharp.astype(float)), dict(tables=(flat, from_lin))):
        with pytest.raises(ValueError):
            lb.lens_blur(image, pred, **(bad if not bad else dict(ok, **bad)))
    for bad in (dict(image=image.astype(np.float32)), dict(image=image[:2]), dict(pred=pred[:5]), dict(pred=np.zeros_like(pred, np.uint8))):
        with pytest.raises(ValueError):
            lb.lens_blur(**dict(dict(image=image, pred=pred, focus=0.5), **bad))
    for bad in ((-1, 0, 0, 0), (65536, 0, 0, 0), (0, 32769, 0, 0), (0, 0, 257, 0), (0, 0, 0, 65536), (0, 0, 0), np.zeros((2, 4), int), np.zeros(4)):
        with pytest.raises(ValueError):
            lb.lens_blur_params(image, pred, bad)
    # one value per image
    two = lb.lens_params(np.stack([pred, pred])[:, None], "disparity", focus=[0.25, 1.0], aperture=[2.0, 4096.0], max_radius=32.0, dof=[0.0, 1.0])
    assert two.dtype == np.int32 and two.tolist() == [[16383, 16, 256, 0], [65535, 32768, 256, 65535]]
    o = lb.lens_blur_options(3, focus_at=(4, 5))
    assert o["focus"] is None and o["focus_at"].tolist() == [[4, 5]] * 3 and o["gain"].tolist() == [64] * 3 and o["cmax8"].tolist() == [128] * 3


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    from genpercept_amd import engine, infer_eval
    from genpercept_amd.pipeline import GenPerceptPipeline
    hdr, math_h = ps.assert_entries_bound(("gp_lens_blur",), "lens_blur.hip", "lens_blur_math.h", contract_off=False)
    args = engine.SYMBOLS["gp_lens_blur"][1]
    assert len(args) == 14 and args[6:11] == [C.c_int] * 5 and engine.SYMBOLS["gp_lens_blur"][0] is C.c_int
    assert callable(engine.lens_blur) and callable(infer_eval.run_refocus)
    assert callable(GenPerceptPipeline.refocus_batch_device) and callable(GenPerceptPipeline.refocus)
    assert "hip_runtime" not in math_h and "thin-lens" in hdr


def lens_args(b, h, w, **ptrs):
    """A valid argument set of gp_lens_blur for these sizes (pointers as given, small integers by default)."""
    ok = dict(image=0x1001, pred=0x2000, sharp=0x3003, params=0x4000, to_lin=0x5002, from_lin=0x6001, B=b, H=h, W=w, space=0, max_c8=64, out=0x7003,
              coc=0x8002)
    ok.update(ptrs)
    return ok


def invalid_cases(ok):
    """The argument sets gp_lens_blur refuses, as changes to a valid set `ok`."""
    return [dict(image=None), dict(pred=None), dict(params=None), dict(to_lin=None), dict(from_lin=None), dict(out=None),
            dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(W=-5), dict(H=16385), dict(W=16385), dict(B=8, H=16384, W=16384),   # B H W = 2^31
            dict(space=2), dict(space=-1), dict(max_c8=-1), dict(max_c8=257), dict(max_c8=1 << 20),
            dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1), dict(params=ok["params"] + 2), dict(params=ok["params"] + 1),
            dict(to_lin=ok["to_lin"] + 1), dict(coc=ok["coc"] + 1), dict(out=ok["image"])]


def call_lens(lib, a):
    return lib.gp_lens_blur(a["image"], a["pred"], a["sharp"], a["params"], a["to_lin"], a["from_lin"], a["B"], a["H"], a["W"], a["space"], a["max_c8"],
                            a["out"], a["coc"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        ok = lens_args(2, 40, 70)
        cases = invalid_cases(ok)
        assert len(cases) == 26
        ps.assert_all_refused(call_lens, lib, ok, cases)
