"""Matting cutouts (gp_foreground), the host half: the level sizes; genpercept_amd/foreground.py (vectorised numpy) bit-equal to a plain
triple-loop np.float32 scalar implementation written here from the definition; tests/foreground_check.cpp, a stand-alone CPU program that runs
the whole multi-level loop over the kernels' own update text (csrc/foreground_update.h, contraction off, under AddressSanitizer and UBSan),
bit-equal to the host route; the quality of the estimate on a synthetic composite with known colours; degenerate alphas; the header, the two
libraries and the ctypes table carry the new entry; its argument checks (they come before the first HIP call, so they run without a GPU)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs  # noqa: E402,F401

NAMES = ("gp_foreground_workspace", "gp_foreground")
f32 = np.float32
same_bits = functools.partial(ps.same_bits, dtype=np.float32)


def random_inputs(rng, h, w):
    """A uint8 image [3, H, W] of random blocks and noise, an alpha of plateaus of 0 and 255 with every kind of byte sprinkled in."""
    img = rng.randint(0, 256, (3, h, w)).astype(np.uint8)
    if h > 2 and w > 2:
        y, x = rng.randint(0, h - 1), rng.randint(0, w - 1)
        img[:, y:y + rng.randint(1, h), x:x + rng.randint(1, w)] = rng.randint(0, 256, (3, 1, 1))
    a = np.where(rng.rand(h, w) < 0.5, 0, 255).astype(np.uint8)
    if h > 2 and w > 2:
        y, x = rng.randint(0, h - 1), rng.randint(0, w - 1)
        a[y:y + rng.randint(1, h), x:x + rng.randint(1, w)] = rng.choice([0, 255])
    sel = rng.rand(h, w) < 0.3
    a[sel] = rng.randint(0, 256, int(sel.sum()))
    return img, a


def synthetic_composite(h, w):
    """A soft disc of alpha over a reddish foreground with a horizontal gradient and a bluish background with a vertical gradient, composited
    and rounded to bytes: (image uint8 [3, H, W], alpha uint8 [H, W], F_true float32 [3, H, W])."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r = np.hypot(yy - 0.5 * (h - 1), xx - 0.5 * (w - 1))
    soft = 0.15 * min(h, w)
    alpha = np.clip((0.35 * min(h, w) - r) / soft + 0.5, 0.0, 1.0)
    a8 = np.floor(alpha * 255.0 + 0.5).astype(np.uint8)
    gx, gy = xx / max(w - 1, 1), yy / max(h - 1, 1)
    fg = np.stack([0.75 + 0.2 * gx, 0.15 + 0.2 * gx, 0.1 + 0.1 * gx])
    bg = np.stack([0.1 + 0.1 * gy, 0.25 + 0.2 * gy, 0.65 + 0.3 * gy])
    a = a8.astype(np.float64) / 255.0
    img = np.floor((a * fg + (1.0 - a) * bg) * 255.0 + 0.5).astype(np.uint8)
    return img, a8, fg.astype(np.float32)


# ---- the definition as plain loops ---------------------------------------------------------------------------------------------------------------
def loops_foreground(image_u8, a8, reg=1e-5, gw=1.0, n_small=10, n_big=2):
    """The definition of include/genpercept_hip.h, literally: np.float32 scalars, one pixel, one neighbour, one channel at a time."""
    H, W = a8.shape
    reg, gw = f32(reg), f32(gw)
    L = 0
    while (1 << L) < max(H, W):
        L += 1
    zero, one, c255 = f32(0.0), f32(1.0), f32(255.0)
    F = B = None
    hp = wp = 1
    for l in range(L + 1):
        hl, wl = (H + (1 << (L - l)) - 1) >> (L - l), (W + (1 << (L - l)) - 1) >> (L - l)
        I = [[[f32(image_u8[c, (y * H) // hl, (x * W) // wl]) / c255 for c in range(3)] for x in range(wl)] for y in range(hl)]
        a = [[f32(a8[(y * H) // hl, (x * W) // wl]) / c255 for x in range(wl)] for y in range(hl)]
        if l == 0:
            F, B = [[list(I[0][0])]], [[list(I[0][0])]]
        else:
            F = [[list(F[(y * hp) // hl][(x * wp) // wl]) for x in range(wl)] for y in range(hl)]
            B = [[list(B[(y * hp) // hl][(x * wp) // wl]) for x in range(wl)] for y in range(hl)]
        for _ in range(n_small if hl <= 32 and wl <= 32 else n_big):
            Fo, Bo = F, B
            F = [[None] * wl for _ in range(hl)]
            B = [[None] * wl for _ in range(hl)]
            for y in range(hl):
                for x in range(wl):
                    ap, Ip = a[y][x], I[y][x]
                    a1 = one - ap
                    a00, a01, a11 = ap * ap, ap * a1, a1 * a1
                    b0, b1 = [ap * Ip[c] for c in range(3)], [a1 * Ip[c] for c in range(3)]
                    for ny, nx in ((y, max(x - 1, 0)), (y, min(x + 1, wl - 1)), (max(y - 1, 0), x), (min(y + 1, hl - 1), x)):
                        da = reg + gw * abs(ap - a[ny][nx])
                        a00, a11 = a00 + da, a11 + da
                        for c in range(3):
                            b0[c] = b0[c] + da * Fo[ny][nx][c]
                            b1[c] = b1[c] + da * Bo[ny][nx][c]
                    det = a00 * a11 - a01 * a01
                    assert det > 0 and type(det) is np.float32
                    inv = one / det
                    fo, bo = [], []
                    for c in range(3):
                        v = inv * (a11 * b0[c] - a01 * b1[c])
                        v = v if v > zero else zero
                        fo.append(v if v < one else one)
                        v = inv * (a00 * b1[c] - a01 * b0[c])
                        v = v if v > zero else zero
                        bo.append(v if v < one else one)
                    F[y][x], B[y][x] = fo, bo
        hp, wp = hl, wl
    return (np.array(F, dtype=np.float32).transpose(2, 0, 1).copy(), np.array(B, dtype=np.float32).transpose(2, 0, 1).copy())


# ---- level sizes -----------------------------------------------------------------------------------------------------------------------------------
def test_level_sizes():
    from genpercept_amd.foreground import level_sizes
    assert level_sizes(1, 1) == [(1, 1)]
    assert level_sizes(1, 2) == [(1, 1), (1, 2)]
    assert level_sizes(33, 32) == [(1, 1), (2, 1), (3, 2), (5, 4), (9, 8), (17, 16), (33, 32)]
    assert level_sizes(37, 300) == [(1, 1), (1, 2), (1, 3), (1, 5), (2, 10), (3, 19), (5, 38), (10, 75), (19, 150), (37, 300)]
    big = level_sizes(4032, 6048)
    assert len(big) == 14 and big[-2] == (2016, 3024) and big[-3] == (1008, 1512) and big[1] == (1, 2) and big[2] == (2, 3)
    for h, w in ((1, 1), (1, 2), (33, 32), (37, 300), (4032, 6048), (16384, 1), (5, 16384)):
        s = level_sizes(h, w)
        assert s[0] == (1, 1) and s[-1] == (h, w)
        assert all(p[0] <= q[0] and p[1] <= q[1] for p, q in zip(s, s[1:]))
        assert len(s) == 1 + int(np.ceil(np.log2(max(h, w)))) if max(h, w) > 1 else len(s) == 1
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError):
            level_sizes(*bad)


# ---- host route against loops -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (7, 5), (33, 32), (37, 70)], ids=lambda s: "x".join(map(str, s)))
def test_host_route_equals_plain_loops(shape):
    from genpercept_amd import foreground as fgh
    h, w = shape
    rng = np.random.RandomState(100 + h)
    img, a8 = random_inputs(rng, h, w)
    for kw in (dict(), dict(reg=3e-4, gw=7.5, n_small=3, n_big=4)) if h < 37 else (dict(),):
        F, B = fgh.estimate_foreground(img, a8, **kw)
        Fl, Bl = loops_foreground(img, a8, **kw)
        assert F.shape == (3, h, w) and same_bits(F, Fl) and same_bits(B, Bl), (shape, kw)


# ---- the kernels' update text on the CPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "foreground_check.cpp")


@pytest.mark.parametrize("shape", [(7, 5), (33, 32), (37, 70)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_build_of_the_kernel_update_equals_the_host_route(check_exe, shape, tmp_path):
    from genpercept_amd import foreground as fgh
    h, w = shape
    rng = np.random.RandomState(200 + h)
    img, a8 = random_inputs(rng, h, w)
    for n, kw in enumerate((dict(reg=1e-5, gw=1.0, n_small=10, n_big=2), dict(reg=1e-6, gw=100.0, n_small=1, n_big=3))):
        src, dst = str(tmp_path / f"in{n}.bin"), str(tmp_path / f"out{n}.bin")
        with open(src, "wb") as f:
            f.write(np.array([h, w, kw["n_small"], kw["n_big"]], np.int32).tobytes() + np.array([kw["reg"], kw["gw"]], np.float32).tobytes())
            f.write(img.tobytes() + a8.tobytes())
        lines, raw = ps.run_check(check_exe, src, dst)
        got = np.frombuffer(raw, np.float32).reshape(2, 3, h, w)
        F, B = fgh.estimate_foreground(img, a8, **kw)
        assert same_bits(got[0], F) and same_bits(got[1], B), (shape, kw)
        want = [int(v) for v in fgh.to_bytes(np.array([0.0, 0.5, 1.0, f32(0.25) * f32(1.0) + (f32(1.0) - f32(0.25)) * f32(0.2)], np.float32))]
        assert [int(v) for v in lines[0].split()] == want == [0, 128, 255, 102]


# ---- quality ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 65), (300, 203)], ids=lambda s: "x".join(map(str, s)))
def test_quality_on_a_synthetic_composite(shape):
    from genpercept_amd import foreground as fgh
    img, a8, f_true = synthetic_composite(*shape)
    stats = {}
    F, B = fgh.estimate_foreground(img, a8, stats=stats)
    assert stats["det_min"] > 0
    band = (a8 >= 26) & (a8 < 230)
    assert band.sum() > 100
    I = img.astype(np.float32) / f32(255.0)
    err = float(np.abs(F - f_true)[:, band].mean())
    err_image = float(np.abs(I - f_true)[:, band].mean())
    a = a8.astype(np.float32) / f32(255.0)
    recon = float(np.abs(a * F + (1 - a) * B - I).max())
    print(f"foreground quality {shape}: band-mean |F - F_true| {err:.4f}, with F = I {err_image:.4f}, reconstruction {recon:.5f}, "
          f"det_min {stats['det_min']:.3e}")
    assert err <= err_image / 5
    assert recon <= 0.01


def test_degenerate_alpha():
    from genpercept_amd import foreground as fgh
    rng = np.random.RandomState(9)
    img, _ = random_inputs(rng, 40, 53)
    I = img.astype(np.float32) / f32(255.0)
    F, _ = fgh.estimate_foreground(img, np.full((40, 53), 255, np.uint8))
    assert np.abs(F - I).max() <= 1e-3
    _, B = fgh.estimate_foreground(img, np.zeros((40, 53), np.uint8))
    assert np.abs(B - I).max() <= 1e-3


def test_cutout_and_composite_follow_the_definition():
    from genpercept_amd import foreground as fgh
    rng = np.random.RandomState(10)
    img, a8 = random_inputs(rng, 21, 34)
    F, _ = fgh.estimate_foreground(img, a8)
    rgba = fgh.cutout_rgba(img, a8)
    assert rgba.shape == (21, 34, 4) and rgba.dtype == np.uint8 and np.array_equal(rgba[..., 3], a8)
    assert np.array_equal(rgba[..., :3], np.minimum((F * f32(255.0) + f32(0.5)).astype(np.int32), 255).transpose(1, 2, 0))
    # a float alpha is quantised first, as the saved byte is
    assert np.array_equal(fgh.cutout_rgba(img, a8.astype(np.float32) / f32(255.0) + f32(0.001)), rgba)
    a = a8.astype(np.float32) / f32(255.0)
    new = rng.randint(0, 256, (3, 21, 34)).astype(np.uint8)
    for N in (new, np.array([10, 200, 255], np.uint8)):
        Nf = np.broadcast_to(N.reshape(3, 1, 1) if N.ndim == 1 else N, (3, 21, 34)).astype(np.float32) / f32(255.0)
        want = np.minimum(((a * F + (f32(1.0) - a) * Nf) * f32(255.0) + f32(0.5)).astype(np.int32), 255).astype(np.uint8)
        assert np.array_equal(fgh.composite(img, a8, N), want)
    opaque = fgh.composite(img, np.full((21, 34), 255, np.uint8), new)
    assert np.abs(opaque.astype(int) - img.astype(int)).max() <= 1
    for bad in (dict(reg=1e-7), dict(reg=1.5), dict(gw=-1.0), dict(gw=101.0), dict(n_small=65), dict(n_small=-1), dict(n_big=0), dict(n_big=5)):
        with pytest.raises(ValueError):
            fgh.estimate_foreground(img, a8, **bad)
    with pytest.raises(ValueError):
        fgh.estimate_foreground(img[:2], a8)
    with pytest.raises(ValueError):
        fgh.composite(img, a8, np.zeros((3, 4, 4), np.uint8))


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    ps.assert_entries_bound(NAMES, "foreground.hip")
    assert len(engine.SYMBOLS["gp_foreground"][1]) == 19 and engine.SYMBOLS["gp_foreground_workspace"] == (C.c_longlong, [C.c_int] * 3)
    assert callable(engine.estimate_foreground) and callable(engine.cutout) and callable(engine.foreground)


def test_workspace_size():
    from genpercept_amd.foreground import level_sizes
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 16385, 8), (1, 8, 16385)):
            assert lib.gp_foreground_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (1031, 2053), (16384, 16384)):
            s = level_sizes(h, w)
            need = 24 * sum(p[0] * p[1] for p in s[:-1][-2:])      # F and B of the two levels below the last one
            one = lib.gp_foreground_workspace(1, h, w)
            assert max(need, 8) == one and one % 8 == 0
            assert lib.gp_foreground_workspace(7, h, w) == 7 * one


def invalid_cases(ok, need_one):
    """The argument sets gp_foreground refuses, as changes to a valid set `ok`."""
    huge = 1 << 62
    nan = float("nan")
    return [dict(image=None), dict(alpha=None), dict(ws=None), dict(fg=None, bg=None, rgba=None, comp=None),
            dict(B=0), dict(B=-3), dict(B=65536, nbytes=huge), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
            dict(H=16385, nbytes=huge), dict(W=16385, nbytes=huge), dict(H=1 << 20, W=1 << 20, nbytes=huge),
            dict(u8=-1), dict(u8=2), dict(u8=0, alpha=ok["alpha"] + 2),
            dict(reg=0.0), dict(reg=9e-7), dict(reg=1.001), dict(reg=-1e-5), dict(reg=nan), dict(gw=-0.5), dict(gw=100.5), dict(gw=nan),
            dict(n_big=0), dict(n_big=5), dict(n_big=-1), dict(n_small=-1), dict(n_small=65),
            dict(rgb=-1), dict(rgb=1 << 24), dict(fg=ok["fg"] + 2), dict(bg=ok["bg"] + 1), dict(rgba=ok["rgba"] + 3),
            dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1), dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=need_one)]


def call_foreground(lib, a):
    return lib.gp_foreground(a["image"], a["alpha"], a["u8"], a["B"], a["H"], a["W"], a["reg"], a["gw"], a["n_small"], a["n_big"], a["new_bg"], a["rgb"],
                             a["fg"], a["bg"], a["rgba"], a["comp"], a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        need = lib.gp_foreground_workspace(2, 40, 40)
        ok = dict(image=0x1001, alpha=0x2003, u8=1, B=2, H=40, W=40, reg=1e-5, gw=1.0, n_small=10, n_big=2, new_bg=None, rgb=0, fg=0x3000, bg=0x4000,
                  rgba=0x5000, comp=0x6001, ws=0x8000, nbytes=need)
        ps.assert_all_refused(call_foreground, lib, ok, invalid_cases(ok, lib.gp_foreground_workspace(1, 40, 40)))
