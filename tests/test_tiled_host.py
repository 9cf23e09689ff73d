"""Tiled high-resolution inference (gp_tile_merge), the host half: the grid rule's properties over an exhaustive sweep; genpercept_amd/tiled.py
(vectorised numpy) bit-equal to a plain scalar loop implementation written here from the definition; tests/tile_check.cpp, a stand-alone CPU
program over the kernels' own arithmetic (csrc/tile_merge_math.h, contraction off, under AddressSanitizer and UBSan), bit-equal to the host
route; tiles that are affine images of the base merge back to it; the degenerate branches of the fit; the header, the two libraries and the
ctypes table carry the new entries; their argument checks (they come before the first HIP call, so they run without a GPU)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs, q16, same_bits64  # noqa: E402,F401

NAMES = ("gp_tile_merge_workspace", "gp_tile_merge")
f32 = np.float32
# C, H, W, T, o
CASES = [(1, 9, 13, 6, 2), (3, 17, 11, 8, 4), (1, 12, 12, 12, 3), (1, 20, 7, 4, 2), (3, 5, 23, 9, 1), (1, 16, 16, 4, 2)]
same_bits = functools.partial(ps.same_bits, dtype=np.float32)


def random_case(rng, c, h, w, size, o, odd=True):
    """(base float32 [C, H, W], tiles float32 [N, C, wh, ww], ys, xs): a smooth base with noise; every tile an affine image of its window of
    the base with noise of its own; with `odd` also values outside [0, 1], a NaN in the base and one in every third tile."""
    from genpercept_amd import tiled
    ys, xs, wh, ww = tiled.tile_grid(h, w, size, o)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (0.5 + 0.3 * np.sin(yy / 5.0 + 0.3 * np.arange(c)[:, None, None]) * np.cos(xx / 7.0) + 0.05 * rng.randn(c, h, w)).astype(f32)
    tiles = []
    for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        s, t = rng.uniform(0.5, 2.0), rng.uniform(-0.25, 0.25)
        tile = ((base[:, y0:y0 + wh, x0:x0 + ww] - t) / s + 0.02 * rng.randn(c, wh, ww)).astype(f32)
        if odd and k % 3 == 1:
            tile.flat[rng.randint(tile.size)] = np.nan
        tiles.append(tile)
    tiles = np.stack(tiles)
    if odd:
        base.flat[rng.randint(base.size)] = np.nan
        base.flat[rng.randint(base.size)], base.flat[rng.randint(base.size)] = 1.5, -0.25
    return base, tiles, ys, xs


# ---- the grid rule -------------------------------------------------------------------------------------------------------------------------------
def test_grid_rule_over_an_exhaustive_sweep():
    """Every axis length up to 200, tile size up to 64 and valid overlap: the window is min(T, L), the count is the rule's, the first tile starts
    at 0, the last ends at L, the origins increase strictly (so the image is covered without a gap) and neighbours overlap by at least o."""
    from genpercept_amd import tiled
    checked = 0
    for L in range(1, 201):
        for T in range(1, 65):
            w = min(T, L)
            for o in range(1, w // 2 + 1):
                ys, got_w = tiled.axis_origins(L, T, o)
                n = 1 if L <= w else -(-(L - o) // (w - o))
                assert got_w == w and ys.dtype == np.int32 and len(ys) == n, (L, T, o)
                assert ys[0] == 0 and ys[-1] + w == L, (L, T, o)
                assert [int(v) for v in ys] == [(k * (L - w)) // (n - 1) if n > 1 else 0 for k in range(n)], (L, T, o)
                if n > 1:
                    d = np.diff(ys)
                    assert d.min() >= 1 and d.max() <= w - o, (L, T, o)  # no gap, and ys[k] + w - ys[k + 1] >= o
                    assert (n - 2) * (w - o) + w < L, (L, T, o)          # one tile fewer cannot cover L with overlaps of o
                checked += 1
            for o in (0, w // 2 + 1, -1):
                with pytest.raises(ValueError):
                    tiled.axis_origins(L, T, o)
    assert checked > 150000
    ys, xs, wh, ww = tiled.tile_grid(2048, 3072, 768, 192)
    assert (wh, ww) == (768, 768) and ys.tolist() == [0, 426, 853, 1280] and xs.tolist() == [0, 576, 1152, 1728, 2304]
    assert tiled.tile_grid(40, 100, 64, 8)[2:] == (40, 64)
    assert len(tiled.tile_grid(16384, 16384, 1024, 512)[0]) == 31 and 31 * 31 <= tiled.MAX_TILES
    for bad in ((16385, 64, 32, 8), (64, 0, 32, 8), (64, 64, 0, 1), (2000, 2000, 64, 16), (64, 64, 32, 17), (64, 64, 32, 2.0), (64.0, 64, 32, 2),
                (1, 64, 32, 1)):
        with pytest.raises(ValueError):
            tiled.tile_grid(*bad)


# ---- the definition as plain loops ---------------------------------------------------------------------------------------------------------------
def loops_fit(base, tiles, ys, xs, align):
    """The fit of the definition, literally: Python integers for the sums, Python floats (IEEE float64, one operation at a time) after them."""
    N, Cn, wh, ww = tiles.shape
    nx = len(xs)
    fits = []
    for k in range(N):
        if align == "none":
            fits.append((1.0, 0.0))
            continue
        y0, x0 = int(ys[k // nx]), int(xs[k % nx])
        n = sP = sG = sPP = sPG = 0
        for c in range(Cn):
            for y in range(wh):
                for x in range(ww):
                    P, G = q16(tiles[k, c, y, x]), q16(base[c, y0 + y, x0 + x])
                    n, sP, sG, sPP, sPG = n + 1, sP + P, sG + G, sPP + P * P, sPG + P * G
        assert sPP < 2 ** 63
        N_ = float(n)
        mp = float(sP) / N_
        mg = float(sG) / N_
        var = float(sPP) / N_ - mp * mp
        cov = float(sPG) / N_ - mp * mg
        with np.errstate(all="ignore"):
            s = float(np.float64(cov) / np.float64(var))  # (0 / 0 is NaN here, not an exception)
        if not (var >= 1.0) or not (s > 0.0):
            s = 1.0
        fits.append((s, (mg - s * mp) / 65535.0))
    return fits


def loops_merge(base, tiles, ys, xs, o, align):
    N, Cn, wh, ww = tiles.shape
    H, W = base.shape[1:]
    nx = len(xs)
    fits = loops_fit(base, tiles, ys, xs, align)
    out = np.zeros((Cn, H, W), np.float32)
    for c in range(Cn):
        for y in range(H):
            for x in range(W):
                acc, wsum = 0.0, 0
                for iy, y0 in enumerate(int(v) for v in ys):
                    for ix, x0 in enumerate(int(v) for v in xs):
                        if y0 <= y < y0 + wh and x0 <= x < x0 + ww:
                            wgt = min(y - y0 + 1, y0 + wh - y, o) * min(x - x0 + 1, x0 + ww - x, o)
                            assert wgt >= 1
                            s, t = fits[iy * nx + ix]
                            acc = acc + float(wgt) * (s * float(tiles[iy * nx + ix, c, y - y0, x - x0]) + t)
                            wsum += wgt
                q = acc / float(wsum)
                q = (q if q < 1.0 else 1.0) if q > 0.0 else 0.0
                out[c, y, x] = np.float32(q)
    return out, fits


@pytest.mark.parametrize("align", ["least_square", "none"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "c%d-%dx%d-T%d-o%d" % s)
def test_host_route_equals_plain_loops(case, align):
    from genpercept_amd import tiled
    c, h, w, size, o = case
    base, tiles, ys, xs = random_case(np.random.RandomState(100 * h + w), c, h, w, size, o)
    got = tiled.tile_merge(base, tiles, ys, xs, o, align)
    s, t = tiled.tile_fit(base, tiles, ys, xs, align)
    want, fits = loops_merge(base, tiles, ys, xs, o, align)
    assert got.shape == (c, h, w) and same_bits(got, want), (case, align)
    assert same_bits64(s, np.array([f[0] for f in fits])) and same_bits64(t, np.array([f[1] for f in fits])), (case, align)
    assert got.min() >= 0.0 and got.max() <= 1.0


# ---- the kernels' arithmetic on the CPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "tile_check.cpp")


@pytest.mark.parametrize("case", CASES + [(1, 70, 101, 32, 8), (3, 50, 77, 24, 5), (1, 33, 200, 33, 16)], ids=lambda s: "c%d-%dx%d-T%d-o%d" % s)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    from genpercept_amd import tiled
    c, h, w, size, o = case
    base, tiles, ys, xs = random_case(np.random.RandomState(7 * h + w), c, h, w, size, o)
    for a, align in enumerate(tiled.ALIGNMENTS):
        src, dst = str(tmp_path / f"in{a}.bin"), str(tmp_path / f"out{a}.bin")
        with open(src, "wb") as f:
            f.write(np.array([c, h, w, size, o, a], np.int32).tobytes() + base.tobytes() + tiles.tobytes())
        raw = ps.run_check(check_exe, src, dst)[1]
        ny, nx, wh, ww = (int(v) for v in np.frombuffer(raw[:16], np.int32))
        assert (ny, nx, wh, ww) == (len(ys), len(xs)) + tiles.shape[2:]
        pos = 16
        got_ys, got_xs = np.frombuffer(raw[pos:pos + 4 * ny], np.int32), np.frombuffer(raw[pos + 4 * ny:pos + 4 * (ny + nx)], np.int32)
        pos += 4 * (ny + nx)
        fit = np.frombuffer(raw[pos:pos + 16 * ny * nx], np.float64).reshape(ny * nx, 2)
        q = np.frombuffer(raw[pos + 16 * ny * nx:], np.float32).reshape(c, h, w)
        assert np.array_equal(got_ys, ys) and np.array_equal(got_xs, xs)
        s, t = tiled.tile_fit(base, tiles, ys, xs, align)
        assert same_bits64(fit[:, 0], s) and same_bits64(fit[:, 1], t), (case, align)
        assert same_bits(q, tiled.tile_merge(base, tiles, ys, xs, o, align)), (case, align)


# ---- what the merge is for ---------------------------------------------------------------------------------------------------------------------------
def smooth_base(h, w):
    """A smooth map in [0.25, 0.8]: its spread inside every 64 x 64 window is at least 0.5"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (0.525 + 0.275 * np.sin(yy / 9.0) * np.cos(xx / 11.0)).astype(f32)[None]


def test_affine_images_of_the_base_merge_back_to_it():
    """Tiles made as float32((G_window - t) / s) with s in [0.5, 2] and t in [-0.25, 0.25]: where the tiles that cover a pixel stay inside [0, 1],
    the merge gives the base back within 1e-5 (float32 rounding of a value <= 3 scaled by <= 2 gives about 4e-7; the truncation to 16 bits
    moves the fitted shift by about (s - 1) / 2 steps of 1 / 65535).  Measured: 7.7e-6 at the worst pixel."""
    from genpercept_amd import tiled
    rng = np.random.RandomState(3)
    h, w, size, o = 200, 260, 64, 16
    base = smooth_base(h, w)
    ys, xs, wh, ww = tiled.tile_grid(h, w, size, o)
    tiles, inside, want_s = [], [], []
    corners = [(0.5, 0.0), (2.0, -0.25), (2.0, 0.2), (0.5, 0.25), (1.0, 0.0)]
    for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        win = base[:, y0:y0 + wh, x0:x0 + ww].astype(np.float64)
        assert win.max() - win.min() >= 0.5
        s, t = corners[k] if k < len(corners) else (rng.uniform(0.5, 2.0), rng.uniform(-0.25, 0.25))
        tile = ((win - t) / s).astype(f32)
        tiles.append(tile)
        inside.append(bool(tile.min() >= 0.0 and tile.max() <= 1.0))
        want_s.append(s)
    tiles = np.stack(tiles)
    got = tiled.tile_merge(base, tiles, ys, xs, o, "least_square")
    s, _ = tiled.tile_fit(base, tiles, ys, xs, "least_square")
    ok = np.ones((h, w), bool)
    for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        if not inside[k]:
            ok[y0:y0 + wh, x0:x0 + ww] = False
    assert sum(inside) >= len(inside) // 3 and ok.mean() > 0.2, (sum(inside), len(inside), ok.mean())
    err = float(np.abs(got[0].astype(np.float64) - base[0].astype(np.float64))[ok].max())
    rel = max(abs(s[k] / want_s[k] - 1.0) for k in range(len(inside)) if inside[k])
    print(f"affine recovery: {sum(inside)} of {len(inside)} tiles inside [0, 1], {ok.mean():.2f} of the pixels checked, max |merged - base| = {err:.3e}, "
          f"max |s / s_true - 1| = {rel:.3e}")
    assert err <= 1e-5


def test_degenerate_tiles_and_single_tiles():
    from genpercept_amd import tiled
    rng = np.random.RandomState(4)
    h, w, size, o = 40, 56, 24, 8
    base = smooth_base(h, w)
    ys, xs, wh, ww = tiled.tile_grid(h, w, size, o)
    n = len(ys) * len(xs)
    wins = np.stack([base[:, y0:y0 + wh, x0:x0 + ww] for y0 in ys for x0 in xs])
    tiles = wins.copy()
    tiles[0] = 0.4                                                    # flat: var = 0
    tiles[1] = f32(0.4) + (rng.rand(1, wh, ww) < 0.5) * f32(1.0 / 65535.0)  # flat to within one step: var <= 1/4
    tiles[2] = 1.0 - wins[2]                                          # anti-correlated: s < 0
    tiles[3] = np.nan                                                 # all NaN: P = 0, flat
    tiles[4, 0, 10, 12] = np.nan                                      # one NaN (where no other tile reaches): fitted as 0, blended as NaN
    s, t = tiled.tile_fit(base, tiles, ys, xs, "least_square")
    sums = tiled.fit_sums(base, tiles, ys, xs)
    assert sums.dtype == np.int64 and sums.shape == (n, 5) and (sums[:, 0] == wh * ww).all() and sums[3, 1] == 0 and sums[3, 3] == 0
    for k in (0, 1, 2, 3):
        mp, mg = sums[k, 1] / sums[k, 0], sums[k, 2] / sums[k, 0]
        assert s[k] == 1.0 and t[k] == (mg - 1.0 * mp) / 65535.0, k
    assert s[4] > 0.9 and s[5] > 0.999 and abs(t[5]) < 1e-5
    got = tiled.tile_merge(base, tiles, ys, xs, o, "least_square")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    y0, x0 = int(ys[4 // len(xs)]), int(xs[4 % len(xs)])
    assert got[0, y0 + 10, x0 + 12] == 0.0                            # NaN -> 0 at the pixel the NaN covers ...
    assert abs(got[0, y0 + 10, x0 + 13] - base[0, y0 + 10, x0 + 13]) < 0.02   # ... and nowhere else (the fit saw one outlier in 576 values)
    # a NaN in the base is a 0 in the fit and never reaches the output
    base_nan = base.copy()
    base_nan[0, 1, 1] = np.nan
    assert np.isfinite(tiled.tile_merge(base_nan, wins, ys, xs, o, "least_square")).all()
    # `none` with one tile: the tile's own bits (values in [0, 1]; outside them the clamp)
    one = rng.rand(3, 30, 30).astype(f32)
    gy, gx, _, _ = tiled.tile_grid(30, 30, 64, 7)
    assert gy.tolist() == [0] and gx.tolist() == [0]
    assert same_bits(tiled.tile_merge(np.zeros((3, 30, 30), f32), one[None], gy, gx, 7, "none"), one)
    one[0, 0, 0], one[1, 2, 3], one[2, 4, 4] = 1.5, -0.5, np.nan
    got = tiled.tile_merge(np.zeros((3, 30, 30), f32), one[None], gy, gx, 7, "none")
    assert got[0, 0, 0] == 1.0 and got[1, 2, 3] == 0.0 and got[2, 4, 4] == 0.0
    # `none` in general: a weighted mean of the tiles, so tiles that are the windows give the base back to rounding
    assert np.abs(tiled.tile_merge(base, wins, ys, xs, o, "none") - base).max() < 1e-7
    # a 2-D base is one channel
    assert same_bits(tiled.tile_merge(base[0], wins, ys, xs, o), tiled.tile_merge(base, wins, ys, xs, o))


def test_options_and_shapes_are_checked():
    from genpercept_amd import tiled
    assert tiled.tiles_options(True, 768, "depth") == dict(size=768, overlap=192, align="least_square", batch=4)
    assert tiled.tiles_options(True, 768, "disparity")["align"] == "least_square"
    for mode in ("matting", "dis", "seg", "normal"):
        assert tiled.tiles_options(True, 512, mode) == dict(size=512, overlap=128, align="none", batch=4)
    assert tiled.tiles_options(dict(size=48, overlap=16, batch=3), 0, "matting") == dict(size=48, overlap=16, align="none", batch=3)
    assert tiled.tiles_options(dict(align="none"), 64, "depth") == dict(size=64, overlap=16, align="none", batch=4)
    for bad in (False, 1, "yes", dict(tile=64), dict(size=1), dict(size=64.0), dict(size=64, overlap=33), dict(size=64, overlap=0), dict(align="affine"),
                dict(batch=0), dict(batch=1.5), dict(size=True), dict(size=32768)):
        with pytest.raises(ValueError):
            tiled.tiles_options(bad, 768, "depth")
    for res in (0, None):
        with pytest.raises(ValueError):
            tiled.tiles_options(True, res, "depth")
        with pytest.raises(ValueError):
            tiled.tiles_options(dict(overlap=8), res, "depth")
    base, tiles, ys, xs = random_case(np.random.RandomState(5), 1, 20, 30, 12, 4, odd=False)
    tiled.tile_merge(base, tiles, ys, xs, 4)
    for args in ((base, tiles[:-1], ys, xs, 4), (base, tiles, ys + 1, xs, 4), (base, tiles, ys, xs[:-1], 4), (base, tiles, ys, xs, 3), (base, tiles, ys, xs, 7),
                 (base, tiles, ys, xs, 4, "affine"), (np.concatenate([base, base]), tiles, ys, xs, 4), (base, tiles[:, :, :, :5], ys, xs, 4),
                 ((base * 255).astype(np.uint8), tiles, ys, xs, 4), (base, tiles, ys.astype(np.float32), xs, 4), (base, np.repeat(tiles, 3, 1), ys, xs, 4)):
        with pytest.raises(ValueError):
            tiled.tile_merge(*args)
    with pytest.raises(ValueError):
        tiled.tile_fit(base, tiles, ys + 9, xs)


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    ps.assert_entries_bound(NAMES, "tile_merge.hip", "tile_merge_math.h")
    assert len(engine.SYMBOLS["gp_tile_merge"][1]) == 19 and engine.SYMBOLS["gp_tile_merge_workspace"] == (C.c_longlong, [C.c_int] * 8)
    assert callable(engine.tile_merge)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 1, 64, 64, 2, 2, 40, 40), (1, 2, 64, 64, 2, 2, 40, 40), (1, 1, 0, 64, 2, 2, 40, 40), (1, 1, 64, 16385, 2, 2, 40, 40),
                    (1, 1, 64, 64, 0, 2, 40, 40), (1, 1, 64, 64, 33, 32, 40, 40), (1, 1, 64, 64, 2, 2, 65, 40), (1, 1, 64, 64, 2, 2, 40, 0),
                    (65536, 1, 64, 64, 2, 2, 40, 40), (1, 1, 64, 64, 2, 2000, 40, 40)):
            assert lib.gp_tile_merge_workspace(*bad) == 0, bad
        for c in (1, 3):
            for h, w, ny, nx, wh, ww in ((40, 40, 1, 1, 40, 40), (70, 101, 3, 5, 32, 32), (4032, 6048, 7, 11, 768, 768)):
                one = lib.gp_tile_merge_workspace(1, c, h, w, ny, nx, wh, ww)
                slabs = min(max(1, min(512, -(-c * wh * ww // 4096))), c * wh)
                assert one == ny * nx * (2 + 5 * slabs) * 8 and lib.gp_tile_merge_workspace(7, c, h, w, ny, nx, wh, ww) == 7 * one


def merge_args(lib, b, c, h, w, size, o, **ptrs):
    """A valid argument set of gp_tile_merge for these sizes (pointers as given, small integers by default), and the host arrays it points to."""
    from genpercept_amd import tiled
    ys, xs, wh, ww = tiled.tile_grid(h, w, size, o)
    ys, xs = np.ascontiguousarray(ys, np.int32), np.ascontiguousarray(xs, np.int32)
    need = int(lib.gp_tile_merge_workspace(b, c, h, w, len(ys), len(xs), wh, ww))
    ok = dict(base=0x1000, tiles=0x2000, B=b, C=c, H=h, W=w, ys=ys.ctypes.data, ny=len(ys), xs=xs.ctypes.data, nx=len(xs), wh=wh, ww=ww, o=o, align=0,
              fit=0x4000, out=0x5000, ws=0x8000, nbytes=need)
    ok.update(ptrs)
    return ok, (ys, xs)


def invalid_cases(ok, keep):
    """The argument sets gp_tile_merge refuses, as changes to a valid set `ok` of a 2 x 1 x 70 x 101 problem with 32 x 32 tiles, overlap 8;
    the host arrays the cases point to are appended to `keep`."""
    huge = 1 << 62

    def arr(v):
        keep.append(np.ascontiguousarray(v, np.int32))
        return keep[-1].ctypes.data

    ys, xs = keep[0], keep[1]
    return [dict(base=None), dict(tiles=None), dict(ys=None), dict(xs=None), dict(out=None), dict(ws=None),
            dict(B=0), dict(B=-1), dict(B=65536, nbytes=huge), dict(C=0), dict(C=2), dict(C=4), dict(C=-1),
            dict(H=0), dict(W=-5), dict(H=16385, nbytes=huge), dict(W=16385, nbytes=huge), dict(H=71), dict(W=100), dict(H=31), dict(W=20),
            dict(wh=0), dict(ww=0), dict(wh=71), dict(wh=31), dict(ww=33), dict(ww=102),
            dict(o=0), dict(o=-1), dict(o=17), dict(o=16), dict(o=12),   # (16 and 12 are in range, but give another grid)
            dict(ny=ok["ny"] - 1), dict(ny=ok["ny"] + 1), dict(nx=ok["nx"] + 1), dict(nx=0), dict(ny=0), dict(ny=1025, nx=1, nbytes=huge),
            dict(ys=arr(ys + 1)), dict(xs=arr(xs[::-1])), dict(ys=arr(np.where(np.arange(len(ys)) == 1, ys + 1, ys))),
            dict(xs=arr(np.where(np.arange(len(xs)) == len(xs) - 1, xs - 1, xs))),
            dict(align=2), dict(align=-1),
            dict(base=ok["base"] + 2), dict(base=ok["base"] + 1), dict(tiles=ok["tiles"] + 2), dict(out=ok["out"] + 2), dict(out=ok["out"] + 3),
            dict(fit=ok["fit"] + 4), dict(fit=ok["fit"] + 1), dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1),
            dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=ok["nbytes"] // 2)]


def call_merge(lib, a):
    return lib.gp_tile_merge(a["base"], a["tiles"], a["B"], a["C"], a["H"], a["W"], a["ys"], a["ny"], a["xs"], a["nx"], a["wh"], a["ww"], a["o"], a["align"],
                             a["fit"], a["out"], a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced (ys and xs are host arrays and are read)."""
    for lib in _libs():
        ok, keep = merge_args(lib, 2, 1, 70, 101, 32, 8)
        keep = list(keep)
        assert ok["ny"] == 3 and ok["nx"] == 4 and ok["nbytes"] > 0
        ps.assert_all_refused(call_merge, lib, ok, invalid_cases(ok, keep))
