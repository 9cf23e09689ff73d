"""Edge-aware upsampling (gp_guided_upsample), the host half: genpercept_amd/guided.py (vectorised numpy) bit-equal to a plain scalar loop
implementation written here from the definition; tests/guided_check.cpp, a stand-alone CPU program over the kernels' own arithmetic
(csrc/guided_solve.h, contraction off, under AddressSanitizer and UBSan), bit-equal to the host route from dumped integer sums; the exactness
that the cap on r buys; the quality of the refinement on a synthetic matte; constant predictions and constant images; the header, the two
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

NAMES = ("gp_guided_upsample_workspace", "gp_guided_upsample")
f32 = np.float32
SIZES = [(1, 1, 1, 1), (1, 7, 3, 20), (5, 4, 5, 4), (9, 13, 35, 50)]
same_bits = functools.partial(ps.same_bits, dtype=np.float32)


def random_inputs(rng, c, h, w, H, W):
    """guide_lo uint8 [3, h, w] and guide uint8 [3, H, W] of noise with a flat block each, a prediction float32 [C, h, w] of plateaus, noise
    and values outside [0, 1]."""
    lo, hi = rng.randint(0, 256, (3, h, w)).astype(np.uint8), rng.randint(0, 256, (3, H, W)).astype(np.uint8)
    for g in (lo, hi):
        n, m = g.shape[1:]
        if n > 2 and m > 2:
            y, x = rng.randint(0, n - 1), rng.randint(0, m - 1)
            g[:, y:y + rng.randint(1, n), x:x + rng.randint(1, m)] = rng.randint(0, 256, (3, 1, 1))
    p = np.where(rng.rand(c, h, w) < 0.5, 0.0, 1.0)
    sel = rng.rand(c, h, w) < 0.5
    p[sel] = rng.rand(int(sel.sum())) * 1.2 - 0.1
    return lo, p.astype(np.float32), hi


# ---- the definition as plain loops ---------------------------------------------------------------------------------------------------------------
def loops_guided(guide_lo, pred, guide, r, eps):
    """The definition of include/genpercept_hip.h, literally: Python integers and Python floats (IEEE float64, one operation at a time), one
    pixel, one window element, one channel at a time."""
    Cn, h, w = pred.shape
    H, W = guide.shape[1:]
    I = [[[int(guide_lo[c, y, x]) for c in range(3)] for x in range(w)] for y in range(h)]
    p = [[[0] * Cn for _ in range(w)] for _ in range(h)]
    for y in range(h):
        for x in range(w):
            for c in range(Cn):
                v = f32(pred[c, y, x])
                v = (v if v < f32(1.0) else f32(1.0)) if v > f32(0.0) else f32(0.0)
                p[y][x][c] = int(v * f32(65535.0))
    e = float(eps) * 65025.0
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    ab = [[[None] * Cn for _ in range(w)] for _ in range(h)]
    for y in range(h):
        for x in range(w):
            win = [(yy, xx) for yy in range(max(y - r, 0), min(y + r, h - 1) + 1) for xx in range(max(x - r, 0), min(x + r, w - 1) + 1)]
            n = len(win)
            sI = [sum(I[yy][xx][c] for yy, xx in win) for c in range(3)]
            sII = {cd: sum(I[yy][xx][cd[0]] * I[yy][xx][cd[1]] for yy, xx in win) for cd in pairs}
            N = float(n)
            NN = N * N
            fI = [float(v) for v in sI]
            s = {}
            for c, d in pairs:
                assert n * sII[c, d] < 2 ** 53 and sI[c] * sI[d] < 2 ** 53
                s[c, d] = (N * float(sII[c, d]) - fI[c] * fI[d]) / NN
                if c == d:
                    s[c, d] = s[c, d] + e
            c00 = s[1, 1] * s[2, 2] - s[1, 2] * s[1, 2]
            c01 = s[0, 2] * s[1, 2] - s[0, 1] * s[2, 2]
            c02 = s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]
            c11 = s[0, 0] * s[2, 2] - s[0, 2] * s[0, 2]
            c12 = s[0, 1] * s[0, 2] - s[0, 0] * s[1, 2]
            c22 = s[0, 0] * s[1, 1] - s[0, 1] * s[0, 1]
            det = (s[0, 0] * c00 + s[0, 1] * c01) + s[0, 2] * c02
            assert det > 0.0
            for ch in range(Cn):
                sp = sum(p[yy][xx][ch] for yy, xx in win)
                sIp = [sum(I[yy][xx][c] * p[yy][xx][ch] for yy, xx in win) for c in range(3)]
                P = float(sp)
                cov = [(N * float(sIp[c]) - fI[c] * P) / NN for c in range(3)]
                a0 = ((c00 * cov[0] + c01 * cov[1]) + c02 * cov[2]) / det
                a1 = ((c01 * cov[0] + c11 * cov[1]) + c12 * cov[2]) / det
                a2 = ((c02 * cov[0] + c12 * cov[1]) + c22 * cov[2]) / det
                b = P / N - ((a0 * (fI[0] / N) + a1 * (fI[1] / N)) + a2 * (fI[2] / N))
                ab[y][x][ch] = (a0, a1, a2, b)
    mean = [[[None] * Cn for _ in range(w)] for _ in range(h)]
    for y in range(h):
        for x in range(w):
            ys, xs = range(max(y - r, 0), min(y + r, h - 1) + 1), range(max(x - r, 0), min(x + r, w - 1) + 1)
            for ch in range(Cn):
                m = []
                for k in range(4):
                    col = 0.0
                    for yy in ys:
                        row = 0.0
                        for xx in xs:
                            row = row + ab[yy][xx][ch][k]
                        col = col + row
                    m.append(col / float(len(ys) * len(xs)))
                mean[y][x][ch] = m

    def index(Y, n_from, n_to):
        q = float((2 * Y + 1) * n_from - n_to) / float(2 * n_to)
        s = q if q > 0.0 else 0.0
        i0 = int(np.floor(s))
        return i0, min(i0 + 1, n_from - 1), s - float(i0)

    out = np.zeros((Cn, H, W), np.float32)
    for Y in range(H):
        i0, i1, fy = index(Y, h, H)
        for X in range(W):
            j0, j1, fx = index(X, w, W)
            g = [float(guide[c, Y, X]) for c in range(3)]
            for ch in range(Cn):
                V = []
                for k in range(4):
                    v00, v01, v10, v11 = mean[i0][j0][ch][k], mean[i0][j1][ch][k], mean[i1][j0][ch][k], mean[i1][j1][ch][k]
                    t0 = v00 + fx * (v01 - v00)
                    t1 = v10 + fx * (v11 - v10)
                    V.append(t0 + fy * (t1 - t0))
                q = (((V[0] * g[0] + V[1] * g[1]) + V[2] * g[2]) + V[3]) / 65535.0
                q = (q if q < 1.0 else 1.0) if q > 0.0 else 0.0
                out[ch, Y, X] = np.float32(q)
    return out


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("r", [1, 3, 32])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_host_route_equals_plain_loops(size, r, c):
    from genpercept_amd import guided as gd
    h, w, H, W = size
    rng = np.random.RandomState(1000 * h + 10 * r + c)
    lo, p, hi = random_inputs(rng, c, h, w, H, W)
    p.flat[0] = np.nan
    for eps in (1e-4, 1.0) if r == 3 else (1e-4,):
        got = gd.guided_upsample(lo, p, hi, r, eps)
        assert got.shape == (c, H, W) and same_bits(got, loops_guided(lo, p, hi, r, eps)), (size, r, c, eps)
    assert got.min() >= 0.0 and got.max() <= 1.0


# ---- the kernels' arithmetic on the CPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "guided_check.cpp")


@pytest.mark.parametrize("case", [(1, 1, 1, 1, 1, 1), (1, 7, 3, 20, 32, 3), (9, 13, 35, 50, 3, 3), (37, 29, 80, 61, 4, 1), (20, 31, 9, 14, 2, 1)],
                         ids=lambda s: "%dx%d-%dx%d-r%d-c%d" % s)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    from genpercept_amd import guided as gd
    h, w, H, W, r, c = case
    rng = np.random.RandomState(300 + h)
    lo, p, hi = random_inputs(rng, c, h, w, H, W)
    for n, eps in enumerate((1e-4, 1e-6, 1.0)):
        sums = gd.window_sums(lo, gd.quantize16(p), r)
        src, dst = str(tmp_path / f"in{n}.bin"), str(tmp_path / f"out{n}.bin")
        with open(src, "wb") as f:
            f.write(np.array([h, w, H, W, r, c], np.int32).tobytes() + np.array([eps], np.float64).tobytes())
            for k in ("N", "S_I", "S_II", "S_p", "S_Ip"):
                assert sums[k].dtype == np.int64
                f.write(np.ascontiguousarray(sums[k]).tobytes())
            f.write(hi.tobytes())
        lines, raw = ps.run_check(check_exe, src, dst)
        ab = np.frombuffer(raw[:c * 4 * h * w * 8], np.float64).reshape(c, 4, h, w)
        q = np.frombuffer(raw[c * 4 * h * w * 8:], np.float32).reshape(c, H, W)
        want_ab = gd.solve(sums, eps)
        assert np.array_equal(ab.view(np.uint64), want_ab.view(np.uint64)), (case, eps)
        assert same_bits(q, gd.guided_upsample(lo, p, hi, r, eps)), (case, eps)
        want = [int(v) for v in gd.quantize16(np.array([0.0, 1.0, np.nan, -0.25, 1.5, 0.5], np.float32))]
        assert [int(v) for v in lines[0].split()] == want == [0, 65535, 0, 0, 65535, 32767]


# ---- what the cap on r is for ---------------------------------------------------------------------------------------------------------------------------
def test_sums_and_products_are_exact_at_the_cap():
    """All-255 bytes and an all-65535 prediction at r = 32: the largest sums there can be.  Every product the solve takes of two integers stays
    below 2^53 and is the same number in float64 and in Python integers; sums accumulated in float64 equal the int64 sums."""
    from genpercept_amd import guided as gd
    h, w, r = 70, 67, 32
    lo = np.full((3, h, w), 255, np.uint8)
    p16 = gd.quantize16(np.ones((1, h, w), np.float32))
    assert p16.dtype == np.uint16 and (p16 == 65535).all()
    sums = gd.window_sums(lo, p16, r)
    assert int(sums["N"].max()) == 65 * 65 and int(sums["S_Ip"].max()) == 4225 * 255 * 65535 and int(sums["S_II"].max()) == 4225 * 255 * 255
    worst = 0
    for y, x in ((0, 0), (32, 33), (h - 1, w - 1), (35, 0)):
        n, sI, sII, sp, sIp = (int(sums[k][..., y, x].max()) for k in ("N", "S_I", "S_II", "S_p", "S_Ip"))
        for u, v in ((n, sIp), (sI, sp), (n, sII), (sI, sI), (n, n)):
            assert u * v < 2 ** 53 and float(u) * float(v) == u * v and int(float(u) * float(v)) == u * v
            worst = max(worst, u * v)
    assert worst == 4225 ** 2 * 255 * 65535 < 2 ** 53
    # the same sums accumulated in float64, element by element in another order (columns first): no rounding anywhere
    If, pf = lo.astype(np.float64), p16.astype(np.float64)
    for name, v in (("S_I", If), ("S_p", pf), ("S_Ip", (pf[:, None] * If[None])), ("S_II", np.stack([If[c] * If[d] for c, d in gd.PAIRS]))):
        acc = np.zeros_like(v)
        zp = np.pad(v, [(0, 0)] * (v.ndim - 2) + [(r, r), (r, r)])
        for dx in range(2 * r + 1):
            col = np.zeros_like(v)
            for dy in range(2 * r + 1):
                col = col + zp[..., dy:dy + h, dx:dx + w]
            acc = acc + col
        assert np.array_equal(acc, sums[name].astype(np.float64)) and np.array_equal(acc.astype(np.int64), sums[name]), name
    out = gd.guided_upsample(lo, np.ones((1, h, w), np.float32), np.full((3, 2 * h, 2 * w), 255, np.uint8), r, 1e-4)
    assert same_bits(out, np.ones((1, 2 * h, 2 * w), np.float32))


# ---- quality ----------------------------------------------------------------------------------------------------------------------------------------------
def synthetic_matte(seed=5, n=256, k=4):
    """A wavy-edged disc as the true alpha [n, n] (antialiased by 4 x 4 supersampling), a noisy two-colour foreground and background composited
    under it into the image uint8 [3, n, n]; the alpha a model working at n / k would give: the k x k box average of the true alpha blurred
    once with a 3 x 3 box.  Returns (image, alpha_true float64, alpha_lo float32 [n / k, n / k])."""
    rng = np.random.RandomState(seed)
    ss = 4
    t = (np.arange(n * ss) + 0.5) / ss
    yy, xx = np.meshgrid(t, t, indexing="ij")
    dy, dx = yy - 0.5 * n, xx - 0.52 * n
    rad = n * (0.31 + 0.035 * np.sin(7.0 * np.arctan2(dy, dx)) + 0.012 * np.sin(23.0 * np.arctan2(dy, dx)))
    alpha = (np.hypot(dy, dx) < rad).astype(np.float64).reshape(n, ss, n, ss).mean(axis=(1, 3))
    fg = np.array([0.85, 0.35, 0.2])[:, None, None] + 0.04 * rng.randn(3, n, n)
    bg = np.array([0.15, 0.4, 0.7])[:, None, None] + 0.04 * rng.randn(3, n, n)
    img = np.floor(np.clip(alpha * fg + (1.0 - alpha) * bg, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    lo = alpha.reshape(n // k, k, n // k, k).mean(axis=(1, 3))
    z = np.pad(lo, 1, mode="edge")
    lo = sum(z[i:i + n // k, j:j + n // k] for i in range(3) for j in range(3)) / 9.0
    return img, alpha, lo.astype(np.float32)


def test_refinement_beats_the_bilinear_upsample():
    """256 x 256 from 64 x 64, r = 4, eps = 1e-4, the guide at the processing size made as the pipeline makes it (the antialiased bilinear
    resize of the bytes).  Mean absolute error against the true alpha: refined / bilinear has to stay below 0.85.  Measured: 0.01668 against
    0.02788, ratio 0.598 (the prototype of the issue, with a box-averaged guide, gave 0.68 on its own matte)."""
    import torch
    from genpercept_amd import guided as gd
    from genpercept_amd.image_util import resize_to
    img, alpha, a_lo = synthetic_matte()
    guide_lo = resize_to(torch.from_numpy(img)[None], (64, 64), "bilinear")[0].numpy()
    assert guide_lo.dtype == np.uint8 and guide_lo.shape == (3, 64, 64)
    refined = gd.guided_upsample(guide_lo, a_lo[None], img, 4, 1e-4)[0]
    plain = np.clip(gd.resize_bilinear(a_lo.astype(np.float64), 256, 256), 0.0, 1.0)
    err, err_plain = float(np.abs(refined - alpha).mean()), float(np.abs(plain - alpha).mean())
    print(f"guided upsampling 64 -> 256: mean |alpha - true| refined {err:.5f}, bilinear {err_plain:.5f}, ratio {err / err_plain:.3f}")
    assert err < 0.85 * err_plain


def test_constant_prediction_and_constant_image():
    from genpercept_amd import guided as gd
    rng = np.random.RandomState(11)
    lo, p, hi = random_inputs(rng, 3, 19, 26, 61, 77)
    for r, eps in ((2, 1e-4), (32, 1e-6), (5, 1.0)):
        for v in (0.0, 1.0, 0.3, 12345.0 / 65535.0):
            const = np.full((3, 19, 26), v, np.float32)
            out = gd.guided_upsample(lo, const, hi, r, eps)
            want = np.float32(np.float64(int(gd.quantize16(const)[0, 0, 0])) / 65535.0)
            assert same_bits(out, np.full((3, 61, 77), want, np.float32)), (r, eps, v)
        # a constant image carries no edges: what is left is the prediction, smoothed twice and upsampled bilinearly
        flat_lo, flat_hi = np.full((3, 19, 26), 77, np.uint8), np.full((3, 61, 77), 201, np.uint8)
        out = gd.guided_upsample(flat_lo, p, flat_hi, r, eps)
        sums = gd.window_sums(flat_lo, gd.quantize16(p), r)
        mean_p = sums["S_p"].astype(np.float64) / sums["N"].astype(np.float64)
        want = gd.resize_bilinear(gd.smooth(mean_p, r), 61, 77) / 65535.0
        want = np.where(want > 0.0, np.where(want < 1.0, want, 1.0), 0.0).astype(np.float32)
        assert same_bits(out, want), (r, eps)


def test_options_and_shapes_are_checked():
    from genpercept_amd import guided as gd
    rng = np.random.RandomState(12)
    lo, p, hi = random_inputs(rng, 1, 6, 7, 12, 15)
    assert same_bits(gd.guided_upsample(lo, p[0], hi), gd.guided_upsample(lo, p, hi, radius=4, eps=1e-4))
    for bad in (dict(radius=0), dict(radius=33), dict(radius=2.5), dict(eps=0.0), dict(eps=1.5), dict(eps=-1e-4), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            gd.guided_upsample(lo, p, hi, **bad)
    for args in ((lo[:2], p, hi), (lo, p[:, :5], hi), (lo, np.concatenate([p, p]), hi), (lo.astype(np.float32), p, hi), (lo, p, hi[:, None]),
                 (lo, (p * 255).astype(np.uint8), hi)):
        with pytest.raises(ValueError):
            gd.guided_upsample(*args)
    assert gd.refine_options(True) == dict(radius=4, eps=1e-4) and gd.refine_options(dict(radius=8)) == dict(radius=8, eps=1e-4)
    for bad in (False, 1, "yes", dict(r=3), dict(radius=40), dict(eps=2.0)):
        with pytest.raises(ValueError):
            gd.refine_options(bad)


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    ps.assert_entries_bound(NAMES, "guided.hip", "guided_solve.h")
    assert len(engine.SYMBOLS["gp_guided_upsample"][1]) == 15 and engine.SYMBOLS["gp_guided_upsample"][1][10] is C.c_double
    assert engine.SYMBOLS["gp_guided_upsample_workspace"] == (C.c_longlong, [C.c_int] * 4)
    assert callable(engine.guided_upsample)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 1, 8, 8), (1, 2, 8, 8), (1, 0, 8, 8), (1, 4, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (-1, 1, 8, 8), (65536, 1, 8, 8), (1, 1, 16385, 8),
                    (1, 3, 8, 16385)):
            assert lib.gp_guided_upsample_workspace(*bad) == 0
        for c in (1, 3):
            for h, w in ((1, 1), (7, 5), (480, 640), (16384, 16384)):
                one = lib.gp_guided_upsample_workspace(1, c, h, w)
                assert one == 2 * 4 * c * h * w * 8 and lib.gp_guided_upsample_workspace(7, c, h, w) == 7 * one


def invalid_cases(ok, need_one):
    """The argument sets gp_guided_upsample refuses, as changes to a valid set `ok`."""
    huge = 1 << 62
    nan = float("nan")
    return [dict(guide_lo=None), dict(pred=None), dict(guide=None), dict(out=None), dict(ws=None),
            dict(B=0), dict(B=-3), dict(B=65536, nbytes=huge), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(h=-1), dict(W=-1),
            dict(h=16385, nbytes=huge), dict(w=16385, nbytes=huge), dict(H=16385), dict(W=16385), dict(h=1 << 20, w=1 << 20, nbytes=huge),
            dict(C=0), dict(C=2), dict(C=4), dict(C=-1), dict(C=3),                       # (C = 3: the workspace of C = 1 is too small)
            dict(r=0), dict(r=33), dict(r=-1), dict(eps=0.0), dict(eps=-1e-4), dict(eps=1.0001), dict(eps=nan), dict(eps=float("inf")),
            dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1), dict(out=ok["out"] + 2), dict(out=ok["out"] + 3),
            dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1), dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=need_one)]


def call_guided(lib, a):
    return lib.gp_guided_upsample(a["guide_lo"], a["pred"], a["C"], a["guide"], a["B"], a["h"], a["w"], a["H"], a["W"], a["r"], a["eps"], a["out"],
                                  a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        need = lib.gp_guided_upsample_workspace(2, 1, 24, 40)
        ok = dict(guide_lo=0x1001, pred=0x2000, C=1, guide=0x3003, B=2, h=24, w=40, H=96, W=160, r=4, eps=1e-4, out=0x5000, ws=0x8000, nbytes=need)
        ps.assert_all_refused(call_guided, lib, ok, invalid_cases(ok, lib.gp_guided_upsample_workspace(1, 1, 24, 40)))
