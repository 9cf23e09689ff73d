"""The stereo and parallax views on the host (genpercept_amd/stereo.py), without a GPU: the numpy route equals plain scalar loops written here
from the definition -- a scatter, source by source, where the numpy route gathers offset by offset -- and a stand-alone CPU build of the
kernels' arithmetic (tests/stereo_check.cpp over csrc/stereo_math.h, built with the ROCm clang++ under the address and undefined-behaviour
sanitizers and run as a child process); the properties the definition is for, with exact expectations; the layouts; the user's terms; the
entries declared, exported, bound, their argument checks with NULL buffers, and the binding's own refusals.  There is no tolerance in this
file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs, same_bits  # noqa: E402,F401

SIZES = [(1, 1), (5, 7), (19, 70), (6, 40)]
# H, W, max_s8, edge, space, NaN block: every size with every max_s8 of {0, 8, 40, 512}; edge 0, a middle value and 65535; both spaces
CASES = [(h, w, m, e, sp, nan) for i, (h, w) in enumerate(SIZES) for j, m in enumerate((0, 8, 40, 512))
         for e, sp, nan in [((0, 2600, 65535)[(i + j) % 3], ("depth", "disparity")[(i + j // 2) % 2], (i + j) % 2 == 1)]]


def scene(rng, h, w, nan=False):
    """One image: (pred float32 [h, w], every row a piecewise-planar surface of its own -- segments of 1 to 19 columns, each with a random
    base and slope, values beyond [0, 1] among them, a block of NaNs on request; image uint8 [3, h, w])."""
    pred = np.empty((h, w), np.float64)
    for y in range(h):
        x = 0
        while x < w:
            n = rng.randint(1, 20)
            pred[y, x:x + n] = (rng.uniform(-0.05, 1.05) + rng.uniform(-0.03, 0.03) * np.arange(n))[: w - x]
            x += n
    if nan:
        pred[h // 3: h // 3 + 2, w // 4: w // 4 + 5] = np.nan
    return pred.astype(np.float32), rng.randint(0, 256, (3, h, w)).astype(np.uint8)


def gain_for(max_s8, rng):
    """A gain whose largest shift is about one and a half times max_s8, so that the clamp is met; either sign."""
    g = min(131072, int(1.5 * max_s8 * 16777216 / 65535)) if max_s8 else 40000
    return g if rng.rand() < 0.5 else -g


# ---- the definition once more, in plain loops ---------------------------------------------------------------------------------------------------------
def loops_views(image, pred, F, table, canvas, space, edge, max_s8, bounded=True):
    """Steps 1 to 6 for one image [3, h, w]: every piece of every source is scattered over the columns it covers.  canvas [3, CH, CW] is
    written in place; returns (holes, near, cover) as lists [V][h][w].  bounded=False: the hole search has no limit."""
    _, h, w = image.shape
    D = ps.loops_nearness(pred, space)
    R = max_s8 // 4 + 1 if bounded else w
    holes, near, cover = [], [], []
    for g, ox, oy, cmask in table:
        vh, vn, vc = [], [], []
        for y in range(h):
            t = [8 * x + max(-max_s8, min(max_s8, ((D[y][x] - F) * g + (1 << 23)) >> 24)) for x in range(w)]
            conn = [abs(D[y][x] - D[y][x + 1]) <= edge for x in range(w - 1)]
            best, who, rgb, cnt = [-1] * w, [0] * w, [None] * w, [0] * w

            def offer(p, value, x, colour):
                cnt[p] += 1
                if value > best[p] or (value == best[p] and x < who[p]):
                    best[p], who[p], rgb[p] = value, x, colour

            for x in range(w - 1, -1, -1):
                c0 = [int(image[k, y, x]) for k in range(3)]
                if x + 1 < w and conn[x]:
                    L = t[x + 1] - t[x]
                    c1 = [int(image[k, y, x + 1]) for k in range(3)]
                    for p in range(w):
                        a = 8 * p - t[x]
                        if L > 0 and 0 <= a < L:
                            offer(p, (D[y][x] * (L - a) + D[y][x + 1] * a + (L >> 1)) // L, x, [(c0[k] * (L - a) + c1[k] * a + (L >> 1)) // L for k in range(3)])
                else:
                    for p in range(w):
                        if t[x] <= 8 * p < t[x] + 4:
                            offer(p, D[y][x], x, c0)
                if x == 0 or not conn[x - 1]:
                    for p in range(w):
                        if t[x] - 4 <= 8 * p < t[x]:
                            offer(p, D[y][x], x, c0)
            rh, rn = [0] * w, list(best)
            out = list(rgb)
            for p in range(w):
                if best[p] >= 0:
                    continue
                rh[p] = 1
                left = next((q for q in range(p - 1, max(-1, p - R - 1), -1) if best[q] >= 0), None)
                right = next((q for q in range(p + 1, min(w, p + R + 1)) if best[q] >= 0), None)
                if left is None and right is None:
                    rn[p], out[p] = 0, [0, 0, 0]
                    continue
                src = left if right is None or (left is not None and best[left] <= best[right]) else right
                rn[p], out[p] = best[src], rgb[src]
            for p in range(w):
                for k in range(3):
                    if cmask >> k & 1:
                        canvas[k, oy + y, ox + p] = out[p][k]
            vh.append(rh), vn.append(rn), vc.append(cnt)
        holes.append(vh), near.append(vn), cover.append(vc)
    return np.array(holes, np.uint8), np.array(near, np.uint16), np.array(cover, np.int64)


def case_inputs(case):
    h, w, max_s8, edge, space, nan = case
    rng = np.random.RandomState(1000 * h + 10 * w + max_s8 % 97)
    pred, image = scene(rng, h, w, nan)
    g = gain_for(max_s8, rng)
    F = int(rng.randint(0, 65536))
    table = [[g, 0, 0, 7], [-g // 2, w, 0, 7]]
    return pred, image, F, table, (h, 2 * w)


def span_lengths(pred, F, g, space, edge, max_s8):
    """L = t_{x+1} - t_x of the connected pairs of an image, one flat array."""
    from genpercept_amd import stereo as st
    D = st.nearness(pred, space)
    s = st.shifts(D, F, g, max_s8)
    L = 8 + s[:, 1:] - s[:, :-1]
    return L[np.abs(D[:, 1:] - D[:, :-1]) <= edge]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-s%d-e%d-%s%s" % (c[:5] + ("-nan" if c[5] else "",)))
def test_host_route_equals_plain_loops(case):
    from genpercept_amd import stereo as st
    h, w, max_s8, edge, space, nan = case
    pred, image, F, table, size = case_inputs(case)
    canvas, holes, near, cover = st.stereo_views_table(image, pred, F, table, size, space, edge, max_s8, want_cover=True)
    want = np.zeros((3,) + size, np.uint8)
    want_holes, want_near, want_cover = loops_views(image, pred, F, table, want, space, edge, max_s8)
    assert same_bits(cover[0], want_cover) and same_bits(holes[0], want_holes) and same_bits(near[0], want_near) and same_bits(canvas[0], want), case
    # the existing-neighbour-within-R bound: the search without a limit finds the same neighbours
    free = np.zeros((3,) + size, np.uint8)
    free_holes, free_near, _ = loops_views(image, pred, F, table, free, space, edge, max_s8, bounded=False)
    assert same_bits(free, want) and same_bits(free_near, want_near) and same_bits(free_holes, want_holes)
    R = max_s8 // 4 + 1
    for k in range(2):
        for y in range(h):
            covered = np.flatnonzero(holes[0, k, y] == 0)
            for p in np.flatnonzero(holes[0, k, y]):
                for side in (covered[covered < p], covered[covered > p]):
                    assert side.size == 0 or np.abs(side - p).min() <= R, (case, k, y, p)


def test_the_cases_met_every_condition():
    """Across the cases above the host result shows holes, columns that two or more pieces cover, stretched, compressed and folded spans
    and a row with nothing covered; how many cases show each."""
    from genpercept_amd import stereo as st
    seen = dict(holes=0, multiple=0, stretched=0, compressed=0, folded=0, empty_row=0)
    for case in CASES:
        h, w, max_s8, edge, space, nan = case
        pred, image, F, table, size = case_inputs(case)
        _, holes, _, cover = st.stereo_views_table(image, pred, F, table, size, space, edge, max_s8, want_cover=True)
        L = np.concatenate([span_lengths(pred, F, g, space, edge, max_s8) for g, _, _, _ in table])
        met = dict(holes=holes.any(), multiple=(cover >= 2).any(), stretched=(L > 8).any(), compressed=((L > 0) & (L < 8)).any(), folded=(L <= 0).any(),
                   empty_row=(holes == 1).all(-1).any())
        for name in seen:
            seen[name] += bool(met[name])
    print(seen)
    assert all(n >= 2 for n in seen.values()), seen


# ---- the kernels' arithmetic on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "stereo_check.cpp")


def run_check_program(check_exe, tmp_path, name, image, pred, F, table, size, space, edge, max_s8, fill=0):
    from genpercept_amd import stereo as st
    h, w = pred.shape
    v = len(table)
    src, dst = str(tmp_path / f"in{name}.bin"), str(tmp_path / f"out{name}.bin")
    with open(src, "wb") as f:
        f.write(np.array([h, w, st.SPACES.index(space), edge, max_s8, v, F, size[0], size[1], fill], np.int32).tobytes()
                + np.array(table, np.int32).tobytes() + pred.tobytes() + image.tobytes())
    raw = ps.run_check(check_exe, src, dst, timeout=120)[1]
    n, nc = v * h * w, 3 * size[0] * size[1]
    assert len(raw) == nc + n + 2 * n + 4 * n
    return (np.frombuffer(raw[:nc], np.uint8).reshape((3,) + tuple(size)), np.frombuffer(raw[nc:nc + n], np.uint8).reshape(v, h, w),
            np.frombuffer(raw[nc + n:nc + 3 * n], np.uint16).reshape(v, h, w), np.frombuffer(raw[nc + 3 * n:], np.int32).reshape(v, h, w))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-s%d-e%d-%s%s" % (c[:5] + ("-nan" if c[5] else "",)))
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    from genpercept_amd import stereo as st
    h, w, max_s8, edge, space, nan = case
    pred, image, F, table, size = case_inputs(case)
    got = run_check_program(check_exe, tmp_path, "a", image, pred, F, table, size, space, edge, max_s8)
    canvas, holes, near, cover = st.stereo_views_table(image, pred, F, table, size, space, edge, max_s8, want_cover=True)
    assert same_bits(got[0], canvas[0]) and same_bits(got[1], holes[0]) and same_bits(got[2], near[0]) and same_bits(got[3].astype(np.int64), cover[0])


def fold_and_cut_row(w=400, lo=20, hi=320):
    """A row (disparity space) that alternates folds and cuts between the columns lo and hi: nothing covers the columns it lands on, over
    more than R of them.  Returns (pred [1, w], F, g, edge, max_s8)."""
    D = np.full(w, 30000, np.int64)
    for x in range(lo, hi):
        D[x] = D[x - 1] - 2432 if x % 2 else D[x - 1] + 2433
    return (D / 65535.0).astype(np.float32)[None], 0, 131072, 2432, 256


def test_the_bound_is_part_of_the_definition(check_exe, tmp_path):
    """Where a row is no surface of planar pieces the nearest covered column can lie further than R away: the hole then takes nothing, on
    every route alike."""
    from genpercept_amd import stereo as st
    pred, F, g, edge, max_s8 = fold_and_cut_row()
    w = pred.shape[1]
    assert same_bits(st.nearness(pred, "disparity")[0, 18:23], np.array([30000, 30000, 32433, 30001, 32434]))
    image = np.random.RandomState(3).randint(1, 256, (3, 1, w)).astype(np.uint8)
    table = [[g, 0, 0, 7]]
    canvas, holes, near = st.stereo_views_table(image, pred, F, table, (1, w), "disparity", edge, max_s8)
    R = max_s8 // 4 + 1
    run = holes[0, 0, 0, 49:349]
    assert run.all() and not holes[0, 0, 0, 48] and not holes[0, 0, 0, 349] and R == 65            # 300 columns that nothing covers
    alone = np.arange(49 + R, 349 - R)
    assert alone.size == 170 and not near[0, 0, 0, alone].any() and not canvas[0, :, 0, alone].any()
    assert canvas[0, :, 0, 49 + R - 1].all() and canvas[0, :, 0, 349 - R].all()
    want = np.zeros((3, 1, w), np.uint8)
    want_holes, want_near, _ = loops_views(image, pred[:1], F, table, want, "disparity", edge, max_s8)
    assert same_bits(canvas[0], want) and same_bits(holes[0], want_holes) and same_bits(near[0], want_near)
    got = run_check_program(check_exe, tmp_path, "f", image, pred, F, table, (1, w), "disparity", edge, max_s8)
    assert same_bits(got[0], canvas[0]) and same_bits(got[1], holes[0]) and same_bits(got[2], near[0])


# ---- what the definition is for -----------------------------------------------------------------------------------------------------------------------
def test_no_gain_returns_the_image():
    from genpercept_amd import stereo as st
    rng = np.random.RandomState(5)
    pred, image = scene(rng, 19, 70, nan=True)
    for space in st.SPACES:
        for edge in (0, 3000, 65535):
            canvas, holes, near = st.stereo_views_table(image, pred, 12345, [[0, 0, 0, 7]], (19, 70), space, edge, 512)
            assert same_bits(canvas[0], image) and not holes.any() and same_bits(near[0, 0], st.nearness(pred, space).astype(np.uint16))
    out = st.stereo_views(image, pred, "sbs", 2, separation=0.0)
    assert same_bits(out[0, :, :, :70], image) and same_bits(out[0, :, :, 70:], image)


def test_a_constant_map_moves_the_image_by_whole_columns():
    from genpercept_amd import stereo as st
    image = np.random.RandomState(6).randint(0, 256, (3, 6, 40)).astype(np.uint8)
    pred = np.full((6, 40), 0.25, np.float32)
    D = int(st.nearness(pred, "disparity")[0, 0])
    assert D == 16383
    for cols in (2, -3, 5):
        g = next(g for g in range(0, 131073) if int(st.shifts(D, 0, g, 512)) == 8 * abs(cols)) * (1 if cols > 0 else -1)
        assert int(st.shifts(D, 0, g, 512)) == 8 * cols
        for edge in (0, 65535):
            canvas, holes, near = st.stereo_views_table(image, pred, 0, [[g, 0, 0, 7]], (6, 40), "disparity", edge, 64)
            lo, hi = max(0, cols), 40 + min(0, cols)
            assert same_bits(canvas[0, :, :, lo:hi], image[:, :, lo - cols:hi - cols])
            strip = np.ones((6, 40), bool)
            strip[:, lo:hi] = False
            assert same_bits(holes[0, 0], strip.astype(np.uint8)) and (near == D).all()
            border = image[:, :, :1] if cols > 0 else image[:, :, -1:]
            assert same_bits(canvas[0][:, strip].reshape(3, 6, abs(cols)), np.broadcast_to(border, (3, 6, abs(cols))))


def test_a_near_square_over_a_far_plane():
    """depth space, the zero-parallax plane on the background: the square moves, the background stays.  The hole opens on the side the square
    moved away from, and every filled byte is the background neighbour's, never the square's."""
    from genpercept_amd import stereo as st
    h, w, top, bottom, left, right, move = 20, 48, 5, 14, 18, 30, 4
    pred = np.full((h, w), 0.9, np.float32)
    pred[top:bottom, left:right] = 0.1
    image = np.random.RandomState(7).randint(0, 200, (3, h, w)).astype(np.uint8)
    image[:, top:bottom, left:right] = 255
    Dn, Df = (int(v) for v in st.nearness(np.float32([0.1, 0.9]), "depth"))
    gain = next(g for g in range(131073) if int(st.shifts(Dn, Df, g, 512)) == 8 * move)
    for g in (gain, -gain):
        s = int(st.shifts(Dn, Df, g, 512)) // 8                                                        # +4: to the right; -4: to the left
        canvas, holes, near = st.stereo_views_table(image, pred, Df, [[g, 0, 0, 7]], (h, w), "depth", 3000, 64)
        want_holes = np.zeros((h, w), np.uint8)
        gap = slice(left, left + s) if s > 0 else slice(right + s, right)
        want_holes[top:bottom, gap] = 1
        assert abs(s) == move and same_bits(holes[0, 0], want_holes)
        neighbour = left - 1 if s > 0 else right
        assert same_bits(canvas[0, :, top:bottom, gap], np.broadcast_to(image[:, top:bottom, neighbour:neighbour + 1], (3, bottom - top, move)))
        assert (canvas[0, :, top:bottom, gap] < 200).all() and (near[0, 0, top:bottom, gap] == Df).all()
        assert (canvas[0, :, top:bottom, left + s:right + s] == 255).all() and (near[0, 0, top:bottom, left + s:right + s] == Dn).all()
        rest = np.ones((h, w), bool)
        rest[top:bottom, min(left, left + s):max(right, right + s)] = False
        assert same_bits(canvas[0][:, rest], image[:, rest])


def test_near_fed_back_as_a_disparity_map_is_stable():
    from genpercept_amd import stereo as st
    q = np.arange(65536)
    assert same_bits(st.quantize16((q / 65535.0).astype(np.float32)).astype(np.int64), q)               # the new map quantises to itself
    for case in (CASES[6], CASES[11]):
        h, w, max_s8, edge, space, _ = case
        pred, image, F, table, size = case_inputs(case)
        canvas, holes, near = st.stereo_views_table(image, pred, F, table[:1], (h, w), space, edge, max_s8)
        again, no_holes, same = st.stereo_views_table(canvas, (near[0] / 65535.0).astype(np.float32), F, [[0, 0, 0, 7]], (h, w), "disparity", edge, max_s8)
        assert same_bits(again, canvas) and not no_holes.any() and same_bits(same, near)


# ---- layouts and the user's terms ---------------------------------------------------------------------------------------------------------------------
def test_layouts_are_the_views_in_their_rectangles():
    from genpercept_amd import stereo as st
    rng = np.random.RandomState(8)
    h, w = 6, 40
    scenes = [scene(rng, h, w) for _ in range(2)]
    pred, image = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    kw = dict(separation=24.0, converge=[0.3, 0.6], edge=0.05, space="disparity")

    def one_view(g):
        F = st.nearness(np.float32(kw["converge"]), "disparity")
        return st.stereo_views_table(image, pred, F, [[g, 0, 0, 7]], (h, w), "disparity", int(np.floor(65535 * 0.05 + 0.5)), 512)

    pair, pair_holes, pair_near = st.stereo_views(image, pred, "pair", 2, want_holes=True, want_near=True, **kw)
    assert pair.shape == (2, 3, h, 2 * w) and pair_holes.shape == (2, 2, h, w) and pair_holes.any()
    table, _ = st.view_table("pair", 2, 24.0, h, w)
    for k in range(2):
        canvas, holes, near = one_view(int(table[k, 0]))
        assert same_bits(pair[:, :, :, k * w:(k + 1) * w], canvas) and same_bits(pair_holes[:, k:k + 1], holes) and same_bits(pair_near[:, k:k + 1], near)
    assert same_bits(st.stereo_views(image, pred, "sbs", 2, **kw), pair)
    assert same_bits(st.stereo_views(image, pred, "over_under", 2, **kw), np.concatenate([pair[..., :w], pair[..., w:]], 2))
    assert same_bits(st.stereo_views(image, pred, "anaglyph", 2, **kw), np.concatenate([pair[:, :1, :, :w], pair[:, 1:, :, w:]], 1))
    quilt = st.stereo_views(image, pred, "quilt", (2, 3), **kw)
    table, size = st.view_table("quilt", (2, 3), 24.0, h, w)
    assert size == (2 * h, 3 * w) and quilt.shape == (2, 3, 2 * h, 3 * w) and table[:, 0].tolist() == sorted(table[:, 0].tolist(), reverse=True)
    for k, (g, ox, oy, cmask) in enumerate(table.tolist()):
        assert (ox, oy, cmask) == ((k % 3) * w, (1 - k // 3) * h, 7)
        assert same_bits(quilt[:, :, oy:oy + h, ox:ox + w], one_view(g)[0])
    three = st.stereo_views(image, pred, "sbs", 3, **kw)
    assert three.shape == (2, 3, h, 3 * w) and same_bits(three[..., w:2 * w], one_view(0)[0]) and same_bits(three[..., w:2 * w], image)
    # bytes outside every rectangle and channels outside a mask keep what they held
    fill = np.full((2, 3, h + 5, 2 * w + 9), 0xA5, np.uint8)
    custom = [[20000, 3, 2, 5], [-20000, w + 7, 4, 2], [9000, 3, 2, 2]]
    canvas, _, _ = st.stereo_views_table(image, pred, [1000, 40000], custom, fill, "disparity", 3000, 100)
    assert canvas is fill
    untouched = np.ones(fill.shape, bool)
    for g, ox, oy, cmask in custom:
        view = st.stereo_views_table(image, pred, [1000, 40000], [[g, 0, 0, 7]], (h, w), "disparity", 3000, 100)[0]
        for ch in range(3):
            if cmask >> ch & 1:
                assert same_bits(canvas[:, ch, oy:oy + h, ox:ox + w], view[:, ch])
                untouched[:, ch, oy:oy + h, ox:ox + w] = False
    assert (canvas[untouched] == 0xA5).all() and untouched.sum() == fill.size - 2 * 4 * h * w


def test_the_users_terms_give_the_documented_integers():
    from genpercept_amd import stereo as st
    table, size = st.view_table("sbs", 2, 32.0, 5, 7)
    assert table.dtype == np.int32 and table.tolist() == [[32769, 0, 0, 7], [-32769, 7, 0, 7]] and size == (5, 14)
    table, size = st.view_table("quilt", (3, 3), 32.0, 5, 7)
    assert table[:, 0].tolist() == [32769, 24576, 16384, 8192, 0, -8192, -16384, -24576, -32769] and size == (15, 21)
    assert table[:, 1:].tolist() == [[0, 10, 7], [7, 10, 7], [14, 10, 7], [0, 5, 7], [7, 5, 7], [14, 5, 7], [0, 0, 7], [7, 0, 7], [14, 0, 7]]
    assert st.view_table("anaglyph", 2, -8.0, 5, 7)[0].tolist() == [[-8192, 0, 0, 1], [8192, 0, 0, 6]]
    assert st.view_table("over_under", 3, 1.0, 5, 7) [0].tolist() == [[1024, 0, 0, 7], [0, 0, 5, 7], [-1024, 0, 10, 7]]
    assert st.view_table("sbs", 1, 32.0, 5, 7)[0].tolist() == [[0, 0, 0, 7]]
    assert st.max_shift8([32769, -32769]) == 128 and st.max_shift8([32769], 32768) == 64 and st.max_shift8([131072]) == 512 and st.max_shift8([0]) == 0
    o = st.plan(2, 5, 7, "sbs", 2, 32.0)
    assert (o["edge"], o["max_s8"], o["converge"], o["converge_at"], o["size"]) == (2621, 64, None, None, (5, 14)) and st.EDGE_DEFAULT == 0.04
    assert st.plan(2, 5, 7, "sbs", 2, 32.0, converge=[0.5, 1.0])["max_s8"] == 128 and st.plan(2, 5, 7, "sbs", 2, 32.0, converge_at=(6, 4))["max_s8"] == 128
    pred = np.float32([[[0.25, np.nan]], [[2.0, 0.5]]])
    assert st.convergence(pred, "depth", st.stereo_options(2)).tolist() == [32768, 32768]
    assert st.convergence(pred, "depth", st.stereo_options(2, converge=0.25)).tolist() == [65535 - 16383] * 2
    assert st.convergence(pred, "disparity", st.stereo_options(2, converge_at=[(0, 0), (1, 0)])).tolist() == [16383, 32767]
    assert st.convergence(pred, "depth", st.stereo_options(2, converge_at=(1, 0))).tolist() == [0, 65535 - 32767]
    image = np.zeros((2, 3, 1, 2), np.uint8)
    for bad in (dict(layout="wiggle"), dict(views=0), dict(views=65), dict(views=2.0), dict(layout="pair", views=3), dict(layout="anaglyph", views=1),
                dict(layout="quilt", views=9), dict(layout="quilt", views=(0, 3)), dict(layout="quilt", views=(9, 8)), dict(separation=128.0),
                dict(separation=float("nan")), dict(separation=-200.0), dict(converge=0.5, converge_at=(0, 0)), dict(converge=1.5), dict(converge=[0.1] * 3),
                dict(converge_at=(2, 0)), dict(converge_at=(0, 1)), dict(converge_at=(0.5, 0)), dict(converge_at=3), dict(edge=-0.1), dict(edge=1.5),
                dict(edge=float("nan")), dict(edge=[0.1]), dict(space="metric")):
        with pytest.raises(ValueError):
            st.stereo_views(image, pred, **bad)
    for bad in (dict(image=image.astype(np.float32)), dict(image=image[:, :2]), dict(pred=pred[:1]), dict(pred=np.zeros((2, 1, 1, 2), np.uint8))):
        with pytest.raises(ValueError):
            st.stereo_views(**dict(dict(image=image, pred=pred), **bad))
    ok = dict(image=image, pred=pred, F=0, table=[[0, 0, 0, 7]], canvas=(1, 2))
    for bad in (dict(table=[[131073, 0, 0, 7]]), dict(table=[[0, 0, 0, 0]]), dict(table=[[0, 0, 0, 8]]), dict(table=[[0, 1, 0, 7]]), dict(table=[[0, 0, -1, 7]]),
                dict(table=[[0, 0, 0, 3], [0, 0, 0, 6]]), dict(table=[[0, 0, 0, 7]] * 2, canvas=(1, 3)), dict(table=np.zeros((0, 4), int)), dict(table=[[0.0] * 4]),
                dict(table=[[0, 0, 0]]), dict(edge=65536), dict(edge=-1), dict(max_s8=513), dict(max_s8=-1), dict(F=[0, 0, 0]), dict(F=0.5),
                dict(canvas=np.zeros((2, 3, 1, 2))), dict(canvas=np.zeros((1, 3, 1, 2), np.uint8)), dict(canvas=(0, 2)), dict(space="metric")):
        with pytest.raises(ValueError):
            st.stereo_views_table(**dict(ok, **bad))
    assert st.stereo_views_table(**dict(ok, table=[[0, 0, 0, 1], [0, 1, 0, 6]], canvas=(1, 3)))[0].shape == (2, 3, 1, 3)      # overlap, no common channel
    assert st.stereo_views_table(**dict(ok, F=[-5, 70000]))[1].shape == (2, 1, 1, 2)                                           # F is clamped


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine, infer_eval
    from genpercept_amd.pipeline import GenPerceptPipeline
    hdr, math_h = ps.assert_entries_bound(["gp_stereo_views", "gp_stereo_views_workspace"], "stereo.hip", "stereo_math.h")
    args = engine.SYMBOLS["gp_stereo_views"][1]
    assert len(args) == 19 and args[4:13] == [C.c_int] * 9 and args[17] is C.c_longlong and engine.SYMBOLS["gp_stereo_views"][0] is C.c_int
    assert engine.SYMBOLS["gp_stereo_views_workspace"] == (C.c_longlong, [C.c_int] * 4)
    assert callable(engine.stereo_views) and callable(infer_eval.run_stereo)
    assert callable(GenPerceptPipeline.stereo_batch_device) and callable(GenPerceptPipeline.stereo)
    assert "hip_runtime" not in math_h and "depth-image-based rendering" in hdr
    for lib in _libs():
        assert lib.gp_stereo_views_workspace(2, 3, 5, 7) == 4 * 2 * 3 * 5 * 7 and lib.gp_stereo_views_workspace(1, 1, 1, 1) == 8
        assert lib.gp_stereo_views_workspace(2, 9, 40, 70) == 2 * lib.gp_stereo_views_workspace(1, 9, 40, 70)
        for bad in ((0, 1, 8, 8), (65536, 1, 8, 8), (1, 0, 8, 8), (1, 65, 8, 8), (1, 1, 0, 8), (1, 1, 8, 16385), (2, 4, 16384, 16384)):
            assert lib.gp_stereo_views_workspace(*bad) == 0


def views_array(rows):
    """A host view table the C entry can read: the int32 array (keep it alive) and its address."""
    a = np.ascontiguousarray(np.array(rows, np.int32))
    return a, a.ctypes.data


def stereo_args(b, h, w, **over):
    """A valid argument set of gp_stereo_views for these sizes: two views side by side (pointers as given, small integers by default)."""
    table = views_array([[30000, 0, 0, 7], [-30000, w, 0, 7]])
    ok = dict(image=0x1001, pred=0x2000, conv=0x3000, views=table[1], B=b, V=2, H=h, W=w, CH=h, CW=2 * w, space=0, edge=2600, max_s8=120,
              canvas=0x7003, holes=0x8001, near=0x9002, workspace=0xA000, workspace_bytes=4 * b * 2 * h * w, _keep=[table[0]])
    ok.update(over)
    return ok


def invalid_cases(ok):
    """The argument sets gp_stereo_views refuses, as changes to a valid set `ok` of two views side by side."""
    h, w = ok["H"], ok["W"]

    def table(rows):
        a, ptr = views_array(rows)
        ok["_keep"].append(a)
        return dict(views=ptr, V=len(rows))

    good = [30000, 0, 0, 7]
    return [dict(image=None), dict(pred=None), dict(conv=None), dict(views=None), dict(canvas=None), dict(workspace=None),
            dict(B=0), dict(B=-1), dict(B=65536), dict(V=0), dict(V=65), dict(H=0), dict(W=-5), dict(H=16385), dict(W=16385), dict(CH=0), dict(CW=0),
            dict(CH=16385), dict(CW=16385), dict(B=4096, H=512, W=512, CH=512, CW=1024, workspace_bytes=1 << 40),                     # B V H W = 2^31
            dict(space=2), dict(space=-1), dict(edge=-1), dict(edge=65536), dict(max_s8=-1), dict(max_s8=513),
            table([[131073, 0, 0, 7], good[:1] + [w, 0, 7]]), table([[-131073, 0, 0, 7]]), table([[0, 0, 0, 0]]), table([[0, 0, 0, 8]]),
            table([[0, -1, 0, 7]]), table([[0, 0, -1, 7]]), table([[0, w + 1, 0, 7]]), table([[0, 0, 1, 7]]), dict(CW=2 * w - 1), dict(CH=h - 1),
            table([good, [-30000, w - 1, 0, 7]]), table([good, [-30000, 0, 0, 7]]), table([[0, 0, 0, 3], [0, 0, 0, 6]]),
            dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1), dict(conv=ok["conv"] + 2), dict(conv=ok["conv"] + 1), dict(near=ok["near"] + 1),
            dict(workspace=ok["workspace"] + 4), dict(workspace=ok["workspace"] + 1), dict(workspace_bytes=ok["workspace_bytes"] - 1), dict(workspace_bytes=0),
            dict(canvas=ok["image"])]


def call_stereo(lib, a):
    return lib.gp_stereo_views(a["image"], a["pred"], a["conv"], a["views"], a["B"], a["V"], a["H"], a["W"], a["CH"], a["CW"], a["space"], a["edge"],
                               a["max_s8"], a["canvas"], a["holes"], a["near"], a["workspace"], a["workspace_bytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        ok = stereo_args(2, 40, 70)
        cases = invalid_cases(ok)
        assert len(cases) == 49
        ps.assert_all_refused(call_stereo, lib, ok, cases)


@pytest.fixture
def library_calls(monkeypatch):
    return ps.library_calls(monkeypatch)


def test_the_binding_refuses_bad_tensors_and_options_before_the_library_is_touched(library_calls):
    import torch
    from genpercept_amd import engine
    image, maps = torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.full((2, 1, 8, 8), 0.5)
    for bad in (dict(image=torch.zeros((2, 3, 8, 8))), dict(image=torch.zeros((8, 8), dtype=torch.uint8)), dict(image=torch.zeros((1, 2, 3, 8, 8), dtype=torch.uint8)),
                dict(image=torch.zeros((2, 4, 8, 8), dtype=torch.uint8)), dict(image=image[:1]), dict(image=image[..., :7]), dict(image=image.numpy()),
                dict(pred=torch.zeros((2, 1, 8, 8), dtype=torch.int32)), dict(pred=maps[:, :, :7]), dict(pred=maps.numpy()),
                dict(layout="wiggle"), dict(views=0), dict(views=65), dict(layout="pair", views=3), dict(layout="quilt", views=4), dict(separation=128.0),
                dict(separation=float("inf")), dict(converge=0.5, converge_at=(1, 1)), dict(converge=-0.5), dict(converge=[0.5] * 3), dict(converge_at=(8, 0)),
                dict(converge_at=(0, 8)), dict(converge_at=(1.5, 0)), dict(edge=2.0), dict(edge=-1.0), dict(space="metric"),
                dict(canvas=torch.zeros((2, 3, 8, 15), dtype=torch.uint8)), dict(canvas=torch.zeros((2, 3, 8, 16)))):
        with pytest.raises(ValueError):
            engine.stereo_views(**dict(dict(image=image, pred=maps), **bad))
    assert library_calls == []
    for good in (dict(), dict(converge=0.3), dict(converge_at=(7, 7)), dict(layout="quilt", views=(2, 2), want_holes=True),
                 dict(canvas=torch.zeros((2, 3, 8, 16), dtype=torch.uint8))):
        with pytest.raises(AssertionError):      # CPU tensors get as far as the assert that they are on the device
            engine.stereo_views(image, maps, **good)
    assert library_calls == []
