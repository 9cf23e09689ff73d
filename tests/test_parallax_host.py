"""The camera moves from one photograph on the host (genpercept_amd/parallax.py), without a GPU: the numpy route equals plain scalar loops
written here from the definition and a stand-alone CPU build of the kernels' arithmetic (tests/parallax_check.cpp over csrc/parallax_math.h,
built with the ROCm clang++ under the address and undefined-behaviour sanitizers and run as a child process, which offers every piece of the
image to every pixel and holds the device's staging bounds to that search); a meta-test that the cases met every branch of the definition;
the properties the definition is for, with exact expectations; the user's terms; the entries declared, exported, bound, their argument
checks with NULL buffers, and the binding's own refusals.  There is no tolerance in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, libs as _libs, same_bits  # noqa: E402,F401

SIZES = [(1, 1), (5, 7), (33, 65), (40, 19)]
ZOOMS = (65536, 80000, 131072)
# H, W, max_s8, edge, space, NaN block: every size with every max_s8 of {0, 8, 40, 256}; every case renders three frames, one at each zoom of
# ZOOMS; edge 0, a middle value and 65535; both spaces; with and without NaN pixels
CASES = [(h, w, m, e, sp, nan) for i, (h, w) in enumerate(SIZES) for j, m in enumerate((0, 8, 40, 256))
         for e, sp, nan in [((2600, 0, 65535)[(i + j) % 3], ("depth", "disparity")[(i + j // 2) % 2], (i + j) % 2 == 1)]]
CASE_ID = lambda c: "%dx%d-s%d-e%d-%s%s" % (c[:5] + ("-nan" if c[5] else "",))  # noqa: E731


def scene(rng, h, w, nan=False):
    """One image: (pred float32 [h, w], a surface of planar patches -- blocks of 1 to 12 pixels on a side, each with a random base and two
    slopes, values beyond [0, 1] among them, a block of NaNs on request; image uint8 [3, h, w])."""
    pred = np.empty((h, w), np.float64)
    y = 0
    while y < h:
        n = rng.randint(1, 13)
        x = 0
        while x < w:
            m = rng.randint(1, 13)
            patch = rng.uniform(-0.05, 1.05) + rng.uniform(-0.02, 0.02) * np.arange(n)[:, None] + rng.uniform(-0.02, 0.02) * np.arange(m)[None]
            pred[y:y + n, x:x + m] = patch[: h - y, : w - x]
            x += m
        y += n
    if nan:
        pred[h // 3: h // 3 + 2, w // 4: w // 4 + 5] = np.nan
    return pred.astype(np.float32), rng.randint(0, 256, (3, h, w)).astype(np.uint8)


def case_inputs(case):
    """pred, image, F and three frames: gains whose largest displacement is about one and a half times max_s8, so that the clamp is met, in
    both directions, with and without a dolly, one frame at each zoom."""
    h, w, max_s8, edge, space, nan = case
    rng = np.random.RandomState(1000 * h + 10 * w + max_s8 % 97)
    pred, image = scene(rng, h, w, nan)
    g = min(131072, int(1.5 * max_s8 * 16777216 / 65535)) if max_s8 else 40000
    g = g if rng.rand() < 0.5 else -g
    gz = min(1 << 24, int(max_s8 * 65536 / max(1, 4 * (max(h, w) - 1)) * 256)) if max_s8 else 1 << 20
    F = int(rng.randint(0, 65536))
    table = [[g, -g // 2, 0, ZOOMS[0]], [-g // 3, g, gz, ZOOMS[1]], [g // 2, g // 4, -gz, ZOOMS[2]]]
    return pred, image, F, table


# ---- the definition once more, in plain loops ---------------------------------------------------------------------------------------------------------
def loops_frames(image, pred, F, table, space, edge, max_s8):
    """Steps 1 to 6 for one image [3, h, w]: every cap and every triangle is scattered over the pixels between the smallest and the largest
    coordinates of its corners.  Returns (frames [V][3][h][w], holes, near, cover, piece [V][h][w])."""
    _, h, w = image.shape
    D = ps.loops_nearness(pred, space)
    img = image.astype(int).tolist()
    R = max_s8 // 4 + 1
    Cx, Cy = 4 * (w - 1), 4 * (h - 1)
    clamp = lambda v: max(-max_s8, min(max_s8, v))  # noqa: E731
    res = []
    for gx, gy, gz, Z in table:
        T = [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                rx, ry, e = 8 * x - Cx, 8 * y - Cy, D[y][x] - F
                dz = (e * gz + (1 << 23)) >> 24
                dx = clamp(((e * gx + (1 << 23)) >> 24) + ((rx * dz + (1 << 15)) >> 16))
                dy = clamp(((e * gy + (1 << 23)) >> 24) + ((ry * dz + (1 << 15)) >> 16))
                T[y][x] = (Cx + ((rx * Z + (1 << 15)) >> 16) + dx, Cy + ((ry * Z + (1 << 15)) >> 16) + dy)
        best = [[-1] * w for _ in range(h)]
        who, rgb, cnt = [[-1] * w for _ in range(h)], [[None] * w for _ in range(h)], [[0] * w for _ in range(h)]

        def offer(p, q, value, ident, colour):
            cnt[q][p] += 1
            if value > best[q][p] or (value == best[q][p] and ident < who[q][p]):
                best[q][p], who[q][p], rgb[q][p] = value, ident, colour

        hc = (4 * Z + 65535) >> 16
        conn = lambda a, b: abs(D[a[0]][a[1]] - D[b[0]][b[1]]) <= edge  # noqa: E731
        for y in range(h):
            for x in range(w):
                ident = 3 * (y * w + x)
                tx, ty = T[y][x]
                for q in range(max(0, (ty - hc) // 8), min(h, (ty + hc) // 8 + 1)):
                    for p in range(max(0, (tx - hc) // 8), min(w, (tx + hc) // 8 + 1)):
                        if tx - hc <= 8 * p < tx + hc and ty - hc <= 8 * q < ty + hc:
                            offer(p, q, D[y][x], ident, [img[k][y][x] for k in range(3)])
                if x + 1 >= w or y + 1 >= h:
                    continue
                for t, corners in enumerate((((y, x), (y, x + 1), (y + 1, x)), ((y, x + 1), (y + 1, x + 1), (y + 1, x)))):
                    a, b, c = corners
                    if not (conn(a, b) and conn(b, c) and conn(a, c)):
                        continue
                    (ax, ay), (bx, by), (cx, cy) = (T[v[0]][v[1]] for v in corners)
                    A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
                    if A <= 0:
                        continue
                    Dv = [D[v[0]][v[1]] for v in corners]
                    for q in range(max(0, min(ay, by, cy) // 8), min(h, max(ay, by, cy) // 8 + 1)):
                        for p in range(max(0, min(ax, bx, cx) // 8), min(w, max(ax, bx, cx) // 8 + 1)):
                            Px, Py = 8 * p, 8 * q
                            wa = (cx - bx) * (Py - by) - (cy - by) * (Px - bx)
                            wb = (ax - cx) * (Py - cy) - (ay - cy) * (Px - cx)
                            wc = A - wa - wb
                            if wa < 0 or wb < 0 or wc < 0:
                                continue
                            mix = lambda va, vb, vc: (wa * va + wb * vb + wc * vc + (A >> 1)) // A  # noqa: E731
                            offer(p, q, mix(*Dv), ident + 1 + t, [mix(*(img[k][v[0]][v[1]] for v in corners)) for k in range(3)])
        out = [[[0] * w for _ in range(h)] for _ in range(3)]
        holes, near = [[0] * w for _ in range(h)], [[0] * w for _ in range(h)]
        for q in range(h):
            for p in range(w):
                value, colour = best[q][p], rgb[q][p]
                if value < 0:
                    holes[q][p] = 1
                    found = []
                    for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1)):                                   # left, right, up, down
                        for d in range(1, R + 1):
                            xx, yy = p + d * sx, q + d * sy
                            if not (0 <= xx < w and 0 <= yy < h):
                                break
                            if best[yy][xx] >= 0:
                                found.append((best[yy][xx], rgb[yy][xx]))
                                break
                    value, colour = (0, [0, 0, 0]) if not found else min(found, key=lambda v: v[0])     # (min keeps the first of equals)
                near[q][p] = value
                for k in range(3):
                    out[k][q][p] = colour[k]
        res.append((out, holes, near, cnt, who))
    return (np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res], np.uint8), np.array([r[2] for r in res], np.uint16),
            np.array([r[3] for r in res], np.int64), np.array([r[4] for r in res], np.int64))


def host_frames(case):
    from genpercept_amd import parallax as pv
    h, w, max_s8, edge, space, nan = case
    pred, image, F, table = case_inputs(case)
    return pv.parallax_frames_table(image, pred, F, table, space, edge, max_s8, want_stats=True)


@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_host_route_equals_plain_loops(case):
    h, w, max_s8, edge, space, nan = case
    pred, image, F, table = case_inputs(case)
    frames, holes, near, stats = host_frames(case)
    want = loops_frames(image, pred, F, table, space, edge, max_s8)
    cover, piece = np.stack([s["cover"] for s in stats[0]]), np.stack([s["piece"] for s in stats[0]])
    assert same_bits(cover, want[3]) and same_bits(piece, want[4]) and same_bits(holes[0], want[1]) and same_bits(near[0], want[2]), case
    assert same_bits(frames[0], want[0]), case


def test_the_cases_met_every_condition():
    """Across the cases above the host result shows a folded triangle, a tie decided by the piece id, a cap that beats a triangle, a clamped
    displacement, a hole with no neighbour and a hole filled from each of the four directions; how many cases show each."""
    names = ("folded", "tie", "cap_over_triangle", "clamped", "alone", "from_left", "from_right", "from_up", "from_down")
    seen = dict.fromkeys(names, 0)
    for case in CASES:
        _, holes, _, stats = host_frames(case)
        met = dict.fromkeys(names, False)
        for k, s in enumerate(stats[0]):
            hole = holes[0, k] == 1
            met["folded"] |= s["folded"] > 0
            met["tie"] |= bool((s["ties"] >= 2).any())
            met["cap_over_triangle"] |= bool(((s["piece"] >= 0) & (s["piece"] % 3 == 0) & (s["triangles"] >= 1)).any())
            met["clamped"] |= s["clamped"]
            met["alone"] |= bool((hole & (s["filled_from"] < 0)).any())
            for d, name in enumerate(names[5:]):
                met[name] |= bool((hole & (s["filled_from"] == d)).any())
        for name in names:
            seen[name] += bool(met[name])
    print(seen)
    assert all(n >= 1 for n in seen.values()), seen


# ---- the kernels' arithmetic on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return ps.build_check(tmp_path_factory, "parallax_check.cpp")


def run_check_program(check_exe, tmp_path, name, image, pred, F, table, space, edge, max_s8):
    from genpercept_amd import parallax as pv
    h, w = pred.shape
    v = len(table)
    src, dst = str(tmp_path / f"in{name}.bin"), str(tmp_path / f"out{name}.bin")
    with open(src, "wb") as f:
        f.write(np.array([h, w, pv.SPACES.index(space), edge, max_s8, v, F], np.int32).tobytes() + np.array(table, np.int32).tobytes() + pred.tobytes()
                + image.tobytes())
    raw = ps.run_check(check_exe, src, dst, timeout=300)[1]
    n = v * h * w
    assert len(raw) == 3 * n + n + 2 * n + 4 * n + 4 * n
    return (np.frombuffer(raw[:3 * n], np.uint8).reshape(v, 3, h, w), np.frombuffer(raw[3 * n:4 * n], np.uint8).reshape(v, h, w),
            np.frombuffer(raw[4 * n:6 * n], np.uint16).reshape(v, h, w), np.frombuffer(raw[6 * n:10 * n], np.int32).reshape(v, h, w),
            np.frombuffer(raw[10 * n:], np.int32).reshape(v, h, w))


@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_cpu_build_of_the_kernel_arithmetic_equals_the_host_route(check_exe, case, tmp_path):
    h, w, max_s8, edge, space, nan = case
    pred, image, F, table = case_inputs(case)
    got = run_check_program(check_exe, tmp_path, "a", image, pred, F, table, space, edge, max_s8)
    frames, holes, near, stats = host_frames(case)
    cover, piece = np.stack([s["cover"] for s in stats[0]]), np.stack([s["piece"] for s in stats[0]])
    assert same_bits(got[3].astype(np.int64), cover) and same_bits(got[4].astype(np.int64), piece)
    assert same_bits(got[0], frames[0]) and same_bits(got[1], holes[0]) and same_bits(got[2], near[0])


# ---- what the definition is for -----------------------------------------------------------------------------------------------------------------------
def test_the_identity_frame_returns_the_image():
    from genpercept_amd import parallax as pv
    rng = np.random.RandomState(5)
    pred, image = scene(rng, 19, 70, nan=True)
    for space in pv.SPACES:
        for edge in (0, 3000, 65535):
            frames, holes, near = pv.parallax_frames_table(image, pred, 12345, [[0, 0, 0, 65536]], space, edge, 256)
            assert same_bits(frames[0, 0], image) and not holes.any() and same_bits(near[0, 0], pv.nearness(pred, space).astype(np.uint16))
    out = pv.parallax_frames(image, pred, "orbit", 3, amount=0.0)
    assert out.shape == (1, 3, 3, 19, 70) and all(same_bits(out[0, k], image) for k in range(3))


def test_a_constant_map_moves_the_image_by_whole_pixels():
    from genpercept_amd import parallax as pv
    image = np.random.RandomState(6).randint(0, 256, (3, 9, 40)).astype(np.uint8)
    pred = np.full((9, 40), 0.25, np.float32)
    D = int(pv.nearness(pred, "disparity")[0, 0])
    assert D == 16383
    for cols, rows in ((2, 0), (-3, 1), (5, -2)):
        gain = lambda n: next(g for g in range(0, 131073) if (D * g + (1 << 23)) >> 24 == 8 * abs(n)) * (1 if n > 0 else -1)  # noqa: E731
        gx, gy = gain(cols), gain(rows)
        for edge in (0, 65535):
            frames, holes, near = pv.parallax_frames_table(image, pred, 0, [[gx, gy, 0, 65536]], "disparity", edge, 64)
            x0, x1, y0, y1 = max(0, cols), 40 + min(0, cols), max(0, rows), 9 + min(0, rows)
            assert same_bits(frames[0, 0, :, y0:y1, x0:x1], image[:, y0 - rows:y1 - rows, x0 - cols:x1 - cols])
            strip = np.ones((9, 40), bool)
            strip[y0:y1, x0:x1] = False
            assert same_bits(holes[0, 0], strip.astype(np.uint8))
            # a hole with a covered pixel in its row or column takes the nearness D; the corner the move exposes in both directions has none
            corner = np.ones((9, 40), bool)
            corner[y0:y1], corner[:, x0:x1] = False, False
            assert (near[0, 0][~corner] == D).all() and not near[0, 0][corner].any() and not frames[0, 0][:, corner].any()


def test_one_row_without_connections_is_the_stereo_view():
    """A one-row image has no triangles, so its surface is all caps: gp_stereo_views' row with every pair cut (edge 0, neighbours that
    differ).  gy = gz = 0 and Z = 65536 then give that view, hole filling included."""
    from genpercept_amd import parallax as pv
    from genpercept_amd import stereo as st
    rng = np.random.RandomState(9)
    w = 90
    pred = (rng.permutation(w) / float(w)).astype(np.float32)[None]
    image = rng.randint(0, 256, (3, 1, w)).astype(np.uint8)
    for space in pv.SPACES:
        assert (np.diff(pv.nearness(pred, space)[0]) != 0).all()
        for g, max_s8 in ((50000, 256), (-131072, 256), (20000, 40), (0, 0)):
            frames, holes, near = pv.parallax_frames_table(image, pred, 30000, [[g, 0, 0, 65536]], space, 0, max_s8)
            canvas, want_holes, want_near = st.stereo_views_table(image, pred, 30000, [[g, 0, 0, 7]], (1, w), space, 0, max_s8)
            assert same_bits(frames[:, 0], canvas) and same_bits(holes, want_holes) and same_bits(near, want_near) and (g == 0 or holes.any())


def test_a_near_square_over_a_far_plane():
    """depth space, the plane that stays put on the background: the square moves, the background stays.  The holes open only on the side the
    move uncovers, and every filled byte is a background neighbour's, never the square's."""
    from genpercept_amd import parallax as pv
    h, w, top, bottom, left, right, move = 24, 48, 8, 17, 18, 30, 4
    pred = np.full((h, w), 0.9, np.float32)
    pred[top:bottom, left:right] = 0.1
    image = np.random.RandomState(7).randint(0, 200, (3, h, w)).astype(np.uint8)
    image[:, top:bottom, left:right] = 255
    Dn, Df = (int(v) for v in pv.nearness(np.float32([0.1, 0.9]), "depth"))
    gain = next(g for g in range(131073) if ((Dn - Df) * g + (1 << 23)) >> 24 == 8 * move)
    for gx, gy in ((gain, 0), (-gain, 0), (0, gain), (0, -gain), (gain, -gain)):
        sx, sy = move * np.sign(gx), move * np.sign(gy)
        frames, holes, near = pv.parallax_frames_table(image, pred, Df, [[gx, gy, 0, 65536]], "depth", 3000, 64)
        was, now = np.zeros((h, w), bool), np.zeros((h, w), bool)
        was[top:bottom, left:right], now[top + sy:bottom + sy, left + sx:right + sx] = True, True
        assert same_bits(holes[0, 0], (was & ~now).astype(np.uint8))                                   # what the square left behind, nothing else
        gap = holes[0, 0] == 1
        assert (frames[0, 0][:, gap] < 200).all() and (near[0, 0][gap] == Df).all()
        assert (frames[0, 0][:, now] == 255).all() and (near[0, 0][now] == Dn).all()
        rest = ~(was | now)
        assert same_bits(frames[0, 0][:, rest], image[:, rest])


def test_overscan_leaves_no_hole_on_a_constant_map():
    from genpercept_amd import parallax as pv
    image = np.random.RandomState(8).randint(0, 256, (3, 33, 47)).astype(np.uint8)
    for value in (0.0, 0.3, 1.0):
        pred = np.full((33, 47), value, np.float32)
        for kw in (dict(path="orbit", frames=8, amount=6.0), dict(path="swing", frames=5, amount=-5.0), dict(path="dolly", frames=4, push=0.05, zoom=1.2, pan=True,
                                                                                                              amount=4.0)):
            for focus in (None, 0.8):
                _, holes = pv.parallax_frames(image, pred, focus=focus, want_holes=True, **kw)
                assert not holes.any(), (value, kw, focus)
    bare = pv.parallax_frames(image, np.zeros((33, 47), np.float32), "orbit", 8, amount=6.0, overscan=False, want_holes=True)[1]
    assert bare.any()


# ---- the user's terms ---------------------------------------------------------------------------------------------------------------------------------
def test_the_users_terms_give_the_documented_integers():
    from genpercept_amd import parallax as pv
    assert pv.amount_gain(16.0) == 32769 and pv.amount_gain(0.0) == 0 and pv.amount_gain(-16.0) == -32769
    assert pv.camera_path("orbit", 4, 16.0).tolist() == [[-16385, 0, 0, 65536], [0, -16385, 0, 65536], [16384, 0, 0, 65536], [0, 16384, 0, 65536]]
    assert pv.camera_path("swing", 4, 16.0).tolist() == [[0, 0, 0, 65536], [-16385, 0, 0, 65536], [0, 0, 0, 65536], [16384, 0, 0, 65536]]
    assert pv.camera_path("dolly", 3, 16.0, push=0.5, zoom=1.5).tolist() == [[0, 0, 0, 65536], [0, 0, 1 << 22, 81920], [0, 0, 1 << 23, 98304]]
    assert pv.camera_path("dolly", 3, 16.0, zoom=1.25, pan=True)[:, 0].tolist() == [-16384, 0, 16385]
    assert pv.camera_path("dolly", 1, 16.0, push=0.5, zoom=1.5).tolist() == [[0, 0, 0, 65536]]
    assert pv.camera_path([[16.0, -8.0, 0.25, 1.5], [0, 0, 0, 1]]).tolist() == [[32769, -16384, 1 << 22, 98304], [0, 0, 0, 65536]]
    assert pv.frame_bounds8([[32769, 0, 0, 65536], [0, -16385, 0, 65536]], 5, 7).tolist() == [128, 64]
    assert pv.frame_bounds8([[32769, 0, 0, 65536]], 5, 7, 32768).tolist() == [64]
    assert pv.frame_bounds8([[0, 0, 1 << 22, 65536]], 101, 201).tolist() == [(800 * 16384 + 32768) >> 16]           # C = 800, dzmax = 16384
    o = pv.plan(2, 101, 201, "orbit", 4, 16.0)
    assert (o["edge"], o["max_s8"], o["focus"], o["focus_at"], o["n_path"]) == (2621, 32, None, None, 4) and o["table"].dtype == np.int32
    assert o["table"].tolist() == [[-16385, 0, 0, 65536 + 5243], [0, -16385, 0, 65536 + 5243], [16384, 0, 0, 65536 + 5243], [0, 16384, 0, 65536 + 5243]]
    assert pv.plan(2, 101, 201, "orbit", 4, 16.0, overscan=False)["table"][:, 3].tolist() == [65536] * 4
    assert pv.plan(2, 101, 201, "orbit", 4, 16.0, focus=[0.5, 1.0])["max_s8"] == 64 and pv.plan(2, 101, 201, "orbit", 4, 16.0, focus_at=(6, 4))["max_s8"] == 64
    part = pv.plan(1, 101, 201, "orbit", 100, 16.0, frame_range=(64, 100))
    assert part["n_path"] == 100 and same_bits(part["table"], pv.plan(1, 101, 201, "orbit", 100, 16.0, frame_range=(40, 100))["table"][24:])
    pred = np.float32([[[0.25, np.nan]], [[2.0, 0.5]]])
    assert pv.focus_plane(pred, "depth", pv.plan(2, 1, 2, amount=0.0)).tolist() == [32768, 32768]
    assert pv.focus_plane(pred, "disparity", pv.plan(2, 1, 2, amount=0.0, focus_at=[(0, 0), (1, 0)])).tolist() == [16383, 32767]
    assert pv.focus_plane(pred, "depth", pv.plan(2, 1, 2, amount=0.0, focus=0.25)).tolist() == [65535 - 16383] * 2
    image8, pred8 = np.zeros((2, 3, 8, 8), np.uint8), np.zeros((2, 8, 8), np.float32)
    for bad in (dict(path="wiggle"), dict(frames=0), dict(frames=4097), dict(frames=2.0), dict(frames=65), dict(amount=float("nan")), dict(amount=130.0),
                dict(amount=100.0, focus=1.0), dict(path="dolly", zoom=2.5), dict(path="dolly", zoom=0.9), dict(path="dolly", push=2.0),
                dict(path="dolly", push=float("inf")), dict(path=[[0, 0, 0, 0.5]]), dict(path=[[0, 0, 0, 2.1]]), dict(path=[[0, 0, 0]]), dict(path=np.zeros((0, 4))),
                dict(path=[[70.0, 0, 0, 1]]), dict(frame_range=(0, 0)), dict(frame_range=(3, 17)), dict(frame_range=(-1, 4)),
                dict(focus=0.5, focus_at=(0, 0)), dict(focus=1.5), dict(focus=[0.1] * 3), dict(focus_at=(8, 0)), dict(focus_at=(0, 8)), dict(focus_at=(0.5, 0)),
                dict(edge=-0.1), dict(edge=1.5), dict(edge=float("nan")), dict(space="metric"), dict(overscan=True)):
        with pytest.raises(ValueError):
            pv.parallax_frames(image8, pred8, **dict(dict(overscan=False), **bad))
    # the last one: 4 pixels of displacement on an 8 x 8 image need a zoom of 1 + 8 / 7 under overscan; without it the path is taken as it is
    assert pv.parallax_frames(image8, pred8, overscan=False).shape == (2, 16, 3, 8, 8)
    assert pv.parallax_frames(image8, pred8, amount=100.0, overscan=False).shape == (2, 16, 3, 8, 8) and pv.plan(2, 8, 8, amount=127.0, overscan=False)["max_s8"] == 254
    image = np.zeros((2, 3, 1, 2), np.uint8)
    for bad in (dict(image=image.astype(np.float32)), dict(image=image[:, :2]), dict(pred=pred[:1]), dict(pred=np.zeros((2, 1, 1, 2), np.uint8))):
        with pytest.raises(ValueError):
            pv.parallax_frames(**dict(dict(image=image, pred=pred, amount=0.0), **bad))
    ok = dict(image=image, pred=pred, F=0, table=[[0, 0, 0, 65536]])
    for bad in (dict(table=[[131073, 0, 0, 65536]]), dict(table=[[0, -131073, 0, 65536]]), dict(table=[[0, 0, (1 << 24) + 1, 65536]]), dict(table=[[0, 0, 0, 65535]]),
                dict(table=[[0, 0, 0, 131073]]), dict(table=[[0, 0, 0, 65536]] * 65), dict(table=np.zeros((0, 4), int)), dict(table=[[0.0, 0, 0, 65536.0]]),
                dict(table=[[0, 0, 0]]), dict(edge=65536), dict(edge=-1), dict(max_s8=257), dict(max_s8=-1), dict(F=[0, 0, 0]), dict(F=0.5), dict(space="metric")):
        with pytest.raises(ValueError):
            pv.parallax_frames_table(**dict(ok, **bad))
    assert pv.parallax_frames_table(**dict(ok, F=[-5, 70000]))[1].shape == (2, 1, 1, 2)                  # F is clamped


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine, infer_eval
    from genpercept_amd.pipeline import GenPerceptPipeline
    hdr, math_h = ps.assert_entries_bound(["gp_parallax_frames", "gp_parallax_frames_workspace"], "parallax.hip", "parallax_math.h")
    args = engine.SYMBOLS["gp_parallax_frames"][1]
    assert len(args) == 17 and args[4:11] == [C.c_int] * 7 and args[15] is C.c_longlong and engine.SYMBOLS["gp_parallax_frames"][0] is C.c_int
    assert engine.SYMBOLS["gp_parallax_frames_workspace"] == (C.c_longlong, [C.c_int] * 4)
    assert callable(engine.parallax_frames) and callable(infer_eval.run_parallax)
    assert callable(GenPerceptPipeline.parallax_batch_device) and callable(GenPerceptPipeline.parallax)
    assert "hip_runtime" not in math_h and '#include "stereo_math.h"' in math_h and "3-D Ken" in hdr
    for name in ("st_nearness", "st_connected", "st_rgb", "gs_quant16"):                                 # reused, not copied
        assert not any(line.lstrip().startswith(("ST_HD", "GS_HD", "PV_HD")) and name + "(" in line.split("{")[0] for line in math_h.splitlines()), name
    for lib in _libs():
        assert lib.gp_parallax_frames_workspace(2, 3, 5, 7) == 4 * 2 * 3 * 5 * 7 and lib.gp_parallax_frames_workspace(1, 1, 1, 1) == 8
        assert lib.gp_parallax_frames_workspace(2, 9, 40, 70) == 2 * lib.gp_parallax_frames_workspace(1, 9, 40, 70)
        for bad in ((0, 1, 8, 8), (65536, 1, 8, 8), (1, 0, 8, 8), (1, 65, 8, 8), (1, 1, 0, 8), (1, 1, 8, 16385), (2, 4, 16384, 16384)):
            assert lib.gp_parallax_frames_workspace(*bad) == 0


def frames_array(rows):
    """A host frame table the C entry can read: the int32 array (keep it alive) and its address."""
    a = np.ascontiguousarray(np.array(rows, np.int32))
    return a, a.ctypes.data


def parallax_args(b, h, w, **over):
    """A valid argument set of gp_parallax_frames for these sizes: two frames (pointers as given, small integers by default)."""
    table = frames_array([[30000, -20000, 100000, 70000], [-30000, 10000, 0, 65536]])
    ok = dict(image=0x1001, pred=0x2000, focus=0x3000, frames=table[1], B=b, V=2, H=h, W=w, space=0, edge=2600, max_s8=120, out=0x7003, holes=0x8001,
              near=0x9002, workspace=0xA000, workspace_bytes=4 * b * 2 * h * w, _keep=[table[0]])
    ok.update(over)
    return ok


def invalid_cases(ok):
    """The argument sets gp_parallax_frames refuses, as changes to a valid set `ok` of two frames."""

    def table(rows):
        a, ptr = frames_array(rows)
        ok["_keep"].append(a)
        return dict(frames=ptr, V=len(rows))

    good = [30000, 0, 0, 65536]
    return [dict(image=None), dict(pred=None), dict(focus=None), dict(frames=None), dict(out=None), dict(workspace=None),
            dict(B=0), dict(B=-1), dict(B=65536), dict(V=0), dict(V=65), dict(H=0), dict(W=-5), dict(H=16385), dict(W=16385),
            dict(B=4096, H=512, W=512, workspace_bytes=1 << 40),                                           # B V H W = 2^31
            dict(space=2), dict(space=-1), dict(edge=-1), dict(edge=65536), dict(max_s8=-1), dict(max_s8=257),
            table([[131073, 0, 0, 65536], good]), table([good, [-131073, 0, 0, 65536]]), table([[0, 131073, 0, 65536]]), table([[0, -131073, 0, 65536]]),
            table([[0, 0, (1 << 24) + 1, 65536]]), table([[0, 0, -(1 << 24) - 1, 65536]]), table([[0, 0, 0, 65535]]), table([[0, 0, 0, 131073]]),
            table([good, [0, 0, 0, 0]]),
            dict(pred=ok["pred"] + 2), dict(pred=ok["pred"] + 1), dict(focus=ok["focus"] + 2), dict(focus=ok["focus"] + 1), dict(near=ok["near"] + 1),
            dict(workspace=ok["workspace"] + 4), dict(workspace=ok["workspace"] + 1), dict(workspace_bytes=ok["workspace_bytes"] - 1), dict(workspace_bytes=0),
            dict(out=ok["image"])]


def call_parallax(lib, a):
    return lib.gp_parallax_frames(a["image"], a["pred"], a["focus"], a["frames"], a["B"], a["V"], a["H"], a["W"], a["space"], a["edge"], a["max_s8"], a["out"],
                                  a["holes"], a["near"], a["workspace"], a["workspace_bytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        ok = parallax_args(2, 40, 70)
        cases = invalid_cases(ok)
        assert len(cases) == 41
        ps.assert_all_refused(call_parallax, lib, ok, cases)


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
                dict(path="wiggle"), dict(frames=0), dict(frames=65), dict(amount=130.0), dict(amount=float("inf")), dict(path="dolly", zoom=3.0),
                dict(path="dolly", zoom=0.5), dict(frame_range=(0, 17)), dict(focus=0.5, focus_at=(1, 1)), dict(focus=-0.5), dict(focus=[0.5] * 3),
                dict(focus_at=(8, 0)), dict(focus_at=(0, 8)), dict(focus_at=(1.5, 0)), dict(edge=2.0), dict(edge=-1.0), dict(space="metric"),
                dict(out=torch.zeros((2, 4, 3, 8, 7), dtype=torch.uint8)), dict(out=torch.zeros((2, 4, 3, 8, 8)))):
        with pytest.raises(ValueError):
            engine.parallax_frames(**dict(dict(image=image, pred=maps, frames=4, amount=1.0, overscan=False), **bad))
    assert library_calls == []
    for good in (dict(), dict(focus=0.3), dict(focus_at=(7, 7)), dict(path="dolly", zoom=1.5, want_holes=True), dict(out=torch.zeros((2, 4, 3, 8, 8), dtype=torch.uint8))):
        with pytest.raises(AssertionError):      # CPU tensors get as far as the assert that they are on the device
            engine.parallax_frames(image, maps, **dict(dict(frames=4, amount=1.0, overscan=False), **good))
    assert library_calls == []
