"""Trimap and boundary bands (gp_mask_band), the host half: eval_metrics.mask_band against a brute-force all-pairs distance and against
scipy.ndimage morphology; trimap_metrics and boundary_iou; the loop options `trimap_radius` / `boundary_iou` of infer_eval with stub pipeline
and evaluators; the header, the two libraries and the ctypes table carry the new entry; the argument checks of the entry (they come before
the first HIP call, so they run without a GPU).  Everything here is integers or one division of integers: every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_eval_mask_host as tm  # noqa: E402  (make_tree, FakePipe, numpy_evaluator, trimap_region: the mask loop's fixtures)
from post_support import libs as _libs  # noqa: E402

NAMES = ("gp_mask_band_workspace", "gp_mask_band")
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
TRIMAP_METRICS = ["mae_t", "mse_t", "sad_t", "sad_fg", "sad_bg"]
BOUNDARY_METRICS = ["biou"]
PLANES = ["band", "fg", "bg", "inner", "trimap"]
GP_ERR_INVALID = 1
THRESHOLDS = [(0, 255), (128, 129), (127, 128), (-1, 256)]
REACHES = [(0, 0), (0, 1), (0, 2), (0, 8), (0, 10 ** 6), (1, 1), (1, 3)]  # (metric, reach)


def random_map(rng, h, w):
    """Plateaus of 0 and 255 with transitional bytes (1, 127, 128, 129, 254 among them) sprinkled in."""
    a = np.where(rng.rand(h, w) < 0.5, 0, 255).astype(np.uint8)
    if h > 2 and w > 2 and rng.rand() < 0.7:
        y, x = rng.randint(0, h - 1), rng.randint(0, w - 1)
        a[y:y + rng.randint(1, h), x:x + rng.randint(1, w)] = rng.choice([0, 255])
    sel = rng.rand(h, w) < 0.15
    a[sel] = rng.choice([1, 64, 127, 128, 129, 200, 254], size=int(sel.sum()))
    return a


def brute_band(a, lo, hi, reach, metric, border):
    """The definition, literally: all-pairs distances to A and to Bc; with border the outside pixels of a frame wide enough to hold the nearest
    one join Bc."""
    h, w = a.shape
    ai = a.astype(np.int64)
    ys, xs = np.mgrid[0:h, 0:w]

    def dist(py, px):                                                # -> [H, W]: the distance to the nearest of the points, inf without points
        if len(py) == 0:
            return np.full((h, w), np.inf)
        dy, dx = np.abs(ys[..., None] - py[None, None]), np.abs(xs[..., None] - px[None, None])
        return (dy * dy + dx * dx if metric == 0 else np.maximum(dy, dx)).min(axis=-1).astype(np.float64)

    d_a = dist(*np.nonzero(ai > lo))
    by, bx = np.nonzero(ai < hi)
    if border:
        m = max(h, w)                                                # the nearest outside pixel is at most min(h, w) / 2 + 1 away
        fy, fx = np.mgrid[-m:h + m, -m:w + m]
        out = (fy < 0) | (fy >= h) | (fx < 0) | (fx >= w)
        by, bx = np.concatenate([by, fy[out]]), np.concatenate([bx, fx[out]])
    d_b = dist(by, bx)
    near_a, near_b = d_a <= reach, d_b <= reach
    u8 = lambda s: (s * 255).astype(np.uint8)
    band = near_a & near_b
    return dict(band=u8(band), fg=u8(~near_b), bg=u8(~near_a), inner=u8((ai > lo) & near_b),
                trimap=np.where(band, 128, np.where(near_a, 255, 0)).astype(np.uint8))


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    from genpercept_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
        assert lib.gp_abi_version() == 3
    assert "mask_band.hip" in SOURCES and "#define GP_ABI_VERSION 3" in hdr
    assert len(engine.SYMBOLS["gp_mask_band"][1]) == 18 and engine.SYMBOLS["gp_mask_band_workspace"] == (C.c_longlong, [C.c_int] * 3)
    assert callable(engine.mask_band) and callable(engine.eval_trimap) and callable(engine.eval_boundary_iou)
    assert list(engine.TRIMAP_METRICS) == list(em.TRIMAP_METRICS) == list(ie.TRIMAP_METRICS) == TRIMAP_METRICS
    assert list(engine.BOUNDARY_METRICS) == list(em.BOUNDARY_METRICS) == list(ie.BOUNDARY_METRICS) == BOUNDARY_METRICS
    assert list(engine.BAND_PLANES) == list(em.BAND_PLANES) == PLANES
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in NAMES)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert lib.gp_mask_band_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (1024, 1024), (1031, 2053), (3, 8200)):
            one = lib.gp_mask_band_workspace(1, h, w)
            assert 4 * h * w <= one <= 4 * h * w + 8 and one % 8 == 0          # one 32-bit word per pixel
            assert lib.gp_mask_band_workspace(7, h, w) == 7 * one and lib.gp_mask_band_workspace(65535, h, w) == 65535 * one


def invalid_cases(ok, need_one):
    """The argument sets gp_mask_band refuses, as changes to a valid set `ok`."""
    huge = 1 << 62
    return [dict(a=None), dict(ws=None), dict(band=None, fg=None, bg=None, inner=None, trimap=None),
            dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
            dict(B=65536, nbytes=huge),
            dict(B=1, H=65536, W=65536, nbytes=huge), dict(B=1, H=1 << 16, W=1 << 15, nbytes=huge),      # H * W > 2^31 - 1
            dict(u8=-1), dict(u8=2), dict(metric=-1), dict(metric=2), dict(border=-1), dict(border=2),
            dict(lo=-2), dict(hi=257), dict(lo=5, hi=5), dict(lo=9, hi=3), dict(lo=256, hi=256), dict(lo=-1, hi=-1),
            dict(reach=-1), dict(metric=0, reach=(1 << 24) + 1), dict(metric=1, reach=4097), dict(metric=1, reach=1 << 24),
            dict(u8=0, a=ok["a"] + 2), dict(ws=ok["ws"] + 4), dict(ws=ok["ws"] + 1),
            dict(nbytes=ok["nbytes"] - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=need_one)]


def call_band(lib, a):
    return lib.gp_mask_band(a["a"], a["u8"], a["B"], a["H"], a["W"], a["lo"], a["hi"], a["metric"], a["reach"], a["border"], a["band"], a["fg"],
                            a["bg"], a["inner"], a["trimap"], a["ws"], a["nbytes"], None)


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    for lib in _libs():
        need = lib.gp_mask_band_workspace(2, 8, 8)
        ok = dict(a=0x1000, u8=1, B=2, H=8, W=8, lo=0, hi=255, metric=0, reach=4, border=0, band=0x2001, fg=0x3003, bg=None, inner=0x4000, trimap=None,
                  ws=0x8000, nbytes=need)
        for kw in invalid_cases(ok, lib.gp_mask_band_workspace(1, 8, 8)):
            assert call_band(lib, dict(ok, **kw)) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_inputs_before_the_library():
    from genpercept_amd import eval_metrics as em
    a = np.zeros((4, 4), np.uint8)
    for kw in (dict(lo=-2, hi=5), dict(lo=5, hi=5), dict(lo=0, hi=257), dict(lo=0, hi=255, reach=-1), dict(lo=0, hi=255, reach=4097, metric=1),
               dict(lo=0, hi=255, metric="manhattan"), dict(lo=0, hi=255, reach=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            em.mask_band(a, **dict(dict(reach=1, metric=0, border=0), **kw))
    with pytest.raises(ValueError):
        em.mask_band(np.zeros((2, 4, 4), np.uint8), 0, 255, 1)
    with pytest.raises(ValueError):
        em.band_reach(-1.0, "euclidean")
    assert em.band_reach(2.5, "euclidean") == 6 and em.band_reach(2.5, "chebyshev") == 2 and em.band_reach(25, 0) == 625
    assert em.boundary_reach(480, 640) == 16 and em.boundary_reach(2048, 2048) == 58 and em.boundary_reach(3, 4) == 1
    assert em.boundary_reach(300, 400, 0.001) == 1 and em.boundary_reach(1000, 1000, 0.02) == max(1, int(round(0.02 * np.sqrt(2e6))))


# ---- the planes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("lo,hi", THRESHOLDS)
def test_mask_band_equals_brute_force(lo, hi, border):
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(1000 + 7 * lo + border)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 9), (9, 1), (3, 4), (7, 5), (13, 13), (12, 13), (13, 6)]
    maps = [random_map(rng, h, w) for h, w in shapes]
    maps += [np.zeros((5, 6), np.uint8), np.full((6, 5), 255, np.uint8), np.full((4, 4), 77, np.uint8)]
    one = np.zeros((9, 11), np.uint8)
    one[4, 7] = 255
    maps += [one, 255 - one, (np.indices((8, 9)).sum(0) % 2 * 255).astype(np.uint8)]
    for a in maps:
        for metric, reach in REACHES:
            got = em.mask_band(a, lo, hi, reach, metric, border)
            want = brute_band(a, lo, hi, reach, metric, border)
            assert list(got) == PLANES
            for k in PLANES:
                assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), (a.shape, metric, reach, k)
            # band, fg and bg partition the image; the sides keep to their own pixels
            assert np.array_equal(got["band"].astype(int) + got["fg"] + got["bg"], np.full(a.shape, 255))
            assert (a[got["fg"] == 255].astype(int) >= hi).all() and (a[got["bg"] == 255].astype(int) <= lo).all()
            assert np.array_equal(got["trimap"], np.where(got["band"] == 255, 128, got["fg"]))
    # the metric's two spellings, and a float map is quantised first
    a = maps[7]
    for k in PLANES:
        assert np.array_equal(em.mask_band(a, lo, hi, 2, "chebyshev", bool(border))[k], em.mask_band(a, lo, hi, 2, 1, border)[k])
        assert np.array_equal(em.mask_band(a, lo, hi, 5, "euclidean", bool(border))[k], em.mask_band(a, lo, hi, 5, 0, border)[k])
    f = (a.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)
    assert np.array_equal(em.quantize_mask(f), a)
    assert all(np.array_equal(em.mask_band(f, lo, hi, 2, 0, border)[k], em.mask_band(a, lo, hi, 2, 0, border)[k]) for k in PLANES)


@pytest.mark.parametrize("d", [1, 2, 5])
def test_chebyshev_planes_equal_scipy_morphology(d):
    """band(chebyshev, border 0) = dilate(a != 0) - erode(a == 255) with a (2 d + 1)^2 square where nothing lies outside the image (dilate pads
    with 0, erode with 1: cv2's defaults); with border 1 the erosion pads with 0; inner(chebyshev, border 1) = "pad with 0, erode d times with
    3 x 3, subtract" (Boundary IoU's mask_to_boundary)."""
    from scipy import ndimage
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(40 + d)
    sq = np.ones((2 * d + 1, 2 * d + 1), bool)
    for h, w in ((1, 1), (5, 7), (13, 13), (31, 40), (64, 65)):
        a = random_map(rng, h, w)
        dil = ndimage.binary_dilation(a != 0, structure=sq, border_value=0)
        for border in (0, 1):
            ero = ndimage.binary_erosion(a == 255, structure=sq, border_value=1 - border)
            got = em.mask_band(a, 0, 255, d, "chebyshev", border)
            assert np.array_equal(got["band"] == 255, dil & ~ero) and np.array_equal(got["fg"] == 255, ero) and np.array_equal(got["bg"] == 255, ~dil)
        g = a > 128
        padded = np.pad(g, 1)
        ero = ndimage.binary_erosion(padded, structure=np.ones((3, 3), bool), iterations=d, border_value=1)[1:-1, 1:-1]
        assert np.array_equal(em.mask_band(a, 128, 129, d, "chebyshev", True)["inner"] == 255, g & ~ero)


def test_euclidean_reach_equals_the_high_word_of_edt_keys():
    """The exact squared distance the structure scores already use (eval_metrics.edt_keys, bit-equal to the device's) gives the same sets."""
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(6)
    maps = [random_map(rng, h, w) for h, w in ((1, 1), (1, 9), (9, 1), (13, 13), (31, 40), (64, 65))] + [np.zeros((7, 9), np.uint8)]
    one = np.zeros((40, 50), np.uint8)
    one[3, 44] = 255
    for a in maps + [one, 255 - one]:
        d_a = (em.edt_keys(a != 0) >> np.uint64(32)).astype(np.int64)
        d_b = (em.edt_keys(a != 255) >> np.uint64(32)).astype(np.int64)
        for reach in (0, 1, 2, 8, 9, 625, 1600, 10 ** 6):
            got = em.mask_band(a, 0, 255, reach, 0, 0)
            assert np.array_equal(got["bg"] == 0, d_a <= reach) and np.array_equal(got["fg"] == 0, d_b <= reach), (a.shape, reach)


def test_euclidean_planes_equal_scipy_distance_transform():
    from scipy import ndimage
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(5)
    for h, w in ((5, 7), (31, 40), (64, 65)):
        a = random_map(rng, h, w)
        for r in (1.0, 2.5, 7.0):
            reach = em.band_reach(r, "euclidean")
            d_a = np.rint(ndimage.distance_transform_edt(a == 0) ** 2)        # squared distance to {a != 0}: integers up to 65^2 + 64^2, exact
            d_b = np.rint(ndimage.distance_transform_edt(a == 255) ** 2)
            got = em.mask_band(a, 0, 255, reach, "euclidean", False)
            assert np.array_equal(got["band"] == 255, (d_a <= reach) & (d_b <= reach)) and np.array_equal(got["fg"] == 255, d_b > reach)


# ---- the two evaluators ------------------------------------------------------------------------------------------------------------------------
def test_trimap_metrics_equal_mask_metrics_over_the_three_regions():
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(9)
    for (h, w), metric, radius in (((31, 40), "euclidean", 2.5), ((64, 65), "chebyshev", 3), ((64, 65), "euclidean", 5)):
        gt = np.clip((np.arange(w)[None] - w // 3) * 40 + 128, 0, 255).repeat(h, 0).astype(np.uint8)
        gt[:3] = 0
        pred = np.clip(gt / 255.0 + 0.2 * rng.randn(h, w), 0, 1).astype(np.float32)
        m = em.trimap_metrics(pred, gt, radius, metric)
        assert list(m)[:5] == TRIMAP_METRICS
        planes = em.mask_band(gt, 0, 255, em.band_reach(radius, metric), metric, False)
        ref = {k: em.mask_metrics(pred, gt, planes[k]) for k in ("band", "fg", "bg")}
        assert m["mae_t"] == ref["band"]["mae"] and m["mse_t"] == ref["band"]["mse"] and m["sad_t"] == ref["band"]["sad"]
        assert m["sad_fg"] == ref["fg"]["sad"] and m["sad_bg"] == ref["bg"]["sad"]
        assert (m["n_t"], m["n_fg_side"], m["n_bg_side"]) == tuple(ref[k]["n"] for k in ("band", "fg", "bg"))
        assert m["n_t"] + m["n_fg_side"] + m["n_bg_side"] == h * w and min(m["n_t"], m["n_fg_side"], m["n_bg_side"]) > 0 and m["sad_t"] > 0
    # a side may be empty (0.0); an empty transition region is the n = 0 error
    flat = np.full((6, 6), 255, np.uint8)
    with pytest.raises(ValueError):
        em.trimap_metrics(flat, flat, 2)
    soft = np.full((6, 6), 100, np.uint8)
    m = em.trimap_metrics(np.zeros((6, 6), np.float32), soft, 2)
    assert m["n_t"] == 36 and m["sad_fg"] == 0.0 and m["sad_bg"] == 0.0 and m["sad_t"] == 3600 / 255000.0


def test_boundary_iou_hand_made_cases():
    from genpercept_amd import eval_metrics as em
    h, w = 40, 50                                                     # d = round(0.02 * 64.03) = 1
    assert em.boundary_reach(h, w) == 1
    g = np.zeros((h, w), np.uint8)
    g[10:30, 10:30] = 255
    same = em.boundary_iou(g, g)
    assert same["biou"] == 1.0 and same["d"] == 1 and same["n_gt_band"] == same["n_pred_band"] == 20 * 20 - 18 * 18
    p = np.zeros((h, w), np.uint8)
    p[32:38, 35:45] = 255
    assert em.boundary_iou(p, g)["biou"] == 0.0 and em.boundary_iou(np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8))["biou"] == 0.0
    # a float prediction goes through the byte: 0.5 * 255 = 127.5 -> 127 is negative, 128.5 / 255 positive
    pf = np.where(g == 255, np.float32(128.5 / 255), np.float32(0.5)).astype(np.float32)
    assert em.boundary_iou(pf, g)["biou"] == 1.0
    # a mask that touches the image edge: the border counts, so the edge pixels are boundary
    e = np.zeros((h, w), np.uint8)
    e[:20, :20] = 255
    r = em.boundary_iou(e, e)
    assert r["biou"] == 1.0 and r["n_gt_band"] == 20 * 20 - 18 * 18
    full = np.full((h, w), 255, np.uint8)
    r = em.boundary_iou(full, full, 0.05)                             # d = 3: the frame of width 3
    assert r["d"] == 3 and r["n_gt_band"] == h * w - (h - 6) * (w - 6) and r["biou"] == 1.0
    # shifted by two columns: the bands of width d = 3 overlap in part
    g2 = np.zeros((h, w), np.uint8)
    g2[10:30, 12:32] = 255
    r = em.boundary_iou(g2, g, 0.05)
    gd = em.mask_band(g, 128, 129, 3, 1, 1)["inner"] == 255
    pd = em.mask_band(g2, 127, 128, 3, 1, 1)["inner"] == 255
    assert r["biou"] == (gd & pd).sum() / (gd | pd).sum() and 0.0 < r["biou"] < 1.0


# ---- the file route and the loop -------------------------------------------------------------------------------------------------------------
def numpy_trimap_evaluator(pred, gt, radius, metric):
    """engine.eval_trimap's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    return [em.trimap_metrics(pred[i].numpy(), gt[i].numpy(), radius, metric) for i in range(pred.shape[0])]


def numpy_boundary_evaluator(pred, gt, ratio):
    """engine.eval_boundary_iou's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    return [em.boundary_iou(pred[i].numpy(), gt[i].numpy(), ratio) for i in range(pred.shape[0])]


def test_band_options_off_leave_the_files_as_they_are_and_on_append_their_columns(tmp_path):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base, pred_dir = str(tmp_path / "data"), str(tmp_path / "pred")
    samples = tm.make_tree(base)
    ie.run_inference(tm.FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="matting")
    outs = {k: str(tmp_path / k) for k in ("file_default", "file_off", "file_on", "loop_default", "loop_off", "loop_on")}
    loop = dict(batch_size=2, evaluator=tm.numpy_evaluator)
    on = dict(trimap_radius=3, trimap_metric="chebyshev", boundary_iou=True, boundary_ratio=0.05)
    stubs = dict(trimap_evaluator=numpy_trimap_evaluator, boundary_evaluator=numpy_boundary_evaluator)
    r_default = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_default"])
    r_off = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_off"], trimap_radius=None, boundary_iou=False)
    r_on = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_on"], **on)
    l_default = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_default"], **loop)
    l_off = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_off"], trimap_radius=None, trimap_evaluator=None,
                                        boundary_iou=False, boundary_evaluator=None, **loop)
    l_on = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_on"], **on, **stubs, **loop)
    assert r_default == r_off == l_default == l_off and list(r_off) == MASK_METRICS + ["max_f_dataset"]
    names = MASK_METRICS + TRIMAP_METRICS + BOUNDARY_METRICS
    assert list(r_on) == list(l_on) == names + ["max_f_dataset"] and r_on == l_on
    assert all(r_on[k] == r_off[k] for k in r_off)

    def files(d):
        csv = open(os.path.join(d, "per_sample_metrics-mask.csv")).read()
        txt = [x for x in open(os.path.join(d, "eval_metrics-mask.txt")).read().splitlines() if "of predictions" not in x]
        return csv, txt

    for k in ("file_off", "loop_default", "loop_off"):
        assert files(outs[k]) == files(outs["file_default"]), k
    csv_off, txt_off = files(outs["file_default"])
    assert csv_off.splitlines()[0] == "filename," + ",".join(MASK_METRICS) and txt_off[-2] == "  ".join(MASK_METRICS)
    assert not any("trimap" in x or "boundary" in x for x in txt_off)
    csv_on, txt_on = files(outs["file_on"])
    assert files(outs["loop_on"]) == (csv_on, txt_on)
    assert csv_on.splitlines()[0] == "filename," + ",".join(names) and txt_on[-2] == "  ".join(names)
    assert txt_on[-1] == "  ".join(f"{r_on[k]:.6g}" for k in names)
    assert any("radius 3" in x and "chebyshev" in x for x in txt_on) and any("boundary IoU" in x and "0.05" in x for x in txt_on)
    assert [x for x in txt_on if "radius 3" not in x and "boundary IoU" not in x][:-2] == txt_off[:-2]
    rows = []
    for line_off, line_on, s in zip(csv_off.splitlines()[1:], csv_on.splitlines()[1:], samples):
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        gt, pred = ie.read_gt_mask(os.path.join(base, s[1])), np.load(os.path.join(pred_dir, name))
        m = dict(em.trimap_metrics(pred, gt, 3, "chebyshev"), **em.boundary_iou(pred, gt, 0.05))
        assert line_on == line_off + "," + ",".join(str(m[k]) for k in TRIMAP_METRICS + BOUNDARY_METRICS)
        rows.append(m)
    for k in TRIMAP_METRICS + BOUNDARY_METRICS:
        assert r_on[k] == sum(m[k] for m in rows) / len(rows), k
    assert r_on["sad_t"] > 0 and 0 < r_on["biou"] < 1
    # one option alone; the Euclidean default; after the matting columns
    only_b = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", boundary_iou=True, boundary_evaluator=numpy_boundary_evaluator, **loop)
    assert list(only_b) == MASK_METRICS + BOUNDARY_METRICS + ["max_f_dataset"]
    assert only_b == ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, boundary_iou=True)
    only_t = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, trimap_radius=2.5, matting=True)
    assert list(only_t) == MASK_METRICS + ["grad", "conn"] + TRIMAP_METRICS + ["max_f_dataset"]
    name0 = os.path.join(os.path.dirname(samples[0][0]), ie.get_pred_name(os.path.basename(samples[0][0]), ie.FileNameMode.id, suffix=".npy"))
    gt0, pred0 = ie.read_gt_mask(os.path.join(base, samples[0][1])), np.load(os.path.join(pred_dir, name0))
    assert em.trimap_metrics(pred0, gt0, 2.5) == em.trimap_metrics(pred0, gt0, 2.5, "euclidean")


def test_band_options_do_not_go_with_region_of(tmp_path):
    from genpercept_amd import infer_eval as ie
    base, pred_dir = str(tmp_path / "data"), str(tmp_path / "pred")
    samples = tm.make_tree(base)
    region_of = tm.trimap_region(base)
    for kw in (dict(trimap_radius=3), dict(boundary_iou=True), dict(trimap_radius=3, boundary_iou=True)):
        with pytest.raises(ValueError):
            ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, region_of=region_of, **kw)
        with pytest.raises(ValueError):
            ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", evaluator=tm.numpy_evaluator, region_of=region_of, **kw)
    for kw in (dict(trimap_radius=-1.0), dict(trimap_radius=3, trimap_metric="manhattan"), dict(boundary_iou=True, boundary_ratio=0.0)):
        with pytest.raises(ValueError):
            ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", evaluator=tm.numpy_evaluator, **kw)
