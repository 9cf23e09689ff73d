"""CPU tests of the seg evaluation: the device entries (gp_seg_decode / gp_eval_seg_workspace / gp_eval_seg) are declared, exported by both
libraries and bound, and refuse bad arguments before any HIP call; the host route (eval_metrics.quantize_seg / palette_labels / seg_gt_labels /
seg_counts / seg_metrics_from_counts / seg_metrics) against a case worked by hand and against a brute-force definition written here; the
readers, the file route and the loop `infer_eval.infer_and_evaluate_seg` with a fake pipeline and the NumPy evaluator in place of
engine.eval_seg, at world sizes 1 and 2 (gloo).

No tolerance: labels, distances and counts are integers, and every value is one prescribed sequence of float64 operations on them, which the
brute force below repeats with its own counts (np.bincount(g * K + c), float64 sums in class order)."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_seg_decode", "gp_eval_seg_workspace", "gp_eval_seg")
SEG_METRICS = ["pixel_acc", "mean_acc", "miou", "fwiou", "colour_rmse"]
GP_ERR_INVALID = 1


def _libs():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


def same(a, b):
    """equal, NaN matching NaN (scalars, lists, arrays, dicts of them)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- symbols -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import build, engine
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert "base_dataset.py:333-346,366" in hdr and "run.py:449-455" in hdr and "GP_ABI_VERSION 3" in re.sub(r"\s+", " ", hdr)
    assert "eval_seg.hip" in build.SOURCES
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
    assert len(engine.SYMBOLS["gp_eval_seg"][1]) == 17 and len(engine.SYMBOLS["gp_seg_decode"][1]) == 10
    assert len(engine.SYMBOLS["gp_eval_seg_workspace"][1]) == 4 and engine.SYMBOLS["gp_eval_seg_workspace"][0] is C.c_longlong
    assert callable(engine.seg_decode) and callable(engine.eval_seg_raw) and callable(engine.eval_seg)
    assert list(engine.SEG_METRICS) == list(em.SEG_METRICS) == list(ie.SEG_METRICS) == SEG_METRICS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in NAMES)
    assert "Seg is not scored" not in open(os.path.join(ROOT, "README.md")).read()


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8, 19), (1, 0, 8, 19), (1, 8, 0, 19), (-1, 8, 8, 19), (1, -8, 8, 19), (1, 8, -8, 19), (1, 8, 8, 0), (1, 8, 8, 193), (1, 8, 8, -1)):
            assert lib.gp_eval_seg_workspace(*bad) == 0, bad
        for k in (1, 2, 19, 150, 192):
            for h, w in ((1, 1), (7, 5), (64, 65), (2048, 2048)):
                one = lib.gp_eval_seg_workspace(1, h, w, k)
                assert one >= 8 * (3 + k * k) and one % 8 == 0
                prev = 0
                for b in (1, 2, 3, 7, 65535):                       # monotone in B, proportional to it
                    cur = lib.gp_eval_seg_workspace(b, h, w, k)
                    assert cur == b * one and cur > prev
                    prev = cur


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced.  (K = 192 with otherwise valid arguments is accepted and would launch: not called here.)"""
    P, G, R, PAL, O, CN, L, WS, D = 0x1000, 0x2000, 0x3000, 0x3800, 0x4000, 0x5000, 0x5800, 0x6000, 0x7000  # all 8-byte aligned
    for lib in _libs():
        need = lib.gp_eval_seg_workspace(2, 8, 8, 19)
        ok = dict(pred=P, u8=0, gt=G, lab=0, tol=0, region=R, pal=PAL, K=19, B=2, H=8, W=8, out=O, counts=CN, labels=L, ws=WS, nbytes=need)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.gp_eval_seg(a["pred"], a["u8"], a["gt"], a["lab"], a["tol"], a["region"], a["pal"], a["K"], a["B"], a["H"], a["W"], a["out"],
                                   a["counts"], a["labels"], a["ws"], a["nbytes"], None)

        huge = 1 << 62
        cases = [dict(pred=None), dict(gt=None), dict(pal=None), dict(out=None), dict(ws=None),
                 dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
                 dict(B=65536, nbytes=lib.gp_eval_seg_workspace(65536, 8, 8, 19)),                        # above the grid's y limit
                 dict(B=1, H=65536, W=65536, nbytes=huge), dict(B=1, H=1 << 16, W=1 << 15, nbytes=huge),  # H * W beyond 2^31 - 1
                 dict(K=0, nbytes=huge), dict(K=-1, nbytes=huge), dict(K=193, nbytes=huge), dict(K=256, nbytes=huge),
                 dict(tol=-1), dict(u8=-1), dict(u8=2), dict(lab=-1), dict(lab=2),
                 dict(out=O + 4), dict(counts=CN + 4), dict(counts=CN + 1), dict(ws=WS + 4),
                 dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=lib.gp_eval_seg_workspace(1, 8, 8, 19)),
                 dict(K=20)]                                                                              # the workspace of K = 19 is too small
        for kw in cases:
            assert call(**kw) == GP_ERR_INVALID, kw
        okd = dict(pred=P, u8=0, pal=PAL, K=19, B=2, H=8, W=8, labels=L, dist=D)

        def decode(**kw):
            a = dict(okd, **kw)
            return lib.gp_seg_decode(a["pred"], a["u8"], a["pal"], a["K"], a["B"], a["H"], a["W"], a["labels"], a["dist"], None)

        for kw in [dict(pred=None), dict(pal=None), dict(labels=None), dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-1), dict(W=-1), dict(B=65536),
                   dict(B=1, H=65536, W=65536), dict(K=0), dict(K=193), dict(u8=-1), dict(u8=2)]:
            assert decode(**kw) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_inputs_before_the_library():
    from genpercept_amd import engine
    pal = np.zeros((4, 3), np.uint8)
    pred, gt = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, 3, dtype=torch.uint8)
    bad = [(torch.zeros(2, 1, 4, 5), gt, pal), (torch.zeros(4, 5), gt, pal), (torch.zeros(2, 3, 4, 5, dtype=torch.int32), gt, pal),
           (pred, gt.float(), pal), (pred, torch.zeros(2, 4, 6, 3, dtype=torch.uint8), pal), (pred, torch.zeros(4, 5, dtype=torch.uint8), pal),
           (pred, torch.zeros(3, 4, 5, dtype=torch.uint8), pal), (pred, torch.zeros(2, 4, 5, 4, dtype=torch.uint8), pal),
           (pred, gt, np.zeros((4, 4), np.uint8)), (pred, gt, np.zeros((4, 3), np.int32)), (pred, gt, np.zeros((0, 3), np.uint8)),
           (pred, gt, np.zeros((193, 3), np.uint8))]
    for p, g, q in bad:
        with pytest.raises(ValueError):
            engine.eval_seg_raw(p, g, q)
    with pytest.raises(ValueError):
        engine.eval_seg_raw(pred, gt, pal, gt_tol=-1)
    with pytest.raises(ValueError):
        engine.eval_seg_raw(pred, gt, pal, region=torch.zeros(2, 4, 6, dtype=torch.bool))
    for p, q in ((torch.zeros(2, 2, 4, 5), pal), (torch.zeros(2, 3, 4, 5, dtype=torch.int64), pal), (pred, np.zeros((4, 2), np.uint8))):
        with pytest.raises(ValueError):
            engine.seg_decode(p, q)


# ---- the host route ------------------------------------------------------------------------------------------------------------------------
HAND_PAL = np.array([[0, 0, 0], [2, 0, 0], [90, 90, 90]], np.uint8)
HAND_Q = np.array([[[1, 0, 0], [0, 0, 0], [2, 0, 0]], [[3, 0, 0], [0, 1, 0], [2, 0, 2]]], np.uint8)
HAND_LABELS = np.array([[0, 1, 1], [1, 255, 0]], np.uint8)
HAND_COLOURS = np.array([[[0, 0, 0], [2, 0, 0], [2, 0, 0]], [[2, 0, 0], [50, 50, 50], [0, 0, 0]]], np.uint8)


def test_hand_case():
    """2 x 3 pixels, K = 3, palette 0 = (0,0,0), 1 = (2,0,0), 2 = (90,90,90).
      pixel  colour    d_0 d_1   class d   ground truth
      (0,0)  (1,0,0)    1   1      0   1   0        the tie: the smaller index
      (0,1)  (0,0,0)    0   4      0   0   1
      (0,2)  (2,0,0)    4   0      1   0   1
      (1,0)  (3,0,0)    9   1      1   1   1
      (1,1)  (0,1,0)    1   5      0   1   void     (label 255; as a colour (50,50,50), which is no palette colour)
      (1,2)  (2,0,2)    8   4      1   4   0
    n = 5, n_void = 1, sum_d = 1 + 0 + 0 + 1 + 4 = 6; conf = [[1, 1, 0], [1, 2, 0], [0, 0, 0]]: row = col = (2, 3, 0), tp = (1, 2, 0),
    union = (3, 4, 0).  pixel_acc = 3 / 5; mean_acc = (1/2 + 2/3) / 2; iou = (1/3, 1/2, NaN): class 2 is in neither map and stays out of
    miou = (1/3 + 1/2) / 2; fwiou = (2 * (1/3) + 3 * (1/2)) / 5; colour_rmse = sqrt(6 / 15) / 255; n_classes = 2."""
    from genpercept_amd import eval_metrics as em
    labels, d = em.palette_labels(HAND_Q, HAND_PAL)
    assert labels.dtype == np.uint8 and d.dtype == np.int32
    assert labels.tolist() == [[0, 0, 1], [1, 0, 1]] and d.tolist() == [[1, 0, 0], [1, 1, 4]]
    assert em.seg_gt_labels(HAND_LABELS, HAND_PAL).tolist() == HAND_LABELS.tolist()
    assert em.seg_gt_labels(HAND_COLOURS, HAND_PAL, 0).tolist() == HAND_LABELS.tolist()
    c = em.seg_counts(HAND_Q, HAND_LABELS, HAND_PAL)
    assert c.dtype == np.int64 and c.tolist() == [5, 1, 6, 1, 1, 0, 1, 2, 0, 0, 0, 0]
    m = em.seg_metrics_from_counts(c, 3)
    assert list(m) == ["n", "n_void"] + SEG_METRICS + ["n_classes", "iou"]
    assert m["n"] == 5 and m["n_void"] == 1 and m["n_classes"] == 2
    assert m["pixel_acc"] == 3.0 / 5.0 and m["mean_acc"] == (1.0 / 2.0 + 2.0 / 3.0) / 2.0 and m["miou"] == (1.0 / 3.0 + 1.0 / 2.0) / 2.0
    assert m["fwiou"] == (2.0 * (1.0 / 3.0) + 3.0 * (1.0 / 2.0)) / 5.0 and m["colour_rmse"] == math.sqrt(6.0 / 15.0) / 255.0
    assert m["iou"][:2] == [1.0 / 3.0, 1.0 / 2.0] and math.isnan(m["iou"][2])
    as_float = (HAND_Q.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)
    for pred in (HAND_Q, as_float):                                        # (W = 3: a [3, H, W] copy of it would read as [H, W, 3])
        for gt in (HAND_LABELS, HAND_COLOURS):
            full = em.seg_metrics(pred, gt, HAND_PAL)
            assert full["conf"].tolist() == [[1, 1, 0], [1, 2, 0], [0, 0, 0]] and same({k: full[k] for k in m}, m)
    region = np.array([[1, 1, 0], [0, 1, 1]], bool)                       # (0,0), (0,1), the void pixel, (1,2)
    assert em.seg_counts(HAND_Q, HAND_LABELS, HAND_PAL, region).tolist() == [3, 1, 5, 1, 1, 0, 1, 0, 0, 0, 0, 0]
    assert em.seg_gt_labels(HAND_COLOURS, HAND_PAL, 4799).tolist() == HAND_LABELS.tolist()      # (50,50,50): d = 7500, 7304, 4800 -> void still ...
    assert em.seg_gt_labels(HAND_COLOURS, HAND_PAL, 4800).tolist() == [[0, 1, 1], [1, 2, 0]]    # ... and class 2 from its distance on


def brute_force(q, gt_labels, pal, region):
    """The definitions, pixel by pixel in Python for the decode, np.bincount(g * K + c) for the matrix, float64 sums in class order."""
    K = len(pal)
    h, w = gt_labels.shape
    c, d = np.zeros((h, w), int), np.zeros((h, w), int)
    for y in range(h):
        for x in range(w):
            best = None
            for k in range(K):
                dk = sum((int(q[y, x, ch]) - int(pal[k, ch])) ** 2 for ch in range(3))
                if best is None or dk < best:
                    best, c[y, x] = dk, k
            d[y, x] = best
    sel = np.ones((h, w), bool) if region is None else region != 0
    scored = sel & (gt_labels < K)
    conf = np.bincount(gt_labels[scored].astype(int) * K + c[scored], minlength=K * K).reshape(K, K)
    n, n_void, sum_d = int(scored.sum()), int((sel & (gt_labels >= K)).sum()), int(d[scored].sum())
    out = dict(n=n, n_void=n_void, labels=c, d=d, conf=conf, sum_d=sum_d)
    if n == 0:
        return out
    row, col, tp = conf.sum(1), conf.sum(0), np.diag(conf)
    union = row + col - tp
    acc = iou = fw = 0.0
    ious = []
    for i in range(K):
        v = float(tp[i]) / float(union[i]) if union[i] > 0 else float("nan")
        ious.append(v)
        if row[i] > 0:
            acc += float(tp[i]) / float(row[i])
            fw += float(row[i]) * v
        if union[i] > 0:
            iou += v
    out.update(pixel_acc=float(tp.sum()) / float(n), mean_acc=acc / float((row > 0).sum()), miou=iou / float((union > 0).sum()), fwiou=fw / float(n),
               colour_rmse=math.sqrt(float(sum_d) / (3.0 * float(n))) / 255.0, n_classes=int((union > 0).sum()), iou=ious)
    return out


def random_case(h, w, K, seed):
    rng = np.random.RandomState(seed)
    pal = rng.randint(0, 256, (K, 3)).astype(np.uint8)
    if K >= 3:
        pal[K - 1] = pal[0]
        pal[1, 0] = min(int(pal[1, 0]), 253)
        pal[2] = pal[1]
        pal[2, 0] += 2
    lab = rng.randint(0, K, (h, w))
    q = np.clip(pal[np.where(rng.rand(h, w) < 0.8, lab, rng.randint(0, K, (h, w)))].astype(int) + rng.randint(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    if K >= 3:
        q[rng.rand(h, w) < 0.05] = pal[1] + np.array([1, 0, 0], np.uint8)  # ties between 1 and 2
    gt = lab.astype(np.uint8)
    gt[rng.rand(h, w) < 0.05] = 255
    return q, gt, pal, rng.rand(h, w) < 0.6


@pytest.mark.parametrize("shape", [(7, 5), (24, 25)])
@pytest.mark.parametrize("K", [1, 2, 7, 19])
def test_seg_metrics_equal_the_brute_force_definition(shape, K):
    from genpercept_amd import eval_metrics as em
    q, gt, pal, region = random_case(*shape, K, seed=100 * K + shape[0])
    for r in (None, region):
        ref = brute_force(q, gt, pal, r)
        labels, d = em.palette_labels(q, pal)
        assert np.array_equal(labels, ref["labels"]) and np.array_equal(d, ref["d"])
        c = em.seg_counts(q, gt, pal, r)
        assert c[0] == ref["n"] and c[1] == ref["n_void"] and c[2] == ref["sum_d"] and np.array_equal(c[3:].reshape(K, K), ref["conf"])
        m = em.seg_metrics_from_counts(c, K)
        for k in SEG_METRICS + ["n_classes"]:
            assert m[k] == ref[k], (k, m[k], ref[k])
        assert same(m["iou"], ref["iou"])
        full = em.seg_metrics(q, gt, pal, r)
        assert same({k: full[k] for k in m}, m) and np.array_equal(full["conf"], ref["conf"])
        # the colour form of the same ground truth: a duplicated colour decodes to its smaller index, another colour is void at gt_tol = 0
        other = pal[0] ^ 0x55
        assert not any(other.tolist() == p.tolist() for p in pal)
        colours = pal[np.minimum(gt, K - 1)]
        colours[gt >= K] = other
        decoded = em.seg_gt_labels(colours, pal, 0)
        assert ((decoded == 255) == (gt >= K)).all()
        known = gt < K
        assert (decoded[known] <= gt[known]).all() and (pal[decoded[known]] == pal[gt[known]]).all()
        assert same({k: v for k, v in em.seg_metrics(q, colours, pal, r).items() if k != "conf"}, em.seg_metrics_from_counts(em.seg_counts(q, decoded, pal, r), K))


def test_quantisation_is_the_float32_product_truncated():
    """Per channel, k / 255 in float32 and its two neighbours: the product of a float32 and 255 is exact in float64, so rounding it once to
    float32 and truncating is an independent statement of `(x * 255.0f)` -> byte.  Also the clip, the NaN rule and the two layouts."""
    from genpercept_amd import eval_metrics as em
    k = np.arange(256, dtype=np.float32)
    x = k / np.float32(255.0)
    xs = np.stack([x, np.nextafter(x, np.float32(-1.0)), np.nextafter(x, np.float32(2.0))], axis=-1).astype(np.float32)[None]   # [1, 256, 3]
    want = np.floor(np.float32(np.clip(xs.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.float64)).astype(np.uint8)
    got = em.quantize_seg(xs)
    assert got.dtype == np.uint8 and got.shape == (1, 256, 3) and np.array_equal(got, want)
    assert np.array_equal(em.quantize_seg(np.ascontiguousarray(np.moveaxis(xs, -1, 0))), want)                # [3, 1, 256]
    assert (got[0, :, 1] <= got[0, :, 0]).all() and (got[0, :, 1] < got[0, :, 0]).any() and (got[0, :, 2] >= got[0, :, 0]).all()
    special = np.array([np.nan, -np.inf, np.inf, -0.0, -0.25, 1.0 + 1e-6, 1.5, 0.999999, 0.5], np.float32).reshape(1, 3, 3)
    assert em.quantize_seg(special).reshape(-1).tolist() == [0, 0, 255, 0, 0, 255, 255, 254, 127]
    assert em.quantize_seg(special.astype(np.float64)).reshape(-1).tolist() == [0, 0, 255, 0, 0, 255, 255, 254, 127]
    u8 = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    assert np.array_equal(em.quantize_seg(u8), u8) and np.array_equal(em.quantize_seg(np.moveaxis(u8, -1, 0)), u8)
    for bad in (np.zeros((4, 5)), np.zeros((4, 5, 2)), np.zeros((4, 5, 3), np.int32)):
        with pytest.raises(ValueError):
            em.quantize_seg(bad)


def test_degenerate_sets():
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(3)
    q = rng.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    # duplicate colours: the larger index never wins
    pal = np.array([[10, 20, 30], [200, 100, 50], [10, 20, 30], [200, 100, 50]], np.uint8)
    labels, _ = em.palette_labels(q, pal)
    assert set(np.unique(labels)) <= {0, 1}
    gt = rng.randint(0, 4, (9, 11)).astype(np.uint8)
    m = em.seg_metrics(q, gt, pal)
    assert m["n_classes"] == 4 and m["iou"][2] == 0.0 and m["iou"][3] == 0.0 and m["conf"][:, 2:].sum() == 0    # in the ground truth only
    # a K = 1 palette: everything is class 0
    one = np.array([[7, 7, 7]], np.uint8)
    m = em.seg_metrics(q, np.zeros((9, 11), np.uint8), one)
    assert m["n"] == 99 and m["pixel_acc"] == 1.0 and m["mean_acc"] == 1.0 and m["miou"] == 1.0 and m["fwiou"] == 1.0 and m["n_classes"] == 1
    assert m["iou"] == [1.0] and m["conf"].tolist() == [[99]] and m["colour_rmse"] > 0.0
    # an all-void image, and an empty region
    for gt2, region in ((np.full((9, 11), 255, np.uint8), None), (gt, np.zeros((9, 11), bool))):
        m = em.seg_metrics(q, gt2, pal, region)
        assert m["n"] == 0 and m["n_void"] == (99 if region is None else 0) and all(math.isnan(m[k]) for k in SEG_METRICS)
        assert math.isnan(m["n_classes"]) and all(math.isnan(v) for v in m["iou"]) and m["conf"].sum() == 0
    for bad in (np.zeros((0, 3), np.uint8), np.zeros((193, 3), np.uint8), np.zeros((4, 3), np.int64), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            em.palette_labels(q, bad)
    with pytest.raises(ValueError):
        em.seg_gt_labels(gt, pal, -1)
    with pytest.raises(ValueError):
        em.seg_metrics_from_counts(np.zeros(10, np.int64), 4)
    big = np.random.RandomState(1).randint(0, 256, (300, 301, 3)).astype(np.uint8)      # more than one chunk
    pal19 = np.random.RandomState(2).randint(0, 256, (19, 3)).astype(np.uint8)
    lab, d = em.palette_labels(big, pal19)
    dd = ((big[:, :, None, :].astype(np.int64) - pal19.astype(np.int64)) ** 2).sum(-1)
    assert np.array_equal(lab, dd.argmin(-1)) and np.array_equal(d, dd.min(-1))


# ---- readers -------------------------------------------------------------------------------------------------------------------------------
def test_read_palette(tmp_path):
    from genpercept_amd import infer_eval as ie
    (tmp_path / "p.txt").write_text("# a palette\n0 0 0 background\n\n128 64 128 road surface  # two words\n  255 0 0\n70 70 70 building\n")
    pal, names = ie.read_palette(str(tmp_path / "p.txt"))
    assert pal.dtype == np.uint8 and pal.tolist() == [[0, 0, 0], [128, 64, 128], [255, 0, 0], [70, 70, 70]]
    assert names == ["background", "road surface", "2", "building"]
    np.save(tmp_path / "p.npy", pal.astype(np.int64))
    pal2, names2 = ie.read_palette(str(tmp_path / "p.npy"))
    assert pal2.dtype == np.uint8 and np.array_equal(pal2, pal) and names2 == ["0", "1", "2", "3"]
    for i, text in enumerate(["0 0\n", "0 0 256\n", "a b c\n", "# nothing\n", "1 2 3\n" * 193]):
        (tmp_path / f"bad{i}.txt").write_text(text)
        with pytest.raises(ValueError):
            ie.read_palette(str(tmp_path / f"bad{i}.txt"))
    np.save(tmp_path / "bad.npy", np.zeros((4, 4)))
    with pytest.raises(ValueError):
        ie.read_palette(str(tmp_path / "bad.npy"))


def test_read_gt_seg(tmp_path):
    from genpercept_amd import infer_eval as ie
    rng = np.random.RandomState(0)
    lab = rng.randint(0, 4, (6, 9)).astype(np.uint8)
    pal = np.array([[0, 0, 0], [128, 64, 128], [255, 0, 0], [70, 70, 70]], np.uint8)
    Image.fromarray(pal[lab]).save(tmp_path / "rgb.png")
    Image.fromarray(np.concatenate([pal[lab], np.full((6, 9, 1), 255, np.uint8)], -1)).save(tmp_path / "rgba.png")
    p = Image.fromarray(lab, mode="P")
    p.putpalette(pal.reshape(-1).tolist())
    p.save(tmp_path / "p.png")
    Image.fromarray(lab).save(tmp_path / "l.png")
    Image.fromarray(lab.astype(np.uint16) * 300).save(tmp_path / "u16.png")
    for name in ("rgb.png", "rgba.png", "p.png"):
        g = ie.read_gt_seg(str(tmp_path / name))
        assert g.dtype == np.uint8 and g.shape == (6, 9, 3) and np.array_equal(g, pal[lab]) and g.flags["C_CONTIGUOUS"]
    g = ie.read_gt_seg(str(tmp_path / "l.png"))
    assert g.dtype == np.uint8 and g.shape == (6, 9) and np.array_equal(g, lab)
    with pytest.raises(ValueError):
        ie.read_gt_seg(str(tmp_path / "u16.png"))


# ---- the file route and the loop -------------------------------------------------------------------------------------------------------------
SIZES = [(24, 32), (24, 32), (24, 32), (20, 28), (24, 32)]  # (H, W): the fourth image has another size
PAL = np.array([[0, 0, 0], [128, 64, 128], [250, 10, 10], [70, 70, 70], [72, 70, 70]], np.uint8)
PAL_NAMES = ["void-ish", "road", "sign", "wall", "wall 2"]


def make_tree(base):
    """5 RGB images that are noisy renderings of a label map in PAL's colours, the label image of each (the second a palettised file, the third a
    single-channel label map with 255 = ignore, the others RGB with a few non-palette pixels) and a region file; filename-list lines with the
    label image in column 6."""
    rng = np.random.RandomState(23)
    samples = []
    for i, (h, w) in enumerate(SIZES):
        scene = os.path.join(base, f"set{i // 3}")
        for d in ("im", "seg", "region"):
            os.makedirs(os.path.join(scene, d), exist_ok=True)
        lab = rng.randint(0, 5, (h // 4, w // 4)).repeat(4, 0).repeat(4, 1).astype(np.uint8)
        seen = np.where(rng.rand(h, w) < 0.85, lab, rng.randint(0, 5, (h, w))).astype(np.uint8)
        rgb = np.clip(PAL[seen].astype(int) + rng.randint(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(scene, "im", f"{i:04d}.png"))
        void = rng.rand(h, w) < 0.05
        path = os.path.join(scene, "seg", f"{i:04d}.png")
        if i == 1:
            p = Image.fromarray(lab, mode="P")
            p.putpalette(PAL.reshape(-1).tolist())
            p.save(path)
        elif i == 2:
            Image.fromarray(np.where(void, 255, lab).astype(np.uint8)).save(path)
        else:
            col = PAL[lab]
            col[void] = (9, 200, 90)
            Image.fromarray(col).save(path)
        Image.fromarray((rng.rand(h, w) < 0.7).astype(np.uint8) * 128).save(os.path.join(scene, "region", f"{i:04d}.png"))
        samples.append([f"set{i // 3}/im/{i:04d}.png", "x", "None", "None", "None", "None", f"set{i // 3}/seg/{i:04d}.png"])
    return samples


def fake_pred(img):
    """A deterministic [3, H, W] float32 colour map in [0, 1] from the RGB image: its own colours, a fifth of a step above k / 255."""
    a = np.asarray(img.convert("RGB")).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis((a + np.float32(0.2)) / np.float32(255.0), -1, 0))


class FakePipe:
    def __init__(self):
        self.single, self.batches = 0, []

    def __call__(self, img, **kw):
        assert kw["batch_size"] == 0 and kw["color_map"] is None and kw["mode"] == "seg"
        self.single += 1
        return SimpleNamespace(pred_np=np.transpose(fake_pred(img), (1, 2, 0)), pred_colored=None)

    def predict_batch_device(self, images, mode, **kw):
        assert mode == "seg" and len({im.size for im in images}) == 1
        self.batches.append(len(images))
        return torch.from_numpy(np.stack([fake_pred(im) for im in images]))


def numpy_evaluator(pred, gt, palette, region, gt_tol):
    """engine.eval_seg's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and pred.dim() == 4 and pred.shape[1] == 3 and gt.dtype == torch.uint8 and gt.dim() in (3, 4)
    assert torch.is_tensor(palette) and palette.dtype == torch.uint8
    return [em.seg_metrics(pred[i].numpy(), gt[i].numpy(), palette.numpy(), None if region is None else region[i].numpy(), gt_tol)
            for i in range(pred.shape[0])]


def region_files(base):
    def region_of(sample, gt):
        r = np.asarray(Image.open(os.path.join(base, sample[6].replace("/seg/", "/region/")))) == 128
        assert r.shape == gt.shape[:2]
        return r
    return region_of


@pytest.mark.parametrize("with_region", [False, True])
def test_evaluate_seg_predictions_npy_and_png_routes(tmp_path, with_region):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base, pred_dir, png_dir, out = (str(tmp_path / d) for d in ("data", "pred", "pred_png", "eval"))
    samples = make_tree(base)
    region_of = region_files(base) if with_region else None
    pipe = FakePipe()
    written = ie.run_inference(pipe, base, samples, pred_dir, ie.FileNameMode.id, mode="seg")
    assert pipe.single == 5 and len(written) == 5
    for p in written:  # the 8-bit image of the same map
        assert np.load(p).shape[-1] == 3
        dst = os.path.join(png_dir, os.path.relpath(p, pred_dir))[:-4] + ".png"
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        Image.fromarray(em.quantize_seg(np.load(p))).save(dst)
    os.remove(written[4])                                            # a sample without a prediction file is skipped ...
    with_gaps = samples[:2] + [["x.png", "x", "None", "None", "None", "None", "None"], ["y.png", "x"]] + samples[2:]  # ... and one without ground truth
    res = ie.evaluate_seg_predictions(pred_dir, base, with_gaps, ie.FileNameMode.id, (PAL, PAL_NAMES), output_dir=out, gt_tol=3, region_of=region_of)
    assert list(res) == SEG_METRICS + ["miou_dataset", "pixel_acc_dataset", "iou_dataset"]
    rows, conf = [], np.zeros((5, 5), np.int64)
    for s, path in zip(samples[:4], written[:4]):
        gt = ie.read_gt_seg(os.path.join(base, s[6]))
        m = em.seg_metrics(np.load(path), gt, PAL, region_of(s, gt) if with_region else None, 3)
        rows.append(m)
        conf += m["conf"]
    for k in SEG_METRICS:
        assert res[k] == sum(r[k] for r in rows) / 4, k
        assert 0.0 < res[k] < 1.0, (k, res[k])
    ds = em.seg_metrics_from_counts([int(conf.sum()), 0, 0] + conf.reshape(-1).tolist(), 5)
    assert res["miou_dataset"] == ds["miou"] and res["pixel_acc_dataset"] == ds["pixel_acc"] and res["iou_dataset"] == ds["iou"]
    assert res["miou_dataset"] != res["miou"] and len(res["iou_dataset"]) == 5 and all(0.0 < v < 1.0 for v in res["iou_dataset"])
    lines = open(os.path.join(out, "per_sample_metrics-seg.csv")).read().splitlines()
    assert lines[0] == "filename," + ",".join(SEG_METRICS) and len(lines) == 1 + 4
    for ln, s, row in zip(lines[1:], samples, rows):
        assert ln == os.path.join(os.path.dirname(s[0]), "pred_" + os.path.basename(s[0])[:-4] + ".npy") + "," + ",".join(str(row[k]) for k in SEG_METRICS)
    txt = open(os.path.join(out, "eval_metrics-seg.txt")).read().splitlines()
    assert txt[-2] == "  ".join(SEG_METRICS) and txt[-1] == "  ".join(f"{res[k]:.6g}" for k in SEG_METRICS)
    assert f"miou_dataset = {res['miou_dataset']:.6g}" in txt and f"pixel_acc_dataset = {res['pixel_acc_dataset']:.6g}" in txt
    assert "iou_dataset of the classes " + ", ".join(PAL_NAMES) + ":" in txt
    for nm, v in zip(PAL_NAMES, res["iou_dataset"]):
        assert f"    {nm} = {v:.6g}" in txt
    # the .png route reads the same bytes; a bare palette names the classes by index
    res_png = ie.evaluate_seg_predictions(png_dir, base, samples[:4], ie.FileNameMode.id, PAL, pred_suffix=".png", gt_tol=3, region_of=region_of)
    assert res_png == res
    empty = ie.evaluate_seg_predictions(pred_dir, base, [["x.png", "x"]], ie.FileNameMode.id, PAL)
    assert all(np.isnan(empty[k]) for k in SEG_METRICS + ["miou_dataset", "pixel_acc_dataset"]) and all(np.isnan(v) for v in empty["iou_dataset"])
    with pytest.raises(ValueError, match="im/0000.png"):
        ie.evaluate_seg_predictions(pred_dir, base, samples[:1], ie.FileNameMode.id, PAL, region_of=lambda s, g: np.zeros(g.shape[:2], bool))


@pytest.mark.parametrize("batch_size", [1, 3])
def test_infer_and_evaluate_seg_equals_files_then_evaluate(tmp_path, batch_size):
    from genpercept_amd import infer_eval as ie
    base, pred_dir, ev_dir, out_dir = (str(tmp_path / d) for d in ("data", "pred", "eval_ref", "eval_dev"))
    samples = make_tree(base)
    region_of = region_files(base) if batch_size == 3 else None
    ie.run_inference(FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="seg")
    ref = ie.evaluate_seg_predictions(pred_dir, base, samples, ie.FileNameMode.id, (PAL, PAL_NAMES), output_dir=ev_dir, gt_tol=3, region_of=region_of)
    pipe = FakePipe()
    res = ie.infer_and_evaluate_seg(pipe, base, samples, (PAL, PAL_NAMES), output_dir=out_dir, batch_size=batch_size, evaluator=numpy_evaluator,
                                    region_of=region_of, gt_tol=3)
    assert pipe.batches == ([1] * 5 if batch_size == 1 else [3, 1, 1])   # (the batch of three mixes colour images and a label map)
    assert res == ref and list(res) == SEG_METRICS + ["miou_dataset", "pixel_acc_dataset", "iou_dataset"]   # equal, not close
    name = "per_sample_metrics-seg.csv"
    assert open(os.path.join(out_dir, name)).read() == open(os.path.join(ev_dir, name)).read()
    a, b = (open(os.path.join(d, "eval_metrics-seg.txt")).read().splitlines() for d in (out_dir, ev_dir))
    assert len(a) == len(b) and [x for x in a if "of predictions" not in x] == [x for x in b if "of predictions" not in x]
    assert not os.path.exists(os.path.join(out_dir, os.path.dirname(samples[0][0])))  # nothing saved unless asked for
    ie.infer_and_evaluate_seg(FakePipe(), base, samples, PAL, output_dir=out_dir, batch_size=2, evaluator=numpy_evaluator, save_predictions=True)
    for s in samples:
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        got = np.load(os.path.join(out_dir, name))
        assert got.ndim == 3 and got.shape[-1] == 3 and got.dtype == np.float32 and np.array_equal(got, np.load(os.path.join(pred_dir, name)))
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_seg(FakePipe(), base, samples, PAL, evaluator=numpy_evaluator, save_predictions=True)
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_seg(FakePipe(), base, samples, PAL, evaluator=numpy_evaluator, rank=2, world=2)

    class OneChannel(FakePipe):
        def predict_batch_device(self, images, mode, **kw):
            return super().predict_batch_device(images, mode, **kw)[:, :1]

    with pytest.raises(ValueError, match="three-channel"):
        ie.infer_and_evaluate_seg(OneChannel(), base, samples, PAL, evaluator=numpy_evaluator)


_WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from genpercept_amd import distributed as gd
from genpercept_amd import infer_eval as ie
import test_eval_seg_host as t
rank, local, world = gd.init_process_group("gloo")
samples = ie.read_filename_list({lst!r})
pipe = t.FakePipe()
res = ie.infer_and_evaluate_seg(pipe, {base!r}, samples, (t.PAL, t.PAL_NAMES), output_dir={out!r}, batch_size=2, rank=rank, world=world,
                                evaluator=t.numpy_evaluator, gt_tol=3)
with open(os.path.join({out!r}, "means_rank%d.json" % rank), "w") as f:
    json.dump(dict(res=res, images=sum(pipe.batches)), f)
dist.barrier()
dist.destroy_process_group()
print("RANK", rank, "OK", flush=True)
"""


def test_infer_and_evaluate_seg_world_size_2_gloo(tmp_path):
    """Two ranks share the five images without overlap, every rank returns the values over ALL images, rank 0 alone writes the table with the
    rows complete and in order.  The dataset-level values come from integer sums (exact in float64): bit for bit the one-process values.  The
    means are float64 sums of at most five terms in [0, 1] taken in another association: 1e-12 absolute is far above 5 * 2^-53."""
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(" ".join(s) for s in samples) + "\n")
    one = ie.infer_and_evaluate_seg(FakePipe(), base, samples, (PAL, PAL_NAMES), output_dir=str(tmp_path / "w1"), batch_size=2, evaluator=numpy_evaluator,
                                    gt_tol=3)
    out = str(tmp_path / "w2")
    os.makedirs(out)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lst=lst, base=base, out=out))
    port = 35500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 2, r.stdout + r.stderr
    seen = 0
    for rank in (0, 1):
        got = json.load(open(os.path.join(out, f"means_rank{rank}.json")))
        seen += got["images"]
        assert list(got["res"]) == list(one)
        for k in SEG_METRICS:
            assert abs(got["res"][k] - one[k]) <= 1e-12, (rank, k, got["res"][k], one[k])
        for k in ("miou_dataset", "pixel_acc_dataset", "iou_dataset"):
            assert got["res"][k] == one[k], (rank, k, got["res"][k], one[k])   # bit for bit
    assert seen == len(samples)                                      # disjoint and complete
    name = "per_sample_metrics-seg.csv"  # rank 0 alone wrote the files, rows in sample order: the table is the one-process table
    assert open(os.path.join(out, name)).read() == open(os.path.join(str(tmp_path / "w1"), name)).read()
    assert len(open(os.path.join(out, name)).read().splitlines()) == 1 + len(samples)
