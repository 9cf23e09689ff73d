"""CPU tests of the dis / matting evaluation: the device entries (gp_eval_mask_workspace / gp_eval_mask) are declared, exported by both
libraries and bound, and refuse bad arguments before any HIP call; the host route (eval_metrics.mask_counts / mask_metrics_from_counts /
mask_metrics) against exact rational arithmetic and against a brute-force definition without histograms; the file route and the loop
`infer_eval.infer_and_evaluate_masks` with a fake pipeline and the NumPy evaluator in place of engine.eval_mask, at world sizes 1 and 2 (gloo).

Bounds.  sad and iou are one correctly rounded quotient of exact integers (1 ulp of the rational value), mae and mse a product and a quotient
(2 ulp).  F_t is seven roundings deep and uses the rounded constants 1.3 and 0.3: numerator (1.3 prec) rec carries at most 5 relative errors of
2^-53 (the constant, the two quotients, two products), the all-positive denominator 0.3 prec + rec at most 4, the quotient 1 more -- 10 ulp of
the exact rational value at most.  The hand case's four values are held to 1 ulp of their fractions, and the brute-force float64 F_t (the
same formula on counts taken from boolean arrays) to 1 ulp.  mean_f is a left-to-right sum of 256 non-negative terms of 10 ulp each:
(256 + 10 + 1) ulp of the exact mean."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_eval_mask_workspace", "gp_eval_mask")
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
GP_ERR_INVALID = 1


def _libs():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


# ---- symbols -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert "run.py:449-455" in hdr
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
    assert len(engine.SYMBOLS["gp_eval_mask"][1]) == 12 and len(engine.SYMBOLS["gp_eval_mask_workspace"][1]) == 3
    assert engine.SYMBOLS["gp_eval_mask_workspace"][0] is C.c_longlong
    assert callable(engine.eval_mask_raw) and callable(engine.eval_mask)
    assert list(engine.MASK_METRICS) == list(em.MASK_METRICS) == list(ie.MASK_METRICS) == MASK_METRICS
    assert engine.MASK_COUNTS == em.MASK_COUNTS == 516
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in NAMES)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert lib.gp_eval_mask_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (1024, 1024), (1031, 2053), (4032, 6048)):
            one = lib.gp_eval_mask_workspace(1, h, w)
            assert one >= 8 * 516 // 2 and one % 8 == 0
            assert lib.gp_eval_mask_workspace(7, h, w) == 7 * one and lib.gp_eval_mask_workspace(65535, h, w) == 65535 * one
            assert lib.gp_eval_mask_workspace(1, w, h) == one and lib.gp_eval_mask_workspace(1, 1, h * w) == one  # H * W alone


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    P, G, R, O, CN, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000  # all 8-byte aligned
    for lib in _libs():
        need = lib.gp_eval_mask_workspace(2, 8, 8)
        ok = dict(pred=P, u8=0, gt=G, region=R, B=2, H=8, W=8, out=O, counts=CN, ws=WS, nbytes=need)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.gp_eval_mask(a["pred"], a["u8"], a["gt"], a["region"], a["B"], a["H"], a["W"], a["out"], a["counts"], a["ws"], a["nbytes"], None)

        huge = 1 << 62
        cases = [dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None),
                 dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
                 dict(B=65536, nbytes=lib.gp_eval_mask_workspace(65536, 8, 8)),                          # above the grid's y limit
                 dict(B=1, H=65536, W=65536, nbytes=huge), dict(B=1, H=1 << 16, W=1 << 15, nbytes=huge),  # H * W beyond 2^31 - 1
                 dict(u8=-1), dict(u8=2),
                 dict(out=O + 4), dict(counts=CN + 4), dict(counts=CN + 1), dict(ws=WS + 4),
                 dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=lib.gp_eval_mask_workspace(1, 8, 8))]
        for kw in cases:
            assert call(**kw) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_inputs_before_the_library():
    from genpercept_amd import engine
    with pytest.raises(ValueError):
        engine.eval_mask_raw(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        engine.eval_mask_raw(torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


# ---- the host route ------------------------------------------------------------------------------------------------------------------------
def within_ulp(value, exact: Fraction, ulps=1):
    """|value - exact| <= ulps * spacing(exact as a double), in exact arithmetic."""
    return abs(Fraction(float(value)) - exact) <= ulps * Fraction(float(np.spacing(abs(float(exact))) if exact != 0 else 0.0))


def exact_f(tp: int, p: int, n_fg: int) -> Fraction:
    prec, rec = Fraction(tp, max(p, 1)), Fraction(tp, max(n_fg, 1))
    den = Fraction(3, 10) * prec + rec
    return Fraction(13, 10) * prec * rec / den if den != 0 else Fraction(0)


def test_hand_case():
    from genpercept_amd import eval_metrics as em
    q, g = np.array([0, 100, 200, 255], np.uint8), np.array([0, 0, 255, 255], np.uint8)
    c = em.mask_counts(q, g)
    assert c.dtype == np.int64 and c.shape == (516,)
    assert tuple(c[:4]) == (4, 555, 155, 13025)
    assert c[4 + 0] == 1 and c[4 + 100] == 1 and c[4:260].sum() == 2 and c[260 + 200] == 1 and c[260 + 255] == 1 and c[260:].sum() == 2
    prec, rec, f = em.mask_curves_from_counts(c)
    for t in range(256):
        want = Fraction(13, 23) if t == 0 else Fraction(13, 18) if t <= 100 else Fraction(1) if t <= 200 else Fraction(13, 16)
        assert within_ulp(f[t], want), (t, f[t], want)
    m = em.mask_metrics_from_counts(c)
    assert list(m) == ["n", "n_fg"] + MASK_METRICS + ["t_max"]
    assert m["n"] == 4 and m["n_fg"] == 2 and m["max_f"] == 1.0 and m["t_max"] == 101 and m["iou"] == 1.0
    assert within_ulp(m["adp_f"], Fraction(13, 16))                                  # t_a = 255: 255 * 4 >= min(1110, 1020)
    assert within_ulp(m["mae"], Fraction(155, 255 * 4)) and within_ulp(m["mse"], Fraction(13025, 65025 * 4)) and within_ulp(m["sad"], Fraction(155, 255000))
    mean = (Fraction(13, 23) + 100 * Fraction(13, 18) + 100 + 55 * Fraction(13, 16)) / 256
    assert within_ulp(m["mean_f"], mean, ulps=267)
    assert em.mask_metrics(q, g) == m and em.mask_metrics(q.astype(np.float32) / np.float32(255.0) + np.float32(1e-3), g) == m


def brute_force(q, g, region):
    """The definitions with boolean arrays per threshold, no histograms: F_t in float64 (f64) and as exact rationals (f)."""
    sel = np.ones(q.shape, bool) if region is None else (region != 0)
    qs, gs = q[sel].astype(int), g[sel].astype(int)
    n, pos = int(sel.sum()), gs > 128
    n_fg = int(pos.sum())
    f, f64 = [], []
    for t in range(256):
        pp = qs >= t
        tp, p = int((pp & pos).sum()), int(pp.sum())
        f.append(exact_f(tp, p, n_fg))
        prec, rec = tp / max(p, 1), tp / max(n_fg, 1)
        f64.append((1.3 * prec * rec) / (0.3 * prec + rec) if 0.3 * prec + rec != 0.0 else 0.0)
    lim = min(2 * int(qs.sum()), 255 * n)
    t_a = next(t for t in range(256) if t * n >= lim)
    inter, union = int(((qs >= 128) & pos).sum()), int(((qs >= 128) | pos).sum())
    return dict(n=n, n_fg=n_fg, f=f, f64=f64, t_a=t_a, max_f=max(f), t_max=f.index(max(f)), mean_f=sum(f) / 256, mae=Fraction(int(np.abs(qs - gs).sum()), 255 * n),
                mse=Fraction(int(((qs - gs) ** 2).sum()), 65025 * n), sad=Fraction(int(np.abs(qs - gs).sum()), 255000),
                iou=Fraction(inter, union) if union else Fraction(0))


def random_case(h, w, seed, mask_like):
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 256, (h, w)).astype(np.uint8)
    q = rng.randint(0, 256, (h, w)).astype(np.uint8)
    if mask_like:
        g = np.where(rng.rand(h, w) < 0.9, np.where(rng.rand(h, w) < 0.4, 255, 0), g).astype(np.uint8)
        q = np.where(rng.rand(h, w) < 0.9, np.where((g > 128) ^ (rng.rand(h, w) < 0.1), 255, 0), q).astype(np.uint8)
    return q, g, rng.rand(h, w) < 0.6


@pytest.mark.parametrize("shape", [(7, 5), (64, 65)])
@pytest.mark.parametrize("mask_like", [False, True])
def test_mask_metrics_equal_the_brute_force_definition(shape, mask_like):
    from genpercept_amd import eval_metrics as em
    q, g, region = random_case(*shape, seed=31 + shape[0], mask_like=mask_like)
    for r in (None, region):
        ref = brute_force(q, g, r)
        c = em.mask_counts(q, g, r)
        m = em.mask_metrics(q, g, r)
        assert m == em.mask_metrics_from_counts(c)
        _, _, f = em.mask_curves_from_counts(c)
        assert m["n"] == ref["n"] == c[0] and m["n_fg"] == ref["n_fg"]
        for t in range(256):
            assert abs(f[t] - ref["f64"][t]) <= np.spacing(ref["f64"][t]), (t, f[t], ref["f64"][t])
            assert within_ulp(f[t], ref["f"][t], ulps=10), (t, f[t], ref["f"][t])
        assert m["max_f"] == max(f) and m["t_max"] == f.index(max(f)) and within_ulp(m["max_f"], ref["max_f"], ulps=10)
        assert m["adp_f"] == f[ref["t_a"]]
        for k in ("mae", "mse"):
            assert within_ulp(m[k], ref[k], ulps=2), (k, m[k], ref[k])   # two roundings: the product, the quotient
        assert within_ulp(m["sad"], ref["sad"]) and within_ulp(m["iou"], ref["iou"])
        assert within_ulp(m["mean_f"], ref["mean_f"], ulps=267)
        total = 0.0
        for t in range(256):
            total = total + f[t]
        assert m["mean_f"] == total / 256.0                               # left to right


def test_edge_cases():
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(3)
    q = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    g = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    # all-background ground truth: no positive, every F_t = 0, the first threshold wins; iou 0 / |pred >= 128|
    m = em.mask_metrics(q, np.minimum(g, 128))
    assert m["n_fg"] == 0 and m["max_f"] == 0.0 and m["mean_f"] == 0.0 and m["adp_f"] == 0.0 and m["t_max"] == 0 and m["iou"] == 0.0
    assert em.mask_metrics(np.zeros_like(q), np.zeros_like(g))["iou"] == 0.0          # the union is empty: 0.0 by definition
    # all-zero prediction: positive only at t = 0
    m = em.mask_metrics(np.zeros_like(q), g)
    n, n_fg = q.size, int((g > 128).sum())
    _, _, f = em.mask_curves_from_counts(em.mask_counts(np.zeros_like(q), g))
    assert within_ulp(f[0], exact_f(n_fg, n, n_fg)) and all(v == 0.0 for v in f[1:]) and m["t_max"] == 0 and m["max_f"] == f[0]
    assert m["adp_f"] == f[0] and m["iou"] == 0.0 and m["mean_f"] == f[0] / 256.0     # t_a = 0
    # all-255 prediction: positive at every threshold, a flat curve; t_a = 255
    m = em.mask_metrics(np.full_like(q, 255), g)
    _, _, f = em.mask_curves_from_counts(em.mask_counts(np.full_like(q, 255), g))
    assert len(set(f)) == 1 and within_ulp(f[0], exact_f(n_fg, n, n_fg)) and m["t_max"] == 0 and m["adp_f"] == f[255]
    assert within_ulp(m["iou"], Fraction(n_fg, n))
    # an empty region
    m = em.mask_metrics(q, g, np.zeros(q.shape, bool))
    assert m["n"] == 0 and m["n_fg"] == 0 and all(np.isnan(m[k]) for k in MASK_METRICS + ["t_max"])
    with pytest.raises(ValueError):
        em.mask_counts(q.astype(np.int32), g)


def test_quantisation_is_the_float32_product_truncated():
    """k / 255 in float32 and its two neighbours: the product of a float32 and 255 is exact in float64, so rounding it once to float32 and
    truncating is an independent statement of `(x * 255.0f)` -> byte.  Also the clip and the NaN rule."""
    from genpercept_amd import eval_metrics as em
    k = np.arange(256, dtype=np.float32)
    x = k / np.float32(255.0)
    xs = np.concatenate([x, np.nextafter(x, np.float32(-1.0)), np.nextafter(x, np.float32(2.0))]).astype(np.float32)
    want = np.floor(np.float32(np.clip(xs.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.float64)).astype(np.uint8)
    got = em.quantize_mask(xs)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[0] == 0 and got[255] == 255 and (np.abs(got[:256].astype(int) - np.arange(256)) <= 1).all()
    assert (got[256:512] <= got[:256]).all() and (got[512:] >= got[:256]).all()
    assert (got[256:512] < got[:256]).any()                          # a step below k / 255 does drop a level somewhere
    special = np.array([np.nan, -np.inf, np.inf, -0.0, -1e-9, 1.0 + 1e-6, 2.0, 0.999999], np.float32)
    assert em.quantize_mask(special).tolist() == [0, 0, 255, 0, 0, 255, 255, 254]
    assert em.quantize_mask(special.astype(np.float64)).tolist() == [0, 0, 255, 0, 0, 255, 255, 254]
    u8 = np.arange(256, dtype=np.uint8)
    assert em.quantize_mask(u8) is u8


# ---- the file route and the loop -------------------------------------------------------------------------------------------------------------
SIZES = [(24, 32), (24, 32), (24, 32), (20, 28), (24, 32)]  # (H, W): the fourth image has another size


def make_tree(base):
    """5 RGB images with an 8-bit mask each (mostly 0 / 255 with a soft edge; the second stored as an RGB file with equal channels) and a
    trimap-like region file; filename-list lines `rgb mask`."""
    rng = np.random.RandomState(17)
    samples = []
    for i, (h, w) in enumerate(SIZES):
        scene = os.path.join(base, f"set{i // 3}")
        for d in ("im", "gt", "trimap"):
            os.makedirs(os.path.join(scene, d), exist_ok=True)
        rgb = rng.randint(0, 255, (h, w, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(os.path.join(scene, "im", f"{i:04d}.png"))
        yy, xx = np.mgrid[0:h, 0:w]
        soft = np.clip((xx - w * (0.3 + 0.1 * i)) * 60 + 128, 0, 255).astype(np.uint8)
        soft[yy < 3] = 0
        Image.fromarray(soft if i != 1 else np.stack([soft] * 3, axis=-1)).save(os.path.join(scene, "gt", f"{i:04d}.png"))
        Image.fromarray(((soft > 0) & (soft < 255) | (rng.rand(h, w) < 0.2)).astype(np.uint8) * 128).save(os.path.join(scene, "trimap", f"{i:04d}.png"))
        samples.append([f"set{i // 3}/im/{i:04d}.png", f"set{i // 3}/gt/{i:04d}.png"])
    return samples


def fake_pred(img):
    """A deterministic [H, W] float32 map in [0, 1] from the RGB image, saturated over most of it."""
    a = np.asarray(img.convert("RGB")).astype(np.float32) / 255.0
    h, w = a.shape[:2]
    ramp = np.clip((np.arange(w, dtype=np.float32)[None] - w * 0.35) * 0.2 + 0.5, 0, 1)
    return np.clip(ramp + (a[..., 0] - 0.5) * 0.3 * (a[..., 1] > 0.8), 0, 1).astype(np.float32)


class FakePipe:
    def __init__(self):
        self.single, self.batches = 0, []

    def __call__(self, img, **kw):
        assert kw["batch_size"] == 0 and kw["color_map"] is None and kw["mode"] in ("dis", "matting")
        self.single += 1
        return SimpleNamespace(pred_np=fake_pred(img), pred_colored=None)

    def predict_batch_device(self, images, mode, **kw):
        assert mode in ("dis", "matting") and len({im.size for im in images}) == 1
        self.batches.append(len(images))
        return torch.from_numpy(np.stack([fake_pred(im)[None] for im in images]))


def numpy_evaluator(pred, gt, region):
    """engine.eval_mask's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    out = []
    for i in range(pred.shape[0]):
        c = em.mask_counts(em.quantize_mask(pred[i].numpy()), gt[i].numpy(), None if region is None else region[i].numpy())
        out.append(dict(em.mask_metrics_from_counts(c), counts=c))
    return out


def trimap_region(base):
    def region_of(sample, gt):
        r = np.asarray(Image.open(os.path.join(base, sample[1].replace("/gt/", "/trimap/")))) == 128
        assert r.shape == gt.shape
        return r
    return region_of


def test_read_gt_mask(tmp_path):
    from genpercept_amd import infer_eval as ie
    a = np.random.RandomState(0).randint(0, 256, (6, 9)).astype(np.uint8)
    Image.fromarray(a).save(tmp_path / "l.png")
    Image.fromarray(np.stack([a] * 3, axis=-1)).save(tmp_path / "rgb.png")
    b = np.stack([a, a, a], axis=-1)
    b[2, 3, 1] ^= 1
    Image.fromarray(b).save(tmp_path / "bad.png")
    Image.fromarray(a.astype(np.uint16) * 200).save(tmp_path / "u16.png")
    for name in ("l.png", "rgb.png"):
        g = ie.read_gt_mask(str(tmp_path / name))
        assert g.dtype == np.uint8 and g.shape == (6, 9) and np.array_equal(g, a) and g.flags["C_CONTIGUOUS"]
    for name in ("bad.png", "u16.png"):
        with pytest.raises(ValueError):
            ie.read_gt_mask(str(tmp_path / name))


@pytest.mark.parametrize("with_region", [False, True])
def test_evaluate_mask_predictions_npy_and_png_routes(tmp_path, with_region):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base, pred_dir, png_dir, out = (str(tmp_path / d) for d in ("data", "pred", "pred_png", "eval"))
    samples = make_tree(base)
    region_of = trimap_region(base) if with_region else None
    pipe = FakePipe()
    written = ie.run_inference(pipe, base, samples, pred_dir, ie.FileNameMode.id, mode="dis")
    assert pipe.single == 5 and len(written) == 5
    for p in written:  # the 8-bit image of the same map
        dst = os.path.join(png_dir, os.path.relpath(p, pred_dir))[:-4] + ".png"
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        Image.fromarray(em.quantize_mask(np.load(p))).save(dst)
    os.remove(written[4])                                            # a sample without a prediction file is skipped ...
    with_gaps = samples[:2] + [["x.png", "None"], ["y.png"]] + samples[2:]  # ... and so is one without ground truth
    res = ie.evaluate_mask_predictions(pred_dir, base, with_gaps, ie.FileNameMode.id, output_dir=out, region_of=region_of)
    assert list(res) == MASK_METRICS + ["max_f_dataset"]
    rows, curves = [], np.zeros((2, 256))
    for s, path in zip(samples[:4], written[:4]):
        gt = ie.read_gt_mask(os.path.join(base, s[1]))
        c = em.mask_counts(em.quantize_mask(np.load(path)), gt, region_of(s, gt) if with_region else None)
        rows.append(em.mask_metrics(np.load(path), gt, region_of(s, gt) if with_region else None))
        prec, rec, _ = em.mask_curves_from_counts(c)
        curves[0] += prec
        curves[1] += rec
    for k in MASK_METRICS:
        assert res[k] == sum(r[k] for r in rows) / 4, k
    p, r = curves[0] / 4, curves[1] / 4
    with np.errstate(all="ignore"):
        want = np.nanmax(np.where(0.3 * p + r != 0, (1.3 * p * r) / (0.3 * p + r), 0.0))
    assert res["max_f_dataset"] == want and 0.0 < want <= 1.0
    assert res["max_f_dataset"] != res["max_f"]                     # the dataset-level value is not the mean of the per-image maxima
    lines = open(os.path.join(out, "per_sample_metrics-mask.csv")).read().splitlines()
    assert lines[0] == "filename," + ",".join(MASK_METRICS) and len(lines) == 1 + 4
    for ln, s, row in zip(lines[1:], samples, rows):
        assert ln == os.path.join(os.path.dirname(s[0]), "pred_" + os.path.basename(s[0])[:-4] + ".npy") + "," + ",".join(str(row[k]) for k in MASK_METRICS)
    txt = open(os.path.join(out, "eval_metrics-mask.txt")).read().splitlines()
    assert txt[-2] == "  ".join(MASK_METRICS) and txt[-1] == "  ".join(f"{res[k]:.6g}" for k in MASK_METRICS)
    assert f"max_f_dataset = {res['max_f_dataset']:.6g}" in txt
    # the .png route reads the same bytes
    res_png = ie.evaluate_mask_predictions(png_dir, base, samples[:4], ie.FileNameMode.id, pred_suffix=".png", region_of=region_of)
    assert res_png == res
    assert all(np.isnan(v) for v in ie.evaluate_mask_predictions(pred_dir, base, [["x.png", "None"]], ie.FileNameMode.id).values())
    with pytest.raises(ValueError, match="im/0000.png"):
        ie.evaluate_mask_predictions(pred_dir, base, samples[:1], ie.FileNameMode.id, region_of=lambda s, g: np.zeros(g.shape, bool))


@pytest.mark.parametrize("batch_size", [1, 3])
def test_infer_and_evaluate_masks_equals_files_then_evaluate(tmp_path, batch_size):
    from genpercept_amd import infer_eval as ie
    base, pred_dir, ev_dir, out_dir = (str(tmp_path / d) for d in ("data", "pred", "eval_ref", "eval_dev"))
    samples = make_tree(base)
    region_of = trimap_region(base) if batch_size == 3 else None
    ie.run_inference(FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="matting")
    ref = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=ev_dir, region_of=region_of)
    pipe = FakePipe()
    res = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=out_dir, batch_size=batch_size, evaluator=numpy_evaluator,
                                      region_of=region_of)
    assert pipe.batches == ([1] * 5 if batch_size == 1 else [3, 1, 1])
    assert res == ref and list(res) == MASK_METRICS + ["max_f_dataset"]   # the same operations in the same order: equal, not close
    name = "per_sample_metrics-mask.csv"
    assert open(os.path.join(out_dir, name)).read() == open(os.path.join(ev_dir, name)).read()
    a, b = (open(os.path.join(d, "eval_metrics-mask.txt")).read().splitlines() for d in (out_dir, ev_dir))
    assert len(a) == len(b) and [x for x in a if "of predictions" not in x] == [x for x in b if "of predictions" not in x]
    assert not os.path.exists(os.path.join(out_dir, os.path.dirname(samples[0][0])))  # nothing saved unless asked for
    ie.infer_and_evaluate_masks(FakePipe(), base, samples, "dis", output_dir=out_dir, batch_size=2, evaluator=numpy_evaluator, save_predictions=True)
    for s in samples:
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        got = np.load(os.path.join(out_dir, name))
        assert got.ndim == 2 and got.dtype == np.float32 and np.array_equal(got, np.load(os.path.join(pred_dir, name)))
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_masks(FakePipe(), base, samples, "dis", evaluator=numpy_evaluator, save_predictions=True)
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_masks(FakePipe(), base, samples, "dis", evaluator=numpy_evaluator, rank=2, world=2)
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_masks(FakePipe(), base, samples, "seg", evaluator=numpy_evaluator)


_WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from genpercept_amd import distributed as gd
from genpercept_amd import infer_eval as ie
import test_eval_mask_host as t
rank, local, world = gd.init_process_group("gloo")
samples = ie.read_filename_list({lst!r})
pipe = t.FakePipe()
res = ie.infer_and_evaluate_masks(pipe, {base!r}, samples, "dis", output_dir={out!r}, batch_size=2, rank=rank, world=world,
                                  evaluator=t.numpy_evaluator)
with open(os.path.join({out!r}, "means_rank%d.json" % rank), "w") as f:
    json.dump(dict(res=res, images=sum(pipe.batches)), f)
dist.barrier()
dist.destroy_process_group()
print("RANK", rank, "OK", flush=True)
"""


def test_infer_and_evaluate_masks_world_size_2_gloo(tmp_path):
    """Two ranks share the five images without overlap, every rank returns the values over ALL images, rank 0 alone writes the table.  The
    means and max_f_dataset are float64 sums of at most five terms in [0, 1] (thousands for sad) taken in another association: 1e-12
    absolute is far above 5 * 2^-53 and far below any real difference."""
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(" ".join(s) for s in samples) + "\n")
    one = ie.infer_and_evaluate_masks(FakePipe(), base, samples, "dis", output_dir=str(tmp_path / "w1"), batch_size=2, evaluator=numpy_evaluator)
    out = str(tmp_path / "w2")
    os.makedirs(out)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lst=lst, base=base, out=out))
    port = 33500 + (os.getpid() % 2000)
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
        for k in one:
            assert abs(got["res"][k] - one[k]) <= 1e-12, (rank, k, got["res"][k], one[k])
    assert seen == len(samples)                                      # disjoint and complete
    name = "per_sample_metrics-mask.csv"  # rank 0 alone wrote the files, rows in sample order: the table is the one-process table
    assert open(os.path.join(out, name)).read() == open(os.path.join(str(tmp_path / "w1"), name)).read()
    assert len(open(os.path.join(out, name)).read().splitlines()) == 1 + len(samples)
