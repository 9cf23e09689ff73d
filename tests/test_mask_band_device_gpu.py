"""Trimap and boundary bands on the device (gp_mask_band): every plane of `engine.mask_band` BIT-EQUAL to the host route
`eval_metrics.mask_band` (itself pinned to a brute-force distance and to scipy morphology in tests/test_mask_band_host.py), over shapes that
take every path of the two kernels (one pixel, one row, rows that are no multiple of anything, several column segments, several row tiles, a
reach above the staged apron), hand-made inputs, both metrics, both border rules, uint8 and float input; batch independence; `eval_trimap`
and `eval_boundary_iou` against their host routes; the argument checks with real buffers around them; the loop options with the real pipeline
at tiny widths.  There is no tolerance in this file: integers, or one float64 division of integers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_band_host import (BOUNDARY_METRICS, GP_ERR_INVALID, MASK_METRICS, PLANES, REACHES, THRESHOLDS, TRIMAP_METRICS, call_band,  # noqa: E402
                                 invalid_cases, random_map)
from post_support import tiny_weights_dict, unaligned  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (3, 64, 65), (1, 300, 3), (1, 257, 515), (1, 3, 8200)]
# the host file's grid, a disc and a square of everyday size, and one reach of each metric above the 1024 columns of apron the row pass stages
GRID = REACHES + [(0, 625), (1, 12), (0, 1500000), (1, 1100)]
FEW = [(0, 8), (1, 3), (0, 10 ** 6), (1, 1100)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def inputs(b, h, w, seed):
    """name -> uint8 [B, H, W]: random blocks, all 0, all 255, a single set pixel, all transitional, a checkerboard."""
    rng = np.random.RandomState(seed)
    single = np.zeros((b, h, w), np.uint8)
    single[:, h // 2, (2 * w) // 3] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    return {"random blocks": np.stack([random_map(rng, h, w) for _ in range(b)]), "all 0": np.zeros((b, h, w), np.uint8),
            "all 255": np.full((b, h, w), 255, np.uint8), "single pixel": single, "all transitional": np.full((b, h, w), 128, np.uint8),
            "checkerboard": np.broadcast_to(((yy + xx) % 2 * 255).astype(np.uint8), (b, h, w)).copy()}


def check(a_np, a_dev, lo, hi, reach, metric, border, what):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    got = ge.mask_band(a_dev, lo, hi, reach, ("euclidean", "chebyshev")[metric], bool(border), want=PLANES)
    assert list(got) == PLANES
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for i in range(a_np.shape[0]):
        want = em.mask_band(a_np[i], lo, hi, reach, metric, border)
        for k in PLANES:
            assert got[k].dtype == np.uint8 and np.array_equal(got[k][i], want[k]), (what, i, lo, hi, metric, reach, border, k,
                                                                                        int((got[k][i] != want[k]).sum()))


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_band_equals_the_host_route(shape):
    b, h, w = shape
    n = 0
    for name, a in inputs(b, h, w, 3000 + h).items():
        a_dev = unaligned(a)
        assert a_dev.data_ptr() % 2 == 1
        for metric, reach in (GRID if name == "random blocks" else FEW):
            for border in (0, 1):
                lo, hi = THRESHOLDS[n % len(THRESHOLDS)]
                n += 1
                check(a, a_dev, lo, hi, reach, metric, border, name)


@gpu
@pytest.mark.parametrize("shape", [(3, 64, 65), (1, 257, 515)], ids=lambda s: "x".join(map(str, s)))
def test_mask_band_float_input_is_quantised_first(shape):
    """Values on and around the k / 255 edges (and NaN, values outside [0, 1]) give the planes of `quantize_mask`'s bytes."""
    from genpercept_amd import eval_metrics as em
    b, h, w = shape
    rng = np.random.RandomState(77)
    k = np.stack([random_map(rng, h, w) for _ in range(b)]).astype(np.float32)
    f = k / np.float32(255.0)
    f = np.where(rng.rand(b, h, w) < 0.3, np.nextafter(f, np.float32(-1.0)), np.where(rng.rand(b, h, w) < 0.3, np.nextafter(f, np.float32(2.0)), f))
    f = f.astype(np.float32)
    f[:, 0, 0], f[:, -1, -1], f[:, h // 2, w // 2] = np.nan, 1.5, -0.25
    q = np.stack([em.quantize_mask(x) for x in f])
    assert len(np.unique(q)) > 6
    f_dev = unaligned(f)
    for n, ((metric, reach), border) in enumerate([(g, bd) for g in [(0, 2), (0, 625), (1, 3), (1, 12)] for bd in (0, 1)]):
        lo, hi = THRESHOLDS[n % len(THRESHOLDS)]
        check(q, f_dev, lo, hi, reach, metric, border, "float")
    from genpercept_amd import engine as ge
    for dt in (torch.float16, torch.float64):                        # other float types go through float32, like eval_mask
        x = torch.from_numpy(q.astype(np.float32) / 255.0 + 0.001).cuda()
        assert torch.equal(ge.mask_band(x.to(dt), 0, 255, 4)["band"], ge.mask_band(x.to(dt).to(torch.float32), 0, 255, 4)["band"])


@gpu
def test_mask_band_is_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    rng = np.random.RandomState(5)
    for h, w in ((64, 65), (257, 515)):
        a = torch.from_numpy(np.stack([random_map(rng, h, w) for _ in range(3)])).cuda()
        for metric, reach, border in (("euclidean", 625, False), ("chebyshev", 12, True), ("euclidean", 2, True)):
            whole = ge.mask_band(a, 0, 255, reach, metric, border, want=PLANES)
            again = ge.mask_band(a, 0, 255, reach, metric, border, want=PLANES)
            for i in range(3):
                one = ge.mask_band(a[i], 0, 255, reach, metric, border, want=PLANES)
                for k in PLANES:
                    assert torch.equal(one[k][0], whole[k][i]) and torch.equal(again[k], whole[k])
            # a subset of the planes, in another order, and the shapes eval_mask takes
            some = ge.mask_band(a[:, None], 0, 255, reach, metric, border, want=("trimap", "band"))
            assert list(some) == ["trimap", "band"] and torch.equal(some["trimap"], whole["trimap"]) and torch.equal(some["band"], whole["band"])
    with pytest.raises(ValueError):
        ge.mask_band(a, 0, 255, 4, want=())
    with pytest.raises(ValueError):
        ge.mask_band(a, 0, 255, 4, want=("band", "edge"))
    with pytest.raises(ValueError):
        ge.mask_band(a, 0, 255, 4, metric="manhattan")
    with pytest.raises(ValueError):
        ge.mask_band(a, 5, 5, 4)
    with pytest.raises(ValueError):
        ge.mask_band(a, 0, 255, 4097, metric="chebyshev")


@gpu
@pytest.mark.parametrize("shape", [(3, 64, 65), (1, 257, 515)], ids=lambda s: "x".join(map(str, s)))
def test_eval_trimap_and_boundary_iou_equal_their_host_routes(shape):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    b, h, w = shape
    rng = np.random.RandomState(11 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    gt = np.stack([np.clip((np.hypot(yy - h * (0.4 + 0.1 * i), xx - w * 0.5) - min(h, w) * 0.3) * -20 + 128, 0, 255).astype(np.uint8) for i in range(b)])
    gt[0, :, : w // 8] = 255                                          # the first object touches the image edge
    pred = np.clip(gt / 255.0 + 0.3 * rng.randn(b, h, w) * (rng.rand(b, h, w) < 0.2), 0, 1).astype(np.float32)
    pred_d, gt_d = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for radius, metric in ((3, "chebyshev"), (2.5, "euclidean"), (25, "euclidean")):
        got = ge.eval_trimap(pred_d, gt_d, radius, metric)
        assert len(got) == b
        for i in range(b):
            want = em.trimap_metrics(pred[i], gt[i], radius, metric)
            assert list(got[i]) == list(want) and list(want)[:5] == TRIMAP_METRICS
            for k in want:
                assert same_bits(got[i][k], want[k]), (radius, metric, i, k, got[i][k], want[k])
            assert want["n_t"] > 0 and want["sad_t"] > 0 and (radius > 3 or min(want["n_fg_side"], want["n_bg_side"]) > 0)
    assert ge.eval_trimap(pred_d, gt_d, 2.5) == ge.eval_trimap(pred_d[:, None], gt_d[:, None], 2.5, "euclidean")
    for ratio in (0.02, 0.05):
        got = ge.eval_boundary_iou(pred_d, gt_d, ratio)
        for i in range(b):
            want = em.boundary_iou(pred[i], gt[i], ratio)
            assert list(got[i]) == list(want) == BOUNDARY_METRICS + ["d", "n_gt_band", "n_pred_band"]
            for k in want:
                assert same_bits(got[i][k], want[k]), (ratio, i, k, got[i][k], want[k])
            assert 0.0 < want["biou"] < 1.0 and want["n_gt_band"] > 0
    q8 = torch.from_numpy(em.quantize_mask(pred)).cuda()
    binary = (gt_d > 128).to(torch.uint8) * 255                       # (P is q >= 128, G is g > 128: the byte 128 sits between them)
    assert ge.eval_boundary_iou(q8, gt_d) == ge.eval_boundary_iou(pred_d, gt_d) and all(m["biou"] == 1.0 for m in ge.eval_boundary_iou(binary, gt_d))
    # an empty transition region is the n = 0 error, naming the image
    flat = gt_d.clone()
    flat[b - 1] = 255
    with pytest.raises(ValueError, match=f"image {b - 1}"):
        ge.eval_trimap(pred_d, flat, 3)


@gpu
def test_mask_band_refuses_invalid_arguments_before_touching_the_device():
    """The host test's cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill."""
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    d = torch.device("cuda", 0)
    need = int(lib.gp_mask_band_workspace(2, 8, 8))
    a = torch.randint(0, 256, (2, 8, 8), dtype=torch.uint8, device=d)
    af = torch.rand(2, 8, 8, device=d)
    planes = torch.full((5, 2, 8, 8), 99, dtype=torch.uint8, device=d)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=d)
    ok = dict(a=a.data_ptr(), u8=1, B=2, H=8, W=8, lo=0, hi=255, metric=0, reach=4, border=0, ws=ws.data_ptr(), nbytes=need,
              **{k: planes[j].data_ptr() for j, k in enumerate(PLANES)})
    cases = [c for c in invalid_cases(ok, int(lib.gp_mask_band_workspace(1, 8, 8))) if "u8" not in c or "a" not in c]
    cases.append(dict(u8=0, a=af.data_ptr() + 2))
    for kw in cases:
        assert call_band(lib, dict(ok, **kw)) == GP_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert (planes == 99).all() and (ws == 0x5A).all()
    assert call_band(lib, ok) == 0                                   # ... and the valid set goes through
    torch.cuda.synchronize()
    assert not (planes == 99).any()


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_infer_and_evaluate_masks_band_options_with_the_pipeline(tiny_weights, tmp_path):
    """The device loop for mode "matting" with trimap_radius=3 and boundary_iou=True: three 96 x 128 images and one 64 x 64, batch_size 2.
    == host evaluate_mask_predictions with the same options over the `.npy` maps it saved, every column bit for bit; with the options off the
    loop gives what it gave before."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(47)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype=torch.bfloat16)
    pipe.to("cuda")
    base, out, ref_dir, off_dir, old_dir = (str(tmp_path / d) for d in ("data", "out", "ref", "off", "old"))
    samples, sizes = [], [(96, 128), (96, 128), (96, 128), (64, 64)]
    for i, (h, w) in enumerate(sizes):
        for sub in ("im", "gt"):
            os.makedirs(os.path.join(base, "set0", sub), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "set0", "im", f"{i:04d}.png"))
        xx = np.arange(w)[None].repeat(h, 0)
        Image.fromarray(np.clip((xx - (w // 3 + 10 * i)) * 6 + 128, 0, 255).astype(np.uint8)).save(os.path.join(base, "set0", "gt", f"{i:04d}.png"))
        samples.append([f"set0/im/{i:04d}.png", f"set0/gt/{i:04d}.png"])
    on = dict(trimap_radius=3, boundary_iou=True)
    try:
        res = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=out, batch_size=2, save_predictions=True, processing_res=0, **on)
        off = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=off_dir, batch_size=2, processing_res=0)
        ref = ie.evaluate_mask_predictions(out, base, samples, ie.FileNameMode.id, output_dir=ref_dir, **on)
        old = ie.evaluate_mask_predictions(out, base, samples, ie.FileNameMode.id, output_dir=old_dir)
        for k in ref:
            print(f"infer_and_evaluate_masks[bf16, bands] {k}: device {res[k]!r} host {ref[k]!r}")
        names = MASK_METRICS + TRIMAP_METRICS + BOUNDARY_METRICS
        assert list(res) == list(ref) == names + ["max_f_dataset"] and all(np.isfinite(v) for v in res.values())
        assert all(same_bits(res[k], ref[k]) for k in res)
        assert list(off) == list(old) == MASK_METRICS + ["max_f_dataset"] and all(same_bits(off[k], res[k]) and same_bits(off[k], old[k]) for k in off)
        assert res["sad_t"] > 0 and res["sad_fg"] >= 0 and res["sad_bg"] >= 0
        name = "per_sample_metrics-mask.csv"
        rows, rows_ref, rows_off, rows_old = (open(os.path.join(d, name)).read().splitlines() for d in (out, ref_dir, off_dir, old_dir))
        assert rows == rows_ref and rows[0] == "filename," + ",".join(names) and len(rows) == 1 + len(samples)
        assert rows_off == rows_old and rows_off[0] == "filename," + ",".join(MASK_METRICS)
        txt = open(os.path.join(out, "eval_metrics-mask.txt")).read()
        assert "radius 3, metric euclidean" in txt and "boundary IoU: band of 0.02" in txt
        assert "radius" not in open(os.path.join(off_dir, "eval_metrics-mask.txt")).read()
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
