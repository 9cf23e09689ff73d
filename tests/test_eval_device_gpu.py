"""Depth evaluation on the device (gp_eval_depth, csrc/eval.hip; engine.eval_depth) against the project's host evaluation
(eval_metrics.py, the restatement of eval.py:168-215, alignment.py:29-94, metric.py:34-158), and the batched device loop
`infer_eval.infer_and_evaluate` with the real pipeline at tiny widths.

The reference side is always host code: `np.linalg.lstsq` for (s, t), and `host_metrics` below -- the float32 apply / clip recipe of
`evaluate_depth` for a GIVEN (s, t), then `eval_metrics.METRICS` in float64.  test_host_metrics_is_evaluate_depth (no GPU) pins that helper to
`evaluate_depth` itself.

Bounds.  n_valid, n_fit: exact.  s, t: one float32 ulp of lstsq's (both sides solve in float64 and round to float32).  delta1..3: exact --
integer counts over n_valid, correctly rounded float64 divisions on both sides.  The other seven: relative 1e-9 against host_metrics WITH THE
DEVICE'S (s, t): float64 sums over at most 2.1e6 non-negative terms in another order (n * 2^-53 = 2.4e-10) plus last-bit `log` / `log10`
differences.

The image with exactly two valid pixels holds pred (0.25, 0.75) and gt (2, 4): two points fit exactly -- in depth space s = 4, t = 1, in
disparity space s = -0.5, t = 0.625, every product and sum exact in float32 -- so the aligned values EQUAL the ground truth and the error
metrics are exactly 0 on both sides.  With arbitrary values an exact two-point fit leaves log(a) - log(g) ~ 1e-8 (float32 rounding of the
aligned value), where one last-bit difference between two `log` implementations (1e-16) is already 1e-8 relative: noise, not a property of the
kernel.  Without alignment the same image gives ordinary, well-conditioned values.
"""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

ALIGNMENTS = [None, "least_square", "least_square_disparity"]
RANGES = [(1e-3, 10.0), (1e-5, float("inf"))]


def host_metrics(pred, gt, mask, s, t, alignment, min_depth, max_depth):
    """evaluate_depth's float32 apply / clip for a given (s, t) -- two roundings, no FMA -- then the ten host metrics in float64."""
    from genpercept_amd import eval_metrics as em
    aligned = pred
    if alignment:
        aligned = pred * np.float32(s) + np.float32(t)
        if alignment == "least_square_disparity":
            aligned, _ = em.disparity2depth(np.clip(aligned, 1e-3, None))
    aligned = np.clip(np.clip(aligned, min_depth, max_depth), 1e-6, None)
    assert aligned.dtype == np.float32
    a, g, m = aligned.astype(np.float64)[None], gt.astype(np.float64)[None], mask.astype(bool)[None]
    with np.errstate(all="ignore"):
        return {k: f(a, g, m) for k, f in em.METRICS.items()}


def host_fit(pred, gt, mask, alignment, max_res):
    """(s, t, n_fit) as evaluate_depth obtains them: lstsq over the (column-subsampled) fit mask, in depth or disparity space."""
    from genpercept_amd import eval_metrics as em
    if not alignment:
        return 1.0, 0.0, 0
    target, m = gt, mask
    if alignment == "least_square_disparity":
        target, pos = em.depth2disparity(gt)
        m = mask & pos & (pred > 0)
    _, s, t = em.align_depth_least_square(target, pred, m, max_res)
    if max_res is not None:
        scale = float(np.min(max_res / np.array(pred.shape[-2:])))
        if scale < 1:
            m = em._nearest_downscale(m, scale)
    return s, t, int(m.sum())


def make_case(b, h, w, seed, max_depth, disparity=False):
    """pred: smooth + noise in [0, 1]; gt = a * pred**1.3 + b + noise (not an affine image of pred; for the disparity protocol a decreasing
    function of pred); mask = range test & random mask.  Zeros are planted in pred and gt."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    pred, gt, mask = [], [], []
    for i in range(b):
        smooth = 0.5 + 0.35 * np.sin(3.1 * xx + 0.7 * i) * np.cos(2.3 * yy - 0.4 * i)
        p = np.clip(smooth + 0.05 * rng.randn(h, w), 0.0, 1.0).astype(np.float32)
        p[rng.rand(h, w) < 0.02] = 0.0
        q = (1.0 - p) if disparity else p
        g = (9.0 * q.astype(np.float64) ** 1.3 + 0.8 + 0.05 * rng.randn(h, w)).astype(np.float32)
        g[rng.rand(h, w) < 0.03] = 0.0
        m = (g > 1e-3) & (g < max_depth) & (rng.rand(h, w) < (0.8 - 0.2 * i))  # another mask per image
        pred.append(p), gt.append(g), mask.append(m)
    return np.stack(pred), np.stack(gt), np.stack(mask)


def nyu_crop(mask):
    from genpercept_amd import infer_eval as ie
    y0, y1, x0, x1 = ie.DATASETS["nyu"]["eval_crop"]
    c = np.zeros_like(mask)
    c[..., y0:y1, x0:x1] = True
    return mask & c


def plant_two_pixel_image(pred, gt, mask, i):
    """Image i: exactly two valid pixels, in columns 0 and 2 (both survive the max_res = 20 column sampling of a 53-wide image), with values
    whose two-point fit is exact (module docstring)."""
    mask[i] = False
    for (y, x), p, g in (((5, 0), 0.25, 2.0), ((20, 2), 0.75, 4.0)):
        pred[i, y, x], gt[i, y, x], mask[i, y, x] = p, g, True


def check_against_host(pred, gt, mask, alignment, max_res, lo, hi):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    tp, tg, tm = torch.from_numpy(pred).to(d), torch.from_numpy(gt).to(d), torch.from_numpy(mask).to(d)
    raw = ge.eval_depth_raw(tp, tg, tm, alignment, max_res, lo, hi).cpu().numpy()
    metrics, (s_all, t_all, nv_all) = ge.eval_depth(tp, tg, tm, alignment, max_res, lo, hi)
    names = list(em.METRICS)
    worst = 0.0
    for i in range(pred.shape[0]):
        tag = (pred.shape, i, alignment, max_res, lo, hi)
        s_h, t_h, n_fit = host_fit(pred[i], gt[i], mask[i], alignment, max_res)
        s_d, t_d, n_valid_d, n_fit_d = raw[i, :4]
        assert n_valid_d == mask[i].sum() == nv_all[i] and n_fit_d == n_fit, (tag, n_valid_d, mask[i].sum(), n_fit_d, n_fit)
        assert s_d == np.float32(s_d) and t_d == np.float32(t_d) and s_all[i] == s_d and t_all[i] == t_d  # float32 values
        print(f"eval_depth {tag}: s dev {s_d!r} host {s_h!r}  t dev {t_d!r} host {t_h!r}")
        assert abs(s_d - s_h) <= np.spacing(np.float32(abs(s_h))), (tag, s_d, s_h)
        assert abs(t_d - t_h) <= np.spacing(np.float32(abs(t_h))), (tag, t_d, t_h)
        ref = host_metrics(pred[i], gt[i], mask[i], s_d, t_d, alignment, lo, hi)
        for j, k in enumerate(names):
            dev = raw[i, 4 + j]
            assert metrics[i][k] == dev
            err = abs(dev - ref[k]) / abs(ref[k]) if ref[k] != 0 else abs(dev)
            worst = max(worst, err)
            print(f"    {k}: dev {dev!r} host {ref[k]!r} rel {err:.3e}")
            if k.startswith("delta"):
                assert dev == ref[k], (tag, k, dev, ref[k])
            else:
                assert abs(dev - ref[k]) <= 1e-9 * abs(ref[k]), (tag, k, dev, ref[k])
    return worst


def test_host_metrics_is_evaluate_depth():
    """No GPU: the reference helper of this file, fed with lstsq's own (s, t), IS eval_metrics.evaluate_depth -- all ten values, bit for bit,
    for every alignment, with the column-subsampled fit and with both depth ranges."""
    from genpercept_amd import eval_metrics as em
    for lo, hi in RANGES:
        for alignment, max_res in [(a, None) for a in ALIGNMENTS] + [("least_square", 20), ("least_square_disparity", 20)]:
            pred, gt, mask = make_case(3, 37, 53, 11, hi, disparity=alignment == "least_square_disparity")
            plant_two_pixel_image(pred, gt, mask, 2)
            for i in range(3):
                s, t, n_fit = host_fit(pred[i], gt[i], mask[i], alignment, max_res)
                assert n_fit >= 2 or not alignment
                with np.errstate(all="ignore"):
                    want = em.evaluate_depth(pred[i], gt[i], mask[i], lo, hi, alignment=alignment, alignment_max_res=max_res)
                got = host_metrics(pred[i], gt[i], mask[i], s, t, alignment, lo, hi)
                assert got == want, (alignment, max_res, lo, hi, i)
                if i == 2 and alignment:
                    assert got["abs_relative_difference"] == 0.0 and got["delta1_acc"] == 1.0


def test_eval_depth_argument_checks():
    """No GPU: gp_eval_depth refuses null pointers, B < 1, an empty image, an unknown alignment and a short workspace before it touches the
    device; the workspace size depends on B and H * W only."""
    import __graft_entry__ as entry
    entry.build()
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    assert lib.gp_eval_depth_workspace(0, 4, 4) == 0 and lib.gp_eval_depth_workspace(1, 0, 4) == 0 and lib.gp_eval_depth_workspace(1, 4, 0) == 0
    one = lib.gp_eval_depth_workspace(1, 480, 640)
    assert one > 0 and one % 8 == 0 and lib.gp_eval_depth_workspace(3, 480, 640) == 3 * one == 3 * lib.gp_eval_depth_workspace(1, 640, 480)
    p = 4096  # any non-null, aligned address: every call below is refused before a kernel is launched

    def call(pred=p, gt=p, mask=p, b=1, h=8, w=8, alignment=1, fit_cols=0, inv=0.0, out=p, ws=p, nbytes=None):
        nbytes = lib.gp_eval_depth_workspace(max(b, 1), max(h, 1), max(w, 1)) if nbytes is None else nbytes
        return lib.gp_eval_depth(pred, gt, mask, b, h, w, alignment, fit_cols, inv, 1e-3, 10.0, out, ws, nbytes, None)
    INVALID = 1
    for kw in (dict(pred=None), dict(gt=None), dict(mask=None), dict(out=None), dict(ws=None), dict(b=0), dict(h=0), dict(w=0), dict(alignment=3),
               dict(alignment=-1), dict(nbytes=lib.gp_eval_depth_workspace(1, 8, 8) - 1), dict(b=2, nbytes=lib.gp_eval_depth_workspace(1, 8, 8)),
               dict(fit_cols=9, inv=2.0), dict(fit_cols=4, inv=0.0)):
        assert call(**kw) == INVALID, kw
    with pytest.raises(NotImplementedError):
        ge.eval_depth_raw(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.bool), "median")


@gpu
@pytest.mark.parametrize("shape", [(1, 7, 5), (3, 37, 53), (2, 480, 640), (1, 1031, 2053)], ids=lambda s: "x".join(map(str, s)))
def test_eval_depth_matches_host(shape, metric_log):
    b, h, w = shape
    worst = 0.0
    for lo, hi in RANGES:
        for alignment in ALIGNMENTS:
            pred, gt, mask = make_case(b, h, w, 100 + h, hi, disparity=alignment == "least_square_disparity")
            if (h, w) == (480, 640):
                mask = nyu_crop(mask)
            if (h, w) == (37, 53):
                plant_two_pixel_image(pred, gt, mask, 2)
            worst = max(worst, check_against_host(pred, gt, mask, alignment, None, lo, hi))
            if (h, w) == (37, 53) and alignment:  # the column-subsampled fit (alignment_max_res): 20 of 53 columns, every row
                worst = max(worst, check_against_host(pred, gt, mask, alignment, 20, lo, hi))
    metric_log(f"eval_depth_vs_host[{b}x{h}x{w}]", worst_rel=worst)


@gpu
def test_eval_depth_too_few_fit_pixels_raises():
    from genpercept_amd import engine as ge
    d = torch.device("cuda", 0)
    pred, gt, mask = make_case(3, 37, 53, 5, 10.0)
    mask[1] = False
    mask[1, 3, 4] = True  # one fit pixel
    args = [torch.from_numpy(x).to(d) for x in (pred, gt, mask)]
    for alignment in ("least_square", "least_square_disparity"):
        with pytest.raises(ValueError):
            ge.eval_depth(*args, alignment, None, 1e-3, 10.0)
    mask[1, 9, 9] = True  # two fit pixels with one pred value: singular
    pred[1, 9, 9] = pred[1, 3, 4]
    with pytest.raises(ValueError):
        ge.eval_depth(torch.from_numpy(pred).to(d), args[1], torch.from_numpy(mask).to(d), "least_square", None, 1e-3, 10.0)
    metrics, (s, t, n_valid) = ge.eval_depth(*args, None, None, 1e-3, 10.0)  # without alignment there is nothing to fit
    assert n_valid[1] == 1 and s[1] == 1.0 and t[1] == 0.0 and np.isfinite(metrics[1]["abs_relative_difference"])


@gpu
def test_eval_depth_is_deterministic_and_batch_independent():
    """Two calls: bit-identical float64 outputs.  Image i inside a batch of 3 == the same image alone (a slice of the batch: other base
    addresses, so the scalar-load path when H * W is odd -- same values, same order), bit for bit."""
    from genpercept_amd import engine as ge
    d = torch.device("cuda", 0)
    for h, w, max_res in ((37, 53, None), (37, 53, 20), (300, 412, None), (1031, 2053, None)):
        pred, gt, mask = make_case(3, h, w, 7 + h, 10.0)
        tp, tg, tm = (torch.from_numpy(x).to(d) for x in (pred, gt, mask))
        for alignment in ("least_square", "least_square_disparity", None):
            a = ge.eval_depth_raw(tp, tg, tm, alignment, max_res, 1e-3, 10.0).cpu()
            b = ge.eval_depth_raw(tp, tg, tm, alignment, max_res, 1e-3, 10.0).cpu()
            assert torch.isfinite(a[:, 2:]).all() and torch.equal(a, b)
            for i in range(3):
                alone = ge.eval_depth_raw(tp[i:i + 1], tg[i:i + 1], tm[i:i + 1], alignment, max_res, 1e-3, 10.0).cpu()
                assert torch.equal(alone[0], a[i]), (h, w, alignment, i, alone[0], a[i])
                copy = ge.eval_depth_raw(tp[i].clone(), tg[i].clone(), tm[i].clone(), alignment, max_res, 1e-3, 10.0).cpu()
                assert torch.equal(copy[0], a[i]), (h, w, alignment, i)


@pytest.fixture(scope="module")
def tiny_weights():
    from oracle import dpt as odpt
    from oracle import sd21 as osd
    uc, vc, dc = osd.UNetCfg.tiny(), osd.VAECfg.tiny(), odpt.DPTCfg.tiny()
    return dict(uc=uc, vc=vc, dc=dc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2),
                dsd=osd.synth_state_dict(odpt.dpt_manifest(dc), 3))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32c"])
def test_infer_and_evaluate_with_the_pipeline(precision, tiny_weights, tmp_path, metric_log):
    """The device loop on a ScanNet-style tree (png / 1000, no crop, `id` naming): three 96 x 128 images and one 64 x 64, batch_size 2.  Its
    means == host evaluate_predictions on the maps it saved (delta exactly, the others to 1e-9 relative: same (s, t) bit for bit, float64
    summation order), and every saved map agrees with the same image run alone through pipe(...) to 2 x the map_mean tolerance of
    tests/test_e2e_gpu.py (bf16 8.4e-3, fp32c 5e-5: other batch sizes pick other tiles / split-K factors, the accumulation order differs)."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    map_mean = {"bf16": 8.4e-3, "fp32c": 5e-5}[precision]
    tw = tiny_weights
    g = torch.Generator().manual_seed(41)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype={"bf16": torch.bfloat16, "fp32c": torch.float32}[precision])
    pipe.to("cuda")
    base, out = str(tmp_path / "data"), str(tmp_path / "out")
    rng = np.random.RandomState(3)
    samples = []
    for i, (h, w) in enumerate([(96, 128), (96, 128), (96, 128), (64, 64)]):
        os.makedirs(os.path.join(base, "scene0000_00", "color"), exist_ok=True)
        os.makedirs(os.path.join(base, "scene0000_00", "depth"), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "scene0000_00", "color", f"{i:06d}.png"))
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        depth_m = 0.8 + 7.0 * (0.5 + 0.4 * np.sin(4 * xx + i) * np.cos(3 * yy)) + 0.3 * rng.rand(h, w)  # inside (1e-3, 10)
        Image.fromarray(np.round(depth_m * 1000).astype(np.uint16)).save(os.path.join(base, "scene0000_00", "depth", f"{i:06d}.png"))
        samples.append([f"scene0000_00/color/{i:06d}.png", f"scene0000_00/depth/{i:06d}.png"])
    try:
        res = ie.infer_and_evaluate(pipe, base, samples, "scannet", output_dir=out, batch_size=2, save_predictions=True, mode="depth", processing_res=0)
        ref = ie.evaluate_predictions(out, base, samples, dataset="scannet", alignment="least_square")
        for k in ref:
            err = abs(res[k] - ref[k]) / abs(ref[k])
            print(f"infer_and_evaluate[{precision}] {k}: device {res[k]!r} host {ref[k]!r} rel {err:.3e}")
            metric_log(f"infer_and_evaluate[{precision}] {k}", device=res[k], host=ref[k])
            assert np.isfinite(res[k])
            if k.startswith("delta"):
                assert res[k] == ref[k], (k, res[k], ref[k])
            else:
                assert abs(res[k] - ref[k]) <= 1e-9 * abs(ref[k]), (k, res[k], ref[k])
        for name in ("eval_metrics-least_square.txt", "per_sample_metrics-least_square.csv"):
            assert os.path.exists(os.path.join(out, name))
        for s, (h, w) in zip(samples, [(96, 128)] * 3 + [(64, 64)]):
            saved = np.load(os.path.join(out, os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy")))
            alone = pipe(Image.open(os.path.join(base, s[0])), processing_res=0, mode="depth", color_map=None, show_progress_bar=False).pred_np
            assert saved.shape == alone.shape == (h, w) and saved.dtype == np.float32
            diff = float(np.abs(saved - alone).mean())
            print(f"infer_and_evaluate[{precision}] {s[0]}: mean |batched - alone| = {diff:.3e}")
            assert diff <= 2 * map_mean, (s[0], diff)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
