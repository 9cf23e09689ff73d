"""Surface-normal evaluation on the device (gp_eval_normal, csrc/eval.hip; engine.eval_normal) against the project's host evaluation
(eval_metrics.normal_angular_error, the reference's angular_loss in float64 plus summary statistics), and the batched device loop
`infer_eval.infer_and_evaluate_normals` with the real pipeline at tiny widths.

Inputs come from a seed: gt = random unit vectors with planted all-zero pixels; pred = gt rotated by a smooth random angle field, plus noise,
kept signed and in the pipeline's [0, 1] encoding; a random explicit mask.  The host side is always normal_angular_error on the same arrays;
`host_angles` below restates its per-pixel part (the function returns statistics only) and every check first ties it to the function.

Bounds.
  n_valid      exact, with an explicit mask and with mask None (any stored gt channel != 0).
  angles_out   within 5 float64 ulp of the host's arccos at valid pixels, NaN elsewhere: the argument of acos is bit-identical by construction
               (products, sums, division, sqrt are correctly rounded on both sides, no FMA), the device library's double acos is specified
               to 4 ulp, 1 for the host libm.  Largest difference seen on an MI355X: see `test_eval_normal_matches_host`.
  median_deg   BIT-EQUAL to np.median(angles_dev[valid] * (180 / pi)) -- the selection is exact -- and within 6 ulp of the host's own median
               (an order statistic moves no more than the values; one more rounding for the average).
  within_*     exactly the host's, under a precondition asserted ON THE HOST VALUES: no host angle within 1e-9 degrees of a threshold, so a
               last-bit acos difference cannot move a count.
  mean_rad, mean_deg, rmse_deg   relative 1e-9: float64 sums of at most 2.1e6 non-negative terms in another order (n * 2^-53 = 2.4e-10), the
               bound tests/test_eval_device_gpu.py derives, plus the 5-ulp acos differences (5.6e-16 each).
"""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

TO_DEG = 180.0 / np.pi
THRESHOLDS = (11.25, 22.5, 30.0)
NAMES = ["mean_rad", "mean_deg", "median_deg", "rmse_deg", "within_11.25", "within_22.5", "within_30"]
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (3, 64, 65), (1, 1031, 2053)]  # n = 1; even median; tail quads + unaligned planes; 2 workgroups; the cap


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_case(b, h, w, seed):
    """(pred signed, pred encoded, gt, mask), float32 [b, 3, h, w] and bool [b, h, w].  In a batch, image 0 has an odd and image 1 an even
    number of valid pixels under both validity rules.  Images of four pixels or fewer keep every pixel valid."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    gt = _unit(rng.randn(b, 3, h, w))
    theta = np.stack([0.35 + 0.3 * np.sin(3.1 * xx + 0.7 * i) * np.cos(2.3 * yy - 0.4 * i) for i in range(b)])[:, None]  # 3 .. 37 degrees
    side = _unit(np.cross(gt, _unit(rng.randn(b, 3, h, w)), axis=1))
    pred = _unit(gt * np.cos(theta) + side * np.sin(theta) + 0.05 * rng.randn(b, 3, h, w)) * (0.5 + rng.rand(b, 1, h, w))
    pred = np.clip(pred, -1.0, 1.0)
    gt = gt.astype(np.float32)
    mask = np.ones((b, h, w), dtype=bool)
    if h * w > 4:
        gt = gt * (rng.rand(b, 1, h, w) >= 0.05)
        mask = rng.rand(b, h, w) < 0.7
        for i in range(min(b, 2)):  # parities: image 0 odd, image 1 even
            want = 1 - i
            nz = (gt[i] != 0).any(axis=0)
            if nz.sum() % 2 != want:
                y, x = np.argwhere(nz)[0]
                gt[i, :, y, x] = 0.0
            if mask[i].sum() % 2 != want:
                y, x = np.argwhere(mask[i])[0]
                mask[i, y, x] = False
    gt = np.ascontiguousarray(gt, dtype=np.float32)
    pred = pred.astype(np.float32)
    enc = ((pred.astype(np.float64) + 1.0) / 2.0).astype(np.float32)
    return pred, enc, gt, mask


_CASES = {}


def case(shape):
    """One input set and one host evaluation per shape, shared by the tests and left unchanged."""
    if shape not in _CASES:
        pred, enc, gt, mask = make_case(*shape, seed=1000 + shape[1])
        for a in (pred, enc, gt, mask):
            a.setflags(write=False)
        _CASES[shape] = (pred, enc, gt, mask)
    return _CASES[shape]


def host_angles(p64, gt):
    """The per-pixel part of eval_metrics.normal_angular_error, [H, W] radians for one image (p64: float64 [3, H, W], decoded)."""
    g = gt.astype(np.float64)
    num = (p64 * g).sum(axis=-3)
    den = np.maximum(np.linalg.norm(p64, axis=-3), 1e-8) * np.maximum(np.linalg.norm(g, axis=-3), 1e-8)
    return np.arccos(np.clip(num / den, -1.0 + 1e-4, 1.0 - 1e-4))


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def dev(*arrays):
    d = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.array(a)).to(d) for a in arrays]  # (a copy: the shared arrays are read-only)


def check_against_host(pred, gt, mask, encoded, tag):
    """All bounds of the module docstring for one call; returns (largest angle difference in ulp, largest relative difference of the sums)."""
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    tp, tg, tm = dev(pred, gt, mask)
    raw, ang = ge.eval_normal_raw(tp, tg, tm, pred_encoded=encoded, gt_encoded=False, want_angles=True)
    metrics, n_valid = ge.eval_normal(tp, tg, tm, pred_encoded=encoded, gt_encoded=False)
    raw, ang = raw.cpu().numpy(), ang.cpu().numpy()
    assert raw.shape == (pred.shape[0], 8) and ang.shape == (pred.shape[0],) + pred.shape[-2:] and ang.dtype == np.float64
    worst_ulp, worst_rel = 0.0, 0.0
    for i in range(pred.shape[0]):
        p64 = pred[i].astype(np.float64) * 2.0 - 1.0 if encoded else pred[i].astype(np.float64)
        valid = mask[i] if mask is not None else (gt[i] != 0).any(axis=0)
        ref = em.normal_angular_error(p64, gt[i], valid)
        ha = host_angles(p64, gt[i])
        hv = ha[valid]
        assert ref["mean_rad"] == float(hv.mean()) and ref["median_deg"] == float(np.median(np.degrees(hv)))  # the helper IS the function
        assert raw[i, 0] == valid.sum() == n_valid[i], (tag, i, raw[i, 0], valid.sum())
        # angles
        assert np.isnan(ang[i][~valid]).all() and not np.isnan(ang[i][valid]).any(), (tag, i)
        dv = ang[i][valid]
        u = float(ulps(dv, hv).max())
        worst_ulp = max(worst_ulp, u)
        print(f"eval_normal {tag} image {i}: n {int(raw[i, 0])}  max |angle dev - host| = {u:.2f} ulp")
        assert u <= 5.0, (tag, i, u)
        # median: exact selection of the device's own angles; near the host's
        med = raw[i, 3]
        assert med == float(np.median(dv * TO_DEG)), (tag, i, med, float(np.median(dv * TO_DEG)))
        assert ulps(med, ref["median_deg"]) <= 6.0, (tag, i, med, ref["median_deg"])
        # fractions: exact, given that no host angle sits on a threshold
        hd = np.degrees(hv)
        gap = min(float(np.abs(hd - t).min()) for t in THRESHOLDS)
        print(f"    nearest host angle to a threshold: {gap:.3e} degrees")
        assert gap > 1e-9, (tag, i, gap)
        for j, k in enumerate(NAMES):
            d = raw[i, 1 + j]
            assert metrics[i][k] == d
            if k.startswith("within"):
                assert d == ref[k], (tag, i, k, d, ref[k])
            elif k != "median_deg":
                rel = abs(d - ref[k]) / abs(ref[k])
                worst_rel = max(worst_rel, rel)
                print(f"    {k}: dev {d!r} host {ref[k]!r} rel {rel:.3e}")
                assert rel <= 1e-9, (tag, i, k, d, ref[k])
    return worst_ulp, worst_rel


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_normal_matches_host(shape, metric_log):
    """Explicit mask and derived mask, encoded and signed predictions.  Largest differences measured once on one MI355X are recorded in
    DESIGN.md section 4 (angles: at most 1 ulp of the host's arccos over all shapes of this file)."""
    pred, enc, gt, mask = case(shape)
    if shape == (3, 64, 65):
        for m in (mask, (gt != 0).any(axis=1)):
            assert m[0].sum() % 2 == 1 and m[1].sum() % 2 == 0
    worst_ulp, worst_rel = 0.0, 0.0
    for p, encoded, m in ((enc, True, mask), (enc, True, None), (pred, False, None)):
        u, r = check_against_host(p, gt, m, encoded, (shape, encoded, m is not None))
        worst_ulp, worst_rel = max(worst_ulp, u), max(worst_rel, r)
    metric_log("eval_normal_vs_host[%dx%dx%d]" % shape, angle_ulp=worst_ulp, worst_rel=worst_rel)


@gpu
def test_eval_normal_unaligned_views():
    """The (3, 64, 65) tensors again as views one element into an allocation: every plane takes the scalar-load path, the mask the byte path.
    Same pixels, same order: bit-identical to the aligned call, and the bounds hold."""
    from genpercept_amd import engine as ge
    pred, enc, gt, mask = case((3, 64, 65))
    d = torch.device("cuda", 0)

    def shifted(a):
        t = torch.from_numpy(np.array(a))
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=d)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 or t.element_size() == 1
        return v

    te, tg, tm = shifted(enc), shifted(gt), shifted(mask)
    ae, ag, am = dev(enc, gt, mask)
    for m_s, m_a in ((tm, am), (None, None)):
        r_s, a_s = ge.eval_normal_raw(te, tg, m_s, want_angles=True)
        r_a, a_a = ge.eval_normal_raw(ae, ag, m_a, want_angles=True)
        assert torch.equal(r_s, r_a) and torch.equal(a_s.view(torch.int64), a_a.view(torch.int64))


def _ties_case(h, w, odd):
    """gt: unit vectors, every pixel valid but a few planted zeros; the valid count is made odd or even."""
    rng = np.random.RandomState(5 + int(odd))
    gt = _unit(rng.randn(1, 3, h, w)).astype(np.float32)
    gt = gt * (rng.rand(1, 1, h, w) >= 0.05)
    valid = (gt[0] != 0).any(axis=0)
    if valid.sum() % 2 != int(odd):
        y, x = np.argwhere(valid)[0]
        gt[0, :, y, x] = 0.0
    return np.ascontiguousarray(gt, dtype=np.float32), (gt[0] != 0).any(axis=0)


@gpu
def test_eval_normal_ties():
    """Whole images of one repeated angle, and two tie groups that the median's two ranks straddle."""
    from genpercept_amd import engine as ge
    lo_ang, hi_ang = float(np.arccos(1.0 - 1e-4)), float(np.arccos(-1.0 + 1e-4))
    for odd in (False, True):
        gt, valid = _ties_case(64, 65, odd)
        n = int(valid.sum())
        assert n % 2 == int(odd)
        (tg,) = dev(gt)
        for sign, want, frac in ((1.0, lo_ang, 1.0), (-1.0, hi_ang, 0.0)):  # pred == gt: the upper clamp; pred == -gt: the lower clamp
            raw, ang = ge.eval_normal_raw(tg * sign, tg, None, pred_encoded=False, want_angles=True)
            raw, ang = raw.cpu().numpy()[0], ang.cpu().numpy()[0]
            dv = ang[valid]
            assert raw[0] == n and (dv == dv[0]).all() and ulps(dv[0], want) <= 5.0
            assert raw[3] == dv[0] * TO_DEG                                   # the median of n equal values is that value, exactly
            assert abs(raw[1] - want) <= 1e-9 * want and abs(raw[2] - want * TO_DEG) <= 1e-9 * want * TO_DEG
            assert abs(raw[4] - want * TO_DEG) <= 1e-9 * want * TO_DEG
            assert tuple(raw[5:8]) == (frac, frac, frac)
        # half of the valid pixels with a zero prediction (num = 0: exactly acos(0)), the others equal to gt
        pred = gt.copy()
        idx = np.argwhere(valid)
        half = idx[: n // 2] if not odd else idx[: n // 2 + 1]               # odd: the larger group is the zero one, the median falls in it
        pred[0][:, half[:, 0], half[:, 1]] = 0.0
        (tp,) = dev(pred)
        raw, ang = ge.eval_normal_raw(tp, tg, None, pred_encoded=False, want_angles=True)
        raw, ang = raw.cpu().numpy()[0], ang.cpu().numpy()[0]
        dv = ang[valid]
        small, big = dv.min(), dv.max()
        assert set(np.unique(dv)) == {small, big} and ulps(small, lo_ang) <= 5.0 and ulps(big, np.pi / 2) <= 5.0
        assert (dv == big).sum() == len(half) and raw[0] == n
        expect = (small * TO_DEG + big * TO_DEG) / 2.0 if not odd else big * TO_DEG
        assert raw[3] == expect == float(np.median(dv * TO_DEG)), (odd, raw[3], expect)
        assert raw[5] == raw[6] == raw[7] == (n - len(half)) / n


@gpu
def test_eval_normal_is_deterministic_and_batch_independent():
    """Two calls: bit-identical outputs.  Image i of the batch of 3 alone (a slice: another base address; a clone: an aligned one) == the same
    image inside the batch, bit for bit."""
    from genpercept_amd import engine as ge
    pred, enc, gt, mask = case((3, 64, 65))
    te, tg, tm = dev(enc, gt, mask)
    for m in (tm, None):
        a, aa = ge.eval_normal_raw(te, tg, m, want_angles=True)
        b, ba = ge.eval_normal_raw(te, tg, m, want_angles=True)
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(aa.view(torch.int64), ba.view(torch.int64))
        for i in range(3):
            mi = None if m is None else m[i:i + 1]
            alone = ge.eval_normal_raw(te[i:i + 1], tg[i:i + 1], mi)
            assert torch.equal(alone[0], a[i]), (i, alone[0], a[i])
            copy = ge.eval_normal_raw(te[i].clone(), tg[i].clone(), None if m is None else m[i].clone())
            assert torch.equal(copy[0], a[i]), i


@gpu
def test_eval_normal_empty_image_in_a_batch():
    from genpercept_amd import engine as ge
    pred, enc, gt, mask = case((3, 64, 65))
    gt2 = gt.copy()
    gt2[1] = 0.0  # no valid pixel under the derived rule
    te, tg, tg2 = dev(enc, gt, gt2)
    full = ge.eval_normal_raw(te, tg, None).cpu()
    raw, ang = ge.eval_normal_raw(te, tg2, None, want_angles=True)
    raw, ang = raw.cpu(), ang.cpu()
    assert raw[1, 0] == 0 and torch.isnan(raw[1, 1:]).all() and torch.isnan(ang[1]).all()
    assert torch.equal(raw[0], full[0]) and torch.equal(raw[2], full[2])
    with pytest.raises(ValueError, match="image 1"):
        ge.eval_normal(te, tg2, None)
    mask2 = mask.copy()
    mask2[2] = False  # and with an explicit mask
    (tm2,) = dev(mask2)
    raw = ge.eval_normal_raw(te, tg, tm2).cpu()
    assert raw[2, 0] == 0 and torch.isnan(raw[2, 1:]).all() and torch.isfinite(raw[:2]).all()
    with pytest.raises(ValueError, match="image 2"):
        ge.eval_normal(te, tg, tm2)


@pytest.fixture(scope="module")
def tiny_weights():
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    return dict(uc=uc, vc=vc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32c"])
def test_infer_and_evaluate_normals_with_the_pipeline(precision, tiny_weights, tmp_path, metric_log):
    """The device loop on a tree with `.npy` normals in column 3: three 96 x 128 images and one 64 x 64, batch_size 2.  Its means ==
    host evaluate_normal_predictions on the maps it saved: fractions exactly, the others to 1e-9 relative."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(43)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype={"bf16": torch.bfloat16, "fp32c": torch.float32}[precision])
    pipe.to("cuda")
    base, out = str(tmp_path / "data"), str(tmp_path / "out")
    rng = np.random.RandomState(4)
    samples, sizes = [], [(96, 128), (96, 128), (96, 128), (64, 64)]
    for i, (h, w) in enumerate(sizes):
        for sub in ("color", "normal"):
            os.makedirs(os.path.join(base, "scene0000_00", sub), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "scene0000_00", "color", f"{i:06d}.png"))
        n = rng.randn(h, w, 3).astype(np.float32)
        n[rng.rand(h, w) < 0.1] = 0.0
        np.save(os.path.join(base, "scene0000_00", "normal", f"{i:06d}.npy"), n)
        samples.append([f"scene0000_00/color/{i:06d}.png", f"scene0000_00/depth/{i:06d}.png", "None", f"scene0000_00/normal/{i:06d}.npy"])
    try:
        res = ie.infer_and_evaluate_normals(pipe, base, samples, output_dir=out, batch_size=2, save_predictions=True, processing_res=0)
        ref = ie.evaluate_normal_predictions(out, base, samples, ie.FileNameMode.id)
        assert list(res) == NAMES
        for k in ref:
            err = abs(res[k] - ref[k]) / abs(ref[k]) if ref[k] != 0 else abs(res[k])
            print(f"infer_and_evaluate_normals[{precision}] {k}: device {res[k]!r} host {ref[k]!r} rel {err:.3e}")
            metric_log(f"infer_and_evaluate_normals[{precision}] {k}", device=res[k], host=ref[k])
            assert np.isfinite(res[k])
            if k.startswith("within"):
                assert res[k] == ref[k], (k, res[k], ref[k])
            else:
                assert abs(res[k] - ref[k]) <= 1e-9 * abs(ref[k]), (k, res[k], ref[k])
        for name in ("eval_metrics-normal.txt", "per_sample_metrics-normal.csv"):
            assert os.path.exists(os.path.join(out, name))
        for s, (h, w) in zip(samples, sizes):
            saved = np.load(os.path.join(out, os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy")))
            assert saved.shape == (h, w, 3) and saved.dtype == np.float32 and saved.min() >= 0.0 and saved.max() <= 1.0
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
