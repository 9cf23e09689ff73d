"""Dis / matting evaluation on the device (gp_eval_mask, csrc/eval.hip; engine.eval_mask) against the host route
(eval_metrics.mask_counts / mask_metrics_from_counts / mask_metrics), and the batched device loop `infer_eval.infer_and_evaluate_masks` with
the real pipeline at tiny widths.

No tolerance anywhere.  The counts are integers: `counts_out` must equal mask_counts of the host's quantisation of the same floats.  The ten
values are one prescribed sequence of correctly rounded float64 operations on those integers: `out` must equal, bit for bit,
mask_metrics_from_counts of the device's own counts and mask_metrics of the host arrays (NaN matches NaN).

Inputs come from a seed.  Mask-like: about 90 % of the pixels exactly 0.0 / 1.0 against a 0 / 255 ground truth -- the ballot path -- with a
soft band between them -- the atomic path, in the same waves; the band holds random floats, exact k / 255 and their float32 neighbours, values
outside [0, 1] and NaN."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (3, 64, 65), (1, 1031, 2053)]  # n = 1; the scalar tail; unaligned planes in a batch, two workgroups; many slabs
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]


def make_case(b, h, w, seed):
    """(pred float32, gt uint8, region bool), [b, h, w]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    edge = np.stack([0.35 + 0.2 * np.sin(2.0 * yy + i) for i in range(b)])                     # the object is right of a wavy edge
    dist = xx[None] - edge
    gt = np.where(dist > 0.02, 255, np.where(dist < -0.02, 0, np.clip((dist + 0.02) / 0.04 * 255, 0, 255))).astype(np.uint8)
    k = rng.randint(0, 256, (b, h, w)).astype(np.float32) / np.float32(255.0)
    soft = np.choose(rng.randint(0, 4, (b, h, w)), [rng.rand(b, h, w).astype(np.float32), k, np.nextafter(k, np.float32(-1.0)),
                                                    np.nextafter(k, np.float32(2.0))]).astype(np.float32)
    hard = ((dist + 0.03 * rng.randn(b, h, w)) > 0).astype(np.float32)                         # exactly 0.0 / 1.0, a noisy boundary
    pred = np.where(rng.rand(b, h, w) < 0.9, hard, soft).astype(np.float32)
    if h * w > 4:
        odd = rng.rand(b, h, w)
        pred[odd < 0.004] = np.nan
        pred[(odd > 0.004) & (odd < 0.008)] = -0.25
        pred[(odd > 0.008) & (odd < 0.012)] = 1.5
    region = rng.rand(b, h, w) < 0.6
    return pred, gt, region


_CASES = {}


def case(shape):
    """One input set and one host evaluation per shape, shared by the tests and left unchanged: (pred, gt, region, q, {use_region: (counts, rows)})."""
    from genpercept_amd import eval_metrics as em
    if shape not in _CASES:
        pred, gt, region = make_case(*shape, seed=2000 + shape[1])
        q = em.quantize_mask(pred)
        host = {}
        for use_region in (False, True):
            counts = np.stack([em.mask_counts(q[i], gt[i], region[i] if use_region else None) for i in range(shape[0])])
            host[use_region] = (counts, np.stack([row_of(em.mask_metrics_from_counts(c)) for c in counts]))
        for a in (pred, gt, region, q, *host[False], *host[True]):
            a.setflags(write=False)
        _CASES[shape] = (pred, gt, region, q, host)
    return _CASES[shape]


def row_of(m):
    """mask_metrics_from_counts' dict as gp_eval_mask's out row."""
    assert list(m) == ["n", "n_fg"] + MASK_METRICS + ["t_max"]
    return np.array([float(v) for v in m.values()], dtype=np.float64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def dev(*arrays):
    d = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.array(a)).to(d) for a in arrays]  # (a copy: the shared arrays are read-only)


def check_against_host(tp, tg, tr, want_counts, want_rows, tag):
    """counts_out == the host's counts; out == mask_metrics_from_counts(device counts) == the host's rows, bit for bit."""
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    raw, counts = ge.eval_mask_raw(tp, tg, tr, want_counts=True)
    alone = ge.eval_mask_raw(tp, tg, tr)
    raw, counts, alone = raw.cpu().numpy(), counts.cpu().numpy(), alone.cpu().numpy()
    b = want_counts.shape[0]
    assert raw.shape == (b, 10) and raw.dtype == np.float64 and counts.shape == (b, 516) and counts.dtype == np.int64
    for i in range(b):
        bad = np.flatnonzero(counts[i] != want_counts[i])
        print(f"eval_mask {tag} image {i}: n {counts[i, 0]} sum_q {counts[i, 1]} sad {counts[i, 2]} sse {counts[i, 3]}  bins 0 / 255: "
              f"{counts[i, 4] + counts[i, 260]} / {counts[i, 259] + counts[i, 515]}  counts differing from the host: {bad.size}")
        assert bad.size == 0, (tag, i, bad[:8], counts[i][bad[:8]], want_counts[i][bad[:8]])
        own = row_of(em.mask_metrics_from_counts(counts[i]))
        print(f"    out {raw[i].tolist()}")
        assert same_bits(raw[i], own), (tag, i, raw[i], own)
        assert same_bits(raw[i], want_rows[i]), (tag, i, raw[i], want_rows[i])
    assert same_bits(alone, raw)  # with and without counts_out
    return raw, counts


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_mask_matches_host_on_mask_like_input(shape):
    from genpercept_amd import eval_metrics as em
    pred, gt, region, q, host = case(shape)
    if shape[1] * shape[2] > 1000:
        sat = float(((q == 0) | (q == 255)).mean())
        assert 0.85 < sat < 0.97 and ((q > 0) & (q < 255)).sum() > 100, sat   # both paths are driven
    tp, tg, tr = dev(pred, gt, region)
    for use_region in (False, True):
        check_against_host(tp, tg, tr if use_region else None, *host[use_region], (shape, use_region))
    for i in range(shape[0]):  # the stored rows ARE mask_metrics of the host arrays
        assert same_bits(host[True][1][i], row_of(em.mask_metrics(pred[i], gt[i], region[i])))


@gpu
@pytest.mark.parametrize("shape", [(3, 64, 65), (1, 1031, 2053)], ids=lambda s: "x".join(map(str, s)))
def test_eval_mask_uniform_random(shape):
    """Uniform-random floats and bytes: nearly every lane of every wave takes the atomic path."""
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(7 + shape[1])
    pred = rng.rand(*shape).astype(np.float32)
    gt = rng.randint(0, 256, shape).astype(np.uint8)
    q8 = rng.randint(0, 256, shape).astype(np.uint8)
    region = rng.rand(*shape) < 0.5
    tp, tg, tq, tr = dev(pred, gt, q8, region)
    for p_host, p_dev, tag in ((em.quantize_mask(pred), tp, "float"), (q8, tq, "uint8")):
        for r_host, r_dev in ((None, None), (region, tr)):
            counts = np.stack([em.mask_counts(p_host[i], gt[i], None if r_host is None else r_host[i]) for i in range(shape[0])])
            rows = np.stack([row_of(em.mask_metrics_from_counts(c)) for c in counts])
            check_against_host(p_dev, tg, r_dev, counts, rows, (shape, tag, r_host is not None))


@gpu
def test_eval_mask_on_the_bytes_postprocess_writes():
    """pred_is_u8 = 1 fed with gp_postprocess's own 8-bit image == the float route on the map it was made from."""
    from genpercept_amd import engine as ge
    pred, gt, region, q, host = case((3, 64, 65))
    clean = np.where(np.isnan(pred), np.float32(0.25), pred)          # (the pipeline's maps hold no NaN)
    tp, tg, tr = dev(clean, gt, region)
    out, _, q8 = ge.postprocess(tp[:, None], (64, 65), "bilinear", q_bits=8)
    assert q8.dtype == torch.uint8 and tuple(q8.shape) == (3, 1, 64, 65)
    for r in (None, tr):
        a, ca = ge.eval_mask_raw(q8, tg, r, want_counts=True)        # [B, 1, H, W] is accepted
        b, cb = ge.eval_mask_raw(tp, tg, r, want_counts=True)         # the unclipped floats: the kernel clips
        c, cc = ge.eval_mask_raw(out[:, 0], tg, r, want_counts=True)
        assert torch.equal(ca, cb) and torch.equal(ca, cc)
        assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and same_bits(a.cpu().numpy(), c.cpu().numpy())


@gpu
def test_eval_mask_unaligned_views():
    """The (3, 64, 65) tensors again as views one element into an allocation.  All three shifted: the planes share a head of three pixels and
    keep the vector loads.  Only one shifted: no common head, every pixel goes the scalar way.  Same counts either way."""
    from genpercept_amd import engine as ge
    pred, gt, region, q, host = case((3, 64, 65))
    d = torch.device("cuda", 0)

    def shifted(a):
        t = torch.from_numpy(np.array(a))
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=d)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    ap, ag, ar, aq = dev(pred, gt, region, q)
    sp, sg, sr, sq = shifted(pred), shifted(gt), shifted(region), shifted(q)
    want = {use: [x.cpu() for x in ge.eval_mask_raw(ap, ag, ar if use else None, want_counts=True)] for use in (False, True)}
    for use in (False, True):
        assert np.array_equal(want[use][1].numpy(), host[use][0])
        for p, g, r in ((sp, sg, sr), (sp, ag, ar), (ap, sg, ar), (ap, ag, sr), (sq, sg, sr), (sq, ag, ar), (aq, sg, sr)):
            if not use and r is sr and p is ap and g is ag:
                continue
            raw, counts = ge.eval_mask_raw(p, g, r if use else None, want_counts=True)
            assert torch.equal(counts.cpu(), want[use][1]) and same_bits(raw.cpu().numpy(), want[use][0].numpy())


@gpu
def test_eval_mask_is_stable_and_batch_independent():
    """Two calls: identical.  Image i alone (a slice: another base address; a clone: an aligned one) == the same image inside the batch of 3.
    An image with an empty region inside a batch: n = n_fg = 0 and NaN for it, its neighbours unchanged; engine.eval_mask names it."""
    from genpercept_amd import engine as ge
    pred, gt, region, q, host = case((3, 64, 65))
    tp, tg, tr = dev(pred, gt, region)
    for r in (None, tr):
        a, ca = ge.eval_mask_raw(tp, tg, r, want_counts=True)
        b, cb = ge.eval_mask_raw(tp, tg, r, want_counts=True)
        assert torch.isfinite(a).all() and same_bits(a.cpu().numpy(), b.cpu().numpy()) and torch.equal(ca, cb)
        for i in range(3):
            ri = None if r is None else r[i:i + 1]
            alone, c1 = ge.eval_mask_raw(tp[i:i + 1], tg[i:i + 1], ri, want_counts=True)
            assert same_bits(alone[0].cpu().numpy(), a[i].cpu().numpy()) and torch.equal(c1[0], ca[i]), i
            copy = ge.eval_mask_raw(tp[i].clone(), tg[i].clone(), None if r is None else r[i].clone())
            assert same_bits(copy[0].cpu().numpy(), a[i].cpu().numpy()), i
    region2 = region.copy()
    region2[1] = False
    (tr2,) = dev(region2)
    full = ge.eval_mask_raw(tp, tg, tr).cpu().numpy()
    raw, counts = ge.eval_mask_raw(tp, tg, tr2, want_counts=True)
    raw, counts = raw.cpu().numpy(), counts.cpu().numpy()
    assert raw[1, 0] == 0 and raw[1, 1] == 0 and np.isnan(raw[1, 2:]).all() and (counts[1] == 0).all()
    assert same_bits(raw[0], full[0]) and same_bits(raw[2], full[2])
    with pytest.raises(ValueError, match="image 1"):
        ge.eval_mask(tp, tg, tr2)
    res = ge.eval_mask(tp, tg, tr)
    assert len(res) == 3
    for i, m in enumerate(res):
        assert list(m)[:7] == MASK_METRICS and same_bits([m[k] for k in MASK_METRICS], host[True][1][i, 2:9])
        assert m["n"] == host[True][0][i, 0] and m["t_max"] == host[True][1][i, 9] and np.array_equal(m["counts"], host[True][0][i])


@pytest.fixture(scope="module")
def tiny_weights():
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    return dict(uc=uc, vc=vc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32c"])
def test_infer_and_evaluate_masks_with_the_pipeline(precision, tiny_weights, tmp_path):
    """The device loop for mode "dis" on a tree of 8-bit masks: three 96 x 128 images and one 64 x 64, batch_size 2.  Its table and its
    values == host evaluate_mask_predictions over the `.npy` maps it saved, bit for bit."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(47)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype={"bf16": torch.bfloat16, "fp32c": torch.float32}[precision])
    pipe.to("cuda")
    base, out, ref_dir = str(tmp_path / "data"), str(tmp_path / "out"), str(tmp_path / "ref")
    samples, sizes = [], [(96, 128), (96, 128), (96, 128), (64, 64)]
    for i, (h, w) in enumerate(sizes):
        for sub in ("im", "gt"):
            os.makedirs(os.path.join(base, "set0", sub), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "set0", "im", f"{i:04d}.png"))
        xx = np.arange(w)[None].repeat(h, 0)
        Image.fromarray(np.clip((xx - (w // 3 + 10 * i)) * 40 + 128, 0, 255).astype(np.uint8)).save(os.path.join(base, "set0", "gt", f"{i:04d}.png"))
        samples.append([f"set0/im/{i:04d}.png", f"set0/gt/{i:04d}.png"])
    try:
        res = ie.infer_and_evaluate_masks(pipe, base, samples, "dis", output_dir=out, batch_size=2, save_predictions=True, processing_res=0)
        ref = ie.evaluate_mask_predictions(out, base, samples, ie.FileNameMode.id, output_dir=ref_dir)
        for k in ref:
            print(f"infer_and_evaluate_masks[{precision}] {k}: device {res[k]!r} host {ref[k]!r}")
        assert list(res) == MASK_METRICS + ["max_f_dataset"] and all(np.isfinite(v) for v in res.values())
        assert res == ref
        name = "per_sample_metrics-mask.csv"
        rows = open(os.path.join(out, name)).read()
        assert rows == open(os.path.join(ref_dir, name)).read() and len(rows.splitlines()) == 1 + len(samples)
        assert os.path.exists(os.path.join(out, "eval_metrics-mask.txt"))
        for s, (h, w) in zip(samples, sizes):
            saved = np.load(os.path.join(out, os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy")))
            assert saved.shape == (h, w) and saved.dtype == np.float32 and saved.min() >= 0.0 and saved.max() <= 1.0
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
