"""Seg evaluation on the device (gp_seg_decode / gp_eval_seg, csrc/eval_seg.hip; engine.seg_decode / eval_seg_raw / eval_seg) against the host
route (eval_metrics.palette_labels / seg_gt_labels / seg_counts / seg_metrics_from_counts), and the batched device loop
`infer_eval.infer_and_evaluate_seg` with the real pipeline at tiny widths.

No tolerance anywhere.  Labels, distances and counts are integers: they must equal the host's.  The values are one prescribed sequence of
correctly rounded float64 operations on those integers: `out` must equal, bit for bit, seg_metrics_from_counts of the device's own counts and
the host route's rows (NaN matches NaN).

Inputs come from a seed.  Seg-like: piecewise-constant regions of palette colours as floats k / 255 with noisy boundaries and +-3 / 255 of
colour noise, a sprinkle of NaN, -0.25 and 1.5; the ground truth is another noisy rendering of the same regions (so the two disagree along
the boundaries and on a few percent of flipped pixels) as exact palette colours plus a few percent of non-palette pixels, or as a label map
with a few percent of ignore labels.  Palettes for K >= 3 hold one duplicated colour (K - 1 == 0) and one pair two steps apart along one
channel (1, 2): the colour in between ties.  K = 2 has room for the pair only and K = 1 for neither, so the tie and accuracy conditions
below are asserted for K >= 2 (with one class pixel_acc is 1 by definition)."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (3, 64, 65), (1, 517, 1031)]
PAIRS = [(s, k) for s in SHAPES for k in (1, 2, 19)] + [(s, k) for s in SHAPES[:4] for k in (150, 192)]
LARGE = SHAPES[3:]
SEG_METRICS = ["pixel_acc", "mean_acc", "miou", "fwiou", "colour_rmse"]
VARIANTS = [(form, tol, use) for form in ("colour", "labels") for tol in (0, 12) for use in (False, True)]


def make_palette(K, seed=7):
    rng = np.random.RandomState(seed + K)
    pal = rng.randint(0, 256, (K, 3)).astype(np.uint8)
    if K >= 2:
        lo = 0 if K == 2 else 1
        pal[lo, 0] = min(int(pal[lo, 0]), 253)
        pal[lo + 1] = pal[lo]
        pal[lo + 1, 0] += 2                             # (x, g, b) and (x + 2, g, b): (x + 1, g, b) ties, the smaller index wins
    if K >= 3:
        pal[K - 1] = pal[0]                             # a duplicate: every pixel nearest to it ties
    return pal


def region_map(rng, b, h, w, K, jitter):
    """Labels of a coarse random grid, looked up at jittered coordinates: blocks of about 12 x 12 pixels with noisy boundaries."""
    gh, gw = h // 12 + 2, w // 12 + 2
    grid = rng.randint(0, K, (b, gh, gw))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.empty((b, h, w), dtype=np.int64)
    for i in range(b):
        y = np.clip(np.rint((yy + jitter * rng.randn(h, w)) / 12.0), 0, gh - 1).astype(int)
        x = np.clip(np.rint((xx + jitter * rng.randn(h, w)) / 12.0), 0, gw - 1).astype(int)
        out[i] = grid[i][y, x]
    return grid, out


def make_case(b, h, w, K, seed):
    """pred float32 [b, 3, h, w], gt colours uint8 [b, h, w, 3], gt labels uint8 [b, h, w], region bool [b, h, w], palette."""
    rng = np.random.RandomState(seed)
    pal = make_palette(K)
    state = rng.get_state()
    _, lab_p = region_map(rng, b, h, w, K, 1.5)
    rng.set_state(state)                                                   # the same grid, other boundary noise
    _, lab_g = region_map(rng, b, h, w, K, 0.0)
    flip = rng.rand(b, h, w) < 0.05
    lab_p = np.where(flip, rng.randint(0, K, (b, h, w)), lab_p)
    col = pal[lab_p].astype(np.int64) + rng.randint(-3, 4, (b, h, w, 3))
    pred = (np.clip(col, 0, 255).astype(np.float32) / np.float32(255.0) + np.float32(0.2 / 255.0)).astype(np.float32)   # k / 255 and a fifth of a step: truncates to k
    tie = rng.rand(b, h, w) < 0.02
    tie[:, 0, 0] = True                                                    # at least one in every image, however small
    if K >= 2:
        mid = pal[0 if K == 2 else 1].astype(np.float32)
        mid[0] += 1
        pred[tie] = (mid + np.float32(0.2)) / np.float32(255.0)
    pred = np.ascontiguousarray(np.moveaxis(pred, -1, 1))
    if h * w > 4:
        odd = rng.rand(b, 3, h, w)
        pred[odd < 0.002] = np.nan
        pred[(odd > 0.002) & (odd < 0.004)] = -0.25
        pred[(odd > 0.004) & (odd < 0.006)] = 1.5
    gt_col = pal[lab_g].copy()
    off = rng.rand(b, h, w) < 0.04
    near = rng.rand(b, h, w) < 0.5                                         # half of them within gt_tol = 12 of their colour (|(2, 2, 2)|^2 = 12), half anywhere
    gt_col[off & near] = np.clip(gt_col[off & near].astype(int) + np.array([2, -2, 2]) * np.where(gt_col[off & near] > 128, -1, 1), 0, 255).astype(np.uint8)
    gt_col[off & ~near] = rng.randint(0, 256, (int((off & ~near).sum()), 3)).astype(np.uint8)
    gt_lab = lab_g.astype(np.uint8)
    ign = rng.rand(b, h, w)
    gt_lab[ign < 0.03] = 255
    if K < 250:
        gt_lab[(ign > 0.03) & (ign < 0.04)] = K + (7 % (255 - K))          # another value >= K
    region = rng.rand(b, h, w) < 0.6
    return pred, np.ascontiguousarray(gt_col), gt_lab, region, pal


_CASES = {}


def row_of(m, K):
    """seg_metrics_from_counts' dict as gp_eval_seg's out row."""
    assert list(m) == ["n", "n_void"] + SEG_METRICS + ["n_classes", "iou"] and len(m["iou"]) == K
    return np.array([float(m[k]) for k in ["n", "n_void"] + SEG_METRICS + ["n_classes"]] + [float(v) for v in m["iou"]], dtype=np.float64)


def case(shape, K):
    """One input set and one host evaluation per (shape, K), shared by the tests and left unchanged."""
    from genpercept_amd import eval_metrics as em
    key = (shape, K)
    if key not in _CASES:
        b, h, w = shape
        pred, gt_col, gt_lab, region, pal = make_case(b, h, w, K, seed=4000 + 13 * h + K)
        q = np.stack([em.quantize_seg(pred[i]) for i in range(b)])          # [b, h, w, 3]
        labels, dist = em.palette_labels(q, pal)
        host = {}
        for form, tol, use in VARIANTS:
            gl = [em.seg_gt_labels(gt_col[i] if form == "colour" else gt_lab[i], pal, tol) for i in range(b)]
            counts = np.stack([em.seg_counts(q[i], gl[i], pal, region[i] if use else None) for i in range(b)])
            host[(form, tol, use)] = (counts, np.stack([row_of(em.seg_metrics_from_counts(c, K), K) for c in counts]))
        attained = np.zeros(dist.shape, dtype=np.int32)                    # how many palette colours sit at the minimum distance
        for k in range(K):
            attained += ((q.astype(np.int32) - pal[k].astype(np.int32)) ** 2).sum(-1) == dist
        assert attained.min() >= 1
        ties = int((attained > 1).sum())
        arrays = [pred, gt_col, gt_lab, region, pal, q, labels, dist] + [a for v in host.values() for a in v]
        for a in arrays:
            a.setflags(write=False)
        _CASES[key] = dict(pred=pred, gt_col=gt_col, gt_lab=gt_lab, region=region, pal=pal, q=q, labels=labels, dist=dist, host=host, ties=ties)
    return _CASES[key]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def dev(*arrays):
    d = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.array(a)).to(d) for a in arrays]  # (a copy: the shared arrays are read-only)


def host_conditions(shape, K, c):
    """What the issue asks of the host route's own result, so that no path is silently idle."""
    for (form, tol, use), (counts, rows) in c["host"].items():
        if shape in LARGE:
            for i in range(shape[0]):
                n, n_void = int(counts[i, 0]), int(counts[i, 1])
                assert 0.01 < n_void / (n + n_void) < 0.10, (shape, K, form, tol, use, n, n_void)
                if K >= 2:
                    assert 0.5 < rows[i, 2] < 0.98, (shape, K, form, tol, use, rows[i, 2])
                assert rows[i, 7] >= min(K if form == "labels" or K < 3 else K - 1, 8), (shape, K, form, rows[i, 7])
    if K >= 2:
        assert c["ties"] >= 1, (shape, K)


def test_the_seeded_cases_exercise_every_path():
    """(CPU.)  The conditions on the host route's result for every (shape, K) of the device tests, except the largest shape (checked where it
    runs).  With a duplicated colour the colour-form ground truth never holds class K - 1, hence K - 1 classes there."""
    for shape, K in PAIRS:
        if shape != SHAPES[-1]:
            host_conditions(shape, K, case(shape, K))


def check_against_host(c, K, tp, tg, tr, tpal, tol, want, tag):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    want_counts, want_rows = want
    raw, counts, labels = ge.eval_seg_raw(tp, tg, tpal, tr, tol, want_counts=True, want_labels=True)
    raw, counts, labels = raw.cpu().numpy(), counts.cpu().numpy(), labels.cpu().numpy()
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts), (tag, np.flatnonzero(counts != want_counts)[:8])
    assert np.array_equal(labels, c["labels"]), tag
    own = np.stack([row_of(em.seg_metrics_from_counts(cc, K), K) for cc in counts])
    assert same_bits(raw, own), (tag, raw, own)
    assert same_bits(raw, want_rows), (tag, raw, want_rows)
    plain = ge.eval_seg_raw(tp, tg, tpal, tr, tol)                      # without counts_out / labels_out: the matrix lives in the workspace
    assert same_bits(plain.cpu().numpy(), raw), tag


@gpu
@pytest.mark.parametrize("shape,K", PAIRS, ids=[f"{s[0]}x{s[1]}x{s[2]}-K{k}" for s, k in PAIRS])
def test_eval_seg_equals_the_host_route(shape, K):
    """Both ground-truth forms, gt_tol 0 and 12, with and without a region: counts, labels and rows."""
    c = case(shape, K)
    host_conditions(shape, K, c)
    tp, tcol, tlab, tr, tpal = dev(c["pred"], c["gt_col"], c["gt_lab"], c["region"], c["pal"])
    for form, tol, use in VARIANTS:
        check_against_host(c, K, tp, tcol if form == "colour" else tlab, tr if use else None, tpal, tol, c["host"][(form, tol, use)], (shape, K, form, tol, use))


@gpu
@pytest.mark.parametrize("K", [19, 192])
def test_eval_seg_uniform_random_input(K):
    """Uniform random colours against uniform random labels: the lanes of a wave hit different entries of the matrix."""
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(99 + K)
    b, h, w = 2, 64, 65
    pal = make_palette(K)
    pred = rng.rand(b, 3, h, w).astype(np.float32)
    gt = rng.randint(0, K + 2, (b, h, w)).astype(np.uint8)                 # a little void: K and K + 1
    tp, tg, tpal = dev(pred, gt, pal)
    raw, counts = ge.eval_seg_raw(tp, tg, tpal, want_counts=True)
    want = np.stack([em.seg_counts(em.quantize_seg(pred[i]), gt[i], pal) for i in range(b)])
    assert np.array_equal(counts.cpu().numpy(), want)
    assert (want[:, 3:] > 0).sum(axis=1).min() > min(K * K, 4000) // 4    # spread over the matrix
    assert same_bits(raw.cpu().numpy(), np.stack([row_of(em.seg_metrics_from_counts(cc, K), K) for cc in want]))


@gpu
@pytest.mark.parametrize("shape,K", [((1, 7, 5), 2), ((3, 64, 65), 19), ((3, 64, 65), 192), ((1, 517, 1031), 19)])
def test_seg_decode_labels_and_distances(shape, K):
    """gp_seg_decode == palette_labels (labels and distances) == gp_eval_seg's labels_out, for float and uint8 predictions."""
    from genpercept_amd import engine as ge
    c = case(shape, K)
    tp, tq, tlab, tpal = dev(c["pred"], np.moveaxis(c["q"], -1, 1), c["gt_lab"], c["pal"])
    for p in (tp, tq.contiguous()):
        labels, dist = ge.seg_decode(p, tpal, want_dist=True)
        assert labels.dtype == torch.uint8 and dist.dtype == torch.int32
        assert np.array_equal(labels.cpu().numpy(), c["labels"]) and np.array_equal(dist.cpu().numpy(), c["dist"])
        assert torch.equal(ge.seg_decode(p, c["pal"]), labels)           # a numpy palette is uploaded
        _, own = ge.eval_seg_raw(p, tlab, tpal, want_labels=True)
        assert torch.equal(own, labels)
    assert torch.equal(ge.seg_decode(tp[0], tpal), ge.seg_decode(tp, tpal)[:1])   # [3, H, W]


@gpu
def test_eval_seg_on_postprocess_bytes():
    """The bytes `postprocess(..., q_bits=8)` writes: uint8 prediction == float prediction."""
    from genpercept_amd import engine as ge
    c = case((3, 64, 65), 19)
    tp, tcol, tr, tpal = dev(c["pred"], c["gt_col"], c["region"], c["pal"])
    out, _, q8 = ge.postprocess(tp, (64, 65), "bilinear", q_bits=8)
    assert q8.dtype == torch.uint8 and tuple(q8.shape) == (3, 3, 64, 65)
    assert np.array_equal(np.moveaxis(q8.cpu().numpy(), 1, -1), c["q"])
    for r in (None, tr):
        a, ca, la = ge.eval_seg_raw(q8, tcol, tpal, r, 12, want_counts=True, want_labels=True)
        for other in (tp, out):                                           # the unclipped floats (the kernel clips) and the clipped ones
            b, cb, lb = ge.eval_seg_raw(other, tcol, tpal, r, 12, want_counts=True, want_labels=True)
            assert torch.equal(ca, cb) and torch.equal(la, lb) and same_bits(a.cpu().numpy(), b.cpu().numpy())


@gpu
@pytest.mark.parametrize("K", [19, 192])
def test_eval_seg_unaligned_views(K):
    """pred, gt, region and palette as views at odd offsets inside larger allocations, one at a time and together: the same bits."""
    from genpercept_amd import engine as ge
    c = case((3, 64, 65), K)
    d = torch.device("cuda", 0)

    def shifted(a, by=1):
        t = torch.from_numpy(np.array(a))
        buf = torch.empty(t.numel() + by, dtype=t.dtype, device=d)
        v = buf[by:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    q = np.ascontiguousarray(np.moveaxis(c["q"], -1, 1))
    ap, aq, acol, alab, ar, apal = dev(c["pred"], q, c["gt_col"], c["gt_lab"], c["region"], c["pal"])
    sp, sq, scol, slab, sr, spal = (shifted(x) for x in (c["pred"], q, c["gt_col"], c["gt_lab"], c["region"], c["pal"]))
    scol3, sq3 = shifted(c["gt_col"], 3), shifted(q, 3)
    for form, ag, sgs in (("colour", acol, (scol, scol3)), ("labels", alab, (slab,))):
        want = [x.cpu() for x in ge.eval_seg_raw(ap, ag, apal, ar, 12, want_counts=True, want_labels=True)]
        assert np.array_equal(want[1].numpy(), c["host"][(form, 12, True)][0])
        combos = [(sp, ag, ar, apal), (ap, ag, sr, apal), (ap, ag, ar, spal), (aq, ag, ar, apal), (sq, ag, ar, apal), (sq3, ag, sr, spal)]
        combos += [(ap, sg, ar, apal) for sg in sgs] + [(sp, sg, sr, spal) for sg in sgs] + [(sq, sg, sr, spal) for sg in sgs]
        for p, g, r, pal in combos:
            raw, counts, labels = ge.eval_seg_raw(p, g, pal, r, 12, want_counts=True, want_labels=True)
            assert torch.equal(counts.cpu(), want[1]) and torch.equal(labels.cpu(), want[2]) and same_bits(raw.cpu().numpy(), want[0].numpy())
    for p in (sp, sq, sq3):
        labels, dist = ge.seg_decode(p, spal, want_dist=True)
        assert np.array_equal(labels.cpu().numpy(), c["labels"]) and np.array_equal(dist.cpu().numpy(), c["dist"])


@gpu
def test_eval_seg_is_stable_and_batch_independent():
    """Three calls: identical.  Image i alone (a slice: another base address; a clone: an aligned one) == the same image inside the batch of 3.
    An image without a scored pixel inside a batch: the two counts and NaN for it, its neighbours unchanged; engine.eval_seg names it."""
    from genpercept_amd import engine as ge
    c = case((3, 64, 65), 150)
    K = 150
    tp, tcol, tr, tpal = dev(c["pred"], c["gt_col"], c["region"], c["pal"])
    for r in (None, tr):
        a, ca, la = ge.eval_seg_raw(tp, tcol, tpal, r, want_counts=True, want_labels=True)
        for _ in range(2):
            b, cb, lb = ge.eval_seg_raw(tp, tcol, tpal, r, want_counts=True, want_labels=True)
            assert same_bits(a.cpu().numpy(), b.cpu().numpy()) and torch.equal(ca, cb) and torch.equal(la, lb)
        for i in range(3):
            ri = None if r is None else r[i:i + 1]
            alone, c1, l1 = ge.eval_seg_raw(tp[i:i + 1], tcol[i:i + 1], tpal, ri, want_counts=True, want_labels=True)
            assert same_bits(alone[0].cpu().numpy(), a[i].cpu().numpy()) and torch.equal(c1[0], ca[i]) and torch.equal(l1[0], la[i]), i
            copy = ge.eval_seg_raw(tp[i].clone(), tcol[i].clone(), tpal, None if r is None else r[i].clone())
            assert same_bits(copy[0].cpu().numpy(), a[i].cpu().numpy()), i
    region2 = c["region"].copy()
    region2[1] = False
    (tr2,) = dev(region2)
    full = ge.eval_seg_raw(tp, tcol, tpal, tr).cpu().numpy()
    raw, counts = ge.eval_seg_raw(tp, tcol, tpal, tr2, want_counts=True)
    raw, counts = raw.cpu().numpy(), counts.cpu().numpy()
    assert raw[1, 0] == 0 and raw[1, 1] == 0 and np.isnan(raw[1, 2:]).all() and (counts[1] == 0).all()
    assert same_bits(raw[0], full[0]) and same_bits(raw[2], full[2])
    with pytest.raises(ValueError, match="image 1"):
        ge.eval_seg(tp, tcol, tpal, tr2)
    res = ge.eval_seg(tp, tcol, tpal, tr)
    host_counts, host_rows = c["host"][("colour", 0, True)]
    assert len(res) == 3
    for i, m in enumerate(res):
        assert list(m)[:5] == SEG_METRICS and same_bits([m[k] for k in SEG_METRICS], host_rows[i, 2:7])
        assert m["n"] == host_counts[i, 0] and m["n_void"] == host_counts[i, 1] and m["n_classes"] == host_rows[i, 7]
        assert m["iou"].shape == (K,) and same_bits(m["iou"], host_rows[i, 8:])
        assert m["conf"].shape == (K, K) and m["conf"].dtype == np.int64 and np.array_equal(m["conf"].reshape(-1), host_counts[i, 3:])


@pytest.fixture(scope="module")
def tiny_weights():
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    return dict(uc=uc, vc=vc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32c"])
def test_infer_and_evaluate_seg_with_the_pipeline(precision, tiny_weights, tmp_path):
    """The device loop for mode "seg" on a tree of colour label images: three 96 x 128 images and one 64 x 64, batch_size 2.  Its table and its
    values == host evaluate_seg_predictions over the `.npy` maps it saved, bit for bit.  The palette is eight corners-and-greys of the colour
    cube, so that whatever the synthetic weights paint lands on several classes."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(53)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype={"bf16": torch.bfloat16, "fp32c": torch.float32}[precision])
    pipe.to("cuda")
    pal = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [0, 255, 0], [0, 0, 255], [64, 64, 64], [192, 192, 192]], np.uint8)
    names = ["black", "white", "grey", "red", "green", "blue", "dark", "light"]
    base, out, ref_dir = str(tmp_path / "data"), str(tmp_path / "out"), str(tmp_path / "ref")
    samples, sizes = [], [(96, 128), (96, 128), (96, 128), (64, 64)]
    rng = np.random.RandomState(5)
    for i, (h, w) in enumerate(sizes):
        for sub in ("im", "seg"):
            os.makedirs(os.path.join(base, "set0", sub), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "set0", "im", f"{i:04d}.png"))
        lab = rng.randint(0, 8, (h // 8, w // 8)).repeat(8, 0).repeat(8, 1)
        col = pal[lab]
        col[rng.rand(h, w) < 0.03] = (10, 200, 90)                        # void
        Image.fromarray(col if i != 1 else lab.astype(np.uint8)).save(os.path.join(base, "set0", "seg", f"{i:04d}.png"))   # the second: a label map
        samples.append([f"set0/im/{i:04d}.png", "x", "None", "None", "None", "None", f"set0/seg/{i:04d}.png"])
    try:
        res = ie.infer_and_evaluate_seg(pipe, base, samples, (pal, names), output_dir=out, batch_size=2, save_predictions=True, processing_res=0)
        ref = ie.evaluate_seg_predictions(out, base, samples, ie.FileNameMode.id, (pal, names), output_dir=ref_dir)
        for k in ref:
            print(f"infer_and_evaluate_seg[{precision}] {k}: device {res[k]!r} host {ref[k]!r}")
        assert list(res) == SEG_METRICS + ["miou_dataset", "pixel_acc_dataset", "iou_dataset"]
        assert all(np.isfinite(res[k]) for k in SEG_METRICS + ["miou_dataset", "pixel_acc_dataset"])
        assert list(res) == list(ref) and all(same_bits(res[k], ref[k]) for k in ref)
        for name in ("per_sample_metrics-seg.csv", "eval_metrics-seg.txt"):
            a, b = (open(os.path.join(d, name)).read().splitlines() for d in (out, ref_dir))
            assert len(a) == len(b) and [x for x in a if "of predictions" not in x] == [x for x in b if "of predictions" not in x]
        assert len(open(os.path.join(out, "per_sample_metrics-seg.csv")).read().splitlines()) == 1 + len(samples)
        for s, (h, w) in zip(samples, sizes):
            saved = np.load(os.path.join(out, os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy")))
            assert saved.shape == (h, w, 3) and saved.dtype == np.float32 and saved.min() >= 0.0 and saved.max() <= 1.0
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
