"""Matting gradient and connectivity errors on the device (gp_eval_matting, csrc/eval_matting.hip; engine.eval_matting) against the host route
(eval_metrics.conn_levels / conn_error / grad_error_map / grad_error), and the batched device loop
`infer_eval.infer_and_evaluate_masks(..., matting=True)` with the real pipeline at tiny widths.

Bounds.  `level_out`, `counts_out` and `conn` are integers up to one correctly rounded division: equal to the host's, bit for bit, with and
without a region, for float and uint8 predictions.  `grad_map_out` is one prescribed sequence of correctly rounded + - * / sqrt per pixel (no
FMA on either side): bit-equal to grad_error_map, NaN cannot occur.  `grad_sum` and `grad` are float64 sums of at most 1.4e5 non-negative
terms taken in another order: 1e-9 relative, the project's bound for such sums (tests/test_eval_device_gpu.py).

Shapes: one pixel; the scalar tail; a map smaller than the filter; unaligned planes in a batch of three with several workgroups; 257 x 515,
where components cross many workgroup borders; and three rows of 8200 pixels, 33 row segments wide.  The hand-made maps below, which
tests/test_eval_matting_host.py shares (serpentine, checkerboards, equal blocks, empty levels, bytes at the thresholds), at 64 x 65 and the
first three at 257 x 515.

Largest differences seen on an MI355X (logged through the `metric_log` fixture): see DESIGN.md section 4."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval_structure_device_gpu import make_case  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (3, 64, 65), (1, 257, 515), (1, 3, 8200)]
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
STRUCTURE_METRICS = ["s_alpha", "max_e", "mean_e", "adp_e", "wf"]
MATTING_METRICS = ["grad", "conn"]
OUT_NAMES = ["n", "grad", "conn", "grad_sum"]
GP_ERR_INVALID = 1
T = [26, 51, 77, 102, 128, 153, 179, 204, 230, 255]  # ceil(255 k / 10)


# ---- the hand-made maps (shared with tests/test_eval_matting_host.py) ---------------------------------------------------------------------------
def serpentine(h, w):
    """A one-pixel-wide path of 255 that covers the image: every other row in full, joined alternately at the right and the left end."""
    s = np.zeros((h, w), np.uint8)
    s[::2] = 255
    for r in range(1, h, 2):
        s[r, w - 1 if (r // 2) % 2 == 0 else 0] = 255
    return s


def checkerboard(h, w, first):
    """255 on the squares of one colour (`first`: whether pixel 0 is one of them), 0 elsewhere: every component is a single pixel."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) % 2 == 0) == bool(first)).astype(np.uint8) * 255


def equal_blocks(h, w):
    """Two components of the same size, the second one listed first in no order but the index: a 2 x 3 block in the lower right corner and one
    near the upper left, plus a smaller third."""
    s = np.zeros((h, w), np.uint8)
    s[h - 2:h, w - 3:w] = 255
    s[1:3, 1:4] = 255
    s[h // 2, w // 2] = 255
    return s


def hand_maps(h, w):
    """name -> (q, g) uint8 [h, w] (h >= 6, w >= 8)."""
    rng = np.random.RandomState(h * 1000 + w)
    noise = rng.randint(0, 256, (h, w)).astype(np.uint8)
    fading = np.minimum(noise, 150).astype(np.uint8)                       # I_k is empty from k = 6 on (T_6 = 153)
    edges = np.array(T + [t - 1 for t in T], np.uint8)[rng.randint(0, 20, (h, w))]   # bytes exactly at the T_k and one below
    ser = serpentine(h, w)
    return {
        "serpentine": (ser, np.maximum(ser, noise)),
        "serpentine both": (ser, ser),
        "checkerboard with pixel 0": (checkerboard(h, w, True), np.full((h, w), 255, np.uint8)),
        "checkerboard without pixel 0": (np.maximum(checkerboard(h, w, False), 30).astype(np.uint8), np.full((h, w), 200, np.uint8)),
        "equal blocks": (equal_blocks(h, w), np.full((h, w), 255, np.uint8)),
        "fading": (fading, noise),
        "thresholds": (edges, np.full((h, w), 255, np.uint8)),
        "thresholds both": (edges, edges[::-1, ::-1].copy()),
        "all 255": (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8)),
        "same": (noise, noise),
    }


def host_eval(q, gt, region=None):
    """The host route for a batch of bytes: (levels [b, h, w] uint8, counts [b, 13], error maps [b, h, w], one dict per image with OUT_NAMES)."""
    from genpercept_amd import eval_metrics as em
    levels, counts, maps, rows = [], [], [], []
    for i in range(q.shape[0]):
        r = None if region is None else region[i]
        c, g = em.conn_error(q[i], gt[i], r), em.grad_error(q[i], gt[i], r)
        levels.append(em.conn_levels(q[i], gt[i]))
        counts.append(c["counts"])
        maps.append(em.grad_error_map(q[i], gt[i]))
        rows.append(dict(n=c["n"], grad=g["grad"], conn=c["conn"], grad_sum=g["grad_sum"]))
    return np.stack(levels), np.stack(counts), np.stack(maps), rows


_CASES = {}


def case(key):
    """One input set and one host evaluation per shape or (hand-made map name, h, w), shared by the tests and left unchanged:
    (pred or None, gt, q, region, whole-image host results, host results inside the region)."""
    from genpercept_amd import eval_metrics as em
    if key not in _CASES:
        if isinstance(key[0], str):
            q, gt = (a[None] for a in hand_maps(key[1], key[2])[key[0]])
            pred = None
        else:
            pred, gt = make_case(*key, seed=2000 + key[1])
            q = em.quantize_mask(pred)
        region = (np.random.RandomState(7 + q.shape[2]).rand(*q.shape) < 0.4).astype(np.uint8) * 3
        if q[0].size > 4:
            region[0, 0, 0], region[0, -1, -1] = 0, 5
        whole, inside = host_eval(q, gt), host_eval(q, gt, region)
        for a in (pred, gt, q, region) + whole[:3] + inside[:3]:
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = (pred, gt, q, region, whole, inside)
    return _CASES[key]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def dev(*arrays):
    d = torch.device("cuda", 0)
    return [None if a is None else torch.from_numpy(np.array(a)).to(d) for a in arrays]  # (a copy: the shared arrays are read-only)


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def check_against_host(tp, tg, tr, want, tag, metric_log=None):
    """level_out, counts_out, conn and grad_map_out == the host's, bit for bit; grad_sum and grad within 1e-9 relative.  Every figure is
    printed before it is asserted."""
    from genpercept_amd import engine as ge
    want_levels, want_counts, want_maps, want_rows = want
    raw, counts, levels, gmap = ge.eval_matting_raw(tp, tg, tr, want_counts=True, want_levels=True, want_grad_map=True)
    alone = ge.eval_matting_raw(tp, tg, tr)
    raw, counts, levels, gmap, alone = raw.cpu().numpy(), counts.cpu().numpy(), levels.cpu().numpy(), gmap.cpu().numpy(), alone.cpu().numpy()
    b = want_counts.shape[0]
    assert raw.shape == (b, 4) and raw.dtype == np.float64 and counts.shape == (b, 13) and levels.shape == want_levels.shape and levels.dtype == np.uint8
    assert gmap.shape == want_maps.shape and gmap.dtype == np.float64
    worst = dict(grad_sum=0.0, grad=0.0, map_ulp=0.0)
    for i in range(b):
        bad_levels = np.flatnonzero(levels[i].reshape(-1) != want_levels[i].reshape(-1))
        bad_counts = np.flatnonzero(counts[i] != want_counts[i])
        bad_map = np.flatnonzero(gmap[i].reshape(-1).view(np.int64) != want_maps[i].reshape(-1).view(np.int64))
        got, host = dict(zip(OUT_NAMES, raw[i].tolist())), want_rows[i]
        ulp = float((np.abs(gmap[i] - want_maps[i]) / np.spacing(np.maximum(want_maps[i], np.finfo(np.float64).tiny))).max())
        worst["map_ulp"] = max(worst["map_ulp"], ulp)
        print(f"eval_matting {tag} image {i}: levels differing from the host: {bad_levels.size}  counts differing: {bad_counts.size}  "
              f"error-map values differing: {bad_map.size} (largest {ulp} ulp)  level counts {counts[i, 2:].tolist()}")
        print(f"    out  {got}\n    host {host}")
        assert bad_levels.size == 0, (tag, i, bad_levels[:8], levels[i].reshape(-1)[bad_levels[:8]], want_levels[i].reshape(-1)[bad_levels[:8]])
        assert bad_counts.size == 0, (tag, i, bad_counts[:8], counts[i][bad_counts[:8]], want_counts[i][bad_counts[:8]])
        assert np.isfinite(gmap[i]).all() and bad_map.size == 0, (tag, i, bad_map[:8], gmap[i].reshape(-1)[bad_map[:8]], want_maps[i].reshape(-1)[bad_map[:8]])
        assert got["n"] == host["n"] and same_bits(got["conn"], host["conn"]), (tag, i, got, host)
        if host["n"] == 0:
            assert np.isnan(raw[i, 1:]).all()
            continue
        assert same_bits(got["grad"], got["grad_sum"] / 1000.0)
        for name in ("grad_sum", "grad"):
            worst[name] = max(worst[name], rel(got[name], host[name]))
            assert rel(got[name], host[name]) <= 1e-9, (tag, i, name, got[name], host[name])
    assert same_bits(alone, raw)  # with and without the optional outputs (the levels then live in the workspace only)
    if metric_log is not None:
        metric_log(f"eval_matting {tag}", **{("rel_" + k if k != "map_ulp" else k): v for k, v in worst.items()})
    return raw, counts, levels, gmap


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_matting_matches_host_on_mask_like_input(shape, metric_log):
    pred, gt, q, region, whole, inside = case(shape)
    if shape in ((3, 64, 65), (1, 257, 515)):
        assert (whole[1][:, 2:] > 0).all()                         # the recipe fills all eleven levels
    tp, tg, tq, tr = dev(pred, gt, q, region)
    a = check_against_host(tp, tg, None, whole, shape, metric_log)
    b = check_against_host(tq, tg, None, whole, (shape, "uint8"))
    check_against_host(tp, tg, tr, inside, (shape, "region"), metric_log)
    check_against_host(tq, tg, tr != 0, inside, (shape, "uint8, bool region"))
    assert same_bits(a[0], b[0])


@gpu
@pytest.mark.parametrize("name", ["serpentine", "serpentine both", "checkerboard with pixel 0", "checkerboard without pixel 0", "equal blocks", "fading",
                                  "thresholds", "thresholds both", "all 255", "same"])
def test_eval_matting_hand_made_maps(name, metric_log):
    pred, gt, q, region, whole, inside = case((name, 64, 65))
    tg, tq, tr = dev(gt, q, region)
    raw, counts, levels, gmap = check_against_host(tq, tg, None, whole, name, metric_log)
    check_against_host(tq, tg, tr, inside, (name, "region"))
    if name in ("all 255", "same"):
        assert raw[0, 2] == 0.0 and raw[0, 1] == 0.0 and not gmap.any()
    if name == "all 255":
        assert (levels == 10).all()
    if name == "equal blocks":
        assert (levels[0, 1:3, 1:4] == 10).all() and levels.sum() == 60
    if name == "fading":
        assert counts[0, 2 + 6:].sum() == 0 and levels.max() == 5


@gpu
@pytest.mark.parametrize("name", ["serpentine", "checkerboard with pixel 0", "equal blocks"])
def test_eval_matting_hand_made_maps_across_many_workgroups(name, metric_log):
    pred, gt, q, region, whole, inside = case((name, 257, 515))
    tg, tq = dev(gt, q)
    raw, counts, levels, gmap = check_against_host(tq, tg, None, whole, (name, 257, 515), metric_log)
    if name == "serpentine":
        assert counts[0, 12] == int((q == 255).sum()) == 129 * 515 + 128                # one component of 66 563 pixels at every level


@gpu
def test_eval_matting_unaligned_views_and_binding_forms():
    """The (3, 64, 65) tensors again as views one element into an allocation; [B, 1, H, W] input; engine.eval_matting's dicts."""
    from genpercept_amd import engine as ge
    pred, gt, q, region, whole, inside = case((3, 64, 65))
    d = torch.device("cuda", 0)

    def shifted(a):
        t = torch.from_numpy(np.array(a))
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=d)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    ap, ag, aq, ar = dev(pred, gt, q, region)
    sp, sg, sq, sr = shifted(pred), shifted(gt), shifted(q), shifted(region)
    want = [x.cpu() for x in ge.eval_matting_raw(ap, ag, ar, want_counts=True, want_levels=True, want_grad_map=True)]
    assert np.array_equal(want[1].numpy(), inside[1]) and np.array_equal(want[2].numpy(), inside[0])
    for p, g, r in ((sp, sg, sr), (sp, ag, ar), (ap, sg, sr), (sq, sg, ar), (sq, ag, sr), (aq, sg, sr)):
        raw, c, lv, gm = ge.eval_matting_raw(p, g, r, want_counts=True, want_levels=True, want_grad_map=True)
        assert torch.equal(c.cpu(), want[1]) and torch.equal(lv.cpu(), want[2]) and torch.equal(gm.cpu(), want[3])
        assert same_bits(raw.cpu().numpy(), want[0].numpy())
    c4 = ge.eval_matting_raw(aq[:, None], ag[:, None], ar[:, None])
    assert same_bits(c4.cpu().numpy(), want[0].numpy())
    res = ge.eval_matting(ap, ag, ar)
    assert len(res) == 3
    for i, m in enumerate(res):
        assert list(m) == OUT_NAMES and same_bits([m[k] for k in OUT_NAMES], want[0][i].numpy()) and isinstance(m["n"], int) and m["n"] == inside[3][i]["n"]
    empty = torch.zeros_like(ar)
    empty[0] = 1
    raw = ge.eval_matting_raw(ap, ag, empty).cpu().numpy()
    assert raw[1, 0] == 0 and np.isnan(raw[1, 1:]).all() and np.isnan(raw[2, 1:]).all() and np.isfinite(raw[0]).all()
    with pytest.raises(ValueError, match="image 1"):
        ge.eval_matting(ap, ag, empty)


@gpu
def test_eval_matting_is_stable_and_batch_independent():
    """Two calls: identical.  Image i alone (a slice: another base address; a clone: an aligned one) == the same image inside the batch of 3.
    A workspace filled with 0xFF before the call changes nothing: every word that is read has been written by the call."""
    from genpercept_amd import engine as ge
    pred, gt, q, region, whole, inside = case((3, 64, 65))
    tp, tg, tr = dev(pred, gt, region)
    a = ge.eval_matting_raw(tp, tg, tr, want_counts=True, want_levels=True, want_grad_map=True)
    b = ge.eval_matting_raw(tp, tg, tr, want_counts=True, want_levels=True, want_grad_map=True)
    assert torch.isfinite(a[0]).all() and same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    for i in range(3):
        one = ge.eval_matting_raw(tp[i:i + 1], tg[i:i + 1], tr[i:i + 1], want_counts=True, want_levels=True, want_grad_map=True)
        assert same_bits(one[0][0].cpu().numpy(), a[0][i].cpu().numpy()) and all(torch.equal(x[0], y[i]) for x, y in zip(one[1:], a[1:])), i
        copy = ge.eval_matting_raw(tp[i].clone(), tg[i].clone(), tr[i].clone())
        assert same_bits(copy[0].cpu().numpy(), a[0][i].cpu().numpy()), i
    lib = ge.load_library()
    nbytes = int(lib.gp_eval_matting_workspace(3, 64, 65))
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=tp.device)
        out = torch.empty((3, 4), dtype=torch.float64, device=tp.device)
        counts = torch.empty((3, 13), dtype=torch.int64, device=tp.device)
        levels = torch.empty((3, 64, 65), dtype=torch.uint8, device=tp.device)
        gmap = torch.empty((3, 64, 65), dtype=torch.float64, device=tp.device)
        st = lib.gp_eval_matting(tp.data_ptr(), 0, tg.data_ptr(), tr.data_ptr(), 3, 64, 65, out.data_ptr(), counts.data_ptr(), levels.data_ptr(),
                                 gmap.data_ptr(), ws.data_ptr(), nbytes, ge._stream_ptr(tp.device))
        assert st == 0
        outs.append((out, counts, levels, gmap))
    for got in outs:
        assert same_bits(got[0].cpu().numpy(), a[0].cpu().numpy()) and all(torch.equal(x, y) for x, y in zip(got[1:], a[1:]))


@gpu
def test_eval_matting_refuses_invalid_arguments_before_touching_the_device():
    """The host test's cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill."""
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    d = torch.device("cuda", 0)
    need = int(lib.gp_eval_matting_workspace(2, 8, 8))
    pred = torch.rand(2, 8, 8, device=d)
    gt = torch.randint(0, 256, (2, 8, 8), dtype=torch.uint8, device=d)
    out = torch.full((2, 4), -7.0, dtype=torch.float64, device=d)
    counts = torch.full((2, 13), -7, dtype=torch.int64, device=d)
    levels = torch.full((2, 8, 8), 99, dtype=torch.uint8, device=d)
    gmap = torch.full((2, 8, 8), -7.0, dtype=torch.float64, device=d)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=d)
    ok = dict(pred=pred.data_ptr(), u8=0, gt=gt.data_ptr(), region=None, B=2, H=8, W=8, out=out.data_ptr(), counts=counts.data_ptr(),
              levels=levels.data_ptr(), gmap=gmap.data_ptr(), ws=ws.data_ptr(), nbytes=need)
    cases = [dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=-1), dict(B=65536), dict(u8=2), dict(u8=-1),
             dict(pred=pred.data_ptr() + 2), dict(out=out.data_ptr() + 4), dict(counts=counts.data_ptr() + 4), dict(gmap=gmap.data_ptr() + 4),
             dict(ws=ws.data_ptr() + 4), dict(nbytes=need - 1), dict(nbytes=0), dict(H=65536, W=65536)]
    for kw in cases:
        a = dict(ok, **kw)
        st = lib.gp_eval_matting(a["pred"], a["u8"], a["gt"], a["region"], a["B"], a["H"], a["W"], a["out"], a["counts"], a["levels"], a["gmap"], a["ws"],
                                 a["nbytes"], None)
        assert st == GP_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (counts == -7).all() and (levels == 99).all() and (gmap == -7.0).all() and (ws == 0x5A).all()


@pytest.fixture(scope="module")
def tiny_weights():
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    return dict(uc=uc, vc=vc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32c"])
def test_infer_and_evaluate_masks_matting_with_the_pipeline(precision, tiny_weights, tmp_path):
    """The device loop for mode "matting" with matting=True and a region: three 96 x 128 images and one 64 x 64, batch_size 2.  == host
    evaluate_mask_predictions(matting=True) over the `.npy` maps it saved: conn and the seven old columns exactly, grad to 1e-9.  With
    matting=False the loop's output equals what the functions that existed before give on the same maps: evaluate_mask_predictions without the
    flag, and eval_metrics.mask_metrics per image."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(47)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype={"bf16": torch.bfloat16, "fp32c": torch.float32}[precision])
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

    def region_of(sample, gt):                                       # a trimap's unknown band, a little widened
        return (gt > 0) & (gt < 255) | (np.arange(gt.shape[1])[None] % 7 == 0)

    try:
        res = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=out, batch_size=2, save_predictions=True, processing_res=0,
                                          region_of=region_of, matting=True)
        off = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=off_dir, batch_size=2, processing_res=0, region_of=region_of)
        ref = ie.evaluate_mask_predictions(out, base, samples, ie.FileNameMode.id, output_dir=ref_dir, region_of=region_of, matting=True)
        old = ie.evaluate_mask_predictions(out, base, samples, ie.FileNameMode.id, output_dir=old_dir, region_of=region_of)
        for k in ref:
            print(f"infer_and_evaluate_masks[{precision}, matting] {k}: device {res[k]!r} host {ref[k]!r}")
        assert list(res) == MASK_METRICS + MATTING_METRICS + ["max_f_dataset"] and all(np.isfinite(v) for v in res.values())
        assert list(off) == list(old) == MASK_METRICS + ["max_f_dataset"] and all(same_bits(off[k], res[k]) and same_bits(off[k], old[k]) for k in off)
        for k in res:
            if k == "grad":
                assert rel(res[k], ref[k]) <= 1e-9, (k, res[k], ref[k])
            else:
                assert same_bits(res[k], ref[k]), (k, res[k], ref[k])
        assert res["conn"] > 0 and res["grad"] > 0
        name = "per_sample_metrics-mask.csv"
        rows, rows_ref, rows_off, rows_old = (open(os.path.join(d, name)).read().splitlines() for d in (out, ref_dir, off_dir, old_dir))
        assert rows[0] == rows_ref[0] == "filename," + ",".join(MASK_METRICS + MATTING_METRICS) and len(rows) == len(rows_ref) == 1 + len(samples)
        assert rows_off == rows_old and rows_off[0] == "filename," + ",".join(MASK_METRICS)
        for a, b, c, s in zip(rows[1:], rows_ref[1:], rows_off[1:], samples):
            fa, fb = a.split(","), b.split(",")
            assert fa[:8] == fb[:8] and fa[9] == fb[9] and rel(float(fa[8]), float(fb[8])) <= 1e-9, (a, b)   # grad is the column before conn
            assert ",".join(fa[:8]) == c                                                                       # the name and the seven old columns
            gt = ie.read_gt_mask(os.path.join(base, s[1]))
            m = em.mask_metrics(np.load(os.path.join(out, fa[0])), gt, region_of(s, gt))
            assert c == fa[0] + "," + ",".join(str(m[k]) for k in MASK_METRICS)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
