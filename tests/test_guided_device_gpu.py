"""Edge-aware upsampling on the device (gp_guided_upsample): the output BIT-EQUAL to the host route genpercept_amd/guided.py (itself pinned to
plain loops and to a CPU build of the kernels' arithmetic in tests/test_guided_host.py), over shapes that take every path of the four kernels
(one pixel, one row, one exact tile with an identity upsample, a one-pixel overhang, a batch, several tiles that are multiples of nothing),
every r of {1, 4, 32} (32 is larger than the small images), three eps, C = 1 and 3, hand-made inputs, byte pointers one byte into their
buffers; batch independence and repeatability; the argument checks with real buffers around them; the pipeline, the cutouts and the dataset
loop with `refine` at tiny widths.  There is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from post_support import assert_refused_with_real_buffers, bits, tiny_weights_dict, unaligned  # noqa: E402
from test_guided_host import call_guided, invalid_cases, random_inputs, same_bits  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (1, 1, 7, 3, 20), (2, 16, 32, 16, 32), (1, 17, 33, 70, 131), (3, 37, 61, 149, 243), (1, 96, 130, 257, 300)]
GRID = [(r, eps) for r in (1, 4, 32) for eps in (1e-6, 1e-4, 1.0)]
KINDS = ["random blocks", "all 0", "all 255 / 1.0", "checkerboard", "soft ramp", "one bright pixel", "odd values"]


def inputs(kind, b, c, h, w, H, W, seed):
    """(guide_lo uint8 [B, 3, h, w], pred float32 [B, C, h, w], guide uint8 [B, 3, H, W])"""
    rng = np.random.RandomState(seed)
    rnd = [random_inputs(rng, c, h, w, H, W) for _ in range(b)]
    lo, p, hi = (np.stack([r[k] for r in rnd]) for k in range(3))
    yy, xx = np.mgrid[0:h, 0:w]
    YY, XX = np.mgrid[0:H, 0:W]
    if kind == "all 0":
        lo[:], p[:], hi[:] = 0, 0.0, 0
    elif kind == "all 255 / 1.0":
        lo[:], p[:], hi[:] = 255, 1.0, 255
    elif kind == "checkerboard":
        lo[:], hi[:] = ((yy + xx) % 2 * 255).astype(np.uint8), ((YY + XX) % 2 * 255).astype(np.uint8)
        p[:] = ((yy + xx) % 2).astype(np.float32)
    elif kind == "soft ramp":
        p[:] = ((xx + yy) / max(h + w - 2, 1)).astype(np.float32)
        lo[:, 1], hi[:, 1] = (xx * 255 // max(w - 1, 1)).astype(np.uint8), (XX * 255 // max(W - 1, 1)).astype(np.uint8)
    elif kind == "one bright pixel":
        lo[:], p[:], hi[:] = 0, 0.0, 0
        lo[:, :, h // 2, (2 * w) // 3], p[:, :, h // 2, (2 * w) // 3], hi[:, :, H // 2, (2 * W) // 3] = 255, 1.0, 255
    elif kind == "odd values":
        k = rng.randint(0, 65536, p.shape).astype(np.float32) / np.float32(65535.0)
        side = rng.randint(0, 3, p.shape)
        p = np.where(side == 0, np.nextafter(k, np.float32(-1.0)), np.where(side == 1, np.nextafter(k, np.float32(2.0)), k)).astype(np.float32)
        flat = p.reshape(b, -1)
        flat[:, 0] = np.nan
        if flat.shape[1] > 2:
            flat[:, -1], flat[:, flat.shape[1] // 2] = 1.5, -0.25
    return lo, p, hi


def check(lo, p, hi, lo_d, p_d, hi_d, r, eps, what):
    from genpercept_amd import engine as ge
    from genpercept_amd import guided as gd
    got = ge.guided_upsample(lo_d, p_d, hi_d, r, eps).cpu().numpy()
    assert got.shape == p.shape[:2] + hi.shape[2:]
    for i in range(lo.shape[0]):
        want = gd.guided_upsample(lo[i], p[i], hi[i], r, eps)
        assert same_bits(got[i], want), (what, i, r, eps, int((got[i].view(np.uint32) != want.view(np.uint32)).sum()), float(np.abs(got[i] - want).max()))


@gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d-%dx%d" % s)
def test_output_equals_the_host_route(shape, c):
    b, h, w, H, W = shape
    n = 0
    for kind in KINDS:
        lo, p, hi = inputs(kind, b, c, h, w, H, W, 7000 + 10 * h + c)
        lo_d, p_d, hi_d = unaligned(lo), torch.from_numpy(p).cuda(), unaligned(hi)
        assert lo_d.data_ptr() % 2 == 1 and hi_d.data_ptr() % 2 == 1
        if kind in ("random blocks", "odd values"):
            for r, eps in GRID:
                check(lo, p, hi, lo_d, p_d, hi_d, r, eps, kind)
        else:
            for r, eps in (GRID[4], GRID[(3 * n + n // 3) % 9]):
                check(lo, p, hi, lo_d, p_d, hi_d, r, eps, kind)
            n += 1


@gpu
def test_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    for (h, w, H, W), c, r in (((37, 61, 149, 243), 1, 4), ((40, 70, 33, 50), 3, 32)):
        lo, p, hi = (torch.from_numpy(v).cuda() for v in inputs("random blocks", 3, c, h, w, H, W, 21))
        whole, again = ge.guided_upsample(lo, p, hi, r, 1e-4), ge.guided_upsample(lo, p, hi, r, 1e-4)
        assert whole.dtype == torch.float32 and tuple(whole.shape) == (3, c, H, W)
        assert torch.equal(whole.view(torch.int32), again.view(torch.int32))
        for i in range(3):
            one = ge.guided_upsample(lo[i], p[i], hi[i], r, 1e-4)
            assert torch.equal(one[0].view(torch.int32), whole[i].view(torch.int32))
        assert float(whole.min()) >= 0.0 and float(whole.max()) <= 1.0
        for dt in (torch.float16, torch.float64):  # other float types go through float32
            assert torch.equal(ge.guided_upsample(lo, p.to(dt), hi, r), ge.guided_upsample(lo, p.to(dt).to(torch.float32), hi, r))
    for bad in (dict(radius=0), dict(radius=33), dict(eps=0.0), dict(eps=2.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            ge.guided_upsample(lo, p, hi, **bad)
    for args in ((lo[:2], p, hi), (lo, p, hi[:2]), (lo.float(), p, hi), (lo, p[:, :2], hi), (lo, (p * 255).to(torch.uint8), hi), (lo, p, hi.float())):
        with pytest.raises(ValueError):
            ge.guided_upsample(*args)


@gpu
def test_refuses_invalid_arguments_before_touching_the_device():
    """The host test's cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill."""
    from genpercept_amd import engine as ge
    from genpercept_amd import guided as gd
    lib = ge.load_library()
    b, c, h, w, H, W = 2, 1, 24, 40, 96, 160
    lo, p, hi = inputs("random blocks", b, c, h, w, H, W, 33)
    lo_d, p_d, hi_d = torch.from_numpy(lo).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(hi).cuda()
    out = torch.full((b, c, H, W), -7.0, device="cuda")
    need = int(lib.gp_guided_upsample_workspace(b, c, h, w))
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = dict(guide_lo=lo_d.data_ptr(), pred=p_d.data_ptr(), C=c, guide=hi_d.data_ptr(), B=b, h=h, w=w, H=H, W=W, r=4, eps=1e-4, out=out.data_ptr(),
              ws=ws.data_ptr(), nbytes=need)
    assert_refused_with_real_buffers(call_guided, lib, ok, invalid_cases(ok, int(lib.gp_guided_upsample_workspace(1, c, h, w))))
    assert bool((out == -7.0).all() and (ws == 0x5A).all())
    assert call_guided(lib, ok) == 0                                 # ... and the valid set goes through
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(b):
        assert same_bits(got[i], gd.guided_upsample(lo[i], p[i], hi[i], 4, 1e-4))


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_refine_with_the_pipeline(tiny_weights, tmp_path, monkeypatch):
    """Three 96 x 128 images at processing_res = 48 (a 32 x 48 map -> 96 x 128), one 64 x 64 image at processing_res = 0 (the plain guided
    filter), at 48 (48 x 48: the very bytes the model saw are the guide) and at 96 (the processing size exceeds the input: resize first, filter
    at the input size): `predict_batch_device(..., refine=...)` ==
    guided.py on the host applied to engine.preprocess's bytes and the raw prediction, bit for bit; without `refine` the result is the same
    before and after; the cutouts are those of the refined alpha; `run_cutouts` and `run_inference` write those bytes; float images and
    match_input_res=False are refused."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import engine as ge
    from genpercept_amd import foreground as fgh
    from genpercept_amd import guided as gd
    from genpercept_amd import infer_eval as ie
    from genpercept_amd.image_util import resize_max_res, resize_to
    tw = tiny_weights
    g = torch.Generator().manual_seed(49)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype=torch.bfloat16)
    pipe.to("cuda")
    base, out, npy, ev0, ev1, ev2 = (str(tmp_path / d) for d in ("data", "out", "npy", "ev0", "ev1", "ev2"))
    samples, images, sizes = [], [], [(96, 128), (96, 128), (96, 128), (64, 64)]
    for i, (h, w) in enumerate(sizes):
        for sub in ("im", "gt"):
            os.makedirs(os.path.join(base, "set0", sub), exist_ok=True)
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : w // 3 + 10 * i] //= 2
        Image.fromarray(rgb.numpy()).save(os.path.join(base, "set0", "im", f"{i:04d}.png"))
        xx = np.arange(w)[None].repeat(h, 0)
        Image.fromarray(np.clip((xx - (w // 3 + 10 * i)) * 6 + 128, 0, 255).astype(np.uint8)).save(os.path.join(base, "set0", "gt", f"{i:04d}.png"))
        samples.append([f"set0/im/{i:04d}.png", f"set0/gt/{i:04d}.png"])
        images.append(rgb.permute(2, 0, 1).contiguous())
    batch, single = torch.stack(images[:3]), images[3][None]
    try:
        before = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=ev0, batch_size=3, processing_res=48)
        # ---- 96 x 128 at processing_res = 48, one and three channels: the processing size is 36 x 48 and the model's map 32 x 48 (the latent
        #      grid rounds 36 down), so the guide at the small size is the image on the map's grid
        lo = ge.preprocess(batch.cuda(), (32, 48), "bilinear")
        assert lo.dtype == torch.uint8 and tuple(lo.shape) == (3, 3, 32, 48)
        lo = lo.cpu().numpy()
        refined = {}
        for mode, refine, kw in (("matting", True, dict(radius=4, eps=1e-4)), ("normal", dict(radius=2, eps=1e-3), dict(radius=2, eps=1e-3))):
            plain = pipe.predict_batch_device(batch, mode, processing_res=48)
            raw = pipe.predict_batch_device(batch, mode, processing_res=48, match_input_res=False)
            got = pipe.predict_batch_device(batch, mode, processing_res=48, refine=refine)
            c = 1 if mode == "matting" else 3
            assert tuple(raw.shape) == (3, c, 32, 48) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, c, 96, 128)
            assert torch.equal(bits(pipe.predict_batch_device(batch, mode, processing_res=48)), bits(plain))
            raw_np, got_np = raw.cpu().numpy(), got.cpu().numpy()
            assert len(np.unique(raw_np)) > 16
            for i in range(3):
                want = gd.guided_upsample(lo[i], raw_np[i], batch[i].numpy(), **kw)
                assert same_bits(got_np[i], np.clip(want, 0.0, 1.0)), (mode, i)
            assert not torch.equal(bits(got), bits(plain))
            refined[mode] = got
        # ---- 64 x 64 at processing_res = 48: the map has the processing size, the guide is what the model saw
        raw = pipe.predict_batch_device(single, "matting", processing_res=48, match_input_res=False)
        got = pipe.predict_batch_device(single, "matting", processing_res=48, refine=True)
        lo1 = ge.preprocess(single.cuda(), (48, 48), "bilinear").cpu().numpy()
        assert tuple(raw.shape) == (1, 1, 48, 48) and tuple(got.shape) == (1, 1, 64, 64)
        assert same_bits(got.cpu().numpy()[0], gd.guided_upsample(lo1[0], raw.cpu().numpy()[0], single[0].numpy()))
        # ---- the plain guided filter (h = H), and a processing size above the input
        for res in (0, 96):
            plain = pipe.predict_batch_device(single, "matting", processing_res=res)
            got = pipe.predict_batch_device(single, "matting", processing_res=res, refine=True)
            assert tuple(plain.shape) == tuple(got.shape) == (1, 1, 64, 64)
            assert same_bits(got.cpu().numpy()[0], gd.guided_upsample(single[0].numpy(), plain.cpu().numpy()[0], single[0].numpy())), res
            assert torch.equal(bits(pipe.predict_batch_device(single, "matting", processing_res=res)), bits(plain))
        # ---- __call__ and infer_batch, on the device route and on the host route
        outs = pipe.infer_batch(batch, "matting", processing_res=48, color_map=None, refine=True)
        for i in range(3):
            assert same_bits(outs[i].pred_np, refined["matting"][i, 0].cpu().numpy())
        one = pipe(Image.open(os.path.join(base, samples[3][0])), processing_res=0, color_map=None, mode="matting", refine=dict(eps=1e-2))
        want = pipe.predict_batch_device(single, "matting", processing_res=0, refine=dict(eps=1e-2))
        assert same_bits(one.pred_np, want[0, 0].cpu().numpy())
        monkeypatch.setenv("GENPERCEPT_HOST_PREPOST", "1")
        raw_h = pipe.infer_batch(batch, "matting", processing_res=48, match_input_res=False, color_map=None)
        outs_h = pipe.infer_batch(batch, "matting", processing_res=48, color_map=None, refine=True)
        assert raw_h[0].pred_np.shape == (32, 48) and tuple(resize_max_res(batch, 48, "bilinear").shape[-2:]) == (36, 48)
        lo_h = resize_to(batch, (32, 48), "bilinear").numpy()
        for i in range(3):
            assert same_bits(outs_h[i].pred_np, gd.guided_upsample(lo_h[i], raw_h[i].pred_np[None], batch[i].numpy())[0])
        with pytest.raises(ValueError):
            pipe.infer_batch(batch.float(), "matting", processing_res=48, color_map=None, refine=True)
        monkeypatch.delenv("GENPERCEPT_HOST_PREPOST")
        # ---- cutouts under the refined alpha
        rgba, alpha = pipe.cutout_batch_device(batch, "matting", processing_res=48, refine=True)
        assert torch.equal(bits(alpha), bits(refined["matting"]))
        want_rgba = [fgh.cutout_rgba(batch[i].numpy(), alpha[i, 0].cpu().numpy()) for i in range(3)]
        for i in range(3):
            assert np.array_equal(rgba[i].cpu().numpy(), want_rgba[i])
        rgba1, _ = pipe.cutout_batch_device(single, "matting", processing_res=48, refine=True)
        want_rgba.append(rgba1[0].cpu().numpy())
        plain_rgba, _ = pipe.cutout_batch_device(batch, "matting", processing_res=48)
        assert not torch.equal(plain_rgba, rgba)
        written = ie.run_cutouts(pipe, base, samples, out, ie.FileNameMode.id, "matting", 3, processing_res=48, refine=True)
        assert written == [os.path.join(out, "set0", "im", f"pred_{i:04d}.png") for i in range(4)]
        for path, ref in zip(written, want_rgba):
            im = Image.open(path)
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), ref)
        saved = ie.run_inference(pipe, base, samples[:3], npy, ie.FileNameMode.id, "matting", processing_res=48, batch_size=3, refine=True)
        for i, path in enumerate(saved):
            assert same_bits(np.load(path), refined["matting"][i, 0].cpu().numpy())
        # ---- what refine does not take
        for bad in (dict(refine=True, match_input_res=False), dict(refine="yes"), dict(refine=dict(radius=33)), dict(refine=dict(eps=0.0)),
                    dict(refine=dict(r=4))):
            with pytest.raises(ValueError):
                pipe.predict_batch_device(batch, "matting", processing_res=48, **bad)
        with pytest.raises(ValueError):
            pipe.predict_batch_device(batch.float(), "matting", processing_res=48, refine=True)
        with pytest.raises(ValueError):
            pipe.cutout_batch_device(batch, "matting", processing_res=48, refine=True, match_input_res=False)
        with pytest.raises(ValueError):
            pipe(batch[:1].float(), processing_res=48, color_map=None, mode="matting", refine=True)
        # ---- the dataset loop with and without it: the same columns, and the plain result as before
        with_refine = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=ev1, batch_size=3, processing_res=48, refine=True)
        after = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=ev2, batch_size=3, processing_res=48)
        assert list(before) == list(after) == list(with_refine)
        assert all(np.float64(before[k]).tobytes() == np.float64(after[k]).tobytes() for k in before)
        assert any(np.float64(before[k]).tobytes() != np.float64(with_refine[k]).tobytes() for k in before)
        assert sorted(os.listdir(ev1)) == sorted(os.listdir(ev2))
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
