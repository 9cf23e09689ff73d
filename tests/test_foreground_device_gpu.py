"""Matting cutouts on the device (gp_foreground): fg, bg, rgba and comp BIT-EQUAL to the host route genpercept_amd/foreground.py (itself
pinned to plain loops and to a CPU build of the kernels' update text in tests/test_foreground_host.py), over shapes that take every path of
the two kernels (one pixel, one row, coarse kernel only, the first level kernel with a one-pixel overhang, a side that reaches 1 early,
several tiles that are multiples of nothing), hand-made inputs, every n_big, n_small 0 and 10, two (reg, gw) pairs, pointers one byte into
their buffers; float alpha; batch independence; both kinds of background; partial outputs; the argument checks with real buffers around
them; the pipeline and the dataset loop at tiny widths.  There is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from post_support import assert_refused_with_real_buffers, tiny_weights_dict, unaligned  # noqa: E402
from test_foreground_host import call_foreground, invalid_cases, random_inputs, same_bits  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 7, 5), (2, 32, 32), (1, 33, 32), (3, 64, 65), (1, 37, 300), (1, 257, 131)]
OUTPUTS = ["fg", "bg", "rgba", "comp"]
DEFAULT = dict(reg=1e-5, gw=1.0, n_small=10, n_big=2)
GRID = [dict(DEFAULT, n_big=nb, n_small=ns) for nb in (1, 2, 4) for ns in (0, 10)] + [dict(reg=2e-3, gw=30.0, n_small=10, n_big=2)]
FEW = [dict(DEFAULT), dict(reg=2e-3, gw=30.0, n_small=0, n_big=4), dict(DEFAULT, n_big=1), dict(DEFAULT, n_big=4)]


def inputs(b, h, w, seed):
    """name -> (image uint8 [B, 3, H, W], alpha uint8 [B, H, W])"""
    rng = np.random.RandomState(seed)
    rnd = [random_inputs(rng, h, w) for _ in range(b)]
    img = np.stack([r[0] for r in rnd])
    yy, xx = np.mgrid[0:h, 0:w]
    full = lambda v: np.full((b, h, w), v, np.uint8)
    single = np.zeros((b, h, w), np.uint8)
    single[:, h // 2, (2 * w) // 3] = 255
    ramp = np.broadcast_to(np.clip((xx + yy) * 255.0 / max(h + w - 2, 1), 0, 255).astype(np.uint8), (b, h, w)).copy()
    checker = np.broadcast_to(((yy + xx) % 2 * 255).astype(np.uint8), (b, h, w)).copy()
    return {"random blocks": (img, np.stack([r[1] for r in rnd])), "all 0": (np.zeros_like(img), full(0)), "all 255": (np.full_like(img, 255), full(255)),
            "image 0, alpha 255": (np.zeros_like(img), full(255)), "checkerboard": (img, checker), "soft ramp": (img, ramp), "one opaque pixel": (img, single)}


def host(img, a8, new, kw):
    """The four outputs of one image by the host route."""
    from genpercept_amd import foreground as fgh
    F, B = fgh.estimate_foreground(img, a8, **kw)
    a = a8.astype(np.float32) / np.float32(255.0)
    N = np.broadcast_to(new.reshape(3, 1, 1) if new.ndim == 1 else new, img.shape).astype(np.float32) / np.float32(255.0)
    rgba = np.concatenate([fgh.to_bytes(F), a8[None]], 0).transpose(1, 2, 0)
    return dict(fg=F, bg=B, rgba=rgba, comp=fgh.to_bytes((a * F) + ((np.float32(1.0) - a) * N)))


def equal(got, want):
    return same_bits(got, want) if want.dtype == np.float32 else (got.dtype == want.dtype and np.array_equal(got, want))


def check(img, a8, new, img_d, alpha_d, new_d, kw, what):
    from genpercept_amd import engine as ge
    got = {k: v.cpu().numpy() for k, v in ge.foreground(img_d, alpha_d, new_d, want=OUTPUTS, **kw).items()}
    assert list(got) == OUTPUTS
    for i in range(img.shape[0]):
        want = host(img[i], a8[i], new if new.ndim == 1 else new[i], kw)
        for k in OUTPUTS:
            assert equal(got[k][i], want[k]), (what, i, kw, k, int((got[k][i] != want[k]).sum()))


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_outputs_equal_the_host_route(shape):
    b, h, w = shape
    rng = np.random.RandomState(17 + h)
    new = rng.randint(0, 256, (b, 3, h, w)).astype(np.uint8)
    new_d = unaligned(new)
    n = 0
    for name, (img, a8) in inputs(b, h, w, 4000 + h).items():
        img_d, a_d = unaligned(img), unaligned(a8)
        assert img_d.data_ptr() % 2 == 1 and a_d.data_ptr() % 2 == 1 and new_d.data_ptr() % 2 == 1
        if name == "random blocks":
            for kw in GRID:
                check(img, a8, new, img_d, a_d, new_d, kw, name)
        else:
            for kw in (FEW[0], FEW[1 + n % 3]):
                check(img, a8, new, img_d, a_d, new_d, kw, name)
            n += 1


@gpu
@pytest.mark.parametrize("shape", [(3, 64, 65), (1, 257, 131)], ids=lambda s: "x".join(map(str, s)))
def test_float_alpha_is_quantised_first(shape):
    """Values on and around the k / 255 edges (and NaN, values outside [0, 1]) give the outputs of `quantize_mask`'s bytes."""
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    b, h, w = shape
    rng = np.random.RandomState(78)
    rnd = [random_inputs(rng, h, w) for _ in range(b)]
    img = np.stack([r[0] for r in rnd])
    f = np.stack([r[1] for r in rnd]).astype(np.float32) / np.float32(255.0)
    f = np.where(rng.rand(b, h, w) < 0.3, np.nextafter(f, np.float32(-1.0)), np.where(rng.rand(b, h, w) < 0.3, np.nextafter(f, np.float32(2.0)), f))
    f = f.astype(np.float32)
    f[:, 0, 0], f[:, -1, -1], f[:, h // 2, w // 2] = np.nan, 1.5, -0.25
    q = np.stack([em.quantize_mask(x) for x in f])
    assert len(np.unique(q)) > 100
    new = np.array([12, 130, 250], np.uint8)
    img_d, f_d = unaligned(img), unaligned(f)
    check(img, q, new, img_d, f_d, new, DEFAULT, "float")
    by_bytes = ge.foreground(img_d, torch.from_numpy(q).cuda(), new, want=OUTPUTS)
    for k, v in ge.foreground(img_d, f_d[:, None], new, want=OUTPUTS).items():
        assert torch.equal(v.view(torch.uint8), by_bytes[k].view(torch.uint8))
    for dt in (torch.float16, torch.float64):                        # other float types go through float32, like eval_mask
        x = torch.from_numpy(q.astype(np.float32) / 255.0 + 0.001).cuda()
        assert torch.equal(ge.cutout(img_d, x.to(dt)), ge.cutout(img_d, x.to(dt).to(torch.float32)))


@gpu
def test_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    rng = np.random.RandomState(6)
    for h, w in ((64, 65), (257, 131)):
        rnd = [random_inputs(rng, h, w) for _ in range(3)]
        img, a = torch.from_numpy(np.stack([r[0] for r in rnd])).cuda(), torch.from_numpy(np.stack([r[1] for r in rnd])).cuda()
        new = torch.from_numpy(rng.randint(0, 256, (3, 3, h, w)).astype(np.uint8)).cuda()
        whole, again = ge.foreground(img, a, new, want=OUTPUTS), ge.foreground(img, a, new, want=OUTPUTS)
        for i in range(3):
            one = ge.foreground(img[i], a[i], new[i], want=OUTPUTS)
            for k in OUTPUTS:
                assert torch.equal(one[k][0].view(torch.uint8), whole[k][i].view(torch.uint8)) and torch.equal(again[k].view(torch.uint8), whole[k].view(torch.uint8))
        F, B = ge.estimate_foreground(img, a)
        assert torch.equal(F.view(torch.int32), whole["fg"].view(torch.int32)) and torch.equal(B.view(torch.int32), whole["bg"].view(torch.int32))
        assert torch.equal(ge.cutout(img, a), whole["rgba"]) and torch.equal(ge.cutout(img, a, new), whole["comp"])
    for bad in (dict(want=()), dict(want=("fg", "edge")), dict(want=("comp",)), dict(reg=1e-7), dict(n_big=5), dict(n_small=65), dict(gw=-1.0)):
        with pytest.raises(ValueError):
            ge.foreground(img, a, **bad)
    with pytest.raises(ValueError):
        ge.foreground(img, a[:2])
    with pytest.raises(ValueError):
        ge.foreground(img.float(), a)
    with pytest.raises(ValueError):
        ge.cutout(img, a, new[:, :, :-1])


@gpu
def test_background_image_and_single_colour():
    from genpercept_amd import engine as ge
    from genpercept_amd import foreground as fgh
    rng = np.random.RandomState(8)
    b, h, w = 2, 45, 70
    rnd = [random_inputs(rng, h, w) for _ in range(b)]
    img, a8 = np.stack([r[0] for r in rnd]), np.stack([r[1] for r in rnd])
    img_d, a_d = torch.from_numpy(img).cuda(), torch.from_numpy(a8).cuda()
    new = rng.randint(0, 256, (b, 3, h, w)).astype(np.uint8)
    got = ge.cutout(img_d, a_d, torch.from_numpy(new).cuda()).cpu().numpy()
    for i in range(b):
        assert np.array_equal(got[i], fgh.composite(img[i], a8[i], new[i]))
    for colour in ((0, 0, 0), (255, 255, 255), (1, 128, 254), np.array([200, 3, 77], np.uint8), torch.tensor([9, 99, 199], dtype=torch.uint8)):
        got = ge.cutout(img_d, a_d, colour).cpu().numpy()
        for i in range(b):
            assert np.array_equal(got[i], fgh.composite(img[i], a8[i], np.asarray(colour, dtype=np.uint8)))
    got = ge.cutout(img_d, a_d).cpu().numpy()
    for i in range(b):
        assert np.array_equal(got[i], fgh.cutout_rgba(img[i], a8[i]))


def _device_call_args(b, h, w, comp_offset=0):
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    d = torch.device("cuda", 0)
    rng = np.random.RandomState(12)
    rnd = [random_inputs(rng, h, w) for _ in range(b)]
    t = dict(img=torch.from_numpy(np.stack([r[0] for r in rnd])).to(d), a=torch.from_numpy(np.stack([r[1] for r in rnd])).to(d),
             fg=torch.full((b, 3, h, w), -7.0, device=d), bg=torch.full((b, 3, h, w), -7.0, device=d),
             rgba=torch.full((b, h, w, 4), 99, dtype=torch.uint8, device=d), comp=torch.full((b * 3 * h * w + 8,), 99, dtype=torch.uint8, device=d),
             af=torch.rand(b, h, w, device=d))
    need = int(lib.gp_foreground_workspace(b, h, w))
    t["ws"] = torch.full((need,), 0x5A, dtype=torch.uint8, device=d)
    ok = dict(image=t["img"].data_ptr(), alpha=t["a"].data_ptr(), u8=1, B=b, H=h, W=w, reg=1e-5, gw=1.0, n_small=10, n_big=2, new_bg=None, rgb=0x102030,
              fg=t["fg"].data_ptr(), bg=t["bg"].data_ptr(), rgba=t["rgba"].data_ptr(), comp=t["comp"].data_ptr() + comp_offset, ws=t["ws"].data_ptr(),
              nbytes=need)
    return lib, t, ok


@gpu
def test_partial_outputs_leave_the_other_buffers_untouched():
    from genpercept_amd import foreground as fgh
    b, h, w = 2, 70, 45
    lib, t, ok = _device_call_args(b, h, w, comp_offset=1)                  # the composite starts one byte into its buffer
    img, a8 = t["img"].cpu().numpy(), t["a"].cpu().numpy()
    want = [host(img[i], a8[i], np.array([0x10, 0x20, 0x30], np.uint8), dict(DEFAULT)) for i in range(b)]
    fills = dict(fg=-7.0, bg=-7.0, rgba=99, comp=99)
    for keep in (("rgba",), ("comp",), ("fg",), ("bg", "comp"), ("fg", "bg", "rgba", "comp")):
        for k in OUTPUTS:
            t[k].fill_(fills[k])
        assert call_foreground(lib, dict(ok, **{k: None for k in OUTPUTS if k not in keep})) == 0
        torch.cuda.synchronize()
        for k in OUTPUTS:
            if k not in keep:
                assert bool((t[k] == fills[k]).all()), (keep, k)
                continue
            got = t[k].cpu().numpy()
            if k == "comp":
                assert got[0] == 99 and (got[1 + b * 3 * h * w:] == 99).all()
                got = got[1:1 + b * 3 * h * w].reshape(b, 3, h, w)
            for i in range(b):
                assert equal(got[i], want[i][k]), (keep, k, i)


@gpu
def test_refuses_invalid_arguments_before_touching_the_device():
    """The host test's cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill."""
    lib, t, ok = _device_call_args(2, 40, 40)
    cases = [c for c in invalid_cases(ok, int(lib.gp_foreground_workspace(1, 40, 40))) if "u8" not in c or "alpha" not in c]
    cases.append(dict(u8=0, alpha=t["af"].data_ptr() + 2))
    assert_refused_with_real_buffers(call_foreground, lib, ok, cases)
    assert bool((t["fg"] == -7.0).all() and (t["bg"] == -7.0).all() and (t["rgba"] == 99).all() and (t["comp"] == 99).all() and (t["ws"] == 0x5A).all())
    assert call_foreground(lib, ok) == 0                             # ... and the valid set goes through
    torch.cuda.synchronize()
    assert not bool((t["fg"] == -7.0).any()) and not bool((t["rgba"][..., :3] == 99).all())


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_cutouts_with_the_pipeline(tiny_weights, tmp_path):
    """`cutout_batch_device` on three 96 x 128 images and one 64 x 64 == foreground.cutout_rgba on the host applied to the same images and to the
    alpha `predict_batch_device` returns, bit for bit; `run_cutouts` writes one RGBA png per sample with those bytes (an RGB composite with a
    background); `predict_batch_device` and `infer_and_evaluate_masks` return what they return without any cutout made in between."""
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import foreground as fgh
    from genpercept_amd import infer_eval as ie
    tw = tiny_weights
    g = torch.Generator().manual_seed(48)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype=torch.bfloat16)
    pipe.to("cuda")
    base, out, out_bg, ev0, ev1 = (str(tmp_path / d) for d in ("data", "out", "out_bg", "ev0", "ev1"))
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
    try:
        before = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=ev0, batch_size=2, processing_res=0)
        want = []
        for batch in (torch.stack(images[:3]), images[3][None]):
            alpha0 = pipe.predict_batch_device(batch, "matting", processing_res=0)
            rgba, alpha = pipe.cutout_batch_device(batch, "matting", processing_res=0)
            assert rgba.is_cuda and alpha.is_cuda and rgba.dtype == torch.uint8 and tuple(rgba.shape) == (batch.shape[0],) + tuple(batch.shape[2:]) + (4,)
            assert alpha.dtype == torch.float32 and tuple(alpha.shape) == (batch.shape[0], 1) + tuple(batch.shape[2:])
            assert torch.equal(alpha.view(torch.int32), alpha0.view(torch.int32))
            assert torch.equal(pipe.predict_batch_device(batch, "matting", processing_res=0).view(torch.int32), alpha0.view(torch.int32))
            a_np, rgba_np = alpha.cpu().numpy(), rgba.cpu().numpy()
            assert len(np.unique(a_np)) > 16
            for i in range(batch.shape[0]):
                ref = fgh.cutout_rgba(batch[i].numpy(), a_np[i, 0])
                assert np.array_equal(rgba_np[i], ref)
                want.append(ref)
            comp, _ = pipe.cutout_batch_device(batch, "dis", (20, 40, 250), processing_res=0)
            a_dis = pipe.predict_batch_device(batch, "dis", processing_res=0).cpu().numpy()
            for i in range(batch.shape[0]):
                assert np.array_equal(comp[i].cpu().numpy(), fgh.composite(batch[i].numpy(), a_dis[i, 0], np.array([20, 40, 250], np.uint8)))
        one = pipe.cutout(Image.open(os.path.join(base, samples[3][0])), processing_res=0)
        assert one.mode == "RGBA" and np.array_equal(np.asarray(one), want[3])
        with pytest.raises(ValueError):
            pipe.cutout_batch_device(images[3][None], "depth", processing_res=0)
        # (batches of three, as above: the model's alpha of an image is not bitwise the same in every batch, the cutout of a given alpha is)
        written = ie.run_cutouts(pipe, base, samples, out, ie.FileNameMode.id, "matting", 3, processing_res=0)
        assert written == [os.path.join(out, "set0", "im", f"pred_{i:04d}.png") for i in range(4)]
        for path, ref in zip(written, want):
            im = Image.open(path)
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), ref)
        half = ie.run_cutouts(pipe, base, samples, out_bg, ie.FileNameMode.id, "matting", 2, 1, 2, background=(255, 255, 255), processing_res=0)
        assert [os.path.basename(p) for p in half] == ["pred_0002.png", "pred_0003.png"] and Image.open(half[0]).mode == "RGB"
        a2 = pipe.predict_batch_device(images[2][None], "matting", processing_res=0).cpu().numpy()[0, 0]
        assert np.array_equal(np.moveaxis(np.asarray(Image.open(half[0])), -1, 0), fgh.composite(images[2].numpy(), a2, np.array([255] * 3, np.uint8)))
        with pytest.raises(ValueError):
            ie.run_cutouts(pipe, base, samples, out, ie.FileNameMode.id, "normal")
        after = ie.infer_and_evaluate_masks(pipe, base, samples, "matting", output_dir=ev1, batch_size=2, processing_res=0)
        assert list(before) == list(after) and all(np.float64(before[k]).tobytes() == np.float64(after[k]).tobytes() for k in before)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
