"""The synthetic depth of field on the device (gp_lens_blur): the refocused bytes and the circle-of-confusion plane BIT-EQUAL to the host route
genpercept_amd/lens_blur.py (itself pinned to plain loops and to a CPU build of the kernel's arithmetic in tests/test_lens_blur_host.py), over
sizes that are multiples of nothing, radii up to 32 pixels (an apron larger than the image), both spaces, both table pairs, a parameter row
per image, a `sharp` mask and a sharp zone, a batch whose middle map is all NaN, a sharp tile next to a fully blurred one, tensors that start
four bytes into their buffers (the kernel allows it for every one); batch independence and repeatability; the parameter table's clamping;
the argument checks with real buffers around them; the pipeline and the dataset loop with `refine` and `tiles` at tiny widths.  There is no
tolerance in this file."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict  # noqa: E402
from test_lens_blur_host import all_tables, call_lens, invalid_cases, lens_args, random_case  # noqa: E402

gpu = pytest.mark.gpu

# B, H, W, max_radius, with a sharp mask and dz > 0
CASES = [(1, 17, 23, 2, False), (2, 40, 70, 8, False), (1, 33, 200, 32, False), (1, 64, 48, 5, True), (3, 16, 16, 32, False)]


batch_case = functools.partial(ps.batch_case, random_case)


def terms(b, max_radius, dz):
    """A different parameter row per image; the call's largest radius is max_radius."""
    k = np.arange(b)
    return dict(focus=(0.2 + 0.3 * k).tolist(), aperture=(4.0 * max_radius - 3.0 * k).tolist(), max_radius=(max_radius - 0.5 * k).tolist(),
                dof=(0.03 + 0.02 * k).tolist() if dz else 0.0)


def device_blur(image_d, pred_d, **kw):
    from genpercept_amd import engine as ge
    out, coc = ge.lens_blur(image_d, pred_d, want_coc=True, **kw)
    assert out.dtype == torch.uint8 and coc.dtype == torch.int16 and out.is_cuda and coc.is_cuda
    return out.cpu().numpy(), coc.cpu().numpy().view(np.uint16)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-r%d%s" % (s[:4] + ("-sharp" if s[4] else "",)))
def test_bytes_equal_the_host_route(case):
    from genpercept_amd import lens_blur as lb
    b, h, w, max_radius, pinned = case
    pred, image, sharp = batch_case(700 + h + w, b, h, w, middle_nan=b == 3)
    pred_d, image_d, sharp_d = offset4(pred), offset4(image), offset4(sharp)
    kw = terms(b, max_radius, pinned)
    rows = lb.lens_params(pred, "depth", **kw)
    assert len({tuple(r) for r in rows.tolist()}) == b and rows[:, 2].max() == 8 * max_radius      # a different row per image
    blurred = 0
    for space in lb.SPACES:
        for name, tables in all_tables().items():
            use = dict(kw, space=space, tables=tables)
            got, got_coc = device_blur(image_d, pred_d, sharp=sharp_d if pinned else None, **use)
            want, want_coc = lb.lens_blur(image, pred, sharp=sharp if pinned else None, want_coc=True, **use)
            assert same_bits(got_coc, want_coc) and same_bits(got, want), (case, space, name)
            blurred += int((want_coc > 3).sum())
            if b == 3:
                assert not want_coc[1].any() and same_bits(want[1], image[1])
    assert blurred > 0


@gpu
def test_a_sharp_tile_next_to_a_fully_blurred_one():
    """Everything left of column 75 -- no multiple of the tile's 32 -- is in focus, everything right of it at the full radius of 32 pixels, in
    front of it (the blur spreads left over sharp tiles, whose own largest c is 0) and behind it (it does not)."""
    from genpercept_amd import lens_blur as lb
    h, w, edge = 33, 200, 75
    image = np.random.RandomState(4).randint(0, 256, (1, 3, h, w)).astype(np.uint8)
    image_d = offset4(image)
    for left, right in ((0.9, 0.1), (0.1, 0.9)):
        pred = np.full((1, 1, h, w), left, np.float32)
        pred[..., edge:] = right
        kw = dict(focus=left, aperture=128.0, max_radius=32.0)
        got, got_coc = device_blur(image_d, offset4(pred), **kw)
        want, want_coc = lb.lens_blur(image, pred, want_coc=True, **kw)
        assert not want_coc[0, :, :edge].any() and (want_coc[0, :, edge:] == 256).all()
        assert same_bits(got_coc, want_coc) and same_bits(got, want), (left, right)
        spreads = not same_bits(want[0, :, :, :32], image[0, :, :, :32]) or not same_bits(want[0, :, :, 32:64], image[0, :, :, 32:64])
        assert same_bits(want[0, :, :, :edge - 32], image[0, :, :, :edge - 32])                   # out of reach
        assert spreads == (right < left) and (right > left or not same_bits(want[0, :, :, 43:64], image[0, :, :, 43:64]))


@gpu
def test_stable_batch_independent_and_focus_at():
    from genpercept_amd import engine as ge
    from genpercept_amd import lens_blur as lb
    for (b, h, w, max_radius), space in (((3, 40, 70, 8), "depth"), ((3, 33, 75, 20), "disparity")):
        pred, image, sharp = batch_case(21, b, h, w)
        pred_d, image_d, sharp_d = torch.from_numpy(pred).cuda(), torch.from_numpy(image).cuda(), torch.from_numpy(sharp).cuda()
        kw = terms(b, max_radius, True)
        whole, again = (device_blur(image_d, pred_d, sharp=sharp_d, space=space, **kw) for _ in range(2))
        assert same_bits(whole[0], again[0]) and same_bits(whole[1], again[1])
        for i in range(b):
            one = device_blur(image_d[i], pred_d[i], sharp=sharp_d[i:i + 1], space=space, **{k: (v[i] if isinstance(v, list) else v) for k, v in kw.items()})
            assert same_bits(one[0][0], whole[0][i]) and same_bits(one[1][0], whole[1][i]), i
        # without the coc plane the bytes are the same; float64 maps and boolean masks are taken too
        assert same_bits(ge.lens_blur(image_d, pred_d, sharp=sharp_d, space=space, **kw).cpu().numpy(), whole[0])
        assert same_bits(ge.lens_blur(image_d, pred_d.double()[:, 0], sharp=sharp_d != 0, space=space, **kw).cpu().numpy(), whole[0])
        # the focus taken from a pixel on the device is the focus of that pixel's value
        at = np.array([[5, 7], [w - 1, h - 1], [0, 3]])
        pred[2, 0, 3, 0] = np.nan                                                                 # (its nearness is 0)
        pred_d = torch.from_numpy(pred).cuda()
        rest = dict(aperture=kw["aperture"], max_radius=kw["max_radius"], space=space)
        got = ge.lens_blur(image_d, pred_d, focus_at=at, **rest).cpu().numpy()
        assert same_bits(got, lb.lens_blur(image, pred, focus_at=at, **rest))
        value = np.nan_to_num(pred[np.arange(b), 0, at[:, 1], at[:, 0]], nan=1.0 if space == "depth" else 0.0).clip(0, 1)
        assert same_bits(got, ge.lens_blur(image_d, pred_d, focus=value.tolist(), **rest).cpu().numpy())
        assert not same_bits(got, image)
    for bad in (dict(), dict(focus=0.5, focus_at=(1, 1)), dict(focus=1.5), dict(focus_at=(w, 0)), dict(focus_at=(0, h)), dict(focus=0.5, space="metric"),
                dict(focus=0.5, max_radius=33.0), dict(focus=0.5, aperture=-1.0), dict(focus=0.5, dof=2.0), dict(focus=[0.5, 0.5]),
                dict(focus=0.5, sharp=sharp_d[:, :5]), dict(focus=0.5, tables=(np.zeros(256, np.uint16), np.zeros(4096, np.uint8)))):
        with pytest.raises(ValueError):
            ge.lens_blur(image_d, pred_d, **bad)
    for bad in (dict(image=image_d.float()), dict(image=image_d[:2]), dict(pred=(pred_d * 255).to(torch.uint8)), dict(image=image_d[:, :2])):
        with pytest.raises(ValueError):
            ge.lens_blur(**dict(dict(image=image_d, pred=pred_d, focus=0.5), **bad))


@gpu
def test_invalid_arguments_with_real_buffers_and_the_clamped_table():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill.  Then the
    valid set goes through with outputs that start four bytes into their buffers, with and without the coc plane; and a parameter table with
    values outside their ranges gives what the host route gives for the values clamped into them."""
    from genpercept_amd import engine as ge
    from genpercept_amd import lens_blur as lb
    lib = ge.load_library()
    b, h, w = 2, 40, 70
    pred, image, sharp = batch_case(33, b, h, w)
    pred_d, image_d, sharp_d = offset4(pred), offset4(image), offset4(sharp)
    tables = lb.srgb_tables()
    to_lin_d, from_lin_d = offset4(tables[0].view(np.int16)), offset4(tables[1])
    rows = np.array([[20000, 3000, 64, 500], [50000, 800, 37, 0]], np.int32)
    params_d = offset4(rows)

    def fresh():
        return dict(out=offset4(np.full((b, 3, h, w), 0x5A, np.uint8)), coc=offset4(np.full((b, h, w), 0x5A5A, np.int16)))

    bufs = fresh()
    ok = lens_args(b, h, w, image=image_d.data_ptr(), pred=pred_d.data_ptr(), sharp=sharp_d.data_ptr(), params=params_d.data_ptr(),
                   to_lin=to_lin_d.data_ptr(), from_lin=from_lin_d.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()})
    untouched = assert_refused_with_real_buffers(call_lens, lib, ok, invalid_cases(ok), bufs, fresh)
    want, want_coc = lb.lens_blur_params(image, pred, rows, "depth", sharp, tables, want_coc=True)
    for with_coc in (True, False):
        bufs = fresh()
        assert call_lens(lib, dict(ok, out=bufs["out"].data_ptr(), coc=bufs["coc"].data_ptr() if with_coc else None)) == 0
        torch.cuda.synchronize()
        assert same_bits(bufs["out"].cpu().numpy(), want)
        assert same_bits(bufs["coc"].cpu().numpy().view(np.uint16), want_coc) if with_coc else torch.equal(bufs["coc"], untouched["coc"])
    # max_c8 sizes the apron and caps cmax8; the other values are clamped into their ranges
    wild_d = offset4(np.array([[70000, 40000, 300, -5], [-3, 2000, 64, 70000]], np.int32))
    bufs = fresh()
    assert call_lens(lib, dict(ok, params=wild_d.data_ptr(), max_c8=40, sharp=None, **{k: v.data_ptr() for k, v in bufs.items()})) == 0
    torch.cuda.synchronize()
    want, want_coc = lb.lens_blur_params(image, pred, [[65535, 32768, 40, 0], [0, 2000, 40, 65535]], "depth", None, tables, want_coc=True)
    assert same_bits(bufs["out"].cpu().numpy(), want) and same_bits(bufs["coc"].cpu().numpy().view(np.uint16), want_coc)
    assert want_coc[0].max() == 40 and not want_coc[1].any()


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_refocus_with_the_pipeline(tiny_weights, tmp_path):
    """Three 96 x 128 images at processing_res = 48: `refocus_batch_device` == lens_blur.py on the host applied to what `predict_batch_device`
    returns, bit for bit, for depth and disparity, plain, with `refine`, with `tiles` and with both; `focus_at` equals the same focus passed
    as a value; `refocus` gives one image; `run_refocus` writes those bytes; what the entry does not take is refused."""
    from PIL import Image
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import lens_blur as lb
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    tiles = dict(size=48, overlap=16, batch=4)
    sharp = torch.zeros((3, 96, 128), dtype=torch.uint8)
    sharp[:, 20:50, 30:70] = 255
    try:
        done = {}
        wide = dict(focus_at=(64, 48), aperture=200.0, max_radius=6.0)
        own = dict(focus=[0.2, 0.5, 0.8], aperture=[300.0, 150.0, 100.0], max_radius=[3.0, 9.5, 5.0], dof=0.01, sharp=sharp, tables=lb.identity_tables())
        extras = dict(plain={}, refine=dict(refine=True), tiles=dict(tiles=tiles), both=dict(refine=dict(radius=2), tiles=tiles))
        for mode, name, settings in (("depth", "plain", (wide, own)), ("depth", "refine", (own,)), ("depth", "tiles", (wide,)), ("depth", "both", (own,)),
                                     ("disparity", "plain", (wide, own)), ("disparity", "tiles", (own,))):
            extra = extras[name]
            pred = pipe.predict_batch_device(batch, mode, processing_res=48, **extra).cpu().numpy()
            for kw in settings:
                got = pipe.refocus_batch_device(batch, mode, processing_res=48, **kw, **extra)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 3, 96, 128)
                host = dict(kw, sharp=sharp.numpy()) if "sharp" in kw else kw
                want = lb.lens_blur(batch.numpy(), pred, space=mode, **host)
                assert same_bits(got.cpu().numpy(), want), (mode, name, sorted(kw))
                assert not same_bits(want, batch.numpy())
                done[mode, name, kw is wide] = want
            if name == "plain":
                value = pred[:, 0, 48, 64].clip(0, 1).tolist()
                got = pipe.refocus_batch_device(batch, mode, focus=value, aperture=200.0, max_radius=6.0, processing_res=48)
                assert same_bits(got.cpu().numpy(), done[mode, name, True])
        assert not same_bits(done["depth", "plain", True], done["depth", "tiles", True])
        one = pipe.refocus(Image.open(os.path.join(data, samples[1][0])), processing_res=48, **wide)
        lone = lb.lens_blur(batch[1:2].numpy(), pipe.predict_batch_device(batch[1:2], "depth", processing_res=48).cpu().numpy(), **wide)
        assert one.mode == "RGB" and same_bits(np.moveaxis(np.asarray(one), -1, 0), lone[0])
        for kw, key in ((dict(), ("depth", "plain", True)), (dict(tiles=tiles), ("depth", "tiles", True))):
            written = ie.run_refocus(pipe, data, samples, str(tmp_path / ("png" + "-".join(kw))), ie.FileNameMode.id, "depth", 3, processing_res=48, **wide, **kw)
            assert len(written) == 3 and all(p.endswith(".png") for p in written)
            for i, path in enumerate(written):
                assert same_bits(np.moveaxis(np.asarray(Image.open(path)), -1, 0), done[key][i])
        for bad in (dict(mode="matting"), dict(mode="normal"), dict(focus=None), dict(focus_at=(1, 1)), dict(focus=2.0), dict(max_radius=40.0),
                    dict(match_input_res=False), dict(tiles="yes"), dict(focus=None, focus_at=(128, 0)), dict(sharp=sharp[:, :5])):
            with pytest.raises(ValueError):
                pipe.refocus_batch_device(batch, **dict(dict(focus=0.5, processing_res=48), **bad))
        with pytest.raises(ValueError):
            pipe.refocus_batch_device(batch.float(), focus=0.5, processing_res=48)
        with pytest.raises(ValueError):
            ie.run_refocus(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "matting", focus=0.5, processing_res=48)
        with pytest.raises(ValueError):
            ie.run_refocus(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", focus=[0.5, 0.5, 0.5], processing_res=48)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
