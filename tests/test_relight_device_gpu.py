"""The relighting on the device (gp_relight): the relit bytes and the shadow plane BIT-EQUAL to the host route genpercept_amd/relight.py (itself
pinned to plain loops and to a CPU build of the kernel's arithmetic in tests/test_relight_host.py), over sizes that are multiples of nothing,
marches up to 64 steps (an apron larger than the image), both spaces and encodings, 1 and 8 lights from every quadrant, a batch whose
middle map is all NaN, occluder and receiver in different tiles, a ramp on which no march ends early, tensors that start four bytes into
their buffers; batch independence and repeatability; the argument checks with real buffers around them; the pipeline and the dataset loop
with `refine` and `tiles` at tiny widths.  There is no tolerance in this file."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict  # noqa: E402
from test_relight_host import (all_tables, call_relight, facing, invalid_cases, light_terms, lights_array, random_case, relight_args, stored,  # noqa: E402
                               valid_rows)

gpu = pytest.mark.gpu

# B, H, W, max_reach
CASES = [(1, 17, 23, 2), (2, 40, 70, 8), (1, 33, 200, 64), (1, 64, 48, 5), (3, 16, 16, 64)]

batch_case = functools.partial(ps.batch_case, random_case)


def device_relight(image_d, normal_d, pred_d, weight_d, **kw):
    from genpercept_amd import engine as ge
    out, shadow = ge.relight(image_d, normal_d, pred_d, weight_d, want_shadow=True, **kw)
    assert out.dtype == torch.uint8 and shadow.dtype == torch.uint8 and out.is_cuda and shadow.is_cuda
    return out.cpu().numpy(), shadow.cpu().numpy()


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-r%d" % s)
def test_bytes_equal_the_host_route(case):
    from genpercept_amd import relight as rl
    b, h, w, max_reach = case
    pred, image, normal, weight = batch_case(900 + h + w, b, h, w, middle_nan=b == 3)
    raw = stored(normal, False, (False,) * 3)
    pred_d, image_d, weight_d, normal_d, raw_d = offset4(pred), offset4(image), offset4(weight), offset4(normal), offset4(raw)
    shadowed, k = 0, 0
    for space in rl.SPACES:
        for encoded in (True, False):
            for n_lights in (1, 8):
                k += 1
                rows = rl.relight_lights(light_terms(n_lights, max_reach), ambient=(0.1 * k, 0.3, 0.5), relief=16.0 + 4.0 * k)
                assert rows[:-1, 19].max() == max_reach
                use_pred, use_weight = k != 3, k % 3 != 0
                kw = dict(lights=rows, encoded=encoded, space=space, tables=list(all_tables().values())[k % 2])
                got, got_sh = device_relight(image_d, normal_d if encoded else raw_d, pred_d if use_pred else None, weight_d if use_weight else None, **kw)
                rows_kw = dict(kw, rows=kw["lights"])
                del rows_kw["lights"]
                want, want_sh = rl.relight_rows(image, normal if encoded else raw, pred if use_pred else None, weight if use_weight else None,
                                                want_shadow=True, **rows_kw)
                assert same_bits(got_sh, want_sh) and same_bits(got, want), (case, space, encoded, n_lights)
                assert want_sh.any() == use_pred and not same_bits(want, image)
                shadowed += int(want_sh.any())
                if b == 3 and use_pred:
                    assert not want_sh[1].any()
    assert shadowed == 7
    # the user's terms give the same call
    terms = dict(lights=light_terms(3, max_reach), ambient=0.2, relief=20.0, flip=(True, False, True))
    flipped = stored(normal, True, terms["flip"])
    got, got_sh = device_relight(image_d, offset4(flipped), pred_d, weight_d, **terms)
    want, want_sh = rl.relight(image, flipped, pred, weight, want_shadow=True, **terms)
    assert same_bits(got_sh, want_sh) and same_bits(got, want) and want_sh.any()


@gpu
def test_occluder_and_receiver_in_different_tiles_and_a_ramp_without_early_exit():
    """40 x 150: a wall at columns 75 .. 78 -- no multiple of the tile's 32 -- lit from each side at a low elevation, so that its shadow
    crosses into the next tiles; and a ramp rising towards the light by more than the ray does, on which every march runs its 64 steps."""
    from genpercept_amd import relight as rl
    h, w = 40, 150
    image = np.random.RandomState(4).randint(0, 256, (1, 3, h, w)).astype(np.uint8)
    image_d, normal_d = offset4(image), offset4(facing(h, w))
    pred = np.full((1, 1, h, w), 0.2, np.float32)
    pred[..., 75:79] = 0.9
    for azimuth, cols in ((180.0, slice(79, 79 + 40)), (0.0, slice(75 - 40, 75))):
        kw = dict(lights=dict(azimuth=azimuth, elevation=12.0, reach=64, bias=0.001), relief=200.0, space="disparity")
        got, got_sh = device_relight(image_d, normal_d, offset4(pred), None, **kw)
        want, want_sh = rl.relight(image, facing(h, w), pred, want_shadow=True, **kw)
        assert same_bits(got_sh, want_sh) and same_bits(got, want), azimuth
        assert (want_sh[0][:, cols] == 255).all() and want_sh.sum() == 255 * h * 64      # 64 columns of shadow, over two tile boundaries
    ramp = np.broadcast_to(np.linspace(0.05, 0.95, w, dtype=np.float32)[None, None, None], (1, 1, h, w)).copy()
    for azimuth, space in ((0.0, "disparity"), (180.0, "depth"), (315.0, "disparity")):
        kw = dict(lights=dict(azimuth=azimuth, elevation=10.0, reach=64, softness=0.05, strength=0.8), relief=500.0, space=space)
        row = rl.relight_lights(kw["lights"], relief=500.0)[0]
        assert 0 < row[15] < 393 // 2                                                     # the ramp gains 393 per column, the ray less
        got, got_sh = device_relight(image_d, normal_d, offset4(ramp), None, **kw)
        want, want_sh = rl.relight(image, facing(h, w), ramp, want_shadow=True, **kw)
        assert same_bits(got_sh, want_sh) and same_bits(got, want), (azimuth, space)
        assert (want_sh[0, 5:-5, 70:80] > 0).all()


@gpu
def test_stable_batch_independent_and_shading_only():
    from genpercept_amd import engine as ge
    from genpercept_amd import relight as rl
    b, h, w = 3, 40, 70
    pred, image, normal, weight = batch_case(21, b, h, w)
    pred_d, image_d, normal_d, weight_d = (torch.from_numpy(a).cuda() for a in (pred, image, normal, weight))
    kw = dict(lights=light_terms(8, 20), ambient=0.25, relief=24.0)
    whole, again = (device_relight(image_d, normal_d, pred_d, weight_d, **kw) for _ in range(2))
    assert same_bits(whole[0], again[0]) and same_bits(whole[1], again[1]) and whole[1].any()
    for i in range(b):
        one = device_relight(image_d[i], normal_d[i], pred_d[i], weight_d[i:i + 1], **kw)
        assert same_bits(one[0][0], whole[0][i]) and same_bits(one[1][0], whole[1][i]), i
    # without the shadow plane the bytes are the same; float64 maps are taken too
    assert same_bits(ge.relight(image_d, normal_d, pred_d, weight_d, **kw).cpu().numpy(), whole[0])
    assert same_bits(ge.relight(image_d, normal_d.double(), pred_d.double()[:, 0], weight_d, **kw).cpu().numpy(), whole[0])
    # the shading-only call is the call with pred and every reach 0
    rows = rl.relight_lights(**kw)
    unshadowed = rows.copy()
    unshadowed[:-1, 13:16] = 0
    unshadowed[:-1, 19] = 0
    plain = device_relight(image_d, normal_d, None, weight_d, lights=rows)
    stepless = device_relight(image_d, normal_d, pred_d, weight_d, lights=unshadowed)
    assert same_bits(plain[0], stepless[0]) and not plain[1].any() and not stepless[1].any() and not same_bits(plain[0], whole[0])
    assert same_bits(plain[0], rl.relight_rows(image, normal, None, weight, rows))
    for bad in (dict(lights=dict(reach=65)), dict(space="metric"), dict(flip=(True,)), dict(ambient=-1.0), dict(weight=weight_d[:, :5]),
                dict(normal=normal_d[:, :2]), dict(pred=pred_d[:2]), dict(tables=(np.zeros(256, np.uint16), np.zeros(4096, np.uint8)))):
        with pytest.raises(ValueError):
            ge.relight(**dict(dict(image=image_d, normal=normal_d, pred=pred_d, weight=weight_d), **bad))


@gpu
def test_invalid_arguments_with_real_buffers():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill.  Then
    the valid set goes through with outputs that start four bytes into their buffers, with and without the shadow plane."""
    from genpercept_amd import engine as ge
    from genpercept_amd import lens_blur as lb
    from genpercept_amd import relight as rl
    lib = ge.load_library()
    b, h, w = 2, 40, 70
    pred, image, normal, weight = batch_case(33, b, h, w)
    pred_d, image_d, normal_d, weight_d = offset4(pred), offset4(image), offset4(normal), offset4(weight)
    tables = lb.srgb_tables()
    to_lin_d, from_lin_d = offset4(tables[0].view(np.int16)), offset4(tables[1])
    rows, ptr = lights_array(valid_rows())

    def fresh():
        return dict(out=offset4(np.full((b, 3, h, w), 0x5A, np.uint8)), shadow=offset4(np.full((b, h, w), 0x5A, np.uint8)))

    bufs, keep = fresh(), []
    ok = relight_args(b, h, w, ptr, image=image_d.data_ptr(), normal=normal_d.data_ptr(), pred=pred_d.data_ptr(), weight=weight_d.data_ptr(),
                      to_lin=to_lin_d.data_ptr(), from_lin=from_lin_d.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()})
    untouched = assert_refused_with_real_buffers(call_relight, lib, ok, invalid_cases(ok, keep), bufs, fresh)
    want, want_sh = rl.relight_rows(image, normal, pred, weight, rows, want_shadow=True)
    for with_shadow in (True, False):
        bufs = fresh()
        assert call_relight(lib, dict(ok, out=bufs["out"].data_ptr(), shadow=bufs["shadow"].data_ptr() if with_shadow else None)) == 0
        torch.cuda.synchronize()
        assert same_bits(bufs["out"].cpu().numpy(), want)
        assert same_bits(bufs["shadow"].cpu().numpy(), want_sh) if with_shadow else torch.equal(bufs["shadow"], untouched["shadow"])
    assert want_sh.any()


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_relight_with_the_pipeline(tiny_weights, tmp_path):
    """Three 64 x 96 images at processing_res = 48: `relight_batch_device` == relight.py on the host applied to what the pipeline itself
    predicts on the device, bit for bit -- in mode normal (the prediction as the encoded normals, with and without a depth map for the
    shadows) and in mode depth (the normals `engine.depth_geometry` fits, the shadows of the map itself), plain, with `refine` and with
    `tiles`; `relight` gives one image; `run_relight` writes those bytes, and with sweep=3 three frames and their GIF."""
    from PIL import Image
    from genpercept_amd import engine as ge
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import relight as rl
    pipe, g = ps.tiny_pipeline(tiny_weights, 61)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 64, 96)
    tiles = dict(size=48, overlap=16, batch=4)
    weight = torch.zeros((3, 64, 96), dtype=torch.uint8)
    weight[:, 10:50, 20:80] = 200
    terms = dict(lights=[dict(azimuth=150.0, elevation=35.0, reach=24, specular=0.5), dict(azimuth=20.0, elevation=60.0, reach=10, softness=0.05)],
                 ambient=0.3, relief=40.0)
    try:
        done = {}
        depth = pipe.predict_batch_device(batch, "depth", processing_res=48)
        for name, extra in (("plain", {}), ("refine", dict(refine=True)), ("tiles", dict(tiles=tiles))):
            normal = pipe.predict_batch_device(batch, "normal", processing_res=48, **extra).cpu().numpy()
            for with_depth in (False, True):
                got, got_sh = pipe.relight_batch_device(batch, "normal", depth=depth if with_depth else None, weight=weight, want_shadow=True,
                                                        processing_res=48, **terms, **extra)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 3, 64, 96)
                want, want_sh = rl.relight(batch.numpy(), normal, depth.cpu().numpy() if with_depth else None, weight.numpy(), want_shadow=True, **terms)
                assert same_bits(got.cpu().numpy(), want) and same_bits(got_sh.cpu().numpy(), want_sh), (name, with_depth)
                assert not same_bits(want, batch.numpy())
            pred = pipe.predict_batch_device(batch, "depth", processing_res=48, **extra)
            fitted = ge.depth_geometry(pred, space="depth")["normal"].cpu().numpy()
            got = pipe.relight_batch_device(batch, "depth", processing_res=48, **terms, **extra)
            want = rl.relight(batch.numpy(), fitted, pred.cpu().numpy(), encoded=False, **terms)
            assert same_bits(got.cpu().numpy(), want) and not same_bits(want, batch.numpy()), name
            done[name] = want
            if name == "plain":
                plain = dict(normal=fitted, pred=pred.cpu().numpy())
        one = pipe.relight(Image.open(os.path.join(data, samples[1][0])), "depth", processing_res=48, **terms)
        pred = pipe.predict_batch_device(batch[1:2], "depth", processing_res=48)
        lone = rl.relight(batch[1:2].numpy(), ge.depth_geometry(pred, space="depth")["normal"].cpu().numpy(), pred.cpu().numpy(), encoded=False, **terms)
        assert one.mode == "RGB" and same_bits(np.moveaxis(np.asarray(one), -1, 0), lone[0])
        written = ie.run_relight(pipe, data, samples, str(tmp_path / "png"), ie.FileNameMode.id, "depth", 3, processing_res=48, **terms)
        assert len(written) == 3 and all(p.endswith(".png") for p in written)
        for i, path in enumerate(written):
            assert same_bits(np.moveaxis(np.asarray(Image.open(path)), -1, 0), done["plain"][i])
        swept = ie.run_relight(pipe, data, samples, str(tmp_path / "sweep"), ie.FileNameMode.id, "depth", 3, sweep=3, animate="gif", processing_res=48, **terms)
        assert len(swept) == 3 and all(len(p) == 4 and p[3].endswith(".gif") and p[0].endswith("_0000.png") for p in swept)
        for i, paths in enumerate(swept):
            frames = [np.moveaxis(np.asarray(Image.open(p)), -1, 0) for p in paths[:3]]
            assert same_bits(frames[0], done["plain"][i]) and not same_bits(frames[1], frames[0]) and not same_bits(frames[2], frames[1])
            with Image.open(paths[3]) as gif:
                assert gif.n_frames == 3 and gif.size == (96, 64)
        turned = [dict(o, azimuth=o["azimuth"] + 120.0) for o in terms["lights"]]                 # frame 1 of 3: a third of the way round
        want = rl.relight(batch.numpy(), plain["normal"], plain["pred"], encoded=False, **dict(terms, lights=turned))
        assert all(same_bits(np.moveaxis(np.asarray(Image.open(swept[i][1])), -1, 0), want[i]) for i in range(3))
        for bad in (dict(mode="matting"), dict(lights=dict(reach=65)), dict(match_input_res=False), dict(tiles="yes"), dict(mode="depth", depth=depth),
                    dict(weight=weight[:, :5])):
            with pytest.raises(ValueError):
                pipe.relight_batch_device(batch, **dict(dict(processing_res=48), **bad))
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
