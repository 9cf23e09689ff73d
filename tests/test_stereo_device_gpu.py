"""The stereo and parallax views on the device (gp_stereo_views): the canvas, the hole plane and the nearness plane BIT-EQUAL to the host route
genpercept_amd/stereo.py (itself pinned to plain loops and to a CPU build of the kernels' arithmetic in tests/test_stereo_host.py), over
sizes that are multiples of nothing, shifts up to 64 pixels (an apron wider than a tile's share of the image, a shift larger than the
image), both spaces, a pair, an anaglyph and a quilt, a convergence plane per image, a batch whose middle map is all NaN, a flat tile next
to one with a step edge, tensors that start four bytes into their buffers; batch independence and repeatability; the argument checks with
real buffers around them; the pipeline and the dataset loop with `refine` and `tiles` at tiny widths.  There is no tolerance in this file."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict  # noqa: E402
from test_stereo_host import call_stereo, fold_and_cut_row, invalid_cases, scene, stereo_args, views_array  # noqa: E402

gpu = pytest.mark.gpu

# B, H, W, the largest shift in pixels, edge
CASES = [(1, 5, 7, 1, 2600), (2, 19, 70, 5, 2600), (1, 9, 300, 64, 2600), (3, 6, 40, 64, 2600), (1, 33, 129, 20, 0), (1, 33, 129, 20, 65535)]
LAYOUTS = [("pair", 2), ("anaglyph", 2), ("quilt", (3, 3))]


batch_case = functools.partial(ps.batch_case, scene)


def device_views(image_d, pred_d, F, table, size, space, edge, max_s8, with_planes=True, fill=0x5A):
    """gp_stereo_views itself on device tensors: (canvas, holes, near) as numpy arrays; the canvas starts as `fill`."""
    from genpercept_amd import engine as ge
    from genpercept_amd import stereo as st
    lib = ge.load_library()
    b, _, h, w = image_d.shape
    v = len(table)
    rows, rows_ptr = views_array(table)
    conv = offset4(np.broadcast_to(np.asarray(F, np.int32), (b,)))
    canvas = offset4(np.full((b, 3) + tuple(size), fill, np.uint8))
    holes, near = offset4(np.full((b, v, h, w), 0x5A, np.uint8)), offset4(np.full((b, v, h, w), 0x5A5A, np.int16))
    nbytes = lib.gp_stereo_views_workspace(b, v, h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
    status = lib.gp_stereo_views(image_d.data_ptr(), pred_d.data_ptr(), conv.data_ptr(), rows_ptr, b, v, h, w, size[0], size[1], st.SPACES.index(space), edge,
                                 max_s8, canvas.data_ptr(), holes.data_ptr() if with_planes else None, near.data_ptr() if with_planes else None,
                                 ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert status == 0
    return canvas.cpu().numpy(), holes.cpu().numpy(), near.cpu().numpy().view(np.uint16)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-s%d-e%d" % s)
def test_bytes_equal_the_host_route(case):
    from genpercept_amd import stereo as st
    b, h, w, shift, edge = case
    pred, image = batch_case(900 + h + w, b, h, w, middle_nan=b == 3)
    pred_d, image_d = offset4(pred), offset4(image)
    F = np.random.RandomState(h).randint(0, 65536, b) if b > 1 else np.array([20000])
    assert len(set(F.tolist())) == b                                                                 # a different plane per image
    met = dict(holes=0, multiple=0)
    for space in st.SPACES:
        for layout, views in LAYOUTS:
            table, size = st.view_table(layout, views, min(2.0 * shift, 127.9), h, w)
            got = device_views(image_d, pred_d, F, table.tolist(), size, space, edge, 8 * shift)
            want = st.stereo_views_table(image, pred, F, table, np.full((b, 3) + size, 0x5A, np.uint8), space, edge, 8 * shift, want_cover=True)
            assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]) and same_bits(got[0], want[0]), (case, space, layout)
            met["holes"] += int(want[1].sum())
            met["multiple"] += int((want[3] >= 2).sum())
            if b == 3:
                assert (want[2][1] == 0).all()                                                         # the map of NaNs is a flat plane at nearness 0
    assert met["holes"] > 0 and met["multiple"] > 0, met


@gpu
def test_a_flat_tile_next_to_a_tile_with_a_step():
    """disparity space, 600 columns, three tiles of 256: a near plane left of column 260 -- no multiple of the tile width --, a far plane in
    the zero-parallax plane right of it.  The near plane moves 20 columns to the left, so the hole it opens, columns 240 .. 259, reaches
    across the boundary between the first tile, which is flat, and the second, which holds the step; the third lies in the zero-parallax
    plane and looks at one source per column."""
    from genpercept_amd import stereo as st
    h, w, step, move = 9, 600, 260, 20
    pred = np.full((1, 1, h, w), 0.2, np.float32)
    pred[..., :step] = 0.8
    image = np.random.RandomState(4).randint(0, 256, (1, 3, h, w)).astype(np.uint8)
    Dn, Df = (int(v) for v in st.nearness(np.float32([0.8, 0.2]), "disparity"))
    g = -next(g for g in range(131073) if int(st.shifts(Dn, Df, g, 512)) == 8 * move)
    for edge, max_s8 in ((3000, 8 * move), (3000, 512), (0, 200)):
        got = device_views(offset4(image), offset4(pred), Df, [[g, 0, 0, 7]], (h, w), "disparity", edge, max_s8)
        want = st.stereo_views_table(image, pred, Df, [[g, 0, 0, 7]], (h, w), "disparity", edge, max_s8)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2]), (edge, max_s8)
        holes = np.zeros((h, w), np.uint8)
        holes[:, step - move:step] = 1
        assert same_bits(want[1][0, 0], holes) and same_bits(want[0][0, :, :, :step - move], image[0, :, :, move:step])
        assert same_bits(want[0][0, :, :, step - move:], np.concatenate([np.repeat(image[0, :, :, step:step + 1], move, 2), image[0, :, :, step:]], 2))
    # a row that is no surface of planar pieces: the bound of the hole search is part of the definition
    pred, F, g, edge, max_s8 = fold_and_cut_row()
    image = np.random.RandomState(3).randint(1, 256, (1, 3, 1, pred.shape[1])).astype(np.uint8)
    got = device_views(offset4(image), offset4(pred[None, None]), F, [[g, 0, 0, 7]], pred.shape, "disparity", edge, max_s8)
    want = st.stereo_views_table(image, pred, F, [[g, 0, 0, 7]], pred.shape, "disparity", edge, max_s8)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2]) and not want[2][0, 0, 0, 130:134].any()


@gpu
def test_stable_batch_independent_and_converge_at():
    from genpercept_amd import engine as ge
    from genpercept_amd import stereo as st
    for (b, h, w, separation, layout, views), space in (((3, 19, 70, 40.0, "sbs", 2), "depth"), ((3, 33, 300, 100.0, "quilt", (2, 2)), "disparity")):
        pred, image = batch_case(21, b, h, w)
        pred_d, image_d = torch.from_numpy(pred).cuda(), torch.from_numpy(image).cuda()
        kw = dict(layout=layout, views=views, separation=separation, converge=[0.2, 0.5, 0.9], edge=0.03, space=space)
        whole, again = (ge.stereo_views(image_d, pred_d, want_holes=True, want_near=True, **kw) for _ in range(2))
        assert whole[0].dtype == torch.uint8 and whole[1].dtype == torch.uint8 and whole[2].dtype == torch.int16 and all(t.is_cuda for t in whole)
        assert all(torch.equal(x, y) for x, y in zip(whole, again))
        want = st.stereo_views(image, pred, want_holes=True, want_near=True, **kw)
        assert same_bits(whole[0].cpu().numpy(), want[0]) and same_bits(whole[1].cpu().numpy(), want[1])
        assert same_bits(whole[2].cpu().numpy().view(np.uint16), want[2]) and want[1].any()
        for i in range(b):
            one = ge.stereo_views(image_d[i], pred_d[i], want_holes=True, want_near=True, **dict(kw, converge=kw["converge"][i]))
            assert all(torch.equal(x[0], y[i]) for x, y in zip(one, whole)), i
        # without the planes, with one of them, into a canvas of the caller's, from float64 maps: the same bytes
        assert torch.equal(ge.stereo_views(image_d, pred_d, **kw), whole[0])
        only = ge.stereo_views(image_d, pred_d, want_near=True, **kw)
        assert len(only) == 2 and torch.equal(only[0], whole[0]) and torch.equal(only[1], whole[2])
        mine = torch.full_like(whole[0], 0x5A)
        assert ge.stereo_views(image_d, pred_d.double()[:, 0], canvas=mine, **kw) is mine and torch.equal(mine, whole[0])
        # the plane taken from a pixel on the device is the plane of that pixel's value; a NaN pixel has the nearness 0
        at = np.array([[5, 7], [w - 1, h - 1], [0, 3]])
        pred[2, 0, 3, 0] = np.nan
        pred_d = torch.from_numpy(pred).cuda()
        rest = dict(kw, separation=min(separation, 60.0))
        del rest["converge"]
        got = ge.stereo_views(image_d, pred_d, converge_at=at, **rest).cpu().numpy()
        assert same_bits(got, st.stereo_views(image, pred, converge_at=at, **rest))
        value = np.nan_to_num(pred[np.arange(b), 0, at[:, 1], at[:, 0]], nan=1.0 if space == "depth" else 0.0).clip(0, 1)
        o = st.plan(b, h, w, rest["layout"], rest["views"], rest["separation"], converge_at=at, edge=rest["edge"])
        F = st.nearness(value.astype(np.float32), space)
        same = st.stereo_views_table(image, pred, F, o["table"], o["size"], space, o["edge"], o["max_s8"])[0]
        assert same_bits(got, same) and same_bits(F, st.convergence(pred[:, 0], space, o))
        assert same_bits(ge.stereo_views(image_d, pred_d, **rest).cpu().numpy(), st.stereo_views(image, pred, **rest))     # neither: the middle
    for bad in (dict(converge=0.5, converge_at=(1, 1)), dict(converge=1.5), dict(converge_at=(w, 0)), dict(converge_at=(0, h)), dict(space="metric"),
                dict(separation=128.0), dict(layout="pair", views=3), dict(edge=2.0), dict(converge=[0.5, 0.5]), dict(canvas=mine[:, :, :5])):
        with pytest.raises(ValueError):
            ge.stereo_views(image_d, pred_d, **bad)
    for bad in (dict(image=image_d.float()), dict(image=image_d[:2]), dict(pred=(pred_d * 255).to(torch.uint8)), dict(image=image_d[:, :2])):
        with pytest.raises(ValueError):
            ge.stereo_views(**dict(dict(image=image_d, pred=pred_d), **bad))


@gpu
def test_invalid_arguments_with_real_buffers():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and the canvas, holes and near keep their
    fill.  Then the valid set goes through, with and without the two planes, and a convergence table with values outside 0 .. 65535 gives
    what the host route gives for the values clamped into it."""
    from genpercept_amd import engine as ge
    from genpercept_amd import stereo as st
    lib = ge.load_library()
    b, h, w = 2, 40, 70
    pred, image = batch_case(33, b, h, w)
    pred_d, image_d = offset4(pred), offset4(image)
    conv_d = offset4(np.array([70000, -3], np.int32))
    nbytes = lib.gp_stereo_views_workspace(b, 2, h, w)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")

    def fresh():
        return dict(canvas=offset4(np.full((b, 3, h, 2 * w), 0x5A, np.uint8)), holes=offset4(np.full((b, 2, h, w), 0x5A, np.uint8)),
                    near=offset4(np.full((b, 2, h, w), 0x5A5A, np.int16)))

    bufs = fresh()
    ok = stereo_args(b, h, w, image=image_d.data_ptr(), pred=pred_d.data_ptr(), conv=conv_d.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes,
                     **{k: v.data_ptr() for k, v in bufs.items()})
    untouched = assert_refused_with_real_buffers(call_stereo, lib, ok, invalid_cases(ok), bufs, fresh)
    table = [[30000, 0, 0, 7], [-30000, w, 0, 7]]
    want = st.stereo_views_table(image, pred, [65535, 0], table, (h, 2 * w), "depth", ok["edge"], ok["max_s8"])
    assert want[1].any()
    for with_planes in (True, False):
        bufs = fresh()
        args = dict(ok, canvas=bufs["canvas"].data_ptr(), holes=bufs["holes"].data_ptr() if with_planes else None,
                    near=bufs["near"].data_ptr() if with_planes else None)
        assert call_stereo(lib, args) == 0
        torch.cuda.synchronize()
        assert same_bits(bufs["canvas"].cpu().numpy(), want[0])
        if with_planes:
            assert same_bits(bufs["holes"].cpu().numpy(), want[1]) and same_bits(bufs["near"].cpu().numpy().view(np.uint16), want[2])
        else:
            assert torch.equal(bufs["holes"], untouched["holes"]) and torch.equal(bufs["near"], untouched["near"])


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_stereo_with_the_pipeline(tiny_weights, tmp_path):
    """Three 96 x 128 images at processing_res = 48: `stereo_batch_device` == stereo.py on the host applied to what `predict_batch_device`
    returns, bit for bit, for depth and disparity, plain, with `refine`, with `tiles` and with both; `stereo` gives one image of the canvas
    size; `run_stereo` writes those bytes; what the entry does not take is refused."""
    from PIL import Image
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import stereo as st
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    tiles = dict(size=48, overlap=16, batch=4)
    try:
        done = {}
        wide = dict(layout="sbs", views=2, separation=100.0, converge_at=(64, 48), edge=0.02)
        own = dict(layout="quilt", views=(2, 3), separation=60.0, converge=[0.2, 0.5, 0.8], edge=0.1)
        extras = dict(plain={}, refine=dict(refine=True), tiles=dict(tiles=tiles), both=dict(refine=dict(radius=2), tiles=tiles))
        for mode, name, settings in (("depth", "plain", (wide, own)), ("depth", "refine", (own,)), ("depth", "tiles", (wide,)), ("depth", "both", (own,)),
                                     ("disparity", "plain", (wide, own)), ("disparity", "tiles", (own,))):
            extra = extras[name]
            pred = pipe.predict_batch_device(batch, mode, processing_res=48, **extra).cpu().numpy()
            for kw in settings:
                got = pipe.stereo_batch_device(batch, mode, processing_res=48, **kw, **extra)
                size = (96, 256) if kw is wide else (192, 384)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, 3) + size
                want = st.stereo_views(batch.numpy(), pred, space=mode, **kw)
                assert same_bits(got.cpu().numpy(), want), (mode, name, sorted(kw))
                assert not same_bits(want[..., :96, :128], batch.numpy())
                done[mode, name, kw is wide] = want
            if name == "plain":
                value = pred[:, 0, 48, 64].clip(0, 1)
                o = st.plan(3, 96, 128, "sbs", 2, 100.0, converge_at=(64, 48), edge=0.02)
                same = st.stereo_views_table(batch.numpy(), pred, st.nearness(value, mode), o["table"], o["size"], mode, o["edge"], o["max_s8"])[0]
                assert same_bits(same, done[mode, name, True])
        assert not same_bits(done["depth", "plain", True], done["depth", "tiles", True])
        one = pipe.stereo(Image.open(os.path.join(data, samples[1][0])), processing_res=48, **wide)
        lone = st.stereo_views(batch[1:2].numpy(), pipe.predict_batch_device(batch[1:2], "depth", processing_res=48).cpu().numpy(), **wide)
        assert one.mode == "RGB" and one.size == (256, 96) and same_bits(np.moveaxis(np.asarray(one), -1, 0), lone[0])
        ana = pipe.stereo(Image.open(os.path.join(data, samples[1][0])), layout="anaglyph", separation=30.0, processing_res=48)
        assert ana.size == (128, 96)
        for kw, key in ((dict(), ("depth", "plain", True)), (dict(tiles=tiles), ("depth", "tiles", True))):
            written = ie.run_stereo(pipe, data, samples, str(tmp_path / ("png" + "-".join(kw))), ie.FileNameMode.id, "depth", 3, processing_res=48, **wide, **kw)
            assert len(written) == 3 and all(p.endswith(".png") for p in written)
            for i, path in enumerate(written):
                assert same_bits(np.moveaxis(np.asarray(Image.open(path)), -1, 0), done[key][i])
        for bad in (dict(mode="matting"), dict(mode="normal"), dict(converge=0.5, converge_at=(1, 1)), dict(converge=2.0), dict(separation=130.0),
                    dict(separation=128.0), dict(match_input_res=False), dict(tiles="yes"), dict(converge_at=(128, 0)), dict(layout="wiggle"),
                    dict(layout="quilt", views=9)):
            with pytest.raises(ValueError):
                pipe.stereo_batch_device(batch, **dict(dict(processing_res=48), **bad))
        with pytest.raises(ValueError):
            pipe.stereo_batch_device(batch.float(), processing_res=48)
        with pytest.raises(ValueError):
            ie.run_stereo(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "matting", processing_res=48)
        with pytest.raises(ValueError):
            ie.run_stereo(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", converge=[0.5, 0.5, 0.5], processing_res=48)
        with pytest.raises(ValueError):
            ie.run_stereo(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", separation=500.0, processing_res=48)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
