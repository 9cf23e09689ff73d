"""The camera moves from one photograph on the device (gp_parallax_frames): the frames, the hole plane and the nearness plane BIT-EQUAL to the
host route genpercept_amd/parallax.py (itself pinned to plain loops and to a CPU build of the kernels' arithmetic in
tests/test_parallax_host.py), over sizes that cross the 32 x 32 tiles both ways and sizes smaller than one, displacements up to 32 pixels,
zooms of 1 x to 2 x, swings, orbits and dollies, both spaces, a plane per image, a map of NaNs, a near square centred on a tile corner at
the widest apron, a flat tile next to one with a step, tensors that start four bytes or one byte into their buffers; batch independence
and repeatability; `focus_at` read on the device; the argument checks with real buffers around them; the pipeline and the dataset loop with
`refine` and `tiles` at tiny widths, with frames and a GIF written.  There is no tolerance in this file."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict, unaligned  # noqa: E402
from test_parallax_host import ZOOMS, call_parallax, frames_array, invalid_cases, parallax_args, scene  # noqa: E402

gpu = pytest.mark.gpu

# B, H, W, max_s8, edge
CASES = [(2, 33, 65, 40, 2600), (2, 70, 40, 256, 2600), (1, 1, 1, 8, 0), (1, 5, 7, 40, 65535)]


batch_case = functools.partial(ps.batch_case, scene)


def table_for(h, w, max_s8):
    """Six frames: one that does not move, gains that meet the clamp in both directions, a dolly either way, every zoom of ZOOMS."""
    g = min(131072, int(1.5 * max_s8 * 16777216 / 65535))
    gz = min(1 << 24, int(max_s8 * 65536 / max(1, 4 * (max(h, w) - 1)) * 256))
    return [[0, 0, 0, ZOOMS[0]], [g, -g // 2, 0, ZOOMS[0]], [-g // 3, g, gz, ZOOMS[1]], [g // 2, g // 4, -gz, ZOOMS[2]], [-g, -g, 0, ZOOMS[1]], [0, 0, gz, ZOOMS[0]]]


def device_frames(image_d, pred_d, F, table, space, edge, max_s8, with_planes=True):
    """gp_parallax_frames itself on device tensors: (frames, holes, near) as numpy arrays; every buffer starts as a fill."""
    from genpercept_amd import engine as ge
    from genpercept_amd import parallax as pv
    lib = ge.load_library()
    b, _, h, w = image_d.shape
    v = len(table)
    rows, rows_ptr = frames_array(table)
    focus = offset4(np.broadcast_to(np.asarray(F, np.int32), (b,)))
    out = unaligned(np.full((b, v, 3, h, w), 0x5A, np.uint8))
    holes, near = unaligned(np.full((b, v, h, w), 0x5A, np.uint8)), offset4(np.full((b, v, h, w), 0x5A5A, np.int16))
    nbytes = lib.gp_parallax_frames_workspace(b, v, h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
    status = lib.gp_parallax_frames(image_d.data_ptr(), pred_d.data_ptr(), focus.data_ptr(), rows_ptr, b, v, h, w, pv.SPACES.index(space), edge, max_s8,
                                    out.data_ptr(), holes.data_ptr() if with_planes else None, near.data_ptr() if with_planes else None, ws.data_ptr(), nbytes,
                                    None)
    torch.cuda.synchronize()
    assert status == 0
    return out.cpu().numpy(), holes.cpu().numpy(), near.cpu().numpy().view(np.uint16)


def assert_same(got, want, what):
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]) and same_bits(got[0], want[0]), what


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-s%d-e%d" % s)
def test_bytes_equal_the_host_route(case):
    from genpercept_amd import parallax as pv
    b, h, w, max_s8, edge = case
    pred, image = batch_case(900 + h + w, b, h, w)
    pred_d, image_d = offset4(pred), unaligned(image)
    F = np.random.RandomState(h).randint(0, 65536, b) if b > 1 else np.array([20000])
    assert len(set(F.tolist())) == b                                                                 # a different plane per image
    table = table_for(h, w, max_s8)
    seen = dict(holes=0, ties=0)
    for space in pv.SPACES:
        got = device_frames(image_d, pred_d, F, table, space, edge, max_s8)
        want = pv.parallax_frames_table(image, pred, F, table, space, edge, max_s8, want_stats=True)
        assert_same(got, want, (case, space))
        assert same_bits(got[0][:, 0], image) and not got[1][:, 0].any()                                # the frame that does not move
        seen["holes"] += int(want[1].sum())
        seen["ties"] += sum(int((s["ties"] >= 2).sum()) for per in want[3] for s in per)
    assert (seen["holes"] > 0 and seen["ties"] > 0) or h * w == 1, seen


@gpu
def test_a_near_square_on_a_tile_corner_and_a_map_of_nans():
    """96 x 96, nine tiles: a near square of 24 x 24 centred on the corner (32, 32) that four tiles share, under diagonal moves of the full
    32 pixels with max_s8 = 256, so that the tile the square lands in receives sources staged from the aprons of all four; then a batch whose
    middle map is all NaN, a flat plane at nearness 0."""
    from genpercept_amd import parallax as pv
    h = w = 96
    pred = np.full((1, 1, h, w), 0.9, np.float32)
    pred[..., 20:44, 20:44] = 0.1
    image = np.random.RandomState(4).randint(0, 200, (1, 3, h, w)).astype(np.uint8)
    image[..., 20:44, 20:44] = 255
    Dn, Df = (int(v) for v in pv.nearness(np.float32([0.1, 0.9]), "depth"))
    gain = next(g for g in range(131073) if ((Dn - Df) * g + (1 << 23)) >> 24 == 256)
    table = [[gx, gy, 0, 65536] for gx in (gain, -gain) for gy in (gain, -gain)] + [[gain, 0, 0, 65536], [131072, -131072, 0, 65536]]
    got = device_frames(offset4(image), offset4(pred), Df, table, "depth", 3000, 256)
    want = pv.parallax_frames_table(image, pred, Df, table, "depth", 3000, 256)
    assert_same(got, want, "square")
    moved = np.zeros((h, w), bool)
    moved[52:76, 52:76] = True                                                                          # frame 0: 32 pixels down and to the right
    assert (want[0][0, 0][:, moved] == 255).all() and (want[2][0, 0][moved] == Dn).all() and want[1][0, 0, 20:44, 20:44].all()
    assert same_bits(want[0][0, 0][:, ~moved & (want[1][0, 0] == 0)], image[0][:, ~moved & (want[1][0, 0] == 0)])
    pred3, image3 = batch_case(17, 3, 40, 70, middle_nan=True)
    table = table_for(40, 70, 100)
    got = device_frames(unaligned(image3), offset4(pred3), [100, 40000, 65535], table, "disparity", 2600, 100, with_planes=True)
    want = pv.parallax_frames_table(image3, pred3, [100, 40000, 65535], table, "disparity", 2600, 100)
    assert_same(got, want, "nan")
    assert (want[2][1][want[1][1] == 0] == 0).all()


@gpu
def test_a_flat_tile_next_to_a_tile_with_a_step():
    """disparity space, 40 x 100: a near plane left of column 37 -- no multiple of the tile width --, a far plane in the plane that stays put
    right of it.  The near plane moves 20 columns to the left, so the hole it opens, columns 17 .. 36, reaches across the boundary between
    the first tile, whose sources are flat, and the second, which holds the step; the third lies in the plane that stays put."""
    from genpercept_amd import parallax as pv
    h, w, step, move = 40, 100, 37, 20
    pred = np.full((1, 1, h, w), 0.2, np.float32)
    pred[..., :step] = 0.8
    image = np.random.RandomState(4).randint(0, 256, (1, 3, h, w)).astype(np.uint8)
    Dn, Df = (int(v) for v in pv.nearness(np.float32([0.8, 0.2]), "disparity"))
    g = -next(g for g in range(131073) if ((Dn - Df) * g + (1 << 23)) >> 24 == 8 * move)
    for edge, max_s8 in ((3000, 8 * move), (3000, 256), (0, 200)):
        got = device_frames(offset4(image), offset4(pred), Df, [[g, 0, 0, 65536]], "disparity", edge, max_s8)
        want = pv.parallax_frames_table(image, pred, Df, [[g, 0, 0, 65536]], "disparity", edge, max_s8)
        assert_same(got, want, (edge, max_s8))
        holes = np.zeros((h, w), np.uint8)
        holes[:, step - move:step] = 1
        assert same_bits(want[1][0, 0], holes) and same_bits(want[0][0, 0, :, :, :step - move], image[0, :, :, move:step])
        assert same_bits(want[0][0, 0, :, :, step - move:], np.concatenate([np.repeat(image[0, :, :, step:step + 1], move, 2), image[0, :, :, step:]], 2))


@gpu
def test_stable_batch_independent_and_focus_at():
    from genpercept_amd import engine as ge
    from genpercept_amd import parallax as pv
    for (b, h, w, kw), space in (((3, 40, 70, dict(path="orbit", frames=5, amount=24.0)), "depth"),
                                 ((3, 33, 100, dict(path="dolly", frames=4, amount=10.0, push=0.04, zoom=1.3, pan=True)), "disparity")):
        pred, image = batch_case(21, b, h, w)
        pred_d, image_d = torch.from_numpy(pred).cuda(), torch.from_numpy(image).cuda()
        kw = dict(kw, focus=[0.2, 0.5, 0.9], edge=0.03, space=space, overscan=False)
        whole, again = (ge.parallax_frames(image_d, pred_d, want_holes=True, want_near=True, **kw) for _ in range(2))
        assert whole[0].dtype == torch.uint8 and whole[1].dtype == torch.uint8 and whole[2].dtype == torch.int16 and all(t.is_cuda for t in whole)
        assert all(torch.equal(x, y) for x, y in zip(whole, again))
        want = pv.parallax_frames(image, pred, want_holes=True, want_near=True, **kw)
        assert same_bits(whole[0].cpu().numpy(), want[0]) and same_bits(whole[1].cpu().numpy(), want[1])
        assert same_bits(whole[2].cpu().numpy().view(np.uint16), want[2]) and want[1].any()
        # an image's bytes do not depend on the batch it is in: the C entry with the integers of the batch's call (max_s8, which bounds the
        # clamp and the hole search, comes from the planes of all its images; a call for one image derives its own, as the host does)
        o = pv.plan(b, h, w, **{k: v for k, v in kw.items() if k != "space"})
        F = pv.focus_plane(pred[:, 0], space, o)
        batch = device_frames(image_d, pred_d, F, o["table"].tolist(), space, o["edge"], o["max_s8"])
        assert same_bits(batch[0], want[0])
        for i in range(b):
            alone = device_frames(image_d[i:i + 1], pred_d[i:i + 1], F[i:i + 1], o["table"].tolist(), space, o["edge"], o["max_s8"])
            assert all(same_bits(x[0], y[i]) for x, y in zip(alone, batch)), i
            one = ge.parallax_frames(image_d[i], pred_d[i], want_holes=True, want_near=True, **dict(kw, focus=kw["focus"][i]))
            lone = pv.parallax_frames(image[i], pred[i], want_holes=True, want_near=True, **dict(kw, focus=kw["focus"][i]))
            assert same_bits(one[0].cpu().numpy(), lone[0]) and same_bits(one[1].cpu().numpy(), lone[1]) and same_bits(one[2].cpu().numpy().view(np.uint16), lone[2])
        # without the planes, with one of them, into a tensor of the caller's, from float64 maps, a part of the path: the same bytes
        assert torch.equal(ge.parallax_frames(image_d, pred_d, **kw), whole[0])
        only = ge.parallax_frames(image_d, pred_d, want_near=True, **kw)
        assert len(only) == 2 and torch.equal(only[0], whole[0]) and torch.equal(only[1], whole[2])
        mine = torch.full_like(whole[0], 0x5A)
        assert ge.parallax_frames(image_d, pred_d.double()[:, 0], out=mine, **kw) is mine and torch.equal(mine, whole[0])
        assert torch.equal(ge.parallax_frames(image_d, pred_d, frame_range=(1, 3), **kw), whole[0][:, 1:3])
        # with overscan no border shows on these maps' frames either way, and the bytes are the host's
        over = dict(kw, overscan=True)
        assert same_bits(ge.parallax_frames(image_d, pred_d, **over).cpu().numpy(), pv.parallax_frames(image, pred, **over))
        # the plane taken from a pixel on the device is the plane of that pixel's value; a NaN pixel has the nearness 0
        at = np.array([[5, 7], [w - 1, h - 1], [0, 3]])
        pred[2, 0, 3, 0] = np.nan
        pred_d = torch.from_numpy(pred).cuda()
        rest = dict(kw, amount=min(kw["amount"], 12.0))
        del rest["focus"]
        got = ge.parallax_frames(image_d, pred_d, focus_at=at, **rest).cpu().numpy()
        assert same_bits(got, pv.parallax_frames(image, pred, focus_at=at, **rest))
        value = np.nan_to_num(pred[np.arange(b), 0, at[:, 1], at[:, 0]], nan=1.0 if space == "depth" else 0.0).clip(0, 1)
        o = pv.plan(b, h, w, focus_at=at, **{k: v for k, v in rest.items() if k != "space"})
        F = pv.nearness(value.astype(np.float32), space)
        same = pv.parallax_frames_table(image, pred, F, o["table"], space, o["edge"], o["max_s8"])[0]
        assert same_bits(got, same) and same_bits(F, pv.focus_plane(pred[:, 0], space, o))
        assert same_bits(ge.parallax_frames(image_d, pred_d, **rest).cpu().numpy(), pv.parallax_frames(image, pred, **rest))      # neither: the middle
    for bad in (dict(focus=0.5, focus_at=(1, 1)), dict(focus=1.5), dict(focus_at=(w, 0)), dict(focus_at=(0, h)), dict(space="metric"), dict(amount=130.0),
                dict(path="dolly", zoom=2.5), dict(edge=2.0), dict(focus=[0.5, 0.5]), dict(out=mine[:, :2]), dict(frames=65), dict(frame_range=(2, 9))):
        with pytest.raises(ValueError):
            ge.parallax_frames(image_d, pred_d, **dict(dict(frames=4, amount=2.0, overscan=False), **bad))
    for bad in (dict(image=image_d.float()), dict(image=image_d[:2]), dict(pred=(pred_d * 255).to(torch.uint8)), dict(image=image_d[:, :2])):
        with pytest.raises(ValueError):
            ge.parallax_frames(**dict(dict(image=image_d, pred=pred_d, amount=2.0), **bad))


@gpu
def test_invalid_arguments_with_real_buffers():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and out, holes and near keep their
    fill.  Then the valid set goes through, with and without the two planes, and a focus table with values outside 0 .. 65535 gives what
    the host route gives for the values clamped into it."""
    from genpercept_amd import engine as ge
    from genpercept_amd import parallax as pv
    lib = ge.load_library()
    b, h, w = 2, 40, 70
    pred, image = batch_case(33, b, h, w)
    pred_d, image_d = offset4(pred), offset4(image)
    focus_d = offset4(np.array([70000, -3], np.int32))
    nbytes = lib.gp_parallax_frames_workspace(b, 2, h, w)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")

    def fresh():
        return dict(out=offset4(np.full((b, 2, 3, h, w), 0x5A, np.uint8)), holes=offset4(np.full((b, 2, h, w), 0x5A, np.uint8)),
                    near=offset4(np.full((b, 2, h, w), 0x5A5A, np.int16)))

    bufs = fresh()
    ok = parallax_args(b, h, w, image=image_d.data_ptr(), pred=pred_d.data_ptr(), focus=focus_d.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes,
                       **{k: v.data_ptr() for k, v in bufs.items()})
    untouched = assert_refused_with_real_buffers(call_parallax, lib, ok, invalid_cases(ok), bufs, fresh)
    table = [[30000, -20000, 100000, 70000], [-30000, 10000, 0, 65536]]                                   # the rows of parallax_args
    want = pv.parallax_frames_table(image, pred, [65535, 0], table, "depth", ok["edge"], ok["max_s8"])
    assert want[1].any()
    for with_planes in (True, False):
        bufs = fresh()
        args = dict(ok, out=bufs["out"].data_ptr(), holes=bufs["holes"].data_ptr() if with_planes else None, near=bufs["near"].data_ptr() if with_planes else None)
        assert call_parallax(lib, args) == 0
        torch.cuda.synchronize()
        assert same_bits(bufs["out"].cpu().numpy(), want[0])
        if with_planes:
            assert same_bits(bufs["holes"].cpu().numpy(), want[1]) and same_bits(bufs["near"].cpu().numpy().view(np.uint16), want[2])
        else:
            assert torch.equal(bufs["holes"], untouched["holes"]) and torch.equal(bufs["near"], untouched["near"])


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_parallax_with_the_pipeline(tiny_weights, tmp_path):
    """Three 96 x 128 images at processing_res = 48: `parallax_batch_device` == parallax.py on the host applied to what
    `predict_batch_device` returns, bit for bit, for depth and disparity, plain, with `refine`, with `tiles` and with both; `parallax` gives
    the frames as images; `run_parallax` writes those bytes as numbered frames and a looping GIF, a path of 70 frames in two parts; what the
    entry does not take is refused."""
    from PIL import Image
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import parallax as pv
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    tiles = dict(size=48, overlap=16, batch=4)
    try:
        done = {}
        orbit = dict(path="orbit", frames=4, amount=30.0, focus_at=(64, 48), edge=0.02)
        dolly = dict(path="dolly", frames=3, amount=8.0, push=0.05, zoom=1.2, pan=True, focus=[0.2, 0.5, 0.8], edge=0.1)
        extras = dict(plain={}, refine=dict(refine=True), tiles=dict(tiles=tiles), both=dict(refine=dict(radius=2), tiles=tiles))
        for mode, name, settings in (("depth", "plain", (orbit, dolly)), ("depth", "refine", (dolly,)), ("depth", "tiles", (orbit,)), ("depth", "both", (dolly,)),
                                     ("disparity", "plain", (orbit, dolly)), ("disparity", "tiles", (dolly,))):
            extra = extras[name]
            pred = pipe.predict_batch_device(batch, mode, processing_res=48, **extra).cpu().numpy()
            for kw in settings:
                got = pipe.parallax_batch_device(batch, mode, processing_res=48, **kw, **extra)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, kw["frames"], 3, 96, 128)
                want = pv.parallax_frames(batch.numpy(), pred, space=mode, **kw)
                assert same_bits(got.cpu().numpy(), want), (mode, name, sorted(kw))
                assert not same_bits(want[:, 1], batch.numpy())
                done[mode, name, kw is orbit] = want
        assert not same_bits(done["depth", "plain", True], done["depth", "tiles", True])
        one = pipe.parallax(Image.open(os.path.join(data, samples[1][0])), processing_res=48, **orbit)
        lone = pv.parallax_frames(batch[1:2].numpy(), pipe.predict_batch_device(batch[1:2], "depth", processing_res=48).cpu().numpy(), **orbit)
        assert len(one) == 4 and all(im.mode == "RGB" and im.size == (128, 96) for im in one)
        assert all(same_bits(np.moveaxis(np.asarray(im), -1, 0), lone[0, k]) for k, im in enumerate(one))
        for kw, key in ((dict(), ("depth", "plain", True)), (dict(tiles=tiles), ("depth", "tiles", True))):
            written = ie.run_parallax(pipe, data, samples, str(tmp_path / ("png" + "-".join(kw))), ie.FileNameMode.id, "depth", 3, processing_res=48, animate="gif",
                                      **orbit, **kw)
            assert len(written) == 3 and all(len(p) == 5 and p[-1].endswith(".gif") and all(q.endswith(".png") for q in p[:4]) for p in written)
            for i, paths in enumerate(written):
                for k, path in enumerate(paths[:4]):
                    assert same_bits(np.moveaxis(np.asarray(Image.open(path)), -1, 0), done[key][i, k])
                with Image.open(paths[-1]) as clip:
                    assert clip.format == "GIF" and clip.n_frames == 4 and clip.size == (128, 96) and clip.info.get("loop") == 0
        # a path of 70 frames is rendered in two calls under one map: the same bytes as the two parts on the host
        long = dict(path="swing", frames=70, amount=12.0, edge=0.05)
        written = ie.run_parallax(pipe, data, samples[:1], str(tmp_path / "long"), ie.FileNameMode.id, "depth", 1, processing_res=48, **long)
        pred = pipe.predict_batch_device(batch[:1], "depth", processing_res=48).cpu().numpy()
        assert len(written) == 1 and len(written[0]) == 70
        for first, end in ((0, 64), (64, 70)):
            want = pv.parallax_frames(batch[:1].numpy(), pred, frame_range=(first, end), **long)
            for k in (first, end - 1):
                assert same_bits(np.moveaxis(np.asarray(Image.open(written[0][k])), -1, 0), want[0, k - first])
        for bad in (dict(mode="matting"), dict(mode="normal"), dict(focus=0.5, focus_at=(1, 1)), dict(focus=2.0), dict(amount=130.0), dict(frames=65),
                    dict(match_input_res=False), dict(tiles="yes"), dict(focus_at=(128, 0)), dict(path="wiggle"), dict(path="dolly", zoom=2.5)):
            with pytest.raises(ValueError):
                pipe.parallax_batch_device(batch, **dict(dict(processing_res=48), **bad))
        with pytest.raises(ValueError):
            pipe.parallax_batch_device(batch.float(), processing_res=48)
        with pytest.raises(ValueError):
            ie.run_parallax(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "matting", processing_res=48)
        with pytest.raises(ValueError):
            ie.run_parallax(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", focus=[0.5, 0.5, 0.5], processing_res=48)
        with pytest.raises(ValueError):
            ie.run_parallax(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", amount=500.0, processing_res=48)
        with pytest.raises(ValueError):
            ie.run_parallax(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "depth", animate="mp4", processing_res=48)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
