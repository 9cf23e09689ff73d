"""The depth geometry on the device (gp_depth_geometry): the point map, the normals, the keep bytes, the four point arrays and the offsets
BIT-EQUAL to the host route genpercept_amd/geometry.py (itself pinned to plain loops and to a CPU build of the kernels' arithmetic in
tests/test_geometry_host.py), over sizes that are multiples of nothing, windows up to r = 8, strides, both spaces, with and without mask and
image, a camera per image, a batch whose middle image is entirely invalid, tensors that start four bytes into their buffers; batch
independence and repeatability; NULL outputs; the argument checks with real buffers around them; the pipeline and the dataset loop with
`refine` and `tiles` at tiny widths.  There is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict  # noqa: E402
from test_geometry_host import PLANES, POINTS, call_geometry, geometry_args, invalid_cases, random_case  # noqa: E402

gpu = pytest.mark.gpu

# B, H, W, r, stride
CASES = [(1, 17, 23, 1, 1), (2, 40, 70, 2, 1), (1, 33, 200, 8, 3), (1, 64, 48, 2, 2), (3, 16, 16, 1, 1)]


def batch_case(seed, b, h, w, middle_invalid=False):
    rng = np.random.RandomState(seed)
    per = [random_case(rng, h, w) for _ in range(b)]
    pred, mask, image, cams = (np.stack([p[k] for p in per]) for k in range(4))
    if middle_invalid:
        pred[b // 2] = np.nan
    return pred[:, None], mask, image, cams


def to_host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def assert_same(got, want, what):
    for k in PLANES + POINTS + ("offsets",):
        assert same_bits(got[k], want[k]), (what, k, got[k].shape, want[k].shape)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-r%d-s%d" % s)
def test_planes_and_points_equal_the_host_route(case):
    from genpercept_amd import engine as ge
    from genpercept_amd import geometry as gm
    b, h, w, r, stride = case
    pred, mask, image, cams = batch_case(900 + h + w, b, h, w, middle_invalid=b == 3)
    assert len({tuple(c) for c in cams}) == b                                   # a different camera per image
    pred_d, mask_d, image_d = offset4(pred), offset4(mask), offset4(image)
    kept = 0
    for space in gm.SPACES:
        for use_mask, use_image in ((False, False), (True, True), (True, False)):
            kw = dict(space=space, radius=r, stride=stride)
            got = to_host(ge.depth_geometry(pred_d, cams, image_d if use_image else None, mask_d if use_mask else None, **kw))
            want = gm.depth_geometry(pred, cams, image if use_image else None, mask if use_mask else None, **kw)
            assert_same(got, want, (case, space, use_mask, use_image))
            kept += int(want["offsets"][-1])
            if b == 3:
                assert want["offsets"][1] == want["offsets"][2] and not want["keep"][1].any()
    assert kept > 0


@gpu
def test_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    for (b, h, w, r, stride), space in (((3, 40, 70, 2, 1), "depth"), ((3, 33, 75, 8, 3), "disparity")):
        pred, mask, image, cams = batch_case(21, b, h, w)
        pred_d, mask_d, image_d = torch.from_numpy(pred).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(image).cuda()
        kw = dict(space=space, radius=r, stride=stride)
        whole, again = (to_host(ge.depth_geometry(pred_d, cams, image_d, mask_d, **kw)) for _ in range(2))
        assert_same(whole, again, "twice")
        off = whole["offsets"]
        for i in range(b):
            one = to_host(ge.depth_geometry(pred_d[i], cams[i], image_d[i], mask_d[i:i + 1], **kw))
            for k in PLANES:
                assert same_bits(one[k][0], whole[k][i]), (i, k)
            for k in POINTS:
                assert same_bits(one[k], whole[k][off[i]:off[i + 1]]), (i, k)
            assert one["offsets"].tolist() == [0, off[i + 1] - off[i]]
        # float64 maps, boolean masks and cameras as a tensor are taken too
        other = to_host(ge.depth_geometry(pred_d.double()[:, 0], torch.from_numpy(cams), image_d, mask_d != 0, **kw))
        assert_same(other, whole, "other dtypes")
    for bad in (dict(space="metric"), dict(radius=9), dict(tau=0.0), dict(min_count=2), dict(min_cos=1.0), dict(stride=65), dict(cameras=cams[:2]),
                dict(image=image_d[:2]), dict(image=image_d.float()), dict(mask=mask_d[:, :5])):
        with pytest.raises(ValueError):
            ge.depth_geometry(pred_d, **dict(dict(cameras=cams), **bad))
    with pytest.raises(ValueError):
        ge.depth_geometry((pred_d * 255).to(torch.uint8), cams)


@gpu
def test_null_outputs_and_invalid_arguments_with_real_buffers():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill.  Then the
    valid set goes through with outputs that start four bytes into their buffers, and every subset of NULL outputs gives the same bits in
    what it does write."""
    from genpercept_amd import engine as ge
    from genpercept_amd import geometry as gm
    lib = ge.load_library()
    b, h, w, stride = 2, 40, 70, 1
    pred, mask, image, cams = batch_case(33, b, h, w)
    pred_d, mask_d, image_d = torch.from_numpy(pred).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(image).cuda()
    cap = b * h * w
    shapes = dict(xyz=((b, 3, h, w), np.float32), normal=((b, 3, h, w), np.float32), keep=((b, h, w), np.uint8), points=((cap, 3), np.float32),
                  point_normals=((cap, 3), np.float32), point_rgb=((cap, 3), np.uint8), point_index=((cap,), np.int32))

    def fresh():
        bufs = {k: offset4(np.full(shape, 0x5A if dt == np.uint8 else -7, dt)) for k, (shape, dt) in shapes.items()}
        bufs["offsets"] = torch.full((b + 1,), -7, dtype=torch.int64, device="cuda")
        return bufs

    bufs = fresh()
    ok, cams_ok = geometry_args(lib, b, h, w, stride, pred=pred_d.data_ptr(), mask=mask_d.data_ptr(), image=image_d.data_ptr(),
                                **{k: v.data_ptr() for k, v in bufs.items()})
    ws = torch.full((ok["nbytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    ok["ws"], ok["cams"] = ws.data_ptr(), cams.ctypes.data
    keep = [cams_ok]
    assert_refused_with_real_buffers(call_geometry, lib, ok, invalid_cases(ok, cams, keep), bufs, fresh)
    assert bool((ws == 0x5A).all())
    want = gm.depth_geometry(pred, cams, image, mask, "depth", ok["r"], ok["tau"], ok["min_count"], ok["min_cos"], stride)
    n = int(want["offsets"][-1])
    assert 0 < n < cap
    subsets = [(), ("xyz", "normal", "keep"), ("points", "point_normals", "point_rgb", "point_index"), ("xyz", "points"), ("normal", "point_normals", "keep"),
               ("xyz", "normal", "keep", "points", "point_normals", "point_rgb", "point_index", "offsets"), ("keep", "point_rgb", "point_index")]
    for null in subsets:
        bufs = fresh()
        args = dict(ok, **{k: v.data_ptr() for k, v in bufs.items()})
        args.update({k: None for k in null})
        if len(null) == 8:
            assert call_geometry(lib, args) == GP_ERR_INVALID      # no output at all
            continue
        assert call_geometry(lib, args) == 0, null
        torch.cuda.synchronize()
        untouched = fresh()
        for k in bufs:
            got = bufs[k].cpu().numpy()
            if k in null:
                assert torch.equal(bufs[k], untouched[k]), (null, k)
            elif k in POINTS:
                assert same_bits(got[:n], want[k]) and torch.equal(bufs[k][n:], untouched[k][n:]), (null, k)
            else:
                assert same_bits(got, want[k]), (null, k)


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    rec = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    assert len(rec) == n
    return rec["p"], rec["n"], rec["c"]


@gpu
def test_pointclouds_with_the_pipeline(tiny_weights, tmp_path):
    """Three 96 x 128 images at processing_res = 48: `pointcloud_batch_device` == geometry.py on the host applied to what
    `predict_batch_device` returns, bit for bit, for depth and disparity, plain, with `refine`, with `tiles` and with both, with the default
    camera and with one camera per image; `pointcloud` gives one image's cloud; `run_pointclouds` writes those points; what the entry does
    not take is refused."""
    from PIL import Image
    from genpercept_amd import geometry as gm
    from genpercept_amd import infer_eval as ie
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    tiles = dict(size=48, overlap=16, batch=4)
    cams = np.stack([gm.default_camera(96, 128, 40.0 + 10.0 * i) for i in range(3)])
    cams[:, 0], cams[:, 1] = (2.0, 0.5, 1.0), (0.5, 1.0, 0.25)
    try:
        clouds = {}
        default, own = (None, True), (cams, dict(radius=1, stride=2, tau=0.2, min_cos=0.05))
        extras = dict(plain={}, refine=dict(refine=True), tiles=dict(tiles=tiles), both=dict(refine=dict(radius=2), tiles=tiles))
        for mode, name, settings in (("depth", "plain", (default, own)), ("depth", "refine", (own,)), ("depth", "tiles", (default,)), ("depth", "both", (own,)),
                                     ("disparity", "plain", (default, own)), ("disparity", "tiles", (own,))):
            extra = extras[name]
            pred = pipe.predict_batch_device(batch, mode, processing_res=48, **extra)
            for cameras, pc in settings:
                got = pipe.pointcloud_batch_device(batch, mode, cameras, pc, processing_res=48, **extra)
                assert all(got[k].is_cuda for k in PLANES + POINTS) and torch.equal(got["pred"].view(torch.int32), pred.view(torch.int32))
                want = gm.depth_geometry(pred.cpu().numpy(), cameras, batch.numpy(), None, mode, **gm.pointcloud_options(pc))
                assert_same(to_host(got), want, (mode, name, pc))
                clouds[mode, name, pc is True] = want
        assert clouds["depth", "plain", True]["offsets"][-1] > 0 and clouds["depth", "plain", False]["offsets"][-1] > 0
        assert not same_bits(clouds["depth", "plain", True]["xyz"], clouds["depth", "tiles", True]["xyz"])
        want = clouds["depth", "plain", True]
        off = want["offsets"]
        one = pipe.pointcloud(Image.open(os.path.join(data, samples[1][0])), processing_res=48)
        lone = gm.depth_geometry(pipe.predict_batch_device(batch[1:2], "depth", processing_res=48).cpu().numpy(), None, batch[1:2].numpy())
        assert sorted(one) == sorted(POINTS) and all(same_bits(one[k], lone[k]) for k in POINTS)
        for kw, key in ((dict(), ("depth", "plain", True)), (dict(tiles=tiles), ("depth", "tiles", True))):
            written = ie.run_pointclouds(pipe, data, samples, str(tmp_path / ("ply" + "-".join(kw))), ie.FileNameMode.id, "depth", 3, processing_res=48, **kw)
            want, off = clouds[key], clouds[key]["offsets"]
            assert len(written) == 3 and all(p.endswith(".ply") for p in written)
            for i, path in enumerate(written):
                p, n, c = read_ply(path)
                assert same_bits(p, want["points"][off[i]:off[i + 1]]) and same_bits(n, want["point_normals"][off[i]:off[i + 1]])
                assert same_bits(c, want["point_rgb"][off[i]:off[i + 1]])
        for bad in (dict(mode="matting"), dict(mode="normal"), dict(pointcloud=dict(radius=9)), dict(pointcloud=False), dict(pointcloud=dict(r=2)),
                    dict(cameras=cams[:2]), dict(match_input_res=False), dict(tiles="yes")):
            with pytest.raises(ValueError):
                pipe.pointcloud_batch_device(batch, **dict(dict(processing_res=48), **bad))
        with pytest.raises(ValueError):
            pipe.pointcloud_batch_device(batch.float(), processing_res=48)
        with pytest.raises(ValueError):
            ie.run_pointclouds(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, "matting", processing_res=48)
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
