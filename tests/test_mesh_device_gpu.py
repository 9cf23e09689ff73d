"""The triangle mesh from depth on the device (gp_depth_mesh behind engine.depth_mesh): the planes, the six mesh arrays and both offset
arrays BIT-EQUAL to the host route genpercept_amd/mesh.py (itself pinned to plain loops and to a CPU build of the kernels' arithmetic in
tests/test_mesh_host.py), over grids of 64, 65 and more nodes a row with a partial last segment, strides, both spaces, with and without mask
and image, a camera per image, a batch whose middle image is entirely invalid, grids without cells, tensors that start four bytes into their
buffers; batch independence and repeatability; NULL outputs; the argument checks with real buffers around them; the pipeline and the
dataset loop with `refine` and `tiles` at tiny widths.  There is no tolerance in this file."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import GP_ERR_INVALID, assert_refused_with_real_buffers, offset4, same_bits, tiny_weights_dict  # noqa: E402
from test_geometry_host import PLANES, random_case  # noqa: E402
from test_mesh_host import MESH, OFFSETS, call_mesh, invalid_cases, mesh_args, parse_glb, read_mesh_ply  # noqa: E402

gpu = pytest.mark.gpu

# B, H, W, r, stride
CASES = [(1, 17, 23, 1, 1), (2, 40, 70, 2, 1), (1, 33, 200, 8, 3), (1, 64, 48, 2, 2), (3, 16, 16, 1, 1), (1, 5, 64, 1, 1), (1, 5, 65, 1, 1),
         (1, 3, 129, 1, 2),      # gw = 65
         (1, 9, 150, 1, 1),      # three segments, the last partial
         (1, 1, 70, 1, 1), (1, 7, 1, 1, 1), (1, 5, 9, 1, 64)]    # no cells
NO_CELLS = CASES[-3:]


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
    for k in PLANES + MESH + OFFSETS:
        assert same_bits(got[k], want[k]), (what, k, got[k].shape, want[k].shape)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%d-r%d-s%d" % s)
def test_planes_mesh_and_offsets_equal_the_host_route(case):
    from genpercept_amd import engine as ge
    from genpercept_amd import mesh as ms
    b, h, w, r, stride = case
    # (the 17 x 23 case is the coverage scene of the host test: every code and an unused kept node)
    pred, mask, image, cams = batch_case(940 if (h, w) == (17, 23) else 900 + h + w, b, h, w, middle_invalid=b == 3)
    assert len({tuple(c) for c in cams}) == b                                   # a different camera per image
    pred_d, mask_d, image_d = offset4(pred), offset4(mask), offset4(image)
    faces = 0
    for space in ms.geometry.SPACES:
        for use_mask, use_image, cut in ((False, False, 0.05), (True, True, 0.05), (True, False, 0.2), (False, True, 0.2)):
            kw = dict(space=space, radius=r, stride=stride, cut=cut)
            got = ge.depth_mesh(pred_d, cams, image_d if use_image else None, mask_d if use_mask else None, **kw)
            assert all(got[k].is_cuda for k in PLANES + MESH) and all(isinstance(got[k], np.ndarray) for k in OFFSETS)
            want = ms.depth_mesh(pred, cams, image if use_image else None, mask if use_mask else None, **kw)
            assert_same(to_host(got), want, (case, space, use_mask, use_image, cut))
            faces += int(want["face_offsets"][-1])
            if b == 3:
                assert want["vertex_offsets"][1] == want["vertex_offsets"][2] and want["face_offsets"][1] == want["face_offsets"][2] and want["face_offsets"][1] > 0
    assert (faces == 0) == (case in NO_CELLS)


@gpu
def test_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    for (b, h, w, r, stride), space in (((3, 40, 70, 2, 1), "depth"), ((3, 33, 150, 1, 2), "disparity")):
        pred, mask, image, cams = batch_case(21, b, h, w)
        pred_d, mask_d, image_d = torch.from_numpy(pred).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(image).cuda()
        kw = dict(space=space, radius=r, stride=stride, cut=0.2)
        whole, again = (to_host(ge.depth_mesh(pred_d, cams, image_d, mask_d, **kw)) for _ in range(2))
        assert_same(whole, again, "twice")
        vo, fo = whole["vertex_offsets"], whole["face_offsets"]
        assert fo[-1] > 0
        for i in range(b):
            one = to_host(ge.depth_mesh(pred_d[i], cams[i], image_d[i], mask_d[i:i + 1], **kw))
            for k in PLANES:
                assert same_bits(one[k][0], whole[k][i]), (i, k)
            for k in MESH:
                off = fo if k == "faces" else vo
                assert same_bits(one[k], whole[k][off[i]:off[i + 1]]), (i, k)      # (the batch's face indices are already local)
            assert one["vertex_offsets"].tolist() == [0, vo[i + 1] - vo[i]] and one["face_offsets"].tolist() == [0, fo[i + 1] - fo[i]]
    for bad in (dict(space="metric"), dict(radius=9), dict(tau=0.0), dict(stride=65), dict(cut=0.0), dict(cut=float("nan")), dict(cut=1.5),
                dict(cameras=cams[:2]), dict(image=image_d[:2]), dict(image=image_d.float()), dict(mask=mask_d[:, :5])):
        with pytest.raises(ValueError):
            ge.depth_mesh(pred_d, **dict(dict(cameras=cams), **bad))


@gpu
def test_null_outputs_and_invalid_arguments_with_real_buffers():
    """The host test's invalid cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill.  Then the
    valid set goes through with arrays that start four bytes into their buffers, and every subset of NULL outputs gives the same bits in
    what it does write and nothing past n and m; with all arrays NULL the two offset arrays equal the full call's."""
    from genpercept_amd import engine as ge
    from genpercept_amd import mesh as ms
    lib = ge.load_library()
    b, h, w, stride, cut = 2, 40, 70, 1, 0.2
    pred, mask, image, cams = batch_case(33, b, h, w)
    want = ms.depth_mesh(pred, cams, image, mask, "depth", radius=2, stride=stride, cut=cut)
    n, m = int(want["vertex_offsets"][-1]), int(want["face_offsets"][-1])
    n_cap, m_cap = b * h * w, 2 * b * (h - 1) * (w - 1)
    assert 0 < n < n_cap and 0 < m < m_cap
    xyz_d, normal_d, keep_d, image_d = offset4(want["xyz"]), offset4(want["normal"]), offset4(want["keep"]), offset4(image)
    shapes = dict(vertices=((n_cap, 3), np.float32), vertex_normals=((n_cap, 3), np.float32), vertex_rgb=((n_cap, 3), np.uint8),
                  vertex_uv=((n_cap, 2), np.float32), vertex_index=((n_cap,), np.int32), faces=((m_cap, 3), np.int32))

    def fresh():
        bufs = {k: offset4(np.full(shape, 0x5A if dt == np.uint8 else -7, dt)) for k, (shape, dt) in shapes.items()}
        for k in OFFSETS:
            bufs[k] = torch.full((b + 1,), -7, dtype=torch.int64, device="cuda")
        return bufs

    bufs = fresh()
    ok = mesh_args(lib, b, h, w, stride, xyz=xyz_d.data_ptr(), normal=normal_d.data_ptr(), keep=keep_d.data_ptr(), image=image_d.data_ptr(), cut=cut,
                   **{k: v.data_ptr() for k, v in bufs.items()})
    ws = torch.full((ok["nbytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    ok["ws"] = ws.data_ptr()
    assert_refused_with_real_buffers(call_mesh, lib, ok, invalid_cases(ok), bufs, fresh)
    assert bool((ws == 0x5A).all())
    subsets = [(), MESH, ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "vertex_index"), ("faces",), ("vertices", "faces"),
               ("vertex_normals", "vertex_uv"), ("vertex_rgb", "vertex_index", "faces"), ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "faces")]
    for null in subsets:
        bufs = fresh()
        args = dict(ok, **{k: v.data_ptr() for k, v in bufs.items()})
        args.update({k: None for k in null})
        assert call_mesh(lib, args) == 0, null
        torch.cuda.synchronize()
        untouched = fresh()
        for k in bufs:
            got = bufs[k].cpu().numpy()
            count = m if k == "faces" else n
            if k in null:
                assert torch.equal(bufs[k], untouched[k]), (null, k)
            elif k in MESH:
                assert same_bits(got[:count], want[k]) and torch.equal(bufs[k][count:], untouched[k][count:]), (null, k)
            else:
                assert same_bits(got, want[k]), (null, k)                        # both offset arrays, with every subset
    # without the normal input: refused with vertex_normals, the same bits in the rest without it
    bufs = fresh()
    args = dict(ok, **{k: v.data_ptr() for k, v in bufs.items()})
    assert call_mesh(lib, dict(args, normal=None)) == GP_ERR_INVALID
    assert call_mesh(lib, dict(args, normal=None, vertex_normals=None, image=None)) == 0
    torch.cuda.synchronize()
    assert all(same_bits(bufs[k].cpu().numpy()[:m if k == "faces" else n], want[k]) for k in ("vertices", "vertex_uv", "vertex_index", "faces"))
    assert bool((bufs["vertex_rgb"][:n] == 255).all()) and torch.equal(bufs["vertex_normals"], fresh()["vertex_normals"])


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_meshes_with_the_pipeline(tiny_weights, tmp_path):
    """Three 96 x 128 images at processing_res = 48: `mesh_batch_device` == mesh.py on the host applied to what `predict_batch_device`
    returns, bit for bit, for depth and disparity, plain, with `refine`, with `tiles` and with both, with the default camera and with one
    camera per image; `mesh` gives one image's arrays; `run_meshes` writes .glb and .ply files that hold those arrays; what the entries do not
    take is refused."""
    from PIL import Image
    from genpercept_amd import geometry as gm
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import mesh as ms
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data = str(tmp_path / "data")
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    tiles = dict(size=48, overlap=16, batch=4)
    cams = np.stack([gm.default_camera(96, 128, 40.0 + 10.0 * i) for i in range(3)])
    cams[:, 0], cams[:, 1] = (2.0, 0.5, 1.0), (0.5, 1.0, 0.25)
    try:
        meshes = {}
        default, own = (None, True), (cams, dict(radius=1, stride=2, tau=0.2, min_cos=0.05, cut=0.2))
        extras = dict(plain={}, refine=dict(refine=True), tiles=dict(tiles=tiles), both=dict(refine=dict(radius=2), tiles=tiles))
        for mode, name, settings in (("depth", "plain", (default, own)), ("depth", "refine", (own,)), ("depth", "tiles", (default,)), ("depth", "both", (own,)),
                                     ("disparity", "plain", (default, own)), ("disparity", "tiles", (own,))):
            extra = extras[name]
            pred = pipe.predict_batch_device(batch, mode, processing_res=48, **extra)
            for cameras, opt in settings:
                got = pipe.mesh_batch_device(batch, mode, cameras, opt, processing_res=48, **extra)
                assert all(got[k].is_cuda for k in PLANES + MESH) and torch.equal(got["pred"].view(torch.int32), pred.view(torch.int32))
                want = ms.depth_mesh(pred.cpu().numpy(), cameras, batch.numpy(), None, mode, **ms.mesh_options(opt))
                assert_same(to_host(got), want, (mode, name, opt))
                meshes[mode, name, opt is True] = want
        assert meshes["depth", "plain", True]["face_offsets"][-1] > 0 and meshes["depth", "plain", False]["face_offsets"][-1] > 0
        one = pipe.mesh(Image.open(os.path.join(data, samples[1][0])), processing_res=48)
        lone = ms.depth_mesh(pipe.predict_batch_device(batch[1:2], "depth", processing_res=48).cpu().numpy(), None, batch[1:2].numpy())
        assert sorted(one) == sorted(MESH) and all(same_bits(one[k], lone[k]) for k in MESH)
        for fmt, kw, key in (("glb", dict(), ("depth", "plain", True)), ("ply", dict(), ("depth", "plain", True)), ("glb", dict(tiles=tiles), ("depth", "tiles", True))):
            written = ie.run_meshes(pipe, data, samples, str(tmp_path / (fmt + "-".join(kw))), ie.FileNameMode.id, "depth", 3, format=fmt, processing_res=48, **kw)
            want, vo, fo = meshes[key], meshes[key]["vertex_offsets"], meshes[key]["face_offsets"]
            assert len(written) == 3 and all(p.endswith("." + fmt) for p in written)
            for i, path in enumerate(written):
                vert, nrm, rgb, uv = (want[k][vo[i]:vo[i + 1]] for k in ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv"))
                faces = want["faces"][fo[i]:fo[i + 1]]
                if fmt == "ply":
                    p, n, c, fv = read_mesh_ply(path)
                    assert same_bits(p, vert) and same_bits(n, nrm) and same_bits(c, rgb) and same_bits(np.ascontiguousarray(fv), faces, np.int32)
                    continue
                doc, accessor, view = parse_glb(path)
                (prim,) = doc["meshes"][0]["primitives"]
                att = prim["attributes"]
                assert same_bits(accessor(att["POSITION"]), np.stack([vert[:, 0], -vert[:, 1], -vert[:, 2]], 1), np.float32)
                assert same_bits(accessor(att["NORMAL"]), np.stack([nrm[:, 0], -nrm[:, 1], -nrm[:, 2]], 1), np.float32)
                assert same_bits(accessor(att["TEXCOORD_0"]), uv, np.float32) and np.array_equal(accessor(prim["indices"]).reshape(-1, 3), faces)
                png = np.asarray(Image.open(io.BytesIO(view(doc["images"][0]["bufferView"]))))
                assert np.array_equal(png, batch[i].permute(1, 2, 0).numpy())       # textured with the sample's own image
        for bad in (dict(mode="matting"), dict(mode="normal"), dict(mesh=False), dict(mesh=dict(r=2)), dict(mesh=dict(cut=0)), dict(mesh=dict(radius=9)),
                    dict(cameras=cams[:2]), dict(match_input_res=False), dict(tiles="yes")):
            with pytest.raises(ValueError):
                pipe.mesh_batch_device(batch, **dict(dict(processing_res=48), **bad))
        with pytest.raises(ValueError):
            pipe.mesh_batch_device(batch.float(), processing_res=48)
        for bad in (dict(mode="matting"), dict(format="obj"), dict(mesh=dict(cut=0))):
            with pytest.raises(ValueError):
                ie.run_meshes(pipe, data, samples, str(tmp_path / "bad"), ie.FileNameMode.id, **dict(dict(processing_res=48), **bad))
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
