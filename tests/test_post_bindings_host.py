"""The checks the bindings of the post-processing ops share (engine._images_u8, _float32 / _float_maps, _same_batch, _post_dims), on CPU
tensors: every input of the table is refused with ValueError before the library is touched -- `engine.load_library` is replaced by a handle
that records every entry asked of it -- and the same calls with valid inputs pass every check and stop at the device assert.  The range of
`_post_dims` is tested on the helper, with integers; `_nearness_plane`, the plane of lens_blur, stereo_views and parallax_frames as a device
tensor, on CPU tensors against `post_common.nearness`, bit for bit.  Nothing is launched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402

U8 = dict(dtype=torch.uint8)


def valid(op):
    """(binding name, positional arguments, keyword arguments, the argument that is the image, the one that is the prediction) of a valid call
    on 8 x 8 inputs; tile_merge takes no image."""
    image, maps = torch.zeros((1, 3, 8, 8), **U8), torch.full((1, 8, 8), 0.5)
    return dict(foreground=("foreground", [image, maps], {}, 0, 1),
                guided_upsample=("guided_upsample", [image, maps[:, None], torch.zeros((1, 3, 16, 16), **U8)], {}, 0, 1),
                tile_merge=("tile_merge", [maps[:, None], maps[:, None, None], [0], [0], 2], {}, None, 0),
                depth_geometry=("depth_geometry", [maps], dict(image=image), "image", 0),
                lens_blur=("lens_blur", [image, maps], dict(focus=0.5), 0, 1),
                stereo_views=("stereo_views", [image, maps], dict(converge_at=(7, 7), want_near=True), 0, 1),
                parallax_frames=("parallax_frames", [image, maps], dict(frames=4, amount=1.0, overscan=False, want_holes=True), 0, 1))[op]


OPS = ["foreground", "guided_upsample", "tile_merge", "depth_geometry", "lens_blur", "stereo_views", "parallax_frames"]
IMAGE_CASES = dict(image_dtype=lambda: torch.zeros((1, 3, 8, 8)), image_rank2=lambda: torch.zeros((8, 8), **U8),
                   image_rank5=lambda: torch.zeros((1, 1, 3, 8, 8), **U8), image_channels=lambda: torch.zeros((1, 4, 8, 8), **U8),
                   shape_mismatch=lambda: torch.zeros((2, 3, 8, 8), **U8))     # (two images, the maps of one)
CASES = [(op, case) for op in OPS for case in list(IMAGE_CASES) + ["pred_dtype"] if op != "tile_merge" or case in ("pred_dtype", "shape_mismatch")]


@pytest.fixture
def library_calls(monkeypatch):
    return ps.library_calls(monkeypatch)


def call(name, args, kwargs):
    from genpercept_amd import engine
    return getattr(engine, name)(*args, **kwargs)


@pytest.mark.parametrize("op,case", CASES, ids=lambda v: v)
def test_bad_inputs_are_refused_before_the_library_is_touched(op, case, library_calls):
    name, args, kwargs, image_at, pred_at = valid(op)
    if case == "pred_dtype":
        args[pred_at] = torch.zeros(tuple(args[pred_at].shape), dtype=torch.int32)
    elif image_at is None:                                          # tile_merge: two bases, the tiles of one
        args[0] = torch.full((2, 1, 8, 8), 0.5)
    elif isinstance(image_at, str):
        kwargs[image_at] = IMAGE_CASES[case]()
    else:
        args[image_at] = IMAGE_CASES[case]()
    with pytest.raises(ValueError):
        call(name, args, kwargs)
    assert library_calls == []


@pytest.mark.parametrize("op", OPS)
def test_valid_inputs_pass_every_check(op, library_calls):
    """The valid sets the cases above change: on CPU tensors they get as far as the assert that the tensors are on the device."""
    name, args, kwargs, _, _ = valid(op)
    with pytest.raises(AssertionError):
        call(name, args, kwargs)
    assert library_calls == []


@pytest.mark.parametrize("dims,ok", [((1, 16384, 8), True), ((1, 8, 16384), True), ((1, 16385, 8), False), ((1, 8, 16385), False), ((65535, 8, 8), True),
                                     ((65536, 8, 8), False), ((8, 16384, 16384), False), ((7, 16384, 16384), True), ((0, 8, 8), False), ((1, 0, 8), False)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_post_dims_range(dims, ok):
    from genpercept_amd.engine import _post_dims
    if ok:
        assert _post_dims(*dims, "the op") is None
        return
    with pytest.raises(ValueError):
        _post_dims(*dims, "the op")
    if dims == (8, 16384, 16384):                                   # B * H * W = 2^31 is over the count limit only
        assert _post_dims(*dims, "the op", count_limit=False) is None


# ---- the plane of lens_blur, stereo_views and parallax_frames ---------------------------------------------------------------------------------------
def plane_maps():
    """Maps float32 [2, 3, 5] with the values the 16-bit rule turns on: 0, 1, below 0, above 1, a NaN, one step of the scale, the middle, the
    last float below 1; (the maps, the (u, v) of the NaN in map 0)."""
    below_one = np.nextafter(np.float32(1), np.float32(0))
    maps = np.linspace(0.05, 0.95, 30, dtype=np.float32).reshape(2, 3, 5)
    maps[0, 0, :4] = [0.0, 1.0, -0.25, 1.75]
    maps[0, 1, 2] = np.nan
    maps[1, 2, 1:4] = [np.float32(1) / np.float32(65535), 0.5, below_one]
    return maps, (2, 1)


@pytest.mark.parametrize("space", ["depth", "disparity"])
def test_nearness_plane_equals_the_host_rule_bit_for_bit(space):
    from genpercept_amd.engine import _nearness_plane
    from genpercept_amd.post_common import F_DEFAULT, nearness
    maps, nan_at = plane_maps()
    pred = torch.from_numpy(maps)

    def same(got, want):
        return got.dtype == torch.int32 and tuple(got.shape) == (2,) and got.is_contiguous() and ps.same_bits(got.numpy().astype(np.int64), want)

    # a value plane: every value of the maps, two at a time, float32 [B] as the parser hands them over (which lets none outside [0, 1] pass;
    # the arithmetic is the pixel plane's and clamps them all the same)
    flat = maps.reshape(-1)
    for k in range(0, flat.size, 2):
        value = flat[k:k + 2].copy()
        assert same(_nearness_plane(pred, value, None, space, F_DEFAULT), nearness(value, space)), value
    assert _nearness_plane(pred, np.float32([np.nan, 0.25]), None, space).tolist() == [0, 16383 if space == "disparity" else 65535 - 16383]
    # a pixel plane: every pixel, read from the map of its own image; the NaN gives 0 in both spaces
    for v in range(3):
        for u in range(5):
            at = np.array([[u, v], [4 - u, 2 - v]], np.int64)
            want = nearness(np.float32([maps[0, v, u], maps[1, 2 - v, 4 - u]]), space)
            assert same(_nearness_plane(pred, None, at, space, F_DEFAULT), want), (u, v)
    at_nan = np.array([nan_at, nan_at], np.int64)
    assert _nearness_plane(pred, None, at_nan, space).tolist() == [0, int(nearness(maps[1, nan_at[1], nan_at[0]], space))]
    # out-of-range values read from the map are clamped, not refused
    ends = _nearness_plane(pred, None, np.array([[2, 0], [3, 2]], np.int64), space).tolist()
    assert ends == ([0, 65534] if space == "disparity" else [65535, 1])
    # the default plane
    assert same(_nearness_plane(pred, None, None, space, F_DEFAULT), np.full(2, 32768, np.int64))
    assert _nearness_plane(pred, None, None, space, 7).tolist() == [7, 7]
