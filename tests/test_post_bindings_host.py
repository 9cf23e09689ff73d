"""The checks the bindings of the post-processing ops share (engine._images_u8, _float32 / _float_maps, _same_batch, _post_dims), on CPU
tensors: every input of the table is refused with ValueError before the library is touched -- `engine.load_library` is replaced by a handle
that records every entry asked of it -- and the same calls with valid inputs pass every check and stop at the device assert.  The range of
`_post_dims` is tested on the helper, with integers.  Nothing is launched."""
import pytest
import torch

U8 = dict(dtype=torch.uint8)


def valid(op):
    """(binding name, positional arguments, keyword arguments, the argument that is the image, the one that is the prediction) of a valid call
    on 8 x 8 inputs; tile_merge takes no image."""
    image, maps = torch.zeros((1, 3, 8, 8), **U8), torch.full((1, 8, 8), 0.5)
    return dict(foreground=("foreground", [image, maps], {}, 0, 1),
                guided_upsample=("guided_upsample", [image, maps[:, None], torch.zeros((1, 3, 16, 16), **U8)], {}, 0, 1),
                tile_merge=("tile_merge", [maps[:, None], maps[:, None, None], [0], [0], 2], {}, None, 0),
                depth_geometry=("depth_geometry", [maps], dict(image=image), "image", 0),
                lens_blur=("lens_blur", [image, maps], dict(focus=0.5), 0, 1))[op]


OPS = ["foreground", "guided_upsample", "tile_merge", "depth_geometry", "lens_blur"]
IMAGE_CASES = dict(image_dtype=lambda: torch.zeros((1, 3, 8, 8)), image_rank2=lambda: torch.zeros((8, 8), **U8),
                   image_rank5=lambda: torch.zeros((1, 1, 3, 8, 8), **U8), image_channels=lambda: torch.zeros((1, 4, 8, 8), **U8),
                   shape_mismatch=lambda: torch.zeros((2, 3, 8, 8), **U8))     # (two images, the maps of one)
CASES = [(op, case) for op in OPS for case in list(IMAGE_CASES) + ["pred_dtype"] if op != "tile_merge" or case in ("pred_dtype", "shape_mismatch")]


@pytest.fixture
def library_calls(monkeypatch):
    """engine.load_library gives a handle whose every entry records its name and fails; the list of those names."""
    from genpercept_amd import engine
    calls = []

    class Handle:
        def __getattr__(self, name):
            def entry(*args):
                calls.append(name)
                raise AssertionError(f"{name} was called")
            return entry

    monkeypatch.setattr(engine, "load_library", lambda *a, **k: Handle())
    return calls


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
