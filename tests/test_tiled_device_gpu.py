"""The tile merge on the device (gp_tile_merge): outputs and fits BIT-EQUAL to the host route genpercept_amd/tiled.py (itself pinned to plain
loops and to a CPU build of the kernels' arithmetic in tests/test_tiled_host.py), over grids of one tile, one row of tiles, 121 tiles with
pixels under four of them, sizes that are multiples of nothing, both alignments, C = 1 and 3, flat tiles and NaNs, tensors that start four
bytes into their buffers; batch independence and repeatability; the argument checks with real buffers around them; the pipeline, the cutouts
and the dataset loops with `tiles` at tiny widths.  There is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_support as ps  # noqa: E402
from post_support import assert_refused_with_real_buffers, bits, offset4, same_bits64, tiny_weights_dict  # noqa: E402
from test_tiled_host import call_merge, invalid_cases, merge_args, random_case, same_bits  # noqa: E402

gpu = pytest.mark.gpu

# B, C, H, W, T, o, align
CASES = [(1, 1, 40, 40, 40, 8, "least_square"), (2, 1, 70, 101, 32, 8, "least_square"), (1, 3, 65, 130, 64, 32, "none"), (1, 1, 96, 96, 16, 8, "least_square"),
         (1, 1, 33, 200, 33, 16, "least_square"), (2, 3, 50, 77, 24, 5, "least_square")]


def batch_case(seed, b, c, h, w, size, o, odd=True):
    rng = np.random.RandomState(seed)
    per = [random_case(rng, c, h, w, size, o, odd) for _ in range(b)]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), per[0][2], per[0][3]


def check(base, tiles, ys, xs, o, align, what):
    from genpercept_amd import engine as ge
    from genpercept_amd import tiled
    got, fit = ge.tile_merge(offset4(base), offset4(tiles), ys, xs, o, align, want_fit=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == base.shape and fit.dtype == torch.float64 and tuple(fit.shape) == tiles.shape[:2] + (2,)
    got, fit = got.cpu().numpy(), fit.cpu().numpy()
    for i in range(base.shape[0]):
        want = tiled.tile_merge(base[i], tiles[i], ys, xs, o, align)
        s, t = tiled.tile_fit(base[i], tiles[i], ys, xs, align)
        assert same_bits64(fit[i, :, 0], s) and same_bits64(fit[i, :, 1], t), (what, i, fit[i, :3], s[:3], t[:3])
        assert same_bits(got[i], want), (what, i, int((got[i].view(np.uint32) != want.view(np.uint32)).sum()), float(np.nanmax(np.abs(got[i] - want))))


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda s: "%dx%dx%dx%d-T%d-o%d-%s" % s)
def test_output_and_fit_equal_the_host_route(case):
    from genpercept_amd import tiled
    b, c, h, w, size, o, align = case
    base, tiles, ys, xs = batch_case(900 + h + w, b, c, h, w, size, o)
    assert tiles.shape[1] == {40: 1, 70: 12, 65: 8, 96: 121, 33: 11, 50: 12}[h]
    check(base, tiles, ys, xs, o, align, case)
    other = [a for a in tiled.ALIGNMENTS if a != align][0]
    check(base, tiles, ys, xs, o, other, case)                      # ... and the alignment the issue's list does not name for this grid
    clean = batch_case(901 + h + w, b, c, h, w, size, o, odd=False)
    check(*clean, o, align, (case, "no odd values"))


@gpu
def test_flat_tiles_and_nans():
    """A batch whose first image holds a flat tile, a tile flat to within one 16-bit step, an anti-correlated tile, a tile of NaNs and one NaN
    in an ordinary tile; the second image is an ordinary one with a NaN in its base."""
    from genpercept_amd import tiled
    rng = np.random.RandomState(77)
    base, tiles, ys, xs = batch_case(78, 2, 1, 40, 56, 24, 8, odd=False)
    wh, ww = tiles.shape[-2:]
    t0 = tiles[0]
    t0[0] = 0.4
    t0[1] = np.float32(0.4) + (rng.rand(1, wh, ww) < 0.5) * np.float32(1.0 / 65535.0)
    t0[2] = 1.0 - base[0][:, int(ys[0]):int(ys[0]) + wh, int(xs[2]):int(xs[2]) + ww]
    t0[3] = np.nan
    t0[4, 0, 10, 12] = np.nan
    base[1, 0, 7, 9] = np.nan
    s, _ = tiled.tile_fit(base[0], tiles[0], ys, xs)
    assert s[0] == s[1] == s[2] == s[3] == 1.0 and s[4] != 1.0 and s[5] != 1.0
    check(base, tiles, ys, xs, 8, "least_square", "degenerate")
    check(base, tiles, ys, xs, 8, "none", "degenerate")


@gpu
def test_stable_and_batch_independent():
    from genpercept_amd import engine as ge
    for (h, w, size, o), c, align in (((70, 101, 32, 8), 1, "least_square"), ((50, 77, 24, 5), 3, "least_square"), ((65, 130, 64, 32), 3, "none")):
        base, tiles, ys, xs = batch_case(21, 3, c, h, w, size, o)
        base_d, tiles_d = torch.from_numpy(base).cuda(), torch.from_numpy(tiles).cuda()
        (whole, fit), (again, fit2) = (ge.tile_merge(base_d, tiles_d, ys, xs, o, align, want_fit=True) for _ in range(2))
        assert torch.equal(whole.view(torch.int32), again.view(torch.int32)) and torch.equal(fit.view(torch.int64), fit2.view(torch.int64))
        for i in range(3):
            one, f1 = ge.tile_merge(base_d[i], tiles_d[i], ys, xs, o, align, want_fit=True)
            assert torch.equal(one[0].view(torch.int32), whole[i].view(torch.int32)) and torch.equal(f1[0].view(torch.int64), fit[i].view(torch.int64))
        assert float(whole.min()) >= 0.0 and float(whole.max()) <= 1.0
        assert torch.equal(ge.tile_merge(base_d.double(), tiles_d.double(), ys, xs, o, align), ge.tile_merge(base_d, tiles_d, ys.tolist(), torch.from_numpy(xs), o, align))
    for args in ((base_d, tiles_d, ys, xs, o, "affine"), (base_d, tiles_d, ys + 1, xs, o, align), (base_d, tiles_d, ys, xs, o + 1, align),
                 (base_d, tiles_d[:, :-1], ys, xs, o, align), (base_d[:2], tiles_d, ys, xs, o, align), (base_d[:, :1], tiles_d, ys, xs, o, align),
                 ((base_d * 255).to(torch.uint8), tiles_d, ys, xs, o, align), (base_d, tiles_d, ys.astype(np.float32), xs, o, align)):
        with pytest.raises(ValueError):
            ge.tile_merge(*args)


@gpu
def test_refuses_invalid_arguments_before_touching_the_device():
    """The host test's cases once more with real device buffers around them: GP_ERR_INVALID, and the buffers keep their fill.  Then the valid
    set goes through with an output that starts four bytes into its buffer."""
    from genpercept_amd import engine as ge
    from genpercept_amd import tiled
    lib = ge.load_library()
    b, c, h, w, size, o = 2, 1, 70, 101, 32, 8
    base, tiles, ys, xs = batch_case(33, b, c, h, w, size, o)
    base_d, tiles_d = torch.from_numpy(base).cuda(), torch.from_numpy(tiles).cuda()
    out_buf = torch.full((b * c * h * w + 4,), -7.0, device="cuda")
    out = out_buf[1:1 + b * c * h * w].view(b, c, h, w)
    fit = torch.full((b, tiles.shape[1], 2), -7.0, dtype=torch.float64, device="cuda")
    ok, keep = merge_args(lib, b, c, h, w, size, o, base=base_d.data_ptr(), tiles=tiles_d.data_ptr(), out=out.data_ptr(), fit=fit.data_ptr())
    ws = torch.full((ok["nbytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    ok["ws"] = ws.data_ptr()
    keep = list(keep)
    assert_refused_with_real_buffers(call_merge, lib, ok, invalid_cases(ok, keep))
    assert bool((out_buf == -7.0).all() and (ws == 0x5A).all() and (fit == -7.0).all())
    assert out.data_ptr() % 16 == 4 and call_merge(lib, ok) == 0      # ... and the valid set goes through
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(b):
        assert same_bits(got[i], tiled.tile_merge(base[i], tiles[i], ys, xs, o))
    assert float(out_buf[0]) == -7.0 and bool((out_buf[1 + b * c * h * w:] == -7.0).all())
    assert call_merge(lib, dict(ok, fit=None, align=1)) == 0            # fit_out is optional
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy()[1], tiled.tile_merge(base[1], tiles[1], ys, xs, o, "none"))


@pytest.fixture(scope="module")
def tiny_weights():
    return tiny_weights_dict()


@gpu
def test_tiles_with_the_pipeline(tiny_weights, tmp_path, monkeypatch):
    """Three 96 x 128 images at processing_res = 48 with tiles of 48, overlap 16 (3 x 4 windows per image, 36 crops in nine passes of four):
    `predict_batch_device(..., tiles=...)` == tiled.py on the host applied to the plain prediction and to the predictions of the same crops sent
    through `predict_batch_device` in the same chunks, bit for bit, for depth (least_square) and matting (none); the plain call is unchanged;
    `infer_batch`, `__call__` and the host route agree; the cutouts are those of the tiled alpha; `run_inference` writes those values; with
    `refine` the base is the refined map; what `tiles` does not take is refused."""
    from PIL import Image
    from genpercept_amd import foreground as fgh
    from genpercept_amd import infer_eval as ie
    from genpercept_amd import tiled
    pipe, g = ps.tiny_pipeline(tiny_weights, 51)
    data, npy, ev0, ev1 = (str(tmp_path / d) for d in ("data", "npy", "ev0", "ev1"))
    samples, batch = ps.write_png_dataset(data, g, 3, 96, 128)
    os.makedirs(os.path.join(data, "set0", "gt"), exist_ok=True)
    for i, smp in enumerate(samples):
        xx = np.arange(128)[None].repeat(96, 0)
        Image.fromarray(np.clip((xx - (40 + 10 * i)) * 6 + 128, 0, 255).astype(np.uint8)).save(os.path.join(data, "set0", "gt", f"{i:04d}.png"))
        smp.append(f"set0/gt/{i:04d}.png")
    opts = dict(size=48, overlap=16, batch=4)
    ys, xs, wh, ww = tiled.tile_grid(96, 128, 48, 16)
    assert (len(ys), len(xs), wh, ww) == (3, 4, 48, 48)
    crops = torch.stack([batch[i, :, y0:y0 + wh, x0:x0 + ww] for i in range(3) for y0 in ys for x0 in xs])

    def tile_predictions(predict):
        return np.concatenate([predict(crops[j:j + 4]) for j in range(0, len(crops), 4)]).reshape(3, 12, -1, wh, ww)

    def device(x, mode, **kw):
        return pipe.predict_batch_device(x, mode, processing_res=48, **kw)

    try:
        tiled_maps, tile_maps = {}, {}
        for mode, align in (("depth", "least_square"), ("matting", "none")):
            plain = device(batch, mode)
            got = device(batch, mode, tiles=opts)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 1, 96, 128)
            assert torch.equal(bits(device(batch, mode)), bits(plain))
            tp = tile_predictions(lambda x: device(x, mode).cpu().numpy())
            assert len(np.unique(tp)) > 16
            plain_np, got_np = plain.cpu().numpy(), got.cpu().numpy()
            for i in range(3):
                assert same_bits(got_np[i], tiled.tile_merge(plain_np[i], tp[i], ys, xs, 16, align)), (mode, i)
            assert not torch.equal(bits(got), bits(plain))
            assert torch.equal(bits(device(batch, mode, tiles=dict(opts, align=align))), bits(got))   # the default alignment of the mode
            tiled_maps[mode], tile_maps[mode] = got, tp
        # ---- three channels, and the other alignment on request
        got = device(batch, "normal", tiles=opts).cpu().numpy()
        plain_np, tp = device(batch, "normal").cpu().numpy(), tile_predictions(lambda x: device(x, "normal").cpu().numpy())
        assert got.shape == (3, 3, 96, 128) and all(same_bits(got[i], tiled.tile_merge(plain_np[i], tp[i], ys, xs, 16, "none")) for i in range(3))
        got = device(batch, "matting", tiles=dict(opts, align="least_square", batch=5)).cpu().numpy()
        plain_np = device(batch, "matting").cpu().numpy()
        tp5 = np.concatenate([device(crops[j:j + 5], "matting").cpu().numpy() for j in range(0, 36, 5)]).reshape(3, 12, 1, wh, ww)
        assert all(same_bits(got[i], tiled.tile_merge(plain_np[i], tp5[i], ys, xs, 16, "least_square")) for i in range(3))
        # ---- with refine: the base is the refined map, the tiles are not refined
        got = device(batch, "matting", refine=True, tiles=opts).cpu().numpy()
        refined = device(batch, "matting", refine=True).cpu().numpy()
        assert all(same_bits(got[i], tiled.tile_merge(refined[i], tile_maps["matting"][i], ys, xs, 16, "none")) for i in range(3))
        # ---- infer_batch and __call__, on the device route and on the host route
        outs = pipe.infer_batch(batch, "depth", processing_res=48, color_map=None, tiles=opts)
        for i in range(3):
            assert same_bits(outs[i].pred_np, tiled_maps["depth"][i, 0].cpu().numpy())
        one = pipe(Image.open(os.path.join(data, samples[1][0])), processing_res=48, color_map=None, mode="matting", tiles=opts)
        assert same_bits(one.pred_np, device(batch[1:2], "matting", tiles=opts)[0, 0].cpu().numpy())
        monkeypatch.setenv("GENPERCEPT_HOST_PREPOST", "1")

        def host(x, **kw):
            return np.stack([o.pred_np[None] for o in pipe.infer_batch(x, "depth", processing_res=48, color_map=None, **kw)])

        base_h, tp_h, outs_h = host(batch), tile_predictions(host), host(batch, tiles=opts)
        for i in range(3):
            assert same_bits(outs_h[i], tiled.tile_merge(base_h[i], tp_h[i], ys, xs, 16, "least_square"))
        with pytest.raises(ValueError):
            pipe.infer_batch(batch.float(), "depth", processing_res=48, color_map=None, tiles=opts)
        monkeypatch.delenv("GENPERCEPT_HOST_PREPOST")
        # ---- cutouts under the tiled alpha, and the dataset loops
        rgba, alpha = pipe.cutout_batch_device(batch, "matting", processing_res=48, tiles=opts)
        assert torch.equal(bits(alpha), bits(tiled_maps["matting"]))
        for i in range(3):
            assert np.array_equal(rgba[i].cpu().numpy(), fgh.cutout_rgba(batch[i].numpy(), alpha[i, 0].cpu().numpy()))
        assert not torch.equal(pipe.cutout_batch_device(batch, "matting", processing_res=48)[0], rgba)
        saved = ie.run_inference(pipe, data, samples, npy, ie.FileNameMode.id, "matting", processing_res=48, batch_size=3, tiles=opts)
        for i, path in enumerate(saved):
            assert same_bits(np.load(path), tiled_maps["matting"][i, 0].cpu().numpy())
        written = ie.run_cutouts(pipe, data, samples, str(tmp_path / "cut"), ie.FileNameMode.id, "matting", 3, processing_res=48, tiles=opts)
        for i, path in enumerate(written):
            assert np.array_equal(np.asarray(Image.open(path)), rgba[i].cpu().numpy())
        before = ie.infer_and_evaluate_masks(pipe, data, samples, "matting", output_dir=ev0, batch_size=3, processing_res=48)
        with_tiles = ie.infer_and_evaluate_masks(pipe, data, samples, "matting", output_dir=ev1, batch_size=3, processing_res=48, tiles=opts)
        assert list(before) == list(with_tiles) and any(np.float64(before[k]).tobytes() != np.float64(with_tiles[k]).tobytes() for k in before)
        # ---- what tiles does not take
        for bad in (dict(tiles=opts, match_input_res=False), dict(tiles="yes"), dict(tiles=dict(size=48, overlap=25)), dict(tiles=dict(tile=48)),
                    dict(tiles=dict(align="affine")), dict(tiles=dict(batch=0)), dict(tiles=dict(size=200, overlap=64))):  # (200: o > min(200, 96) / 2)
            with pytest.raises(ValueError):
                device(batch, "matting", **bad)
        for bad in (dict(tiles=True), dict(tiles=dict(overlap=16))):
            with pytest.raises(ValueError):
                pipe.predict_batch_device(batch, "matting", processing_res=0, **bad)
        with pytest.raises(ValueError):
            device(batch.float(), "matting", tiles=opts)
        with pytest.raises(ValueError):
            pipe.cutout_batch_device(batch, "matting", processing_res=48, tiles=opts, match_input_res=False)
        with pytest.raises(ValueError):
            pipe(batch[:1].float(), processing_res=48, color_map=None, mode="matting", tiles=opts)
        # processing_res = 0 with an explicit size: the windows go through the model as they are
        got = pipe.predict_batch_device(batch[:1], "matting", processing_res=0, tiles=opts).cpu().numpy()
        plain_np = pipe.predict_batch_device(batch[:1], "matting", processing_res=0).cpu().numpy()
        tp0 = np.concatenate([pipe.predict_batch_device(crops[j:j + 4], "matting", processing_res=0).cpu().numpy() for j in range(0, 12, 4)])
        assert same_bits(got[0], tiled.tile_merge(plain_np[0], tp0, ys, xs, 16, "none"))
    finally:
        if pipe._engine is not None:
            pipe._engine.close()
