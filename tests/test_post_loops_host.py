"""Host tests (no GPU) of the dataset loops of the post-processing ops -- `infer_eval.run_refocus`, `run_stereo`, `run_cutouts`,
`run_pointclouds` and `run_parallax` -- with a fake pipeline whose `*_batch_device` entries return CPU tensors made from the input images, so
that a result paired with the wrong sample shows: the files lie under `output_dir/<scene>/` with the names of `get_pred_name`, come back in
sample order and hold the bytes the fake returned for that sample; a group never exceeds batch_size and never mixes sizes; two ranks of a
world of two write exactly the files of one.  `run_parallax` reaches `engine.parallax_frames` itself, which is replaced here."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

SIZES = [(6, 8), (6, 8), (8, 6), (6, 8), (6, 8)]   # (H, W): the third image has another size
BACKGROUND = (10, 200, 90)


def write_dataset(base):
    """Five PNGs in two scene directories; (samples, their uint8 [3, H, W] arrays)."""
    rng = np.random.RandomState(11)
    samples, arrays = [], []
    for i, (h, w) in enumerate(SIZES):
        rel = f"scene{i // 3:04d}_00/color/{i:06d}.png"
        os.makedirs(os.path.dirname(os.path.join(base, rel)), exist_ok=True)
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(base, rel))
        samples.append([rel])
        arrays.append(np.ascontiguousarray(np.moveaxis(a, -1, 0)))
    return samples, arrays


# ---- what the fake returns for one image [3, H, W], in numpy --------------------------------------------------------------------------------
def refocused(a):
    return 255 - a


def canvas(a):
    return np.concatenate([a, 255 - a], 2)


def rgba(a):
    return np.concatenate([np.moveaxis(a, 0, -1), (a[0] ^ a[1])[..., None]], -1)


def composite(a, bg):
    return (a // 2 + np.asarray(bg, np.uint8).reshape(3, 1, 1) // 2).astype(np.uint8)


def cloud(a):
    """n = 1 + (the sum of the bytes mod 5) points: (points float32 [n, 3], normals float32 [n, 3], rgb uint8 [n, 3])."""
    n = 1 + int(a.sum()) % 5
    flat = a.reshape(3, -1).T[:n]
    return flat.astype(np.float32) / 7.0, -flat.astype(np.float32), flat.copy()


def clip(a, first, end):
    """Frames first .. end of a path: frame k adds k to every byte."""
    return np.stack([(a.astype(np.int64) + k).astype(np.uint8) for k in range(first, end)])


class FakePipe:
    """The post-processing entries of GenPerceptPipeline on CPU tensors; `groups` records the (H, W) of the images of every call."""

    def __init__(self):
        self.groups = []

    def _stack(self, images, mode, modes):
        assert mode in modes
        arrays = [np.ascontiguousarray(np.moveaxis(np.asarray(im.convert("RGB")), -1, 0)) for im in images]
        self.groups.append([a.shape[1:] for a in arrays])
        return arrays

    def refocus_batch_device(self, images, mode, focus, focus_at, aperture, max_radius, dof, sharp, tables, **opts):
        assert (focus, focus_at, sharp, tables, opts) == (0.5, None, None, None, dict(refine=True))
        return torch.from_numpy(np.stack([refocused(a) for a in self._stack(images, mode, ("depth", "disparity"))]))

    def stereo_batch_device(self, images, mode, layout, views, separation, converge, converge_at, edge, **opts):
        assert (layout, views, separation, converge, converge_at, edge, opts) == ("sbs", 2, 4.0, None, (1, 2), 0.04, dict(refine=True))
        return torch.from_numpy(np.stack([canvas(a) for a in self._stack(images, mode, ("depth", "disparity"))]))

    def cutout_batch_device(self, images, mode, background, foreground_options, **opts):
        assert foreground_options is None and opts == dict(refine=True)
        arrays = self._stack(images, mode, ("matting", "dis"))
        out = [rgba(a) if background is None else composite(a, background) for a in arrays]
        return torch.from_numpy(np.stack(out)), torch.zeros((len(arrays), 1) + arrays[0].shape[1:])

    def pointcloud_batch_device(self, images, mode, cameras, pointcloud, **opts):
        assert cameras is None and pointcloud is True and opts == dict(refine=True)
        clouds = [cloud(a) for a in self._stack(images, mode, ("depth", "disparity"))]
        out = {k: torch.from_numpy(np.concatenate([c[j] for c in clouds])) for j, k in enumerate(("points", "point_normals", "point_rgb"))}
        out["offsets"] = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds])]).astype(np.int64)
        return out

    def _post_inputs(self, images, mode, modes, what, needs, inference_options, preflight=None):
        assert inference_options == dict(refine=True)
        rgb = torch.from_numpy(np.stack(self._stack(images, mode, modes)))
        preflight(rgb)
        return rgb, torch.full((rgb.shape[0], 1) + tuple(rgb.shape[-2:]), 0.5)


def read_ply(path):
    from genpercept_amd.geometry import PLY_DTYPE
    raw = open(path, "rb").read()
    rec = np.frombuffer(raw[raw.index(b"end_header\n") + 11:], PLY_DTYPE)
    return (np.stack([rec[k] for k in "xyz"], 1), np.stack([rec["n" + k] for k in "xyz"], 1), np.stack([rec[k] for k in ("red", "green", "blue")], 1))


def read_png(path):
    return np.asarray(Image.open(path))


# op: (the loop, its mode, its arguments, the suffix, what a file holds, what the fake returned for the image)
LOOPS = dict(
    refocus=("run_refocus", "depth", dict(focus=0.5), ".png", read_png, lambda a: np.moveaxis(refocused(a), 0, -1)),
    stereo=("run_stereo", "disparity", dict(separation=4.0, converge_at=(1, 2)), ".png", read_png, lambda a: np.moveaxis(canvas(a), 0, -1)),
    cutouts=("run_cutouts", "matting", dict(), ".png", read_png, rgba),
    cutouts_background=("run_cutouts", "dis", dict(background=BACKGROUND), ".png", read_png, lambda a: np.moveaxis(composite(a, BACKGROUND), 0, -1)),
    pointclouds=("run_pointclouds", "depth", dict(), ".ply", read_ply, cloud))


def same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("op", list(LOOPS))
def test_a_loop_writes_every_samples_own_result_in_order_in_groups_of_one_size(op, tmp_path):
    from genpercept_amd import infer_eval as ie
    loop, mode, kwargs, suffix, read, expected = LOOPS[op]
    base = str(tmp_path / "data")
    samples, arrays = write_dataset(base)
    names = [os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=suffix)) for s in samples]
    assert names[0] == os.path.join("scene0000_00", "color", "pred_000000" + suffix)

    def run(out, **more):
        pipe = FakePipe()
        written = getattr(ie, loop)(pipe, base, samples, str(tmp_path / out), ie.FileNameMode.id, **dict(dict(mode=mode, refine=True, **kwargs), **more))
        assert all(len(g) <= more.get("batch_size", 1) and len(set(g)) == 1 for g in pipe.groups)
        return [os.path.relpath(p, str(tmp_path / out)) for p in written], [len(g) for g in pipe.groups]

    for out, batch_size, prefetch, groups in (("b1", 1, 2, [1] * 5), ("b2", 2, 0, [2, 1, 2]), ("b3", 3, 2, [2, 1, 2])):
        assert run(out, batch_size=batch_size, prefetch=prefetch) == (names, groups)
        for name, a in zip(names, arrays):
            assert same(read(os.path.join(str(tmp_path / out), name)), expected(a)), (out, name)
    parts = [run("w2", batch_size=2, rank=rank, world=2) for rank in (0, 1)]
    assert parts[0] == (names[:3], [2, 1]) and parts[1] == (names[3:], [2])
    listed = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path / "w2")) for d, _, files in os.walk(str(tmp_path / "w2")) for f in files)
    assert listed == sorted(names)
    for name in names:
        assert open(os.path.join(str(tmp_path / "w2"), name), "rb").read() == open(os.path.join(str(tmp_path / "b2"), name), "rb").read()
    with pytest.raises(ValueError):
        run("bad", rank=2, world=2)
    with pytest.raises(ValueError):
        run("bad", mode="normal")
    assert not os.path.exists(str(tmp_path / "bad"))


def test_run_parallax_renders_a_long_path_in_parts_and_numbers_the_stills(tmp_path, monkeypatch):
    from genpercept_amd import engine
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples, arrays = write_dataset(base)
    ranges = []

    def parallax_frames(image, pred, path, frames, amount, push, zoom, pan, focus, focus_at, edge, overscan, frame_range, space):
        assert (path, frames, amount, push, zoom, pan, focus, focus_at, edge, overscan, space) == ("orbit", 70, 1.0, 0.0, 1.0, False, 0.25, None, 0.04, True, "depth")
        assert pred.shape == (image.shape[0], 1) + tuple(image.shape[-2:])
        ranges.append(frame_range)
        return torch.from_numpy(np.stack([clip(a, *frame_range) for a in image.numpy()]))

    monkeypatch.setattr(engine, "parallax_frames", parallax_frames)
    stems = [os.path.join(os.path.dirname(s[0]), "pred_" + os.path.basename(s[0])[:-4]) for s in samples]

    def run(out, **more):
        pipe = FakePipe()
        del ranges[:]
        written = ie.run_parallax(pipe, base, samples, str(tmp_path / out), ie.FileNameMode.id, **dict(dict(frames=70, amount=1.0, focus=0.25, refine=True), **more))
        assert all(len(g) <= more.get("batch_size", 1) and len(set(g)) == 1 for g in pipe.groups)
        assert ranges == [(0, 64), (64, 70)] * len(pipe.groups)
        return [[os.path.relpath(p, str(tmp_path / out)) for p in paths] for paths in written], [len(g) for g in pipe.groups]

    stills = [[f"{stem}_{k:04d}.png" for k in range(70)] for stem in stems]
    assert run("b2", batch_size=2, animate="gif") == ([s + [stem + ".gif"] for s, stem in zip(stills, stems)], [2, 1, 2])
    for paths, stem, a in zip(stills, stems, arrays):
        frames = clip(a, 0, 70)
        for k in (0, 1, 63, 64, 69):
            assert same(read_png(os.path.join(str(tmp_path / "b2"), paths[k])), np.moveaxis(frames[k], 0, -1)), paths[k]
        assert Image.open(os.path.join(str(tmp_path / "b2"), stem + ".gif")).n_frames == 70
    parts = [run("w2", batch_size=3, rank=rank, world=2) for rank in (0, 1)]
    assert parts[0] == (stills[:3], [2, 1]) and parts[1] == (stills[3:], [2])
    listed = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path / "w2")) for d, _, files in os.walk(str(tmp_path / "w2")) for f in files)
    assert listed == sorted(p for s in stills for p in s)
    for bad in (dict(mode="normal"), dict(animate="mp4"), dict(amount=[1.0, 2.0]), dict(rank=2, world=2)):
        with pytest.raises(ValueError):
            run("bad", **bad)
    assert not os.path.exists(str(tmp_path / "bad"))
