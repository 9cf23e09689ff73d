"""Dataset inference loop and evaluation driver next to the hot path.

Mirrors, for RGB + depth datasets listed in the reference's `data_split/*/filename_list_*.txt` format:
  * infer.py:408-447        -- per image: PIL RGB -> pipe(..., batch_size=0, color_map=None, ...) -> `.npy` under the scene directory,
                               named by get_pred_name (src/dataset/base_dataset.py:531-545, PerceptionFileNameMode :43-49);
  * eval.py:143-244         -- per image: load prediction, least-squares alignment (depth or disparity space), clip to the dataset's
                               depth range, ten metrics (eval_metrics.py), mean over images, `eval_metrics-<alignment>.txt` + per-sample csv;
  * src/dataset/nyu_dataset.py:39-58, base_dataset.py:399-413 -- NYUv2 decoding (png / 1000), validity (min < d < max) and Eigen crop.
Pinned to the reference by tests/golden/infer_eval_ref.npz (naming modes; disparity-space alignment and max_resolution fits come from
the reference's alignment.py).  The loops for surface normals and for dis / matting masks follow the same pattern; the reference has no
evaluation script for either, their metrics are defined in eval_metrics.py.  Nothing here touches the GPU except through the pipeline
object handed in.
"""
from __future__ import annotations

import os
from enum import Enum
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
from PIL import Image

from . import eval_metrics as em


class FileNameMode(Enum):
    """Prediction file naming modes (PerceptionFileNameMode, base_dataset.py:43-49)."""
    id = 1        # id.png
    rgb_id = 2    # rgb_id.png
    i_d_rgb = 3   # i_d_1_rgb.png
    rgb_i_d = 4


def get_pred_name(rgb_basename: str, name_mode: FileNameMode, suffix: str = ".png") -> str:
    if name_mode == FileNameMode.rgb_id:
        pred = "pred_" + rgb_basename.split("_")[1]
    elif name_mode == FileNameMode.i_d_rgb:
        pred = rgb_basename.replace("_rgb.", "_pred.")
    elif name_mode == FileNameMode.id:
        pred = "pred_" + rgb_basename
    elif name_mode == FileNameMode.rgb_i_d:
        pred = "pred_" + "_".join(rgb_basename.split("_")[1:])
    else:
        raise NotImplementedError(name_mode)
    return os.path.splitext(pred)[0] + suffix


def read_filename_list(path: str) -> List[List[str]]:
    """One sample per line: `rgb_rel_path depth_rel_path [filled_rel_path]` (base_dataset.py:97-103)."""
    with open(path, "r") as f:
        return [ln.split() for ln in f.read().splitlines() if ln.strip()]


# Dataset conventions the evaluation needs (config/dataset/eval/*.yaml + src/dataset/{nyu,kitti,eth3d,scannet,diode}_dataset.py): depth
# range, naming mode, how the ground truth is stored, evaluation crop / mask.  Pinned to the reference classes by tests/golden/datasets_ref.npz.
#   gt: ("png", divisor) | ("eth3d_bin", (H, W)) | ("npy", None)
DATASETS: Dict[str, dict] = {
    "nyu": dict(min_depth=1e-3, max_depth=10.0, name_mode=FileNameMode.rgb_id, gt=("png", 1000.0), eval_crop=(45, 471, 41, 601)),
    "kitti": dict(min_depth=1e-5, max_depth=80.0, name_mode=FileNameMode.id, gt=("png", 256.0), kitti_bm_crop=True, valid_mask_crop="eigen"),
    "eth3d": dict(min_depth=1e-5, max_depth=float("inf"), name_mode=FileNameMode.id, gt=("eth3d_bin", (4032, 6048))),
    "scannet": dict(min_depth=1e-3, max_depth=10.0, name_mode=FileNameMode.id, gt=("png", 1000.0)),
    "diode": dict(min_depth=0.6, max_depth=350.0, name_mode=FileNameMode.id, gt=("npy", None), mask_from_file=True),
}
DATASETS["nyu_v2"] = DATASETS["nyu"]  # `name:` of config/dataset/eval/data_nyu_test.yaml


def read_depth_png(path: str, depth_scale: float) -> np.ndarray:
    return np.asarray(Image.open(path)).astype(np.float32) * np.float32(depth_scale)


def kitti_benchmark_crop(img: np.ndarray) -> np.ndarray:
    """kitti_dataset.py:83-110: bottom-aligned, horizontally centred 352 x 1216 window of a [.., H, W] array (RGB and depth alike)."""
    h, w = img.shape[-2:]
    top, left = int(h - 352), int((w - 1216) / 2)
    return img[..., top:top + 352, left:left + 1216]


def kitti_eval_mask(h: int, w: int, kind: Optional[str]) -> np.ndarray:
    """kitti_dataset.py:112-133: Garg (ECCV16) / Eigen (NIPS14) evaluation window as a boolean [h, w] mask (None: everything)."""
    m = np.zeros((h, w), dtype=bool)
    if kind is None:
        m[:] = True
    elif kind == "garg":
        m[int(0.40810811 * h):int(0.99189189 * h), int(0.03594771 * w):int(0.96405229 * w)] = True
    elif kind == "eigen":
        m[int(0.3324324 * h):int(0.91351351 * h), int(0.0359477 * w):int(0.96405229 * w)] = True
    else:
        raise ValueError(f"Unknown crop type: {kind}")
    return m


def read_gt_depth(path: str, dataset: str) -> np.ndarray:
    """Ground-truth depth [H, W] float32 in metres as the reference's dataset class decodes it (after the KITTI benchmark crop)."""
    cfg = DATASETS[dataset]
    kind, arg = cfg["gt"]
    if kind == "png":          # kitti / 256 (kitti_dataset.py:60-68), scannet and nyu / 1000 (scannet_dataset.py:31-38, nyu_dataset.py:39-46)
        d = np.asarray(Image.open(path)).astype(np.float32) / np.float32(arg)
    elif kind == "eth3d_bin":  # eth3d_dataset.py:38-57: raw float32, inf = no measurement -> 0
        d = np.fromfile(path, dtype=np.float32).copy()
        d[d == np.inf] = 0.0
        d = d.reshape(arg)
    elif kind == "npy":        # diode_dataset.py:37-50
        d = np.load(path).squeeze().astype(np.float32)
    else:
        raise ValueError(kind)
    if cfg.get("kitti_bm_crop"):
        d = kitti_benchmark_crop(d)
    return d


def dataset_valid_mask(depth: np.ndarray, dataset: str, mask_path: Optional[str] = None) -> np.ndarray:
    """base_dataset.py:410-413 range test, then the dataset's evaluation crop (NYU Eigen crop, KITTI Garg / Eigen window) or, for DIODE,
    the mask file that ships with the sample (diode_dataset.py:72-78)."""
    cfg = DATASETS[dataset]
    if cfg.get("mask_from_file"):
        if mask_path is None:
            raise ValueError("DIODE samples carry their validity mask as a third path")
        return np.load(mask_path).squeeze().astype(bool)
    m = valid_mask_of(depth, cfg["min_depth"], cfg["max_depth"], cfg.get("eval_crop"))
    if "valid_mask_crop" in cfg:
        m = m & kitti_eval_mask(depth.shape[-2], depth.shape[-1], cfg["valid_mask_crop"])
    return m


def valid_mask_of(depth: np.ndarray, min_depth: float, max_depth: float, eval_crop: Optional[Tuple[int, int, int, int]] = None) -> np.ndarray:
    m = (depth > min_depth) & (depth < max_depth)          # base_dataset.py:410-413
    if eval_crop is not None:                               # nyu_dataset.py:51-56
        c = np.zeros_like(m)
        y0, y1, x0, x1 = eval_crop
        c[y0:y1, x0:x1] = True
        m = m & c
    return m


def _shard(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world size {world}")
    from .distributed import shard_range
    return shard_range(n_items, rank, world)


def _decode_ahead(items: Sequence, load: Callable, prefetch: int):
    """(item, load(item)) in order, the next `prefetch` images decoded by a helper thread meanwhile (prefetch <= 0: inline)."""
    if prefetch <= 0 or len(items) < 2:
        for s in items:
            yield s, load(s)
        return
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1) as loader:
        pending, it = deque(), iter(items)
        for s in it:
            pending.append((s, loader.submit(load, s)))
            if len(pending) > prefetch:
                break
        while pending:
            s, fut = pending.popleft()
            img = fut.result()
            nxt = next(it, None)
            if nxt is not None:
                pending.append((nxt, loader.submit(load, nxt)))
            yield s, img


def _size_groups(loaded: Iterable, batch_size: int):
    """Consecutive (item, image) pairs whose images have one size, at most batch_size per group; order is kept."""
    group: list = []
    for s, img in loaded:
        if group and (len(group) >= batch_size or img.size != group[0][1].size):
            yield group
            group = []
        group.append((s, img))
    if group:
        yield group


def _load_rgb(base_dir: str, rgb_rel: str, rgb_crop: Optional[Callable[[np.ndarray], np.ndarray]]) -> Image.Image:
    img = Image.open(os.path.join(base_dir, rgb_rel)).convert("RGB")
    if rgb_crop is not None:  # KITTI: the benchmark crop is applied to the RGB as well (kitti_dataset.py:70-74)
        img = Image.fromarray(np.ascontiguousarray(np.moveaxis(rgb_crop(np.moveaxis(np.asarray(img), -1, 0)), 0, -1)))
    return img


def _pred_name(rgb_rel: str, name_mode: FileNameMode, suffix: str = ".npy") -> str:
    return os.path.join(os.path.dirname(rgb_rel), get_pred_name(os.path.basename(rgb_rel), name_mode, suffix=suffix))


def _save_path(output_dir: str, rgb_rel: str, name_mode: FileNameMode, suffix: str) -> str:
    """Where a sample's result goes, `output_dir/<scene>/<get_pred_name>`; the scene directory is made."""
    save_to = os.path.join(output_dir, _pred_name(rgb_rel, name_mode, suffix))
    os.makedirs(os.path.dirname(save_to), exist_ok=True)
    return save_to


def _chw_image(px: np.ndarray) -> Image.Image:
    """A uint8 [3, H, W] array as a PIL RGB image."""
    return Image.fromarray(np.ascontiguousarray(np.moveaxis(px, 0, -1)))


def _write_rgb(px: np.ndarray, save_to: str) -> str:
    _chw_image(px).save(save_to)
    return save_to


def _write_frames(clip: np.ndarray, save_to: str, animate: Optional[str], frame_ms: int) -> List[str]:
    """The frames uint8 [V, 3, H, W] of one sample as numbered files `<stem>_0000.png`, ... next to `save_to` and, with animate="gif", one
    looping `<stem>.gif` of them after those; the paths written."""
    stem = os.path.splitext(save_to)[0]
    stills = [_chw_image(px) for px in clip]
    paths = [f"{stem}_{k:04d}.png" for k in range(len(stills))]
    for still, path_k in zip(stills, paths):
        still.save(path_k)
    if animate == "gif":
        paths.append(stem + ".gif")
        stills[0].save(paths[-1], save_all=True, append_images=stills[1:], duration=int(frame_ms), loop=0)
    return paths


def _one_value_each(values: Dict, at_name: str, at) -> None:
    """The terms a dataset loop uses for every sample: each of `values` (name -> value) is one number or None, `at` one pixel (u, v) or None."""
    if any(np.ndim(v) != 0 for v in values.values()) or (at is not None and np.shape(at) != (2,)):
        names = list(values)
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} are one value each and {at_name} one pixel (u, v), used for every sample")


def _post_loop(base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, suffix: str, batch_size: int, rank: int,
               world: int, prefetch: int, run_group: Callable, write: Callable) -> list:
    """The loop of the post-processing runs (`run_cutouts` ... `run_parallax`): this rank's `shard_range` of the samples, decoded `prefetch`
    ahead, consecutive images of one size together, at most batch_size of them.  `run_group(images)` gives the results of a group on the
    host, one per image in order; `write(result, save_to)` saves one of them, save_to being `output_dir/<scene>/<get_pred_name>` with
    `suffix`, and returns what the run reports for the sample: that path or a list of paths.  Returns those, in sample order."""
    if world > 1:
        lo, hi = _shard(len(samples), rank, world)
        samples = samples[lo:hi]
    written = []
    for group in _size_groups(_decode_ahead(samples, lambda s: _load_rgb(base_dir, s[0], None), prefetch), max(1, batch_size)):
        results = run_group([img for _, img in group])
        assert len(results) == len(group)
        for (smp, _), result in zip(group, results):
            written.append(write(result, _save_path(output_dir, smp[0], name_mode, suffix)))
    return written


def run_inference(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
                  denoise_steps: int = 1, ensemble_size: int = 1, processing_res: int = 0, match_input_res: bool = True,
                  resample_method: str = "bilinear", fix_timesteps=None, prompt: str = "", rgb_crop: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                  prefetch: int = 2, batch_size: int = 1, rank: int = 0, world: int = 1, refine=None, tiles=None) -> List[str]:
    """infer.py:408-447.  Returns the paths written.  rgb_crop: e.g. kitti_benchmark_crop (applied to the [3, H, W] image).
    refine (None, True or dict(radius=..., eps=...)): passed to the pipeline, which then brings each map to the input size by the guided filter.
    tiles (None, True or dict(size=..., overlap=..., align=..., batch=...)): passed to the pipeline too, which then runs tiled inference.
    prefetch > 0: the next `prefetch` images are decoded (and cropped) by a helper thread while the engine works on the current one, and the .npy
    files are written by another -- the role the DataLoader workers play in the reference's loop; order and results are those of prefetch = 0.
    batch_size > 1: consecutive samples of one image size go through `pipe.infer_batch` together, up to batch_size per call (same file names,
    same order).  world > 1: this call handles `shard_range(len(samples), rank, world)` of the filtered list, one process per GPU."""
    written = []
    samples = [s for s in samples if len(s) < 2 or s[1] != "None"]  # kitti_dataset.py:47: entries without ground truth are skipped
    if world > 1:
        lo, hi = _shard(len(samples), rank, world)
        samples = samples[lo:hi]

    def load(rgb_rel):
        return _load_rgb(base_dir, rgb_rel, rgb_crop)

    def save(rgb_rel, pred_np):
        save_to = _save_path(output_dir, rgb_rel, name_mode, ".npy")
        np.save(save_to, pred_np)
        return save_to

    extra = {k: v for k, v in (("refine", refine), ("tiles", tiles)) if v is not None}

    def infer(img):
        return pipe(img, denoising_steps=denoise_steps, ensemble_size=ensemble_size, processing_res=processing_res, match_input_res=match_input_res,
                    batch_size=0, color_map=None, show_progress_bar=False, resample_method=resample_method, mode=mode,
                    fix_timesteps=fix_timesteps, prompt=prompt, **extra)

    if batch_size > 1:
        for group in _size_groups(_decode_ahead(samples, lambda s: load(s[0]), prefetch), batch_size):
            outs = pipe.infer_batch([img for _, img in group], mode, processing_res=processing_res, match_input_res=match_input_res,
                                    resample_method=resample_method, color_map=None, fix_timesteps=fix_timesteps, prompt=prompt,
                                    denoising_steps=denoise_steps, ensemble_size=ensemble_size, **extra)
            assert len(outs) == len(group)
            for (smp, _), out in zip(group, outs):
                written.append(save(smp[0], out.pred_np))
        return written
    loaded = _decode_ahead(samples, lambda s: load(s[0]), prefetch)  # (a decode error surfaces at the image it belongs to)
    if prefetch <= 0 or len(samples) < 2:
        return [save(s[0], infer(img).pred_np) for s, img in loaded]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1) as writer:
        saves = [writer.submit(save, s[0], infer(img).pred_np) for s, img in loaded]
        return [f.result() for f in saves]


def run_cutouts(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "matting",
                batch_size: int = 1, rank: int = 0, world: int = 1, background=None, prefetch: int = 2, foreground_options: Optional[dict] = None,
                **inference_options) -> List[str]:
    """One cutout per sample with `pipe.cutout_batch_device` (modes matting and dis): an RGBA `.png` whose colours are the estimated foreground
    colours and whose A is the predicted alpha byte, or, with a `background` (one colour of three bytes, or a uint8 [3, H, W] image for samples of
    that size), the RGB composite over it.  Batching and sharding as `run_inference`: consecutive samples of one image size go through one call,
    up to batch_size of them; world > 1: this call handles `shard_range(len(samples), rank, world)` of the list.  Returns the paths written.
    inference_options go to `pipe.predict_batch_device`; `refine=True` (or dict(radius=..., eps=...)) among them sharpens the alpha with the
    guided filter before the colours are estimated, and `tiles=True` (or dict(size=..., overlap=..., align=..., batch=...)) makes it the alpha
    of tiled inference."""
    import torch
    if mode not in ("matting", "dis"):
        raise ValueError(f"cutouts need an alpha map: mode 'matting' or 'dis', got {mode!r}")

    def cutouts(images):
        bg = background
        if torch.is_tensor(bg) and bg.dim() == 3:
            bg = bg[None].expand(len(images), -1, -1, -1)
        return pipe.cutout_batch_device(images, mode, bg, foreground_options, **inference_options)[0].cpu().numpy()

    def write(px, save_to):
        (Image.fromarray(px) if background is None else _chw_image(px)).save(save_to)
        return save_to

    return _post_loop(base_dir, samples, output_dir, name_mode, ".png", batch_size, rank, world, prefetch, cutouts, write)


def run_pointclouds(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
                    batch_size: int = 1, rank: int = 0, world: int = 1, cameras=None, pointcloud=True, prefetch: int = 2, **inference_options) -> List[str]:
    """One point cloud per sample with `pipe.pointcloud_batch_device` (modes depth and disparity): a binary little-endian `.ply` with x y z
    nx ny nz (float) and red green blue (uchar) per vertex, the kept pixels of the sample in row-major order (`geometry.write_ply`).
    cameras: None (`geometry.default_camera`, a viewing convention) or eight values s, t, fx, fy, cx, cy, z_min, z_max used for every sample;
    pointcloud: True or dict(radius=..., tau=..., min_count=..., min_cos=..., stride=...).  Batching, sharding and prefetch as `run_cutouts`.
    Returns the paths written.  inference_options go to `pipe.predict_batch_device`, `refine` and `tiles` among them."""
    from .geometry import write_ply
    if mode not in ("depth", "disparity"):
        raise ValueError(f"point clouds need a depth map: mode 'depth' or 'disparity', got {mode!r}")
    if cameras is not None and np.asarray(cameras).shape != (8,):
        raise ValueError(f"cameras: None or eight values used for every sample, got shape {np.asarray(cameras).shape}")

    def clouds(images):
        out = pipe.pointcloud_batch_device(images, mode, cameras, pointcloud, **inference_options)
        off = out["offsets"]
        arrays = [out[k].cpu().numpy() for k in ("points", "point_normals", "point_rgb")]
        return [[a[off[i]:off[i + 1]] for a in arrays] for i in range(len(off) - 1)]

    def write(cloud, save_to):
        write_ply(save_to, *cloud)
        return save_to

    return _post_loop(base_dir, samples, output_dir, name_mode, ".ply", batch_size, rank, world, prefetch, clouds, write)


MESH_FORMATS = ("glb", "ply")


def run_meshes(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
               batch_size: int = 1, rank: int = 0, world: int = 1, cameras=None, mesh=True, format: str = "glb", prefetch: int = 2,
               **inference_options) -> List[str]:
    """One triangle mesh per sample with `pipe.mesh_batch_device` (modes depth and disparity), cut at the depth edges: a binary glTF `.glb`
    textured with the sample's own image (`mesh.write_glb`), or with format "ply" a binary little-endian `.ply` with the vertex record of
    `run_pointclouds` and a face list (`mesh.write_mesh_ply`).  cameras: None (`geometry.default_camera`, a viewing convention) or eight values
    used for every sample; mesh: True or dict(radius=..., tau=..., min_count=..., min_cos=..., stride=..., cut=...).  Batching, sharding and
    prefetch as `run_cutouts`.  Returns the paths written.  inference_options go to `pipe.predict_batch_device`, `refine` and `tiles` among them."""
    from .mesh import mesh_options, write_glb, write_mesh_ply
    if mode not in ("depth", "disparity"):
        raise ValueError(f"meshes need a depth map: mode 'depth' or 'disparity', got {mode!r}")
    if format not in MESH_FORMATS:
        raise ValueError(f"format is one of {MESH_FORMATS}, got {format!r}")
    if cameras is not None and np.asarray(cameras).shape != (8,):
        raise ValueError(f"cameras: None or eight values used for every sample, got shape {np.asarray(cameras).shape}")
    mesh_options(mesh)

    def meshes(images):
        out = pipe.mesh_batch_device(images, mode, cameras, mesh, **inference_options)
        v, f = out["vertex_offsets"], out["face_offsets"]
        a = {k: out[k].cpu().numpy() for k in ("vertices", "vertex_normals", "vertex_rgb", "vertex_uv", "faces")}
        return [dict({k: a[k][v[i]:v[i + 1]] for k in a if k != "faces"}, faces=a["faces"][f[i]:f[i + 1]], image=np.moveaxis(np.asarray(img), -1, 0))
                for i, img in enumerate(images)]

    def write(m, save_to):
        if format == "glb":
            write_glb(save_to, m["vertices"], m["vertex_normals"], m["vertex_uv"], m["faces"], image=m["image"])
        else:
            write_mesh_ply(save_to, m["vertices"], m["vertex_normals"], m["vertex_rgb"], m["faces"])
        return save_to

    return _post_loop(base_dir, samples, output_dir, name_mode, "." + format, batch_size, rank, world, prefetch, meshes, write)


def run_refocus(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
                batch_size: int = 1, rank: int = 0, world: int = 1, focus=None, focus_at=None, aperture=8.0, max_radius=16.0, dof=0.0, tables=None,
                prefetch: int = 2, **inference_options) -> List[str]:
    """One refocused photograph per sample with `pipe.refocus_batch_device` (modes depth and disparity): an RGB `.png`, synthetic depth of
    field under the sample's own prediction.  focus (a value of the map in [0, 1]) or focus_at (a pixel (u, v)), aperture, max_radius and dof
    are one value each, used for every sample.  Batching, sharding and prefetch as `run_cutouts`.  Returns the paths written.
    inference_options go to `pipe.predict_batch_device`, `refine` and `tiles` among them."""
    from .lens_blur import lens_blur_options
    if mode not in ("depth", "disparity"):
        raise ValueError(f"a refocus needs a depth map: mode 'depth' or 'disparity', got {mode!r}")
    _one_value_each(dict(focus=focus, aperture=aperture, max_radius=max_radius, dof=dof), "focus_at", focus_at)
    lens_blur_options(1, focus, focus_at, aperture, max_radius, dof)

    def refocused(images):
        return pipe.refocus_batch_device(images, mode, focus, focus_at, aperture, max_radius, dof, None, tables, **inference_options).cpu().numpy()

    return _post_loop(base_dir, samples, output_dir, name_mode, ".png", batch_size, rank, world, prefetch, refocused, _write_rgb)


def run_stereo(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
               batch_size: int = 1, rank: int = 0, world: int = 1, layout="sbs", views=2, separation=16.0, converge=None, converge_at=None, edge=0.04,
               prefetch: int = 2, **inference_options) -> List[str]:
    """One stereo frame per sample with `pipe.stereo_batch_device` (modes depth and disparity): the canvas of the layout -- a side-by-side
    pair, an anaglyph, a quilt -- as an RGB `.png`, rendered under the sample's own prediction.  separation, converge (a value of the map in
    [0, 1]) or converge_at (a pixel (u, v)) and edge are one value each, used for every sample.  Batching, sharding and prefetch as
    `run_cutouts`.  Returns the paths written.  inference_options go to `pipe.predict_batch_device`, `refine` and `tiles` among them."""
    from .stereo import stereo_options, view_table
    if mode not in ("depth", "disparity"):
        raise ValueError(f"a stereo view needs a depth map: mode 'depth' or 'disparity', got {mode!r}")
    _one_value_each(dict(separation=separation, converge=converge, edge=edge), "converge_at", converge_at)
    stereo_options(1, converge, converge_at, edge)
    view_table(layout, views, separation, 1, 1)

    def canvases(images):
        return pipe.stereo_batch_device(images, mode, layout, views, separation, converge, converge_at, edge, **inference_options).cpu().numpy()

    return _post_loop(base_dir, samples, output_dir, name_mode, ".png", batch_size, rank, world, prefetch, canvases, _write_rgb)


def run_parallax(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "depth",
                 batch_size: int = 1, rank: int = 0, world: int = 1, path="orbit", frames: int = 16, amount: float = 16.0, push: float = 0.0,
                 zoom: float = 1.0, pan: bool = False, focus=None, focus_at=None, edge=0.04, overscan: bool = True, animate: Optional[str] = None,
                 frame_ms: int = 40, prefetch: int = 2, **inference_options) -> List[List[str]]:
    """A camera move per sample with `engine.parallax_frames` under the sample's own prediction (modes depth and disparity): the frames as
    numbered RGB files `<name>_0000.png`, `<name>_0001.png`, ... and, with animate="gif", one looping `<name>.gif` of them (PIL, `frame_ms`
    per frame) after them.  The model runs once per batch; a path longer than the 64 frames of one call is rendered in parts under that
    one map (`frame_range`).  amount, push, zoom, focus (a value of the map in [0, 1]) or focus_at (a pixel (u, v)) and edge are one value
    each, used for every sample.  Batching, sharding and prefetch as `run_stereo`.  Returns the paths written, one list per sample.
    inference_options go to `pipe.predict_batch_device`, `refine` and `tiles` among them."""
    from . import engine as ge
    from .parallax import MAX_FRAMES, camera_path, plan
    from .post_common import _edge16, _plane
    if mode not in ("depth", "disparity"):
        raise ValueError(f"a camera move needs a depth map: mode 'depth' or 'disparity', got {mode!r}")
    if animate not in (None, "gif"):
        raise ValueError(f"animate is None or 'gif', got {animate!r}")
    _one_value_each(dict(amount=amount, push=push, zoom=zoom, focus=focus, edge=edge), "focus_at", focus_at)
    terms = (path, frames, amount, push, zoom, pan, focus, focus_at, edge, overscan)
    _plane(1, focus, focus_at, "focus", "focus_at", exactly_one=False)
    _edge16(edge)
    n_path = len(camera_path(path, frames, amount, push, zoom, pan))      # (the terms that need no image size are checked before any is read)

    def clips(images):
        rgb, pred = pipe._post_inputs(images, mode, ("depth", "disparity"), "a camera move", "a depth map", inference_options,
                                      lambda images: plan(int(images.shape[0]), int(images.shape[-2]), int(images.shape[-1]), *terms,
                                                          (0, min(n_path, MAX_FRAMES))))
        parts = [ge.parallax_frames(rgb, pred, *terms, (first, min(first + MAX_FRAMES, n_path)), space=mode).cpu().numpy()
                 for first in range(0, n_path, MAX_FRAMES)]
        out = np.concatenate(parts, 1)
        assert out.shape[1] == n_path
        return out

    return _post_loop(base_dir, samples, output_dir, name_mode, ".png", batch_size, rank, world, prefetch, clips,
                      lambda clip, save_to: _write_frames(clip, save_to, animate, frame_ms))


def run_relight(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: str, name_mode: FileNameMode, mode: str = "normal",
                batch_size: int = 1, rank: int = 0, world: int = 1, lights=True, ambient=0.35, relief=64.0, flip=(False, False, False), tables=None,
                sweep: Optional[int] = None, animate: Optional[str] = None, frame_ms: int = 40, prefetch: int = 2, **inference_options):
    """One relit photograph per sample with `pipe.relight_batch_device` (mode normal: shading only; modes depth and disparity: the normals
    fitted to the sample's own prediction and its cast shadows): an RGB `.png`.  lights, ambient, relief, flip and tables as that entry takes
    them, used for every sample.  With sweep=n every sample gives n frames in which every light's azimuth goes once round (frame i adds
    360 i / n degrees), numbered `<name>_0000.png`, ... and, with animate="gif", one looping `<name>.gif` after them (`frame_ms` per frame):
    the model runs once per batch and `engine.relight` n times under that one prediction.  Batching, sharding and prefetch as `run_refocus`.
    Returns the paths written -- with sweep a list of paths per sample.  inference_options go to `pipe.predict_batch_device`, `refine` and
    `tiles` among them."""
    from . import engine as ge
    from .relight import check_flip, relight_lights, relight_options
    if mode not in ("normal", "depth", "disparity"):
        raise ValueError(f"a relight needs a normal map or a depth map: mode 'normal', 'depth' or 'disparity', got {mode!r}")
    if animate not in (None, "gif") or (animate is not None and sweep is None):
        raise ValueError(f"animate is None or, with a sweep, 'gif', got {animate!r}")
    if sweep is not None and (isinstance(sweep, bool) or not isinstance(sweep, (int, np.integer)) or not 1 <= sweep <= 3600):
        raise ValueError(f"sweep is None or a number of frames in 1 .. 3600, got {sweep!r}")
    check_flip(flip)
    opts = relight_options(lights)
    turned = [[dict(o, azimuth=o["azimuth"] + 360.0 * i / sweep) for o in opts] for i in range(sweep)] if sweep is not None else [opts]
    for frame in turned:
        relight_lights(frame, ambient, relief)      # (every frame's terms are checked before any image is read)

    def clips(images):
        maps = pipe._relight_maps(images, mode, None, "depth", inference_options)
        frames = [ge.relight(lights=frame, ambient=ambient, relief=relief, flip=flip, tables=tables, **maps).cpu().numpy() for frame in turned]
        return np.stack(frames, 1)

    def write(clip, save_to):
        return _write_rgb(clip[0], save_to) if sweep is None else _write_frames(clip, save_to, animate, frame_ms)

    return _post_loop(base_dir, samples, output_dir, name_mode, ".png", batch_size, rank, world, prefetch, clips, write)


def _write_metric_files(output_dir: str, tag: str, names: List[str], per_sample, result: Dict[str, float], header: str) -> None:
    """`per_sample_metrics<tag>.csv` (one row per prediction file) and `eval_metrics<tag>.txt` (header, metric names, means)."""
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, f"per_sample_metrics{tag}.csv"), "w") as f:
        f.write("filename," + ",".join(names) + "\n")
        for nm, vals in per_sample:
            f.write(nm + "," + ",".join(str(v) for v in vals) + "\n")
    with open(os.path.join(output_dir, f"eval_metrics{tag}.txt"), "w") as f:
        f.write(header)
        f.write("  ".join(names) + "\n" + "  ".join(f"{result[k]:.6g}" for k in names) + "\n")


def _write_eval_files(output_dir: str, alignment: Optional[str], names: List[str], per_sample, result: Dict[str, float], prediction_dir: str,
                      dataset: str) -> None:
    """eval.py:217-244: `per_sample_metrics-<alignment>.csv` and `eval_metrics-<alignment>.txt`."""
    cfg = DATASETS[dataset]
    header = f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on dataset: {dataset}\n"
    header += f"min_depth = {cfg['min_depth']}\nmax_depth = {cfg['max_depth']}\n"
    _write_metric_files(output_dir, f"-{alignment}" if alignment else "", names, per_sample, result, header)


def _write_normal_eval_files(output_dir: str, names: List[str], per_sample, result: Dict[str, float], prediction_dir: Optional[str],
                             gt_column: int) -> None:
    """`per_sample_metrics-normal.csv` and `eval_metrics-normal.txt`, laid out like the depth files."""
    header = f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on normals: column {gt_column} of the filename list\n"
    _write_metric_files(output_dir, "-normal", names, per_sample, result, header)


def _gt_rel(s: Sequence[str], gt_column: int) -> Optional[str]:
    """The ground-truth path of a filename-list line, None where the column is absent or "None"."""
    return s[gt_column] if len(s) > gt_column and s[gt_column] != "None" else None


def _same_size(smp: Sequence[str], pred_shape, gt_shape) -> None:
    if tuple(pred_shape) != tuple(gt_shape):
        raise ValueError(f"{smp[0]}: prediction {tuple(pred_shape)} and ground truth {tuple(gt_shape)} differ in size")


def _region(region_of: Optional[Callable], smp: Sequence[str], gt: np.ndarray) -> Optional[np.ndarray]:
    """`region_of(sample, gt)` as a bool array of the ground truth's height and width (None without region_of)."""
    if region_of is None:
        return None
    r = np.asarray(region_of(smp, gt)) != 0
    if r.shape != gt.shape[:2]:
        raise ValueError(f"{smp[0]}: region {r.shape} and ground truth {gt.shape[:2]} differ in size")
    return r


def _evaluate_files(prediction_dir: str, samples: Sequence[Sequence[str]], gt_column: int, pred_name_of: Callable, score: Callable, names: List[str]):
    """The skeleton of the file routes: samples without ground truth (column gt_column absent or "None") or without a prediction file are
    skipped; `score(sample, ground-truth path, prediction path)` reads both, checks their sizes and returns the image's metric dict.
    Returns (rows [(prediction name, values in `names` order)], the means of the per-image values: eval.py's reduction)."""
    sums = {k: 0.0 for k in names}
    per_sample = []
    for s in samples:
        rel = _gt_rel(s, gt_column)
        if rel is None:
            continue
        pred_name = pred_name_of(s)
        pred_path = os.path.join(prediction_dir, pred_name)
        if not os.path.exists(pred_path):
            continue
        m = score(s, rel, pred_path)
        for k in names:
            sums[k] += m[k]
        per_sample.append((pred_name, [m[k] for k in names]))
    n = len(per_sample)
    return per_sample, {k: (sums[k] / n if n else float("nan")) for k in names}


def evaluate_predictions(prediction_dir: str, base_dir: str, samples: Sequence[Sequence[str]], dataset: str = "nyu",
                         alignment: str = "least_square", alignment_max_res: Optional[int] = None, output_dir: Optional[str] = None,
                         pred_suffix: str = ".npy", read_gt: Optional[Callable[[str], np.ndarray]] = None) -> Dict[str, float]:
    """eval.py:143-244: mean of the per-image metrics; optionally writes `eval_metrics-<alignment>.txt` and `per_sample_metrics-...csv`."""
    cfg = DATASETS[dataset]
    names = list(em.METRICS.keys())

    def score(s, depth_rel, pred_path):
        gt = read_gt(os.path.join(base_dir, depth_rel)) if read_gt else read_gt_depth(os.path.join(base_dir, depth_rel), dataset)
        vm = dataset_valid_mask(gt, dataset, os.path.join(base_dir, s[2]) if cfg.get("mask_from_file") and len(s) > 2 else None)
        return em.evaluate_depth(np.load(pred_path), gt, vm, cfg["min_depth"], cfg["max_depth"], alignment=alignment, alignment_max_res=alignment_max_res)

    per_sample, result = _evaluate_files(prediction_dir, samples, 1, lambda s: _pred_name(s[0], cfg["name_mode"], pred_suffix), score, names)
    if output_dir is not None:
        _write_eval_files(output_dir, alignment, names, per_sample, result, prediction_dir, dataset)
    return result


# ---- surface normals: ground truth and the `.npy` route ---------------------------------------------------------------------------------
NORMAL_METRICS = ["mean_rad", "mean_deg", "median_deg", "rmse_deg", "within_11.25", "within_22.5", "within_30"]  # normal_angular_error's keys, in order


def read_gt_normal(path: str) -> np.ndarray:
    """Ground-truth normals as float32 [3, H, W]: a `.npy` of signed, linear, not necessarily unit vectors stored [H, W, 3] or [3, H, W] -- the
    raster the reference's _load_normal_data yields for column 3 of a filename-list line (src/dataset/base_dataset.py:362-363).  Other
    formats: pass a `read_gt` callable to the evaluation functions."""
    if os.path.splitext(path)[1].lower() != ".npy":
        raise ValueError(f"{path}: normal ground truth is read from .npy files only (pass read_gt= for other formats)")
    n = np.load(path)
    if n.ndim != 3 or 3 not in (n.shape[0], n.shape[-1]):
        raise ValueError(f"{path}: expected [H, W, 3] or [3, H, W], got {n.shape}")
    if n.shape[-1] == 3:  # [H, W, 3] (a [3, H, 3] array is read as three rows of it: the raster's own layout wins)
        n = np.moveaxis(n, -1, 0)
    return np.ascontiguousarray(n, dtype=np.float32)


def normal_valid_mask(gt: np.ndarray) -> np.ndarray:
    """base_dataset.py:416-418: a pixel is valid where any of the three ground-truth channels is non-zero.  gt [3, H, W] -> bool [H, W]."""
    return (np.asarray(gt) != 0).any(axis=0)


def evaluate_normal_predictions(prediction_dir: str, base_dir: str, samples: Sequence[Sequence[str]], name_mode: FileNameMode, gt_column: int = 3,
                                output_dir: Optional[str] = None, read_gt: Optional[Callable[[str], np.ndarray]] = None) -> Dict[str, float]:
    """The `.npy` route for what `run_inference(mode="normal")` writes ([H, W, 3] in [0, 1]): per image decode_normals ->
    normal_angular_error over normal_valid_mask(gt), then the mean of the per-image values (eval.py's reduction).  Samples without a normal
    path (column gt_column absent or "None") or without a prediction file are skipped.  Optionally writes `eval_metrics-normal.txt` and
    `per_sample_metrics-normal.csv`."""
    names = list(NORMAL_METRICS)

    def score(s, rel, pred_path):
        gt = (read_gt or read_gt_normal)(os.path.join(base_dir, rel))
        pred = em.decode_normals(np.load(pred_path))
        _same_size(s, pred.shape, gt.shape)
        return em.normal_angular_error(pred, gt, normal_valid_mask(gt))

    per_sample, result = _evaluate_files(prediction_dir, samples, gt_column, lambda s: _pred_name(s[0], name_mode), score, names)
    if output_dir is not None:
        _write_normal_eval_files(output_dir, names, per_sample, result, prediction_dir, gt_column)
    return result


# ---- the loops where predictions never leave the GPU ------------------------------------------------------------------------------------
def _all_reduce_sum(acc: np.ndarray) -> np.ndarray:
    """The float64 vector summed over the ranks of an initialised torch.distributed (on the device for nccl); unchanged for one process."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return acc
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.from_numpy(np.ascontiguousarray(acc, dtype=np.float64)).to(dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def _evaluation_loop(samples: Sequence[Sequence[str]], keep: Callable, load: Callable, score_group: Callable, names: List[str], batch_size: int,
                     rank: int, world: int, prefetch: int):
    """The sharding and combining core under `_infer_and_score`.  `samples` filtered by `keep`, then sharded
    (`shard_range`), the index in the filtered list riding along; images decoded ahead by `load(sample)` and grouped by size, at most batch_size
    per group; `score_group([((index, sample), image), ...])` -> one list of metric values (in `names` order) per image.  With
    torch.distributed initialised the rows of all ranks are combined: float64 sums and a count by all_reduce, rows by all_gather_object.
    Returns (rows [(index, sample, values)] in sample order, means over all samples, whether this rank writes the files)."""
    samples = [s for s in samples if keep(s)]
    lo, hi = _shard(len(samples), rank, world) if world > 1 else (0, len(samples))
    items = [(i, samples[i]) for i in range(lo, hi)]  # the index in the filtered list rides along: the rows of all ranks are ordered by it
    rows = []  # (sample index, sample, metric values)
    for group in _size_groups(_decode_ahead(items, lambda it: load(it[1]), prefetch), batch_size):
        values = score_group(group)
        assert len(values) == len(group)
        for ((idx, smp), _), vals in zip(group, values):
            rows.append((idx, list(smp), [float(v) for v in vals]))

    acc = np.zeros(len(names) + 1, dtype=np.float64)  # metric sums of this rank, then its image count
    for _, _, vals in rows:
        acc[:-1] += vals
        acc[-1] += 1
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        acc = _all_reduce_sum(acc)
        parts: list = [None] * dist.get_world_size()
        dist.all_gather_object(parts, rows)
        rows = [r for part in parts for r in part]
        writer = dist.get_rank() == 0
    else:
        writer = True
    rows.sort(key=lambda r: r[0])
    n = int(acc[-1])
    result = {k: (float(acc[j]) / n if n else float("nan")) for j, k in enumerate(names)}
    return rows, result, writer


def _infer_options(denoise_steps, ensemble_size, processing_res, match_input_res, resample_method, fix_timesteps, prompt, refine=None,
                   tiles=None) -> dict:
    """The inference options a device loop passes through, as the keyword arguments of `pipe.predict_batch_device` (`refine` and `tiles` only
    when set)."""
    options = dict(processing_res=processing_res, match_input_res=match_input_res, resample_method=resample_method, fix_timesteps=fix_timesteps,
                   prompt=prompt, denoising_steps=denoise_steps, ensemble_size=ensemble_size)
    if refine is not None:
        options["refine"] = refine
    if tiles is not None:
        options["tiles"] = tiles
    return options


def _upload(arrays, device):
    """the arrays of a batch stacked and sent to the device (one copy, not waited for)"""
    import torch
    return torch.from_numpy(np.stack(arrays)).to(device, non_blocking=True)


def _infer_and_score(pipe, base_dir: str, samples, mode: str, channels: int, infer_options: dict, keep: Callable, read_gt: Callable, gt_dims: int,
                     score_batch: Callable, names: List[str], pred_name_of: Callable, batch_size: int, rank: int, world: int, prefetch: int,
                     save_predictions: bool, prediction_dir: Optional[str], output_dir: Optional[str], rgb_crop: Optional[Callable] = None):
    """The skeleton of the device loops, on top of `_evaluation_loop`.  Per batch: `pipe.predict_batch_device(images, mode, **infer_options)`
    gives [B, channels, H, W] maps that stay on the device; `read_gt(sample)` decodes each ground truth on the host, its first gt_dims
    dimensions checked against the last gt_dims of the maps (2: H x W, 3: a [3, H, W] ground truth); `score_batch(pred, gts, samples,
    indices)` uploads and scores them: one metric dict per image.  save_predictions: the maps are also written as `run_inference` would,
    [H, W] or [H, W, 3] `.npy` under prediction_dir (default: output_dir).  Returns (means over all samples, the rows of the per-sample file
    if this rank is to write the files -- output_dir given and rank 0 -- else None, prediction_dir, the number of images of all ranks)."""
    if prediction_dir is None:
        prediction_dir = output_dir
    if save_predictions and prediction_dir is None:
        raise ValueError("save_predictions needs prediction_dir or output_dir")

    def score_group(group):
        smps = [smp for (_, smp), _ in group]
        pred = pipe.predict_batch_device([img for _, img in group], mode, **infer_options)
        if pred.dim() != 4 or pred.shape[0] != len(group) or pred.shape[1] != channels:
            raise ValueError(f"evaluation in mode {mode!r} needs {'one' if channels == 1 else 'three'}-channel maps [B, {channels}, H, W], got "
                             f"{tuple(pred.shape)}")
        gts = []
        for smp in smps:
            gt = np.asarray(read_gt(smp))
            _same_size(smp, pred.shape[-gt_dims:], gt.shape[:gt_dims])
            gts.append(gt)
        metrics = score_batch(pred, gts, smps, [idx for (idx, _), _ in group])
        assert len(metrics) == len(group)
        if save_predictions:
            pred_host = (pred[:, 0] if channels == 1 else pred).cpu().numpy()
            for smp, p in zip(smps, pred_host):
                os.makedirs(os.path.dirname(os.path.join(prediction_dir, pred_name_of(smp))), exist_ok=True)
                np.save(os.path.join(prediction_dir, pred_name_of(smp)), p if channels == 1 else np.transpose(p, (1, 2, 0)))
        return [[m[k] for k in names] for m in metrics]

    rows, result, writer = _evaluation_loop(samples, keep, lambda smp: _load_rgb(base_dir, smp[0], rgb_crop), score_group, names, batch_size, rank,
                                            world, prefetch)
    per_sample = [(pred_name_of(smp), vals) for _, smp, vals in rows] if output_dir is not None and writer else None
    return result, per_sample, prediction_dir, len(rows)


def infer_and_evaluate(pipe, base_dir: str, samples: Sequence[Sequence[str]], dataset: str, output_dir: Optional[str] = None, batch_size: int = 4,
                       rank: int = 0, world: int = 1, alignment: Optional[str] = "least_square", alignment_max_res: Optional[int] = None,
                       save_predictions: bool = False, evaluator: Optional[Callable] = None, mode: str = "depth", denoise_steps: int = 1,
                       ensemble_size: int = 1, processing_res: int = 0, match_input_res: bool = True, resample_method: str = "bilinear",
                       fix_timesteps=None, prompt: str = "", prefetch: int = 2, prediction_dir: Optional[str] = None) -> Dict[str, float]:
    """infer.py:408-447 and eval.py:143-244 in one loop, without the `.npy` round trip: batches of equal-sized images (grouping and sharding as
    in `run_inference`) go through `pipe.predict_batch_device`, the maps stay on the device, and `evaluator` -- `engine.eval_depth` unless
    given: (pred, gt, mask, alignment, alignment_max_res, min_depth, max_depth) -> (one metric dict per image, ...) -- aligns and scores them
    there.  Ground truth and validity mask are decoded on the host exactly as `evaluate_predictions` does (read_gt_depth, dataset_valid_mask;
    KITTI: benchmark crop of RGB and depth) and uploaded per batch.  save_predictions: the maps are also written as `run_inference` would,
    under prediction_dir (default: output_dir).  With torch.distributed initialised the per-image rows of all ranks are combined (float64
    sums and a count by all_reduce, rows by all_gather_object); rank 0 writes `eval_metrics-<alignment>.txt` and
    `per_sample_metrics-<alignment>.csv` with rows in sample order; every rank returns the means over all samples."""
    cfg = DATASETS[dataset]
    names = list(em.METRICS.keys())
    if evaluator is None:
        from .engine import eval_depth as evaluator

    def score_batch(pred, gts, smps, _):
        vms = [dataset_valid_mask(gt, dataset, os.path.join(base_dir, smp[2]) if cfg.get("mask_from_file") and len(smp) > 2 else None)
               for gt, smp in zip(gts, smps)]
        return evaluator(pred[:, 0], _upload(gts, pred.device), _upload(vms, pred.device), alignment, alignment_max_res, cfg["min_depth"],
                         cfg["max_depth"])[0]

    options = _infer_options(denoise_steps, ensemble_size, processing_res, match_input_res, resample_method, fix_timesteps, prompt)
    result, per_sample, prediction_dir, _ = _infer_and_score(
        pipe, base_dir, samples, mode, 1, options, lambda s: len(s) < 2 or s[1] != "None",
        lambda smp: read_gt_depth(os.path.join(base_dir, smp[1]), dataset), 2, score_batch, names, lambda smp: _pred_name(smp[0], cfg["name_mode"]),
        batch_size, rank, world, prefetch, save_predictions, prediction_dir, output_dir, kitti_benchmark_crop if cfg.get("kitti_bm_crop") else None)
    if per_sample is not None:
        _write_eval_files(output_dir, alignment, names, per_sample, result, prediction_dir, dataset)
    return result


def infer_and_evaluate_normals(pipe, base_dir: str, samples: Sequence[Sequence[str]], output_dir: Optional[str] = None,
                               name_mode: FileNameMode = FileNameMode.id, gt_column: int = 3, batch_size: int = 4, rank: int = 0, world: int = 1,
                               save_predictions: bool = False, prediction_dir: Optional[str] = None, evaluator: Optional[Callable] = None,
                               read_gt: Optional[Callable[[str], np.ndarray]] = None, denoise_steps: int = 1, ensemble_size: int = 1,
                               processing_res: int = 0, match_input_res: bool = True, resample_method: str = "bilinear", fix_timesteps=None,
                               prompt: str = "", prefetch: int = 2) -> Dict[str, float]:
    """`infer_and_evaluate` for surface normals: batches go through `pipe.predict_batch_device(mode="normal")`, the [B, 3, H, W] maps (the
    [0, 1] encoding) stay on the device, and `evaluator` -- `engine.eval_normal` unless given: (pred, gt, mask, pred_encoded, gt_encoded) ->
    (one dict per image with NORMAL_METRICS, ...) -- scores them there against the signed ground truth of column gt_column (read_gt_normal
    or `read_gt`), decoded on the host and uploaded per batch, with mask None: the derived rule of normal_valid_mask.  What it computes per
    image is `evaluate_normal_predictions`' quantity; sharding, the torch.distributed combination, the rank-0 files (`eval_metrics-normal.txt`,
    `per_sample_metrics-normal.csv`) and the return value on every rank are `infer_and_evaluate`'s.  save_predictions: the maps are also
    written as `run_inference(mode="normal")` would, [H, W, 3] `.npy` under prediction_dir (default: output_dir)."""
    names = list(NORMAL_METRICS)
    if evaluator is None:
        from .engine import eval_normal as evaluator

    def score_batch(pred, gts, smps, _):
        return evaluator(pred, _upload([np.asarray(gt, dtype=np.float32) for gt in gts], pred.device), None, True, False)[0]

    options = _infer_options(denoise_steps, ensemble_size, processing_res, match_input_res, resample_method, fix_timesteps, prompt)
    result, per_sample, prediction_dir, _ = _infer_and_score(
        pipe, base_dir, samples, "normal", 3, options, lambda s: _gt_rel(s, gt_column) is not None,
        lambda smp: (read_gt or read_gt_normal)(os.path.join(base_dir, _gt_rel(smp, gt_column))), 3, score_batch, names,
        lambda smp: _pred_name(smp[0], name_mode), batch_size, rank, world, prefetch, save_predictions, prediction_dir, output_dir)
    if per_sample is not None:
        _write_normal_eval_files(output_dir, names, per_sample, result, prediction_dir, gt_column)
    return result


# ---- dis / matting: 8-bit masks and alpha maps ------------------------------------------------------------------------------------------------
MASK_METRICS = list(em.MASK_METRICS)  # per-image values, in order; the dataset-level "max_f_dataset" comes on top
STRUCTURE_METRICS = list(em.STRUCTURE_METRICS)  # with structure=True: appended to the per-image columns, the means and the files
MATTING_METRICS = list(em.MATTING_METRICS)  # with matting=True: appended after them
TRIMAP_METRICS = list(em.TRIMAP_METRICS)  # with trimap_radius: the transition-region and side scores of the trimap-free matting protocol, after them
BOUNDARY_METRICS = list(em.BOUNDARY_METRICS)  # with boundary_iou=True: Boundary IoU, last


def read_gt_mask(path: str) -> np.ndarray:
    """An 8-bit mask / alpha map as uint8 [H, W].  A three-channel file whose channels are equal gives channel 0 (the rule of the reference's
    _read_depth_file, src/dataset/base_dataset.py:399-408); an alpha channel on top is ignored.  Other formats: pass a `read_gt` callable."""
    a = np.asarray(Image.open(path))
    if a.ndim == 3 and a.shape[2] in (3, 4):
        if not (np.all(a[:, :, 0] == a[:, :, 1]) and np.all(a[:, :, 0] == a[:, :, 2])):
            raise ValueError(f"{path}: the three channels differ; a mask is one channel")
        a = a[:, :, 0]
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"{path}: expected an 8-bit single-channel image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _read_mask_prediction(path: str) -> np.ndarray:
    """What `run_inference(mode="dis" | "matting")` writes (`.npy`, float [H, W] in [0, 1]) or the 8-bit `.png` of the same map."""
    if os.path.splitext(path)[1].lower() == ".npy":
        p = np.load(path).squeeze()
        if p.ndim != 2:
            raise ValueError(f"{path}: expected a single-channel map, got {p.shape}")
        return p
    return read_gt_mask(path)


def _max_f_of_mean_curves(curve_sums: np.ndarray, n: int) -> float:
    """The usual dis protocol: max_t F_t of the DATASET-MEAN precision and recall curves.  curve_sums: float64 [512] = the per-image precision
    curves summed, then the recall curves; n images."""
    if n == 0:
        return float("nan")
    best = 0.0
    for t in range(256):
        p, r = float(curve_sums[t]) / n, float(curve_sums[256 + t]) / n
        den = 0.3 * p + r
        best = max(best, (1.3 * p * r) / den if den != 0.0 else 0.0)
    return best


def _sum_curves(counts_in_order) -> np.ndarray:
    acc = np.zeros(512, dtype=np.float64)
    for c in counts_in_order:
        prec, rec, _ = em.mask_curves_from_counts(c)
        acc[:256] += prec
        acc[256:] += rec
    return acc


def _mask_options(region_of, structure: bool, matting: bool, trimap_radius, trimap_metric, boundary_iou: bool, boundary_ratio: float,
                  evaluators: Optional[dict] = None):
    """The optional mask metrics of one call, checked, in column order: ([(column names, score, prefix errors)], all the column names, the
    header lines of the band options).  score(pred, gt, region) -> one dict per image of a batch.  evaluators None: the file route, a batch is
    one image and eval_metrics scores it; else the device loop's evaluator arguments by option (None: engine's), which take the same
    arguments.  prefix errors: the option derives its region from the ground truth, so its ValueError has to name the images."""
    if structure and region_of is not None:
        raise ValueError("structure scores are whole-image quantities: structure=True does not go with region_of")
    if (trimap_radius is not None or boundary_iou) and region_of is not None:
        raise ValueError("trimap_radius / boundary_iou derive their regions from the ground truth: they do not go with region_of")
    options, note = [], ""

    def add(columns, host, device, args_of, prefix=False):
        if evaluators is None:
            fn = getattr(em, host)
            options.append((list(columns), lambda p, g, r: [fn(*args_of(p, g, r))], prefix))
        else:
            from . import engine
            fn = evaluators.get(device) or getattr(engine, device)
            options.append((list(columns), lambda p, g, r: fn(*args_of(p, g, r)), prefix))

    if structure:
        add(STRUCTURE_METRICS, "structure_metrics", "eval_structure", lambda p, g, r: (p, g))
    if matting:
        add(MATTING_METRICS, "matting_metrics", "eval_matting", lambda p, g, r: (p, g, r))
    if trimap_radius is not None:
        em.band_reach(trimap_radius, trimap_metric)  # (raises on a bad radius or metric)
        add(TRIMAP_METRICS, "trimap_metrics", "eval_trimap", lambda p, g, r: (p, g, trimap_radius, trimap_metric), prefix=True)
        note += f"    trimap from the ground truth: radius {trimap_radius:g}, metric {trimap_metric}\n"
    if boundary_iou:
        if not boundary_ratio > 0:
            raise ValueError(f"boundary_ratio is > 0, got {boundary_ratio}")
        add(BOUNDARY_METRICS, "boundary_iou", "eval_boundary_iou", lambda p, g, r: (p, g, boundary_ratio))
        note += f"    boundary IoU: band of {boundary_ratio:g} of the image diagonal\n"
    return options, list(MASK_METRICS) + [k for columns, _, _ in options for k in columns], note


def _with_mask_options(metrics: List[dict], options, pred, gt, region, who: Callable[[], str]) -> List[dict]:
    """`metrics` (one dict per image of the batch pred, gt, region) with the columns of `_mask_options` added; who(): the images' names."""
    for columns, score, prefix in options:
        try:
            more = score(pred, gt, region)
        except ValueError as e:
            if not prefix:
                raise
            raise ValueError(f"{who()}: {e}") from None
        assert len(more) == len(metrics)
        metrics = [dict(m, **{k: v[k] for k in columns}) for m, v in zip(metrics, more)]
    return metrics


def _write_mask_eval_files(output_dir: str, names: List[str], per_sample, result: Dict[str, float], prediction_dir: Optional[str],
                           note: str = "") -> None:
    """`per_sample_metrics-mask.csv` and `eval_metrics-mask.txt`, laid out like the depth files; the dataset-level value sits in the header."""
    header = f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on 8-bit masks: column 1 of the filename list\n{note}"
    header += f"max_f_dataset = {result['max_f_dataset']:.6g}\n"
    _write_metric_files(output_dir, "-mask", names, per_sample, result, header)


def evaluate_mask_predictions(prediction_dir: str, base_dir: str, samples: Sequence[Sequence[str]], name_mode: FileNameMode,
                              output_dir: Optional[str] = None, pred_suffix: str = ".npy", region_of: Optional[Callable] = None,
                              read_gt: Optional[Callable[[str], np.ndarray]] = None, structure: bool = False,
                              matting: bool = False, trimap_radius: Optional[float] = None, trimap_metric: str = "euclidean",
                              boundary_iou: bool = False, boundary_ratio: float = 0.02) -> Dict[str, float]:
    """The file route for what `run_inference(mode="dis" | "matting")` writes (`.npy`) or for 8-bit `.png` maps (pred_suffix): per image
    eval_metrics.mask_metrics against the 8-bit ground truth of column 1 (read_gt_mask or `read_gt`), over `region_of(sample, gt)` (a bool
    array, e.g. a trimap's unknown region; None: every pixel).  Returns the means of the per-image MASK_METRICS and "max_f_dataset", the
    maximum F of the dataset-mean precision / recall curves.  Samples without ground truth ("None") or without a prediction file are
    skipped.  Optionally writes `eval_metrics-mask.txt` and `per_sample_metrics-mask.csv`.  structure: the dis structure scores
    (eval_metrics.structure_metrics: STRUCTURE_METRICS, whole-image quantities, so not together with region_of) as five more columns.
    matting: the gradient and connectivity errors (eval_metrics.matting_metrics: MATTING_METRICS, summed over the same region) as two more
    columns, after the structure columns if both are asked for.  trimap_radius: the trimap-free matting protocol (eval_metrics.trimap_metrics:
    TRIMAP_METRICS over the transition region and the two sides of the trimap that the ground-truth alpha gives with a disc -- trimap_metric
    "euclidean" -- or a square -- "chebyshev" -- of that radius) as five more columns.  boundary_iou: Boundary IoU (eval_metrics.boundary_iou
    with boundary_ratio of the diagonal) as one more column, last.  Neither goes with region_of; a header line states radius, metric, ratio."""
    options, names, note = _mask_options(region_of, structure, matting, trimap_radius, trimap_metric, boundary_iou, boundary_ratio)
    counts = []

    def score(s, rel, pred_path):
        gt = (read_gt or read_gt_mask)(os.path.join(base_dir, rel))
        pred = _read_mask_prediction(pred_path)
        _same_size(s, pred.shape, gt.shape)
        region = _region(region_of, s, gt)
        c = em.mask_counts(em.quantize_mask(pred), gt, region)
        if c[0] == 0:
            raise ValueError(f"{s[0]}: no pixel to evaluate the mask on (n = 0)")
        counts.append(c)
        return _with_mask_options([em.mask_metrics_from_counts(c)], options, pred, gt, region, lambda: s[0])[0]

    per_sample, result = _evaluate_files(prediction_dir, samples, 1, lambda s: _pred_name(s[0], name_mode, pred_suffix), score, names)
    result["max_f_dataset"] = _max_f_of_mean_curves(_sum_curves(counts), len(per_sample))
    if output_dir is not None:
        _write_mask_eval_files(output_dir, names, per_sample, result, prediction_dir, note)
    return result


def infer_and_evaluate_masks(pipe, base_dir: str, samples: Sequence[Sequence[str]], mode: str, output_dir: Optional[str] = None,
                             name_mode: FileNameMode = FileNameMode.id, batch_size: int = 4, rank: int = 0, world: int = 1,
                             save_predictions: bool = False, prediction_dir: Optional[str] = None, evaluator: Optional[Callable] = None,
                             read_gt: Optional[Callable[[str], np.ndarray]] = None, region_of: Optional[Callable] = None, denoise_steps: int = 1,
                             ensemble_size: int = 1, processing_res: int = 0, match_input_res: bool = True, resample_method: str = "bilinear",
                             fix_timesteps=None, prompt: str = "", prefetch: int = 2, structure: bool = False,
                             structure_evaluator: Optional[Callable] = None, matting: bool = False,
                             matting_evaluator: Optional[Callable] = None, trimap_radius: Optional[float] = None,
                             trimap_metric: str = "euclidean", trimap_evaluator: Optional[Callable] = None, boundary_iou: bool = False,
                             boundary_ratio: float = 0.02, boundary_evaluator: Optional[Callable] = None, refine=None, tiles=None) -> Dict[str, float]:
    """`infer_and_evaluate` for mode "dis" or "matting": batches go through `pipe.predict_batch_device(mode=mode)`, the float [B, 1, H, W] maps
    stay on the device, and `evaluator` -- `engine.eval_mask` unless given: (pred, gt, region) -> one dict per image with MASK_METRICS and
    "counts" -- quantises and scores them there against the 8-bit ground truth of column 1 (and `region_of(sample, gt)`, if given), decoded on
    the host and uploaded per batch.  What it computes per image is `evaluate_mask_predictions`' quantity, bit for bit; sharding, the
    torch.distributed combination, the rank-0 files (`eval_metrics-mask.txt`, `per_sample_metrics-mask.csv`) and the return value on every
    rank are `infer_and_evaluate`'s, with one more float64 all_reduce for the precision / recall curves behind "max_f_dataset".
    save_predictions: the maps are also written as `run_inference` would, float32 [H, W] `.npy` under prediction_dir (default: output_dir).
    structure: the dis structure scores as five more per-image columns (STRUCTURE_METRICS), from a second device call on the same uploaded
    batch -- `structure_evaluator`, `engine.eval_structure` unless given: (pred, gt) -> one dict per image; not together with region_of.
    matting: the gradient and connectivity errors as two more per-image columns (MATTING_METRICS, after the structure columns), from a further
    device call on the same uploaded batch and region -- `matting_evaluator`, `engine.eval_matting` unless given: (pred, gt, region) -> one
    dict per image.  trimap_radius: the trimap-free matting protocol as five more columns (TRIMAP_METRICS), the trimap made on the device from
    the uploaded ground truth -- `trimap_evaluator`, `engine.eval_trimap` unless given: (pred, gt, radius, metric) -> one dict per image.
    boundary_iou: Boundary IoU as one more column (BOUNDARY_METRICS, last) -- `boundary_evaluator`, `engine.eval_boundary_iou` unless given:
    (pred, gt, ratio) -> one dict per image.  Neither goes with region_of; a header line of the text file states radius, metric and ratio.
    refine (None, True or dict(radius=..., eps=...)): the maps come to the input size by the guided filter with the image as guide, so that
    a dataset can be scored with and without it; files and columns are the same.  tiles (None, True or dict(size=..., overlap=..., align=...,
    batch=...)): the maps are those of tiled inference (`pipe.predict_batch_device(..., tiles=...)`); files and columns are the same."""
    if mode not in ("dis", "matting"):
        raise ValueError(f"mask evaluation is for mode 'dis' or 'matting', got {mode!r}")
    options, names, note = _mask_options(region_of, structure, matting, trimap_radius, trimap_metric, boundary_iou, boundary_ratio,
                                         dict(eval_structure=structure_evaluator, eval_matting=matting_evaluator, eval_trimap=trimap_evaluator,
                                              eval_boundary_iou=boundary_evaluator))
    if evaluator is None:
        from .engine import eval_mask as evaluator
    counts = []  # (sample index, counts) of this rank's images

    def score_batch(pred, gts, smps, indices):
        gt_t = _upload(gts, pred.device)
        region_t = _upload([_region(region_of, smp, gt) for smp, gt in zip(smps, gts)], pred.device) if region_of is not None else None
        metrics = evaluator(pred[:, 0], gt_t, region_t)
        assert len(metrics) == len(smps)
        counts.extend((idx, np.asarray(m["counts"])) for idx, m in zip(indices, metrics))
        return _with_mask_options(metrics, options, pred[:, 0], gt_t, region_t, lambda: ", ".join(smp[0] for smp in smps))

    infer_options = _infer_options(denoise_steps, ensemble_size, processing_res, match_input_res, resample_method, fix_timesteps, prompt, refine, tiles)
    result, per_sample, prediction_dir, n = _infer_and_score(
        pipe, base_dir, samples, mode, 1, infer_options, lambda s: _gt_rel(s, 1) is not None,
        lambda smp: (read_gt or read_gt_mask)(os.path.join(base_dir, smp[1])), 2, score_batch, names, lambda smp: _pred_name(smp[0], name_mode),
        batch_size, rank, world, prefetch, save_predictions, prediction_dir, output_dir)
    counts.sort(key=lambda c: c[0])
    result["max_f_dataset"] = _max_f_of_mean_curves(_all_reduce_sum(_sum_curves([c for _, c in counts])), n)
    if per_sample is not None:
        _write_mask_eval_files(output_dir, names, per_sample, result, prediction_dir, note)
    return result


# ---- seg: colour maps against a user-supplied palette -----------------------------------------------------------------------------------------
SEG_METRICS = list(em.SEG_METRICS)  # per-image values, in order; "miou_dataset", "pixel_acc_dataset" and "iou_dataset" come on top


def read_palette(path: str) -> Tuple[np.ndarray, List[str]]:
    """(palette uint8 [K, 3], names) from a text file -- one `r g b [name]` per line, `#` starts a comment, a class without a name is called by
    its index -- or from a `.npy` of shape [K, 3] (integers in 0..255; names = the indices)."""
    if os.path.splitext(path)[1].lower() == ".npy":
        a = np.load(path)
        if a.ndim != 2 or a.shape[1] != 3 or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
            raise ValueError(f"{path}: expected integers in 0..255 of shape [K, 3], got {a.dtype} {a.shape}")
        rows, names = [tuple(int(v) for v in r) for r in a], [str(k) for k in range(a.shape[0])]
    else:
        rows, names = [], []
        with open(path, "r") as f:
            for no, line in enumerate(f, 1):
                parts = line.split("#", 1)[0].split()
                if not parts:
                    continue
                try:
                    rgb = tuple(int(v) for v in parts[:3])
                except ValueError:
                    rgb = ()
                if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
                    raise ValueError(f"{path}:{no}: expected `r g b [name]` with 0 <= r, g, b <= 255, got {line.strip()!r}")
                rows.append(rgb)
                names.append(" ".join(parts[3:]) or str(len(names)))
    if not 1 <= len(rows) <= em.SEG_MAX_K:
        raise ValueError(f"{path}: a palette has 1 to {em.SEG_MAX_K} colours, got {len(rows)}")
    return np.array(rows, dtype=np.uint8).reshape(-1, 3), names


def read_gt_seg(path: str) -> np.ndarray:
    """Seg ground truth as the reference's column 6 stores it (src/dataset/base_dataset.py:333-346,366): an RGB or palettised image gives the
    colour form uint8 [H, W, 3] (an alpha channel is dropped), a single-channel 8-bit image the label map uint8 [H, W].  Other formats: pass
    a `read_gt` callable."""
    img = Image.open(path)
    if img.mode in ("P", "RGB", "RGBA"):
        return np.ascontiguousarray(np.asarray(img.convert("RGB")))
    if img.mode == "L":
        return np.ascontiguousarray(np.asarray(img))
    raise ValueError(f"{path}: expected an RGB, palettised or 8-bit single-channel image, got mode {img.mode}")


def _read_seg_prediction(path: str) -> np.ndarray:
    """What `run_inference(mode="seg")` writes (`.npy`, float [H, W, 3] in [0, 1]) or the 8-bit RGB `.png` of the same map."""
    if os.path.splitext(path)[1].lower() == ".npy":
        p = np.load(path)
        if p.ndim != 3 or p.shape[-1] != 3:
            raise ValueError(f"{path}: expected a colour map [H, W, 3], got {p.shape}")
        return p
    a = np.asarray(Image.open(path))
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.dtype != np.uint8:
        raise ValueError(f"{path}: expected an 8-bit RGB image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a[:, :, :3])


def _palette_and_names(palette) -> Tuple[np.ndarray, List[str]]:
    """palette: uint8 [K, 3], or the (palette, names) pair `read_palette` returns"""
    names = None
    if isinstance(palette, (tuple, list)) and len(palette) == 2 and isinstance(palette[1], (tuple, list)) and all(isinstance(n, str) for n in palette[1]):
        palette, names = palette
    pal = em._check_palette(np.asarray(palette))
    names = [str(k) for k in range(pal.shape[0])] if names is None else list(names)
    if len(names) != pal.shape[0]:
        raise ValueError(f"{len(names)} names for {pal.shape[0]} palette colours")
    return np.ascontiguousarray(pal), names


def _seg_dataset_values(result: Dict, conf_sum: np.ndarray, K: int) -> None:
    """The usual protocol: scores of the SUMMED confusion matrix of all images (float64 [K * K], exact below 2^53) into `result`."""
    conf = [int(v) for v in conf_sum]
    m = em.seg_metrics_from_counts([sum(conf), 0, 0] + conf, K)
    result["miou_dataset"], result["pixel_acc_dataset"], result["iou_dataset"] = m["miou"], m["pixel_acc"], list(m["iou"])


def _write_seg_eval_files(output_dir: str, names: List[str], per_sample, result: Dict, prediction_dir: Optional[str], gt_column: int,
                          class_names: List[str]) -> None:
    """`per_sample_metrics-seg.csv` and `eval_metrics-seg.txt`, laid out like the depth files; the dataset-level values and the per-class IoU
    (one `name = value` line per palette colour) sit in the header."""
    header = f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on seg labels: column {gt_column} of the filename list\n"
    header += f"miou_dataset = {result['miou_dataset']:.6g}\npixel_acc_dataset = {result['pixel_acc_dataset']:.6g}\n"
    header += "iou_dataset of the classes " + ", ".join(class_names) + ":\n"
    header += "".join(f"    {nm} = {v:.6g}\n" for nm, v in zip(class_names, result["iou_dataset"]))
    _write_metric_files(output_dir, "-seg", names, per_sample, result, header)


def evaluate_seg_predictions(prediction_dir: str, base_dir: str, samples: Sequence[Sequence[str]], name_mode: FileNameMode, palette,
                             output_dir: Optional[str] = None, pred_suffix: str = ".npy", gt_column: int = 6, gt_tol: int = 0,
                             region_of: Optional[Callable] = None, read_gt: Optional[Callable[[str], np.ndarray]] = None) -> Dict:
    """The file route for what `run_inference(mode="seg")` writes (`.npy`, float [H, W, 3]) or for 8-bit RGB `.png` maps (pred_suffix): per image
    eval_metrics.seg_metrics against the ground truth of column gt_column (read_gt_seg or `read_gt`: a colour image or a label map), with
    `palette` (uint8 [K, 3], or the pair `read_palette` returns) and gt_tol, over `region_of(sample, gt)` (a bool array; None: every pixel).
    Returns the means of the per-image SEG_METRICS and, from the summed confusion matrix of all images, "miou_dataset", "pixel_acc_dataset"
    and "iou_dataset" (a list of K).  Samples without ground truth (column absent or "None") or without a prediction file are skipped.
    Optionally writes `eval_metrics-seg.txt` and `per_sample_metrics-seg.csv`."""
    pal, class_names = _palette_and_names(palette)
    K = pal.shape[0]
    names = list(SEG_METRICS)
    conf_sum = np.zeros(K * K, dtype=np.float64)

    def score(s, rel, pred_path):
        gt = (read_gt or read_gt_seg)(os.path.join(base_dir, rel))
        pred = _read_seg_prediction(pred_path)
        _same_size(s, pred.shape[:2], gt.shape[:2])
        m = em.seg_metrics(pred, gt, pal, _region(region_of, s, gt), gt_tol)
        if m["n"] == 0:
            raise ValueError(f"{s[0]}: no pixel to evaluate the segmentation on (n = 0)")
        conf_sum[:] += m["conf"].reshape(-1)
        return m

    per_sample, result = _evaluate_files(prediction_dir, samples, gt_column, lambda s: _pred_name(s[0], name_mode, pred_suffix), score, names)
    _seg_dataset_values(result, conf_sum, K)
    if output_dir is not None:
        _write_seg_eval_files(output_dir, names, per_sample, result, prediction_dir, gt_column, class_names)
    return result


def infer_and_evaluate_seg(pipe, base_dir: str, samples: Sequence[Sequence[str]], palette, output_dir: Optional[str] = None,
                           name_mode: FileNameMode = FileNameMode.id, batch_size: int = 4, rank: int = 0, world: int = 1,
                           save_predictions: bool = False, prediction_dir: Optional[str] = None, evaluator: Optional[Callable] = None,
                           read_gt: Optional[Callable[[str], np.ndarray]] = None, region_of: Optional[Callable] = None, denoise_steps: int = 1,
                           ensemble_size: int = 1, processing_res: int = 0, match_input_res: bool = True, resample_method: str = "bilinear",
                           fix_timesteps=None, prompt: str = "", prefetch: int = 2, gt_column: int = 6, gt_tol: int = 0) -> Dict:
    """`infer_and_evaluate` for mode "seg": batches go through `pipe.predict_batch_device(mode="seg")`, the float [B, 3, H, W] colour maps stay
    on the device, and `evaluator` -- `engine.eval_seg` unless given: (pred, gt, palette, region, gt_tol) -> one dict per image with SEG_METRICS
    and "conf" -- quantises, decodes and scores them there against the ground truth of column gt_column (read_gt_seg or `read_gt`; and
    `region_of(sample, gt)`, if given), decoded on the host and uploaded per batch (a batch that mixes colour images and label maps goes up as
    label maps).  What it computes per image is `evaluate_seg_predictions`' quantity, bit for bit; sharding, the torch.distributed
    combination, the rank-0 files (`eval_metrics-seg.txt`, `per_sample_metrics-seg.csv`) and the return value on every rank are
    `infer_and_evaluate`'s, with one more float64 all_reduce for the K x K confusion matrix behind the dataset-level values.
    save_predictions: the maps are also written as `run_inference(mode="seg")` would, float32 [H, W, 3] `.npy` under prediction_dir (default:
    output_dir)."""
    import torch
    pal, class_names = _palette_and_names(palette)
    K = pal.shape[0]
    names = list(SEG_METRICS)
    if evaluator is None:
        from .engine import eval_seg as evaluator
    conf_sum = np.zeros(K * K, dtype=np.float64)  # this rank's images
    pal_dev: dict = {}  # the palette goes up once per device

    def score_batch(pred, gts, smps, _):
        regions = [_region(region_of, smp, gt) for smp, gt in zip(smps, gts)]
        if len({g.ndim for g in gts}) > 1:
            gts = [em.seg_gt_labels(g, pal, gt_tol) for g in gts]
        if pred.device not in pal_dev:
            pal_dev[pred.device] = torch.from_numpy(pal).to(pred.device)
        metrics = evaluator(pred, _upload(gts, pred.device), pal_dev[pred.device], _upload(regions, pred.device) if region_of is not None else None,
                            gt_tol)
        for m in metrics:
            conf_sum[:] += np.asarray(m["conf"]).reshape(-1)
        return metrics

    options = _infer_options(denoise_steps, ensemble_size, processing_res, match_input_res, resample_method, fix_timesteps, prompt)
    result, per_sample, prediction_dir, _ = _infer_and_score(
        pipe, base_dir, samples, "seg", 3, options, lambda s: _gt_rel(s, gt_column) is not None,
        lambda smp: (read_gt or read_gt_seg)(os.path.join(base_dir, _gt_rel(smp, gt_column))), 2, score_batch, names,
        lambda smp: _pred_name(smp[0], name_mode), batch_size, rank, world, prefetch, save_predictions, prediction_dir, output_dir)
    _seg_dataset_values(result, _all_reduce_sum(conf_sum), K)
    if per_sample is not None:
        _write_seg_eval_files(output_dir, names, per_sample, result, prediction_dir, gt_column, class_names)
    return result
