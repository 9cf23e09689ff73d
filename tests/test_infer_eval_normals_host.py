"""Host tests (no GPU) of the surface-normal evaluation protocol in `infer_eval`: ground-truth reader and validity rule, the `.npy` route
`evaluate_normal_predictions`, and the loop `infer_and_evaluate_normals` with a fake pipeline and the NumPy evaluator
(eval_metrics.normal_angular_error) injected in place of engine.eval_normal; the world-size-2 combination runs over gloo in two processes."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(24, 32), (24, 32), (24, 32), (20, 28), (24, 32)]  # (H, W): the fourth image has another size
NAMES = ["mean_rad", "mean_deg", "median_deg", "rmse_deg", "within_11.25", "within_22.5", "within_30"]


def make_tree(base):
    """5 RGB images and ground-truth normals (signed, not unit length, a tenth of the pixels all-zero = invalid), stored alternately as
    [H, W, 3] and [3, H, W] `.npy` files; filename-list lines `rgb depth filled normal`."""
    rng = np.random.RandomState(11)
    samples = []
    for i, (h, w) in enumerate(SIZES):
        scene = os.path.join(base, f"scene{i // 3:04d}_00")
        for d in ("color", "normal"):
            os.makedirs(os.path.join(scene, d), exist_ok=True)
        Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(scene, "color", f"{i:06d}.png"))
        n = (rng.randn(h, w, 3) * (0.5 + rng.rand(h, w, 1))).astype(np.float32)
        n[rng.rand(h, w) < 0.1] = 0.0
        np.save(os.path.join(scene, "normal", f"{i:06d}.npy"), n if i % 2 == 0 else np.moveaxis(n, -1, 0))
        samples.append([f"scene{i // 3:04d}_00/color/{i:06d}.png", f"scene{i // 3:04d}_00/depth/{i:06d}.png", "None",
                        f"scene{i // 3:04d}_00/normal/{i:06d}.npy"])  # (the depth file is never opened here)
    return samples


def fake_pred(img):
    """A deterministic [H, W, 3] float32 map in [0, 1] from the RGB image."""
    a = np.asarray(img.convert("RGB")).astype(np.float32) / 255.0
    return np.stack([a[..., 0] * 0.6 + a[..., 1] * 0.4, a[..., 1], 0.5 + 0.5 * a[..., 2]], axis=-1).astype(np.float32)


class FakePipe:
    def __init__(self):
        self.single, self.batches = 0, []

    def __call__(self, img, **kw):
        assert kw["batch_size"] == 0 and kw["color_map"] is None and kw["mode"] == "normal"
        self.single += 1
        return SimpleNamespace(pred_np=fake_pred(img), pred_colored=None)

    def predict_batch_device(self, images, mode, **kw):
        assert mode == "normal" and len({im.size for im in images}) == 1
        self.batches.append(len(images))
        return torch.from_numpy(np.stack([np.moveaxis(fake_pred(im), -1, 0) for im in images]))


def numpy_evaluator(pred, gt, mask, pred_encoded, gt_encoded):
    """engine.eval_normal's contract on CPU tensors: decode as asked, the derived validity rule for mask None."""
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    assert mask is None and pred_encoded and not gt_encoded
    out = []
    for p, g in zip(pred, gt):
        p, g = p.numpy(), g.numpy()
        out.append(em.normal_angular_error(p.astype(np.float64) * 2.0 - 1.0, g, ie.normal_valid_mask(g)))
    return out, None


def test_read_gt_normal_and_valid_mask(tmp_path):
    from genpercept_amd import infer_eval as ie
    rng = np.random.RandomState(0)
    n = rng.randn(6, 9, 3).astype(np.float64)
    n[2, 3] = 0.0
    n[4, 5] = (0.0, 0.0, -0.25)  # one non-zero channel is enough
    np.save(tmp_path / "hwc.npy", n)
    np.save(tmp_path / "chw.npy", np.moveaxis(n, -1, 0))
    a, b = ie.read_gt_normal(str(tmp_path / "hwc.npy")), ie.read_gt_normal(str(tmp_path / "chw.npy"))
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (3, 6, 9) and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, np.moveaxis(n, -1, 0).astype(np.float32)) and np.array_equal(a, b)
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(tmp_path / "n.png")
    for bad in ("n.png", "n.exr", "n"):
        with pytest.raises(ValueError):
            ie.read_gt_normal(str(tmp_path / bad))
    np.save(tmp_path / "flat.npy", np.zeros((6, 9)))
    with pytest.raises(ValueError):
        ie.read_gt_normal(str(tmp_path / "flat.npy"))
    m = ie.normal_valid_mask(a)
    assert m.dtype == bool and m.shape == (6, 9) and not m[2, 3] and m[4, 5] and m.sum() == 6 * 9 - 1
    assert np.array_equal(m, (a != 0).any(axis=0))


def test_evaluate_normal_predictions_is_per_image_angular_error(tmp_path):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base, pred_dir, out = str(tmp_path / "data"), str(tmp_path / "pred"), str(tmp_path / "eval")
    samples = make_tree(base)
    pipe = FakePipe()
    written = ie.run_inference(pipe, base, samples, pred_dir, ie.FileNameMode.id, mode="normal")
    assert pipe.single == 5 and len(written) == 5
    os.remove(written[4])                                                         # a sample without a prediction file is skipped ...
    with_gaps = samples[:2] + [["x.png", "None"], ["y.png", "None", "None", "None"]] + samples[2:]   # ... and so is one without a normal path
    res = ie.evaluate_normal_predictions(pred_dir, base, with_gaps, ie.FileNameMode.id, output_dir=out)
    assert list(res) == NAMES == list(ie.NORMAL_METRICS)
    rows = []
    for s, path in zip(samples[:4], written[:4]):
        gt = ie.read_gt_normal(os.path.join(base, s[3]))
        pred = np.load(path)
        assert pred.shape == gt.shape[1:] + (3,)
        rows.append(em.normal_angular_error(em.decode_normals(pred), gt, ie.normal_valid_mask(gt)))
    for k in NAMES:
        assert res[k] == sum(r[k] for r in rows) / 4, k
    lines = open(os.path.join(out, "per_sample_metrics-normal.csv")).read().splitlines()
    assert lines[0] == "filename," + ",".join(NAMES) and len(lines) == 1 + 4
    for ln, s, r in zip(lines[1:], samples, rows):
        assert ln == os.path.join(os.path.dirname(s[0]), "pred_" + os.path.basename(s[0])[:-4] + ".npy") + "," + ",".join(str(r[k]) for k in NAMES)
    txt = open(os.path.join(out, "eval_metrics-normal.txt")).read().splitlines()
    assert txt[-2] == "  ".join(NAMES) and txt[-1] == "  ".join(f"{res[k]:.6g}" for k in NAMES)
    # a read_gt callable replaces the reader; nothing to evaluate gives NaN
    res2 = ie.evaluate_normal_predictions(pred_dir, base, samples, ie.FileNameMode.id, read_gt=lambda p: ie.read_gt_normal(p) * 2.0)
    for k in NAMES:
        assert res2[k] == res[k]   # only directions matter, and a power of two scales every float32 exactly
    assert all(np.isnan(v) for v in ie.evaluate_normal_predictions(pred_dir, base, [["x.png", "None"]], ie.FileNameMode.id).values())


@pytest.mark.parametrize("batch_size", [1, 3])
def test_infer_and_evaluate_normals_equals_files_then_evaluate(tmp_path, batch_size):
    from genpercept_amd import infer_eval as ie
    base, pred_dir, ev_dir, out_dir = (str(tmp_path / d) for d in ("data", "pred", "eval_ref", "eval_dev"))
    samples = make_tree(base)
    ie.run_inference(FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="normal")
    ref = ie.evaluate_normal_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=ev_dir)
    pipe = FakePipe()
    res = ie.infer_and_evaluate_normals(pipe, base, samples, output_dir=out_dir, batch_size=batch_size, evaluator=numpy_evaluator)
    assert pipe.batches == ([1] * 5 if batch_size == 1 else [3, 1, 1])
    assert list(res) == NAMES
    for k in NAMES:
        assert abs(res[k] - ref[k]) <= 1e-12, (k, res[k], ref[k])
    name = "per_sample_metrics-normal.csv"
    assert open(os.path.join(out_dir, name)).read() == open(os.path.join(ev_dir, name)).read()
    a, b = (open(os.path.join(d, "eval_metrics-normal.txt")).read().splitlines() for d in (out_dir, ev_dir))
    assert len(a) == len(b) and [x for x in a if "of predictions" not in x] == [x for x in b if "of predictions" not in x]
    assert not os.path.exists(os.path.join(out_dir, os.path.dirname(samples[0][0])))  # nothing saved unless asked for
    # save_predictions writes what run_inference writes
    ie.infer_and_evaluate_normals(FakePipe(), base, samples, output_dir=out_dir, batch_size=2, evaluator=numpy_evaluator, save_predictions=True)
    for s in samples:
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        got = np.load(os.path.join(out_dir, name))
        assert got.ndim == 3 and got.shape[-1] == 3 and np.array_equal(got, np.load(os.path.join(pred_dir, name)))
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_normals(FakePipe(), base, samples, evaluator=numpy_evaluator, save_predictions=True)
    with pytest.raises(ValueError):
        ie.infer_and_evaluate_normals(FakePipe(), base, samples, evaluator=numpy_evaluator, rank=2, world=2)


_WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from genpercept_amd import distributed as gd
from genpercept_amd import infer_eval as ie
import test_infer_eval_normals_host as t
rank, local, world = gd.init_process_group("gloo")
samples = ie.read_filename_list({lst!r})
res = ie.infer_and_evaluate_normals(t.FakePipe(), {base!r}, samples, output_dir={out!r}, batch_size=2, rank=rank, world=world,
                                    evaluator=t.numpy_evaluator)
with open(os.path.join({out!r}, "means_rank%d.json" % rank), "w") as f:
    json.dump(res, f)
dist.barrier()
dist.destroy_process_group()
print("RANK", rank, "OK", flush=True)
"""


def test_infer_and_evaluate_normals_world_size_2_gloo(tmp_path):
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(" ".join(s) for s in samples) + "\n")
    one = ie.infer_and_evaluate_normals(FakePipe(), base, samples, output_dir=str(tmp_path / "w1"), batch_size=2, evaluator=numpy_evaluator)
    out = str(tmp_path / "w2")
    os.makedirs(out)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lst=lst, base=base, out=out))
    port = 31500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 2, r.stdout + r.stderr
    for rank in (0, 1):  # every rank returns the means over ALL samples
        two = json.load(open(os.path.join(out, f"means_rank{rank}.json")))
        for k in one:
            assert abs(two[k] - one[k]) <= 1e-12, (rank, k, two[k], one[k])
    name = "per_sample_metrics-normal.csv"  # rank 0 alone wrote the files, rows in sample order: the table is the one-process table
    assert open(os.path.join(out, name)).read() == open(os.path.join(str(tmp_path / "w1"), name)).read()
    assert len(open(os.path.join(out, name)).read().splitlines()) == 1 + len(samples)
