"""Host tests (no GPU) of the batched, rank-sharded dataset loop: `infer_eval.run_inference(batch_size, rank, world)` and
`infer_eval.infer_and_evaluate` with a fake pipeline and the NumPy evaluator (eval_metrics.evaluate_depth) injected in place of
engine.eval_depth; the world-size-2 combination of the per-image rows runs over gloo in two processes."""
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


def make_tree(base):
    """A ScanNet-style tree (png / 1000, `id` naming): 5 RGB images and depth maps inside (1e-3, 10) with a few invalid (0) pixels."""
    rng = np.random.RandomState(7)
    samples = []
    for i, (h, w) in enumerate(SIZES):
        scene = os.path.join(base, f"scene{i // 3:04d}_00")
        os.makedirs(os.path.join(scene, "color"), exist_ok=True)
        os.makedirs(os.path.join(scene, "depth"), exist_ok=True)
        Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(scene, "color", f"{i:06d}.png"))
        depth = rng.rand(h, w) * 8 + 0.7
        depth[rng.rand(h, w) < 0.1] = 0.0
        Image.fromarray((depth * 1000).astype(np.uint16)).save(os.path.join(scene, "depth", f"{i:06d}.png"))
        samples.append([f"scene{i // 3:04d}_00/color/{i:06d}.png", f"scene{i // 3:04d}_00/depth/{i:06d}.png"])
    return samples


def fake_pred(img):
    """A deterministic [H, W] float32 map in [0, 1] from the RGB image: not an affine image of anything the ground truth holds."""
    a = np.asarray(img.convert("RGB")).astype(np.float32)
    return ((a[..., 0] * 0.5 + a[..., 1] * 0.3 + a[..., 2] * 0.2) / 255.0).astype(np.float32)


class FakePipe:
    def __init__(self):
        self.single, self.batches = 0, []

    def __call__(self, img, **kw):
        assert kw["batch_size"] == 0 and kw["color_map"] is None and kw["mode"] == "depth"
        self.single += 1
        return SimpleNamespace(pred_np=fake_pred(img), pred_colored=None)

    def infer_batch(self, images, mode, **kw):
        assert mode == "depth" and kw["color_map"] is None
        assert len({im.size for im in images}) == 1
        self.batches.append(len(images))
        return [SimpleNamespace(pred_np=fake_pred(im), pred_colored=None) for im in images]

    def predict_batch_device(self, images, mode, **kw):
        assert mode == "depth" and len({im.size for im in images}) == 1
        self.batches.append(len(images))
        return torch.from_numpy(np.stack([fake_pred(im) for im in images]))[:, None]


def numpy_evaluator(pred, gt, mask, alignment, alignment_max_res, min_depth, max_depth):
    from genpercept_amd import eval_metrics as em
    return [em.evaluate_depth(p.numpy(), g.numpy(), m.numpy(), min_depth, max_depth, alignment=alignment, alignment_max_res=alignment_max_res)
            for p, g, m in zip(pred, gt, mask)], None


def rel(paths, root):
    return [os.path.relpath(p, root) for p in paths]


def test_run_inference_batched_groups_and_files(tmp_path):
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    one, bat = FakePipe(), FakePipe()
    w1 = ie.run_inference(one, base, samples, str(tmp_path / "p1"), ie.FileNameMode.id, mode="depth")
    assert one.single == 5 and one.batches == []
    for prefetch in (2, 0):
        bat.batches = []
        out = str(tmp_path / f"pb{prefetch}")
        wb = ie.run_inference(bat, base, samples, out, ie.FileNameMode.id, mode="depth", batch_size=3, prefetch=prefetch)
        assert bat.batches == [3, 1, 1] and bat.single == 0
        assert rel(wb, out) == rel(w1, str(tmp_path / "p1")) == [os.path.join(os.path.dirname(s[0]), "pred_" + os.path.basename(s[0])[:-4] + ".npy")
                                                                  for s in samples]
        for a, b in zip(w1, wb):
            assert np.array_equal(np.load(a), np.load(b))
    # a group never exceeds batch_size
    bat.batches = []
    ie.run_inference(bat, base, samples, str(tmp_path / "pb2"), ie.FileNameMode.id, mode="depth", batch_size=2)
    assert bat.batches == [2, 1, 1, 1]


@pytest.mark.parametrize("batch_size", [1, 3])
def test_run_inference_shards_are_disjoint_and_complete(tmp_path, batch_size):
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    full = rel(ie.run_inference(FakePipe(), base, samples, str(tmp_path / "all"), ie.FileNameMode.id), str(tmp_path / "all"))
    parts = []
    for rank in (0, 1):
        out = str(tmp_path / f"r{rank}")
        # an entry without ground truth is dropped BEFORE the list is sharded (kitti_dataset.py:47)
        with_none = samples[:1] + [["x.png", "None"]] + samples[1:]
        parts.append(rel(ie.run_inference(FakePipe(), base, with_none, out, ie.FileNameMode.id, batch_size=batch_size, rank=rank, world=2), out))
    assert parts[0] == full[:3] and parts[1] == full[3:]
    assert not set(parts[0]) & set(parts[1]) and sorted(parts[0] + parts[1]) == sorted(full)
    with pytest.raises(ValueError):
        ie.run_inference(FakePipe(), base, samples, str(tmp_path / "bad"), ie.FileNameMode.id, rank=2, world=2)


def test_infer_and_evaluate_equals_files_then_evaluate(tmp_path):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    pred_dir, ev_dir, out_dir = str(tmp_path / "pred"), str(tmp_path / "eval_ref"), str(tmp_path / "eval_dev")
    ie.run_inference(FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="depth")
    for alignment, max_res in (("least_square", None), ("least_square_disparity", None), ("least_square", 16)):
        ref = ie.evaluate_predictions(pred_dir, base, samples, dataset="scannet", alignment=alignment, alignment_max_res=max_res, output_dir=ev_dir)
        pipe = FakePipe()
        res = ie.infer_and_evaluate(pipe, base, samples, "scannet", output_dir=out_dir, batch_size=3, alignment=alignment, alignment_max_res=max_res,
                                    evaluator=numpy_evaluator)
        assert pipe.batches == [3, 1, 1]
        assert list(res) == list(em.METRICS)
        for k in ref:
            assert abs(res[k] - ref[k]) <= 1e-12, (alignment, k, res[k], ref[k])
        for name in (f"eval_metrics-{alignment}.txt", f"per_sample_metrics-{alignment}.csv"):
            assert os.path.exists(os.path.join(out_dir, name))
        # same per-sample table (file names, order, values) and the same summary apart from the line that names the prediction directory
        assert open(os.path.join(out_dir, f"per_sample_metrics-{alignment}.csv")).read() == open(os.path.join(ev_dir, f"per_sample_metrics-{alignment}.csv")).read()
        a, b = (open(os.path.join(d, f"eval_metrics-{alignment}.txt")).read().splitlines() for d in (out_dir, ev_dir))
        assert len(a) == len(b) and [x for x in a if "of predictions" not in x] == [x for x in b if "of predictions" not in x]
        assert not os.path.exists(os.path.join(out_dir, os.path.dirname(samples[0][0])))  # nothing saved unless asked for
    # save_predictions writes what run_inference writes
    ie.infer_and_evaluate(FakePipe(), base, samples, "scannet", output_dir=out_dir, batch_size=2, evaluator=numpy_evaluator, save_predictions=True)
    for s in samples:
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        assert np.array_equal(np.load(os.path.join(out_dir, name)), np.load(os.path.join(pred_dir, name)))
    with pytest.raises(ValueError):
        ie.infer_and_evaluate(FakePipe(), base, samples, "scannet", evaluator=numpy_evaluator, save_predictions=True)


_WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from genpercept_amd import distributed as gd
from genpercept_amd import infer_eval as ie
import test_infer_eval_batched_host as t
rank, local, world = gd.init_process_group("gloo")
samples = ie.read_filename_list({lst!r})
res = ie.infer_and_evaluate(t.FakePipe(), {base!r}, samples, "scannet", output_dir={out!r}, batch_size=2, rank=rank, world=world,
                            evaluator=t.numpy_evaluator)
with open(os.path.join({out!r}, "means_rank%d.json" % rank), "w") as f:
    json.dump(res, f)
dist.barrier()
dist.destroy_process_group()
print("RANK", rank, "OK", flush=True)
"""


def test_infer_and_evaluate_world_size_2_gloo(tmp_path):
    import json
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = make_tree(base)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(" ".join(s) for s in samples) + "\n")
    one = ie.infer_and_evaluate(FakePipe(), base, samples, "scannet", output_dir=str(tmp_path / "w1"), batch_size=2, evaluator=numpy_evaluator)
    out = str(tmp_path / "w2")
    os.makedirs(out)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lst=lst, base=base, out=out))
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 2, r.stdout + r.stderr
    for rank in (0, 1):  # every rank returns the means over ALL samples
        two = json.load(open(os.path.join(out, f"means_rank{rank}.json")))
        for k in one:
            assert abs(two[k] - one[k]) <= 1e-12, (rank, k, two[k], one[k])
    # rank 0 alone wrote the files, rows in sample order: the table is the one-process table
    name = "per_sample_metrics-least_square.csv"
    assert open(os.path.join(out, name)).read() == open(os.path.join(str(tmp_path / "w1"), name)).read()
    assert len(open(os.path.join(out, name)).read().splitlines()) == 1 + len(samples)
