"""CPU tests of the host side: the C-ABI library loads and exports every declared symbol, config inference, pre/post
processing, pipeline argument validation, sharding, and the world-size-2 gather over gloo."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    assert declared == set(engine.SYMBOLS), declared ^ set(engine.SYMBOLS)
    for prec, code in (("fp16", 1), ("bf16", 2)):  # both element-type builds carry the whole C-ABI
        lib = engine.load_library(prec)
        for name in declared:
            assert hasattr(lib, name), (prec, name)
        assert lib.gp_version().startswith(b"genpercept_hip") and prec.encode() in lib.gp_version()
        assert lib.gp_element_dtype() == code
    assert lib.gp_packed_rows(320) == 512 and lib.gp_latent_size(768) == 96 and lib.gp_latent_size(511) == 63
    assert lib.gp_dpt_out_size(96) == 768 and lib.gp_dpt_out_size(9) == 96


def test_abi_version_and_precision_entry_points():
    """GP_ABI_VERSION of the header == gp_abi_version() of both libraries (the r5 removal of gp_timings.sat_events is version 3);
    gp_set_precision argument handling needs no GPU; torch dtypes map to engine precisions the way run.py:273-281 asks (fp32 = the contract precision)."""
    import ctypes as C
    from genpercept_amd import engine
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    ver = int(re.search(r"#define GP_ABI_VERSION (\d+)", hdr).group(1))
    assert ver >= 3
    for prec in ("bf16", "fp16"):
        lib = engine.load_library(prec)
        assert lib.gp_abi_version() == ver
        assert lib.gp_set_precision(None, 1) == 1 and lib.gp_get_precision(None) == 0  # GP_ERR_INVALID on a null engine; native by default
    assert C.sizeof(engine.GpTimings) == 72  # the frozen layout of ABI version 3 (no trailing sat_events)
    assert engine.precision_of(torch.float32) == "fp32c" and engine.precision_of(torch.float16) == "fp16"
    assert engine.precision_of(torch.bfloat16) == "bf16" and engine.precision_of(None) == "bf16"
    assert engine.ENGINE_PRECISIONS["fp32c"] == ("bf16", 1)
    with pytest.raises(ValueError):
        engine.precision_of(torch.int8)
    from genpercept_amd import GenPerceptPipeline
    pipe = GenPerceptPipeline(unet={}, vae={}, text_encoder=np.zeros((2, 1024), np.float32), torch_dtype=torch.float32)
    assert pipe._precision == "fp32c" and pipe.dtype == torch.float32
    assert pipe.to(dtype=torch.float16)._precision == "fp16" and pipe.dtype == torch.float16


def test_library_contains_gfx950_code_objects():
    from genpercept_amd import engine
    for path in engine.LIB_PATHS.values():
        blob = open(path, "rb").read()
        assert b"gfx950" in blob and b"igemm_kernel" in blob and b"flash_attn64_kernel" in blob and b"flash_attn64_split_kernel" in blob and b"c_gn_apply_split_kernel" in blob


def test_default_config_is_sd21():
    import ctypes as C
    from genpercept_amd import engine
    lib = engine.load_library()
    cfg = engine.GpConfig()
    lib.gp_default_config(C.byref(cfg))
    assert list(cfg.unet_block_out) == [320, 640, 1280, 1280] and list(cfg.unet_num_heads) == [5, 10, 20, 20]
    assert list(cfg.vae_block_out) == [128, 256, 512, 512] and abs(cfg.vae_scaling_factor - 0.18215) < 1e-7
    assert abs(cfg.unet_norm_eps - 1e-5) < 1e-12 and abs(cfg.vae_norm_eps - 1e-6) < 1e-12


def test_engine_requires_gpu_no_fallback():
    from genpercept_amd.engine import Engine
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        Engine(0)


def test_config_inference_from_state_dict_shapes():
    from genpercept_amd import config as gc
    from oracle import dpt as odpt
    from oracle import sd21 as osd
    meta = lambda m: {k: torch.empty(s, device="meta") for k, s in m.items()}  # noqa: E731
    u = gc.infer_unet_config(meta(osd.unet_manifest()))
    assert u.block_out_channels == (320, 640, 1280, 1280) and u.num_heads == (5, 10, 20, 20) and u.cross_attention_dim == 1024
    assert u.down_has_attn == (True, True, True, False) and u.layers_per_block == 2 and u.has_out
    ut = gc.infer_unet_config(meta(osd.unet_manifest(osd.UNetCfg.tiny())))
    assert ut.block_out_channels == (64, 128, 256, 256) and ut.cross_attention_dim == 64
    v = gc.infer_vae_config(meta(osd.vae_manifest()))
    assert v.block_out_channels == (128, 256, 512, 512) and v.layers_per_block == 2 and v.latent_channels == 4
    dec_only = {k: t for k, t in meta(osd.vae_manifest()).items() if not k.startswith("encoder")}
    assert gc.infer_vae_config(dec_only).block_out_channels == (128, 256, 512, 512)
    d = gc.infer_dpt_config(meta(odpt.dpt_manifest()))
    assert d.neck_hidden_sizes == (320, 640, 1280, 1280) and d.fusion_hidden_size == 256
    with pytest.raises(KeyError):
        gc.infer_unet_config({})


def test_resize_semantics():
    from genpercept_amd import image_util as iu
    img = torch.randint(0, 256, (1, 3, 480, 640), dtype=torch.uint8)
    out = iu.resize_max_res(img, 768, "bilinear")
    assert out.shape == (1, 3, 576, 768) and out.dtype == torch.uint8  # int() truncation of 480 * 1.2
    assert iu.resize_max_res(torch.zeros(1, 3, 333, 500, dtype=torch.uint8), 768).shape == (1, 3, int(333 * 768 / 500), 768)
    same = iu.resize_to(img, (480, 640), "bilinear")
    assert same is img
    with pytest.raises(ValueError):
        iu.get_resample_method("lanczos")
    assert iu.get_resample_method("nearest") == "nearest-exact"
    col = iu.colorize_depth_maps(np.linspace(0, 1, 12, dtype=np.float32).reshape(3, 4), 0, 1)
    assert col.shape == (1, 3, 3, 4) and col.min() >= 0 and col.max() <= 1


def test_pipeline_validation_without_gpu():
    from genpercept_amd import GenPerceptPipeline

    class BadSched:
        beta_start, beta_end, prediction_type = 0.00085, 0.012, "v_prediction"

    # any DDIM config is accepted (one step with a beta != 1 scheduler runs the engine's denoising loop); only beta == 1 + v_prediction
    # without clipping is the closed form x0 = -v
    assert not GenPerceptPipeline(unet={}, vae={}, scheduler=BadSched())._x0_is_neg_v
    with pytest.raises(ValueError):
        GenPerceptPipeline(unet={}, vae={}, genpercept_pipeline=False)  # the multi-step archs need their scheduler
    multi = GenPerceptPipeline(unet={}, vae={}, scheduler=BadSched(), genpercept_pipeline=False, rgb_blending=True)
    assert multi.default_denoising_steps == 10 and multi.rgb_blending and not multi.genpercept_pipeline
    with pytest.raises(AssertionError):  # genpercept_pipeline.py:141-143: a customised head needs the one-step beta == 1 pipeline
        GenPerceptPipeline(unet={}, vae={}, scheduler=BadSched(), customized_head={"neck.x": torch.zeros(1)}, head_type="identity")
    class Lcm:
        _class_name, beta_start, beta_end = "LCMScheduler", 0.00085, 0.012
    with pytest.raises(NotImplementedError):
        GenPerceptPipeline(unet={}, vae={}, scheduler=Lcm())
    pipe = GenPerceptPipeline(unet={}, vae={}, scheduler={"beta_start": 1.0, "beta_end": 1.0, "prediction_type": "v_prediction", "clip_sample": False},
                              text_encoder=np.zeros((2, 1024), np.float32), default_denoising_steps=10)
    assert pipe.default_denoising_steps == 1 and pipe.rgb_blending and pipe.latent_scale_factor == 0.18215
    assert pipe.text_embed.shape == (1, 2, 1024) and pipe.dtype == torch.bfloat16
    with pytest.raises(AssertionError):
        pipe(torch.zeros(1, 3, 8, 8))  # mode missing
    with pytest.raises(AssertionError):
        pipe(torch.zeros(3, 8, 8), mode="depth")  # wrong rank
    with pytest.raises(RuntimeError):
        pipe.to("cpu")


def test_v1_empty_text_embed_fixture_shape():
    """The only fixture-like artefact of the reference (GenPercept_v1/empty_text_embed.npy) is [77,1024] fp16; rows [0:2]
    are what the v2 pipeline's do_not_pad tokenisation yields.  tests/golden/refexec_v1_tiny.npz stores it whole (`embed_77`, written
    by make_goldens.py from that file) beside the rows [0:2] it was run with."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "refexec_v1_tiny.npz"))
    e = g["embed_77"]
    assert e.shape == (77, 1024) and e.dtype == np.float16
    assert np.array_equal(g["embed_rows_0_2"], e[:2]) and np.isfinite(e).all()


def test_shard_range_partitions_the_batch():
    from genpercept_amd.distributed import shard_range
    for n, w in [(64, 8), (10, 4), (3, 8), (7, 2), (1, 1)]:
        spans = [shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1
    assert shard_range(64, 3, 8) == (24, 32)


_WORKER = r"""
import os, sys, torch
sys.path.insert(0, {root!r})
from genpercept_amd import distributed as gd
rank, local, world = gd.init_process_group("gloo")
n_total = 5
lo, hi = gd.shard_range(n_total, rank, world)
local_out = torch.stack([torch.full((1, 4, 6), float(i)) for i in range(lo, hi)]) if hi > lo else torch.zeros((0, 1, 4, 6))
gd.barrier()
full = gd.gather_results(local_out, n_total, dst=0)
allf = gd.gather_results(local_out, n_total, dst=None)
ok = allf.shape == (n_total, 1, 4, 6) and all(float(allf[i].mean()) == i for i in range(n_total))
if rank == 0:
    ok = ok and full.shape == (n_total, 1, 4, 6) and all(float(full[i].mean()) == i for i in range(n_total))
else:
    ok = ok and full is None
# second call with other values: the preallocated buffers are reused (same storage on the receiving rank), the values are the new ones
full2 = gd.gather_results(local_out + 10.0, n_total, dst=0)
if rank == 0:
    ok = ok and full2.data_ptr() == full.data_ptr() and all(float(full2[i].mean()) == i + 10.0 for i in range(n_total))
# equal shards: the receive buffer is the result (a view, no compaction copy)
eq = gd.gather_results(torch.full((2, 1, 4, 6), float(rank)), 2 * world, dst=None)
ok = ok and eq.shape[0] == 2 * world and all(float(eq[2 * r].mean()) == r and float(eq[2 * r + 1].mean()) == r for r in range(world))
ok = ok and len(gd._gatherers) == 3 and not gd._gatherers[((1, 4, 6), torch.float32, "cpu", 2 * world, None, world, rank)].ragged
# clone=True: the caller's copy survives the next call with the same key (ADVICE r5: the default result is a view of the reused buffer)
keep = gd.gather_results(local_out, n_total, dst=None, clone=True)
again = gd.gather_results(local_out + 3.0, n_total, dst=None)
ok = ok and keep.data_ptr() != again.data_ptr() and all(float(keep[i].mean()) == i for i in range(n_total)) and float(again[0].mean()) == 3.0
# a key built for another process group (world size / rank) is never reused: simulate a stale entry and check it is dropped
gd._gatherers[((9,), torch.float32, "cpu", 1, None, world + 1, rank)] = object()
_ = gd.gather_results(torch.full((1, 2, 2, 2), 1.0), world, dst=None)
ok = ok and not any(k[5] != world for k in gd._gatherers)
mx = gd.max_over_ranks(float(rank + 1), torch.device("cpu"))
ok = ok and mx == float(world)
print("RANK", rank, "OK" if ok else "FAIL", flush=True)
sys.exit(0 if ok else 1)
"""


def test_gather_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 2, r.stdout + r.stderr


def test_product_manifests_equal_oracle_manifests_and_public_counts():
    from genpercept_amd import config as gc
    from genpercept_amd import weights as gw
    from oracle import dpt as odpt
    from oracle import sd21 as osd
    assert list(gw.unet_manifest().items()) == list(osd.unet_manifest().items())
    assert list(gw.vae_manifest().items()) == list(osd.vae_manifest().items())
    assert list(gw.dpt_manifest().items()) == list(odpt.dpt_manifest().items())
    assert gw.count_params(gw.unet_manifest()) == 865_910_724 and gw.count_params(gw.vae_manifest()) == 83_653_863
    assert gw.count_params(gw.dpt_manifest()) == 18_474_753
    tu = gc.UNetConfig(block_out_channels=(64, 128, 256, 256), num_heads=(1, 2, 4, 4), cross_attention_dim=64)
    assert list(gw.unet_manifest(tu).items()) == list(osd.unet_manifest(osd.UNetCfg.tiny()).items())
    nohead = gc.UNetConfig(has_out=False)
    assert "conv_out.weight" not in gw.unet_manifest(nohead) and len(gw.unet_manifest(nohead)) == 682
    a, b = gw.synth_state_dict(gw.unet_manifest(tu), 1), osd.synth_state_dict(osd.unet_manifest(osd.UNetCfg.tiny()), 1)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_find_batch_size_clamp_matches_reference():
    """genpercept_amd.batchsize mirrors the reference's find_batch_size (genpercept/util/batchsize.py:51-81): given the batch
    that fits, the clamp against the ensemble size must reproduce the reference's answers (tests/golden/batchsize_ref.npz);
    the hot path (ensemble_size == 1) always gets 1, as does a host without a GPU."""
    import numpy as np
    from genpercept_amd import batchsize as bsz
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batchsize_ref.npz"))
    assert int(g["no_gpu"]) == 1
    n_checked = 0
    for vram, res, dt, ens, bs_table, bs_ret in g["rows"]:
        if bs_table == 1 and bs_ret == 1:
            # either the table's bs is 1 or nothing fitted (the reference returns 1 both ways): only the ensemble-1 rule is checkable
            assert bsz.clamp_batch_size(1, int(ens)) == 1 if ens == 1 else True
            continue
        assert bsz.clamp_batch_size(int(bs_table), int(ens)) == int(bs_ret), (vram, res, dt, ens, bs_table, bs_ret)
        n_checked += 1
    assert n_checked > 100
    for ens in (1, 2, 10):
        for res in (384, 768, 1024):
            b = bsz.find_batch_size(ens, res, torch.bfloat16, total_vram_gb=288.0)
            assert 1 <= b <= ens
    assert bsz.find_batch_size(1, 768, torch.bfloat16, total_vram_gb=288.0) == 1
    assert bsz.find_batch_size(10, 768, None, total_vram_gb=1.0) == 1          # nothing fits -> 1
    assert bsz.find_batch_size(64, 768, None, total_vram_gb=288.0) in (32, 64)  # 288 GB: the whole ensemble or its half


def test_infer_eval_driver_matches_reference(tmp_path):
    """genpercept_amd.infer_eval against outputs of the reference's own functions (tests/golden/infer_eval_ref.npz):
    get_pred_name for every naming mode, least-squares alignment with max_resolution, the disparity-space protocol; then the
    inference loop + evaluation on a synthetic NYU-style tree with a stand-in pipeline (file layout, masks, metric reduction)."""
    import numpy as np
    from PIL import Image
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "infer_eval_ref.npz"))
    n = 0
    for key, want in zip(g["name_keys"], g["name_vals"]):
        mode, bn, suf = str(key).split("|")
        try:
            got = ie.get_pred_name(bn, ie.FileNameMode[mode], suffix=suf)
        except Exception as e:
            got = "!" + type(e).__name__
        assert got == str(want), (key, got, want)
        n += 1
    assert n == 56
    gt, pred, mask = g["gt"], g["pred"], g["mask"]
    for mr in (32, 64, 200):
        a, s, t = em.align_depth_least_square(gt, pred, mask, max_resolution=mr)
        np.testing.assert_allclose([s, t], g[f"align_maxres{mr}_st"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(a, g[f"align_maxres{mr}"], rtol=1e-5, atol=1e-5)
    # disparity-space protocol (eval.py:181-200) through evaluate_depth's internals
    gdisp, gpos = em.depth2disparity(gt)
    pd = g["pred_disp"]
    m = mask & gpos & (pd > 0)
    d, _, _ = em.align_depth_least_square(gdisp, pd, m)
    depth, _ = em.disparity2depth(np.clip(d, 1e-3, None))
    np.testing.assert_allclose(depth, g["disp_protocol_depth"], rtol=1e-4, atol=1e-5)

    # end to end on a synthetic NYU-style tree
    base, outd = tmp_path / "data", tmp_path / "pred"
    rng = np.random.RandomState(0)
    samples = []
    for i in range(3):
        scene = base / "test" / f"room_{i:04d}"
        scene.mkdir(parents=True)
        depth_m = (rng.rand(480, 640) * 8 + 0.7).astype(np.float32)
        Image.fromarray((depth_m * 1000).astype(np.uint16)).save(scene / f"depth_{i:04d}.png")
        Image.fromarray(rng.randint(0, 255, (480, 640, 3), dtype=np.uint8)).save(scene / f"rgb_{i:04d}.png")
        samples.append([f"test/room_{i:04d}/rgb_{i:04d}.png", f"test/room_{i:04d}/depth_{i:04d}.png"])
    (base / "list.txt").write_text("\n".join(" ".join(s) for s in samples) + "\n")
    assert ie.read_filename_list(str(base / "list.txt")) == samples

    class FakePipe:  # affine-invariant prediction: a scaled/shifted copy of the GT (what the LS alignment undoes)
        def __call__(self, img, **kw):
            assert kw["batch_size"] == 0 and kw["color_map"] is None and kw["mode"] == "depth"
            idx = FakePipe.i
            FakePipe.i += 1
            d = np.asarray(Image.open(base / samples[idx][1])).astype(np.float32) / 1000.0
            from types import SimpleNamespace
            return SimpleNamespace(pred_np=(0.1 * d + 0.05).astype(np.float32), pred_colored=None)
    FakePipe.i = 0
    written = ie.run_inference(FakePipe(), str(base), samples, str(outd), ie.FileNameMode.rgb_id, mode="depth")
    assert [os.path.relpath(w, outd) for w in written] == [f"test/room_{i:04d}/pred_{i:04d}.npy" for i in range(3)]
    # the decode-ahead / write-behind threads change neither order nor results (prefetch = 0 is the plain loop)
    FakePipe.i = 0
    outd0 = tmp_path / "pred_serial"
    written0 = ie.run_inference(FakePipe(), str(base), samples, str(outd0), ie.FileNameMode.rgb_id, mode="depth", prefetch=0)
    assert [os.path.relpath(w, outd0) for w in written0] == [os.path.relpath(w, outd) for w in written]
    for a, b in zip(written, written0):
        assert np.array_equal(np.load(a), np.load(b))
    FakePipe.i = 0
    with pytest.raises(FileNotFoundError):  # a missing image surfaces as the loader's exception, not as a hang
        ie.run_inference(FakePipe(), str(base), samples[:1] + [["test/none.png", "x"]] + samples[1:], str(tmp_path / "pred_bad"), ie.FileNameMode.rgb_id)
    res = ie.evaluate_predictions(str(outd), str(base), samples, dataset="nyu", alignment="least_square", output_dir=str(tmp_path / "eval"))
    assert res["abs_relative_difference"] < 1e-3 and res["delta1_acc"] > 0.999
    assert os.path.exists(tmp_path / "eval" / "eval_metrics-least_square.txt")
    vm = ie.valid_mask_of(np.full((480, 640), 5.0, np.float32), 1e-3, 10.0, ie.DATASETS["nyu"]["eval_crop"])
    assert vm.sum() == (471 - 45) * (601 - 41) and not vm[44, 100] and vm[45, 41] and not vm[470, 601]


def test_lora_adapters_are_merged_into_base_weights():
    """run.py:345-357: a PEFT-wrapped UNet checkpoint (base_layer / lora_A / lora_B keys, alpha = r) must load as W + B @ A."""
    from genpercept_amd.weights import merge_lora_state_dict
    g = torch.Generator().manual_seed(0)
    r, cin, cout = 8, 64, 96
    base = torch.randn(cout, cin, generator=g)
    a = torch.randn(r, cin, generator=g) * 0.1
    b = torch.randn(cout, r, generator=g) * 0.1
    plain = {"blk.attn1.to_k.weight": torch.randn(cout, cin, generator=g), "blk.norm.weight": torch.ones(cin)}
    assert merge_lora_state_dict(plain) is plain
    sd = {"blk.attn1.to_q.base_layer.weight": base, "blk.attn1.to_q.lora_A.default.weight": a, "blk.attn1.to_q.lora_B.default.weight": b,
          "blk.attn1.to_out.0.base_layer.weight": base.clone(), "blk.attn1.to_out.0.base_layer.bias": torch.zeros(cout),
          "blk.attn1.to_out.0.lora_A.default.weight": a, "blk.attn1.to_out.0.lora_B.default.weight": b, **plain}
    m = merge_lora_state_dict(sd)
    assert set(m) == {"blk.attn1.to_q.weight", "blk.attn1.to_out.0.weight", "blk.attn1.to_out.0.bias", "blk.attn1.to_k.weight", "blk.norm.weight"}
    x = torch.randn(5, cin, generator=g)
    want = x @ base.t() + (x @ a.t()) @ b.t()          # what the PEFT module computes with alpha / r = 1
    torch.testing.assert_close(x @ m["blk.attn1.to_q.weight"].t(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(merge_lora_state_dict(sd, scale=0.5)["blk.attn1.to_q.weight"], base + 0.5 * b @ a)


def test_image_util_matches_reference():
    """Host pre/post processing against outputs of the reference's genpercept/util/image_util.py
    (tests/golden/image_util_ref.npz): Spectral colouring incl. clipping, CHW->HWC, resize_max_res's truncating size rule, method names."""
    import numpy as np
    from genpercept_amd import image_util as iu
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "image_util_ref.npz"))
    np.testing.assert_allclose(iu.colorize_depth_maps(g["depth"], 0, 1, cmap="Spectral"), g["colored_spectral"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(iu.colorize_depth_maps(g["depth"][0], 0.1, 0.9, cmap="Spectral"), g["colored_single"], rtol=0, atol=1e-7)
    np.testing.assert_array_equal(iu.chw2hwc(g["chw"]), g["hwc"])
    for h, w, mr, nh, nw in g["resize_sizes"]:
        out = iu.resize_max_res(torch.zeros(1, 3, int(h), int(w), dtype=torch.uint8), int(mr))
        assert tuple(out.shape[-2:]) == (int(nh), int(nw)), (h, w, mr, out.shape, nh, nw)
    for name, want in zip(g["resample_keys"], g["resample_vals"]):
        try:
            got = iu.get_resample_method(str(name))
        except ValueError:
            got = "!ValueError"
        assert got == str(want), (name, got, want)


def test_genpercept_import_path_shim():
    """`from genpercept import GenPerceptPipeline` (run.py:33, infer.py:30) resolves to this engine's pipeline."""
    import genpercept
    import genpercept.genpercept_pipeline as gpp
    from genpercept_amd.pipeline import GenPerceptOutput, GenPerceptPipeline
    assert genpercept.GenPerceptPipeline is GenPerceptPipeline and genpercept.GenPerceptOutput is GenPerceptOutput
    assert gpp.GenPerceptPipeline is GenPerceptPipeline
    assert GenPerceptPipeline.latent_scale_factor == 0.18215


def _fake_reference_checkout(root):
    """A stand-in for a GenPercept checkout: the package layout run.py / infer.py import from (genpercept/__init__.py:18,
    genpercept/models/{dpt_head,custom_unet}.py, genpercept/util/), with marker classes instead of the reference's diffusers wrappers."""
    pkg = root / "genpercept"
    (pkg / "models").mkdir(parents=True)
    (pkg / "util").mkdir()
    (pkg / "__init__.py").write_text("REFERENCE_PACKAGE = True\nfrom .genpercept_pipeline import GenPerceptPipeline, GenPerceptOutput\n")
    (pkg / "genpercept_pipeline.py").write_text("class GenPerceptPipeline:\n    ORIGIN = 'reference'\nclass GenPerceptOutput:\n    pass\n")
    (pkg / "models" / "dpt_head.py").write_text(
        "class DPTNeckHeadForUnetAfterUpsample:\n    ORIGIN = 'reference'\n"
        "class DPTNeckHeadForUnetAfterUpsampleIdentity(DPTNeckHeadForUnetAfterUpsample):\n    pass\n")
    (pkg / "models" / "custom_unet.py").write_text("class CustomUNet2DConditionModel:\n    ORIGIN = 'reference'\n")
    (pkg / "util" / "batchsize.py").write_text("ORIGIN = 'reference'\n")
    # run.py:33,49,51 / infer.py:30,46,48 -- the three import lines, in the reference's order, then what it does with the names
    (root / "run.py").write_text(
        "import sys\n"
        "from genpercept import GenPerceptPipeline\n"
        "from genpercept.models.dpt_head import DPTNeckHeadForUnetAfterUpsample, DPTNeckHeadForUnetAfterUpsampleIdentity\n"
        "from genpercept.models.custom_unet import CustomUNet2DConditionModel\n"
        "import genpercept, genpercept.genpercept_pipeline as gpp\n"
        "from genpercept.util import batchsize\n"
        "assert not hasattr(genpercept, 'REFERENCE_PACKAGE'), 'the reference package shadows the shim'\n"
        "assert GenPerceptPipeline.__module__ == 'genpercept_amd.pipeline', GenPerceptPipeline.__module__\n"
        "assert gpp.GenPerceptPipeline is GenPerceptPipeline\n"
        "assert DPTNeckHeadForUnetAfterUpsampleIdentity.ORIGIN == CustomUNet2DConditionModel.ORIGIN == batchsize.ORIGIN == 'reference'\n"
        "print('DROPIN-OK', sys.argv[1:])\n")
    return root


def test_run_py_import_lines_resolve_with_the_shim_on_the_path(tmp_path):
    """VERDICT r3 missing #2: run.py:33,49,51 (infer.py:30,46,48) import `genpercept`, `genpercept.models.dpt_head` and
    `genpercept.models.custom_unet` at module top.  With this repository ahead of a reference checkout on sys.path the first must be the
    engine's pipeline and the other two must still resolve to the checkout's files (the shim extends its __path__)."""
    ref = _fake_reference_checkout(tmp_path / "GenPercept")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}]; sys.path.append({str(ref)!r})\n" + (ref / "run.py").read_text())
    r = subprocess.run([sys.executable, "-c", code, "--mode", "depth"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "DROPIN-OK ['--mode', 'depth']" in r.stdout, r.stdout + r.stderr
    # the checkout appended AFTER the shim was imported is still found (the path is rescanned per sub-module import)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}]\nimport genpercept\nsys.path.append({str(ref)!r})\n"
            "from genpercept.models.custom_unet import CustomUNet2DConditionModel as C\nassert C.ORIGIN == 'reference'\n"
            "import genpercept.genpercept_pipeline as g\nassert g.GenPerceptPipeline.__module__ == 'genpercept_amd.pipeline'\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    # without a checkout on the path the model modules are absent, loudly
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path[:0] = [{ROOT!r}]\nimport genpercept.models.dpt_head"],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "ModuleNotFoundError" in r.stderr


def test_dropin_launcher_runs_a_reference_script_unchanged(tmp_path):
    """`python run.py` puts the checkout's directory at sys.path[0] (the reference's own package would win); `python -m
    genpercept_amd.dropin <checkout>/run.py args` orders the path [this repository, checkout, ...] and runs the script as __main__."""
    ref = _fake_reference_checkout(tmp_path / "GenPercept")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, str(ref / "run.py")], capture_output=True, text=True, env=env, cwd=str(ref))
    assert r.returncode != 0 and "shadows the shim" in r.stderr  # the problem the launcher exists for
    r = subprocess.run([sys.executable, "-m", "genpercept_amd.dropin", str(ref / "run.py"), "--checkpoint", "ckpt"],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and "DROPIN-OK ['--checkpoint', 'ckpt']" in r.stdout, r.stdout + r.stderr
    from genpercept_amd import dropin
    order = dropin.path_order(str(ref / "run.py"), path=["", str(ref), "/x", ROOT])
    assert order[:2] == [ROOT, str(ref)] and order.count(ROOT) == 1 and order.count(str(ref)) == 1


def test_customized_head_kind_like_the_reference():
    """genpercept_pipeline.py:474,483-484: only DPTNeckHeadForUnetAfterUpsampleIdentity is a valid customized_head; the ReLU-terminated
    DPTNeckHeadForUnetAfterUpsample (same keys! run.py:303-307 loads it from `dpt_head/`) raises ValueError."""
    from genpercept_amd.pipeline import GenPerceptPipeline

    class DPTNeckHeadForUnetAfterUpsample:  # stands in for the reference module: only the class name and state_dict() matter
        def state_dict(self):
            return {"neck.fusion_stage.layers.0.projection.weight": torch.zeros(1)}

    class DPTNeckHeadForUnetAfterUpsampleIdentity(DPTNeckHeadForUnetAfterUpsample):
        pass

    sched = dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False)
    with pytest.raises(ValueError):
        GenPerceptPipeline(unet={}, vae={}, scheduler=sched, customized_head=DPTNeckHeadForUnetAfterUpsample())
    with pytest.raises(ValueError):
        GenPerceptPipeline(unet={}, vae={}, scheduler=sched, customized_head="/ckpt/run1/dpt_head")
    with pytest.raises(ValueError):
        GenPerceptPipeline(unet={}, vae={}, scheduler=sched, customized_head={"neck.x": torch.zeros(1)}, head_type="relu")
    for head, kw in ((DPTNeckHeadForUnetAfterUpsampleIdentity(), {}), ("/ckpt/run1/dpt_head_identity", {}), ({"neck.x": torch.zeros(1)}, {"head_type": "identity"})):
        p = GenPerceptPipeline(unet={}, vae={}, scheduler=sched, customized_head=head, **kw)
        assert p._head_kind == "identity"
    assert GenPerceptPipeline(unet={}, vae={}, scheduler=sched, customized_head={"neck.x": torch.zeros(1)})._head_kind is None


def test_finetuned_vae_decoder_directories(tmp_path):
    """run.py:308-312: vae_decoder/model.safetensors (keys without the `decoder.` prefix) + vae_post_quant_conv/model.safetensors are
    composed over the base VAE; from_pretrained(load_decoder_ckpt=...) does it by path."""
    from safetensors.torch import save_file
    from genpercept_amd import config as gc
    from genpercept_amd import weights as gw
    from genpercept_amd.pipeline import GenPerceptPipeline, compose_finetuned_vae
    vc = gc.VAEConfig(block_out_channels=(64, 64, 64, 64))
    base = gw.synth_state_dict(gw.vae_manifest(vc), seed=4)
    tuned = gw.synth_state_dict(gw.vae_manifest(vc), seed=5)
    (tmp_path / "sd" / "vae").mkdir(parents=True)
    (tmp_path / "ft" / "vae_decoder").mkdir(parents=True)
    (tmp_path / "ft" / "vae_post_quant_conv").mkdir(parents=True)
    save_file(dict(base), str(tmp_path / "sd" / "vae" / "diffusion_pytorch_model.safetensors"))
    save_file({k[len("decoder."):]: v for k, v in tuned.items() if k.startswith("decoder.")}, str(tmp_path / "ft" / "vae_decoder" / "model.safetensors"))
    save_file({k[len("post_quant_conv."):]: v for k, v in tuned.items() if k.startswith("post_quant_conv.")},
              str(tmp_path / "ft" / "vae_post_quant_conv" / "model.safetensors"))
    sd = compose_finetuned_vae(str(tmp_path / "sd" / "vae"), str(tmp_path / "ft"))
    assert set(sd) == set(base)
    for k in sd:
        src = tuned if k.startswith(("decoder.", "post_quant_conv.")) else base
        assert torch.equal(sd[k], src[k]), k
    pipe = GenPerceptPipeline.from_pretrained(str(tmp_path / "sd"), unet={}, load_decoder_ckpt=str(tmp_path / "ft"),
                                              scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False))
    assert torch.equal(pipe._vae_src["decoder.conv_in.weight"], tuned["decoder.conv_in.weight"])
    bad = {k: v for k, v in tuned.items() if k.startswith("decoder.") and "conv_out" not in k}
    save_file({k[len("decoder."):]: v for k, v in bad.items()}, str(tmp_path / "ft" / "vae_decoder" / "model.safetensors"))
    with pytest.raises(KeyError):
        compose_finetuned_vae(str(tmp_path / "sd" / "vae"), str(tmp_path / "ft"))


def test_encode_text_hf_clip_branch(tmp_path):
    """genpercept_pipeline.py:360-372 with REAL HF objects (a randomly initialised small CLIPTextModel and a CLIPTokenizer built from an
    on-the-fly vocabulary; no checkpoint exists offline): padding='do_not_pad' gives the BOS, EOS pair for the empty prompt, the embedding
    is cached, and -- CLIP's causal mask -- it equals rows [0:2] of the 77-token padded encoding the v1 pipeline stores as
    empty_text_embed.npy, which is why the engine accepts either."""
    import json
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
    from genpercept_amd.pipeline import GenPerceptPipeline
    json.dump({"<|startoftext|>": 0, "<|endoftext|>": 1, "a</w>": 2, "b</w>": 3, "a": 4, "b": 5}, open(tmp_path / "vocab.json", "w"))
    open(tmp_path / "merges.txt", "w").write("#version: 0.2\n")
    tok = CLIPTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"), model_max_length=77)
    torch.manual_seed(0)
    enc = CLIPTextModel(CLIPTextConfig(vocab_size=8, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                       max_position_embeddings=77, bos_token_id=0, eos_token_id=1)).eval()
    pipe = GenPerceptPipeline(unet={}, vae={}, scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False),
                              text_encoder=enc, tokenizer=tok)
    assert pipe.text_embed is None
    pipe.encode_text("")
    assert tuple(pipe.text_embed.shape) == (1, 2, 64) and pipe.text_embed.dtype == torch.float32
    with torch.no_grad():
        e77 = enc(tok("", padding="max_length", max_length=77, return_tensors="pt").input_ids)[0]
    assert torch.allclose(pipe.text_embed, e77[:, :2], atol=1e-5)
    first = pipe.text_embed
    pipe.encode_text("a b")  # a non-empty prompt (infer.py --prompt): more tokens, new embedding
    assert pipe.text_embed.shape[1] == 4 and pipe.text_embed is not first


def test_dataset_conventions_match_reference_classes(tmp_path):
    """tests/golden/datasets_ref.npz: KITTI / ETH3D / ScanNet / DIODE / NYU conventions read off the reference's dataset classes
    (depth ranges, naming mode, KITTI benchmark crop + Garg / Eigen masks, ground-truth decoding)."""
    from PIL import Image
    from genpercept_amd import infer_eval as ie
    g = np.load(os.path.join(ROOT, "tests", "golden", "datasets_ref.npz"))
    for name in ("kitti", "eth3d", "scannet", "diode", "nyu"):
        cfg = ie.DATASETS[name]
        assert [cfg["min_depth"], cfg["max_depth"]] == list(g[f"{name}_range"]), name
        assert cfg["name_mode"].name == str(g[f"{name}_name_mode"]), name
    for h, w, top, left, ch, cw in g["kitti_crop_boxes"]:
        idx = np.arange(h * w).reshape(h, w)
        c = ie.kitti_benchmark_crop(idx)
        assert c.shape == (ch, cw) and c[0, 0] == top * w + left
        depth = np.full((ch, cw), 5.0, dtype=np.float32)
        depth[::7, ::5] = 0.0
        depth[1::11, 2::9] = 90.0
        for crop in ("eigen", "garg", None):
            want = np.unpackbits(g[f"kitti_mask_{crop}_{h}x{w}"])[: ch * cw].reshape(ch, cw).astype(bool)
            got = ie.valid_mask_of(depth, 1e-5, 80.0) & ie.kitti_eval_mask(ch, cw, crop)
            assert np.array_equal(got, want), (h, w, crop)
    raw = g["raw_png_values"]
    Image.fromarray(raw.astype(np.uint16)).save(tmp_path / "d.png")
    for name in ("scannet", "nyu"):
        assert np.array_equal(ie.read_gt_depth(str(tmp_path / "d.png"), name), g[f"{name}_decoded"].astype(np.float32))
    big = np.zeros((375, 1242), dtype=np.uint16)
    big[23:, 13:1229] = 7
    big[40, 100] = 12345
    Image.fromarray(big).save(tmp_path / "k.png")
    kd = ie.read_gt_depth(str(tmp_path / "k.png"), "kitti")
    assert kd.shape == (352, 1216) and kd[40 - 23, 100 - 13] == np.float32(12345 / 256.0) and np.all(kd[:, 0] == np.float32(7 / 256.0))
    assert np.array_equal((raw / 256.0).astype(np.float32), g["kitti_decoded"].astype(np.float32))  # the decode rule itself
    buf = raw.copy()
    buf[2, 3] = np.inf
    buf.tofile(tmp_path / "e.bin")
    ie.DATASETS["_eth3d_small"] = dict(ie.DATASETS["eth3d"], gt=("eth3d_bin", (6, 8)))
    try:
        assert np.array_equal(ie.read_gt_depth(str(tmp_path / "e.bin"), "_eth3d_small"), g["eth3d_decoded"])
    finally:
        del ie.DATASETS["_eth3d_small"]
    np.save(tmp_path / "d.npy", raw[:, :, None])
    assert np.array_equal(ie.read_gt_depth(str(tmp_path / "d.npy"), "diode"), g["diode_decoded"][0])
    m = (raw > 500)
    np.save(tmp_path / "m.npy", m[:, :, None].astype(np.uint8))
    assert np.array_equal(ie.dataset_valid_mask(raw, "diode", str(tmp_path / "m.npy")), m)
    with pytest.raises(ValueError):
        ie.dataset_valid_mask(raw, "diode")


def test_normal_angular_error_matches_reference_angular_loss():
    """The normal evaluator is DEFINED by the reference's angular_loss (geometry_losses.py:550-590); its mean (radians) must equal it."""
    from genpercept_amd import eval_metrics as em
    g = np.load(os.path.join(ROOT, "tests", "golden", "datasets_ref.npz"))
    r = em.normal_angular_error(g["normal_pred"], g["normal_gt"], g["normal_mask"])
    assert abs(r["mean_rad"] - float(g["angular_loss_mean_rad"])) <= 2e-6
    assert abs(r["mean_deg"] - np.degrees(r["mean_rad"])) < 1e-9 and 0.0 <= r["within_11.25"] <= r["within_22.5"] <= r["within_30"] <= 1.0
    same = em.normal_angular_error(g["normal_gt"], g["normal_gt"])
    assert same["mean_deg"] < 1.0  # the clamp at 1 - 1e-4 leaves acos(0.9999) = 0.81 degrees, like the reference
    enc = np.moveaxis((g["normal_gt"][0] + 1.0) / 2.0, 0, -1)  # what the pipeline returns for mode='normal'
    assert np.allclose(em.decode_normals(enc), g["normal_gt"][0], atol=1e-6)


_BENCH_WORKER = r"""
import io, json, os, sys, contextlib, torch
sys.path.insert(0, {root!r})
import bench
from genpercept_amd import distributed as gd

class StubEngine:                      # stands in for genpercept_amd.engine.Engine: infer() marks every image with its GLOBAL index
    calls = 0
    def __init__(self, local_rank, precision):
        self.rank = int(os.environ["RANK"]); self.world = int(os.environ["WORLD_SIZE"])
    def infer(self, rgb, mode):
        StubEngine.calls += 1
        lo, hi = gd.shard_range(4 * self.world, self.rank, self.world)
        assert rgb.shape[0] == hi - lo and rgb.dtype == torch.uint8
        return torch.stack([torch.full((1, rgb.shape[2], rgb.shape[3]), float(i)) for i in range(lo, hi)]) / 16.0
    def close(self):
        pass

buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    line = bench.main(["--gpus", "2", "--steps", "3", "--warmup", "1", "--res", "32"] + {extra!r}, engine_factory=StubEngine, device="cpu")
rank = int(os.environ["RANK"])
full = "--full" in {extra!r}
ok = StubEngine.calls == 1 + 3 + full     # warm-up + timed steps (+ with --full the gather-alone leg's one infer)
if rank == 0:
    printed = json.loads(buf.getvalue().strip().splitlines()[-1])
    ok = ok and printed == line and line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1 and line["scaling"] == "weak"
    g = line["config"]["gather_ms"]
    ok = ok and line["config"]["global_batch"] == 8 and ((g is not None and g >= 0) if full else g is None)
    ok = ok and abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) <= 1e-2 * line["value"] and line["higher_is_better"] is True
else:
    ok = ok and line is None and buf.getvalue().strip() == ""   # ONE JSON line, from rank 0 only
sys.stderr.write("<rank%d:%s>\n" % (rank, "OK" if ok else "FAIL " + buf.getvalue()))
sys.stderr.flush()
sys.exit(0 if ok else 1)
"""


def test_bench_single_rank_precision_legs_with_a_stub_engine(capsys):
    """bench.py's N = 1 control flow around the engine -- the benched bf16 leg, then the fp16 library, then the contract precision, each timed with the same
    steps -- executed on CPU with a stub engine: ONE JSON line carrying value / value_fp16 / value_fp32c, and no profile / parity fields when those legs are off.
    Those legs run with --full only: a plain run builds the benched engine alone and calls it for the warm-up and the timed steps, nothing more."""
    import json
    import time
    import bench
    built = []

    class Stub:
        def __init__(self, local_rank, precision):
            built.append(precision)
            self.precision, self.calls, self.closed = precision, 0, False

        def infer(self, rgb, mode):
            assert not self.closed and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (4, 3, 32, 32)
            self.calls += 1
            time.sleep(0.005)  # (a step long enough for the 3-decimal ms_per_step of the line to resolve it)
            return torch.full((4, 1, 32, 32), {"bf16": 0.25, "fp16": 0.5, "fp32c": 0.75}[self.precision])

        def close(self):
            self.closed = True

    engines = []

    class Counted(Stub):
        def __init__(self, local_rank, precision):
            super().__init__(local_rank, precision)
            engines.append(self)

    # plain run: no --no-* option needed (the stub has no set_profile and there are no weights for the CPU oracle: either leg would raise)
    line = bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--res", "32"], engine_factory=Counted, device="cpu")
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == line and built == ["bf16"] and engines[0].calls == 1 + 2 and engines[0].closed
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "bf16" and line["higher_is_better"] is True
    assert abs(line["value"] - 4 * 2 / (line["ms_per_step"] * 2e-3)) <= 1e-2 * line["value"]
    assert line["roofline"] is None and line["stages"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert line["config"]["gather_ms"] is None and not any(k.endswith(("_fp16", "_fp32c")) for k in line)
    built.clear()
    line = bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--res", "32", "--full", "--no-cpu", "--no-profile"], engine_factory=Stub, device="cpu")
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == line and built == ["bf16", "fp16", "fp32c"]
    assert line["n_gpus"] == 1 and line["dtype"] == "bf16" and line["metric"].startswith("images/sec at 768x768 bf16")
    for k in ("value", "value_fp16", "value_fp32c", "ms_per_step_fp16", "ms_per_step_fp32c"):
        assert line[k] > 0, k
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None and line["value_within_tolerance"] is None
    assert abs(line["value"] - 4 * 2 / (line["ms_per_step"] * 2e-3)) <= 1e-2 * line["value"]
    # a non-default precision is labelled as such and runs no other leg
    built.clear()
    line = bench.main(["--gpus", "1", "--steps", "1", "--warmup", "0", "--res", "32", "--full", "--no-cpu", "--no-profile", "--precision", "fp32c"],
                      engine_factory=Stub, device="cpu")
    capsys.readouterr()
    assert built == ["fp32c"] and line["dtype"] == "fp32c" and "NOT BASELINE" in line["metric"] and "value_fp16" not in line and "value_fp32c" not in line


def test_bench_dump_outputs_writes_the_last_timed_step(tmp_path, capsys, monkeypatch):
    """--dump-outputs DIR: each timed leg's maps of its LAST timed step (the stub returns a new value per call) as DIR/<mode>_<precision>.npy
    float32; --steps sets the number of timed calls exactly; a map above its share of the byte budget is a fixed seeded sample, the same
    from run to run.  The legs, and so the files, are the same with and without --full; a plain line reports the headline leg alone."""
    import bench

    class Stub:
        def __init__(self, local_rank, precision):
            self.calls = 0

        def infer(self, rgb, mode):
            self.calls += 1
            stub.last = self
            b, _, h, w = rgb.shape
            return torch.arange(b * 3 * h * w, dtype=torch.float32).reshape(b, 3, h, w) / (b * 3 * h * w) + self.calls

        def close(self):
            pass

    stub = Stub(0, "bf16")
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--res", "16", "--mode", "normal", "--no-cpu", "--no-profile"]
    line = bench.main(argv + ["--no-fp16", "--dump-outputs", str(tmp_path / "a")], engine_factory=Stub, device="cpu")
    capsys.readouterr()
    assert stub.last.calls == 2 + 3 and line["steps"] == 3 and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "a")) == ["normal_bf16.npy", "normal_fp32c.npy"]
    for name in ("normal_bf16", "normal_fp32c"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (4, 3, 16, 16) and line["dumped_outputs"]["arrays"][name]["sampled"] is False
        np.testing.assert_array_equal(a, (np.arange(4 * 3 * 16 * 16, dtype=np.float32).reshape(4, 3, 16, 16) / (4 * 3 * 16 * 16) + 5))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4 * 1000)  # three legs, 1000 float32 elements each
    for d in ("b", "c"):
        line = bench.main(argv + ["--dump-outputs", str(tmp_path / d)], engine_factory=Stub, device="cpu")
        capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "b")) == ["normal_bf16.npy", "normal_fp16.npy", "normal_fp32c.npy"]
    for name in ("normal_bf16", "normal_fp16", "normal_fp32c"):
        b, c = np.load(tmp_path / "b" / f"{name}.npy"), np.load(tmp_path / "c" / f"{name}.npy")
        assert b.shape == (1000,) and b.dtype == np.float32 and np.array_equal(b, c)
        assert line["dumped_outputs"]["arrays"][name] == {"shape": [4, 3, 16, 16], "stored": 1000, "sampled": True}
        assert np.all(np.diff(b) > 0) and b.min() >= 5 and b.max() < 6  # sorted flat indices into the last step's map
    assert not any(k.endswith(("_fp16", "_fp32c")) for k in line) and line["stages"] is None
    line = bench.main(argv + ["--full", "--dump-outputs", str(tmp_path / "d")], engine_factory=Stub, device="cpu")
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "d")) == sorted(os.listdir(tmp_path / "b")) and line["value_fp16"] > 0 and line["value_fp32c"] > 0
    for name in ("normal_bf16", "normal_fp16", "normal_fp32c"):
        assert np.array_equal(np.load(tmp_path / "b" / f"{name}.npy"), np.load(tmp_path / "d" / f"{name}.npy"))
    with pytest.raises(SystemExit):
        bench.main(argv[:2] + ["--steps", "0"], engine_factory=Stub, device="cpu")


def test_bench_multi_gpu_path_world_size_2_gloo(tmp_path):
    """bench.py's own N > 1 code (init_process_group from the torchrun environment, WORLD_SIZE == --gpus check, contiguous shards, the timed
    loop with barrier + max over ranks, the in-step result gather to rank 0, the gather-alone leg, ONE JSON line from rank 0) executed on
    CPU with gloo and a stub engine -- VERDICT r3 item 8: that code had never run anywhere.  Once with --full (+ the gather-alone leg) and once
    as a plain run (the timed steps, their in-step gather included, and nothing else)."""
    for i, extra in enumerate((["--full", "--no-cpu", "--no-profile", "--no-fp16"], [])):
        script = tmp_path / f"bench_worker{i}.py"
        script.write_text(_BENCH_WORKER.format(root=ROOT, extra=extra))
        port = 31500 + (os.getpid() % 2000) + 2 * i
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
               str(script)]
        # CPU only, also on a GPU machine: with a device visible init_process_group would pick nccl and bind rank r to GPU r
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        assert r.returncode == 0, (extra, r.stdout + r.stderr)
        assert "<rank0:OK>" in r.stderr and "<rank1:OK>" in r.stderr, r.stdout + r.stderr
    # a launcher whose WORLD_SIZE disagrees with --gpus is refused (r1 silently measured one GPU)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE 1 != --gpus 2" in (r.stdout + r.stderr)
