"""What the host and GPU tests of the post-processing ops (foreground, guided, tiled, geometry, lens_blur, stereo, parallax) share: the
sanitizer build of a stand-alone check program and its run, bit comparisons, the scalar 16-bit quantiser, both libraries, the drivers of the
"declared, exported, bound" and "refused without a GPU" tests, the library handle that records every call, the nearness in plain loops and
the batch of scenes, and for the GPU tests misaligned device views, the tiny model weights, the tiny pipeline, the three-PNG dataset and
the "refused with real buffers around it" driver.  A plain module: the tests import it the way they import one another (their directory is put on sys.path)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
GP_ERR_INVALID = 1


# ---- check programs ---------------------------------------------------------------------------------------------------------------------
def clangxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("amdclang++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def build_check(tmp_path_factory, src, extra_flags=("-ffp-contract=off",)):
    """tests/`src` built with the ROCm clang++ under AddressSanitizer and UBSan, warnings as errors; the path of the program.  Skips where
    that compiler is not on the machine."""
    cxx = clangxx()
    if cxx is None:
        pytest.skip(f"the ROCm clang++ is not on this machine: {src} cannot be built")
    stem = os.path.splitext(src)[0]
    exe = tmp_path_factory.mktemp(stem) / stem
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *extra_flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-Werror", os.path.join(TESTS, src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_check(exe, src, dst, timeout=60):
    """One run of a check program on the input file `src`: it exits 0 and ends its output with "ok".  Returns (its output lines, the bytes
    it wrote to `dst`)."""
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0 and run.stdout.splitlines()[-1] == "ok", (run.returncode, run.stdout, run.stderr)
    with open(dst, "rb") as f:
        return run.stdout.splitlines(), f.read()


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, dtype=None):
    """Two arrays of one dtype (`dtype`, where given) and shape with the same bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and (dtype is None or a.dtype == dtype) and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits64(a, b):
    return same_bits(a, b, np.float64)


def q16(v):
    """The 16-bit quantiser on one value, in scalar float32 steps."""
    v = np.float32(v)
    v = (v if v < np.float32(1.0) else np.float32(1.0)) if v > np.float32(0.0) else np.float32(0.0)
    return int(v * np.float32(65535.0))


# ---- symbols and arguments --------------------------------------------------------------------------------------------------------------
def libs():
    """Both element-type libraries as they stand in the tree (a missing one is an error, not a skip)."""
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


def assert_entries_bound(names, hip_source, math_header=None, contract_off=True):
    """Every entry of `names` is declared in the public header, listed in engine.SYMBOLS, exported by both libraries with those ctypes and
    named in INTEGRATION.md; the ABI version is 3; `hip_source` is built; the arithmetic header `math_header` (under csrc/), where the op has
    one, pins contraction off.  Returns (the public header's text, the arithmetic header's text or None)."""
    from genpercept_amd import engine
    from genpercept_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    for lib in libs():
        for name in names:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
        assert lib.gp_abi_version() == 3
    assert hip_source in SOURCES and "#define GP_ABI_VERSION 3" in hdr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in names)
    math_h = open(os.path.join(ROOT, "genpercept_amd", "csrc", math_header)).read() if math_header else None
    if math_h is not None and contract_off:
        assert "#pragma clang fp contract(off)" in math_h
    return hdr, math_h


def assert_all_refused(call, lib, ok, cases):
    """Every change of `cases` to the valid argument set `ok` is refused by the entry's argument checks."""
    for kw in cases:
        assert call(lib, dict(ok, **kw)) == GP_ERR_INVALID, kw


def library_calls(monkeypatch):
    """engine.load_library gives a handle whose every entry records its name and fails; the list of those names.  (The test files wrap
    this in a fixture of the same name.)"""
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


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def loops_nearness(pred, space):
    """The nearness of a map [h, w] in plain loops, as lists [h][w]: the scalar quantiser, mirrored in depth space, 0 for a NaN."""
    h, w = pred.shape
    D = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            v = np.float32(pred[y, x])
            if np.isnan(v):
                continue
            q = q16(v)
            D[y][x] = q if space == "disparity" else 65535 - q
    return D


def batch_case(scene, seed, b, h, w, middle_nan=False):
    """b images of `scene(rng, h, w)`, which returns (pred [h, w], further arrays of the image ...): (pred [b, 1, h, w], the further
    arrays stacked ...); middle_nan makes the middle map all NaN."""
    rng = np.random.RandomState(seed)
    per = [scene(rng, h, w) for _ in range(b)]
    pred, *rest = (np.stack([p[k] for p in per]) for k in range(len(per[0])))
    if middle_nan:
        pred[b // 2] = np.nan
    return (pred[:, None], *rest)


# ---- GPU tests (torch is imported where it is used: the host tests above need none) ------------------------------------------------------
def offset4(x):
    """The array on the device as a contiguous view that starts four bytes into a 16-byte aligned buffer."""
    import torch
    x = np.ascontiguousarray(x)
    per = 4 // x.dtype.itemsize
    flat = torch.empty(x.size + per, dtype=torch.from_numpy(x).dtype, device="cuda")
    v = flat[per:].view(x.shape)
    v.copy_(torch.from_numpy(x))
    assert v.data_ptr() % 16 == 4 and v.storage_offset() == per
    return v


def unaligned(x):
    """The array on the device as a contiguous view that starts one element (one byte of a uint8 array) into its buffer."""
    import torch
    flat = torch.empty(x.size + 1, dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    v = flat[1:].view(x.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return v


def bits(t):
    """A float32 tensor's bits as int32, for torch.equal (NaNs compare by their bits)."""
    import torch
    return t.contiguous().view(torch.int32)


def tiny_weights_dict():
    """The tiny UNet and VAE of the oracle with synthetic weights: what the pipeline tests of the ops run."""
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    return dict(uc=uc, vc=vc, usd=osd.synth_state_dict(osd.unet_manifest(uc), 1), vsd=osd.synth_state_dict(osd.vae_manifest(vc), 2))


def tiny_pipeline(tw, seed):
    """The one-step bf16 pipeline over the weights `tw` of `tiny_weights_dict`, on the GPU, its text embedding drawn from a generator
    seeded with `seed`: (the pipeline, that generator, for the test's images)."""
    import torch
    from genpercept_amd import GenPerceptPipeline
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn(2, tw["uc"].cross_attention_dim, generator=g)
    pipe = GenPerceptPipeline(unet=tw["usd"], vae=tw["vsd"], scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False,
                                                                                       steps_offset=1, timestep_spacing="leading"),
                              text_encoder=ctx, tokenizer=None, torch_dtype=torch.bfloat16)
    pipe.to("cuda")
    return pipe, g


def write_png_dataset(data, g, n, h, w):
    """n random h x w images from the generator `g`, each with a darker left part and a weaker green below a row of its own, written as
    `data`/set0/im/0000.png ...: (the samples of a filename list, the images as one uint8 [n, 3, h, w] tensor)."""
    import torch
    from PIL import Image
    samples, images = [], []
    os.makedirs(os.path.join(data, "set0", "im"), exist_ok=True)
    for i in range(n):
        rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rgb[:, : 40 + 10 * i] //= 2
        rgb[30 + 5 * i:, :, 1] //= 3
        Image.fromarray(rgb.numpy()).save(os.path.join(data, "set0", "im", f"{i:04d}.png"))
        samples.append([f"set0/im/{i:04d}.png"])
        images.append(rgb.permute(2, 0, 1).contiguous())
    return samples, torch.stack(images)


def assert_refused_with_real_buffers(call, lib, ok, cases, bufs=None, fresh=None):
    """`assert_all_refused` with real device buffers in `ok`, then a synchronisation; the buffers `bufs` still equal what `fresh()` makes
    (their fill), which is returned."""
    import torch
    assert_all_refused(call, lib, ok, cases)
    torch.cuda.synchronize()
    untouched = fresh() if fresh is not None else None
    if untouched is not None:
        assert all(torch.equal(bufs[k], untouched[k]) for k in bufs)
    return untouched
