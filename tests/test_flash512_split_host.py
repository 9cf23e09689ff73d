"""flash_attn512_split_kernel (attention.hip) without a GPU: the recipe's own error, the kernel's resources, the planner, the argument checks.

  * model: the kernel's arithmetic in fp32 torch on the CPU -- bf16 split of q, k, v; S = scale (q_hi k_hi + q_lo k_hi + q_hi k_lo); fp32
    softmax; p = p_hi + p_lo; O = p_hi v_hi + p_lo v_hi + p_hi v_lo -- against float64 attention.  It must stay under HALF the GPU gate
    (3e-5, tests/test_flash512_split_gpu.py): the recipe alone is inside the gate, what the kernel adds is summation order;
  * resources: attention.hip compiled to assembly with build.FLAGS for both element types; the kernel neither spills nor uses scratch;
  * planner (gp_c_attention_plan): every contract-precision shape the suite and the benchmark run today stays on the path it had (unfused for
    head_dim 512, flash_attn64_split for head_dim 64); the fused kernel takes over above 8 GiB of unfused workspace or by switch;
  * arguments: gp_flash_attention_hd512_split refuses a stride not divisible by 4, an 8-byte-aligned pointer and ld < 1536 before any launch
    (fake addresses, never dereferenced).
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "genpercept_amd", "csrc", "attention.hip")
KERNEL = "_Z26flash_attn512_split_kernel"
SWITCH = "GENPERCEPT_C_FLASH512"
SCALE = 512 ** -0.5


# ---- the recipe in fp32 ------------------------------------------------------------------------------------------------------------------
def _split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def emulate_split_attention(q, k, v, scale):
    """[b, t, 512] fp32 each -> the recipe's result in fp32 (module docstring)"""
    qh, ql = _split(q)
    kh, kl = _split(k)
    vh, vl = _split(v)
    s = (qh @ kh.transpose(-1, -2) + ql @ kh.transpose(-1, -2) + qh @ kl.transpose(-1, -2)) * scale
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    ph, pl = _split(p)
    o = ph @ vh + pl @ vh + ph @ vl
    return o / p.sum(dim=-1, keepdim=True)


def _inputs(b, t, variant):
    g = torch.Generator().manual_seed(1000 * b + t)
    s = 1.5 * (math.sqrt(3.0) if variant == "wide" else 1.0)
    qkv = torch.randn(b * t, 1536, generator=g) * torch.tensor([s] * 1024 + [1.0] * 512)
    if variant == "ramp":
        ramp = 0.5 + 1.5 * torch.arange(t, dtype=torch.float32) / t
        qkv[:, 512:1024] *= ramp.repeat(b)[:, None]
    return qkv


SHAPES = [(1, 1), (1, 31), (1, 37), (2, 64), (3, 100), (2, 256), (1, 1200), (1, 2500)]
MODEL_CASES = [(b, t, "plain") for b, t in SHAPES] + [(b, t, v) for v in ("wide", "ramp") for b, t in SHAPES if t > 1]


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_recipe_alone_is_inside_half_the_gate(case):
    b, t, variant = case
    qkv = _inputs(b, t, variant)
    q, k, v = (qkv[:, i * 512:(i + 1) * 512].reshape(b, t, 512) for i in range(3))
    ref = torch.softmax(q.double() @ k.double().transpose(-1, -2) * SCALE, dim=-1) @ v.double()
    out = emulate_split_attention(q, k, v, SCALE)
    rel = ((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"recipe{case}: rel_rms={rel:.3e}")
    assert rel <= 1.5e-5, rel


# ---- resources ---------------------------------------------------------------------------------------------------------------------------
def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.parametrize("elt", ["bf16", "fp16"])
def test_kernel_neither_spills_nor_uses_scratch(elt, tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not on this machine: the resources of flash_attn512_split_kernel cannot be read")
    from genpercept_amd.build import FLAGS
    out = tmp_path / "attention.s"
    defs = ["-DGP_F16=1"] if elt == "fp16" else []
    r = subprocess.run([hipcc, *FLAGS, *defs, "--cuda-device-only", "-S", SRC, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = out.read_text().splitlines()
    names = [i for i, ln in enumerate(lines) if re.match(r"\s*\.name:\s+" + KERNEL, ln)]
    assert names, "flash_attn512_split_kernel is not in attention.hip's code object"
    name = names[0]
    m0 = max(i for i in range(name) if lines[i].lstrip().startswith("- .agpr_count:"))
    m1 = next((i for i in range(name, len(lines)) if lines[i].lstrip().startswith("- .agpr_count:")), len(lines))
    meta = dict(m.groups() for m in (re.match(r"  [ -] \.(\w+):\s+(\S+)\s*$", ln) for ln in lines[m0:m1]) if m)
    assert int(meta["vgpr_spill_count"]) == 0, meta
    assert int(meta["private_segment_fixed_size"]) == 0, meta
    start = next(i for i, ln in enumerate(lines) if re.match(KERNEL + r"\w*:", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel " + KERNEL))
    assert not [ln for ln in lines[start:end] if re.match(r"\s*scratch_", ln)], "scratch access in flash_attn512_split_kernel"


# ---- planner and argument checks (the built library, no GPU) ------------------------------------------------------------------------------
def _lib():
    from genpercept_amd import engine as ge
    try:
        return ge, ge.load_library("bf16")
    except (ImportError, OSError) as e:
        pytest.skip(f"the bf16 library is not built: {e}")


def test_planner_keeps_todays_shapes_and_takes_over_above_8_gib(monkeypatch):
    ge, _ = _lib()
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv("GENPERCEPT_C_NO_FLASH", raising=False)
    assert ge.c_attention_plan(4, 9216, 1, 512) == (0, 10 * 4 * 9216 * 9216)          # batch 4 at 768^2: unfused, as before
    assert ge.c_attention_plan(8, 9216, 1, 512)[0] == 0                               # batch 8 at 768^2 (6.8 GB): the largest shape run today
    assert ge.c_attention_plan(1, 16640, 1, 512) == (0, 10 * 16640 * 16640)           # the 130 x 128 map of test_vae_attention_contract_precision
    assert ge.c_attention_plan(4, 16384, 1, 512) == (2, 6144 * 4 * 16384)             # 10.7 GB unfused -> fused, 6 KiB per token (T % 64 == 0: no padding)
    assert ge.c_attention_plan(1, 147456, 1, 512)[0] == 2                             # one image at 3072^2
    assert ge.c_attention_plan(4, 9216, 5, 64)[0] == 1                                # head_dim 64 keeps flash_attn64_split
    assert ge.c_attention_plan(1, 100, 1, 512) == (0, 10 * 100 * 128)                 # Tpad = 128
    monkeypatch.setenv(SWITCH, "1")
    assert ge.c_attention_plan(1, 120, 1, 512) == (2, 4096 * 120 + 2048 * 128)        # planes: q | k hi + lo per token, V^T hi + lo per padded token
    assert ge.c_attention_plan(4, 9216, 5, 64)[0] == 1
    monkeypatch.setenv(SWITCH, "0")
    assert ge.c_attention_plan(4, 16384, 1, 512) == (0, 10 * 4 * 16384 * 16384)
    assert ge.c_attention_plan(1, 147456, 1, 512)[0] == 0
    monkeypatch.delenv(SWITCH)
    assert ge.c_attention_plan(4, 16384, 1, 512)[0] == 2                              # the switch is read again at every call
    path, ws = C.c_int(0), C.c_longlong(0)
    lib = ge.load_library("bf16")
    assert lib.gp_c_attention_plan(0, 64, 1, 512, C.byref(path), C.byref(ws)) == 1    # GP_ERR_INVALID
    assert lib.gp_c_attention_plan(1, 64, 1, 100, C.byref(path), C.byref(ws)) == 1
    assert lib.gp_c_attention_plan(1, 64, 1, 512, None, C.byref(ws)) == 1


def test_entry_refuses_bad_arguments_before_any_launch():
    _, lib = _lib()
    A16, A8 = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 8)
    INV = 1  # GP_ERR_INVALID
    f = lib.gp_flash_attention_hd512_split
    assert f(A16, 1538, A16, 1, 64, SCALE, None) == INV        # stride not divisible by 4
    assert f(A8, 1536, A16, 1, 64, SCALE, None) == INV         # 8-byte-aligned input
    assert f(A16, 1536, A8, 1, 64, SCALE, None) == INV         # 8-byte-aligned output
    assert f(A16, 1532, A16, 1, 64, SCALE, None) == INV        # ld < 1536
    assert f(None, 1536, A16, 1, 64, SCALE, None) == INV and f(A16, 1536, None, 1, 64, SCALE, None) == INV
    assert f(A16, 1536, A16, 0, 64, SCALE, None) == INV and f(A16, 1536, A16, 1, 0, SCALE, None) == INV
    assert lib.gp_pool_bytes(None, None) == INV
