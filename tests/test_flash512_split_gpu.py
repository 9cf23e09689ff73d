"""flash_attn512_split_kernel (attention.hip) on the GPU: the contract precision's one-head, head_dim-512 attention with scores and
probabilities kept on the CU.

  * the kernel (+ c_qkv_planes) through `engine.flash_attention_hd512_split` against float64 attention on the same fp32 inputs.  The gate,
    rel-rms <= 3e-5, is `test_flash_attention_split_operands`' own (the head_dim-64 twin of the same recipe); the recipe alone measures
    2.5e-6 .. 1.3e-5 in fp32 emulation on these inputs (tests/test_flash512_split_host.py);
  * bitwise reproducibility, and independence of an image's result from the batch it is in;
  * through the engine (`precision="fp32c"`, GENPERCEPT_C_FLASH512): the VAE mid-block attention against the fp32 oracle and against the
    unfused path at 2e-4 of the branch (`test_vae_attention_contract_precision`'s gate), the launch log, and the pool's size with and without
    the fused kernel on a map whose logits alone are 1.1 GB.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "GENPERCEPT_C_FLASH512"
SCALE = 512 ** -0.5


def _dev():
    return torch.device("cuda", 0)


def _bf16_only():
    from genpercept_amd import engine as e
    if e.act_dtype() != torch.bfloat16:
        pytest.skip("the contract precision lives in the bf16 library")
    return e


def _inputs(b, t, variant):
    """fp32 qkv [b*t, 1536]: q, k of element std 1.5 (logit std 2.25 at scale 512^-0.5), v of std 1.  "wide": q, k std 1.5 sqrt(3) (logit std
    6.7).  "ramp": key j scaled by 0.5 + 1.5 j / t, which raises the running maximum several times per row."""
    g = torch.Generator().manual_seed(1000 * b + t)
    s = 1.5 * (math.sqrt(3.0) if variant == "wide" else 1.0)
    qkv = torch.randn(b * t, 1536, generator=g) * torch.tensor([s] * 1024 + [1.0] * 512)
    if variant == "ramp":
        ramp = 0.5 + 1.5 * torch.arange(t, dtype=torch.float32) / t
        qkv[:, 512:1024] *= ramp.repeat(b)[:, None]
    return qkv


def _ref64(qkv, b, t):
    q, k, v = (qkv[:, i * 512:(i + 1) * 512].reshape(b, t, 512).double() for i in range(3))
    return (torch.softmax(q @ k.transpose(-1, -2) * SCALE, dim=-1) @ v).reshape(b * t, 512)


CASES = [(1, 1, "plain"), (1, 31, "plain"), (1, 37, "plain"), (2, 64, "plain"), (3, 100, "plain"), (2, 256, "plain"), (1, 1200, "plain"),
         (1, 2500, "plain"), (2, 256, "wide"), (1, 1200, "wide"), (1, 200, "ramp"), (2, 1000, "ramp")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_flash512_split_vs_float64(case, metric_log):
    """T below one 32-key tile, ragged against 32 / 64 / 128, exact multiples, several 64-query blocks, B > 1 offsets; wide logits; a moving
    running maximum.  Finite, rel-rms <= 3e-5 of float64, and the operand's third block repeats its first ([hi | lo | hi])."""
    e = _bf16_only()
    b, t, variant = case
    qkv = _inputs(b, t, variant)
    ref = _ref64(qkv, b, t)
    out, op = e.flash_attention_hd512_split(qkv.to(_dev()), b, t, SCALE, return_operand=True)
    out, op = out.cpu(), op.cpu()
    err = (out.double() - ref).abs()
    rel = (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    metric_log(f"flash_attn512_split{case}", rel_rms=rel, max_abs=err.max().item())
    print(f"flash_attn512_split{case}: rel_rms={rel:.3e} max_abs={err.max().item():.3e}")
    assert torch.isfinite(out).all()
    assert torch.equal(op[:, :512], op[:, 1024:]), "[hi | lo | hi]: the third block is not the first"
    assert rel <= 3e-5, rel


def test_flash512_split_is_reproducible_and_batch_independent():
    e = _bf16_only()
    d = _dev()
    qkv = _inputs(2, 256, "plain").to(d)
    a = e.flash_attention_hd512_split(qkv, 2, 256, SCALE, return_operand=True)[1]
    b = e.flash_attention_hd512_split(qkv, 2, 256, SCALE, return_operand=True)[1]
    assert torch.equal(a, b), "two calls differ"
    qkv = _inputs(3, 100, "plain").to(d)
    whole = e.flash_attention_hd512_split(qkv, 3, 100, SCALE, return_operand=True)[1]
    alone = e.flash_attention_hd512_split(qkv[100:200].contiguous(), 1, 100, SCALE, return_operand=True)[1]
    assert torch.equal(whole[100:200], alone), "image 1 of a batch of 3 differs from the same image alone"


# ---- through the engine ------------------------------------------------------------------------------------------------------------------
_P = "decoder.mid_block.attentions.0"
_cache = {}


def _vae_sd():
    """weights of test_vae_attention_contract_precision: to_q / to_k x 3, logits of a few units"""
    if "sd" not in _cache:
        from oracle import sd21 as osd
        vsd = osd.synth_state_dict(osd.vae_manifest(osd.VAECfg()), 21)
        for n in ("to_q", "to_k"):
            vsd[f"{_P}.{n}.weight"] = vsd[f"{_P}.{n}.weight"] * 3.0
        _cache["sd"] = vsd
    return _cache["sd"]


def _run(x, switch, monkeypatch, profile=0):
    """vae_mid_attention of a fresh fp32c engine created under GENPERCEPT_C_FLASH512 = switch (None: unset) -> (out, launch names, pool bytes)"""
    from genpercept_amd.engine import Engine
    from oracle import sd21 as osd
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    eng = Engine(0, osd.UNetCfg.tiny(), osd.VAECfg(), None, precision="fp32c")
    try:
        eng.load_state_dict("vae", _vae_sd())
        eng.finalize()
        if profile:
            eng.set_profile(profile)
        out = eng.vae_mid_attention(x.cuda(), decoder=True).cpu()
        names = [n for _, _, n in eng.launch_log()] if profile else []
        return out, names, eng.pool_bytes()
    finally:
        eng.close()


@pytest.mark.parametrize("hw", [(12, 10), (20, 13)])
def test_vae_attention_through_the_fused_kernel(hw, metric_log, monkeypatch):
    _bf16_only()
    from oracle import sd21 as osd
    vc = osd.VAECfg()
    x = torch.randn(2, 512, hw[0], hw[1], generator=torch.Generator().manual_seed(hw[0]))
    with torch.no_grad():
        ref = osd.vae_mid_attention(x, _vae_sd(), _P, vc.norm_num_groups, vc.norm_eps)
    fused, names1, _ = _run(x, "1", monkeypatch, profile=3)
    unfused, names0, _ = _run(x, "0", monkeypatch, profile=3)
    _, names_unset, _ = _run(x, None, monkeypatch, profile=3)
    branch = (ref - x).pow(2).mean().sqrt()
    r = ((fused - ref).pow(2).mean().sqrt() / branch).item()
    r0 = ((fused - unfused).pow(2).mean().sqrt() / branch).item()
    metric_log(f"vae_attn_contract_flash512{hw}", rel_rms_of_branch=r, vs_unfused=r0, max_abs=(fused - ref).abs().max().item())
    print(f"vae_attn_contract_flash512{hw}: vs oracle {r:.3e}, vs unfused {r0:.3e}")
    assert any("flash_attn512_split" in n for n in names1), names1
    assert not any("flash_attn512_split" in n for n in names0), names0
    assert not any("flash_attn512_split" in n for n in names_unset), "the fused kernel ran with the switch unset at a small size"
    assert torch.isfinite(fused).all() and r <= 2e-4, r
    assert r0 <= 2e-4, r0


def test_fused_attention_keeps_the_logits_out_of_the_pool(metric_log, monkeypatch):
    """130 x 128 map, one image: T = Tpad = 16640, the fp32 logits alone are T * Tpad * 4 = 1.108 GB."""
    _bf16_only()
    h, w = 130, 128
    t = h * w
    logits = t * t * 4
    x = torch.randn(1, 512, h, w, generator=torch.Generator().manual_seed(h))
    fused, _, pool1 = _run(x, "1", monkeypatch)
    unfused, _, pool0 = _run(x, "0", monkeypatch)
    r = ((fused - unfused).pow(2).mean().sqrt() / (unfused - x).pow(2).mean().sqrt()).item()
    metric_log("vae_attn_contract_flash512_pool", pool_fused=pool1, pool_unfused=pool0, logits_bytes=logits, fused_vs_unfused=r)
    print(f"pool: fused {pool1 / 1e9:.3f} GB, unfused {pool0 / 1e9:.3f} GB, logits {logits / 1e9:.3f} GB; fused vs unfused {r:.3e}")
    assert pool1 < logits, (pool1, logits)
    assert pool0 >= logits, (pool0, logits)
    assert torch.isfinite(fused).all() and r <= 2e-4, r
