"""GroupNorm offset invariance of the contract precision, end to end.  GroupNorm removes any offset that is the same for every channel of a
group, and a diffusers ResnetBlock2D's conv1 feeds nothing but norm2 (resnet.py forward: conv1 -> (+ time_emb_proj) -> norm2), so adding a
group-constant offset to conv1's bias leaves the exact output of the pipeline unchanged.  What it does change is the arithmetic: every norm2
input now has mean / std = 100 in every group, the regime where single-pass fp32 {sum, sum of squares} statistics lose eps (mean / std)^2 of the
variance (2e-4 at 100) and scale whole groups by the error.  The contract precision's statistics are centred (csrc/contract.hip:
c_gn_stats_kernel), so the shifted weights must land where the unshifted ones do.

Offsets: 100 x the standard deviation of that group's norm2 input, measured with the fp32 oracle on the fixture's image (sign random per group),
in every resnet of the VAE encoder, the UNet and the VAE decoder.  Both weight sets run through the fp32c engine and are compared with the live
oracle of the UNSHIFTED weights at the outlier stress test's fixture size (256^2)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RES = 256
RATIO = 100.0


def _rel_rms(out, ref):
    out, ref = out.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(((out - ref) ** 2).mean()) / (np.sqrt(((ref - ref.mean()) ** 2).mean()) + 1e-30))


@pytest.fixture(scope="module")
def fixture():
    from genpercept_amd import config as gc
    from genpercept_amd import weights as gw
    from oracle import pipeline as opipe
    from oracle import sd21 as osd
    torch.set_num_threads(max(1, min(os.cpu_count() or 8, 16)))
    ucfg, vcfg = gc.UNetConfig(), gc.VAEConfig()
    usd = gw.synth_state_dict(gw.unet_manifest(ucfg), seed=0)
    vsd = gw.synth_state_dict(gw.vae_manifest(vcfg), seed=1)
    ctx = torch.randn(2, 1024, generator=torch.Generator().manual_seed(2))
    g = torch.Generator().manual_seed(5)
    noise = torch.randint(0, 256, (1, 3, RES, RES), generator=g, dtype=torch.uint8).float()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, RES), torch.linspace(0, 1, RES), indexing="ij")
    rgb8 = (0.5 * noise + 0.5 * torch.stack([yy, xx, (yy + xx) / 2])[None] * 255.0).round().clamp(0, 255).to(torch.uint8)
    # the oracle's GroupNorm, recording the per-group standard deviation of every resnet norm2 input on the way
    stds, gn = {}, osd._gn

    def recording_gn(x, sd, p, groups, eps):
        if p.endswith(".norm2"):
            model = "unet" if sd is usd else "vae" if sd is vsd else None
            assert model is not None
            stds[(model, p[: -len(".norm2")])] = x[0].double().reshape(groups, -1).std(dim=1, unbiased=False)
        return gn(x, sd, p, groups, eps)

    osd._gn = recording_gn
    try:
        with torch.no_grad():
            ref = opipe.single_infer(vsd, osd.VAECfg(), usd, osd.UNetCfg(), opipe.normalize_rgb(rgb8), ctx, "depth")[0].numpy()
    finally:
        osd._gn = gn
    assert ref.std() > 0.05, "the fixture must leave a non-degenerate map"
    # the shifted weights: conv1.bias[c] += +-RATIO * std(group of c)
    gs = torch.Generator().manual_seed(7)
    shifted = {"unet": dict(usd), "vae": dict(vsd)}
    for (model, p), sd_ in stds.items():
        b = shifted[model][p + ".conv1.bias"].clone()
        groups = sd_.numel()
        sign = torch.where(torch.rand(groups, generator=gs) < 0.5, -1.0, 1.0).double()
        b += (RATIO * sign * sd_).float().repeat_interleave(b.numel() // groups)
        shifted[model][p + ".conv1.bias"] = b
    n_unet = sum(1 for m, _ in stds if m == "unet")
    n_vae = sum(1 for m, _ in stds if m == "vae")
    assert n_unet == 22 and n_vae >= 20, (n_unet, n_vae)  # every resnet of the UNet, the VAE encoder and the VAE decoder
    return dict(ucfg=ucfg, vcfg=vcfg, plain={"unet": usd, "vae": vsd}, shifted=shifted, ctx=ctx, rgb8=rgb8, ref=ref)


def _run(fx, weights):
    from genpercept_amd.engine import Engine
    eng = Engine(0, fx["ucfg"], fx["vcfg"], None, precision="fp32c")
    try:
        eng.load_state_dict("vae", weights["vae"])
        eng.load_state_dict("unet", weights["unet"])
        eng.set_context(fx["ctx"])
        eng.finalize()
        out = eng.infer(fx["rgb8"].to(torch.device("cuda", 0)), "depth")
        assert torch.isfinite(out).all()
        o0 = out[0].cpu().numpy()
    finally:
        eng.close()
    ref = fx["ref"]
    return dict(mean_abs=float(np.abs(o0 - ref).mean()), max_abs=float(np.abs(o0 - ref).max()), rel_rms=_rel_rms(o0, ref))


def test_group_constant_conv1_offsets_leave_the_contract_precision_unchanged(fixture, metric_log):
    plain = _run(fixture, fixture["plain"])
    shifted = _run(fixture, fixture["shifted"])
    metric_log("groupnorm_offset_invariance[fp32c]", **{f"plain_{k}": v for k, v in plain.items()}, **{f"shifted_{k}": v for k, v in shifted.items()})
    assert plain["mean_abs"] <= 1e-3 and plain["rel_rms"] <= 1e-3, plain
    assert shifted["mean_abs"] <= 1e-3 and shifted["rel_rms"] <= 1e-3, shifted      # north_star, both readings
    # Measured on MI355X: plain 4.34e-6 / 5.35e-5, shifted 1.06e-5 / 1.31e-4 (2.43x / 2.44x).  The build before the centred statistics:
    # shifted 3.17e-5 / 3.88e-4 (7.6x / 7.6x).  The fp32 oracle itself on the shifted weights: 2.3e-4 / 2.7e-3 (outside 1e-3).
    # What remains is the x * scale + shift form on fp32 data (the kernel tests' 8 * 2^-24 (mean / std) |gamma| term): scale and shift are
    # fp32, shift ~ 100 |gamma|, so each norm2 output carries a per-channel systematic ~2^-25 * 100 |gamma|, the order of the split products'
    # own noise the plain run sits at.  (The exact invariance of the shifted weights, float64 oracle with the norm2 inputs stored in fp32:
    # 9.1e-7 / 1.1e-5, so storage alone is 0.2x of the plain run.)  Gate: 3x -- the single-pass statistics fail it by 2.5x.
    assert shifted["mean_abs"] <= 3 * plain["mean_abs"], (shifted, plain)
    assert shifted["rel_rms"] <= 3 * plain["rel_rms"], (shifted, plain)
