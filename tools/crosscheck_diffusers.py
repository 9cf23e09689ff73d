#!/usr/bin/env python3
"""One-off validation tool: compare the fp32 oracle (oracle/) with the real `diffusers` modules.

The build container and the GPU boxes have neither `diffusers` nor SD2.1 weights, which is why the VAE / UNet restatement is
"parity unpinned" by reference fixtures.  On any machine that has `diffusers` (>= 0.25) and, optionally, a
local SD2.1 checkpoint, this script closes that gap:

    python tools/crosscheck_diffusers.py                       # random-initialised diffusers modules (architecture check)
    python tools/crosscheck_diffusers.py --sd21 /path/to/sd21  # the real stabilityai/stable-diffusion-2-1 weights

It instantiates UNet2DConditionModel / AutoencoderKL, copies their state dicts into the oracle (zero missing / unexpected keys is the
first check), runs both on the same seeded inputs on the CPU in fp32 and reports max / rms differences per stage.  It is a
validation tool, not a code path: nothing in genpercept_amd/ or bench.py imports it.

One-command form for a machine that has diffusers but not this build container:

    python tools/crosscheck_diffusers.py --verify tests/golden/crosscheck_tiny.npz

The committed fixture (written here, offline, by `--emit`; tests/test_block_identities.py keeps it in step with the oracle) holds a TINY configuration of
the SD2.1 topology -- same block types, widths 64 / 128 / 256 / 256, seeded weights that `oracle.sd21.synth_state_dict` regenerates (per-module checksums
in the fixture detect a torch build that draws other numbers) -- with seeded inputs and the ORACLE's outputs for encode_rgb, the UNet at t = 1 (sample
and the four up-block features), and the decoder.  `--verify` instantiates diffusers' UNet2DConditionModel / AutoencoderKL with that configuration,
loads the regenerated weights (zero missing / unexpected keys is the first check), runs them on the fixture's inputs and prints, per stage,
    <stage>  rel max diff <d>   (<= tol: OK)
then `OK` (exit 0: row 8c's "parity unpinned" is closed for the block internals) or `MISMATCH` (exit 1).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), num_heads=(1, 2, 4, 4), cross_attention_dim=64)
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128))
SEEDS = dict(unet=101, vae=102, inputs=103)


def _checksums(sd):
    """per tensor: sum and sum of squares in float64, each correctly rounded (math.fsum), so that no thread count or reduction order moves a bit"""
    import math
    import numpy as np
    rows = []
    for v in sd.values():
        a = v.double().numpy().ravel()
        rows.append([math.fsum(a), math.fsum(a * a)])
    return np.array(rows, dtype=np.float64)


def build_fixture():
    """inputs, oracle outputs and weight checksums of the tiny configuration (pure oracle: runs in the build container)"""
    import numpy as np
    from oracle import sd21 as osd
    ucfg, vcfg = osd.UNetCfg(**TINY_UNET), osd.VAECfg(**TINY_VAE)
    usd = osd.synth_state_dict(osd.unet_manifest(ucfg), SEEDS["unet"])
    vsd = osd.synth_state_dict(osd.vae_manifest(vcfg), SEEDS["vae"])
    g = torch.Generator().manual_seed(SEEDS["inputs"])
    rgb = torch.rand(1, 3, 72, 88, generator=g) * 2 - 1      # latent 9 x 11: not divisible by 8 -> the upsample_size rule is exercised
    ctx = torch.randn(1, 2, ucfg.cross_attention_dim, generator=g)
    with torch.no_grad():
        lat = osd.encode_rgb(vsd, vcfg, rgb)
        v, feats = osd.unet_forward(usd, ucfg, lat, 1, ctx)
        dec = osd.vae_decode(vsd, vcfg, -v / vcfg.scaling_factor)
    out = dict(rgb=rgb.numpy(), ctx=ctx.numpy(), latent=lat.numpy(), unet=v.numpy(), dec=dec.numpy(), unet_checksums=_checksums(usd), vae_checksums=_checksums(vsd),
               config=np.array(repr(dict(unet=TINY_UNET, vae=TINY_VAE, seeds=SEEDS, timestep=1, torch=torch.__version__))))
    for i, f in enumerate(feats):
        out[f"feat{i}"] = f.numpy()
    return out


def verify_fixture(path, tol):
    import numpy as np
    try:
        from diffusers import AutoencoderKL, UNet2DConditionModel
    except ImportError:
        print("diffusers is not installed here: nothing to verify (this is expected in the build container)")
        return 2
    from oracle import sd21 as osd
    fx = np.load(path)
    ucfg, vcfg = osd.UNetCfg(**TINY_UNET), osd.VAECfg(**TINY_VAE)
    usd = osd.synth_state_dict(osd.unet_manifest(ucfg), SEEDS["unet"])
    vsd = osd.synth_state_dict(osd.vae_manifest(vcfg), SEEDS["vae"])
    if not (np.allclose(_checksums(usd), fx["unet_checksums"], rtol=1e-9) and np.allclose(_checksums(vsd), fx["vae_checksums"], rtol=1e-9)):
        print("this torch build regenerates other weights than the fixture was written with: run the direct mode (no --verify) instead")
        return 3
    unet = UNet2DConditionModel(sample_size=16, in_channels=4, out_channels=4, block_out_channels=TINY_UNET["block_out_channels"],
                                down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
                                layers_per_block=2, cross_attention_dim=TINY_UNET["cross_attention_dim"], attention_head_dim=TINY_UNET["num_heads"],
                                use_linear_projection=True).eval()
    vae = AutoencoderKL(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=TINY_VAE["block_out_channels"], layers_per_block=2,
                        down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4, norm_num_groups=32, sample_size=64).eval()
    ok = True
    for name, mod, sd in (("unet", unet, usd), ("vae", vae, vsd)):
        r = mod.load_state_dict(sd, strict=False)
        print(f"{name}: missing {len(r.missing_keys)}, unexpected {len(r.unexpected_keys)}")
        ok &= not (r.missing_keys or r.unexpected_keys)

    def report(stage, a, b):
        nonlocal ok
        d = float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
        print(f"{stage:14s} rel max diff {d:.3e}   ({'<= tol: OK' if d <= tol else '> tol'})")
        ok &= d <= tol

    rgb, ctx = torch.from_numpy(fx["rgb"]), torch.from_numpy(fx["ctx"])
    with torch.no_grad():
        lat = vae.quant_conv(vae.encoder(rgb))[:, :4] * 0.18215
        report("vae.encode", fx["latent"], lat.numpy())
        lat_o = torch.from_numpy(fx["latent"])
        v = unet(lat_o, 1, encoder_hidden_states=ctx).sample
        report("unet(t=1)", fx["unet"], v.numpy())
        dec = vae.decoder(vae.post_quant_conv(-torch.from_numpy(fx["unet"]) / 0.18215))
        report("vae.decode", fx["dec"], dec.numpy())
    print("(the four up-block features of the fixture are the CUSTOM UNet's outputs, custom_unet.py:365-400: compare them with the reference's "
          "CustomUNet2DConditionModel if /root/reference is importable; plain diffusers does not return them)")
    print("OK" if ok else "MISMATCH")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sd21", default=None, help="directory with unet/ and vae/ in diffusers layout")
    ap.add_argument("--size", type=int, default=128, help="test image edge (multiple of 8)")
    ap.add_argument("--tol", type=float, default=2e-4, help="max |oracle - diffusers| / max |diffusers| per stage")
    ap.add_argument("--emit", default=None, help="write the tiny-configuration fixture (inputs + oracle outputs; needs no diffusers)")
    ap.add_argument("--verify", default=None, help="check diffusers against a fixture written by --emit")
    args = ap.parse_args()
    if args.emit:
        import numpy as np
        np.savez_compressed(args.emit, **build_fixture())
        print(f"wrote {args.emit}")
        return 0
    if args.verify:
        return verify_fixture(args.verify, args.tol)
    try:
        from diffusers import AutoencoderKL, UNet2DConditionModel
    except ImportError:
        print("diffusers is not installed here: nothing to cross-check (this is expected in the build container)")
        return 2
    from oracle import sd21 as osd

    torch.manual_seed(0)
    ucfg, vcfg = osd.UNetCfg(), osd.VAECfg()
    if args.sd21:
        unet = UNet2DConditionModel.from_pretrained(args.sd21, subfolder="unet").eval()
        vae = AutoencoderKL.from_pretrained(args.sd21, subfolder="vae").eval()
    else:  # architecture-only check with random weights of the SD2.1 configuration (Appendix A of SURVEY.md)
        unet = UNet2DConditionModel(sample_size=96, in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
                                    down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",),
                                    up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3, layers_per_block=2, cross_attention_dim=1024,
                                    attention_head_dim=(5, 10, 20, 20), use_linear_projection=True).eval()
        vae = AutoencoderKL(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                            down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4, norm_num_groups=32,
                            sample_size=768).eval()
    usd = {k: v.float() for k, v in unet.state_dict().items()}
    vsd = {k: v.float() for k, v in vae.state_dict().items()}
    ok = True
    for name, sd, man in (("unet", usd, osd.unet_manifest(ucfg)), ("vae", vsd, osd.vae_manifest(vcfg))):
        missing, extra = sorted(set(man) - set(sd)), sorted(set(sd) - set(man))
        bad_shape = [k for k in man if k in sd and tuple(sd[k].shape) != tuple(man[k])]
        print(f"{name}: {len(sd)} tensors; missing {len(missing)}, unexpected {len(extra)}, shape mismatches {len(bad_shape)}")
        ok &= not (missing or extra or bad_shape)
    g = torch.Generator().manual_seed(1)
    rgb = torch.rand(1, 3, args.size, args.size, generator=g) * 2 - 1
    ctx = torch.randn(1, 2, 1024, generator=g)

    def report(stage, a, b):
        nonlocal ok
        d = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
        print(f"{stage:14s} rel max diff {d:.3e}")
        ok &= d <= args.tol

    with torch.no_grad():
        lat_ref = vae.quant_conv(vae.encoder(rgb))[:, :4] * 0.18215          # genpercept_pipeline.py:488-505 (mean of the posterior)
        report("vae.encode", osd.encode_rgb(vsd, vcfg, rgb), lat_ref)
        v_ref = unet(lat_ref, 1, encoder_hidden_states=ctx).sample             # genpercept_pipeline.py:455-457, t = 1
        report("unet(t=1)", osd.unet_forward(usd, ucfg, lat_ref, 1, ctx)[0], v_ref)
        dec_ref = vae.decoder(vae.post_quant_conv(-v_ref / 0.18215))           # scheduler beta = 1: pred_x0 = -v; :507-526
        report("vae.decode", osd.vae_decode(vsd, vcfg, -v_ref / 0.18215), dec_ref)
    print("OK" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
