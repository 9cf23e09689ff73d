#!/usr/bin/env python3
"""Kernel-only timing of flash_attn64 at the UNet's four levels and of flash_attn512 at the VAE's mid block (batch 4): HIP events around
back-to-back launches.
--hd512-split: the contract precision's VAE attention instead -- flash_attn512_split (+ its operand planes) against the unfused chain (head
split, logits GEMM, softmax, P.V GEMM, merge) of the same build at batch 4, T = 9216, and the fused kernel alone at B = 1, T = 36864, which
the unfused chain cannot serve within 8 GiB; per-launch times from the engine's launch log (profiling level 3) of gp_vae_mid_attention, with
the shader clock / socket power sampled over the timed calls.  Prints the result as JSON; --out FILE also writes it there
(profiles/r08_flash512_split.json is one such run).
usage: python tools/attn_bench.py [--hd512-only | --hd512-split [--out FILE]]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpercept_amd import engine as e  # noqa: E402


def hd512(d):
    for b, t in ((4, 9216), (1, 9216), (4, 2304)):
        c = 512
        g = torch.Generator().manual_seed(t)
        qk = (torch.randn(b, t, 2 * c, generator=g)).to(d).to(e.act_dtype())
        vt = torch.randn(b, c, t, generator=g).to(d).to(e.act_dtype())
        scale = 2.0 / c ** 0.5
        for _ in range(2):
            e.flash_attention_hd512(qk[:, :, :c], qk[:, :, c:], vt, scale)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                e.flash_attention_hd512(qk[:, :, :c], qk[:, :, c:], vt, scale)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 5)
        fl = 4.0 * b * t * t * c
        print(f"hd512 B={b} T={t:5d}  {best * 1e3:8.1f} us  {fl / best / 1e9:7.1f} TFLOP/s", flush=True)


CHAIN = ("c_heads_split", "c_softmax_split", "c_heads_merge_split", "c_qkv_planes", "flash_attn512_split")


def hd512_split_leg(switch, b, hw, passes=3):
    """median per-launch ms of the attention core inside gp_vae_mid_attention, GENPERCEPT_C_FLASH512 = switch (None: unset, the planner decides)"""
    from bench import ClockPowerSampler
    from genpercept_amd import config as gc
    from genpercept_amd import weights as gw
    from genpercept_amd.engine import Engine
    if switch is None:
        os.environ.pop("GENPERCEPT_C_FLASH512", None)
    else:
        os.environ["GENPERCEPT_C_FLASH512"] = switch
    vcfg = gc.VAEConfig()
    eng = Engine(0, gc.UNetConfig(), vcfg, None, precision="fp32c")
    try:
        eng.load_state_dict("vae", gw.synth_state_dict(gw.vae_manifest(vcfg), seed=1))
        eng.finalize()
        x = torch.randn(b, 512, hw, hw, generator=torch.Generator().manual_seed(hw)).cuda()
        eng.vae_mid_attention(x, decoder=True)
        torch.cuda.synchronize()
        eng.set_profile(3)
        with ClockPowerSampler("cuda:0") as smp:
            for _ in range(passes):
                eng.vae_mid_attention(x, decoder=True)
            torch.cuda.synchronize()
        # the marks of gp_vae_mid_attention calls accumulate, n per call; the log prices a launch by the NEXT mark, so it has passes * n - 1 rows and
        # call k's launches are rows k n .. k n + n - 2 (a call's last launch, the layout conversion, ends at the next call's first mark)
        log = eng.launch_log()
        n = (len(log) + 1) // passes
        assert n * passes == len(log) + 1, (len(log), passes)
        runs = [log[k * n:k * n + n - 1] for k in range(passes)]
        assert all(r[i][2] == runs[0][i][2] for r in runs for i in range(n - 1))
        idx = [i for i, r in enumerate(runs[0]) if r[2].split()[0] in CHAIN]
        rows = []
        for i in range(idx[0], idx[-1] + 1):
            ms = sorted(r[i][0] for r in runs if len(r) > i)
            rows.append({"launch": runs[0][i][2], "ms": round(ms[len(ms) // 2], 4)})
        t = hw * hw
        total = sum(r["ms"] for r in rows)
        return {"switch": switch, "B": b, "T": t, "launches": rows, "ms": round(total, 4), "tflops_algorithmic": round(4.0 * b * t * t * 512 / total / 1e9, 1),
                "pool_bytes": eng.pool_bytes(), "clock_power": smp.summary()}
    finally:
        eng.close()


def hd512_split():
    out = {"what": "contract precision, VAE mid-block attention core inside gp_vae_mid_attention: launch log (level 3), median of 3 calls, measured once",
           "unfused_b4_T9216": hd512_split_leg("0", 4, 96), "fused_b4_T9216": hd512_split_leg("1", 4, 96), "fused_b1_T36864": hd512_split_leg(None, 1, 192)}
    out["fused_over_unfused_T9216"] = round(out["fused_b4_T9216"]["ms"] / out["unfused_b4_T9216"]["ms"], 3)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)
    for k in ("unfused_b4_T9216", "fused_b4_T9216", "fused_b1_T36864"):
        print(k, out[k]["ms"], "ms", [(r["launch"].split()[0], r["ms"]) for r in out[k]["launches"]], out[k]["clock_power"], flush=True)
    print("fused / unfused at T = 9216:", out["fused_over_unfused_T9216"], flush=True)


def main():
    d = torch.device("cuda", 0)
    if "--hd512-split" in sys.argv:
        hd512_split()
        return
    hd512(d)
    if "--hd512-only" in sys.argv:
        return
    for t, heads in ((9216, 5), (2304, 10), (576, 20), (144, 20)):
        b, c = 4, heads * 64
        tpad = (t + 63) // 64 * 64
        g = torch.Generator().manual_seed(t)
        qk = torch.randn(b, t, 2 * c, generator=g).to(d).to(e.act_dtype())
        vt = torch.zeros(b, c, tpad, dtype=e.act_dtype(), device=d)
        vt[:, :, :t] = torch.randn(b, c, t, generator=g).to(d).to(e.act_dtype())
        for _ in range(3):
            e.flash_attention(qk[:, :, :c], qk[:, :, c:], vt, heads)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                e.flash_attention(qk[:, :, :c], qk[:, :, c:], vt, heads)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20)
        fl = 4.0 * b * heads * t * t * 64
        print(f"T={t:5d} heads={heads:2d}  {best * 1e3:8.1f} us  {fl / best / 1e9:7.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
