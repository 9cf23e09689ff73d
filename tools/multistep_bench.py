#!/usr/bin/env python3
"""Throughput of the multi-step archs on one MI355X (not the headline metric: bench.py measures the one-step path BASELINE.json names).

    python tools/multistep_bench.py [--archs marigold|rgb_blending] [--denoise-steps 10] [--batch 4] [--res 768] [--precision bf16]

One JSON line: images/s, ms per batch, ms per denoising step (encode + n x UNet + decode on synthetic weights / images).

    python tools/multistep_bench.py --ensemble 10 [--res 768] [--iters 5] [--reduction median]

The ensembling stage alone (no engine): E members of one image held on the device, `ensemble_depth(max_res=50)` timed on the device route
(gp_ensemble_gather / gp_ensemble_reduce) and on the GENPERCEPT_HOST_ENSEMBLE=1 route (framework ops) in the same run, wall clock with a
device synchronise on both sides (the host optimiser is part of the stage), plus the optimiser alone and the reduce call alone."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _wall_ms(fn, iters):
    """median wall-clock ms of fn() over `iters` runs after one warm-up, a device synchronise on both sides of every run"""
    fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def ensemble_leg(a):
    import warnings
    import numpy as np
    from genpercept_amd import engine as ge
    from genpercept_amd import ensemble as gens
    from genpercept_amd.image_util import resize_max_res_size
    e, res = a.ensemble, a.res
    d = torch.device("cuda", 0)
    # members like the multi-step archs produce them: affine distortions of one smooth map plus a little independent noise
    g = torch.Generator().manual_seed(0)
    yy, xx = np.mgrid[0:res, 0:res].astype(np.float32)
    base = torch.from_numpy(0.5 + 0.4 * np.sin(xx / 97.0) * np.cos(yy / 71.0))
    sc, sh = 0.6 + 1.2 * torch.rand(e, generator=g), 0.4 * torch.rand(e, generator=g) - 0.2
    members = (base[None] * sc.view(e, 1, 1) + sh.view(e, 1, 1) + 0.01 * torch.randn((e, res, res), generator=g))[:, None].to(d)
    kw = dict(scale_invariant=True, shift_invariant=True, max_res=50, reduction=a.reduction)
    warnings.simplefilter("ignore")  # scipy's finite differences on the fp32 parameter vector
    os.environ.pop("GENPERCEPT_HOST_ENSEMBLE", None)
    ms_dev = _wall_ms(lambda: gens.ensemble_depth(members, **kw), a.iters)
    dev, _ = gens.ensemble_depth(members, **kw)
    os.environ["GENPERCEPT_HOST_ENSEMBLE"] = "1"
    ms_host = _wall_ms(lambda: gens.ensemble_depth(members, **kw), a.iters)
    ref, _ = gens.ensemble_depth(members, **kw)
    os.environ.pop("GENPERCEPT_HOST_ENSEMBLE", None)
    # the optimiser alone, on the arrays the gather hands it
    h, w = resize_max_res_size(res, res, 50) if res > 50 else (res, res)
    small, mm = ge.ensemble_gather(members[:, 0][None], h, w)
    flat, mmh = small.cpu().numpy().reshape(e, -1), mm.cpu().numpy()[0]
    t0 = time.perf_counter()
    for _ in range(a.iters):
        par = gens._fit(flat, mmh[:, 0], mmh[:, 1], True, a.reduction, 0.02, 2, 1e-3)
    ms_fit = (time.perf_counter() - t0) * 1e3 / a.iters
    # the reduce call alone (three launches), device events around 20 calls
    s32, t32 = par[None, :e].astype(np.float32), par[None, e:].astype(np.float32)
    s_dev, t_dev = torch.from_numpy(s32).to(d), torch.from_numpy(t32).to(d)
    m4 = members[:, 0][None].contiguous()
    ge.ensemble_reduce(m4, s_dev, t_dev, a.reduction, False)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(20):
        ge.ensemble_reduce(m4, s_dev, t_dev, a.reduction, False)
    ev1.record()
    torch.cuda.synchronize()
    ms_reduce = ev0.elapsed_time(ev1) / 20
    ideal = (4 * e + 12) * res * res  # members read once, pred written, read and written again by the normalise pass
    print(json.dumps({"ensemble": e, "res": res, "reduction": a.reduction, "iters": a.iters,
                      "ms_stage_device_route": round(ms_dev, 3), "ms_stage_host_switch_route": round(ms_host, 3), "ms_host_optimiser": round(ms_fit, 3),
                      "ms_reduce_call": round(ms_reduce, 4), "reduce_ideal_bytes": ideal, "reduce_gbps_of_ideal_bytes": round(ideal / ms_reduce / 1e6, 1),
                      "max_abs_diff_between_routes": float((dev - ref).abs().max())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default="marigold", choices=["marigold", "rgb_blending"])
    ap.add_argument("--denoise-steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32c"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ensemble", type=int, default=0, help="E > 0: time the test-time ensembling stage of one image alone (both routes) instead")
    ap.add_argument("--reduction", default="median", choices=["median", "mean"])
    a = ap.parse_args()
    if a.ensemble > 0:
        return ensemble_leg(a)
    from genpercept_amd import config as gc
    from genpercept_amd import weights as gw
    from genpercept_amd.engine import Engine
    from genpercept_amd.scheduler import DDIMSchedulerCustomized
    marigold = a.archs == "marigold"
    ucfg, vcfg = gc.UNetConfig(in_channels=8 if marigold else 4), gc.VAEConfig()
    eng = Engine(0, ucfg, vcfg, None, precision=a.precision)
    eng.load_state_dict("vae", gw.synth_state_dict(gw.vae_manifest(vcfg), seed=1))
    eng.load_state_dict("unet", gw.synth_state_dict(gw.unet_manifest(ucfg), seed=0))
    eng.set_context(torch.randn(2, ucfg.cross_attention_dim, generator=torch.Generator().manual_seed(2)))
    eng.finalize()
    sched = DDIMSchedulerCustomized(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                                    steps_offset=1, prediction_type="v_prediction")  # hf_configs/scheduler_beta_0.00085_0.012
    plan = sched.plan(a.denoise_steps)
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    rgb = torch.randint(0, 256, (a.batch, 3, a.res, a.res), dtype=torch.uint8, device=d, generator=g)
    noise = torch.randn(a.batch, 4, a.res // 8, a.res // 8, device=d, generator=g) if marigold else None
    t0 = time.perf_counter()
    out = eng.infer_steps(rgb, "depth", plan, noise)  # first pass folds the time embedding of every timestep of the schedule (host)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    eng.infer_steps(rgb, "depth", plan, noise)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = eng.infer_steps(rgb, "depth", plan, noise)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
    assert torch.isfinite(out).all()
    eng.set_profile(1)
    eng.infer_steps(rgb, "depth", plan, noise)
    tm = eng.timings()
    print(json.dumps({"archs": a.archs, "denoise_steps": a.denoise_steps, "batch": a.batch, "res": a.res, "dtype": a.precision,
                      "images_per_s": round(a.batch / dt, 2), "ms_per_batch": round(dt * 1e3, 2),
                      "ms_encode": round(tm["ms_encode"], 2), "ms_loop": round(tm["ms_unet"], 2), "ms_per_step": round(tm["ms_unet"] / a.denoise_steps, 3),
                      "ms_decode": round(tm["ms_head"], 2), "first_call_s": round(first, 2)}))


if __name__ == "__main__":
    main()
