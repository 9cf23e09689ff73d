#!/usr/bin/env python3
"""Headline benchmark: images/sec of the one-step GenPercept path (depth head: SD2.1 VAE encoder -> UNet (t=1) -> VAE
decoder) at 768x768, bf16 elements / fp32 accumulate, batch 4 per GPU, synthetic RGB resident in HBM, random-init weights
of the exact SD2.1 architecture (BASELINE.json configs[1]; no checkpoints exist offline).

  python bench.py --gpus 1 --steps 5 --warmup 2
  python bench.py --gpus 1 --steps 5 --warmup 2 --full   # + the other precisions, profiles, roofline, CPU baseline and parity
  python bench.py --gpus 8 ...                           # spawns its own 8 ranks (re-executes itself under torch.distributed.run)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one pass of the hot path over one batch per GPU (gp_infer).  N > 1: one process per GPU, the batch of N*B
independent images is sharded contiguously, weights replicated, no collective on the data path ("weak" scaling); the step
then ends with the optional result gather of BASELINE.json configs[4] (RCCL gather of the fp32 maps to rank 0 over xGMI),
inside the timed region.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: it builds the engine of --precision, runs the warm-up and the timed steps,
writes the maps of --dump-outputs when it is given and prints the line (`value`, `ms_per_step`, per-step min / median / max,
`clock_power`).  Everything else runs only with --full, each part still switchable off by its --no-* option, and is null
(or absent) in a plain line:
  gather_ms    N > 1: the result gather alone (same tensors, 5 calls), max over ranks.
  roofline     the dominant kernel, conv3x3_halo3_kernel: algorithmic flops of its launches / their summed duration, from HIP events
               on the engine's stream in an instrumented pass right after the timed region (events around ~300 launches would perturb
               the timed region itself); `family_*` = the whole implicit-GEMM conv / linear family; `peak` = the nominal 2.5 PFLOP/s,
               `peak_measured` = this chip's own back-to-back-MFMA rate (gp_mfma_peak_tflops) measured in the same run.
  cpu_baseline the fp32 oracle (oracle/, a restatement: kind "port") timed on the host cores at the benched size: ONE 768x768 image --
               image 0 of the benched batch, so the same run also reports
  parity       HIP map vs that fp32 oracle map at the benched size (mean / max |delta| on [0,1], rel-rms, AbsRel after the reference's least-squares
               alignment) for every precision timed in the run: the benched bf16, the fp16 library (`value_fp16`) and the CONTRACT precision
               (`value_fp32c`: fp32 storage + split-bf16 matrix products, what torch_dtype=float32 selects -- the build inside north_star's
               1e-3 under both readings); `within_1e-3` = {precision: {mean_abs, rel_rms}} (same K steps, same barriers for each leg).
  stages       per-stage times from a pass with FOUR events only (profiling level 1); the per-kernel sums of `roofline` come from a second,
               per-launch-instrumented pass whose ~500 event pairs cost ~7 % and must not leak into `unet_mfma_util`.
  value_fp16, value_fp32c
               N = 1, --precision bf16: the fp16 library and the contract precision, each built and timed like the headline leg.

--dump-outputs DIR writes, on rank 0, the maps each timed leg returned in its LAST timed step as DIR/<mode>_<precision>.npy (float32, [B,C,H,W];
rank 0's shard, or the gathered batch when N > 1).  Inputs, weights and context are seeded, so two builds run with the same arguments can be
compared array for array.  The files hold at most DUMP_BUDGET_BYTES together: a leg whose map exceeds its equal share is stored as a fixed,
seeded sample (flat indices torch.randperm(numel, seed DUMP_SEED)[:k], sorted; 1-D).  The set of legs, and so of files, does not depend on
--full: a plain run with --dump-outputs also runs the fp16 and contract-precision legs (same warm-up and steps) for their maps, and reports
nothing of them in its line.
"""
import argparse
import contextlib
import json
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TFLOP_PER_IMAGE_768_DPT = 5.473  # VAE-enc 2.609 + UNet 2.137 + DPT head 0.726
TFLOP_PER_IMAGE_768 = 10.50  # VAE-enc 2.609 + UNet 2.137 + VAE-dec 5.754 (2*MAC of conv/linear/QK^T/PV)
PEAK_BF16_TFLOPS = 2500.0    # MI355X dense bf16 / fp16 MFMA (MI355X_MICROARCH.md)
DUMP_BUDGET_BYTES = 64 << 20  # --dump-outputs: all arrays together
DUMP_SEED = 0


def synthetic_rgb(batch: int, res: int, seed: int, device) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    noise = torch.randint(0, 256, (batch, 3, res, res), generator=g, dtype=torch.uint8).float()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, res), torch.linspace(0, 1, res), indexing="ij")
    smooth = torch.stack([yy, xx, (yy + xx) / 2])[None] * 255.0
    return (0.5 * noise + 0.5 * smooth).round().clamp(0, 255).to(torch.uint8).to(device)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def source_build_id() -> str:
    """sha1 over the HIP sources + the C-ABI header: what a PMC / profile artefact must carry to count as THIS build's (there is no .git on
    the GPU box)."""
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(ROOT, "genpercept_amd", "csrc")
    for f in sorted(os.listdir(d)) + ["../../include/genpercept_hip.h"]:
        if f.endswith((".hip", ".h")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:12]


def parity_vs(ref, out) -> dict:
    """HIP map vs the fp32 oracle map (both [C,H,W] on the host, values in [0,1]) under BOTH readings of north_star's "within 1e-3 rel":
    mean_abs = mean |delta| on the [0,1] map (max_abs beside it) and rel_rms = rms(out - ref) / rms(ref - mean(ref)), the deviation relative
    to the map's own signal; plus AbsRel after the reference's least-squares alignment (eval.py protocol: src/util/alignment.py:29-76,
    metric.py:34-44), channel 0."""
    import numpy as np
    from genpercept_amd.eval_metrics import abs_relative_difference, align_depth_least_square
    r, o = ref.double().numpy(), out.double().numpy()
    d = np.abs(o - r)
    gt = r[0].clip(1e-3, None)
    aligned, _, _ = align_depth_least_square(gt, o[0], np.ones_like(gt, dtype=bool))
    rel_rms = float(np.sqrt(((o - r) ** 2).mean()) / (np.sqrt(((r - r.mean()) ** 2).mean()) + 1e-30))
    return {"mean_abs": float(d.mean()), "max_abs": float(d.max()), "rel_rms": rel_rms,
            "absrel_ls": float(abs_relative_difference(np.clip(aligned, 1e-3, None), gt)), "ref": "fp32 oracle (oracle/), image 0 of the benched batch",
            "within_1e-3": {"mean_abs": bool(d.mean() <= 1e-3), "rel_rms": bool(rel_rms <= 1e-3)}}


def dump_outputs(out_dir: str, arrays: dict) -> dict:
    """Write each host tensor of `arrays` as out_dir/<name>.npy in float32 within DUMP_BUDGET_BYTES in all (module docstring); returns
    {name: {"shape": full shape, "stored": elements written, "sampled": bool}}."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1) // 4  # float32 elements per array
    info = {}
    for name, t in arrays.items():
        flat = t.detach().float().cpu().contiguous().reshape(-1)
        sampled = flat.numel() > share
        if sampled:
            idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(DUMP_SEED))[:share].sort().values
            a = flat[idx].numpy()
        else:
            a = flat.numpy().reshape(tuple(t.shape))
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32, copy=False))
        info[name] = {"shape": list(t.shape), "stored": int(a.size), "sampled": sampled}
    return info


def respawn_under_torchrun(n: int):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run --nproc-per-node N bench.py ...`."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execv(sys.executable, cmd)


def device_sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


class ClockPowerSampler:
    """Socket power and shader clock of the benched GPU, read from the amdgpu hwmon files while the timed steps run (a thread that sleeps 20 ms
    between two small sysfs reads: nothing on the launch path).  The pool's boxes differ by more than a round's gains and the chip is
    power-limited under this load (profiles/r04_power_samples.json), so the line carries the clock / power it was measured at: a +-2 % change
    can then be told from a slower box.  Every field is null where the files are not readable."""

    def __init__(self, dev):
        self.rows, self.stop, self.thread, self.files = [], False, None, None
        try:
            import glob
            want = None
            try:
                pr = torch.cuda.get_device_properties(torch.device(dev))
                want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
            except Exception:
                pass
            cands = []
            for hw in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
                pw = next((f for f in (hw + "/power1_average", hw + "/power1_input") if os.path.exists(f)), None)
                fq = hw + "/freq1_input"
                if pw and os.path.exists(fq):
                    bdf = os.path.basename(os.path.realpath(os.path.join(hw, "..", "..")))
                    cands.append((bdf, pw, fq))
            pick = [c for c in cands if want and c[0].startswith(want)] or cands
            if pick:
                self.files = pick[0]
        except Exception:
            self.files = None

    def _run(self):
        _, pw, fq = self.files
        while not self.stop:
            try:
                self.rows.append((int(open(pw).read()) / 1e6, int(open(fq).read()) / 1e6))
            except Exception:
                pass
            time.sleep(0.02)

    def __enter__(self):
        if self.files:
            import threading
            self.thread = threading.Thread(target=self._run, daemon=True)
            self.thread.start()
        return self

    def __exit__(self, *a):
        self.stop = True
        if self.thread:
            self.thread.join(timeout=1.0)

    def summary(self):
        if not self.rows:
            return {"samples": 0, "power_w_mean": None, "sclk_mhz_mean": None, "note": "amdgpu hwmon power1_average / freq1_input not readable here"}
        pw, fq = [r[0] for r in self.rows], [r[1] for r in self.rows]
        return {"samples": len(self.rows), "power_w_mean": round(sum(pw) / len(pw), 1), "power_w_max": round(max(pw), 1),
                "sclk_mhz_mean": round(sum(fq) / len(fq), 1), "sclk_mhz_min": round(min(fq), 1),
                "source": f"amdgpu hwmon (sysfs) of PCI device {self.files[0]}, every 20 ms over the timed steps"}


def timed_steps(step, warmup: int, steps: int, dev, stats: dict = None):
    """The timing contract: `warmup` untimed steps, then EXACTLY `steps` steps bracketed by barrier + device synchronize on both sides; the
    elapsed time is the MAX over ranks.  Returns (seconds, last step's result).  With `stats` (a dict) on a GPU, ONE event is recorded per step
    on the stream the engine launches on (torch's current stream) -- not per launch -- and the per-step durations (this rank's) and the
    clock / power samples of the timed region are left in it."""
    from genpercept_amd import distributed as gd
    o = None
    for _ in range(warmup):
        o = step()
    on_gpu = torch.device(dev).type == "cuda"
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if (on_gpu and stats is not None) else None
    device_sync(dev)
    gd.barrier()
    device_sync(dev)
    with ClockPowerSampler(dev) if evs is not None else contextlib.nullcontext() as smp:
        t0 = time.perf_counter()
        if evs is not None:
            evs[0].record()
        for i in range(steps):
            o = step()
            if evs is not None:
                evs[i + 1].record()
        device_sync(dev)
        gd.barrier()
        el = time.perf_counter() - t0
    if evs is not None:
        per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
        stats["ms_per_step_min"] = round(per[0], 3)
        stats["ms_per_step_median"] = round(per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2]), 3)
        stats["ms_per_step_max"] = round(per[-1], 3)
        stats["clock_power"] = smp.summary()
    return gd.max_over_ranks(el, dev), o


def main(argv=None, engine_factory=None, device=None):
    """`engine_factory(local_rank, precision) -> engine` and `device` exist for the CPU (gloo) test of the N > 1 path, which runs this very
    function with a stub engine (tests/test_host.py); the product run passes neither."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4, help="images per GPU per step")
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--mode", default="depth", help="depth | normal | ... (VAE-decoder head); use --head dpt for the DPT disparity head")
    ap.add_argument("--head", default="vae", choices=["vae", "dpt"], help="BASELINE.json configs[1]/[2] = vae (depth/normal), configs[3] = dpt")
    ap.add_argument("--cpu-res", type=int, default=768, help="edge of the single image timed on the CPU oracle (the benched size)")
    ap.add_argument("--cpu-threads", type=int, default=32, help="torch CPU threads for the baseline leg (256 oversubscribes badly)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32c"],
                    help="precision of the benched engine (bf16 = BASELINE.json's dtype; fp16 = the reference's --half_precision; fp32c = the contract "
                         "precision: fp32 storage + split-bf16 matrix products, what torch_dtype=float32 selects)")
    ap.add_argument("--no-gather", action="store_true", help="N > 1: leave the result maps on their GPUs")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline (module docstring): gather_ms, the profiled passes (stages, roofline), "
                         "the fp16 and contract-precision legs, the CPU oracle baseline and parity; the --no-* options below drop single parts")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU oracle baseline and parity")
    ap.add_argument("--no-profile", action="store_true", help="--full: skip the profiled passes (stages, roofline, measured MFMA peaks)")
    ap.add_argument("--no-fp16", action="store_true", help="skip the second timed leg with the fp16 library (--full, or --dump-outputs: its map)")
    ap.add_argument("--no-fp32c", action="store_true", help="skip the third timed leg with the contract precision (fp32 storage, split-bf16 products; --full, or --dump-outputs: its map)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write each timed leg's last-step maps as DIR/<mode>_<precision>.npy (float32, <= 64 MB in all; see the module docstring)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args.gpus)  # does not return

    from genpercept_amd import config as gc
    from genpercept_amd import distributed as gd
    from genpercept_amd import engine as ge
    from genpercept_amd import weights as gw
    from genpercept_amd.engine import Engine

    rank, local_rank, world = gd.init_process_group()
    if world != max(args.gpus, 1):
        raise SystemExit(f"bench.py: WORLD_SIZE {world} != --gpus {args.gpus} (the multi-GPU configuration would silently not be measured)")
    n_gpus = world
    if device is None:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    else:
        dev = torch.device(device)

    if world > 1:  # every rank synthesises the same weights on the host: share the cores instead of oversubscribing them N times
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))
    dpt = args.head == "dpt"
    if dpt:
        args.mode = "disparity"
    ucfg, vcfg = gc.UNetConfig(has_out=not dpt), gc.VAEConfig()
    dcfg = gc.DPTConfig() if dpt else None
    t0 = time.time()
    usd = vsd = dsd = None
    if engine_factory is None:
        usd = gw.synth_state_dict(gw.unet_manifest(ucfg), seed=0)
        vsd = gw.synth_state_dict(gw.vae_manifest(vcfg), seed=1)
        dsd = gw.synth_state_dict(gw.dpt_manifest(dcfg), seed=3) if dpt else None
    ctx = torch.randn(2, ucfg.cross_attention_dim, generator=torch.Generator().manual_seed(2))

    def build_engine(precision):
        if engine_factory is not None:
            return engine_factory(local_rank, precision)
        e = Engine(local_rank, ucfg, vcfg, dcfg, precision=precision)
        e.load_state_dict("vae", vsd)
        e.load_state_dict("unet", usd)
        if dpt:
            e.load_state_dict("dpt", dsd)
        e.set_context(ctx)
        e.finalize()
        return e

    eng = build_engine(args.precision)
    t_load = time.time() - t0
    lib_prec = ge.ENGINE_PRECISIONS[args.precision][0]  # the element-type library behind the benched precision (fp32c lives in the bf16 library)

    n_total = args.batch * n_gpus
    lo, hi = gd.shard_range(n_total, rank, n_gpus)
    rgb = synthetic_rgb(n_total, args.res, 1234, "cpu")[lo:hi].to(dev)
    do_gather = n_gpus > 1 and not args.no_gather

    dumps = {}  # --dump-outputs: {"<mode>_<precision>": last timed step's maps}, rank 0 only

    def timed(engine, precision):
        """one step = one pass of the hot path over this rank's shard (+ the result gather of configs[4] when N > 1)"""
        def step():
            o = engine.infer(rgb, args.mode)
            if do_gather:
                return gd.gather_results(o, n_total, dst=0)  # rank 0: [N*B, C, H, W]; others: None
            return o
        st = {}
        el, o = timed_steps(step, args.warmup, args.steps, dev, st)
        timed.stats = st
        if o is not None:
            assert torch.isfinite(o).all()
            if do_gather:
                assert o.shape[0] == n_total
            if args.dump_outputs and rank == 0:
                dumps[f"{args.mode}_{precision}"] = o.detach().cpu()
        return el, o

    elapsed, out = timed(eng, args.precision)
    step_stats = timed.stats
    ms_per_step = elapsed / args.steps * 1e3
    images = n_total * args.steps
    value = images / elapsed
    out0 = out[0].float().cpu() if (args.full and out is not None and rank == 0) else None  # image 0 of the benched batch: the parity sample

    gather_ms = None
    if do_gather and args.full:  # the gather alone (same tensors), max over ranks
        loc = eng.infer(rgb, args.mode)
        gather_ms = round(timed_steps(lambda: gd.gather_results(loc, n_total, dst=0), 0, 5, dev)[0] / 5 * 1e3, 3)

    roofline = None
    stages = None
    if args.full and not args.no_profile:
        eng.set_profile(1)  # four events per pass: the stage times are not perturbed by per-launch instrumentation
        eng.reset_timings()
        eng.infer(rgb, args.mode)
        tm1 = eng.timings()
        eng.set_profile(2)  # an event pair around every conv / GEMM / attention launch: their summed durations
        eng.reset_timings()
        eng.infer(rgb, args.mode)
        tm = eng.timings()
        halo_exec = eng.halo_executed_flops() if hasattr(eng, "halo_executed_flops") else tm["flops_halo"]
        eng.set_profile(0)
        peak_meas = ge.mfma_peak_tflops(local_rank, lib_prec) if rank == 0 else None
        peak_meas16 = ge.mfma_peak_tflops_shape(local_rank, 1, lib_prec) if rank == 0 else None  # the dominant kernel's own MFMA shape
        # the dominant kernel's inner loop in isolation (gp_mfma_lds_probe, ~10 ms each): 16 MFMAs + 8 fragment reads per wave at two waves per SIMD,
        # alone / with the per-step barrier, the weight stream and the halo stream of the real kernel (constant operand bits: an upper bound)
        loop_probe = None
        if rank == 0:
            try:
                loop_probe = {"mfma_and_fragment_reads": round(ge.mfma_lds_probe(local_rank, 8, 2, 0, lib_prec), 1),
                              "plus_barrier_weight_and_halo_streams": round(ge.mfma_lds_probe(local_rank, 8, 2, 19, lib_prec), 1)}
            except Exception:
                loop_probe = None
        scale = (args.res / 768.0) ** 2 * ((TFLOP_PER_IMAGE_768_DPT / TFLOP_PER_IMAGE_768) if dpt else 1.0)
        if tm["ms_halo"] > 0:
            ach = tm["flops_halo"] / (tm["ms_halo"] * 1e-3) / 1e12
            fam = tm["flops_igemm"] / (tm["ms_igemm"] * 1e-3) / 1e12
            # HBM traffic of the dominant kernel: PMC passes (separate --pmc runs; FETCH_SIZE doubled on gfx950) are a different command
            # (tools/gpu_pmc_traffic.sh); their summary counts only when it was taken from THESE sources (build id = sha1 of csrc/)
            bid = source_build_id()
            traffic, traffic_note = None, f"null: no PMC summary of this build ({bid}) under profiles/ (tools/gpu_pmc_traffic.sh collects it)"
            try:
                import glob
                cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_summary*.json")), reverse=True)  # newest round first
                seen = []
                for tf in cands:
                    tj = json.load(open(tf))
                    seen.append(f"{os.path.basename(tf)}: {tj.get('build_id')}")
                    if tj.get("build_id") != bid:
                        continue
                    sel = lambda d: sum(v["sum_kb"] for k, v in d.items() if "conv3x3_halo3" in k)  # noqa: E731
                    nd = sum(v["dispatches"] for k, v in tj["FETCH_SIZE"].items() if "conv3x3_halo3" in k)
                    traffic = round((2.0 * sel(tj["FETCH_SIZE"]) + sel(tj["WRITE_SIZE"])) * 1024.0 / max(nd, 1))
                    traffic_note = f"HBM bytes per launch, PMC (2*FETCH_SIZE + WRITE_SIZE), same build ({bid}), profiles/{os.path.basename(tf)}"
                    break
                else:
                    if seen:
                        traffic_note = f"null: no PMC summary under profiles/ is of this build ({bid}); newest: {seen[0]}"
            except Exception:
                pass
            # matrix-pipe busy fraction per kernel from the SQ counters (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE ... in their own run:
            # tools/sessions/gpu_r06_pmc.sh); like `traffic` it only counts when it was taken from THESE sources
            mfma_busy, mfma_busy_note = None, f"null: no SQ-counter summary of this build ({bid}) under profiles/ (tools/sessions/gpu_r06_pmc.sh collects it)"
            try:
                import glob
                for mf in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_mfma_summary*.json")), reverse=True):
                    mj = json.load(open(mf))
                    if mj.get("build_id") != bid:
                        continue
                    pick = {}
                    for k, v in mj["kernels"].items():
                        if "mfma_busy_fraction" in v and any(t in k for t in ("conv3x3_halo3", "pgemm_kernel", "flash_attn64", "flash_attn512", "igemm_kernel", "conv_img")):
                            pick[k] = {"mfma_busy_fraction": v["mfma_busy_fraction"], "dispatches": v["dispatches"],
                                       "valu_per_mfma_busy_cycle": v.get("valu_per_mfma_busy_cycle"), "lds_bank_conflict_cycles": v.get("SQ_LDS_BANK_CONFLICT")}
                    halo = [(v["SQ_VALU_MFMA_BUSY_CYCLES"], v["GRBM_GUI_ACTIVE"]) for k, v in mj["kernels"].items() if "conv3x3_halo3" in k and v.get("GRBM_GUI_ACTIVE")]
                    mfma_busy = {"dominant_kernel_family": round(sum(a for a, _ in halo) / (sum(b for _, b in halo) / 8.0 * 1024.0), 4) if halo else None,
                                 "per_kernel": pick}
                    mfma_busy_note = (f"SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 256 CUs x 4 SIMDs) per kernel, rocprofv3 --pmc, same build ({bid}), "
                                      f"profiles/{os.path.basename(mf)}")
                    break
            except Exception:
                pass
            roofline = {"bound": "mfma", "kernel": f"conv3x3_halo3_kernel (3x3 stride-1 convs of the large maps, v_mfma_f32_16x16x32_{'f16' if args.precision == 'fp16' else 'bf16'})",
                        "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
                        "peak_measured": round(peak_meas, 1) if peak_meas and peak_meas > 0 else None,
                        "frac_of_measured_peak": round(ach / peak_meas, 4) if peak_meas and peak_meas > 0 else None,
                        "peak_measured_16x16x32": round(peak_meas16, 1) if peak_meas16 and peak_meas16 > 0 else None,
                        "inner_loop_probe": loop_probe,
                        # `achieved` counts ALGORITHMIC flops (2 M N 9 Cin).  The x2-upsample convs run as four 2x2-tap phase convolutions and execute 4/9 of theirs:
                        # `executed_achieved` is the rate of the arithmetic actually issued (what the matrix pipe sustains), `achieved` the useful-work rate
                        "executed_achieved": round(halo_exec / (tm["ms_halo"] * 1e-3) / 1e12, 2), "executed_frac": round(halo_exec / (tm["ms_halo"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                        "traffic": traffic, "traffic_note": traffic_note,
                        "mfma_busy_fraction": mfma_busy, "mfma_busy_note": mfma_busy_note,
                        "launches": tm["n_halo"], "flops_per_launch_avg": tm["flops_halo"] / max(tm["n_halo"], 1),
                        "avg_launch_ms": tm["ms_halo"] / max(tm["n_halo"], 1), "sum_ms": round(tm["ms_halo"], 3),
                        "family_kernel": "conv3x3_halo3_kernel + pgemm_kernel + igemm_kernel (every conv / linear launch)",
                        "family_achieved": round(fam, 2), "family_frac": round(fam / PEAK_BF16_TFLOPS, 4), "family_launches": tm["n_igemm"],
                        "family_sum_ms": round(tm["ms_igemm"], 3),
                        "attn_achieved": round(tm["flops_attn"] / max(tm["ms_attn"], 1e-9) / 1e9, 2), "attn_launches": tm["n_attn"],
                        "pipeline_achieved": round(TFLOP_PER_IMAGE_768 * scale * args.batch / (ms_per_step * 1e-3), 2),
                        "pipeline_frac": round(TFLOP_PER_IMAGE_768 * scale * args.batch / (ms_per_step * 1e-3) / PEAK_BF16_TFLOPS, 4)}
        stages = {"ms_encode": round(tm1["ms_encode"], 3), "ms_unet": round(tm1["ms_unet"], 3), "ms_head": round(tm1["ms_head"], 3),
                  "ms_unet_per_launch_instrumented": round(tm["ms_unet"], 3),
                  "ms_igemm_sum": round(tm["ms_igemm"], 3), "ms_attn_sum": round(tm["ms_attn"], 3), "kernel_launches": tm["n_launches"],
                  # executed conv / linear / attention flops; below SURVEY's 10.50 because the 2-token cross-attention is folded (F6)
                  "executed_tflop_per_image": round((tm["flops_igemm"] + tm["flops_attn"]) / 1e12 / args.batch, 3),
                  # second half of BASELINE.json's metric: UNet stage alone, 2.137 ALGORITHMIC TFLOP per 768x768 image
                  "unet_mfma_util": round(2.137 * (args.res / 768.0) ** 2 * args.batch / (max(tm1["ms_unet"], 1e-9) * 1e-3) / PEAK_BF16_TFLOPS, 4)}

    # ---- second timed leg: the fp16 library (the build that meets north_star's 1e-3), same steps / barriers ---------------------------
    fp16 = None
    out0_f16 = None
    # a plain run with --dump-outputs runs the fp16 and contract-precision legs too, for their maps alone: the dumped set does not depend on --full
    other_legs = args.precision == "bf16" and n_gpus == 1 and (args.full or args.dump_outputs is not None)
    if other_legs and not args.no_fp16:  # (N > 1 measures scaling of the headline dtype only: no second engine build per rank)
        eng.close()
        eng = build_engine("fp16")
        el16, o16 = timed(eng, "fp16")
        if args.full:
            if o16 is not None and rank == 0:
                out0_f16 = o16[0].float().cpu()
            fp16 = {"value_fp16": round(images / el16, 3), "ms_per_step_fp16": round(el16 / args.steps * 1e3, 3),
                    "ms_per_step_fp16_min": timed.stats.get("ms_per_step_min"), "ms_per_step_fp16_median": timed.stats.get("ms_per_step_median")}
            if rank == 0 and dev.type == "cuda":  # the chip's own back-to-back-MFMA rate with fp16 operands (the bf16 figure is roofline.peak_measured): same instruction
                pk16 = ge.mfma_peak_tflops(local_rank, "fp16")  # count, lower sustained clock -- the guide's micro-benchmarks show the same 6-9 % gap
                fp16["peak_measured_fp16"] = round(pk16, 1) if pk16 and pk16 > 0 else None
            if not args.no_profile:
                eng.set_profile(1)
                eng.reset_timings()
                eng.infer(rgb, args.mode)
                t16 = eng.timings()
                eng.set_profile(0)
                fp16["stages_fp16"] = {"ms_encode": round(t16["ms_encode"], 3), "ms_unet": round(t16["ms_unet"], 3), "ms_head": round(t16["ms_head"], 3)}

    # ---- third timed leg: the CONTRACT precision (gp_set_precision(GP_PREC_CONTRACT): fp32 storage, split-bf16 matrix products -- three MFMAs
    # per product), the build torch_dtype=float32 selects and the one inside north_star's 1e-3 under BOTH readings; same steps / barriers -------
    fp32c = None
    out0_c = None
    if other_legs and not args.no_fp32c:
        eng.close()
        eng = build_engine("fp32c")
        elc, oc = timed(eng, "fp32c")
        if args.full:
            if oc is not None and rank == 0:
                out0_c = oc[0].float().cpu()
            fp32c = {"value_fp32c": round(images / elc, 3), "ms_per_step_fp32c": round(elc / args.steps * 1e3, 3),
                     "ms_per_step_fp32c_min": timed.stats.get("ms_per_step_min"), "ms_per_step_fp32c_median": timed.stats.get("ms_per_step_median")}
            if not args.no_profile:
                eng.set_profile(1)
                eng.reset_timings()
                eng.infer(rgb, args.mode)
                tc = eng.timings()
                eng.set_profile(0)
                fp32c["stages_fp32c"] = {"ms_encode": round(tc["ms_encode"], 3), "ms_unet": round(tc["ms_unet"], 3), "ms_head": round(tc["ms_head"], 3)}
                # useful (algorithmic) flops per second of the whole pass; the matrix cores execute three times that in this precision
                sc = (args.res / 768.0) ** 2 * ((TFLOP_PER_IMAGE_768_DPT / TFLOP_PER_IMAGE_768) if dpt else 1.0)
                fp32c["pipeline_achieved_fp32c"] = round(TFLOP_PER_IMAGE_768 * sc * args.batch / (elc / args.steps), 2)
                fp32c["pipeline_executed_frac_fp32c"] = round(3.0 * TFLOP_PER_IMAGE_768 * sc * args.batch / (elc / args.steps) / PEAK_BF16_TFLOPS, 4)

    cpu = None
    parity = None
    if args.full and rank == 0 and n_gpus == 1 and not args.no_cpu and not dpt:
        from oracle import pipeline as opipe  # CPU baseline leg only: the oracle is the checker and the reported baseline, never the product
        from oracle import sd21 as osd
        nthr = max(1, min(os.cpu_count(), args.cpu_threads))
        torch.set_num_threads(nthr)
        r = args.cpu_res
        same = r == args.res
        x = opipe.normalize_rgb(synthetic_rgb(n_total, r, 1234, "cpu")[:1] if same else synthetic_rgb(1, r, 99, "cpu"))
        with torch.no_grad():
            t0 = time.perf_counter()
            ref = opipe.single_infer(vsd, osd.VAECfg(), usd, osd.UNetCfg(), x, ctx, args.mode)
            dt = time.perf_counter() - t0
        if same and out0 is not None:  # the map just timed on the GPU against the map just timed on the CPU: same image, same weights
            parity = {args.precision: parity_vs(ref[0], out0),
                      "tolerance": "north_star: 'within 1e-3 rel of the reference', reported under two metrics per library: mean_abs = mean |HIP - oracle| "
                                   "on the [0,1] map; rel_rms = rms(HIP - oracle) / rms(oracle - mean(oracle)).  within_1e-3.{mean_abs,rel_rms} per library."}
            if out0_f16 is not None:
                parity["fp16"] = parity_vs(ref[0], out0_f16)
            if out0_c is not None:
                parity["fp32c"] = parity_vs(ref[0], out0_c)
            w = parity[args.precision]["within_1e-3"]
            if not (w["mean_abs"] and w["rel_rms"]):
                parity["note"] = (f"the benched {args.precision} value is outside 1e-3 under " + " and ".join(k for k, v in w.items() if not v) +
                                  " (bf16 MFMA operands floor the map at ~2.3e-3 mean_abs; DESIGN.md section 4); value_fp32c is the number of the contract "
                                  "precision (fp32 storage + split-bf16 products), inside 1e-3 under both readings; value_fp16 is the fp16 library's, "
                                  "inside 1e-3 under mean_abs only")
        cpu = {"value": round(1.0 / dt, 5), "unit": f"images/sec at {r}x{r} fp32", "cores": nthr, "cpu_model": cpu_model(), "kind": "port",
               "sample": f"1 image {r}x{r} ({TFLOP_PER_IMAGE_768 * (r / 768.0) ** 2:.3f} TFLOP), torch-CPU fp32 restatement of the diffusers path "
                         f"(oracle/), timed directly at this size: {dt:.1f} s",
               "seconds": round(dt, 2)}
        assert torch.isfinite(ref).all()

    dumped = dump_outputs(args.dump_outputs, dumps) if (args.dump_outputs and rank == 0) else None

    if rank == 0:
        head_name = "DPT disparity head" if dpt else f"{args.mode} head"
        cfg_idx = 3 if dpt else (1 if args.mode == "depth" else 2)
        dt_label = "bf16" if args.precision == "bf16" else f"{args.precision} (NOT BASELINE.json's dtype: --precision {args.precision})"
        line = {"metric": f"images/sec at 768x768 {dt_label} ({'depth' if not dpt and args.mode == 'depth' else head_name})", "value": round(value, 3), "unit": "images/sec", "n_gpus": n_gpus,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
                # per-step durations from one event per step (rank 0's stream) and the clock / power the timed region ran at: resolution below the
                # pool's box-to-box spread (ms_per_step stays the contract's wall-clock figure, max over ranks)
                "ms_per_step_min": step_stats.get("ms_per_step_min"), "ms_per_step_median": step_stats.get("ms_per_step_median"),
                "ms_per_step_max": step_stats.get("ms_per_step_max"), "clock_power": step_stats.get("clock_power"),
                "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
                "config": {"workload": (f"{head_name}, SD2.1 VAE-enc + UNet(t=1) + " + ("DPT neck/head" if dpt else "VAE-dec") +
                                        f", {args.res}x{args.res}, batch {args.batch}/GPU (BASELINE.json configs[{cfg_idx}]" +
                                        (f"; N = {n_gpus}: configs[4]'s sharding, {args.batch} per GPU" if n_gpus > 1 else "") + ")"),
                           "global_batch": n_total, "resolution": args.res,
                           "parallelism": f"dp{n_gpus} (batch-sharded, weights replicated, no data-path collective" +
                                          (", result maps gathered to rank 0 over RCCL inside the step)" if do_gather else ")"),
                           "gather_ms": gather_ms,
                           "weights": "random-init SD2.1 architecture (865.9M + 83.7M params)", "load_s": round(t_load, 1)},
                "roofline": roofline, "cpu_baseline": cpu, "stages": stages, "parity": parity,
                # does `value` (the benched dtype) meet north_star's 1e-3 tolerance?  per metric; null when the oracle leg did not run
                "value_within_tolerance": parity[args.precision]["within_1e-3"] if parity else None}
        if dumped is not None:
            line["dumped_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped}
        if parity and "fp16" in parity:
            line["value_fp16_within_tolerance"] = parity["fp16"]["within_1e-3"]
        if fp16:
            line.update(fp16)
        if fp32c:
            line.update(fp32c)
            if parity and "fp32c" in parity:
                line["value_fp32c_within_tolerance"] = parity["fp32c"]["within_1e-3"]
                line["within_1e-3"] = {k: v["within_1e-3"] for k, v in parity.items() if isinstance(v, dict) and "within_1e-3" in v}
        print(json.dumps(line), flush=True)
    eng.close()
    if world > 1:
        torch.distributed.destroy_process_group()
    return line if rank == 0 else None


if __name__ == "__main__":
    main()
