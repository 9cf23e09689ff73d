"""Time the device depth (or, with --normals, surface-normal; with --masks, dis / matting; with --structure, dis structure-score; with --matting, matting Grad / Conn; with --seg, seg palette decode + confusion matrix; with --band, trimap / boundary bands) evaluation against the host evaluation, and the batched device loop on the tiny pipeline.

  python tools/eval_bench.py --out profiles/<name>.json

1. `engine.eval_depth` (gp_eval_depth: two passes of 9 bytes per pixel + two finalisers) at 1 x 4032 x 6048 (ETH3D) and 4 x 480 x 640 (NYU),
   least-squares alignment: device events around `iters` back-to-back calls after a warm-up, against `eval_metrics.evaluate_depth` on the same
   arrays on the host (wall clock; one run at ETH3D size, it takes seconds).  Also what the host loop pays before it can evaluate: the copy of
   the prediction to the host.  The two sides' values are compared on the spot (they must agree to 1e-9).
2. `infer_eval.infer_and_evaluate` images/s at batch_size 1 and 4 on the tiny synthetic-weight pipeline, 16 images of 480 x 640 in a temporary
   ScanNet-style tree (a measurement of the loop's overheads -- decode, upload, launch count --, not of the full-size model).

  python tools/eval_bench.py --normals --out profiles/<name>.json

3. `--normals` (instead of 1 and 2): `engine.eval_normal` (gp_eval_normal: the angle pass, 24 bytes + the mask byte in and an 8-byte key out per
   pixel, then six selection passes of 8 bytes per pixel, plus the small finaliser / pick kernels) at 4 x 480 x 640 and 1 x 4032 x 6048 with the
   derived validity rule, against `eval_metrics.normal_angular_error` on the same arrays on the host, timed and compared the same way.

  python tools/eval_bench.py --masks --out profiles/<name>.json

4. `--masks` (instead of 1 and 2): the `gp_eval_mask` entry behind `engine.eval_mask` (one count pass of 5 bytes per pixel -- the float map and the 8-bit ground
   truth --, 6 with a region, and one finalising workgroup per image) at 4 x 1024 x 1024 and 1 x 4032 x 6048, on a 0 / 255 mask and on
   uniform-random values, against `eval_metrics.mask_metrics` on the same arrays on the host (wall clock), and against the time the bytes
   alone cost at the device-to-device copy bandwidth measured in the same process.  The two sides' values are compared on the spot (bit-equal).

  python tools/eval_bench.py --structure --out profiles/<name>.json

5. `--structure` (instead of 1 and 2): the `gp_eval_structure` entry behind `engine.eval_structure` (S-measure, E-measure, weighted F: seven
   launches, the exact distance transform among them) at 4 x 1024 x 1024 and 1 x 2048 x 2048, on a mask-like input (a disc, 3 % of the
   prediction flipped) and on a single far object (a small square in one corner: the row search of the distance transform spans the image),
   against `eval_metrics.structure_metrics` on the same arrays on the host (wall clock, one run: it takes seconds).  The exact scores are
   compared on the spot (bit-equal), wf to 1e-8.  `--no-host` skips the host route (for a kernel trace of the device calls alone).

  python tools/eval_bench.py --matting --out profiles/<name>.json

6. `--matting` (instead of 1 and 2): the `gp_eval_matting` entry behind `engine.eval_matting` (gradient and connectivity error: 26 launches,
   the ten-stage union-find labelling among them) at 4 x 480 x 640 and 1 x 2048 x 2048 on an alpha-like input (a disc with a soft edge and
   thin strands, the prediction = the alpha plus noise in the soft band and a few detached blobs), against `eval_metrics.matting_metrics` on
   the same arrays on the host (wall clock, one run).  conn is compared on the spot (bit-equal), grad to 1e-9.  `--no-host` skips the host
   route (for a kernel trace of the device calls alone).

  python tools/eval_bench.py --seg --out profiles/<name>.json

7. `--seg` (instead of 1 and 2): the `gp_eval_seg` entry behind `engine.eval_seg` (palette decode of prediction and colour ground truth, the
   K x K confusion matrix in LDS, three launches) at 4 x 480 x 640 with K = 19 and K = 150 and at 1 x 2048 x 2048 with K = 150, on a seg-like
   input (blocks of palette colours, +-3 / 255 of colour noise, 5 % of the pixels flipped, 4 % of the ground truth off the palette): device
   events around `iters` back-to-back calls after a warm-up, for the C entry on preallocated buffers and for `engine.eval_seg` itself (which
   allocates, copies the result down and synchronises), against `eval_metrics.seg_metrics` on the same arrays on the host (wall clock, one
   run).  The two sides' values are compared on the spot (bit-equal).  The result carries the shader clock sampled meanwhile and the build id.

  python tools/eval_bench.py --band --out profiles/<name>.json

8. `--band` (instead of 1 and 2): the `gp_mask_band` entry behind `engine.mask_band` (a column pass and a row pass) and the two evaluators
   composed from it, `engine.eval_trimap` (radius 25, Euclidean) and `engine.eval_boundary_iou` (the 2 % Chebyshev band), at 4 x 480 x 640 and
   1 x 2048 x 2048 on the alpha-like input of `--matting`: device events around `iters` back-to-back calls after a warm-up, against
   `eval_metrics.mask_band` / `trimap_metrics` / `boundary_iou` on the same arrays on the host (wall clock, one run).  Planes and values are
   compared on the spot (bit-equal).  The band call's bytes -- the 1 + planes per pixel it has to move, and the 18 + planes it does move with
   its scratch word -- are set against the device-to-device copy bandwidth measured in the same process.  `--no-host` skips the host route.

  python tools/eval_bench.py --foreground --out profiles/<name>.json

9. `--foreground` (instead of 1 and 2): the `gp_foreground` entry behind `engine.cutout` (multi-level foreground estimation: one coarse launch
   and one launch per level above 32 x 32; the RGBA cutout alone is written) at 4 x 480 x 640 and 1 x 2048 x 2048 on the alpha-like input
   of `--matting` under a two-gradient image: device events around `iters` back-to-back calls after a warm-up, for the C entry on
   preallocated buffers and for `engine.cutout` itself, against `foreground.cutout_rgba` on the same arrays on the host (wall clock, one run);
   the cutouts are compared on the spot (bit-equal).  Per-level kernel times come from a kernel trace taken in a run of its own,

     rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/eval_bench.py --foreground --trace-run
     python tools/eval_bench.py --foreground --kernel-trace <dir>/.../<pid>_kernel_trace.csv --out profiles/<name>.json

   (`--trace-run`: the device calls alone, nothing timed; `--kernel-trace`: the median duration of each launch of a call, per shape, and the
   bytes the last level has to move -- image, alpha, the level below's F and B, the RGBA bytes -- over its time, next to the
   device-to-device copy bandwidth measured in the same process).  Without a trace the per-level fields say "not measured".  `--n-big N`
   sets the iterations of the levels above 32 x 32 (default 2); a level launch with N = 1 is what one launch of a plain, unfused form costs.

  python tools/eval_bench.py --guided --out profiles/<name>.json

10. `--guided` (instead of 1 and 2): the `gp_guided_upsample` entry behind `engine.guided_upsample` (guided filter with the image as guide, four
   launches) at 480 x 640 -> 1920 x 2560 and 768 x 768 -> 3072 x 3072, one channel, radius 4, eps 1e-4, on the `--foreground` image and its
   alpha-like map box-reduced to the small size: device events around `iters` back-to-back calls after a warm-up, for the C entry on
   preallocated buffers and for `engine.guided_upsample` itself, against `guided.guided_upsample` on the same arrays on the host (wall clock,
   one run); the maps are compared on the spot (bit-equal).  `--no-host` skips the host route.

  python tools/eval_bench.py --tiles --out profiles/<name>.json

11. `--tiles` (instead of 1 and 2): the `gp_tile_merge` entry behind `engine.tile_merge` (the merge of tiled inference: fit, solve and blend
   launches) at 2048 x 3072 and 4032 x 6048 with size = 768, overlap = 192, one channel, on a smooth map with noise as the base and affine
   images of its windows with noise of their own as the tiles: device events around `iters` back-to-back calls after a warm-up, for the C
   entry on preallocated buffers with the alignment `least_square` (three launches) and `none` (solve and blend alone, two launches) and for
   `engine.tile_merge` itself, against `tiled.tile_merge` on the same arrays on the host (wall clock, one run); maps and fits are compared on
   the spot (bit-equal).  The bytes the blend pass has to move (every tile once, the output once) over the time of the `none` call stand
   next to the device-to-device copy bandwidth measured in the same process.  `--no-host` skips the host route.

  python tools/eval_bench.py --geometry --out profiles/<name>.json

12. `--geometry` (instead of 1 and 2): the `gp_depth_geometry` entry behind `engine.depth_geometry` (point map, normals, keep bytes and the
   compacted point cloud: four launches) at 1 x 768 x 768 and 1 x 2048 x 3072 with radius 2 and stride 1, depth space, the default camera,
   on a smooth map with noise and a depth edge down the middle and a random image: the median of five repetitions, each device events
   around `iters` back-to-back calls after a warm-up, for the C entry on preallocated buffers, and `engine.depth_geometry` itself
   (allocations and its one read of the offsets included), against `geometry.depth_geometry` on the same arrays on the host (wall clock,
   one run); every output is compared on the spot (bit-equal).  The bytes the call has to move (4 B/px read, 25 B/px planes, 31 B/point)
   over the device time stand next to the device-to-device copy bandwidth measured in the same process.  `--no-host` skips the host route.

  python tools/eval_bench.py --lens-blur --out profiles/<name>.json

13. `--lens-blur` (instead of 1 and 2): the `gp_lens_blur` entry behind `engine.lens_blur` (synthetic depth of field, one launch) at
   1 x 768 x 768 and 1 x 2048 x 3072 with aperture = max_radius = 16, depth space, sRGB tables, on three maps: a scene (a smooth map with
   noise and a depth edge down the middle, focus 0.5), the worst case (every pixel at the full radius) and a map in focus everywhere but a
   64 x 64 patch, which shows what the search bound over the staged region saves; the output bits are the same either way.  The median of
   25 consecutive calls, each between two device events, after 0.3 s of the same call as warm-up, for the C entry on preallocated buffers and for `engine.lens_blur` itself,
   against `lens_blur.lens_blur` on the same arrays on the host (wall clock, one run; compared on the spot, bit-equal).  The host route is
   timed at a size only while the rate of the size before predicts a minute or less; otherwise the row says so.  Offsets per second are
   counted twice, tested (what the kernel walks) and contributing (what the definition sums), and the vector-ALU instructions of the
   tested offsets over the time stand next to the issue rate of the card (one wave64 instruction per SIMD every 2 cycles).  `--no-host`
   skips the host route.

  python tools/eval_bench.py --stereo --out profiles/<name>.json

14. `--stereo` (instead of 1 and 2): the `gp_stereo_views` entry behind `engine.stereo_views` (stereo and parallax views, two launches) at
   1 x 768 x 768 and 1 x 2048 x 3072 for `sbs` with two views and a 3 x 3 quilt, separation 32, depth space, the default edge and
   convergence plane, on the scene of `--lens-blur` (a smooth map with noise and a depth edge down the middle) and a random image.  The
   median of 25 consecutive calls, each between two device events, after 0.3 s of the same call as warm-up, for the C entry on
   preallocated buffers and for `engine.stereo_views` itself, against `stereo.stereo_views` on the same arrays on the host (wall clock,
   one run; compared on the spot, bit-equal).  The host route is timed at a size only while its rate per pixel and view at the size
   before predicts a minute or less; otherwise the row says so.  The bytes the call has to move (image and map read once, every view's
   three colour bytes written, the plane of four bytes written and read) over the device time stand in the row.  `--no-host` skips the
   host route.
  python tools/eval_bench.py --parallax --out profiles/<name>.json

15. `--parallax` (instead of 1 and 2): the `gp_parallax_frames` entry behind `engine.parallax_frames` (camera moves from one photograph,
   two launches) at 1 x 768 x 768 and 1 x 2048 x 3072 for a 16-frame orbit with amount 16 and a 16-frame dolly to 1.25 x (push 0.02),
   depth space, the default edge and plane, with overscan, on the scene and image of `--stereo`.  The median of 25 consecutive calls, each
   between two device events, after 0.3 s of the same call as warm-up, for the C entry on preallocated buffers and for
   `engine.parallax_frames` itself, against `parallax.parallax_frames` on the host for the first two frames of the path (wall clock, one
   run; compared on the spot, bit-equal; timed at a size only while the rate at the size before predicts a minute or less).  In the same
   run the `gp_stereo_views` side-by-side pair at separation 16 on the same arrays, so that a frame's time stands next to a view's.
   `--no-host` skips the host route.
  python tools/eval_bench.py --relight --out profiles/<name>.json

16. `--relight` (instead of 1 and 2): the `gp_relight` entry behind `engine.relight` (new lights on a photograph, one launch) at
   1 x 768 x 768 and 1 x 2048 x 3072, disparity space, sRGB tables, for one light without shadows (the streaming form: 18 bytes per pixel,
   whose rate stands next to the device-to-device copy bandwidth measured in the same process), one light with reach 32 and three lights
   with reach 64 on the scene of `--stereo` with its normals by central differences, and the worst case: three lights with reach 64 over a
   ramp that rises towards them faster than their rays, so that no march ends early.  The median of 25 consecutive calls, each between two
   device events, after 0.3 s of the same call as warm-up, for the C entry on preallocated buffers and for `engine.relight` itself,
   against `relight.relight` on the same arrays on the host (wall clock, one run; compared on the spot, bit-equal; timed at a size only
   while the same case's rate per pixel at the size before predicts a minute or less).  `--no-host` skips the host route.
  python tools/eval_bench.py --mesh --out profiles/<name>.json

17. `--mesh` (instead of 1 and 2): the `gp_depth_mesh` entry behind `engine.depth_mesh` (triangle meshes cut at depth edges: four launches)
   at 1 x 768 x 768 and 1 x 2048 x 3072 with stride 1 and 2 and cut 0.05, depth space, the default camera, on the scene and image of
   `--geometry`.  The median of 25 consecutive calls, each between two device events, after 0.3 s of the same call as warm-up, for the C
   entry alone on preallocated buffers with the planes given, and for the whole `engine.depth_mesh` (both entries, allocations and its one
   read of the offsets), against `mesh.depth_mesh` on the host (wall clock, one run; every plane, array and offset compared on the spot,
   bit-equal).  In the same run, as the yardstick, the point-cloud call `engine.depth_geometry` at the same shapes, and `gp_depth_geometry`
   with and without its point arrays, whose difference is its count, scan and scatter launches.  The vertex and face counts and the bytes
   the call has to move (5 B/node read, 27 B/vertex read, 39 B/vertex and 12 B/face written) stand next to each time and to the
   device-to-device copy bandwidth measured in the same process.  `--no-host` skips the host route.
Needs a GPU; there is no CPU fall-back."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_events(call, iters):
    """ms per call: device events around `iters` back-to-back calls after a warm-up of three"""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def case(b, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    pred = np.stack([np.clip(0.5 + 0.35 * np.sin(3.1 * xx + i) * np.cos(2.3 * yy) + 0.05 * rng.standard_normal((h, w), dtype=np.float32), 0, 1)
                     for i in range(b)]).astype(np.float32)
    gt = (9.0 * pred ** 1.3 + 0.8 + 0.05 * rng.standard_normal(pred.shape, dtype=np.float32)).astype(np.float32)
    mask = (gt > 1e-3) & (gt < 10.0) & (rng.random(pred.shape, dtype=np.float32) < 0.8)
    return pred, gt, mask


def bench_eval(b, h, w, iters, host_runs):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    pred, gt, mask = case(b, h, w, 1)
    tp, tg, tm = (torch.from_numpy(x).to(d) for x in (pred, gt, mask))
    dev_ms = time_events(lambda: ge.eval_depth_raw(tp, tg, tm, "least_square", None, 1e-3, 10.0), iters)
    t0 = time.perf_counter()
    metrics, _ = ge.eval_depth(tp, tg, tm, "least_square", None, 1e-3, 10.0)  # with the 14-double copy and the host synchronise
    call_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(5):
        back = tp.cpu()
    copy_ms = (time.perf_counter() - t0) * 1e3 / 5
    assert back.shape == tp.shape
    host_ms = []
    for _ in range(host_runs):
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            ref = [em.evaluate_depth(pred[i], gt[i], mask[i], 1e-3, 10.0, alignment="least_square") for i in range(b)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    worst = max(abs(metrics[i][k] - ref[i][k]) / abs(ref[i][k]) for i in range(b) for k in ref[i])
    assert worst <= 1e-9, worst
    nbytes = 2 * 9 * b * h * w
    return dict(shape=[b, h, w], device_ms_per_call=dev_ms, device_iters=iters, device_gb_per_s=nbytes / dev_ms / 1e6, bytes_per_call=nbytes,
                device_call_with_sync_ms=call_ms, prediction_copy_to_host_ms=copy_ms, host_evaluate_depth_ms=min(host_ms), host_runs=host_runs,
                host_over_device=min(host_ms) / dev_ms, worst_rel_device_vs_host=worst)


def normal_case(b, h, w, seed):
    """gt: Gaussian directions (float32, a twentieth of the pixels all-zero); pred: gt plus Gaussian noise, in the pipeline's [0, 1] encoding."""
    rng = np.random.default_rng(seed)
    gt = rng.standard_normal((b, 3, h, w), dtype=np.float32)
    pred = gt + 0.35 * rng.standard_normal((b, 3, h, w), dtype=np.float32)
    pred /= np.maximum(np.sqrt((pred * pred).sum(axis=1, keepdims=True)), 1e-6)
    enc = ((pred + 1.0) * 0.5).astype(np.float32)
    gt *= rng.random((b, 1, h, w), dtype=np.float32) >= 0.05
    return enc, gt


def bench_eval_normal(b, h, w, iters, host_runs):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    enc, gt = normal_case(b, h, w, 2)
    tp, tg = (torch.from_numpy(x).to(d) for x in (enc, gt))
    dev_ms = time_events(lambda: ge.eval_normal_raw(tp, tg), iters)
    t0 = time.perf_counter()
    metrics, n_valid = ge.eval_normal(tp, tg)  # with the 8-double copy and the host synchronise
    call_ms = (time.perf_counter() - t0) * 1e3
    host_ms = []
    for _ in range(host_runs):
        t0 = time.perf_counter()
        ref = [em.normal_angular_error(enc[i].astype(np.float64) * 2.0 - 1.0, gt[i], (gt[i] != 0).any(axis=0)) for i in range(b)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    worst = max(abs(metrics[i][k] - ref[i][k]) / abs(ref[i][k]) for i in range(b) for k in ref[i])
    assert worst <= 1e-9, worst
    angle_bytes, select_bytes = (24 + 8) * b * h * w, 6 * 8 * b * h * w  # mask None: no mask byte
    nbytes = angle_bytes + select_bytes
    return dict(shape=[b, h, w], n_valid=[int(v) for v in n_valid], device_ms_per_call=dev_ms, device_iters=iters, launches_per_call=14,
                bytes_per_call=nbytes, angle_pass_bytes=angle_bytes, selection_bytes=select_bytes, device_gb_per_s=nbytes / dev_ms / 1e6,
                device_call_with_sync_ms=call_ms, host_normal_angular_error_ms=min(host_ms), host_runs=host_runs,
                host_over_device=min(host_ms) / dev_ms, worst_rel_device_vs_host=worst)


def mask_case(b, h, w, seed, kind):
    """kind "mask": prediction exactly 0.0 / 1.0 and ground truth 0 / 255, a noisy copy of one another; "uniform": random floats and bytes."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((b, h, w), dtype=np.float32), rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    obj = np.stack([(xx - 0.5) ** 2 + (yy - 0.5) ** 2 < (0.15 + 0.05 * i) ** 2 for i in range(b)])
    flip = rng.random((b, h, w), dtype=np.float32) < 0.03
    return (obj ^ flip).astype(np.float32), (obj * 255).astype(np.uint8)


def copy_bandwidth(d, nbytes=1 << 28, iters=20):
    """Device-to-device copy of nbytes: GB/s of traffic (read + write), device events over `iters` copies after a warm-up."""
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=d).random_(0, 256), torch.empty(nbytes, dtype=torch.uint8, device=d)
    return 2 * nbytes / time_events(lambda: dst.copy_(src), iters) / 1e6


def time_eval_mask(tp, tg, iters):
    """ms per gp_eval_mask call: the C entry itself on preallocated buffers (the two launches, none of the binding's tensor bookkeeping)."""
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    b, h, w = (int(v) for v in tp.shape)
    nbytes = int(lib.gp_eval_mask_workspace(b, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=tp.device)
    out = torch.empty((b, 10), dtype=torch.float64, device=tp.device)
    stream = int(torch.cuda.current_stream(tp.device).cuda_stream)

    def call():
        st = lib.gp_eval_mask(tp.data_ptr(), int(tp.dtype == torch.uint8), tg.data_ptr(), None, b, h, w, out.data_ptr(), None, ws.data_ptr(), nbytes, stream)
        assert st == ge.GP_OK, st

    return time_events(call, iters)


def bench_eval_mask(b, h, w, kind, iters, host_runs, copy_gb_per_s):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    pred, gt = mask_case(b, h, w, 3, kind)
    tp, tg = (torch.from_numpy(x).to(d) for x in (pred, gt))
    dev_ms = time_eval_mask(tp, tg, iters)
    t0 = time.perf_counter()
    metrics = ge.eval_mask(tp, tg)  # with the copy of the 10 values and 516 counts per image and the host synchronise
    call_ms = (time.perf_counter() - t0) * 1e3
    host_ms = []
    for _ in range(host_runs):
        t0 = time.perf_counter()
        ref = [em.mask_metrics(pred[i], gt[i]) for i in range(b)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    for i in range(b):
        assert all(metrics[i][k] == ref[i][k] for k in em.MASK_METRICS) and metrics[i]["n"] == ref[i]["n"], (i, metrics[i], ref[i])
    nbytes = 5 * b * h * w
    floor_ms = nbytes / copy_gb_per_s / 1e6
    return dict(shape=[b, h, w], input=kind, device_ms_per_call=dev_ms, device_iters=iters, launches_per_call=2, bytes_per_call=nbytes,
                device_gb_per_s=nbytes / dev_ms / 1e6, copy_gb_per_s=copy_gb_per_s, bytes_alone_ms=floor_ms, device_over_bytes_alone=dev_ms / floor_ms,
                device_call_with_sync_ms=call_ms, host_mask_metrics_ms=min(host_ms), host_runs=host_runs, host_over_device=min(host_ms) / dev_ms,
                device_equals_host=True)


def structure_case(b, h, w, seed, kind):
    """kind "mask": mask_case's disc; "far": one 16 x 16 object in the bottom-right corner, found by the prediction up to 3 % flips."""
    if kind == "mask":
        return mask_case(b, h, w, seed, "mask")
    rng = np.random.default_rng(seed)
    obj = np.zeros((b, h, w), dtype=bool)
    obj[:, h - 24:h - 8, w - 24:w - 8] = True
    flip = rng.random((b, h, w), dtype=np.float32) < 0.03
    return (obj ^ flip).astype(np.float32), (obj * 255).astype(np.uint8)


def time_eval_structure(tp, tg, iters):
    """ms per gp_eval_structure call: the C entry itself on preallocated buffers (the seven launches, none of the binding's bookkeeping)."""
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    b, h, w = (int(v) for v in tp.shape)
    nbytes = int(lib.gp_eval_structure_workspace(b, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=tp.device)
    out = torch.empty((b, 15), dtype=torch.float64, device=tp.device)
    stream = int(torch.cuda.current_stream(tp.device).cuda_stream)

    def call():
        st = lib.gp_eval_structure(tp.data_ptr(), int(tp.dtype == torch.uint8), tg.data_ptr(), b, h, w, out.data_ptr(), None, None, ws.data_ptr(), nbytes,
                                   stream)
        assert st == ge.GP_OK, st

    return time_events(call, iters)


def bench_eval_structure(b, h, w, kind, iters, host):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    pred, gt = structure_case(b, h, w, 5, kind)
    tp, tg = (torch.from_numpy(x).to(d) for x in (pred, gt))
    dev_ms = time_eval_structure(tp, tg, iters)
    t0 = time.perf_counter()
    metrics = ge.eval_structure(tp, tg)  # with the copy of the 15 values per image and the host synchronise
    call_ms = (time.perf_counter() - t0) * 1e3
    res = dict(shape=[b, h, w], input=kind, device_ms_per_call=dev_ms, device_iters=iters, launches_per_call=7, device_call_with_sync_ms=call_ms,
               workspace_bytes=int(ge.load_library().gp_eval_structure_workspace(b, h, w)), scores_image_0={k: metrics[0][k] for k in em.STRUCTURE_METRICS})
    if host:
        t0 = time.perf_counter()
        ref = [em.structure_metrics(pred[i], gt[i]) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        worst = 0.0
        for i in range(b):
            assert all(metrics[i][k] == ref[i][k] for k in ("s_alpha", "max_e", "mean_e", "adp_e", "n_fg", "cx", "cy")), (i, metrics[i], ref[i])
            worst = max(worst, abs(metrics[i]["wf"] - ref[i]["wf"]) / ref[i]["wf"])
        assert worst <= 1e-8, worst
        res.update(host_structure_metrics_ms=host_ms, host_runs=1, host_over_device=host_ms / dev_ms, s_and_e_equal_host=True, wf_worst_rel_device_vs_host=worst)
    return res


def matting_case(b, h, w, seed):
    """(pred float32 in [0, 1], alpha uint8): a disc whose edge fades over 6 % of the image, crossed by thin strands; the prediction adds noise
    where the alpha is soft, loses a third of the strands and gains a few detached blobs."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, h, dtype=np.float32), np.linspace(-1, 1, w, dtype=np.float32), indexing="ij")
    preds, gts = [], []
    for i in range(b):
        r = np.sqrt((xx - 0.1 * i) ** 2 + yy ** 2)
        alpha = np.clip((0.6 - r) / 0.12 + 0.5, 0, 1)
        strands = (np.abs(np.sin(40 * np.arctan2(yy, xx - 0.1 * i))) > 0.97) & (r > 0.55) & (r < 0.8)
        alpha = np.maximum(alpha, strands * 0.7).astype(np.float32)
        soft = (alpha > 0) & (alpha < 1)
        pred = alpha + soft * 0.15 * rng.standard_normal((h, w), dtype=np.float32)
        pred[strands & (rng.random((h, w), dtype=np.float32) < 0.33)] = 0
        pred[(rng.random((h, w), dtype=np.float32) < 2e-4) & (r > 0.85)] = 0.9
        preds.append(np.clip(pred, 0, 1))
        gts.append((alpha * 255).astype(np.uint8))
    return np.stack(preds).astype(np.float32), np.stack(gts)


def time_eval_matting(tp, tg, iters):
    """ms per gp_eval_matting call: the C entry itself on preallocated buffers (the 26 launches, none of the binding's bookkeeping)."""
    from genpercept_amd import engine as ge
    lib = ge.load_library()
    b, h, w = (int(v) for v in tp.shape)
    nbytes = int(lib.gp_eval_matting_workspace(b, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=tp.device)
    out = torch.empty((b, 4), dtype=torch.float64, device=tp.device)
    stream = int(torch.cuda.current_stream(tp.device).cuda_stream)

    def call():
        st = lib.gp_eval_matting(tp.data_ptr(), int(tp.dtype == torch.uint8), tg.data_ptr(), None, b, h, w, out.data_ptr(), None, None, None,
                                 ws.data_ptr(), nbytes, stream)
        assert st == ge.GP_OK, st

    return time_events(call, iters)


def bench_eval_matting(b, h, w, iters, host):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    pred, gt = matting_case(b, h, w, 5)
    tp, tg = (torch.from_numpy(x).to(d) for x in (pred, gt))
    dev_ms = time_eval_matting(tp, tg, iters)
    t0 = time.perf_counter()
    metrics = ge.eval_matting(tp, tg)  # with the copy of the 4 values per image and the host synchronise
    call_ms = (time.perf_counter() - t0) * 1e3
    res = dict(shape=[b, h, w], input="alpha", device_ms_per_call=dev_ms, device_iters=iters, launches_per_call=26, device_call_with_sync_ms=call_ms,
               workspace_bytes=int(ge.load_library().gp_eval_matting_workspace(b, h, w)), scores_image_0={k: metrics[0][k] for k in em.MATTING_METRICS})
    if host:
        t0 = time.perf_counter()
        ref = [em.matting_metrics(pred[i], gt[i]) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        worst = 0.0
        for i in range(b):
            assert metrics[i]["conn"] == ref[i]["conn"], (i, metrics[i], ref[i])
            worst = max(worst, abs(metrics[i]["grad"] - ref[i]["grad"]) / ref[i]["grad"])
        assert worst <= 1e-9, worst
        res.update(host_matting_metrics_ms=host_ms, host_runs=1, host_over_device=host_ms / dev_ms, conn_equals_host=True, grad_worst_rel_device_vs_host=worst)
    return res


def seg_case(b, h, w, K, seed):
    """pred float32 [b, 3, h, w], colour ground truth uint8 [b, h, w, 3], palette uint8 [K, 3]"""
    rng = np.random.RandomState(seed)
    pal = rng.randint(0, 256, (K, 3)).astype(np.uint8)
    lab = rng.randint(0, K, (b, h // 16 + 1, w // 16 + 1)).repeat(16, 1).repeat(16, 2)[:, :h, :w]
    seen = np.where(rng.rand(b, h, w) < 0.05, rng.randint(0, K, (b, h, w)), lab)
    col = np.clip(pal[seen].astype(np.int16) + rng.randint(-3, 4, (b, h, w, 3)), 0, 255).astype(np.float32)
    pred = np.ascontiguousarray(np.moveaxis((col + np.float32(0.2)) / np.float32(255.0), -1, 1))
    gt = pal[lab]
    off = rng.rand(b, h, w) < 0.04
    gt[off] = rng.randint(0, 256, (int(off.sum()), 3)).astype(np.uint8)
    return pred, np.ascontiguousarray(gt), pal


def bench_eval_seg(b, h, w, K, iters, host):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    pred, gt, pal = seg_case(b, h, w, K, 11)
    tp, tg, tpal = (torch.from_numpy(x).to(d) for x in (pred, gt, pal))
    nbytes = int(lib.gp_eval_seg_workspace(b, h, w, K))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    out = torch.empty((b, 8 + K), dtype=torch.float64, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def entry():
        st = lib.gp_eval_seg(tp.data_ptr(), 0, tg.data_ptr(), 0, 0, None, tpal.data_ptr(), K, b, h, w, out.data_ptr(), None, None, ws.data_ptr(), nbytes, stream)
        assert st == ge.GP_OK, st

    entry_ms = time_events(entry, iters)
    call_ms = time_events(lambda: ge.eval_seg(tp, tg, tpal), iters)
    decode_ms = time_events(lambda: ge.seg_decode(tp, tpal), iters)
    metrics = ge.eval_seg(tp, tg, tpal)
    res = dict(shape=[b, h, w], K=K, input="seg-like, colour ground truth", gp_eval_seg_ms_per_call=entry_ms, engine_eval_seg_ms_per_call=call_ms,
               engine_seg_decode_ms_per_call=decode_ms, device_iters=iters, launches_per_call=3, workspace_bytes=nbytes,
               scores_image_0={k: metrics[0][k] for k in em.SEG_METRICS})
    if host:
        t0 = time.perf_counter()
        ref = [em.seg_metrics(pred[i], gt[i], pal) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        for i in range(b):
            assert all(metrics[i][k] == ref[i][k] for k in em.SEG_METRICS) and np.array_equal(metrics[i]["conf"], ref[i]["conf"]), (i, metrics[i], ref[i])
            assert np.array_equal(metrics[i]["iou"], np.array(ref[i]["iou"]), equal_nan=True)
        res.update(host_seg_metrics_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, values_equal_host=True)
    return res


def bench_band(b, h, w, iters, host, copy_gb_per_s):
    from genpercept_amd import engine as ge
    from genpercept_amd import eval_metrics as em
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    pred, gt = matting_case(b, h, w, 5)
    tp, tg = (torch.from_numpy(x).to(d) for x in (pred, gt))
    nbytes = int(lib.gp_mask_band_workspace(b, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    planes = torch.empty((3, b, h, w), dtype=torch.uint8, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)
    d_b = em.boundary_reach(h, w, 0.02)
    settings = [dict(name="trimap of the alpha: disc of radius 25", src=tg, lo=0, hi=255, metric=0, reach=625, border=0, want=("band", "fg", "bg")),
                dict(name=f"inner band of the mask: square of radius {d_b} (2 % of the diagonal), border", src=tg, lo=128, hi=129, metric=1, reach=d_b,
                     border=1, want=("inner",))]
    rows = []
    for st in settings:
        outs = [planes[st["want"].index(k)].data_ptr() if k in st["want"] else None for k in ge.BAND_PLANES]

        def entry():
            rc = lib.gp_mask_band(st["src"].data_ptr(), 1, b, h, w, st["lo"], st["hi"], st["metric"], st["reach"], st["border"], *outs, ws.data_ptr(), nbytes,
                                  stream)
            assert rc == ge.GP_OK, rc

        entry_ms = time_events(entry, iters)
        metric = ("euclidean", "chebyshev")[st["metric"]]
        call_ms = time_events(lambda: ge.mask_band(st["src"], st["lo"], st["hi"], st["reach"], metric, bool(st["border"]), want=st["want"]), iters)
        got = {k: v.cpu().numpy() for k, v in ge.mask_band(st["src"], st["lo"], st["hi"], st["reach"], metric, bool(st["border"]), want=st["want"]).items()}
        must, moved = (1 + len(st["want"])) * b * h * w, (18 + len(st["want"])) * b * h * w
        row = dict(setting=st["name"], metric=metric, reach=st["reach"], planes=list(st["want"]), gp_mask_band_ms_per_call=entry_ms,
                   engine_mask_band_ms_per_call=call_ms, launches_per_call=2, workspace_bytes=nbytes, bytes_needed=must, bytes_moved=moved,
                   needed_gb_per_s=must / entry_ms / 1e6, moved_gb_per_s=moved / entry_ms / 1e6, copy_gb_per_s=copy_gb_per_s,
                   needed_bytes_alone_ms=must / copy_gb_per_s / 1e6, band_fraction_image_0=float((got[st["want"][0]][0] == 255).mean()))
        if host:
            t0 = time.perf_counter()
            ref = [em.mask_band(gt[i], st["lo"], st["hi"], st["reach"], st["metric"], st["border"]) for i in range(b)]
            host_ms = (time.perf_counter() - t0) * 1e3
            assert all(np.array_equal(got[k][i], ref[i][k]) for k in st["want"] for i in range(b))
            row.update(host_mask_band_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, planes_equal_host=True)
        rows.append(row)
    res = dict(shape=[b, h, w], input="alpha", device_iters=iters, mask_band=rows)
    for name, dev, ref_of in (("eval_trimap", lambda: ge.eval_trimap(tp, tg, 25, "euclidean"), lambda i: em.trimap_metrics(pred[i], gt[i], 25, "euclidean")),
                              ("eval_boundary_iou", lambda: ge.eval_boundary_iou(tp, tg, 0.02), lambda i: em.boundary_iou(pred[i], gt[i], 0.02))):
        ms = time_events(dev, iters)
        metrics = dev()
        row = dict(engine_ms_per_call=ms, values_image_0=metrics[0])
        if host:
            t0 = time.perf_counter()
            ref = [ref_of(i) for i in range(b)]
            host_ms = (time.perf_counter() - t0) * 1e3
            assert metrics == ref, (name, metrics, ref)
            row.update(host_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / ms, values_equal_host=True)
        res[name] = row
    return res


FOREGROUND_SHAPES = ((4, 480, 640), (1, 2048, 2048))


def foreground_case(b, h, w, seed):
    """An image of two colour gradients mixed by the alpha-like map of `matting_case` (+ noise), and that map's bytes."""
    from genpercept_amd import eval_metrics as em
    rng = np.random.default_rng(seed)
    _, gt = matting_case(b, h, w, seed)
    a = gt.astype(np.float32)[:, None] / 255.0
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    fg = np.stack([0.75 + 0.2 * xx, 0.15 + 0.2 * xx, 0.1 + 0.1 * xx])[None]
    bg = np.stack([0.1 + 0.1 * yy, 0.25 + 0.2 * yy, 0.65 + 0.3 * yy])[None]
    img = a * fg + (1 - a) * bg + 0.01 * rng.standard_normal((b, 3, h, w), dtype=np.float32)
    return em.quantize_mask(img), gt


def foreground_level_times(trace_csv):
    """{number of level launches of a call: [median ms of the coarse launch, of each level launch]} from a rocprofv3 kernel trace of
    `--foreground --trace-run` (the first three calls of each shape are its warm-up)."""
    import csv
    rows = []
    with open(trace_csv, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "fg_coarse_kernel" in name or "fg_level_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), "fg_coarse_kernel" in name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    calls, cur = [], None
    for _, coarse, ms in rows:
        if coarse:
            cur = [ms]
            calls.append(cur)
        elif cur is not None:
            cur.append(ms)
    out = {}
    for n in sorted({len(c) - 1 for c in calls}):
        timed = [c for c in calls if len(c) - 1 == n][3:]
        if timed:
            out[n] = [float(np.median([c[j] for c in timed])) for j in range(n + 1)]
    return out


def bench_foreground(b, h, w, iters, host, copy_gb_per_s, level_ms, trace_run, n_big=2):
    from genpercept_amd import engine as ge
    from genpercept_amd import foreground as fgh
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    img, a8 = foreground_case(b, h, w, 5)
    ti, ta = torch.from_numpy(img).to(d), torch.from_numpy(a8).to(d)
    nbytes = int(lib.gp_foreground_workspace(b, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    rgba = torch.empty((b, h, w, 4), dtype=torch.uint8, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def entry():
        rc = lib.gp_foreground(ti.data_ptr(), ta.data_ptr(), 1, b, h, w, 1e-5, 1.0, 10, n_big, None, 0, None, None, rgba.data_ptr(), None, ws.data_ptr(), nbytes,
                               stream)
        assert rc == ge.GP_OK, rc

    sizes = fgh.level_sizes(h, w)
    above = [s for s in sizes if s[0] > fgh.SMALL or s[1] > fgh.SMALL]
    if trace_run:
        for _ in range(3 + iters):
            entry()
        torch.cuda.synchronize()
        return dict(shape=[b, h, w], launches_per_call=1 + len(above))
    entry_ms = time_events(entry, iters)
    call_ms = time_events(lambda: ge.cutout(ti, ta, n_big=n_big), iters)
    got = ge.cutout(ti, ta, n_big=n_big).cpu().numpy()
    (hp, wp), (hl, wl) = sizes[-2], sizes[-1]
    last_bytes = b * (hl * wl * (3 + 1 + 4) + hp * wp * 24)
    res = dict(shape=[b, h, w], input="two gradients under an alpha-like map", options=dict(fgh.DEFAULTS, n_big=n_big), levels=[list(s) for s in sizes],
               gp_foreground_ms_per_call=entry_ms, engine_cutout_ms_per_call=call_ms, device_iters=iters, launches_per_call=1 + len(above),
               workspace_bytes=nbytes, last_level_bytes_needed=last_bytes, copy_gb_per_s=copy_gb_per_s,
               last_level_bytes_alone_ms=last_bytes / copy_gb_per_s / 1e6)
    ms = level_ms.get(len(above))
    if ms:
        res.update(coarse_launch_ms=ms[0], level_launch_ms=[dict(level=list(s), ms=t) for s, t in zip(above, ms[1:])], launches_sum_ms=float(sum(ms)),
                   last_level_gb_per_s=last_bytes / ms[-1] / 1e6, last_level_over_copy_rate=last_bytes / ms[-1] / 1e6 / copy_gb_per_s)
    else:
        res.update(coarse_launch_ms="not measured", level_launch_ms="not measured", last_level_gb_per_s="not measured")
    if host:
        t0 = time.perf_counter()
        ref = [fgh.cutout_rgba(img[i], a8[i], n_big=n_big) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(got[i], ref[i]) for i in range(b))
        res.update(host_cutout_rgba_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, cutout_equals_host=True)
    return res


GUIDED_SHAPES = ((1, 480, 640, 1920, 2560), (1, 768, 768, 3072, 3072))


def bench_guided(b, h, w, H, W, iters, host, radius=4, eps=1e-4):
    """gp_guided_upsample on preallocated buffers and engine.guided_upsample itself against guided.guided_upsample on the host."""
    from genpercept_amd import engine as ge
    from genpercept_amd import guided as gd
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    img, a8 = foreground_case(b, H, W, 5)
    k = H // h
    lo = img.reshape(b, 3, h, k, w, k).astype(np.float32).mean(axis=(3, 5))
    lo = np.floor(lo + 0.5).astype(np.uint8)
    pred = (a8.reshape(b, 1, h, k, w, k).astype(np.float32).mean(axis=(3, 5)) / 255.0).astype(np.float32)
    tl, tp, tg = torch.from_numpy(lo).to(d), torch.from_numpy(pred).to(d), torch.from_numpy(img).to(d)
    nbytes = int(lib.gp_guided_upsample_workspace(b, 1, h, w))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    out = torch.empty((b, 1, H, W), dtype=torch.float32, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def entry():
        rc = lib.gp_guided_upsample(tl.data_ptr(), tp.data_ptr(), 1, tg.data_ptr(), b, h, w, H, W, radius, eps, out.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == ge.GP_OK, rc

    entry_ms = time_events(entry, iters)
    call_ms = time_events(lambda: ge.guided_upsample(tl, tp, tg, radius, eps), iters)
    got = ge.guided_upsample(tl, tp, tg, radius, eps).cpu().numpy()
    res = dict(shape=[b, h, w, H, W], channels=1, input="two gradients under an alpha-like map, box-reduced", options=dict(radius=radius, eps=eps),
               gp_guided_upsample_ms_per_call=entry_ms, engine_guided_upsample_ms_per_call=call_ms, device_iters=iters, launches_per_call=4,
               workspace_bytes=nbytes)
    if host:
        t0 = time.perf_counter()
        ref = [gd.guided_upsample(lo[i], pred[i], img[i], radius, eps) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32)) for i in range(b))
        res.update(host_guided_upsample_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
    return res


TILE_SHAPES = ((1, 2048, 3072), (1, 4032, 6048))


def bench_tiles(b, h, w, iters, host, copy_gb_per_s, size=768, overlap=192):
    """gp_tile_merge on preallocated buffers (least_square and none) and engine.tile_merge itself against tiled.tile_merge on the host."""
    from genpercept_amd import engine as ge
    from genpercept_amd import tiled
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(9)
    base = case(b, h, w, 9)[0][:, None]
    ys, xs, wh, ww = tiled.tile_grid(h, w, size, overlap)
    n = len(ys) * len(xs)
    tiles = np.empty((b, n, 1, wh, ww), np.float32)
    for i in range(b):
        for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
            s, t = rng.uniform(0.5, 2.0), rng.uniform(-0.25, 0.25)
            tiles[i, k] = (base[i, :, y0:y0 + wh, x0:x0 + ww] - t) / s + 0.01 * rng.standard_normal((1, wh, ww), dtype=np.float32)
    tb, tt = torch.from_numpy(base).to(d), torch.from_numpy(tiles).to(d)
    ys32, xs32 = np.ascontiguousarray(ys, np.int32), np.ascontiguousarray(xs, np.int32)
    nbytes = int(lib.gp_tile_merge_workspace(b, 1, h, w, len(ys), len(xs), wh, ww))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def entry(align):
        rc = lib.gp_tile_merge(tb.data_ptr(), tt.data_ptr(), b, 1, h, w, ys32.ctypes.data, len(ys), xs32.ctypes.data, len(xs), wh, ww, overlap, align, None,
                               out.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == ge.GP_OK, rc

    fit_ms, none_ms = time_events(lambda: entry(0), iters), time_events(lambda: entry(1), iters)
    call_ms = time_events(lambda: ge.tile_merge(tb, tt, ys, xs, overlap), iters)
    got, fit = ge.tile_merge(tb, tt, ys, xs, overlap, want_fit=True)
    got, fit = got.cpu().numpy(), fit.cpu().numpy()
    blend_bytes = b * (n * wh * ww + h * w) * 4
    fit_bytes = b * 2 * n * wh * ww * 4
    res = dict(shape=[b, 1, h, w], grid=[len(ys), len(xs), wh, ww], options=dict(size=size, overlap=overlap), input="smooth map with noise; affine images of its windows",
               gp_tile_merge_ms_per_call=fit_ms, gp_tile_merge_none_ms_per_call=none_ms, engine_tile_merge_ms_per_call=call_ms, device_iters=iters,
               launches_per_call=3, launches_per_call_none=2, workspace_bytes=nbytes, blend_bytes_needed=blend_bytes, fit_bytes_needed=fit_bytes,
               blend_gb_per_s=blend_bytes / none_ms / 1e6, copy_gb_per_s=copy_gb_per_s, blend_over_copy_rate=blend_bytes / none_ms / 1e6 / copy_gb_per_s,
               blend_bytes_alone_ms=blend_bytes / copy_gb_per_s / 1e6, fit_pass_ms=fit_ms - none_ms, fit_gb_per_s=fit_bytes / max(fit_ms - none_ms, 1e-9) / 1e6,
               note="blend time = the `none` call (solve + blend launches); fit time = the difference of the two calls")
    if host:
        t0 = time.perf_counter()
        ref = [tiled.tile_merge(base[i], tiles[i], ys, xs, overlap) for i in range(b)]
        host_ms = (time.perf_counter() - t0) * 1e3
        ref_fit = [np.stack(tiled.tile_fit(base[i], tiles[i], ys, xs), axis=1) for i in range(b)]
        assert all(np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32)) for i in range(b))
        assert all(np.array_equal(fit[i].view(np.uint64), ref_fit[i].view(np.uint64)) for i in range(b))
        res.update(host_tile_merge_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
    return res


GEOMETRY_SHAPES = ((1, 768, 768), (1, 2048, 3072))


def bench_geometry(b, h, w, iters, host, copy_gb_per_s, radius=2, stride=1, repeats=5):
    """gp_depth_geometry on preallocated buffers (every output, image and default camera) and engine.depth_geometry itself against
    geometry.depth_geometry on the host."""
    from genpercept_amd import engine as ge
    from genpercept_amd import geometry as gm
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(13)
    pred = case(b, h, w, 13)[0]
    pred[:, :, w // 2:] = np.clip(pred[:, :, w // 2:] + 0.2, 0, 1)   # a depth edge down the middle
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    radius, tau, min_count, min_cos, stride = gm.check_options(radius, stride=stride)
    cams = gm.check_cameras(None, b, h, w)
    tp, ti = torch.from_numpy(pred).to(d), torch.from_numpy(image).to(d)
    cap = b * (-(-h // stride)) * (-(-w // stride))
    outs = [torch.empty(s, dtype=t, device=d) for s, t in (((b, 3, h, w), torch.float32), ((b, 3, h, w), torch.float32), ((b, h, w), torch.uint8),
                                                          ((cap, 3), torch.float32), ((cap, 3), torch.float32), ((cap, 3), torch.uint8),
                                                          ((cap,), torch.int32), ((b + 1,), torch.int64))]
    nbytes = int(lib.gp_depth_geometry_workspace(b, h, w, stride))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def entry():
        rc = lib.gp_depth_geometry(tp.data_ptr(), None, ti.data_ptr(), cams.ctypes.data, b, h, w, 0, radius, tau, min_count, min_cos, stride,
                                   *[o.data_ptr() for o in outs], ws.data_ptr(), nbytes, stream)
        assert rc == ge.GP_OK, rc

    runs = sorted(time_events(entry, iters) for _ in range(repeats))
    entry_ms = runs[len(runs) // 2]
    call_ms = sorted(time_events(lambda: ge.depth_geometry(tp, None, ti, radius=radius, stride=stride), max(1, iters // 5)) for _ in range(3))[1]
    got = ge.depth_geometry(tp, None, ti, radius=radius, stride=stride)
    n = int(got["offsets"][-1])
    need = b * h * w * (4 + 25) + 31 * n
    res = dict(shape=[b, 1, h, w], options=dict(radius=radius, tau=tau, min_count=min_count, min_cos=min_cos, stride=stride, space="depth"),
               input="smooth map with noise and a depth edge down the middle; random image; default camera", points=n, points_worst_case=cap,
               gp_depth_geometry_us_per_call=1e3 * entry_ms, gp_depth_geometry_us_per_call_runs=[1e3 * r for r in runs], device_iters=iters,
               repeats=repeats, statistic="median of the repeats; each is device events around `device_iters` back-to-back calls after a warm-up",
               engine_depth_geometry_ms_per_call=call_ms, launches_per_call=4, workspace_bytes=nbytes, bytes_needed=need,
               bytes_needed_rule="4 B/px read, 25 B/px planes, 31 B/point", gb_per_s=need / entry_ms / 1e6, copy_gb_per_s=copy_gb_per_s,
               over_copy_rate=need / entry_ms / 1e6 / copy_gb_per_s, bytes_alone_us=need / copy_gb_per_s / 1e3)
    if host:
        t0 = time.perf_counter()
        ref = gm.depth_geometry(pred[:, None], None, image, radius=radius, stride=stride)
        host_ms = (time.perf_counter() - t0) * 1e3
        for k, v in ref.items():
            g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
            assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g.view(np.uint8), v.view(np.uint8)), k
        res.update(host_depth_geometry_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
    return res


LENS_SHAPES = ((1, 768, 768), (1, 2048, 3072))
LENS_VALU_PER_TAP = 18          # vector-ALU instructions per tested offset in the compiled gather loop of lb_gather_kernel (its ISA, -O3, gfx950)
LENS_VALU_ISSUE_CYCLES = 2      # a SIMD issues one wave64 vector instruction per 2 cycles (MI355X_MICROARCH.md, per-instruction constants)
LENS_SIMDS = 256 * 4
LENS_CLOCK_MHZ = 2400.0         # the nominal shader clock the issue rate is stated at (the sampled mean also covers the host route's idle time)


def lens_taps(pred, rows, space, d):
    """(tested, contributing) offsets of one gp_lens_blur call, counted with torch ops on the device (a count for the benchmark, not a product
    path).  tested: per 32 x 16 tile n(cm) for the largest c of its staged region, times the tile's pixels inside the image.  contributing: the
    sources of step 4 over all output pixels."""
    import torch.nn.functional as F
    from genpercept_amd import lens_blur as lb
    b, h, w = pred.shape
    tested = contributing = 0
    counts = torch.tensor([lb.disc_count(c) for c in range(lb.MAX_C8 + 1)], device=d)
    R = (int(rows[:, 2].max()) + 4) >> 3
    for k in range(b):
        Dn = lb.nearness(pred[k], space)
        D = torch.from_numpy(Dn).to(d)
        c = torch.from_numpy(lb.circle_of_confusion(Dn, np.isnan(pred[k]), rows[k])).to(d)
        ph, pw = -(-h // 16) * 16, -(-w // 32) * 32
        padded = F.pad(c[None, None].float(), (R, R + pw - w, R, R + ph - h))
        cm = F.max_pool2d(padded, (16 + 2 * R, 32 + 2 * R), stride=(16, 32))[0, 0].long()
        inside = F.avg_pool2d(F.pad(torch.ones((1, 1, h, w), device=d), (0, pw - w, 0, ph - h)), (16, 32), divisor_override=1)[0, 0].long()
        tested += int((counts[cm] * inside).sum())
        Dp, cp = F.pad(D, (R, R, R, R)), F.pad(c, (R, R, R, R))
        cmax = int(c.max())
        total = torch.zeros((), dtype=torch.int64, device=d)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                d2 = 64 * (dx * dx + dy * dy)
                if d2 > (cmax + 4) ** 2:
                    continue
                Dq, cq = Dp[R + dy:R + dy + h, R + dx:R + dx + w], cp[R + dy:R + dy + h, R + dx:R + dx + w]
                # (an offset that leaves the image has c = 0 there and contributes only at d2 = 0, which stays inside)
                r = torch.where(Dq >= D, cq, torch.minimum(cq, c))
                total += (d2 <= (r + 4) ** 2).sum()
        contributing += int(total)
    return tested, contributing


def lens_timed_calls(call, n, warm_s=0.3):
    """ms of each of n consecutive calls, a device event between every two, after warm_s seconds of the same call: a window of a few calls
    after the host route has kept the card idle would measure the clock coming up."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for _ in range(10):
            call()
        torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for k in range(n):
        call()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(n)]


def bench_lens_blur(b, h, w, iters, host, host_budget_s=60.0, radius=16.0, timed=25):
    """gp_lens_blur on preallocated buffers and engine.lens_blur itself at aperture = max_radius = `radius`, sRGB tables, depth space, on three
    maps -- a scene (smooth map with noise and a depth edge down the middle, focus 0.5), the worst case (every pixel at the full radius) and a
    map in focus everywhere but a 64 x 64 patch -- against lens_blur.lens_blur on the host.  The output bits are compared where the host
    runs."""
    from genpercept_amd import engine as ge
    from genpercept_amd import lens_blur as lb
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    scene = case(b, h, w, 17)[0]
    scene[:, :, w // 2:] = np.clip(scene[:, :, w // 2:] + 0.2, 0, 1)
    patch = np.zeros((b, h, w), np.float32)
    patch[:, h // 2 - 32:h // 2 + 32, w // 2 - 32:w // 2 + 32] = 1.0
    maps = dict(scene=(scene, 0.5), worst_case=(np.ones((b, h, w), np.float32), 0.0), in_focus_but_a_patch=(patch, 0.0))
    ti = torch.from_numpy(image).to(d)
    to_lin, from_lin = ge._lens_tables(None, d)
    out = torch.empty((b, 3, h, w), dtype=torch.uint8, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)
    res = dict(shape=[b, 3, h, w], options=dict(aperture=radius, max_radius=radius, dof=0.0, space="depth", tables="srgb"), launches_per_call=1,
               workspace_bytes=0, timed_calls=timed, statistic="median of `timed_calls` consecutive calls, each between two device events, after 0.3 s of the same call as warm-up",
               valu_rule=f"tested offsets / 64 lanes * {LENS_VALU_PER_TAP} vector instructions (the compiled gather loop) * {LENS_VALU_ISSUE_CYCLES} cycles "
                         f"/ ({LENS_SIMDS} SIMDs * the shader clock * the time)", maps={})
    host_s = 0.0
    for name, (pred, focus) in maps.items():
        tp = torch.from_numpy(pred).to(d)
        rows = lb.lens_params(pred[:, None], "depth", focus=focus, aperture=radius, max_radius=radius)
        params = torch.from_numpy(rows).to(d)
        max_c8 = int(rows[:, 2].max())

        def entry():
            rc = lib.gp_lens_blur(ti.data_ptr(), tp.data_ptr(), None, params.data_ptr(), to_lin.data_ptr(), from_lin.data_ptr(), b, h, w, 0, max_c8,
                                  out.data_ptr(), None, stream)
            assert rc == ge.GP_OK, rc

        entry_runs = sorted(lens_timed_calls(entry, timed))
        entry_ms = entry_runs[len(entry_runs) // 2]
        call = lambda: ge.lens_blur(ti, tp, focus=focus, aperture=radius, max_radius=radius)  # noqa: E731
        call_ms = float(np.median(lens_timed_calls(call, timed)))
        got = call().cpu().numpy()
        tested, contributing = lens_taps(pred, rows, "depth", d)
        row = dict(focus=focus, gp_lens_blur_us_per_call=1e3 * entry_ms, gp_lens_blur_us_min_max=[1e3 * entry_runs[0], 1e3 * entry_runs[-1]], engine_lens_blur_us_per_call=1e3 * call_ms, tested_offsets=tested,
                   contributing_offsets=contributing, tested_offsets_per_s=tested / entry_ms * 1e3, contributing_offsets_per_s=contributing / entry_ms * 1e3,
                   valu_instructions=tested / 64 * LENS_VALU_PER_TAP)
        predicted_s = LENS_HOST_S_PER_PIXEL[0] * h * w   # (0 at the first size)
        if host and predicted_s <= host_budget_s:
            t0 = time.perf_counter()
            ref = lb.lens_blur(image, pred[:, None], focus=focus, aperture=radius, max_radius=radius)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), name
            row.update(host_lens_blur_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
            host_s = max(host_s, host_ms / 1e3)
        elif host:
            row["host"] = f"not timed at this size: about {predicted_s:.0f} s by the rate of the smaller size, above the budget of {host_budget_s:.0f} s"
        res["maps"][name] = row
    if host_s:
        LENS_HOST_S_PER_PIXEL[0] = host_s / (h * w)
    return res


LENS_HOST_S_PER_PIXEL = [0.0]   # the host route's rate at the last size it ran at, to decide whether the next size is timed

STEREO_SHAPES = ((1, 768, 768), (1, 2048, 3072))
STEREO_LAYOUTS = (("sbs", 2), ("quilt", (3, 3)))
STEREO_HOST_S_PER_PIXEL_VIEW = [0.0]   # as above, per pixel and view


def bench_stereo(b, h, w, host, host_budget_s=60.0, separation=32.0, timed=25):
    """gp_stereo_views on preallocated buffers and engine.stereo_views itself for the layouts of STEREO_LAYOUTS at `separation`, depth space,
    the default edge and convergence plane, on a scene (smooth map with noise and a depth edge down the middle) and a random image, against
    stereo.stereo_views on the host.  The output bits are compared where the host runs."""
    from genpercept_amd import engine as ge
    from genpercept_amd import stereo as st
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    pred = case(b, h, w, 17)[0]
    pred[:, :, w // 2:] = np.clip(pred[:, :, w // 2:] + 0.2, 0, 1)
    ti, tp = torch.from_numpy(image).to(d), torch.from_numpy(pred).to(d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)
    res = dict(shape=[b, 3, h, w], options=dict(separation=separation, edge=st.EDGE_DEFAULT, converge=None, space="depth"), launches_per_call=2, timed_calls=timed,
               statistic="median of `timed_calls` consecutive calls, each between two device events, after 0.3 s of the same call as warm-up", layouts={})
    host_rate = 0.0
    for layout, views in STEREO_LAYOUTS:
        o = st.plan(b, h, w, layout, views, separation)
        table, (ch, cw), v = o["table"], o["size"], int(o["table"].shape[0])
        conv = torch.full((b,), st.F_DEFAULT, dtype=torch.int32, device=d)
        canvas = torch.empty((b, 3, ch, cw), dtype=torch.uint8, device=d)
        nbytes = lib.gp_stereo_views_workspace(b, v, h, w)
        ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)

        def entry():
            rc = lib.gp_stereo_views(ti.data_ptr(), tp.data_ptr(), conv.data_ptr(), table.ctypes.data, b, v, h, w, ch, cw, 0, o["edge"], o["max_s8"],
                                     canvas.data_ptr(), None, None, ws.data_ptr(), nbytes, stream)
            assert rc == ge.GP_OK, rc

        entry_runs = sorted(lens_timed_calls(entry, timed))
        entry_ms = entry_runs[len(entry_runs) // 2]
        call = lambda: ge.stereo_views(ti, tp, layout, views, separation)  # noqa: E731
        call_ms = float(np.median(lens_timed_calls(call, timed)))
        got, holes = (t.cpu().numpy() for t in ge.stereo_views(ti, tp, layout, views, separation, want_holes=True))
        moved = b * h * w * (7 + v * (3 + 8))   # image 3 + map 4 read once; per view 3 colour bytes written, the plane written and read
        row = dict(views=v, canvas=[ch, cw], max_s8=o["max_s8"], workspace_bytes=int(nbytes), gp_stereo_views_us_per_call=1e3 * entry_ms,
                   gp_stereo_views_us_min_max=[1e3 * entry_runs[0], 1e3 * entry_runs[-1]], engine_stereo_views_us_per_call=1e3 * call_ms,
                   hole_share=float(holes.mean()), bytes_moved=moved, gb_per_s=moved / entry_ms / 1e6)
        predicted_s = STEREO_HOST_S_PER_PIXEL_VIEW[0] * h * w * v   # (0 at the first size)
        if host and predicted_s <= host_budget_s:
            t0 = time.perf_counter()
            ref = st.stereo_views(image, pred[:, None], layout, views, separation)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), layout
            row.update(host_stereo_views_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
            host_rate = max(host_rate, host_ms / 1e3 / (h * w * v))
        elif host:
            row["host"] = f"not timed at this size: about {predicted_s:.0f} s by the rate of the smaller size, above the budget of {host_budget_s:.0f} s"
        res["layouts"][layout] = row
    if host_rate:
        STEREO_HOST_S_PER_PIXEL_VIEW[0] = host_rate
    return res


PARALLAX_SHAPES = STEREO_SHAPES
PARALLAX_PATHS = (("orbit", dict(path="orbit", frames=16, amount=16.0)), ("dolly", dict(path="dolly", frames=16, push=0.02, zoom=1.25)))
PARALLAX_HOST_FRAMES = 2                 # the host route renders the first frames of a path only
PARALLAX_HOST_S_PER_PIXEL_FRAME = [0.0]  # as above, per pixel and frame


def bench_parallax(b, h, w, host, host_budget_s=60.0, timed=25):
    """gp_parallax_frames on preallocated buffers and engine.parallax_frames itself for the paths of PARALLAX_PATHS, depth space, the default
    edge and plane, with overscan, on the scene and image of bench_stereo, against parallax.parallax_frames on the host (its first
    PARALLAX_HOST_FRAMES frames); next to them gp_stereo_views for a side-by-side pair at separation 16 on the same arrays in the same run."""
    from genpercept_amd import engine as ge
    from genpercept_amd import parallax as pv
    from genpercept_amd import stereo as st
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    pred = case(b, h, w, 17)[0]
    pred[:, :, w // 2:] = np.clip(pred[:, :, w // 2:] + 0.2, 0, 1)
    ti, tp = torch.from_numpy(image).to(d), torch.from_numpy(pred).to(d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)
    plane = torch.full((b,), st.F_DEFAULT, dtype=torch.int32, device=d)
    res = dict(shape=[b, 3, h, w], options=dict(edge=st.EDGE_DEFAULT, focus=None, space="depth", overscan=True), launches_per_call=2, timed_calls=timed,
               statistic="median of `timed_calls` consecutive calls, each between two device events, after 0.3 s of the same call as warm-up", paths={})

    so = st.plan(b, h, w, "sbs", 2, 16.0)
    canvas = torch.empty((b, 3) + tuple(so["size"]), dtype=torch.uint8, device=d)
    sbytes = lib.gp_stereo_views_workspace(b, 2, h, w)
    sws = torch.empty((sbytes // 8,), dtype=torch.int64, device=d)

    def stereo_entry():
        rc = lib.gp_stereo_views(ti.data_ptr(), tp.data_ptr(), plane.data_ptr(), so["table"].ctypes.data, b, 2, h, w, so["size"][0], so["size"][1], 0, so["edge"],
                                 so["max_s8"], canvas.data_ptr(), None, None, sws.data_ptr(), sbytes, stream)
        assert rc == ge.GP_OK, rc

    stereo_ms = float(np.median(lens_timed_calls(stereo_entry, timed)))
    res["stereo_sbs_separation_16"] = dict(gp_stereo_views_us_per_call=1e3 * stereo_ms, us_per_view=1e3 * stereo_ms / 2, max_s8=so["max_s8"])
    host_rate = 0.0
    for name, kw in PARALLAX_PATHS:
        o = pv.plan(b, h, w, **kw)
        table, v = o["table"], int(o["table"].shape[0])
        out = torch.empty((b, v, 3, h, w), dtype=torch.uint8, device=d)
        nbytes = lib.gp_parallax_frames_workspace(b, v, h, w)
        ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=d)

        def entry():
            rc = lib.gp_parallax_frames(ti.data_ptr(), tp.data_ptr(), plane.data_ptr(), table.ctypes.data, b, v, h, w, 0, o["edge"], o["max_s8"],
                                        out.data_ptr(), None, None, ws.data_ptr(), nbytes, stream)
            assert rc == ge.GP_OK, rc

        entry_runs = sorted(lens_timed_calls(entry, timed))
        entry_ms = entry_runs[len(entry_runs) // 2]
        call = lambda: ge.parallax_frames(ti, tp, **kw)  # noqa: E731
        call_ms = float(np.median(lens_timed_calls(call, timed)))
        got, holes = (t.cpu().numpy() for t in ge.parallax_frames(ti, tp, want_holes=True, **kw))
        us_per_frame = 1e3 * entry_ms / v
        row = dict(frames=v, max_s8=o["max_s8"], zoom_first_last=[int(table[0, 3]), int(table[-1, 3])], workspace_bytes=int(nbytes),
                   gp_parallax_frames_us_per_call=1e3 * entry_ms, gp_parallax_frames_us_min_max=[1e3 * entry_runs[0], 1e3 * entry_runs[-1]],
                   us_per_frame=us_per_frame, frame_over_stereo_view=us_per_frame / (1e3 * stereo_ms / 2), engine_parallax_frames_us_per_call=1e3 * call_ms,
                   hole_share=float(holes.mean()))
        n_host = min(PARALLAX_HOST_FRAMES, v)
        predicted_s = PARALLAX_HOST_S_PER_PIXEL_FRAME[0] * h * w * n_host   # (0 at the first size)
        if host and predicted_s <= host_budget_s:
            t0 = time.perf_counter()
            ref = pv.parallax_frames(image, pred[:, None], frame_range=(0, n_host), **kw)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert got.dtype == ref.dtype and np.array_equal(got[:, :n_host], ref), name
            row.update(host_parallax_frames_ms=host_ms, host_frames=n_host, host_runs=1, host_ms_per_frame=host_ms / n_host,
                       host_frame_over_device_frame=host_ms / n_host / (entry_ms / v), output_equals_host=True)
            host_rate = max(host_rate, host_ms / 1e3 / (h * w * n_host))
        elif host:
            row["host"] = f"not timed at this size: about {predicted_s:.0f} s by the rate of the smaller size, above the budget of {host_budget_s:.0f} s"
        res["paths"][name] = row
    if host_rate:
        PARALLAX_HOST_S_PER_PIXEL_FRAME[0] = host_rate
    return res


RELIGHT_SHAPES = STEREO_SHAPES
RELIGHT_HOST_S_PER_PIXEL = {}   # as above, per pixel, for every case by its name (shading and marching cost differently)


def relight_cases():
    """name -> (the lights, whether the map is passed, which map)."""
    side = dict(azimuth=150.0, elevation=35.0, specular=0.5)
    three = [dict(side, reach=64), dict(azimuth=20.0, elevation=50.0, intensity=0.6, reach=64, softness=0.02), dict(azimuth=270.0, elevation=30.0, intensity=0.4, reach=64)]
    towards = [dict(azimuth=a, elevation=2.0, intensity=0.5, reach=64, softness=0.05) for a in (-30.0, 0.0, 30.0)]
    return dict(one_light_shading_only=([dict(side, shadows=False)], False, "scene"), one_light_reach_32=([dict(side, reach=32)], True, "scene"),
                three_lights_reach_64=(three, True, "scene"), worst_case_ramp_three_lights_reach_64=(towards, True, "ramp"))


def bench_relight(b, h, w, host, copy_gb_per_s, host_budget_s=60.0, timed=25):
    """gp_relight on preallocated buffers and engine.relight itself for the cases of `relight_cases`, disparity space, sRGB tables, ambient
    0.35, relief 256, on a scene (the smooth map with noise and an edge down the middle of `--stereo`, its normals by central differences,
    encoded) and on a ramp that rises towards its three lights faster than their rays, so that no march ends early, against relight.relight
    on the host.  The output bits are compared where the host runs."""
    from genpercept_amd import engine as ge
    from genpercept_amd import relight as rl
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(17)
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    scene = case(b, h, w, 17)[0]
    scene[:, :, w // 2:] = np.clip(scene[:, :, w // 2:] + 0.2, 0, 1)
    ramp = np.broadcast_to(np.linspace(0.02, 0.98, w, dtype=np.float32)[None, None], (b, h, w)).copy()
    gy, gx = np.gradient(scene.astype(np.float64), axis=(1, 2))
    n = np.stack([256.0 * gx, 256.0 * gy, -np.ones_like(gx)], 1)     # (disparity space: nearer is larger, the surface tilts away from the rise)
    normal = (0.5 * n / np.sqrt((n * n).sum(1, keepdims=True)) + 0.5).astype(np.float32)
    maps = dict(scene=scene, ramp=ramp)
    ti, tn = torch.from_numpy(image).to(d), torch.from_numpy(normal).to(d)
    tm = {k: torch.from_numpy(v).to(d) for k, v in maps.items()}
    to_lin, from_lin = ge._lens_tables(None, d)
    out = torch.empty((b, 3, h, w), dtype=torch.uint8, device=d)
    stream = int(torch.cuda.current_stream(d).cuda_stream)
    opts = dict(ambient=0.35, relief=256.0, space="disparity")
    res = dict(shape=[b, 3, h, w], options=dict(opts, tables="srgb", encoded=True), launches_per_call=1, workspace_bytes=0, timed_calls=timed,
               statistic="median of `timed_calls` consecutive calls, each between two device events, after 0.3 s of the same call as warm-up", cases={})
    for name, (lights, with_map, which) in relight_cases().items():
        rows = rl.relight_lights(lights, opts["ambient"], opts["relief"])
        n_lights, reach = len(rows) - 1, int(rows[:-1, rl.REACH].max())
        tp = tm[which] if with_map else None

        def entry():
            rc = lib.gp_relight(ti.data_ptr(), tn.data_ptr(), tp.data_ptr() if with_map else None, None, rows.ctypes.data, to_lin.data_ptr(),
                                from_lin.data_ptr(), b, h, w, n_lights, 1, 0, 1, reach, out.data_ptr(), None, stream)
            assert rc == ge.GP_OK, rc

        entry_runs = sorted(lens_timed_calls(entry, timed))
        entry_ms = entry_runs[len(entry_runs) // 2]
        call = lambda: ge.relight(ti, tn, tp, lights=lights, want_shadow=True, **opts)  # noqa: E731
        call_ms = float(np.median(lens_timed_calls(call, timed)))
        got, shadow = (t.cpu().numpy() for t in call())
        moved = b * h * w * (18 + (4 if with_map else 0))    # three float planes and three bytes read, three bytes written, the map once
        row = dict(lights=n_lights, max_reach=reach, map=which if with_map else None, gp_relight_us_per_call=1e3 * entry_ms,
                   gp_relight_us_min_max=[1e3 * entry_runs[0], 1e3 * entry_runs[-1]], engine_relight_us_per_call=1e3 * call_ms,
                   shadowed_share=float((shadow > 0).mean()), bytes_moved=moved, gb_per_s=moved / entry_ms / 1e6, copy_gb_per_s=copy_gb_per_s)
        predicted_s = RELIGHT_HOST_S_PER_PIXEL.get(name, 0.0) * h * w   # (0 at the first size)
        if host and predicted_s <= host_budget_s:
            t0 = time.perf_counter()
            ref = rl.relight(image, normal, maps[which] if with_map else None, lights=lights, **opts)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), name
            row.update(host_relight_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
            RELIGHT_HOST_S_PER_PIXEL[name] = host_ms / 1e3 / (h * w)
        elif host:
            row["host"] = f"not timed at this size: about {predicted_s:.0f} s by the rate of the smaller size, above the budget of {host_budget_s:.0f} s"
        res["cases"][name] = row
    return res


MESH_SHAPES = GEOMETRY_SHAPES
MESH_STRIDES = (1, 2)


def bench_mesh(b, h, w, stride, host, copy_gb_per_s, cut=0.05, radius=2, timed=25):
    """gp_depth_mesh alone on preallocated buffers with the planes given, and the whole engine.depth_mesh, against mesh.depth_mesh on the
    host; the point-cloud call of engine.depth_geometry and the compaction launches of gp_depth_geometry in the same run as the yardstick."""
    from genpercept_amd import engine as ge
    from genpercept_amd import geometry as gm
    from genpercept_amd import mesh as ms
    d = torch.device("cuda", 0)
    lib = ge.load_library()
    rng = np.random.default_rng(13)
    pred = case(b, h, w, 13)[0]
    pred[:, :, w // 2:] = np.clip(pred[:, :, w // 2:] + 0.2, 0, 1)   # a depth edge down the middle
    image = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    o = ms.check_mesh_options(radius, stride=stride, cut=cut)
    cams = gm.check_cameras(None, b, h, w)
    tp, ti = torch.from_numpy(pred).to(d), torch.from_numpy(image).to(d)
    gh, gw = -(-h // stride), -(-w // stride)
    n_cap, m_cap = b * gh * gw, 2 * b * (gh - 1) * (gw - 1)
    planes = [torch.empty(s, dtype=t, device=d) for s, t in (((b, 3, h, w), torch.float32), ((b, 3, h, w), torch.float32), ((b, h, w), torch.uint8))]
    points = [torch.empty(s, dtype=t, device=d) for s, t in (((n_cap, 3), torch.float32), ((n_cap, 3), torch.float32), ((n_cap, 3), torch.uint8),
                                                            ((n_cap,), torch.int32), ((b + 1,), torch.int64))]
    arrays = [torch.empty(s, dtype=t, device=d) for s, t in (((n_cap, 3), torch.float32), ((n_cap, 3), torch.float32), ((n_cap, 3), torch.uint8),
                                                            ((n_cap, 2), torch.float32), ((n_cap,), torch.int32), ((m_cap, 3), torch.int32),
                                                            ((b + 1,), torch.int64), ((b + 1,), torch.int64))]
    g_bytes, m_bytes = int(lib.gp_depth_geometry_workspace(b, h, w, stride)), int(lib.gp_depth_mesh_workspace(b, h, w, stride))
    ws_g, ws_m = (torch.empty((n // 8,), dtype=torch.int64, device=d) for n in (g_bytes, m_bytes))
    stream = int(torch.cuda.current_stream(d).cuda_stream)

    def geometry_entry(with_points):
        rc = lib.gp_depth_geometry(tp.data_ptr(), None, ti.data_ptr(), cams.ctypes.data, b, h, w, 0, o["radius"], o["tau"], o["min_count"], o["min_cos"], stride,
                                   *[p.data_ptr() for p in planes], *[p.data_ptr() if with_points else None for p in points], ws_g.data_ptr(), g_bytes, stream)
        assert rc == ge.GP_OK, rc

    def mesh_entry():
        rc = lib.gp_depth_mesh(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), ti.data_ptr(), b, h, w, stride, o["cut"],
                               *[a.data_ptr() for a in arrays], ws_m.data_ptr(), m_bytes, stream)
        assert rc == ge.GP_OK, rc

    def median_ms(call):
        runs = sorted(lens_timed_calls(call, timed))
        return runs[len(runs) // 2], [runs[0], runs[-1]]

    geometry_entry(False)
    mesh_ms, mesh_min_max = median_ms(mesh_entry)
    planes_ms, _ = median_ms(lambda: geometry_entry(False))
    cloud_ms, _ = median_ms(lambda: geometry_entry(True))
    kw = dict(radius=radius, stride=stride)
    call_ms, _ = median_ms(lambda: ge.depth_mesh(tp, None, ti, cut=cut, **kw))
    yard_ms, _ = median_ms(lambda: ge.depth_geometry(tp, None, ti, **kw))
    got = ge.depth_mesh(tp, None, ti, cut=cut, **kw)
    n, m, points_n = int(got["vertex_offsets"][-1]), int(got["face_offsets"][-1]), int(ge.depth_geometry(tp, None, ti, **kw)["offsets"][-1])
    read, written = 5 * n_cap + 27 * n, 39 * n + 12 * m
    compact_ms, compact_bytes = cloud_ms - planes_ms, n_cap + 27 * points_n + 31 * points_n
    res = dict(shape=[b, 1, h, w], options=dict(o, space="depth"), input="smooth map with noise and a depth edge down the middle; random image; default camera",
               grid=[gh, gw], vertices=n, faces=m, vertices_worst_case=n_cap, faces_worst_case=m_cap, kept_grid_pixels=points_n,
               gp_depth_mesh_us_per_call=1e3 * mesh_ms, gp_depth_mesh_us_min_max=[1e3 * v for v in mesh_min_max], timed_calls=timed,
               statistic="median of `timed_calls` consecutive calls, each between two device events, after 0.3 s of the same call as warm-up",
               launches_per_call=4, workspace_bytes=m_bytes, bytes_read=read, bytes_written=written,
               bytes_rule="read 5 B/node and 27 B/vertex; written 39 B/vertex and 12 B/face; the workspace (1 B/node twice, 16 B/segment) not counted",
               gb_per_s=(read + written) / mesh_ms / 1e6, copy_gb_per_s=copy_gb_per_s, over_copy_rate=(read + written) / mesh_ms / 1e6 / copy_gb_per_s,
               bytes_alone_us=(read + written) / copy_gb_per_s / 1e3, engine_depth_mesh_us_per_call=1e3 * call_ms,
               yardstick=dict(engine_depth_geometry_us_per_call=1e3 * yard_ms, gp_depth_geometry_planes_only_us=1e3 * planes_ms,
                              gp_depth_geometry_with_points_us=1e3 * cloud_ms, count_scan_scatter_us=1e3 * compact_ms, count_scan_scatter_bytes=compact_bytes,
                              count_scan_scatter_gb_per_s=compact_bytes / max(compact_ms, 1e-9) / 1e6,
                              bytes_rule="read 1 B/node and 27 B/point, written 31 B/point",
                              mesh_over_compaction_time=mesh_ms / max(compact_ms, 1e-9),
                              mesh_over_compaction_time_per_byte=(mesh_ms / (read + written)) / (max(compact_ms, 1e-9) / compact_bytes)))
    if host:
        t0 = time.perf_counter()
        ref = ms.depth_mesh(pred[:, None], None, image, cut=cut, **kw)
        host_ms = (time.perf_counter() - t0) * 1e3
        for k, v in ref.items():
            g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
            assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g.view(np.uint8), v.view(np.uint8)), k
        res.update(host_depth_mesh_ms=host_ms, host_runs=1, host_over_engine_call=host_ms / call_ms, output_equals_host=True)
    return res


def bench_loop(n_images, batch_sizes, repeats):
    from PIL import Image
    from genpercept_amd import GenPerceptPipeline
    from genpercept_amd import infer_eval as ie
    from oracle import sd21 as osd
    uc, vc = osd.UNetCfg.tiny(), osd.VAECfg.tiny()
    g = torch.Generator().manual_seed(0)
    pipe = GenPerceptPipeline(unet=osd.synth_state_dict(osd.unet_manifest(uc), 1), vae=osd.synth_state_dict(osd.vae_manifest(vc), 2),
                              scheduler=dict(beta_start=1.0, beta_end=1.0, prediction_type="v_prediction", clip_sample=False, steps_offset=1,
                                             timestep_spacing="leading"),
                              text_encoder=torch.randn(2, uc.cross_attention_dim, generator=g), tokenizer=None)
    pipe.to("cuda")
    out = {}
    with tempfile.TemporaryDirectory() as base:
        rng = np.random.RandomState(0)
        samples = []
        os.makedirs(os.path.join(base, "s", "color"))
        os.makedirs(os.path.join(base, "s", "depth"))
        for i in range(n_images):
            Image.fromarray(rng.randint(0, 255, (480, 640, 3), dtype=np.uint8)).save(os.path.join(base, "s", "color", f"{i:06d}.png"))
            Image.fromarray((1000 * (0.8 + 8 * rng.rand(480, 640))).astype(np.uint16)).save(os.path.join(base, "s", "depth", f"{i:06d}.png"))
            samples.append([f"s/color/{i:06d}.png", f"s/depth/{i:06d}.png"])
        means = {}
        for bs in batch_sizes:
            ie.infer_and_evaluate(pipe, base, samples[:bs], "scannet", batch_size=bs, processing_res=0)  # warm-up of this batch shape
            best = float("inf")
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                means[bs] = ie.infer_and_evaluate(pipe, base, samples, "scannet", batch_size=bs, processing_res=0)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            out[f"batch_size_{bs}_images_per_s"] = n_images / best
        # the host loop it replaces: run_inference (.npy per image) + evaluate_predictions
        with tempfile.TemporaryDirectory() as pred_dir:
            ie.run_inference(pipe, base, samples[:1], pred_dir, ie.FileNameMode.id, processing_res=0)
            t0 = time.perf_counter()
            ie.run_inference(pipe, base, samples, pred_dir, ie.FileNameMode.id, processing_res=0)
            ie.evaluate_predictions(pred_dir, base, samples, dataset="scannet")
            out["host_loop_run_inference_plus_evaluate_predictions_images_per_s"] = n_images / (time.perf_counter() - t0)
    out.update(n_images=n_images, image_size=[480, 640], pipeline="tiny synthetic weights, bf16, VAE-decoder head", repeats=repeats)
    pipe._engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--normals", action="store_true", help="time engine.eval_normal against normal_angular_error instead")
    ap.add_argument("--masks", action="store_true", help="time gp_eval_mask against mask_metrics instead")
    ap.add_argument("--structure", action="store_true", help="time gp_eval_structure against structure_metrics instead")
    ap.add_argument("--matting", action="store_true", help="time gp_eval_matting against matting_metrics instead")
    ap.add_argument("--seg", action="store_true", help="time gp_eval_seg against seg_metrics instead")
    ap.add_argument("--band", action="store_true", help="time gp_mask_band, eval_trimap and eval_boundary_iou against their host routes instead")
    ap.add_argument("--foreground", action="store_true", help="time gp_foreground / engine.cutout against foreground.cutout_rgba instead")
    ap.add_argument("--n-big", type=int, default=2, help="with --foreground: iterations of a level above 32 x 32 (1 .. 4)")
    ap.add_argument("--trace-run", action="store_true", help="with --foreground: the device calls alone, for a kernel trace taken around this run")
    ap.add_argument("--kernel-trace", default=None, help="with --foreground: the kernel trace csv of a --trace-run, for the per-level times")
    ap.add_argument("--guided", action="store_true", help="time gp_guided_upsample / engine.guided_upsample against guided.guided_upsample instead")
    ap.add_argument("--tiles", action="store_true", help="time gp_tile_merge / engine.tile_merge against tiled.tile_merge instead")
    ap.add_argument("--geometry", action="store_true", help="time gp_depth_geometry / engine.depth_geometry against geometry.depth_geometry instead")
    ap.add_argument("--lens-blur", action="store_true", help="time gp_lens_blur / engine.lens_blur against lens_blur.lens_blur instead")
    ap.add_argument("--stereo", action="store_true", help="time gp_stereo_views / engine.stereo_views against stereo.stereo_views instead")
    ap.add_argument("--parallax", action="store_true", help="time gp_parallax_frames / engine.parallax_frames against parallax.parallax_frames instead")
    ap.add_argument("--relight", action="store_true", help="time gp_relight / engine.relight against relight.relight instead")
    ap.add_argument("--mesh", action="store_true", help="time gp_depth_mesh / engine.depth_mesh against mesh.depth_mesh instead")
    ap.add_argument("--no-host", action="store_true",
                    help="with --structure, --matting, --seg, --band, --foreground, --guided, --tiles, --geometry, --lens-blur, --stereo, --parallax, "
                         "--relight or --mesh: the device calls alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU")
    if a.mesh:
        import bench
        bw = copy_bandwidth(torch.device("cuda", 0))
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_mesh(*s, stride, not a.no_host, bw) for s in MESH_SHAPES for stride in MESH_STRIDES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, mesh=rows)
    elif a.relight:
        import bench
        bw = copy_bandwidth(torch.device("cuda", 0))
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_relight(*s, not a.no_host, bw) for s in RELIGHT_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, relight=rows)
    elif a.parallax:
        import bench
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_parallax(*s, not a.no_host) for s in PARALLAX_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   parallax=rows)
    elif a.stereo:
        import bench
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_stereo(*s, not a.no_host) for s in STEREO_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   stereo=rows)
    elif a.lens_blur:
        import bench
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_lens_blur(*s, a.iters, not a.no_host) for s in LENS_SHAPES]
        summary = clock.summary()
        mhz = LENS_CLOCK_MHZ
        for r in rows:
            for m in r["maps"].values():
                m["valu_issue_share"] = m["valu_instructions"] * LENS_VALU_ISSUE_CYCLES / (LENS_SIMDS * mhz * 1e6 * m["gp_lens_blur_us_per_call"] * 1e-6)
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=summary,
                   shader_clock_mhz_used=mhz, lens_blur=rows)
    elif a.geometry:
        import bench
        bw = copy_bandwidth(torch.device("cuda", 0))
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_geometry(*s, a.iters, not a.no_host, bw) for s in GEOMETRY_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, geometry=rows)
    elif a.tiles:
        import bench
        bw = copy_bandwidth(torch.device("cuda", 0))
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_tiles(*s, a.iters, not a.no_host, bw) for s in TILE_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, tiles=rows)
    elif a.guided:
        import bench
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_guided(*s, a.iters, not a.no_host) for s in GUIDED_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   guided=rows)
    elif a.foreground:
        import bench
        if a.trace_run:
            print(json.dumps([bench_foreground(b, h, w, a.iters, False, 0.0, {}, True, a.n_big) for (b, h, w) in FOREGROUND_SHAPES]))
            return
        bw = copy_bandwidth(torch.device("cuda", 0))
        level_ms = foreground_level_times(a.kernel_trace) if a.kernel_trace else {}
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_foreground(b, h, w, a.iters, not a.no_host, bw, level_ms, False, a.n_big) for (b, h, w) in FOREGROUND_SHAPES]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, per_level_times="rocprofv3 kernel trace of a separate run" if level_ms else "not measured", foreground=rows)
    elif a.band:
        import bench
        bw = copy_bandwidth(torch.device("cuda", 0))
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_band(b, h, w, a.iters, not a.no_host, bw) for (b, h, w) in ((4, 480, 640), (1, 2048, 2048))]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   copy_gb_per_s=bw, band=rows)
    elif a.seg:
        import bench
        with bench.ClockPowerSampler("cuda:0") as clock:
            rows = [bench_eval_seg(b, h, w, K, a.iters, not a.no_host) for (b, h, w, K) in ((4, 480, 640, 19), (4, 480, 640, 150), (1, 2048, 2048, 150))]
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box", build_id=bench.source_build_id(), clock=clock.summary(),
                   eval_seg=rows)
    elif a.matting:
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box",
                   eval_matting=[bench_eval_matting(b, h, w, a.iters, not a.no_host) for (b, h, w) in ((4, 480, 640), (1, 2048, 2048))])
    elif a.structure:
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box",
                   eval_structure=[bench_eval_structure(b, h, w, kind, a.iters, not a.no_host) for (b, h, w) in ((4, 1024, 1024), (1, 2048, 2048))
                                   for kind in ("mask", "far")])
    elif a.masks:
        bw = copy_bandwidth(torch.device("cuda", 0))
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box",
                   eval_mask=[bench_eval_mask(b, h, w, kind, a.iters, runs, bw) for (b, h, w, runs) in ((4, 1024, 1024, 3), (1, 4032, 6048, 1))
                              for kind in ("mask", "uniform")])
    elif a.normals:
        res = dict(device=torch.cuda.get_device_name(0), note="measured once on one pool box",
                   eval_normal=[bench_eval_normal(4, 480, 640, a.iters, 3), bench_eval_normal(1, 4032, 6048, a.iters, 1)])
    else:
        res = dict(device=torch.cuda.get_device_name(0), eval_depth=[bench_eval(1, 4032, 6048, a.iters, 1), bench_eval(4, 480, 640, a.iters, 3)])
    if (not a.skip_loop and not a.normals and not a.masks and not a.structure and not a.matting and not a.seg and not a.band and not a.foreground
            and not a.guided and not a.tiles and not a.geometry and not a.lens_blur and not a.stereo and not a.parallax and not a.relight and not a.mesh):
        res["infer_and_evaluate"] = bench_loop(16, (1, 4), 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
