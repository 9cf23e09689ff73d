"""Depth evaluation protocol next to the hot path: least-squares alignment and the ten metrics
`eval.py` reports, restated in numpy (float64) so "AbsRel unchanged" can be stated for predictions of this engine.

Semantics follow /root/reference/src/util/alignment.py:29-94 (align_depth_least_square, depth2disparity) and
/root/reference/src/util/metric.py:34-158; pinned by tests/golden/metrics_ref.npz (outputs of those reference functions).
Per-image masked means, then a mean over images — exactly the reference's reduction order.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np


def _nearest_downscale(x: np.ndarray, scale: float) -> np.ndarray:
    """What alignment.py:45-55 does to a [H, W] array: torch.nn.Upsample(scale_factor, mode="nearest") applied to the [1, H, W] tensor,
    which torch reads as (batch, channels, length) -- so only the LAST axis is resampled: width floor(W * scale), source column
    floor(dst * (1 / scale)).  Kept as is: the evaluation protocol is defined by what the reference computes."""
    w = x.shape[-1]
    ow = int(np.floor(w * scale))
    ix = np.minimum(np.floor(np.arange(ow) * np.float32(1.0 / scale)).astype(np.int64), w - 1)
    return x[..., ix]


def align_depth_least_square(gt: np.ndarray, pred: np.ndarray, valid_mask: np.ndarray, max_resolution: Optional[int] = None) -> Tuple[np.ndarray, float, float]:
    """min_{s,t} || s * pred + t - gt ||^2 over valid pixels; returns (s * pred + t, s, t).  With max_resolution the fit runs on a
    nearest-downscaled copy (alignment.py:43-55) and the result is applied to the full-resolution prediction."""
    g = np.asarray(gt).squeeze()
    p = np.asarray(pred).squeeze()
    m = np.asarray(valid_mask).squeeze().astype(bool)
    if max_resolution is not None:
        scale = float(np.min(max_resolution / np.array(np.asarray(pred).shape[-2:])))
        if scale < 1:
            g, p, m = _nearest_downscale(g, scale), _nearest_downscale(p, scale), _nearest_downscale(m, scale)
    a = np.stack([p[m], np.ones_like(p[m])], axis=1)
    x = np.linalg.lstsq(a, g[m], rcond=None)[0]
    scale, shift = float(x[0]), float(x[1])
    return np.asarray(pred) * scale + shift, scale, shift


def depth2disparity(depth: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    d = np.zeros_like(depth)
    pos = depth > 0
    d[pos] = 1.0 / depth[pos]
    return d, pos


def disparity2depth(disparity: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    return depth2disparity(disparity)  # alignment.py:93-94


def _masked_mean(x: np.ndarray, mask: Optional[np.ndarray]) -> np.ndarray:
    if mask is None:
        return x.mean(axis=(-1, -2))
    return np.where(mask, x, 0.0).sum(axis=(-1, -2)) / mask.sum(axis=(-1, -2))


def abs_relative_difference(out, tgt, mask=None) -> float:
    return float(_masked_mean(np.abs(out - tgt) / tgt, mask).mean())


def squared_relative_difference(out, tgt, mask=None) -> float:
    return float(_masked_mean(np.abs(out - tgt) ** 2 / tgt, mask).mean())


def rmse_linear(out, tgt, mask=None) -> float:
    return float(np.sqrt(_masked_mean((out - tgt) ** 2, mask)).mean())


def rmse_log(out, tgt, mask=None) -> float:
    return float(np.sqrt(_masked_mean((np.log(out) - np.log(tgt)) ** 2, mask)).mean())


def log10(out, tgt, mask=None) -> float:
    d = np.abs(np.log10(out) - np.log10(tgt))
    return float(d[mask].mean() if mask is not None else d.mean())


def threshold_percentage(out, tgt, thr: float, mask=None) -> float:
    r = np.maximum(out / tgt, tgt / out)
    return float(_masked_mean((r < thr).astype(np.float64), mask).mean())


def delta1_acc(out, tgt, mask=None) -> float:
    return threshold_percentage(out, tgt, 1.25, mask)


def delta2_acc(out, tgt, mask=None) -> float:
    return threshold_percentage(out, tgt, 1.25 ** 2, mask)


def delta3_acc(out, tgt, mask=None) -> float:
    return threshold_percentage(out, tgt, 1.25 ** 3, mask)


def i_rmse(out, tgt, mask=None) -> float:
    return float(np.sqrt(_masked_mean((1.0 / out - 1.0 / tgt) ** 2, mask)).mean())


def silog_rmse(out, tgt, mask=None) -> float:
    diff = np.log(out) - np.log(tgt)
    if mask is not None:
        diff = np.where(mask, diff, 0.0)
        n = mask.sum(axis=(-1, -2))
    else:
        n = diff.shape[-1] * diff.shape[-2]
    first = (diff ** 2).sum(axis=(-1, -2)) / n
    second = diff.sum(axis=(-1, -2)) ** 2 / (n ** 2)
    return float(np.sqrt(np.mean(first - second)) * 100)


METRICS = {f.__name__: f for f in (abs_relative_difference, squared_relative_difference, rmse_linear, rmse_log, log10, delta1_acc, delta2_acc,
                                    delta3_acc, i_rmse, silog_rmse)}


def evaluate_depth(pred: np.ndarray, gt: np.ndarray, valid_mask: np.ndarray, min_depth: float = 1e-3, max_depth: float = 10.0,
                   alignment: str = "least_square", alignment_max_res: Optional[int] = None) -> Dict[str, float]:
    """eval.py:168-215 for one image: LS alignment in depth space ("least_square") or in disparity space ("least_square_disparity"),
    clip to the dataset range and to d > 0, ten metrics."""
    pred = np.asarray(pred)
    gt_a = np.asarray(gt)
    vm = np.asarray(valid_mask).astype(bool)
    if alignment == "least_square":
        aligned, _, _ = align_depth_least_square(gt_a, pred, vm, alignment_max_res)
    elif alignment == "least_square_disparity":
        gt_disp, gt_pos = depth2disparity(gt_a)
        m = vm & gt_pos & (pred > 0)
        disp, _, _ = align_depth_least_square(gt_disp, pred, m, alignment_max_res)
        aligned, _ = disparity2depth(np.clip(disp, 1e-3, None))
    elif alignment in (None, "", "none"):
        aligned = pred
    else:
        raise NotImplementedError(alignment)
    aligned = np.clip(np.clip(aligned, min_depth, max_depth), 1e-6, None)
    a, g, m = (np.asarray(x, dtype=np.float64)[None] for x in (aligned.squeeze(), gt_a.squeeze(), vm.squeeze()))
    m = m.astype(bool)
    return {k: f(a, g, m) for k, f in METRICS.items()}


# ---- surface normals ---------------------------------------------------------------------------------------------------------------------
# The reference has no normal EVALUATION script; the only definition of "angular error" in its tree is angular_loss
# (genpercept/losses/geometry_losses.py:550-590): cosine similarity along the channel axis, clamped to [-1 + eps, 1 - eps] (eps 1e-4),
# acos, mean over the valid pixels.  The evaluator below is that quantity (radians -> degrees) plus the summary statistics normal
# benchmarks report; pinned to the reference function by tests/golden/datasets_ref.npz.
def normal_angular_error(pred: np.ndarray, gt: np.ndarray, valid_mask: Optional[np.ndarray] = None, eps: float = 1e-4) -> Dict[str, float]:
    """pred, gt: [..., 3, H, W] normal maps (any scale: only directions matter); valid_mask: [..., 1 | absent, H, W] or None.
    pred may be the pipeline's [0, 1] encoding: pass decode_normals(pred_np) first."""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    num = (p * g).sum(axis=-3)
    den = np.maximum(np.linalg.norm(p, axis=-3), 1e-8) * np.maximum(np.linalg.norm(g, axis=-3), 1e-8)  # torch.cosine_similarity's eps
    ang = np.arccos(np.clip(num / den, -1.0 + eps, 1.0 - eps))
    if valid_mask is not None:
        m = np.asarray(valid_mask).astype(bool)
        if m.ndim == ang.ndim + 1:
            m = m[..., 0, :, :]
        ang = ang[m]
    else:
        ang = ang.reshape(-1)
    deg = np.degrees(ang)
    return {"mean_rad": float(ang.mean()), "mean_deg": float(deg.mean()), "median_deg": float(np.median(deg)), "rmse_deg": float(np.sqrt((deg ** 2).mean())),
            "within_11.25": float((deg < 11.25).mean()), "within_22.5": float((deg < 22.5).mean()), "within_30": float((deg < 30.0).mean())}


def decode_normals(pred_np: np.ndarray) -> np.ndarray:
    """GenPerceptOutput.pred_np of mode='normal' is [H, W, 3] in [0, 1] = (n + 1) / 2 (genpercept_pipeline.py:469-472): back to [3, H, W] in [-1, 1]."""
    return np.moveaxis(np.asarray(pred_np, dtype=np.float64) * 2.0 - 1.0, -1, -3)


# ---- dis / matting ------------------------------------------------------------------------------------------------------------------------
# The reference has no metric for its dis and matting checkpoints (genpercept_trainer.py:1169 is a TODO).  The definitions below are this
# project's, stated once in include/genpercept_hip.h (gp_eval_mask): everything is computed on the 8-BIT prediction -- the byte run.py:449-455
# saves -- against an 8-bit ground truth, so every per-pixel quantity is an integer, the reductions are exact, and each value is one fixed
# sequence of float64 operations on integer counts.  The device entry runs the same sequence and is bit-equal.
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
MASK_COUNTS = 4 + 2 * 256  # n, sum_q, sad, sse, hist_bg[256], hist_fg[256]


def quantize_mask(pred: np.ndarray) -> np.ndarray:
    """(clip(pred, 0, 1) * 255).astype(uint8) with the product in float32 and NaN -> 0 (run.py:449-455); uint8 input is returned as it is."""
    pred = np.asarray(pred)
    if pred.dtype == np.uint8:
        return pred
    if not np.issubdtype(pred.dtype, np.floating):
        raise ValueError(f"a float map in [0, 1] or its uint8 quantisation, got {pred.dtype}")
    x = pred.astype(np.float32)
    x = np.clip(np.where(np.isnan(x), np.float32(0.0), x), np.float32(0.0), np.float32(1.0))
    return (x * np.float32(255.0)).astype(np.uint8)


def mask_counts(q: np.ndarray, g: np.ndarray, region: Optional[np.ndarray] = None) -> np.ndarray:
    """The integer counts of one image, int64 [516] = n, sum q, sum |q - g|, sum (q - g)^2, hist_bg[256] (counts of q where g <= 128),
    hist_fg[256] (where g > 128), over the pixels with region != 0 (None: all).  q, g: uint8 arrays of one shape."""
    q, g = np.asarray(q), np.asarray(g)
    if q.dtype != np.uint8 or g.dtype != np.uint8 or q.shape != g.shape:
        raise ValueError(f"q and g must be uint8 arrays of one shape, got {q.dtype} {q.shape} and {g.dtype} {g.shape}")
    q, g = q.reshape(-1), g.reshape(-1)
    if region is not None:
        sel = np.asarray(region).reshape(-1) != 0
        if sel.shape != q.shape:
            raise ValueError("region does not match the maps")
        q, g = q[sel], g[sel]
    qi, gi = q.astype(np.int64), g.astype(np.int64)
    d = np.abs(qi - gi)
    fg = g > 128
    out = np.empty(MASK_COUNTS, dtype=np.int64)
    out[0], out[1], out[2], out[3] = q.size, qi.sum(), d.sum(), (d * d).sum()
    out[4:260] = np.bincount(q[~fg], minlength=256)
    out[260:516] = np.bincount(q[fg], minlength=256)
    return out


def mask_curves_from_counts(counts) -> Tuple[list, list, list]:
    """(precision, recall, F) for the 256 thresholds "q >= t", Python floats: TP_t = sum_{v >= t} hist_fg[v], P_t = TP_t + sum_{v >= t}
    hist_bg[v], prec = TP_t / max(P_t, 1), rec = TP_t / max(n_fg, 1), F_t = (1.3 * prec * rec) / (0.3 * prec + rec), 0.0 when the
    denominator is 0 (beta^2 = 0.3)."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != MASK_COUNTS:
        raise ValueError(f"expected {MASK_COUNTS} counts, got {len(c)}")
    hist_bg, hist_fg = c[4:260], c[260:516]
    n_fg = sum(hist_fg)
    prec, rec, f = [0.0] * 256, [0.0] * 256, [0.0] * 256
    tp = bgp = 0
    for t in range(255, -1, -1):
        tp += hist_fg[t]
        bgp += hist_bg[t]
        p, r = tp / max(tp + bgp, 1), tp / max(n_fg, 1)
        den = 0.3 * p + r
        prec[t], rec[t], f[t] = p, r, ((1.3 * p * r) / den if den != 0.0 else 0.0)
    return prec, rec, f


def mask_metrics_from_counts(counts) -> Dict[str, float]:
    """The values of gp_eval_mask's `out` from the counts, in its order: n, n_fg, mae, mse, sad, max_f, mean_f, adp_f, iou, t_max (n and n_fg
    ints; n = 0: NaN for the other eight).  Plain float64 *, /, + in the order the header prescribes; the 256-term sum runs left to right."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != MASK_COUNTS:
        raise ValueError(f"expected {MASK_COUNTS} counts, got {len(c)}")
    n, sum_q, sad, sse = c[:4]
    hist_bg, hist_fg = c[4:260], c[260:516]
    n_fg = sum(hist_fg)
    if n == 0:
        nan = float("nan")
        return dict(n=0, n_fg=0, mae=nan, mse=nan, sad=nan, max_f=nan, mean_f=nan, adp_f=nan, iou=nan, t_max=nan)
    _, _, f = mask_curves_from_counts(c)
    total, best, t_max = f[0], f[0], 0
    for t in range(1, 256):
        total = total + f[t]
        if f[t] > best:
            best, t_max = f[t], t
    t_a = (min(2 * sum_q, 255 * n) + n - 1) // n  # the smallest integer with t_a * n >= min(2 * sum_q, 255 * n)
    tp = sum(hist_fg[128:])
    union = tp + sum(hist_bg[128:]) + n_fg - tp
    return dict(n=n, n_fg=n_fg, mae=sad / (255.0 * n), mse=sse / (65025.0 * n), sad=sad / 255000.0, max_f=best, mean_f=total / 256.0,
                adp_f=f[t_a], iou=(tp / union if union != 0 else 0.0), t_max=float(t_max))


def mask_metrics(pred: np.ndarray, gt: np.ndarray, region: Optional[np.ndarray] = None) -> Dict[str, float]:
    """One image: pred a float map in [0, 1] (quantised by `quantize_mask`) or uint8, gt uint8, region optional (non-zero = scored)."""
    return mask_metrics_from_counts(mask_counts(quantize_mask(pred), gt, region))


# ---- dis structure scores: S-measure, E-measure, weighted F -------------------------------------------------------------------------------
# The other three columns of the DIS5K table.  Definitions: include/genpercept_hip.h (gp_eval_structure); the functions below restate them.
# S and E are fixed sequences of float64 operations on integer counts (bit-equal to the device); the weighted F shares keys, Et, E, EA and
# the minimum with the device bit for bit and differs in exp's last bits and in the order of the two float64 sums.
STRUCTURE_METRICS = ["s_alpha", "max_e", "mean_e", "adp_e", "wf"]
STRUCTURE_COUNTS = 5 + 20 + 2 * 256  # n_fg, sum_fg x, sum_fg y, cx, cy, 4 x (N, a, a2, b, c), hist_bg[256], hist_fg[256]
EDT_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)  # every key of an image without foreground
# the normalised 7 x 7 Gaussian, sigma = 5 (the same literals as csrc/eval_structure.hip ES_K)
WF_K_HEX = """
    0x1.1075d7f1e0af6p-6, 0x1.2d1d7fa535fb0p-6, 0x1.3fbc331b753f8p-6, 0x1.4631b947fa56fp-6, 0x1.3fbc331b753f8p-6, 0x1.2d1d7fa535fb0p-6, 0x1.1075d7f1e0af6p-6,
    0x1.2d1d7fa535fb0p-6, 0x1.4cc8a6b9e9761p-6, 0x1.615cabadc2e2fp-6, 0x1.688018ee505f7p-6, 0x1.615cabadc2e2fp-6, 0x1.4cc8a6b9e9761p-6, 0x1.2d1d7fa535fb0p-6,
    0x1.3fbc331b753f8p-6, 0x1.615cabadc2e2fp-6, 0x1.77367232eb477p-6, 0x1.7ecadfe6d5847p-6, 0x1.77367232eb477p-6, 0x1.615cabadc2e2fp-6, 0x1.3fbc331b753f8p-6,
    0x1.4631b947fa56fp-6, 0x1.688018ee505f7p-6, 0x1.7ecadfe6d5847p-6, 0x1.8686809d3875ep-6, 0x1.7ecadfe6d5847p-6, 0x1.688018ee505f7p-6, 0x1.4631b947fa56fp-6,
    0x1.3fbc331b753f8p-6, 0x1.615cabadc2e2fp-6, 0x1.77367232eb477p-6, 0x1.7ecadfe6d5847p-6, 0x1.77367232eb477p-6, 0x1.615cabadc2e2fp-6, 0x1.3fbc331b753f8p-6,
    0x1.2d1d7fa535fb0p-6, 0x1.4cc8a6b9e9761p-6, 0x1.615cabadc2e2fp-6, 0x1.688018ee505f7p-6, 0x1.615cabadc2e2fp-6, 0x1.4cc8a6b9e9761p-6, 0x1.2d1d7fa535fb0p-6,
    0x1.1075d7f1e0af6p-6, 0x1.2d1d7fa535fb0p-6, 0x1.3fbc331b753f8p-6, 0x1.4631b947fa56fp-6, 0x1.3fbc331b753f8p-6, 0x1.2d1d7fa535fb0p-6, 0x1.1075d7f1e0af6p-6"""
WF_K = np.array([float.fromhex(v) for v in WF_K_HEX.replace("\n", " ").split(",")], dtype=np.float64).reshape(7, 7)
WF_C = float.fromhex("-0x1.1be9bff2e94bfp-3")  # log(0.5) / 5


def _check_q_g(q, g):
    q, g = np.asarray(q), np.asarray(g)
    if q.dtype != np.uint8 or g.dtype != np.uint8 or q.shape != g.shape or q.ndim != 2:
        raise ValueError(f"q and g must be uint8 [H, W] arrays of one shape, got {q.dtype} {q.shape} and {g.dtype} {g.shape}")
    if q.shape[0] < 1 or q.shape[1] < 1 or q.shape[0] > 32767 or q.shape[1] > 32767 or q.size > 0x7FFFFFFF:
        raise ValueError(f"1 <= H, W <= 32767 and H * W <= 2^31 - 1, got {q.shape}")
    return q, g


def structure_counts(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """The integer counts of one image behind S and E, int64 [537] = n_fg, sum_fg x, sum_fg y, cx, cy, then for the blocks LT, RT, LB, RB the
    centroid cuts (N, a = sum q, a2 = sum q^2, b = sum G, c = sum q G), then hist_bg[256], hist_fg[256].  q, g: uint8 [H, W]; G = g > 128."""
    q, g = _check_q_g(q, g)
    h, w = q.shape
    fg = g > 128
    out = np.zeros(STRUCTURE_COUNTS, dtype=np.int64)
    ys, xs = np.nonzero(fg)
    n_fg = int(ys.size)
    sx, sy = int(xs.sum()), int(ys.sum())
    cx = (2 * sx + n_fg) // (2 * n_fg) if n_fg else 0
    cy = (2 * sy + n_fg) // (2 * n_fg) if n_fg else 0
    out[:5] = n_fg, sx, sy, cx, cy
    qi, gi = q.astype(np.int64), fg.astype(np.int64)
    for k, (rows, cols) in enumerate(((slice(0, cy + 1), slice(0, cx + 1)), (slice(0, cy + 1), slice(cx + 1, w)),
                                      (slice(cy + 1, h), slice(0, cx + 1)), (slice(cy + 1, h), slice(cx + 1, w)))):
        qq, gg = qi[rows, cols], gi[rows, cols]
        out[5 + 5 * k:10 + 5 * k] = qq.size, qq.sum(), (qq * qq).sum(), gg.sum(), (qq * gg).sum()
    out[25:281] = np.bincount(q[~fg], minlength=256)
    out[281:537] = np.bincount(q[fg], minlength=256)
    return out


def _e_term(p: float, g: float, mp: float, mg: float) -> float:
    ap, ag = p - mp, g - mg
    phi = ((2.0 * ap) * ag) / (ap * ap + ag * ag)
    return ((phi + 1.0) * (phi + 1.0)) / 4.0


def e_curve_from_counts(counts) -> list:
    """E_t for the 256 thresholds "q >= t" from the two class histograms (Python floats)."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != STRUCTURE_COUNTS:
        raise ValueError(f"expected {STRUCTURE_COUNTS} counts, got {len(c)}")
    hist_bg, hist_fg = c[25:281], c[281:537]
    n_fg = sum(hist_fg)
    n = n_fg + sum(hist_bg)
    dm1 = float(max(n - 1, 1))
    e = [0.0] * 256
    tp = bp = 0
    for t in range(255, -1, -1):
        tp += hist_fg[t]
        bp += hist_bg[t]
        p = tp + bp
        if n_fg == 0:
            e[t] = float(n - p) / dm1
        elif n_fg == n:
            e[t] = float(p) / dm1
        else:
            mp, mg = p / n, n_fg / n
            s = float(tp) * _e_term(1.0, 1.0, mp, mg)
            s = s + float(bp) * _e_term(1.0, 0.0, mp, mg)
            s = s + float(n_fg - tp) * _e_term(0.0, 1.0, mp, mg)
            s = s + float(n - n_fg - bp) * _e_term(0.0, 0.0, mp, mg)
            e[t] = s / dm1
    return e


def _s_object(N: int, a: int, a2: int) -> float:
    xb, m2 = a / (255.0 * N), a2 / (65025.0 * N)
    d = m2 - xb * xb
    if d < 0.0:
        d = 0.0
    var = 0.0 if N == 1 else (d * N) / (N - 1)
    return (2.0 * xb) / ((xb * xb + 1.0) + math.sqrt(var))


def _s_block(N: int, a: int, a2: int, b: int, c: int) -> float:
    xb, yb = a / (255.0 * N), b / N
    sxx = syy = sxy = 0.0
    if N > 1:
        sxx = (a2 / 65025.0 - (xb * xb) * N) / (N - 1)
        syy = (b - (yb * yb) * N) / (N - 1)
        sxy = (c / 255.0 - (xb * yb) * N) / (N - 1)
    A, Bq = ((4.0 * xb) * yb) * sxy, (xb * xb + yb * yb) * (sxx + syy)
    if A != 0.0 and Bq != 0.0:
        return A / Bq
    return 1.0 if A == 0.0 and Bq == 0.0 else 0.0


def structure_from_counts(counts) -> Dict[str, float]:
    """S and E from `structure_counts`: n, n_fg, s_alpha, s_object, s_region, max_e, mean_e, adp_e, cx, cy -- gp_eval_structure's values of
    the same names, bit for bit (s_object = s_region = NaN in the degenerate S branches)."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    e = e_curve_from_counts(c)
    hist_bg, hist_fg = c[25:281], c[281:537]
    n_fg = sum(hist_fg)
    n = n_fg + sum(hist_bg)
    total, best = e[0], e[0]
    for t in range(1, 256):
        total = total + e[t]
        if e[t] > best:
            best = e[t]
    sum_q = sum(v * (hist_bg[v] + hist_fg[v]) for v in range(256))
    t_a = (min(2 * sum_q, 255 * n) + n - 1) // n
    nan = float("nan")
    if n_fg == 0:
        s, so, sr = 1.0 - sum_q / (255.0 * n), nan, nan
    elif n_fg == n:
        s, so, sr = sum_q / (255.0 * n), nan, nan
    else:
        u = n_fg / n
        a_fg, a2_fg = sum(v * hist_fg[v] for v in range(256)), sum(v * v * hist_fg[v] for v in range(256))
        a_bg, a2_bg = sum((255 - v) * hist_bg[v] for v in range(256)), sum((255 - v) * (255 - v) * hist_bg[v] for v in range(256))
        so = u * _s_object(n_fg, a_fg, a2_fg) + (1.0 - u) * _s_object(n - n_fg, a_bg, a2_bg)
        sr = 0.0
        for k in range(4):
            N, a, a2, b, cc = c[5 + 5 * k:10 + 5 * k]
            if N != 0:
                sr = sr + (N / n) * _s_block(N, a, a2, b, cc)
        s = 0.5 * so + 0.5 * sr
        if s < 0.0:
            s = 0.0
    return dict(n=n, n_fg=n_fg, s_alpha=s, s_object=so, s_region=sr, max_e=best, mean_e=total / 256.0, adp_e=e[t_a], cx=c[3], cy=c[4])


def edt_keys(G: np.ndarray) -> np.ndarray:
    """The exact Euclidean distance transform with nearest-foreground indices of a boolean [H, W] array, as uint64 keys (d2 << 32 | idx): d2 the
    squared distance to the nearest True pixel, idx = y' * W + x' its row-major index, the smallest index among the equidistant ones (a True
    pixel: (0, itself)).  No True pixel: every key EDT_NO_KEY.  Two passes: per column the nearest True pixel above-or-at and below-or-at
    gives each (row, column) its better candidate key; per row, pixel x minimises key(x') + ((x - x')^2 << 32), one offset at a time, until
    the offset's square passes every pixel's best d2."""
    G = np.asarray(G).astype(bool)
    if G.ndim != 2 or G.shape[0] > 32767 or G.shape[1] > 32767:
        raise ValueError(f"a boolean [H, W] array with H, W <= 32767, got {G.shape}")
    h, w = G.shape
    if not G.any():
        return np.full((h, w), EDT_NO_KEY, dtype=np.uint64)
    far = np.uint64((0x7FFFFFFF << 32) | 0xFFFFFFFF)
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    up = np.maximum.accumulate(np.where(G, ys, -1), axis=0)                  # the nearest True row at or above, -1: none
    dn = np.minimum.accumulate(np.where(G, ys, h)[::-1], axis=0)[::-1]       # at or below, h: none
    ku = np.where(up >= 0, (((ys - up) ** 2) << 32) | (np.maximum(up, 0) * w + xs), 0).astype(np.uint64)
    ku[up < 0] = far
    kd = np.where(dn < h, (((dn - ys) ** 2) << 32) | (np.minimum(dn, h - 1) * w + xs), 0).astype(np.uint64)
    kd[dn >= h] = far
    col = np.minimum(ku, kd)
    best = col.copy()
    shift = np.uint64(32)
    for r in range(1, w):
        if r * r > int(best.max() >> shift):
            break
        add = np.uint64((r * r) << 32)
        np.minimum(best[:, r:], col[:, :-r] + add, out=best[:, r:])          # the candidate r columns to the left
        np.minimum(best[:, :-r], col[:, r:] + add, out=best[:, :-r])         # ... to the right
    return best


def weighted_f(q: np.ndarray, g: np.ndarray, keys: Optional[np.ndarray] = None) -> Dict[str, float]:
    """The weighted F-measure (beta^2 = 1) of the 8-bit prediction q against G = g > 128: wf, wf_precision, wf_recall, wf_sum_fg, wf_sum_bg as
    gp_eval_structure defines them (`keys`: edt_keys(G), computed here unless given)."""
    q, g = _check_q_g(q, g)
    h, w = q.shape
    fg = g > 128
    n_fg = int(fg.sum())
    if n_fg == 0:
        return dict(wf=0.0, wf_precision=0.0, wf_recall=0.0, wf_sum_fg=0.0, wf_sum_bg=0.0)
    if keys is None:
        keys = edt_keys(fg)
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    d2 = (keys >> np.uint64(32)).astype(np.float64)
    et = (255 - q.reshape(-1)[idx].astype(np.int64)).astype(np.float64) / 255.0
    e = np.where(fg, et, q.astype(np.float64) / 255.0)
    pad = np.zeros((h + 6, w + 6), dtype=np.float64)   # a tap outside the image adds K * 0.0 = +0.0: the same bits as skipping it
    pad[3:h + 3, 3:w + 3] = et
    ea = np.zeros((h, w), dtype=np.float64)
    for i in range(7):
        for j in range(7):
            ea = ea + WF_K[i, j] * pad[i:i + h, j:j + w]
    ew = np.where(fg, np.minimum(ea, e), e * (2.0 - np.exp(WF_C * np.sqrt(d2))))
    s_fg, s_bg = float(ew[fg].sum()), float(ew[~fg].sum())
    tpw = n_fg - s_fg
    rec = 1.0 - s_fg / n_fg
    den = tpw + s_bg
    prec = tpw / den if den != 0.0 else 0.0
    wf = ((2.0 * rec) * prec) / (rec + prec) if rec + prec != 0.0 else 0.0
    return dict(wf=wf, wf_precision=prec, wf_recall=rec, wf_sum_fg=s_fg, wf_sum_bg=s_bg)


def structure_metrics(pred: np.ndarray, gt: np.ndarray) -> Dict[str, float]:
    """One image: pred a float map in [0, 1] (quantised by `quantize_mask`) or uint8, gt uint8, both [H, W].  STRUCTURE_METRICS and the other
    values of `structure_from_counts` and `weighted_f`."""
    q = quantize_mask(pred)
    m = structure_from_counts(structure_counts(q, gt))
    m.update(weighted_f(q, gt))
    return m


# ---- matting: gradient and connectivity errors ----------------------------------------------------------------------------------------------
# The other two columns of the matting table beside SAD and MSE (Rhemann et al. 2009).  Definitions: include/genpercept_hip.h (gp_eval_matting);
# the functions below restate them.  Conn is integers up to one division (bit-equal to the device); the gradient error map is one prescribed
# sequence of float64 + - * / sqrt per pixel (bit-equal) and its sum differs from the device's in the order of the additions.
MATTING_METRICS = ["grad", "conn"]
MATTING_COUNTS = 2 + 11  # n, conn_num, the counts of the levels 0..10 over the whole image
CONN_T = [26, 51, 77, 102, 128, 153, 179, 204, 230, 255]  # T_k = ceil(255 k / 10), k = 1..10
# the 9-tap Gaussian (sigma = 1.4) and its derivative, each divided by its L2 norm (the same literals as csrc/eval_matting.hip MT_G, MT_D)
GRAD_G_HEX = """0x1.5f2161173037cp-7, 0x1.05c2b72947cf6p-4, 0x1.d49edcea5016bp-3, 0x1.f7af85f5976d7p-2, 0x1.4506d2f73739dp-1, 0x1.f7af85f5976d7p-2,
    0x1.d49edcea5016bp-3, 0x1.05c2b72947cf6p-4, 0x1.5f2161173037cp-7"""
GRAD_D_HEX = """0x1.62b49a56df053p-5, 0x1.8ca37e89855ffp-3, 0x1.d9645351e6fcbp-2, 0x1.fcd0621654797p-2, 0x0.0p+0, -0x1.fcd0621654797p-2,
    -0x1.d9645351e6fcbp-2, -0x1.8ca37e89855ffp-3, -0x1.62b49a56df053p-5"""
GRAD_G = np.array([float.fromhex(v) for v in GRAD_G_HEX.replace("\n", " ").split(",")], dtype=np.float64)
GRAD_D = np.array([float.fromhex(v) for v in GRAD_D_HEX.replace("\n", " ").split(",")], dtype=np.float64)


def _components_min_index(mask: np.ndarray) -> np.ndarray:
    """int64 [H * W]: for every pixel of the boolean [H, W] mask the smallest row-major index of its 4-connected component (a pixel outside
    the mask: itself).  A union-find over the pixel indices in array form: every round hooks the larger of an edge's two roots to the
    smaller (np.minimum.at), then flattens by pointer jumping; an edge whose ends share a root leaves the list.  Each round at least halves
    the number of trees that still have a neighbour, so the number of rounds is logarithmic in the longest component."""
    h, w = mask.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    a = np.concatenate([idx[:, :-1][mask[:, :-1] & mask[:, 1:]], idx[:-1][mask[:-1] & mask[1:]]])
    b = np.concatenate([idx[:, 1:][mask[:, :-1] & mask[:, 1:]], idx[1:][mask[:-1] & mask[1:]]])
    p = idx.reshape(-1).copy()
    while a.size:
        pa, pb = p[a], p[b]
        sel = pa != pb
        a, b, pa, pb = a[sel], b[sel], pa[sel], pb[sel]
        if not a.size:
            break
        np.minimum.at(p, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp
    return p


def _largest_component(mask: np.ndarray) -> np.ndarray:
    """The largest 4-connected component of a boolean [H, W] mask as a boolean array; among components of equal size the one that holds the
    smallest row-major index; an empty mask gives an empty one."""
    if not mask.any():
        return np.zeros_like(mask)
    root = _components_min_index(mask).reshape(mask.shape)
    sizes = np.bincount(root[mask], minlength=mask.size)
    return mask & (root == int(np.argmax(sizes)))  # argmax: the first, so the smallest root, among equal sizes


def conn_levels(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """uint8 [H, W], 0..10: level(x) = (the smallest k in 1..10 with x outside Omega_k) - 1, 10 if x is in all ten; Omega_k the largest
    4-connected component of { min(q, g) >= T_k } (ties: the component with the smallest row-major index)."""
    q, g = _check_q_g(q, g)
    m = np.minimum(q, g)
    level = np.full(q.shape, 10, dtype=np.uint8)
    for k in range(10, 0, -1):
        level[~_largest_component(m >= CONN_T[k - 1])] = k - 1
    return level


def _conn_terms(q: np.ndarray, g: np.ndarray, level: np.ndarray) -> np.ndarray:
    """int64 [H, W]: |dg' - dq'| per pixel, d = 10 v - 255 level kept when >= 383 (the published 0.15 on this scale), else 0."""
    base = 255 * level.astype(np.int64)
    dg, dq = 10 * g.astype(np.int64) - base, 10 * q.astype(np.int64) - base
    return np.abs(np.where(dg >= 383, dg, 0) - np.where(dq >= 383, dq, 0))


def _region_of(region, shape) -> Optional[np.ndarray]:
    if region is None:
        return None
    sel = np.asarray(region) != 0
    if sel.shape != tuple(shape):
        raise ValueError("region does not match the maps")
    return sel


def conn_error(q: np.ndarray, g: np.ndarray, region: Optional[np.ndarray] = None) -> Dict[str, object]:
    """conn = conn_num / 2550000.0 (NaN for an empty region), conn_num = sum over the region of the per-pixel terms (int), n = |region|,
    level_counts int64 [11] over the WHOLE image, counts int64 [13] = n, conn_num, level_counts (gp_eval_matting's counts_out)."""
    q, g = _check_q_g(q, g)
    sel = _region_of(region, q.shape)
    level = conn_levels(q, g)
    term = _conn_terms(q, g, level)
    n = int(q.size if sel is None else sel.sum())
    num = int(term.sum() if sel is None else term[sel].sum())
    lc = np.bincount(level.reshape(-1), minlength=11).astype(np.int64)
    return dict(conn=(num / 2550000.0 if n else float("nan")), conn_num=num, n=n, level_counts=lc,
                counts=np.concatenate([np.array([n, num], dtype=np.int64), lc]))


def _grad_amp(x: np.ndarray) -> np.ndarray:
    """The gradient magnitude of one 8-bit map: mat2gray in integers, the two separable filters (rows first, taps in index order, replicate
    border, plain float64 products and sums starting from 0.0), sqrt(gx * gx + gy * gy)."""
    h, w = x.shape
    lo, hi = int(x.min()), int(x.max())
    xn = (x.astype(np.int64) - lo).astype(np.float64) / float(hi - lo) if hi > lo else np.zeros((h, w), dtype=np.float64)
    px = xn[:, np.clip(np.arange(-4, w + 4), 0, w - 1)]
    row_d, row_g = np.zeros((h, w), dtype=np.float64), np.zeros((h, w), dtype=np.float64)
    for j in range(9):
        row_d = row_d + GRAD_D[j] * px[:, j:j + w]
        row_g = row_g + GRAD_G[j] * px[:, j:j + w]
    rows = np.clip(np.arange(-4, h + 4), 0, h - 1)
    pd, pg = row_d[rows], row_g[rows]
    gx, gy = np.zeros((h, w), dtype=np.float64), np.zeros((h, w), dtype=np.float64)
    for i in range(9):
        gx = gx + GRAD_G[i] * pd[i:i + h]
        gy = gy + GRAD_D[i] * pg[i:i + h]
    return np.sqrt(gx * gx + gy * gy)


def grad_error_map(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """float64 [H, W]: err = (amp_q - amp_g)^2 per pixel (gp_eval_matting's grad_map_out, the same bits)."""
    q, g = _check_q_g(q, g)
    d = _grad_amp(q) - _grad_amp(g)
    return d * d


def grad_error(q: np.ndarray, g: np.ndarray, region: Optional[np.ndarray] = None) -> Dict[str, float]:
    """grad = grad_sum / 1000.0, grad_sum = the sum of the error map over the region (NaN for an empty region), n = |region|."""
    q, g = _check_q_g(q, g)
    sel = _region_of(region, q.shape)
    err = grad_error_map(q, g)
    n = int(q.size if sel is None else sel.sum())
    s = float(err.sum() if sel is None else err[sel].sum()) if n else float("nan")
    return dict(grad=s / 1000.0, grad_sum=s, n=n)


def matting_metrics(pred: np.ndarray, gt: np.ndarray, region: Optional[np.ndarray] = None) -> Dict[str, float]:
    """One image: pred a float map in [0, 1] (quantised by `quantize_mask`) or uint8, gt uint8, both [H, W]; region optional (non-zero =
    scored; the filters and the labelling always see the whole image).  MATTING_METRICS."""
    q = quantize_mask(pred)
    return dict(grad=grad_error(q, gt, region)["grad"], conn=conn_error(q, gt, region)["conn"])


# ---- trimap and boundary bands: the matting transition-region scores, Boundary IoU ----------------------------------------------------------
# "Within reach of a set and within reach of its complement", exactly.  Definitions: include/genpercept_hip.h (gp_mask_band); the functions
# below restate them with numpy alone (capped column distances and one pass per horizontal offset for the disc -- equal to thresholding
# edt_keys' high word --, two 1-D running-window passes for the square) and
# are bit-equal to the device planes.
TRIMAP_METRICS = ["mae_t", "mse_t", "sad_t", "sad_fg", "sad_bg"]
BOUNDARY_METRICS = ["biou"]
BAND_PLANES = ["band", "fg", "bg", "inner", "trimap"]
BAND_METRIC = {"euclidean": 0, "chebyshev": 1, 0: 0, 1: 1}
BAND_MAX_REACH = (1 << 24, 4096)  # per metric: a squared radius, a radius


def band_reach(radius: float, metric) -> int:
    """gp_mask_band's integer `reach` of a real radius: floor(radius^2) for the Euclidean disc, floor(radius) for the Chebyshev square."""
    if metric not in BAND_METRIC:
        raise ValueError(f"metric is 'euclidean' (0) or 'chebyshev' (1), got {metric!r}")
    if not radius >= 0:
        raise ValueError(f"a radius is >= 0, got {radius}")
    return int(math.floor(radius * radius)) if BAND_METRIC[metric] == 0 else int(math.floor(radius))


def boundary_reach(h: int, w: int, ratio: float = 0.02) -> int:
    """Boundary IoU's band width in pixels: `ratio` of the image diagonal, rounded, at least 1."""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def _check_band_args(lo: int, hi: int, reach: int, metric, border) -> Tuple[int, int, int, int, int]:
    if metric not in BAND_METRIC:
        raise ValueError(f"metric is 'euclidean' (0) or 'chebyshev' (1), got {metric!r}")
    m = BAND_METRIC[metric]
    lo, hi, reach = int(lo), int(hi), int(reach)
    if not -1 <= lo < hi <= 256:
        raise ValueError(f"-1 <= lo < hi <= 256, got lo = {lo}, hi = {hi}")
    if not 0 <= reach <= BAND_MAX_REACH[m]:
        raise ValueError(f"0 <= reach <= {BAND_MAX_REACH[m]} for metric {m}, got {reach}")
    return lo, hi, reach, m, int(bool(border))


def _window_any(s: np.ndarray, d: int, axis: int) -> np.ndarray:
    """Whether any element of the boolean array within d positions along `axis` is set (a running window over a cumulative sum)."""
    n = s.shape[axis]
    c = np.concatenate([np.zeros_like(s.take([0], axis=axis), dtype=np.int64), np.cumsum(s, axis=axis, dtype=np.int64)], axis=axis)
    i = np.arange(n)
    return c.take(np.minimum(i + d, n - 1) + 1, axis=axis) - c.take(np.maximum(i - d, 0), axis=axis) > 0


def _within_reach(s: np.ndarray, reach: int, metric: int) -> np.ndarray:
    """Pixels whose distance to the nearest set pixel of the boolean [H, W] array is <= reach (none when the array is empty).  Chebyshev: two
    1-D running windows.  Euclidean: what `(edt_keys(s) >> 32) <= reach` gives, without the full transform (whose row search runs until the
    FARTHEST pixel is settled, a minute on a 2048 x 2048 alpha): the vertical distance to the column's nearest set pixel, capped just above
    the radius, then one pass per horizontal offset up to the radius."""
    if metric == 1:
        return _window_any(_window_any(s, reach, 0), reach, 1)
    h, w = s.shape
    rv = math.isqrt(reach)
    ys = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(s, ys, -(h + rv + 1)), axis=0)             # the nearest set row at or above (far away: none)
    dn = np.minimum.accumulate(np.where(s, ys, 2 * h + rv + 1)[::-1], axis=0)[::-1]  # ... at or below
    dv = np.minimum(np.minimum(ys - up, dn - ys), rv + 1)
    d2 = dv * dv
    hit = d2 <= reach
    for dx in range(1, min(rv, w - 1) + 1):
        c = d2 <= reach - dx * dx
        hit[:, dx:] |= c[:, :-dx]
        hit[:, :-dx] |= c[:, dx:]
    return hit


def mask_band(a: np.ndarray, lo: int, hi: int, reach: int, metric="euclidean", border=False) -> Dict[str, np.ndarray]:
    """gp_mask_band on the host for one map: a float [H, W] in [0, 1] (quantised by `quantize_mask`) or uint8.  A = {a > lo}, Bc = {a < hi};
    returns the uint8 planes BAND_PLANES: band (within reach of both), fg (out of Bc's reach), bg (out of A's reach), inner (in A and within
    Bc's reach), each 0 / 255, and trimap (0 / 128 / 255 for bg / band / fg).  metric "euclidean" (0): reach is a squared radius; "chebyshev"
    (1): a radius.  border: the outside of the image counts as Bc."""
    lo, hi, reach, m, border = _check_band_args(lo, hi, reach, metric, border)
    q = quantize_mask(a)
    if q.ndim != 2 or q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"one [H, W] map, got {q.shape}")
    h, w = q.shape
    in_a = q.astype(np.int64) > lo
    near_a = _within_reach(in_a, reach, m)
    near_b = _within_reach(q.astype(np.int64) < hi, reach, m)
    if border:
        ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
        e = np.minimum(np.minimum(ys + 1, h - ys), np.minimum(xs + 1, w - xs))
        near_b = near_b | ((e * e if m == 0 else e) <= reach)
    u8 = lambda sel: np.where(sel, 255, 0).astype(np.uint8)
    band = near_a & near_b
    return dict(band=u8(band), fg=u8(~near_b), bg=u8(~near_a), inner=u8(in_a & near_b),
                trimap=np.where(band, 128, np.where(near_a, 255, 0)).astype(np.uint8))


def trimap_from_counts(c_t, c_fg, c_bg) -> Dict[str, float]:
    """TRIMAP_METRICS and the three region sizes from gp_eval_mask's counts over the transition region, the foreground side and the background
    side: mae_t = sad / (255.0 n_t), mse_t = sse / (65025.0 n_t) (NaN for an empty transition region), sad_* = sad / 255000.0 (0.0 for an
    empty region)."""
    (n_t, _, sad_t, sse_t), (n_f, _, sad_f, _), (n_b, _, sad_b, _) = ([int(v) for v in np.asarray(c).reshape(-1)[:4]] for c in (c_t, c_fg, c_bg))
    nan = float("nan")
    return dict(mae_t=sad_t / (255.0 * n_t) if n_t else nan, mse_t=sse_t / (65025.0 * n_t) if n_t else nan, sad_t=sad_t / 255000.0,
                sad_fg=sad_f / 255000.0, sad_bg=sad_b / 255000.0, n_t=n_t, n_fg_side=n_f, n_bg_side=n_b)


def trimap_metrics(pred: np.ndarray, gt: np.ndarray, radius: float, metric="euclidean") -> Dict[str, float]:
    """The trimap-free matting protocol for one image: the trimap comes from the ground-truth alpha (dilate(gt != 0) - erode(gt == 255) with a
    disc or square of `radius`, nothing outside the image), SAD / MSE / MAD over the transition region and SAD over the two sides.  pred a
    float map in [0, 1] or uint8, gt uint8.  Raises ValueError when the transition region is empty."""
    planes = mask_band(gt, 0, 255, band_reach(radius, metric), metric, False)
    q = quantize_mask(pred)
    m = trimap_from_counts(*(mask_counts(q, gt, planes[k]) for k in ("band", "fg", "bg")))
    if m["n_t"] == 0:
        raise ValueError("no pixel in the transition region (n = 0)")
    return m


def boundary_iou(pred: np.ndarray, gt: np.ndarray, ratio: float = 0.02) -> Dict[str, float]:
    """Boundary IoU (Cheng et al. 2021) of one image: d = boundary_reach(H, W, ratio); G_d, P_d the pixels of G = gt > 128 and of
    P = q >= 128 within Chebyshev distance d of the other side, the outside of the image included; biou = |G_d & P_d| / |G_d | P_d|, 0.0 when
    both are empty.  Also d and the two band sizes."""
    q = quantize_mask(pred)
    h, w = q.shape
    d = boundary_reach(h, w, ratio)
    g_d = mask_band(gt, 128, 129, d, 1, True)["inner"]
    p_d = mask_band(q, 127, 128, d, 1, True)["inner"]
    c = mask_counts(p_d, g_d)
    return dict(biou=mask_metrics_from_counts(c)["iou"], d=d, n_gt_band=int(c[260:516].sum()), n_pred_band=int(c[1]) // 255)


# ---- seg: palette decode and confusion-matrix scores -----------------------------------------------------------------------------------------
# Mode seg is colour regression against an RGB label image (src/dataset/base_dataset.py:333-346,366); the reference has neither a palette nor a
# decode nor a metric for it.  The definitions below are this project's, stated once in include/genpercept_hip.h (gp_seg_decode, gp_eval_seg):
# the user supplies the palette, everything is computed on the 8-BIT prediction (run.py:449-455, per channel), the decode and the counts are
# integers, and each value is one fixed sequence of float64 operations on the counts.  The device entry runs the same sequence and is bit-equal.
SEG_METRICS = ["pixel_acc", "mean_acc", "miou", "fwiou", "colour_rmse"]
SEG_MAX_K = 192
SEG_VOID = 255  # seg_gt_labels' label of a void pixel (any value >= K is void)


def _check_palette(palette) -> np.ndarray:
    pal = np.asarray(palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= SEG_MAX_K:
        raise ValueError(f"palette: uint8 [K, 3] with 1 <= K <= {SEG_MAX_K}, got {pal.dtype} {pal.shape}")
    return pal


def quantize_seg(pred: np.ndarray) -> np.ndarray:
    """The 8-bit colour image uint8 [H, W, 3] of a seg prediction: `quantize_mask` per channel of a float map stored [H, W, 3] (what
    `run_inference(mode="seg")` writes) or [3, H, W] (a slice of `predict_batch_device`); uint8 input is only brought to [H, W, 3].  An
    [3, H, 3] array is read as [H, W, 3] with H = 3: the file's own layout wins."""
    pred = np.asarray(pred)
    if pred.ndim != 3 or 3 not in (pred.shape[0], pred.shape[-1]):
        raise ValueError(f"expected [H, W, 3] or [3, H, W], got {pred.shape}")
    if pred.shape[-1] != 3:
        pred = np.moveaxis(pred, 0, -1)
    return np.ascontiguousarray(quantize_mask(pred))


def palette_labels(rgb_u8: np.ndarray, palette) -> Tuple[np.ndarray, np.ndarray]:
    """(labels uint8 [...], d int32 [...]) of a uint8 colour array [..., 3]: d_k = (r - pr_k)^2 + (g - pg_k)^2 + (b - pb_k)^2 in integers, the
    label is the smallest k attaining the minimum, d that minimum.  Pixels go in chunks of 65536, so that K = 192 on a megapixel stays in memory."""
    pal = _check_palette(palette).astype(np.int32)
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError(f"expected a uint8 colour array [..., 3], got {rgb.dtype} {rgb.shape}")
    flat = rgb.reshape(-1, 3)
    labels, dist = np.empty(flat.shape[0], dtype=np.uint8), np.empty(flat.shape[0], dtype=np.int32)
    for lo in range(0, flat.shape[0], 65536):
        px = flat[lo:lo + 65536].astype(np.int32)
        d = np.zeros((px.shape[0], pal.shape[0]), dtype=np.int32)
        for c in range(3):
            diff = px[:, c:c + 1] - pal[None, :, c]
            d += diff * diff
        k = d.argmin(axis=1)  # the first index of the minimum
        labels[lo:lo + 65536] = k
        dist[lo:lo + 65536] = d[np.arange(px.shape[0]), k]
    return labels.reshape(rgb.shape[:-1]), dist.reshape(rgb.shape[:-1])


def seg_gt_labels(gt: np.ndarray, palette, gt_tol: int = 0) -> np.ndarray:
    """The ground-truth label map uint8 [H, W], void = 255.  gt: a uint8 colour image [H, W, 3] (decoded by `palette_labels`; a pixel whose
    minimum squared distance exceeds gt_tol is void) or a uint8 label map [H, W] (values >= K are void; gt_tol is ignored)."""
    pal = _check_palette(palette)
    gt = np.asarray(gt)
    if int(gt_tol) < 0:
        raise ValueError(f"gt_tol: a squared distance >= 0, got {gt_tol}")
    if gt.dtype != np.uint8 or gt.ndim not in (2, 3) or (gt.ndim == 3 and gt.shape[-1] != 3):
        raise ValueError(f"gt: a uint8 colour image [H, W, 3] or label map [H, W], got {gt.dtype} {gt.shape}")
    if gt.ndim == 2:
        return np.where(gt >= pal.shape[0], np.uint8(SEG_VOID), gt).astype(np.uint8)
    labels, d = palette_labels(gt, pal)
    return np.where(d > int(gt_tol), np.uint8(SEG_VOID), labels).astype(np.uint8)


def seg_counts(q: np.ndarray, gt_labels: np.ndarray, palette, region: Optional[np.ndarray] = None) -> np.ndarray:
    """The integer counts of one image, int64 [3 + K * K] = n (scored: in the region and not void), n_void (in the region but void), sum_d (the
    prediction's minimum distances summed over the scored pixels), conf[g][c] row-major (row = ground-truth class, column = predicted class).
    q: the uint8 colour image [H, W, 3] of the prediction (`quantize_seg`); gt_labels: uint8 [H, W], values >= K void (`seg_gt_labels`)."""
    pal = _check_palette(palette)
    K = pal.shape[0]
    q, g = np.asarray(q), np.asarray(gt_labels)
    if q.dtype != np.uint8 or g.dtype != np.uint8 or q.ndim != 3 or q.shape[-1] != 3 or q.shape[:2] != g.shape:
        raise ValueError(f"q must be uint8 [H, W, 3] and gt_labels uint8 [H, W], got {q.dtype} {q.shape} and {g.dtype} {g.shape}")
    c, d = palette_labels(q, pal)
    sel = np.ones(g.shape, dtype=bool) if region is None else np.asarray(region) != 0
    if sel.shape != g.shape:
        raise ValueError("region does not match the maps")
    void = g >= K
    scored = sel & ~void
    out = np.empty(3 + K * K, dtype=np.int64)
    out[0], out[1], out[2] = scored.sum(), (sel & void).sum(), d[scored].astype(np.int64).sum()
    out[3:] = np.bincount(g[scored].astype(np.int64) * K + c[scored].astype(np.int64), minlength=K * K)
    return out


def seg_metrics_from_counts(counts, K: int) -> dict:
    """The values of gp_eval_seg's `out` from the counts: n, n_void (ints), SEG_METRICS, n_classes, iou (a list of K floats, NaN where the
    class is in neither map).  Plain float64 + * / sqrt in the order the header prescribes, classes in increasing index; n = 0: NaN for
    everything but the two counts."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != 3 + K * K:
        raise ValueError(f"expected {3 + K * K} counts for K = {K}, got {len(c)}")
    n, n_void, sum_d = c[:3]
    nan = float("nan")
    if n == 0:
        return dict(n=0, n_void=n_void, pixel_acc=nan, mean_acc=nan, miou=nan, fwiou=nan, colour_rmse=nan, n_classes=nan, iou=[nan] * K)
    conf = c[3:]
    sum_tp = n_rows = n_classes = 0
    acc = iou_sum = fw = 0.0
    iou = [nan] * K
    for i in range(K):
        row, col, tp = sum(conf[i * K:(i + 1) * K]), sum(conf[i::K]), conf[i * K + i]
        union = row + col - tp
        sum_tp += tp
        if union > 0:
            iou[i] = float(tp) / float(union)
        if row > 0:
            acc = acc + float(tp) / float(row)
            fw = fw + float(row) * iou[i]
            n_rows += 1
        if union > 0:
            iou_sum = iou_sum + iou[i]
            n_classes += 1
    return dict(n=n, n_void=n_void, pixel_acc=float(sum_tp) / float(n), mean_acc=acc / float(n_rows), miou=iou_sum / float(n_classes),
                fwiou=fw / float(n), colour_rmse=math.sqrt(float(sum_d) / (3.0 * float(n))) / 255.0, n_classes=n_classes, iou=iou)


def seg_metrics(pred: np.ndarray, gt: np.ndarray, palette, region: Optional[np.ndarray] = None, gt_tol: int = 0) -> dict:
    """One image: pred a float colour map in [0, 1], [H, W, 3] or [3, H, W] (quantised by `quantize_seg`), or uint8; gt a uint8 colour image
    [H, W, 3] or label map [H, W]; palette uint8 [K, 3]; region optional (non-zero = scored).  `seg_metrics_from_counts` plus "conf" (int64
    [K, K])."""
    pal = _check_palette(palette)
    K = pal.shape[0]
    c = seg_counts(quantize_seg(pred), seg_gt_labels(gt, pal, gt_tol), pal, region)
    return dict(seg_metrics_from_counts(c, K), conf=c[3:].reshape(K, K).copy())
