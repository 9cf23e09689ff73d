"""Depth evaluation protocol next to the hot path: least-squares alignment and the ten metrics
`eval.py` reports, restated in numpy (float64) so "AbsRel unchanged" can be stated for predictions of this engine.

Semantics follow /root/reference/src/util/alignment.py:29-94 (align_depth_least_square, depth2disparity) and
/root/reference/src/util/metric.py:34-158; pinned by tests/golden/metrics_ref.npz (outputs of those reference functions).
Per-image masked means, then a mean over images — exactly the reference's reduction order.
"""
from __future__ import annotations

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
