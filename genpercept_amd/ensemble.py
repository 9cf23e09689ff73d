"""Test-time ensembling of the multi-step archs (reference: genpercept/util/ensemble.py:43-205, called from
genpercept_pipeline.py:290-297 with scale_invariant=True, shift_invariant=True, max_res=50).

Each of the E predictions of one image is affine-invariant, so they are first aligned (per-member scale s and shift t minimising the
summed pairwise RMS distance plus a regulariser pulling the ensembled map to [0,1]; BFGS from the min/max initialisation, at most
`max_iter` steps on maps reduced to `max_res` pixels), then reduced per pixel (median = torch.median, i.e. the LOWER middle value
for even E) and rescaled to [0,1].  The optimiser works on E x (<= 50 x 50) numbers on the host.

fp32 members on a GPU take the device route: gp_ensemble_gather (the reduced maps and their min / max, one launch for all images), one
copy to the host, the optimiser per image, gp_ensemble_reduce (align, median / mean, rescale: one streaming pass over the members of all
images).  CPU tensors, other dtypes and GENPERCEPT_HOST_ENSEMBLE=1 run the same steps as tensor ops wherever `depth` lives.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from .image_util import resize_max_res, resize_max_res_size


def _lower_median(a: np.ndarray) -> np.ndarray:
    """torch.median(dim=0) semantics on [E, ...]: element (E-1)//2 of the sorted values (no averaging)."""
    return np.sort(a, axis=0)[(a.shape[0] - 1) // 2]


def _reduce(aligned: torch.Tensor, reduction: str, want_uncertainty: bool):
    if reduction == "mean":
        pred = aligned.mean(dim=0, keepdim=True)
        unc = aligned.std(dim=0, keepdim=True) if want_uncertainty else None
    else:
        pred = aligned.median(dim=0, keepdim=True).values
        unc = (aligned - pred).abs().median(dim=0, keepdim=True).values if want_uncertainty else None
    return pred, unc


def _apply(maps, param, n: int, affine: bool):
    """maps * s + t (affine) or maps * s for the optimiser's vector [s_0 .. s_{n-1}, t_0 .. t_{n-1}]: [n,1,H,W] tensors or [n, pixels] arrays."""
    p = np.asarray(param, dtype=np.float64)
    s = p[:n]
    if torch.is_tensor(maps):
        st = torch.from_numpy(s).to(maps).view(n, 1, 1, 1)
        return maps * st + torch.from_numpy(p[n:]).to(maps).view(n, 1, 1, 1) if affine else maps * st
    s32 = s.astype(np.float32).reshape(n, 1)  # the reference casts the optimiser's float64 vector to the maps' fp32
    return maps * s32 + p[n:].astype(np.float32).reshape(n, 1) if affine else maps * s32


def _fit(flat: np.ndarray, lo: np.ndarray, hi: np.ndarray, affine: bool, reduction: str, regularizer_strength: float, max_iter: int,
         tol: float) -> np.ndarray:
    """The host optimiser on the reduced members flat fp32 [n, pixels] with their min `lo` / max `hi` [n]: the float64 vector [s, t] (or [s])."""
    n = flat.shape[0]
    if affine:
        s0 = 1.0 / np.maximum(hi - lo, np.float32(1e-6))
        x0 = np.concatenate([s0, -s0 * lo])
    else:
        x0 = 1.0 / np.maximum(hi, np.float32(1e-6))
    iu, ju = np.triu_indices(n, k=1)

    def cost(param) -> float:
        al = _apply(flat, param, n, affine)
        c = float(np.sqrt(np.mean((al[iu] - al[ju]) ** 2, axis=1, dtype=np.float32)).astype(np.float64).sum()) if len(iu) else 0.0
        if regularizer_strength > 0:
            pred = al.mean(axis=0, dtype=np.float32) if reduction == "mean" else _lower_median(al)
            c += (abs(0.0 - float(pred.min())) + abs(1.0 - float(pred.max()))) * regularizer_strength
        return c

    import scipy.optimize
    res = scipy.optimize.minimize(cost, x0.astype(np.float32), method="BFGS", tol=tol, options={"maxiter": max_iter, "disp": False})
    return res.x


def _device_route(depth: torch.Tensor) -> bool:
    return depth.is_cuda and depth.dtype == torch.float32 and not os.environ.get("GENPERCEPT_HOST_ENSEMBLE")


def _ensemble_device(depth: torch.Tensor, affine: bool, output_uncertainty: bool, reduction: str, regularizer_strength: float, max_iter: int,
                     tol: float, max_res: Optional[int]):
    """Scale(-and-shift)-invariant ensembling of depth fp32 [B,E,H,W] on the device: one gather launch, one device -> host copy, B host
    optimisations, one reduce call.  Returns ([B,1,H,W], uncertainty [B,1,H,W] or None) on the device."""
    from . import engine as ge
    b, n, h0, w0 = (int(v) for v in depth.shape)
    h, w = h0, w0
    if max_res is not None and max(h0, w0) > max_res:
        h, w = resize_max_res_size(h0, w0, max_res)
    buf = torch.empty((b * n * (h * w + 2),), dtype=torch.float32, device=depth.device)
    ge.ensemble_gather(depth, h, w, out=buf)
    host = buf.cpu().numpy()
    flat, mm = host[:b * n * h * w].reshape(b, n, h * w), host[b * n * h * w:].reshape(b, n, 2)
    param = np.stack([_fit(flat[i], mm[i, :, 0], mm[i, :, 1], affine, reduction, regularizer_strength, max_iter, tol) for i in range(b)])
    scale = param[:, :n].astype(np.float32)
    shift = param[:, n:].astype(np.float32) if affine else None
    pred, unc = ge.ensemble_reduce(depth, scale, shift, reduction, output_uncertainty)
    return pred[:, None], (unc[:, None] if unc is not None else None)


def ensemble_depth(depth: torch.Tensor, scale_invariant: bool = True, shift_invariant: bool = True, output_uncertainty: bool = False,
                   reduction: str = "median", regularizer_strength: float = 0.02, max_iter: int = 2, tol: float = 1e-3,
                   max_res: Optional[int] = 1024) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """depth [E,1,H,W] -> ([1,1,H,W] in [0,1], uncertainty [1,1,H,W] or None)."""
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"Expecting 4D tensor of shape [B,1,H,W]; got {depth.shape}.")
    if reduction not in ("mean", "median"):
        raise ValueError(f"Unrecognized reduction method: {reduction}.")
    if not scale_invariant and shift_invariant:
        raise ValueError("Pure shift-invariant ensembling is not supported.")
    n = depth.shape[0]
    affine = scale_invariant and shift_invariant
    if _device_route(depth):
        if not scale_invariant:
            raise ValueError("Unrecognized alignment.")
        return _ensemble_device(depth[:, 0][None], affine, output_uncertainty, reduction, regularizer_strength, max_iter, tol, max_res)

    if scale_invariant:
        small = depth.to(torch.float32)
        if max_res is not None and max(small.shape[2:]) > max_res:
            small = resize_max_res(small, max_res, "nearest-exact")
        flat = small.reshape(n, -1).cpu().numpy()
        param = _fit(flat, flat.min(axis=1), flat.max(axis=1), affine, reduction, regularizer_strength, max_iter, tol)
        depth = _apply(depth, param, n, affine)

    pred, unc = _reduce(depth, reduction, output_uncertainty)
    d_max = pred.max()
    if affine:
        d_min = pred.min()
    elif scale_invariant:
        d_min = 0
    else:
        raise ValueError("Unrecognized alignment.")
    rng = (d_max - d_min).clamp(min=1e-6)
    pred = (pred - d_min) / rng
    if output_uncertainty:
        unc = unc / rng
    return pred, unc


def ensemble_depth_batch(depth: torch.Tensor, scale_invariant: bool = True, shift_invariant: bool = True, output_uncertainty: bool = False,
                         reduction: str = "median", regularizer_strength: float = 0.02, max_iter: int = 2, tol: float = 1e-3,
                         max_res: Optional[int] = 1024) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """`ensemble_depth` for the members of B images at once: depth [B,E,1,H,W] or [B,E,H,W] -> ([B,1,H,W], uncertainty [B,1,H,W] or None),
    image i being what `ensemble_depth(depth[i])` returns.  On the device route the whole batch costs one gather launch, one copy to the
    host, B host optimisations and one reduce call."""
    if depth.dim() == 4:
        depth = depth[:, :, None]
    if depth.dim() != 5 or depth.shape[2] != 1:
        raise ValueError(f"Expecting a tensor of shape [B,E,1,H,W] or [B,E,H,W]; got {depth.shape}.")
    if reduction not in ("mean", "median"):
        raise ValueError(f"Unrecognized reduction method: {reduction}.")
    if not scale_invariant and shift_invariant:
        raise ValueError("Pure shift-invariant ensembling is not supported.")
    if _device_route(depth):
        if not scale_invariant:
            raise ValueError("Unrecognized alignment.")
        return _ensemble_device(depth[:, :, 0], scale_invariant and shift_invariant, output_uncertainty, reduction, regularizer_strength,
                                max_iter, tol, max_res)
    outs = [ensemble_depth(depth[i], scale_invariant, shift_invariant, output_uncertainty, reduction, regularizer_strength, max_iter, tol, max_res)
            for i in range(depth.shape[0])]
    return torch.cat([p for p, _ in outs], dim=0), (torch.cat([u for _, u in outs], dim=0) if output_uncertainty else None)
