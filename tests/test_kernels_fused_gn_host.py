"""CPU side of tests/test_kernels_fused_gn_gpu.py: the gates of the GroupNorm-fused conv and of the decoder tail are proven before a GPU sees
them.  On the SAME inputs (the generators are imported; the eight-image case runs one image, cin2560 three of its twenty weight masks):

  * Model inside the gate.  A plain float32 evaluation of what the kernels do -- fp32 scale = rstd gamma and shift = beta - mean scale from
    two-pass statistics, one fma, SiLU as v / (1 + exp(-v)), ONE rounding to 16 bits, an fp32 convolution, bias, residual, ReLU, one output
    rounding (the tail: fp32 mean of three, clip, shift, no rounding) -- lies inside every gate.  e_used is logged, not gated.
  * Mutants rejected.  One 8-channel slot taking the next slot's scale / shift; the padding holding act(shift) (the transform run over the
    zeros); one slot of ONE pixel left un-normalised; SiLU of the 16-bit-rounded pre-activation (asserted in bf16; fp16 rejects it only marginally:
    logged); for the tail the channel mean taken after the clip.  Each puts elements outside the gate.  In cin2560 the mutated slot is one that the
    run's mask weights.
"""
import pytest
import torch
import torch.nn.functional as F

from test_kernels_fused_gn_gpu import (FGN_CASES, TAIL_CASES, TAIL_KNZ, border_share, e_used, fgn_inputs, operand_interval, output_bound, padding_not_zero,
                                       slot_mask, tail_f, tail_inputs, tail_interval, tail_outside)
from test_kernels_interval_gpu import GROUPS
from test_kernels_interval_host import DTYPES, interval, outside

CIN2560_HOST_RUNS = (0, 7, 19)


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


# ---- the float32 model ---------------------------------------------------------------------------------------------------------------------------
def scale_shift_f32(x16, gamma, beta, eps):
    """fp32 scale, shift [B,1,C] from two-pass statistics"""
    x = x16.float()
    b, hw, c = x.shape
    flat = x.view(b, hw, GROUPS, c // GROUPS).permute(0, 2, 1, 3).reshape(b, GROUPS, -1)   # (a contiguous reduction: summed in blocks)
    mean = flat.mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(((flat - mean) ** 2).mean(dim=2, keepdim=True) + eps)
    ex = lambda t: t.expand(b, GROUPS, c // GROUPS).reshape(b, 1, c)
    scale = ex(rstd) * gamma
    return scale, beta - ex(mean) * scale


def act_f32(v, silu):
    return v * (1.0 / (1.0 + torch.exp(-v))) if silu else v


def transform_f32(x16, scale, shift, silu, dt, rounded_pre=False):
    """the staged operand: 16 bit(act(fma(x, scale, shift))) as float32 [B,HW,C].  The product of two fp32 numbers is exact in float64: the
    float64 sum rounded to fp32 is the fma.  rounded_pre (mutant): the pre-activation is rounded to 16 bits before the SiLU"""
    v = (x16 * scale.double() + shift.double()).float()
    if rounded_pre:
        v = v.to(dt).float()
    return act_f32(v, silu).to(dt).float()


def conv_f32(n, wt, bias, hw, ups, res, relu, pad=None):
    """fp32 conv3x3 of the staged operand n [B,HW,C] (+ bias, residual, ReLU) -> [B,Ho,Wo,O] float32 before the output rounding; pad [B,1,C]: the
    padding ring holds this value (mutant), else zeros"""
    b, _, c = n.shape
    t = n.view(b, hw[0], hw[1], c).permute(0, 3, 1, 2)
    if ups:
        t = F.interpolate(t, scale_factor=2, mode="nearest")
    tp = F.pad(t, (1, 1, 1, 1))
    if pad is not None:
        ring = torch.ones_like(tp)
        ring[:, :, 1:-1, 1:-1] = 0
        tp = tp + ring * pad.view(b, c, 1, 1)
    y = F.conv2d(tp, wt.float(), bias.float()).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.float()
    return y.clamp_min(0) if relu else y


def slot_takes_next(t, s):
    """[B,1,C] table with the entries of slot s replaced by those of slot s + 1"""
    t = t.clone()
    t[..., 8 * s:8 * s + 8] = t[..., 8 * s + 8:8 * s + 16]
    return t


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", FGN_CASES, ids=[c[0] for c in FGN_CASES])
def test_conv_gn_model_inside_gate_and_mutants_outside(case, dt, metric_log):
    name, b, h, w, cin, cout, ups, silu, res_relu, env, path, ratio, epss = case
    b = 1 if name == "several_tiles_per_wg" else b
    x, gamma, beta, wt_all, bias, res = fgn_inputs(case, dt, batch=b)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    runs = [(f" m{m}", m) for m in CIN2560_HOST_RUNS] if name == "cin2560" else [("", None)]
    for eps in epss:
        c, dd, pad64 = operand_interval(x, gamma, beta, eps, silu, dt)
        scale, shift = scale_shift_f32(x, gamma, beta, eps)
        n = transform_f32(x, scale, shift, silu, dt)
        for sfx, m in runs:
            tag = f"{name}{sfx} eps{eps} {_name(dt)}"
            wt = wt_all if m is None else wt_all * slot_mask(cin, m)
            y, err, _ = output_bound(c, dd, wt, bias.double(), (h, w), ups, res, res_relu)
            conv = lambda t, pad=None: conv_f32(t, wt, bias, (h, w), ups, res, res_relu, pad).to(dt)
            model = conv(n)
            bad, gr = interval(model, y, err)
            used = e_used(model, y, err)
            metric_log(f"host_model[conv_gn {tag}]", gate_ratio=gr, e_used=used, flip_share=float((dd > 0).double().mean()))
            assert bad == 0, f"{tag}: the float32 model leaves the gate at {bad} elements (gate ratio {gr:.3g}, e_used {used:.3g})"
            # the variant the GPU file passes as wrong=, where it passes it
            if border_share(ho, wo) >= 0.02:
                f = outside(padding_not_zero(c, pad64, wt, bias.double(), (h, w), ups, res, res_relu), y, err, dt)
                assert f >= 0.02, f"{tag}: padding with act(shift) (float64): only {f:.3g} outside"
            s = 5 if m is None else m                       # a slot the run's mask weights
            mutants = {"slot takes the next slot's scale / shift": conv(transform_f32(x, slot_takes_next(scale, s), slot_takes_next(shift, s), silu, dt)),
                       "padding holds act(shift)": conv(n, act_f32(shift, silu).to(dt).float())}
            raw = n.clone()
            p0 = (h // 2) * w + w // 2                      # an interior pixel of image 0
            raw[0, p0, 8 * s:8 * s + 8] = x[0, p0, 8 * s:8 * s + 8].float()
            mutants["one slot of one pixel un-normalised"] = conv(raw)
            for mname, v in mutants.items():
                nb, _ = interval(v, y, err)
                metric_log(f"host_mutant[conv_gn {tag} {mname}]", outside=nb)
                assert nb > 0, f"{tag}: mutant '{mname}' is not rejected"
            if silu:
                nb, _ = interval(conv(transform_f32(x, scale, shift, silu, dt, rounded_pre=True)), y, err)
                metric_log(f"host_mutant[conv_gn {tag} SiLU of the rounded pre-activation]", outside=nb)
                assert nb > 0 or dt == torch.float16, f"{tag}: SiLU of the rounded pre-activation is not rejected"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", TAIL_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in TAIL_CASES])
def test_decoder_tail_model_inside_gate_and_mutants_outside(case, dt, metric_log):
    b, h, w = case
    x, gamma, beta, wt, bias = tail_inputs(case, dt)
    c, dd, pad64 = operand_interval(x, gamma, beta, 1e-6, True, dt)
    y, err, s = output_bound(c, dd, wt, bias.double(), (h, w), knz=TAIL_KNZ)
    yw = padding_not_zero(c, pad64, wt, bias.double(), (h, w))
    scale, shift = scale_shift_f32(x, gamma, beta, 1e-6)
    n = transform_f32(x, scale, shift, True, dt)
    conv = lambda t, pad=None: conv_f32(t, wt, bias, (h, w), False, None, False, pad)
    raw_n = n.clone()
    p0 = (h // 2) * w + w // 2
    raw_n[0, p0, 40:48] = x[0, p0, 40:48].float()
    three = {"model": conv(n),
             "slot takes the next slot's scale / shift": conv(transform_f32(x, slot_takes_next(scale, 5), slot_takes_next(shift, 5), True, dt)),
             "padding holds act(shift)": conv(n, act_f32(shift, True).to(dt).float()),
             "one slot of one pixel un-normalised": conv(raw_n),
             "SiLU of the rounded pre-activation": conv(transform_f32(x, scale, shift, True, dt, rounded_pre=True))}

    def finish(c3, mean3, raw, mean_after_clip=False):
        """the kernel's epilogue in float32"""
        if mean3 and mean_after_clip:
            c3 = (c3.clamp(-1, 1) + 1) * 0.5
            return (c3[..., 0:1] + c3[..., 1:2] + c3[..., 2:3]) / 3.0
        v = (c3[..., 0:1] + c3[..., 1:2] + c3[..., 2:3]) / 3.0 if mean3 else c3
        return v if raw else (v.clamp(-1, 1) + 1) * 0.5

    for mean3 in (False, True):
        for raw in (False, True):
            tag = f"decoder_tail{case}[mean3={int(mean3)} raw={int(raw)}] {_name(dt)}"
            lo, hi, yv = tail_interval(y, err, s, mean3, raw)
            if not raw:
                clipped = float((yv.abs() > 1).double().mean())
                metric_log(f"host_clipped[{tag}]", clipped=clipped)
                assert 0.02 <= clipped <= 0.35, f"{tag}: {clipped:.3g} of the reference is clipped"
            wv = yw.mean(-1, keepdim=True) if mean3 else yw
            f = float(tail_outside(wv if raw else tail_f(wv), lo, hi).double().mean())
            assert (f >= 0.02) if raw else (f > 0), f"{tag}: padding with act(shift) (float64): only {f:.3g} outside"   # (the GPU file passes it on the raw forms)
            for mname, c3 in three.items():
                out = finish(c3, mean3, raw).double()
                nb = int(tail_outside(out, lo, hi).sum())
                if mname == "model":
                    gr = float(((out - (lo + hi) / 2).abs() / ((hi - lo) / 2)).max())
                    metric_log(f"host_model[{tag}]", gate_ratio=gr)
                    assert nb == 0, f"{tag}: the float32 model leaves the gate at {nb} elements (gate ratio {gr:.3g})"
                else:
                    metric_log(f"host_mutant[{tag} {mname}]", outside=nb)
                    assert nb > 0 or (mname.startswith("SiLU") and dt == torch.float16), f"{tag}: mutant '{mname}' is not rejected"
            if mean3 and not raw:
                nb = int(tail_outside(finish(three["model"], True, False, mean_after_clip=True).double(), lo, hi).sum())
                metric_log(f"host_mutant[{tag} mean after the clip]", outside=nb)
                assert nb > 0, f"{tag}: the mean taken after the clip is not rejected"
