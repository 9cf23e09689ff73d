"""CPU side of tests/test_kernels_interval_gpu.py: the interval gates are proven before a GPU sees them.  For every case list of the GPU file,
on the SAME inputs (the generators are imported):

  * a plain float32 evaluation of the operation in its well-conditioned order (two-pass statistics, fp32 softmax with the maximum subtracted,
    attention with P rounded to 16 bits and an fp32 row sum) uses at most HALF of E before its own rounding to 16 bits, and rounds into the
    interval: correct arithmetic leaves half of E to the GPU's different summation order.  (The half applies to E, not to the logged gate ratio
    |out - y64| / (ulp16 / 2 + E): any correctly rounded 16-bit output reaches ~1 there wherever E is small against the output rounding.  In the
    attention bound it applies to E beyond the 16-bit rounding of P, which every evaluation of the algorithm shares);
  * the nearest wrong variants fall outside: at least 2 % of their elements outside the interval (the wrong= mechanism of _check_interval), or,
    for statistics, a gate ratio >= 8 against the scale / shift bounds.

One near variant cannot be rejected by ANY worst-case bound of this form and is evaluated, not asserted: an attention row
sum taken from the ROUNDED probabilities.  With e_j the rounding error of p_j (|e_j| <= u16 p_j) that variant's error is sum_j e_j (v_j - o) to
first order, at most u16 sum_j p_j |v_j - o| <= u16 (sum_j p_j |v_j| + |o|) = E + one half-ulp of the output: inside the interval by construction.

Very large cases run a reduced batch / head count here (the kinds of case all appear).
"""
import math

import numpy as np
import pytest
import torch

from test_contract_kernels_gpu import _gn_scale_shift_bounds, _gn_single_pass_f32
from test_kernels_interval_gpu import (CONV_STATS_CASES, FLASH512_CASES, FLASH512_SCALE, FLASH64_CASES, FOLD_CASES, GN_CASES, GROUPS, LN_CASES, LOG2E, NEG512_CASES, NEG64_CASES,
                                       SOFTMAX_CASES, SOFTMAX_SCALE, attn_ref_bound, conv_stats_inputs, cross_inputs, cross_ref_bound, flash512_inputs,
                                       flash64_inputs, fold_inputs, fold_ref_bound, gn_inputs, gn_ratios, gn_ref_bound, group_stats, heads_merge, heads_split,
                                       ln_inputs, ln_ref_bound, negative_logit_inputs, norm_ref_bound, outlier_inputs, padded_keys_counted, r16, softmax_inputs, softmax_ref_bound, spiky_inputs,
                                       stats_ref_bounds, ulp16)

DTYPES = [torch.bfloat16, torch.float16]
HALF = 0.5


def interval(out16, y64, err):
    """(elements outside RNE16(y +- E), gate ratio) -- the two figures of _check_interval"""
    dt = out16.dtype
    lo, hi = (y64 - err).float().to(dt).double(), (y64 + err).float().to(dt).double()
    o = out16.double()
    return int((~((o >= lo) & (o <= hi))).sum()), float(((o - y64).abs() / (0.5 * ulp16(y64, dt) + err)).max())


def outside(v64, y64, err, dt):
    """fraction of a wrong variant's elements outside the interval"""
    lo, hi = (y64 - err).float().to(dt).double(), (y64 + err).float().to(dt).double()
    v = v64.float().to(dt).double()
    return float((~((v >= lo) & (v <= hi))).double().mean())


def inside_half(name, y32, y64, err, dt, fixed=0.0):
    """the float32 result uses at most half of E (beyond `fixed`, the part of E that is no matter of summation order: the 16-bit rounding of the
    attention probabilities), and its 16-bit rounding lies in the interval"""
    assert y32.dtype == torch.float32
    used = float((((y32.double() - y64).abs() - fixed).clamp_min(0.0) / (err - fixed).clamp_min(1e-300)).max()) if y32.numel() else 0.0
    n, ratio = interval(y32.to(dt), y64, err)
    assert n == 0 and used <= HALF, f"{name}: the float32 evaluation uses {used:.3g} of E ({n} elements outside the interval, gate ratio {ratio:.3g})"
    return used


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------------
def gn_f32(x16, gamma, beta, eps, silu, dt, mean_rstd=None):
    """float32, two-pass statistics; mean_rstd overrides them (wrong variants)"""
    x = x16.float()
    b, hw, c = x.shape
    if mean_rstd is None:
        xg = x.view(b, hw, GROUPS, c // GROUPS)
        flat = xg.permute(0, 2, 1, 3).reshape(b, GROUPS, -1)   # (a contiguous reduction: torch sums it in blocks, as the kernels do, not element by element)
        mean = flat.mean(dim=2).view(b, 1, GROUPS, 1)
        rstd = 1.0 / torch.sqrt(((flat - flat.mean(dim=2, keepdim=True)) ** 2).mean(dim=2).view(b, 1, GROUPS, 1) + eps)
        z = ((xg - mean) * rstd).reshape(b, hw, c) * gamma + beta
    else:
        mean, rstd = (t.float() for t in mean_rstd)
        z = (x - mean) * rstd * gamma + beta
    if silu:
        z = z * torch.sigmoid(z)
    return z


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_f32_within_half_gate(case, dt):
    name, b, c, hw, silu, sigma, env = case
    batch = 1 if hw * c * b > 4_000_000 else None   # (HW = 70000: one image)
    for ratio in gn_ratios(dt):
        x, gamma, beta = gn_inputs(case, ratio, dt, batch=batch)
        for eps in (1e-5, 1e-6):
            y64, err, _ = gn_ref_bound(x, gamma, beta, eps, silu)
            inside_half(f"{name} r{ratio} eps{eps}", gn_f32(x, gamma, beta, eps, silu, dt), y64, err, dt)


def _case(name):
    return next(c for c in GN_CASES if c[0] == name)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_groupnorm_wrong_statistics_fall_outside(dt):
    """HW = 37, C = 320 (370 values per group, chunks of 19 and 18 pixels): one pixel dropped, the last chunk dropped, the count off by one, the
    unbiased variance -- at every offset"""
    case = _case("stats1_apply2_hw37_b3")
    for ratio in gn_ratios(dt):
        x, gamma, beta = gn_inputs(case, ratio, dt)
        y64, err, _ = gn_ref_bound(x, gamma, beta, 1e-6, False)
        variants = {"one pixel dropped": group_stats(x, 1e-6, drop=1), "last chunk dropped": group_stats(x, 1e-6, drop=18),
                    "count + 1": group_stats(x, 1e-6, count_off=1), "count - 1": group_stats(x, 1e-6, count_off=-1),
                    "unbiased variance": group_stats(x, 1e-6, unbiased=True)}
        for vname, (mean, rstd) in variants.items():
            v, _, _ = norm_ref_bound(x, mean, rstd, gamma.double(), beta.double())
            f = outside(v, y64, err, dt)
            assert f >= 0.02, f"{vname} at ratio {ratio}: only {f:.3g} outside"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_groupnorm_ragged_last_chunk_dropped_falls_outside(dt):
    """HW = 4100: the last non-empty chunk holds 3 pixels (chunk 241 of 17-pixel chunks); a finalize that skipped it, or counted the empty
    chunks 242 .. 255 as full (n_all = 256 * 17 pixels), falls outside"""
    case = _case("stats1_apply2_hw4100_empty_chunks")
    for ratio in gn_ratios(dt):
        x, gamma, beta = gn_inputs(case, ratio, dt)
        y64, err, _ = gn_ref_bound(x, gamma, beta, 1e-6, False)
        cpg = x.shape[2] // GROUPS
        for vname, (mean, rstd), need in (("3-pixel chunk dropped", group_stats(x, 1e-6, drop=3), 0.02 if ratio else 0.0),
                                          ("empty chunks counted", group_stats(x, 1e-6, count_off=(256 * 17 - 4100) * cpg), 0.02)):
            v, _, _ = norm_ref_bound(x, mean, rstd, gamma.double(), beta.double())
            f = outside(v, y64, err, dt)
            # (at offset 0 three pixels of 4100 move the statistics by 7e-4 of a standard deviation at most: below the output rounding of both
            # element types, nothing to see; with an offset the count error multiplies the mean)
            assert f >= need, f"{vname} at ratio {ratio}: only {f:.3g} outside"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["stats1_small_sigma", "small_reg4_small_sigma"])
def test_groupnorm_wrong_eps_falls_outside(name, dt):
    """spread 2^-6 (variance 2.4e-4): eps 1e-5 for 1e-6 and the reverse change rstd by 1.8 %"""
    case = _case(name)
    x, gamma, beta = gn_inputs(case, 0, dt)
    for eps, other in ((1e-5, 1e-6), (1e-6, 1e-5)):
        y64, err, _ = gn_ref_bound(x, gamma, beta, eps, case[4])
        v, _, _ = gn_ref_bound(x, gamma, beta, other, case[4])
        f = outside(v, y64, err, dt)
        assert f >= 0.02, f"eps {other} for {eps}: only {f:.3g} outside"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_groupnorm_silu_of_rounded_preactivation_falls_outside(dt):
    case = _case("stats1_apply2_silu_hw64")
    x, gamma, beta = gn_inputs(case, 0, dt)
    y64, err, z = gn_ref_bound(x, gamma, beta, 1e-5, True)
    zr = r16(z, dt)
    f = outside(zr * torch.sigmoid(zr), y64, err, dt)
    assert f >= 0.02, f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_single_pass_statistics_fall_outside_at_the_large_offsets(dt):
    """fp32 single-pass {sum, sum of squares} partials finalised with qk - sk mk (_gn_single_pass_f32), HW = 4100 x 128 channels.  Against the
    statistics gate (scale / shift, _gn_scale_shift_bounds) the variant sits >= 8x outside at mean / std = 32 in both element types; against the
    OUTPUT gate it is visible where its error exceeds the output rounding: fp16 at mean / std = 256 (bf16 at 32 loses ~5e-5 of rstd, a fiftieth
    of the bf16 half-ulp -- that case is the statistics gate's)."""
    case = _case("stats1_apply2_hw4100_empty_chunks")
    top = gn_ratios(dt)[-1]
    for ratio in (32, top):
        x, gamma, beta = gn_inputs(case, ratio, dt)
        wsc, wsh = _gn_single_pass_f32(x.float(), GROUPS, 1e-6, gamma, beta)
        sc64, sh64, bound_sc, bound_sh = stats_ref_bounds(x, gamma, beta, 1e-6)
        rw = max(float(((wsc - sc64).abs() / bound_sc).max()), float(((wsh - sh64).abs() / bound_sh).max()))
        assert rw >= 8.0, f"ratio {ratio}: single-pass statistics only {rw:.3g}x the scale / shift gate"
        if dt == torch.float16 and ratio == 256:
            y64, err, _ = gn_ref_bound(x, gamma, beta, 1e-6, False)
            f = outside(x * wsc[:, None] + wsh[:, None], y64, err, dt)
            assert f >= 0.02, f"ratio {ratio}: single-pass statistics only {f:.3g} outside the output gate"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CONV_STATS_CASES, ids=[c[0] for c in CONV_STATS_CASES])
def test_conv_statistics_f32_two_pass_within_half_gate(case, dt):
    """the tensor a conv of these inputs stores (fp32 conv on the CPU, rounded to 16 bits -- the statistics gate is about the tensor, whatever
    wrote it): float32 two-pass statistics within half the scale / shift gate at every offset, single-pass ones >= 8x outside at mean / std = 256"""
    name, b, h, w, cin, cout, ks, form, with_res = case[:9]
    for ratio in gn_ratios(dt):
        x, wt, bias, gamma, beta, res = conv_stats_inputs(case, ratio, dt)
        if form != "conv":
            x = torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")
        y = torch.nn.functional.conv2d(x[:1], wt, bias, padding=ks // 2)
        if with_res:
            y = y + res[:1]
        y = r16(y.permute(0, 2, 3, 1).reshape(1, -1, cout).double(), dt)
        sc64, sh64, bound_sc, bound_sh = stats_ref_bounds(y, gamma, beta, 1e-6)
        yg = y.float().view(1, -1, GROUPS, cout // GROUPS).permute(0, 2, 1, 3).reshape(1, GROUPS, -1)   # (contiguous reduction: summed in blocks)
        mean = yg.mean(dim=2).view(1, 1, GROUPS, 1)
        rstd = 1.0 / torch.sqrt(((yg - yg.mean(dim=2, keepdim=True)) ** 2).mean(dim=2).view(1, 1, GROUPS, 1) + 1e-6)
        ex = lambda t: t.expand(1, 1, GROUPS, cout // GROUPS).reshape(1, cout)
        sc = ex(rstd) * gamma
        sh = beta - ex(mean) * sc
        r = max(float(((sc.double() - sc64).abs() / bound_sc).max()), float(((sh.double() - sh64).abs() / bound_sh).max()))
        assert r <= HALF, f"{name} r{ratio}: float32 two-pass statistics at {r:.3g} of the gate"
        if ratio == 256:   # (at 32 the short rows of these maps lose 0.3 .. 4 gates: the single-pass form is only marginal there)
            wsc, wsh = _gn_single_pass_f32(y.float(), GROUPS, 1e-6, gamma, beta)
            rw = max(float(((wsc - sc64).abs() / bound_sc).max()), float(((wsh - sh64).abs() / bound_sh).max()))
            assert rw >= 8.0, f"{name} r{ratio}: single-pass statistics only {rw:.3g}x the gate"


# ---- LayerNorm and the cross-attention fold --------------------------------------------------------------------------------------------------
def ln_f32(x16, gamma, beta, dt, eps=1e-5):
    x = x16.float()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    return (x - mean) * rstd * gamma + beta


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", LN_CASES)
def test_layernorm_f32_within_half_gate_and_wrong_variants_outside(case, dt):
    x, gamma, beta = ln_inputs(case, dt)
    y64, err = ln_ref_bound(x, gamma, beta)
    inside_half(f"layernorm{case}", ln_f32(x, gamma, beta, dt), y64, err, dt)
    rows, c, offset = case
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    variants = {"unbiased variance": (mean, (var * c / (c - 1) + 1e-5).rsqrt()),
                "last 8-channel vector dropped": (x[:, :-8].mean(1, keepdim=True), (((x[:, :-8] - x[:, :-8].mean(1, keepdim=True)) ** 2).mean(1, keepdim=True) + 1e-5).rsqrt())}
    for vname, (m, rs) in variants.items():
        v, _, _ = norm_ref_bound(x, m, rs, gamma.double(), beta.double())
        f = outside(v, y64, err, dt)
        need = 0.02 if (c <= 640 or dt == torch.float16 or vname.startswith("last")) else 0.0   # (1 / 2C of rstd at C >= 1280 is below the bf16 rounding)
        assert f >= need, f"layernorm{case} {vname}: only {f:.3g} outside"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", FOLD_CASES)
def test_cross_fold_f32_within_half_gate_and_wrong_variants_outside(case, dt):
    rows, c, heads = case
    if rows > 2500:
        case = (2500,) + case[1:]   # reduced row count on the CPU (the inputs of the first rows differ from the GPU case's: same generator, other seed)
    y, p = fold_inputs(case, dt)
    y64, err, (U, u0, G, c0) = fold_ref_bound(y, p, heads)
    yf = y.float()
    mean = yf.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((yf - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    ph = torch.sigmoid(((yf - mean) * rstd) @ U.float().t() + u0.float())
    out32 = yf + c0.float() + ph @ G.float()
    inside_half(f"cross_fold_y{case}", out32, y64, err, dt)
    out = out32.to(dt)
    n64, nerr = ln_ref_bound(out.double(), p["g3"].float(), p["b3"].float())
    inside_half(f"cross_fold_n3{case}", ln_f32(out.double(), p["g3"].float(), p["b3"].float(), dt), n64, nerr, dt)
    # wrong: the logit scale 1 / sqrt(d) missing from the fold; the last head left out; norm3 of the unrounded trunk
    dlog = (((y - y.mean(1, keepdim=True)) * (((y - y.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True) + 1e-5).rsqrt()) @ U.t() + u0)
    base = y + c0
    variants = {"logits not divided by 8": base + torch.sigmoid(8.0 * dlog) @ G,
                "last head dropped": base + torch.sigmoid(dlog[:, :-1]) @ G[:-1] if heads > 1 else None}
    for vname, v in variants.items():
        if v is not None:
            f = outside(v, y64, err, dt)
            assert f >= 0.02, f"cross_fold{case} {vname}: only {f:.3g} outside"
    n_unrounded, _ = ln_ref_bound(y64, p["g3"].float(), p["b3"].float())
    f = outside(n_unrounded, n64, nerr, dt)
    assert f >= 0.02, f"cross_fold{case} norm3 of the unrounded trunk: only {f:.3g} outside"


# ---- attention --------------------------------------------------------------------------------------------------------------------------------
def attn_f32(q, k, v, scale, dt, t_pad=0, rounded_sum=False, sc=None):
    """float32 attention with P rounded to the element type and an fp32 row sum.  q, k, v float64 [..., T, hd] of 16-bit values.  Wrong-variant
    knobs: t_pad zero keys counted in the row sum, the row sum of the rounded P, another exponent scale sc (log2 units per logit unit)"""
    s = q.float() @ k.float().transpose(-1, -2)
    sc = np.float32(scale * LOG2E if sc is None else sc)
    m = s.max(-1, keepdim=True).values
    if t_pad:
        m = m.clamp_min(0.0)
    p = torch.exp2((s - m) * sc)
    p16 = p.to(dt).float()
    l = (p16 if rounded_sum else p).sum(-1, keepdim=True)
    if t_pad:
        l = l + t_pad * torch.exp2(-m * sc)
    return (p16 @ v.float()) / l


def _attention_checks(name, q, k, v, scale, dt, hd, padded_tile=0):
    o, err, p, e_p = attn_ref_bound(q, k, v, scale, dt, hd)
    ratio = inside_half(name, attn_f32(q, k, v, scale, dt), o, err, dt, fixed=e_p)
    t = q.shape[-2]
    if t < 2 and not padded_tile:
        return ratio
    variants = {"scale without log2 e": attn_f32(q, k, v, scale, dt, sc=scale), "1 / sqrt(d) of another head size": attn_f32(q, k, v, scale * math.sqrt(0.5), dt)}
    if padded_tile:   # (the negative-logit inputs: a flat softmax, made for this variant alone)
        variants = {"padded keys in the row sum": attn_f32(q, k, v, scale, dt, t_pad=(-t) % padded_tile)}
    for vname, vout in variants.items():
        f = outside(vout.double(), o, err, dt)
        assert f >= 0.02, f"{name} {vname}: only {f:.3g} outside"
    # one key dropped in a peaked row: the key with the largest probability of each row
    top = p.argmax(-1, keepdim=True)
    pd = p.scatter(-1, top, 0.0)
    od = (pd / pd.sum(-1, keepdim=True)) @ v
    peaked = (p.gather(-1, top) > 0.25).expand_as(o)
    if bool(peaked.any()):
        lo, hi = (o - err).float().to(dt).double(), (o + err).float().to(dt).double()
        vd = od.float().to(dt).double()
        f = float((~((vd >= lo) & (vd <= hi)))[peaked].double().mean())
        assert f >= 0.5, f"{name} dominant key dropped: only {f:.3g} of the peaked rows' elements outside"
    # reported, not asserted (see the docstring): the row sum of the rounded probabilities
    _ = outside(attn_f32(q, k, v, scale, dt, rounded_sum=True).double(), o, err, dt)
    return ratio


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", FLASH64_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in FLASH64_CASES])
def test_flash64_f32_within_half_gate_and_wrong_variants_outside(case, dt):
    b, t, heads = case
    q, k, v = flash64_inputs(case, dt)
    hs = min(heads, 2) if t >= 1200 else heads   # reduced head count on the CPU for the long sequences (the first heads of the GPU case's tensors)
    q, k, v = (heads_split(z, heads)[:1, :hs] for z in (q, k, v))
    _attention_checks(f"flash64{case}", q, k, v, 0.125, dt, 64)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", NEG64_CASES)
def test_flash64_negative_logits_padded_keys_fall_outside(case, dt):
    b, t, heads = case
    q, k, v = (heads_split(z, heads) for z in negative_logit_inputs(b, t, heads * 64, dt, 1.5, 0.4))
    _attention_checks(f"flash64_neg{case}", q, k, v, 0.125, dt, 64, padded_tile=64)
    f = outside(padded_keys_counted(q, k, v, 0.125, 64), *attn_ref_bound(q, k, v, 0.125, dt, 64)[:2], dt)   # (the variant as the GPU file passes it)
    assert f >= 0.02, f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", NEG512_CASES)
def test_flash512_negative_logits_padded_keys_fall_outside(case, dt):
    b, t, _ = case
    q, k, v = negative_logit_inputs(b, t, 512, dt, 0.5, 0.166)
    _attention_checks(f"flash512_neg{case}", q, k, v, FLASH512_SCALE, dt, 512, padded_tile=32)
    f = outside(padded_keys_counted(q, k, v, FLASH512_SCALE, 32), *attn_ref_bound(q, k, v, FLASH512_SCALE, dt, 512)[:2], dt)
    assert f >= 0.02, f


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_flash64_spiky_f32_within_half_gate(dt):
    q, k, v = spiky_inputs(dt)
    _attention_checks("flash64_spiky", q, k, v, 0.125, dt, 64)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", FLASH512_CASES)
def test_flash512_f32_within_half_gate_and_wrong_variants_outside(case, dt):
    q, k, v = flash512_inputs(case, dt)
    _attention_checks(f"flash512{case}", q[:1], k[:1], v[:1], FLASH512_SCALE, dt, 512)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_flash512_outliers_f32_within_half_gate(dt):
    q, k, v = outlier_inputs(dt)
    o, err, _, e_p = attn_ref_bound(q, k, v, 1.0, dt, 512)
    inside_half("flash512_outliers", attn_f32(q, k, v, 1.0, dt), o, err, dt, fixed=e_p)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("L", [2, 77])
def test_cross_attention_f32_within_half_gate_and_wrong_variants_outside(L, dt):
    q, kc, vc = cross_inputs(L, dt)
    o, err = cross_ref_bound(q, kc, vc)
    rows, c = q.shape
    heads = c // 64
    qh, kh, vh = q.float().view(rows, heads, 64).transpose(0, 1), kc.view(L, heads, 64).transpose(0, 1), vc.view(L, heads, 64).transpose(0, 1)
    f32 = lambda scale: (torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1) @ vh).transpose(0, 1).reshape(rows, c)
    inside_half(f"cross_attn_L{L}", f32(0.125), o, err, dt)
    for vname, v in (("exp2 for exp", f32(0.125 / LOG2E)), ("1 / sqrt(d) of another head size", f32(0.125 * math.sqrt(0.5)))):
        f = outside(v.double(), o, err, dt)
        assert f >= 0.02, f"cross_attn_L{L} {vname}: only {f:.3g} outside"


# ---- row softmax ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", SOFTMAX_CASES)
def test_softmax_f32_within_half_gate_and_wrong_variants_outside(case, dt):
    rows, t, ld = case
    for f16_logits in (False, True):
        if f16_logits and not (ld % 4 == 0 and ld <= 16384):
            continue
        x = softmax_inputs(case, f16_logits)
        y64, err = softmax_ref_bound(x.double(), t, SOFTMAX_SCALE)
        out = torch.zeros(rows, ld)
        out[:, :t] = torch.softmax(x[:, :t] * np.float32(SOFTMAX_SCALE), dim=1)
        inside_half(f"softmax{case}", out, y64, err, dt)
        variants = {}
        if ld > t:
            w = torch.softmax(x.double() * SOFTMAX_SCALE, dim=1)   # the padding columns counted in the sum
            w[:, t:] = 0
            variants["sum over ld columns"] = w
            nz = out.clone()
            nz[:, t:] = out[:, :t].max()
            variants["padding columns not zeroed"] = nz.double()
        if t > 1:
            variants["scale without log2 e"] = torch.cat([torch.softmax(x[:, :t].double() * (SOFTMAX_SCALE / LOG2E), dim=1), y64[:, t:]], dim=1)
        for vname, v in variants.items():
            f = outside(v, y64, err, dt)
            need = 0.99 * (ld - t) / ld if vname == "padding columns not zeroed" else 0.02   # (every padding element, nothing else)
            assert f >= need, f"softmax{case} {vname}: only {f:.3g} outside (need {need:.3g})"
