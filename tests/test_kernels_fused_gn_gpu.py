"""Float64 interval gates for the kernels that normalise their operand on the way into an MFMA (GPU), both libraries: gp_conv2d_gn
(conv3x3_halo3_kernel<UPS, FUSED = 1 | 2> and conv3x3_halo2_kernel with in_scale set: GroupNorm apply (+ SiLU) inside the halo staging),
gp_decoder_tail (conv_few_kernel<1>), and the 16-bit bilinear_kernel.

The normalised operand is rounded to 16 bits BEFORE the MFMA, so a rounding flip moves an output by ulp16 |w|: no per-element interval around
ONE operand tensor expresses that.  The gate therefore carries the operand as an interval (operand_interval):

    y, e_n = norm_ref_bound(x, float64 group statistics, gamma, beta, silu)       the project's budgets, unchanged
    lo = r16(y - e_n), hi = r16(y + e_n), c = (lo + hi) / 2, d = (hi - lo) / 2    d == 0 wherever no flip is possible (share logged)

and the output follows by interval arithmetic (output_bound; conv_ref64 is the per-tap matmul of the exact file; the x2 nearest upsample
replicates c and d; the zero padding belongs to the NORMALISED tensor: c = d = 0 there):

    y_c = conv_ref64(c, w) + bias [+ residual]
    E   = conv_ref64(d, |w|)                                                      the operand's rounding flips
        + (K_nz + 2) 2^-24 (conv_ref64(|c| + d, |w|) + |bias| [+ |residual|])     fp32 accumulation in ANY order: K_nz non-zero weights per output
                                                                                  (adding an exact zero rounds nothing), the bias and the residual add

ReLU is 1-Lipschitz: applied to y_c, E unchanged.  The assertion is _check_interval of the exact file for every element; logged besides its
gate_ratio: e_used = max (|out - y_c| - ulp16(y_c) / 2)+ / E, the share of E in use beyond the output rounding.

Decoder tail (fp32 output: no output rounding): y_c, E per channel with K_nz = 1152; mean3: y = mean_k y_c, E' = mean_k E + 3 * 2^-24 mean_k S
(two v_add and the division; S the absolute sum above); clipped forms: [f(y - E') - 2^-23, f(y + E') + 2^-23], f(v) = (clamp(v, -1, 1) + 1) / 2
monotone, the slack two roundings at values <= 1 (the v_add of 1 at <= 2: 2^-24 * 2; the product with 0.5 is exact).

Wrong variant passed to every gate whose border share is >= 2 %: the float64 result whose padding holds act(shift) -- the un-normalised zero
pushed through the transform -- instead of 0.  tests/test_kernels_fused_gn_host.py proves on the CPU, on these inputs, that a float32 model
of the kernels lies inside every gate and that one-slot mutants fall outside.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernels_exact_gpu import DBG_HALO2, _dev, _eng, _tag, check_path, conv_ref64, precision, ulp16  # noqa: F401 (precision: autouse)
from test_kernels_glue_contract_gpu import C_BILINEAR_CASES
from test_kernels_interval_gpu import E23, E24, GROUPS, gate, gn_inputs, group_stats, norm_ref_bound, r16, seed_of

pytestmark = pytest.mark.gpu

TAIL_KNZ = 9 * 128
GN_MAXC = 2560   # conv_halo.hip: the widest input whose scale / shift table fits the kernel's LDS


# ---- the normalised operand as an interval, the output bound ---------------------------------------------------------------------------------
def operand_interval(x, gamma, beta, eps, silu, dtype):
    """x [B,HW,C] float64 (16-bit values).  Returns (c, d, pad): centre and radius of the 16-bit operand the MFMA may read, and [B,1,C]
    act(shift) rounded to 16 bits -- what a padding pixel holds when the transform runs over the un-normalised zero (the wrong variant)"""
    mean, rstd = group_stats(x, eps)
    ga, be = gamma.double(), beta.double()
    y, e_n, _ = norm_ref_bound(x, mean, rstd, ga, be, silu)
    lo, hi = r16(y - e_n, dtype), r16(y + e_n, dtype)
    sh = be - mean * rstd * ga
    return (lo + hi) / 2, (hi - lo) / 2, r16(sh * torch.sigmoid(sh) if silu else sh, dtype)


def _map(t, hw, ups):
    b, _, ch = t.shape
    t = t.reshape(b, hw[0], hw[1], ch)
    return F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1) if ups else t


def output_bound(c, d, wt, bias, hw, ups=False, res=None, relu=False, knz=None):
    """c, d [B,HW,C], wt [O,C,3,3], bias [O], res [B,Ho,Wo,O] or None, all float64.  Returns (y_c, E, S) [B,Ho,Wo,O]"""
    c4, d4 = _map(c, hw, ups), _map(d, hw, ups)
    wa = wt.abs()
    y = conv_ref64(c4, wt, bias)
    s = conv_ref64(c4.abs() + d4, wa, bias.abs())
    if res is not None:
        y, s = y + res, s + res.abs()
    k = (wt != 0).sum(dim=(1, 2, 3)).double() if knz is None else knz
    err = conv_ref64(d4, wa) + (k + 2) * E24 * s
    return (y.clamp_min(0) if relu else y), err, s


def padding_not_zero(c, pad, wt, bias, hw, ups=False, res=None, relu=False):
    """the wrong variant: y_c with `pad` [B,1,C] in the padding ring"""
    c4 = _map(c, hw, ups)
    b, ho, wo, ch = c4.shape
    xp = pad.reshape(b, 1, 1, ch).expand(b, ho + 2, wo + 2, ch).clone()
    xp[:, 1:-1, 1:-1] = c4
    y = conv_ref64(xp, wt, bias, pad=(0, 0), out_hw=(ho, wo))
    if res is not None:
        y = y + res
    return y.clamp_min(0) if relu else y


def border_share(ho, wo):
    return (ho * wo - max(ho - 2, 0) * max(wo - 2, 0)) / (ho * wo)


def e_used(out, y, err):
    """share of E in use beyond the output rounding (16-bit outputs)"""
    return float((((out.double() - y).abs() - 0.5 * ulp16(y, out.dtype)).clamp_min(0) / err).max())


# ---- gp_conv2d_gn -------------------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, Cin, Cout, ups, silu, residual + ReLU, env, path, group offset in standard deviations, eps values)
# path 1 = the persistent kernel conv3x3_halo3_kernel<UPS, FUSED>, 8 = the per-tile conv3x3_halo2_kernel (GENPERCEPT_IGEMM_DBG = 256)
_HALO2 = {"GENPERCEPT_IGEMM_DBG": str(DBG_HALO2)}
FGN_CASES = [
    ("persist_silu", 2, 20, 18, 128, 128, False, True, False, {}, 1, 0, (1e-6, 1e-5)),      # ragged tiles (2 x 2 of 16 x 16), two images
    ("persist_affine", 1, 17, 33, 64, 128, False, False, False, {}, 1, 0, (1e-6,)),         # FUSED = 1, one chunk: no chunk-ahead transform
    ("ups_silu", 1, 9, 11, 128, 128, True, True, False, {}, 1, 0, (1e-6,)),                 # UPS kernel, output 18 x 22
    ("ups_affine", 1, 8, 10, 64, 128, True, False, False, {}, 1, 0, (1e-6,)),               # UPS kernel, output 16 x 20
    # 10 channels per group: group borders inside the 8-channel slots and the 64-channel chunks (the group 60 .. 69 spans two chunks)
    ("groups_of_10", 1, 16, 24, 320, 128, False, True, False, {}, 1, 0, (1e-6,)),
    # three channel slices of the output, the last ragged (320 = 128 + 128 + 64); 6 channels per group; residual and ReLU epilogue
    ("slices_res_relu", 1, 16, 16, 192, 320, False, True, True, {}, 1, 0, (1e-6,)),
    # 25 tiles x 2 slices = 50 tile-slices per image against 256 / 8 = 32 workgroups: a workgroup walks several tiles
    ("several_tiles_per_wg", 8, 80, 80, 64, 256, False, True, False, {}, 1, 0, (1e-6,)),
    ("per_tile", 2, 33, 20, 128, 128, False, True, False, _HALO2, 8, 0, (1e-6,)),
    ("per_tile_ups", 1, 12, 10, 64, 128, True, True, False, _HALO2, 8, 0, (1e-6,)),
    # the shape of persist_silu with every group 8 standard deviations off zero: cancellation in shift = beta - mean * scale
    ("big_mean", 2, 20, 18, 128, 128, False, True, False, {}, 1, 8, (1e-6,)),
    # GN_MAXC: 40 chunks.  Run 20 times; in run m the weights are non-zero only on the 8-channel slots s with s % 20 == m (K_nz = 9 * 128: the bound
    # stays at the 128-channel size), so each of the 320 slots carries weight exactly once
    ("cin2560", 1, 16, 17, GN_MAXC, 128, False, True, False, {}, 1, 0, (1e-6,)),
]
CIN2560_RUNS = 20


def fgn_inputs(case, dtype, batch=None):
    """x [B,HW,Cin] (16-bit values, float64), gamma, beta (fp32): the gn_inputs recipe; wt [Cout,Cin,3,3] = r16(randn / sqrt(9 Cin_nz)), bias fp32,
    residual (16-bit values) or None.  CPU tensors."""
    name, b, h, w, cin, cout, ups, silu, res_relu, env, path, ratio, epss = case
    b = batch or b
    x, gamma, beta = gn_inputs((f"fused_gn_{name}", b, cin, h * w, silu, 1.0, {}), ratio, dtype)
    g = torch.Generator().manual_seed(seed_of("fused_gn_w", name))
    cin_nz = cin // CIN2560_RUNS if name == "cin2560" else cin
    wt = r16((torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin_nz)).double(), dtype)
    bias = 0.5 * torch.randn(cout, generator=g)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    res = r16(torch.randn(b, ho, wo, cout, generator=g).double(), dtype) if res_relu else None
    return x, gamma, beta, wt, bias, res


def slot_mask(cin, m):
    """[1,Cin,1,1]: 1 on the channels of the 8-channel slots s with s % 20 == m"""
    return ((torch.arange(cin) // 8) % CIN2560_RUNS == m).double().view(1, cin, 1, 1)


def fgn_runs(case):
    """weight masks of the case's launches: (suffix, m) -- m = None: the whole weight"""
    return [(f" m{m}", m) for m in range(CIN2560_RUNS)] if case[0] == "cin2560" else [("", None)]


# Measured on an MI355X, largest over the eps values and runs of a case (records, not thresholds) -- gate_ratio / e_used, bf16 | fp16 (a single
# flipped operand uses all of its d |w|, so e_used near 1 is no alarm: the float32 model of the host file reads the same figures on the same inputs):
#   persist_silu 0.921 / 0.475 | 0.608 / 0.163      persist_affine 0.952 / 0.664 | 0.736 / 0.213      ups_silu 0.910 / 0.486 | 0.589 / 0.233
#   ups_affine 0.949 / 0.662 | 0.724 / 0.272        groups_of_10 0.757 / 0.211 | 0.289 / 0.043        slices_res_relu 0.894 / 0.210 | 0.574 / 0.061
#   several_tiles_per_wg 0.973 / 0.877 | 0.813 / 0.490   per_tile 0.926 / 0.500 | 0.594 / 0.196       per_tile_ups 0.969 / 0.623 | 0.821 / 0.478
#   big_mean 0.920 / 0.495 | 0.636 / 0.179          cin2560 (20 runs) 0.933 / 0.624 | 0.647 / 0.344
# share of operand elements with d > 0: 0.4 - 1.2 % bf16 (4.6 % big_mean), 2.6 - 6.6 % fp16 (25.7 % big_mean); the wrong variant sits outside on
# 4.9 % (several_tiles_per_wg: its whole border) to 22 % of the elements
@pytest.mark.parametrize("case", FGN_CASES, ids=[c[0] for c in FGN_CASES])
def test_conv_gn_interval(case, metric_log, monkeypatch):
    e = _eng()
    name, b, h, w, cin, cout, ups, silu, res_relu, env, want, ratio, epss = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d, dt = _dev(), e.act_dtype()
    x, gamma, beta, wt_all, bias, res = (None if t is None else t.to(d) for t in fgn_inputs(case, dt))
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    xd = x.to(dt).contiguous().view(b, h, w, cin)
    resd = res.to(dt) if res_relu else None
    failures = []
    for eps in epss:
        c, dd, pad = operand_interval(x, gamma, beta, eps, silu, dt)
        share = float((dd > 0).double().mean())
        for sfx, m in fgn_runs(case):
            wt = wt_all if m is None else wt_all * slot_mask(cin, m).to(d)
            tag = f"conv_gn[{name}{sfx} eps{eps}]"
            wp = e.pack_weight(wt.float().cpu(), device=d)
            e.last_igemm_path()
            out = e.conv2d_gn(xd, wp, bias, cout, gamma, beta, GROUPS, eps, silu, ups=ups, residual=resd, act="relu" if res_relu else "none")
            path, _ = check_path(tag, want)
            y, err, _ = output_bound(c, dd, wt, bias.double(), (h, w), ups, res, res_relu)
            wrong = padding_not_zero(c, pad, wt, bias.double(), (h, w), ups, res, res_relu) if border_share(ho, wo) >= 0.02 else None
            gate(tag, out, y, err, metric_log, failures, wrong=wrong)
            metric_log(_tag(f"interval_used[{tag}]"), path=path, e_used=e_used(out, y, err), flip_share=share)
    assert not failures, "\n".join(failures)


def test_conv_gn_refuses_more_than_gn_maxc_channels():
    """Cin = 2624 (41 chunks) does not fit the kernel's scale / shift table: GP_ERR_INVALID, and the output is not touched"""
    e = _eng()
    d, dt = _dev(), e.act_dtype()
    b, h, w, cin, cout = 1, 16, 16, GN_MAXC + 64, 128
    g = torch.Generator().manual_seed(seed_of("fused_gn_refusal"))
    x = torch.randn(b, h, w, cin, generator=g).to(d).to(dt)
    wp = e.pack_weight(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin), device=d)
    gamma, beta, bias = torch.ones(cin, device=d), torch.zeros(cin, device=d), torch.zeros(cout, device=d)
    out = torch.full((b, h, w, cout), float("nan"), dtype=dt, device=d)
    st = e.load_library().gp_conv2d_gn(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, out.data_ptr(), b, h, w, cin, cout, 0, e.ACT["none"],
                                       gamma.data_ptr(), beta.data_ptr(), GROUPS, 1e-6, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == e.GP_ERR_INVALID, st
    assert bool(torch.isnan(out).all()), "a refused launch must leave the output as it was"


# ---- gp_decoder_tail ----------------------------------------------------------------------------------------------------------------------------
# (B, H, W): ragged tiles, two images; 3 x 10 x 10 = 300 tiles on at most 256 workgroups: a workgroup takes several tiles
TAIL_CASES = [(2, 33, 17), (3, 160, 160)]


def tail_inputs(case, dtype):
    """the generator of test_decoder_tail_fused (tests/test_kernels_gpu.py) with the weight factor 1.5 for its 3: at 3, 39 - 61 % of the outputs
    are clipped and hide the conv.  Returns x [B,HW,128] (16-bit values, float64), gamma, beta, wt [3,128,3,3] (float64), bias"""
    b, h, w = case
    g = torch.Generator().manual_seed(h * 100 + w + b)
    x = torch.randn(b, 128, h, w, generator=g) * 1.5 + 0.3
    wt = torch.randn(3, 128, 3, 3, generator=g) / math.sqrt(128 * 9) * 1.5
    bias = torch.randn(3, generator=g) * 0.2
    gamma, beta = torch.randn(128, generator=g) * 0.3 + 1.0, torch.randn(128, generator=g) * 0.2
    return r16(x.permute(0, 2, 3, 1).contiguous().view(b, h * w, 128).double(), dtype), gamma, beta, r16(wt.double(), dtype), bias


def tail_f(v):
    return (v.clamp(-1, 1) + 1) / 2


def tail_interval(y, err, s, mean3, raw):
    """y, E, S [B,H,W,3] per channel -> (lo, hi, y') [B,H,W,1 or 3]: the interval of the fp32 output and the float64 value before the clip"""
    if mean3:
        y, err = y.mean(-1, keepdim=True), err.mean(-1, keepdim=True) + 3 * E24 * s.mean(-1, keepdim=True)   # v_add, v_add, the division by 3
    if raw:
        return y - err, y + err, y
    return tail_f(y - err) - E23, tail_f(y + err) + E23, y   # v_add 1 (at <= 2: 2^-23), the exact product with 0.5


def tail_outside(v, lo, hi):
    return ~((v >= lo) & (v <= hi))


def tail_gate(name, out, lo, hi, log, failures, wrong=None):
    """lo <= out <= hi for every element of an fp32 output [B,H,W,K]; gate_ratio = max |out - mid| / half width"""
    o = out.double()
    bad = tail_outside(o, lo, hi)
    n = int(bad.sum())
    ratio = float(((o - (lo + hi) / 2).abs() / ((hi - lo) / 2)).max())
    rec = dict(mismatches=n, elements=out.numel(), gate_ratio=ratio)
    if wrong is not None:
        rec["wrong_outside"] = float(tail_outside(wrong, lo, hi).double().mean())
    log(_tag(f"interval[{name}]"), **rec)
    if n:
        idx = bad.flatten().nonzero()[:5, 0]
        first = [(int(i), float(lo.flatten()[i]), float(hi.flatten()[i]), float(o.flatten()[i])) for i in idx]
        failures.append(f"{name}: {n} elements outside the interval, max ratio {ratio:.3g}; first (index, lo, hi, got): {first}")
    if wrong is not None and rec["wrong_outside"] < 0.02:
        failures.append(f"{name}: the wrong variant is not rejected ({rec['wrong_outside']:.3g})")


def assert_clip_matters(name, y):
    """a condition on the inputs, not a measurement: the clip has to matter (>= 2 % of the float64 values beyond +-1), but most pixels have to
    discriminate (<= 35 %)"""
    clipped = float((y.abs() > 1).double().mean())
    assert 0.02 <= clipped <= 0.35, f"{name}: {clipped:.3g} of the reference is clipped"
    return clipped


# Measured on an MI355X (records, not thresholds) -- gate_ratio of the raw forms, three channels / mean3, bf16 | fp16 (the clipped forms read 1.00
# wherever an output is exactly 0 or 1 against a half width of 2^-23):
#   (2, 33, 17) 0.459 / 0.283 | 0.169 / 0.103      (3, 160, 160) 0.663 / 0.417 | 0.232 / 0.120
# clipped share of the reference: (2, 33, 17) 32.5 % / 13.5 %, (3, 160, 160) 31.0 % / 5.0 %; wrong variant outside: 17.1 % / 2.5 % (the border)
@pytest.mark.parametrize("case", TAIL_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in TAIL_CASES])
def test_decoder_tail_interval(case, metric_log):
    e = _eng()
    b, h, w = case
    d, dt = _dev(), e.act_dtype()
    x, gamma, beta, wt, bias = (t.to(d) for t in tail_inputs(case, dt))
    xd = x.to(dt).contiguous().view(b, h, w, 128)
    wp = e.pack_weight(wt.float().cpu(), device=d)
    c, dd, pad = operand_interval(x, gamma, beta, 1e-6, True, dt)
    y, err, s = output_bound(c, dd, wt, bias.double(), (h, w), knz=TAIL_KNZ)
    yw = padding_not_zero(c, pad, wt, bias.double(), (h, w))
    metric_log(_tag(f"interval_used[decoder_tail{case}]"), flip_share=float((dd > 0).double().mean()))
    failures = []
    for mean3 in (False, True):
        for raw in (False, True):
            name = f"decoder_tail{case}[mean3={int(mean3)} raw={int(raw)}]"
            out = e.decoder_tail(xd, wp, bias, gamma, beta, GROUPS, 1e-6, mean3, raw=raw).permute(0, 2, 3, 1)
            lo, hi, yv = tail_interval(y, err, s, mean3, raw)
            if not raw:
                metric_log(_tag(f"clipped[{name}]"), clipped=assert_clip_matters(name, yv))
            # wrong variant on the raw forms: the border is 2.5 % of the 160 x 160 case, and the clip hides up to a third of it
            tail_gate(name, out, lo, hi, metric_log, failures, wrong=(yw.mean(-1, keepdim=True) if mean3 else yw) if raw else None)
    assert not failures, "\n".join(failures)


# ---- gp_bilinear (16-bit bilinear_kernel) -------------------------------------------------------------------------------------------------------
def bilinear_cases():
    """C_BILINEAR_CASES with C rounded up to a multiple of 8 (the 16-bit kernel moves 8-channel vectors): the last, 48 -> 192 at C = 232, wraps the
    grid loop"""
    return [(hw_in, hw_out, align, b, (c + 7) // 8 * 8) for hw_in, hw_out, align, b, c in C_BILINEAR_CASES]


def bilinear_inputs(case, dtype):
    (hi, wi), (ho, wo), align, b, c = case
    g = torch.Generator().manual_seed(seed_of("bilinear16", hi, wi, ho, wo, align, b, c))
    return r16(torch.randn(b, hi, wi, c, generator=g).double(), dtype)


def bilinear_ref_bound(x, case):
    """y64, E as test_c_bilinear_interval derives them (the same kernel template), on the 16-bit inputs; and the wrong variant: the other
    align_corners setting"""
    (hi, wi), (ho, wo), align, b, c = case
    x64 = x.permute(0, 3, 1, 2)
    y64 = F.interpolate(x64, size=(ho, wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    yabs = F.interpolate(x64.abs(), size=(ho, wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    # <= 4 roundings at the source coordinate's size per axis move the weights l, 1 - l; a moved weight shifts the result by that times the
    # difference of two taps (<= 2 max |x|); then the four weight products and the four-term sum: 8 roundings at sum w |tap|
    err = 4 * E24 * (max(hi, 1) + max(wi, 1)) * 2 * float(x64.abs().max()) + 8 * E24 * yabs
    wrong = F.interpolate(x64, size=(ho, wo), mode="bilinear", align_corners=not align).permute(0, 2, 3, 1) if (hi, wi) != (1, 1) else None
    return y64, err, wrong


@pytest.mark.parametrize("case", bilinear_cases())
def test_bilinear_interval(case, metric_log):
    e = _eng()
    d, dt = _dev(), e.act_dtype()
    x = bilinear_inputs(case, dt).to(d)
    out = e.bilinear(x.to(dt), case[1], case[2])
    y64, err, wrong = bilinear_ref_bound(x, case)
    failures = []
    gate(f"bilinear{case}", out, y64, err, metric_log, failures, wrong=wrong)  # measured: bf16 <= 0.995, fp16 <= 0.960 (output rounding alone reaches 1)
    assert not failures, "\n".join(failures)
