"""Float64 and bit-exact tests of the 16-bit elementwise / layout kernels between the matrix products (csrc/elementwise.hip), both libraries,
through the stateless gp_* test entries: rgb_prologue, concat, concat_stats (+ gn_finalize_tiles mode 4), the statistics rows of rgb_conv_in
(mode 3), nchw <-> nhwc, ddim_init, ddim_step, decode_epilogue, scale_pad, pointwise_small, relu, add, dpt_final, minmax_norm.  The fp32
forms of the contract precision (the same templates instantiated for float) run the same checks from tests/test_kernels_glue_contract_gpu.py
(the run_* functions below take `contract`).

References are float64 on the values the kernel reads; nothing of a kernel's tiling is emulated.
  * Pure data movement and single roundings are bit-exact: zero mismatches (check_exact).
  * Arithmetic kernels get a float64 bound E with every term written beside the instruction it pays for (E24 = 2^-24, one fp32 rounding;
    the compiler may contract a * b + c into one v_fma, which only removes roundings).  16-bit outputs: RNE16(y64 - E) <= out <= RNE16(y64 + E)
    (_check_interval); fp32 outputs: |out - y64| <= E.  The gate ratio goes to parity_log.jsonl.
  * Every strided or partial destination is prefilled with a sentinel bit pattern, with a guard tail behind the tensor: what the kernel
    must not touch is unchanged, what it must zero is zero.
  * Every test evaluates its nearest wrong variant, which must change bits or leave the gate (wrong_outside >= 0.02).
  * Grid-stride loops wrap once in one case per kernel: more than 4096 * 256 items (grid_for; contract.hip's cgrid: 8192 * 256).
tests/test_kernels_glue_host.py evaluates the same references in float32 on the CPU and checks the argument validation of the entries.
"""
import math

import numpy as np
import pytest
import torch

from test_contract_kernels_gpu import _gn_scale_shift_bounds
from test_kernels_exact_gpu import _dev, _eng, _tag, check_exact, precision  # noqa: F401 (precision: autouse, both libraries)
from test_kernels_interval_gpu import E24, GROUPS, gate, gn_ratios, group_stats, r16, seed_of, stats_ref_bounds

pytestmark = pytest.mark.gpu

WRAP = 4096 * 256        # items of one pass of an elementwise.hip grid-stride loop (grid_for)
WRAP_C = 8192 * 256      # the same for contract.hip (cgrid)
GUARD = 64               # sentinel elements behind every destination
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------
def elt(contract):
    """element type of the activations: the library's 16-bit type, or fp32 in the contract precision"""
    return torch.float32 if contract else _eng().act_dtype()


def wrap_items(contract):
    return WRAP_C if contract else WRAP


def ints(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def sentinel(numel, dt, device):
    """flat buffer of numel + GUARD elements, every one the sentinel bit pattern"""
    buf = torch.empty(numel + GUARD, dtype=dt, device=device)
    ints(buf).fill_(SENT16 if buf.element_size() == 2 else SENT32)
    return buf


def is_sentinel(t):
    return ints(t) == (SENT16 if t.element_size() == 2 else SENT32)


def assert_untouched(name, t):
    n = int((~is_sentinel(t)).sum())
    assert n == 0, f"{name}: {n} elements outside the destination were written"


def check_f32(name, out, y64, err, log, failures, wrong=None):
    """fp32 output: |out - y64| <= E for every element (NaN must meet NaN); logs the gate ratio max |out - y64| / E"""
    o = out.double()
    nan_ok = torch.isnan(o) & torch.isnan(y64)
    d = (o - y64).abs()
    bad = ~((d <= err) | nan_ok)
    ratio = float(torch.where(d > 0, d / (err + 1e-300), torch.zeros_like(d)).nan_to_num(0.0).max()) if o.numel() else 0.0
    rec = dict(mismatches=int(bad.sum()), elements=out.numel(), gate_ratio=ratio)
    if wrong is not None:
        rec["wrong_outside"] = float(((wrong - y64).abs() > err).double().mean())
    log(_tag(f"interval[{name}]"), **rec)
    if rec["mismatches"]:
        idx = bad.flatten().nonzero()[:5, 0]
        first = [(int(i), float(o.flatten()[i]), float(y64.flatten()[i]), float(err.expand_as(y64).flatten()[i])) for i in idx]
        failures.append(f"{name}: {rec['mismatches']} elements beyond E, max ratio {ratio:.3g}; first (index, got, y64, E): {first}")
    if wrong is not None and rec["wrong_outside"] < 0.02:
        failures.append(f"{name}: the wrong variant is not rejected ({rec['wrong_outside']:.3g})")


def check_out(name, out, y64, err, log, failures, wrong=None):
    """the gate of an arithmetic kernel's output in either storage type"""
    if out.dtype == torch.float32:
        check_f32(name, out, y64, err, log, failures, wrong)
    else:
        gate(name, out, y64, err if torch.is_tensor(err) else torch.full_like(y64, err), log, failures, wrong=wrong)


def differs(name, out, wrong):
    """a wrong variant of a bit-exact kernel must change bits"""
    assert int((out.float() != wrong.float()).sum()) > 0, f"{name}: the wrong variant gives the same bits"


# ---- rgb_prologue / c_rgb_split ------------------------------------------------------------------------------------------------------------
# (B, H, W, Cpad): HW = 1, HW = 37, one wrap of the loop over pixels
RGB_CASES = [(3, 1, 1, 8), (3, 37, 1, 64), (2, 5, 7, 16), (1, 1, WRAP + 300, 8)]


def rgb_inputs(case, u8):
    b, h, w, _ = case
    g = torch.Generator().manual_seed(seed_of("rgb", b, h, w, u8))
    if u8:
        x = torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8)
        x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)[: x.numel()]
        return x
    return torch.rand(b, 3, h, w, generator=g) * 2 - 1


def rgb_values(rgb):
    """the fp32 value of every real channel: x / 255 * 2 - 1 in fp32 in that order (u8), or the float itself"""
    return (rgb.float() / 255.0 * 2.0 - 1.0) if rgb.dtype == torch.uint8 else rgb.float()


def run_rgb_prologue(case, u8, contract, log):
    e = _eng()
    b, h, w, cpad = case
    if contract:
        cpad = 64
        if b * h * w > WRAP:
            w = WRAP_C // 8 + 300   # (c_rgb_split_kernel: 8 items per pixel)
    d = _dev()
    rgb = rgb_inputs((b, h, w, cpad), u8)
    v = rgb_values(rgb).permute(0, 2, 3, 1).reshape(-1, 3).to(d)         # (evaluated on the CPU: IEEE division)
    vw = rgb_values(rgb).reshape(-1, 3).to(d)                            # wrong variant: NCHW read as NHWC
    rgb = rgb.to(d)
    name = f"rgb_prologue[{b}x{h}x{w} cpad {cpad} {'u8' if u8 else 'f32'}{' contract' if contract else ''}]"
    if contract:
        buf = sentinel(b * h * w * 192, torch.bfloat16, d)
        e.rgb_prologue(rgb, buf, cpad, contract=True)
        out = buf[:-GUARD].view(-1, 192)
        full = torch.zeros(b * h * w, 64, device=d)
        full[:, :3] = v
        hi = full.to(torch.bfloat16)
        lo = (full - hi.float()).to(torch.bfloat16)
        check_exact(name, out, torch.cat([hi, lo, hi], dim=1), log)      # A order [hi | lo | hi], RNE both times, channels 3 .. 63 zero
        if b * h * w > 3:
            differs(name, out[:, 64:128], hi)                            # B order [hi | hi | lo] where A order is due
            wfull = torch.zeros_like(full)
            wfull[:, :3] = vw
            differs(name, out[:, :64], wfull.to(torch.bfloat16))
    else:
        dt = e.act_dtype()
        buf = sentinel(b * h * w * cpad, dt, d)
        e.rgb_prologue(rgb, buf, cpad)
        out = buf[:-GUARD].view(-1, cpad)
        want = torch.zeros(b * h * w, cpad, dtype=dt, device=d)
        want[:, :3] = v.to(dt)                                           # RNE16 of the fp32 value; channels 3 .. Cpad-1 zero
        check_exact(name, out, want, log)
        if b * h * w > 3:
            wrong = torch.zeros_like(want)
            wrong[:, :3] = vw.to(dt)
            differs(name, out, wrong)
    assert_untouched(name, buf[-GUARD:])


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", RGB_CASES)
def test_rgb_prologue_exact(case, u8, metric_log):
    run_rgb_prologue(case, u8, False, metric_log)  # measured: 0 mismatches, both libraries


# ---- concat (16-bit / fp32) ----------------------------------------------------------------------------------------------------------------
# (Ca, Cb, pixels): the UNet's widths; the last case wraps the loop (pixels * (Ca + Cb) / vector > one pass)
CONCAT_CASES = [(8, 8, 1), (8, 8, 3 * 37), (320, 640, 3 * 37), (1280, 1280, 37), (320, 640, None)]


def run_concat(case, contract, log):
    e = _eng()
    ca, cb, pixels = case
    vec = 4 if contract else 8
    if pixels is None:
        pixels = wrap_items(contract) // ((ca + cb) // vec) + 3
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("concat", ca, cb, pixels))
    a = torch.randn(pixels, ca, generator=g).to(dt).to(d)
    b = torch.randn(pixels, cb, generator=g).to(dt).to(d)
    out = e.concat(a, b, contract=contract)
    name = f"concat[{ca}+{cb} x {pixels}{' contract' if contract else ''}]"
    check_exact(name, out, torch.cat([a, b], dim=1), log)                # [hidden, skip]
    differs(name, out, torch.cat([b, a], dim=1))                         # wrong variant: [skip, hidden]


@pytest.mark.parametrize("case", CONCAT_CASES)
def test_concat_exact(case, metric_log):
    run_concat(case, False, metric_log)  # measured: 0 mismatches


# ---- concat_stats: the copy + GroupNorm partials, finalised (gn_finalize_tiles_kernel mode 4) ------------------------------------------------
# (name, Ca, Cb, B, HW, bm, groups): bm 0 = concat_stats_bm's choice.  (1280, 1280): 320 vectors per pixel = two blockIdx.y slices, the second
# with 64 of 256 threads at work.  HW = 192 is a multiple of every tile size.
CAT_STATS_CASES = [
    ("c16_b3", 8, 8, 3, 48, 0, 2),
    ("c960_12x12", 320, 640, 2, 144, 0, 32),
    ("c2560_two_slices", 1280, 1280, 1, 144, 0, 32),
    ("c960_bm16", 320, 640, 2, 192, 16, 32), ("c960_bm32", 320, 640, 2, 192, 32, 32), ("c960_bm48", 320, 640, 2, 192, 48, 32),
    ("c960_bm64", 320, 640, 2, 192, 64, 32),
    ("c2560_bm64", 1280, 1280, 2, 192, 64, 32),
]


def cat_stats_inputs(case, ratio, dtype):
    """gn_inputs of tests/test_kernels_interval_gpu.py for any group count: x [B,HW,C] of 16-bit values (float64), every channel of a group
    sharing an offset of `ratio` group standard deviations with a different sign per group and image; gamma, beta (fp32)"""
    name, ca, cb, b, hw, bm, groups = case
    c = ca + cb
    g = torch.Generator().manual_seed(seed_of("catstats", name, ratio))
    chan = 0.75 + 0.5 * torch.rand(c, generator=g, dtype=torch.float64)
    x = torch.randn(b, hw, c, generator=g, dtype=torch.float64) * chan
    sign = 1.0 - 2.0 * ((torch.arange(groups).view(1, 1, groups) + torch.arange(b).view(b, 1, 1)) % 2).double()
    x = x + (ratio * sign).repeat_interleave(c // groups, dim=2)
    gamma = (1 + 0.3 * torch.randn(c, generator=g)).float()
    beta = (0.5 * torch.randn(c, generator=g)).float()
    return r16(x, dtype), gamma, beta


def stats_bounds(y, gamma, beta, eps, groups):
    """stats_ref_bounds for any group count"""
    if groups == GROUPS:
        return stats_ref_bounds(y, gamma, beta, eps)
    mean, rstd = group_stats(y, eps, groups=groups)
    mean, rstd = mean[:, 0], rstd[:, 0]
    ga, be = gamma.double(), beta.double()
    sc = rstd * ga
    bound_sc, bound_sh = _gn_scale_shift_bounds(sc, mean.abs() * rstd, ga.abs(), be.abs())
    return sc, be - mean * sc, bound_sc, bound_sh


def single_pass_stats(y, bm, gamma, beta, eps, groups):
    """wrong variant: fp32 {sum, sum of squares} per (bm pixels, channel), summed pixel by pixel, finalised with qk - sk * mk -- what
    concat_stats_kernel wrote before it centred its partials.  y [B,HW,C] float64 of 16-bit values; returns float64 scale, shift [B,C]"""
    b, hw, c = y.shape
    t = y.float().view(b, hw // bm, bm, c)
    s = torch.zeros(b, hw // bm, c, dtype=torch.float32, device=y.device)
    q = torch.zeros_like(s)
    for r in range(bm):
        s = s + t[:, :, r]
        q = q + t[:, :, r] * t[:, :, r]
    mk = s / bm
    m2k = (q - s * mk).clamp_min(0.0)
    cpg = c // groups
    n_all = float(hw * cpg)
    mean = (s.view(b, -1, groups, cpg).sum(dim=(1, 3)) / n_all)                                  # [B,G] fp32
    m2 = (m2k + bm * (mk - mean.repeat_interleave(cpg, dim=1)[:, None]) ** 2).view(b, -1, groups, cpg).sum(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(m2 / n_all + eps)
    sc = rstd.repeat_interleave(cpg, dim=1).double() * gamma.double()
    return sc, beta.double() - mean.repeat_interleave(cpg, dim=1).double() * sc


def stats_ratios(sc, sh, y, gamma, beta, eps, groups):
    sc64, sh64, bound_sc, bound_sh = stats_bounds(y, gamma, beta, eps, groups)
    return float(((sc.double() - sc64).abs() / bound_sc).max()), float(((sh.double() - sh64).abs() / bound_sh).max())


@pytest.mark.parametrize("case", CAT_STATS_CASES, ids=[c[0] for c in CAT_STATS_CASES])
def test_concat_statistics_interval(case, metric_log):
    e = _eng()
    name, ca, cb, b, hw, bm, groups = case
    d, dt = _dev(), e.act_dtype()
    eps = 1e-6
    failures = []
    for ratio in gn_ratios(dt):
        x, gamma, beta = cat_stats_inputs(case, ratio, dt)
        x, gamma, beta = x.to(d), gamma.to(d), beta.to(d)
        a, bb = x[..., :ca].to(dt).contiguous(), x[..., ca:].to(dt).contiguous()
        out, sc, sh, used = e.concat_stats(a, bb, gamma, beta, groups, eps, bm)
        assert used == (bm or e.concat_stats_bm(hw, b * hw, ca + cb)) and hw % used == 0, (name, used)
        check_exact(f"concat_stats[{name} r{ratio}]", out, torch.cat([a, bb], dim=2), metric_log, bm=used)
        differs(name, out, torch.cat([bb, a], dim=2))
        r_sc, r_sh = stats_ratios(sc, sh, out.double(), gamma, beta, eps, groups)
        w_sc, w_sh = stats_ratios(*single_pass_stats(out.double(), used, gamma, beta, eps, groups), out.double(), gamma, beta, eps, groups)
        metric_log(_tag(f"interval_stats[concat {name} r{ratio}]"), bm=used, gate_ratio_scale=r_sc, gate_ratio_shift=r_sh, wrong_single_pass=max(w_sc, w_sh))
        # measured: bf16 <= 0.14, fp16 <= 0.14 at every offset and tile size.  With the single-pass {sum, sum x^2} partials the kernel wrote before (same
        # inputs): bf16 1.36 at offset 32 with bm 48 (<= 0.13 elsewhere); fp16 0.75 - 0.86 (bm 16) and 2.6 - 2.9 (bm 32 .. 64) at offset 8, 9.4 - 40 at
        # 32, 203 - 1030 at 256
        if not (r_sc <= 1.0 and r_sh <= 1.0):
            failures.append(f"{name} r{ratio}: scale {r_sc:.3g}, shift {r_sh:.3g}")
        if dt == torch.float16 and ratio == 256 and max(w_sc, w_sh) <= 1.0:   # the single-pass form leaves the gate where the grid allows the offset
            failures.append(f"{name} r{ratio}: single-pass statistics are not rejected ({max(w_sc, w_sh):.3g})")
    assert not failures, "\n".join(failures)


# ---- rgb_conv_in: the statistics rows of the persistent workgroups ("mode 3": {sum, centred M2} + pixel counts) ---------------------------------
# (B, H, W, Cout): 17 x 33 and 40 x 24 leave ragged 16 x 16 tiles; Cout = 160 has a second channel slice of 32
RGB_STATS_CASES = [(1, 17, 33, 128), (3, 17, 33, 128), (1, 40, 24, 128), (3, 40, 24, 128), (2, 17, 33, 160)]


def rgb_stats_inputs(case, u8, ratio, dtype):
    """the image, 3 -> Cout weights of 16-bit values scaled for a unit-spread output (the image has variance 1 / 3), a bias carrying a
    group-constant offset of `ratio`, gamma, beta"""
    b, h, w, cout = case
    g = torch.Generator().manual_seed(seed_of("rgbstats", b, h, w, cout, u8, ratio))
    rgb = torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8) if u8 else torch.rand(b, 3, h, w, generator=g) * 2 - 1
    wt = (torch.randn(cout, 3, 3, 3, generator=g) / 3.0).to(dtype).float()
    sign = 1.0 - 2.0 * (torch.arange(GROUPS) % 2).float()
    bias = (ratio * sign).repeat_interleave(cout // GROUPS) + 0.1 * torch.randn(cout, generator=g)
    return rgb, wt, bias, 1 + 0.3 * torch.randn(cout, generator=g), 0.5 * torch.randn(cout, generator=g)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", RGB_STATS_CASES)
def test_rgb_conv_in_statistics_interval(case, u8, metric_log):
    e = _eng()
    b, h, w, cout = case
    d, dt = _dev(), e.act_dtype()
    eps = 1e-6
    failures = []
    for ratio in (0, 8):
        rgb, wt, bias, gamma, beta = (t.to(d) for t in rgb_stats_inputs(case, u8, ratio, dt))
        wp = e.pack_weight(wt, 64, device=d)
        y, sc, sh = e.rgb_conv_in_stats(rgb, wp, bias, cout, gamma, beta, GROUPS, eps)
        name = f"rgb_conv_in_stats[{b}x{h}x{w}x{cout} {'u8' if u8 else 'f32'} r{ratio}]"
        check_exact(name, y, e.rgb_conv_in(rgb, wp, bias, cout), metric_log)   # the statistics epilogue leaves the output as it is
        y64 = y.double().view(b, h * w, cout)
        r_sc, r_sh = stats_ratios(sc, sh, y64, gamma, beta, eps, GROUPS)
        # wrong variant: the last image row left out of the statistics (a pixel count or a tile lost)
        mean, rstd = group_stats(y64, eps, drop=w)
        wsc = rstd[:, 0] * gamma.double()
        rw = max(stats_ratios(wsc, beta.double() - mean[:, 0] * wsc, y64, gamma, beta, eps, GROUPS))
        metric_log(_tag(f"interval_stats[{name}]"), gate_ratio_scale=r_sc, gate_ratio_shift=r_sh, wrong_row_dropped=rw)
        # measured: bf16 <= 0.083, fp16 <= 0.091 (both offsets), the wrong variant >= 2900.  With the raw {sum, sum x^2} rows the kernel wrote before:
        # bf16 <= 0.69, fp16 up to 1.10 (1 x 17 x 33 x 128, uint8, offset 8: the failure that had the kernel centre its sums about the bias)
        if not (r_sc <= 1.0 and r_sh <= 1.0 and rw > 1.0):
            failures.append(f"{name}: scale {r_sc:.3g}, shift {r_sh:.3g}, wrong variant {rw:.3g}")
    assert not failures, "\n".join(failures)


# ---- layout: fp32 NCHW -> NHWC (zero-padded channels) and back -------------------------------------------------------------------------------
# (B, C, H, W, Cpad / ld)
LAYOUT_CASES = [(3, 4, 1, 1, 8), (3, 5, 37, 1, 64), (2, 3, 5, 7, 3), (1, 5, 1, 16400, 64)]


def run_nchw_to_nhwc(case, contract, log):
    e = _eng()
    b, c, h, w, cpad = case
    if contract and h * w > 10000:
        w *= 2   # (one pass of cgrid is twice as long)
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("nchw", *case))
    x = (torch.randn(b, c, h, w, generator=g) * torch.exp(2 * torch.randn(b, c, h, w, generator=g))).to(d)
    buf = sentinel(b * h * w * cpad, dt, d)
    e.nchw_to_nhwc(x, buf, cpad, contract=contract)
    out = buf[:-GUARD].view(b, h * w, cpad)
    want = torch.zeros(b, h * w, cpad, dtype=dt, device=d)
    want[..., :c] = x.view(b, c, h * w).transpose(1, 2).to(dt)            # RNE16 of the fp32 value (fp32: the value); channels >= C zero
    name = f"nchw_to_nhwc{case}{' contract' if contract else ''}"
    check_exact(name, out, want, log)
    assert_untouched(name, buf[-GUARD:])
    if h * w > 1:
        wrong = torch.zeros_like(want)
        wrong[..., :c] = x.reshape(b, h * w, c).to(dt)                    # NCHW read as NHWC
        differs(name, out, wrong)


def run_nhwc_to_nchw(case, contract, log):
    e = _eng()
    b, c, h, w, ld = case
    if contract and h * w > 10000:
        w *= 2
    ld = max(ld, c)
    if h * w > 10000:
        c, ld = 64, 72   # (the loop runs over B * C * HW outputs)
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("nhwc", *case))
    x = torch.randn(b * h * w, ld, generator=g).to(dt).to(d)
    out = e.nhwc_to_nchw(x, b, c, h, w, ld, contract=contract)
    name = f"nhwc_to_nchw{case}{' contract' if contract else ''}"
    check_exact(name, out, x.view(b, h * w, ld)[..., :c].transpose(1, 2).float().reshape(b, c, h, w).contiguous(), log)   # widening is exact
    if h * w > 1:
        differs(name, out, x[:, :c].float().reshape(b, c, h, w))         # NHWC read as NCHW


@pytest.mark.parametrize("case", LAYOUT_CASES)
def test_layout_kernels_exact(case, metric_log):
    run_nchw_to_nhwc(case, False, metric_log)  # measured: 0 mismatches
    run_nhwc_to_nchw(case, False, metric_log)


# ---- the denoising state: ddim_init, ddim_step ---------------------------------------------------------------------------------------------
# (B, HW, L, ld, off)
DDIM_INIT_CASES = [(3, 1, 4, 8, 0), (3, 37, 4, 8, 4), (2, 37, 4, 72, 4), (1, WRAP // 4 + 50, 4, 8, 4)]


def run_ddim_init(case, contract, log):
    e = _eng()
    b, hw, L, ld, off = case
    if contract and hw > 10000:
        hw = WRAP_C // 4 + 50
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("ddim_init", *case))
    noise = (torch.randn(b, L, hw, 1, generator=g) * 1.5).to(d)
    name = f"ddim_init{case}{' contract' if contract else ''}"
    lat = sentinel(b * hw * ld, dt, d)
    sample = sentinel(b * hw * L, torch.float32, d)
    e.ddim_init(noise, lat, sample, b, hw, 1, L, ld, off, contract=contract)
    nh = noise.view(b, L, hw).transpose(1, 2).contiguous()                # [B,HW,L]
    check_exact(name + " sample", sample[:-GUARD].view(b, hw, L), nh, log)                         # the sample is the noise
    lv = lat[:-GUARD].view(b, hw, ld)
    check_exact(name + " latent", lv[..., off:off + L], nh.to(dt), log)                            # its copy: RNE16(noise)
    mask = torch.ones(ld, dtype=torch.bool, device=d)
    mask[off:off + L] = False
    assert_untouched(name, lv[..., mask])
    assert_untouched(name, lat[-GUARD:])
    assert_untouched(name, sample[-GUARD:])
    if hw > 1:
        differs(name, sample[:-GUARD].view(b, hw, L), noise.reshape(b, hw, L))   # NCHW read as NHWC
    # noise == nullptr: the sample is the widened channels [0, L) of the latent tensor, which is left alone
    g2 = torch.Generator().manual_seed(seed_of("ddim_init_lat", *case))
    lat2 = torch.randn(b * hw, ld, generator=g2).to(dt).to(d)
    keep = lat2.clone()
    sample2 = sentinel(b * hw * L, torch.float32, d)
    e.ddim_init(None, lat2, sample2, b, hw, 1, L, ld, off, contract=contract)
    check_exact(name + " from latent", sample2[:-GUARD].view(b * hw, L), keep[:, :L].float().contiguous(), log)
    assert torch.equal(ints(lat2), ints(keep)), f"{name}: the latent tensor changed"
    assert_untouched(name, sample2[-GUARD:])
    if off:
        differs(name, sample2[:-GUARD].view(b * hw, L), keep[:, off:off + L].float())   # channels [off, off + L) read instead


@pytest.mark.parametrize("case", DDIM_INIT_CASES)
def test_ddim_init_exact(case, metric_log):
    run_ddim_init(case, False, metric_log)  # measured: 0 mismatches


def ddim_coef(clip):
    """one v-prediction step at alpha_t = 0.6, alpha_prev = 0.81, as fp32 numbers (scheduler.py: step_coefficients)"""
    a, s = math.sqrt(0.6), math.sqrt(0.4)
    k = dict(x0_sample=a, x0_model=-s, eps_sample=s, eps_model=a, prev_x0=0.9, prev_eps=math.sqrt(1 - 0.81), clip=clip)
    return {n: float(np.float32(v)) for n, v in k.items()}


def ddim_ref_bound(m, s, k, swap=False, no_clip=False):
    """float64 step on the values the kernel reads (model m, sample s) and the bounds of x0 and of the new sample.
    swap / no_clip: the wrong variants (x0_model and eps_model exchanged; the clip left out)"""
    x0m, epm = (k["eps_model"], k["x0_model"]) if swap else (k["x0_model"], k["eps_model"])
    t1, t2 = k["x0_sample"] * s, x0m * m
    x0 = t1 + t2
    e_x0 = 3 * E24 * (t1.abs() + t2.abs())                                # x0: two v_mul and the v_add (or v_mul + v_fma), at sum |terms|
    if k["clip"] > 0 and not no_clip:
        x0 = x0.clamp(-k["clip"], k["clip"])                              # fminf / fmaxf: exact and 1-Lipschitz, the bound passes through
    t3, t4 = k["eps_sample"] * s, epm * m
    eps = t3 + t4
    e_eps = 3 * E24 * (t3.abs() + t4.abs())                               # eps: the same three roundings
    prev = k["prev_x0"] * x0 + k["prev_eps"] * eps
    e_prev = (abs(k["prev_x0"]) * e_x0 + abs(k["prev_eps"]) * e_eps       # the errors of x0 and eps carried through
              + 3 * E24 * (abs(k["prev_x0"]) * (x0.abs() + e_x0) + abs(k["prev_eps"]) * (eps.abs() + e_eps)))   # prev: three roundings at sum |terms|
    return x0, e_x0, prev, e_prev


# (pixels, L, ldm, ldu, ldx, off, clip, want x0_out): ldm != ldu != ldx
DDIM_STEP_CASES = [(3, 4, 8, 16, 12, 0, 0.0, True), (3 * 37, 4, 8, 16, 12, 4, 1.0, True), (37, 4, 12, 8, 4, 4, 1.0, False), (3 * 37, 4, 8, 72, 12, 0, 0.0, False),
                   (WRAP // 4 + 50, 4, 8, 16, 12, 4, 1.0, True)]


def run_ddim_step(case, contract, log):
    e = _eng()
    pixels, L, ldm, ldu, ldx, off, clip, want_x0 = case
    if contract and pixels > 10000:
        pixels = WRAP_C // 4 + 50
    d, dt = _dev(), elt(contract)
    k = ddim_coef(clip)
    g = torch.Generator().manual_seed(seed_of("ddim_step", *case))
    sample = (torch.randn(pixels, L, generator=g) * 1.5).to(d)
    uin = sentinel(pixels * ldu, dt, d)
    failures = []
    for step in range(2):   # the second step runs on the sample the first one left
        name = f"ddim_step{case}{' contract' if contract else ''} step {step}"
        model = torch.randn(pixels, ldm, generator=g).to(dt).to(d)
        x0_out = sentinel(pixels * ldx, dt, d) if want_x0 else None
        s_in = sample.clone()
        e.ddim_update(model, ldm, sample, uin, ldu, off, x0_out, ldx, pixels, L, k, contract=contract)
        m64, s64 = model[:, :L].double(), s_in.double()
        x0, e_x0, prev, e_prev = ddim_ref_bound(m64, s64, k)
        _, _, w_swap, _ = ddim_ref_bound(m64, s64, k, swap=True)
        check_f32(name + " sample", sample, prev, e_prev, log, failures, wrong=w_swap)           # measured: bf16 0.45, fp16 0.44, contract 0.41
        uv = uin[:-GUARD].view(pixels, ldu)
        check_exact(name + " unet input", uv[:, off:off + L], sample.to(dt), log)                  # RNE16 of the fp32 value stored in `sample` (fp32: the value)
        mask = torch.ones(ldu, dtype=torch.bool, device=d)
        mask[off:off + L] = False
        assert_untouched(name, uv[:, mask])
        assert_untouched(name, uin[-GUARD:])
        if want_x0:
            xv = x0_out[:-GUARD].view(pixels, ldx)
            wrong = ddim_ref_bound(m64, s64, k, no_clip=True)[0] if clip > 0 else ddim_ref_bound(m64, s64, k, swap=True)[0]
            check_out(name + " x0", xv[:, :L].contiguous(), x0, e_x0, log, failures, wrong=wrong)  # measured: bf16 / fp16 <= 1.00 (output rounding), contract <= 0.62
            assert_untouched(name, xv[:, L:])
            assert_untouched(name, x0_out[-GUARD:])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", DDIM_STEP_CASES)
def test_ddim_step_interval(case, metric_log):
    run_ddim_step(case, False, metric_log)


# ---- decode_epilogue: channel mean, clip, (x + 1) / 2, NHWC -> fp32 NCHW -------------------------------------------------------------------
# (B, HW, ld)
DECODE_CASES = [(3, 1, 4), (3, 37, 8), (2, 37, 64), (1, WRAP + 300, 4)]


def decode_ref_bound(c, mean3, raw, clip_first=False):
    """c float64 [B,HW,3] -> ([B,1|3,HW], E).  clip_first: the wrong variant that clips before the channel mean"""
    if mean3:
        cc = c.clamp(-1, 1) if clip_first else c
        t1 = cc[..., 0] + cc[..., 1]
        t2 = t1 + cc[..., 2]
        v = (t2 / 3.0)[:, None]
        err = (E24 * (t1.abs() + t2.abs()) / 3.0 + E24 * v[:, 0].abs())[:, None]   # two v_add, then the correctly rounded division by 3
    else:
        v = c.transpose(1, 2)
        err = torch.zeros_like(v)
    if raw:
        return v, err
    w = v.clamp(-1, 1) + 1.0                                                      # clip: exact; + 1: one rounding; * 0.5: exact
    return w * 0.5, 0.5 * (err + E24 * w.abs())


def run_decode_epilogue(case, contract, log):
    e = _eng()
    b, hw, ld = case
    if contract and hw > 10000:
        hw = WRAP_C + 300
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("decode", *case))
    x = (torch.randn(b * hw, ld, generator=g) * 0.9).to(dt).to(d)         # a third of the values beyond the clip
    c = x[:, :3].double().view(b, hw, 3)
    failures = []
    for mean3, raw in ((1, 0), (0, 0), (1, 1), (0, 1)) if hw < 10000 else ((1, 0),):
        nc = 1 if mean3 else 3
        buf = sentinel(b * nc * hw, torch.float32, d)
        e.decode_epilogue(x, b, hw, 1, ld, mean3, raw, buf, contract=contract)
        y64, err = decode_ref_bound(c, mean3, raw)
        wrong = decode_ref_bound(c, mean3, raw, clip_first=True)[0] if (mean3 and not raw) else None
        name = f"decode_epilogue{case} mean3={mean3} raw={raw}{' contract' if contract else ''}"
        check_f32(name, buf[:-GUARD].view(b, nc, hw), y64, err, log, failures, wrong=wrong)      # measured: bf16 0.67, fp16 0.87, contract 0.994 (E counts the roundings exactly)
        assert_untouched(name, buf[-GUARD:])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", DECODE_CASES)
def test_decode_epilogue_interval(case, metric_log):
    run_decode_epilogue(case, False, metric_log)


# ---- scale_pad, add, relu ------------------------------------------------------------------------------------------------------------------
# (pixels, C, ldi, ldo)
SCALE_PAD_CASES = [(3, 4, 8, 64), (3 * 37, 4, 12, 8), (37, 5, 5, 7), (WRAP // 8 + 7, 4, 4, 8)]


@pytest.mark.parametrize("case", SCALE_PAD_CASES)
def test_scale_pad_interval(case, metric_log):
    e = _eng()
    pixels, c, ldi, ldo = case
    d, dt = _dev(), e.act_dtype()
    g = torch.Generator().manual_seed(seed_of("scale_pad", *case))
    x = torch.randn(pixels, ldi, generator=g).to(dt).to(d)
    scale = float(np.float32(0.18215))
    buf = sentinel(pixels * ldo, dt, d)
    e.scale_pad(x, buf, pixels, c, ldi, ldo, scale)
    out = buf[:-GUARD].view(pixels, ldo)
    y64 = x[:, :c].double() * scale
    failures = []
    gate(f"scale_pad{case}", out[:, :c].contiguous(), y64, E24 * y64.abs(), metric_log, failures,   # one v_mul at |result|; measured: <= 1.00 (output rounding)
         wrong=x[:, :c].double() / scale)                                  # wrong variant: divided by the scaling factor
    assert float(out[:, c:].float().abs().max() if ldo > c else 0.0) == 0.0, "columns [C, ldo) must be zero"
    assert_untouched("scale_pad", buf[-GUARD:])
    assert not failures, "\n".join(failures)


ADD_CASES = [8, 3 * 37 * 8, WRAP * 8 + 64]   # elements (vectors of 8; the contract form: of 4)


def run_add(n, contract, log):
    e = _eng()
    if contract and n > 10000:
        n = WRAP_C * 4 + 64
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("add", n))
    a = torch.randn(n, generator=g).to(dt).to(d)
    b = (torch.randn(n, generator=g) * 3).to(dt).to(d)
    out = e.add(a, b, contract=contract)
    y64 = a.double() + b.double()
    name = f"add[{n}{' contract' if contract else ''}]"
    if contract:
        check_exact(name, out, y64.float(), log)                         # one fp32 add: RN32 of the exact sum (float64 holds it exactly)
        differs(name, out, a - b)
    else:
        failures = []
        gate(name, out, y64, E24 * y64.abs(), log, failures, wrong=a.double() - b.double())   # the fp32 v_add at |result|; measured: <= 1.00 (output rounding)
        assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", ADD_CASES)
def test_add_interval(n, metric_log):
    run_add(n, False, metric_log)


@pytest.mark.parametrize("n", ADD_CASES)
def test_relu_exact(n, metric_log):
    e = _eng()
    d, dt = _dev(), e.act_dtype()
    g = torch.Generator().manual_seed(seed_of("relu", n))
    x = torch.randn(n, generator=g)
    tiny = 2.0 ** -133 if dt == torch.bfloat16 else 2.0 ** -24           # the smallest subnormal
    x[:8] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), tiny, -tiny, 3 * tiny, -3 * tiny])
    x = x.to(dt)
    want = torch.where(x.float() > 0, x, torch.zeros_like(x)).to(d)      # (on the CPU: subnormals kept)
    out = e.relu(x.to(d))
    check_exact(f"relu[{n}]", out, want, metric_log)                     # compared by value: -0 and +0 are one value; measured: 0 mismatches
    differs("relu", out, x.to(d))


# ---- pointwise_small (post_quant_conv), dpt_final ------------------------------------------------------------------------------------------
# (pixels, Cin, Cout, ldi, ldo, bias)
POINTWISE_CASES = [(3, 4, 4, 8, 64, True), (3 * 37, 4, 4, 12, 8, True), (37, 8, 8, 8, 8, False), (37, 1, 3, 5, 7, True), (WRAP + 300, 4, 4, 8, 8, True)]


def run_pointwise_small(case, contract, log):
    e = _eng()
    pixels, cin, cout, ldi, ldo, with_bias = case
    if contract and pixels > 10000:
        pixels = WRAP_C + 300
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("pointwise", *case))
    x = torch.randn(pixels, ldi, generator=g).to(dt).to(d)
    w = (torch.randn(cout, cin, generator=g) / math.sqrt(cin)).to(d)
    bias = (0.5 * torch.randn(cout, generator=g)).to(d) if with_bias else None
    s = float(np.float32(-1.0 / 0.18215))
    buf = sentinel(pixels * ldo, dt, d)
    e.pointwise_small(x, buf, w, bias, pixels, ldi, ldo, s, contract=contract)
    out = buf[:-GUARD].view(pixels, ldo)
    xs = x[:, :cin].double() * s
    b64 = bias.double() if with_bias else torch.zeros(cout, dtype=torch.float64, device=d)
    y64 = xs @ w.double().t() + b64
    mag = xs.abs() @ w.double().abs().t() + b64.abs()
    err = (cin + 2) * E24 * mag                                           # v_mul by in_scale, then Cin v_fma onto the bias (a += w * x is contracted): (terms + 1) roundings at sum |w x| + |bias|, one more for in_scale
    wrong = (x[:, :cin].double() @ w.double().t() + b64) * s if with_bias else x[:, :cin].double() @ w.double().t()   # in_scale applied after the weights (and the bias) / not at all
    name = f"pointwise_small{case}{' contract' if contract else ''}"
    failures = []
    check_out(name, out[:, :cout].contiguous(), y64, err, log, failures, wrong=wrong)   # measured: 16-bit <= 1.00 (output rounding), contract <= 0.53
    assert float(out[:, cout:].float().abs().max() if ldo > cout else 0.0) == 0.0, "columns [Cout, ldo) must be zero"
    assert_untouched(name, buf[-GUARD:])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", POINTWISE_CASES)
def test_pointwise_small_interval(case, metric_log):
    run_pointwise_small(case, False, metric_log)


# (B, HW, Cin)
DPT_FINAL_CASES = [(3, 1, 32), (3, 37, 32), (2, 37, 8), (1, WRAP + 300, 32)]


def run_dpt_final(case, contract, log):
    e = _eng()
    b, hw, cin = case
    if contract and hw > 10000:
        hw = WRAP_C + 300
    d, dt = _dev(), elt(contract)
    g = torch.Generator().manual_seed(seed_of("dpt_final", *case))
    x = torch.randn(b, hw, cin, generator=g).abs().to(dt).to(d)          # (the producing conv applies ReLU)
    w = (torch.randn(cin, generator=g) / math.sqrt(cin)).to(d)
    bias = float(np.float32(0.37))
    out = e.dpt_final(x, w, bias, contract=contract)
    y64 = x.double() @ w.double() + bias
    err = (cin + 1) * E24 * (x.double().abs() @ w.double().abs() + abs(bias))   # Cin v_fma onto the bias (a += x * w is contracted): (terms + 1) roundings at sum |w x| + |bias|
    failures = []
    check_f32(f"dpt_final{case}{' contract' if contract else ''}", out, y64, err, log, failures,   # measured: bf16 0.12, fp16 0.10, contract 0.13
              wrong=x.double() @ w.double().flip(0) + bias)                # wrong variant: the channels in reverse order
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", DPT_FINAL_CASES)
def test_dpt_final_interval(case, metric_log):
    run_dpt_final(case, False, metric_log)


# ---- minmax_norm: per image (x - min) / (max - min) ------------------------------------------------------------------------------------------
# (B, n): n = 1 (every image constant: NaN, Appendix B.13), one value per thread, 16385, and more than one pass of the apply kernel's 64-block
# partial pass (64 * 256 * 4)
MINMAX_CASES = [(3, 1), (3, 255), (3, 16385), (2, 64 * 256 * 4 + 77), (1, WRAP + 300)]


def minmax_inputs(case):
    """images with different ranges; in the B = 3 cases with n > 1 image 1 is constant"""
    b, n = case
    g = torch.Generator().manual_seed(seed_of("minmax", *case))
    x = torch.randn(b, n, generator=g) * (1 + 3 * torch.arange(b).float().view(b, 1)) + 5 * torch.arange(b).float().view(b, 1)
    if b == 3 and n > 1:
        x[1] = 0.75
    return x


def minmax_ref_bound(x64, per_batch=False):
    mn = x64.min() if per_batch else x64.min(dim=1, keepdim=True).values   # min and max of fp32 numbers: exact
    mx = x64.max() if per_batch else x64.max(dim=1, keepdim=True).values
    y = (x64 - mn) / (mx - mn)                                             # 0 / 0 = NaN for a constant image
    return y, 3.01 * E24 * y.abs()                                         # v_sub (x - min), v_sub (max - min), the correctly rounded division: three relative roundings


@pytest.mark.parametrize("case", MINMAX_CASES)
def test_minmax_norm_interval(case, metric_log):
    e = _eng()
    x = minmax_inputs(case).to(_dev())
    out = e.minmax_norm(x)
    y64, err = minmax_ref_bound(x.double())
    if case[0] == 3 and case[1] > 1:
        assert bool(torch.isnan(out[1]).all()) and not bool(torch.isnan(out[0]).any() | torch.isnan(out[2]).any()), "the constant image alone is NaN"
    failures = []
    check_f32(f"minmax_norm{case}", out, y64, err, metric_log, failures,   # measured: 0.93 (both libraries: E counts the three roundings exactly)
              wrong=minmax_ref_bound(x.double(), per_batch=True)[0].nan_to_num(7.0) if case[0] > 1 and case[1] > 1 else None)   # min-max over the batch
    assert not failures, "\n".join(failures)
