"""Kernel-level tests of the contract precision (gp_set_precision(GP_PREC_CONTRACT), csrc/contract.hip): every kernel between and inside the
split-bf16 matrix products, called through the gp_c_* test entry points, against a float64 reference computed on the exact fp32 values the
kernel reads.

Error model (csrc/contract.hip header): x = hi + lo, hi = bf16(x), lo = bf16(x - hi), so |x - hi - lo| <= 2^-17 |x|; a product keeps
hi.hi + lo.hi + hi.lo and drops lo.lo (<= 2^-18 |a w|), so the operand error is <= 3 * 2^-16 |a w| per product; the MFMA accumulates in fp32.
Gates derived from it:
  * products        |y - y64| <= 2^-14 sum_k |a_k w_k| + 2^-22 |y64|
  * GroupNorm       |y - y64| <= 2^-15 (|y64| + |beta|) + 8 * 2^-24 (|mean| / std) |gamma|   (the second term: the x * scale + shift form on fp32
                    data rounds x * scale, the shift and their sum at the magnitude of mean / std); scale and shift themselves:
                    |scale - scale64| <= (2^-19 + 2^-26 r) |scale64|, r = |mean| / std (the row means carry the fp32 rounding of the row
                    sums, a few eps |mean|, and Chan's cross term 2 sum_k n_k (m_k - mean) dm_k turns that into ~ eps r / 4 of the variance: the
                    first measurement, 0.94 of a plain 2^-19 gate at r = 895, showed the term), |shift - shift64| <= 2^-19 |beta| +
                    |gamma| (r (2^-19 + 2^-26 r) + 16 * 2^-24 (1 + r)) (shift = beta - mean * scale carries the scale's relative error at r |gamma|)
  * LayerNorm       |y - y64| <= 2^-15 (|y64| + |beta|) + 2^-20 (1 + |mean| / std) |gamma|
  * softmax         |p - p64| <= 2^-16 p64 (+ 2^-40): the exponent's argument is rounded at |x - max| <= 30, 2^-19 relative
Every test also evaluates the nearest WRONG variant on the CPU (hi-only operands, a product without its lo.hi or its hi.lo term, a truncated lo,
single-pass GroupNorm statistics) and asserts that the gate is at least 8x below that variant's error: a gate that cannot tell the variants
apart tests nothing.  The measured values are in the comments next to each gate."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

E14, E15, E16, E19, E22, E24 = 2.0 ** -14, 2.0 ** -15, 2.0 ** -16, 2.0 ** -19, 2.0 ** -22, 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def e():
    from genpercept_amd import engine
    engine.set_default_precision("bf16")
    if engine.act_dtype() != torch.bfloat16:
        pytest.skip("the contract precision lives in the bf16 library")
    return engine


def hi_lo(x):
    """the split of fp32 x: (hi, lo) as fp32 values, both rounded to nearest even"""
    hi = x.float().to(torch.bfloat16).float()
    return hi, (x.float() - hi).to(torch.bfloat16).float()


def unsplit(s, c):
    """value hi + lo of an A-order split operand [..., 3c] (checks the order [hi | lo | hi] on the way)"""
    assert torch.equal(s[..., :c], s[..., 2 * c:]), "A order is [hi | lo | hi]"
    return s[..., :c].double() + s[..., c:2 * c].double()


def gate_ratio(err, bound):
    return float((err / bound).max())


# ---- the split itself: bit-exact -------------------------------------------------------------------------------------------------------------
def _trunc_bf16(x):
    return (x.float().view(torch.int32) & ~0xFFFF).view(torch.float32)


@pytest.mark.parametrize("rows,c,ld", [(1, 8, 8), (7, 64, 68), (1000, 320, 320), (4097, 72, 76)])
@pytest.mark.parametrize("b_order", [0, 1])
def test_split_is_round_to_nearest_even_in_both_orders(e, rows, c, ld, b_order, metric_log):
    g = torch.Generator().manual_seed(rows + c + b_order)
    x = torch.randn(rows, ld, generator=g) * torch.exp(4 * torch.randn(rows, ld, generator=g))
    edge = torch.tensor([0.0, -0.0, 3.38e38, -3.38e38, 3.3e38, 1e-39, -3e-40, 1.4e-45, -1.4e-45, 1.17549435e-38, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9])
    flat = x.view(-1)
    flat[: min(edge.numel(), flat.numel())] = edge[: flat.numel()]
    d = _dev()
    for act, scale in (("none", 1.0), ("none", 0.5), ("relu", 0.125)):
        v = x[:, :c] * scale
        if act == "relu":
            v = v.clamp_min(0.0)
        out = e.c_split3(x.to(d)[:, :c], b_order=bool(b_order), act=act, scale=scale).cpu()  # (row stride ld)
        hi = v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        want = torch.cat([hi, hi, lo] if b_order else [hi, lo, hi], dim=1)
        same = out.view(torch.int16) == want.view(torch.int16)
        if act == "relu":  # (fmaxf(-0, 0) may keep the sign of the zero: value equality there; measured: 2-4 signed-zero differences per case)
            same = out.float() == want.float()
        metric_log(f"c_split3[{rows}x{c} ld {ld} {'B' if b_order else 'A'} {act} {scale}]", mismatches=int((~same).sum()))
        assert bool(same.all()), f"{int((~same).sum())} elements differ from RNE hi / lo"  # measured: 0 (bit-exact, subnormals included)
        # discriminator: a lo made by truncation differs in a sizeable fraction of the elements
        lo_t = _trunc_bf16(v - hi.float()).to(torch.bfloat16)
        frac = float((lo_t.view(torch.int16) != lo.view(torch.int16)).float().mean())
        assert frac >= 0.2 or rows * c < 64, frac


# ---- split products: every kernel the contract conv / linear launches ------------------------------------------------------------------------
def _coherent(shape, g, lo_sign=1.0):
    """positive values whose lo parts are all positive (x = hi (1 + u 2^-9), u in [0.25, 0.75]): the dropped-term errors add up instead of
    cancelling, the hardest case for the gate and the one that separates the wrong variants"""
    hi = (0.25 + torch.rand(shape, generator=g)).to(torch.bfloat16).float()
    return hi * (1.0 + lo_sign * (0.25 + 0.5 * torch.rand(shape, generator=g)) * 2.0 ** -9)


# (name, B, H, W, Cin, Cout, ks, stride, ups, tile, dbg, act, residual, expected path) -- path (igemm_path): 1 halo 16-row tiles, 2 halo phases,
# 3 persistent GEMM, 4 conv_img + split-K reduce, 5 split-K igemm + reduce, 6 igemm, 7 halo 12-row tiles.  The residual is signed (randn), so
# ReLU and SiLU act on both signs.  The contract linears run on the generic igemm (the persistent GEMM has no fp32
# epilogue), so path 3 is not among them.
PRODUCT_CASES = [
    ("halo3_16row", 1, 40, 36, 320, 320, 3, 1, 0, 5, 2 << 20, "none", True, 1),
    ("halo3_12row", 2, 24, 40, 128, 192, 3, 1, 0, 5, 1 << 20, "none", False, 7),
    ("halo3_silu_residual", 1, 24, 24, 128, 128, 3, 1, 0, 5, 2 << 20, "silu", True, 1),
    ("halo_phases_x2", 1, 20, 24, 320, 320, 3, 1, 1, 5, 0, "none", False, 2),
    ("conv_img_24", 1, 24, 24, 1280, 1280, 3, 1, 0, 0, 0, "none", True, 4),
    ("conv_img_12_k23040", 4, 12, 12, 2560, 320, 3, 1, 0, 0, 0, "none", True, 4),  # (12^2: four images per 576-pixel tile)
    ("splitk_igemm_k23040", 1, 12, 12, 2560, 1280, 3, 1, 0, 0, 0, "none", False, 5),
    ("splitk_igemm_stride2_ragged", 2, 33, 31, 320, 200, 3, 2, 0, 0, 0, "none", False, 5),
    ("igemm_stride2_ragged", 2, 33, 31, 320, 200, 3, 2, 0, 1, 0, "none", False, 6),
    ("igemm_linear", 1, 64, 64, 640, 640, 1, 1, 0, 0, 0, "none", True, 6),
    ("igemm_linear_geglu", 1, 32, 32, 320, 2560, 1, 1, 0, 0, 0, "geglu", False, 6),
    ("igemm_linear_inplace_residual", 2, 32, 32, 1280, 1280, 1, 1, 0, 0, 0, "none", "inplace", 6),
    ("igemm_linear_relu_residual", 1, 32, 32, 320, 320, 1, 1, 0, 0, 0, "relu", True, 6),
]


def _conv64(x, w, bias, stride, ups):
    """float64 NCHW conv with the engine's padding conventions (stride 2: diffusers' Downsample2D pads right / bottom only)"""
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if w.shape[-1] == 1:
        return F.conv2d(x, w, bias)
    if stride == 2:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    return F.conv2d(x, w, bias, padding=1)


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=[c[0] for c in PRODUCT_CASES])
def test_split_products_keep_all_three_terms(e, case, metric_log, monkeypatch):
    name, b, h, w, cin, cout, ks, stride, ups, tile, dbg, act, with_res, want_path = case
    monkeypatch.setenv("GENPERCEPT_IGEMM_DBG", str(dbg))
    g = torch.Generator().manual_seed(cin * 7 + cout + h)
    x = _coherent((b, cin, h, w), g)
    wt = _coherent((cout, cin, ks, ks), g) * 2.0 ** -math.ceil(math.log2(cin * ks * ks))  # (a power of two keeps the lo parts coherent)
    bias = torch.rand(cout, generator=g)
    bias_dev = bias
    if act == "geglu":  # the bias in the packed row order (gp_pack_weight(geglu=1)): per 32-row block, value j at 8 (j % 16 // 4) + j % 4, gate + 4
        idx = torch.arange(cout)
        r = torch.where(idx >= cout // 2, idx - cout // 2, idx)
        bias_dev = torch.empty_like(bias)
        bias_dev[(r // 16) * 32 + ((r % 16) // 4) * 8 + (idx >= cout // 2).long() * 4 + (r % 4)] = bias
    d = _dev()
    xs = e.c_split3(x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(d)).view(b, h, w, 3 * cin)
    wp = e.pack_weight_split(wt, geglu=act == "geglu", device=d)
    wph = e.pack_weight_phases_split(wt, device=d) if ups else None
    ho = (h + 1 - 3) // 2 + 1 if stride == 2 else (2 * h if ups else h)
    wo = (w + 1 - 3) // 2 + 1 if stride == 2 else (2 * w if ups else w)
    nout = cout // 2 if act == "geglu" else cout
    res = torch.randn(b, ho, wo, nout, generator=g) if with_res else None
    res_d = res.to(d) if with_res else None
    y, path, _, _ = e.c_conv2d(xs, wp, bias_dev.to(d), cout, ks, stride=stride, pad=(0, 0) if stride == 2 else (1, 1), out_hw=(ho, wo), ups=bool(ups),
                               w_phases=wph, residual=res_d, act=act, tile=tile, out=res_d if with_res == "inplace" else None)
    y = y.cpu().double()
    assert path == want_path, f"{name}: kernel path {path}, expected {want_path}"
    # float64 references on the exact fp32 operands, and the CPU wrong variants
    x64, w64, b64 = x.double(), wt.double(), bias.double()
    xh, xl = (t.double() for t in hi_lo(x))
    wh, wl = (t.double() for t in hi_lo(wt))
    conv = lambda a, k, bb: _conv64(a, k, bb, stride, ups).permute(0, 2, 3, 1)
    z64 = conv(x64, w64, b64)
    zabs = conv(x64.abs(), w64.abs(), b64.abs())
    zhh = conv(xh, wh, b64)
    variants = {"hi only": zhh, "no lo.hi": zhh + conv(xh, wl, None), "no hi.lo": zhh + conv(xl, wh, None)}
    if act == "geglu":
        def gg(z):
            return z[..., :nout] * F.gelu(z[..., nout:])  # diffusers GEGLU: hidden, gate = proj(x).chunk(2)
        # GEGLU of a product pair: |d(a gelu(g))| <= |gelu(g)| da + 1.13 |a| dg
        bound = E14 * (F.gelu(z64[..., nout:]).abs() * zabs[..., :nout] + 1.13 * z64[..., :nout].abs() * zabs[..., nout:]) + E22 * gg(z64).abs() + 1e-30
        ref = gg(z64)
        variants = {k: gg(v) for k, v in variants.items()}
    else:
        ref = z64
        bound = E14 * (zabs + (res.double().abs() if with_res else 0.0)) + E22 * z64.abs()
    if with_res:
        ref = ref + res.double()
        variants = {k: v + res.double() for k, v in variants.items()}
    if act in ("silu", "relu"):  # applied after the residual, as the epilogue does; |act'| <= 1.1
        fa = F.silu if act == "silu" else F.relu
        ref, variants, bound = fa(ref), {k: fa(v) for k, v in variants.items()}, bound * 1.1
    err = (y - ref).abs()
    r = gate_ratio(err, bound)
    rv = {k: gate_ratio((v - ref).abs(), bound) for k, v in variants.items()}
    metric_log(f"c_conv[{name}]", path=path, gate_ratio=r, rel_max=float(err.max() / ref.abs().max()), **{f"wrong[{k}]": v for k, v in rv.items()})
    assert torch.isfinite(y).all() and r <= 1.0, (name, r)  # measured: <= 0.062 of the gate over all cases
    for k, v in rv.items():  # measured: hi only >= 25x, no lo.hi >= 12.9x, no hi.lo >= 12.4x (GEGLU the lowest)
        assert v >= 8.0, f"{name}: the gate does not separate the '{k}' variant ({v:.2f}x)"


# ---- GroupNorm: centred statistics -----------------------------------------------------------------------------------------------------------
def _gn_input(b, hw, c, groups, ratio, g):
    """unit-spread data; every channel of a group shares an offset of `ratio` standard deviations (random sign per group and image)"""
    x = torch.randn(b, hw, c, generator=g) * (0.5 + torch.rand(c, generator=g))
    off = ratio * torch.sign(torch.randn(b, 1, groups, generator=g)) * (1.0 + torch.rand(b, 1, groups, generator=g))
    return (x + off.repeat_interleave(c // groups, dim=2)).float()


def _gn64(x, groups, eps, gamma, beta):
    b, hw, c = x.shape
    xg = x.double().view(b, hw, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = (rstd.expand(b, 1, groups, c // groups).reshape(b, c)) * gamma.double()
    mean_c = mean.expand(b, 1, groups, c // groups).reshape(b, c)
    shift = beta.double() - mean_c * scale
    ratio_c = (mean_c.abs() * rstd.expand(b, 1, groups, c // groups).reshape(b, c))
    y = (x.double() - mean_c[:, None]) * scale[:, None] + beta.double()
    return y, scale, shift, ratio_c


def _gn_single_pass_f32(x, groups, eps, gamma, beta):
    """the wrong variant: the fp32 single-pass {sum, sum of squares} row partials the statistics pass used to write (same rows as
    c_gn_stat_rows, per-thread sequential sums), finalised with qk - sk mk"""
    b, hw, c = x.shape
    bm = max(8, min(1024, 16384 // c * 4, hw))
    xs = x.numpy().astype(np.float32)
    scale = np.zeros((b, c), np.float64)
    shift = np.zeros((b, c), np.float64)
    for bi in range(b):
        sk, qk, nk = [], [], []
        for p0 in range(0, hw, bm):
            rows = xs[bi, p0:p0 + bm]
            s = np.zeros(c, np.float32)
            q = np.zeros(c, np.float32)
            for r in rows:
                s += r
                q += r * r
            sk.append(s); qk.append(q); nk.append(np.float32(len(rows)))
        sk, qk, nk = np.array(sk), np.array(qk), np.array(nk)[:, None]
        cpg = c // groups
        for gi in range(groups):
            sl = slice(gi * cpg, (gi + 1) * cpg)
            n_all = np.float32(hw * cpg)
            mean = np.float32(sk[:, sl].sum(dtype=np.float32) / n_all)
            mk = (sk[:, sl] / nk).astype(np.float32)
            m2 = (np.maximum(qk[:, sl] - sk[:, sl] * mk, 0) + nk * (mk - mean) ** 2).sum(dtype=np.float32)
            rstd = np.float32(1.0 / np.sqrt(np.float32(m2 / n_all) + np.float32(eps)))
            scale[bi, sl] = rstd * gamma.numpy()[sl]
            shift[bi, sl] = beta.numpy()[sl] - mean * scale[bi, sl]
    return torch.from_numpy(scale), torch.from_numpy(shift)


def _gn_scale_shift_bounds(sc64, ratio_c, ga, be):
    rel_sc = E19 + 2.0 ** -26 * ratio_c
    # (the mean's own rounding is relative to E|x| <= |mean| + std, hence 1 + r: at r = 0 a plain 16 * 2^-24 r |gamma| term left the shift
    # gate at 0.90 with only |beta| to carry it)
    return rel_sc * sc64.abs(), E19 * be + ga * (ratio_c * rel_sc + 16 * E24 * (1 + ratio_c)) + 1e-30


def _gn_gates(y, sc, sh, x, groups, eps, gamma, beta, silu, wrong, name, log):
    y64, sc64, sh64, ratio_c = _gn64(x, groups, eps, gamma, beta)
    ga, be = gamma.double().abs(), beta.double().abs()
    # per element (SiLU: |silu'| <= 1.1 on the pre-activation error)
    bound_y = E15 * (y64.abs() + be) + 8 * E24 * ratio_c[:, None] * ga
    ref = F.silu(y64) if silu else y64
    r_y = gate_ratio((y - ref).abs(), bound_y * (1.1 if silu else 1.0))
    bound_sc, bound_sh = _gn_scale_shift_bounds(sc64, ratio_c, ga, be)
    r_sc = gate_ratio((sc.double() - sc64).abs(), bound_sc)
    r_sh = gate_ratio((sh.double() - sh64).abs(), bound_sh)
    wsc, wsh = wrong
    rw_sc, rw_sh = gate_ratio((wsc - sc64).abs(), bound_sc), gate_ratio((wsh - sh64).abs(), bound_sh)
    y_wrong = (x.double() * wsc[:, None] + wsh[:, None])
    rw_y = gate_ratio((y_wrong - y64).abs(), bound_y)
    log(name, gate_ratio_y=r_y, gate_ratio_scale=r_sc, gate_ratio_shift=r_sh, wrong_single_pass_scale=rw_sc, wrong_single_pass_shift=rw_sh,
        wrong_single_pass_y=rw_y, max_ratio=float(ratio_c.max()))
    assert r_y <= 1.0 and r_sc <= 1.0 and r_sh <= 1.0, (name, r_y, r_sc, r_sh)  # measured: y <= 0.39, scale <= 0.16, shift <= 0.15
    return rw_sc, rw_sh, rw_y


# (B, HW, C, mean / std, silu): C = 64 rows are 1024 pixels (below, at, above with a short last row), C = 320 rows 204 pixels (96^2 latents)
GN_CASES = [(2, 900, 64, 0, False), (1, 1024, 64, 100, True), (2, 2500, 64, 300, False), (1, 9216, 320, 0, True), (1, 9216, 320, 100, False),
            (2, 9216, 320, 300, False)]


@pytest.mark.parametrize("case", GN_CASES)
def test_groupnorm_statistics_pass_large_mean(e, case, metric_log):
    b, hw, c, ratio, silu = case
    groups, eps = 32, 1e-6
    g = torch.Generator().manual_seed(hw + c + ratio)
    x = _gn_input(b, hw, c, groups, ratio, g)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.5 * torch.randn(c, generator=g)
    d = _dev()
    out, sc, sh = e.c_groupnorm_split(x.view(b, hw, 1, c).to(d), gamma.to(d), beta.to(d), groups, eps, silu)
    y = unsplit(out.cpu().view(b, hw, 3 * c), c)
    wrong = _gn_single_pass_f32(x, groups, eps, gamma, beta)
    rw_sc, rw_sh, rw_y = _gn_gates(y, sc.cpu(), sh.cpu(), x, groups, eps, gamma, beta, silu, wrong, f"c_groupnorm{case}", metric_log)
    if ratio >= 100:  # the single-pass statistics (a CPU emulation, not the old kernel's summation order) fail the element gate and sit >= 8x above the scale / shift gates
        assert rw_y > 1.0 and max(rw_sc, rw_sh) >= 8.0, (rw_y, rw_sc, rw_sh)  # measured: y 13x - 1900x, scale 138x - 18000x


@pytest.mark.parametrize("case", [(1, 48, 48, 320, 320, 3, 100), (2, 32, 32, 640, 640, 1, 300), (1, 24, 24, 640, 640, 3, 0)])
def test_groupnorm_statistics_of_a_contract_conv_output(e, case, metric_log):
    """the GroupNorm after a contract conv (ResnetBlock2D: conv1 -> norm2) with a group-constant offset carried by the conv's bias"""
    b, h, w, cin, cout, ks, ratio = case
    groups, eps = 32, 1e-6
    g = torch.Generator().manual_seed(cin + h + ratio)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) / math.sqrt(cin * ks * ks)
    bias = (ratio * torch.sign(torch.randn(groups, generator=g))).repeat_interleave(cout // groups) + 0.1 * torch.randn(cout, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(cout, generator=g), 0.5 * torch.randn(cout, generator=g)
    d = _dev()
    xs = e.c_split3(x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().to(d)).view(b, h, w, 3 * cin)
    y, _, sc, sh = e.c_conv2d(xs, e.pack_weight_split(wt, device=d), bias.to(d), cout, ks, gn=(gamma.to(d), beta.to(d), groups, eps))
    yc = y.cpu().view(b, h * w, cout)  # the exact fp32 tensor the statistics pass read
    _, sc64, sh64, ratio_c = _gn64(yc, groups, eps, gamma, beta)
    bound_sc, bound_sh = _gn_scale_shift_bounds(sc64, ratio_c, gamma.double().abs(), beta.double().abs())
    r_sc, r_sh = gate_ratio((sc.cpu().double() - sc64).abs(), bound_sc), gate_ratio((sh.cpu().double() - sh64).abs(), bound_sh)
    wsc, wsh = _gn_single_pass_f32(yc, groups, eps, gamma, beta)
    rw = max(gate_ratio((wsc - sc64).abs(), bound_sc), gate_ratio((wsh - sh64).abs(), bound_sh))
    metric_log(f"c_conv_gn{case}", gate_ratio_scale=r_sc, gate_ratio_shift=r_sh, wrong_single_pass=rw, max_ratio=float(ratio_c.max()))
    assert r_sc <= 1.0 and r_sh <= 1.0, (r_sc, r_sh)  # measured: scale <= 0.14, shift <= 0.13 (r >= 100)
    if ratio >= 100:
        assert rw >= 8.0, rw  # measured: 146x (r = 100), 396x (r = 300)


# ---- LayerNorm and softmax -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c,offset", [(1, 320, 0.0), (333, 640, 10.0), (1024, 1280, 3.0), (5, 2048, 30.0)])
def test_layernorm_split(e, rows, c, offset, metric_log):
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows, c, generator=g) + offset * torch.randn(rows, 1, generator=g)).float()
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.5 * torch.randn(c, generator=g)
    out = e.c_layernorm_split(x.to(_dev()), gamma.to(_dev()), beta.to(_dev())).cpu()
    y = unsplit(out, c)
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    y64 = (x64 - mean) / torch.sqrt(((x64 - mean) ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    std = ((x64 - mean) ** 2).mean(1, keepdim=True).sqrt()
    bound = E15 * (y64.abs() + beta.double().abs()) + 2.0 ** -20 * gamma.double().abs() * (1 + mean.abs() / std)
    r = gate_ratio((y - y64).abs(), bound)
    rw = gate_ratio((out[:, :c].double() - y64).abs(), bound)  # wrong variant: the hi part alone
    metric_log(f"c_layernorm[{rows}x{c} off {offset}]", gate_ratio=r, wrong_hi_only=rw)
    assert r <= 1.0 and rw >= 8.0, (r, rw)  # measured: <= 0.24; hi only >= 95x


@pytest.mark.parametrize("rows,t", [(3, 77), (64, 4096), (4, 16384), (3, 20000), (2, 36864)])
def test_softmax_split(e, rows, t, metric_log):
    ld = (t + 3) // 4 * 4
    g = torch.Generator().manual_seed(t)
    x = torch.full((rows, ld), float("nan"))
    x[:, :t] = torch.rand(rows, t, generator=g) * 240.0  # scale 1/8: logits spread over 30 units
    out = e.c_softmax_split(x.to(_dev()), t, 0.125).cpu()
    p = unsplit(out, ld)
    p64 = torch.softmax(x[:, :t].double() * 0.125, dim=1)
    assert bool((p[:, t:] == 0).all()), "columns beyond T must be zero"
    bound = E16 * p64 + 2.0 ** -40
    r = gate_ratio((p[:, :t] - p64).abs(), bound)
    rw = gate_ratio((out[:, :t].double() - p64).abs(), bound)
    metric_log(f"c_softmax[{rows}x{t}]", gate_ratio=r, wrong_hi_only=rw, kernel="long" if ld > 16384 else "register")
    assert r <= 1.0 and rw >= 8.0, (r, rw)  # measured: <= 0.51 (both kernels); hi only >= 242x
