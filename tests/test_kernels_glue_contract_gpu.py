"""Float64 and bit-exact tests of the contract precision's glue kernels (bf16 library) through their stateless test entries.

c_rgb_split (csrc/contract.hip) and the float instantiations of csrc/elementwise.hip's templates (concat, nchw_f32_to_nhwc, nhwc_to_nchw_f32,
ddim_init, ddim_step, decode_epilogue, pointwise_small, add, dpt_final) run the checks of tests/test_kernels_glue_gpu.py with fp32 storage:
the same references and bounds, |out - y64| <= E in place of the 16-bit interval, one case per kernel that wraps the fp32 grid cap's
8192 * 256 items.  Tested here: the kernels that exist in this precision only, c_heads_split and c_heads_merge_split (bit-exact RNE hi / lo
in the right order and position, as test_split_is_round_to_nearest_even_in_both_orders), c_cross_fold and c_cross_attn_small, and the float
form of bilinear through its own entry gp_c_bilinear (float64 bounds).  A split operand
x = hi + lo carries 2^-17 |x| (tests/test_contract_kernels_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import test_kernels_glue_gpu as glue
from test_contract_kernels_gpu import unsplit
from test_kernels_glue_gpu import GUARD, WRAP_C, assert_untouched, check_f32, differs, sentinel
from test_kernels_exact_gpu import _dev, check_exact
from test_kernels_interval_gpu import E24, cross_inputs, cross_ref_bound, fold_inputs, fold_ref_bound, seed_of

pytestmark = pytest.mark.gpu

E15, E17 = 2.0 ** -15, 2.0 ** -17


@pytest.fixture(autouse=True)
def e():
    from genpercept_amd import engine
    engine.set_default_precision("bf16")
    return engine


# ---- the fp32 forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", glue.RGB_CASES)
def test_c_rgb_split_exact(case, u8, metric_log):
    glue.run_rgb_prologue(case, u8, True, metric_log)  # measured: 0 mismatches


@pytest.mark.parametrize("case", glue.CONCAT_CASES)
def test_c_concat_exact(case, metric_log):
    glue.run_concat(case, True, metric_log)  # measured: 0 mismatches


@pytest.mark.parametrize("case", glue.LAYOUT_CASES)
def test_c_layout_kernels_exact(case, metric_log):
    glue.run_nchw_to_nhwc(case, True, metric_log)  # measured: 0 mismatches
    glue.run_nhwc_to_nchw(case, True, metric_log)


@pytest.mark.parametrize("case", glue.DDIM_INIT_CASES)
def test_c_ddim_init_exact(case, metric_log):
    glue.run_ddim_init(case, True, metric_log)  # measured: 0 mismatches


@pytest.mark.parametrize("case", glue.DDIM_STEP_CASES)
def test_c_ddim_step_interval(case, metric_log):
    glue.run_ddim_step(case, True, metric_log)


@pytest.mark.parametrize("case", glue.DECODE_CASES)
def test_c_decode_epilogue_interval(case, metric_log):
    glue.run_decode_epilogue(case, True, metric_log)


@pytest.mark.parametrize("case", glue.POINTWISE_CASES)
def test_c_pointwise_small_interval(case, metric_log):
    glue.run_pointwise_small(case, True, metric_log)


@pytest.mark.parametrize("n", glue.ADD_CASES)
def test_c_add_exact(n, metric_log):
    glue.run_add(n, True, metric_log)  # measured: 0 mismatches


@pytest.mark.parametrize("case", glue.DPT_FINAL_CASES)
def test_c_dpt_final_interval(case, metric_log):
    glue.run_dpt_final(case, True, metric_log)


# ---- head split / merge: bit-exact RNE hi / lo, order and position ---------------------------------------------------------------------------
def split_rne(x):
    """(hi, lo) bf16 of fp32 x, both rounded to nearest even"""
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def wide(shape, g):
    """fp32 values over many binades"""
    return torch.randn(shape, generator=g) * torch.exp(2 * torch.randn(shape, generator=g))


# (B, T, heads, hd): the last case wraps the q / k loop (B * T * heads * hd / 8 * 2 items)
HEADS_CASES = [(2, 1, 5, 64), (2, 77, 5, 64), (2, 128, 5, 64), (2, 1, 1, 512), (2, 77, 1, 512), (2, 128, 1, 512), (1, WRAP_C // 128 + 40, 1, 512)]


@pytest.mark.parametrize("case", HEADS_CASES)
def test_c_heads_split_exact(e, case, metric_log):
    b, t, heads, hd = case
    c, tpad = heads * hd, (t + 63) // 64 * 64
    ld = 3 * c + 4
    d = _dev()
    g = torch.Generator().manual_seed(seed_of("heads_split", *case))
    qkv = wide((b * t, ld), g).to(d)
    vbuf = sentinel(b * heads * hd * 3 * tpad, torch.bfloat16, d)
    qs, ks, _ = e.c_heads_split(qkv, b, t, heads, hd, vbuf[:-GUARD].view(b * heads, hd, 3 * tpad))
    vts = vbuf[:-GUARD].view(b * heads, hd, 3 * tpad)
    per_head = lambda x: x.view(b, t, heads, hd).permute(0, 2, 1, 3).reshape(b * heads, t, hd)   # [B*heads][T][hd]
    q, k, v = (per_head(qkv[:, i * c:(i + 1) * c]) for i in range(3))
    name = f"c_heads_split{case}"
    qh, ql = split_rne(q)
    check_exact(name + " Qs", qs, torch.cat([qh, ql, qh], dim=2), metric_log)      # A order [hi | lo | hi]
    kh, kl = split_rne(k)
    check_exact(name + " Ks", ks, torch.cat([kh, kh, kl], dim=2), metric_log)      # B order [hi | hi | lo]
    vt = torch.zeros(b * heads, hd, tpad, device=d)
    vt[:, :, :t] = v.transpose(1, 2)                                               # V transposed, zero in [T, Tpad)
    vh, vl = split_rne(vt)
    check_exact(name + " Vts", vts, torch.cat([vh, vh, vl], dim=2), metric_log)    # measured: 0 mismatches (all three)
    assert float(vts.view(b * heads, hd, 3, tpad)[..., t:].float().abs().max() if tpad > t else 0.0) == 0.0, "columns [T, Tpad) of every block must be zero"
    assert_untouched(name, vbuf[-GUARD:])
    differs(name, ks, torch.cat([kh, kl, kh], dim=2))                              # wrong variants: A order where B order is due,
    if t > 1:
        vn = torch.zeros(b * heads, hd, tpad, device=d)                            # V not transposed (token-major rows read as channel-major)
        vn.view(b * heads, -1)[:, :t * hd] = v.reshape(b * heads, -1)
        differs(name, vts[:, :, :tpad], vn.to(torch.bfloat16))
    differs(name, qs[:, :, :hd], per_head(qkv[:, c:2 * c]).to(torch.bfloat16))     # q and k exchanged


# (B, T, heads, hd): the last case wraps the loop (B * T * heads * hd / 8 items)
MERGE_CASES = [(2, 1, 5, 64), (2, 77, 5, 64), (2, 128, 1, 512), (1, WRAP_C // 40 + 9, 5, 64)]


@pytest.mark.parametrize("case", MERGE_CASES)
def test_c_heads_merge_split_exact(e, case, metric_log):
    b, t, heads, hd = case
    c = heads * hd
    d = _dev()
    g = torch.Generator().manual_seed(seed_of("heads_merge", *case))
    o = wide((b * heads, t, hd), g).to(d)
    out = e.c_heads_merge_split(o, b, heads)
    merged = o.view(b, heads, t, hd).permute(0, 2, 1, 3).reshape(b * t, c)         # head h at columns [h hd, (h + 1) hd)
    hi, lo = split_rne(merged)
    name = f"c_heads_merge_split{case}"
    check_exact(name, out, torch.cat([hi, lo, hi], dim=1), metric_log)             # A order; measured: 0 mismatches
    differs(name, out, torch.cat([hi, hi, lo], dim=1))                             # wrong variants: B order,
    if t > 1 and heads > 1:
        differs(name, out[:, :c], o.view(b, heads * t, hd).reshape(b * t, c).to(torch.bfloat16))   # the heads not interleaved back


# ---- c_cross_fold --------------------------------------------------------------------------------------------------------------------------
# (rows, C, heads): C = 64 uses 8 of a wave's 64 lanes, 640 fills the second vector of a lane partly, 2048 is the supported bound; rows % 4 != 0
# leaves a ragged last workgroup (one wave per row, four rows per workgroup)
C_FOLD_CASES = [(301, 64, 1), (5, 320, 5), (1001, 320, 5), (302, 640, 10), (577, 1280, 20), (7, 2048, 32)]


@pytest.mark.parametrize("want_n3", [True, False], ids=["n3", "no_n3"])
@pytest.mark.parametrize("case", C_FOLD_CASES)
def test_c_cross_fold_interval(e, case, want_n3, metric_log):
    rows, c, heads = case
    d = _dev()
    y, p = fold_inputs(case, torch.float32)                                       # (fp32 values: no input rounding)
    y, p = y.to(d), {k: v.to(d) for k, v in p.items()}
    # fold_ref_bound's E is the fp32 arithmetic of the folded form alone (the 16-bit file adds the input and output roundings through RNE16); the
    # fp32 kernel forms (y - mean) * rstd * U per element instead of one v_fma: two more roundings on the dot product's terms
    y64, err, (U, u0, G, c0) = fold_ref_bound(y, p, heads)
    mean = y.mean(1, keepdim=True)
    yhat = (y - mean) * (((y - mean) ** 2).mean(1, keepdim=True) + 1e-5).rsqrt()
    err = err + (2 * E24 * (yhat.abs() @ U.abs().t()) * 0.25) @ G.abs()           # (through the sigmoid, slope <= 1 / 4, onto G)
    f = lambda t: t.float().contiguous()
    yo, n3 = e.c_cross_fold(f(y), f(U), f(u0), f(G), f(c0), f(p["g3"]), f(p["b3"]), want_n3=want_n3)
    failures = []
    # wrong variant: the LayerNorm affine applied inside the fold as well (U already carries gamma2, u0 carries beta2)
    n2 = yhat * p["g2"] + p["b2"]
    wrong = y + c0 + torch.sigmoid(n2 @ U.t() + u0) @ G
    # the tables are rounded to fp32 before the kernel reads them: the reference takes the rounded tables
    Uf, u0f, Gf, c0f = (f(t).double() for t in (U, u0, G, c0))
    y64r = y + c0f + torch.sigmoid(yhat @ Uf.t() + u0f) @ Gf
    check_f32(f"c_cross_fold_y{case}", yo, y64r, err, metric_log, failures, wrong=wrong)   # measured: <= 0.44
    if want_n3:
        # norm3 reads the trunk AS STORED: the float64 LayerNorm of the kernel's own y_out, with the bound of test_layernorm_split
        x64 = yo.double()
        m3 = x64.mean(1, keepdim=True)
        var3 = ((x64 - m3) ** 2).mean(1, keepdim=True)
        g3, b3 = f(p["g3"]).double(), f(p["b3"]).double()
        n64 = (x64 - m3) / torch.sqrt(var3 + 1e-5) * g3 + b3
        bound = E15 * (n64.abs() + b3.abs()) + 2.0 ** -20 * g3.abs() * (1 + m3.abs() / var3.sqrt())
        r = float(((unsplit(n3, c) - n64).abs() / bound).max())
        rw = float(((n3[:, :c].double() - n64).abs() / bound).max())              # wrong variant: the hi part alone
        metric_log(f"c_cross_fold_n3{case}", gate_ratio=r, wrong_hi_only=rw)
        if not (r <= 1.0 and rw >= 8.0):                                           # measured: <= 0.25; hi only >= 119x
            failures.append(f"n3{case}: gate ratio {r:.3g}, hi only {rw:.3g}")
    assert not failures, "\n".join(failures)


# ---- c_cross_attn_small: the online softmax over L keys in fp32 ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 77])
def test_c_cross_attention_interval(e, L, metric_log):
    d = _dev()
    q, kc, vc = cross_inputs(L, torch.float32)                                    # rows 500, C 320: 2500 (row, head) threads, not a multiple of 256
    q, kc, vc = q.to(d), kc.to(d), vc.to(d)
    out = e.c_cross_attention(q.float(), kc, vc)
    o, err = cross_ref_bound(q, kc, vc)                                            # the 16-bit kernel's fp32 arithmetic: the same loop (products of fp32 numbers round once more: inside its 66 E24)
    err = err + E17 * o.abs()                                                      # the output split: hi + lo = o (1 + 2^-17)
    failures = []
    check_f32(f"c_cross_attn_L{L}", unsplit(out, q.shape[1]), o, err, metric_log, failures)   # measured: <= 0.19
    rw = float(((out[:, :q.shape[1]].double() - o).abs() / err).max())            # wrong variant: the hi part alone
    metric_log(f"c_cross_attn_L{L}_hi_only", wrong_hi_only=rw)
    assert not failures and rw >= 8.0, ("\n".join(failures), rw)                  # measured: hi only >= 42x


# ---- c_bilinear ----------------------------------------------------------------------------------------------------------------------------
# ((Hi, Wi), (Ho, Wo), align_corners, B, C): the DPT head's x2 steps (align_corners True) and its final resize; the last case wraps the loop
C_BILINEAR_CASES = [((12, 12), (24, 24), True, 2, 64), ((5, 7), (11, 3), False, 3, 4), ((1, 1), (3, 2), True, 1, 8), ((37, 1), (64, 5), False, 2, 8),
                    ((48, 48), (192, 192), True, 1, 228)]


@pytest.mark.parametrize("case", C_BILINEAR_CASES)
def test_c_bilinear_interval(e, case, metric_log):
    (hi, wi), (ho, wo), align, b, c = case
    d = _dev()
    g = torch.Generator().manual_seed(seed_of("c_bilinear", hi, wi, ho, wo, align, b, c))
    x = torch.randn(b, hi, wi, c, generator=g).to(d)
    out = e.c_bilinear(x, (ho, wo), align)
    x64 = x.double().permute(0, 3, 1, 2)
    y64 = F.interpolate(x64, size=(ho, wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    yabs = F.interpolate(x64.abs(), size=(ho, wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    # source coordinate: the scale (a division), its product with the index (+ 0.5, - 0.5 without align_corners): <= 4 roundings at the
    # coordinate's size, so the weights l, 1 - l move by 4 E24 max(coordinate, 1) per axis; a moved weight shifts the result by that times the
    # difference of two taps (<= 2 max |x|; a coordinate rounded across an integer lands in the next cell, where the interpolant is continuous).
    # Then the four weight products and the four-term sum: 8 roundings at sum w |tap|.
    err = 4 * E24 * (max(hi, 1) + max(wi, 1)) * 2 * float(x64.abs().max()) + 8 * E24 * yabs
    wrong = F.interpolate(x64, size=(ho, wo), mode="bilinear", align_corners=not align).permute(0, 2, 3, 1)
    failures = []
    check_f32(f"c_bilinear{case}", out, y64, err, metric_log, failures, wrong=wrong if (hi, wi) != (1, 1) else None)   # measured: <= 0.10
    assert not failures, "\n".join(failures)
