"""CPU side of tests/test_kernels_glue_gpu.py and tests/test_kernels_glue_contract_gpu.py.

  * On the inputs and with the references of the GPU files, a plain float32 evaluation of each arithmetic kernel stays within its bound E, and
    the nearest wrong variant falls outside (as tests/test_kernels_interval_host.py does for the norm and attention kernels).  Within HALF of
    E where E has room for another summation order (the dot products, the statistics).  The bounds of ddim_step, decode_epilogue and
    minmax_norm count exactly the two or three roundings any float32 evaluation makes, so a float32 evaluation can use all of E (measured
    here: up to 0.57, 0.86 and 0.94): those are held to E itself.
  * The concat statistics: fp32 two-pass statistics of the stored tensor use at most half of the scale / shift gates at every offset; the
    single-pass {sum, sum of squares} partials leave the gate in the fp16 library at mean / std = 256.
  * Every new test entry refuses what would fault with GP_ERR_INVALID before any HIP call: the small integers that stand for device pointers
    are never dereferenced (tests/test_ensemble_device_host.py).
  * Coverage guard: every launcher csrc/kernels.h declares is reached from a test entry of csrc/kernel_abi.hip, or is listed below with the
    launcher that reaches it.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_kernels_glue_gpu import (CAT_STATS_CASES, DECODE_CASES, MINMAX_CASES, cat_stats_inputs, ddim_coef, ddim_ref_bound, decode_ref_bound, minmax_inputs,
                                   minmax_ref_bound, single_pass_stats, stats_bounds, stats_ratios)
from test_kernels_interval_gpu import E24, gn_ratios, group_stats, r16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpercept_amd", "csrc")
GP_ERR_INVALID = 1
DTYPES = [torch.bfloat16, torch.float16, torch.float32]   # the two libraries' element types and the contract precision's storage
HALF = 0.5


def used(y32, y64, err):
    """largest fraction of E a float32 evaluation uses (0 where both the error and E are zero)"""
    d = (y32.double() - y64).abs()
    return float(torch.where(d > 0, d / (err + 1e-300), torch.zeros_like(d)).nan_to_num(0.0).max())


def outside(w64, y64, err):
    return float(((w64 - y64).abs() > err).double().mean())


# ---- float32 evaluations against the float64 bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_ddim_step_f32_within_gate(dt, clip):
    g = torch.Generator().manual_seed(11)
    k = ddim_coef(clip)
    s = torch.randn(3 * 37, 4, generator=g) * 1.5
    for _ in range(2):
        m = torch.randn(3 * 37, 4, generator=g).to(dt).float()
        kf = {n: torch.tensor(v, dtype=torch.float32) for n, v in k.items()}
        fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()   # a * b + c * d compiles to v_mul, v_fma: two roundings
        x0 = fma(kf["x0_sample"], s, kf["x0_model"] * m)
        if clip > 0:
            x0 = x0.clamp(-clip, clip)
        prev = fma(kf["prev_x0"], x0, kf["prev_eps"] * fma(kf["eps_sample"], s, kf["eps_model"] * m))
        x64, e_x0, p64, e_prev = ddim_ref_bound(m.double(), s.double(), k)
        assert used(x0, x64, e_x0) <= 1.0 and used(prev, p64, e_prev) <= 1.0
        assert outside(ddim_ref_bound(m.double(), s.double(), k, swap=True)[2], p64, e_prev) >= 0.02
        if clip > 0:
            assert outside(ddim_ref_bound(m.double(), s.double(), k, no_clip=True)[0], x64, e_x0) >= 0.02
        s = prev


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", DECODE_CASES[:3])
def test_decode_epilogue_f32_within_gate(case, dt):
    b, hw, ld = case
    g = torch.Generator().manual_seed(b * hw + ld)
    c = (torch.randn(b, hw, 3, generator=g) * 0.9).to(dt).float()
    for mean3, raw in ((1, 0), (0, 0), (1, 1), (0, 1)):
        v = ((c[..., 0] + c[..., 1] + c[..., 2]) / 3.0)[:, None] if mean3 else c.transpose(1, 2)
        if not raw:
            v = (v.clamp(-1, 1) + 1.0) * 0.5
        y64, err = decode_ref_bound(c.double(), mean3, raw)
        assert used(v, y64, err) <= 1.0, (case, mean3, raw)
        if mean3 and not raw and hw > 1:
            assert outside(decode_ref_bound(c.double(), mean3, raw, clip_first=True)[0], y64, err) >= 0.02


@pytest.mark.parametrize("case", MINMAX_CASES[:4])
def test_minmax_norm_f32_within_gate(case):
    x = minmax_inputs(case)
    mn, mx = x.min(dim=1, keepdim=True).values, x.max(dim=1, keepdim=True).values
    y32 = (x - mn) / (mx - mn)
    y64, err = minmax_ref_bound(x.double())
    assert used(y32, y64, err) <= 1.0
    assert torch.equal(torch.isnan(y32), torch.isnan(y64))
    if case[0] == 3 and case[1] > 1:   # the constant image alone is NaN; min-max over the batch is rejected
        assert bool(torch.isnan(y64[1]).all()) and not bool(torch.isnan(y64[0]).any())
        assert outside(minmax_ref_bound(x.double(), per_batch=True)[0].nan_to_num(7.0), y64, err) >= 0.02


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_small_dot_products_f32_within_half_gate(dt):
    """pointwise_small (Cin terms behind an in_scale product, onto the bias) and dpt_final (Cin terms onto the bias), sequentially in fp32"""
    g = torch.Generator().manual_seed(5)
    for cin, cout in ((4, 4), (8, 8), (5, 3), (32, 1)):
        x = torch.randn(500, cin, generator=g).to(dt).float()
        w = torch.randn(cout, cin, generator=g) / cin ** 0.5
        bias = 0.5 * torch.randn(cout, generator=g)
        s = torch.tensor(-1.0 / 0.18215, dtype=torch.float32) if cin <= 8 else torch.tensor(1.0)
        xs = x * s
        acc = bias.expand(500, cout).clone()
        for c in range(cin):   # one v_fma per term: the product is not rounded
            acc = (acc.double() + w[:, c].double() * xs[:, c:c + 1].double()).float()
        y64 = (x.double() * float(s)) @ w.double().t() + bias.double()
        mag = (x.double() * float(s)).abs() @ w.double().abs().t() + bias.double().abs()
        assert used(acc, y64, (cin + 1) * E24 * mag) <= HALF, (cin, cout)      # dpt_final's bound; pointwise_small's has cin + 2
        assert outside((x.double() @ w.double().t() + bias.double()) * float(s), y64, (cin + 2) * E24 * mag) >= 0.02 or cin > 8


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CAT_STATS_CASES, ids=[c[0] for c in CAT_STATS_CASES])
def test_concat_statistics_f32_within_half_gate(case, dt):
    name, ca, cb, b, hw, bm, groups = case
    eps = 1e-6
    for ratio in gn_ratios(dt):
        x, gamma, beta = cat_stats_inputs(case, ratio, dt)
        cpg = (ca + cb) // groups
        flat = x.float().view(b, hw, groups, cpg).permute(0, 2, 1, 3).reshape(b, groups, -1)
        mean = flat.mean(dim=2)
        rstd = 1.0 / torch.sqrt(((flat - mean[..., None]) ** 2).mean(dim=2) + eps)
        sc = rstd.repeat_interleave(cpg, dim=1) * gamma
        sh = beta - mean.repeat_interleave(cpg, dim=1) * sc
        r_sc, r_sh = stats_ratios(sc, sh, x, gamma, beta, eps, groups)
        assert r_sc <= HALF and r_sh <= HALF, (name, ratio, r_sc, r_sh)
        tile = bm or 16
        w = max(stats_ratios(*single_pass_stats(x, tile, gamma, beta, eps, groups), x, gamma, beta, eps, groups))
        if dt == torch.float16 and ratio == 256:
            assert w > 1.0, (name, w)   # the single-pass partials leave the gate


def test_concat_stats_bm_on_the_unet_shapes():
    """the tile choice on the UNet's concat shapes, 12^2 .. 96^2 latents at batch 1 and 4 (host arithmetic): the largest of 64, 48, 32, 16 that
    divides the image and still gives 512 workgroups, else the smallest that divides it"""
    from genpercept_amd import engine
    lib = _libs()[0]
    for side, chans in ((12, 2560), (24, 2560), (24, 1920), (48, 1920), (48, 1280), (48, 960), (96, 960), (96, 640)):
        for b in (1, 4):
            hw = side * side
            slices = (chans // 8 + 255) // 256
            valid = [m for m in (64, 48, 32, 16) if hw % m == 0]
            full = [m for m in valid if (b * hw // m) * slices >= 512]
            want = full[0] if full else valid[-1]
            assert lib.gp_concat_stats_bm(hw, b * hw, chans) == want == engine.concat_stats_bm(hw, b * hw, chans), (side, b, chans)
    assert lib.gp_concat_stats_bm(144, 144, 2560) == 16 and lib.gp_concat_stats_bm(9216, 4 * 9216, 640) == 64 and lib.gp_concat_stats_bm(9216, 9216, 640) == 16
    assert lib.gp_concat_stats_bm(37, 37, 64) == 0 and lib.gp_concat_stats_bm(0, 0, 64) == 0


# ---- argument validation ---------------------------------------------------------------------------------------------------------------------
def _libs():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


P, Q, R, S = 0x10000, 0x20000, 0x30000, 0x40000   # 16-byte aligned stand-ins for device pointers
COEF = (C.c_float * 7)(1, 1, 1, 1, 1, 1, 0)

# entry -> (valid arguments by name, in call order; the stream is appended), [changes that must be refused]
ENTRIES = {
    "gp_rgb_prologue": (dict(rgb=P, is_u8=1, out=Q, B=1, H=4, W=4, Cpad=8, contract=0),
                        [dict(rgb=None), dict(out=None), dict(out=Q + 8), dict(Cpad=12), dict(Cpad=0), dict(B=0), dict(H=0), dict(W=0), dict(is_u8=0, rgb=P + 2),
                         dict(contract=1, Cpad=8)]),
    "gp_concat": (dict(a=P, Ca=8, b=Q, Cb=16, out=R, pixels=5, contract=0),
                  [dict(a=None), dict(b=None), dict(out=None), dict(a=P + 8), dict(b=Q + 2), dict(out=R + 4), dict(Ca=12), dict(Cb=4), dict(Ca=0), dict(pixels=0)]),
    "gp_concat_stats": (dict(a=P, Ca=8, b=Q, Cb=8, out=R, B=2, HW=48, bm=16, bm_used=None, gamma=S, beta=S, groups=2, eps=1e-6, scale=S, shift=S),
                        [dict(a=None), dict(b=None), dict(out=None), dict(a=P + 8), dict(out=R + 8), dict(Ca=12), dict(Cb=0), dict(HW=40), dict(HW=37, bm=0),
                         dict(bm=-16), dict(bm=32), dict(B=0), dict(beta=None), dict(scale=None), dict(shift=None), dict(groups=0), dict(groups=3)]),
    "gp_rgb_conv_in_stats": (dict(rgb=P, is_u8=1, w=Q, bias=None, out=R, B=1, H=17, W=33, Cout=128, gamma=S, beta=S, groups=32, eps=1e-6, scale=S, shift=S),
                             [dict(rgb=None), dict(w=None), dict(out=None), dict(Cout=100), dict(Cout=0), dict(gamma=None), dict(beta=None), dict(scale=None),
                              dict(shift=None), dict(groups=0), dict(groups=48), dict(B=0), dict(H=0), dict(out=R + 8), dict(w=Q + 8)]),
    "gp_nchw_to_nhwc": (dict(x=P, out=Q, B=1, C=4, H=3, W=3, Cpad=8, contract=0), [dict(x=None), dict(out=None), dict(Cpad=3), dict(C=0), dict(B=0), dict(H=0)]),
    "gp_nhwc_to_nchw": (dict(x=P, out=Q, B=1, C=4, H=3, W=3, ld=8, contract=0), [dict(x=None), dict(out=None), dict(ld=3), dict(C=0), dict(W=0)]),
    "gp_ddim_init": (dict(noise=P, lat=Q, sample=R, B=1, H=3, W=3, L=4, ld=8, off=4, contract=0),
                     [dict(lat=None), dict(sample=None), dict(off=5), dict(off=-1), dict(ld=7), dict(L=0), dict(noise=None, off=8), dict(B=0)]),
    "gp_ddim_update": (dict(model=P, ldm=8, sample=Q, uin=R, ldu=8, off=4, x0=S, ldx=4, pixels=9, L=4, coef=COEF, contract=0),
                       [dict(model=None), dict(sample=None), dict(uin=None), dict(coef=None), dict(off=5), dict(off=-4), dict(ldu=7), dict(ldm=3), dict(ldx=3),
                        dict(pixels=0), dict(L=0)]),
    "gp_decode_epilogue": (dict(x=P, out=Q, B=1, H=3, W=3, ld=4, mean3=1, raw=0, contract=0),
                           [dict(x=None), dict(out=None), dict(ld=2), dict(ld=6), dict(ld=3), dict(x=P + 4), dict(B=0)]),
    "gp_scale_pad": (dict(x=P, out=Q, pixels=9, C=4, ldi=4, ldo=8, scale=1.0), [dict(x=None), dict(out=None), dict(ldi=3), dict(ldo=3), dict(C=0), dict(pixels=0)]),
    "gp_pointwise_small": (dict(x=P, out=Q, w=R, bias=None, pixels=9, Cin=4, Cout=4, ldi=8, ldo=8, in_scale=1.0, contract=0),
                           [dict(x=None), dict(out=None), dict(w=None), dict(Cin=9), dict(Cin=0), dict(Cout=9), dict(Cout=0), dict(ldo=3), dict(ldi=3), dict(pixels=0)]),
    "gp_relu": (dict(x=P, out=Q, n=64), [dict(x=None), dict(out=None), dict(x=P + 2), dict(out=Q + 8), dict(n=60), dict(n=0)]),
    "gp_add": (dict(a=P, b=Q, out=R, n=64, contract=0), [dict(a=None), dict(b=None), dict(out=None), dict(a=P + 2), dict(b=Q + 4), dict(out=R + 8), dict(n=60), dict(n=0)]),
    "gp_dpt_final": (dict(x=P, w=Q, bias=0.5, out=R, B=1, HW=9, Cin=32, contract=0),
                     [dict(x=None), dict(w=None), dict(out=None), dict(Cin=12), dict(Cin=0), dict(x=P + 8), dict(B=0), dict(HW=0)]),
    "gp_minmax_norm": (dict(x=P, B=2, n=100), [dict(x=None), dict(B=0), dict(n=0), dict(B=65536)]),
}
# the contract forms (contract = 1) refuse the fp32 vector conditions in the bf16 library and everything in the fp16 library
CONTRACT_ENTRIES = {
    "gp_rgb_prologue": (dict(rgb=P, is_u8=1, out=Q, B=1, H=4, W=4, Cpad=64, contract=1), [dict(Cpad=8), dict(out=Q + 8), dict(rgb=None)]),
    "gp_concat": (dict(a=P, Ca=4, b=Q, Cb=8, out=R, pixels=5, contract=1), [dict(Ca=6), dict(Cb=2), dict(a=P + 8), dict(out=R + 4)]),
    "gp_nchw_to_nhwc": (dict(x=P, out=Q, B=1, C=4, H=3, W=3, Cpad=8, contract=1), [dict(Cpad=3)]),
    "gp_nhwc_to_nchw": (dict(x=P, out=Q, B=1, C=4, H=3, W=3, ld=8, contract=1), [dict(ld=3)]),
    "gp_ddim_init": (dict(noise=P, lat=Q, sample=R, B=1, H=3, W=3, L=4, ld=8, off=4, contract=1), [dict(off=5)]),
    "gp_ddim_update": (dict(model=P, ldm=8, sample=Q, uin=R, ldu=8, off=4, x0=S, ldx=4, pixels=9, L=4, coef=COEF, contract=1), [dict(off=5), dict(ldx=3)]),
    "gp_decode_epilogue": (dict(x=P, out=Q, B=1, H=3, W=3, ld=3, mean3=1, raw=0, contract=1), [dict(ld=2)]),
    "gp_pointwise_small": (dict(x=P, out=Q, w=R, bias=None, pixels=9, Cin=4, Cout=4, ldi=8, ldo=8, in_scale=1.0, contract=1), [dict(Cin=9), dict(ldo=3)]),
    "gp_add": (dict(a=P, b=Q, out=R, n=64, contract=1), [dict(n=62), dict(a=P + 4)]),
    "gp_dpt_final": (dict(x=P, w=Q, bias=0.5, out=R, B=1, HW=9, Cin=32, contract=1), [dict(Cin=6), dict(x=P + 8)]),
    "gp_c_heads_split": (dict(qkv=P, ld=960, Qs=Q, Ks=R, Vts=S, B=2, T=77, Tpad=128, heads=5, hd=64),
                         [dict(qkv=None), dict(Qs=None), dict(Ks=None), dict(Vts=None), dict(hd=32), dict(hd=96), dict(Tpad=100), dict(Tpad=64), dict(ld=956),
                          dict(ld=962), dict(qkv=P + 8), dict(Vts=S + 8), dict(T=0), dict(heads=0)]),
    "gp_c_heads_merge_split": (dict(O=P, out=Q, B=2, T=77, heads=5, hd=64), [dict(O=None), dict(out=None), dict(hd=60), dict(O=P + 8), dict(out=Q + 8), dict(T=0)]),
    "gp_c_cross_fold": (dict(y=P, y_out=Q, n3=R, U=S, u0=S, G=S, c0=S, g3=S, b3=S, rows=5, C=320, heads=5, eps=1e-5),
                        [dict(y=None), dict(y_out=None), dict(U=None), dict(u0=None), dict(G=None), dict(c0=None), dict(g3=None), dict(b3=None), dict(C=2056),
                         dict(C=324), dict(C=0), dict(y=P + 8), dict(n3=R + 8), dict(U=S + 4), dict(rows=0), dict(heads=0)]),
    "gp_c_cross_attention": (dict(q=P, kc=Q, vc=R, out=S, rows=5, C=320, L=2), [dict(q=None), dict(kc=None), dict(vc=None), dict(out=None), dict(C=96), dict(C=0),
                                                                                  dict(L=0), dict(rows=0), dict(q=P + 8), dict(out=S + 8)]),
    "gp_c_bilinear": (dict(x=P, out=Q, B=1, Hi=3, Wi=3, Ho=6, Wo=6, C=8, align=1), [dict(x=None), dict(out=None), dict(C=6), dict(C=0), dict(Hi=0), dict(Wo=0),
                                                                                     dict(x=P + 8), dict(out=Q + 4)]),
}


def _call(lib, name, args):
    return getattr(lib, name)(*args.values(), None)   # (the stream)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_invalid_arguments_are_refused_without_a_gpu(name):
    ok, bad = ENTRIES[name]
    for lib in _libs():
        for kw in bad:
            assert _call(lib, name, dict(ok, **kw)) == GP_ERR_INVALID, (name, kw)


@pytest.mark.parametrize("name", sorted(CONTRACT_ENTRIES))
def test_contract_forms_refuse_invalid_arguments_and_the_fp16_library(name):
    ok, bad = CONTRACT_ENTRIES[name]
    bf16, fp16 = _libs()
    for kw in bad:
        assert _call(bf16, name, dict(ok, **kw)) == GP_ERR_INVALID, (name, kw)
    assert _call(fp16, name, ok) == GP_ERR_INVALID, name   # the contract precision lives in the bf16 library


def test_every_new_entry_has_validation_cases():
    from genpercept_amd import engine
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    new = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr[hdr.index("gp_status gp_rgb_prologue("):]))
    assert new - {"gp_concat_stats_bm"} == set(ENTRIES) | set(CONTRACT_ENTRIES)
    for name in new:
        assert name in engine.SYMBOLS
    for name, (ok, _) in list(ENTRIES.items()) + list(CONTRACT_ENTRIES.items()):
        assert len(ok) + 1 == len(engine.SYMBOLS[name][1]), name   # (+ the stream)


# ---- coverage guard --------------------------------------------------------------------------------------------------------------------------
# launchers no test entry calls by name, with the launcher (called from an entry) that reaches them
REACHED_THROUGH = {
    "launch_groupnorm_apply": "launch_groupnorm (gp_groupnorm)",
    "launch_c_gn_stats": "launch_c_groupnorm_scale_shift (gp_c_groupnorm_split, gp_c_conv2d)",
    "launch_conv_halo": "launch_igemm, tile hint 5 (gp_conv2d, gp_conv2d_up2, gp_conv2d_gn, gp_conv2d_stats, gp_c_conv2d)",
    "launch_pgemm": "launch_igemm, tile hint 7 (gp_gemm, gp_gemm_qkv, gp_conv2d_stats)",
    "launch_conv_img": "launch_igemm on 576-pixel maps (gp_conv2d, gp_c_conv2d)",
}


def test_every_launcher_is_reached_from_a_test_entry():
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    abi = open(os.path.join(CSRC, "kernel_abi.hip")).read()
    declared = set(re.findall(r"^void (launch_[a-z0-9_]+)\(", hdr, flags=re.M))
    called = set(re.findall(r"\b(launch_[a-z0-9_]+)\(", abi))
    assert len(declared) >= 50, sorted(declared)
    missing = declared - called - set(REACHED_THROUGH)
    assert not missing, f"launchers without a test entry: {sorted(missing)} (add a gp_* entry to kernel_abi.hip and a test, or list the launcher that reaches it)"
    stale = (set(REACHED_THROUGH) & called) | (set(REACHED_THROUGH) - declared)
    assert not stale, f"listed launchers that now have an entry, or no longer exist: {sorted(stale)}"
    srcs = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(".hip") and f != "kernel_abi.hip")
    for name, via in REACHED_THROUGH.items():
        parent = via.split()[0].rstrip(",")
        assert parent in called and re.search(rf"\b{name}\(", srcs), (name, via)
