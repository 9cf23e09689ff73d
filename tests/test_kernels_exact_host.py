"""CPU side of tests/test_kernels_exact_gpu.py: the bit-exact GPU gates can fail, and only for kernel reasons.

  * every case of the GPU tables meets the operand condition sum |x w| + |bias| + |res| <= 2^24 g, so a nonzero mismatch count can only
    come from the kernel, and an fp32 sum of such operands in any order is the exact result;
  * the expected value float64 -> float32 -> 16 bit equals a from-scratch integer round-to-nearest-even, ties included, for bf16 and fp16;
  * the nearest wrong variants of every case family, evaluated here on the same kind of operands, differ from the expected bits in at least
    a stated number of elements: the inputs are rich enough to catch them.
"""
import math

import pytest
import torch

from test_kernels_exact_gpu import (CONV_CASES, FP32_EXACT, GEMM_CASES, HEADLINE_LAUNCHES, conv_ref64, parse_launch, exact_bias, exact_res, exact_w, exact_x,
                                    rne16, worst_sum)

DTYPES = [torch.bfloat16, torch.float16]


def _k_of_headline(case):
    op, kv, flags = parse_launch(case[0])
    return (kv["N"] // 8 if "geglu" in flags else kv["K"]), "+res" in flags


def test_operand_condition_every_gpu_case():
    ks = [(c[6] * c[6] * c[4], c[13]) for c in CONV_CASES] + [(c[3], c[5]) for c in GEMM_CASES] + [_k_of_headline(c) for c in HEADLINE_LAUNCHES]
    ks += [(4 * 192, True), (9 * 192, True), (27, False), (9 * 128, True), (640, True), (128, False), (1280, False), (2560, False)]
    for k, with_res in ks:
        assert worst_sum(k, True, with_res) <= FP32_EXACT, (k, worst_sum(k, True, with_res))
    # the tie-heavy case: integers, |x|, |w| <= 3, K = 128 (GEMM) and |x|, |w| <= 1, K = 1152 (conv), bias 1.5 * 2^11 at most
    assert 128 * 9 + 1.5 * 2 ** 11 <= FP32_EXACT and 1152 + 1.5 * 2 ** 11 <= FP32_EXACT


def test_fp32_sum_in_any_order_is_exact():
    """K = 23040 (the longest conv of the GPU tables): float32 sums in a shuffled order and in 8 slices equal the float64 result"""
    g = torch.Generator().manual_seed(0)
    k = 23040
    x, w = exact_x((64, k), g, "cpu"), exact_w((k,), g, "cpu")
    bias = exact_bias(64, k, g, "cpu")
    res = exact_res((64,), k, g, "cpu")
    ref = (x * w).sum(1) + bias + res
    prod = (x * w).float()
    perm = torch.randperm(k, generator=g)
    seq = torch.zeros(64, dtype=torch.float32)
    for i in perm[:4096].tolist():   # a sequential fp32 accumulation (subset: the bound holds for any prefix)
        seq += prod[:, i]
    assert torch.equal(seq.double(), (x * w)[:, perm[:4096]].sum(1))
    sliced = sum(prod[:, s::8].sum(1, dtype=torch.float32) for s in range(8)) + bias.float() + res.float()
    assert torch.equal(sliced.double(), ref)


# ---- rounding -----------------------------------------------------------------------------------------------------------------------------
def _int_rne(v32, dtype):
    """round-to-nearest-even of fp32 to bf16 / fp16 (normal range) by integer arithmetic on the bit patterns, returned as float64 values"""
    u = v32.view(torch.int32).long() & 0xffffffff
    sign = (u >> 31) & 1
    if dtype == torch.bfloat16:
        r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
        bits = (r << 16) & 0xffffffff
        return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).int().view(torch.float32).double()
    e = ((u >> 23) & 0xff) - 127
    mant = (u & 0x7fffff) | 0x800000      # 24 significant bits
    m, rem = mant >> 13, mant & 0x1fff     # keep 11
    up = (rem > 0x1000) | ((rem == 0x1000) & ((m & 1) == 1))
    m = m + up.long()
    val = m.double() * torch.pow(2.0, (e - 10).double())
    return torch.where(sign == 1, -val, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_expected_value_is_integer_rne(dtype):
    g = torch.Generator().manual_seed(1)
    mant = 8 if dtype == torch.bfloat16 else 11
    # random fp32 values over the binades the tests produce, plus exact ties (a half unit of the 16-bit format) and near-ties
    v = (torch.rand(200000, generator=g, dtype=torch.float64) * 2 - 1) * torch.pow(2.0, torch.randint(-12, 12, (200000,), generator=g).double())
    v = v[v.abs() >= 2.0 ** -14].float()   # (normal range of fp16)
    q = torch.randint(1 << (mant - 1), 1 << mant, (50000,), generator=g).double()
    sc = torch.pow(2.0, torch.randint(-10, 5, (50000,), generator=g).double())
    ties = ((q + 0.5) * sc).float()
    near = torch.cat([torch.nextafter(ties, torch.full_like(ties, math.inf)), torch.nextafter(ties, torch.full_like(ties, -math.inf))])
    allv = torch.cat([v, ties, -ties, near])
    got = rne16(allv.double(), dtype).double()
    assert torch.equal(got, _int_rne(allv, dtype))
    # ties really are decided to even: half of them round up
    up = (rne16(ties.double(), dtype).double() > ties.double()).double().mean().item()
    assert 0.4 < up < 0.6, up


# ---- wrong variants -------------------------------------------------------------------------------------------------------------------
def r16(v, dtype):
    """16-bit rounding of a float64 value through fp32 (as a kernel would store it), back to float64"""
    return v.float().to(dtype).double()


def _trunc16(v, dtype):
    """truncation toward zero to the 16-bit format (normal range)"""
    mant = 8 if dtype == torch.bfloat16 else 11
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-30)))
    q = torch.pow(2.0, e - (mant - 1))
    return torch.trunc(v / q) * q


def _half_away16(v, dtype):
    mant = 8 if dtype == torch.bfloat16 else 11
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-30)))
    q = torch.pow(2.0, e - (mant - 1))
    return torch.sign(v) * torch.floor(v.abs() / q + 0.5) * q


def _differ(a, b):
    return int((a != b).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_family_wrong_variants_change_bits(dtype):
    """M = 512, N = 320 (a ragged 64-column block after two of 128), K = 640 (ten 64-channel chunks), bias and 16-bit residual"""
    g = torch.Generator().manual_seed(2)
    m, n, k = 512, 320, 640
    a, bt = exact_x((m, k), g, "cpu"), exact_w((n, k), g, "cpu")
    bias = exact_bias(n, k, g, "cpu")
    res = exact_res((m, n), k, g, "cpu")
    acc = a @ bt.t()
    exp = rne16(acc + bias + res, dtype).double()
    total = m * n
    variants = {
        "rounded before the residual add": (r16(r16(acc + bias, dtype) + res, dtype), total // 32),
        "rounded before the bias add": (r16(r16(acc, dtype) + bias + res, dtype), total // 32),
        "16-bit split-K partials (4 slices)": (r16(sum(r16(a[:, s::4] @ bt[:, s::4].t(), dtype) for s in range(4)) + bias + res, dtype), total // 32),
        "truncation": (_trunc16(acc + bias + res, dtype), total // 32),
        "last 64-channel K chunk dropped": (r16(a[:, :-64] @ bt[:, :-64].t() + bias + res, dtype), total // 2),
        "residual read from the neighbouring row": (r16(acc + bias + res.roll(1, 0), dtype), total // 2),
        "bias missing in the last ragged column block": (torch.cat([exp[:, :256], r16(acc[:, 256:] + res[:, 256:], dtype)], 1), 256 * 64 // 2),
    }
    for name, (v, need) in variants.items():
        n_diff = _differ(v, exp)
        assert n_diff >= need, f"{name}: only {n_diff} elements differ (need {need})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_heavy_rounding_variants_change_bits(dtype):
    """the tie-heavy GPU case (integers |x|, |w| <= 3, K = 128, bias 1.5 * 2^P): round-half-away and truncation lose on many elements"""
    p = 8 if dtype == torch.bfloat16 else 11
    g = torch.Generator().manual_seed(99)
    a, bt = exact_x((512, 128), g, "cpu", lim=3, q=1.0), exact_x((256, 128), g, "cpu", lim=3, q=1.0)
    ref = a @ bt.t() + 1.5 * 2 ** p
    exp = rne16(ref, dtype).double()
    assert _differ(_half_away16(ref, dtype), exp) >= ref.numel() // 8
    assert _differ(_trunc16(ref, dtype), exp) >= ref.numel() // 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile_rows", [16, 12])
def test_halo_seam_variant_changes_bits(dtype, tile_rows):
    """a halo row zeroed at a tile seam (the input row just below / above it missing from the neighbouring tile's output row) changes
    almost every element of the two output rows at each seam; window of a 40 x 36 map, 128 -> 128 channels, with residual"""
    g = torch.Generator().manual_seed(3 + tile_rows)
    b, h, w, c, o = 1, 40, 36, 128, 128
    x, wt = exact_x((b, h, w, c), g, "cpu"), exact_w((o, c, 3, 3), g, "cpu")
    bias = exact_bias(o, 9 * c, g, "cpu")
    res = exact_res((b, h, w, o), 9 * c, g, "cpu")
    exp = rne16(conv_ref64(x, wt, bias) + res, dtype).double()
    for seam in range(tile_rows, h, tile_rows):
        for orow, zero_in in ((seam - 1, seam), (seam, seam - 1)):   # last row of the upper tile reads input row `seam`, and vice versa
            xz = x.clone()
            xz[:, zero_in] = 0
            v = r16(conv_ref64(xz, wt, bias)[:, orow] + res[:, orow], dtype)
            n_diff = _differ(v, exp[:, orow])
            assert n_diff >= w * o * 3 // 4, (seam, orow, n_diff)
