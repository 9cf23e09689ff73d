"""Bit-exact tests of the 16-bit conv / GEMM kernel paths (GPU), both libraries, every case pinned to the kernel it must reach.

Exact operands: x = i * 2^-4 and w = j * 2^-8 * s (|i|, |j| <= 15, s a power of two), bias and residual integer multiples of the product
grid g = 2^-12 * s, and sum_k |x_k w_k| + |bias| + |res| <= 2^24 g for every output.  Then every partial sum of every summation order --
MFMA, split-K, conv_img K slices, phase-summed weights -- is an fp32 number: the fp32 pre-activation of a correct kernel IS the float64
result, and its 16-bit output is, bit for bit, RNE16(float32(float64 result)) (the float64 -> float32 step is asserted exact, so nothing
rounds twice).  A seam, tap, K-chunk, residual, bias, zero-fill or double-rounding error changes bits: the assertion is ZERO mismatching
elements (values compared, so +0 and -0 are one value).  tests/test_kernels_exact_host.py shows on the CPU that the operands meet the
condition and that the nearest wrong variants of every family change bits on these inputs.

The references are float64 on the GPU: per-tap matmuls (conv) and plain matmuls (GEMM), never a library convolution (Winograd / FFT
algorithms are not exact).  Where an epilogue evaluates a transcendental (SiLU, GEGLU's erf) the exact form cannot hold; those cases
assert instead that the output is RNE16 of some value within the kernel's own error bound E of the float64 result (see _check_interval).

Paths (gp_last_igemm_path): 1 halo 16-row tiles, 2 halo phases (x2 upsample), 3 persistent GEMM (+ row tile), 4 conv_img + split-K
reduce, 5 split-K igemm + reduce, 6 generic igemm, 7 halo 12-row tiles, 8 per-tile halo; 0 = no conv / GEMM launcher ran.

The non-matrix 16-bit kernels (GroupNorm, LayerNorm, the cross-attention fold, row softmax, flash attention, the GroupNorm statistics of the
conv epilogues), which exact operands cannot express, are held to per-element float64 intervals in tests/test_kernels_interval_gpu.py, the
outputs of the GroupNorm-fused conv input and of the decoder tail in tests/test_kernels_fused_gn_gpu.py; the former's docstring lists what
remains out of scope.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

XQ, WQ, GQ = 2.0 ** -4, 2.0 ** -8, 2.0 ** -12   # grids of x, w (times s) and of their products
OPS_LIM = 15                                     # |i|, |j| <= 15
FP32_EXACT = 2.0 ** 24                           # partial sums stay exact while sum |terms| <= 2^24 g
DBG_TR12, DBG_TR16, DBG_HALO2 = 1 << 20, 2 << 20, 256   # GENPERCEPT_IGEMM_DBG: force 12-row / 16-row tiles, the per-tile halo kernel


# ---- exact operands (shared with tests/test_kernels_exact_host.py) ---------------------------------------------------------------------
def bias_lim(k):
    """|bias| <= bias_lim(K) g: comparable to the sum of K products (std ~ 80 sqrt(K) g)"""
    return 64 * int(math.isqrt(k)) + 63


def res_scale(k):
    """residual = r * res_scale(K) g with |r| <= 255: a power of two, so the residual is a 16-bit number (8 significant bits) on the grid"""
    return 2 ** max(0, int(math.log2(max(1.0, math.sqrt(k) / 2))))


def worst_sum(k, bias=True, res=True):
    """largest possible sum |x w| + |bias| + |res| of one output, in units of g"""
    return k * OPS_LIM * OPS_LIM + (bias_lim(k) if bias else 0) + (255 * res_scale(k) if res else 0)


def exact_x(shape, gen, device, lim=OPS_LIM, q=XQ):
    return torch.randint(-lim, lim + 1, shape, generator=gen, device=device).double() * q


def exact_w(shape, gen, device, s=1.0, lim=OPS_LIM):
    return torch.randint(-lim, lim + 1, shape, generator=gen, device=device).double() * (WQ * s)


def exact_bias(n, k, gen, device, s=1.0):
    b = bias_lim(k)
    return torch.randint(-b, b + 1, (n,), generator=gen, device=device).double() * (GQ * s)


def exact_res(shape, k, gen, device, s=1.0):
    return torch.randint(-255, 256, shape, generator=gen, device=device).double() * (res_scale(k) * GQ * s)


def rne16(v64, dtype):
    """float64 -> float32 (asserted exact) -> 16-bit (round to nearest, ties to even)"""
    v32 = v64.float()
    assert torch.equal(v32.double(), v64), "the float64 reference is not an fp32 number: the operand condition is violated"
    return v32.to(dtype)


# ---- float64 references on the device --------------------------------------------------------------------------------------------------
def conv_ref64(x, w, bias=None, stride=1, pad=(1, 1), out_hw=None, ups_hw=None):
    """x [B,H,W,C] float64 NHWC, w [O,C,k,k] -> [B,Ho,Wo,O] float64: sum over taps of plain matmuls, image by image"""
    if ups_hw is not None:
        x = F.interpolate(x.permute(0, 3, 1, 2), size=ups_hw, mode="nearest").permute(0, 2, 3, 1)
    b, h, wd, c = x.shape
    o, _, k, _ = w.shape
    ho, wo = out_hw or (h, wd)
    pt, pl = pad if k == 3 else (0, 0)
    hp, wp = max(h + pt, pt + stride * (ho - 1) + k), max(wd + pl, pl + stride * (wo - 1) + k)
    out = torch.empty((b, ho, wo, o), dtype=torch.float64, device=x.device)
    wt = w.permute(2, 3, 1, 0).contiguous()   # [k][k][C][O]
    for i in range(b):
        xp = torch.zeros((hp, wp, c), dtype=torch.float64, device=x.device)
        xp[pt:pt + h, pl:pl + wd] = x[i]
        acc = torch.zeros((ho * wo, o), dtype=torch.float64, device=x.device)
        for dy in range(k):
            for dx in range(k):
                patch = xp[dy:dy + stride * (ho - 1) + 1:stride, dx:dx + stride * (wo - 1) + 1:stride]
                acc += patch.reshape(-1, c) @ wt[dy, dx]
        if bias is not None:
            acc += bias
        out[i] = acc.view(ho, wo, o)
    return out


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def _eng():
    from genpercept_amd import engine
    return engine


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def precision(request):
    """every case runs against both libraries: bf16 elements (libgenpercept_hip.so) and fp16 elements (libgenpercept_hip_f16.so)"""
    from genpercept_amd import engine
    engine.set_default_precision(request.param)
    yield request.param
    engine.set_default_precision("bf16")


def _tag(name):
    return name + ("" if _eng().act_dtype() == torch.bfloat16 else "[fp16]")


def check_exact(name, out, expected, log, path=None, bm=None, **extra):
    """zero mismatching elements; logs the count and the first few (flat index, expected bits, output bits)"""
    assert out.shape == expected.shape and out.dtype == expected.dtype, (out.shape, expected.shape, out.dtype, expected.dtype)
    o, e = out.float(), expected.float()
    bad = ~((o == e) | (torch.isnan(o) & torch.isnan(e)))
    n = int(bad.sum())
    first = []
    if n:
        idx = bad.flatten().nonzero()[:5, 0]
        ib = torch.int16 if out.element_size() == 2 else torch.int32
        first = [(int(i), hex(int(expected.flatten().view(ib)[i]) & 0xffffffff), hex(int(out.flatten().view(ib)[i]) & 0xffffffff)) for i in idx]
    log(_tag(f"exact[{name}]"), mismatches=n, elements=out.numel(), path=path, pgemm_bm=bm, first=str(first), **extra)
    assert n == 0, f"{name}: {n} of {out.numel()} elements differ from RNE16(float64); first (index, expected, got): {first}"


def check_path(name, want_path, want_bm=None):
    path, bm = _eng().last_igemm_path()
    assert path == want_path, f"{name}: kernel path {path}, expected {want_path}"
    if want_bm is not None:
        assert bm == want_bm, f"{name}: persistent GEMM row tile {bm}, expected {want_bm}"
    return path, bm


def ulp16(v, dtype):
    """spacing of the 16-bit format at |v| (subnormal spacing of fp16 below 2^-14)"""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def _check_interval(name, out, y64, err_bound, log, path, wrong=None, bm=None):
    """out must be RNE16 of a value within err_bound of the float64 result: RNE16(y - E) <= out <= RNE16(y + E) (rounding is monotonic).
    The ratio logged is max |out - y| / (ulp16(y) / 2 + E): <= 1 for a correct kernel.  `wrong` = a wrong variant's float64 result: the
    fraction of its elements outside the same interval is logged and must be large."""
    dt = out.dtype
    lo, hi = (y64 - err_bound).float().to(dt).double(), (y64 + err_bound).float().to(dt).double()
    o = out.double()
    bad = ~((o >= lo) & (o <= hi))
    n = int(bad.sum())
    ratio = float(((o - y64).abs() / (0.5 * ulp16(y64, dt) + err_bound)).max())
    rec = dict(mismatches=n, elements=out.numel(), path=path, pgemm_bm=bm, gate_ratio=ratio)
    if wrong is not None:
        wv = wrong.float().to(dt).double()
        rec["wrong_outside"] = float((~((wv >= lo) & (wv <= hi))).double().mean())
    log(_tag(f"interval[{name}]"), **rec)
    assert n == 0, f"{name}: {n} elements outside RNE16(y +- E); max ratio {ratio:.3g}"
    if wrong is not None:
        assert rec["wrong_outside"] >= 0.02, f"{name}: the wrong variant is not rejected ({rec['wrong_outside']:.3g})"


# ---- conv cases through gp_conv2d ------------------------------------------------------------------------------------------------------
# (name, B, H, W, Cin, Cout, ks, stride, pad, ups_hw, tile, env, act, residual, n_store, s, want_path)
CONV_CASES = [
    # halo, 16-row tiles forced / 12-row tiles forced: H, W not multiples of 12 or 16, several channel slices incl. a ragged one
    ("halo16_37x50", 1, 37, 50, 256, 320, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR16)}, "none", True, 0, 1.0, 1),
    ("halo12_37x50", 1, 37, 50, 256, 320, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR12)}, "none", True, 0, 1.0, 7),
    ("halo12_31x95_b2", 2, 31, 95, 128, 128, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR12)}, "none", True, 0, 1.0, 7),
    # more tiles than CUs: workgroups take several tiles (4 x 9 x 10 = 360 16x16 tiles, 4 x 12 x 10 = 480 12x16 tiles)
    ("halo16_many_tiles", 4, 144, 160, 64, 128, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR16)}, "none", True, 0, 1.0, 1),
    ("halo12_many_tiles", 4, 144, 160, 64, 128, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR12)}, "none", False, 0, 1.0, 7),
    # per-tile halo kernel (conv3x3_halo2_kernel), plain and nine-tap x2 upsample
    ("halo2_tiles", 2, 33, 40, 128, 256, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_HALO2)}, "none", True, 0, 1.0, 8),
    ("halo2_tiles_ups", 1, 12, 10, 64, 128, 3, 1, (1, 1), (24, 20), 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_HALO2)}, "none", False, 0, 1.0, 8),
    # x2 upsample through the nine-tap halo kernel (gp_conv2d passes no phase weights)
    ("halo_ninetap_ups", 2, 17, 23, 128, 128, 3, 1, (1, 1), (34, 46), 5, {}, "none", True, 0, 1.0, 1),
    # ReLU in the staged epilogue
    ("halo16_relu", 1, 40, 36, 128, 128, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR16)}, "relu", True, 0, 1.0, 1),
    # whole-image tiles (conv_img): 24x24 (one image per unit) and 12x12 (four per unit), uneven K slices, two images per unit (12x24)
    ("conv_img_24", 4, 24, 24, 128, 128, 3, 1, (1, 1), None, 0, {}, "none", True, 0, 1.0, 4),
    ("conv_img_24_k5760", 2, 24, 24, 640, 64, 3, 1, (1, 1), None, 0, {}, "none", True, 0, 1.0, 4),
    ("conv_img_12", 8, 12, 12, 192, 192, 3, 1, (1, 1), None, 0, {}, "none", True, 0, 1.0, 4),
    ("conv_img_12x24", 2, 12, 24, 320, 128, 3, 1, (1, 1), None, 0, {}, "none", False, 0, 1.0, 4),
    # split-K igemm + reduce (K slices of 9 x 64-channel chunks)
    ("splitk_12_k23040", 1, 12, 12, 2560, 1280, 3, 1, (1, 1), None, 0, {}, "none", True, 0, 1.0, 5),
    ("splitk_ragged", 1, 9, 11, 1280, 200, 3, 1, (1, 1), None, 2, {}, "none", True, 0, 1.0, 5),
    # generic implicit GEMM, every tile configuration (1 = 128x128, 2 = 64x64, 3 = 256x32, 4 = 256x128, 6 = 128x64)
    ("igemm_t1", 2, 16, 16, 64, 64, 3, 1, (1, 1), None, 1, {}, "none", True, 0, 1.0, 6),
    ("igemm_t2", 1, 17, 19, 64, 200, 3, 1, (1, 1), None, 2, {}, "none", True, 0, 1.0, 6),
    ("igemm_t3", 3, 9, 7, 64, 32, 3, 1, (1, 1), None, 3, {}, "none", True, 0, 1.0, 6),
    ("igemm_t4", 2, 33, 31, 128, 320, 3, 1, (1, 1), None, 4, {}, "none", True, 0, 1.0, 6),
    ("igemm_t6", 1, 40, 36, 256, 128, 3, 1, (1, 1), None, 6, {}, "none", True, 0, 1.0, 6),
    # direct epilogue (ldo % 8 != 0): 100 output channels
    ("igemm_direct_ldo100", 1, 13, 15, 192, 100, 3, 1, (1, 1), None, 1, {}, "none", True, 0, 1.0, 6),
    # stride 2: symmetric pad 1 (UNet Downsample2D) and right / bottom pad only (VAE encoder Downsample2D)
    ("s2_pad1", 2, 30, 40, 64, 128, 3, 2, (1, 1), None, 0, {}, "none", False, 0, 1.0, 6),
    ("s2_pad0", 2, 31, 40, 64, 128, 3, 2, (0, 0), None, 0, {}, "none", False, 0, 1.0, 6),
    # nearest upsample fused into the generic conv's gather: x2 and to a size that is not x2
    ("ups_to_size", 2, 7, 10, 128, 64, 3, 1, (1, 1), (15, 20), 0, {}, "none", False, 0, 1.0, 6),
    ("ups_x2_igemm", 2, 8, 10, 128, 64, 3, 1, (1, 1), (16, 20), 0, {}, "none", True, 0, 1.0, 6),
    # Cout = 4 stored into 64 zero-filled channels (latent layout); 1x1 conv of a map
    ("cout4_store64", 1, 10, 12, 128, 4, 3, 1, (1, 1), None, 0, {}, "none", False, 64, 1.0, 6),
    # scale s = 2^-3 (smaller products, more binades below the output's rounding point)
    ("halo16_s", 1, 32, 48, 128, 128, 3, 1, (1, 1), None, 5, {"GENPERCEPT_IGEMM_DBG": str(DBG_TR16)}, "none", True, 0, 0.125, 1),
]


def _conv_prefilled(xd, wp, bias, cout, ks, b, ho, wo, nst, stride=1, pad=(1, 1), residual=None, ups_hw=None, act="none", tile=0):
    """gp_conv2d into an output prefilled with NaN: every element, the zero-filled columns beyond Cout included, must be written"""
    e = _eng()
    _, hi, wi, cin = xd.shape
    uh, uw = ups_hw if ups_hw else (0, 0)
    out = torch.full((b, ho, wo, nst), float("nan"), dtype=e.act_dtype(), device=xd.device)
    st = e.load_library().gp_conv2d(xd.data_ptr(), wp.data_ptr(), bias.data_ptr(), None if residual is None else residual.data_ptr(), out.data_ptr(),
                                    b, hi, wi, cin, cout, ks, stride, pad[0] if ks == 3 else 0, pad[1] if ks == 3 else 0, ho, wo, uh, uw, e.ACT[act],
                                    nst, 0, tile, torch.cuda.current_stream().cuda_stream)
    assert st == 0, f"gp_conv2d failed ({st})"
    return out


def _conv_operands(b, h, w, cin, cout, ks, s, with_res, ho, wo, nst, seed, d, cin_real=None):
    g = torch.Generator(device=d).manual_seed(seed)
    k = ks * ks * (cin_real or cin)
    x = exact_x((b, h, w, cin_real or cin), g, d)
    wt = exact_w((cout, cin_real or cin, ks, ks), g, d, s)
    bias = exact_bias(cout, k, g, d, s)
    res = exact_res((b, ho, wo, nst), k, g, d, s) if with_res else None
    return x, wt, bias, res, k


def _h16(t):
    return t.to(_eng().act_dtype())


def _pack(wt, cin_pad=None, geglu=False):
    e = _eng()
    w32 = wt.float().cpu()
    assert torch.equal(w32.to(e.act_dtype()).double(), wt.cpu()), "weights must be 16-bit numbers"
    return e.pack_weight(w32, cin_pad, geglu=geglu, device=_dev())


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_exact(case, metric_log, monkeypatch):
    e = _eng()
    name, b, h, w, cin, cout, ks, stride, pad, ups, tile, env, act, with_res, n_store, s, want = case
    for kname, v in env.items():
        monkeypatch.setenv(kname, v)
    d = _dev()
    hin, win = ups if ups else (h, w)
    # stride 2: pad 1 on every side, or (VAE) the right / bottom pad only
    ho, wo = (hin, win) if stride == 1 else ((hin - 1) // 2 + 1, (win - 1) // 2 + 1) if pad == (1, 1) else ((hin - 2) // 2 + 1, (win - 2) // 2 + 1)
    nst = n_store or cout
    x, wt, bias, res, k = _conv_operands(b, h, w, cin, cout, ks, s, with_res, ho, wo, nst, zlib.crc32(name.encode()) % 100003, d)
    assert worst_sum(k, True, with_res) <= FP32_EXACT
    e.last_igemm_path()
    y = _conv_prefilled(_h16(x), _pack(wt), bias.float(), cout, ks, b, ho, wo, nst, stride=stride, pad=pad, ups_hw=ups,
                        residual=_h16(res) if with_res else None, act=act, tile=tile)
    path, bm = check_path(name, want)
    ref = conv_ref64(x, wt, bias, stride, pad, (ho, wo), ups)
    if with_res:
        ref = ref + res[..., :cout]
    if act == "relu":
        ref = ref.clamp_min(0)
    exp = torch.zeros((b, ho, wo, nst), dtype=e.act_dtype(), device=d)
    exp[..., :cout] = rne16(ref, e.act_dtype())
    check_exact(name, y, exp, metric_log, path)


def test_conv_upsample_x2_phase_kernel_exact(metric_log):
    """gp_conv2d_up2: four 2 x 2-tap phase convolutions with phase-summed weights (a sum of up to four j * 2^-8 weights: at most 6 significant bits,
    a 16-bit number) -- the result must equal the nine-tap conv of the upsampled map bit for bit"""
    e = _eng()
    d = _dev()
    for (b, h, w, cin, cout, with_res) in [(2, 24, 40, 128, 128, True), (1, 17, 33, 64, 64, False), (2, 31, 47, 192, 320, True)]:
        name = f"up2_phases_{b}x{h}x{w}x{cin}x{cout}"
        x, wt, bias, res, k = _conv_operands(b, h, w, cin, cout, 3, 1.0, with_res, 2 * h, 2 * w, cout, h * w + cin, d)
        assert worst_sum(4 * cin, True, with_res) <= FP32_EXACT
        e.last_igemm_path()
        y = e.conv2d_up2(_h16(x), _pack(wt), e.pack_weight_phases(wt.float().cpu(), device=d), bias.float(), cout,
                         residual=_h16(res) if with_res else None)
        path, _ = check_path(name, 2)
        ref = conv_ref64(x, wt, bias, ups_hw=(2 * h, 2 * w))
        if with_res:
            ref = ref + res
        check_exact(name, y, rne16(ref, e.act_dtype()), metric_log, path)


def test_conv_upsample_x2_no_phases_switch(metric_log, monkeypatch):
    """GENPERCEPT_NO_UP_PHASES: the x2-upsample conv leaves the phase kernel.  Only the phase launcher reads the phase weights
    (conv_halo.hip: launch_halo3_ph), so with the switch on the engine's launch is the nine-tap halo launch gp_conv2d makes: path 1,
    bit-exact; the phase-kernel entry gp_conv2d_up2 refuses rather than run something else."""
    e = _eng()
    d = _dev()
    monkeypatch.setenv("GENPERCEPT_NO_UP_PHASES", "1")
    b, h, w, cin, cout = 2, 24, 40, 128, 128
    x, wt, bias, res, k = _conv_operands(b, h, w, cin, cout, 3, 1.0, True, 2 * h, 2 * w, cout, 4242, d)
    with pytest.raises(RuntimeError):
        e.conv2d_up2(_h16(x), _pack(wt), e.pack_weight_phases(wt.float().cpu(), device=d), bias.float(), cout, residual=_h16(res))
    e.last_igemm_path()
    y = _conv_prefilled(_h16(x), _pack(wt), bias.float(), cout, 3, b, 2 * h, 2 * w, cout, ups_hw=(2 * h, 2 * w), residual=_h16(res), tile=5)
    path, _ = check_path("ninetap_no_up_phases", 1)
    check_exact("ninetap_no_up_phases", y, rne16(conv_ref64(x, wt, bias, ups_hw=(2 * h, 2 * w)) + res, e.act_dtype()), metric_log, path)


def test_conv_small_cin_padded_exact(metric_log):
    """conv_in form: 3 real input channels zero-padded to 64 (input and packed weight)"""
    e = _eng()
    d = _dev()
    g = torch.Generator(device=d).manual_seed(5)
    x = exact_x((2, 24, 24, 3), g, d)
    wt = exact_w((128, 3, 3, 3), g, d)
    bias = exact_bias(128, 27, g, d)
    xp = torch.zeros((2, 24, 24, 64), dtype=torch.float64, device=d)
    xp[..., :3] = x
    e.last_igemm_path()
    y = e.conv2d(_h16(xp), _pack(wt, 64), bias.float(), 128, 3)
    path, _ = check_path("conv_in_pad64", 6)
    check_exact("conv_in_pad64", y, rne16(conv_ref64(x, wt, bias), e.act_dtype()), metric_log, path)


def test_rgb_conv_in_float_exact(metric_log):
    """gp_rgb_conv_in with float input (K = 27 as one MFMA k-step): not a launch_igemm kernel, so the path reads 0"""
    e = _eng()
    d = _dev()
    g = torch.Generator(device=d).manual_seed(6)
    b, h, w, cout = 2, 37, 50, 128
    x = exact_x((b, 3, h, w), g, d)
    wt = exact_w((cout, 3, 3, 3), g, d)
    bias = exact_bias(cout, 27, g, d)
    e.last_igemm_path()
    y = e.rgb_conv_in(x.float(), _pack(wt, 64), bias.float(), cout)
    path, _ = check_path("rgb_conv_in_f32", 0)
    check_exact("rgb_conv_in_f32", y, rne16(conv_ref64(x.permute(0, 2, 3, 1), wt, bias), e.act_dtype()), metric_log, path)


def test_conv_silu_epilogue_interval(metric_log, monkeypatch):
    """SiLU epilogue (silu_f: x * rcp(1 + __expf(-x))): not exactly rounded, so the output must be RNE16 of a value within
    E = |silu(z)| (|z| + 8) 2^-23 of silu64(z) -- __expf's argument scaling costs |z| 2^-24 relative, v_exp / v_rcp / the add and product a
    few 2^-24 more.  The float64 z is exact (exact operands).  Wrong variant: SiLU of the 16-bit-rounded pre-activation."""
    e = _eng()
    d = _dev()
    monkeypatch.setenv("GENPERCEPT_IGEMM_DBG", str(DBG_TR16))
    b, h, w, cin, cout = 2, 20, 36, 128, 128
    x, wt, bias, res, k = _conv_operands(b, h, w, cin, cout, 3, 1.0, True, h, w, cout, 77, d)
    e.last_igemm_path()
    y = e.conv2d(_h16(x), _pack(wt), bias.float(), cout, 3, residual=_h16(res), act="silu", tile=5)
    path, _ = check_path("halo16_silu", 1)
    z = conv_ref64(x, wt, bias) + res
    y64 = z * torch.sigmoid(z)
    eb = y64.abs() * (z.abs() + 8) * 2.0 ** -23
    zr = rne16(z, e.act_dtype()).double()
    _check_interval("halo16_silu", y, y64, eb, metric_log, path, wrong=zr * torch.sigmoid(zr))


# ---- GEMM cases through gp_gemm --------------------------------------------------------------------------------------------------------
def gemm_raw(a, bt, out, m, n, k, bias=None, bias_mode=1, res=None, ldres=0, ldo=None, n_store=0, act="none", out_fp32=0, batch=1, a_bs=0,
             bt_bs=0, out_bs=0, tile=0, n_rows=None):
    e = _eng()
    st = e.load_library().gp_gemm(a.data_ptr(), a.stride(-2), bt.data_ptr(), bt.stride(-2), None if bias is None else bias.data_ptr(), bias_mode,
                                  None if res is None else res.data_ptr(), ldres, out.data_ptr(), ldo or n_store or n, m, n, k, n_rows or n,
                                  n_store or n, e.ACT[act], out_fp32, batch, a_bs, bt_bs, out_bs, tile, torch.cuda.current_stream().cuda_stream)
    assert st == 0, f"gp_gemm failed ({st})"


# (name, M, N, K, tile, residual, n_store, act, out_fp32, env, s, want_path, want_bm)
GEMM_CASES = [
    ("igemm_t1", 1000, 320, 1280, 1, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_t2_ragged", 100, 72, 128, 2, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_t3", 300, 24, 192, 3, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_t4", 4800, 320, 320, 4, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_t4_k2304", 70, 64, 2304, 4, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_auto_small_m", 576, 1280, 320, 0, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_relu", 1000, 256, 512, 1, True, 0, "relu", 0, {}, 1.0, 6, None),
    # direct epilogue: ldo % 8 != 0, and the column zero-fill n_store > N (must store exact zeros)
    ("igemm_direct_n100", 500, 100, 256, 1, True, 0, "none", 0, {}, 1.0, 6, None),
    ("igemm_zero_fill", 300, 130, 256, 4, True, 136, "none", 0, {}, 1.0, 6, None),
    ("igemm_zero_fill_direct", 300, 130, 256, 1, True, 132, "none", 0, {}, 1.0, 6, None),
    # fp32 output (the exact float32 value itself) and fp16 output in either library
    ("igemm_out_fp32", 1000, 320, 1280, 1, False, 0, "none", 1, {}, 1.0, 6, None),
    ("igemm_out_fp16", 1000, 320, 1280, 4, False, 0, "none", 2, {}, 1.0, 6, None),
    # persistent GEMM: 128-row tiles (4-deep ring; several tiles per workgroup, ragged last tile; 5, 40 and 10 K-steps per tile), 256-row tiles
    # (3-deep ring) with a ragged tail
    ("pgemm128_ragged", 4801, 320, 320, 7, True, 0, "none", 0, {}, 1.0, 3, 128),
    ("pgemm128_k2560", 9216, 640, 2560, 7, True, 0, "none", 0, {}, 1.0, 3, 128),
    ("pgemm128_k640", 4801, 320, 640, 7, True, 0, "none", 0, {}, 1.0, 3, 128),
    ("pgemm256_ragged", 200003, 128, 128, 7, True, 0, "none", 0, {}, 1.0, 3, 256),
    ("pgemm_auto_relu", 36864, 320, 320, 0, True, 0, "relu", 0, {}, 1.0, 3, None),
    ("pgemm_zero_fill", 9000, 320, 256, 0, True, 328, "none", 0, {}, 1.0, 3, None),
]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_exact(case, metric_log, monkeypatch):
    e = _eng()
    name, m, n, k, tile, with_res, n_store, act, out_fp32, env, s, want, want_bm = case
    for kname, v in env.items():
        monkeypatch.setenv(kname, v)
    d = _dev()
    nst = n_store or n
    g = torch.Generator(device=d).manual_seed(m + n + k + tile)
    a, bt = exact_x((m, k), g, d), exact_w((n, k), g, d, s)
    bias = exact_bias(n, k, g, d, s)
    res = exact_res((m, nst), k, g, d, s) if with_res else None
    assert worst_sum(k, True, with_res) <= FP32_EXACT
    odt = {0: e.act_dtype(), 1: torch.float32, 2: torch.float16}[out_fp32]
    out = torch.full((m, nst), float("nan"), dtype=odt, device=d)
    e.last_igemm_path()
    gemm_raw(_h16(a), _h16(bt), out, m, n, k, bias=bias.float(), res=_h16(res) if with_res else None, ldres=nst, n_store=nst, act=act,
             out_fp32=out_fp32, tile=tile)
    path, bm = check_path(name, want, want_bm)
    ref = a @ bt.t() + bias
    if with_res:
        ref = ref + res[:, :n]
    if act == "relu":
        ref = ref.clamp_min(0)
    exp = torch.zeros((m, nst), dtype=odt, device=d)
    exp[:, :n] = ref.float() if out_fp32 == 1 else rne16(ref, odt)
    if out_fp32 == 1:
        assert torch.equal(exp[:, :n].double(), ref)
    check_exact(name, out, exp, metric_log, path, bm)


@pytest.mark.parametrize("tile", [1, 7])
def test_gemm_residual_in_place_exact(tile, metric_log):
    """out = A Bt^T + bias + out (residual == output buffer, the engine's trunk updates)"""
    e = _eng()
    d = _dev()
    m, n, k = 4801, 320, 640
    g = torch.Generator(device=d).manual_seed(11 + tile)
    a, bt, bias = exact_x((m, k), g, d), exact_w((n, k), g, d), None
    bias = exact_bias(n, k, g, d)
    res = exact_res((m, n), k, g, d)
    out = _h16(res)
    e.last_igemm_path()
    gemm_raw(_h16(a), _h16(bt), out, m, n, k, bias=bias.float(), res=out, ldres=n, tile=tile)
    path, bm = check_path(f"gemm_res_inplace_t{tile}", 6 if tile == 1 else 3)
    check_exact(f"gemm_res_inplace_t{tile}", out, rne16(a @ bt.t() + bias + res, e.act_dtype()), metric_log, path, bm)


def test_gemm_batched_row_bias_exact(metric_log):
    """the V^T projection form: out[b][c][t] = sum_k W[c][k] x[b][t][k] + bias[c] (row bias, shared A), zero-filled to Tpad columns"""
    e = _eng()
    d = _dev()
    bsz, t, c, tpad = 3, 100, 128, 128
    g = torch.Generator(device=d).manual_seed(3)
    wv, x = exact_w((c, c), g, d), exact_x((bsz, t, c), g, d)
    bias = exact_bias(c, c, g, d)
    out = torch.full((bsz, c, tpad), 7.0, dtype=e.act_dtype(), device=d)
    e.last_igemm_path()
    gemm_raw(_h16(wv), _h16(x), out, c, t, c, bias=bias.float(), bias_mode=2, ldo=tpad, n_store=tpad, batch=bsz, a_bs=0, bt_bs=t * c,
             out_bs=c * tpad, n_rows=t)
    path, _ = check_path("bgemm_rowbias", 6)
    exp = torch.zeros_like(out)
    exp[:, :, :t] = rne16(torch.einsum("ck,btk->bct", wv, x) + bias[None, :, None], e.act_dtype())
    check_exact("bgemm_rowbias", out, exp, metric_log, path)


@pytest.mark.parametrize("case", [(4, 576, 320), (2, 2304, 640), (1, 400, 64), (3, 272, 128), (4, 144, 1280)])
def test_gemm_qkv_exact(case, metric_log):
    """gp_gemm_qkv: q | k row-major and V^T [B][C][Tpad] with zeros beyond T, one persistent-GEMM launch"""
    e = _eng()
    d = _dev()
    b, t, c = case
    g = torch.Generator(device=d).manual_seed(b * 1000 + t + c)
    x, w = exact_x((b * t, c), g, d), exact_w((3 * c, c), g, d)
    wp = _pack(w)
    e.last_igemm_path()
    qk, vt = e.gemm_qkv(_h16(x), wp.reshape(wp.shape[0], -1), b, t, c)
    path, bm = check_path(f"qkv{case}", 3)
    ref = rne16(x @ w.t(), e.act_dtype())
    check_exact(f"qkv_qk{case}", qk, ref[:, :2 * c], metric_log, path, bm)
    vexp = torch.zeros_like(vt)
    vexp[:, :, :t] = ref[:, 2 * c:].reshape(b, t, c).permute(0, 2, 1)
    check_exact(f"qkv_vt{case}", vt, vexp, metric_log, path, bm)


@pytest.mark.parametrize("mc", [(200, 128), (4801, 128), (2304, 64)])
def test_gemm_geglu_interval(mc, metric_log):
    """GEGLU epilogue: hidden * gelu_erf_f(gate), erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7).  Bound per element, with h, a the
    exact pre-activations: E = |h| (|a|/2 (1.5e-7 + E_t (a^2/2 + 10) 2^-23) + |gelu(a)| 2^-23) + |y| 2^-23 -- the erf approximation as an
    absolute term in |a|, the fp32 steps of its evaluation (the exp2 argument a^2/2 log2 e, the rcp, the polynomial) relative to the tail
    E_t = 1 - erf(|a|/sqrt 2), the two products.  The tanh form of GELU (|difference| up to ~2e-4 |h|) must fall outside on >= 2 % of elements."""
    m, c = mc
    _geglu_interval(f"geglu{mc}", m, c, 4 + m, metric_log, 6 if m < 256 else 3, None)


def _geglu_interval(name, m, c, seed, log, want_path, want_bm):
    """GEGLU projection [m, c] x [8c, c]^T (+ bias) -> hidden * gelu(gate), [m, 4c], under the bound of test_gemm_geglu_interval"""
    e = _eng()
    d = _dev()
    g = torch.Generator(device=d).manual_seed(seed)
    a, w = exact_x((m, c), g, d), exact_w((8 * c, c), g, d, 4.0)
    bias = exact_bias(8 * c, c, g, d, 4.0)
    assert worst_sum(c, True, False) <= FP32_EXACT
    half = 4 * c
    idx = torch.arange(8 * c)
    r = torch.where(idx >= half, idx - half, idx)
    dst = (r // 16) * 32 + ((r % 16) // 4) * 8 + (idx >= half).long() * 4 + (r % 4)
    pb = torch.empty_like(bias)
    pb[dst.to(d)] = bias
    e.last_igemm_path()
    y = e.conv2d(_h16(a).reshape(1, 1, m, c), _pack(w, geglu=True), pb.float(), 8 * c, 1, act="geglu").reshape(m, half)
    path, bm = check_path(name, want_path, want_bm)
    proj = a @ w.t() + bias
    hdn, gate = proj[:, :half], proj[:, half:]
    tail = torch.special.erfc(gate.abs() / math.sqrt(2))
    gel = 0.5 * gate * (1 + torch.special.erf(gate / math.sqrt(2)))
    y64 = hdn * gel
    eb = hdn.abs() * (0.5 * gate.abs() * (1.5e-7 + tail * (gate * gate / 2 + 10) * 2.0 ** -23) + gel.abs() * 2.0 ** -23) + y64.abs() * 2.0 ** -23
    tanh_gelu = 0.5 * gate * (1 + torch.tanh(math.sqrt(2 / math.pi) * (gate + 0.044715 * gate ** 3)))
    _check_interval(name, y, y64, eb, log, path, wrong=hdn * tanh_gelu, bm=bm)


def test_round_half_even_ties_exact(metric_log, monkeypatch):
    """tie-heavy: integer operands |x|, |w| <= 3 and a bias of 1.5 * 2^P (P = 8 bf16, 11 fp16) put most outputs in [2^P, 2^(P+1)), one bit
    wider than the element type -- every odd output is a tie that round-half-to-even decides (about half of them); GEMM and halo conv."""
    e = _eng()
    d = _dev()
    p = 8 if e.act_dtype() == torch.bfloat16 else 11
    g = torch.Generator(device=d).manual_seed(99)
    m, n, k = 4096, 256, 128
    a, bt = exact_x((m, k), g, d, lim=3, q=1.0), exact_x((n, k), g, d, lim=3, q=1.0)
    bias = torch.full((n,), 1.5 * 2 ** p, dtype=torch.float64, device=d)
    for tile, want in ((1, 6), (7, 3)):
        out = torch.empty((m, n), dtype=e.act_dtype(), device=d)
        e.last_igemm_path()
        gemm_raw(_h16(a), _h16(bt), out, m, n, k, bias=bias.float(), tile=tile)
        path, bm = check_path(f"ties_gemm_t{tile}", want)
        ref = a @ bt.t() + bias
        ties = int(((ref.abs() >= 2 ** p) & (ref.abs() < 2 ** (p + 1)) & (ref.remainder(2) == 1)).sum())
        assert ties > m * n // 8, ties
        check_exact(f"ties_gemm_t{tile}", out, rne16(ref, e.act_dtype()), metric_log, path, bm, ties=ties)
    x, wt = exact_x((1, 40, 36, 128), g, d, lim=1, q=1.0), exact_x((128, 128, 3, 3), g, d, lim=1, q=1.0)
    cb = torch.full((128,), 1.5 * 2 ** p, dtype=torch.float64, device=d)
    monkeypatch.setenv("GENPERCEPT_IGEMM_DBG", str(DBG_TR16))
    e.last_igemm_path()
    y = e.conv2d(_h16(x), _pack(wt), cb.float(), 128, 3, tile=5)
    path, _ = check_path("ties_halo", 1)
    check_exact("ties_halo", y, rne16(conv_ref64(x, wt, cb), e.act_dtype()), metric_log, path)


# ---- headline configuration: the distinct conv / GEMM launches of one 768 x 768, batch-4 pass (bf16 engine), written as the engine's launch
# log describes them (op, kernel, M = output pixels or rows, N = output columns, K = reduction length, flags).  Every launch of that log
# through launch_igemm is here except two kinds: "conv3x3 halo+gn+silu" (the GroupNorm + SiLU fused into the input staging is not
# expressible with exact operands; the three shapes M=2359296 N=128 K=1152 / K=2304 run below with a plain input and the same epilogue flags)
# and the tails outside launch_igemm (rgb_conv_in, conv_few, post_quant_conv).  "+stats" runs through gp_conv2d_stats / gp_conv2d_up2_stats
# and also checks the GroupNorm scale / shift the epilogue leaves; the stride-2 "+stats" launches run through gp_conv2d without statistics
# (the statistics entry has no stride), which stores the same tensor.  "geglu" runs the interval check of test_gemm_geglu_interval.
# N = 4 convs store into the 64-channel latent layout.
# (launch, path): path as gp_last_igemm_path reports it, with the persistent GEMM's row tile as (3, rows)
HEADLINE_LAUNCHES = [
    ("bgemm igemm M=512 N=9216 K=512 batch=4", 6),
    ("conv3x3 halo M=147456 N=512 K=2304 +stats", 1),
    ("conv3x3 halo M=147456 N=512 K=4608 +res +stats", 1),
    ("conv3x3 halo M=147456 N=512 K=4608 +stats", 1),
    ("conv3x3 halo M=2359296 N=128 K=1152 +res +stats", 1),
    ("conv3x3 halo M=2359296 N=128 K=1152 +stats", 1),
    ("conv3x3 halo M=2359296 N=128 K=2304 +stats", 1),
    ("conv3x3 halo M=36864 N=320 K=2880 +res +stats", 1),
    ("conv3x3 halo M=36864 N=320 K=2880 +stats", 1),
    ("conv3x3 halo M=36864 N=320 K=576 +stats", 1),
    ("conv3x3 halo M=36864 N=320 K=5760 +stats", 1),
    ("conv3x3 halo M=36864 N=320 K=8640 +stats", 1),
    ("conv3x3 halo M=36864 N=512 K=4608 +res +stats", 7),
    ("conv3x3 halo M=36864 N=512 K=4608 +stats", 7),
    ("conv3x3 halo M=36864 N=512 K=576 +stats", 7),
    ("conv3x3 halo M=589824 N=256 K=1152 +stats", 1),
    ("conv3x3 halo M=589824 N=256 K=2304 +res +stats", 1),
    ("conv3x3 halo M=589824 N=256 K=2304 +stats", 1),
    ("conv3x3 halo M=589824 N=256 K=4608 +stats", 1),
    ("conv3x3 halo M=9216 N=640 K=11520 +stats", 7),
    ("conv3x3 halo M=9216 N=640 K=17280 +stats", 7),
    ("conv3x3 halo M=9216 N=640 K=2880 +stats", 7),
    ("conv3x3 halo M=9216 N=640 K=5760 +res +stats", 7),
    ("conv3x3 halo M=9216 N=640 K=5760 +stats", 7),
    ("conv3x3 halo M=9216 N=640 K=8640 +stats", 7),
    ("conv3x3 igemm M=2304 N=1280 K=11520", 4),
    ("conv3x3 igemm M=2304 N=1280 K=11520 +res", 4),
    ("conv3x3 igemm M=2304 N=1280 K=17280", 4),
    ("conv3x3 igemm M=2304 N=1280 K=23040", 4),
    ("conv3x3 igemm M=2304 N=1280 K=5760", 4),
    ("conv3x3 igemm M=36864 N=4 K=2880", 6),
    ("conv3x3 igemm M=36864 N=4 K=4608", 6),
    ("conv3x3 igemm M=576 N=1280 K=11520", 4),
    ("conv3x3 igemm M=576 N=1280 K=11520 +res", 4),
    ("conv3x3 igemm M=576 N=1280 K=23040", 4),
    ("conv3x3s2 igemm M=147456 N=256 K=2304 +stats", 6),
    ("conv3x3s2 igemm M=2304 N=640 K=5760", 5),
    ("conv3x3s2 igemm M=36864 N=512 K=4608 +stats", 6),
    ("conv3x3s2 igemm M=576 N=1280 K=11520", 5),
    ("conv3x3s2 igemm M=589824 N=128 K=1152 +stats", 6),
    ("conv3x3s2 igemm M=9216 N=320 K=2880 +stats", 6),
    ("conv3x3up halo M=147456 N=512 K=4608 +stats", 2),
    ("conv3x3up halo M=2304 N=1280 K=11520", 2),
    ("conv3x3up halo M=2359296 N=256 K=2304 +stats", 2),
    ("conv3x3up halo M=36864 N=640 K=5760", 2),
    ("conv3x3up halo M=589824 N=512 K=4608 +stats", 2),
    ("conv3x3up halo M=9216 N=1280 K=11520", 2),
    ("gemm igemm M=576 N=1280 K=1280", 6),
    ("gemm igemm M=576 N=1280 K=1280 +res", 6),
    ("gemm igemm M=576 N=1280 K=2560", 6),
    ("gemm igemm M=576 N=1280 K=5120 +res", 6),
    ("gemm pgemm M=147456 N=512 K=256", (3, 256)),
    ("gemm pgemm M=2304 N=10240 K=1280 geglu", (3, 256)),
    ("gemm pgemm M=2304 N=1280 K=1280", (3, 128)),
    ("gemm pgemm M=2304 N=1280 K=1280 +res", (3, 128)),
    ("gemm pgemm M=2304 N=1280 K=1920", (3, 128)),
    ("gemm pgemm M=2304 N=1280 K=2560", (3, 128)),
    ("gemm pgemm M=2304 N=1280 K=5120 +res", (3, 128)),
    ("gemm pgemm M=2304 N=1280 K=640", (3, 128)),
    ("gemm pgemm M=2304 N=3840 K=1280 q|k|vT", (3, 128)),
    ("gemm pgemm M=2359296 N=128 K=256", (3, 256)),
    ("gemm pgemm M=36864 N=1024 K=512", (3, 256)),
    ("gemm pgemm M=36864 N=2560 K=320 geglu", (3, 256)),
    ("gemm pgemm M=36864 N=320 K=1280 +res", (3, 128)),
    ("gemm pgemm M=36864 N=320 K=320", (3, 128)),
    ("gemm pgemm M=36864 N=320 K=320 +res", (3, 128)),
    ("gemm pgemm M=36864 N=320 K=320 +res +stats", (3, 128)),
    ("gemm pgemm M=36864 N=320 K=640", (3, 128)),
    ("gemm pgemm M=36864 N=320 K=960", (3, 128)),
    ("gemm pgemm M=36864 N=512 K=512 +res +stats", (3, 128)),
    ("gemm pgemm M=36864 N=960 K=320 q|k|vT", (3, 256)),
    ("gemm pgemm M=576 N=10240 K=1280 geglu", (3, 128)),
    ("gemm pgemm M=576 N=3840 K=1280 q|k|vT", (3, 128)),
    ("gemm pgemm M=589824 N=256 K=128", (3, 256)),
    ("gemm pgemm M=589824 N=256 K=512", (3, 256)),
    ("gemm pgemm M=9216 N=1920 K=640 q|k|vT", (3, 128)),
    ("gemm pgemm M=9216 N=5120 K=640 geglu", (3, 256)),
    ("gemm pgemm M=9216 N=640 K=1280", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=1920", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=2560 +res", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=320", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=640", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=640 +res", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=640 +res +stats", (3, 128)),
    ("gemm pgemm M=9216 N=640 K=960", (3, 128)),
]


def parse_launch(desc):
    """'conv3x3up halo M=147456 N=512 K=4608 +stats' -> (op, {M, N, K, batch}, flags)"""
    words = desc.split()
    kv = {w.split("=")[0]: int(w.split("=")[1]) for w in words if "=" in w}
    return words[0], kv, set(w for w in words[2:] if "=" not in w)


def _side(pixels_per_image):
    s = math.isqrt(pixels_per_image)
    assert s * s == pixels_per_image
    return s


def _stats_check(name, y, scale, shift, b, cout, log, groups=32, eps=1e-6):
    """scale / shift (gamma = 1, beta = 0) against float64 statistics of exactly the tensor stored"""
    yg = y.double().reshape(b, -1, groups, cout // groups).permute(0, 2, 1, 3).reshape(b, groups, -1)
    mean, var = yg.mean(dim=2), yg.var(dim=2, unbiased=False)
    sc = (var + eps).rsqrt().repeat_interleave(cout // groups, dim=1)
    sh = -mean.repeat_interleave(cout // groups, dim=1) * sc
    e_sc = float(((scale.double() - sc).abs() / sc.abs().clamp_min(1e-3)).max())
    e_sh = float((shift.double() - sh).abs().max())
    log(_tag(f"stats[{name}]"), scale_rel=e_sc, shift_abs=e_sh)
    assert e_sc < 2e-4 and e_sh < 2e-4, (name, e_sc, e_sh)


@pytest.mark.parametrize("case", HEADLINE_LAUNCHES, ids=[c[0] for c in HEADLINE_LAUNCHES])
def test_headline_launch_exact(case, metric_log):
    """auto tile selection (hint 0), as the engine launches these shapes; every output element compared"""
    e = _eng()
    name, want = case
    op, kv, flags = parse_launch(name)
    want_path, want_bm = want if isinstance(want, tuple) else (want, None)
    m, n, k = kv["M"], kv["N"], kv["K"]
    b = 4
    with_res, stats = "+res" in flags, "+stats" in flags
    d = _dev()
    g = torch.Generator(device=d).manual_seed(zlib.crc32(name.encode()))
    dt = e.act_dtype()
    ones, zeros = torch.ones(n, device=d), torch.zeros(n, device=d)
    scale = shift = None
    if op.startswith("conv3x3"):
        cin = k // 9
        ho = wo = _side(m // b)
        if op == "conv3x3up":
            hi = ho // 2
        elif op == "conv3x3s2":
            hi = 2 * ho
        else:
            hi = ho
        nst = 64 if n == 4 else n
        x, wt, bias, res, kk = _conv_operands(b, hi, hi, cin, n, 3, 1.0, with_res, ho, wo, nst, zlib.crc32(name.encode()) % 100003, d)
        assert worst_sum(kk, True, with_res) <= FP32_EXACT
        xd, wp = _h16(x), _pack(wt)
        resd = _h16(res) if with_res else None
        e.last_igemm_path()
        if op == "conv3x3up":
            wph = e.pack_weight_phases(wt.float().cpu(), device=d)
            if stats:
                y, scale, shift = e.conv2d_up2_stats(xd, wp, wph, bias.float(), n, ones, zeros, 32, 1e-6, residual=resd)
            else:
                y = e.conv2d_up2(xd, wp, wph, bias.float(), n, residual=resd)
            ref = conv_ref64(x, wt, bias, ups_hw=(ho, wo))
        elif op == "conv3x3s2":
            pad = (0, 0) if n in (128, 256, 512) else (1, 1)   # VAE encoder Downsample2D pads right / bottom only, the UNet's pads 1
            y = _conv_prefilled(xd, wp, bias.float(), n, 3, b, ho, wo, n, stride=2, pad=pad)
            ref = conv_ref64(x, wt, bias, 2, pad, (ho, wo))
        elif stats:
            y, scale, shift = e.conv2d_stats(xd, wp, bias.float(), n, 3, ones, zeros, 32, 1e-6, residual=resd)
            ref = conv_ref64(x, wt, bias)
        else:
            y = _conv_prefilled(xd, wp, bias.float(), n, 3, b, ho, wo, nst, residual=resd)
            ref = conv_ref64(x, wt, bias)
        path, bm = check_path(name, want_path, want_bm)
        del xd, wp
        if with_res:
            ref += res[..., :n]
        exp = torch.zeros((b, ho, wo, nst), dtype=dt, device=d)
        exp[..., :n] = rne16(ref, dt)
        del ref
    elif "q|k|vT" in flags:
        c = k
        t = m // b
        x, wq = exact_x((m, c), g, d), exact_w((3 * c, c), g, d)
        wp = _pack(wq)
        e.last_igemm_path()
        qk, vt = e.gemm_qkv(_h16(x), wp.reshape(wp.shape[0], -1), b, t, c)
        path, bm = check_path(name, want_path, want_bm)
        ref = rne16(x @ wq.t(), dt)
        vexp = torch.zeros_like(vt)
        vexp[:, :, :t] = ref[:, 2 * c:].reshape(b, t, c).permute(0, 2, 1)
        check_exact(name + " vT", vt, vexp, metric_log, path, bm)
        y, exp = qk, ref[:, :2 * c]
    elif "geglu" in flags:
        _geglu_interval(name, m, k, zlib.crc32(name.encode()), metric_log, want_path, want_bm)
        return
    elif op == "bgemm":   # out[b][c][t] = W[c][k] x[b][t][k] + bias[c]
        t, c = n, m
        wv, x = exact_w((c, k), g, d), exact_x((b, t, k), g, d)
        bias = exact_bias(c, k, g, d)
        y = torch.full((b, c, t), float("nan"), dtype=dt, device=d)
        e.last_igemm_path()
        gemm_raw(_h16(wv), _h16(x), y, c, t, k, bias=bias.float(), bias_mode=2, ldo=t, n_store=t, batch=b, bt_bs=t * k, out_bs=c * t, n_rows=t)
        path, bm = check_path(name, want_path, want_bm)
        exp = rne16(torch.einsum("ck,btk->bct", wv, x) + bias[None, :, None], dt)
    else:   # gemm: M rows of K -> N columns (+ column bias, + residual)
        a, bt = exact_x((m, k), g, d), exact_w((n, k), g, d)
        bias = exact_bias(n, k, g, d)
        res = exact_res((m, n), k, g, d) if with_res else None
        assert worst_sum(k, True, with_res) <= FP32_EXACT
        e.last_igemm_path()
        if stats:   # the 1x1 conv form of the same GEMM: B images of M / B pixels, with the statistics epilogue
            hw = _side(m // b)
            y, scale, shift = e.conv2d_stats(_h16(a).reshape(b, hw, hw, k), _pack(bt), bias.float(), n, 1, ones, zeros, 32, 1e-6,
                                             residual=_h16(res).reshape(b, hw, hw, n) if with_res else None)
            y = y.reshape(m, n)
        else:
            y = torch.full((m, n), float("nan"), dtype=dt, device=d)
            gemm_raw(_h16(a), _h16(bt), y, m, n, k, bias=bias.float(), res=_h16(res) if with_res else None, ldres=n)
        path, bm = check_path(name, want_path, want_bm)
        ref = a @ bt.t() + bias
        if with_res:
            ref += res
        exp = rne16(ref, dt)
    check_exact(name, y, exp, metric_log, path, bm)
    if scale is not None:
        _stats_check(name, y, scale, shift, b, n, metric_log)
