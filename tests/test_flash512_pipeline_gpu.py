"""flash_attn512_kernel (attention.hip) after its P.V phase was pipelined: the paths that change touched, at the smallest shapes that reach them.

The kernel is called through engine.flash_attention_hd512(q, k, vt, scale, ncu) with both element-type libraries and compared with fp32 torch
attention on the same 16-bit-rounded operands, with the tolerance of test_kernels_gpu.py::test_flash_attention_hd512 (its `check`, same
mean_factor: the rounding of the stored result alone is the generic mean gate, see the comment there).  `ncu` sizes the launch, so the shapes
stay tiny:

  (1, 32, 1)    one tile: the V^T fragments requested under the softmax have nothing before them; the only tile is also the last one (its
                sixteen DMA pieces go through the empty buffer resource)
  (1, 33, 1)    one full tile, then a last tile with one valid key
  (1, 64, 0)    two tiles, never cut along the keys
  (2, 300, 2)   6 query blocks on 2 workgroups: whole rounds only, three items per workgroup -- the hand-allocated accumulators are zeroed,
                filled, read out and zeroed again; the item barrier and the DMA drain between items
  (2, 300, 4)   one round + 2 left-over blocks in 2 key parts each, merged by the combine kernel
  (1, 1131, 4)  two rounds + 1 left-over block in 4 key parts

Every case also asserts that two calls give bitwise equal outputs and that the flipped batch gives the flipped result, bit for bit.
"""
import pytest
import torch

from test_kernels_gpu import _dev, _eng, check, precision, rbf  # noqa: F401  (precision: autouse, both libraries)

pytestmark = pytest.mark.gpu

C = 512
CASES = [(1, 32, 1), (1, 33, 1), (1, 64, 0), (2, 300, 2), (2, 300, 4), (1, 1131, 4)]


def _run(q, k, v, scale, ncu):
    """q, k, v: fp32 CPU tensors holding 16-bit-representable values -> the kernel's output (device tensor)"""
    e, d = _eng(), _dev()
    b, t, _ = q.shape
    tpad = (t + 63) // 64 * 64
    vt = torch.zeros(b, C, tpad, dtype=e.act_dtype(), device=d)
    vt[:, :, :t] = v.transpose(1, 2).to(d).to(e.act_dtype())
    qk = torch.cat([q, k], dim=-1).to(d).to(e.act_dtype())          # row stride 1024, as the engine's fused q/k projection gives it
    return e.flash_attention_hd512(qk[..., :C], qk[..., C:], vt, scale, ncu)


def _check_all(name, q, k, v, scale, ncu, log):
    ref = torch.softmax((q @ k.transpose(1, 2)) * scale, dim=-1) @ v
    y = _run(q, k, v, scale, ncu)
    check(name, y, ref, log, mean_factor=1.25)
    assert torch.equal(_run(q, k, v, scale, ncu), y), f"{name}: two calls differ"
    y_flipped = _run(q.flip(0), k.flip(0), v.flip(0), scale, ncu)
    assert torch.equal(y_flipped.flip(0), y), f"{name}: the flipped batch does not give the flipped result"


@pytest.mark.parametrize("case", CASES)
def test_flash512_pipeline(case, metric_log):
    b, t, ncu = case
    g = torch.Generator().manual_seed(1000 * b + t + ncu)
    q, k, v = (rbf(torch.randn(b, t, C, generator=g)) for _ in range(3))
    _check_all(f"flash512_pipeline{case}", q, k, v, 2.5 / C ** 0.5, ncu, metric_log)   # logits of std 2.5, as test_flash_attention_hd512


@pytest.mark.parametrize("ncu", [2, 4])
def test_flash512_pipeline_growing_logits(ncu, metric_log):
    """Logits that grow along the keys in steps of about 16 in log2 units (the lazy-rescale threshold is 8): every query's reference maximum
    moves in tile 0 (always), in tile 2 -- the middle of the item, with accumulated P.V behind it and V^T fragments already requested under the
    softmax -- and in tile 8, the item's last tile, which is also masked (T = 278: keys 256 .. 277).  ncu = 2: 6 query blocks as three whole
    items per workgroup; ncu = 4: one round + 2 left-over blocks in 2 key parts (tiles 0-3 and 4-8), whose maxima differ by the same steps
    in the combine kernel (one block per image is cut, so the flipped batch still gives the flipped result).

    q = noise + ones, k_j = noise + s_j / 16 * ones: q.k_j gains 32 s_j (+- 1.4 s_j), times scale = 512^-1/2 and log2(e) that is 2.04 s_j in
    log2 units, on top of logits of std 1.4; s = 0, 8, 16 for tiles 0-1, 2-7, 8."""
    b, t = 2, 278
    g = torch.Generator().manual_seed(17)
    ones = torch.ones(C)
    q = rbf(torch.randn(b, t, C, generator=g) + ones)
    tile = torch.arange(t) // 32
    s = torch.where(tile < 2, 0.0, torch.where(tile < 8, 8.0, 16.0))
    k = rbf(torch.randn(b, t, C, generator=g) + s[None, :, None] / 16 * ones)
    v = rbf(torch.randn(b, t, C, generator=g))
    _check_all(f"flash512_pipeline_growing[ncu={ncu}]", q, k, v, 1.0 / C ** 0.5, ncu, metric_log)
