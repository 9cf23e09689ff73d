"""Test-time ensembling on the device (csrc/ensemble.hip through engine.ensemble_gather / engine.ensemble_reduce and the device route of
genpercept_amd.ensemble): against the reference's own outputs (tests/golden/ensemble_ref.npz), bitwise against the framework ops the kernels
replace (median path, gather), against float64 within the forward-error bound of the fp32 arithmetic (mean path), batch independence, and the
pipeline on top.  Every map is a few thousand pixels at most."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (3, 5), (37, 53), (64, 64)]
U = 2.0 ** -24  # unit roundoff of fp32


def _members(e, h, w, seed=0):
    g = torch.Generator().manual_seed(1000 * e + 10 * h + w + seed)
    return torch.rand((e, 1, h, w), generator=g) * 2.0 + 0.25


def _params(e):
    """fixed fp32 (s, t) per member; the middle member's scale is negative (it reverses the order)"""
    s = torch.linspace(0.6, 1.9, e) if e > 1 else torch.tensor([0.8])
    s[e // 2] = -s[e // 2]
    t = torch.linspace(-0.3, 0.4, e) if e > 1 else torch.tensor([0.1])
    return s.float(), t.float()


def _framework_median(maps, s, t):
    """What ensemble.py computes on CPU tensors after the optimiser: maps [E,1,H,W] * s + t, median(dim=0), the second median for the
    uncertainty, min / max, clamp, divide.  t None: scale-only (d_min = 0)."""
    n = maps.shape[0]
    al = maps * s.view(n, 1, 1, 1) + t.view(n, 1, 1, 1) if t is not None else maps * s.view(n, 1, 1, 1)
    pred = al.median(dim=0, keepdim=True).values
    unc = (al - pred).abs().median(dim=0, keepdim=True).values
    d_max = pred.max()
    d_min = pred.min() if t is not None else 0
    rng = (d_max - d_min).clamp(min=1e-6)
    return (pred - d_min) / rng, unc / rng


def _device_median(maps, s, t, dev_maps=None):
    from genpercept_amd import engine
    d = maps[:, 0][None].cuda() if dev_maps is None else dev_maps
    pred, unc = engine.ensemble_reduce(d, s[None], None if t is None else t[None], "median", True)
    torch.cuda.synchronize()
    return pred.cpu()[None], unc.cpu()[None]


def _assert_median_bitwise(maps, s, t, dev_maps=None):
    ref_p, ref_u = _framework_median(maps, s, t)
    pred, unc = _device_median(maps, s, t, dev_maps)
    assert pred.shape == ref_p.shape and unc.shape == ref_u.shape
    assert torch.equal(pred, ref_p), float((pred - ref_p).abs().max())
    assert torch.equal(unc, ref_u), float((unc - ref_u).abs().max())


def _count_calls(monkeypatch, name):
    from genpercept_amd import engine
    real, calls = getattr(engine, name), []

    def wrapper(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)

    monkeypatch.setattr(engine, name, wrapper)
    return calls


# 1. against the reference -------------------------------------------------------------------------------------------------------------
def test_device_route_equals_the_reference(monkeypatch):
    from genpercept_amd.ensemble import ensemble_depth
    monkeypatch.delenv("GENPERCEPT_HOST_ENSEMBLE", raising=False)
    calls = _count_calls(monkeypatch, "ensemble_reduce")
    g = np.load(os.path.join(GOLD, "ensemble_ref.npz"))
    cases = [str(c) for c in g["cases"]]
    assert sorted(g[c + "/in"].shape[0] for c in cases) == [1, 3, 4, 5, 5, 6, 7]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy's finite differences on the fp32 parameter vector the reference hands it
        for i, c in enumerate(cases):
            kw = {"shift_invariant": True, **json.loads(str(g[c + "/kw"]))}
            pred, unc = ensemble_depth(torch.from_numpy(g[c + "/in"]).cuda(), scale_invariant=True, max_res=50, **kw)
            assert len(calls) == i + 1, "the device route was not taken"
            assert pred.is_cuda and pred.shape == (1, 1, 40, 48)
            err = float(np.abs(pred.cpu().numpy() - g[c + "/pred"]).max())
            print(f"{c}: max|pred - golden| = {err:.3e}")
            assert err <= 1e-6, c
            assert (unc is not None) == (c + "/unc" in g.files)
            if unc is not None:
                erru = float(np.abs(unc.cpu().numpy() - g[c + "/unc"]).max())
                print(f"{c}: max|unc - golden| = {erru:.3e}")
                assert erru <= 1e-6, c


# 2. bitwise against the framework ops, median -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [1, 2, 3, 4, 5, 16, 17, 33])
@pytest.mark.parametrize("h,w", SHAPES)
def test_median_is_bitwise_the_framework_ops(h, w, e):
    _assert_median_bitwise(_members(e, h, w), *_params(e))


@pytest.mark.parametrize("e", [4, 5, 16, 17])
def test_median_tie_break_on_duplicated_values(e):
    """members quantised to 1/8 steps, scales +-1 / 2 and shifts in 1/8 steps: the aligned values (and their deviations) tie at many pixels"""
    maps = (_members(e, 37, 53, seed=7) * 8).round() / 8
    s = torch.tensor([1.0, -1.0, 2.0, 1.0] * 9)[:e]
    t = torch.tensor([0.0, 3.0, -1.5, 0.125] * 9)[:e]
    al = maps * s.view(e, 1, 1, 1) + t.view(e, 1, 1, 1)
    srt = al.sort(dim=0).values
    assert float((srt[1:] == srt[:-1]).any(dim=0).float().mean()) > 0.2  # ties at more than a fifth of the pixels (E = 4; nearly all at E >= 16)
    _assert_median_bitwise(maps, s, t)


@pytest.mark.parametrize("e", [3, 17])
def test_median_constant_maps_clamp_the_range(e):
    maps = torch.linspace(0.2, 0.9, e).view(e, 1, 1, 1).expand(e, 1, 37, 53).contiguous()
    s, t = torch.ones(e), torch.zeros(e)
    pred, unc = _device_median(maps, s, t)
    assert float(pred.abs().max()) == 0.0 and float(unc.max()) > 1e4  # pred - d_min = 0; the deviations are divided by rng = 1e-6
    _assert_median_bitwise(maps, s, t)


@pytest.mark.parametrize("e", [4, 17])
def test_median_scale_only(e):
    maps, (s, _) = _members(e, 37, 53, seed=3), _params(e)
    _assert_median_bitwise(maps, s.abs(), None)
    pred, _ = _device_median(maps, s.abs(), None)
    assert float(pred.max()) == 1.0 and float(pred.min()) > 0.0  # d_min = 0: the minimum is not moved to 0
    _assert_median_bitwise(maps, s, None)


@pytest.mark.parametrize("e", [5, 17])
def test_median_on_a_base_pointer_offset_by_one_float(e):
    """the members start 4 bytes past a 16-byte boundary: scalar loads of the same values"""
    maps = _members(e, 64, 64, seed=5)
    buf = torch.empty((maps.numel() + 1,), dtype=torch.float32, device="cuda")
    dev = buf[1:].view(1, e, 64, 64)
    dev.copy_(maps[:, 0][None])
    assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    _assert_median_bitwise(maps, *_params(e), dev_maps=dev)


# 3. mean / standard deviation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2, 3, 8, 17])
@pytest.mark.parametrize("h,w", SHAPES)
def test_mean_and_std_within_the_fp32_forward_error(h, w, e):
    """Against float64 on the fp32-aligned members.  With u = 2^-24, M = max|a|, the true range rng (clamped at 1e-6 like the kernel's):
    pred: a recursive fp32 sum of E terms has forward error <= (E - 1) u sum|a_i| <= (E - 1) u E M; the division by E adds u M: E u M on the
      mean.  Subtracting d_min, dividing by rng and the rounding of rng itself add three more roundings of values <= M: (E + 3) u M / rng.
    uncertainty: std = sqrt(sum d_i^2 / (E - 1)), d_i = a_i - mean.  Each computed d_i is off by at most the mean's E u M plus its own rounding
      u |d_i| <= 2 u M: delta = (E + 2) u M, which moves the 2-norm of d by <= sqrt(E) delta and so std by <= sqrt(E / (E - 1)) delta.  The E
      squares, their recursive sum, the division and the square root are E + 3 roundings of positive terms, halved by the root: a relative
      (E + 3) / 2 u of std.  The final division by rng adds a relative u plus rng's own relative error: rng = d_max - d_min, each end off by
      E u M, one rounding: 2 E u M / rng + u."""
    from genpercept_amd import engine
    maps, (s, t) = _members(e, h, w, seed=11), _params(e)
    al = (maps * s.view(e, 1, 1, 1) + t.view(e, 1, 1, 1)).double()  # the fp32-aligned members
    mean, std = al.mean(dim=0), al.std(dim=0)
    d_min, d_max = mean.min(), mean.max()
    rng = float((d_max - d_min).clamp(min=1e-6))
    ref_p, ref_u = (mean - d_min) / rng, std / rng
    pred, unc = engine.ensemble_reduce(maps[:, 0][None].cuda(), s[None], t[None], "mean", True)
    pred, unc = pred.cpu().double(), unc.cpu().double()
    m = float(al.abs().max())
    bound_p = (e + 3) * U * m / rng
    err_p = float((pred - ref_p).abs().max())
    delta = (e + 2) * U * m
    rel_rng = 2 * e * U * m / rng + U
    bound_u = (np.sqrt(e / (e - 1)) * delta + ((e + 3) / 2 + 1) * U * float(std.max())) / rng + float(ref_u.max()) * rel_rng
    err_u = float((unc - ref_u).abs().max())
    print(f"mean E={e} {h}x{w}: pred err {err_p:.3e} (bound {bound_p:.3e}), unc err {err_u:.3e} (bound {bound_u:.3e})")
    assert err_p <= bound_p
    assert err_u <= bound_u


def test_std_of_one_member_is_nan_like_torch_std():
    from genpercept_amd import engine
    maps = _members(1, 3, 5)
    pred, unc = engine.ensemble_reduce(maps[:, 0][None].cuda(), torch.ones(1, 1), torch.zeros(1, 1), "mean", True)
    assert bool(torch.isnan(unc).all()) and bool(torch.isnan(maps.std(dim=0)).all())
    assert float(pred.min()) == 0.0 and float(pred.max()) == 1.0


# 4. batch independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["median", "mean"])
def test_an_image_is_bitwise_the_same_alone_and_in_a_batch(reduction):
    from genpercept_amd import engine
    e, h, w = 5, 37, 53
    maps = torch.stack([_members(e, h, w, seed=20 + i)[:, 0] * (1.0 + i) for i in range(3)]).cuda()  # [3, E, H, W], different contents
    s = torch.stack([_params(e)[0] * (1.0 + 0.1 * i) for i in range(3)])
    t = torch.stack([_params(e)[1] - 0.2 * i for i in range(3)])
    pb, ub = engine.ensemble_reduce(maps, s, t, reduction, True)
    p1, u1 = engine.ensemble_reduce(maps[1:2].clone(), s[1:2], t[1:2], reduction, True)
    assert torch.equal(pb[1:2], p1) and torch.equal(ub[1:2], u1)
    assert not torch.equal(pb[0], pb[1]) and not torch.equal(pb[1], pb[2])
    for i in range(3):  # the (min, max) slabs are per image
        assert float(pb[i].min()) == 0.0 and float(pb[i].max()) == 1.0


# 5. gather ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,small_hw", [((96, 128), (37, 50)), ((130, 97), (50, 37)), ((40, 48), (40, 48))])
def test_gather_is_bitwise_resize_max_res(hw, small_hw):
    from genpercept_amd import engine
    from genpercept_amd.image_util import resize_max_res, resize_max_res_size
    x = torch.randn((2, 3, *hw), generator=torch.Generator().manual_seed(hw[0]))
    size = resize_max_res_size(*hw, 50) if max(hw) > 50 else hw
    assert tuple(size) == small_hw
    ref = resize_max_res(x, 50, "nearest-exact") if max(hw) > 50 else x
    small, mm = engine.ensemble_gather(x.cuda(), *size)
    assert small.shape == (2, 3, *small_hw) and mm.shape == (2, 3, 2)
    assert torch.equal(small.cpu(), ref)
    assert torch.equal(mm[..., 0].cpu(), ref.amin(dim=(2, 3))) and torch.equal(mm[..., 1].cpu(), ref.amax(dim=(2, 3)))


# 6. whole function, both routes -------------------------------------------------------------------------------------------------------
def _distorted_stack(phase=0.0):
    yy, xx = np.mgrid[0:96, 0:128].astype(np.float32)
    base = torch.from_numpy(0.5 + 0.4 * np.sin(xx / 17.0 + np.float32(phase)) * np.cos(yy / 13.0))
    return torch.stack([base * s + t for s, t in ((1.0, 0.0), (1.7, -0.3), (0.6, 0.2), (1.2, 0.1))])[:, None]


def test_both_routes_of_ensemble_depth_agree_bitwise(monkeypatch):
    from genpercept_amd.ensemble import ensemble_depth, ensemble_depth_batch
    monkeypatch.delenv("GENPERCEPT_HOST_ENSEMBLE", raising=False)
    calls = _count_calls(monkeypatch, "ensemble_reduce")
    d0, d1 = _distorted_stack(), _distorted_stack(0.7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host0, _ = ensemble_depth(d0, max_res=50)
        host1, hu1 = ensemble_depth(d1, max_res=50, output_uncertainty=True)
        assert calls == []
        dev0, none = ensemble_depth(d0.cuda(), max_res=50)
        assert calls == [(1, 4, 96, 128)] and none is None and dev0.is_cuda and dev0.shape == (1, 1, 96, 128)
        assert torch.equal(dev0.cpu(), host0)
        dev1, du1 = ensemble_depth(d1.cuda(), max_res=50, output_uncertainty=True)
        assert torch.equal(dev1.cpu(), host1) and torch.equal(du1.cpu(), hu1)
        del calls[:]
        pb, ub = ensemble_depth_batch(torch.stack([d0, d1]).cuda(), max_res=50, output_uncertainty=True)
        assert calls == [(2, 4, 96, 128)]
        assert pb.shape == (2, 1, 96, 128) and torch.equal(pb[0:1].cpu(), host0) and torch.equal(pb[1:2].cpu(), host1) and torch.equal(ub[1:2].cpu(), hu1)
        # the switch: the host's tensor ops on the device tensor, no kernel of csrc/ensemble.hip
        del calls[:]
        monkeypatch.setenv("GENPERCEPT_HOST_ENSEMBLE", "1")
        sw, _ = ensemble_depth(d0.cuda(), max_res=50)
        assert calls == [] and sw.is_cuda and sw.shape == (1, 1, 96, 128) and float(sw.min()) == 0.0 and float(sw.max()) == 1.0
    with pytest.raises(ValueError, match="Unrecognized alignment"):
        monkeypatch.delenv("GENPERCEPT_HOST_ENSEMBLE", raising=False)
        ensemble_depth(d0.cuda(), scale_invariant=False, shift_invariant=False)


# 7. pipeline --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_ensembles_the_batch_with_one_device_call(monkeypatch):
    from genpercept_amd import GenPerceptPipeline
    from oracle import sd21 as osd
    sched = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False, steps_offset=1,
                 prediction_type="v_prediction", timestep_spacing="leading")
    golden = np.load(os.path.join(GOLD, "e2e_multistep.npz"))
    vc, uc4 = osd.VAECfg.tiny(), osd.UNetCfg.tiny()
    u4 = osd.synth_state_dict(osd.unet_manifest(uc4), seed=1)
    vsd = osd.synth_state_dict(osd.vae_manifest(vc), seed=2)
    monkeypatch.delenv("GENPERCEPT_HOST_ENSEMBLE", raising=False)
    calls = _count_calls(monkeypatch, "ensemble_reduce")
    pipe = GenPerceptPipeline(unet=u4, vae=vsd, scheduler=dict(sched), text_encoder=torch.as_tensor(golden["ctx"]), tokenizer=None,
                              genpercept_pipeline=False, rgb_blending=False, torch_dtype=torch.bfloat16).to("cuda")
    img = torch.as_tensor(golden["sq_rgb"][0])
    images = torch.stack([img, img.flip(-1).roll(7, -2)])  # two different 64 x 64 uint8 images
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pipe.predict_batch_device(images, "depth", processing_res=0, denoising_steps=2, ensemble_size=3, generator=torch.Generator().manual_seed(3))
        assert calls == [(2, 3, 64, 64)]  # once, for the batch
        assert out.is_cuda and out.shape == (2, 1, 64, 64) and out.dtype == torch.float32
        for i in range(2):
            assert float(out[i].min()) == 0.0 and float(out[i].max()) == 1.0
        assert not torch.equal(out[0], out[1])
        monkeypatch.setenv("GENPERCEPT_HOST_ENSEMBLE", "1")
        del calls[:]
        host = pipe.predict_batch_device(images, "depth", processing_res=0, denoising_steps=2, ensemble_size=3, generator=torch.Generator().manual_seed(3))
        assert calls == []
    assert host.is_cuda and host.shape == out.shape
    for i in range(2):
        assert float(host[i].min()) == 0.0 and float(host[i].max()) == 1.0
