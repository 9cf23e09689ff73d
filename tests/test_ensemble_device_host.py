"""CPU tests of the device ensembling entries (gp_ensemble_gather / gp_ensemble_workspace / gp_ensemble_reduce): declared, exported, bound;
argument validation, which runs before any HIP call and so needs no GPU; the host route of `ensemble_depth` never touches the engine; the
pipeline makes ONE batched ensembling call for B images, through stub engine entries implemented in torch on the CPU."""
import ctypes as C
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("gp_ensemble_gather", "gp_ensemble_workspace", "gp_ensemble_reduce")
GP_ERR_INVALID = 1


def _libs():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    assert "genpercept/util/ensemble.py:43-205" in hdr and "genpercept_pipeline.py:289-298" in hdr
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
    assert len(engine.SYMBOLS["gp_ensemble_gather"][1]) == 10 and len(engine.SYMBOLS["gp_ensemble_reduce"][1]) == 13
    assert engine.SYMBOLS["gp_ensemble_workspace"][0] is C.c_longlong
    assert "ensemble.hip" in __import__("genpercept_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(engine.ensemble_gather) and callable(engine.ensemble_reduce)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8)):
            assert lib.gp_ensemble_workspace(*bad) == 0
        for e, h, w in ((1, 1, 1), (5, 37, 53), (10, 768, 768), (64, 4096, 4096)):
            one = lib.gp_ensemble_workspace(1, e, h, w)
            assert one > 0 and one % 8 == 0
            assert lib.gp_ensemble_workspace(7, e, h, w) == 7 * one and lib.gp_ensemble_workspace(65535, e, h, w) == 65535 * one


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    P, Q, R, WS = 0x1000, 0x2000, 0x3000, 0x4000  # depth, scale / small, pred / minmax, workspace (8-byte aligned)
    for lib in _libs():
        need = lib.gp_ensemble_workspace(2, 3, 8, 8)
        ok = dict(depth=P, scale=Q, shift=None, B=2, E=3, H=8, W=8, reduction=0, pred=R, unc=None, ws=WS, nbytes=need)

        def reduce(**kw):
            a = dict(ok, **kw)
            return lib.gp_ensemble_reduce(a["depth"], a["scale"], a["shift"], a["B"], a["E"], a["H"], a["W"], a["reduction"], a["pred"], a["unc"], a["ws"],
                                          a["nbytes"], None)

        big = lib.gp_ensemble_workspace(1, 3, 65536, 65536)
        cases = [dict(E=0), dict(E=-1), dict(E=65), dict(reduction=-1), dict(reduction=2), dict(depth=None), dict(scale=None), dict(pred=None),
                 dict(ws=None), dict(B=1, H=65536, W=65536, nbytes=big), dict(B=1, H=1 << 16, W=1 << 15, nbytes=big), dict(B=0), dict(B=-3),
                 dict(B=65536, nbytes=lib.gp_ensemble_workspace(65536, 3, 8, 8)), dict(H=0), dict(W=0), dict(nbytes=need - 1), dict(nbytes=0),
                 dict(ws=WS + 4)]
        for kw in cases:
            assert reduce(**kw) == GP_ERR_INVALID, kw
        okg = dict(depth=P, B=2, E=3, H=8, W=8, h=4, w=4, small=Q, minmax=R)

        def gather(**kw):
            a = dict(okg, **kw)
            return lib.gp_ensemble_gather(a["depth"], a["B"], a["E"], a["H"], a["W"], a["h"], a["w"], a["small"], a["minmax"], None)

        for kw in [dict(depth=None), dict(small=None), dict(minmax=None), dict(B=0), dict(E=0), dict(H=0), dict(W=0), dict(h=0), dict(w=0),
                   dict(H=65536, W=65536), dict(h=65536, w=65536), dict(B=65536, E=65536)]:
            assert gather(**kw) == GP_ERR_INVALID, kw


def test_cpu_tensors_never_touch_the_engine(monkeypatch):
    from genpercept_amd import engine
    from genpercept_amd.ensemble import ensemble_depth, ensemble_depth_batch

    def boom(*a, **k):
        raise AssertionError("the host route must not load the library")

    for name in ("load_library", "ensemble_gather", "ensemble_reduce"):
        monkeypatch.setattr(engine, name, boom)
    g = np.load(os.path.join(GOLD, "ensemble_ref.npz"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in ("affine_unc7", "scale_med6"):
            kw = {"shift_invariant": True, **json.loads(str(g[c + "/kw"]))}
            x = torch.from_numpy(g[c + "/in"])
            pred, unc = ensemble_depth(x, scale_invariant=True, max_res=50, **kw)
            assert np.abs(pred.numpy() - g[c + "/pred"]).max() <= 1e-6
            if c + "/unc" in g.files:
                assert np.abs(unc.numpy() - g[c + "/unc"]).max() <= 1e-6
            # the batch entry on CPU tensors is the single entry per image
            pb, ub = ensemble_depth_batch(torch.stack([x, x.flip(-1)]), scale_invariant=True, max_res=50, **kw)
            p1, u1 = ensemble_depth(x.flip(-1), scale_invariant=True, max_res=50, **kw)
            assert pb.shape == (2, 1, 40, 48) and torch.equal(pb[0:1], pred) and torch.equal(pb[1:2], p1)
            assert (ub is None) == (unc is None) and (ub is None or (torch.equal(ub[0:1], unc) and torch.equal(ub[1:2], u1)))
        pb4, _ = ensemble_depth_batch(torch.stack([x, x])[:, :, 0], scale_invariant=True, shift_invariant=False, max_res=50)  # [B,E,H,W]
        assert torch.equal(pb4[0:1], pred)
    with pytest.raises(ValueError):
        ensemble_depth_batch(torch.zeros(2, 3, 3, 4, 4))
    with pytest.raises(ValueError):
        ensemble_depth_batch(torch.zeros(2, 3, 1, 4, 4), reduction="mode")
    with pytest.raises(ValueError):
        ensemble_depth_batch(torch.zeros(2, 3, 1, 4, 4), scale_invariant=False, shift_invariant=True)
    with pytest.raises(ValueError, match="Unrecognized alignment"):
        ensemble_depth_batch(torch.zeros(2, 3, 1, 4, 4), scale_invariant=False, shift_invariant=False)


class _FakeLib:
    @staticmethod
    def gp_latent_size(x):
        for _ in range(3):
            x = (x - 2) // 2 + 1
        return x


class _FakeEngine:
    """Records the noise the pipeline hands to the engine; members differ by an affine map of one base map that depends on the image."""

    def __init__(self):
        self.lib, self.calls = _FakeLib(), []

    def set_context(self, e):
        pass

    def set_timestep(self, t):
        pass

    def infer_steps(self, rgb, mode, plan, noise):
        self.calls.append((tuple(rgb.shape), noise.clone()))
        b, _, h, w = rgb.shape
        base = torch.linspace(0.1, 0.9, h * w).reshape(1, 1, h, w) ** (1.0 + rgb.float().mean(dim=(1, 2, 3)).reshape(b, 1, 1, 1) / 255.0)
        k = noise.reshape(b, -1)[:, :1].reshape(b, 1, 1, 1)
        return base * (1 + 0.1 * k) + 0.05 * k


def _cpu_gather(depth, h, w, out=None):
    """engine.ensemble_gather in torch on the CPU"""
    from genpercept_amd.image_util import resize_to
    b, e = depth.shape[:2]
    small = resize_to(depth, (h, w), "nearest-exact").contiguous()
    mm = torch.stack([small.amin(dim=(2, 3)), small.amax(dim=(2, 3))], dim=-1)
    if out is not None:
        out.copy_(torch.cat([small.reshape(-1), mm.reshape(-1)]))
    return small, mm


def _cpu_reduce(depth, scale=None, shift=None, reduction="median", output_uncertainty=False):
    """engine.ensemble_reduce in torch on the CPU: the computation of ensemble.py's host route, per image"""
    from genpercept_amd.ensemble import _reduce
    preds, uncs = [], []
    for i in range(depth.shape[0]):
        al = depth[i][:, None] * torch.as_tensor(scale[i]).view(-1, 1, 1, 1)
        if shift is not None:
            al = al + torch.as_tensor(shift[i]).view(-1, 1, 1, 1)
        pred, unc = _reduce(al, reduction, output_uncertainty)
        d_min = pred.min() if shift is not None else 0
        rng = (pred.max() - d_min).clamp(min=1e-6)
        preds.append(((pred - d_min) / rng)[0])
        uncs.append((unc / rng)[0] if output_uncertainty else None)
    return torch.cat(preds), (torch.cat(uncs) if output_uncertainty else None)


def test_pipeline_makes_one_batched_ensembling_call(monkeypatch):
    from types import SimpleNamespace
    from genpercept_amd import GenPerceptPipeline, engine, ensemble
    sched = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False, steps_offset=1,
                 prediction_type="v_prediction")
    monkeypatch.setenv("GENPERCEPT_HOST_PREPOST", "1")
    monkeypatch.delenv("GENPERCEPT_HOST_ENSEMBLE", raising=False)
    monkeypatch.setattr(GenPerceptPipeline, "_device", torch.device("cpu"), raising=False)
    pipe = GenPerceptPipeline(unet={}, vae={}, text_encoder=np.zeros((2, 8), np.float32), scheduler=sched, genpercept_pipeline=False, rgb_blending=False)
    pipe._device = torch.device("cpu")
    pipe._engine, pipe._timestep, pipe._ctx_loaded = _FakeEngine(), 1, None
    pipe.vae_config = SimpleNamespace(latent_channels=4)
    pipe.mode = "depth"
    seen = {"gather": [], "reduce": [], "batch": []}

    def gather(depth, h, w, out=None):
        seen["gather"].append((tuple(depth.shape), h, w))
        return _cpu_gather(depth, h, w, out)

    def reduce(depth, scale=None, shift=None, reduction="median", output_uncertainty=False):
        seen["reduce"].append((tuple(depth.shape), np.asarray(scale).shape, None if shift is None else np.asarray(shift).shape, reduction))
        return _cpu_reduce(depth, scale, shift, reduction, output_uncertainty)

    real_batch = ensemble.ensemble_depth_batch

    def batch(depth, **kw):
        seen["batch"].append((tuple(depth.shape), kw))
        return real_batch(depth, **kw)

    monkeypatch.setattr(engine, "ensemble_gather", gather)
    monkeypatch.setattr(engine, "ensemble_reduce", reduce)
    monkeypatch.setattr(ensemble, "ensemble_depth_batch", batch)
    x = torch.stack([torch.full((3, 64, 80), -0.5), torch.full((3, 64, 80), 0.25)])
    opts = dict(steps=4, ensemble_size=3, batch_size=2, generator=torch.Generator().manual_seed(9), ensemble_kwargs={"reduction": "mean", "max_iter": 3})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = pipe._predict(x, None, "", opts)                         # CPU members: the host route, no engine entry
        assert seen["gather"] == [] and seen["reduce"] == [] and len(seen["batch"]) == 1
        calls_host, pipe._engine.calls = pipe._engine.calls, []
        monkeypatch.setattr(ensemble, "_device_route", lambda d: d.dtype == torch.float32)   # as if the members were on a GPU
        opts["generator"] = torch.Generator().manual_seed(9)
        dev = pipe._predict(x, None, "", opts)
    # one batch call with the kwargs passed through; inside it one gather and one reduce for both images (64 x 80 -> 40 x 50 at max_res 50)
    assert [b[0] for b in seen["batch"]] == [(2, 3, 1, 64, 80)] * 2
    assert all(b[1] == dict(scale_invariant=True, shift_invariant=True, max_res=50, reduction="mean", max_iter=3) for b in seen["batch"])
    assert seen["gather"] == [((2, 3, 64, 80), 40, 50)]
    assert seen["reduce"] == [((2, 3, 64, 80), (2, 3), (2, 3), "mean")]
    # the generator is consumed in the same order as before: per image, E = 3 members in engine calls of 2 + 1
    g = torch.Generator().manual_seed(9)
    for calls in (calls_host, pipe._engine.calls):
        assert [c[0][0] for c in calls] == [2, 1, 2, 1]
    for c in pipe._engine.calls:
        assert torch.equal(c[1], torch.randn((c[0][0], 4, 8, 10), generator=g))
    # and the stubbed device route computes what the host route does (the stubs are the host's tensor ops)
    assert dev.shape == (2, 1, 64, 80) and torch.equal(dev, host)
    for i in range(2):
        assert dev[i].min() == 0 and dev[i].max() == 1
