"""CPU tests of the device normal-evaluation entries (gp_eval_normal_workspace / gp_eval_normal): declared, exported by both libraries, bound;
the workspace rule; argument validation, which runs before any HIP call and so needs no GPU."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_eval_normal_workspace", "gp_eval_normal")
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
    for cite in ("genpercept/losses/geometry_losses.py:550-590", "src/dataset/base_dataset.py:362-363", "416-418"):
        assert cite in hdr
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
    assert len(engine.SYMBOLS["gp_eval_normal"][1]) == 12 and len(engine.SYMBOLS["gp_eval_normal_workspace"][1]) == 3
    assert engine.SYMBOLS["gp_eval_normal_workspace"][0] is C.c_longlong
    assert callable(engine.eval_normal_raw) and callable(engine.eval_normal)
    from genpercept_amd import infer_eval as ie
    assert list(engine.NORMAL_METRICS) == list(ie.NORMAL_METRICS)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert lib.gp_eval_normal_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (480, 640), (1031, 2053), (4032, 6048)):
            one = lib.gp_eval_normal_workspace(1, h, w)
            assert one >= 8 * h * w and one % 8 == 0          # at least the 8-byte key per pixel
            assert lib.gp_eval_normal_workspace(7, h, w) == 7 * one and lib.gp_eval_normal_workspace(65535, h, w) == 65535 * one
            assert lib.gp_eval_normal_workspace(1, w, h) == one and lib.gp_eval_normal_workspace(1, 1, h * w) == one  # H * W alone


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    P, G, M, O, A, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000  # all 8-byte aligned
    for lib in _libs():
        need = lib.gp_eval_normal_workspace(2, 8, 8)
        ok = dict(pred=P, gt=G, mask=M, B=2, H=8, W=8, decode=1, out=O, angles=None, ws=WS, nbytes=need)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.gp_eval_normal(a["pred"], a["gt"], a["mask"], a["B"], a["H"], a["W"], a["decode"], a["out"], a["angles"], a["ws"], a["nbytes"],
                                      None)

        huge = 1 << 62
        cases = [dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None),
                 dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
                 dict(B=65536, nbytes=lib.gp_eval_normal_workspace(65536, 8, 8)),            # above the grid's y limit
                 dict(B=1, H=65536, W=65536, nbytes=huge), dict(B=1, H=1 << 16, W=1 << 15, nbytes=huge),   # H * W beyond the index arithmetic
                 dict(decode=-1), dict(decode=4),
                 dict(mask=None, decode=2), dict(mask=None, decode=3),                        # the derived rule needs the signed ground truth
                 dict(out=O + 4), dict(angles=A + 4), dict(ws=WS + 4), dict(angles=A + 1),
                 dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=lib.gp_eval_normal_workspace(1, 8, 8))]
        for kw in cases:
            assert call(**kw) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_shapes_before_the_library():
    from genpercept_amd import engine
    with pytest.raises(ValueError):
        engine.eval_normal_raw(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError):
        engine.eval_normal_raw(torch.zeros(4, 4), torch.zeros(4, 4))
