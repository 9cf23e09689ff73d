"""CPU tests of the dis structure scores (S-measure, E-measure, weighted F): the device entries (gp_eval_structure_workspace /
gp_eval_structure) are declared, exported by both libraries and bound, and refuse bad arguments before any HIP call; the Gaussian table; the
host route (eval_metrics.structure_counts / structure_from_counts / edt_keys / weighted_f / structure_metrics) against scipy's distance
transform, a brute force over all foreground pixels and per-pixel float evaluations of the published formulas; hand cases; the file route and
the loop `infer_eval.infer_and_evaluate_masks(..., structure=True)` with a fake pipeline and the NumPy evaluators, at world sizes 1 and 2.

Bounds.  E_t from counts is under 30 rounded operations on exact integers (30 * 2^-53 = 3.3e-15 relative); the per-pixel mean over at most
4160 pixels in another order carries at most n * 2^-53 = 4.6e-13: 1e-12 relative.  S: the m2 - xb^2 form of the variance carries about 2e-16
absolute, the smallest non-zero variance of 8-bit data over 4160 pixels is about 4e-9, so sigma is good to about 1e-12 and S to 1e-9
absolute."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_eval_mask_host as tm  # noqa: E402  (make_tree, FakePipe, numpy_evaluator, random_case: the mask loop's fixtures)

NAMES = ("gp_eval_structure_workspace", "gp_eval_structure")
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
STRUCTURE_METRICS = ["s_alpha", "max_e", "mean_e", "adp_e", "wf"]
GP_ERR_INVALID = 1


def _libs():
    import __graft_entry__ as ge
    ge.build()
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


# ---- symbols -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from genpercept_amd import engine
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    hdr = open(os.path.join(ROOT, "include", "genpercept_hip.h")).read()
    declared = set(re.findall(r"\b(gp_[a-z0-9_]+)\s*\(", hdr))
    for lib in _libs():
        for name in NAMES:
            assert name in declared and name in engine.SYMBOLS
            fn = getattr(lib, name)
            assert fn.restype is engine.SYMBOLS[name][0] and list(fn.argtypes) == list(engine.SYMBOLS[name][1])
    assert len(engine.SYMBOLS["gp_eval_structure"][1]) == 12 and len(engine.SYMBOLS["gp_eval_structure_workspace"][1]) == 3
    assert engine.SYMBOLS["gp_eval_structure_workspace"][0] is C.c_longlong
    assert callable(engine.eval_structure_raw) and callable(engine.eval_structure)
    assert list(engine.STRUCTURE_METRICS) == list(em.STRUCTURE_METRICS) == list(ie.STRUCTURE_METRICS) == STRUCTURE_METRICS
    assert engine.STRUCTURE_COUNTS == em.STRUCTURE_COUNTS == 537 and engine.STRUCTURE_OUT == len(engine.STRUCTURE_OUT_NAMES) == 15
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in NAMES)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert lib.gp_eval_structure_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (1024, 1024), (1031, 2053), (32767, 32767)):
            one = lib.gp_eval_structure_workspace(1, h, w)
            assert one >= 8 * h * w and one % 8 == 0          # at least the keys
            assert lib.gp_eval_structure_workspace(7, h, w) == 7 * one and lib.gp_eval_structure_workspace(65535, h, w) == 65535 * one


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    P, G, O, CN, E, WS = 0x1000, 0x2000, 0x4000, 0x5000, 0x6000, 0x8000  # all 8-byte aligned
    for lib in _libs():
        need = lib.gp_eval_structure_workspace(2, 8, 8)
        ok = dict(pred=P, u8=0, gt=G, B=2, H=8, W=8, out=O, counts=CN, edt=E, ws=WS, nbytes=need)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.gp_eval_structure(a["pred"], a["u8"], a["gt"], a["B"], a["H"], a["W"], a["out"], a["counts"], a["edt"], a["ws"], a["nbytes"], None)

        huge = 1 << 62
        cases = [dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None),
                 dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
                 dict(B=65536, nbytes=huge),                                                              # above the grid's limit
                 dict(B=1, H=32768, W=8, nbytes=huge), dict(B=1, H=8, W=32768, nbytes=huge),              # d2 would reach 2^31
                 dict(B=1, H=65536, W=65536, nbytes=huge),
                 dict(u8=-1), dict(u8=2), dict(pred=P + 2),
                 dict(out=O + 4), dict(counts=CN + 4), dict(counts=CN + 1), dict(edt=E + 4), dict(ws=WS + 4),
                 dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=lib.gp_eval_structure_workspace(1, 8, 8))]
        for kw in cases:
            assert call(**kw) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_inputs_before_the_library():
    from genpercept_amd import engine
    with pytest.raises(ValueError):
        engine.eval_structure_raw(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        engine.eval_structure_raw(torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


# ---- the Gaussian table ------------------------------------------------------------------------------------------------------------------------
def test_gaussian_table():
    """Each entry within 1 ulp of exp(-(dx^2 + dy^2) / 50) / sum (in 60-digit decimals), the sum within 4 ulp of 1, symmetric, and the same
    literals in the kernel file."""
    from decimal import Decimal, getcontext
    from genpercept_amd import eval_metrics as em
    getcontext().prec = 60
    raw = {(i, j): (Decimal(-((i - 3) ** 2 + (j - 3) ** 2)) / Decimal(50)).exp() for i in range(7) for j in range(7)}
    total = sum(raw.values())
    k = em.WF_K
    assert k.shape == (7, 7) and k.dtype == np.float64
    for (i, j), v in raw.items():
        want = v / total
        assert abs(Decimal(float(k[i, j])) - want) <= Decimal(float(np.spacing(float(want)))), (i, j)
    assert abs(Fraction(math.fsum(k.reshape(-1))) - 1) <= 4 * Fraction(np.spacing(1.0))
    assert abs(sum(Fraction(float(v)) for v in k.reshape(-1)) - 1) <= 4 * Fraction(np.spacing(1.0))
    assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])
    assert em.WF_C == math.log(0.5) / 5
    src = open(os.path.join(ROOT, "genpercept_amd", "csrc", "eval_structure.hip")).read()
    lits = re.findall(r"0x1\.[0-9a-f]+p-6", src[src.index("ES_K[49]"):src.index("ES_WF_C")])
    assert lits == re.findall(r"0x1\.[0-9a-f]+p-6", em.WF_K_HEX) and len(lits) == 49
    assert float.fromhex(re.search(r"ES_WF_C = (-0x[0-9a-fp.\-]+);", src).group(1)) == em.WF_C


# ---- the distance transform ----------------------------------------------------------------------------------------------------------------
def brute_keys(G):
    h, w = G.shape
    ys, xs = np.nonzero(G)
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return ((d2.astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)).min(-1)


def edt_inputs():
    rng = np.random.RandomState(5)
    out = []
    for shape in ((1, 1), (1, 2), (2, 1), (7, 5), (33, 40), (64, 65)):
        for density in (0.02, 0.4):
            G = rng.rand(*shape) < density
            G[rng.randint(shape[0]), rng.randint(shape[1])] = True
            out.append(G)
    corner = np.zeros((40, 64), bool)
    corner[39, 63] = True
    sym = np.zeros((21, 31), bool)                  # mirror-symmetric about column 15: every pixel of that column has two nearest pixels
    sym[5:16, 10] = sym[5:16, 20] = True
    cross = np.zeros((31, 31), bool)                # four equidistant pixels from the centre
    cross[15, 5] = cross[15, 25] = cross[5, 15] = cross[25, 15] = True
    return out + [corner, sym, cross, np.ones((4, 6), bool)]


def test_edt_keys_equal_scipy_and_the_brute_force():
    from scipy import ndimage
    from genpercept_amd import eval_metrics as em
    for G in edt_inputs():
        k = em.edt_keys(G)
        assert k.dtype == np.uint64 and k.shape == G.shape
        d2 = (k >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(d2, np.rint(ndimage.distance_transform_edt(~G) ** 2).astype(np.int64)), G.shape
        assert np.array_equal(k, brute_keys(G)), G.shape
        idx = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert G.reshape(-1)[idx].all() and np.array_equal(idx[G], np.flatnonzero(G))   # a foreground pixel: (0, itself)
    assert (em.edt_keys(np.zeros((3, 4), bool)) == em.EDT_NO_KEY).all()
    sym = edt_inputs()[-3]
    k = em.edt_keys(sym)
    assert (k[5:16, 15] & np.uint64(0xFFFFFFFF) == np.arange(5, 16) * 31 + 10).all()     # the tie goes to the smaller index: the left column


def test_edt_keys_is_fast_enough():
    """1024 x 1024 with a single far object -- the slowest case, the row search spans the image -- well under a minute."""
    import time
    from genpercept_amd import eval_metrics as em
    G = np.zeros((1024, 1024), bool)
    G[1000:1010, 1000:1010] = True
    t0 = time.time()
    k = em.edt_keys(G)
    assert time.time() - t0 < 40.0
    assert int(k[0, 0] >> np.uint64(32)) == 2 * 1000 * 1000 and int(k[0, 0] & np.uint64(0xFFFFFFFF)) == 1000 * 1024 + 1000


# ---- E and S against per-pixel evaluations -------------------------------------------------------------------------------------------------------
def e_reference(q, g):
    """The toolbox formula per pixel on boolean arrays (its eps terms dropped, as the header says), 256 thresholds."""
    G = g > 128
    n, n_fg = G.size, int(G.sum())
    out = []
    for t in range(256):
        pb = q >= t
        if n_fg == 0:
            out.append(float((~pb).sum()) / max(n - 1, 1))
        elif n_fg == n:
            out.append(float(pb.sum()) / max(n - 1, 1))
        else:
            ap, ag = pb.astype(np.float64) - pb.mean(), G.astype(np.float64) - G.mean()
            phi = 2.0 * ap * ag / (ap * ap + ag * ag)
            out.append(float(((phi + 1.0) ** 2 / 4.0).sum()) / max(n - 1, 1))
    return out


def s_reference(q, g):
    """S-measure per pixel in floats: np.mean, np.std(ddof=1), block SSIM; the centroid in exact rationals, halves up."""
    G = g > 128
    p = q.astype(np.float64) / 255.0
    h, w = G.shape
    n, n_fg = G.size, int(G.sum())
    if n_fg == 0:
        return 1.0 - p.mean(), None, None
    if n_fg == n:
        return p.mean(), None, None

    def obj(x):
        mu, sigma = x.mean(), (x.std(ddof=1) if x.size > 1 else 0.0)
        return 2.0 * mu / (mu * mu + 1.0 + sigma)

    u = n_fg / n
    so = u * obj(p[G]) + (1.0 - u) * obj(1.0 - p[~G])
    ys, xs = np.nonzero(G)
    cx = math.floor(Fraction(int(xs.sum()), n_fg) + Fraction(1, 2))
    cy = math.floor(Fraction(int(ys.sum()), n_fg) + Fraction(1, 2))
    sr = 0.0
    for rows, cols in ((slice(0, cy + 1), slice(0, cx + 1)), (slice(0, cy + 1), slice(cx + 1, w)), (slice(cy + 1, h), slice(0, cx + 1)),
                       (slice(cy + 1, h), slice(cx + 1, w))):
        x, y = p[rows, cols].reshape(-1), G[rows, cols].reshape(-1).astype(np.float64)
        N = x.size
        if N == 0:
            continue
        mx, my = x.mean(), y.mean()
        sxx, syy, sxy = (((x - mx) ** 2).sum() / (N - 1), ((y - my) ** 2).sum() / (N - 1), ((x - mx) * (y - my)).sum() / (N - 1)) if N > 1 else (0.0, 0.0, 0.0)
        a, bq = 4.0 * mx * my * sxy, (mx * mx + my * my) * (sxx + syy)
        # (the published code compares the exact products with 0; in floats a block of constant data gives sums of squares of rounding size)
        qk = a / bq if abs(a) > 1e-30 and abs(bq) > 1e-30 else (1.0 if abs(a) <= 1e-30 and abs(bq) <= 1e-30 else 0.0)
        sr += N / n * qk
    return max(0.5 * so + 0.5 * sr, 0.0), so, sr


def structure_cases():
    out = []
    for shape in ((7, 5), (64, 65)):
        for mask_like in (False, True):
            q, g, _ = tm.random_case(*shape, seed=31 + shape[0], mask_like=mask_like)
            out.append((q, g))
    rng = np.random.RandomState(9)
    q = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    g = np.zeros((9, 11), np.uint8)
    g[:, 10] = 255                                   # foreground in the last column only: empty right blocks
    out.append((q, g))
    g2 = np.zeros((9, 11), np.uint8)
    g2[8, :] = 255                                   # ... in the last row only: empty bottom blocks
    out.append((q, g2))
    return out


def test_e_curve_equals_the_per_pixel_formula():
    from genpercept_amd import eval_metrics as em
    for q, g in structure_cases() + [(np.full((5, 6), 77, np.uint8), np.zeros((5, 6), np.uint8)), (np.full((5, 6), 77, np.uint8), np.full((5, 6), 255, np.uint8))]:
        c = em.structure_counts(q, g)
        e, ref = em.e_curve_from_counts(c), e_reference(q, g)
        for t in range(256):
            assert abs(e[t] - ref[t]) <= 1e-12 * abs(ref[t]), (q.shape, t, e[t], ref[t])
        m = em.structure_from_counts(c)
        total = 0.0
        for t in range(256):
            total = total + e[t]
        assert m["max_e"] == max(e) and m["mean_e"] == total / 256.0
        lim = min(2 * int(q.astype(np.int64).sum()), 255 * q.size)
        assert m["adp_e"] == e[next(t for t in range(256) if t * q.size >= lim)]


def test_s_measure_equals_the_per_pixel_formula():
    from genpercept_amd import eval_metrics as em
    for q, g in structure_cases():
        m = em.structure_from_counts(em.structure_counts(q, g))
        s, so, sr = s_reference(q, g)
        assert np.isfinite([m["s_alpha"], m["s_object"], m["s_region"]]).all()
        assert abs(m["s_alpha"] - s) <= 1e-9 and abs(m["s_object"] - so) <= 1e-9 and abs(m["s_region"] - sr) <= 1e-9, (q.shape, m, s, so, sr)


def test_structure_counts():
    from genpercept_amd import eval_metrics as em
    q, g = structure_cases()[3]
    c = em.structure_counts(q, g)
    G = g > 128
    ys, xs = np.nonzero(G)
    assert c.dtype == np.int64 and c.shape == (537,)
    assert c[0] == G.sum() and c[1] == xs.sum() and c[2] == ys.sum()
    assert c[3] == math.floor(Fraction(int(xs.sum()), int(G.sum())) + Fraction(1, 2)) and c[4] == math.floor(Fraction(int(ys.sum()), int(G.sum())) + Fraction(1, 2))
    blocks = c[5:25].reshape(4, 5)
    assert blocks[:, 0].sum() == q.size and blocks[:, 1].sum() == q.astype(np.int64).sum() and blocks[:, 3].sum() == G.sum()
    assert blocks[:, 2].sum() == (q.astype(np.int64) ** 2).sum() and blocks[:, 4].sum() == q[G].astype(np.int64).sum()
    assert blocks[0, 0] == (c[4] + 1) * (c[3] + 1) and blocks[3, 0] == (q.shape[0] - c[4] - 1) * (q.shape[1] - c[3] - 1)
    mc = em.mask_counts(q, g)
    assert np.array_equal(c[25:], mc[4:])            # the same two histograms as gp_eval_mask's
    with pytest.raises(ValueError):
        em.structure_counts(q.astype(np.int32), g)
    with pytest.raises(ValueError):
        em.structure_counts(q.reshape(-1), g.reshape(-1))


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
def hand_gt():
    g = np.zeros((24, 30), np.uint8)
    g[8:15, 9:21] = 255                              # an object at least 8 pixels from every border
    return g


def test_hand_perfect_and_inverted_prediction():
    from genpercept_amd import eval_metrics as em
    g = hand_gt()
    n, n_fg = g.size, int((g > 128).sum())
    m = em.structure_metrics(g.copy(), g)
    assert list(m)[:10] == ["n", "n_fg", "s_alpha", "s_object", "s_region", "max_e", "mean_e", "adp_e", "cx", "cy"]
    assert m["n"] == n and m["n_fg"] == n_fg and (m["cx"], m["cy"]) == (15, 11)   # means 14.5 and 11.0: the half goes up
    assert abs(m["s_alpha"] - 1.0) <= 1e-15 and abs(m["s_object"] - 1.0) <= 1e-15 and abs(m["s_region"] - 1.0) <= 1e-15
    assert m["max_e"] == n / (n - 1) and m["adp_e"] == n / (n - 1)
    assert m["wf"] == 1.0 and m["wf_precision"] == 1.0 and m["wf_recall"] == 1.0 and m["wf_sum_fg"] == 0.0 and m["wf_sum_bg"] == 0.0
    e = em.e_curve_from_counts(em.structure_counts(g.copy(), g))
    assert e[0] < 1.0 and all(v == n / (n - 1) for v in e[1:])
    assert em.structure_metrics(g.astype(np.float32) / np.float32(255.0), g) == m      # the float route quantises to the same bytes
    inv = em.structure_metrics(255 - g, g)
    assert inv["s_alpha"] == 0.0 and inv["s_object"] == 0.0 and inv["s_region"] < 0.0   # clamped at 0
    assert abs(inv["max_e"] - 0.25 * n / (n - 1)) <= 1e-15 and inv["adp_e"] <= 1e-30
    # every foreground pixel has EA = the table's sum = 1 = E: nothing of the object is found
    assert inv["wf_sum_fg"] == float(n_fg) and inv["wf_recall"] == 0.0 and inv["wf_precision"] == 0.0 and inv["wf"] == 0.0
    assert n - n_fg < inv["wf_sum_bg"] < 2 * (n - n_fg)


def test_hand_degenerate_ground_truth_and_single_pixel():
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(1)
    q = rng.randint(0, 256, (6, 7)).astype(np.uint8)
    n, sq = q.size, int(q.astype(np.int64).sum())
    m = em.structure_metrics(q, np.zeros_like(q))
    assert m["n_fg"] == 0 and m["s_alpha"] == 1.0 - sq / (255.0 * n) and np.isnan(m["s_object"]) and np.isnan(m["s_region"])
    assert m["wf"] == 0.0 and m["wf_precision"] == 0.0 and m["wf_recall"] == 0.0 and (m["cx"], m["cy"]) == (0, 0)
    e = em.e_curve_from_counts(em.structure_counts(q, np.zeros_like(q)))
    assert all(e[t] == float((q < t).sum()) / (n - 1) for t in range(256)) and m["max_e"] == e[255]
    m = em.structure_metrics(q, np.full_like(q, 255))
    assert m["n_fg"] == n and m["s_alpha"] == sq / (255.0 * n) and np.isnan(m["s_object"]) and np.isnan(m["s_region"])
    e = em.e_curve_from_counts(em.structure_counts(q, np.full_like(q, 255)))
    assert all(e[t] == float((q >= t).sum()) / (n - 1) for t in range(256)) and m["max_e"] == n / (n - 1)
    assert 0.0 < m["wf"] < 1.0 and m["wf_sum_bg"] == 0.0 and m["wf_precision"] == 1.0
    one = np.array([[255]], np.uint8)
    zero = np.array([[0]], np.uint8)
    m = em.structure_metrics(one, one)                # n = 1: max(n - 1, 1) keeps the E quotient finite
    assert m["s_alpha"] == 1.0 and m["max_e"] == 1.0 and m["mean_e"] == 1.0 and m["adp_e"] == 1.0 and m["wf"] == 1.0
    m = em.structure_metrics(zero, zero)
    assert m["s_alpha"] == 1.0 and m["max_e"] == 1.0 and m["mean_e"] == 255.0 / 256.0 and m["wf"] == 0.0
    m = em.structure_metrics(zero, one)
    assert m["s_alpha"] == 0.0 and m["max_e"] == 1.0 and m["adp_e"] == 1.0 and m["wf_sum_fg"] == float(em.WF_K[3, 3])
    g = np.zeros((1, 2), np.uint8)                    # two pixels, one of each class: every block has N <= 1
    g[0, 1] = 255
    m = em.structure_metrics(g.copy(), g)
    assert np.isfinite([m[k] for k in STRUCTURE_METRICS]).all() and m["max_e"] == 2.0 and m["wf"] == 1.0


def test_weighted_f_follows_the_published_steps():
    """weighted_f against a direct transcription of the published algorithm on top of scipy's distance transform with indices (which breaks
    ties its own way: the inputs here have a unique nearest pixel wherever q differs among the candidates -- q is constant on the object)."""
    from scipy import ndimage
    from genpercept_amd import eval_metrics as em
    rng = np.random.RandomState(12)
    g = hand_gt()
    G = g > 128
    q = np.where(G, 200, rng.randint(0, 120, g.shape)).astype(np.uint8)
    dst, (iy, ix) = ndimage.distance_transform_edt(~G, return_indices=True)
    p, gf = q / 255.0, G.astype(np.float64)
    e = np.abs(p - gf)
    et = np.where(G, e, e[iy, ix])
    ea = ndimage.correlate(et, em.WF_K, mode="constant", cval=0.0)
    min_ea = np.where(G & (ea < e), ea, e)
    b = np.where(G, 1.0, 2.0 - np.exp(math.log(0.5) / 5 * dst))
    ew = min_ea * b
    tpw = gf.sum() - ew[G].sum()
    fpw = ew[~G].sum()
    r, pr = 1.0 - ew[G].mean(), tpw / (tpw + fpw)
    want = 2.0 * r * pr / (r + pr)
    m = em.weighted_f(q, g)
    assert abs(m["wf"] - want) <= 1e-12 and abs(m["wf_recall"] - r) <= 1e-12 and abs(m["wf_precision"] - pr) <= 1e-12
    assert 0.3 < m["wf"] < 0.95


# ---- the file route and the loop -------------------------------------------------------------------------------------------------------------
def numpy_structure_evaluator(pred, gt):
    """engine.eval_structure's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    return [em.structure_metrics(pred[i].numpy(), gt[i].numpy()) for i in range(pred.shape[0])]


def test_structure_off_leaves_the_files_as_they_are_and_on_adds_five_columns(tmp_path):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    base, pred_dir = str(tmp_path / "data"), str(tmp_path / "pred")
    samples = tm.make_tree(base)
    ie.run_inference(tm.FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="dis")
    outs = {k: str(tmp_path / k) for k in ("file_default", "file_off", "file_on", "loop_default", "loop_off", "loop_on")}
    r_default = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_default"])
    r_off = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_off"], structure=False)
    r_on = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_on"], structure=True)
    l_default = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", output_dir=outs["loop_default"], batch_size=2, evaluator=tm.numpy_evaluator)
    l_off = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", output_dir=outs["loop_off"], batch_size=2, evaluator=tm.numpy_evaluator,
                                        structure=False, structure_evaluator=None)
    l_on = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", output_dir=outs["loop_on"], batch_size=2, evaluator=tm.numpy_evaluator,
                                       structure=True, structure_evaluator=numpy_structure_evaluator)
    assert r_default == r_off == l_default == l_off and list(r_off) == MASK_METRICS + ["max_f_dataset"]
    assert list(r_on) == list(l_on) == MASK_METRICS + STRUCTURE_METRICS + ["max_f_dataset"] and r_on == l_on
    assert all(r_on[k] == r_off[k] for k in r_off)

    def files(d):
        csv = open(os.path.join(d, "per_sample_metrics-mask.csv")).read()
        txt = [x for x in open(os.path.join(d, "eval_metrics-mask.txt")).read().splitlines() if "of predictions" not in x]
        return csv, txt

    for k in ("file_off", "loop_default", "loop_off"):
        assert files(outs[k]) == files(outs["file_default"]), k
    csv_off, txt_off = files(outs["file_default"])
    assert csv_off.splitlines()[0] == "filename," + ",".join(MASK_METRICS) and txt_off[-2] == "  ".join(MASK_METRICS)
    csv_on, txt_on = files(outs["file_on"])
    assert files(outs["loop_on"]) == (csv_on, txt_on)
    assert csv_on.splitlines()[0] == "filename," + ",".join(MASK_METRICS + STRUCTURE_METRICS) and txt_on[-2] == "  ".join(MASK_METRICS + STRUCTURE_METRICS)
    assert txt_on[-1] == "  ".join(f"{r_on[k]:.6g}" for k in MASK_METRICS + STRUCTURE_METRICS)
    rows = []
    for line_off, line_on, s in zip(csv_off.splitlines()[1:], csv_on.splitlines()[1:], samples):
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        m = em.structure_metrics(np.load(os.path.join(pred_dir, name)), ie.read_gt_mask(os.path.join(base, s[1])))
        assert line_on == line_off + "," + ",".join(str(m[k]) for k in STRUCTURE_METRICS)
        rows.append(m)
    for k in STRUCTURE_METRICS:
        assert r_on[k] == sum(m[k] for m in rows) / len(rows) and 0.0 <= r_on[k] <= 1.01, k
    region_of = tm.trimap_region(base)
    with pytest.raises(ValueError, match="region_of"):
        ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, region_of=region_of, structure=True)
    with pytest.raises(ValueError, match="region_of"):
        ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", evaluator=tm.numpy_evaluator, region_of=region_of, structure=True,
                                    structure_evaluator=numpy_structure_evaluator)


_WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch.distributed as dist
from genpercept_amd import distributed as gd
from genpercept_amd import infer_eval as ie
import test_eval_structure_host as t
rank, local, world = gd.init_process_group("gloo")
samples = ie.read_filename_list({lst!r})
pipe = t.tm.FakePipe()
res = ie.infer_and_evaluate_masks(pipe, {base!r}, samples, "dis", output_dir={out!r}, batch_size=2, rank=rank, world=world,
                                  evaluator=t.tm.numpy_evaluator, structure=True, structure_evaluator=t.numpy_structure_evaluator)
with open(os.path.join({out!r}, "means_rank%d.json" % rank), "w") as f:
    json.dump(dict(res=res, images=sum(pipe.batches)), f)
dist.barrier()
dist.destroy_process_group()
print("RANK", rank, "OK", flush=True)
"""


def test_structure_loop_world_size_2_gloo(tmp_path):
    """Two ranks share the five images; every rank returns the means over all images (float64 sums of five terms in another association:
    1e-12 absolute, as for the mask loop), rank 0 alone writes the table, which is the one-process table."""
    from genpercept_amd import infer_eval as ie
    base = str(tmp_path / "data")
    samples = tm.make_tree(base)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(" ".join(s) for s in samples) + "\n")
    one = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "dis", output_dir=str(tmp_path / "w1"), batch_size=2, evaluator=tm.numpy_evaluator,
                                      structure=True, structure_evaluator=numpy_structure_evaluator)
    out = str(tmp_path / "w2")
    os.makedirs(out)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lst=lst, base=base, out=out))
    port = 35500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 2, r.stdout + r.stderr
    seen = 0
    for rank in (0, 1):
        got = json.load(open(os.path.join(out, f"means_rank{rank}.json")))
        seen += got["images"]
        assert list(got["res"]) == list(one) == MASK_METRICS + STRUCTURE_METRICS + ["max_f_dataset"]
        for k in one:
            assert abs(got["res"][k] - one[k]) <= 1e-12, (rank, k, got["res"][k], one[k])
    assert seen == len(samples)
    name = "per_sample_metrics-mask.csv"
    assert open(os.path.join(out, name)).read() == open(os.path.join(str(tmp_path / "w1"), name)).read()
    assert len(open(os.path.join(out, name)).read().splitlines()) == 1 + len(samples)
