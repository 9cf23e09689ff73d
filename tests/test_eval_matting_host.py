"""Matting gradient and connectivity errors, the host half: the C-ABI's argument checks (refused before any HIP call, so they run without a
GPU), the host route (eval_metrics.conn_levels / conn_error / grad_error_map / grad_error / matting_metrics) against independent
constructions on top of scipy (ndimage.label with its default 4-connectivity + bincount + argmax; ndimage.correlate1d(mode="nearest")), and
the file route / dataset loop with matting=True against the same functions.

Bounds.  Levels, level counts and conn_num are integers: equal, no tolerance; conn is one correctly rounded division of conn_num: equal.
The gradient error map against correlate1d: the same products in possibly another order of additions, about 20 roundings of 2^-53 each on
filter outputs <= 2.7 (the positive half of D sums to 1.2, G to 2.3; amp <= 3.8, err <= 16; the recipe's values stay below 4): an absolute
error below 1e-13, bound 1e-12 absolute.  The tables: 1 ulp of the float64 evaluation of their formulas."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_eval_mask_host as tm  # noqa: E402  (make_tree, FakePipe, numpy_evaluator, trimap_region: the mask loop's fixtures)
from test_eval_structure_device_gpu import make_case  # noqa: E402  (the recipe of the device tests)
from test_eval_matting_device_gpu import T, hand_maps  # noqa: E402  (the hand-made maps of the device tests)

NAMES = ("gp_eval_matting_workspace", "gp_eval_matting")
MASK_METRICS = ["mae", "mse", "sad", "max_f", "mean_f", "adp_f", "iou"]
STRUCTURE_METRICS = ["s_alpha", "max_e", "mean_e", "adp_e", "wf"]
MATTING_METRICS = ["grad", "conn"]
GP_ERR_INVALID = 1


def _libs():
    """Both element-type libraries as they stand in the tree (a missing one is an error, not a skip)."""
    from genpercept_amd import engine
    return [engine.load_library(p) for p in ("bf16", "fp16")]


# ---- the independent constructions -----------------------------------------------------------------------------------------------------------
def scipy_levels(q, g):
    from scipy import ndimage
    m = np.minimum(q, g)
    inside = np.zeros((11,) + q.shape, bool)
    for k in range(1, 11):
        lab, n = ndimage.label(m >= T[k - 1])                               # default structure: 4-connectivity; labels in raster order
        if n:
            sizes = np.bincount(lab.reshape(-1))[1:]
            inside[k] = lab == 1 + int(np.argmax(sizes))                    # the first among equal sizes = the one met first in raster order
    level = np.full(q.shape, 10, np.int64)
    for k in range(10, 0, -1):
        level[~inside[k]] = k - 1
    return level.astype(np.uint8)


def scipy_grad_map(q, g):
    from scipy import ndimage
    from genpercept_amd import eval_metrics as em

    def amp(x):
        lo, hi = int(x.min()), int(x.max())
        xn = (x.astype(np.float64) - lo) / float(hi - lo) if hi > lo else np.zeros(x.shape)
        gx = ndimage.correlate1d(ndimage.correlate1d(xn, em.GRAD_D, axis=1, mode="nearest"), em.GRAD_G, axis=0, mode="nearest")
        gy = ndimage.correlate1d(ndimage.correlate1d(xn, em.GRAD_G, axis=1, mode="nearest"), em.GRAD_D, axis=0, mode="nearest")
        return np.sqrt(gx * gx + gy * gy)

    return (amp(q) - amp(g)) ** 2


def all_cases():
    from genpercept_amd import eval_metrics as em
    out = []
    for shape in ((3, 64, 65), (1, 257, 515), (1, 7, 5), (1, 1, 2), (1, 1, 1), (1, 3, 8200)):
        pred, gt = make_case(*shape, seed=2000 + shape[1])
        q = em.quantize_mask(pred)
        out += [(f"recipe {shape} image {i}", q[i], gt[i]) for i in range(shape[0])]
    for h, w in ((6, 8), (64, 65)):
        out += [(f"{name} {h}x{w}", q, g) for name, (q, g) in hand_maps(h, w).items()]
    out += [(f"{name} 257x515", *hand_maps(257, 515)[name]) for name in ("serpentine", "checkerboard with pixel 0", "equal blocks")]
    return out


# ---- symbols and arguments -------------------------------------------------------------------------------------------------------------------
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
    assert len(engine.SYMBOLS["gp_eval_matting"][1]) == 14 and len(engine.SYMBOLS["gp_eval_matting_workspace"][1]) == 3
    assert engine.SYMBOLS["gp_eval_matting_workspace"][0] is C.c_longlong
    assert callable(engine.eval_matting_raw) and callable(engine.eval_matting)
    assert list(engine.MATTING_METRICS) == list(em.MATTING_METRICS) == list(ie.MATTING_METRICS) == MATTING_METRICS
    assert engine.MATTING_COUNTS == em.MATTING_COUNTS == 13 and engine.MATTING_OUT == len(engine.MATTING_OUT_NAMES) == 4
    assert em.CONN_T == T == [-((-255 * k) // 10) for k in range(1, 11)]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{n}`" in text for n in NAMES)


def test_workspace_size():
    for lib in _libs():
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
            assert lib.gp_eval_matting_workspace(*bad) == 0
        for h, w in ((1, 1), (1, 2), (7, 5), (64, 65), (1024, 1024), (1031, 2053), (3, 8200)):
            one = lib.gp_eval_matting_workspace(1, h, w)
            assert one >= 47 * h * w and one % 8 == 0          # the row sums, the three label arrays, the three byte maps
            assert lib.gp_eval_matting_workspace(7, h, w) == 7 * one and lib.gp_eval_matting_workspace(65535, h, w) == 65535 * one


def test_invalid_arguments_are_refused_without_a_gpu():
    """Every case is refused by the argument checks, which come before the first HIP call: the small integers that stand for device pointers
    are never dereferenced."""
    P, G, R, O, CN, LV, GM, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6001, 0x7000, 0x8000  # 8-byte aligned but the levels (bytes)
    for lib in _libs():
        need = lib.gp_eval_matting_workspace(2, 8, 8)
        ok = dict(pred=P, u8=0, gt=G, region=R, B=2, H=8, W=8, out=O, counts=CN, levels=LV, gmap=GM, ws=WS, nbytes=need)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.gp_eval_matting(a["pred"], a["u8"], a["gt"], a["region"], a["B"], a["H"], a["W"], a["out"], a["counts"], a["levels"], a["gmap"],
                                       a["ws"], a["nbytes"], None)

        huge = 1 << 62
        cases = [dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None),
                 dict(B=0), dict(B=-3), dict(H=0), dict(W=0), dict(H=-1), dict(W=-1),
                 dict(B=65536, nbytes=huge),                                                              # above the grid's limit
                 dict(B=1, H=65536, W=65536, nbytes=huge), dict(B=1, H=1 << 16, W=1 << 15, nbytes=huge),  # H * W > 2^31 - 1
                 dict(u8=-1), dict(u8=2), dict(pred=P + 2),
                 dict(out=O + 4), dict(counts=CN + 4), dict(counts=CN + 1), dict(gmap=GM + 4), dict(gmap=GM + 1), dict(ws=WS + 4),
                 dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-8), dict(nbytes=lib.gp_eval_matting_workspace(1, 8, 8))]
        for kw in cases:
            assert call(**kw) == GP_ERR_INVALID, kw


def test_binding_refuses_bad_inputs_before_the_library():
    from genpercept_amd import engine
    with pytest.raises(ValueError):
        engine.eval_matting_raw(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        engine.eval_matting_raw(torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
def test_filter_tables():
    """g(x) = exp(-x^2 / (2 s^2)) / (s sqrt(2 pi)), d(x) = -x g(x) / s^2, s = 1.4, x = -4..4, each table divided by its L2 norm.  The literals
    were generated in float64, so each entry is within 1 ulp of the float64 evaluation of these formulas; against the formulas in 60-digit
    decimals the float64 evaluation itself is off by the rounding of its exponent (|x^2 / (2 s^2)| <= 4.1 carries up to 4 ulp of relative
    error into exp) and of the norm: 16 ulp.  Half size 4 is what the toolboxes' rule gives for eps = 1e-2.  The same literals in the kernel
    file."""
    from decimal import Decimal, getcontext
    from genpercept_amd import eval_metrics as em
    getcontext().prec = 60
    s = Decimal("1.4")
    pi = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
    assert math.ceil(1.4 * math.sqrt(-2 * math.log(math.sqrt(2 * math.pi) * 1.4 * 1e-2))) == 4
    g = [(-(Decimal(x) ** 2) / (2 * s * s)).exp() / (s * (2 * pi).sqrt()) for x in range(-4, 5)]
    d = [-Decimal(x) * v / (s * s) for x, v in zip(range(-4, 5), g)]
    x = np.arange(-4, 5, dtype=np.float64)
    g64 = np.exp(-x * x / (2 * 1.4 * 1.4)) / (1.4 * np.sqrt(2 * np.pi))
    d64 = -x * g64 / (1.4 * 1.4)
    for table, exact, f64 in ((em.GRAD_G, g, g64), (em.GRAD_D, d, d64)):
        norm = sum(v * v for v in exact).sqrt()
        f64 = f64 / np.sqrt((f64 * f64).sum())
        assert table.shape == (9,) and table.dtype == np.float64
        for i, v in enumerate(exact):
            want = v / norm
            assert abs(table[i] - f64[i]) <= np.spacing(abs(f64[i])), i
            assert abs(Decimal(float(table[i])) - want) <= 16 * Decimal(float(np.spacing(abs(float(want))))), i
    assert em.GRAD_G[4] == float.fromhex("0x1.4506d2f73739dp-1") and em.GRAD_D[3] == float.fromhex("0x1.fcd0621654797p-2")
    assert em.GRAD_D[4] == 0.0 and not np.signbit(em.GRAD_D[4]) and em.GRAD_D[0] > 0
    assert np.array_equal(em.GRAD_G, em.GRAD_G[::-1]) and np.array_equal(em.GRAD_D, -em.GRAD_D[::-1])
    src = open(os.path.join(ROOT, "genpercept_amd", "csrc", "eval_matting.hip")).read()
    lit = r"-?0x[01]\.[0-9a-f]+p[-+][0-9]+"
    for name, end, hexes in (("MT_G[MT_TAPS]", "MT_D[MT_TAPS]", em.GRAD_G_HEX), ("MT_D[MT_TAPS]", "// the workspace", em.GRAD_D_HEX)):
        lits = re.findall(lit, src[src.index(name):src.index(end, src.index(name) + 1)])
        assert lits == re.findall(lit, hexes) and len(lits) == 9, name


# ---- conn ------------------------------------------------------------------------------------------------------------------------------------
def test_conn_levels_equal_the_scipy_construction():
    from genpercept_amd import eval_metrics as em
    full = set()
    for name, q, g in all_cases():
        level = em.conn_levels(q, g)
        want = scipy_levels(q, g)
        assert level.dtype == np.uint8 and level.shape == q.shape and np.array_equal(level, want), name
        r = em.conn_error(q, g)
        assert np.array_equal(r["level_counts"], np.bincount(want.reshape(-1), minlength=11)) and r["n"] == q.size
        assert np.array_equal(r["counts"], np.concatenate([[q.size, r["conn_num"]], r["level_counts"]])) and r["counts"].shape == (13,)
        lv = want.astype(np.int64)
        dg, dq = 10 * g.astype(np.int64) - 255 * lv, 10 * q.astype(np.int64) - 255 * lv
        num = int(np.abs(dg * (dg / 2550.0 >= 0.15) - dq * (dq / 2550.0 >= 0.15)).sum())          # the published form of the cut
        assert r["conn_num"] == num and r["conn"] == num / 2550000.0, name
        if (r["level_counts"] > 0).all():
            full.add(name)
    assert {"recipe (3, 64, 65) image 0", "recipe (1, 257, 515) image 0"} <= full       # the recipe fills all eleven levels
    # the recipe's scores: conn_num / 2550 (the sum in alpha units) is 332.7 and 10529.4; conn is that in thousands
    for shape, units in (((3, 64, 65), 332.7), ((1, 257, 515), 10529.4)):
        pred, gt = make_case(*shape, seed=2000 + shape[1])
        r = em.conn_error(em.quantize_mask(pred)[0], gt[0])
        assert round(r["conn_num"] / 2550.0, 1) == units and r["conn"] == r["conn_num"] / 2550000.0


def test_conn_hand_made_maps():
    from genpercept_amd import eval_metrics as em
    one = np.array([[200]], np.uint8)
    assert em.conn_levels(one, one)[0, 0] == 7 and em.conn_error(one, one)["conn_num"] == 0          # T_7 = 179 <= 200 < T_8 = 204
    assert em.conn_levels(one, np.array([[20]], np.uint8))[0, 0] == 0
    r = em.conn_error(one, np.array([[20]], np.uint8))
    assert r["conn_num"] == 2000 and r["conn"] == 2000 / 2550000.0                                   # dq = 2000 >= 383, dg = 200 < 383
    maps = hand_maps(64, 65)
    q, g = maps["all 255"]
    assert (em.conn_levels(q, g) == 10).all() and em.conn_error(q, g)["conn"] == 0.0
    q, g = maps["same"]
    assert em.conn_error(q, g)["conn"] == 0.0 and em.grad_error(q, g)["grad"] == 0.0 and not em.grad_error_map(q, g).any()
    q, g = maps["serpentine both"]
    assert np.array_equal(em.conn_levels(q, g), (q == 255) * 10)                                     # one component through every row
    q, g = maps["checkerboard with pixel 0"]
    lv = em.conn_levels(q, g)
    assert lv[0, 0] == 10 and lv.sum() == 10                                                         # Omega_k = { pixel 0 } for every k
    q, g = maps["checkerboard without pixel 0"]
    lv = em.conn_levels(q, g)
    assert lv[0, 1] == 7 and lv.sum() == q.size + 6                                                  # I_1 is everything; then pixel 1 alone, up to 200
    q, g = maps["equal blocks"]
    lv = em.conn_levels(q, g)
    assert (lv[1:3, 1:4] == 10).all() and lv.sum() == 60                                             # the tie goes to the smaller index
    q, g = maps["fading"]
    assert em.conn_levels(q, g).max() == 5
    q, g = maps["thresholds"]
    lv = em.conn_levels(q, g)
    for k in range(1, 11):
        assert (lv[q == T[k - 1] - 1] <= k - 1).all() and (lv[q < T[0]] == 0).all()
    # the float form of the published code puts byte 153 on the other side of k = 6 when the thresholds come from np.arange(0, 1.1, 0.1)
    assert not (153 / 255.0 >= np.arange(0, 1.1, 0.1)[6]) and 153 >= T[5]


def test_region_restricts_only_the_sums():
    from genpercept_amd import eval_metrics as em
    pred, gt = make_case(3, 64, 65, seed=2064)
    q = em.quantize_mask(pred)
    rng = np.random.RandomState(3)
    for i in range(3):
        region = rng.rand(64, 65) < 0.3
        level = em.conn_levels(q[i], gt[i])
        term = em._conn_terms(q[i], gt[i], level)
        r, whole = em.conn_error(q[i], gt[i], region), em.conn_error(q[i], gt[i])
        assert r["conn_num"] == int(term[region].sum()) and r["n"] == int(region.sum()) and np.array_equal(r["level_counts"], whole["level_counts"])
        assert r["conn_num"] < whole["conn_num"] == int(term.sum())
        err = em.grad_error_map(q[i], gt[i])
        gr = em.grad_error(q[i], gt[i], region.astype(np.uint8) * 7)
        assert gr["grad_sum"] == float(err[region].sum()) and gr["grad"] == gr["grad_sum"] / 1000.0 and gr["n"] == r["n"]
        m = em.matting_metrics(pred[i], gt[i], region)
        assert list(m) == MATTING_METRICS and m["conn"] == r["conn"] and m["grad"] == gr["grad"]
    empty = em.conn_error(q[0], gt[0], np.zeros((64, 65), bool))
    assert empty["n"] == 0 and math.isnan(empty["conn"]) and math.isnan(em.grad_error(q[0], gt[0], np.zeros((64, 65), bool))["grad"])
    with pytest.raises(ValueError):
        em.conn_error(q[0], gt[0], np.zeros((3, 3), bool))


def test_the_labelling_is_fast_enough():
    """257 x 515, the recipe and the serpentine (one component of 66 563 pixels and 257 turns): array operations only."""
    import time
    from genpercept_amd import eval_metrics as em
    pred, gt = make_case(1, 257, 515, seed=2257)
    t0 = time.perf_counter()
    em.matting_metrics(pred[0], gt[0])
    em.conn_levels(*hand_maps(257, 515)["serpentine"])
    assert time.perf_counter() - t0 < 5.0


# ---- grad ------------------------------------------------------------------------------------------------------------------------------------
def test_grad_error_map_equals_the_scipy_construction():
    from genpercept_amd import eval_metrics as em
    worst = 0.0
    for name, q, g in all_cases():
        err = em.grad_error_map(q, g)
        want = scipy_grad_map(q, g)
        assert err.dtype == np.float64 and err.shape == q.shape and np.isfinite(err).all() and err.max() <= 16.0, name
        worst = max(worst, float(np.abs(err - want).max()))
        assert np.abs(err - want).max() <= 1e-12, name
    print("grad_error_map against correlate1d: largest absolute difference", worst)
    const = np.full((9, 12), 77, np.uint8)
    assert not em._grad_amp(const).any()                                                             # a constant map: all zeros, amp = 0
    ramp = np.arange(12, dtype=np.uint8)[None].repeat(9, 0)
    assert np.array_equal(em.grad_error_map(const, ramp), em._grad_amp(ramp) ** 2) and em._grad_amp(ramp)[4, 6] > 0.05
    for shape in ((7, 5), (1, 2), (1, 1), (2, 1)):                                                  # smaller than the filter
        rng = np.random.RandomState(shape[0])
        q, g = rng.randint(0, 256, shape).astype(np.uint8), rng.randint(0, 256, shape).astype(np.uint8)
        assert np.abs(em.grad_error_map(q, g) - scipy_grad_map(q, g)).max() <= 1e-12


# ---- the file route and the loop -------------------------------------------------------------------------------------------------------------
def numpy_matting_evaluator(pred, gt, region):
    """engine.eval_matting's contract on CPU tensors."""
    from genpercept_amd import eval_metrics as em
    assert pred.dtype == torch.float32 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    return [em.matting_metrics(pred[i].numpy(), gt[i].numpy(), None if region is None else region[i].numpy()) for i in range(pred.shape[0])]


@pytest.mark.parametrize("with_region", [False, True])
def test_matting_off_leaves_the_files_as_they_are_and_on_adds_two_columns(tmp_path, with_region):
    from genpercept_amd import eval_metrics as em
    from genpercept_amd import infer_eval as ie
    from test_eval_structure_host import numpy_structure_evaluator
    base, pred_dir = str(tmp_path / "data"), str(tmp_path / "pred")
    samples = tm.make_tree(base)
    region_of = tm.trimap_region(base) if with_region else None
    ie.run_inference(tm.FakePipe(), base, samples, pred_dir, ie.FileNameMode.id, mode="matting")
    outs = {k: str(tmp_path / k) for k in ("file_default", "file_off", "file_on", "loop_default", "loop_off", "loop_on")}
    common = dict(region_of=region_of)
    loop = dict(batch_size=2, evaluator=tm.numpy_evaluator, region_of=region_of)
    r_default = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_default"], **common)
    r_off = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_off"], matting=False, **common)
    r_on = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, output_dir=outs["file_on"], matting=True, **common)
    l_default = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_default"], **loop)
    l_off = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_off"], matting=False, matting_evaluator=None, **loop)
    l_on = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", output_dir=outs["loop_on"], matting=True,
                                       matting_evaluator=numpy_matting_evaluator, **loop)
    assert r_default == r_off == l_default == l_off and list(r_off) == MASK_METRICS + ["max_f_dataset"]
    assert list(r_on) == list(l_on) == MASK_METRICS + MATTING_METRICS + ["max_f_dataset"] and r_on == l_on
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
    assert csv_on.splitlines()[0] == "filename," + ",".join(MASK_METRICS + MATTING_METRICS) and txt_on[-2] == "  ".join(MASK_METRICS + MATTING_METRICS)
    assert txt_on[-1] == "  ".join(f"{r_on[k]:.6g}" for k in MASK_METRICS + MATTING_METRICS)
    rows = []
    for line_off, line_on, s in zip(csv_off.splitlines()[1:], csv_on.splitlines()[1:], samples):
        name = os.path.join(os.path.dirname(s[0]), ie.get_pred_name(os.path.basename(s[0]), ie.FileNameMode.id, suffix=".npy"))
        gt = ie.read_gt_mask(os.path.join(base, s[1]))
        m = em.matting_metrics(np.load(os.path.join(pred_dir, name)), gt, None if region_of is None else region_of(s, gt))
        assert line_on == line_off + "," + ",".join(str(m[k]) for k in MATTING_METRICS)
        rows.append(m)
    for k in MATTING_METRICS:
        assert r_on[k] == sum(m[k] for m in rows) / len(rows) and r_on[k] > 0.0, k
    if not with_region:                                                                              # both flags: structure first, then matting
        both = ie.infer_and_evaluate_masks(tm.FakePipe(), base, samples, "matting", batch_size=2, evaluator=tm.numpy_evaluator, structure=True,
                                           structure_evaluator=numpy_structure_evaluator, matting=True, matting_evaluator=numpy_matting_evaluator)
        both_f = ie.evaluate_mask_predictions(pred_dir, base, samples, ie.FileNameMode.id, structure=True, matting=True)
        assert list(both) == MASK_METRICS + STRUCTURE_METRICS + MATTING_METRICS + ["max_f_dataset"] and both == both_f
        assert all(both[k] == r_on[k] for k in r_on)
