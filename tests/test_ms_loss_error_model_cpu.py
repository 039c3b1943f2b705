"""CPU: the checks of tests/test_gpu_ms_loss.py bite.  tests/_ms_loss_ref.py restates K29 (az_ms_loss.hip) per pixel in float32
and states the rules a GPU result is held to; here
  * the restatement agrees with the reference's own fp64 evaluation of dispnet_disp and default_disp
    (tests/golden/g17_ms_loss.npz) under the derived golden bounds;
  * the launch constants the map sizes are built around are still in the source;
  * the restatement passes its own rules on every case, and each wrong kernel of MUTANTS -- a deliberately wrong copy of the
    restatement playing the kernel -- is rejected by the rules on at least one case, which is named;
  * az_ms_loss_fwd / _bwd are in the C ABI, exported, and validate on the host before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest

from activezero_amd import _lib, build
from tests import _ms_loss_ref as M
from tests import _reduce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_ms_loss.npz")


# ---- the restatement against the reference's fp64 evaluation -------------------------------------------------------------
@pytest.mark.parametrize("name,nd", [("dispnet", 7), ("default", 1)])
def test_restatement_agrees_with_the_reference_in_fp64(name, nd, capsys):
    g = np.load(GOLDEN)
    preds = [g[f"{name}_pred{k}"] for k in range(nd)]
    gt, mask = g[f"{name}_gt"], g[f"{name}_mask"]
    shifts = tuple(range(nd))
    weights = M.DISPNET_WEIGHTS[:nd] if name == "dispnet" else (1.0,)
    assert [p.shape for p in preds] == [(gt.shape[0], 1, gt.shape[2] >> s, gt.shape[3] >> s) for s in shifts]
    loss, _, means, _ = M.ms_scalars(preds, shifts, weights, gt, mask, 0.0, math.inf)
    ratios = {"loss": M.golden_scalar_ratio(np.float32(loss), g[f"{name}_loss64"], f"{name} loss")}
    for k in range(nd):
        ratios[f"mean{k}"] = M.golden_scalar_ratio(np.float32(means[k]), g[f"{name}_means64"][k], f"{name} mean {k}")
    # the reference's own float32 result: the same five units (its terms round as ours do, its mean sums in float32 pairwise)
    assert abs(float(g[f"{name}_loss32"]) - float(g[f"{name}_loss64"])) <= 5 * 2.0 ** -24 * float(g[f"{name}_loss64"])
    counts = [c for _, c in M.ms_fwd(preds, shifts, gt, mask, 0.0, math.inf)]
    assert all(c >= 1 for c in counts) and counts[0] > 1000 * (nd > 1)
    grads = M.ms_bwd(preds, shifts, weights, gt, mask, 0.0, math.inf, 1.0, counts)
    for k in range(nd):
        ratios[f"grad{k}"] = M.golden_grad_ratio(grads[k], g[f"{name}_grad64_{k}"], weights[k], counts[k], f"{name} grad {k}")
        assert np.array_equal(grads[k] == 0, g[f"{name}_grad64_{k}"] == 0)
    with capsys.disabled():
        print(f"\n  {name}: restatement err / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()), end="")
    # the range forms name the same pixels: the masks were built as 0 < gt < 64
    assert np.array_equal(M.ms_fwd_acc(preds, shifts, gt, None, 0.0, 64.0), M.ms_fwd_acc(preds, shifts, gt, mask, 0.0, math.inf))


def test_one_valid_pixel_leaves_the_other_scales_empty():
    """the issue's example: one valid pixel at (1, 1) gives [4.5, nan, ...]; the empty scales' gradients are zeros"""
    gt = np.full((1, 1, 64, 64), 10.0, dtype=M.F32)
    mask = np.zeros((1, 1, 64, 64), dtype=np.uint8)
    mask[0, 0, 1, 1] = 1
    shifts = tuple(range(7))
    preds = [np.full((1, 1, 64 >> s, 64 >> s), 15.0, dtype=M.F32) for s in shifts]
    loss, _, means, _ = M.ms_scalars(preds, shifts, M.DISPNET_WEIGHTS, gt, mask, 0.0, math.inf)
    assert means[0] == 4.5 and all(math.isnan(m) for m in means[1:]) and math.isnan(loss)
    counts = [c for _, c in M.ms_fwd(preds, shifts, gt, mask, 0.0, math.inf)]
    grads = M.ms_bwd(preds, shifts, M.DISPNET_WEIGHTS, gt, mask, 0.0, math.inf, 1.0, counts)
    assert counts == [1, 0, 0, 0, 0, 0, 0] and grads[0][0, 0, 1, 1] == 1.0 and int((grads[0] != 0).sum()) == 1
    assert all(np.array_equal(g, np.zeros_like(g)) for g in grads[1:])


# ---- the constants in the source ------------------------------------------------------------------------------------------
def test_the_launch_constants_are_still_in_the_source():
    with open(os.path.join(ROOT, "activezero_amd", "csrc", "az_ms_loss.hip")) as f:
        src = f.read()
    assert "#define MS_BLOCK 256" in src and M.BLOCK == 256
    assert "#define MS_GRID_CAP 1024 " in src and M.GRID_CAP == 1024
    assert "blocks += g > MS_GRID_CAP ? MS_GRID_CAP : g;" in src  # one cap, forward and backward
    assert src.count("hipLaunchKernelGGL(") == 2 and src.count("dim3(grid), dim3(MS_BLOCK)") == 2
    assert "az_block_sum_f64<2, MS_BLOCK>(v, acc + 2 * k);" in src
    assert _lib.CONST["AZ_MS_LOSS_MAX"] == M.MS_LOSS_MAX == 8
    assert M.N_BIG == 262437 and 4 * M.N_BIG < 1.1 * 2 ** 20  # the one large map: 1 MB


# ---- mutants ----------------------------------------------------------------------------------------------------------------
def _fwd(defect):
    for c in M.all_cases():
        for mode, mask, lo, hi in M.modes(c):
            args = (c["preds"], c["shifts"], c["gt"], mask, lo, hi)
            yield (f"az_ms_loss_fwd {c['name']} {mode}", lambda: M.ms_fwd_acc(*args, defect=defect), lambda got: M.check_fwd(got, *args))


def _bwd(defect):
    for c in M.all_cases(nonfinite_preds=True):
        for mode, mask, lo, hi in M.modes(c):
            counts = [n for _, n in M.ms_fwd(c["preds"], c["shifts"], c["gt"], mask, lo, hi)]
            args = (c["preds"], c["shifts"], c["weights"], c["gt"], mask, lo, hi, M.GLOSS, counts)
            yield (f"az_ms_loss_bwd {c['name']} {mode}", lambda: M.ms_bwd(*args, defect=defect), lambda got: M.check_bwd(got, *args))


MUTANTS = [  # (what is wrong, the runs it is tried on, the defect of tests/_ms_loss_ref.py)
    ("source index dst * 2^s + 1", _fwd, "src_plus1"),
    ("scale sizes by ceil instead of floor", _fwd, "ceil_size"),
    ("the mask read at the prediction's own index (forward)", _fwd, "mask_own_index"),
    ("the mask read at the prediction's own index (backward)", _bwd, "mask_own_index"),
    ("one shared count for all scales (forward)", _fwd, "shared_count"),
    ("one shared count for all scales (backward)", _bwd, "shared_count"),
    ("the weights in reverse order", _bwd, "weights_reversed"),
    ("w * (s * clamp) for (w * s) * clamp", _bwd, "mul_order"),
    ("the last n % 256 pixels of a prediction dropped (forward)", _fwd, "tail"),
    ("the last n % 256 pixels of a prediction dropped (backward)", _bwd, "tail"),
    ("only the first grid pass taken (forward)", _fwd, "one_pass"),
    ("only the first grid pass taken (backward)", _bwd, "one_pass"),
    ("a batch stride of h * w for the gt read (forward)", _fwd, "batch_stride_hw"),
    ("a batch stride of h * w for the gt read (backward)", _bwd, "batch_stride_hw"),
    ("an empty scale multiplied instead of selected", _bwd, "empty_mul"),
    ("a gradient clamp through fmin / fmax that drops NaN", _bwd, "clamp_fmin"),
]


@pytest.mark.parametrize("runs", [_fwd, _bwd], ids=lambda f: f.__name__[1:])
def test_the_restatement_passes_its_own_rules_on_every_case(runs):
    n = 0
    for name, kernel, rule in runs(None):
        rule(kernel())
        n += 1
    assert n == 4 * (len(M.FLAT_SHAPES) + len(M.SHAPES) + 2)


def test_the_scalar_rule_accepts_the_formula_and_rejects_a_wrong_weight():
    for c in M.all_cases()[-3:-1]:
        for mode, mask, lo, hi in M.modes(c):
            args = (c["preds"], c["shifts"], c["weights"], c["gt"], mask, lo, hi)
            loss, _, means, _ = M.ms_scalars(*args)
            M.check_scalars(np.float32(loss), np.asarray(means, dtype=np.float32), *args)
            wrong = loss - (c["weights"][3] - c["weights"][4]) * means[3]  # scale 3 with scale 4's weight
            with pytest.raises(AssertionError, match="loss"):
                M.check_scalars(np.float32(wrong), np.asarray(means, dtype=np.float32), *args)
            with pytest.raises(AssertionError, match=r"scale_means\[2\]"):
                M.check_scalars(np.float32(loss), np.asarray(means[:2] + [means[3]] + means[3:], dtype=np.float32), *args)


@pytest.mark.parametrize("what,runs,defect", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_rejected_by_the_rules(what, runs, defect, capsys):
    tried = 0
    for name, kernel, rule in runs(defect):
        tried += 1
        try:
            rule(kernel())
        except AssertionError as err:
            with capsys.disabled():
                print(f"\n  mutant '{what}' rejected by case {tried}: {name}\n    {err}", end="")
            return
    pytest.fail(f"mutant '{what}' survived all {tried} cases: a case is missing")


def test_the_special_pixels_sit_where_kernels_go_wrong():
    assert M.special_positions(693 // 3 * 3, 231) == [0, 230, 231, 255, 256, 461, 462, 511, 512, 692]
    assert M.special_positions(M.N_BIG, M.N_BIG) == [0, 255, 256, 511, 512, 262143, 262144, M.N_BIG - 1]
    big = M.all_cases()[-1]
    assert big["preds"][0].size == M.N_BIG and big["shifts"] == (0,)
    for i in M.special_positions(M.N_BIG, M.N_BIG):  # valid under the mask and under both ranges
        assert big["mask"].ravel()[i] != 0 and 1.0 < big["gt"].ravel()[i] < 192.0
    only0 = M.all_cases()[len(M.FLAT_SHAPES)]
    for mode, mask, lo, hi in M.modes(only0):
        counts = [n for _, n in M.ms_fwd(only0["preds"], only0["shifts"], only0["gt"], mask, lo, hi)]
        assert counts[0] > 100 and counts[1:] == [0, 0, 0], mode
    for c in M.all_cases():  # every scale of every other case has valid pixels under every mode; sizes are the floors
        B, H, W = c["shape"]
        assert [p.shape for p in c["preds"]] == [(B, 1, H >> s, W >> s) for s in c["shifts"]]
        if c is not only0:
            for mode, mask, lo, hi in M.modes(c):
                assert all(n >= 1 for _, n in M.ms_fwd(c["preds"], c["shifts"], c["gt"], mask, lo, hi)), (c["name"], mode)
    assert [c["preds"][-1].shape[2:] for c in M.all_cases()[-3:-1]] == [(1, 1), (1, 3)]


# ---- the entry points in the C ABI ------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_validate_on_the_host():
    build.build()
    handle = _lib.lib()
    for name in ("az_ms_loss_fwd", "az_ms_loss_bwd"):
        assert name in _lib.declared_symbols() and hasattr(handle, name)
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # additive change
    assert _lib.MS_LOSS_DESC.itemsize == 32 and _lib.MS_LOSS_DESC.names == ("pred", "grad", "shift", "h", "w", "reserved")
    OK, EINVAL, ENULL = (_lib.CONST[k] for k in ("AZ_OK", "AZ_EINVAL", "AZ_ENULL"))
    buf = (ctypes.c_double * 32)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    B, H, W = 2, 67, 131

    def table(rows):
        d = np.zeros(len(rows), dtype=_lib.MS_LOSS_DESC)
        for k, r in enumerate(rows):
            d[k] = r
        return d

    good = table([(p, p, s, H >> s, W >> s, 0) for s in range(7)])
    wts = np.ones(8, dtype=np.float32)

    def fwd(acc=p, descs=good, nd=None, gt=p, b=B, h=H, w=W):
        return handle.az_ms_loss_fwd(acc, None if descs is None else descs.ctypes.data, len(descs) if nd is None else nd, gt,
                                     None, 0.0, math.inf, b, h, w, None)

    def bwd(descs=good, weights=wts, nd=None, gt=p, gloss=p, acc=p, b=B, h=H, w=W):
        return handle.az_ms_loss_bwd(None if descs is None else descs.ctypes.data, None if weights is None else weights.ctypes.data,
                                     len(descs) if nd is None else nd, gt, None, 0.0, math.inf, gloss, acc, b, h, w, None)

    # every call below fails validation or has nothing to do: none launches
    assert fwd(acc=None) == ENULL and fwd(gt=None) == ENULL and fwd(descs=None, nd=1) == ENULL
    assert bwd(acc=None) == ENULL and bwd(gt=None) == ENULL and bwd(gloss=None) == ENULL and bwd(weights=None) == ENULL
    assert bwd(descs=None, nd=1) == ENULL
    assert fwd(nd=0) == EINVAL and bwd(nd=0) == EINVAL
    nine = table([(p, p, 0, H, W, 0)] * 9)
    assert fwd(descs=nine) == EINVAL and bwd(descs=nine) == EINVAL and fwd(descs=nine, nd=8, b=0) == OK
    assert fwd(descs=table([(0, p, 0, H, W, 0)])) == ENULL
    for bad in ((p, p, 1, H >> 1, (W >> 1) + 1, 0),   # ceil, not floor
                (p, p, 1, (H >> 1) + 1, W >> 1, 0),
                (p, p, 0, H, W - 1, 0),
                (p, p, 7, 0, 1, 0),                   # H < 2^s: a zero-sized scale
                (p, p, 8, 0, 0, 0),
                (p, p, -1, H, W, 0), (p, p, 31, 0, 0, 0)):
        assert fwd(descs=table([bad])) == EINVAL and bwd(descs=table([bad])) == EINVAL, bad
    assert fwd(b=-1) == EINVAL
    assert fwd(b=0) == OK and bwd(b=0) == OK  # an empty batch: nothing to launch
    assert bwd(descs=table([(p, 0, s, H >> s, W >> s, 0) for s in range(7)])) == OK  # no gradient wanted: nothing to launch
