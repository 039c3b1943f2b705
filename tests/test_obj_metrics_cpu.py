"""CPU: the checks of tests/test_gpu_obj_metrics.py and tests/test_gpu_eval_mask.py bite.  tests/_obj_metrics_ref.py restates
K22 az_obj_metrics through _reduce_ref.k12_metrics and K23 az_eval_mask per pixel; here
  * the restatements give hand-written known answers, and K23's agrees with F.interpolate and the cast chain of the
    reference's test.py:112-193 on the CPU;
  * the entry points are in the C ABI (version 6: additive) and validate on the host, before any launch;
  * the launch constants the sizes are built around are still in the source;
  * the restatement passes its own rules on every case of the GPU test, and each wrong kernel of MUTANTS -- a deliberately
    wrong copy of the restatement playing the kernel -- is rejected by the rules on one of those cases, which is named."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from activezero_amd import _lib, build
from tests import _obj_metrics_ref as O
from tests import _reduce_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "activezero_amd", "csrc")
F32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


# ---- K22: known answers --------------------------------------------------------------------------------------------
def _tiny(dp, mask, label, L=3):
    n = len(dp)
    a = lambda v: np.asarray(v, dtype=F32).reshape(1, 1, 1, n)
    return dict(dg=a([10] * n), zg=a([0.5] * n), dp=a(dp), zp=a([0.5] * n), fb=np.array([5.0], dtype=F32),
                mask=np.asarray(mask, dtype=np.uint8).reshape(1, 1, 1, n), label=np.asarray(label, dtype=np.int32).reshape(1, 1, 1, n),
                L=L, B=1, n=n, per_batch=n, name="tiny")


def test_known_answers_of_the_restatement():
    #            label 0      label 1           label 2: present, fully masked     outside on either side
    c = _tiny(dp=[9.5, 8.5, 7.75, NAN, 7.0, 1.0, 1.0, 8.0], mask=[1, 1, 1, 0, 0, 1, 1, 2],
              label=[0, 1, 1, 1, 2, 3, -1, 0])
    acc, present, stats = O.k22_exact(c, c["zp"])
    assert stats.tolist() == [2]
    assert present.tolist() == [[2, 3, 1]]  # the unmasked NaN pixel of label 1 is present; the outside pixels nowhere
    # dd: label 0 {0.5, 2}, label 1 {1.5, 2.25}; explicit depth_pred == depth_gt: no depth error
    assert acc[0, 0].tolist() == [2.5, 1, 0, 0, 0, 0, 0, 2]   # dd = 2 is not > 2; mask byte 2 counts
    assert acc[0, 1].tolist() == [3.75, 2, 1, 0, 0, 0, 0, 2]
    assert acc[0, 2].tolist() == [0] * 8
    O.check_k22((acc, present, stats), c, c["zp"])
    # the focal-length path: depth_pred = 5 / dp; label 0: |0.5 - 5/9.5| = 26.3 mm and |0.5 - 5/8| = 125 mm -> clipped to 100
    acc, _, _ = O.k22_exact(c, None)
    assert acc[0, 0, 4:].tolist() == [2, 2, 2, 2]
    assert abs(acc[0, 0, 3] - (1000 * abs(0.5 - 5 / 9.5) + 100)) < 1e-3


def test_a_nan_prediction_poisons_the_sums_of_its_own_object_only():
    c = _tiny(dp=[9.5, NAN, 7.75, 7.0], mask=[1, 1, 1, 1], label=[0, 1, 1, 2])
    acc, present, stats = O.k22_exact(c, None)
    assert math.isnan(acc[0, 1, 0]) and math.isnan(acc[0, 1, 3]) and acc[0, 1, 7] == 2
    assert acc[0, 1, 1] == 1 and acc[0, 1, 4] == 1  # NaN > t is false: the finite pixel alone is counted (5 / 7.75 is 145 mm off)
    assert np.isfinite(acc[0, 0]).all() and np.isfinite(acc[0, 2]).all() and acc[0, 2, 0] == 3.0
    O.check_k22((acc, present, stats), c, None)
    clean = acc.copy()
    clean[0, 1, 0] = 2.25  # a kernel that dropped the NaN
    with pytest.raises(AssertionError, match="label 1 acc\\[0\\]"):
        O.check_k22((clean, present, stats), c, None)
    spread = acc.copy()
    spread[0, 0, 0] = NAN  # ... or let it reach another object
    with pytest.raises(AssertionError, match="label 0 acc\\[0\\]"):
        O.check_k22((spread, present, stats), c, None)


def test_known_answers_of_the_wrappers_formulas():
    c = _tiny(dp=[9.5, 8.5, 7.75, 9.0, 7.0], mask=[1, 1, 1, 0, 0], label=[0, 1, 1, 1, 2])
    vals, lims, count = O.obj_err_scalars(c, c["zp"], per_image=False)
    assert count.tolist() == [1, 1, 1]
    assert vals[0, 0] == 0.5 and vals[0, 1] == (1.5 + 2.25) / 2 and math.isnan(vals[0, 2])  # present, fully masked: NaN, count 1
    assert vals[1, :2].tolist() == [0, 0] and vals[2, :2].tolist() == [0, 0] and (lims[:, :2] < 1e-3).all()


# ---- the C surface --------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_typed(handle):
    P, I, Q, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    declared = _lib.declared_symbols()
    for name in ("az_obj_metrics", "az_eval_mask"):
        assert name in declared and getattr(handle, name).argtypes == _lib._SIGS[name]
    assert _lib._SIGS["az_obj_metrics"] == [P] * 10 + [I, I, Q, P]
    assert _lib._SIGS["az_eval_mask"] == [P] * 5 + [I] * 3 + [P] + [I] * 6 + [Fl, I, Fl, P]
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # entry points were only added
    assert _lib.CONST["AZ_OBJ_MAX_LABELS"] == O.MAX_LABELS == 64


def test_obj_metrics_rejects_before_any_launch(handle):
    """every call below must be refused on the host: there is no device here"""
    buf = (ctypes.c_double * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ENULL, EINVAL, EUNSUP = (_lib.CONST[k] for k in ("AZ_ENULL", "AZ_EINVAL", "AZ_EUNSUPPORTED"))

    def call(acc=p, present=p, stats=p, dg=p, zg=p, dp=p, zp=None, fb=p, mask=p, label=None, B=1, L=1, per_image=4):
        return handle.az_obj_metrics(acc, present, stats, dg, zg, dp, zp, fb, mask, label, B, L, per_image, None)

    for hole in ("acc", "present", "stats", "dg", "zg", "dp", "mask"):
        assert call(**{hole: None}) == ENULL, hole
    assert call(fb=None) == ENULL and call(fb=None, zp=p, B=0) == 0  # one depth source is required; B = 0: nothing to do
    assert call(L=0) == EINVAL and call(L=-1) == EINVAL and call(B=-1) == EINVAL and call(per_image=-1) == EINVAL
    assert call(L=65) == EUNSUP and call(L=64, B=0) == 0 and call(L=17, per_image=0) == 0
    assert call(per_image=2 ** 31) == EUNSUP


def test_eval_mask_rejects_before_any_launch(handle):
    buf = (ctypes.c_double * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ENULL, EINVAL = _lib.CONST["AZ_ENULL"], _lib.CONST["AZ_EINVAL"]

    def call(mask=p, count=p, disp=p, depth=p, robot=None, r64=0, hr=0, wr=0, rs=None, s64=0, hs=0, ws=0, B=1, H=2, W=2, bg=1):
        return handle.az_eval_mask(mask, count, disp, depth, robot, r64, hr, wr, rs, s64, hs, ws, B, H, W, 192.0, bg, 1.25, None)

    for hole in ("mask", "count", "disp", "depth"):
        assert call(**{hole: None}) == ENULL, hole
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -2}) == EINVAL
    assert call(robot=p, hr=0, wr=4) == EINVAL and call(robot=p, hr=4, wr=-1) == EINVAL and call(robot=p, r64=2, hr=2, wr=2) == EINVAL
    assert call(rs=p, hs=0, ws=4) == EINVAL and call(rs=p, hs=4, ws=0) == EINVAL and call(rs=p, s64=-1, hs=2, ws=2) == EINVAL


def test_the_python_surface():
    from activezero_amd import ops
    from activezero_amd.utils import cascade_metrics as cm, gt_prep

    def params(fn):
        return [(n, q.default) for n, q in inspect.signature(fn).parameters.items()]

    none = inspect.Parameter.empty
    assert params(ops.obj_metrics) == [("disp_gt", none), ("depth_gt", none), ("disp_pred", none), ("mask", none), ("label", None),
                                       ("num_labels", 1), ("focal_x_baseline", None), ("depth_pred", None)]
    assert params(cm.compute_obj_err) == params(cm.compute_obj_err_per_image) == [
        ("disp_gt", none), ("depth_gt", none), ("disp_pred", none), ("focal_length", none), ("baseline", none), ("label", none),
        ("mask", none), ("obj_total_num", 17)]
    assert params(cm.compute_err_metric_per_image) == params(cm.compute_err_metric)
    assert params(gt_prep.prepare_test_mask) == [("img_disp_l", none), ("img_depth_l", none), ("max_disp", none), ("exclude_bg", True),
                                                 ("robot_mask", None), ("realsense_depth", None), ("depth_hi", 1.25)]
    d = torch.zeros(1, 1, 4, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.obj_metrics(d, d, d, d > 0, focal_x_baseline=torch.ones(1))
    with pytest.raises(RuntimeError, match="GPU"):
        gt_prep.prepare_test_mask(d, d, 192)
    assert ops.MAX_LABELS == 64
    # the buffer the three outputs share: fp64 words, the int32 part padded to whole words
    assert [ops._obj_words(b, nl) for b, nl in ((1, 1), (1, 2), (4, 17), (3, 64))] == [9, 18, 579, 1633]
    acc, present, stats = ops._obj_views(np.arange(18.0), 1, 2)
    assert acc.shape == (1, 2, 8) and present.shape == (1, 2) and present.dtype == np.int32 and stats.shape == (1,)


# ---- the launch constants ------------------------------------------------------------------------------------------
def test_the_launch_constants_are_still_in_the_source():
    with open(os.path.join(CSRC, "az_obj_metrics.hip")) as f:
        src = f.read()
    assert "#define OM_BLOCK 256" in src and O.BLOCK == 256
    assert "#define OM_GRID_CAP 1024  // workgroups over all images" in src and O.GRID_CAP == 1024
    assert "long long bpi = (per_image + OM_BLOCK - 1) / OM_BLOCK;" in src
    assert "const long long cap = B >= OM_GRID_CAP ? 1 : OM_GRID_CAP / B;" in src and "if (bpi > cap) bpi = cap;" in src
    assert "dim3((unsigned)(bpi * B)), dim3(OM_BLOCK)" in src
    assert "const long long stride = (long long)blocks_per_image * OM_BLOCK;" in src
    assert [O.blocks_per_image(b, p) for b, p in ((1, 1), (1, 256), (1, 257), (1, O.N_CAP), (3, 231), (2, 10 ** 6), (2000, 300))] == \
        [1, 1, 2, 1024, 1, 512, 1]
    assert O.N_CAP == 262437 and O.N_CAP > O.GRID_CAP * O.BLOCK
    # K12 and K22 share one statement of the per-pixel terms
    with open(os.path.join(CSRC, "az_disp_loss.hip")) as f:
        k12 = f.read()
    for text in (src, k12):
        assert '#include "az_disp_terms.h"' in text and "az_dm_pixel(" in text and "2e-3f" not in text and "1000.f" not in text


# ---- the rules against the restatement and against wrong kernels ---------------------------------------------------
_CASES = {}


def all_cases():
    """the GPU test's own inputs, smallest images first, built once"""
    for k in range(len(O.SHAPES)):
        if k not in _CASES:
            _CASES[k] = list(O.cases(k))
        yield from _CASES[k]


def test_the_restatement_passes_its_own_rules_on_every_case():
    n = 0
    for c, path, zp in all_cases():
        O.check_k22(O.k22_exact(c, zp), c, zp, what=path)
        n += 1
    assert n == len(O.SHAPES) * len(O.LAYOUTS) * 2
    outside = sum(c["outside"] for c, path, _ in all_cases() if path == "fb")
    assert outside >= 100


MUTANTS = [  # (what is wrong, the defect of tests/_obj_metrics_ref.k22)
    ("the mask is ignored for the sums", "mask_ignored"),
    ("presence is counted from masked pixels only", "present_masked"),
    ("label == l + 1", "label_plus1"),
    ("the last label is dropped", "last_dropped"),
    ("labels outside [0, L) are clamped into L - 1", "clamped"),
    ("a wave's lanes are reduced without regard to their labels", "wave_merge"),
    ("fb of image 0 for every image", "fb0"),
    ("a workgroup's pixels past an image boundary go to the previous image", "image_boundary"),
    ("the last n % 256 pixels of an image are skipped", "tail"),
    ("only the first grid pass is taken", "one_pass"),
    ("dd >= 1 for dd > 1", "ge0"),
    ("dd >= 2 for dd > 2", "ge1"),
    ("dz >= 2e-3 for dz > 2e-3", "ge2"),
    ("dz >= 4e-3 for dz > 4e-3", "ge3"),
    ("dz >= 8e-3 for dz > 8e-3", "ge4"),
]


@pytest.mark.parametrize("what,defect", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_rejected_by_the_rules(what, defect, capsys):
    tried = 0
    for c, path, zp in all_cases():
        tried += 1
        try:
            O.check_k22(O.k22_exact(c, zp, defect), c, zp, what=path)
        except AssertionError as err:
            with capsys.disabled():
                print(f"\n  mutant '{what}' rejected by case {tried}: {c['name']} {path}\n    {err}", end="")
            return
    pytest.fail(f"mutant '{what}' survived all {tried} cases: a case is missing")


# ---- K23 -----------------------------------------------------------------------------------------------------------
def _torch_chain(disp, depth, max_disp, exclude_bg, robot, rs, depth_hi=1.25):
    """test.py:112-117, 162-193 with torch's own operators"""
    H, W = disp.shape[-2:]
    mask = (disp < max_disp) * (disp > 0)
    if exclude_bg:
        mask = mask * ((depth > 0) & (depth < depth_hi))
    if robot is not None:
        r = F.interpolate(robot.unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False).type(torch.int)
        mask = mask * (r == 0)
    if rs is not None:
        s = F.interpolate(rs.unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False)
        mask = mask * (s > 0)
    return mask.type(torch.bool)


AUX = [((12, 20), (12, 20)), ((12, 20), (24, 40)), ((12, 21), (16, 28)), ((12, 20), (5, 7)), ((33, 65), (540, 960)), ((5, 7), (3, 10))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("hw,aux", AUX, ids=[f"{a[0]}x{a[1]}->{h[0]}x{h[1]}" for h, a in AUX])
def test_eval_mask_restatement_agrees_with_interpolate_and_the_cast_chain(hw, aux, dtype):
    disp, depth, robot, rs = O.eval_mask_case(2, *hw, aux, dtype, 8500 + hw[0] + aux[1])
    T = torch.from_numpy
    seen = set()
    for bg in (False, True):
        for use_robot in (False, True):
            for use_rs in (False, True):
                got, count = O.eval_mask(disp, depth, 192, bg, robot if use_robot else None, rs if use_rs else None)
                want = _torch_chain(T(disp), T(depth), 192, bg, T(robot) if use_robot else None, T(rs) if use_rs else None)
                assert got.dtype == bool and np.array_equal(got, want.numpy()) and count == int(want.sum())
                seen.add(count)
    assert len(seen) >= 6 and min(seen) > 0  # every term removes pixels, none removes all


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_eval_mask_known_answers_at_the_exclusive_bounds(dtype):
    t = np.dtype(dtype).type
    below1 = np.nextafter(t(1), t(0))
    disp = np.array([100, 192, R.down(192), 0, R.up(0), 100, 100, 100], dtype=F32).reshape(1, 1, 1, 8)
    ok = np.full((1, 1, 1, 8), 0.5, dtype=F32)
    assert O.eval_mask(disp, ok, 192)[0].ravel().tolist() == [True, False, True, False, True, True, True, True]
    depth = np.array([1.25, R.down(1.25), 0, -0.0, R.up(0), 1, 2, NAN], dtype=F32).reshape(1, 1, 1, 8)
    d100 = np.full((1, 1, 1, 8), 100, dtype=F32)
    assert O.eval_mask(d100, depth, 192)[0].ravel().tolist() == [False, True, False, False, True, True, False, False]
    assert O.eval_mask(d100, depth, 192, exclude_bg=False)[1] == 8
    robot = np.array([below1, 1, -0.5, -below1, -1, 0, -0.0, 2.5], dtype=dtype).reshape(1, 1, 8)
    assert below1 < 1 and (dtype is np.float32 or F32(below1) == 1)  # the float64 0.999... a float32 round trip would turn into 1
    assert O.eval_mask(d100, ok, 192, robot=robot)[0].ravel().tolist() == [True, False, True, True, False, True, True, False]
    rs = np.array([0, -0.0, np.finfo(dtype).tiny, -1, 1, NAN, np.inf, 0.25], dtype=dtype).reshape(1, 1, 8)
    assert O.eval_mask(d100, ok, 192, realsense=rs)[0].ravel().tolist() == [False, False, True, False, True, False, True, True]
    T = torch.from_numpy
    for kw in (dict(robot=robot), dict(realsense=rs), dict(robot=robot, realsense=rs)):
        want = _torch_chain(T(disp), T(depth), 192, True, T(kw["robot"]) if "robot" in kw else None,
                            T(kw["realsense"]) if "realsense" in kw else None)
        assert np.array_equal(O.eval_mask(disp, depth, 192, **kw)[0], want.numpy())


def test_nearest_source_index_at_integer_and_other_ratios():
    assert O.nearest_src(6, 6).tolist() == [0, 1, 2, 3, 4, 5] and O.nearest_src(3, 6).tolist() == [0, 2, 4]
    assert O.nearest_src(6, 3).tolist() == [0, 0, 1, 1, 2, 2]                 # an upscale
    assert O.nearest_src(21, 28).tolist() == [int(math.floor(i * 4 / 3)) for i in range(21)]  # 4:3
    assert O.nearest_src(7, 10).tolist() == [0, 1, 2, 4, 5, 7, 8]
