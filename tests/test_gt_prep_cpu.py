"""CPU side of the ground-truth preparation (K18, az_gt_prep.hip) and the error images (K19, az_error_img.hip): the
restatements of tests/_gt_prep_ref.py against hand-written known answers, the exported C entry points, their host-side
argument validation, and the signatures of the drop-in image functions.  No kernel is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _gt_prep_ref as ref

NEW = ("az_gt_from_right", "az_error_img")
EINVAL, EUNSUP = -1, -4
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


# ---- K18 restatement ------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    far = 8.0  # = W: lands nowhere, is not counted
    rows = [[2.5, 1.25, far, far, far, far, far, far],     # 0 and 1 both reach column 2: the smaller j wins; holes elsewhere
            [-0.5, -1.0, NAN, INF, far, 1.25, 2.0, -INF],  # -0.5 lands in place; -1, NaN, +-inf are counted; 6 + 2 = W is off
            [far, 1.999, far, 2.0, far, far, far, far]]    # 1.999 shifts by 1, 2.0 by 2
    d = torch.tensor(rows).view(1, 1, 3, 8)
    extra = torch.arange(48.0).view(1, 2, 3, 8) + 100  # two channels, told apart by value
    keep = -torch.arange(24.0).view(1, 1, 3, 8)
    disp_l, extra_l, keep_s, mask, stats = ref.gt_from_right(d, extra, keep, size=(3, 8), lo=1.25, hi=2.5)
    want = torch.zeros(3, 8)
    want[0, 2], want[1, 0], want[1, 6], want[2, 2], want[2, 5] = 2.5, -0.5, 1.25, 1.999, 2.0
    assert torch.equal(disp_l[0, 0], want)
    src_col = {(0, 2): 0, (1, 0): 0, (1, 6): 5, (2, 2): 1, (2, 5): 3}
    for c in range(2):
        want_e = torch.zeros(3, 8)
        for (y, t), j in src_col.items():
            want_e[y, t] = extra[0, c, y, j]
        assert torch.equal(extra_l[0, c], want_e)
    assert torch.equal(keep_s, keep)  # ratio 1: resized only, not warped
    # the bounds are exclusive: 2.5 (= hi) and 1.25 (= lo) are out, 1.999 and 2.0 are in
    want_m = torch.zeros(3, 8, dtype=torch.bool)
    want_m[2, 2] = want_m[2, 5] = True
    assert mask.dtype == torch.bool and torch.equal(mask[0, 0], want_m)
    assert stats.tolist() == [4, 2]


@pytest.mark.parametrize("hw", [(8, 12), (9, 13), (7, 5), (2, 2), (3, 3)])
def test_restatement_halving_reads_every_second_pixel(hw):
    """the factor 0.5 is source 2 * dst at every even or odd input size"""
    x = torch.arange(float(hw[0] * hw[1])).view(1, 1, *hw)
    h, w = hw[0] // 2, hw[1] // 2
    assert torch.equal(ref.resize_nearest(x, scale_factor=0.5), x[:, :, ::2, ::2][:, :, :h, :w])
    # ... and so is the formula the kernel evaluates, min((int)floorf(dst * scale), in - 1), scale = float(1 / 0.5)
    for n_in, n_out in ((hw[0], h), (hw[1], w)):
        idx = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * np.float32(2.0)).astype(np.int64), n_in - 1)
        assert idx.tolist() == [2 * i for i in range(n_out)]


def test_restatement_other_ratios_follow_the_formula():
    x = torch.arange(81.0).view(1, 1, 9, 9)
    idx = np.minimum(np.floor(np.arange(6, dtype=np.float32) * (np.float32(9) / np.float32(6))).astype(np.int64), 8)
    assert idx.tolist() == [0, 1, 3, 4, 6, 7]
    assert torch.equal(ref.resize_nearest(x, size=(6, 6)), x[:, :, idx][:, :, :, idx])
    assert torch.equal(ref.resize_nearest(x, size=(9, 9)), x)


# ---- K19 restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disp", "depth"])
def test_a_value_on_an_inner_bound_falls_in_the_upper_class(kind):
    b = ref.bounds(kind)
    assert b.dtype == np.float32 and b[0] == 0 and np.isinf(b[11]) and (np.diff(b) > 0).all()
    assert ref.classes(b[1:11], kind).tolist() == list(range(1, 11))
    assert ref.classes(np.nextafter(b[1:11], np.float32(0)), kind).tolist() == list(range(0, 10))
    assert ref.classes(np.array([0.0, -0.0, np.inf, np.nan, -1e-9], np.float32), kind).tolist() == [0, 0, -1, -1, -1]
    # the generator's on-the-bound pixels really are on the bounds, as float32
    est, gt = ref.on_the_bound(kind)
    assert np.array_equal(ref.scaled_error(est, gt, kind, 3.0 if kind == "disp" else 1.0), b[1:11])


@pytest.mark.parametrize("kind", ["disp", "depth"])
def test_generator_fills_every_class_and_the_hostile_pixels_come_out_as_stated(kind):
    h, w = 12, 150
    est, gt, mask = ref.error_case(0, 1, h, w, kind)
    cls = ref.classes(ref.scaled_error(est, gt, kind, 3.0 if kind == "disp" else 1.0), kind)
    counts = np.bincount(cls[mask & (cls >= 0)], minlength=11)
    assert (counts >= 50).all(), counts
    assert 0.15 < 1 - mask.mean() < 0.25
    img = ref.error_img(est, gt, mask, kind).reshape(h * w, 3)
    col = ref.colours()
    on_bound, hostile = ref.special_pixels(h, w)
    assert min(on_bound + hostile) >= 10 * w  # below the legend
    for k, p in enumerate(on_bound):
        assert np.array_equal(img[p], col[k + 1])
    # gt = 0 with an error: the relative quotient is +inf, the absolute one 2 / 3 (disp) or 2 (depth) decides: coloured
    assert np.array_equal(img[hostile[0]], col[5 if kind == "disp" else 2])
    # gt = 0 = est: 0 / 0 is NaN for disp (black); depth has no quotient by gt: class 0, black as well
    # est = gt: class 0; NaN / inf predictions, a NaN ground truth: no class
    for p in hostile[1:6]:
        assert not img[p].any()
    # a negative ground truth: the disparity quotient is negative, no class; the depth error is |gt - est| = 2
    assert np.array_equal(img[hostile[6]], np.zeros(3) if kind == "disp" else col[2])
    assert not img.reshape(h, w, 3)[10:][~mask[0, 10:]].any()  # mask off: black


def test_restatement_legend_and_clipping():
    col = ref.colours()
    assert col.dtype == np.float32 and col[1, 0] == np.float32(49) / np.float32(255)
    for h, w in ((12, 230), (12, 150), (7, 33), (1, 1)):
        z = np.zeros((2, h, w), np.float32)
        img = ref.error_img(z, z + 1, np.zeros((2, h, w), bool), "disp")  # mask off everywhere: the legend alone
        assert img.shape == (2, h, w, 3) and img.dtype == np.float32
        for y in range(h):
            for x in range(w):
                want = col[x // 20] if (y < 10 and x < 220) else np.zeros(3, np.float32)
                assert np.array_equal(img[0, y, x], want) and np.array_equal(img[1, y, x], want)


# ---- the C surface --------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_typed(handle):
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} missing from include/azhip.h"
        assert getattr(handle, name).argtypes == _lib._SIGS[name]
        assert getattr(handle, name).restype is ctypes.c_int
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib._SIGS["az_gt_from_right"] == [P] * 8 + [I] * 7 + [Fl] * 4 + [P]
    assert _lib._SIGS["az_error_img"] == [P] * 4 + [I, Fl, Fl] + [I] * 4 + [P]
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # entry points were only added


def test_gt_from_right_rejects_before_any_launch(handle):
    """every call below must be refused on the host: there is no device here"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = handle.az_gt_from_right

    def call(disp_l=p, extra_l=None, keep_s=None, mask=p, stats=p, disp_r=p, extra=None, keep=None, n=1, ce=0, ck=0,
             hin=8, win=12, h=4, w=6, sh=2.0, sw=2.0):
        return f(disp_l, extra_l, keep_s, mask, stats, disp_r, extra, keep, n, ce, ck, hin, win, h, w, sh, sw, 0.0, 192.0, None)

    for hole in ("disp_l", "stats", "disp_r"):  # required pointers (mask may be NULL)
        assert call(**{hole: None}) == EINVAL
    # channel counts and their pointers must agree, both ways, inputs and outputs
    assert call(ce=1) == EINVAL and call(ce=1, extra=p) == EINVAL and call(ce=1, extra_l=p) == EINVAL
    assert call(extra=p, extra_l=p) == EINVAL and call(extra=p) == EINVAL and call(extra_l=p) == EINVAL
    assert call(ck=2) == EINVAL and call(ck=2, keep=p) == EINVAL and call(ck=2, keep_s=p) == EINVAL
    assert call(keep=p, keep_s=p) == EINVAL and call(keep=p) == EINVAL
    assert call(ce=-1) == EINVAL and call(ck=-1) == EINVAL
    for name in ("n", "hin", "win", "h", "w"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL
    assert call(sh=0.0) == EINVAL and call(sw=-2.0) == EINVAL and call(sh=NAN) == EINVAL and call(sw=INF) == EINVAL
    assert call(h=9) == EUNSUP and call(w=13) == EUNSUP  # no upsampling
    assert call(win=8194, w=4097) == EUNSUP and call(win=5000, w=5000, sw=1.0) == EUNSUP  # the LDS winner table ends at 4096


def test_error_img_rejects_before_any_launch(handle):
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = handle.az_error_img
    # az_error_img(out, est, gt, mask, kind, abs_thres, rel_thres, layout, B, H, W, stream)
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert f(*ptrs, 0, 3.0, 0.05, 0, 1, 12, 230, None) == EINVAL
    for kind in (-1, 2):
        assert f(p, p, p, p, kind, 3.0, 0.05, 0, 1, 12, 230, None) == EINVAL
    for layout in (-1, 2):
        assert f(p, p, p, p, 0, 3.0, 0.05, layout, 1, 12, 230, None) == EINVAL
    for dims in ((0, 12, 230), (1, 0, 230), (1, 12, 0), (-1, 12, 230)):
        assert f(p, p, p, p, 1, 1.0, 0.05, 1, *dims, None) == EINVAL


# ---- the Python surface -----------------------------------------------------------------------------------------
def test_drop_in_signatures_match_the_reference():
    """utils/util.py:185 and :214-216, by parameter name and default"""
    from activezero_amd.utils import error_images as ei

    def params(fn):
        return [(n, q.default) for n, q in inspect.signature(fn).parameters.items()]

    none = inspect.Parameter.empty
    assert params(ei.disp_error_img) == [("D_est_tensor", none), ("D_gt_tensor", none), ("mask", none), ("abs_thres", 3.0),
                                         ("rel_thres", 0.05), ("dilate_radius", 1)]
    assert params(ei.depth_error_img) == [("D_est_tensor", none), ("D_gt_tensor", none), ("mask", none), ("abs_thres", 1.0),
                                          ("dilate_radius", 1)]
    assert callable(ei.disp_error_img_tensor) and callable(ei.depth_error_img_tensor)


def test_python_surface_refuses_cpu_tensors_and_wrong_shapes():
    from activezero_amd import ops
    from activezero_amd.utils import gt_prep

    sig = inspect.signature(ops.gt_from_right)
    assert [(n, q.default) for n, q in sig.parameters.items() if q.kind is q.KEYWORD_ONLY] == [
        ("scale_factor", 0.5), ("size", None), ("lo", 0.0), ("hi", INF), ("check", False)]
    d = torch.zeros(1, 1, 8, 12)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gt_from_right(d)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.error_img(d, d, d > 0)
    with pytest.raises(RuntimeError, match="kind"):
        ops.error_img(d, d, d > 0, kind="flow")
    with pytest.raises(RuntimeError, match="2 tensors"):
        gt_prep.prepare_sim_gt((d,), 192, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        gt_prep.prepare_sim_gt({"img_disp_R": d, "img_depth_L": d}, 192, device="cpu")
