"""CPU: the restatements of tests/_test_inputs_ref.py are what they claim to be -- K26's is ATen's bilinear resize and pad
(held against torch's own CPU operators), K25's gives the hand-computed labels -- and the two entry points of
csrc/az_test_inputs.hip refuse bad arguments with the codes include/azhip.h states, before any launch."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from activezero_amd import _lib, build
from tests import _test_inputs_ref as T

F32 = np.float32


# ---- the restatements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,pad", list(zip(T.SIZE_PAIRS, T.PADS)) + [(T.LARGE[:2], T.LARGE[2])],
                         ids=lambda v: "x".join(map(str, np.ravel(v))))
def test_k26_restatement_is_atens_bilinear_resize_and_pad(sizes, pad):
    (hin, win), (h, w) = sizes
    src = T.normalise(T.random_levels(7000 + hin, 1, hin, win))
    want = F.pad(F.interpolate(torch.from_numpy(src), (h, w), mode="bilinear", align_corners=False),
                 (0, pad[1], pad[0], 0, 0, 0, 0, 0), mode="constant", value=0).numpy()
    mine = T.resize_pad(src, (h, w), pad)
    assert mine.shape == want.shape == (1, 3, h + pad[0], w + pad[1])
    err = np.abs(mine - want.astype(np.float64)).max()
    print(f"\n  {hin}x{win} -> {h}x{w}: max |restatement - torch| = {err / (T.bound(src) / 6):.2f} M 2^-24", end="")
    assert err <= T.bound(src)
    if (hin, win) == (h, w):  # the identity returns its input unchanged, in torch as in the restatement
        assert np.array_equal(mine[:, :, pad[0]:, :w], src) and np.array_equal(want[:, :, pad[0]:, :w], src)
    pads = np.ones(mine.shape, dtype=bool)
    pads[:, :, pad[0]:, :w] = False
    assert not mine[pads].any() and not np.signbit(mine[pads]).any()


def test_k26_axis_is_float32_throughout():
    i0, i1, l0, l1 = T.axis(720, 540)
    # 540 rows from 720: scale 4/3 rounded to float32; row 1 reads from 4/3 * 1.5 - 0.5 = 1.5 (rounded: 1.5000001)
    assert (i0[0], i1[0], l1[0]) == (0, 1, F32(F32(720) / F32(540) * F32(0.5) - F32(0.5)))
    assert i0[1] == 1 and l1[1] == F32(F32(4) / F32(3) * F32(1.5) - F32(0.5)) - F32(1)
    assert i0[-1] == 718 and i1[-1] == 719 and np.array_equal(l0, F32(1) - l1)
    i0, i1, l0, l1 = T.axis(5, 5)
    assert i0.tolist() == [0, 1, 2, 3, 4] and i1.tolist() == [1, 2, 3, 4, 4] and not l1.any() and (l0 == 1).all()


def test_k26_normalise_gives_torchs_bits():
    levels = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    x = (torch.from_numpy(levels).float() / 255)[:, None].expand(1, 3, 16, 16)
    want = (x - torch.tensor(T.MEAN).view(1, 3, 1, 1)) / torch.tensor(T.STD).view(1, 3, 1, 1)
    assert np.array_equal(T.normalise(levels), want.numpy())


def test_k25_restatement_gives_the_hand_computed_labels():
    """focal_length 400, baseline 0.0625: their product is 25 exactly.  v = 0: no depth, no disparity; v = 1: one millimetre,
    25 / 0.001; v = 1000: one metre, 25 pixels; v = 65535: the largest 16-bit value"""
    mm = np.array([[[0, 1, 1000, 65535]]], dtype=np.uint16)
    disp_l, depth_l, disp_r, depth_r = T.depth_labels(mm, mm[:, :, ::-1], 400.0, 0.0625)
    assert all(a.dtype == F32 and a.shape == (1, 1, 1, 4) for a in (disp_l, depth_l, disp_r, depth_r))
    assert depth_l.ravel().tolist() == [0.0, F32(0.001), 1.0, F32(65.535)]
    assert depth_l.ravel()[1].view(np.uint32) == 0x3A83126F  # float32(0.001)
    assert disp_l.ravel()[:3].tolist() == [0.0, 25000.0, 25.0]
    big = float(disp_l.ravel()[3])
    assert abs(big * 65.535 - 25.0) <= 25.0 * 2.0 ** -23 and disp_l.ravel()[3] == F32(25.0 / (65535 / 1000))
    assert np.array_equal(disp_r, disp_l[..., ::-1]) and np.array_equal(depth_r, depth_l[..., ::-1])


def test_k25_restatement_int32_window_and_clamp():
    mm = np.array([[[-5, 0, 70000], [3, 2, 1]]], dtype=np.int32)
    disp, depth, _, _ = T.depth_labels(mm, mm, 400.0, 0.0625)
    assert depth[0, 0, 0].tolist() == [F32(-0.005), 0.0, 70.0] and disp[0, 0, 0].tolist() == [0.0, 0.0, F32(25.0 / 70.0)]
    win, _, _, _ = T.depth_labels(mm, mm, 400.0, 0.0625, origin=[[1, 1]], window=(1, 2))
    assert np.array_equal(win, disp[:, :, 1:, 1:])
    far, _, _, _ = T.depth_labels(mm, mm, 400.0, 0.0625, origin=[[9, -4]], window=(1, 2))  # clamped into the map
    assert np.array_equal(far, disp[:, :, 1:, :2])


# ---- the C ABI -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


def test_entry_points_are_declared_and_exported(handle):
    assert {"az_depth_labels", "az_test_images"} <= set(_lib.declared_symbols())
    assert hasattr(handle, "az_depth_labels") and hasattr(handle, "az_test_images")
    assert (_lib.CONST["AZ_DEPTH_U16"], _lib.CONST["AZ_DEPTH_I32"]) == (0, 1)
    assert _lib.CONST["AZ_ABI_VERSION"] == 6  # additions only: no signature changed


def test_az_depth_labels_refuses_bad_arguments_before_any_launch(handle):
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(outs=(p, p, p, p), mm=(p, p), dtype=0, fl=p, bl=p, origin=p, dims=(1, 8, 8, 4, 4))

    def call(**kw):
        a = {**ok, **kw}
        return handle.az_depth_labels(*a["outs"], *a["mm"], a["dtype"], a["fl"], a["bl"], a["origin"], *a["dims"], None)

    EINVAL, ENULL = _lib.CONST["AZ_EINVAL"], _lib.CONST["AZ_ENULL"]
    for k in range(4):
        assert call(outs=tuple(None if j == k else p for j in range(4)), dtype=7) == ENULL
    assert call(mm=(None, p), dtype=7) == ENULL and call(mm=(p, None), dtype=7) == ENULL
    assert call(fl=None, dtype=7) == ENULL and call(bl=None, dtype=7) == ENULL
    for dtype in (-1, 2, 16):
        assert call(dtype=dtype) == EINVAL
    for dims in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, -1, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0)):
        assert call(dims=dims) == EINVAL
    assert call(dims=(1, 8, 8, 9, 4)) == EINVAL and call(dims=(1, 8, 8, 4, 9)) == EINVAL  # a window larger than the map
    assert call(origin=None, dims=(1, 8, 8, 4, 8)) == EINVAL  # without an origin the window is the map
    assert call(origin=None, dims=(1, 8, 8, 8, 4)) == EINVAL


def test_az_test_images_refuses_bad_arguments_before_any_launch(handle):
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, ENULL = _lib.CONST["AZ_EINVAL"], _lib.CONST["AZ_ENULL"]
    good = (1, 0, 4, 4, 3, 3, 1, 1)  # N, N_second, Hin, Win, H, W, top_pad, right_pad

    def call(out=p, src=p, second=None, u8=0, dims=good):
        return handle.az_test_images(out, src, second, u8, *dims, None)

    assert call(out=None, u8=5) == ENULL and call(src=None, u8=5) == ENULL
    assert call(dims=(1, 1, 4, 4, 3, 3, 1, 1)) == ENULL  # a second source is announced but missing
    for u8 in (-1, 2):
        assert call(u8=u8) == EINVAL
    for k in (0, 2, 3, 4, 5):  # N, Hin, Win, H, W must be positive
        for v in (0, -3):
            assert call(dims=tuple(v if j == k else g for j, g in enumerate(good))) == EINVAL
    for k in (1, 6, 7):        # N_second and the pads may be zero, not negative
        assert call(dims=tuple(-1 if j == k else g for j, g in enumerate(good))) == EINVAL
    big = 2 ** 31 - 1
    assert call(dims=(1, 0, 4, 4, big, 3, 1, 0), u8=0) == _lib.CONST["AZ_EUNSUPPORTED"]  # H + top_pad leaves the int range


# ---- the host side ---------------------------------------------------------------------------------------------------
def test_ops_and_helpers_refuse_cpu_tensors_and_bad_shapes():
    from activezero_amd import ops
    from activezero_amd.datasets import dataset_utils_gpu as dg
    from activezero_amd.utils import gt_prep

    mm = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.depth_labels(mm, mm, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="uint16 or torch.int32"):
        ops.depth_labels(mm.float(), mm.float(), 1.0, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.test_images(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="float32 or torch.uint8"):
        ops.test_images(torch.zeros(1, 3, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="outside"):
        dg.depth_to_labels(mm, mm, 1.0, 1.0, crop=(2, 2, 4, 4))
    with pytest.raises(RuntimeError, match="smaller"):
        gt_prep.prepare_test_images(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), size=(4, 4), pad_to=(3, 4))
    defaults = {k: v.default for k, v in inspect.signature(gt_prep.prepare_test_images).parameters.items()}
    assert defaults["size"] == (540, 960) and defaults["pad_to"] == (544, 960)  # test.py:118-131, configs/config.py:80-81


def test_stereo_constants_are_the_loaders_two_lines():
    from activezero_amd.datasets.dataset_utils_gpu import stereo_constants

    ext_l, ext_r = np.eye(4), np.eye(4)
    ext_l[:3, 3], ext_r[:3, 3] = (0.1, 0.2, 0.3), (0.13, 0.24, 0.3)
    k = np.array([[892.62, 0, 960], [0, 892.62, 540], [0, 0, 1]])
    focal_length, baseline = stereo_constants(ext_l, ext_r, k)
    assert focal_length == 892.62 / 2 and isinstance(float(baseline), float)
    assert abs(baseline - math.sqrt((0.1 - 0.13) ** 2 + (0.2 - 0.24) ** 2)) < 1e-16  # (the homogeneous 1 cancels)


def test_rehearsal_summary_is_json():
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import test_rehearsal as tr

    out = tr._jsonable({"a": np.array([1.0, np.nan]), "b": [{"c": float("inf"), "prefix": "scene-1"}], "n": 3})
    assert out == {"a": [1.0, None], "b": [{"c": None, "prefix": "scene-1"}], "n": 3.0} and json.loads(json.dumps(out)) == out
    assert (tr.SIZE, tr.PAD_TO, tr.MAX_DISP, tr.OBJ_NUM) == ((540, 960), (544, 960), 192, 18)
