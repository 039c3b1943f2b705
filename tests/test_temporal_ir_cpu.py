"""CPU side of the temporal IR pattern (K17, az_temporal_ir.hip) and of az_ir_pattern_mode: the fp64 restatement
tests/_temporal_ir_ref.py checked against closed forms, the exported C entry points, and their host-side argument
validation.  No kernel is launched."""
import ctypes

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _temporal_ir_ref as ref

NEW = ("az_temporal_ir_workspace", "az_temporal_ir", "az_ir_pattern_mode")
EINVAL, EUNSUP, EWORK = -1, -4, -5


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("t", [2, 7, 16])
def test_restatement_of_an_exact_ramp_is_its_slope(t):
    rng = np.random.default_rng(t)
    slope, offset = rng.uniform(-9, 9, (5, 6)), rng.uniform(20, 120, (5, 6))
    stack = offset[None] + slope[None] * np.arange(t)[:, None, None]
    want = np.abs(slope) * (t - 1) / 255
    assert np.abs(ref.fit_diff(stack) - want).max() <= 1e-12


def test_restatement_blur_equals_the_double_loop():
    img = np.random.default_rng(5).random((7, 9))
    assert np.abs(ref.box_blur(img, 5) - ref.box_blur_bruteforce(img, 5)).max() <= 1e-14
    # reflect-101: the edge pixel is not repeated
    assert [ref.reflect101(i, 7) for i in (-2, -1, 0, 6, 7, 8)] == [2, 1, 0, 6, 5, 4]


def test_restatement_of_a_constant_stack_is_all_zero():
    pattern, _ = ref.temporal_ir_pattern(np.full((7, 12, 14), 80.0), ks=5)
    assert pattern.shape == (12, 14) and not pattern.any()
    # so is a stack whose every pixel brightens alike: the difference image is constant
    pattern, _ = ref.temporal_ir_pattern(np.arange(7.0)[:, None, None] * np.ones((7, 12, 14)), ks=5)
    assert not pattern.any()


def test_generator_keeps_the_decision_away_from_the_threshold():
    """the condition of the GPU comparison: at most 0.1 % of an image within 1e-5 of the threshold, 2-15 % ones at T = 7"""
    for (h, w), ks in (((24, 29), 9), ((37, 53), 11), ((67, 93), 11)):
        pattern, margin = ref.temporal_ir_pattern(ref.exposure_stack(0, 7, h, w), ks)
        assert (np.abs(margin) < 1e-5).mean() <= 1e-3
        assert 0.02 < pattern.mean() < 0.15


def test_new_symbols_are_exported_and_typed(handle):
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} missing from include/azhip.h"
        assert name in _lib._SIGS
        assert getattr(handle, name).argtypes == _lib._SIGS[name]
    assert handle.az_temporal_ir_workspace.restype is ctypes.c_longlong
    assert handle.az_temporal_ir_workspace(8, 7, 540, 960, 11) >= (8 * 540 * 960 + 2 * 8) * 4
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # additive change


def test_argument_validation_happens_before_any_launch(handle):
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    big = 1 << 30
    # az_temporal_ir(pattern, workspace, workspace_bytes, stack, stack_is_u8, B, T, H, W, ks, threshold, stream)
    tir, need = handle.az_temporal_ir, handle.az_temporal_ir_workspace
    assert tir(None, p, big, p, 0, 1, 7, 24, 29, 9, 0.005, None) == EINVAL
    assert tir(p, None, big, p, 0, 1, 7, 24, 29, 9, 0.005, None) == EINVAL
    assert tir(p, p, big, None, 1, 1, 7, 24, 29, 9, 0.005, None) == EINVAL
    for t in (1, 0, 17):
        assert tir(p, p, big, p, 0, 1, t, 24, 29, 9, 0.005, None) == EUNSUP
        assert need(1, t, 24, 29, 9) == EUNSUP
    for ks in (10, 1, 33, -3):
        assert tir(p, p, big, p, 1, 1, 7, 24, 29, ks, 0.005, None) == EUNSUP
        assert need(1, 7, 24, 29, ks) == EUNSUP
    assert tir(p, p, big, p, 0, 1, 7, 4, 29, 9, 0.005, None) == EINVAL  # H <= ks / 2
    assert tir(p, p, big, p, 0, 1, 7, 24, 4, 9, 0.005, None) == EINVAL  # W <= ks / 2
    assert need(1, 7, 15, 200, 31) == EINVAL and need(1, 7, 16, 200, 31) > 0
    assert tir(p, p, big, p, 0, 0, 7, 24, 29, 9, 0.005, None) == EINVAL
    assert tir(p, p, need(1, 7, 24, 29, 9) - 1, p, 0, 1, 7, 24, 29, 9, 0.005, None) == EWORK
    # az_ir_pattern_mode(pattern, workspace, workspace_bytes, img_ir, img, B, H, W, ks, threshold, mode, stream)
    irm = handle.az_ir_pattern_mode
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert irm(ptrs[0], ptrs[1], big, ptrs[2], ptrs[3], 1, 37, 53, 11, 0.005, 1, None) == EINVAL
    assert irm(p, p, big, p, p, 1, 37, 53, 11, 0.005, 2, None) == EINVAL  # no such mode
    assert irm(p, p, big, p, p, 1, 37, 53, 11, 0.005, -1, None) == EINVAL
    assert irm(p, p, big, p, p, 1, 7, 53, 11, 0.005, 1, None) == EINVAL  # image smaller than the window
    assert irm(p, p, 16, p, p, 1, 37, 53, 11, 0.005, 1, None) == EWORK
    assert irm(p, p, 16, p, p, 1, 37, 53, 11, 0.005, 0, None) == EWORK


def test_python_surface_refuses_cpu_tensors_and_wrong_dtypes():
    from activezero_amd.datasets import dataset_utils_gpu as du

    with pytest.raises(RuntimeError, match="GPU"):
        du.get_temporal_ir_pattern(torch.zeros(7, 24, 29))
    with pytest.raises(RuntimeError, match="GPU"):
        du.get_temporal_ir_pattern(torch.zeros(2, 7, 24, 29, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="float32 or torch.uint8"):
        du.get_temporal_ir_pattern(torch.zeros(7, 24, 29, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        du.get_temporal_ir_pattern(torch.zeros(24, 29))
    a = torch.zeros(37, 53)
    with pytest.raises(RuntimeError, match="GPU"):
        du.get_ir_pattern(a, a)
    with pytest.raises(RuntimeError, match="GPU"):
        du.get_smoothed_ir_pattern(a, a)
