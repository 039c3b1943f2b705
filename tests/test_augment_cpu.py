"""CPU side of the loader's augmentation (K20, az_augment.hip): the fp64 restatement tests/_augment_ref.py checked against
closed forms, the conditions on its input generator, its fp32 emulation and a set of mutants held against the derived
bound, the exported C entry points with their host-side argument validation, and the refusals of the Python surface.
No kernel is launched."""
import ctypes

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _augment_ref as ref

NEW = ("az_augment_workspace", "az_augment")
EINVAL, EUNSUP, EWORK = -1, -4, -5
SIZES = tuple((hw, ks) for hw, ks, _ in ref.CASES)  # the shapes of the GPU cases
ROWS = ((0.1, 1.4, 1.2), (2.0, 1.4, 0.8), (1.0, 0.4, 1.2))


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


# ---- the restatement against closed forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.1, 0.7, 2.0])
def test_blur_leaves_a_constant_image_and_the_interior_of_a_ramp_unchanged(sigma):
    assert np.abs(ref.gaussian_blur(np.full((12, 14), 0.37), 9, sigma) - 0.37).max() <= 1e-15
    ramp = np.tile(np.arange(20.0) / 40.0, (13, 1))  # horizontal: symmetric taps average to the centre
    assert np.abs(ref.gaussian_blur(ramp, 9, sigma) - ramp)[:, 4:-4].max() <= 1e-15
    assert abs(ref.weights(9, sigma).sum() - 1.0) <= 1e-15 and abs(ref.weights(31, sigma).sum() - 1.0) <= 1e-15


def test_reflection_does_not_repeat_the_edge_and_a_small_sigma_is_the_identity():
    assert [ref.reflect(i, 7) for i in (-2, -1, 0, 6, 7, 8)] == [2, 1, 0, 6, 5, 4]
    img = np.arange(35.0).reshape(5, 7) / 35.0
    pad = np.pad(img, 4, mode="reflect")  # what gaussian_blur pads with, against the index rule
    for y in (-2, -1, 5, 6):
        for x in (-2, -1, 7, 8):
            assert pad[y + 4, x + 4] == img[ref.reflect(y, 5), ref.reflect(x, 7)]
    assert np.abs(ref.gaussian_blur(img, 9, 0.1) - img).max() <= 1e-15


def test_unit_factors_are_identities_and_the_orders_differ_on_an_image_that_clamps():
    img = ref.unit(ref.make_image(0, 24, 29))
    assert np.abs(ref.adjust_brightness(img, 1.0) - img).max() == 0.0
    assert np.abs(ref.adjust_contrast(img, 1.0) - img).max() <= 1e-16
    a, b = ref.augment(img, None, 1.4, 1.2, False), ref.augment(img, None, 1.4, 1.2, True)
    assert np.abs(a - b).max() > 1e-3
    mild = 0.3 + 0.3 * img  # without a clamp the two adjustments commute
    assert np.abs(ref.augment(mild, None, 1.1, 1.1, False) - ref.augment(mild, None, 1.1, 1.1, True)).max() <= 1e-14
    # the grey weights sum to 0.9999: the mean of a constant image is not the constant
    assert abs(ref.grey_mean(np.full((4, 4), 0.5)) - 0.49995) <= 1e-15


# ---- conditions on the generator (conditions, not tolerances) --------------------------------------------------------------
@pytest.mark.parametrize("contrast_first", [False, True])
def test_generator_exercises_both_clamps(contrast_first):
    for (h, w), ks, seeds in ref.CASES[1:]:  # every image of every GPU case from 24 x 29 up
        for seed in seeds:
            hi, lo = ref.clamp_shares(ref.make_image(seed, h, w), 0.1, 1.4, 1.2, contrast_first, ks)
            print(f"{h}x{w} seed {seed} contrast_first {contrast_first}: {hi:.3f} clamp at 1, {lo:.3f} at 0")
            assert hi >= 0.01 and lo >= 0.01


# ---- the emulation and the mutants against the bound -----------------------------------------------------------------------
def test_the_emulation_passes_the_bound():
    worst, errs = 0.0, []
    for (h, w), ks in SIZES:
        img = ref.make_image(0, h, w)
        for sigma, b, c in ROWS:
            for contrast_first in (False, True):
                for flags in range(4):
                    s = sigma if flags & 1 else None
                    bc = (b, c) if flags & 2 else (None, None)
                    for im in (img, ref.emu_unit(img)):  # uint8 and float32 input
                        r, e = ref.ratio(ref.emulate(im, s, *bc, contrast_first, ks), im, s, *bc, contrast_first, ks)
                        worst = max(worst, r)
                        if flags == 3:
                            errs.append(e)
    print(f"emulation: worst ratio {worst:.3f}; largest error per full case {min(errs):.2e} .. {max(errs):.2e}")
    assert worst <= 1.0
    assert worst <= ref.EMU_WORST_RATIO * 1.0001  # the record in the helper is what this prints


MUTANTS = [  # (mutant, sigma, b, c, contrast_first)
    ("seam_tap_dropped", 2.0, 1.4, 0.8, False), ("edge_repeated", 2.0, 1.4, 0.8, False),
    ("weights_not_normalised", 2.0, 1.4, 0.8, True), ("horizontal_only", 1.0, 0.4, 1.2, False),
    ("mean_before_brightness", 0.1, 1.4, 1.2, False), ("mean_of_other", 1.0, 0.4, 1.2, True),
    ("grey_weights_sum_to_one", 1.0, 1.0, 0.5, False), ("grey_weights_sum_to_one", 1.0, 1.0, 1.2, True),
    ("orders_swapped", 0.1, 1.4, 1.2, False), ("no_high_clamp", 0.1, 1.4, 1.2, True), ("no_low_clamp", 0.1, 1.4, 1.2, False),
    ("tile_dropped", 2.0, 1.4, 0.8, True), ("channels_permuted", 1.0, 0.4, 1.2, False),
]


@pytest.mark.parametrize("mutant,sigma,b,c,contrast_first", MUTANTS)
def test_every_mutant_fails_the_bound(mutant, sigma, b, c, contrast_first):
    img, other = ref.make_image(0, 67, 93), ref.make_image(1, 67, 93)
    good, _ = ref.ratio(ref.emulate(img, sigma, b, c, contrast_first), img, sigma, b, c, contrast_first)
    bad, _ = ref.ratio(ref.emulate(img, sigma, b, c, contrast_first, mutant=mutant, other=other), img, sigma, b, c,
                       contrast_first)
    print(f"{mutant}: ratio {bad:.3g} (unmutated {good:.3f})")
    assert good <= 1.0 < bad


# ---- symbols, return codes, the Python surface -----------------------------------------------------------------------------
def test_new_symbols_are_exported_and_typed(handle):
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} missing from include/azhip.h"
        assert name in _lib._SIGS
        assert getattr(handle, name).argtypes == _lib._SIGS[name]
    assert handle.az_augment_workspace.restype is ctypes.c_longlong
    need = [handle.az_augment_workspace(b, 540, 960, 9) for b in (1, 2, 3, 8, 64)]
    assert all(n > 0 for n in need) and need == sorted(need) and need[-1] > need[0]  # monotone in B
    assert need[3] >= 8 * 15 * 17 * 4  # one float per 64 x 32 tile and image
    assert _lib.expected_abi_version() == 6 and handle.az_abi_version() == 6  # additive change


def test_argument_validation_happens_before_any_launch(handle):
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    big = 1 << 30
    # az_augment(out, workspace, workspace_bytes, img, img_is_u8, params, B, H, W, ks, flags, stream)
    aug, need = handle.az_augment, handle.az_augment_workspace
    assert aug(None, p, big, p, 0, p, 1, 24, 29, 9, 3, None) == EINVAL
    assert aug(p, None, big, p, 0, p, 1, 24, 29, 9, 3, None) == EINVAL
    assert aug(p, p, big, None, 1, p, 1, 24, 29, 9, 3, None) == EINVAL
    for flags in (1, 2, 3):  # params may be NULL only when both flags are clear
        assert aug(p, p, big, p, 0, None, 1, 24, 29, 9, flags, None) == EINVAL
    for flags in (-1, 4):
        assert aug(p, p, big, p, 0, p, 1, 24, 29, 9, flags, None) == EINVAL
    for b in (0, -2):
        assert aug(p, p, big, p, 0, p, b, 24, 29, 9, 3, None) == EINVAL
        assert need(b, 24, 29, 9) == EINVAL
    for ks in (10, 1, 33, -3):
        assert aug(p, p, big, p, 1, p, 1, 24, 29, ks, 3, None) == EUNSUP
        assert aug(p, p, big, p, 1, None, 1, 24, 29, ks, 0, None) == EUNSUP
        assert need(1, 24, 29, ks) == EUNSUP
    assert aug(p, p, big, p, 0, p, 1, 4, 29, 9, 3, None) == EINVAL  # H <= ks / 2
    assert aug(p, p, big, p, 0, p, 1, 24, 4, 9, 3, None) == EINVAL  # W <= ks / 2
    assert need(1, 4, 7, 9) == EINVAL and need(1, 5, 4, 9) == EINVAL and need(1, 5, 7, 9) > 0
    assert need(1, 15, 200, 31) == EINVAL and need(1, 16, 200, 31) > 0
    for flags in (0, 1, 2, 3):
        assert aug(p, p, need(1, 24, 29, 9) - 1, p, 0, p, 1, 24, 29, 9, flags, None) == EWORK
    assert aug(p, p, 0, p, 1, None, 2, 67, 93, 9, 0, None) == EWORK


def test_python_surface_refuses_what_it_cannot_run():
    from activezero_amd.datasets import dataset_utils_gpu as du

    with pytest.raises(RuntimeError, match="GPU"):
        du.augment_images(torch.zeros(24, 29))
    with pytest.raises(RuntimeError, match="GPU"):
        du.augment_images(torch.zeros(2, 24, 29, dtype=torch.uint8), sigma=1.0, brightness=1.2, contrast=0.9)
    with pytest.raises(RuntimeError, match="float32 or torch.uint8"):
        du.augment_images(torch.zeros(24, 29, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="together"):
        du.augment_images(torch.zeros(24, 29), brightness=1.2)
    with pytest.raises(RuntimeError, match="together"):
        du.augment_images(torch.zeros(24, 29), sigma=1.0, contrast=1.2)
    with pytest.raises(RuntimeError, match=r"\[H,W\] or \[B,H,W\]"):
        du.augment_images(torch.zeros(29))
    with pytest.raises(RuntimeError, match=r"\[H,W\] or \[B,H,W\]"):
        du.augment_images(torch.zeros(1, 2, 24, 29))
    with pytest.raises(TypeError):
        du.augment_images(np.zeros((24, 29), np.float32))
    # the dataset takes the switch without touching a device
    from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset
    assert SyntheticMessytableDataset(length=1, device="cpu").augment is False
    assert SyntheticMessytableDataset(length=1, device="cpu", augment=True).augment is True
