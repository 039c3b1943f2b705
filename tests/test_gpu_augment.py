"""GPU: the loader's blur, colour jitter and normalisation (K20, az_augment.hip) through augment_images, data_augmentation
and SyntheticMessytableDataset(augment=True), against the fp64 restatement tests/_augment_ref.py.

Rule: every element of every output lies within the helper's derived per-element bound of the restatement (ratio <= 1; the
bound counts the kernel's roundings and is not fitted to anything, see the helper's docstring); each case prints its worst
ratio before it asserts.  Where the issue demands equal bits -- both stages off against torch's fp32 (x - mean) / std, uint8
against the float32 image u8 / 255, a batch against its images one by one, [H,W] against [1,H,W], one run against the next --
the comparison is torch.equal.  Input generator: the helper's make_image (8 x 8 blocks, dots, noise; uint8)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, ops  # noqa: E402
from activezero_amd.datasets.dataset_utils_gpu import augment_images, data_augmentation  # noqa: E402
from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset  # noqa: E402
from tests import _augment_ref as ref  # noqa: E402

DEV = "cuda:0"
ROWS = ((0.1, 1.4, 1.2), (2.0, 1.4, 0.8), (1.0, 0.4, 1.2))  # (sigma, brightness, contrast)


def f32_image(u8):
    """the float32 image u8 / 255, every element correctly rounded (numpy divides; nothing multiplies by a reciprocal)"""
    return u8.astype(np.float32) / np.float32(255)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def col(values):
    return torch.tensor(values, dtype=torch.float32, device=DEV)


def held(got, imgs, params, ks, what):
    """got [B,3,H,W] against the restatement of every image with its own (sigma, b, c, contrast_first); any of sigma / b
    None = stage off"""
    worst = 0.0
    for i, (img, (sigma, b, c, first)) in enumerate(zip(imgs, params)):
        r, e = ref.ratio(got[i].cpu().numpy(), img, sigma, b, c, bool(first), ks)
        print(f"{what} image {i} (sigma {sigma}, b {b}, c {c}, contrast first {first}): worst ratio {r:.3f}, "
              f"largest error {e:.3g}")
        worst = max(worst, r)
    assert worst <= 1.0, f"{what}: worst error / bound = {worst:.4g}"


@pytest.mark.parametrize("case", range(len(ref.CASES)))
def test_augmented_images_vs_restatement(case):
    hw, ks, seeds = ref.CASES[case]
    imgs = [ref.make_image(seed, *hw) for seed in seeds]
    batch = dev(np.stack(imgs))
    n = len(imgs)
    for shift in (0, 1):  # the rows walk across the shapes and the images of a batch; every row meets both orders
        rows = [ROWS[(case + shift + i) % 3] for i in range(n)]
        for flip in (0, 1):
            first = [(i + flip) % 2 for i in range(n)]  # mixed orders within a batch
            got = augment_images(batch, col([r[0] for r in rows]), col([r[1] for r in rows]), col([r[2] for r in rows]),
                                 col(first), ks)
            assert got.shape == (n, 3) + hw and got.dtype == torch.float32
            held(got, imgs, [r + (f,) for r, f in zip(rows, first)], ks, f"{hw} ks {ks}")


@pytest.mark.parametrize("hw", [(37, 53), (40, 64)])
def test_flag_combinations_and_the_bits_of_the_plain_normalisation(hw):
    u8 = ref.make_image(3, *hw)
    x8, x32 = dev(u8), dev(f32_image(u8))
    sigma, b, c = ROWS[1]
    for blur in (False, True):
        for jitter in (False, True):
            for first in ((False, True) if jitter else (False,)):
                got = augment_images(x8, sigma if blur else None, b if jitter else None, c if jitter else None,
                                     first if jitter else None)
                assert got.shape == (3,) + hw
                held(got[None], [u8], [(sigma if blur else None, b if jitter else None, c if jitter else None, first)], 9,
                     f"{hw} blur {blur} jitter {jitter}")
    # both stages off: torch's own fp32 (x - mean) / std, bit for bit
    mean, std = col(ref.MEAN).view(3, 1, 1), col(ref.STD).view(3, 1, 1)
    want = ((x32[None].expand(3, -1, -1) - mean) / std).contiguous()
    plain = augment_images(x32)  # params = NULL
    assert torch.equal(plain, want)
    assert torch.equal(augment_images(x8), want)
    # the same through the C entry point with a parameter block it must ignore
    h, w = hw
    ws_bytes = _lib.lib().az_augment_workspace(1, h, w, 9)
    ws, out = torch.empty(ws_bytes // 4, device=DEV), torch.empty(1, 3, h, w, device=DEV)
    junk = col([[float("nan"), -3.0, float("inf"), 1.0]])
    ops._call("az_augment", out.data_ptr(), ws.data_ptr(), ws_bytes, x32.data_ptr(), 0, junk.data_ptr(), 1, h, w, 9, 0,
              ops._stream())
    assert torch.equal(out[0], want)


@pytest.mark.parametrize("hw", [(37, 53), (40, 64)])  # scalar and vector loads
def test_uint8_and_float32_images_give_the_same_bits(hw):
    u8 = np.stack([ref.make_image(seed, *hw) for seed in (4, 5)])
    x8, x32 = dev(u8), dev(f32_image(u8))
    for sigma, bc in ((None, (None, None)), (1.0, (None, None)), (None, (1.4, 1.2)), (1.0, (1.4, 1.2))):
        a = augment_images(x8, sigma, *bc, None if bc[0] is None else col([0, 1]))
        b = augment_images(x32, sigma, *bc, None if bc[0] is None else col([0, 1]))
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_batch_equals_images_one_by_one_and_runs_repeat():
    imgs = dev(np.stack([ref.make_image(seed, 67, 93) for seed in range(3)]))
    sigma, b, c, first = col([0.1, 2.0, 1.0]), col([1.4, 1.4, 0.4]), col([1.2, 0.8, 1.2]), col([0, 1, 1])
    whole = augment_images(imgs, sigma, b, c, first)
    assert whole.shape == (3, 3, 67, 93)
    assert torch.equal(whole, augment_images(imgs, sigma, b, c, first))  # two runs of the same call
    for i in range(3):
        one = augment_images(imgs[i], sigma[i:i + 1], b[i:i + 1], c[i:i + 1], first[i:i + 1])
        assert one.shape == (3, 67, 93)
        assert torch.equal(whole[i], one)  # the mean does not depend on B
        assert torch.equal(augment_images(imgs[i:i + 1], float(sigma[i]), float(b[i]), float(c[i]), bool(first[i]))[0], one)


def test_documented_meaning_of_parameters_torchvision_would_refuse():
    u8 = ref.make_image(6, 37, 53)
    x = dev(u8)
    # sigma <= 0: the unblurred image
    assert torch.equal(augment_images(x, 0.0), augment_images(x))
    assert torch.equal(augment_images(x, -1.0, 1.4, 1.2, True), augment_images(x, None, 1.4, 1.2, True))
    # a negative factor is clamped like any other value: brightness -1 first -> all zero -> contrast of a zero image
    held(augment_images(x, None, -1.0, 1.2, False)[None], [u8], [(None, -1.0, 1.2, False)], 9, "negative brightness")
    # NaN propagates, and stays in its own image
    both = augment_images(torch.stack([x, x]), col([float("nan"), 1.0]), col([1.4, 1.4]), col([1.2, 1.2]), col([0, 0]))
    assert bool(torch.isnan(both[0]).all()) and torch.equal(both[1], augment_images(x, 1.0, 1.4, 1.2, False))


def test_bad_arguments_raise_and_launch_nothing():
    x = dev(ref.make_image(0, 24, 29))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="AZ_EUNSUPPORTED"):
        augment_images(x, 1.0, kernel_size=10)
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):
        augment_images(x[:4], 1.0)  # H <= ks / 2
    with pytest.raises(RuntimeError, match="together"):
        augment_images(x, 1.0, brightness=1.2)
    with pytest.raises(RuntimeError, match="float32 or torch.uint8"):
        augment_images(x.double())
    with pytest.raises(RuntimeError, match="expected 1 values"):
        augment_images(x, col([1.0, 2.0]))
    torch.cuda.synchronize()


def test_data_augmentation_draws_once_and_applies_per_view():
    items, views, h, w = 8, 2, 37, 53
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)  # noqa: E731
    x = dev(np.stack([ref.make_image(seed, h, w) for seed in range(items * views)]).reshape(items, views, h, w))
    aug = data_augmentation(True, True, generator=gen(), items=items)
    for p, (lo, hi) in ((aug.sigma, (0.1, 2.0)), (aug.brightness, (0.4, 1.4)), (aug.contrast, (0.8, 1.2))):
        assert p.shape == (items,) and p.device.type == "cuda"
        assert bool((p >= lo).all()) and bool((p <= hi).all()) and float(p.max() - p.min()) > 0.1 * (hi - lo)
    out = aug(x)
    order = aug.last_order
    assert out.shape == (items, views, 3, h, w) and order.shape == (items * views,)
    assert set(order.tolist()) == {0.0, 1.0}  # every image draws its own order
    rep = lambda p: p.repeat_interleave(views)  # noqa: E731  (the views of an item share sigma, b and c)
    want = augment_images(x.view(-1, h, w), rep(aug.sigma), rep(aug.brightness), rep(aug.contrast), order)
    assert torch.equal(out.view(-1, 3, h, w), want)
    again = aug(x)  # the order is drawn anew at each application
    assert not torch.equal(aug.last_order, order) and not torch.equal(again, out)
    # the same seed gives the same bits
    aug2 = data_augmentation(True, True, generator=gen(), items=items)
    assert torch.equal(aug2.sigma, aug.sigma) and torch.equal(aug2(x), out)
    # [B,H,W] input; one drawn set serves any number of images; the switches
    one = data_augmentation(True, True, generator=gen())
    flat = one(x[:, 0])
    assert flat.shape == (items, 3, h, w)
    assert torch.equal(flat, augment_images(x[:, 0], one.sigma.expand(items), one.brightness.expand(items),
                                            one.contrast.expand(items), one.last_order))
    off = data_augmentation(generator=gen())
    assert off.sigma is None and off.brightness is None and torch.equal(off(x[:, 0]), augment_images(x[:, 0]))
    blur_only = data_augmentation(True, False, generator=gen(), kernel_size=5, sigma=(0.5, 0.5))
    assert torch.equal(blur_only(x[:, 0]), augment_images(x[:, 0], 0.5, kernel_size=5))


def test_loader_default_is_unchanged_and_augmented_items_follow_the_restatement():
    h, w = 64, 128
    plain = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV)
    off = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV, augment=False)
    on = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV, augment=True)
    a, b, c = plain[1], off[1], on[1]
    tensors = [k for k in a if k != "prefix"]
    assert a.keys() == b.keys() == c.keys()
    assert all(torch.equal(a[k], b[k]) for k in tensors)
    left, right = plain._views(plain._gen(1, 1))[:2]
    assert torch.equal(a["img_sim_L"], plain._normalise(left)) and torch.equal(a["img_sim_R"], plain._normalise(right))
    # the library's plain normalisation is the loader's, bit for bit
    assert torch.equal(augment_images(left), a["img_sim_L"])
    # augment=True changes the two simulated images and nothing else: the real images keep the normalisation only
    sim = ("img_sim_L", "img_sim_R")
    assert all(torch.equal(a[k], c[k]) for k in tensors if k not in sim)
    assert all(not torch.equal(a[k], c[k]) for k in sim)
    again = on[1]
    assert all(torch.equal(again[k], c[k]) for k in tensors)  # reproducible per index
    assert not torch.equal(on[0]["img_sim_L"], c["img_sim_L"])
    p = on.augmentation_params(1)
    assert p["sigma"].shape == (1,) and p["contrast_first"].shape == (2,)
    sigma, bright, contrast = (float(p[k]) for k in ("sigma", "brightness", "contrast"))
    assert 0.1 <= sigma <= 2.0 and 0.4 <= bright <= 1.4 and 0.8 <= contrast <= 1.2
    for view, (key, grey) in enumerate(zip(sim, (left, right))):
        assert c[key].shape == (3, h, w) and c[key].dtype == torch.float32 and c[key].is_contiguous()
        held(c[key][None], [grey.cpu().numpy()], [(sigma, bright, contrast, float(p["contrast_first"][view]))], 9, key)
