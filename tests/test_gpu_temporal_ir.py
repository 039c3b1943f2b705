"""GPU: the temporal IR pattern (K17, az_temporal_ir.hip), get_ir_pattern / get_smoothed_ir_pattern (az_ir_pattern_mode)
and the synthetic loader's temporal=True real patterns, against fp64 restatements.

Input generator of the temporal cases (tests/_temporal_ir_ref.py exposure_stack): rng = default_rng(100 + seed);
tex = integers(20, 120); dots = random < 0.06; frame k = clip(rint(tex + dots * k * (12 + 8 * random) + normal(0, 1.5)),
0, 255).

Rule: the pattern equals the restatement's at every pixel whose fp64 margin d - mean - threshold satisfies
|margin| >= 1e-5, and at most 0.1 % of an image may lie inside that band (a condition on the inputs, asserted, not a
tolerance: an fp32 evaluation of the same arithmetic moves the margin by a few 1e-7).  The share of ones must lie in
2-15 % so that an all-zero output cannot pass (the restatement gives 5.7-8.6 % on this generator at T = 7).  At T = 2 the
generator's dots rise by one step of 12-20 grey levels against noise of 1.5 * sqrt(2): the RESTATEMENT marks 26-27 % of
the pixels there, above the 15 %, so for T = 2 the upper bound is the restatement's own share instead (every case also
asserts the share within 0.1 % of the restatement's, the cap on excluded pixels)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd.datasets.dataset_utils_gpu import (get_ir_pattern, get_smoothed_ir_pattern,  # noqa: E402
                                                       get_smoothed_ir_pattern2, get_temporal_ir_pattern)
from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset  # noqa: E402
from oracle import ir_pattern_oracle as io  # noqa: E402
from tests import _temporal_ir_ref as ref  # noqa: E402

DEV = "cuda:0"
BAND, CAP = 1e-5, 1e-3


def agrees(got, want, margin, what):
    """the rule of the module docstring for one image; prints its figures before it asserts"""
    inside = np.abs(margin) < BAND
    wrong = (got != want) & ~inside
    print(f"{what}: ones {got.mean():.4f} (restatement {want.mean():.4f}), inside the band {int(inside.sum())}, "
          f"differing {int((got != want).sum())}, differing outside the band {int(wrong.sum())}")
    assert inside.mean() <= CAP, f"{what}: {inside.mean():.5f} of the image within {BAND} of the threshold"
    assert not wrong.any(), f"{what}: {int(wrong.sum())} pixels differ, smallest |margin| {np.abs(margin[wrong]).min():.3g}"
    assert abs(got.mean() - want.mean()) <= CAP
    assert set(np.unique(got).tolist()) <= {0.0, 1.0}


def dev_stack(stack, dtype=torch.float32):
    return torch.tensor(stack, dtype=dtype, device=DEV)


@pytest.mark.parametrize("hw,ks,t,batch", [
    ((24, 29), 9, 7, 1),      # smaller than one tile both ways
    ((37, 53), 11, 7, 1),     # ragged partial tiles, odd W: scalar load path
    ((67, 93), 11, 2, 1),     # T limits
    ((67, 93), 11, 16, 1),
    ((16, 200), 31, 7, 1),    # halo 15 of 16 rows: reflection across nearly the whole height
    ((135, 240), 11, 7, 3),   # several tiles, B = 3
])
def test_temporal_pattern_vs_restatement(hw, ks, t, batch):
    stacks = np.stack([ref.exposure_stack(seed, t, *hw) for seed in range(batch)])
    got = get_temporal_ir_pattern(dev_stack(stacks), ks, 0.005).cpu().numpy()
    assert got.shape == (batch,) + hw and got.dtype == np.float32
    for b in range(batch):
        want, margin = ref.temporal_ir_pattern(stacks[b], ks, 0.005)
        agrees(got[b], want, margin, f"{hw} ks {ks} T {t} image {b}")
        assert 0.02 < got[b].mean() < (0.15 if t > 2 else want.mean() + CAP)


def test_uint8_and_float32_stacks_give_the_same_bits():
    for hw in ((37, 53), (40, 64)):  # scalar and vector loads
        stack = ref.exposure_stack(1, 7, *hw)
        a = get_temporal_ir_pattern(dev_stack(stack), 11)
        b = get_temporal_ir_pattern(dev_stack(stack, torch.uint8), 11)
        assert torch.equal(a, b) and 0.02 < float(a.mean()) < 0.15


def test_batch_equals_images_one_by_one_and_3d_equals_4d():
    stacks = dev_stack(np.stack([ref.exposure_stack(seed, 7, 67, 93) for seed in range(3)]), torch.uint8)
    whole = get_temporal_ir_pattern(stacks)
    assert whole.shape == (3, 67, 93)
    for i in range(3):
        one = get_temporal_ir_pattern(stacks[i])
        assert one.shape == (67, 93)
        assert torch.equal(whole[i], one)
        assert torch.equal(get_temporal_ir_pattern(stacks[i:i + 1])[0], one)


def test_constant_stack_gives_all_zeros():
    for dtype in (torch.float32, torch.uint8):
        out = get_temporal_ir_pattern(torch.full((2, 7, 37, 53), 80, dtype=dtype, device=DEV))
        assert out.shape == (2, 37, 53) and not out.any()
    # one flat image beside a live one: the flat one alone is zero
    live = dev_stack(ref.exposure_stack(0, 7, 37, 53))
    out = get_temporal_ir_pattern(torch.stack([torch.full_like(live, 80.0), live]))
    assert not out[0].any() and torch.equal(out[1], get_temporal_ir_pattern(live))


def test_channel_strided_stack_equals_its_contiguous_copy():
    wide = dev_stack(np.stack([ref.exposure_stack(2, 14, 37, 53)]), torch.uint8)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(get_temporal_ir_pattern(view), get_temporal_ir_pattern(view.contiguous()))
    assert torch.equal(get_temporal_ir_pattern(view.float()), get_temporal_ir_pattern(view.contiguous()))


def test_bad_arguments_raise_and_launch_nothing():
    stack = dev_stack(ref.exposure_stack(0, 7, 24, 29))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="AZ_EUNSUPPORTED"):
        get_temporal_ir_pattern(stack, ks=10)
    with pytest.raises(RuntimeError, match="AZ_EUNSUPPORTED"):
        get_temporal_ir_pattern(stack[:1])  # T = 1
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):
        get_temporal_ir_pattern(stack[:, :5], ks=11)  # H <= ks / 2
    with pytest.raises(RuntimeError, match="float32 or torch.uint8"):
        get_temporal_ir_pattern(stack.double())
    with pytest.raises(RuntimeError, match="GPU"):
        get_temporal_ir_pattern(stack.cpu())
    torch.cuda.synchronize()


def dataset_pair(hw):
    """the generator of tests/test_gpu_dataset.py"""
    rng = np.random.default_rng(hw[0])
    base = rng.random(hw)
    dots = (rng.random(hw) < 0.08) * 0.4
    return np.clip(base * 0.5 + dots, 0, 1), base * 0.5


@pytest.mark.parametrize("hw", [(37, 53), (67, 93)])
def test_plain_and_smoothed_patterns_vs_fp64(hw):
    ir, plain = dataset_pair(hw)
    a, b = torch.tensor(ir, dtype=torch.float32, device=DEV), torch.tensor(plain, dtype=torch.float32, device=DEV)
    before = get_smoothed_ir_pattern2(a, b, 11, 0.005)
    # mode 1: diff > diff_avg, against the oracle at threshold 0
    want, margin = io.get_smoothed_ir_pattern2(ir, plain, 11, threshold=0.0, return_margin=True)
    got = get_smoothed_ir_pattern(a, b, 11).cpu().numpy()
    agrees(got, want, margin, f"get_smoothed_ir_pattern {hw}")
    assert 0.01 < got.mean() < 0.5
    # mode 0: dataset_utils.py:12-17 in fp64
    diff = np.abs(ir - plain)
    diff = (diff - np.min(diff)) / (np.max(diff) - np.min(diff))
    want0 = np.zeros_like(diff)
    want0[diff > 0.005] = 1
    got0 = get_ir_pattern(a, b, 0.005).cpu().numpy()
    agrees(got0, want0, diff - 0.005, f"get_ir_pattern {hw}")
    assert 0.01 < got0.mean() < 0.5
    # batched form, and az_ir_pattern untouched by its neighbours
    assert torch.equal(get_ir_pattern(torch.stack([a, a]), torch.stack([b, b]))[1], torch.tensor(got0, device=DEV))
    assert torch.equal(get_smoothed_ir_pattern2(a, b, 11, 0.005), before)


def test_loader_default_is_unchanged_and_temporal_patterns_follow_the_restatement():
    h, w = 64, 128
    plain = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV)
    off = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV, temporal=False)
    on = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=True, device=DEV, temporal=True)
    a, b, c = plain[1], off[1], on[1]
    tensors = [k for k in a if k != "prefix"]
    assert a.keys() == b.keys() == c.keys()
    assert all(torch.equal(a[k], b[k]) for k in tensors) and a["prefix"] == b["prefix"]
    # temporal=True changes the two real patterns and nothing else
    real = ("img_real_L_reproj", "img_real_R_reproj")
    assert all(torch.equal(a[k], c[k]) for k in tensors if k not in real)
    stack = on._temporal_stack(1)
    assert stack.shape == (2, 7, h, w) and stack.dtype == torch.uint8
    for view, key in enumerate(real):
        pat = c[key]
        assert pat.shape == (1, h, w) and pat.dtype == torch.float32
        want, margin = ref.temporal_ir_pattern(stack[view].cpu().numpy(), 11, 0.005)
        agrees(pat[0].cpu().numpy(), want, margin, key)
        assert 0.02 < float(pat.mean()) < 0.15
    # without the real item the keyword has nothing to do
    sim = SyntheticMessytableDataset(length=2, height=h, width=w, onReal=False, device=DEV, temporal=True)
    assert all(torch.equal(sim[1][k], a[k]) for k in sim[1] if k != "prefix")
