"""GPU: the fused ground-truth preparation (K18, az_gt_from_right) against the operator chain it replaces, restated in
tests/_gt_prep_ref.py (CPU F.interpolate, .type(torch.int), the committed scatter oracle, the compares).  Everything is
index, truncation and compare logic: every output and both counters must be EQUAL (torch.equal), no tolerance.

Input generator (`field`): rng = default_rng(seed); every full-resolution pixel draws one of: an integer k in [0, W)
(fraction .0), float32(k + 0.999), uniform(0, W / 2), a value >= W (W, W + 0.5, 3e9, 1e10), a value in (-1, 0) (-0.5,
-0.999), with shares 0.25 / 0.2 / 0.35 / 0.1 / 0.1; every third output row is a ramp of slope -1, d = c - j for j <= c,
which sends c + 1 sources to the one destination c (row 0: c = (W - 1) // 2, the winner's value c is the mask's `hi`), and
its column c + 1 holds `lo`, which lands alone at c + 1 + lo: pixels exactly on both bounds; `hostile` puts -1.0, -3.5, NaN, +inf, -inf on 4 % of the pixels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.utils import gt_prep  # noqa: E402
from activezero_amd.utils.warp_ops import apply_disparity_cu  # noqa: E402
from tests import _gt_prep_ref as ref  # noqa: E402

DEV = "cuda:0"


def out_size(hin, win, kw):
    return tuple(kw["size"]) if "size" in kw else (int(hin * kw["scale_factor"]), int(win * kw["scale_factor"]))


def field(seed, n, hin, win, kw, hostile=True, lo=2.0):
    h, w = out_size(hin, win, kw)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, w, (n, 1, hin, win)).astype(np.float64)
    kinds = rng.choice(5, (n, 1, hin, win), p=[0.25, 0.2, 0.35, 0.1, 0.1])
    d = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3],
                  [k, k + 0.999, rng.uniform(0, w / 2, k.shape), rng.choice([w, w + 0.5, 3e9, 1e10], k.shape)],
                  rng.choice([-0.5, -0.999], k.shape))
    # the source pixel of every output pixel, from the resize itself
    iy = torch.arange(float(hin)).view(1, 1, hin, 1).expand(1, 1, hin, win).contiguous()
    ix = torch.arange(float(win)).view(1, 1, 1, win).expand(1, 1, hin, win).contiguous()
    ys = ref.resize_nearest(iy, **kw)[0, 0, :, 0].long().numpy()
    xs = ref.resize_nearest(ix, **kw)[0, 0, 0, :].long().numpy()
    assert len(ys) == h and len(xs) == w
    for y in range(0, h, 3):
        c = (w - 1) // 2 + y % 2
        for j in range(min(c, w - 1) + 1):
            d[:, 0, ys[y], xs[j]] = c - j
        d[:, 0, ys[y], xs[c + 1]] = lo
    if hostile:
        bad = rng.random(d.shape) < 0.04
        d[bad] = rng.choice([-1.0, -3.5, np.nan, np.inf, -np.inf], int(bad.sum()))
    return torch.tensor(d, dtype=torch.float32)


def channels(seed, n, c, hin, win):
    if c == 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, c, hin, win, generator=g) + torch.arange(1.0, c + 1).view(1, c, 1, 1)  # channel c lies in (c, c + 1)


def dev(t):
    return None if t is None else t.to(DEV)


def same(got, want, what):
    if want is None:
        assert got is None, what
        return
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    diff = int((got != want).sum())
    print(f"{what}: {tuple(want.shape)}, {diff} elements differ")
    assert torch.equal(got, want), f"{what}: {diff} elements differ"


def compare(d, extra, keep, kw, lo, hi):
    want = ref.gt_from_right(d, extra, keep, lo=lo, hi=hi, **kw)
    got = ops.gt_from_right(dev(d), dev(extra), dev(keep), lo=lo, hi=hi, **kw)
    for g, w, what in zip(got, want, ("disp_l", "extra_l", "keep_s", "mask", "stats")):
        same(g, w, what)
    return got, want


# (N, Hin, Win, resize, Ce, Ck, lo); hi = (W - 1) // 2: pixels lie exactly on both bounds (see `field`)
CASES = {
    "W5_less_than_a_wave":          (2, 12, 10, {"scale_factor": 0.5}, 0, 0, 1.0),
    "W70_two_lane_passes_7_rows":   (1, 14, 140, {"scale_factor": 0.5}, 1, 1, 2.0),
    "W129_N2_odd_input_sizes":      (2, 7, 259, {"scale_factor": 0.5}, 2, 2, 2.0),
    "N2_odd_height_only":           (2, 11, 24, {"scale_factor": 0.5}, 2, 1, 2.0),
    "odd_width_only":               (1, 8, 27, {"scale_factor": 0.5}, 1, 2, 2.0),
    "ratio_1":                      (1, 5, 33, {"size": (5, 33)}, 1, 0, 2.0),
    "ratio_1p5_9_to_6":             (1, 9, 9, {"size": (6, 6)}, 0, 2, 1.0),
    "W4096_H1":                     (1, 2, 8192, {"scale_factor": 0.5}, 1, 1, 2.0),
}


def case(name, seed):
    n, hin, win, kw, ce, ck, lo = CASES[name]
    hi = float((out_size(hin, win, kw)[1] - 1) // 2)
    return field(seed, n, hin, win, kw, lo=lo), channels(1, n, ce, hin, win), channels(2, n, ck, hin, win), kw, lo, hi


@pytest.mark.parametrize("name", list(CASES))
def test_fused_call_equals_the_chain(name):
    d, extra, keep, kw, lo, hi = case(name, 9)
    (disp_l, _, _, mask, stats), want = compare(d, extra, keep, kw, lo, hi)
    # the case is not vacuous: something lands, something misses, something is refused, and pixels sit ON both bounds
    w_stats = want[4].tolist()
    assert w_stats[0] > 0 and 0 < w_stats[1] < want[0].numel()
    assert (want[0] == lo).any() and (want[0] == hi).any() and (want[0] == 0).any()
    assert mask.dtype == torch.bool and disp_l.shape == (d.shape[0], 1) + out_size(*d.shape[2:], kw)


def test_mask_is_a_view_and_both_forms_come_back():
    d = field(3, 1, 14, 140, {"scale_factor": 0.5}, hostile=False)
    disp_l, _, _, mask, stats = ops.gt_from_right(dev(d), lo=0.0, hi=30.0)
    assert mask.dtype == torch.bool and mask.is_contiguous()
    u8 = ops._mask_u8(mask, disp_l)
    assert u8.dtype == torch.uint8 and u8.data_ptr() == mask.data_ptr()  # same bytes, no copy
    assert ops._mask_u8(u8, disp_l).data_ptr() == mask.data_ptr()
    assert set(u8.unique().tolist()) <= {0, 1} and int(u8.sum()) == int(stats[1])


def test_check_raises_on_a_hostile_field_only():
    kw = {"scale_factor": 0.5}
    clean, hostile = field(5, 1, 14, 140, kw, hostile=False), field(5, 1, 14, 140, kw, hostile=True)
    out = ops.gt_from_right(dev(clean), check=True)
    assert int(out[4][0]) == 0
    with pytest.raises(AssertionError, match="not finite"):
        ops.gt_from_right(dev(hostile), check=True)
    assert int(ops.gt_from_right(dev(hostile))[4][0]) > 0  # without check: counted, not raised


def test_check_is_available_through_the_prepare_helpers():
    kw = {"scale_factor": 0.5}
    clean, hostile = field(6, 1, 14, 140, kw, hostile=False).to(DEV), field(6, 1, 14, 140, kw, hostile=True).to(DEV)
    depth = channels(3, 1, 1, 14, 140).to(DEV)
    assert len(gt_prep.prepare_sim_gt((clean, depth), 192, check=True)) == 3
    assert len(gt_prep.prepare_sim_gt((hostile, depth), 192)) == 3  # counted on the device, not raised
    with pytest.raises(AssertionError, match="not finite"):
        gt_prep.prepare_sim_gt((hostile, depth), 192, check=True)
    with pytest.raises(AssertionError, match="not finite"):
        gt_prep.prepare_test_gt((hostile, depth, depth), size=(7, 70), check=True)
    assert len(gt_prep.prepare_test_gt((clean, depth, depth), size=(7, 70), check=True)) == 3


def test_two_calls_give_identical_bytes():
    d, extra, keep, kw, lo, hi = case("W129_N2_odd_input_sizes", 9)
    args = [dev(d), dev(extra), dev(keep)]
    a, b = ops.gt_from_right(*args, lo=lo, hi=hi, **kw), ops.gt_from_right(*args, lo=lo, hi=hi, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def raw_call(d, extra, keep, h, w, lo, hi, with_mask, sentinel):
    """az_gt_from_right on output buffers pre-filled with a sentinel (scale factor 0.5)"""
    n, _, hin, win = d.shape
    ce, ck = (0 if t is None else t.shape[1] for t in (extra, keep))
    full = lambda c: torch.full((n, c, h, w), sentinel, device=DEV) if c else None  # noqa: E731
    disp_l, extra_l, keep_s = full(1), full(ce), full(ck)
    mask = torch.full((n, 1, h, w), 0xAB, dtype=torch.uint8, device=DEV) if with_mask else None
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = ops._p
    ops._call("az_gt_from_right", p(disp_l), p(extra_l), p(keep_s), p(mask), p(stats), p(d), p(extra), p(keep), n, ce, ck,
              hin, win, h, w, 2.0, 2.0, lo, hi, ops._stream())
    return disp_l, extra_l, keep_s, mask, stats


@pytest.mark.parametrize("with_mask", [True, False])
def test_sentinel_filled_outputs_are_fully_overwritten_and_mask_may_be_null(with_mask):
    d, extra, keep, kw, lo, hi = case("W70_two_lane_passes_7_rows", 11)
    want = ref.gt_from_right(d, extra, keep, lo=lo, hi=hi, **kw)
    got = raw_call(dev(d), dev(extra), dev(keep), 7, 70, lo, hi, with_mask, 12345.0)
    for g, w, what in zip(got[:3], want[:3], ("disp_l", "extra_l", "keep_s")):
        same(g, w, what)
    same(got[4], want[4], "stats")  # the mask pixels are counted with or without a mask pointer
    if with_mask:
        same(got[3].view(torch.bool), want[3], "mask")
    else:
        assert got[3] is None


def test_training_size_through_prepare_sim_gt():
    """[4,1,1080,1920] -> 540 x 960 with keep = depth: the synthetic loader's batch through prepare_sim_gt, against the
    three lines tools/train_rehearsal.py held before (train.py:255-272 on this library's own scatter warp)"""
    from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset

    ds = SyntheticMessytableDataset(length=4, height=540, width=960, onReal=False, device=DEV)
    sample = next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)))
    assert sample["img_disp_R"].shape == (4, 1, 1080, 1920)
    disp_gt_l, depth_gt, mask = gt_prep.prepare_sim_gt(sample, 192)
    half = lambda t: F.interpolate(t, scale_factor=0.5, mode="nearest", recompute_scale_factor=False)  # noqa: E731
    img_disp_r = half(sample["img_disp_R"])
    want_disp = apply_disparity_cu(img_disp_r, img_disp_r.type(torch.int))
    want_mask = (want_disp < 192) * (want_disp > 0)
    assert torch.equal(disp_gt_l, want_disp) and torch.equal(depth_gt, half(sample["img_depth_L"]))
    assert mask.dtype == torch.bool and torch.equal(mask, want_mask)
    assert 0 < int(mask.sum()) < mask.numel()
    # the tensors themselves are accepted in place of the sample
    again = gt_prep.prepare_sim_gt((sample["img_disp_R"], sample["img_depth_L"]), 192)
    assert all(torch.equal(a, b) for a, b in zip(again, (disp_gt_l, depth_gt, mask)))


def test_prepare_test_gt_equals_its_chain():
    """test.py:91-110 at [1,1,36,64] with size=(18,32): disparity and depth warped together, the label resized"""
    kw = {"size": (18, 32)}
    d = field(21, 1, 36, 64, kw, hostile=False)
    depth, label = channels(4, 1, 1, 36, 64), torch.randint(0, 17, (1, 1, 36, 64)).float()
    want_disp, want_depth, want_label, _, _ = ref.gt_from_right(d, depth, label, **kw)
    data = {"img_disp_R": d.to(DEV), "img_depth_R": depth.to(DEV), "img_label": label.to(DEV)}
    img_disp_l, img_depth_l, img_label = gt_prep.prepare_test_gt(data, size=(18, 32))
    same(img_disp_l, want_disp, "img_disp_l")
    same(img_depth_l, want_depth, "img_depth_l")
    same(img_label, want_label.type(torch.int), "img_label")
    assert (want_disp != 0).any() and (want_depth != 0).any()
