"""GPU: K25 az_depth_labels and K26 az_test_images (csrc/az_test_inputs.hip) against the restatements of
tests/_test_inputs_ref.py -- K25 bit for bit, K26's float image form within 6 M 2^-24 (M the largest tap; the bound is derived
there and met by torch's own CPU operator in tests/test_test_inputs_cpu.py), its grey-level form bit for bit against the float
form --, the synthetic test-mode dataset, and tools/test_rehearsal.py, the loop of test.py around them, against the torch
operator form of the same lines on the same prediction."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.datasets.dataset_utils_gpu import augment_images, depth_to_labels  # noqa: E402
from activezero_amd.datasets.messytable_test_synthetic import SyntheticMessytableTestDataset  # noqa: E402
from activezero_amd.utils import gt_prep  # noqa: E402
from activezero_amd.utils.result_images import PANELS  # noqa: E402
from tests import _gt_prep_ref as G  # noqa: E402
from tests import _obj_metrics_ref as O  # noqa: E402
from tests import _reduce_ref as R  # noqa: E402
from tests import _test_inputs_ref as T  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
FOCAL, BASE = 446.31, 0.055


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    for name, g, w in zip(("disp_l", "depth_l", "disp_r", "depth_r"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, (what, name, tuple(g.shape), w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)


# ---- K25 -------------------------------------------------------------------------------------------------------------
def test_depth_labels_every_uint16_value():
    left = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    right = np.random.default_rng(2500).permutation(65536).astype(np.uint16).reshape(1, 256, 256)
    got = ops.depth_labels(dev(left), dev(right), FOCAL, BASE)
    same(got, T.depth_labels(left, right, FOCAL, BASE), "every value")
    assert float(got[0][0, 0, 0, 0]) == 0.0 and float(got[1][0, 0, 0, 0]) == 0.0  # v = 0: no disparity, no depth


def _maps(seed, shape, dtype=np.uint16):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 65536, (2,) + shape).astype(dtype)
    a[rng.random(a.shape) < 0.1] = 0  # holes
    return a[0], a[1]


def test_depth_labels_two_items_with_their_own_constants():
    fl, bl = np.array([446.31, 901.5]), np.array([0.055, 0.1203])
    for shape in ((2, 13, 37), (2, 8, 24)):  # a pitch that is no multiple of four, one that is
        left, right = _maps(2510 + shape[2], shape)
        got = ops.depth_labels(dev(left), dev(right), dev(fl), dev(bl))
        want = T.depth_labels(left, right, fl, bl)
        same(got, want, shape)
        # (item 1 with item 0's constants would be another map)
        assert not np.array_equal(want[0][1], T.depth_labels(left[1:], right[1:], fl[0], bl[0])[0][0])
        # float32 constants, as the item dictionary holds them, are taken as the float64 values they are
        got32 = ops.depth_labels(dev(left), dev(right), dev(fl.astype(F32)), dev(bl.astype(F32)))
        same(got32, T.depth_labels(left, right, fl.astype(F32).astype(np.float64), bl.astype(F32).astype(np.float64)), "f32")


WINDOWS = [(0, 0, 8, 16), (16, 24, 8, 16), (3, 5, 6, 7), (17, 33, 7, 7), (2, 4, 5, 12), (0, 0, 24, 40)]


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "-".join(map(str, w)))
def test_depth_labels_one_window_for_every_item(win):
    """the origin, the far corner, an odd width (w2 = 7) at an odd and at the last column, a source quad that is aligned with
    an output pitch that allows vector stores, and the whole map as a window"""
    left, right = _maps(2520, (2, 24, 40))
    y0, x0, h2, w2 = win
    got = depth_to_labels(dev(left), dev(right), FOCAL, BASE, crop=win)
    same(got, T.depth_labels(left, right, FOCAL, BASE, [[y0, x0]] * 2, (h2, w2)), win)
    whole = T.depth_labels(left, right, FOCAL, BASE)
    assert np.array_equal(got[2].cpu().numpy(), whole[2][:, :, y0:y0 + h2, x0:x0 + w2])


@pytest.mark.parametrize("origins,window", [([[0, 0], [16, 24]], (8, 16)), ([[3, 5], [17, 33]], (7, 7)), ([[1, 8], [0, 3]], (23, 32)),
                                            ([[-3, 100], [30, -1]], (6, 7))], ids=["corners", "odd", "mixed alignment", "clamped"])
def test_depth_labels_a_window_per_item(origins, window):
    left, right = _maps(2530, (2, 24, 40))
    origin = torch.tensor(origins, dtype=torch.int32).to(DEV)
    got = depth_to_labels(dev(left), dev(right), FOCAL, BASE, crop=(origin, window))
    same(got, T.depth_labels(left, right, FOCAL, BASE, origins, window), origins)


def test_depth_labels_whole_map_and_single_item_form():
    left, right = _maps(2540, (1, 12, 20))
    got = depth_to_labels(dev(left[0]), dev(right[0]), FOCAL, BASE)
    assert all(tuple(g.shape) == (1, 12, 20) for g in got)
    same([g[None] for g in got], T.depth_labels(left, right, FOCAL, BASE), "single")
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):  # no origin: the window is the map
        ops._call("az_depth_labels", *(got[0].data_ptr(),) * 4, dev(left).data_ptr(), dev(right).data_ptr(), 0,
                  dev(np.array([FOCAL])).data_ptr(), dev(np.array([BASE])).data_ptr(), None, 1, 12, 20, 6, 20, None)


def test_depth_labels_int32_with_zero_negative_and_large_values():
    rng = np.random.default_rng(2550)
    for shape in ((2, 9, 11), (1, 6, 16)):
        left = rng.integers(-3000, 200000, shape).astype(np.int32)
        right = rng.integers(0, 70000, shape).astype(np.int32)
        left.ravel()[:6] = (0, -1, -2 ** 31, 2 ** 31 - 1, 65536, 1)
        right.ravel()[-3:] = (0, 65535, 100000)
        got = ops.depth_labels(dev(left), dev(right), FOCAL, BASE)
        want = T.depth_labels(left, right, FOCAL, BASE)
        same(got, want, shape)
        assert (want[0][left[:, None] <= 0] == 0).all() and (want[1][left[:, None] < 0] < 0).all()
        origin = torch.tensor([[1, 3]] * shape[0], dtype=torch.int32).to(DEV)
        same(ops.depth_labels(dev(left), dev(right), FOCAL, BASE, origin, (4, 8)),
             T.depth_labels(left, right, FOCAL, BASE, [[1, 3]] * shape[0], (4, 8)), "int32 window")


def test_depth_labels_does_not_synchronise():
    left, right = _maps(2560, (2, 24, 40))
    a, b = dev(left), dev(right)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        depth_to_labels(a, b, FOCAL, BASE)
        depth_to_labels(a, b, FOCAL, BASE, crop=(2, 4, 8, 16))
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- K26, the float image form ---------------------------------------------------------------------------------------
def _float_case(seed, n, hin, win):
    return T.normalise(T.random_levels(seed, n, hin, win))


def check_images(got, src, size, pad, what):
    want = T.resize_pad(src, size, pad)
    got = got.cpu().numpy()
    assert got.dtype == F32 and got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"\n  {what}: max |kernel - restatement| = {err / (T.bound(src) / 6):.2f} M 2^-24", end="")
    assert err <= T.bound(src), (what, err, T.bound(src))
    pads = np.ones(got.shape, dtype=bool)
    pads[:, :, pad[0]:, :size[1]] = False
    assert not got.view(np.uint32)[pads].any(), what  # the bits of +0.0


SMALL = list(zip(T.SIZE_PAIRS, T.PADS)) + [(((6, 10), (9, 12)), (1, 4))]  # the last: a padded pitch of 16, vector stores


@pytest.mark.parametrize("sizes,pad", SMALL, ids=lambda v: "x".join(map(str, np.ravel(v))))
def test_images_float_form_small_sizes(sizes, pad):
    (hin, win), size = sizes
    src = _float_case(2600 + hin, 3, hin, win)
    check_images(ops.test_images(dev(src), size=size, pad=pad), src, size, pad, f"{sizes} one source")
    # the second view from its own tensor: the same images in the same order
    both = ops.test_images(dev(src[:2]), dev(src[2:]), size=size, pad=pad)
    check_images(both, src, size, pad, f"{sizes} two sources")
    if (hin, win) == size:  # the identity only pads: bit-equal to its finite input
        assert torch.equal(both[:, :, pad[0]:, :win].cpu(), torch.from_numpy(src))


def test_images_float_form_at_the_test_size():
    (hin, win), size, pad = T.LARGE
    src = _float_case(2610, 2, hin, win)
    img_l, img_r = gt_prep.prepare_test_images(dev(src[:1]), dev(src[1:]))
    assert tuple(img_l.shape) == tuple(img_r.shape) == (1, 3, 544, 960)
    check_images(torch.cat([img_l, img_r]), src, size, pad, "720x1280 -> 540x960")


def test_images_sim_branch_only_pads():
    src = _float_case(2620, 2, 20, 28)
    img_l, img_r = gt_prep.prepare_test_images(dev(src[:1]), dev(src[1:]), size=(20, 28), pad_to=(24, 32))
    want = F.pad(torch.from_numpy(src), (0, 4, 4, 0, 0, 0, 0, 0), mode="constant", value=0)
    assert torch.equal(torch.cat([img_l, img_r]).cpu(), want)


def test_images_non_finite_taps_follow_ieee():
    """a NaN and an inf tap: exactly the outputs whose four taps include one of them -- with any weight, 0 too: 0 * inf is
    NaN, as in ATen -- are not finite, and no pad element is touched"""
    for (hin, win), size, pad in (((13, 17), (13, 17), (4, 0)), ((33, 47), (20, 31), (1, 2)), ((5, 6), (7, 9), (0, 3))):
        src = _float_case(2630 + hin, 1, hin, win)
        src[0, 0, hin // 2, win // 3] = np.nan
        src[0, 1, hin // 3, win // 2] = np.inf
        src[0, 2, hin - 1, win - 1] = -np.inf
        got = ops.test_images(dev(src), size=size, pad=pad).cpu().numpy()
        want = T.resize_pad(src, size, pad)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and not np.isfinite(want).all()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin].astype(np.float64) - want[fin]).max() <= T.bound(src)
        assert not got[:, :, :pad[0]].view(np.uint32).any() and not got[:, :, :, size[1]:].view(np.uint32).any()


def test_images_do_not_synchronise():
    src = dev(_float_case(2640, 2, 20, 28))
    levels = dev(T.random_levels(2641, 2, 20, 28))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.test_images(src, size=(15, 21), pad=(1, 3))
        ops.test_images(levels[:1], levels[1:], size=(15, 21), pad=(1, 3))
        gt_prep.prepare_test_images(src[:1], src[1:], size=(15, 21), pad_to=(16, 24))
        gt_prep.prepare_test_images(levels[:1], levels[1:], size=(20, 28), pad_to=(24, 28))
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- K26, the grey-level form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,pad", SMALL + [(T.LARGE[:2], T.LARGE[2])], ids=lambda v: "x".join(map(str, np.ravel(v))))
def test_images_level_form_equals_float_form_of_the_normalised_levels(sizes, pad):
    (hin, win), size = sizes
    levels = dev(T.random_levels(2700 + hin, 2, hin, win))
    if min(hin, win) > 4:  # (az_augment takes no image of fewer pixels than its blur reflects, whatever its switches)
        normalised = augment_images(levels)
        assert torch.equal(normalised.cpu(), torch.from_numpy(T.normalise(levels.cpu().numpy())))
    else:                  # ... so the one-row case takes the restatement of the same three operations
        normalised = dev(T.normalise(levels.cpu().numpy()))
    got = ops.test_images(levels[:1], levels[1:], size=size, pad=pad)
    assert torch.equal(got, ops.test_images(normalised, size=size, pad=pad))


def test_images_level_form_every_level_in_every_channel():
    levels = dev(np.arange(256, dtype=np.uint8).reshape(1, 16, 16))
    want = augment_images(levels)
    got = ops.test_images(levels, pad=(2, 1))  # the identity: every level leaves as its normalised value, per channel
    assert torch.equal(got[:, :, 2:, :16], want) and not got[:, :, :2].any() and not got[:, :, :, 16:].any()
    assert torch.equal(ops.test_images(levels, size=(11, 23), pad=(0, 1)), ops.test_images(want, size=(11, 23), pad=(0, 1)))


# ---- the synthetic test item -----------------------------------------------------------------------------------------
def test_synthetic_test_item_dictionary():
    """keys, shapes and dtypes as the module's docstring lists them; the labels are K25's restatement on the item's own maps"""
    h, w, hr, wr = 36, 48, 48, 64
    ds = SyntheticMessytableTestDataset(length=3, height=h, width=w, real_size=(hr, wr), device=DEV)
    item = ds[1]
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    want = {"img_sim_L": ((3, h, w), f32), "img_sim_R": ((3, h, w), f32),
            "img_disp_L": ((1, 2 * h, 2 * w), f32), "img_depth_L": ((1, 2 * h, 2 * w), f32),
            "img_disp_R": ((1, 2 * h, 2 * w), f32), "img_depth_R": ((1, 2 * h, 2 * w), f32),
            "img_depth_sim_realsense": ((2 * h, 2 * w), f64), "focal_length": ((1, 1, 1), f32), "baseline": ((1, 1, 1), f32),
            "img_real_L": ((3, hr, wr), f32), "img_real_R": ((3, hr, wr), f32),
            "img_real_L_levels": ((hr, wr), u8), "img_real_R_levels": ((hr, wr), u8),
            "img_depth_real_realsense": ((hr, wr), f64), "robot_mask": ((2 * h, 2 * w), f64),
            "img_label": ((1, 2 * h, 2 * w), f32)}
    host = {"intrinsic": (3, 3), "intrinsic_l": (3, 3), "extrinsic": (4, 4), "extrinsic_l": (4, 4)}
    assert set(item) == set(want) | set(host) | {"prefix"}
    for k, (shape, dtype) in want.items():
        assert tuple(item[k].shape) == shape and item[k].dtype == dtype and item[k].device.type == "cuda", k
    for k, shape in host.items():
        assert isinstance(item[k], np.ndarray) and item[k].shape == shape and item[k].dtype == np.float64, k
    assert isinstance(item["prefix"], str)
    # the labels: K25 on the uint16 millimetre maps
    mm_l, mm_r = ds.depth_mm(1)
    assert mm_l.dtype == mm_r.dtype == torch.uint16 and tuple(mm_l.shape) == (2 * h, 2 * w)
    mm = [m.cpu().view(torch.int16).numpy().view(np.uint16)[None] for m in (mm_l, mm_r)]
    assert 400 < mm[0].min() and mm[0].max() < 1600 and (mm[1] == 0).any()  # metres as millimetres; the right view has holes
    labels = T.depth_labels(mm[0], mm[1], ds.focal_length, ds.baseline)
    for k, lab in zip(("img_disp_L", "img_depth_L", "img_disp_R", "img_depth_R"), labels):
        assert torch.equal(item[k].cpu(), torch.from_numpy(lab[0])), k
    assert float(item["focal_length"]) == F32(ds.focal_length) and float(item["baseline"]) == F32(ds.baseline)
    # value conventions
    lab = item["img_label"]
    assert torch.equal(lab, lab.round()) and len(lab.unique()) >= 3 and 17 in lab.unique().tolist() and lab.min() >= 0
    assert (item["img_depth_real_realsense"] == 0).any() and (item["img_depth_sim_realsense"] == 0).any()
    assert set(item["robot_mask"].unique().tolist()) == {0.0, 0.3, 0.6, 1.0}
    assert torch.equal(item["img_real_L"], augment_images(item["img_real_L_levels"]))
    # determinism per index, variation across indices, and the default collate
    again = ds[1]
    assert all(torch.equal(item[k], again[k]) for k in want)
    assert not torch.equal(item["img_real_L_levels"], ds[2]["img_real_L_levels"])
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0)))
    assert tuple(batch["img_disp_R"].shape) == (2, 1, 2 * h, 2 * w) and tuple(batch["robot_mask"].shape) == (2, 2 * h, 2 * w)
    assert tuple(batch["intrinsic_l"].shape) == (2, 3, 3) and len(batch["prefix"]) == 2


# ---- the loop of test.py ---------------------------------------------------------------------------------------------
def test_rehearsal_against_the_torch_operator_form(tmp_path):
    """tools/test_rehearsal.py at the smallest size the network takes (252 x 256 padded to 256 x 256: the extractor pools
    64 x 64 windows at a quarter of the resolution), B = 2, 32 disparities: it runs to the end, writes its JSON and the
    images, and on the SAME pred_disp the torch operator form of test.py:91-233 gives the same ground truth, label and mask
    (exactly, as tests/test_gpu_gt_prep.py and tests/test_gpu_eval_mask.py hold K18 and K23), the same network inputs (K26's
    bound) and the same per-image metrics and object table (the bounds of tests/_obj_metrics_ref.py for K22)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import test_rehearsal as tr
    from activezero_amd.nets.psmnet.psmnet_3 import PSMNet

    size, pad_to, real_size, md, obj_num = (252, 256), (256, 256), (336, 342), 32, 18
    ds = SyntheticMessytableTestDataset(length=2, height=size[0], width=size[1], real_size=real_size, device=DEV, max_disp=md)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)
    torch.manual_seed(1)
    model = PSMNet(md).to(DEV)
    batches = []
    summary = tr.run(loader, model, str(tmp_path), md, size, pad_to, obj_num, on_batch=lambda *b: batches.append(b))
    assert json.load(open(tmp_path / "metrics.json")) == summary and summary["instances"] == 2
    for panel in PANELS:
        assert sorted(os.listdir(tmp_path / panel)) == ["synthetic-test-00000.png", "synthetic-test-00001.png"]

    (data, out), = batches
    pred_disp = out["pred_disp"]
    assert tuple(pred_disp.shape) == (2, 1) + size and bool(torch.isfinite(pred_disp).all())
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in data.items()}
    # test.py:91-110
    disp_l, depth_l, label, _, _ = G.gt_from_right(cpu["img_disp_R"], extra=cpu["img_depth_R"], keep=cpu["img_label"], size=size)
    label = label.type(torch.int)
    assert torch.equal(out["img_disp_l"].cpu(), disp_l) and torch.equal(out["img_depth_l"].cpu(), depth_l)
    assert torch.equal(out["img_label"].cpu(), label)
    # :112-117, 162-193
    robot = F.interpolate(cpu["robot_mask"].unsqueeze(1), size, mode="nearest", recompute_scale_factor=False).type(torch.int) == 0
    ground = (depth_l > 0) & (depth_l < 1.25)
    mask = (disp_l < md) * (disp_l > 0) * ground * robot
    realsense = F.interpolate(cpu["img_depth_real_realsense"].unsqueeze(1), size, mode="nearest", recompute_scale_factor=False)
    mask = (mask * (realsense > 0)).type(torch.bool)
    assert torch.equal(out["mask"].cpu(), mask) and 0.05 < mask.float().mean() < 0.95
    # :118-146
    src = torch.cat([cpu["img_real_L"], cpu["img_real_R"]]).numpy()
    check_images(torch.cat([out["img_L"], out["img_R"]]), src, size, (pad_to[0] - size[0], pad_to[1] - size[1]), "rehearsal")
    again = tr.evaluate_batch(data, model, md, size, pad_to, obj_num, levels=True)  # the grey-level form: the same inputs
    assert torch.equal(again["img_L"], out["img_L"]) and torch.equal(again["img_R"], out["img_R"])
    # :209-233 on the same prediction
    fb = (cpu["focal_length"] * cpu["baseline"]).reshape(-1).numpy()
    c = dict(B=2, n=2 * size[0] * size[1], per_batch=size[0] * size[1], L=obj_num, name="rehearsal", fb=fb,
             dg=disp_l.numpy(), zg=depth_l.numpy(), dp=pred_disp.cpu().numpy(), mask=mask.numpy().astype(np.uint8),
             label=label.numpy().astype(np.int32))
    for b in range(2):
        want = R.metrics_scalars(*O.image_slice(c, None, b))
        assert sorted(out["err_metrics"][b]) == sorted(R.METRIC_KEYS)
        for key, (v, lim) in want.items():
            assert abs(out["err_metrics"][b][key] - v) <= lim, (b, key, out["err_metrics"][b][key], v, lim)
    vals, lims, count = O.obj_err_scalars(c, None, per_image=True)
    assert np.array_equal(out["obj_err"][3], count) and count.max() == 2 and (count > 0).sum() >= 3
    for k in range(3):
        seen = count > 0
        assert np.array_equal(np.isnan(out["obj_err"][k]), np.isnan(vals[k]))
        ok = seen & np.isfinite(vals[k])
        assert (np.abs(out["obj_err"][k][ok] - vals[k][ok]) <= lims[k][ok]).all(), k
        assert not out["obj_err"][k][~seen].any()
    # ... and the summary is the loop's arithmetic on those numbers (test.py:275-282)
    for key in R.METRIC_KEYS:
        assert summary["metrics"][key] == pytest.approx(sum(e[key] for e in out["err_metrics"]) / 2, rel=1e-12)
    for k, name in enumerate(("disp_err", "depth_err", "depth_4_err")):
        for l in np.flatnonzero(count):
            if np.isfinite(vals[k][l]):
                assert summary["objects"][name][l] == pytest.approx(out["obj_err"][k][l] / count[l], rel=1e-12)
    assert summary["objects"]["disp_err"][obj_num - 2] is None  # an object no instance shows: 0 / 0
