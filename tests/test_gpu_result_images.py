"""GPU: the six result images of a test batch (K24, az_result_images) byte for byte against what matplotlib's plt.imsave wrote
for the committed cases (tests/golden/g16_result_images.npz) and against the numpy restatement of tests/_result_images_ref.py.
The kernel evaluates the same float32 operations with IEEE division, then compares, truncates and looks up: every byte must
be EQUAL, no tolerance.  Both kernel variants run: four pixels per thread (W % 4 == 0 and aligned maps: `contract`, the
full-size image, an aligned pitch) and one pixel per thread (every other case, a misaligned view)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.utils import error_images as ei  # noqa: E402
from activezero_amd.utils import result_images as ri  # noqa: E402
from tests import _result_images_ref as ref  # noqa: E402

DEV = torch.device("cuda", 0)
CASES = ("one_on", "one_off", "batch3", "clip", "boundary", "md100", "contract", "pitched")
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def golden(name):
    """the case's tensors on the device (the prediction as a VIEW of its stored form) and plt.imsave's bytes, once per case"""
    if name not in _cache:
        if "golden" not in _cache:
            _cache["golden"] = ref.golden_cases()
        case, want = _cache["golden"][name]
        want.setflags(write=False)
        y0, h, w = (int(v) for v in case["view"])
        t = {"pred": dev(case["pred"])[:, :, y0:y0 + h, :w], "gt_disp": dev(case["gt_disp"]), "gt_depth": dev(case["gt_depth"]),
             "mask": dev(case["mask"]), "focal": dev(case["focal"]), "baseline": dev(case["baseline"]),
             "max_disp": float(case["max_disp"])}
        _cache[name] = (case, t, want)
    return _cache[name]


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    px = (got != want).any(-1)
    print(f"{what}: {want.shape}, {int(px.sum())} pixels differ")
    assert np.array_equal(got, want), f"{what}: {int(px.sum())} pixels differ, first (b, panel, y, x) {np.argwhere(px)[:6].tolist()}"


def render(t, **kw):
    return ops.result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"], t["focal"] * t["baseline"], t["max_disp"], **kw)


@pytest.mark.parametrize("name", CASES)
def test_every_committed_case_is_imsaves_bytes(name):
    case, t, want = golden(name)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # nothing below may synchronise
    try:
        fb = t["focal"] * t["baseline"]
        got, flags = ops.result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"], fb, t["max_disp"], return_flags=True)
        shaped = (t["focal"].view(-1, 1, 1, 1), t["baseline"].view(-1, 1, 1, 1))  # test.py's [B,1,1,1]
        again = ri.render_result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"].view(torch.bool), *shaped, t["max_disp"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    same(got, want, f"{name} ops.result_images")
    same(again, want, f"{name} render_result_images")
    ref_img, ref_flags = ref.run_case(case)
    assert np.array_equal(ref_img, want)
    assert flags.dtype == torch.int32 and flags.cpu().numpy().tolist() == ref_flags.tolist()


def test_flags_per_image_and_per_panel():
    _, t, _ = golden("batch3")
    _, flags = render(t, return_flags=True)
    # image 0: nothing bad; image 1: masked pixels, bad in all four maps; image 2: one gt_disp == -1, panel 1 alone
    assert flags.tolist() == [0, 0b11011, 0b00010]
    _, t, _ = golden("one_off")
    assert render(t, return_flags=True)[1].tolist() == [0b11011]
    # a prediction that IS -1, and one whose depth is: fb / pred == -1
    pred = torch.tensor([[[[-1.0, 5.0]]], [[[5.0, -2.0]]]], device=DEV)
    ones = torch.ones_like(pred)
    _, flags = ops.result_images(pred, ones, ones, ones > 0, torch.tensor([3.0, 2.0], device=DEV), 192, return_flags=True)
    assert flags.tolist() == [0b00001, 0b01000]


def test_mask_as_bool_and_as_uint8_and_other_thresholds():
    case, t, want = golden("clip")
    same(ops.result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"].view(torch.bool), t["focal"] * t["baseline"], 192), want, "bool mask")
    same(ops.result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"] * 255, t["focal"] * t["baseline"], 192), want, "uint8 mask of 255s")
    kw = dict(depth_hi=0.9, disp_abs_thres=2.0, disp_rel_thres=0.1, depth_scale=100.0, depth_abs_thres=0.5)
    same(render(t, **kw), ref.run_case(case, **kw)[0], "other thresholds")


@pytest.mark.parametrize("name,pad", [("pitched", None), ("contract", (4, 8)), ("contract", (3, 5)), ("contract", "shifted")],
                         ids=["stored", "aligned-pitch", "odd-pitch", "misaligned-base"])
def test_a_pitched_view_equals_its_contiguous_copy(name, pad):
    case, t, want = golden(name)
    pred = t["pred"]
    if pad == "shifted":  # W % 4 == 0 but the view starts one float off a 16-byte boundary
        store = torch.full((pred.shape[0], 1, pred.shape[2], pred.shape[3] + 4), 7777.0, device=DEV)
        store[:, :, :, 1:1 + pred.shape[3]] = pred
        view = store[:, :, :, 1:1 + pred.shape[3]]
    elif pad is not None:
        store = torch.full((pred.shape[0], 1, pred.shape[2] + pad[0], pred.shape[3] + pad[1]), 7777.0, device=DEV)
        store[:, :, pad[0]:, :pred.shape[3]] = pred
        view = store[:, :, pad[0]:, :pred.shape[3]]
    else:
        view = pred
    assert not view.is_contiguous() and torch.equal(view, pred)
    fb = t["focal"] * t["baseline"]
    same(ops.result_images(view, t["gt_disp"], t["gt_depth"], t["mask"], fb, t["max_disp"]), want, "the view")
    same(ops.result_images(view.contiguous(), t["gt_disp"], t["gt_depth"], t["mask"], fb, t["max_disp"]), want, "its copy")


def full_size():
    """B = 1 at 540 x 960: seeded random maps, about 30 % masked, a few NaN / inf / -1 values; the restatement's bytes"""
    if "full" not in _cache:
        pd, gd, gz, mask, focal, baseline = ref.random_maps(2409, 1, 540, 960, masked=0.3, quantum=False)
        flat = pd.reshape(-1)
        flat[[1000, 200000, 300001]] = np.nan, np.inf, -1.0
        gd.reshape(-1)[[5000, 400000]] = -1.0, np.nan
        gz.reshape(-1)[[7000, 450000]] = np.inf, -1.0
        want, flags = ref.result_images(pd, gd, gz, mask, focal, baseline, 192.0)
        want.setflags(write=False)
        t = {k: dev(v) for k, v in dict(pred=pd, gt_disp=gd, gt_depth=gz, mask=mask, focal=focal, baseline=baseline).items()}
        _cache["full"] = (dict(t, max_disp=192.0), want, flags)
    return _cache["full"]


def test_full_size_equals_the_restatement_and_overwrites_its_outputs():
    t, want, want_flags = full_size()
    assert 0.25 < 1 - float(t["mask"].float().mean()) < 0.35
    fb = t["focal"] * t["baseline"]
    same(ops.result_images(t["pred"], t["gt_disp"], t["gt_depth"], t["mask"], fb, 192), want, "540 x 960")
    # the aligned pitch of a padded prediction (test.py:208): rows from 4 of 544 x 992
    store = torch.full((1, 1, 544, 992), 7777.0, device=DEV)
    store[:, :, 4:, :960] = t["pred"]
    same(ops.result_images(store[:, :, 4:, :960], t["gt_disp"], t["gt_depth"], t["mask"], fb, 192), want, "540 x 960 of 544 x 992")
    # through the C entry point into sentinel-filled buffers: every byte and the flags are written, twice the same
    for fill in (0xA5, 0x5A):
        out = torch.full((1, 6, 540, 960, 4), fill, dtype=torch.uint8, device=DEV)
        flags = torch.full((1,), -12345, dtype=torch.int32, device=DEV)
        ops._call("az_result_images", out.data_ptr(), flags.data_ptr(), t["pred"].data_ptr(), 960, 540 * 960, t["gt_disp"].data_ptr(),
                  t["gt_depth"].data_ptr(), t["mask"].view(torch.uint8).data_ptr(), fb.data_ptr(), 192.0, 1.25, 3.0, 0.05, 1000.0, 1.0,
                  1, 540, 960, ops._stream())
        same(out, want, f"sentinel {fill:#x}")
        assert flags.tolist() == want_flags.tolist() == [0b11011]


def test_error_panels_are_k19s_colours():
    """K19's error_img on the same inputs, its float colours x 255: the shared table header did not drift"""
    for t in (full_size()[0], golden("batch3")[1]):
        got = render(t)
        disp = ei.disp_error_img_tensor(t["pred"], t["gt_disp"], t["mask"].view(torch.bool))  # [B,3,H,W]
        fb = (t["focal"] * t["baseline"]).cpu().numpy().reshape(-1, 1, 1, 1)
        with np.errstate(all="ignore"):
            pred_depth = dev(fb / t["pred"].cpu().numpy())  # one IEEE division, as numpy rounds it
        depth = ei.depth_error_img_tensor(pred_depth * 1000, t["gt_depth"] * 1000, t["mask"].view(torch.bool))
        for m, k19 in ((2, disp), (5, depth)):
            rgb = (k19 * 255).permute(0, 2, 3, 1)
            assert torch.equal(got[:, m, :, :, :3], rgb.to(torch.uint8)), ops.RESULT_PANELS[m]  # imsave's (c * 255).astype(uint8)
            assert bool((got[:, m, :, :, 3] == 255).all())


def test_refuses_what_it_cannot_read():
    d = torch.zeros(2, 1, 4, 6, device=DEV)
    fb = torch.ones(2, device=DEV)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.result_images(d, torch.zeros(2, 1, 4, 5, device=DEV), d, d > 0, fb, 192)
    with pytest.raises(RuntimeError, match="one value per batch element"):
        ops.result_images(d, d, d, d > 0, fb[:1], 192)
    with pytest.raises(RuntimeError, match="stride 1"):
        ops.result_images(torch.zeros(2, 1, 6, 4, device=DEV).transpose(2, 3), d, d, d > 0, fb, 192)
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):
        ops.result_images(d, d, d, d > 0, fb, 0.0)
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):
        ops.result_images(d[:, :, :1].expand(2, 1, 4, 6), d, d, d > 0, fb, 192)  # a row stride below W
