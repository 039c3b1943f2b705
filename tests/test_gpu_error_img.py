"""GPU: the error colour images (K19, az_error_img) against the numpy restatement of tests/_gt_prep_ref.py.  The kernel
evaluates the same float32 operations with IEEE division, then compares and selects: every output must be EQUAL
(np.array_equal), no tolerance.  Inputs: ref.error_case -- all eleven classes, pixels exactly on the ten inner bounds,
gt = 0 with and without an error, est = gt, NaN / inf predictions, a NaN and a negative ground truth, the mask off on about
a fifth of the image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.utils import error_images as ei  # noqa: E402
from tests import _gt_prep_ref as ref  # noqa: E402

DEV = "cuda:0"
SIZES = [(1, 12, 230), (3, 12, 230), (1, 12, 150), (3, 12, 150), (1, 7, 33), (3, 7, 33), (1, 1, 1), (1, 540, 960)]
_cache = {}


def case(kind, b, h, w):
    """inputs on the device and the restatement's image, computed once per (kind, size)"""
    key = (kind, b, h, w)
    if key not in _cache:
        est, gt, mask = ref.error_case(b * 1000 + h, b, h, w, kind)
        want = ref.error_img(est, gt, mask, kind)
        want.setflags(write=False)
        _cache[key] = (torch.tensor(est, device=DEV), torch.tensor(gt, device=DEV), torch.tensor(mask, device=DEV), want)
    return _cache[key]


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    diff = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"{what}: {want.shape}, {diff} components differ")
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32)), f"{what}: {diff} components differ"


@pytest.mark.parametrize("bhw", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["disp", "depth"])
def test_both_layouts_equal_the_restatement(kind, bhw):
    est, gt, mask, want = case(kind, *bhw)
    same(ops.error_img(est, gt, mask, kind, channels_first=False), want, f"{kind} [B,H,W,3]")
    same(ops.error_img(est, gt, mask, kind, channels_first=True), np.ascontiguousarray(want.transpose(0, 3, 1, 2)), f"{kind} [B,3,H,W]")
    if bhw[1] > 10:  # below the legend the image is not one colour: classes and black both occur
        body = want[:, 10:].reshape(-1, 3)
        assert len(np.unique(body, axis=0)) == 11


def test_mask_forms_thresholds_and_sentinel():
    est, gt, mask, _ = case("disp", 3, 12, 230)
    est_n, gt_n, mask_n = est.cpu().numpy(), gt.cpu().numpy(), mask.cpu().numpy()
    want = ref.error_img(est_n, gt_n, mask_n, "disp", abs_thres=2.0, rel_thres=0.1)
    same(ops.error_img(est, gt, mask.view(torch.uint8), "disp", 2.0, 0.1, channels_first=False), want, "uint8 mask, other thresholds")
    want = ref.error_img(est_n, gt_n, mask_n, "depth", abs_thres=0.5)
    same(ops.error_img(est[:, None], gt[:, None], mask[:, None], "depth", 0.5, channels_first=False), want, "[B,1,H,W] arguments")
    # the output is fully written: a sentinel-filled buffer through the C entry point
    out = torch.full((3, 12, 230, 3), 12345.0, device=DEV)
    ops._call("az_error_img", out.data_ptr(), est.data_ptr(), gt.data_ptr(), mask.view(torch.uint8).data_ptr(), 0, 3.0, 0.05, 0,
              3, 12, 230, ops._stream())
    same(out, ref.error_img(est_n, gt_n, mask_n, "disp"), "sentinel-filled output")


@pytest.mark.parametrize("hw", [(12, 230), (12, 150), (7, 33)])
def test_drop_in_functions_and_tensor_variants(hw):
    for kind, drop_in, tensor in (("disp", ei.disp_error_img, ei.disp_error_img_tensor),
                                  ("depth", ei.depth_error_img, ei.depth_error_img_tensor)):
        est, gt, mask, want = case(kind, 3, *hw)
        # as train.py:353 calls it: [1,1,H,W] slices of image 0 -> the [H,W,3] float32 numpy image
        img = drop_in(est[[0]][:, None], gt[[0]][:, None], mask[[0]][:, None])
        assert isinstance(img, np.ndarray) and img.dtype == np.float32 and img.shape == hw + (3,)
        assert np.array_equal(img.view(np.int32), want[0].view(np.int32))
        # the reference's own calling convention, [1,B,H,W], returns image 0 as well
        assert np.array_equal(drop_in(est[None], gt[None], mask[None]), want[0])
        t = tensor(est[:, None], gt[:, None], mask[:, None])
        assert t.is_cuda and t.shape == (3, 3) + hw
        same(t, np.ascontiguousarray(want.transpose(0, 3, 1, 2)), f"{kind} tensor variant")
        # train.py:354-356 on the drop-in's result is image 0 of the tensor variant
        assert np.array_equal(np.ascontiguousarray(img[None].transpose([0, 3, 1, 2])), t[:1].cpu().numpy())
