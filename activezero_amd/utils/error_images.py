"""Colour-coded error images on the GPU -- `disp_error_img` / `depth_error_img` of the reference's utils/util.py:185-244,
computed by the K19 kernel (az_error_img, include/azhip.h) instead of by eleven boolean-indexed numpy passes over host
copies of prediction, ground truth and mask.

Deliberately NOT named utils/util.py: that module also holds the reference's logger and TensorBoard writers, which must
stay the reference's.  Opt in with one line in train.py / test.py, after their own `from utils.util import ...`:

    from utils.error_images import disp_error_img, depth_error_img

The two drop-ins take the reference's arguments and return its [H,W,3] float32 numpy image of image 0 (one device-to-host
copy of the finished image).  train.py:353-356 converts that straight back into a [1,3,H,W] tensor; the `_tensor` variants
return [B,3,H,W] on the device for every image of the batch, with no host sync at all.
"""
from activezero_amd import ops


def _squeezed(est, gt, mask):
    """the reference's `.squeeze(0)` of its [1,B,H,W] / [B,1,H,W] arguments down to [B,H,W]"""
    out = []
    for t in (est, gt, mask):
        t = t.detach()
        while t.dim() > 3 and 1 in t.shape[:-2]:
            t = t.squeeze(list(t.shape[:-2]).index(1))
        if t.dim() == 2:
            t = t[None]
        out.append(t.contiguous())
    return out


def disp_error_img_tensor(D_est_tensor, D_gt_tensor, mask, abs_thres=3.0, rel_thres=0.05):
    est, gt, m = _squeezed(D_est_tensor, D_gt_tensor, mask)
    return ops.error_img(est, gt, m, "disp", abs_thres, rel_thres, channels_first=True)


def depth_error_img_tensor(D_est_tensor, D_gt_tensor, mask, abs_thres=1.0):
    est, gt, m = _squeezed(D_est_tensor, D_gt_tensor, mask)
    return ops.error_img(est, gt, m, "depth", abs_thres, channels_first=True)


def disp_error_img(D_est_tensor, D_gt_tensor, mask, abs_thres=3.0, rel_thres=0.05, dilate_radius=1):
    est, gt, m = _squeezed(D_est_tensor, D_gt_tensor, mask)
    return ops.error_img(est[:1], gt[:1], m[:1], "disp", abs_thres, rel_thres, channels_first=False)[0].cpu().numpy()


def depth_error_img(D_est_tensor, D_gt_tensor, mask, abs_thres=1.0, dilate_radius=1):
    est, gt, m = _squeezed(D_est_tensor, D_gt_tensor, mask)
    return ops.error_img(est[:1], gt[:1], m[:1], "depth", abs_thres, channels_first=False)[0].cpu().numpy()
