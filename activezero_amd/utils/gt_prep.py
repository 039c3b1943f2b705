"""The ground truth of a step, made on the GPU -- the lines of the reference's train.py:248-272 and test.py:91-110
around `apply_disparity_cu`: three (five) F.interpolate(mode="nearest") calls on the 2x-resolution maps, a float-to-int
cast, the scatter warp with its two synchronising sign checks, and the compares of the mask.  Here they are ONE launch of
the fused K18 kernel (az_gt_from_right, include/azhip.h): the full-resolution maps are read at the resized indices, no
resized or integer intermediate exists, and nothing synchronises.

An addition, not a shadow of a reference module.  Opt in inside train_sample (train.py) with

    from utils.gt_prep import prepare_sim_gt
    disp_gt_l, depth_gt, mask = prepare_sim_gt(sample, cfg.MODEL.MAX_DISP)

in place of train.py:248-249, 255-272, and in test.py with `prepare_test_gt(data)` in place of :82-85, 91-110 and
`prepare_test_mask(...)` (the fused K23 kernel, az_eval_mask) in place of the mask lines :112-117, 162-193, and
`img_L, img_R = prepare_test_images(img_L, img_R)` (the fused K26 kernel, az_test_images) in place of the bilinear resizes and
pads of the network's inputs, :118-131, 141-146.
"""
import torch

from activezero_amd import ops


def _tensors(sample_or_tensors, keys, device):
    """the named items of a sample dict, or the tensors themselves in that order, on the GPU"""
    if isinstance(sample_or_tensors, dict):
        ts = [sample_or_tensors[k] for k in keys]
    else:
        ts = list(sample_or_tensors)
        if len(ts) != len(keys):
            raise RuntimeError(f"expected {len(keys)} tensors ({', '.join(keys)}), got {len(ts)}")
    if device is None:
        device = next((t.device for t in ts if t.device.type == "cuda"), None) or torch.device("cuda")
    return [t.to(device).contiguous() for t in ts]  # a no-op for what a GPU loader already delivers


def prepare_sim_gt(sample_or_tensors, max_disp, device=None, check=False):
    """train.py:248-272: `sample` (keys img_disp_R, img_depth_L) or the pair (disp_r, depth_l), both [B,1,2H,2W] ->
    disp_gt_l [B,1,H,W] (the right view's disparity warped to the left view), depth_gt [B,1,H,W] (nearest resize) and
    mask [B,1,H,W] bool = (disp_gt_l < max_disp) * (disp_gt_l > 0).  A disparity <= -1 or not finite is counted on the
    device and lands nowhere; it raises AssertionError, as the reference's sign assertion would, only with check=True, which
    reads that counter (the one host sync; the reference's check costs two per step)."""
    disp_r, depth_l = _tensors(sample_or_tensors, ("img_disp_R", "img_depth_L"), device)
    disp_gt_l, _, depth_gt, mask, _ = ops.gt_from_right(disp_r, keep=depth_l, scale_factor=0.5, lo=0.0, hi=float(max_disp),
                                                        check=check)
    return disp_gt_l, depth_gt, mask


def prepare_test_gt(sample_or_tensors, size=(540, 960), device=None, check=False):
    """test.py:91-110: `data` (keys img_disp_R, img_depth_R, img_label) or the triple (disp_r, depth_r, label), each
    [B,1,Hin,Win] -> img_disp_l, img_depth_l [B,1,H,W] (right disparity and right depth warped to the left view by the one
    truncated disparity) and img_label [B,1,H,W] int32 (nearest resize, `.type(torch.int)`).  check=True: as in prepare_sim_gt."""
    disp_r, depth_r, label = _tensors(sample_or_tensors, ("img_disp_R", "img_depth_R", "img_label"), device)
    if label.dtype != torch.float32:  # (test.py interpolates the float label the loader delivers)
        label = label.to(torch.float32)
    img_disp_l, img_depth_l, label_s, _, _ = ops.gt_from_right(disp_r, extra=depth_r, keep=label, size=size, check=check)
    return img_disp_l, img_depth_l, label_s.type(torch.int)


def prepare_test_images(img_L, img_R, size=(540, 960), pad_to=(544, 960)):
    """test.py:118-131, 141-146: the two views of a test batch -> img_L, img_R [B,3,pad_to[0],pad_to[1]] float32, resized to
    `size` with F.interpolate(mode="bilinear", align_corners=False)'s arithmetic and padded at the top and on the right with
    zeros, in ONE launch of the fused K26 kernel (az_test_images) for both views.  Each view is [B,3,Hin,Win] float32 as the
    loader normalised it (data["img_real_L"], or data["img_sim_L"], which is already at `size` and is only padded), or
    [B,Hin,Win] uint8 grey levels, normalised on the way as the loader would have.  The results are the two halves of one
    tensor.  Nothing synchronises."""
    (h, w), (hp, wp) = (int(s) for s in size), (int(s) for s in pad_to)
    if hp < h or wp < w:
        raise RuntimeError(f"pad_to {(hp, wp)} is smaller than size {(h, w)}")
    device = next((t.device for t in (img_L, img_R) if t.device.type == "cuda"), None) or torch.device("cuda")
    img_L, img_R = img_L.to(device).contiguous(), img_R.to(device).contiguous()
    out = ops.test_images(img_L, img_R, size=(h, w), pad=(hp - h, wp - w))
    return out[:img_L.shape[0]], out[img_L.shape[0]:]


def prepare_test_mask(img_disp_l, img_depth_l, max_disp, exclude_bg=True, robot_mask=None, realsense_depth=None, depth_hi=1.25):
    """test.py:112-117, 162-193: the evaluation mask [B,1,H,W] bool of
        (img_disp_l < max_disp) * (img_disp_l > 0) * ((img_depth_l > 0) & (img_depth_l < 1.25))   (the last if exclude_bg)
        * (F.interpolate(robot_mask, (H, W), mode="nearest").type(torch.int) == 0)                 (LOSSES.ONREAL)
        * (F.interpolate(realsense_depth, (H, W), mode="nearest") > 0)                             (LOSSES.EXCLUDE_ZEROS)
    in ONE launch of the fused K23 kernel (az_eval_mask): robot_mask / realsense_depth are the loader's maps, [B,h,w] or
    [B,1,h,w] at their own size, float32 or float64, read in place in their own type; None leaves the term out.  Nothing
    synchronises."""
    mask, _ = ops.eval_mask(img_disp_l, img_depth_l, max_disp, exclude_bg, robot_mask, realsense_depth, depth_hi)
    return mask
