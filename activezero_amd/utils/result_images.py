"""The six result images of a test batch on the GPU -- test.py:235-272 of the reference with `save_img` of its
utils/test_util.py:59-107, rendered by the K24 kernel (az_result_images, include/azhip.h) instead of by six device-to-host
copies and six matplotlib passes per instance at batch size 1.  The batch leaves the GPU as finished RGBA bytes in one copy;
the host only compresses PNGs, with Pillow.  matplotlib is not needed at run time: the bytes are the ones its plt.imsave
writes (tests/golden/g16_result_images.npz, tools/make_result_image_goldens.py).

Deliberately NOT named utils/test_util.py: that module also holds the reference's GAN image writer and its figure code,
which must stay the reference's.  Opt in with one line in test.py, after its own `from utils.test_util import ...`:

    from utils.result_images import render_result_images, save_result_images

and replace test.py:235-272 by

    images = render_result_images(pred_disp, img_disp_l, img_depth_l, mask, img_focal_length, img_baseline, cfg.MODEL.MAX_DISP)
    save_result_images(log_dir, prefixes, images)
"""
import os

import numpy as np

from activezero_amd import ops

PANELS = ops.RESULT_PANELS  # save_img's directories, in its order


def render_result_images(pred_disp, img_disp_l, img_depth_l, mask, focal_length, baseline, max_disp, depth_hi=1.25):
    """test.py's tensors -> uint8 [B,6,H,W,4] on the device, panels in PANELS' order.  pred_disp [B,1,H,W], as cropped by
    test.py:208 (a view: it is not copied); img_disp_l, img_depth_l, mask [B,1,H,W]; focal_length, baseline [B,1,1,1] (or
    anything with B elements), multiplied in float32 exactly as test.py:209 multiplies them.  No host sync."""
    b = pred_disp.shape[0]
    fb = focal_length.detach().reshape(b) * baseline.detach().reshape(b)
    return ops.result_images(pred_disp.detach(), img_disp_l.detach().contiguous(), img_depth_l.detach().contiguous(),
                             mask.detach(), fb, max_disp, depth_hi=depth_hi)


def save_result_images(log_dir, prefixes, images):
    """Writes <log_dir>/<panel>/<prefix>.png for the six panels of every image: `images` uint8 [B,6,H,W,4] (a device tensor:
    ONE device-to-host copy of the whole batch; or a numpy array), `prefixes` one name per image (or one string when B is 1).
    The contract is the decoded pixels, not the PNG's metadata; missing directories are made.  Returns the paths."""
    from PIL import Image

    arr = images if isinstance(images, np.ndarray) else images.detach().cpu().numpy()
    if arr.dtype != np.uint8 or arr.ndim != 5 or arr.shape[1] != len(PANELS) or arr.shape[4] != 4:
        raise RuntimeError(f"images: expected uint8 [B,6,H,W,4], got {arr.dtype} {tuple(arr.shape)}")
    if isinstance(prefixes, str):
        prefixes = [prefixes]
    if len(prefixes) != arr.shape[0]:
        raise RuntimeError(f"{len(prefixes)} prefixes for {arr.shape[0]} images")
    paths = []
    for b, prefix in enumerate(prefixes):
        for m, panel in enumerate(PANELS):
            path = os.path.join(log_dir, panel, prefix) + ".png"
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(np.ascontiguousarray(arr[b, m])).save(path)  # [H,W,4] uint8: RGBA
            paths.append(path)
    return paths
