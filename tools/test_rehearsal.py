#!/usr/bin/env python3
"""test.py:69-311 restated for the keys this path consumes, driven by the synthetic test-mode loader
(datasets/messytable_test_synthetic.py): DataLoader -> ground truth from the right view (K18) -> the network's padded inputs
(K26) -> evaluation mask (K23) -> eval forward of the 3-channel PSMNet (ADAPTER=False) -> error metrics and per-object
errors of every image (K22) -> the six result images (K24), written as PNGs -- at ANY batch size, where the reference runs
one instance at a time.  The reference's own test.py imports yacs and cv2, neither of which exists in this image, so this
script is the executable rehearsal of "drops into test.py": the same calls in the same order on the same item dictionary.

    python tools/test_rehearsal.py --instances 4 --batch 2 --out test_rehearsal_out [--levels] [--small]
--levels: the real views go to the network from their uint8 grey levels (K26's device-loader form), not from the float images.
--small: 252 x 256 items padded to 256 x 256 and 32 disparities instead of test.py's 540 x 960 -> 544 x 960 and 192.
The averaged metrics and the object table are printed and written to <out>/metrics.json."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activezero_amd.datasets.messytable_test_synthetic import SyntheticMessytableTestDataset  # noqa: E402
from activezero_amd.nets.psmnet.psmnet_3 import PSMNet  # noqa: E402
from activezero_amd.utils.cascade_metrics import compute_err_metric_per_image, compute_obj_err_per_image  # noqa: E402
from activezero_amd.utils.gt_prep import prepare_test_gt, prepare_test_images, prepare_test_mask  # noqa: E402
from activezero_amd.utils.result_images import render_result_images, save_result_images  # noqa: E402

MAX_DISP, OBJ_NUM = 192, 18                      # configs/config.py:8, 56
SIZE, PAD_TO, REAL_SIZE = (540, 960), (544, 960), (720, 1280)  # test.py:91-131, configs/config.py:80-81


def evaluate_batch(data, model, max_disp=MAX_DISP, size=SIZE, pad_to=PAD_TO, obj_num=OBJ_NUM, levels=False):
    """test.py:73-260 for one batch of LOSSES.ONREAL, EXCLUDE_BG, EXCLUDE_ZEROS items (the defaults).  Returns what the
    rest of the loop needs: pred_disp (the crop, a view), the ground truth, the mask, the metrics per image (a list of
    dicts), the four per-object arrays summed over the images as test.py:230-233 sums them, and the rendered images."""
    img_disp_l, img_depth_l, img_label = prepare_test_gt(data, size)                       # :82-110, one launch
    views = ("img_real_L_levels", "img_real_R_levels") if levels else ("img_real_L", "img_real_R")
    img_L, img_R = prepare_test_images(data[views[0]], data[views[1]], size, pad_to)       # :118-146, one launch
    mask = prepare_test_mask(img_disp_l, img_depth_l, max_disp, True, data["robot_mask"],
                             data["img_depth_real_realsense"])                             # :112-117, 162-193, one launch
    model.eval()
    with torch.no_grad():
        pred = model(img_L, img_R)                                                          # :206
    top_pad, right_pad = pad_to[0] - size[0], pad_to[1] - size[1]
    pred_disp = pred[:, :, top_pad:, :] if right_pad == 0 else pred[:, :, top_pad:, :-right_pad]  # :208
    focal_length, baseline = data["focal_length"].to(pred.device), data["baseline"].to(pred.device)
    err_metrics = compute_err_metric_per_image(img_disp_l, img_depth_l, pred_disp, focal_length, baseline, mask)  # :212
    obj_err = compute_obj_err_per_image(img_disp_l, img_depth_l, pred_disp, focal_length, baseline, img_label, mask,
                                        obj_num)                                            # :220-233
    images = render_result_images(pred_disp, img_disp_l, img_depth_l, mask, focal_length, baseline, max_disp)  # :235-260
    return {"pred_disp": pred_disp, "img_L": img_L, "img_R": img_R, "img_disp_l": img_disp_l, "img_depth_l": img_depth_l,
            "img_label": img_label, "mask": mask, "err_metrics": err_metrics, "obj_err": obj_err, "images": images}


def _jsonable(v):
    """NaN (an object no instance shows, or one that is fully masked) has no JSON spelling: null"""
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_jsonable(x) for x in v]
    if isinstance(v, str):
        return v
    v = float(v)
    return v if math.isfinite(v) else None


def run(loader, model, log_dir, max_disp=MAX_DISP, size=SIZE, pad_to=PAD_TO, obj_num=OBJ_NUM, levels=False, on_batch=None):
    """the loop of test.py:73-285 over `loader`; returns the summary it also writes to <log_dir>/metrics.json.
    on_batch(data, out): called with every batch and what evaluate_batch made of it"""
    total_err = None
    total_obj = tuple(np.zeros(obj_num) for _ in range(4))
    per_instance = []
    for data in loader:
        out = evaluate_batch(data, model, max_disp, size, pad_to, obj_num, levels)
        if on_batch is not None:
            on_batch(data, out)
        for prefix, err in zip(data["prefix"], out["err_metrics"]):
            total_err = dict(err) if total_err is None else {k: total_err[k] + err[k] for k in err}  # :215-216
            per_instance.append({"prefix": prefix, **err})
        for total, part in zip(total_obj, out["obj_err"]):
            total += part
        save_result_images(log_dir, list(data["prefix"]), out["images"])                    # :263-272, one copy per batch
    n = len(per_instance)
    disp_err, depth_err, depth_4_err, count = total_obj
    with np.errstate(invalid="ignore", divide="ignore"):                                    # :280-282 (0 / 0 for an absent object)
        objects = {"disp_err": disp_err / count, "depth_err": depth_err / count, "depth_4_err": depth_4_err / count,
                   "count": count}
    summary = _jsonable({"instances": n, "metrics": {k: v / n for k, v in total_err.items()}, "objects": objects,
                         "per_instance": per_instance})
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "metrics.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out", default="test_rehearsal_out")
    ap.add_argument("--levels", action="store_true", help="feed the real views as uint8 grey levels")
    ap.add_argument("--small", action="store_true", help="252 x 256 items, 32 disparities")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    size, pad_to, real_size, max_disp = ((252, 256), (256, 256), (336, 342), 32) if a.small else (SIZE, PAD_TO, REAL_SIZE, MAX_DISP)
    ds = SyntheticMessytableTestDataset(length=a.instances, height=size[0], width=size[1], real_size=real_size, device=dev,
                                        max_disp=max_disp)
    loader = torch.utils.data.DataLoader(ds, batch_size=a.batch, shuffle=False, num_workers=0)
    torch.manual_seed(1)
    model = PSMNet(max_disp).to(dev)
    summary = run(loader, model, a.out, max_disp, size, pad_to, levels=a.levels)
    print(json.dumps({k: summary[k] for k in ("instances", "metrics", "objects")}))


if __name__ == "__main__":
    main()
