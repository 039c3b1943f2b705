#!/usr/bin/env python3
"""train.py:220-432 (train_sample + train_sample_onreal) restated for the keys this path consumes, driven by
the synthetic MessytableDataset-shaped loader: DataLoader -> sim step (psmnet_disp + patch reprojection) ->
real step (patch reprojection), ADAPTER=False (3-channel PSMNet; the adapter is outside the path).  The
reference's own train.py imports yacs / tensorboardX / torchvision, none of which exist in this image, so
this script is the executable rehearsal of "drops into train.py": the same calls in the same order on the
same item dictionary.

    python tools/train_rehearsal.py --iters 4 --batch 2 [--augment]
--augment: the simulated images go through the reference's default augmentation (blur + colour jitter, K20)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activezero_amd.datasets.messytable_synthetic import SyntheticMessytableDataset  # noqa: E402
from activezero_amd.nets.psmnet.psmnet_3 import PSMNet  # noqa: E402
from activezero_amd.utils import disp_losses  # noqa: E402
from activezero_amd.utils.error_images import disp_error_img_tensor  # noqa: E402
from activezero_amd.utils.gt_prep import prepare_sim_gt  # noqa: E402
from activezero_amd.utils.reprojection import get_reproj_error_patch  # noqa: E402

MAX_DISP, PATCH = 192, 11  # configs/config.py:12, 41
IMG_OUTPUTS = {}  # the last step's train.py:357-363 images (what the TensorBoard writer would get)


def train_sample(sample, model, opt):
    """train.py:237-312 (sim) and :369-419 (real)"""
    model.train()
    img_L, img_R = sample["img_sim_L"], sample["img_sim_R"]
    disp_gt_l, _, mask = prepare_sim_gt(sample, MAX_DISP)                     # :248-272, one launch
    opt.zero_grad()
    out = model(img_L, img_R)
    sim_loss = disp_losses.psmnet_disp(out, disp_gt_l, mask)                  # losses.py:162-183
    reproj, _, _ = get_reproj_error_patch(sample["img_sim_L_reproj"], sample["img_sim_R_reproj"], out[0], mask, PATCH)
    sim_loss = sim_loss + reproj                                              # losses.py:95-97
    sim_loss.backward()
    opt.step()
    pred_disp = out[0].detach()
    IMG_OUTPUTS["disp_err"] = disp_error_img_tensor(pred_disp[[0]], disp_gt_l[[0]], mask[[0]])  # :353-356, no host copy
    opt.zero_grad()
    out = model(sample["img_real_L"], sample["img_real_R"])
    real_loss, _, _ = get_reproj_error_patch(sample["img_real_L_reproj"], sample["img_real_R_reproj"], out[0], None, PATCH)
    real_loss.backward()
    opt.step()
    return float(sim_loss.detach()), float(real_loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--augment", action="store_true", help="blur and colour-jitter the simulated images (dataset_utils.py:49-83)")
    ap.add_argument("--optimizer", choices=("torch", "fused"), default="torch",
                    help="fused: activezero_amd.optim.FusedAdam (K27 / K28) in place of torch.optim.Adam")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ds = SyntheticMessytableDataset(length=a.iters * a.batch, device=dev, augment=a.augment)
    loader = torch.utils.data.DataLoader(ds, batch_size=a.batch, shuffle=False, num_workers=0)
    torch.manual_seed(1)
    model = PSMNet(MAX_DISP).to(dev)
    if a.optimizer == "fused":
        from activezero_amd.optim import FusedAdam
        opt = FusedAdam(model.parameters(), lr=2e-4, betas=(0.9, 0.999))
    else:
        opt = torch.optim.Adam(model.parameters(), lr=2e-4, betas=(0.9, 0.999))
    for i, sample in enumerate(loader):
        s, r = train_sample(sample, model, opt)
        print(f"iter {i}: sim loss {s:.4f}  real reprojection loss {r:.5f}", flush=True)


if __name__ == "__main__":
    main()
