#!/usr/bin/env python3
"""End-to-end training-dynamics check: N Adam steps of the bench workload (small size) on the HIP
path and on stock PyTorch-ROCm modules (3-D aggregation on MIOpen, extractor as plain modules),
same seed, same data.  Prints both loss curves; they must track each other (single-step parity is
what tests/ pin; this looks at the compounded effect of forward + backward + optimizer).

    --optimizer fused
compares, on the HIP path alone, the run under activezero_amd.optim.FusedAdam (K27 / K28) with the same run under
torch.optim.Adam: recorded, not gated -- Adam's sign-like first step amplifies last-bit differences."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def run(backend, steps, b, h, w, md, optimizer="torch"):
    from activezero_amd.nets.psmnet.psmnet_3 import PSMNet
    from tools import eager_psmnet

    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    model = PSMNet(md).to(dev).train()
    if optimizer == "fused":
        from activezero_amd.optim import FusedAdam
        opt = FusedAdam(model.parameters(), lr=2e-4, betas=(0.9, 0.999))
    else:
        opt = torch.optim.Adam(model.parameters(), lr=2e-4, betas=(0.9, 0.999))
    il, ir, gt = bench.synth_batch(b, h, w, md, dev, 1234)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        if backend == "hip":
            loss = bench.disp_loss(model(il, ir), gt, md)
        else:  # stock PyTorch-ROCm operators over the same module's parameters
            loss = eager_psmnet.eager_loss(eager_psmnet.eager_forward(model, il, ir), gt, md)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--optimizer", choices=("torch", "fused"), default="torch")
    a = ap.parse_args()
    if a.optimizer == "fused":
        hip = run("hip", a.steps, a.batch, a.height, a.width, a.maxdisp, "fused")
        ref = run("hip", a.steps, a.batch, a.height, a.width, a.maxdisp)
        names = ("FusedAdam", "torch.optim.Adam")
    else:
        hip = run("hip", a.steps, a.batch, a.height, a.width, a.maxdisp)
        ref = run("miopen", a.steps, a.batch, a.height, a.width, a.maxdisp)
        names = ("hip", "torch-rocm")
    worst = 0.0
    for i, (x, y) in enumerate(zip(hip, ref)):
        rel = abs(x - y) / max(abs(y), 1e-12)
        worst = max(worst, rel)
        print(f"step {i:3d}  {names[0]} {x:.6f}  {names[1]} {y:.6f}  rel diff {rel:.2e}")
    print(f"worst relative loss difference over {a.steps} steps: {worst:.2e}")
