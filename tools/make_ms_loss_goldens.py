"""Write tests/golden/g17_ms_loss.npz: the reference's own `dispnet_disp` and `default_disp` (utils/losses.py:17-32, 71-72),
imported from the reference tree and run on the CPU, the yardstick of K29 (az_ms_loss.hip, ops.multiscale_disp_loss).
Needs the reference tree (AZ_REFERENCE, default /root/reference) and no GPU; only data is written.

    python tools/make_ms_loss_goldens.py [--check]

utils/losses.py imports configs.config (yacs) and, through utils/reprojection.py, cupy / pynvrtc at module level; the two
functions read nothing from them, so inert stand-ins are put in their place, as tools/make_goldens.py does for G12-G14.

Keys.  dispnet_* -- (B,H,W) = (2,67,131), seven scales down to 1x2, every size odd somewhere: gt, mask (bool), pred0..pred6
(float32 inputs), loss32 (the reference in float32), loss64 / means64 [7] / grad64_0..6 (the reference on the inputs cast to
double: the loss, each scale's smooth_l1 mean, the gradients of the loss).  default_* -- (2,24,40) with G10's mask
construction (gt == 0 rows, a run beyond maxdisp = 64): gt, mask, pred0, loss32, loss64, means64 [1], grad64_0.
--check compares a fresh run with the committed file instead of writing it."""
import argparse
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
PATH = os.path.join(REPO, "tests", "golden", "g17_ms_loss.npz")
sys.path.insert(0, REPO)
from tests._weights import seeded  # noqa: E402

DISPNET_WEIGHTS = (1, 1, 1, 0.8, 0.6, 0.4, 0.2)  # utils/losses.py:19, for the per-scale means only


def reference_losses():
    """the reference's utils.losses with inert stand-ins for the packages its module-level imports name"""
    sys.path.insert(1, REF)
    for name in ("cupy", "cupy.cuda", "pynvrtc", "pynvrtc.compiler", "opt_einsum"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cupy.cuda"].function = types.SimpleNamespace(Module=object)
    sys.modules["pynvrtc.compiler"].Program = object
    if "configs.config" not in sys.modules:
        pkg, m = types.ModuleType("configs"), types.ModuleType("configs.config")
        pkg.__path__, m.cfg, pkg.config = [], types.SimpleNamespace(), m
        sys.modules["configs"], sys.modules["configs.config"] = pkg, m
    return importlib.import_module("utils.losses")


def evaluate(fn, preds, gt, mask, single):
    """fp32 loss, and in fp64 (inputs cast to double) the loss, the per-scale means and the gradients"""
    call = (lambda ps, g, m: fn(ps[0], g, m)) if single else fn
    out = {"loss32": call(preds, gt, mask).detach()}
    ps64 = [p.double().requires_grad_() for p in preds]
    loss = call(ps64, gt.double(), mask)
    grads = torch.autograd.grad(loss, ps64)
    out["loss64"] = loss.detach()
    # scale k's mean from the reference itself: its loop stops with the shorter list, so the first k + 1 predictions give
    # the first k + 1 terms (fp64: the difference of two partial sums is good to 1e-15)
    partial = [torch.zeros((), dtype=torch.float64)] + [call(ps64[:k + 1], gt.double(), mask).detach() for k in range(len(ps64))]
    weights = (1,) if single else DISPNET_WEIGHTS
    out["means64"] = torch.stack([(partial[k + 1] - partial[k]) / weights[k] for k in range(len(ps64))])
    for k, g in enumerate(grads):
        out[f"grad64_{k}"] = g
    return out


def arrays():
    losses = reference_losses()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # size_average= and uint8 indexing: deprecated, still what the reference calls
        # dispnet_disp
        b, h, w = 2, 67, 131
        gt = seeded((b, 1, h, w), 1701, 0.0, 60.0)
        gt[:, :, 5:10] = 0.0         # invalid rows (gt == 0); row 0 stays valid: the 1x2 scale reads nothing else
        gt[1, 0, 40:, 90:] = 70.0    # beyond maxdisp
        mask = (gt < 64.0) & (gt > 0)
        preds = [(gt[:, :, ::1 << k, ::1 << k][:, :, :h >> k, :w >> k] + seeded((b, 1, h >> k, w >> k), 1710 + k, -3.0, 3.0))
                 for k in range(7)]
        res = evaluate(losses.dispnet_disp, preds, gt, mask, single=False)
        out.update({"dispnet_gt": gt, "dispnet_mask": mask, **{f"dispnet_pred{k}": p for k, p in enumerate(preds)},
                    **{f"dispnet_{k}": v for k, v in res.items()}})
        # default_disp, G10's mask construction
        b, h, w = 2, 24, 40
        gt = seeded((b, 1, h, w), 1001, 0.0, 60.0)
        gt[:, :, :3] = 0.0
        gt[0, 0, 10, :5] = 70.0
        mask = (gt < 64.0) & (gt > 0)
        preds = [gt + seeded((b, 1, h, w), 1720, -3.0, 3.0)]
        res = evaluate(losses.default_disp, preds, gt, mask, single=True)
        out.update({"default_gt": gt, "default_mask": mask, "default_pred0": preds[0],
                    **{f"default_{k}": v for k, v in res.items()}})
    out = {k: v.detach().contiguous().numpy() for k, v in out.items()}
    out["torch_version"] = np.array(torch.__version__)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    new = arrays()
    if args.check:
        old = np.load(PATH)
        bad = [k for k in new if k != "torch_version" and not (k in old.files and np.array_equal(old[k], new[k], equal_nan=True))]
        print(f"torch {new['torch_version']} against the file written with {old['torch_version']}: "
              f"{len(bad)} of {len(new) - 1} arrays differ {bad}")
        return 1 if bad else 0
    np.savez_compressed(PATH, **new)
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes) with torch {new['torch_version']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
