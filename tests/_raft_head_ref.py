"""Plain-torch checker of the RAFT-Stereo prediction head (K15 convex upsampling, K16 sequence loss), written
from the formulas of include/azhip.h -- evaluated in fp64 (the yardstick) and fp32 (how far an fp32 evaluation
may sit from it) on the CPU; differentiable through autograd.  tests/golden/g14_raft_head.npz pins it to the
reference (tests/test_raft_head_cpu.py)."""
import torch

from tests._weights import seeded


def convex_upsample(flow, mask, factor, channels=None, negate=False):
    """up[n,d,y f+i,x f+j] = sum_k softmax_k(mask[n, k f f + i f + j, y, x]) * f * flow[n,d,y+ky-1,x+kx-1], k = 3 ky + kx,
    zero outside the map.  flow [N,D,h,w], mask [N,9 f f,h,w], both of flow's dtype."""
    n, d, h, w = flow.shape
    f = factor
    d_out = d if channels is None else channels
    p = torch.softmax(mask.reshape(n, 9, f, f, h, w), dim=1)
    padded = torch.zeros(n, d_out, h + 2, w + 2, dtype=flow.dtype, device=flow.device)
    padded[:, :, 1:-1, 1:-1] = f * flow[:, :d_out]
    up = torch.zeros(n, d_out, f, f, h, w, dtype=flow.dtype, device=flow.device)
    for ky in range(3):
        for kx in range(3):
            up = up + p[:, None, 3 * ky + kx] * padded[:, :, None, None, ky:ky + h, kx:kx + w]
    # [n, d, i, j, y, x] -> [n, d, y, i, x, j]
    up = up.permute(0, 1, 4, 2, 5, 3).reshape(n, d_out, f * h, f * w)
    return -up if negate else up


def sequence_weights(n, loss_gamma=0.9):
    g = loss_gamma ** (15.0 / (n - 1)) if n > 1 else 1.0  # n = 1: weight 1 (the reference divides by zero)
    return [g ** (n - 1 - i) for i in range(n)]


def sequence_loss(flow_preds, flow_gt, valid, loss_gamma=0.9, max_flow=700, disparity=False):
    """sum_i w_i * mean over {valid >= 0.5 and |gt| < max_flow} of |pred_i - t|, t = -gt (t = gt for disparities)"""
    target = flow_gt if disparity else -flow_gt
    ok = (valid >= 0.5) & (flow_gt.abs() < max_flow)
    count = ok.sum()
    loss = 0.0
    for w, pred in zip(sequence_weights(len(flow_preds), loss_gamma), flow_preds):
        err = (pred - target).abs()
        loss = loss + w * torch.where(ok, err, torch.zeros_like(err)).sum() / count
    return loss


def make_mask_logits(shape, seed):
    """[N,C,h,w] logits scaled per pixel so that some pixels are near one-hot and some near uniform"""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    scale = torch.rand(n, 1, h, w, generator=g, dtype=torch.float64)
    scale = torch.where(scale < 0.25, 0.05, torch.where(scale > 0.75, 12.0, 2.0)).to(torch.float64)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


def g14_upsample_inputs(g, tag):
    """the inputs tools/make_goldens.py g14_raft_head() made case `tag` from: factor, flow, mask logits, cotangent"""
    f, n, d, h, w, sd, zero_y = (int(v) for v in g[f"{tag}_meta"])
    flow = seeded((n, d, h, w), sd, -3.0, 3.0)
    if zero_y:
        flow[:, 1] = 0.0
    mask = make_mask_logits((n, 9 * f * f, h, w), sd + 1)
    cot = seeded((n, d, f * h, f * w), sd + 2)
    return f, flow, mask, cot


def g14_sequence_inputs(g, n_pred):
    """predictions, ground truth and validity map of the golden's sequence-loss cases"""
    shape, sd = (2, 1, 36, 52), int(g["seeds"][2])
    gt = seeded(shape, sd, -40.0, 820.0)
    valid = (seeded(shape, sd + 1, 0.0, 1.0) > 0.1).float()
    valid[:, :, 5:17, 20:41] = 0.0
    preds = [-gt + seeded(shape, sd + 10 + i, -3.0, 3.0) * (1.0 + 0.2 * (n_pred - i)) for i in range(n_pred)]
    return preds, gt, valid
