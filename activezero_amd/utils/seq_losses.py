"""Sequence loss -- replacement for `sequence_loss` of the reference's utils/losses.py:34-69, computed by the
fused K16 kernel (az_seq_loss_{fwd,bwd}): one autograd node for the whole list of predictions, no
boolean-index compaction and no host sync.

Deliberately NOT named utils/losses.py, for the reason given in utils/disp_losses.py.  Integration is one line
there, after the reference's own definition: `from utils.seq_losses import sequence_loss`.
"""
from activezero_amd import ops


def sequence_loss(flow_preds, flow_gt, valid, loss_gamma=0.9, max_flow=700):
    """sum_i gamma'^(n-1-i) * mean_valid |flow_preds[i] + flow_gt|, gamma' = loss_gamma^(15/(n-1)); a pixel is
    valid when valid >= 0.5 and |flow_gt| < max_flow.  The reference's NaN / inf assertions would each cost a
    host sync: call activezero_amd.ops.sequence_loss(..., check=True) to have them.  n = 1 (a division by zero
    in the reference) gives the single prediction weight 1."""
    return ops.sequence_loss(flow_preds, flow_gt, valid, loss_gamma, max_flow)
