"""RAFT-Stereo's convex upsampling -- replacement for `RAFTStereo.upsample_flow` of the reference's
nets/raft/raft_stereo.py:74-86, computed by the fused K15 kernel (az_convex_up_{fwd,bwd}): the mask is read
once, nothing of its size is materialised or saved for backward.

The reference method reads the factor from the yacs config; here it is an argument, so binding it is one line
after the class in nets/raft/raft_stereo.py:
`RAFTStereo.upsample_flow = lambda self, flow, mask: upsample_flow(flow, mask, 2 ** cfg.MODEL.N_DOWNSAMPLE)`
"""
from activezero_amd import ops


def upsample_flow(flow, mask, factor):
    """[N,D,h,w] flow, [N,9*factor^2,h,w] mask (fp32, or fp16 as the mask head emits under autocast) ->
    [N,D,factor*h,factor*w]: every channel, as the reference method returns them."""
    return ops.convex_upsample(flow.float(), mask, factor)


def upsample_disparity(flow, mask, factor):
    """The `flow_up[:, :1]` of raft_stereo.py:189 folded in: only the x channel is computed -> [N,1,factor*h,factor*w].
    (Still a flow, i.e. minus the disparity; utils.seq_losses.sequence_loss takes it as the reference's does.)"""
    return ops.convex_upsample(flow.float(), mask, factor, channels=1)
