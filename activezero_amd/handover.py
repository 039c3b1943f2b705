"""Gradient hand-over between the consumers of one tensor: the input-gradient kernels add the other consumers'
contributions in their epilogue instead of leaving the sum to the autograd engine's pairwise adds.

This module owns the bookkeeping (GradSlot, slot_register in forward, slot_contribute / slot_leftover in backward) and
the one summing kernel launch behind it (sum_parts, az_sum4); the autograd nodes that use it are in conv3d.py.
"""
import os

import torch

from .ops import _call, _chk, _p, _stream

# A tensor with several consumers gets one gradient per consumer and the autograd engine adds them pairwise: 8 `add_` kernels
# over V0- / V1-sized tensors per step (1.8 ms on the main stream, tools/aten_sources.py).  Every input-gradient kernel can add
# a tensor in its epilogue, so the autograd nodes of conv3d.py do the sum themselves: each one that is NOT the last to run keeps
# its contribution in the tensor's GradSlot and returns None to the engine; the last one launches its input gradient with the
# kept contribution(s) as `residual` and returns the total.  Correct for any execution order; a contribution that is a plain
# tensor (the residual branch of a BatchNorm unit) is handed over the same way.  What the engine sees is a sum whose other terms
# are None.  Safety net for pruned graphs (a consumer that registered in forward and never runs in backward): the producing
# _ConvBN node adds whatever is still parked in its output's slot to the gradient it receives.
_HANDOVER = os.environ.get("AZ_GRAD_HANDOVER", "1") != "0"  # (read once) 0: every consumer returns its own gradient


class GradSlot:
    __slots__ = ("expect", "left", "parts")

    def __init__(self):
        self.expect, self.left, self.parts = 0, 0, []


def slot_register(t):
    """forward: one more consumer of t whose backward will call slot_contribute"""
    if not (_HANDOVER and torch.is_grad_enabled() and t.requires_grad):
        return None
    s = getattr(t, "az_gslot", None)
    if s is None:
        node = t.grad_fn
        # only tensors produced by a _ConvBN node: that node is the safety net (slot_leftover) for contributions parked by
        # consumers whose siblings the engine pruned; everything else keeps the engine's own accumulation
        if node is None or type(node).__name__ != "_ConvBNBackward":
            return None
        s = t.az_gslot = GradSlot()
        node.az_out_slot = s
    s.expect += 1
    s.left = s.expect
    return s


def sum_parts(parts):
    while len(parts) > 1:
        take, parts = parts[:4], parts[4:]
        take = [_chk(t.contiguous(), "grad") for t in take]
        if any(t.shape != take[0].shape for t in take):
            raise RuntimeError(f"sum_parts: shapes differ, {[tuple(t.shape) for t in take]}")
        out = torch.empty_like(take[0])  # (of the contiguous copy: az_sum4 writes linearly, a part may arrive in any format)
        ptrs = [_p(t) for t in take] + [None] * (4 - len(take))
        _call("az_sum4", _p(out), ptrs[0], ptrs[1], ptrs[2], ptrs[3], out.numel(), _stream())
        parts = [out] + parts
    return parts[0]


def slot_contribute(slot, make=None, plain=None):
    """backward of one consumer: `make(residual)` launches its input gradient with `residual` added in the epilogue, or `plain`
    is a gradient that already exists.  Returns what this consumer hands to the engine (None unless it is the last one)."""
    if slot is None or slot.expect < 2:
        return make(None) if make is not None else plain
    slot.left -= 1
    if slot.left > 0:
        slot.parts.append(make(None) if make is not None else plain)
        return None
    parts, slot.parts, slot.left = slot.parts, [], slot.expect
    res = sum_parts(parts) if parts else None
    if make is not None:
        return make(res)
    return plain if res is None else sum_parts([plain, res])


def slot_leftover(ctx, gy):
    """producer side: contributions parked in the output's slot by consumers whose siblings never ran (pruned graphs)"""
    slot = getattr(ctx, "az_out_slot", None)
    if slot is None or not slot.parts:
        return gy
    parts, slot.parts, slot.left = slot.parts, [], slot.expect
    return sum_parts([gy] + parts)
