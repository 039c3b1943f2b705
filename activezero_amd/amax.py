"""Operand scales of the f16x3 arithmetic (include/azhip.h, az_roll_common.h): every operand of an f16x3 kernel is scaled
by a power of two taken from its largest finite magnitude, its "amax", a device array of AMAX_SLOTS floats.

This module owns how an amax gets to the launch that needs it:
  * activations and gradients carry it as an attribute, attached by the kernel that wrote them (BatchNorm apply /
    backward, residual sums, through a pre-zeroed array from ZEROS) and valid while the tensor's version counter stands
    (_set_amax / _get_amax); absmax() takes it with a pass of az_absmax when nobody attached one;
  * weights get theirs once per version -- once per optimizer step -- from the cache behind weight_amax(), which
    prime_weight_amax() fills for a whole model in one call of az_absmax_multi.
"""
import os
import threading

import numpy as np
import torch

from . import profiler
from ._lib import ABSMAX_DESC, CONST
from .ops import _call, _p, _stream

AMAX_SLOTS = CONST["AZ_AMAX_FLOATS"]  # floats of an "amax array" (include/azhip.h: 16 slots, 256 bytes apart)
_STRIDE = CONST["AZ_AMAX_STRIDE"]    # floats from one slot to the next


class _ZeroPool:
    """Pre-zeroed amax arrays for the kernels that take max |.| of what they write with atomicMax (BatchNorm apply,
    residual sums): one fill kernel per 256 arrays instead of a memset in front of every launch (measured:
    +0.1-0.16 ms per BatchNorm apply with the memset in the stream).  A slot is handed out once; the block lives as long
    as any of its slots."""

    def __init__(self):
        self.lock = threading.Lock()
        self.blocks = {}  # device index -> [tensor, next]

    def take(self, like):
        idx = like.device.index
        with self.lock:
            blk = self.blocks.get(idx)
            if blk is None or blk[1] + AMAX_SLOTS > blk[0].numel():
                blk = self.blocks[idx] = [torch.zeros(256 * AMAX_SLOTS, dtype=torch.float32, device=like.device), 0]
            i = blk[1]
            blk[1] = i + AMAX_SLOTS
            return blk[0][i:i + AMAX_SLOTS]


ZEROS = _ZeroPool()


def _set_amax(t, am):
    """attach the device scalar max |t| to the tensor object (valid while the tensor's version counter stands)"""
    t.az_amax = (am, t._version)


def _get_amax(t):
    a = getattr(t, "az_amax", None)
    return a[0] if (a is not None and a[1] == t._version) else None


# AZ_DEBUG_AMAX=1 (read once): every amax attached to a tensor is checked against a fresh pass of az_absmax when it is
# used (synchronises; include/azhip.h, "CONTRACT of a caller-supplied amax": too small = clipped operands)
_DEBUG_AMAX = os.environ.get("AZ_DEBUG_AMAX", "0") not in ("", "0")


def check_amax(t, am):
    """raise if the amax array `am` is below the largest finite magnitude of t (a stale attribute)"""
    fresh = t.new_empty(AMAX_SLOTS)
    _call("az_absmax", _p(fresh), _p(t), t.numel(), _stream())
    have, true = float(am[::_STRIDE].max()), float(fresh[::_STRIDE].max())  # (the slots of an amax array)
    if not have >= true:
        raise RuntimeError(f"stale amax: {have:.6g} attached to a tensor whose largest finite magnitude is {true:.6g} "
                           "(written through a raw pointer or .data without packing.touched / a fresh amax.absmax?)")


def absmax(t):
    """device scalar max |t| (largest finite magnitude), the operand scale of the f16x3 kernels: taken by the kernel that
    produced t where that is one of this library's (BatchNorm apply / backward, residual sums), by a pass of az_absmax
    otherwise"""
    am = _get_amax(t)
    if am is not None and _DEBUG_AMAX:
        check_amax(t, am)
    if am is None:
        am = t.new_empty(AMAX_SLOTS)
        with profiler.scope("absmax", bytes=4.0 * t.numel(), bound="hbm"):
            _call("az_absmax", _p(am), _p(t), t.numel(), _stream())
        _set_amax(t, am)
    return am


_W_AMAX = {}  # (data_ptr, version, device, numel) -> (amax array of a weight tensor, the tensor: its address stays its own)
_W_LOCK = threading.Lock()


def _w_key(w):
    return (w.data_ptr(), w._version, w.device.index, w.numel())


def remember_weight_amax(weight, am):
    """`am` is the amax array of `weight` at its current version"""
    with _W_LOCK:
        if len(_W_AMAX) > 512:
            _W_AMAX.clear()
        _W_AMAX[_w_key(weight)] = (am, weight)


def weight_amax(weight, w):
    """amax array of the weight tensor `weight` (w: its detached contiguous form), once per version: the forward pack of
    an optimizer step computes it, the input gradient's pack reuses it"""
    with _W_LOCK:
        hit = _W_AMAX.get(_w_key(weight))
    if hit is not None:
        return hit[0]
    am = absmax(w)
    remember_weight_amax(weight, am)
    return am


def absmax_tables(rows):
    """launch_tables (packing.py) of az_absmax_multi: one descriptor per tensor, dicts with src, amax, n"""
    from .packing import launch_tables
    return launch_tables(ABSMAX_DESC, rows, lambda r: r["n"])


class MultiAbsmax:
    """az_absmax_multi (include/azhip.h) for sets of tensors that come back step after step: the amax arrays of all of them
    in one call -- the largest FINITE magnitude of each, the bits az_absmax gives, where a max-norm of the tensor would be
    inf / NaN after one bad element and flush every finite weight to zero (az_common.h).  The device tables of a set are
    uploaded once (the only blocking copy) and found again by the addresses and lengths they describe, so they stay right
    for whatever tensor lives at those addresses; the caller keeps the amax arrays alive."""

    def __init__(self, limit=8):
        self.tables, self.limit = {}, limit

    def clear(self):
        self.tables.clear()

    def run(self, tensors, rows):
        """rows[i] (an amax array, any content) <- the amax array of tensors[i] (contiguous fp32 on one device)"""
        dev = tensors[0].device
        key = tuple((t.data_ptr(), t.numel(), r.data_ptr()) for t, r in zip(tensors, rows))
        tab = self.tables.get(key)
        if tab is None:
            descs, block_desc, first, nblocks = absmax_tables([dict(src=p, amax=a, n=n) for p, n, a in key])
            if len(self.tables) >= self.limit:
                self.tables.clear()
            tab = self.tables[key] = (torch.from_numpy(descs.view(np.uint8)).to(dev), torch.from_numpy(block_desc).to(dev),
                                      torch.from_numpy(first).to(dev), len(key), nblocks)
        descs, block_desc, first, nd, nblocks = tab
        with torch.cuda.device(dev), profiler.scope("absmax", bytes=4.0 * sum(k[1] for k in key), bound="hbm"):
            _call("az_absmax_multi", _p(descs), _p(block_desc), _p(first), nd, nblocks, _stream())


_PRIME = MultiAbsmax()
_PRIME_ROWS = {}  # (device index, ((data_ptr, numel), ...)) -> the [len, AMAX_SLOTS] arrays of that set of weights


def prime_weight_amax(weights):
    """The amax arrays of all given weight tensors in ONE call of az_absmax_multi instead of a memset + reduction per weight
    and step: fills the per-version cache that the f16x3 packers read.  Weights whose current version is already cached are
    skipped; called at the start of a forward pass.  A set of weights keeps its arrays from step to step (rewritten in
    stream order, as the rows of packing.PackPlan are), so that the call's device tables are uploaded once per set."""
    with _W_LOCK:
        todo = [w for w in weights if w is not None and w.is_cuda and w.dtype == torch.float32 and w.numel() > 0
                and _w_key(w) not in _W_AMAX]
        if not todo:
            return
        dets = [w.detach().contiguous() for w in todo]
        key = (dets[0].device.index, tuple((d.data_ptr(), d.numel()) for d in dets))
        arr = _PRIME_ROWS.get(key)
        if arr is None:
            if len(_PRIME_ROWS) >= _PRIME.limit:
                _PRIME_ROWS.clear()
                _PRIME.clear()
            arr = _PRIME_ROWS[key] = torch.empty(len(todo), AMAX_SLOTS, dtype=torch.float32, device=dets[0].device)
        _PRIME.run(dets, list(arr))
    for i, w in enumerate(todo):
        remember_weight_amax(w, arr[i])
