"""Operand scales of the f16x3 arithmetic (include/azhip.h, az_roll_common.h): every operand of an f16x3 kernel is scaled
by a power of two taken from its largest finite magnitude, its "amax", a device array of AMAX_SLOTS floats.

This module owns how an amax gets to the launch that needs it:
  * activations and gradients carry it as an attribute, attached by the kernel that wrote them (BatchNorm apply /
    backward, residual sums, through a pre-zeroed array from ZEROS) and valid while the tensor's version counter stands
    (_set_amax / _get_amax); absmax() takes it with a pass of az_absmax when nobody attached one;
  * weights get theirs once per version -- once per optimizer step -- from the cache behind weight_amax(), which
    prime_weight_amax() fills for a whole model in one call of az_absmax_multi; an entry answers only for the tensor it
    was taken from (Source: the record every address-keyed table of this library keeps of its sources).
"""
import os
import threading
import weakref

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


def debug_check(t, am):
    """AZ_DEBUG_AMAX=1: the memoised amax array `am` of the weight t still bounds it (a stale one: t was written through
    `.data` or a raw pointer without packing.touched)"""
    if _DEBUG_AMAX:
        check_amax(t, am)


def absmax(t):
    """device scalar max |t| (largest finite magnitude), the operand scale of the f16x3 kernels: taken by the kernel that
    produced t where that is one of this library's (BatchNorm apply / backward, residual sums), by a pass of az_absmax
    otherwise"""
    am = _get_amax(t)
    if am is not None and _DEBUG_AMAX:
        check_amax(t, am)
    if am is None:
        if not t.is_contiguous():  # (the kernel reads t.numel() floats from its pointer)
            raise RuntimeError("absmax: the tensor must be contiguous")
        am = t.new_empty(AMAX_SLOTS)
        with profiler.scope("absmax", bytes=4.0 * t.numel(), bound="hbm"):
            _call("az_absmax", _p(am), _p(t), t.numel(), _stream())
        _set_amax(t, am)
    return am


class Source:
    """What an address-keyed table of this library remembers of a tensor it made an entry from, so that the entry answers
    for that tensor alone.  A key of (address, version counter) cannot tell: `p.data = x`, module.to() / .cpu() / .cuda() /
    .float() and vector_to_parameters replace a parameter's storage WITHOUT moving its counter, the old block is freed, and
    another tensor -- or the same parameter, two assignments later -- can stand at the old address with the old counter.
      * the storage the entry was made from is pinned (a detached alias): while the entry lives the allocator cannot hand
        that address to anybody else;
      * the tensor itself is kept (weak = True: by weak reference), and a hit is verified (answers): the caller's tensor
        must lie at the recorded address in the pinned storage, and be the recorded tensor -- which must not have left --
        or an alias of the same shape whose counter stands where the recorded tensor's does (a detached alias or the
        gated alias of a training pass: they share the counter).
    What this cannot see is a write through `.data` or a raw pointer into storage that stays where it is: after one,
    call packing.touched(*tensors)."""
    __slots__ = ("_src", "pin", "ptr", "store", "weak")

    def __init__(self, t, weak=False):
        self.weak = weak
        base = t._base  # (a whole-tensor view -- the gated alias of a training pass -- stands for the tensor it views:
        if base is not None and base.data_ptr() == t.data_ptr() and base.shape == t.shape and base.stride() == t.stride():
            t = base    # the alias would stay behind in the old storage when the parameter's is replaced)
        self._src = weakref.ref(t) if weak else t
        self.pin = t.detach()
        self.ptr, self.store = t.data_ptr(), t.untyped_storage()._cdata

    def stands(self):
        """the recorded tensor, if it is alive and still where it was; None otherwise"""
        src = self._src() if self.weak else self._src
        if src is None or src.data_ptr() != self.ptr or src.untyped_storage()._cdata != self.store:
            return None
        return src

    __call__ = stands  # (where a weak reference stood before: "dead" now includes "has left its address")

    def answers(self, t):
        if t is None or t.data_ptr() != self.ptr or t.untyped_storage()._cdata != self.store:
            return False
        src = self.stands()
        if src is None:
            return False
        return src is t or (src._version == t._version and src.shape == t.shape and src.stride() == t.stride())


def sources(tensors):
    return tuple(Source(t) if t is not None else None for t in tensors)


def same_sources(srcs, tensors):
    """every entry of `srcs` (sources(...) at the time of the entry) answers for the tensor at its place"""
    return len(srcs) == len(tensors) and all((t is None) if s is None else s.answers(t) for s, t in zip(srcs, tensors))


_W_AMAX = {}  # (data_ptr, version, device, numel) -> (amax array of a weight tensor, the Source it was taken from)
_W_LOCK = threading.Lock()


def _w_key(w):
    return (w.data_ptr(), w._version, w.device.index, w.numel())


def remember_weight_amax(weight, am):
    """`am` is the amax array of `weight` at its current version"""
    with _W_LOCK:
        if len(_W_AMAX) > 512:
            _W_AMAX.clear()
        _W_AMAX[_w_key(weight)] = (am, Source(weight))


def _remembered(weight):
    """the cached amax array of `weight`, None when there is none or the entry under its key was taken from another tensor
    (call with _W_LOCK held)"""
    hit = _W_AMAX.get(_w_key(weight))
    return hit[0] if (hit is not None and hit[1].answers(weight)) else None


def weight_amax(weight, w):
    """amax array of the weight tensor `weight` (w: its detached contiguous form), once per version: the forward pack of
    an optimizer step computes it, the input gradient's pack reuses it"""
    with _W_LOCK:
        am = _remembered(weight)
    if am is not None:
        debug_check(w, am)
        return am
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
# (rows are found by address alone, which is safe because nobody is ANSWERED from them by address: every call rewrites all
#  rows of its set from the tensors that stand there now, and a row reaches a launch only through _W_AMAX's verified hit)


def prime_weight_amax(weights):
    """The amax arrays of all given weight tensors in ONE call of az_absmax_multi instead of a memset + reduction per weight
    and step: fills the per-version cache that the f16x3 packers read.  Weights whose current version is already cached are
    skipped; called at the start of a forward pass.  A set of weights keeps its arrays from step to step (rewritten in
    stream order, as the rows of packing.PackPlan are), so that the call's device tables are uploaded once per set."""
    with _W_LOCK:
        todo = [w for w in weights if w is not None and w.is_cuda and w.dtype == torch.float32 and w.numel() > 0
                and _remembered(w) is None]
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
