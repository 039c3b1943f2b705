"""Weight images: the memo of packed weights between no_grad forwards and the per-step pack plan of the f16x3 kernels.

The kernels read weights from packed images, not from PyTorch's layouts.  This module owns how an image is reused:
  * memo(): the inference-time memo the packers of conv3d.py, conv2d.py and nets/raft/gru.py go through, with the key
    rule (cache_key), the lock and touched(), which tells the version counters in those keys about raw-pointer writes;
  * PackPlan / prepack / planned_pack: during training, every f16x3 image of a model's parameters in one launch per
    optimizer step, into persistent buffers.
"""
import os
import threading

import numpy as np
import torch

from . import amax
from ._lib import CONST, PACK_DESC
from .amax import AMAX_SLOTS
from .ops import _call, _p, _stream

# Inference-time memo of packed weights and folded BatchNorm affine maps (pure functions of parameters
# that do not change between no_grad forwards).  Whether a call may use it is decided by the CALLER
# (`cache=` = "autograd is off at the call site", conv3d.conv_bn / conv2d.conv_bn_eval), never inside an autograd
# Function.  Keys hold the tensors' storage address AND version counter, so an optimizer step or a
# load_state_dict (both write in place) invalidates them; a BatchNorm's key also holds
# num_batches_tracked, because this library's own train kernels update running_mean / running_var
# through raw pointers and then bump the counters themselves (touched()).
# What a key does NOT say is whose (address, counter) it is: `p.data = t`, module.to() / .cpu() / .cuda() / .float()
# and vector_to_parameters replace a parameter's storage without moving its counter, and another tensor with an
# equal counter -- or the same parameter, later -- can stand at the old address.  So each entry records its sources
# (amax.Source): the storage it was packed from stays pinned while the entry lives, and every hit is verified --
# the recorded tensor must still stand where it was packed, and the caller's tensor must be it or an alias of it
# (detached, or the gated alias of a training pass).  What nothing here can see is a write through `.data` or a raw
# pointer into storage that stays where it is: after one, call touched(*tensors).
# A lock makes the dicts safe under the threads of nn.DataParallel (train.py:540-541).
PACK_CACHE, AFFINE_CACHE = {}, {}
CACHE_LOCK = threading.Lock()


def cache_key(*tensors):
    return tuple((t.data_ptr(), t._version, t.device.index) for t in tensors if t is not None)


Source, sources, same_sources = amax.Source, amax.sources, amax.same_sources  # (the rule of every address-keyed table, stated once)


def cache_get(cache, key):
    with CACHE_LOCK:
        return cache.get(key)


def cache_put(cache, key, value, limit):
    with CACHE_LOCK:
        if len(cache) > limit:
            cache.clear()
        cache[key] = value


def memo(cache, key, make, keep, limit):
    """make()'s value, remembered in `cache` under `key` (None: not memoised, the call site has autograd on) together with
    the source tensors `keep` the key was taken from; a hit answers only for those tensors (same_sources); a cache that has
    grown past `limit` entries is emptied"""
    if key is None:
        return make()
    keep = tuple(keep)
    hit = cache_get(cache, key)
    if hit is not None and same_sources(hit[1], keep):
        return hit[0]
    value = make()
    cache_put(cache, key, (value, sources(keep)), limit)
    return value


def touched(*tensors):
    """Bump the version counters of buffers a kernel has just written through their raw pointers (BatchNorm
    running statistics and call counter): the memoised inference operands are keyed on them."""
    torch.autograd.graph.increment_version([t for t in tensors if t is not None])  # (one call for all of them)


# ---- pack plan (round 5): every f16x3 weight image of a model in ONE launch per optimizer step ----------------------------
# A training step used to pack each convolution weight twice (forward image, flipped / swapped input-gradient image), one
# launch and one allocation each: ~175 launches of ~4 us per step on the main stream.  The plan remembers, per device, which
# images the registered parameters were asked for (recorded by the first step's per-call packs), keeps ONE persistent buffer
# per image and a descriptor table on the device, and `prepack` rewrites all of them with az_pack_f16_multi when the
# parameters' version counters have moved.  _pack_f16 (conv3d.py, conv2d.py) then returns the plan's buffer.
#   * persistent buffers are safe in stream order: only main-stream kernels (forward, input gradient) read packed images,
#     and the next step's prepack is enqueued behind them on the same stream;
#   * only tensors registered through prepack() -- live nn.Parameters, held by weak reference -- have entries: derived
#     weights (the merged kernels of K3', DataParallel replicas) change address every step and keep the per-call route;
#   * an entry is valid for one (address, version counter): optimizer steps and load_state_dict write in place and bump it;
#   * an address belongs to the registered parameter only while that parameter stands there: once its storage has been
#     replaced (`p.data = t`, module.to(), vector_to_parameters) the plan answers for nobody at the old address, and the
#     next prepack drops what it held for it.
PACK_2D_SAME, PACK_2D_ROLL, PACK_3D_GATHER, PACK_3D_ROLL, PACK_3D_ROLL2 = (
    CONST["AZ_PACK_" + k] for k in ("2D_SAME", "2D_ROLL", "3D_GATHER", "3D_ROLL", "3D_ROLL2"))
_PLAN_ON = os.environ.get("AZ_PACK_PLAN", "1") != "0"  # (read once) 0: every image packed by its own launch, as in round 4


def launch_tables(dtype, rows, work):
    """The tables of az_pack_f16_multi / az_wgrad_unpack_multi (include/azhip.h) as numpy arrays: descs, one `dtype` struct
    per row (a dict of the struct's fields; pad_ stays zero); block_desc, the descriptor of every workgroup (descriptor i has
    work(rows[i]) elements, 256 per workgroup, its workgroups consecutive); first_block, the first workgroup of every
    descriptor; and the number of workgroups"""
    descs = np.zeros(len(rows), dtype=dtype)
    for name in dtype.names:
        if name != "pad_":
            descs[name] = [row[name] for row in rows]
    nb = np.array([(work(row) + 255) // 256 for row in rows], dtype=np.int64)
    return descs, np.repeat(np.arange(len(rows), dtype=np.int32), nb), (np.cumsum(nb) - nb).astype(np.int32), int(nb.sum())


def pack_tables(rows):
    """launch_tables of az_pack_f16_multi: two fp16 parts per weight"""
    return launch_tables(PACK_DESC, rows, lambda r: 2 * r["taps"] * r["cin"] * r["cout"])


class _PackEntry:
    __slots__ = ("wref", "kind", "cin", "cout", "ci_real", "co_real", "s_co", "s_ci", "taps", "flip", "packed", "amax",
                 "version", "index")


class PackPlan:
    """the images of one device"""

    def __init__(self, device):
        self.device = device
        self.lock = threading.RLock()
        self.registered = {}   # data_ptr -> weak amax.Source of the parameter: it and the storage it was registered with
        self.entries = {}      # (data_ptr, kind, cin, cout, ci_real, co_real, s_co, s_ci, taps, flip) -> _PackEntry
        self.amax_rows = {}    # data_ptr -> (row tensor [AMAX_SLOTS], the parameter's Source)
        self.amax_blocks = []  # [tensor [256, AMAX_SLOTS], next row]
        self.table = None      # (descs, block_desc, first_block, nd, nblocks, entry list) on the device: the last one used
        self.tables = {}       # tuple of registered addresses -> table + the amax pointers it was built with
        self.launches = 0      # az_pack_f16_multi launches so far (tests)
        self.amax_op = amax.MultiAbsmax()  # az_absmax_multi and its device tables, per set of stale weights

    # -- weight amax rows: persistent, so that the descriptor table stays valid across steps
    def amax_row(self, w):
        ptr = w.data_ptr()
        hit = self.amax_rows.get(ptr)
        if hit is not None and hit[1]() is w:  # (the row of this parameter, not of one that stood here before it)
            return hit[0]
        if not self.amax_blocks or self.amax_blocks[-1][1] >= self.amax_blocks[-1][0].shape[0]:
            self.amax_blocks.append([torch.zeros(256, AMAX_SLOTS, dtype=torch.float32, device=self.device), 0])
        blk = self.amax_blocks[-1]
        row = blk[0][blk[1]]
        blk[1] += 1
        return row

    def owner(self, ptr):
        """the registered parameter that stands at this address; None once it has died or its storage was replaced
        (`p.data = t`, module.to(), vector_to_parameters: the address is then free for another tensor)"""
        r = self.registered.get(ptr)
        return r() if r is not None else None

    def owns(self, weight):
        """the registered parameter `weight` is -- itself or an alias over its storage with its version counter's value
        (detached, or the gated alias of a training pass) -- or None"""
        r = self.registered.get(weight.data_ptr())
        return r() if (r is not None and r.answers(weight)) else None

    def purge(self):
        dead = [p for p in self.registered if self.owner(p) is None]
        if dead:
            dead = set(dead)
            for p in dead:
                del self.registered[p]
                self.amax_rows.pop(p, None)
            self.entries = {k: e for k, e in self.entries.items() if k[0] not in dead}
            self.table = None
            self.tables.clear()
            self.amax_op.clear()

    def lookup(self, weight, kind, cin, cout, ci_real, co_real, s_co, s_ci, taps, flip):
        """(entry, fresh): the entry of this image of a registered live parameter (created on first request), and whether its
        buffer already holds the image of the parameter's current version; None for unregistered tensors"""
        ptr = weight.data_ptr()
        with self.lock:
            if self.owns(weight) is None:
                return None, False
            key = (ptr, kind, cin, cout, ci_real, co_real, int(s_co), int(s_ci), taps, bool(flip))
            e = self.entries.get(key)
            if e is not None and e.wref is not self.registered[ptr]:
                e = None  # (an image of the parameter that stood at this address before: never served, replaced below)
            if e is None:
                e = _PackEntry()
                e.wref, e.kind, e.cin, e.cout, e.ci_real, e.co_real = self.registered[ptr], kind, cin, cout, ci_real, co_real
                e.s_co, e.s_ci, e.taps, e.flip = int(s_co), int(s_ci), taps, bool(flip)
                e.packed = torch.empty(taps * cin * cout, dtype=torch.float32, device=self.device)  # two fp16 parts per weight
                e.amax, e.version = None, -1
                self.entries[key] = e
                self.table = None  # rebuilt at the next prepack
                self.tables.clear()
            return e, e.version == weight._version

    def _build_table(self, todo):
        descs, block_desc, first, nblocks = pack_tables([
            dict(dst=e.packed.data_ptr(), src=e.wref().data_ptr(), amax=e.amax.data_ptr(), s_co=e.s_co, s_ci=e.s_ci,
                 kind=e.kind, cin=e.cin, cout=e.cout, ci_real=e.ci_real, co_real=e.co_real, taps=e.taps, flip=e.flip)
            for e in todo])
        dev = self.device
        self.table = (torch.from_numpy(descs.view(np.uint8)).to(dev), torch.from_numpy(block_desc).to(dev),
                      torch.from_numpy(first).to(dev), len(todo), nblocks, list(todo))

    def register(self, w):
        """the address of parameter `w` is its own from now on, for as long as it stands there"""
        with self.lock:
            r = self.registered.get(w.data_ptr())
            if r is None or r() is not w:
                self.registered[w.data_ptr()] = Source(w, weak=True)

    def prepack(self, weights):
        """register `weights` (nn.Parameters) and bring every recorded image of THEIRS up to their current version in one
        launch (a table per set of weights: another live model's images are not this call's business); the amax arrays of
        all of them in one call of az_absmax_multi (as prime_weight_amax)"""
        with self.lock:
            self.purge()
            mine = []
            for w in weights:
                if w is None or not w.is_cuda or w.dtype != torch.float32 or w.device != self.device:
                    continue
                self.register(w)
                mine.append(w.data_ptr())
            setkey = tuple(sorted(set(mine)))
            owned = set(setkey)
            todo = [e for k, e in self.entries.items()  # (the images of the parameters that stand there NOW)
                    if k[0] in owned and e.wref is self.registered[k[0]] and e.wref() is not None]
            stale = [e for e in todo if e.version != e.wref()._version]
            if not stale:
                return
            with torch.no_grad(), torch.cuda.device(self.device):
                # amax rows of the weights behind the stale images (persistent rows: rewritten in place by az_absmax_multi)
                ws = {}
                for e in stale:
                    w = e.wref()
                    ws[w.data_ptr()] = w
                wl = list(ws.values())
                rows = []
                for w in wl:
                    row = self.amax_row(w)
                    self.amax_rows[w.data_ptr()] = (row, self.registered[w.data_ptr()])
                    rows.append(row)
                self.amax_op.run([w.detach() for w in wl], rows)
                for w, row in zip(wl, rows):
                    amax.remember_weight_amax(w, row)
                for e in stale:
                    e.amax = self.amax_rows[e.wref().data_ptr()][0]
                todo = [e for e in todo if e.amax is not None]
                tab = self.tables.get(setkey)
                if tab is None or tab[5] != todo or any(e.amax.data_ptr() != p for e, p in zip(todo, tab[6])):
                    self._build_table(todo)
                    tab = self.table + ([e.amax.data_ptr() for e in todo],)
                    if len(self.tables) > 8:
                        self.tables.clear()
                    self.tables[setkey] = tab
                descs, block_desc, first, nd, nblocks, elist, _ = tab
                _call("az_pack_f16_multi", _p(descs), _p(block_desc), _p(first), nd, nblocks, _stream())
                self.launches += 1
                for e in elist:
                    e.version = e.wref()._version
                self.table = tab[:6]  # (the last table used: tests read it)


_PLANS = {}


def pack_plan(device):
    with CACHE_LOCK:
        p = _PLANS.get(device)
        if p is None:
            p = _PLANS[device] = PackPlan(device)
        return p


def prepack(weights):
    """start of a training forward pass: all f16x3 images of these parameters in one launch (PackPlan)"""
    ws = [w for w in weights if w is not None and w.is_cuda]
    if _PLAN_ON and ws:
        pack_plan(ws[0].device).prepack(ws)


def planned_pack(weight, w, kind, cin, cout, ci_real, co_real, s_co, s_ci, taps, flip, pack_now):
    """the plan's (buffer, amax) for this image of a registered parameter, packed by `pack_now(packed, w_amax)` -- the
    per-tensor launch -- when the plan has not brought it up to date (first step, or no prepack this step); None for tensors
    the plan does not own"""
    if not _PLAN_ON or not w.is_cuda:
        return None
    plan = pack_plan(w.device)
    e, fresh = plan.lookup(weight, kind, cin, cout, ci_real, co_real, s_co, s_ci, taps, flip)
    if e is None:
        return None
    if not fresh:
        with plan.lock:
            w_amax = amax.weight_amax(weight, w)
            pack_now(e.packed, w_amax)
            e.amax, e.version = w_amax, weight._version
            # (this entry's amax pointer may have changed: prepack compares the pointers its table was built with)
    return e.packed, e.amax
