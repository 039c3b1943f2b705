"""The ConvGRU's input-row sources (activezero_amd/nets/raft/gru.py: _source) and a recycled allocation address.

_source sends an NCHW image of at most 128 channels through az_rows_concat as an image the first time it sees the tensor,
and through a cached channels-last copy when the same tensor comes back.  Its caches are keyed by (address, version,
device) and hold weak references.  An entry of _ROWS_CACHE left by a tensor that has died, at an address the allocator
has since handed to another tensor, must not answer for the new tensor: before the fix it did, the new tensor took the
cached-copy route at its FIRST appearance and ROW_CONVERSIONS counted one conversion too many -- observed on the GPU as
`made == 3` instead of 2 in tests/test_gpu_raft_gru.py::test_gru_update_with_assembled_rows_equals_the_slice_assignments
once earlier tests of the same process had left the allocator in another state.  No kernel is launched: _source only
inspects its argument, and the copy is a torch permute."""
import weakref

import torch

from activezero_amd.nets.raft import gru as G
from activezero_amd.packing import cache_key


def _fresh_caches(monkeypatch):
    monkeypatch.setattr(G, "_ROWS_CACHE", {})
    monkeypatch.setattr(G, "_SEEN_ONCE", {})


def test_a_stale_rows_entry_at_a_recycled_key_does_not_answer_for_a_new_tensor(monkeypatch):
    _fresh_caches(monkeypatch)
    t = torch.randn(2, 36, 5, 7)
    dead = torch.randn(2, 36, 5, 7)
    stale_rows = dead.permute(0, 2, 3, 1).contiguous()
    ref = weakref.ref(dead)
    G._ROWS_CACHE[cache_key(t)] = (stale_rows, ref)  # what a dead tensor leaves behind once t recycles its address
    del dead
    assert ref() is None
    before = G.ROW_CONVERSIONS
    src, kind = G._source(t)
    assert src is t and kind == 1  # first appearance: the image route, as with an empty cache
    assert G.ROW_CONVERSIONS == before
    # ... and an entry for ANOTHER live tensor under the same key (same address after an in-place free) is no better
    other = torch.randn(2, 36, 5, 7)
    _fresh_caches(monkeypatch)
    G._ROWS_CACHE[cache_key(t)] = (other.permute(0, 2, 3, 1).contiguous(), weakref.ref(other))
    src, kind = G._source(t)
    assert src is t and kind == 1 and G.ROW_CONVERSIONS == before


def test_the_second_appearance_still_takes_the_cached_copy(monkeypatch):
    _fresh_caches(monkeypatch)
    t = torch.randn(2, 36, 5, 7)
    before = G.ROW_CONVERSIONS
    assert G._source(t)[1] == 1
    rows, kind = G._source(t)  # the same tensor again: one conversion, then hits
    assert kind == 0 and torch.equal(rows, t.permute(0, 2, 3, 1)) and G.ROW_CONVERSIONS == before + 1
    again, kind = G._source(t)
    assert kind == 0 and again is rows and G.ROW_CONVERSIONS == before + 1
    wide = torch.randn(1, 220, 5, 7)  # too wide for the kernel's image tile: cached at once
    assert G._source(wide)[1] == 0 and G.ROW_CONVERSIONS == before + 2
