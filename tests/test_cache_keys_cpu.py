"""The address-keyed tables and a recycled address, on the CPU, with no kernel involved; and proof that the cache-coherence
harness (tests/_cache_coherence.py) can fail.

Every table between a parameter and a launch is keyed by (data_ptr, _version, device).  `p.data = t`, module.to() and
vector_to_parameters replace a parameter's storage and leave `_version` alone, so a second parameter of the same shape can
stand at the first one's old address with the first one's counter value.  Constructed here with a caller-owned buffer (the
allocator is not asked to cooperate): packing.memo, costconv._merged_kernels, amax.weight_amax and PackPlan.lookup each
answered for the second parameter with the first one's entry before they verified their hits (amax.Source).

The mutants are toy memos, each wrong in one way a key can be wrong, each rejected by the check named for it."""
import gc

import pytest
import torch

from activezero_amd import amax, costconv, packing
from tests import _cache_coherence as H
from tests._weights import seeded

DEV = torch.device("cpu")
CPU_WRITES = [w for w in H.WRITES if w != "fused_adam_step"]  # (FusedAdam's kernels: tests/test_gpu_cache_coherence.py)


# ---- a toy site: a "packed weight" and a folded BatchNorm map through packing.memo, in pure torch ---------------------------
def _toy_make(device):
    torch.manual_seed(0)
    unit = torch.nn.Sequential(torch.nn.Conv3d(2, 3, 1, bias=False), torch.nn.BatchNorm3d(3)).to(device).eval()
    with torch.no_grad():
        unit[1].weight.copy_(seeded((3,), 1, 0.5, 1.5))
        unit[1].bias.copy_(seeded((3,), 2, -0.2, 0.2))
        unit[1].running_mean.copy_(seeded((3,), 3, -0.2, 0.2))
        unit[1].running_var.copy_(seeded((3,), 4, 0.5, 1.5))
    return unit, None


def _toy_call(flavour):
    def call(unit, _inputs):
        w, bn = unit[0].weight, unit[1]
        pack = lambda: w.detach() * 2.0
        if flavour == "correct":
            image = packing.memo(packing.PACK_CACHE, packing.cache_key(w), pack, (w,), 8)
        else:  # the mutants keep the parameter OBJECT alive and believe their key
            key = (w.data_ptr(),) if flavour == "no_version" else packing.cache_key(w)
            hit = packing.PACK_CACHE.get(key)
            if hit is None:
                hit = packing.PACK_CACHE[key] = (pack(), w)
            image = hit[0]
        src = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)

        def fold():
            scale = bn.weight.detach() / (bn.running_var + bn.eps).sqrt()
            return scale, bn.bias.detach() - bn.running_mean * scale

        scale, shift = packing.memo(packing.AFFINE_CACHE, (packing.cache_key(*src), float(bn.eps)), fold, src, 8)
        return image, scale, shift
    return call


def toy(flavour):
    return H.Site("toy:" + flavour, _toy_make, _toy_call(flavour), weight=lambda unit: (unit[0], "weight"))


@pytest.mark.parametrize("write", CPU_WRITES)
def test_the_correct_memo_passes_every_write(write, monkeypatch):
    H.check(toy("correct"), H.WRITES[write][0], DEV, monkeypatch)


def test_the_correct_memo_passes_the_recycled_address(monkeypatch):
    H.check_recycled(toy("correct"), DEV, monkeypatch)


def test_the_correct_memo_survives_an_eviction(monkeypatch):
    def evict():
        for i in range(12):  # past the toy's limit of 8: cache.clear() runs
            t = torch.zeros(1)
            packing.memo(packing.PACK_CACHE, ("filler", i), lambda: t, (t,), 8)
        assert len(packing.PACK_CACHE) < 8
    H.check_unchanged(toy("correct"), DEV, monkeypatch, evict)
    H.check(toy("correct"), H.w_inplace, DEV, monkeypatch, between=evict)


def test_a_memo_keyed_without_the_version_counter_is_rejected(monkeypatch):
    with pytest.raises(AssertionError, match="stale after the write"):
        H.check(toy("no_version"), H.w_inplace, DEV, monkeypatch)


def test_a_memo_that_does_not_pin_or_verify_its_source_is_rejected_by_the_recycled_address(monkeypatch):
    """(address, version) with the parameter object kept alive -- this library's rule before amax.Source"""
    site = toy("no_pin")
    for write in CPU_WRITES:  # ... which every ordinary write lets through: the construction is what finds it
        H.check(site, H.WRITES[write][0], DEV, monkeypatch)
    with pytest.raises(AssertionError, match="B at a recycled address was answered with another tensor's entry"):
        H.check_recycled(site, DEV, monkeypatch)


def test_a_write_that_does_not_change_the_answer_is_refused(monkeypatch):
    def nothing(unit, device):
        with torch.no_grad():
            unit[0].weight.mul_(1.0)
    with pytest.raises(AssertionError, match="the case cannot fail"):
        H.check(toy("correct"), nothing, DEV, monkeypatch)


def test_same_is_bitwise():
    a = torch.tensor([0.0, float("nan")])
    assert H.same((a,), (a.clone(),)) and not H.same((a,), (torch.tensor([-0.0, float("nan")]),))
    assert not H.same((a,), (a, a)) and not H.same((a,), (a.double(),))


# ---- the library's own tables ---------------------------------------------------------------------------------------------
class _Holder(torch.nn.Module):
    cache_coherence_weight = True

    def __init__(self, w):
        super().__init__()
        self.weight = torch.nn.Parameter(w)


def test_merged_kernels_at_a_recycled_address(monkeypatch):
    def call(mod, _):
        with torch.no_grad():
            return costconv._merged_kernels(mod.weight, 8)
    site = H.Site("merged_kernels", lambda dev: (_Holder(seeded((32, 64, 3, 3, 3), 7, -0.3, 0.3)), None), call,
                  weight=lambda mod: (mod, "weight"))
    H.check_recycled(site, DEV, monkeypatch)
    H.check(site, H.w_data_assign, DEV, monkeypatch)
    H.check(site, H.w_inplace, DEV, monkeypatch)


def test_weight_amax_at_a_recycled_address(monkeypatch):
    misses = []

    def stub(t):  # stands for az_absmax: records that the cache asked for a fresh one
        misses.append(t.data_ptr())
        return t.detach().abs().max().reshape(1).clone()
    monkeypatch.setattr(amax, "absmax", stub)

    def call(mod, _):
        return amax.weight_amax(mod.weight, mod.weight.detach())
    site = H.Site("weight_amax", lambda dev: (_Holder(seeded((4, 4, 3, 3, 3), 8, -0.3, 0.3)), None), call,
                  weight=lambda mod: (mod, "weight"))
    H.check_recycled(site, DEV, monkeypatch)
    # and the cache is still a cache: one miss per tensor and version, hits (aliases included) after it
    with H.nothing_remembered(monkeypatch):
        w = torch.nn.Parameter(seeded((4, 4, 3, 3, 3), 9))
        del misses[:]
        first = amax.weight_amax(w, w.detach())
        assert amax.weight_amax(w, w.detach()) is first and amax.weight_amax(w.detach(), w.detach()) is first
        assert amax.weight_amax(w.view_as(w), w.detach()) is first and len(misses) == 1
        with torch.no_grad():
            w.mul_(4.0)
        assert float(amax.weight_amax(w, w.detach())) == 4.0 * float(first) and len(misses) == 2


def test_a_source_pins_its_storage_and_notices_that_its_tensor_left():
    p = torch.nn.Parameter(seeded((8, 8), 10))
    s = amax.Source(p)
    ptr = p.data_ptr()
    assert s.answers(p) and s.answers(p.detach()) and s.stands() is p
    assert not s.answers(p.detach()[:4]) and not s.answers(p.detach().t())  # (other shapes / strides over the same bytes)
    p.data = torch.zeros(8, 8)        # `p.data = t`: the counter stays, the storage goes
    gc.collect()
    assert s.stands() is None and not s.answers(p) and s.pin.data_ptr() == ptr  # the old block is still held: not recyclable
    q = torch.nn.Parameter(s.pin)     # another parameter over the very same bytes, same counter value
    assert q.data_ptr() == ptr and not s.answers(q)
    alias = q.view_as(q)              # (what overlap._Gate hands the layers of a training pass)
    via = amax.Source(alias)
    assert via.stands() is q and via.answers(q) and via.answers(alias)
    q.data = torch.ones(8, 8)
    assert via.stands() is None and not via.answers(alias) and not via.answers(torch.nn.Parameter(s.pin))
    weak = amax.Source(q, weak=True)
    assert weak() is q
    del q, alias, via  # (the alias keeps its base alive, `via` the tensor it recorded)
    gc.collect()
    assert weak() is None


ARGS = (packing.PACK_3D_ROLL, 32, 32, 32, 32, 32 * 27, 27, 27, False)


@pytest.mark.parametrize("route", ["lookup_alone", "register_then_lookup"])
def test_the_pack_plan_at_a_recycled_address(route):
    """PackPlan.lookup on the CPU (prepack itself only takes device tensors: its registration step is `register`, its first
    step `purge`; tests/test_gpu_cache_coherence.py runs the real prepack)"""
    plan = packing.PackPlan(DEV)
    w0 = seeded((32, 32, 3, 3, 3), 11, -0.3, 0.3)
    buf = w0.clone()
    a = torch.nn.Parameter(buf.view_as(buf))
    plan.register(a)
    e, fresh = plan.lookup(a, *ARGS)
    assert e is not None and not fresh
    e.version = a._version  # (as a pack would leave it)
    assert plan.lookup(a, *ARGS) == (e, True) and plan.lookup(a.detach(), *ARGS) == (e, True)
    ptr, version = a.data_ptr(), a._version
    a.data = a.detach().clone()
    buf.data.mul_(1.5)
    b = torch.nn.Parameter(buf.view_as(buf))
    assert b.data_ptr() == ptr and b._version == version
    if route == "lookup_alone":
        assert plan.lookup(b, *ARGS) == (None, False)  # nobody's address: the per-call route packs B's values
        assert plan.lookup(a, *ARGS) == (None, False)  # A has moved: not registered where it stands now
    else:
        plan.purge()
        plan.register(b)
        e2, fresh = plan.lookup(b, *ARGS)
        assert e2 is not None and e2 is not e and not fresh and e2.wref() is b
        plan.register(a)
        ea, fresh = plan.lookup(a, *ARGS)
        assert ea is not e and ea is not e2 and not fresh and ea.wref() is a
    # a version bump of the owner that an alias with its own counter has not seen: not served as fresh
    with torch.no_grad():
        b.mul_(2.0)
    assert plan.lookup(torch.nn.Parameter(buf.view_as(buf)), *ARGS)[1] is False
