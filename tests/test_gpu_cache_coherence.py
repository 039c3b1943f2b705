"""GPU: every host-side table between a parameter and a launch, held to one rule per kind of write
(tests/_cache_coherence.py): after a write, the next call is BIT-equal to the same call with nothing remembered.

Sites (one small call each, through the entry point the networks use):
  * eval3d_*       agg3d.conv_bn, eval + no_grad, stride 1 on (1, 5, 7, 19) in every arithmetic, stride 2 and transposed on
                   (1, 4, 8, 16): PACK_CACHE through _pack and _pack_f16, AFFINE_CACHE, _W_AMAX;
  * costvol        LazyCostVolume into agg3d.conv_bn (the eval path of dres0[0]);
  * eval2d_*       the extractor's conv+BatchNorm unit in eval mode: conv2d.conv_bn_eval for the 3x3 and 1x1 32-multiple layers
                   (_PACK2D_CACHE through _pack_image, AFFINE_CACHE), the generic route for the 3-channel stride-2 first layer;
                   only the gather bf16x6 row of conv2d.KERNELS has a memoised caller today, so pack2d_* call
                   conv2d._pack_image with cache=True directly for the gather f16x3 and roll bf16x6 rows too (1x1 40 -> 12 with
                   padded channel counts, 3x3 32 -> 32) and compare image bytes;
  * merged         costconv._merged_kernels under no_grad (_MERGED_CACHE);  weight_amax: amax.weight_amax (_W_AMAX);
  * train3d_*      the training forward of a unit after packing.prepack + amax.prime_weight_amax, as PSMNet's pass does
                   (PackPlan's entries, amax_rows, _PRIME_ROWS, _W_AMAX).  Train-mode outputs pass through float atomics
                   downstream, so these compare what the launch was HANDED -- image and amax array -- with the per-tensor
                   packer and a fresh az_absmax of the current weight;
  * gru_*          two chained ConvGRU updates on the same context tensors, no_grad (bf16 image) and under autograd in both
                   operand formats (h1 / bf16 images, forward and flipped; _CTX_CACHE, _ROWS_CACHE, _SEEN_ONCE).
Writes: tests/_cache_coherence.py WRITES, the library's own train-mode kernels moving the running statistics, an eviction
between the two calls, and the constructed recycled address (check_recycled).  `.data` writes WITHOUT packing.touched are
promised nothing but a loud AZ_DEBUG_AMAX (the last test, in a child process: the switch is read at import)."""
import gc
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import agg3d, amax, conv2d, conv3d, costconv, packing  # noqa: E402
from activezero_amd.nets.psmnet import psmnet_submodule_3 as sub3  # noqa: E402
from activezero_amd.nets.raft import gru as G  # noqa: E402
from tests import _cache_coherence as H  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = torch.device("cuda", 0)


# ---- sites ------------------------------------------------------------------------------------------------------------------
def _init_bn(bn, seed):
    with torch.no_grad():
        bn.weight.copy_(seeded((bn.num_features,), seed, 0.5, 1.5))
        bn.bias.copy_(seeded((bn.num_features,), seed + 1, -0.2, 0.2))
        bn.running_mean.copy_(seeded((bn.num_features,), seed + 2, -0.2, 0.2))
        bn.running_var.copy_(seeded((bn.num_features,), seed + 3, 0.5, 1.5))


def _unit(conv, bn, seed):
    with torch.no_grad():
        conv.weight.copy_(seeded(tuple(conv.weight.shape), seed, -0.06, 0.06))
    _init_bn(bn, seed + 10)
    return torch.nn.Sequential(conv, bn).to(DEV).eval()


def _unit3d(cin, cout, kind, seed):
    if kind == "t2":
        conv = torch.nn.ConvTranspose3d(cin, cout, 3, padding=1, output_padding=1, stride=2, bias=False)
    else:
        conv = torch.nn.Conv3d(cin, cout, 3, stride=2 if kind == "s2" else 1, padding=1, bias=False)
    return _unit(conv, torch.nn.BatchNorm3d(cout), seed)


def _eval3d(cin, cout, kind, arith, vol):
    def make(device):
        return _unit3d(cin, cout, kind, 100 + cin), seeded((1,) + vol + (cin,), 31, -1.0, 1.0).to(DEV)

    def call(unit, x):
        with torch.no_grad():
            return agg3d.conv_bn(x, unit, relu=True, arith=arith)

    def train(unit, x):
        with torch.no_grad():
            agg3d.conv_bn(0.5 * x + 0.3, unit, relu=True, arith=arith)
    return H.Site(f"eval3d_{kind}_{cin}_{cout}_{arith}", make, call, weight=lambda u: (u[0], "weight"), train=train)


def _costvol():
    def make(device):
        feats = tuple(seeded((1, 32, 7, 19), 40 + i, -1.0, 1.0).to(DEV) for i in range(2))
        return _unit3d(64, 32, "s1", 164), feats

    def call(unit, feats):
        with torch.no_grad():
            return agg3d.conv_bn(agg3d.volume_from_features(feats[0], feats[1], 8, lazy=True), unit, relu=True)
    return H.Site("costvol_64_32", make, call, weight=lambda u: (u[0], "weight"))


def _eval2d(cin, cout, k, stride, folded):
    def make(device):
        unit = _unit(torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False), torch.nn.BatchNorm2d(cout), 200 + cin)
        x = seeded((1, cin, 9, 16), 51, -1.0, 1.0).to(DEV).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():  # (the precondition, asserted: this layer does / does not take the folded kernel)
            assert (conv2d.conv_bn_eval(x, unit[0], unit[1], True) is not None) == folded
        return unit, x

    def call(unit, x):
        with torch.no_grad():
            return sub3._convbn_unit(x, unit, relu=True)

    def train(unit, x):
        with torch.no_grad():
            sub3._convbn_unit(0.5 * x + 0.3, unit, relu=True)
    return H.Site(f"eval2d_{k}x{k}s{stride}_{cin}_{cout}", make, call, weight=lambda u: (u[0], "weight"), train=train)


class _Holder(torch.nn.Module):
    cache_coherence_weight = True

    def __init__(self, w):
        super().__init__()
        self.weight = torch.nn.Parameter(w)


def _holder_site(name, shape, call, scale=0.06):
    return H.Site(name, lambda device: (_Holder(seeded(shape, 61, -scale, scale)).to(DEV), None), call,
                  weight=lambda m: (m, "weight"))


def _merged_call(mod, _):
    with torch.no_grad():
        return costconv._merged_kernels(mod.weight, 8)


def _amax_value(am):
    """the value of an amax array: the largest of its slots (the floats between the slots are never written)"""
    return am[::amax._STRIDE].max().reshape(1)


def _weight_amax_call(mod, _):
    return _amax_value(amax.weight_amax(mod.weight, mod.weight.detach()))


def _pack2d_f16_call(mod, _):  # 1x1 40 -> 12: channel counts padded to 48 / 32, as tests/test_gpu_pack_plan.py packs it
    with torch.no_grad():
        packed, w_amax = conv2d._pack_image(conv2d.GATHER_F16, mod.weight, 48, 32, 40, 1, 1, 1, False, 40, 12, cache=True)
        return packed, _amax_value(w_amax)


def _pack2d_roll_call(mod, _):
    with torch.no_grad():
        return conv2d._pack_image(conv2d.ROLL_X6, mod.weight, 32, 32, 32 * 9, 9, cache=True)[0]


def _pack2d_call(mod, _):
    with torch.no_grad():
        return conv2d._pack_image(conv2d.GATHER_X6, mod.weight, 48, 32, 40, 1, 1, 1, False, 40, 12, cache=True)[0]


def _handed(unit, x, arith="f16x3"):
    """(image, amax value) the f16x3 launch of this training forward was handed"""
    used = []
    orig = conv3d._pack_f16

    def spy(*a, **k):
        r = orig(*a, **k)
        used.append((r[0].clone(), _amax_value(r[1])))
        return r
    conv3d._pack_f16 = spy
    try:
        with torch.enable_grad():
            agg3d.conv_bn(x, unit, relu=True, arith=arith)
    finally:
        conv3d._pack_f16 = orig
    assert len(used) == 1, "the training forward did not take the f16x3 route"
    return used[0]


def _train3d(c, prepack_once=False):
    """prepack_once: only the first call of a module registers its weight with the plan -- the recycled address then meets
    PackPlan.lookup alone"""
    def make(device):
        unit = _unit3d(c, c, "s1", 300 + c).train()
        return unit, seeded((1, 5, 7, 19, c), 71, -1.0, 1.0).to(DEV)

    def call(unit, x):
        w = unit[0].weight
        if not (prepack_once and getattr(unit, "was_prepacked", False)):
            packing.prepack([w])
            unit.was_prepacked = True
        amax.prime_weight_amax([w])
        return _handed(unit, x)

    def fresh(unit, x):
        w = unit[0].weight.detach().clone()
        cin, cout, s_out, s_in = conv3d._fwd_launch(w, conv3d.CONV_S1)
        am = w.new_empty(amax.AMAX_SLOTS)
        amax._call("az_absmax", amax._p(am), amax._p(w), w.numel(), amax._stream())
        packed = torch.empty(conv3d._lib.lib().az_conv3d_packed_floats_f16(cin, cout), dtype=torch.float32, device=DEV)
        conv3d._call("az_conv3d_pack_weights_f16", conv3d._p(packed), conv3d._p(w), conv3d._p(am), cin, cout, s_out, s_in, 0,
                     conv3d.CONV_S1, conv3d._stream())
        return packed, _amax_value(am)
    return H.Site(f"train3d_{c}_{c}" + ("_lookup_alone" if prepack_once else ""), make, call, fresh=fresh,
                  weight=lambda u: (u[0], "weight"), skip=("bn_eps",))  # (what the launch is handed does not depend on the BatchNorm)


def _gru(mode):
    b, c, cx, h, w = 2, 32, (36, 60), 21, 35  # the smallest ConvGRU of tests/test_gpu_gru_fp64.py

    def make(device):
        from tests.test_gpu_raft_gru import _inputs
        torch.manual_seed(11)
        mod = G.ConvGRU(c, sum(cx)).to(DEV)
        if mode != "eval":
            mod.train_arithmetic = mode
        hid, ctx, xs = _inputs(b, c, cx, h, w, 79)
        cot = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(4)).to(DEV)
        return mod, (hid.to(DEV), [t.to(DEV) for t in ctx], [t.to(DEV) for t in xs], cot)

    def call(mod, inputs):
        hid, ctx, xs, cot = inputs
        if mode == "eval":
            with torch.no_grad():
                return mod(mod(hid, *ctx, *xs), *ctx, *xs)
        with torch.enable_grad():
            leaves = [hid.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in xs]
            s2 = mod(mod(leaves[0], *ctx, *leaves[1:]), *ctx, *leaves[1:])  # (the same context tensors in both updates)
            # state and input gradients: through the flipped images, and free of float atomics (the weight gradients are not)
            return (s2,) + torch.autograd.grad((s2 * cot).sum(), leaves)
    return H.Site(f"gru_{mode}", make, call, weight=lambda m: (m.convq, "weight"))


EVAL3D = [_eval3d(c, c, "s1", arith, (5, 7, 19)) for c in (32, 64) for arith in ("f16x3", "bf16x6", "fp32")] + \
         [_eval3d(32, 64, "s2", "f16x3", (4, 8, 16)), _eval3d(64, 32, "t2", "f16x3", (4, 8, 16))]
EVAL2D = [_eval2d(32, 32, 3, 1, True), _eval2d(64, 32, 1, 1, True), _eval2d(3, 32, 3, 2, False)]
PACKERS = [_holder_site("merged_kernels", (32, 64, 3, 3, 3), _merged_call),
           _holder_site("weight_amax", (32, 32, 3, 3, 3), _weight_amax_call),
           _holder_site("pack2d_f16_1x1_40_12", (12, 40, 1, 1), _pack2d_f16_call),
           _holder_site("pack2d_1x1_40_12", (12, 40, 1, 1), _pack2d_call),
           _holder_site("pack2d_roll_32_32", (32, 32, 3, 3), _pack2d_roll_call)]
TRAIN3D = [_train3d(32), _train3d(64)]
GRU = [_gru("eval"), _gru("f16x1"), _gru("bf16")]
SITES = EVAL3D + [_costvol()] + EVAL2D + PACKERS + TRAIN3D + GRU


def _cases():
    out = []
    for site in SITES:
        with_bn = not (site in PACKERS or site in GRU)
        for name, (_fn, needs_bn) in H.WRITES.items():
            if (needs_bn and not with_bn) or name in site.skip:
                continue
            out.append(pytest.param(site, name, id=f"{site.name}-{name}"))
        if site.train is not None:
            out.append(pytest.param(site, "train_kernels", id=f"{site.name}-train_kernels"))
    return out


@pytest.mark.parametrize("site,write", _cases())
def test_the_call_after_a_write_equals_a_call_with_nothing_remembered(site, write, monkeypatch):
    if write == "train_kernels":
        # running statistics moved by the library's own train-mode kernels (raw pointers + packing.touched), no optimizer step
        def fn(unit, device):
            _module, x = site.make(device)
            unit.train()
            for _ in range(2):
                site.train(unit, x)
            unit.eval()
    else:
        fn = H.WRITES[write][0]
    H.check(site, fn, DEV, monkeypatch)


# ---- eviction ---------------------------------------------------------------------------------------------------------------
def _evict_everything():
    """push every memo past its limit, so that its clear() runs"""
    for cache, limit in ((packing.PACK_CACHE, 256), (packing.AFFINE_CACHE, 512), (conv2d._PACK2D_CACHE, 256),
                         (costconv._MERGED_CACHE, 16), (G._PACK_CACHE, 64)):
        had = len(cache)
        for i in range(limit + 2 - had):
            packing.cache_put(cache, ("filler", i), (None, ()), limit)
        assert len(cache) <= 2, "the cache was not emptied"
    filler = torch.zeros(1)
    had = len(amax._W_AMAX)
    for i in range(514 - had):
        amax._W_AMAX[("filler", i)] = (None, None)
    amax.remember_weight_amax(filler, filler)
    assert len(amax._W_AMAX) == 1


EVICTED = [EVAL3D[0], EVAL3D[1], EVAL2D[0], PACKERS[0], PACKERS[1], GRU[0], GRU[1]]


@pytest.mark.parametrize("site", EVICTED, ids=lambda s: s.name)
def test_an_eviction_between_two_calls_changes_nothing(site, monkeypatch):
    H.check_unchanged(site, DEV, monkeypatch, _evict_everything)
    H.check(site, H.w_inplace, DEV, monkeypatch, between=_evict_everything)


# ---- a recycled address -------------------------------------------------------------------------------------------------------
RECYCLED = [EVAL3D[0], EVAL3D[1], EVAL3D[3], EVAL3D[6], EVAL3D[7], SITES[len(EVAL3D)], EVAL2D[0]] + PACKERS + \
           TRAIN3D + [_train3d(32, prepack_once=True), _train3d(64, prepack_once=True)] + GRU


@pytest.mark.parametrize("site", RECYCLED, ids=lambda s: s.name)
def test_a_recycled_address_is_not_answered_with_the_entry_of_the_tensor_that_left(site, monkeypatch):
    """inference memos (eval3d / costvol / eval2d / pack2d / gru), _W_AMAX (weight_amax, and eval3d f16x3), _MERGED_CACHE
    (merged_kernels) and PackPlan -- train3d: prepack([B]) then lookup; train3d_*_lookup_alone: lookup alone"""
    H.check_recycled(site, DEV, monkeypatch)


# ---- the amax attribute of an activation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["mul_4", "zero_through_a_view"])
def test_an_activation_modified_in_place_loses_its_attached_amax(how, monkeypatch):
    with H.nothing_remembered(monkeypatch):
        first, second = _unit3d(32, 32, "s1", 400).train(), _unit3d(32, 32, "s1", 410)
        with torch.no_grad():
            first[1].weight[0] = 8.0  # channel 0 carries the largest values: zeroing it lowers max |y|
            first[1].bias[0] = 1.0
            y = agg3d.conv_bn(seeded((1, 5, 7, 19, 32), 81, -1.0, 1.0).to(DEV), first, relu=True, arith="f16x3")
            attached = amax._get_amax(y)
            assert attached is not None, "the BatchNorm apply attached no amax: the case cannot fail"
            attached = attached.clone()
            if how == "mul_4":
                y.mul_(4.0)
            else:
                y[..., :1].zero_()
            now = y.new_empty(amax.AMAX_SLOTS)
            amax._call("az_absmax", amax._p(now), amax._p(y), y.numel(), amax._stream())
            assert float(now[::amax._STRIDE].max()) != float(attached[::amax._STRIDE].max()), "max |y| did not move: the case cannot fail"
            got = agg3d.conv_bn(y, second, relu=True, arith="f16x3")
            want = agg3d.conv_bn(y.clone(), second, relu=True, arith="f16x3")
        assert H.same((got,), (want,))


# ---- the ConvGRU's caches are still caches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x1", "bf16"])
def test_the_gru_converts_its_context_once_and_its_inputs_once(mode, monkeypatch):
    site = _gru(mode)
    with H.nothing_remembered(monkeypatch):
        mod, (hid, ctx, xs, _cot) = site.make(DEV)
        counts = []
        for _ in range(2):
            c0, r0 = G.CTX_CONVERSIONS, G.ROW_CONVERSIONS
            with torch.enable_grad():
                state = hid.clone().requires_grad_(True)
                mod(mod(state, *ctx, *xs), *ctx, *xs)
            counts.append((G.CTX_CONVERSIONS - c0, G.ROW_CONVERSIONS - r0))
        # two chained updates: the context rows once; each input as an image first, through its cached copy the second time;
        # the same tensors in the next pair of updates: nothing is converted again
        assert counts == [(1, 2), (0, 0)], counts
        packs = len(G._PACK_CACHE)
        assert packs == 2, packs  # (wz | wr) and wq forward images, remembered
        with torch.enable_grad():
            mod(hid.clone().requires_grad_(True), *ctx, *xs)
        assert len(G._PACK_CACHE) == packs


@pytest.mark.parametrize("what", ["context_in_place", "context_dead_and_recycled", "input_in_place"])
def test_the_gru_follows_its_context_and_its_inputs(what, monkeypatch):
    """_CTX_CACHE, _ROWS_CACHE and _SEEN_ONCE are keyed on ACTIVATIONS: an in-place write bumps their counter, and an entry
    whose source has died is not served to the tensor that stands at its address now (constructed: the context tensors are
    views of a caller-owned buffer, so the new ones have the dead ones' address and counter value)"""
    site = _gru("f16x1")
    with H.nothing_remembered(monkeypatch):
        mod, (hid, ctx, xs, cot) = site.make(DEV)
        buf = torch.stack(ctx).contiguous()
        del ctx
        views = [buf[i] for i in range(3)]
        before = H._tuple(site.call(mod, (hid, views, xs, cot)))
        where = [(t.data_ptr(), t._version) for t in views]
        c0 = G.CTX_CONVERSIONS
        with torch.no_grad():
            if what == "context_in_place":
                views[0].mul_(1.5)
            elif what == "input_in_place":
                xs[0].mul_(1.5)
            else:
                del views
                gc.collect()
                buf.data.mul_(1.5)
                views = [buf[i] for i in range(3)]
                assert [(t.data_ptr(), t._version) for t in views] == where
        got = H._tuple(site.call(mod, (hid, views, xs, cot)))
        if what != "input_in_place":
            assert G.CTX_CONVERSIONS - c0 == 1
        want = site.fresh(mod, (hid, [t.clone() for t in views], [t.clone() for t in xs], cot), monkeypatch)
        assert not H.same(before, want), "the write does not change the answer: the case cannot fail"
        assert H.same(got, want)


# ---- .data writes without packing.touched: promised nothing, but AZ_DEBUG_AMAX is loud about them ----------------------------
_CHILD = """
import torch
from activezero_amd import agg3d, packing
from tests.test_gpu_cache_coherence import DEV, _unit3d, seeded
unit = _unit3d(32, 32, "s1", 500)
x = seeded((1, 5, 7, 19, 32), 91, -1.0, 1.0).to(DEV)
with torch.no_grad():
    agg3d.conv_bn(x, unit, relu=True, arith="f16x3")
    unit[0].weight.data.mul_(4.0)          # max |w| four times larger, and no version counter knows
    if {touched}:
        packing.touched(unit[0].weight)
    agg3d.conv_bn(x, unit, relu=True, arith="f16x3")
print("REACHED THE END")
"""


@pytest.mark.parametrize("touched", [False, True], ids=["without_touched", "with_touched"])
def test_a_data_write_without_touched_trips_the_amax_debug_switch(touched, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(touched=touched))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AZ_DEBUG_AMAX="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, str(script)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    if touched:
        assert r.returncode == 0 and "REACHED THE END" in r.stdout, r.stderr[-2000:]
    else:
        assert r.returncode != 0 and "stale amax" in r.stderr and "packing.touched" in r.stderr, (r.stdout, r.stderr[-2000:])
