"""GPU: the kernels that turn a whole map into a few numbers, per accumulator -- K12 az_disp_loss_fwd / _bwd and az_disp_metrics,
K16 az_seq_loss_fwd / _bwd, az_absmax and az_absmax_multi -- through the C ABI and through the wrappers, against the
restatement and by the rules of tests/_reduce_ref.py: counts exact, gradients equal as values, sums within the reordering
bound of fsum of the float32 terms, absmax bit for bit.  Map sizes sit on both sides of the block, of the 1024-block
reduction cap and of the 4096-block element-wise cap; special pixels sit on every threshold, on the range mask's ends and on
both sides of every batch boundary (tests/test_reduce_error_model_cpu.py shows which wrong kernels fail here).
The weights' amax -- amax.prime_weight_amax, packing.PackPlan.prepack -- is the largest FINITE magnitude, az_absmax's bits:
a weight tensor with one inf / NaN element spoils the output channel that reads it and no other."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import amax, conv2d, conv3d, ops, packing  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from activezero_amd.utils import cascade_metrics as cm  # noqa: E402
from tests import _nonfinite as NF  # noqa: E402
from tests import _reduce_ref as R  # noqa: E402
from tests._weights import seeded  # noqa: E402
from tests.test_gpu_f16x3_contract import bound as contract_bound  # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES = list(range(len(R.MAP_SHAPES)))
SHAPE_IDS = ["x".join(map(str, s)) for s in R.MAP_SHAPES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def zeros64(n):
    return torch.zeros(n, dtype=torch.float64, device=DEV)


def report(capsys, name, info):
    with capsys.disabled():
        print(f"\n  {name}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in info.items()), end="")
    for k, v in info.items():
        if isinstance(v, float):
            WORST[k] = max(WORST.get(k, 0.0), v)


WORST = {}  # accumulator -> largest err / bound over the cases run so far (printed when the file's last test is done)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\n  largest err / bound per sum over this run: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


# ---- K12 loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SHAPES, ids=SHAPE_IDS)
def test_disp_loss_forward_per_accumulator(k, capsys):
    c = R.loss_case(R.MAP_SHAPES[k], 7200 + k)
    p3, p2, p1, gt, m = (dev(a) for a in (*c["preds"], c["gt"], c["mask"]))
    for mode, mask, lo, hi in R.loss_modes(c):
        acc = zeros64(4)
        args = (_p(p3), _p(p2), _p(p1), _p(gt), _p(m) if mask is not None else None, float(lo), float(hi), c["n"], _stream())
        _call("az_disp_loss_fwd", _p(acc), *args)
        report(capsys, f"az_disp_loss_fwd {c['name']} {mode}", R.check_k12_fwd(host(acc), c["preds"], c["gt"], mask, lo, hi))
        _call("az_disp_loss_fwd", _p(acc), *args)  # the header promises +=
        R.check_k12_fwd(host(acc), c["preds"], c["gt"], mask, lo, hi, calls=2, what="az_disp_loss_fwd, two calls")
        # the wrapper's scalar, and its gradient under an upstream factor
        ps = [t.clone().requires_grad_() for t in (p3, p2, p1)]
        loss = ops.disp_loss(*ps, gt, m if mask is not None else None, lo, hi)
        want, lim = R.disp_loss_scalar(c["preds"], c["gt"], mask, lo, hi)
        count = R.k12_fwd(c["preds"], c["gt"], mask, lo, hi)[1]
        assert loss.dtype == torch.float32 and abs(loss.item() - want) <= lim, (mode, loss.item(), want, lim)
        (loss * 1.75).backward()
        R.check_k12_bwd([host(p.grad) for p in ps], c["preds"], c["gt"], mask, lo, hi, 1.75, count, what=f"ops.disp_loss {mode}")


@pytest.mark.parametrize("k", SHAPES, ids=SHAPE_IDS)
def test_disp_loss_backward_equals_the_restatement(k, capsys):
    c = R.loss_case(R.MAP_SHAPES[k], 7200 + k, nonfinite_preds=True)
    p3, p2, p1, gt, m = (dev(a) for a in (*c["preds"], c["gt"], c["mask"]))
    gloss = torch.tensor([1.75], device=DEV)
    for mode, mask, lo, hi in R.loss_modes(c):
        count = R.k12_fwd(c["preds"], c["gt"], mask, lo, hi)[1]
        acc = torch.tensor([0.0, 0.0, 0.0, count], dtype=torch.float64, device=DEV)
        gs = [torch.full_like(p3, float("nan")) for _ in range(3)]
        _call("az_disp_loss_bwd", *(_p(g) for g in gs), _p(p3), _p(p2), _p(p1), _p(gt), _p(m) if mask is not None else None,
              float(lo), float(hi), _p(gloss), _p(acc), *R.LOSS_WEIGHTS, c["n"], _stream())
        info = R.check_k12_bwd([host(g) for g in gs], c["preds"], c["gt"], mask, lo, hi, 1.75, count)
        info["NaN kept"] = int(np.isnan(host(gs[0])).sum())
        report(capsys, f"az_disp_loss_bwd {c['name']} {mode}: equal elements", info)
        assert c["n"] < 40 or info["NaN kept"] >= 1


def test_disp_loss_over_an_empty_mask():
    """count 0: the loss is NaN, as the reference's mean over nothing; the kernel's gradient is s = gloss / 0 = inf times
    nothing -- every pixel is invalid and gets 0 -- and fp64 autograd of the reference's expression gives the same classes"""
    c = R.loss_case((2, 1, 24, 40), 7290)
    empty = np.zeros_like(c["mask"])
    ps = [dev(p).requires_grad_() for p in c["preds"]]
    loss = ops.disp_loss(*ps, dev(c["gt"]), dev(empty))
    assert math.isnan(loss.item())
    loss.backward()
    ok = torch.from_numpy(empty != 0)
    ref = [torch.from_numpy(p).double().requires_grad_() for p in c["preds"]]
    gt64 = torch.from_numpy(c["gt"]).double()
    rl = sum(w * F.smooth_l1_loss(p[ok], gt64[ok], reduction="mean") for w, p in zip(R.LOSS_WEIGHTS, ref))
    assert math.isnan(float(rl))
    rl.backward()
    for p, r, want in zip(ps, ref, R.k12_bwd(c["preds"], c["gt"], empty, 0.0, math.inf, 1.0, 0)):
        NF.same_classes(p.grad, r.grad, "ops.disp_loss over an empty mask")
        assert float(p.grad.abs().max()) == 0.0 and np.array_equal(host(p.grad), want)


# ---- K12 metrics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SHAPES, ids=SHAPE_IDS)
def test_disp_metrics_per_accumulator(k, capsys):
    c = R.metrics_case(R.MAP_SHAPES[k], 7300 + k)
    dg, zg, dp, zp, fb, m = (dev(c[key]) for key in ("dg", "zg", "dp", "zp", "fb", "mask"))
    for path, zp_np, zp_dev in (("fb", None, None), ("depth_pred", c["zp"], zp)):
        acc = zeros64(8)
        args = (_p(dg), _p(zg), _p(dp), _p(zp_dev), _p(fb), _p(m), c["B"], c["per_batch"], _stream())
        ref = (c["dg"], c["zg"], c["dp"], zp_np, c["fb"], c["mask"], c["per_batch"])
        _call("az_disp_metrics", _p(acc), *args)
        report(capsys, f"az_disp_metrics {c['name']} {path}", R.check_k12_metrics(host(acc), *ref))
        _call("az_disp_metrics", _p(acc), *args)
        R.check_k12_metrics(host(acc), *ref, calls=2, what="az_disp_metrics, two calls")
        focal = fb.reshape(-1, 1, 1, 1)
        got = cm.compute_err_metric(dg, zg, dp, focal, torch.ones_like(focal), m.bool(), depth_pred=zp_dev)
        want = R.metrics_scalars(*ref)
        assert sorted(got) == sorted(R.METRIC_KEYS)
        for key, (v, lim) in want.items():
            assert abs(got[key] - v) <= lim, (path, key, got[key], v, lim)


# ---- K16 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SHAPES, ids=SHAPE_IDS)
def test_seq_loss_forward_per_accumulator(k, capsys):
    c = R.seq_case(R.MAP_SHAPES[k], 7400 + k)
    gt = dev(c["gt"])
    for vkey in ("valid_f32", "valid_u8", "valid_bool"):
        v = dev(c[vkey])
        for tsign in (1, -1):
            preds = c["preds"](tsign)
            p = dev(preds[0])
            acc = zeros64(3)
            args = (_p(p), _p(gt), _p(v), int(vkey != "valid_f32"), R.MAX_FLOW, tsign, c["n"], _stream())
            _call("az_seq_loss_fwd", _p(acc), *args)
            info = R.check_k16_fwd(host(acc), preds[0], c["gt"], c[vkey], R.MAX_FLOW, tsign)
            report(capsys, f"az_seq_loss_fwd {c['name']} {vkey} tsign={tsign}", info)
            _call("az_seq_loss_fwd", _p(acc), *args)
            R.check_k16_fwd(host(acc), preds[0], c["gt"], c[vkey], R.MAX_FLOW, tsign, calls=2, what="az_seq_loss_fwd, two calls")
            # the wrapper: two predictions, its own weights, an upstream factor
            ps = [dev(q).requires_grad_() for q in preds]
            loss = ops.sequence_loss(ps, gt, v, loss_gamma=0.9, max_flow=R.MAX_FLOW, disparity=tsign == 1)
            weights = [0.9 ** 15.0, 1.0]
            want, lim = R.seq_loss_scalar(preds, c["gt"], c[vkey], R.MAX_FLOW, tsign, weights)
            assert loss.dtype == torch.float32 and abs(loss.item() - want) <= lim, (vkey, tsign, loss.item(), want, lim)
            (loss * 0.5).backward()
            for q, t, w in zip(preds, ps, weights):
                R.check_k16_bwd(host(t.grad), q, c["gt"], c[vkey], R.MAX_FLOW, tsign, 0.5, info["count"], w, what="ops.sequence_loss")


@pytest.mark.parametrize("k", SHAPES, ids=SHAPE_IDS)
def test_seq_loss_backward_equals_the_restatement(k, capsys):
    c = R.seq_case(R.MAP_SHAPES[k], 7400 + k, nonfinite_preds=True)
    gt = dev(c["gt"])
    gloss = torch.tensor([0.5], device=DEV)
    for vkey in ("valid_f32", "valid_u8"):
        v = dev(c[vkey])
        for tsign in (1, -1):
            pred = c["preds"](tsign)[1]
            p = dev(pred)
            count = R.k16_fwd(pred, c["gt"], c[vkey], R.MAX_FLOW, tsign)[1]
            acc = torch.tensor([0.0, count, 0.0], dtype=torch.float64, device=DEV)
            g = torch.full_like(p, float("nan"))
            _call("az_seq_loss_bwd", _p(g), _p(p), _p(gt), _p(v), int(vkey != "valid_f32"), R.MAX_FLOW, tsign, _p(gloss), _p(acc),
                  0.9, c["n"], _stream())
            info = R.check_k16_bwd(host(g), pred, c["gt"], c[vkey], R.MAX_FLOW, tsign, 0.5, count, 0.9)
            report(capsys, f"az_seq_loss_bwd {c['name']} {vkey} tsign={tsign}: equal elements", info)


def test_seq_loss_over_an_empty_mask():
    c = R.seq_case((2, 1, 24, 40), 7490)
    nothing = np.zeros_like(c["valid_f32"])
    ps = [dev(q).requires_grad_() for q in c["preds"](-1)]
    loss = ops.sequence_loss(ps, dev(c["gt"]), dev(nothing))
    assert math.isnan(float(loss))
    loss.backward()
    for t in ps:  # every pixel invalid: 0 everywhere, whatever s = w / 0 is
        assert float(t.grad.abs().max()) == 0.0


# ---- absmax -----------------------------------------------------------------------------------------------------------
def _absmax(x):
    am = torch.full((R.AMAX_FLOATS,), 7.0, device=DEV)  # (the zeroing is included, as the header says)
    _call("az_absmax", _p(am), _p(x), x.numel(), _stream())
    return host(am)


def _absmax_multi(tensors, rows):
    amax.MultiAbsmax().run(tensors, rows)


@pytest.mark.parametrize("n", R.ABSMAX_N)
def test_absmax_bit_for_bit(n, capsys):
    seen = []
    for name, x in R.absmax_cases(n):
        xd = dev(x)
        want = R.check_absmax(_absmax(xd), x, what=f"az_absmax {name}")
        row = torch.full((R.AMAX_FLOATS,), 7.0, device=DEV)
        _absmax_multi([xd], [row])
        R.check_absmax(host(row), x, what=f"az_absmax_multi {name}")
        seen.append(f"0x{want:08x}")
    with capsys.disabled():
        print(f"\n  az_absmax, az_absmax_multi n={n}: {len(seen)} cases equal: {' '.join(seen)}", end="")


def test_absmax_refuses_a_misaligned_pointer_and_launches_nothing():
    x = dev(R.F32(np.arange(1, 42)))
    am = torch.full((R.AMAX_FLOATS,), 7.0, device=DEV)
    assert x.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match="AZ_EINVAL"):
        _call("az_absmax", _p(am), x.data_ptr() + 4, 40, _stream())
    torch.cuda.synchronize()
    assert bool((am == 7.0).all()), "the refused call wrote its output"


def test_absmax_multi_takes_ragged_tensors_in_one_launch(capsys):
    """several tensors of ragged lengths, one of them 4 bytes off 16-byte alignment (a float's alignment suffices), rows that
    are not adjacent: each row equals az_absmax of its tensor, and the rows between them are not touched"""
    lengths = (1, 2, 3, 255, 256, 257, 1021, 70001, 5)
    xs = [seeded((n,), 7600 + i, -2.0 - i, 2.0 + i).numpy() for i, n in enumerate(lengths)]
    xs[3][7], xs[4][255], xs[6][1020], xs[7][256 * 17] = np.inf, np.nan, -99.5, 1e30
    xs[8][:] = np.nan
    holder = dev(np.concatenate([[0.0], xs[5]]).astype(np.float32))
    ts = [dev(x) for x in xs]
    ts[5] = holder[1:]
    assert ts[5].data_ptr() % 16 == 4
    rows = torch.full((2 * len(ts), R.AMAX_FLOATS), 7.0, device=DEV)
    _absmax_multi(ts, [rows[2 * i] for i in range(len(ts))])
    out = host(rows)
    got = []
    for i, x in enumerate(xs):
        got.append(R.check_absmax(out[2 * i], x, what=f"az_absmax_multi tensor {i} (n = {x.size})"))
        assert got[-1] == R.amax_read(_absmax(ts[i] if i != 5 else dev(x)))
        assert (out[2 * i + 1] == 7.0).all(), "a row of no descriptor was written"
    with capsys.disabled():
        print(f"\n  az_absmax_multi, {len(ts)} tensors in one launch: " + " ".join(f"0x{g:08x}" for g in got), end="")


# ---- the weights' amax ------------------------------------------------------------------------------------------------
BAD = {"finite": None, "one inf": float("inf"), "one NaN": float("nan"), "all zero": 0.0}
CO_BAD, CI_BAD = 5, 9


def _weight(shape, seed, kind):
    w = seeded(shape, seed, -0.2, 0.2)
    if kind == "all zero":
        w.zero_()
    elif BAD[kind] is not None:
        w[(CO_BAD, CI_BAD) + tuple(s // 2 for s in shape[2:])] = BAD[kind]  # the centre tap: every output of channel CO_BAD reads it
    return w


def _bump(p):
    with torch.no_grad():
        p.mul_(1.0)  # same values, next version: what an optimizer step does to the caches


@pytest.mark.parametrize("kind", list(BAD))
def test_weight_amax_is_az_absmax_of_the_weight_on_every_route(kind):
    ws = [torch.nn.Parameter(_weight(s, 7700 + i, kind).to(DEV)) for i, s in enumerate(((32, 32, 3, 3, 3), (64, 64, 3, 3), (12, 40, 1, 1)))]
    want = [R.amax_read(_absmax(w.detach())) for w in ws]
    assert want == [R.absmax_bits(host(w)) for w in ws]
    amax.prime_weight_amax(ws)
    for w, bits in zip(ws, want):
        assert R.amax_read(host(amax.weight_amax(w, w.detach()))) == bits, "prime_weight_amax"
    plan = packing.PackPlan(DEV)
    plan.prepack(ws)
    for w in ws:  # an image per weight, so that the next prepack has something stale
        taps = w[0, 0].numel()
        e, _ = plan.lookup(w, packing.PACK_2D_SAME, 64, 64, w.shape[1], w.shape[0], w.shape[1] * taps, taps, taps, False)
        assert e is not None
    for round_ in range(2):  # the second round rewrites the persistent rows in place
        plan.prepack(ws)
        for w, bits in zip(ws, want):
            assert R.amax_read(host(plan.amax_rows[w.data_ptr()][0])) == bits, "PackPlan.prepack"
            assert R.amax_read(host(amax.weight_amax(w, w.detach()))) == bits
        for w in ws:
            _bump(w)


def _layer3d(x, w):
    return conv3d._conv(x, w, conv3d.CONV_S1, conv3d.F16X3).permute(0, 4, 1, 2, 3)


def _layer2d(x, w):
    return conv2d._run_same(x, x, w, 64, 64, 3, 3, 1, False, True).permute(0, 3, 1, 2)


LAYERS = {"conv3d 32->32": ((32, 32, 3, 3, 3), (1, 32, 6, 16, 32), _layer3d, F.conv3d),
          "conv2d 64->64": ((64, 64, 3, 3), (1, 64, 16, 24), _layer2d, F.conv2d)}


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("layer", list(LAYERS))
def test_a_bad_weight_spoils_its_own_output_channel_only(layer, kind, capsys):
    """the default route: the parameter is registered with the pack plan; its first forward takes the amax from
    prime_weight_amax and packs per call, the next one -- after an optimizer step -- from PackPlan.prepack's rows and
    az_pack_f16_multi.  Yardstick: torch's fp64 convolution on the CPU under the bound of tests/test_gpu_f16x3_contract.py"""
    wshape, xshape, run, conv = LAYERS[layer]
    w = _weight(wshape, 7800, kind)
    x = seeded(xshape, 7801)
    keep = torch.ones(wshape[0], dtype=torch.bool)
    if kind in ("one inf", "one NaN"):
        keep[CO_BAD] = False
    x64, w64 = x.double(), w.double()[keep]
    ref = conv(x64, w64, padding=1)
    s_ab = conv(x64.abs(), w64.abs(), padding=1)
    sum_b = conv(torch.ones_like(x64), w64.abs(), padding=1)
    sum_a = conv(x64.abs(), torch.ones_like(w64), padding=1)
    lim = contract_bound(s_ab, sum_b, sum_a, float(x.abs().max()), NF.finite_amax(w))
    prm = torch.nn.Parameter(w.to(DEV))
    xg = x.permute(0, *range(2, x.dim()), 1).contiguous().to(DEV)  # channels last
    with torch.no_grad():
        for route in ("prime_weight_amax", "PackPlan.prepack"):
            packing.prepack([prm])
            amax.prime_weight_amax([prm])
            got = run(xg, prm).double().cpu()
            err = (got[:, keep] - ref).abs()
            worst = float((err / lim.clamp_min(1e-300)).max())
            with capsys.disabled():
                print(f"\n  {layer}, weights {kind}, amax by {route}: max err/bound {worst:.3f} over {int(keep.sum())} channels; "
                      f"{int((~torch.isfinite(got[:, ~keep])).sum())} of {got[:, ~keep].numel()} outputs of the bad channel non-finite", end="")
            assert torch.isfinite(got[:, keep]).all(), route
            assert worst <= 1.0, (route, worst)
            if kind == "all zero":
                assert float(got.abs().max()) == 0.0
            else:
                assert float(got[:, keep].abs().max()) > 0.1, "the channels that do not read the bad weight lost their values"
            assert not torch.isfinite(got[:, ~keep]).any(), "an output that reads the bad weight stayed finite"
            _bump(prm)
    plan = packing.pack_plan(DEV)
    assert any(e.wref() is prm and e.version >= 0 for e in plan.entries.values()), "the layer did not go through the plan"


def test_the_weights_amax_costs_no_host_synchronisation_and_no_launch_per_weight(monkeypatch):
    shapes = ((32, 32, 3, 3, 3), (64, 64, 3, 3, 3), (64, 64, 3, 3), (128, 320, 3, 3))
    planned = [torch.nn.Parameter(seeded(s, 7900 + i, -0.3, 0.3).to(DEV)) for i, s in enumerate(shapes)]
    loose = [torch.nn.Parameter(seeded(s, 7950 + i, -0.3, 0.3).to(DEV)) for i, s in enumerate(shapes)]
    plan = packing.PackPlan(DEV)
    plan.prepack(planned)
    for w in planned:
        taps = w[0, 0].numel()
        plan.lookup(w, packing.PACK_2D_SAME, w.shape[1], w.shape[0], w.shape[1], w.shape[0], w.shape[1] * taps, taps, taps, False)
    plan.prepack(planned)          # first time: the tables are uploaded
    amax.prime_weight_amax(loose)
    calls = []
    real = ops._call
    monkeypatch.setattr(packing, "_call", lambda name, *a: (calls.append(name), real(name, *a)))
    monkeypatch.setattr(amax, "_call", lambda name, *a: (calls.append(name), real(name, *a)))
    for w in planned + loose:
        _bump(w)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        plan.prepack(planned)
        amax.prime_weight_amax(loose)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == ["az_absmax_multi", "az_pack_f16_multi", "az_absmax_multi"], calls
    for w in planned + loose:
        assert R.amax_read(host(amax.weight_amax(w, w.detach()))) == R.absmax_bits(host(w))
    assert calls[3:] == [], "a cached weight amax was taken again"
