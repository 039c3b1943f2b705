"""GPU: NaN, +inf and -inf through every fused ReLU and clamp of the library, against torch in fp64 -- by class, not by value.

The fp64 tests of the kernels feed finite data; tests/test_gpu_f16x3_contract.py feeds non-finite operands to raw convolutions
only.  A ReLU written fmaxf(y, 0) (v_max_f32: the operand that is NOT NaN) turns a NaN into 0, a floor of -inf turns it into
-inf, and a clamp written fminf(fmaxf(..)) turns it into a bound: a diverged step then trains on with a finite loss where the
reference reports NaN.  The rule every case below holds the kernels to (include/azhip.h, "Non-finite values"): a NaN read by an
output is a NaN in that output, through every fused activation; what an inf becomes is the reference's point-wise result
(relu(-inf) = 0, clip(inf, 0, 100) = 100); an output that read nothing poisoned holds the bits of the launch on clean operands.

No tolerance anywhere: every assertion is equality of class maps (tests/_nonfinite.py: finite / NaN / +inf / -inf) or equality
of bits; every case prints its class counts before it asserts.  The launch helpers, route tables and operands are those of the
fp64 test files; each convolution case asserts the route it takes as those files do."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import agg3d, amax, bn2d, conv2d, conv3d, ops  # noqa: E402
from activezero_amd.nets.psmnet import psmnet_3 as psm3  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from activezero_amd.utils import cascade_metrics as cm  # noqa: E402
from oracle import metrics_oracle as mo  # noqa: E402
from oracle import psmnet_oracle as po  # noqa: E402
from tests import _bn_fp64ref as BR  # noqa: E402
from tests import _c1_fp64ref as C1  # noqa: E402
from tests import _nonfinite as NF  # noqa: E402
from tests import _raft_head_ref as RH  # noqa: E402
from tests import _softargmin_fp64ref as SR  # noqa: E402
from tests import test_gpu_c1_fp64 as TC1  # noqa: E402
from tests import test_gpu_conv2d_fp64 as C2  # noqa: E402
from tests import test_gpu_conv3d_s1 as S1  # noqa: E402
from tests import test_gpu_conv3d_s2 as S2  # noqa: E402
from tests.test_gpu_bn_fp64 import EPS, MOM  # noqa: E402
from tests._weights import load_procedural, seeded  # noqa: E402

DEV = torch.device("cuda:0")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def shown(test):
    """the class counts every check prints are part of the run's output, pass or fail: the test's body runs with capture
    disabled (as `with capsys.disabled():` around it would, without the indentation)"""
    sig = inspect.signature(test)

    def run(*args, capsys, **kwargs):
        with capsys.disabled():
            return test(*args, **kwargs)

    run.__name__, run.__doc__, run.__module__, run.__qualname__ = test.__name__, test.__doc__, test.__module__, test.__qualname__
    run.__signature__ = sig.replace(parameters=[*sig.parameters.values(), inspect.Parameter("capsys", inspect.Parameter.KEYWORD_ONLY)])
    return run


# ---- (a) the point-wise kernels through the C ABI ---------------------------------------------------------------------------------
# (the call patterns of k_apply / k_fwd2d of tests/test_gpu_bn_fp64.py; those assert a finite maximum, these the amax contract)
def _amax_holds(am, y, what):
    assert float(am[::64].max()) == NF.finite_amax(y), (what, "the amax array is not the largest finite magnitude stored")


def launch_apply(x, scale, shift, res, relu):
    _, V, C = x.shape
    y = torch.full_like(x, 7.0)
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_bn3d_apply", _p(y), _p(x), _p(scale), _p(shift), _p(res), int(relu), V, C, _p(am), _stream())
    _amax_holds(am, y, "az_bn3d_apply")
    return y


def launch_add_relu(a, b, relu):
    y = torch.full_like(a, 7.0)
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_add_relu", _p(y), _p(a), _p(b), int(relu), a.numel(), _p(am), _stream())
    _amax_holds(am, y, "az_add_relu")
    return y


def launch_fwd2d(x, res, gamma, beta, relu):
    """az_bn2d_fwd -> y, the four statistics outputs [G, C] and the two running statistics"""
    G, V, C = x.shape
    wsb = S1.lib().az_bn2d_workspace(G, V, C)
    ws = torch.full((wsb // 4,), NAN, device=DEV)
    y = torch.full_like(x, 7.0)
    o = torch.full((4, G, C), 7.0, device=DEV)
    rm, rv = torch.linspace(-1.0, 1.0, C, device=DEV), torch.linspace(0.5, 2.0, C, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
    _call("az_bn2d_fwd", _p(y), _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]), _p(rm), _p(rv), _p(x), _p(res), _p(gamma), _p(beta), _p(ws), wsb,
          int(relu), G, V, C, EPS, MOM, _p(nbt), None, None, 0, _p(am), _stream())
    _amax_holds(am, y, "az_bn2d_fwd")
    assert int(nbt) == G
    return y, {"mean": o[0], "invstd": o[1], "scale": o[2], "shift": o[3], "running_mean": rm, "running_var": rv}


X_BAD = ((3, 4, NAN), (-1, 6, INF), (20, 8, -INF))       # (voxel, channel, value) planted in x ...
RES_BAD = ((7, 10, NAN), (11, 12, INF), (-1, 14, -INF))  # ... and in the residual: other channels, the last voxel among them
SCALE_NAN_CH, SHIFT_NINF_CH = 16, 18


def plant(t, spots, group=0):
    t = t.clone()
    for v, c, val in spots:
        t[group, v, c] = val
    return t


def pointwise_ref(x, scale, shift, res, relu):
    """relu?(x * scale + shift + res) by torch in fp64 (F.relu keeps a NaN, relu(-inf) = 0)"""
    y = x.double().cpu() * scale.double().cpu()[:, None, :] + shift.double().cpu()[:, None, :]
    if res is not None:
        y = y + res.double().cpu()
    return F.relu(y) if relu else y


def nothing_poisoned(x, scale, shift, res):
    """the elements whose x, residual, scale and shift are all finite"""
    ok = torch.isfinite(x) & (torch.isfinite(scale) & torch.isfinite(shift))[:, None, :]
    return (ok if res is None else ok & torch.isfinite(res)).cpu()


def _apply_case(C, V, relu, with_res, what):
    x, _, res, gamma, beta = BR.make_inputs(1, V, C, 9100 + C, device=DEV)
    res = res if with_res else None
    sc, sh = gamma.view(1, C).contiguous(), beta.view(1, C).contiguous()
    clean = launch_apply(x, sc, sh, res, relu)
    xb, rb = plant(x, X_BAD), (plant(res, RES_BAD) if with_res else None)
    scb, shb = sc.clone(), sh.clone()
    scb[0, SCALE_NAN_CH], shb[0, SHIFT_NINF_CH] = NAN, -INF
    got = launch_apply(xb, scb, shb, rb, relu)
    NF.same_classes(got, pointwise_ref(xb, scb, shb, rb, relu), what)
    NF.untouched(got, clean, nothing_poisoned(xb, scb, shb, rb), what)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("C", BR.CHANNELS)
@shown
def test_bn3d_apply_keeps_nan_and_maps_inf_as_fp64_does(C, relu, with_res):
    """37 voxels: a ragged last block for every channel count"""
    assert 37 % BR.vpb(C) != 0
    _apply_case(C, 37, relu, with_res, f"az_bn3d_apply C={C} relu={relu} res={with_res}")


@shown
def test_bn3d_apply_on_a_grid_that_walks():
    """more float4 items than 4096 blocks of 256 hold: the grid-stride loop runs, the last voxel is poisoned"""
    C, V = 32, 131075
    assert "apply_trips" in BR.regimes(V, C) and V * C // 4 > BR.GRID_CAP * 256
    _apply_case(C, V, True, True, f"az_bn3d_apply C={C} nvox={V} relu res")


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("C", BR.CHANNELS)
@shown
def test_add_relu_keeps_nan_and_maps_inf_as_fp64_does(C, relu):
    V = 37
    a, _, b, _, _ = BR.make_inputs(1, V, C, 9200 + C, device=DEV)
    clean = launch_add_relu(a, b, relu)
    ab, bb = plant(a, X_BAD), plant(b, RES_BAD)
    got = launch_add_relu(ab, bb, relu)
    ref = ab.double().cpu() + bb.double().cpu()
    what = f"az_add_relu C={C} relu={relu}"
    NF.same_classes(got, F.relu(ref) if relu else ref, what)
    NF.untouched(got, clean, (torch.isfinite(ab) & torch.isfinite(bb)).cpu(), what)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@shown
def test_bn2d_fwd_poison_stays_in_its_statistic_group(relu):
    """two statistic groups, group 0 poisoned (x, residual, a NaN gamma, a -inf beta): its output has the classes of
    relu?(x * scale + shift + res) in fp64 for the (scale, shift) the launch itself returns, the NaN channels' statistics
    are NaN, and group 1 -- output and the four statistics outputs -- holds the clean launch's bits"""
    G, V, C = 2, 37, 64
    x, _, res, gamma, beta = BR.make_inputs(G, V, C, 9300, device=DEV)
    clean, cfin = launch_fwd2d(x, res, gamma, beta, relu)
    xb, rb = plant(x, X_BAD), plant(res, RES_BAD)
    got, fin = launch_fwd2d(xb, rb, gamma, beta, relu)
    what = f"az_bn2d_fwd G=2 relu={relu}"
    NF.same_classes(got, pointwise_ref(xb, fin["scale"], fin["shift"], rb, relu), what)
    nan_ch = X_BAD[0][1]
    for k in ("mean", "invstd", "scale", "shift"):
        assert bool(torch.isnan(fin[k][0, nan_ch])), (k, "of the channel that holds a NaN is not NaN")
        NF.untouched(fin[k][1:], cfin[k][1:], torch.ones(1, C, dtype=torch.bool), f"{what} {k} of group 1")
    NF.untouched(got[1:], clean[1:], torch.ones(1, V, C, dtype=torch.bool), f"{what} group 1")
    # group 0: the channels nothing was planted in, and in them the elements the residual's poison is not at
    keep = nothing_poisoned(xb, torch.ones(G, C, device=DEV), torch.ones(G, C, device=DEV), rb)
    for _, c, _ in X_BAD:
        keep[0, :, c] = False
    NF.untouched(got, clean, keep, f"{what} unpoisoned channels")

    # the same with the poison in gamma / beta: point-wise again, both groups read them
    gb, bb = gamma.clone(), beta.clone()
    gb[SCALE_NAN_CH], bb[SHIFT_NINF_CH] = NAN, -INF
    got, fin = launch_fwd2d(x, res, gb, bb, relu)
    NF.same_classes(got, pointwise_ref(x, fin["scale"], fin["shift"], res, relu), what + " NaN gamma, -inf beta")
    assert bool(torch.isnan(got[:, :, SCALE_NAN_CH]).all())
    keep = torch.ones(G, V, C, dtype=torch.bool)
    keep[:, :, SCALE_NAN_CH] = keep[:, :, SHIFT_NINF_CH] = False
    NF.untouched(got, clean, keep, what + " NaN gamma, -inf beta")


@shown
def test_bn_backward_masks_agree_on_a_nan_forward_value():
    """the backward's ReLU mask is `value > 0` of the saved output or of the recomputed x * scale + shift: false for a NaN in
    either form, so the two launches mask the same elements now that the forward stores the NaN (it stored 0 before)"""
    C, V = 32, 37
    x, dy, _, gamma, beta = BR.make_inputs(1, V, C, 9350, device=DEV)
    mean, invstd = BR.moments32(x, EPS)
    sc = (gamma * invstd).contiguous()
    sh = (beta - mean * sc).contiguous()
    v, c, _ = X_BAD[0]
    xb = plant(x, X_BAD[:1])
    y = launch_apply(xb, sc, sh, None, True)
    assert bool(torch.isnan(y[0, v, c])) and int(torch.isnan(y).sum()) == 1

    def dz_of(y_, sc_, sh_):
        wsb = S1.lib().az_bn3d_bwd_workspace(V, C)
        ws, dx, dz = torch.empty(wsb // 4, device=DEV), torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        dg, db, coef = (torch.empty(n, device=DEV) for n in (C, C, 3 * C))
        am = torch.zeros(amax.AMAX_SLOTS, device=DEV)
        _call("az_bn3d_bwd", _p(dx), _p(dz), _p(dg), _p(db), _p(coef), _p(ws), wsb, _p(dy), _p(y_), _p(xb), _p(mean), _p(invstd), _p(gamma),
              _p(sc_), _p(sh_), 1, V, C, _p(am), 0, _stream())
        return dz

    saved, remask = dz_of(y, None, None), dz_of(None, sc, sh)
    print(f"\n  az_bn3d_bwd dz at the NaN element: saved y {float(saved[0, v, c])}, recomputed {float(remask[0, v, c])}", end="")
    assert torch.equal(saved.view(torch.int32), remask.view(torch.int32))
    assert float(saved[0, v, c]) == 0.0 and bool(torch.isfinite(saved).all())


# ---- (b) train-mode BatchNorm end to end: statistics, finalize, apply ------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@shown
def test_train_mode_bn2d_spreads_a_nan_over_its_channel(relu):
    """one NaN in one channel: the whole output channel, its mean, invstd and running statistics are NaN -- as
    F.relu(BatchNorm2d(C).double().train()(x)) has it -- and every other channel holds the clean run's bits"""
    n, C, h, w, ch = 2, 64, 9, 11, 20
    x = seeded((n, C, h, w), 9400)
    xb = x.clone()
    xb[1, ch, 4, 5] = NAN
    gamma, beta = seeded((C,), 9401, 0.5, 1.5), seeded((C,), 9402, -0.5, 0.5)

    def run(t):
        bn = torch.nn.BatchNorm2d(C).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        y = bn2d.bn_act(t.to(DEV).contiguous(memory_format=torch.channels_last), bn, relu=relu)
        return y.detach().contiguous(), bn

    clean, bn_c = run(x)
    got, bn_g = run(xb)
    ref_bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        ref_bn.weight.copy_(gamma)
        ref_bn.bias.copy_(beta)
        ref = ref_bn(xb.double())
        ref = F.relu(ref) if relu else ref
    what = f"bn2d.bn_act train relu={relu}"
    NF.same_classes(got, ref, what)
    assert bool(torch.isnan(got[:, ch]).all()) and bool(torch.isnan(ref[:, ch]).all())
    others = torch.ones(1, C, 1, 1, dtype=torch.bool)
    others[0, ch] = False
    NF.untouched(got, clean, others, what)
    for k in ("running_mean", "running_var"):
        NF.same_classes(getattr(bn_g, k), getattr(ref_bn, k), f"{what} {k}")
        NF.untouched(getattr(bn_g, k), getattr(bn_c, k), others.view(C), f"{what} {k}")
    # mean and invstd of the same layer through the C ABI
    rows_ = lambda t: t.permute(0, 2, 3, 1).reshape(1, n * h * w, C).contiguous().to(DEV)  # noqa: E731
    y2, fin = launch_fwd2d(rows_(xb), None, gamma.to(DEV), beta.to(DEV), relu)
    assert torch.equal(NF.classes(y2.view(n, h, w, C).permute(0, 3, 1, 2)).cpu(), NF.classes(got).cpu())
    for k in ("mean", "invstd", "running_mean", "running_var"):
        m = torch.isnan(fin[k]).view(C).cpu()
        print(f"\n  {what} {k}: NaN in channels {m.nonzero().view(-1).tolist()}", end="")
        assert torch.equal(m, ~others.view(C)), k


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@shown
def test_train_mode_convbn3d_unit_turns_nan_everywhere(relu):
    """one NaN in one input channel of a convbn_3d unit in .train(): the convolution puts it into every output channel and
    train-mode BatchNorm spreads it over each of them, as F.relu(BatchNorm3d(conv3d(x))) in fp64 has it; the running
    statistics are NaN"""
    unit = load_procedural(psm3.convbn_3d(32, 32, 3, 1, 1), "t.cb.").to(DEV).train()
    ref_unit = load_procedural(po._cb3(32, 32, 1), "t.cb.").double().train()
    x = seeded((2, 32, 5, 6, 18), 9410)
    x[0, 7, 2, 3, 9] = NAN
    y = S1.ncdhw(agg3d.conv_bn(S1.cl(x), unit, relu=relu))
    with torch.no_grad():
        ref = ref_unit(x.double())
        ref = F.relu(ref) if relu else ref
    what = f"convbn_3d train relu={relu}"
    NF.same_classes(y, ref, what)
    assert bool(torch.isnan(y).all())
    for k in ("running_mean", "running_var"):
        NF.same_classes(getattr(unit[1], k), getattr(ref_unit[1], k), f"{what} {k}")
        assert bool(torch.isnan(getattr(unit[1], k)).all())


# ---- (c) the convolution epilogues on every forward route ---------------------------------------------------------------------------
def _corners(spatial):
    first, last = tuple(0 for _ in spatial), tuple(n - 1 for n in spatial)
    return first, tuple(n // 2 for n in spatial), last


def epilogue_case(what, x, launch, conv64, fn, sc, sh, relu):
    """injection A and injection B on one route.  x: the input (NC.. on the CPU); launch(x, res) -> the output in the
    reference's layout; conv64: the fp64 convolution of x; fn: the layer's fp64 torch operator (for NF.reads); sc, sh: the
    epilogue's affine map (None: the launch has none)"""
    b = conv64.shape[0]
    res = seeded(tuple(conv64.shape), 9500) * 0.5
    clean = launch(x, res)
    # A: NaN, +inf, -inf in the residual at three voxels (every channel): the last voxel of the last image -- in the ragged
    # last tile row and column --, the first voxel, one in the middle
    first, mid, last = _corners(conv64.shape[2:])
    bad = res.clone()
    bad[(b - 1, slice(None)) + last] = NAN
    bad[(0, slice(None)) + first] = INF
    bad[(0, slice(None)) + mid] = -INF
    y = conv64 if sc is None else conv64 * sc.double().view((1, -1) + (1,) * (conv64.dim() - 2)) + sh.double().view((1, -1) + (1,) * (conv64.dim() - 2))
    ref = y + bad.double()
    got = launch(x, bad)
    NF.same_classes(got, F.relu(ref) if relu else ref, what + " A (residual)")
    NF.untouched(got, clean, torch.isfinite(bad), what + " A (residual)")
    # B: a NaN in the input at an interior voxel and at a corner voxel, one channel each
    first, mid, last = _corners(x.shape[2:])
    xb = x.clone()
    xb[(0, 3) + mid] = NAN
    xb[(x.shape[0] - 1, 5) + last] = NAN
    r = NF.reads(torch.isnan(xb).any(1, keepdim=True), fn)
    assert tuple(r.shape[2:]) == tuple(conv64.shape[2:]) and 0 < int(r.sum()) < r.numel()
    got = launch(xb, res)
    NF.all_nan(got, r, what + " B (input)")
    NF.untouched(got, clean, ~r, what + " B (input)")


def _affine(cout, seed):
    sc, sh = seeded((cout,), seed) * 0.5 + 1.0, seeded((cout,), seed + 1) * 0.3
    sc[::5] *= -1.0
    return sc, sh


ARITHS = ("f16x3", "bf16x6", "fp32")
RELU_IDS = {False: "linear", True: "relu"}
S1_SHAPE = (1, 5, 7, 19)                         # a second half patch that is partly outside, ragged rows and columns
# the transposed layers read (2, 3, 4, 17); the stride-2 layers WRITE it (their bf16x6 / fp32 wrapper refuses odd input sizes)
T2_COARSE, S2_FINE = (2, 3, 4, 17), (2, 6, 8, 34)
# the smallest ragged shape of the 2-D sweep that has the three voxels injection A needs (the one-pixel shape has not)
C2_SHAPE = (2, 13, 22)
assert S1_SHAPE in S1.SMALL and T2_COARSE in S2.T2_COARSE and S2_FINE == S2.fine_of(T2_COARSE)
assert C2_SHAPE == min((s for s in C2.SMALL if (s[1] % 8 or s[2] % 16) and s[1] * s[2] >= 3), key=lambda s: s[0] * s[1] * s[2])
S1_EPI = [(ci, co, a, r) for (ci, co) in S1.PAIRS for a in ARITHS for r in (False, True)]
S2_EPI = [(t, ci, co, a, r) for t in (False, True) for (ci, co) in S2.PAIRS for a in ARITHS for r in (False, True)]
CONV3 = lambda stride: (lambda m, w: F.conv3d(m, w, stride=stride, padding=1))  # noqa: E731
DECONV3 = lambda m, w: F.conv_transpose3d(m, w, stride=2, padding=1, output_padding=1)  # noqa: E731
CONV2 = lambda m, w: F.conv2d(m, w, padding=1)  # noqa: E731


@pytest.mark.parametrize("cin,cout,arith,relu", S1_EPI, ids=[f"{ci}x{co}-{a}-{RELU_IDS[r]}" for (ci, co, a, r) in S1_EPI])
@shown
def test_conv3d_s1_epilogues(cin, cout, arith, relu):
    x, wt, _ = S1.operands(cin, cout, S1_SHAPE)
    name = S1.route("fwd", cin, cout, arith, S1_SHAPE)
    sc, sh = _affine(cout, 9510)
    wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)

    def launch(xv, res):
        with torch.no_grad():
            return S1.ncdhw(conv3d._conv(S1.cl(xv), wd, conv3d.CONV_S1, S1.PREC[arith], scale=scd, shift=shd, residual=S1.cl(res),
                                         relu=relu))

    epilogue_case(f"s1 {cin}->{cout} {arith} relu={relu} [{name}]", x, launch, S1.reference("fwd", cin, cout, S1_SHAPE)["y"].cpu(),
                  CONV3(1), sc, sh, relu)


@pytest.mark.parametrize("transposed,cin,cout,arith,relu", S2_EPI,
                         ids=[f"{'t2' if t else 's2'}-{ci}x{co}-{a}-{RELU_IDS[r]}" for (t, ci, co, a, r) in S2_EPI])
@shown
def test_conv3d_s2_epilogues(transposed, cin, cout, arith, relu):
    shape = T2_COARSE if transposed else S2_FINE
    x, wt, _ = S2.operands(transposed, cin, cout, shape)
    name = S2.route("fwd", transposed, cin, cout, arith, shape)
    sc, sh = _affine(cout, 9520)
    wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)

    def launch(xv, res):
        return S2.run("fwd", transposed, cin, cout, arith, S2.cl(xv), wd, None, residual=S2.cl(res), scale=scd, shift=shd, relu=relu)

    epilogue_case(f"{'t2' if transposed else 's2'} {cin}->{cout} {arith} relu={relu} [{name}]", x, launch,
                  S2.reference("fwd", transposed, cin, cout, shape)["y"].cpu(), DECONV3 if transposed else CONV3(2), sc, sh, relu)


# the 2-D launches that carry an epilogue: az_conv2d_roll_fwd (bf16x6: affine + residual + ReLU), az_conv2d_roll_fwd_f16 (the
# residual only: the wrapper launches it without scale / shift / ReLU), and the generic kernel in both arithmetics
C2_EPI = [("roll", ci, co, "bf16x6", r) for (ci, co) in C2.PAIRS for r in (False, True)]
C2_EPI += [("same", ci, co, "f16x3", False) for (ci, co) in C2.PAIRS]
C2_EPI += [("generic", 128, 128, a, r) for a in C2.ARITHS for r in (False, True)]


def _c2_route(how, cin, cout, arith):
    if how == "roll":
        return C2.route_conv(cin, cout, arith, C2_SHAPE, C2.G33, "epi", force_roll=True)
    return C2.route_conv(cin, cout, arith, C2_SHAPE, C2.G33, "res" if how == "same" else "epi")


@pytest.mark.parametrize("how,cin,cout,arith,relu", C2_EPI, ids=[f"{h}-{ci}x{co}-{a}-{RELU_IDS[r]}" for (h, ci, co, a, r) in C2_EPI])
@shown
def test_conv2d_epilogues(how, cin, cout, arith, relu):
    x, wt, _ = C2.operands(cin, cout, C2_SHAPE, C2.G33)
    name = _c2_route(how, cin, cout, arith)
    sc, sh = (None, None) if how == "same" else _affine(cout, 9530)
    wd = wt.to(DEV)
    scd, shd = (None, None) if sc is None else (sc.to(DEV), sh.to(DEV))

    def launch(xv, res):
        xr, rr = C2.rows(xv), C2.rows(res)
        with torch.no_grad():
            if how == "same":
                return C2.run_conv("fwd", cin, cout, arith, C2.G33, xr, wd, res=rr)
            k = conv2d.KERNELS[f"{'roll' if how == 'roll' else 'gather'} {arith}"]
            return C2.nchw(C2.launch(k, xr, wd, cin, cout, scale=scd, shift=shd, res=rr, relu=relu))

    epilogue_case(f"2-D {cin}->{cout} {arith} relu={relu} [{name}]", x, launch,
                  C2.reference("fwd", cin, cout, C2_SHAPE, C2.G33)["y"].cpu(), CONV2, sc, sh, relu)


@shown
def test_every_forward_route_is_swept():
    """the cases above take every forward route the current switches leave to the three families (tests/test_gpu_switches.py
    runs this file again with AZ_CONV_ROLL=0: the bf16x6 32-channel layers on az_conv3d_m128.hip)"""
    names = {S1.route("fwd", ci, co, a, S1_SHAPE) for (ci, co, a, _) in S1_EPI}
    want = ["roll f16x3", "gather f16x3", "gather fp32", "gather bf16x6"] + (["roll2 f16x3"] if S1.opt("AZ_CONV_ROLL64") else [])
    want += ["roll bf16x6" if conv3d._ROLL else ("m128 bf16x6" if S1.opt("AZ_CONV_M128") else "gather bf16x6")]
    names |= {S2.route("fwd", t, ci, co, a, T2_COARSE if t else S2_FINE) for (t, ci, co, a, _) in S2_EPI}
    want += ["t2 f16x3", "gather m1 f16x3", "gather m2 f16x3", "t2 bf16x6", "gather m1 bf16x6", "gather m2 bf16x6", "gather m1 fp32",
             "gather m2 fp32"]
    want += ["s2roll f16x3"] * bool(S2.opt("AZ_CONV_S2ROLL")) + ["t2roll f16x3"] * bool(S2.opt("AZ_CONV_T2ROLL"))
    names |= {_c2_route(h, ci, co, a) for (h, ci, co, a, _) in C2_EPI}
    want += ["roll NT2 bf16x6 epi", "roll NT4 bf16x6 epi", "generic NW4 3x3d1 bf16x6 epi", "generic NW4 3x3d1 f16x3 epi"]
    want += ["roll NT2 f16x3 res", "roll64 f16x3 res"] if conv2d._ROLL2D else []
    missing = [w for w in want if not any(w in n for n in names)]
    print("\n  forward routes: " + ", ".join(sorted(names)), end="")
    assert not missing, (missing, sorted(names))
    # every rolling route has a ReLU-off case (the floor of -inf) and a ReLU-on case
    for fam in (S1_EPI, S2_EPI):
        assert {c[-1] for c in fam} == {False, True}


# ---- (d) the input-gradient launches (EPI 0 / 2 of the rolling kernels with a floor of -inf) -------------------------------------------
def dgrad_case(what, dy, res, launch, fn):
    """launch(dy, res or None) -> the input gradient in the reference's layout"""
    first, mid, last = _corners(dy.shape[2:])
    dyb = dy.clone()
    dyb[(0, 3) + mid] = NAN
    dyb[(dy.shape[0] - 1, 5) + last] = NAN
    r = NF.reads(torch.isnan(dyb).any(1, keepdim=True), fn)
    assert tuple(r.shape[2:]) == tuple(res.shape[2:]) and 0 < int(r.sum()) < r.numel()
    for rr, tag in ((None, "plain"), (res, "+residual")):
        clean = launch(dy, rr)
        got = launch(dyb, rr)
        print(f"\n  {what} {tag}: -inf in the result: {int((got == -INF).sum())}", end="")
        NF.all_nan(got, r, f"{what} {tag} NaN in dy")
        NF.untouched(got, clean, ~r, f"{what} {tag} NaN in dy")
    _, rmid, rlast = _corners(res.shape[2:])
    resb = res.clone()
    resb[(0, slice(None)) + rmid] = NAN
    resb[(res.shape[0] - 1, 7) + rlast] = NAN
    got = launch(dy, resb)
    NF.same_classes(got, resb.double(), f"{what} NaN in the residual")  # (the gradient itself is finite)
    NF.untouched(got, clean, torch.isfinite(resb), f"{what} NaN in the residual")


DGRAD_ARITHS = ("f16x3", "bf16x6")
S1_DGRAD = [(ci, co, a) for (ci, co) in S1.PAIRS for a in DGRAD_ARITHS]
S2_DGRAD = [(t, ci, co, a) for t in (False, True) for (ci, co) in S2.PAIRS for a in DGRAD_ARITHS]
C2_DGRAD = [(ci, co, a) for (ci, co) in C2.PAIRS for a in C2.ARITHS]


@pytest.mark.parametrize("cin,cout,arith", S1_DGRAD, ids=[f"{ci}x{co}-{a}" for (ci, co, a) in S1_DGRAD])
@shown
def test_conv3d_s1_input_gradient(cin, cout, arith):
    _, wt, dy = S1.operands(cin, cout, S1_SHAPE)
    name = S1.route("dgrad", cin, cout, arith, S1_SHAPE)
    res = seeded((S1_SHAPE[0], cin) + S1_SHAPE[1:], 9600) * 1e-2
    wd = wt.to(DEV)
    launch = lambda g, r: S1.run("dgrad", cin, cout, arith, None, wd, S1.cl(g), residual=None if r is None else S1.cl(r))  # noqa: E731
    dgrad_case(f"s1 dgrad {cin}->{cout} {arith} [{name}]", dy, res, launch, CONV3(1))


@pytest.mark.parametrize("transposed,cin,cout,arith", S2_DGRAD, ids=[f"{'t2' if t else 's2'}-{ci}x{co}-{a}" for (t, ci, co, a) in S2_DGRAD])
@shown
def test_conv3d_s2_input_gradient(transposed, cin, cout, arith):
    shape = T2_COARSE if transposed else S2_FINE
    x, wt, dy = S2.operands(transposed, cin, cout, shape)
    name = S2.route("dgrad", transposed, cin, cout, arith, shape)
    res = seeded(tuple(x.shape), 9610) * 1e-2
    wd = wt.to(DEV)
    launch = lambda g, r: S2.run("dgrad", transposed, cin, cout, arith, None, wd, S2.cl(g), residual=None if r is None else S2.cl(r))  # noqa: E731
    # (the input gradient of a stride-2 layer is the transposed map of dy, and the reverse)
    dgrad_case(f"{'t2' if transposed else 's2'} dgrad {cin}->{cout} {arith} [{name}]", dy, res, launch, CONV3(2) if transposed else DECONV3)


@pytest.mark.parametrize("cin,cout,arith", C2_DGRAD, ids=[f"{ci}x{co}-{a}" for (ci, co, a) in C2_DGRAD])
@shown
def test_conv2d_input_gradient(cin, cout, arith):
    _, wt, dy = C2.operands(cin, cout, C2_SHAPE, C2.G33)
    name = C2.route_conv(cout, cin, arith, C2_SHAPE, C2.G33, "res")
    res = seeded((C2_SHAPE[0], cin) + C2_SHAPE[1:], 9620) * 1e-2
    wd = wt.to(DEV)
    launch = lambda g, r: C2.run_conv("dgrad", cin, cout, arith, C2.G33, C2.rows(g), wd, res=None if r is None else C2.rows(r))  # noqa: E731
    dgrad_case(f"2-D dgrad {cin}->{cout} {arith} [{name}]", dy, res, launch, CONV2)


@shown
def test_the_input_gradients_run_on_the_rolling_kernels():
    names = {S1.route("dgrad", ci, co, a, S1_SHAPE) for (ci, co, a) in S1_DGRAD}
    names |= {S2.route("dgrad", t, ci, co, a, T2_COARSE if t else S2_FINE) for (t, ci, co, a) in S2_DGRAD}
    names |= {C2.route_conv(co, ci, a, C2_SHAPE, C2.G33, "res") for (ci, co, a) in C2_DGRAD}
    want = ["roll f16x3"] + ["roll2 f16x3"] * bool(S1.opt("AZ_CONV_ROLL64")) + ["roll bf16x6"] * bool(conv3d._ROLL)
    want += ["s2roll f16x3"] * bool(S2.opt("AZ_CONV_S2ROLL")) + ["t2roll f16x3"] * bool(S2.opt("AZ_CONV_T2ROLL"))
    want += ["roll NT2 bf16x6 res", "roll NT4 bf16x6 res", "roll NT2 f16x3 res", "roll64 f16x3 res"] if conv2d._ROLL2D else []
    missing = [w for w in want if not any(w in n for n in names)]
    print("\n  input-gradient routes: " + ", ".join(sorted(names)), end="")
    assert not missing, (missing, sorted(names))


# ---- (e) the classifier kernel's fused operand map relu(in * scale + shift) -------------------------------------------------------------
# the smallest shape of test_gpu_c1_fp64.REGIMES in which a voxel has all of its 27 neighbours (a NaN at it reaches all 27 taps
# of its channel's weight gradient, as the assertions below say; the one-voxel and one-row shapes have no such voxel)
C1_SHAPE = min((s for s in TC1.REGIMES if min(s[1:]) >= 3), key=lambda s: s[0] * s[1] * s[2] * s[3])
C1_VOXEL, C1_CH = (0, 2, 3, 6), 9  # (channel 9: shift <= -2, the ReLU clamps every clean value of it to 0)


def _c1_case():
    assert C1_SHAPE == (2, 5, 7, 13)
    TC1.assert_plan(C1_SHAPE)
    o = TC1.operands(C1_SHAPE)
    x = o["x"].clone()
    x[(C1_VOXEL[0], C1_CH) + C1_VOXEL[1:]] = NAN
    p64, _ = C1.operand(x, *o["affine"])  # fp64 relu(in * sc + sh): clamp_min keeps the NaN
    assert int(torch.isnan(p64).sum()) == 1
    return o, x, TC1.cl(x), p64


@shown
def test_c1_fwd_fused_operand_keeps_a_nan():
    b, d, h, w = C1_SHAPE
    o, x, xr, p64 = _c1_case()
    r = NF.reads(torch.isnan(x).any(1, keepdim=True), CONV3(1))
    out = torch.full((b * d * h * w,), 7.0, device=DEV)
    clean = torch.full_like(out, 7.0)
    _call("az_conv3d_c1_fwd", _p(clean), _p(o["xr"]), _p(o["wd"]), None, _p(o["sc"]), _p(o["sh"]), b, d, h, w, _stream())
    _call("az_conv3d_c1_fwd", _p(out), _p(xr), _p(o["wd"]), None, _p(o["sc"]), _p(o["sh"]), b, d, h, w, _stream())
    out, clean = out.view(b, 1, d, h, w), clean.view(b, 1, d, h, w)
    NF.same_classes(out, F.conv3d(p64, o["w"].double(), padding=1), "az_conv3d_c1_fwd")
    assert torch.equal(torch.isnan(out).cpu(), r) and int(r.sum()) == 27
    NF.untouched(out, clean, ~r, "az_conv3d_c1_fwd")


@shown
def test_c1_wgrad_fused_operand_keeps_a_nan():
    b, d, h, w = C1_SHAPE
    o, x, xr, p64 = _c1_case()
    gw, gw_clean = torch.full((864,), 7.0, device=DEV), torch.full((864,), 7.0, device=DEV)
    _call("az_conv3d_c1_wgrad", _p(gw_clean), _p(o["xr"]), _p(o["gr"]), _p(o["sc"]), _p(o["sh"]), b, d, h, w, _stream())
    _call("az_conv3d_c1_wgrad", _p(gw), _p(xr), _p(o["gr"]), _p(o["sc"]), _p(o["sh"]), b, d, h, w, _stream())
    gw, gw_clean = gw.view(1, 32, 3, 3, 3), gw_clean.view(1, 32, 3, 3, 3)
    ref = torch.nn.grad.conv3d_weight(p64, (1, 32, 3, 3, 3), o["dy"].double(), padding=1)
    NF.same_classes(gw, ref, "az_conv3d_c1_wgrad")
    nan = torch.isnan(gw).cpu()
    assert int(nan.sum()) == 27 and bool(nan[0, C1_CH].all())
    # (the other channels' sums are atomic: their order is not fixed, so they are compared by class only)


# ---- (f) K12: the disparity loss, its gradient and the metrics ---------------------------------------------------------------------------
K12_SHAPE = (2, 1, 9, 33)
PIX_NAN3, PIX_NAN2, PIX_NAN1 = (0, 0, 2, 5), (1, 0, 4, 20), (1, 0, 8, 32)  # a NaN prediction per head (the last pixel among them)
PIX_NAN_Z, PIX_ZERO_DISP = (0, 0, 3, 7), (1, 0, 6, 11)                     # a NaN depth_gt; disp_pred = 0: the predicted depth is inf


def _k12_inputs():
    gt = seeded(K12_SHAPE, 9700, 1.0, 30.0)
    mask = seeded(K12_SHAPE, 9701) > -0.6
    for p in (PIX_NAN3, PIX_NAN2, PIX_NAN1, PIX_NAN_Z, PIX_ZERO_DISP):
        mask[p] = True
    preds = [gt + seeded(K12_SHAPE, 9702 + k, -2.5, 2.5) for k in range(3)]
    focal, base = torch.full((2, 1, 1, 1), 450.0), torch.full((2, 1, 1, 1), 0.055)
    zg = focal * base / gt
    dp = preds[0].clamp(min=0.5)
    return gt, mask, preds, focal, base, zg, dp


def _loss_and_grads(preds, gt, mask):
    ps = [p.to(DEV).requires_grad_() for p in preds]
    loss = ops.disp_loss(*ps, gt.to(DEV), mask.to(DEV))
    return loss.detach(), [g.detach() for g in torch.autograd.grad(loss, ps)]


@shown
def test_k12_loss_and_gradient_keep_nan():
    gt, mask, preds, focal, base, zg, dp = _k12_inputs()
    bad = [p.clone() for p in preds]
    for p, pix in zip(bad, (PIX_NAN3, PIX_NAN2, PIX_NAN1)):
        p[pix] = NAN
    loss, grads = _loss_and_grads(bad, gt, mask)
    ref_p = [p.double().requires_grad_() for p in bad]
    ref_loss = po.psmnet_disp_loss(tuple(ref_p), gt.double(), mask)
    ref_g = torch.autograd.grad(ref_loss, ref_p)
    print(f"\n  loss {float(loss)} (fp64 autograd {float(ref_loss.detach())})", end="")
    assert bool(torch.isnan(loss)) and bool(torch.isnan(ref_loss))
    for k, (g, rg, pix) in enumerate(zip(grads, ref_g, (PIX_NAN3, PIX_NAN2, PIX_NAN1))):
        NF.same_classes(g, rg, f"az_disp_loss_bwd g_pred{3 - k}")
        assert bool(torch.isnan(g[pix])) and int(torch.isnan(g).sum()) == 1 and int(torch.isinf(g).sum()) == 0


@shown
def test_k12_metrics_keep_nan_and_clip_inf():
    gt, mask, preds, focal, base, zg, dp = _k12_inputs()
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731

    def both(dpv, zgv, mk):
        return (cm.compute_err_metric(dev(gt), dev(zgv), dev(dpv), dev(focal), dev(base), dev(mk)),
                mo.compute_err_metric(gt, zgv, dpv, focal, base, mk))

    def same_nan_keys(have, want, what):
        print(f"\n  {what}: NaN in {sorted(k for k in have if np.isnan(have[k]))} (oracle: {sorted(k for k in want if np.isnan(want[k]))})", end="")
        assert sorted(have) == sorted(want)
        for k in want:
            assert np.isnan(have[k]) == np.isnan(want[k]) and np.isinf(have[k]) == np.isinf(want[k]), (what, k, have[k], want[k])

    dpb, zgb = dp.clone(), zg.clone()
    dpb[PIX_NAN3], zgb[PIX_NAN_Z], dpb[PIX_ZERO_DISP] = NAN, NAN, 0.0
    have, want = both(dpb, zgb, mask)
    same_nan_keys(have, want, "metrics, NaN prediction + NaN depth_gt + zero disparity")
    assert np.isnan(have["epe"]) and np.isnan(have["depth_abs_err"])
    for k in ("bad1", "bad2", "depth_err2", "depth_err4", "depth_err8"):  # the counters: a NaN error is no error above a threshold
        assert np.isfinite(have[k]) and np.isfinite(want[k]), (k, have[k], want[k])
    # a NaN depth_gt alone: the disparity metrics stay finite, depth_abs_err is NaN (torch.clip keeps it)
    zgn = zg.clone()
    zgn[PIX_NAN_Z] = NAN
    have, want = both(dp, zgn, mask)
    same_nan_keys(have, want, "metrics, NaN depth_gt alone")
    assert np.isnan(have["depth_abs_err"]) and np.isfinite(have["epe"])
    # the zero disparity alone: every metric finite (clip(inf, 0, 100) = 100)
    dpz = dp.clone()
    dpz[PIX_ZERO_DISP] = 0.0
    have, want = both(dpz, zg, mask)
    same_nan_keys(have, want, "metrics, zero disparity alone")
    assert all(np.isfinite(v) for v in have.values())


@shown
def test_k12_masked_out_nan_changes_nothing():
    gt, mask, preds, focal, base, zg, dp = _k12_inputs()
    out = [(0, 0, 1, 1), (1, 0, 7, 30), (0, 0, 8, 0)]
    for p in out:
        mask[p] = False
    loss, grads = _loss_and_grads(preds, gt, mask)
    bad = [p.clone() for p in preds]
    dpb, zgb, gtb = dp.clone(), zg.clone(), gt.clone()
    for t, pix in zip(bad, out):
        t[pix] = NAN
    dpb[out[0]], zgb[out[1]], dpb[out[2]] = NAN, NAN, 0.0
    loss_b, grads_b = _loss_and_grads(bad, gtb, mask)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(loss.view(1)), bits(loss_b.view(1))) and bool(torch.isfinite(loss))
    for a, b_ in zip(grads, grads_b):
        assert torch.equal(bits(a), bits(b_))
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    m0 = cm.compute_err_metric(dev(gt), dev(zg), dev(dp), dev(focal), dev(base), dev(mask))
    m1 = cm.compute_err_metric(dev(gt), dev(zgb), dev(dpb), dev(focal), dev(base), dev(mask))
    print(f"\n  masked-out NaN: loss {float(loss)} / {float(loss_b)}, metrics equal: {m0 == m1}", end="")
    assert m0 == m1 and all(np.isfinite(v) for v in m0.values())


# ---- (g) pins: the soft-argmin head and convex upsampling ----------------------------------------------------------------------------
@shown
def test_softargmin_nan_logit_forward_and_backward():
    """A NaN logit at one coarse voxel.  The max searches drop it, exp(x - max) brings it back: every fine pixel whose trilinear
    footprint holds the voxel is NaN, and so is the gradient of every coarse voxel such a pixel reads.  The class maps come from
    the axis matrices of tests/_softargmin_fp64ref.py applied to the poison's indicator in fp64 (their weights are not negative;
    the matrices applied to the NaN itself would spread it over whole rows through their zero entries: 0 * NaN)."""
    B, d, h, w = 1, 8, 5, 7
    lg = seeded((B, d, h, w), 9800, -2.0, 2.0)
    bad = lg.clone()
    bad[0, 3, 2, 4] = NAN
    gout = seeded((B, 1, 4 * h, 4 * w), 9801)
    Ad, Ah, Aw = (torch.from_numpy(SR.axis_matrix(n)) for n in (d, h, w))
    ind = torch.isnan(bad).double()
    u_bad = torch.einsum("Dk,Yy,Xx,bkyx->bDYX", Ad, Ah, Aw, ind) > 0   # the upsampled logits that read the voxel
    pix_bad = u_bad.any(1, keepdim=True)                               # softmax over D: the whole pixel
    g_bad = torch.einsum("Dk,Yy,Xx,bDYX->bkyx", Ad, Ah, Aw, pix_bad.expand(B, 4 * d, 4 * h, 4 * w).double()) > 0

    def run(t):
        x = t.view(B, 1, d, h, w).to(DEV).requires_grad_()
        out = ops.softargmin(x)
        (g,) = torch.autograd.grad(out, x, gout.to(DEV))
        return out.detach(), g.detach().view(B, d, h, w)

    out_c, g_c = run(lg)
    out, g = run(bad)
    ref = SR.head(lg.numpy(), gout.numpy().reshape(B, 4 * h, 4 * w))
    nanned = lambda a, m: torch.where(m, torch.full_like(torch.from_numpy(a), NAN), torch.from_numpy(a))  # noqa: E731
    NF.same_classes(out, nanned(ref["out"][:, None], pix_bad), "az_softargmin_fwd")
    NF.untouched(out, out_c, ~pix_bad, "az_softargmin_fwd")
    # the gradient: every coarse voxel a NaN pixel reads is NaN.  The backward kernel also multiplies a quad's ZERO shares
    # (f_m1 / f_p1 of az_softargmin.hip: the x cell a pixel does not touch), so the cells one further in x may be NaN as well
    # -- a zero-weight tap of the interpolation, not a fused activation; nothing beyond that ring may change.
    ring = F.max_pool3d(g_bad.double(), (1, 1, 3), stride=1, padding=(0, 0, 1)) > 0
    NF.all_nan(g, g_bad, "az_softargmin_bwd")
    extra = torch.isnan(g).cpu() & ~g_bad
    print(f"\n  az_softargmin_bwd: {int(extra.sum())} further NaN, all within one cell in x: {not bool((extra & ~ring).any())}", end="")
    assert not bool((extra & ~ring).any()) and int(torch.isinf(g).sum()) == 0
    # (by class only: up to three tiles add to a coarse row with float atomics, the gradient's last bits depend on their order)
    zero = torch.zeros(B, d, h, w, dtype=torch.float64)
    NF.same_classes(torch.where(ring, zero, g.double().cpu()), torch.where(ring, zero, torch.from_numpy(ref["grad"])),
                    "az_softargmin_bwd outside the ring")
    assert bool(torch.isfinite(g_c).all())
    assert 0 < int(pix_bad.sum()) < pix_bad.numel() and 0 < int(g_bad.sum()) < int(ring.sum()) < g_bad.numel()


@shown
def test_convex_upsample_nan_mask_logit_forward_and_backward():
    n, h, w, f, d = 1, 5, 9, 4, 2
    flow = seeded((n, d, h, w), 9810, -3.0, 3.0)
    mask = RH.make_mask_logits((n, 9 * f * f, h, w), 9811)
    mask[0, 4 * f * f + 1 * f + 2, 2, 5] = NAN  # tap k = 4 of the subpixel (i, j) = (1, 2) of the coarse pixel (2, 5)
    cot = seeded((n, d, f * h, f * w), 9812)
    fl, mk = flow.to(DEV).requires_grad_(), mask.to(DEV).requires_grad_()
    up = ops.convex_upsample(fl, mk, f)
    gf, gm = torch.autograd.grad(up, (fl, mk), cot.to(DEV))
    fl64, mk64 = flow.double().requires_grad_(), mask.double().requires_grad_()
    up64 = RH.convex_upsample(fl64, mk64, f)
    gf64, gm64 = torch.autograd.grad(up64, (fl64, mk64), cot.double())
    NF.same_classes(up, up64, "az_convex_up_fwd")
    NF.same_classes(gf, gf64, "az_convex_up_bwd d flow")
    NF.same_classes(gm, gm64, "az_convex_up_bwd d mask")
    assert int(torch.isnan(up).sum()) == d and int(torch.isnan(gm).sum()) == 9


# ---- (h) the whole model, once ------------------------------------------------------------------------------------------------------
@shown
def test_whole_model_reports_a_nan_pixel():
    """one NaN pixel in the left image.  Train mode: the first convolution puts it into all 32 channels, train-mode BatchNorm
    spreads a channel's NaN over the whole channel: all three predictions are NaN at every pixel and so is the loss.  Eval mode:
    the output is NaN at least at that pixel."""
    from activezero_amd.utils import disp_losses
    il, ir = (seeded((1, 3, 256, 256), 9900 + i, -2.0, 2.0) for i in range(2))
    il[0, 1, 100, 131] = NAN
    gt = (1.0 + 28.0 * seeded((1, 1, 256, 256), 9902, 0.0, 1.0)).to(DEV)
    model = load_procedural(psm3.PSMNet(32), "g4.").to(DEV).train()
    preds = model(il.to(DEV), ir.to(DEV))
    loss = disp_losses.psmnet_disp(preds, gt, po.disparity_mask(gt, 32))
    print(f"\n  train: loss {float(loss.detach())}, NaN share of the predictions " + " ".join(f"{float(torch.isnan(p).float().mean()):.3f}" for p in preds),
          end="")
    assert len(preds) == 3 and all(bool(torch.isnan(p).all()) for p in preds)
    assert bool(torch.isnan(loss))
    model = load_procedural(psm3.PSMNet(32), "g4.").to(DEV).eval()
    with torch.no_grad():
        out = model(il.to(DEV), ir.to(DEV))
    print(f"\n  eval: NaN share of the output {float(torch.isnan(out).float().mean()):.3f}", end="")
    assert bool(torch.isnan(out[0, 0, 100, 131]))
