"""GPU: the 32 -> 1 classifier convolutions of az_conv3d_c1.hip -- c1_fwd_kernel (az_conv3d_c1_fwd), c1_dgrad_kernel
(az_conv3d_c1_dgrad), c1_wgrad_kernel (az_conv3d_c1_wgrad) -- element-wise against fp64, in every launch regime: forward depth
segments of one plane, of several planes with and without a ragged last segment, of the whole depth; weight-gradient workgroups
with one item and with a strided list of two; the fused BatchNorm + ReLU operand; the fused addend.

Every launch goes through the C ABI (ops._call); every output, the 864-float weight gradient too, sits between NaN sentinel
bands that must be untouched afterwards, and no output element may be left NaN.  Each case asserts the plan it is meant to reach
through az_conv3d_c1_plan (and that the restated plan of tests/_c1_fp64ref.py is the library's) and runs the three checks of
tests/_c1_fp64ref.py; tests/test_c1_error_model_cpu.py shows that those checks reject the defects they are meant to see.  The
last test prints the largest ratios per kernel and regime.

The weight gradient is also run with `in` and `grad_logits` embedded in larger buffers whose floats before and after the volume
hold 1e4.  The ABI has no strides, so only the neighbours in the flat buffer can be planted: a read before batch 0 / plane 0 or
past the last plane lands there.  A read past a tile's tail INSIDE the volume lands on real neighbours of the next row or plane,
which cannot be planted; such a read is seen by the value checks of the ragged shapes instead."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, conv3d  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _c1_fp64ref as C1  # noqa: E402
from tests import _fp64ref as R  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
BAND = 1024  # floats of a sentinel band
# shape (B, D, H, W) -> (forward dseg, forward depth segments, planes of the last segment, weight-gradient ntiles, grid)
REGIMES = {
    (1, 1, 1, 1): (1, 1, 1, 1, 1),
    (1, 2, 1, 47): (1, 2, 1, 4, 4),
    (2, 5, 7, 13): (1, 5, 1, 10, 10),
    (2, 3, 9, 17): (1, 3, 1, 12, 12),
    (1, 4, 8, 33): (1, 4, 1, 8, 8),
    (3, 5, 11, 65): (1, 5, 1, 90, 90),
    (3, 7, 40, 130): (2, 4, 1, 525, 525),        # ragged last segment: 1 of 2 planes
    (1, 20, 64, 160): (3, 7, 2, 800, 800),       # ragged last segment: 2 of 3 planes
    (1, 2050, 3, 5): (3, 684, 1, 2050, 2048),    # two workgroups of the weight gradient walk
    (768, 3, 8, 16): (3, 1, 3, 2304, 2048),      # dseg = D; blockIdx.z up to 767; 256 workgroups take two items
    (1, 48, 16, 240): (2, 24, 2, 768, 768),      # production depth and width
}
SHAPES = list(REGIMES)
SEGMENTED = [s for s in SHAPES if REGIMES[s][0] >= 2]
AFFINE_SHAPES = [(2, 5, 7, 13), (1, 4, 8, 33)] + SEGMENTED
WORST = {}  # (kernel, regime) -> [a, b, c, case of the largest (b)]


def lib():
    return _lib.lib()


def sid(s):
    return "x".join(map(str, s))


def guarded(n):
    """(whole buffer, the n floats between two NaN bands)"""
    whole = torch.full((n + 2 * BAND,), NAN, device=DEV)
    return whole, whole[BAND:BAND + n]


def bands_intact(whole, n):
    return bool(torch.isnan(whole[:BAND]).all()) and bool(torch.isnan(whole[BAND + n:]).all())


def cl(t):
    """[B,32,D,H,W] -> the kernels' channels-last [B,D,H,W,32] on the GPU"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def where(shape):
    """fp64 references of the larger cases: GEMMs on the GPU"""
    return (DEV, True) if shape[0] * shape[1] * shape[2] * shape[3] >= 50000 else ("cpu", False)


def assert_plan(shape):
    """the regime the case is meant to reach, from the library's own plan; returns (forward regime, weight-gradient regime)"""
    b, d, h, w = shape
    dseg, nseg, last, ntiles, grid = REGIMES[shape]
    out = (ctypes.c_longlong * 4)()
    assert lib().az_conv3d_c1_plan(out, *shape) == 0
    assert tuple(out) == C1.plan(shape), (tuple(out), C1.plan(shape))
    assert (out[0], out[2], out[3]) == (dseg, ntiles, grid), (shape, tuple(out))
    assert C1.segments(shape) == (nseg, last) and out[1] == b * -(-h // 8) * -(-w // 16) * nseg
    fwd = "dseg = 1" if dseg == 1 else "dseg = D" if nseg == 1 else f"dseg >= 2{', ragged last segment' if last != dseg else ''}"
    return fwd, ("walking workgroups" if ntiles > grid else "one item per workgroup")


# ---- operands and references --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def operands(shape):
    b, d, h, w = shape
    seed = 9300 + 7 * b + 3 * d + 5 * h + w
    o = dict(x=seeded((b, 32, d, h, w), seed), w=seeded((1, 32, 3, 3, 3), seed + 1, -0.3, 0.3),
             dy=seeded((b, 1, d, h, w), seed + 2) * 1e-3, addend=seeded((b, 1, d, h, w), seed + 3), affine=C1.affine_pair(seed + 4))
    o["xr"], o["gr"], o["ar"], o["wd"] = cl(o["x"]), o["dy"].to(DEV).contiguous(), o["addend"].to(DEV).contiguous(), o["w"].to(DEV)
    o["sc"], o["sh"] = o["affine"][0].to(DEV), o["affine"][1].to(DEV)
    return o


def _reference(kind, shape, affine):
    """(R.exact of the operation, the grant of the fused operand or None); read-only, shared by the tests of a shape"""
    o = operands(shape)
    dev, gemm = where(shape)
    if kind == "dgrad":
        return R.exact("dgrad", o["dy"].to(dev), o["w"].to(dev), gemm=gemm), None
    q = (o["w"] if kind == "fwd" else o["dy"]).to(dev)
    p, pre = C1.operand(o["x"].to(dev), *(o["affine"] if affine else (None, None)))
    ex = R.exact(kind, p, q, gemm=gemm)
    ex = {k: ex[k] for k in ("y", "S", "Q2")}
    return ex, (C1.operand_grant(kind, pre, q, gemm=gemm) if affine else None)


small_reference = functools.lru_cache(maxsize=None)(_reference)   # forward, weight gradient: outputs of B D H W and 864 values
dgrad_reference = functools.lru_cache(maxsize=1)(_reference)      # 32 B D H W values


def reference(kind, shape, affine=False):
    return dgrad_reference(kind, shape, affine) if kind == "dgrad" else small_reference(kind, shape, affine)


def record(kernel, regime, label, r, capsys):
    w = WORST.setdefault((kernel, regime), [0.0, 0.0, 0.0, ""])
    if r[1] >= w[1]:
        w[3] = label
    w[:3] = [max(u, v) for u, v in zip(w, r)]
    with capsys.disabled():
        print(f"\n{label}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")


# ---- launches through the C ABI -----------------------------------------------------------------------------------------------------
def run_fwd(shape, xr, wd, addend=None, sc=None, sh=None):
    b, d, h, w = shape
    n = b * d * h * w
    whole, out = guarded(n)
    _call("az_conv3d_c1_fwd", _p(out), _p(xr), _p(wd), _p(addend), _p(sc), _p(sh), b, d, h, w, _stream())
    torch.cuda.synchronize()
    assert bands_intact(whole, n), "the forward wrote outside its output"
    assert not bool(torch.isnan(out).any()), "a logit was not written"
    return out.view(b, 1, d, h, w)


def run_dgrad(shape, gr, wd):
    b, d, h, w = shape
    n = b * d * h * w * 32
    whole, out = guarded(n)
    _call("az_conv3d_c1_dgrad", _p(out), _p(gr), _p(wd), b, d, h, w, _stream())
    torch.cuda.synchronize()
    assert bands_intact(whole, n), "the input gradient wrote outside its output"
    assert not bool(torch.isnan(out).any()), "an input-gradient element was not written"
    return out.view(b, d, h, w, 32).permute(0, 4, 1, 2, 3)


def run_wgrad(shape, xr, gr, sc=None, sh=None):
    b, d, h, w = shape
    whole, out = guarded(864)
    _call("az_conv3d_c1_wgrad", _p(out), _p(xr), _p(gr), _p(sc), _p(sh), b, d, h, w, _stream())
    torch.cuda.synchronize()
    assert bands_intact(whole, 864), "the weight gradient wrote outside its 864 floats"
    assert not bool(torch.isnan(out).any())
    return out.view(1, 32, 3, 3, 3)


def embedded(t, fill=1.0e4):
    """t's floats with as many floats of `fill` before and behind them (what a read outside the tensor would find)"""
    n = t.numel()
    whole = torch.full((3 * n,), fill, device=DEV)
    whole[n:2 * n] = t.reshape(-1)
    return whole[n:2 * n]


# ---- the three kernels at every shape -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_fwd_vs_fp64(shape, with_addend, capsys):
    regime, _ = assert_plan(shape)
    o = operands(shape)
    got = run_fwd(shape, o["xr"], o["wd"], o["ar"] if with_addend else None)
    ex, _ = reference("fwd", shape)
    r = C1.check(got, "fwd", shape, ex, addend=o["addend"] if with_addend else None)
    record("fwd", regime, f"fwd {shape} [{regime}{' + addend' if with_addend else ''}]", r, capsys)
    assert max(r) <= 1.0, (regime, r)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_dgrad_vs_fp64(shape, capsys):
    assert_plan(shape)
    o = operands(shape)
    got = run_dgrad(shape, o["gr"], o["wd"])
    ex, _ = reference("dgrad", shape)
    r = C1.check(got, "dgrad", shape, ex)
    record("dgrad", "one plane tile per workgroup", f"dgrad {shape}", r, capsys)
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_wgrad_vs_fp64(shape, capsys):
    _, regime = assert_plan(shape)
    o = operands(shape)
    got = run_wgrad(shape, o["xr"], o["gr"])
    ex, _ = reference("wgrad", shape)
    r = C1.check(got, "wgrad", shape, ex)
    record("wgrad", regime, f"wgrad {shape} [{regime}, {C1.wgrad_roundings(shape)} roundings]", r, capsys)
    assert max(r) <= 1.0, (regime, r)


# ---- the fused BatchNorm + ReLU operand -----------------------------------------------------------------------------------------------
def assert_affine_operand(o):
    """what the pair is built for: channels clamped everywhere, channels never clamped, scales of both signs, a positive shift"""
    p, _ = C1.operand(o["x"], *o["affine"])
    assert bool((p[:, 8:12] == 0).all()) and bool((p[:, 12:16] > 0).all())
    sc, sh = o["affine"]
    assert bool((sc > 0).any()) and bool((sc < 0).any()) and bool((sh < 0).any()) and bool((sh[0:4] > 0.5).all())
    frac = float((p > 0).double().mean())
    assert 0.2 < frac < 0.8, frac


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=sid)
def test_fwd_fused_affine_vs_fp64(shape, capsys):
    regime, _ = assert_plan(shape)
    o = operands(shape)
    assert_affine_operand(o)
    ex, grant = reference("fwd", shape, True)
    for add in (None, o["ar"]):
        got = run_fwd(shape, o["xr"], o["wd"], add, o["sc"], o["sh"])
        r = C1.check(got, "fwd", shape, ex, addend=o["addend"] if add is not None else None, grant=grant)
        record("fwd affine", regime, f"fwd affine {shape} [{regime}{' + addend' if add is not None else ''}]", r, capsys)
        assert max(r) <= 1.0, (regime, r)
    # the affine does change the result: the plain operand is far outside the bounds
    plain = run_fwd(shape, o["xr"], o["wd"])
    assert min(C1.check(plain, "fwd", shape, ex, grant=grant)) > 1.0


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=sid)
def test_wgrad_fused_affine_vs_fp64(shape, capsys):
    _, regime = assert_plan(shape)
    o = operands(shape)
    ex, grant = reference("wgrad", shape, True)
    got = run_wgrad(shape, o["xr"], o["gr"], o["sc"], o["sh"])
    r = C1.check(got, "wgrad", shape, ex, grant=grant)
    record("wgrad affine", regime, f"wgrad affine {shape} [{regime}]", r, capsys)
    assert max(r) <= 1.0, (regime, r)
    assert min(C1.check(run_wgrad(shape, o["xr"], o["gr"]), "wgrad", shape, ex, grant=grant)) > 1.0


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 13), (3, 5, 11, 65), (1, 2050, 3, 5), (1, 48, 16, 240)], ids=sid)
def test_wgrad_with_large_values_around_its_operands(shape, affine, capsys):
    """`in` and `grad_logits` embedded between floats of 1e4 (module docstring): one of them multiplied into a sum of magnitude
    <= 1e-3 K is far outside every bound"""
    _, regime = assert_plan(shape)
    o = operands(shape)
    ex, grant = reference("wgrad", shape, affine)
    sc, sh = (o["sc"], o["sh"]) if affine else (None, None)
    got = run_wgrad(shape, embedded(o["xr"]), embedded(o["gr"]), sc, sh)
    r = C1.check(got, "wgrad", shape, ex, grant=grant)
    record("wgrad embedded", regime, f"wgrad embedded {shape} [{regime}{', affine' if affine else ''}]", r, capsys)
    assert max(r) <= 1.0, (regime, r)


# ---- run to run -------------------------------------------------------------------------------------------------------------------
TWICE = [(3, 5, 11, 65), (3, 7, 40, 130), (1, 2050, 3, 5), (768, 3, 8, 16)]


@pytest.mark.parametrize("shape", TWICE, ids=sid)
def test_fwd_and_dgrad_are_bit_identical_over_two_runs(shape):
    o = operands(shape)
    for add, sc, sh in ((None, None, None), (o["ar"], o["sc"], o["sh"])):
        assert torch.equal(run_fwd(shape, o["xr"], o["wd"], add, sc, sh), run_fwd(shape, o["xr"], o["wd"], add, sc, sh))
    assert torch.equal(run_dgrad(shape, o["gr"], o["wd"]), run_dgrad(shape, o["gr"], o["wd"]))


@pytest.mark.parametrize("shape", TWICE, ids=sid)
def test_wgrad_over_two_runs_differs_by_the_order_of_its_atomics_at_most(shape, capsys):
    """the lane chains and shuffles are fixed; the four LDS atomics and the `grid` global atomics come in any order:
    |run 1 - run 2| <= 2 gamma_(4 + grid) S and <= the bound of check (a), and each run passes check (a)"""
    o = operands(shape)
    ex, _ = reference("wgrad", shape)
    a, b = run_wgrad(shape, o["xr"], o["gr"]).clone(), run_wgrad(shape, o["xr"], o["gr"]).clone()
    ra, rb, rd = C1.check(a, "wgrad", shape, ex)[0], C1.check(b, "wgrad", shape, ex)[0], C1.order_ratio(a, b, shape, ex)
    with capsys.disabled():
        print(f"\nwgrad twice {shape}: (a) {ra:.4f} and {rb:.4f}, difference / order bound {rd:.4f}, bit-identical: {torch.equal(a, b)}")
    assert max(ra, rb, rd) <= 1.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """one of in_scale / in_shift alone; B or D of 0; B or D above 65535 (refused on the host before any launch: the buffers are
    those of the small shape); the same dimensions through az_conv3d_c1_plan"""
    shape = (2, 3, 4, 5)
    b, d, h, w = shape
    x, g, wt, s = torch.zeros(b, d, h, w, 32, device=DEV), torch.zeros(b, d, h, w, device=DEV), torch.zeros(864, device=DEV), torch.ones(32, device=DEV)
    whole_o, out = guarded(b * d * h * w)
    whole_gx, gx = guarded(b * d * h * w * 32)
    whole_gw, gw = guarded(864)
    fwd = lambda sc, sh, dims: _call("az_conv3d_c1_fwd", _p(out), _p(x), _p(wt), None, _p(sc), _p(sh), *dims, _stream())
    wgr = lambda sc, sh, dims: _call("az_conv3d_c1_wgrad", _p(gw), _p(x), _p(g), _p(sc), _p(sh), *dims, _stream())
    dgr = lambda dims: _call("az_conv3d_c1_dgrad", _p(gx), _p(g), _p(wt), *dims, _stream())
    bad_dims = [(0, d, h, w), (b, 0, h, w), (65536, d, h, w), (b, 65536, h, w)]
    for f in (fwd, wgr):
        for sc, sh in ((s, None), (None, s)):
            with pytest.raises(RuntimeError):
                f(sc, sh, shape)
        for dims in bad_dims:
            with pytest.raises(RuntimeError):
                f(None, None, dims)
    for dims in bad_dims:
        with pytest.raises(RuntimeError):
            dgr(dims)
    torch.cuda.synchronize()
    # nothing was launched: the outputs still hold their sentinels
    assert bool(torch.isnan(whole_o).all()) and bool(torch.isnan(whole_gx).all()) and bool(torch.isnan(whole_gw).all())
    plan = (ctypes.c_longlong * 4)()
    codes = [lib().az_conv3d_c1_plan(plan, *dims) for dims in bad_dims]
    assert codes == [_lib.CONST["AZ_EINVAL"]] * 2 + [_lib.CONST["AZ_EUNSUPPORTED"]] * 2
    assert lib().az_conv3d_c1_plan(None, *shape) == _lib.CONST["AZ_ENULL"]
    fwd(s, s, shape), wgr(s, s, shape), dgr(shape)  # (the base launches are accepted)
    torch.cuda.synchronize()
    assert bands_intact(whole_o, out.numel()) and bands_intact(whole_gx, gx.numel()) and bands_intact(whole_gw, 864)


# ---- the wiring through conv3d.conv_logits --------------------------------------------------------------------------------------------
def test_conv_logits_with_a_deferred_affine_and_an_addend(capsys):
    """conv_logits(x, conv, addend, affine = a filled DeferredAffine): the forward is the C-ABI forward bit for bit; x.grad (the
    gradient with respect to the OPERAND relu(x scale + shift): conv_bn's backward takes it from there), the weight gradient and
    the addend's gradient pass the checks of the direct launches"""
    shape = (3, 7, 40, 130)
    fwd_regime, wg_regime = assert_plan(shape)
    o = operands(shape)
    da = conv3d.DeferredAffine()
    da.scale, da.shift = o["sc"], o["sh"]
    assert da.pending
    conv = torch.nn.Conv3d(32, 1, 3, padding=1, bias=False).to(DEV)
    conv.weight.data.copy_(o["w"])
    xg, ag = o["xr"].clone().requires_grad_(), o["ar"][:, 0].clone().requires_grad_()
    y = conv3d.conv_logits(xg, conv, ag, affine=da)
    assert torch.equal(y.detach(), run_fwd(shape, o["xr"], o["wd"], o["ar"], o["sc"], o["sh"])[:, 0])
    ex, grant = reference("fwd", shape, True)
    r = C1.check(y.detach().unsqueeze(1), "fwd", shape, ex, addend=o["addend"], grant=grant)
    record("conv_logits fwd", fwd_regime, f"conv_logits fwd {shape}", r, capsys)
    assert max(r) <= 1.0, r
    y.backward(o["gr"][:, 0])
    torch.cuda.synchronize()
    assert torch.equal(ag.grad, o["gr"][:, 0])
    r = C1.check(xg.grad.permute(0, 4, 1, 2, 3), "dgrad", shape, reference("dgrad", shape)[0])
    record("conv_logits dgrad", "one plane tile per workgroup", f"conv_logits x.grad {shape}", r, capsys)
    assert max(r) <= 1.0, r
    ex, grant = reference("wgrad", shape, True)
    r = C1.check(conv.weight.grad, "wgrad", shape, ex, grant=grant)
    record("conv_logits wgrad", wg_regime, f"conv_logits weight.grad {shape}", r, capsys)
    assert max(r) <= 1.0, r


def test_zz_largest_ratios(capsys):
    """the last test of the module: the largest ratio of each check per kernel and regime over the cases run"""
    with capsys.disabled():
        print("\nlargest err / bound:  (a)  (b)  (c)   [case of the largest (b)]")
        for (k, regime), r in sorted(WORST.items()):
            print(f"  {k:18s} {regime:34s} " + "  ".join(f"{v:7.4f}" for v in r[:3]) + f"   {r[3]}")
    assert all(max(r[:3]) <= 1.0 for r in WORST.values())
