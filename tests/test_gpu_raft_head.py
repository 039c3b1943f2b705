"""GPU parity of the RAFT-Stereo prediction head: K15 convex upsampling (az_convex_up_{fwd,bwd}) and K16 sequence
loss (az_seq_loss_{fwd,bwd}) through activezero_amd.ops, against the reference's outputs (golden G14) and against
the fp64 checker tests/_raft_head_ref.py.

The rule for every fp32 tensor (the one G13 uses): max |hip - ref64| <= max(3 e_ref, 2e-6 max |ref64|), e_ref =
max |ref32 - ref64| -- three times the distance of the reference's own fp32 arithmetic from exact, with a floor of
about twenty fp32 roundings of the tensor's largest value (a 9-term softmax and a 9-term sum)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.nets.raft import upsample  # noqa: E402
from activezero_amd.utils import seq_losses  # noqa: E402
from tests import _raft_head_ref as ref  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = "cuda:0"


def dev(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.to(DEV).contiguous()


def t64(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.detach().cpu().double()


def within(got, ref64, ref32, what):
    """the parity rule of the module docstring; prints each figure before it asserts"""
    got, ref64, ref32 = t64(got), t64(ref64), t64(ref32)
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    e_ref = (ref32 - ref64).abs().max().item()
    bound = max(3.0 * e_ref, 2e-6 * ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    print(f"{what}: err {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{what}: max |hip - ref64| {err:.3e} > {bound:.3e} (e_ref {e_ref:.3e})"


def fp16_ordinal(x):
    """fp16 values as integers that order like the values: neighbours differ by 1"""
    b = x.contiguous().view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


def within_one_fp16_ulp(got16, ref64, what):
    assert got16.dtype == torch.float16
    d = (fp16_ordinal(got16.cpu()) - fp16_ordinal(t64(ref64).half())).abs().max().item()
    print(f"{what}: {d} fp16 ulp")
    assert d <= 1, f"{what}: {d} fp16 ulp from the rounded fp64 value"


def run_hip(flow, mask, f, cot, channels=None, negate=False):
    fl, mk = dev(flow).requires_grad_(True), dev(mask).requires_grad_(True)
    up = ops.convex_upsample(fl, mk, f, channels, negate)
    gf, gm = torch.autograd.grad(up, (fl, mk), dev(cot))
    return up.detach(), gf, gm


def run_ref(flow, mask, f, cot, dtype, channels=None, negate=False):
    fl, mk = flow.to(dtype).requires_grad_(True), mask.to(dtype).requires_grad_(True)
    up = ref.convex_upsample(fl, mk, f, channels, negate)
    gf, gm = torch.autograd.grad(up, (fl, mk), cot.to(dtype))
    return up.detach(), gf, gm


# ---------------------------------------------------------------------------------------------- G14 parity
@pytest.mark.parametrize("tag", ["a", "b"])
def test_g14_upsampling_fp32(golden, tag):
    g = golden("g14_raft_head")
    f, flow, mask, cot = ref.g14_upsample_inputs(g, tag)
    up, gf, gm = run_hip(flow, mask, f, cot)
    (uy, ux), (my, mx) = g["up_lat"], g["gmask_lat"]
    within(up[..., ::uy, ::ux], g[f"{tag}_up64"], g[f"{tag}_up32"], f"{tag} up")
    within(gf, g[f"{tag}_gflow64"], g[f"{tag}_gflow32"], f"{tag} g_flow")
    within(gm[..., ::my, ::mx], g[f"{tag}_gmask64"], g[f"{tag}_gmask32"], f"{tag} g_mask")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g14_upsampling_fp16_mask(golden, tag):
    """e_ref is the reference's own mixed-precision evaluation (fp16 softmax, fp32 product) against fp64 of the same
    fp16-valued inputs: we must be at least as close to exact"""
    g = golden("g14_raft_head")
    f, flow, mask, cot = ref.g14_upsample_inputs(g, tag)
    up, gf, gm = run_hip(flow, mask.half(), f, cot)
    (uy, ux), (my, mx) = g["up_lat"], g["gmask_lat"]
    within(up[..., ::uy, ::ux], g[f"{tag}_up64_h"], g[f"{tag}_up_amp"], f"{tag} up (fp16 mask)")
    within(gf, g[f"{tag}_gflow64_h"], g[f"{tag}_gflow_amp"], f"{tag} g_flow (fp16 mask)")
    within_one_fp16_ulp(gm[..., ::my, ::mx], g[f"{tag}_gmask64_h"], f"{tag} g_mask (fp16)")


@pytest.mark.parametrize("n_pred", [4, 22])
def test_g14_sequence_loss(golden, n_pred):
    g = golden("g14_raft_head")
    preds, gt, valid = ref.g14_sequence_inputs(g, n_pred)
    ps = [dev(p).requires_grad_(True) for p in preds]
    loss = seq_losses.sequence_loss(ps, dev(gt), dev(valid), float(g["loss_gamma"]), float(g["max_flow"]))
    grads = torch.stack(torch.autograd.grad(loss, ps))
    st = int(g["seq_lat"])
    within(loss, g[f"s{n_pred}_loss64"], g[f"s{n_pred}_loss32"], f"n={n_pred} loss")
    within(grads[..., ::st, ::st], g[f"s{n_pred}_grads64"], g[f"s{n_pred}_grads32"], f"n={n_pred} grads")


# ------------------------------------------------------------------------------------- random shapes, fp64 checker
SHAPES = [  # N, D, h, w, factor, channels, negate, fp16 mask
    (1, 2, 7, 13, 4, None, False, False),    # odd h, odd w
    (2, 2, 5, 67, 4, None, False, False),    # w not a multiple of 64
    (1, 2, 3, 131, 8, None, False, False),
    (1, 2, 1, 9, 4, None, False, False),     # h = 1: the halo is the whole tile
    (1, 2, 9, 1, 8, None, False, False),     # w = 1
    (2, 1, 2, 2, 4, None, False, False),     # h = w = 2, D = 1
    (1, 2, 1, 1, 8, None, True, False),
    (3, 2, 6, 10, 4, None, False, False),    # N = 3
    (3, 2, 4, 6, 8, 1, False, False),        # channels = 1
    (2, 2, 11, 21, 4, 1, True, False),       # channels = 1 and negate: the disparity
    (2, 2, 11, 21, 4, 2, True, False),
    (2, 2, 5, 9, 8, 1, True, True),
    (1, 2, 8, 70, 4, None, False, True),
]


@pytest.mark.parametrize("n,d,h,w,f,channels,negate,half", SHAPES)
def test_random_shapes_against_the_fp64_checker(n, d, h, w, f, channels, negate, half):
    """The 1-ulp rule of an fp16 g_mask holds for its subnormals too (one ulp = 6e-8 ABSOLUTE): where the bracket
    G_k - sum p_m G_m of a near-uniform pixel cancels to ~1e-4 of |G| ~ 10, the plain fp32 evaluation of the checker
    is up to 38 fp16 ulp off (268 of the 80 640 elements of case [1-2-8-70-4-None-False-True]) -- which is why the
    fp16 backward evaluates the softmax terms and the bracket in fp64."""
    sd = 5000 + 17 * h + 3 * w + f + n
    flow = seeded((n, d, h, w), sd, -4.0, 4.0)
    mask = ref.make_mask_logits((n, 9 * f * f, h, w), sd + 1)
    if half:
        mask = mask.half()
    cot = seeded((n, channels or d, f * h, f * w), sd + 2)
    up, gf, gm = run_hip(flow, mask, f, cot, channels, negate)
    r64 = run_ref(flow, mask.float(), f, cot, torch.float64, channels, negate)
    r32 = run_ref(flow, mask.float(), f, cot, torch.float32, channels, negate)
    assert up.shape == (n, channels or d, f * h, f * w) and gf.shape == flow.shape and gm.shape == mask.shape
    within(up, r64[0], r32[0], "up")
    within(gf, r64[1], r32[1], "g_flow")
    if channels == 1 and d == 2:
        assert not gf[:, 1].any(), "g_flow of a channel that was not computed must be zero"
    if half:
        assert gm.dtype == torch.float16
        within_one_fp16_ulp(gm, r64[2], "g_mask (fp16)")
    else:
        within(gm, r64[2], r32[2], "g_mask")


def test_module_functions_match_the_op():
    flow = dev(seeded((2, 2, 6, 10), 5101, -3.0, 3.0))
    mask = dev(ref.make_mask_logits((2, 144, 6, 10), 5102))
    full = upsample.upsample_flow(flow, mask, 4)
    assert full.shape == (2, 2, 24, 40)
    assert torch.equal(upsample.upsample_disparity(flow, mask, 4), full[:, :1])
    assert torch.equal(ops.convex_upsample(flow, mask, 4, channels=1, negate=True), -full[:, :1])
    with pytest.raises(RuntimeError):
        ops.convex_upsample(flow, mask[:, :143].contiguous(), 4)
    with pytest.raises(RuntimeError):
        ops.convex_upsample(flow, mask, 3)
    with pytest.raises(RuntimeError):
        ops.convex_upsample(flow, mask.double(), 4)
    with pytest.raises(RuntimeError):
        ops.convex_upsample(flow, mask[:, :, :5].contiguous(), 4)


def test_cotangent_at_an_odd_storage_offset():
    """a contiguous grad_up that is a view 4 bytes into a buffer is not 16-byte aligned: same gradients as an aligned copy"""
    f, h, w = 4, 5, 7
    flow, mask = seeded((1, 2, h, w), 5151, -3.0, 3.0), ref.make_mask_logits((1, 144, h, w), 5152)
    cot = seeded((1, 2, f * h, f * w), 5153)
    buf = torch.zeros(cot.numel() + 1, device=DEV)
    view = buf[1:].view(cot.shape)
    view.copy_(dev(cot))
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    fl, mk = dev(flow).requires_grad_(True), dev(mask).requires_grad_(True)
    gf, gm = torch.autograd.grad(ops.convex_upsample(fl, mk, f), (fl, mk), view)
    _, gf0, gm0 = run_hip(flow, mask, f, cot)
    assert torch.equal(gf, gf0) and torch.equal(gm, gm0)


def test_production_size_once():
    """BASELINE configs[4]: mask [4,144,136,240] (544x960 at 1/4), forward and backward, the disparity form"""
    n, h, w, f = 4, 136, 240, 4
    flow = seeded((n, 2, h, w), 5201, -30.0, 30.0)
    flow[:, 1] = 0.0
    mask = ref.make_mask_logits((n, 9 * f * f, h, w), 5202)
    cot = seeded((n, 1, f * h, f * w), 5203)
    up, gf, gm = run_hip(flow, mask, f, cot, 1, True)
    r64 = run_ref(flow, mask, f, cot, torch.float64, 1, True)
    r32 = run_ref(flow, mask, f, cot, torch.float32, 1, True)
    within(up, r64[0], r32[0], "up")
    within(gf, r64[1], r32[1], "g_flow")
    within(gm, r64[2], r32[2], "g_mask")


# ------------------------------------------------------------------------------------------------ edge values
@pytest.mark.parametrize("half,big", [(False, 80.0), (True, 60000.0)])
def test_extreme_logits_stay_finite(half, big):
    g = torch.Generator().manual_seed(5301)
    mask = torch.where(torch.rand(1, 144, 5, 9, generator=g) < 0.5, -big, big)
    mask[:, :, 0, 0] = big   # all equal at one pixel
    mask[:, :, 0, 1] = -big
    if half:
        mask = mask.half()
    flow = seeded((1, 2, 5, 9), 5302, -3.0, 3.0)
    cot = seeded((1, 2, 20, 36), 5303)
    up, gf, gm = run_hip(flow, mask, 4, cot)
    for name, t in (("up", up), ("g_flow", gf), ("g_mask", gm)):
        assert torch.isfinite(t).all(), f"{name} has inf / NaN"
    r64 = run_ref(flow, mask.float(), 4, cot, torch.float64)
    r32 = run_ref(flow, mask.float(), 4, cot, torch.float32)
    within(up, r64[0], r32[0], "up")
    within(gf, r64[1], r32[1], "g_flow")


@pytest.mark.parametrize("f", [4, 8])
def test_all_equal_mask_gives_exact_ninths(f):
    """integer flow: the nine-term sums are exact, so the output is the correctly rounded f * sum / 9"""
    h, w = 6, 11
    flow = torch.from_numpy(np.random.default_rng(5401).integers(-40, 41, size=(1, 2, h, w)).astype(np.float32))
    mask = torch.full((1, 9 * f * f, h, w), 1.375)
    up = ops.convex_upsample(dev(flow), dev(mask), f).cpu()
    s = torch.nn.functional.avg_pool2d(flow, 3, 1, 1, divisor_override=1)  # exact integer sums, zero padding
    want = (f * (s / 9.0)).repeat_interleave(f, 2).repeat_interleave(f, 3)
    assert torch.equal(up, want)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_flow_pixel_stays_in_its_window(bad):
    f, h, w, y0, x0 = 4, 7, 9, 3, 5
    flow = seeded((1, 2, h, w), 5501, -3.0, 3.0)
    flow[0, 0, y0, x0] = bad
    mask = ref.make_mask_logits((1, 144, h, w), 5502) * 0.1  # every tap has weight: the whole window is touched
    up = ops.convex_upsample(dev(flow), dev(mask), f).cpu()
    touched = torch.zeros(h, w, dtype=torch.bool)
    touched[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = True
    touched = touched.repeat_interleave(f, 0).repeat_interleave(f, 1)
    assert torch.isfinite(up[0, 1]).all()
    assert torch.isfinite(up[0, 0][~touched]).all()
    assert (~torch.isfinite(up[0, 0][touched])).all()


def test_gradients_are_bit_identical_over_three_runs():
    n, h, w, f = 2, 23, 37, 4
    flow = seeded((n, 2, h, w), 5601, -3.0, 3.0)
    mask = ref.make_mask_logits((n, 144, h, w), 5602)
    cot = seeded((n, 2, f * h, f * w), 5603)
    runs = [run_hip(flow, mask, f, cot) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[1], runs[0][1]), "g_flow differs from run to run"
        assert torch.equal(r[2], runs[0][2]), "g_mask differs from run to run"
        assert torch.equal(r[0], runs[0][0])


def test_central_differences_at_a_tiny_size():
    """fp32 central differences of sum(up * cot) along random directions, against the analytic gradients"""
    f, h, w = 4, 3, 4
    flow = seeded((1, 2, h, w), 5701, -2.0, 2.0)
    mask = seeded((1, 144, h, w), 5702, -1.5, 1.5)
    cot = seeded((1, 2, f * h, f * w), 5703)
    _, gf, gm = run_hip(flow, mask, f, cot)

    def value(fl, mk):
        return (ops.convex_upsample(dev(fl), dev(mk), f).double() * dev(cot).double()).sum().item()

    # step sizes: the value is a sum of 768 fp32 outputs of size <= 8, known to ~1e-4, so a difference over 2 eps is
    # good to ~1e-4 / eps; linear in the flow (no truncation error), O(eps^2) relative truncation in the mask
    eps_f, eps_m = 5e-2, 2e-2
    for k in range(4):
        df, dm = seeded(flow.shape, 5710 + k), seeded(mask.shape, 5720 + k)
        num_f = (value(flow + eps_f * df, mask) - value(flow - eps_f * df, mask)) / (2 * eps_f)
        num_m = (value(flow, mask + eps_m * dm) - value(flow, mask - eps_m * dm)) / (2 * eps_m)
        ana_f = (gf.cpu().double() * df.double()).sum().item()
        ana_m = (gm.cpu().double() * dm.double()).sum().item()
        print(f"direction {k}: flow {num_f:.6f} vs {ana_f:.6f}, mask {num_m:.6f} vs {ana_m:.6f}")
        assert abs(num_f - ana_f) <= 5e-3 * max(1.0, abs(ana_f)), (num_f, ana_f)
        assert abs(num_m - ana_m) <= 5e-3 * max(1.0, abs(ana_m)), (num_m, ana_m)


# ---------------------------------------------------------------------------------------------- sequence loss
def seq_inputs(n_pred, shape=(2, 1, 20, 28), sd=5801):
    gt = seeded(shape, sd, -40.0, 820.0)
    valid = (seeded(shape, sd + 1, 0.0, 1.0) > 0.2).float()
    valid[:, :, 2:6, 3:12] = 0.0
    gt[0, 0, 10, 10], valid[0, 0, 10, 10] = 12.5, 1.0
    preds = [-gt + seeded(shape, sd + 10 + i, -3.0, 3.0) for i in range(n_pred)]
    preds[0][0, 0, 10, 10] = -12.5  # pred == target at a valid pixel: sign(0) = 0
    return preds, gt, valid


def test_sequence_loss_special_cases():
    preds, gt, valid = seq_inputs(3)
    ps = [dev(p).requires_grad_(True) for p in preds]
    loss = ops.sequence_loss(ps, dev(gt), dev(valid))
    grads = torch.autograd.grad(loss * 1.0, ps)
    r = [p.double().requires_grad_(True) for p in preds]
    want = ref.sequence_loss(r, gt.double(), valid.double())
    want_g = torch.autograd.grad(want, r)
    r32 = [p.clone().requires_grad_(True) for p in preds]
    want32 = ref.sequence_loss(r32, gt, valid)
    want_g32 = torch.autograd.grad(want32, r32)
    within(loss, want.detach(), want32.detach(), "loss")
    for i in range(3):
        within(grads[i], want_g[i], want_g32[i], f"grad {i}")
    assert grads[0][0, 0, 10, 10].item() == 0.0
    # a byte map and the same map as floats agree bit for bit
    for vmap in (dev(valid).to(torch.uint8), dev(valid) > 0.5):
        ps2 = [dev(p).requires_grad_(True) for p in preds]
        loss2 = ops.sequence_loss(ps2, dev(gt), vmap)
        assert torch.equal(loss2, loss)
        for a, b in zip(torch.autograd.grad(loss2, ps2), grads):
            assert torch.equal(a, b)
    # disparities against +gt: the same loss, negated gradients
    ps3 = [(-dev(p)).requires_grad_(True) for p in preds]
    loss3 = ops.sequence_loss(ps3, dev(gt), dev(valid), disparity=True)
    assert torch.equal(loss3, loss)
    for a, b in zip(torch.autograd.grad(loss3, ps3), grads):
        assert torch.equal(a, -b)
    # the upstream gradient is honoured
    ps4 = [dev(p).requires_grad_(True) for p in preds]
    (ops.sequence_loss(ps4, dev(gt), dev(valid)) * 2.5).backward()
    within(ps4[1].grad, 2.5 * want_g[1], 2.5 * want_g32[1], "scaled grad")


def test_sequence_loss_all_invalid_is_nan_like_the_reference():
    preds, gt, valid = seq_inputs(2)
    assert math.isnan(ops.sequence_loss([dev(p) for p in preds], dev(gt), torch.zeros_like(dev(valid))).item())


def test_sequence_loss_single_prediction_has_weight_one():
    preds, gt, valid = seq_inputs(1)
    p = dev(preds[0]).requires_grad_(True)
    loss = ops.sequence_loss([p], dev(gt), dev(valid))
    r = preds[0].double().requires_grad_(True)
    want = ref.sequence_loss([r], gt.double(), valid.double())
    r32 = preds[0].clone().requires_grad_(True)
    want32 = ref.sequence_loss([r32], gt, valid)
    within(loss, want.detach(), want32.detach(), "loss")
    within(torch.autograd.grad(loss, p)[0], torch.autograd.grad(want, r)[0], torch.autograd.grad(want32, r32)[0], "grad")


def test_sequence_loss_check_raises_and_default_does_not_sync():
    preds, gt, valid = seq_inputs(3)
    ps = [dev(p) for p in preds]
    g, v = dev(gt), dev(valid)
    assert math.isfinite(ops.sequence_loss(ps, g, v, check=True).item())
    for bad in (float("nan"), float("inf")):
        broken = [p.clone() for p in ps]
        broken[1][1, 0, 0, 0] = bad  # an invalid pixel counts too: the reference asserts on the whole prediction
        with pytest.raises(AssertionError):
            ops.sequence_loss(broken, g, v, check=True)
        ops.sequence_loss(broken, g, v)  # no check, no raise
    ps = [p.requires_grad_(True) for p in ps]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = ops.sequence_loss(ps, g, v)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(p.grad is not None for p in ps)


# ------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_22_iterations():
    """22 x (upsample_disparity -> sequence_loss) on [2,144,34,60] against the checker's autograd"""
    n, h, w, f, iters = 2, 34, 60, 4, 22
    gt = seeded((n, 1, f * h, f * w), 5901, 2.0, 90.0)
    gt[0, 0, :9, :40] = 750.0
    valid = (seeded((n, 1, f * h, f * w), 5902, 0.0, 1.0) > 0.15).float()
    flows, masks = [], []
    for i in range(iters):
        fl = -gt[:, :, ::f, ::f] / f + seeded((n, 1, h, w), 5910 + i, -1.0, 1.0) * (1.0 + 0.1 * (iters - i))
        flows.append(torch.cat([fl, torch.zeros_like(fl)], 1).contiguous())
        masks.append(ref.make_mask_logits((n, 144, h, w), 5950 + i))

    def run(up_fn, loss_fn, conv):
        fs = [conv(x).requires_grad_(True) for x in flows]
        ms = [conv(x).requires_grad_(True) for x in masks]
        loss = loss_fn([up_fn(a, b) for a, b in zip(fs, ms)], conv(gt), conv(valid))
        grads = torch.autograd.grad(loss, fs + ms)
        return loss.detach(), grads[:iters], grads[iters:]

    got = run(lambda a, b: upsample.upsample_disparity(a, b, f), seq_losses.sequence_loss, dev)
    r64 = run(lambda a, b: ref.convex_upsample(a, b, f, channels=1), ref.sequence_loss, lambda x: x.double())
    r32 = run(lambda a, b: ref.convex_upsample(a, b, f, channels=1), ref.sequence_loss, lambda x: x.clone())
    within(got[0], r64[0], r32[0], "loss")
    for i in range(iters):
        within(got[1][i], r64[1][i], r32[1][i], f"g_flow[{i}]")
        within(got[2][i], r64[2][i], r32[2][i], f"g_mask[{i}]")
