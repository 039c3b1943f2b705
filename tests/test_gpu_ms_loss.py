"""GPU: K29, the multi-scale masked smooth-L1 disparity loss (csrc/az_ms_loss.hip, ops.multiscale_disp_loss,
utils/disp_losses.py dispnet_disp / default_disp and their range forms) against tests/_ms_loss_ref.py: accumulators, loss,
per-scale means and every gradient element under that file's rules, on every case under a byte mask, a bool mask and both
range rules; gradients for a subset of the predictions; replay; no host sync; K12 as a cross-check; non-finite inputs;
the wrapper's errors; and the reference's own fp64 evaluation (tests/golden/g17_ms_loss.npz) under the derived bounds.
tests/test_ms_loss_error_model_cpu.py shows on the CPU that these rules reject the wrong kernels of its list."""
import math
import os

import numpy as np
import pytest
import torch

from activezero_amd import _lib, ops
from activezero_amd.utils import disp_losses
from tests import _ms_loss_ref as M
from tests import _nonfinite as NF
from tests import _reduce_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_ms_loss.npz")
N_CASES = len(M.FLAT_SHAPES) + len(M.SHAPES) + 2


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases are read-only)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def raw_fwd(preds, shifts, gt, mask, lo, hi):
    """az_ms_loss_fwd through the C ABI: the accumulators [nd, 2]"""
    acc = torch.zeros(len(preds), 2, dtype=torch.float64, device="cuda")
    m = None if mask is None else (mask.view(torch.uint8) if mask.dtype == torch.bool else mask)
    descs = ops._ms_descs(preds, [None] * len(preds), shifts)
    b, _, h, w = gt.shape
    ops._call("az_ms_loss_fwd", acc.data_ptr(), descs.ctypes.data, len(preds), gt.data_ptr(), ops._p(m), float(lo), float(hi),
              b, h, w, ops._stream())
    return host(acc)


def run(case, mask, lo, hi, need=None, gloss=M.GLOSS):
    """(loss, scale_means, [grad or None]) of ops.multiscale_disp_loss, one backward with grad_output = gloss"""
    need = [True] * len(case["preds"]) if need is None else need
    ps = [dev(p).requires_grad_(n) for p, n in zip(case["preds"], need)]
    loss = ops.multiscale_disp_loss(ps, dev(case["gt"]), dev(mask), case["shifts"], case["weights"], lo, hi)
    if any(need):
        (loss * gloss).backward()
    return loss, loss.scale_means, [host(p.grad) for p in ps]


@pytest.mark.parametrize("index", range(N_CASES))
def test_accumulators_scalars_and_gradients_on_every_case(index):
    c, cn = M.all_cases()[index], M.all_cases(nonfinite_preds=True)[index]
    worst = {}
    for mode, mask, lo, hi in M.modes(c):
        args = (c["preds"], c["shifts"], c["gt"], mask, lo, hi)
        acc = raw_fwd([dev(p) for p in c["preds"]], c["shifts"], dev(c["gt"]), dev(mask), lo, hi)
        for k, v in M.check_fwd(acc, *args).items():
            worst[k] = max(worst.get(k, 0.0), v)
        loss, means, grads = run(c, mask, lo, hi)
        assert loss.dtype == means.dtype == torch.float32 and loss.shape == () and means.shape == (len(c["preds"]),)
        assert not means.requires_grad
        wargs = (c["preds"], c["shifts"], c["weights"], c["gt"], mask, lo, hi)
        worst["scalars"] = max(worst.get("scalars", 0.0), M.check_scalars(host(loss), host(means), *wargs))
        counts = [int(n) for n in acc[:, 1]]
        M.check_bwd(grads, *wargs, M.GLOSS, counts)
        # NaN / +inf / -inf predictions on valid pixels: the backward's values; the forward sums by class
        nargs = (cn["preds"], cn["shifts"], cn["gt"], mask, lo, hi)
        nacc = raw_fwd([dev(p) for p in cn["preds"]], cn["shifts"], dev(cn["gt"]), dev(mask), lo, hi)
        M.check_fwd(nacc, *nargs)
        _, _, ngrads = run(cn, mask, lo, hi)
        M.check_bwd(ngrads, cn["preds"], cn["shifts"], cn["weights"], cn["gt"], mask, lo, hi, M.GLOSS, [int(n) for n in nacc[:, 1]])
    print(f"\n  {c['name']}: largest err / bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()), end="")


@pytest.mark.parametrize("subset", ["none", "first", "every other", "all"])
def test_gradients_for_a_subset_of_the_predictions(subset):
    c = M.all_cases()[-3]  # 2 x 127 x 65, seven scales
    nd = len(c["preds"])
    need = {"none": [False] * nd, "first": [k == 0 for k in range(nd)], "every other": [k % 2 == 1 for k in range(nd)],
            "all": [True] * nd}[subset]
    for mode, mask, lo, hi in M.modes(c):
        loss, means, grads = run(c, mask, lo, hi, need)
        assert loss.requires_grad == any(need)
        counts = [n for _, n in M.ms_fwd(c["preds"], c["shifts"], c["gt"], mask, lo, hi)]
        M.check_bwd(grads, c["preds"], c["shifts"], c["weights"], c["gt"], mask, lo, hi, M.GLOSS, counts, need)
        M.check_scalars(host(loss), host(means), c["preds"], c["shifts"], c["weights"], c["gt"], mask, lo, hi)


def test_a_second_backward_over_a_retained_graph_gives_equal_values():
    c = M.all_cases(nonfinite_preds=True)[-2]
    ps = [dev(p).requires_grad_() for p in c["preds"]]
    loss = ops.multiscale_disp_loss(ps, dev(c["gt"]), dev(c["mask"]), c["shifts"], c["weights"])
    first = torch.autograd.grad(loss, ps, retain_graph=True)
    second = torch.autograd.grad(loss, ps)
    for a, b in zip(first, second):
        assert a.data_ptr() != b.data_ptr()
        R.check_grad(host(b), host(a), "replay")


def test_dispnet_disp_and_default_disp_never_synchronise():
    g = np.load(GOLDEN)
    gt, mask = dev(g["dispnet_gt"]), dev(g["dispnet_mask"])
    ps = [dev(g[f"dispnet_pred{k}"]).requires_grad_() for k in range(7)]
    gt1, mask1, p1 = dev(g["default_gt"]), dev(g["default_mask"]), dev(g["default_pred0"]).requires_grad_()
    calls = []
    real = ops._call
    ops._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # nothing below may synchronise
    try:
        out = [disp_losses.dispnet_disp(ps, gt, mask), disp_losses.dispnet_disp_range(ps, gt, 64.0),
               disp_losses.default_disp(p1, gt1, mask1), disp_losses.default_disp_range(p1, gt1, 64.0)]
        for loss in out:
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops._call = real
    assert calls == ["az_ms_loss_fwd"] * 4 + ["az_ms_loss_bwd"] * 4, calls  # one launch forward, one backward, each
    for a, b in ((out[0], out[1]), (out[2], out[3])):  # the masks were built as 0 < gt < 64: the same pixels, one float32 rounding
        assert abs(float(a.detach()) - float(b.detach())) <= 2.0 ** -23 * abs(float(a.detach()))
        assert np.array_equal(host(a.scale_means) > 0, host(b.scale_means) > 0) and a.scale_means.shape == b.scale_means.shape
    assert all(p.grad is not None for p in ps + [p1])


def test_three_full_resolution_predictions_are_k12():
    """ops.disp_loss is nd = 3, shifts 0, weights (1, 0.7, 0.5): the same counts, the same gradients as values, and a loss
    inside both wrappers' scalar bounds"""
    c = R.loss_case((2, 1, 24, 40), 7610)
    for mode, mask, lo, hi in R.loss_modes(c):
        gt, m = dev(c["gt"]), dev(mask)
        a = [dev(p).requires_grad_() for p in c["preds"]]
        b = [dev(p).requires_grad_() for p in c["preds"]]
        l12 = ops.disp_loss(*a, gt, m, lo, hi)
        l29 = ops.multiscale_disp_loss(b, gt, m, None, R.LOSS_WEIGHTS, lo, hi)
        (l12 * M.GLOSS).backward()
        (l29 * M.GLOSS).backward()
        for k, (x, y) in enumerate(zip(a, b)):
            R.check_grad(host(y.grad), host(x.grad), f"{mode} g_pred[{k}] against K12")
        acc = raw_fwd([p.detach() for p in b], (0, 0, 0), gt, m, lo, hi)
        acc4 = np.array([acc[0, 0], acc[1, 0], acc[2, 0], acc[0, 1]])
        assert acc[0, 1] == acc[1, 1] == acc[2, 1]
        R.check_k12_fwd(acc4, c["preds"], c["gt"], mask, lo, hi, what="az_ms_loss_fwd as K12")
        want, bound = R.disp_loss_scalar(c["preds"], c["gt"], mask, lo, hi)
        assert abs(float(host(l12)) - want) <= bound and abs(float(host(l29)) - want) <= bound, mode
        M.check_scalars(host(l29), host(l29.scale_means), c["preds"], (0, 0, 0), R.LOSS_WEIGHTS, c["gt"], mask, lo, hi)


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------
def _plain_case():
    """2 x 12 x 20, scales 0..2, every pixel valid but (0, 0, 2, 2); |p - g| < 1 everywhere"""
    rng = np.random.default_rng(7620)
    B, H, W, shifts = 2, 12, 20, (0, 1, 2)
    gt = rng.uniform(5.0, 50.0, (B, 1, H, W)).astype(M.F32)
    mask = np.ones((B, 1, H, W), dtype=np.uint8)
    mask[0, 0, 2, 2] = 0
    preds = [(gt[:, :, ::1 << s, ::1 << s][:, :, :H >> s, :W >> s] + rng.uniform(-0.9, 0.9, (B, 1, H >> s, W >> s)).astype(M.F32))
             .astype(M.F32) for s in shifts]
    return dict(preds=preds, gt=gt, mask=mask, shifts=shifts, weights=M.DISPNET_WEIGHTS[:3], shape=(B, H, W), name="plain")


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "+inf", "-inf"])
def test_a_non_finite_prediction_counts_on_a_valid_pixel_only(bad):
    c = _plain_case()
    _, _, clean_grads = run(c, c["mask"], 0.0, math.inf)
    clean_loss, clean_means, _ = run(c, c["mask"], 0.0, math.inf)
    for k, s in enumerate(c["shifts"]):
        # at a valid pixel of prediction k: (1, 1) of scale k meets (1 << s, 1 << s)
        p = dict(c, preds=[q.copy() for q in c["preds"]])
        p["preds"][k][1, 0, 1, 1] = bad
        loss, means, grads = run(p, c["mask"], 0.0, math.inf)
        want = math.nan if math.isnan(bad) else math.inf  # SL1(inf) = inf - 0.5
        NF.same_classes(loss.reshape(1), torch.tensor([want], dtype=torch.float64), f"loss, {bad} in prediction {k}")
        want_means = host(clean_means).astype(np.float64)
        want_means[k] = want
        NF.same_classes(means, torch.from_numpy(want_means), f"scale_means, {bad} in prediction {k}")
        hit = np.zeros(grads[k].shape, dtype=bool)
        hit[1, 0, 1, 1] = True
        count =[n for _, n in M.ms_fwd(c["preds"], c["shifts"], c["gt"], c["mask"], 0.0, math.inf)][k]
        ws = (M.F32(c["weights"][k]) * (M.F32(M.GLOSS) / M.F32(count)))
        got = grads[k][1, 0, 1, 1]
        if math.isnan(bad):
            assert math.isnan(got)
        else:
            assert got == ws * M.F32(math.copysign(1.0, bad))  # the clamp: +-1
        for j in range(len(grads)):  # every other element holds the clean launch's bits
            keep = torch.from_numpy(~hit) if j == k else torch.ones(grads[j].shape, dtype=torch.bool)
            NF.untouched(torch.from_numpy(grads[j]), torch.from_numpy(clean_grads[j]), keep, f"g_pred[{j}], {bad} in prediction {k}")
    # at the invalid pixel (scale 0: (2, 2); scale 1: (1, 1) meets (2, 2)): ignored
    p = dict(c, preds=[q.copy() for q in c["preds"]])
    p["preds"][0][0, 0, 2, 2] = bad
    p["preds"][1][0, 0, 1, 1] = bad
    loss, means, grads = run(p, c["mask"], 0.0, math.inf)
    assert host(loss) == host(clean_loss) and np.array_equal(host(means), host(clean_means))
    for j in range(len(grads)):
        assert np.array_equal(grads[j], clean_grads[j]) and grads[0][0, 0, 2, 2] == 0 and grads[1][0, 0, 1, 1] == 0


def test_a_nan_ground_truth_is_invalid_under_the_range_rule_and_nan_under_a_set_mask_byte():
    c = _plain_case()
    c["mask"] = np.ones_like(c["mask"])
    gt = c["gt"].copy()
    gt[1, 0, 4, 8] = np.nan  # read by scale 0 at (4, 8), scale 1 at (2, 4), scale 2 at (1, 2)
    p = dict(c, gt=gt)
    for lo, hi in R.RANGES:
        loss, means, grads = run(p, None, lo, hi)
        counts = [n for _, n in M.ms_fwd(c["preds"], c["shifts"], gt, None, lo, hi)]
        assert counts == [q.size - 1 for q in c["preds"]]
        assert math.isfinite(float(host(loss))) and bool(torch.isfinite(means).all())
        M.check_scalars(host(loss), host(means), c["preds"], c["shifts"], c["weights"], gt, None, lo, hi)
        M.check_bwd(grads, c["preds"], c["shifts"], c["weights"], gt, None, lo, hi, M.GLOSS, counts)
        assert grads[0][1, 0, 4, 8] == 0 and grads[1][1, 0, 2, 4] == 0 and grads[2][1, 0, 1, 2] == 0
        assert all(not np.isnan(g).any() for g in grads)
    loss, means, grads = run(p, c["mask"], 0.0, math.inf)
    assert math.isnan(float(host(loss))) and bool(torch.isnan(means).all())
    counts = [q.size for q in c["preds"]]
    M.check_bwd(grads, c["preds"], c["shifts"], c["weights"], gt, c["mask"], 0.0, math.inf, M.GLOSS, counts)
    assert [int(np.isnan(g).sum()) for g in grads] == [1, 1, 1]
    assert math.isnan(grads[0][1, 0, 4, 8]) and math.isnan(grads[1][1, 0, 2, 4]) and math.isnan(grads[2][1, 0, 1, 2])


# ---- the wrapper's errors ---------------------------------------------------------------------------------------------------
def test_wrapper_errors():
    gt = torch.zeros(2, 1, 20, 36, device="cuda")
    mk = lambda s, dh=0, dw=0: torch.zeros(2, 1, (20 >> s) + dh, (36 >> s) + dw, device="cuda")
    ops.multiscale_disp_loss([mk(0), mk(1), mk(4)], gt, shifts=(0, 1, 4))  # 1 x 2 at scale 4: fine
    with pytest.raises(RuntimeError, match=r"preds\[1\]: shape"):
        ops.multiscale_disp_loss([mk(0), mk(1, dw=1)], gt, shifts=(0, 1))  # ceil, not floor
    with pytest.raises(RuntimeError, match=r"preds\[0\]: shape"):
        ops.multiscale_disp_loss([mk(1)], gt)
    with pytest.raises(RuntimeError, match=r"preds\[1\]: shape"):
        ops.multiscale_disp_loss([mk(0), mk(0)[:1]], gt)
    with pytest.raises(RuntimeError, match="1..8 predictions"):
        ops.multiscale_disp_loss([mk(0)] * (_lib.CONST["AZ_MS_LOSS_MAX"] + 1), gt)
    with pytest.raises(RuntimeError, match="1..8 predictions"):
        ops.multiscale_disp_loss([], gt)
    with pytest.raises(RuntimeError, match="no pixels at scale 1/32"):  # H = 20 < 2^5, as the reference raises
        ops.multiscale_disp_loss([torch.zeros(2, 1, 0, 1, device="cuda")], gt, shifts=(5,))
    with pytest.raises(RuntimeError, match="no pixels"):
        disp_losses.dispnet_disp([mk(s) for s in range(7)], gt, gt > 0)
    with pytest.raises(RuntimeError, match="mask: shape"):
        ops.multiscale_disp_loss([mk(0)], gt, torch.ones(2, 1, 20, 35, dtype=torch.bool, device="cuda"))
    with pytest.raises(RuntimeError, match="disp_gt: expected"):
        ops.multiscale_disp_loss([mk(0)[:, 0]], gt[:, 0])
    with pytest.raises(RuntimeError, match="3 predictions, 2 shifts"):
        ops.multiscale_disp_loss([mk(0)] * 3, gt, shifts=(0, 0))
    with pytest.raises(RuntimeError, match="float32"):
        ops.multiscale_disp_loss([mk(0).double()], gt)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.multiscale_disp_loss([mk(0).cpu()], gt)


# ---- the reference's fp64 evaluation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nd", [("dispnet", 7), ("default", 1)])
def test_golden_reference_fp64(name, nd):
    g = np.load(GOLDEN)
    gt, mask = dev(g[f"{name}_gt"]), dev(g[f"{name}_mask"])
    weights = M.DISPNET_WEIGHTS[:nd] if name == "dispnet" else (1.0,)
    counts = [n for _, n in M.ms_fwd([g[f"{name}_pred{k}"] for k in range(nd)], tuple(range(nd)), g[f"{name}_gt"], g[f"{name}_mask"],
                                     0.0, math.inf)]
    for form in ("mask", "range"):
        ps = [dev(g[f"{name}_pred{k}"]).requires_grad_() for k in range(nd)]
        if name == "dispnet":
            loss = disp_losses.dispnet_disp(ps, gt, mask) if form == "mask" else disp_losses.dispnet_disp_range(ps, gt, 64.0)
        else:
            loss = disp_losses.default_disp(ps[0], gt, mask) if form == "mask" else disp_losses.default_disp_range(ps[0], gt, 64.0)
        loss.backward()
        ratios = {"loss": M.golden_scalar_ratio(host(loss), g[f"{name}_loss64"], f"{name} {form} loss")}
        for k in range(nd):
            ratios[f"mean{k}"] = M.golden_scalar_ratio(host(loss.scale_means)[k], g[f"{name}_means64"][k], f"{name} {form} mean {k}")
            ratios[f"grad{k}"] = M.golden_grad_ratio(host(ps[k].grad), g[f"{name}_grad64_{k}"], weights[k], counts[k],
                                                     f"{name} {form} grad {k}")
        print(f"\n  {name} ({form}): err / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()), end="")
