"""CPU side of the RAFT-Stereo prediction head (K15 convex upsampling, K16 sequence loss): the fp64 checker
tests/_raft_head_ref.py against the reference's outputs (golden G14), the exported C entry points and their
host-side argument validation, and the Python surface.  No kernel is launched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build
from tests import _raft_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("az_convex_up_fwd", "az_convex_up_bwd_workspace", "az_convex_up_bwd", "az_seq_loss_fwd", "az_seq_loss_bwd")


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


def rel_close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * np.abs(b).max()


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("fp16_valued_mask", [False, True])
def test_checker_fp64_equals_the_reference_upsampling(golden, tag, fp16_valued_mask):
    g = golden("g14_raft_head")
    f, flow, mask, cot = ref.g14_upsample_inputs(g, tag)
    if fp16_valued_mask:
        mask = mask.half().float()
    key = "64_h" if fp16_valued_mask else "64"
    fl, mk = flow.double().requires_grad_(True), mask.double().requires_grad_(True)
    up = ref.convex_upsample(fl, mk, f)
    gf, gm = torch.autograd.grad(up, (fl, mk), cot.double())
    (uy, ux), (my, mx) = g["up_lat"], g["gmask_lat"]
    rel_close(up.detach()[..., ::uy, ::ux], g[f"{tag}_up{key}"])
    rel_close(gf, g[f"{tag}_gflow{key}"])
    rel_close(gm[..., ::my, ::mx], g[f"{tag}_gmask{key}"])
    # the folds: leading channel only, and the sign
    up1 = ref.convex_upsample(fl, mk, f, channels=1, negate=True)
    assert torch.equal(up1, -up[:, :1])


@pytest.mark.parametrize("n_pred", [4, 22])
def test_checker_fp64_equals_the_reference_sequence_loss(golden, n_pred):
    g = golden("g14_raft_head")
    preds, gt, valid = ref.g14_sequence_inputs(g, n_pred)
    ps = [p.double().requires_grad_(True) for p in preds]
    loss = ref.sequence_loss(ps, gt.double(), valid.double(), float(g["loss_gamma"]), float(g["max_flow"]))
    grads = torch.stack(torch.autograd.grad(loss, ps))
    st = int(g["seq_lat"])
    rel_close(loss.item(), g[f"s{n_pred}_loss64"])
    rel_close(grads[..., ::st, ::st], g[f"s{n_pred}_grads64"])
    # a disparity prediction against +gt is the same loss
    loss_d = ref.sequence_loss([-p for p in ps], gt.double(), valid.double(), float(g["loss_gamma"]),
                               float(g["max_flow"]), disparity=True)
    assert loss_d.item() == loss.item()


def test_golden_holds_arrays_only_and_is_small(golden):
    path = os.path.join(ROOT, "tests", "golden", "g14_raft_head.npz")
    assert os.path.getsize(path) < 300 * 1024
    g = golden("g14_raft_head")  # allow_pickle=False: arrays only
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


def test_new_symbols_are_exported_and_typed(handle):
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared, f"{name} missing from include/azhip.h"
        assert name in _lib._SIGS
        fn = getattr(handle, name)
        assert fn.argtypes == _lib._SIGS[name]
    assert handle.az_convex_up_bwd_workspace.restype is ctypes.c_longlong
    assert handle.az_convex_up_bwd_workspace(4, 1, 136, 240) == 4 * 9 * 136 * 240 * 4


def test_argument_validation_happens_before_any_launch(handle):
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)  # 16-byte aligned inside buf
    ENULL, EINVAL, EUNSUP, EWORK = -2, -1, -4, -5
    # az_convex_up_fwd(up, flow, mask, mask_f16, N, D, D_out, h, w, factor, mask_channels, sign, stream)
    fwd = handle.az_convex_up_fwd
    assert fwd(None, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert fwd(p, None, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert fwd(p, p, None, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert fwd(p, p, p, 0, 1, 2, 2, -1, 4, 4, 144, 1, None) == EINVAL
    assert fwd(p, p, p, 0, 1, 2, 3, 4, 4, 4, 144, 1, None) == EINVAL  # D_out > D
    assert fwd(p, p, p, 0, 1, 2, 0, 4, 4, 4, 144, 1, None) == EINVAL
    assert fwd(p, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 2, None) == EINVAL  # sign
    assert fwd(p, p, p, 0, 1, 2, 2, 4, 4, 3, 81, 1, None) == EUNSUP  # f = 3
    assert fwd(p, p, p, 0, 1, 3, 3, 4, 4, 4, 144, 1, None) == EUNSUP  # D = 3
    assert fwd(p, p, p, 0, 1, 2, 2, 4, 4, 4, 143, 1, None) == EUNSUP  # channels != 9 f^2
    assert fwd(p, p, p, 1, 1, 2, 2, 4, 4, 8, 144, 1, None) == EUNSUP
    q = ctypes.c_void_p(p.value + 4)  # up / g_up are accessed as float4
    assert fwd(q, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == EINVAL
    assert handle.az_convex_up_bwd(p, p, p, 1 << 20, q, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == EINVAL
    # az_convex_up_bwd(g_mask, g_flow, ws, ws_bytes, g_up, flow, mask, mask_f16, N, D, D_out, h, w, f, C, sign, stream)
    bwd = handle.az_convex_up_bwd
    assert bwd(None, p, p, 1 << 20, p, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert bwd(p, p, p, 1 << 20, None, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert bwd(p, p, None, 1 << 20, p, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == ENULL
    assert bwd(p, p, p, 1 << 20, p, p, p, 0, 1, 2, 2, 4, 0 - 4, 4, 144, 1, None) == EINVAL
    assert bwd(p, p, p, 1 << 20, p, p, p, 0, 1, 2, 2, 4, 4, 3, 81, 1, None) == EUNSUP
    assert bwd(p, p, p, 1 << 20, p, p, p, 0, 1, 3, 1, 4, 4, 4, 144, 1, None) == EUNSUP
    assert bwd(p, p, p, 1 << 20, p, p, p, 0, 1, 2, 2, 4, 4, 8, 144, 1, None) == EUNSUP
    assert bwd(p, p, p, 16, p, p, p, 0, 1, 2, 2, 4, 4, 4, 144, 1, None) == EWORK
    assert handle.az_convex_up_bwd_workspace(1, 0, 4, 4) == EINVAL
    # az_seq_loss_fwd(acc3, pred, gt, valid, valid_u8, max_flow, tsign, n, stream)
    assert handle.az_seq_loss_fwd(None, p, p, p, 0, 700.0, -1, 4, None) == ENULL
    assert handle.az_seq_loss_fwd(p, p, p, None, 1, 700.0, -1, 4, None) == ENULL
    assert handle.az_seq_loss_fwd(p, p, p, p, 0, 700.0, -1, -4, None) == EINVAL
    assert handle.az_seq_loss_fwd(p, p, p, p, 0, 700.0, 0, 4, None) == EINVAL
    # az_seq_loss_bwd(g, pred, gt, valid, valid_u8, max_flow, tsign, gloss, acc3, weight, n, stream)
    assert handle.az_seq_loss_bwd(p, p, p, p, 0, 700.0, -1, None, p, 1.0, 4, None) == ENULL
    assert handle.az_seq_loss_bwd(None, p, p, p, 0, 700.0, -1, p, p, 1.0, 4, None) == ENULL
    assert handle.az_seq_loss_bwd(p, p, p, p, 0, 700.0, 3, p, p, 1.0, 4, None) == EINVAL


def test_ops_refuse_cpu_tensors():
    from activezero_amd import ops

    flow, mask = torch.zeros(1, 2, 4, 4), torch.zeros(1, 144, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.convex_upsample(flow, mask, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.convex_upsample(flow, mask.half(), 4, channels=1, negate=True)
    pred = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sequence_loss([pred, pred], pred, torch.ones_like(pred))
    with pytest.raises(AssertionError):
        ops.sequence_loss([], pred, torch.ones_like(pred))


def test_module_surface():
    import inspect

    from activezero_amd import ops
    from activezero_amd.nets.raft import upsample
    from activezero_amd.utils import seq_losses

    assert list(inspect.signature(upsample.upsample_flow).parameters) == ["flow", "mask", "factor"]
    assert list(inspect.signature(upsample.upsample_disparity).parameters) == ["flow", "mask", "factor"]
    sig = inspect.signature(seq_losses.sequence_loss)  # the reference's signature, utils/losses.py:34
    assert list(sig.parameters) == ["flow_preds", "flow_gt", "valid", "loss_gamma", "max_flow"]
    assert sig.parameters["loss_gamma"].default == 0.9 and sig.parameters["max_flow"].default == 700
    sig = inspect.signature(ops.convex_upsample)
    assert list(sig.parameters) == ["flow", "mask", "factor", "channels", "negate"]
    sig = inspect.signature(ops.sequence_loss)
    assert list(sig.parameters)[:6] == ["flow_preds", "flow_gt", "valid", "loss_gamma", "max_flow", "check"]
    assert sig.parameters["check"].default is False


def test_sequence_weights_follow_the_reference_rule():
    w = ref.sequence_weights(22, 0.9)
    assert w[-1] == 1.0 and abs(w[0] - 0.9 ** 15) < 1e-15
    assert ref.sequence_weights(1) == [1.0]


def test_isa_lint_passes_on_the_built_library(handle):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint

    assert os.path.exists(isa_lint.OBJDUMP), f"{isa_lint.OBJDUMP} is missing: the packed-fp32 lint cannot run"
    bad = isa_lint.risky_packed_ops(_lib.LIB_PATH)
    assert not bad, "\n".join(f"{k}: {i}" for k, i in bad[:20])
