"""GPU: K23 az_eval_mask / ops.eval_mask / gt_prep.prepare_test_mask bit for bit against the torch operator chain of the
reference's test.py:112-117, 162-193 -- F.interpolate(mode="nearest"), .type(torch.int), the compares and products -- run on the
same device, and against the numpy restatement of tests/_obj_metrics_ref.py.  Auxiliary maps at ratio 1, ratio 2, 4:3 and
an upscale, float32 and float64, every combination of the three optional terms; the count equals mask.sum(); the outputs are
fully overwritten; two calls give identical bytes; nothing synchronises."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import ops  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from activezero_amd.utils import gt_prep  # noqa: E402
from tests import _obj_metrics_ref as O  # noqa: E402

DEV = torch.device("cuda", 0)
MAX_DISP = 192
# (H, W) and the auxiliary maps' sizes: ratio 1, ratio 2, 4:3, an upscale
SIZES = [((5, 7), ((5, 7), (10, 14), (7, 10), (3, 4))),
         ((12, 21), ((12, 21), (24, 42), (16, 28), (5, 8))),
         ((12, 20), ((12, 20), (24, 40), (16, 27), (6, 10))),
         ((33, 65), ((33, 65), (66, 130), (44, 87), (20, 33)))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def torch_chain(disp, depth, exclude_bg, robot, rs):
    """test.py:112-117, 162-193 with torch's own operators, on the tensors' device"""
    H, W = disp.shape[-2:]
    mask = (disp < MAX_DISP) * (disp > 0)
    if exclude_bg:
        mask = mask * ((depth > 0) & (depth < 1.25))
    if robot is not None:
        r = F.interpolate(robot.unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False).type(torch.int)
        mask = mask * (r == 0)
    if rs is not None:
        s = F.interpolate(rs.unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False)
        mask = mask * (s > 0)
    return mask.type(torch.bool)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,aux_sizes", SIZES, ids=[f"{h}x{w}" for (h, w), _ in SIZES])
def test_eval_mask_equals_the_torch_chain(hw, aux_sizes, B, dtype):
    H, W = hw
    counts = set()
    for k, aux in enumerate(aux_sizes):
        disp, depth, robot, rs = O.eval_mask_case(B, H, W, aux, dtype, 8600 + 7 * k + H)
        d, z, r, s = dev(disp), dev(depth), dev(robot), dev(rs)
        assert r.dtype == s.dtype == (torch.float32 if dtype is np.float32 else torch.float64)
        for bg, use_r, use_s in itertools.product((False, True), repeat=3):
            kw = dict(robot_mask=r if use_r else None, realsense_depth=s if use_s else None)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                mask, count = ops.eval_mask(d, z, MAX_DISP, bg, **kw)
                again = gt_prep.prepare_test_mask(d, z, MAX_DISP, bg, **{k2: (v if v is None else v.unsqueeze(1)) for k2, v in kw.items()})
            finally:
                torch.cuda.set_sync_debug_mode("default")
            want = torch_chain(d, z, bg, r if use_r else None, s if use_s else None)
            assert mask.dtype == torch.bool and mask.shape == (B, 1, H, W) and count.dtype == torch.int32
            assert torch.equal(mask, want), (aux, bg, use_r, use_s, int((mask != want).sum()))
            assert torch.equal(mask.view(torch.uint8), want.view(torch.uint8))  # the bytes are 0 / 1
            assert torch.equal(again, mask)
            assert int(count) == int(want.sum())
            ref, n = O.eval_mask(disp, depth, MAX_DISP, bg, robot if use_r else None, rs if use_s else None)
            assert np.array_equal(mask.cpu().numpy(), ref) and n == int(count)
            counts.add(int(count))
    assert len(counts) >= 8


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_eval_mask_overwrites_its_outputs_and_repeats_itself(dtype):
    B, H, W, aux = 3, 33, 65, (44, 87)
    disp, depth, robot, rs = O.eval_mask_case(B, H, W, aux, dtype, 8700)
    d, z, r, s = dev(disp), dev(depth), dev(robot), dev(rs)
    f64 = int(dtype is np.float64)
    outs = []
    for fill in (0xA5, 0x5A):
        mask = torch.full((B, 1, H, W), fill, dtype=torch.uint8, device=DEV)
        count = torch.full((1,), -12345, dtype=torch.int32, device=DEV)
        guard = torch.full((64,), fill, dtype=torch.uint8, device=DEV)  # (allocated right after: a neighbour, not a proof)
        _call("az_eval_mask", _p(mask), _p(count), _p(d), _p(z), _p(r), f64, aux[0], aux[1], _p(s), f64, aux[0], aux[1], B, H, W,
              float(MAX_DISP), 1, 1.25, _stream())
        assert int(mask.max()) == 1 and int(count) == int(mask.sum()) > 0
        assert bool((guard == fill).all())
        outs.append((mask, count))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # identical bytes
    want, n = O.eval_mask(disp, depth, MAX_DISP, True, robot, rs)
    assert np.array_equal(outs[0][0].cpu().numpy().astype(bool), want) and n == int(outs[0][1])


def test_eval_mask_reads_float64_maps_without_a_float32_round_trip():
    """0.99999999 truncates to 0 (the robot term holds); as a float32 it would be 1.0 (the term fails)"""
    d = torch.full((1, 1, 2, 2), 50.0, device=DEV)
    z = torch.full((1, 1, 2, 2), 0.5, device=DEV)
    robot = torch.tensor([[[0.99999999, 1.0], [-0.99999999, -0.5]]], dtype=torch.float64, device=DEV)
    assert float(robot[0, 0, 0].float()) == 1.0
    mask, count = ops.eval_mask(d, z, MAX_DISP, True, robot_mask=robot)
    assert mask.view(-1).tolist() == [True, False, True, True] and int(count) == 3
    mask32, _ = ops.eval_mask(d, z, MAX_DISP, True, robot_mask=robot.float())
    assert mask32.view(-1).tolist() == [False, False, False, True]


def test_eval_mask_refuses_what_it_cannot_read():
    d = torch.zeros(2, 1, 4, 6, device=DEV)
    with pytest.raises(RuntimeError, match="float32 or float64"):
        ops.eval_mask(d, d, MAX_DISP, robot_mask=torch.zeros(2, 4, 6, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="expected \\[2,h,w\\]"):
        ops.eval_mask(d, d, MAX_DISP, realsense_depth=torch.zeros(1, 4, 6, device=DEV))
    with pytest.raises(RuntimeError, match="one shape"):
        ops.eval_mask(d, torch.zeros(2, 1, 2, 6, device=DEV), MAX_DISP)
