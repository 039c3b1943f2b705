"""Which 3-D launches run on the f16x3 kernels is ONE rule (conv3d._f16_launch_ok), and the three places that need the
answer -- the forward (_conv), the input gradient (_input_grad) and the decision to have BatchNorm-backward write d(raw)
as pre-split fp16 pairs (_presplit_ok) -- get the same one for the same launch.  If _presplit_ok said yes where
_input_grad then falls back to bf16x6, the pairs would be read as floats: wrong gradients without an error.

Pure host logic: tensors are shape stand-ins, the library handle and the pack / run functions are recorders."""
import itertools

import pytest
import torch

from activezero_amd import _lib, conv3d
from activezero_amd.conv3d import CONV_S1, CONV_S2, DECONV_S2, F16X3

OFF32 = 0xffffff00  # a batch element addressed through a 32-bit buffer offset must stay below this many bytes

# The rule, one row per launch (index map, operand channels ci, result channels co): the byte limit that governs it.
#   None      taken at every size (a flat-address f16x3 kernel)
#   "element" D*H*W*max(ci, co)*4 < OFF32                                  (the depth-rolling stride-1 kernels)
#   "t2roll"  D*H*W*64*4 < OFF32 and 8*D*H*W*32*4 < OFF32                  (transposed 64 -> 32: input and 8x output)
#   "s2roll"  "element" while AZ_CONV_S2ROLL is on, None when it is off    (stride-2 32 -> 64)
#   "never"   no f16x3 kernel for these channel counts
RULE = {
    (CONV_S1, 32, 32): "element", (CONV_S1, 64, 32): "element", (CONV_S1, 64, 64): "element", (CONV_S1, 32, 64): None,
    (CONV_S2, 32, 32): None, (CONV_S2, 64, 32): None, (CONV_S2, 64, 64): None, (CONV_S2, 32, 64): "s2roll",
    (DECONV_S2, 32, 32): None, (DECONV_S2, 64, 32): "t2roll", (DECONV_S2, 64, 64): None, (DECONV_S2, 32, 64): None,
    (CONV_S1, 16, 32): "never", (CONV_S2, 32, 128): "never", (DECONV_S2, 128, 64): "never",
}
DUAL = {CONV_S1: CONV_S1, CONV_S2: DECONV_S2, DECONV_S2: CONV_S2}


def _first_over(bytes_per_voxel):
    """smallest voxel count of a batch element that no longer fits"""
    return -(-OFF32 // bytes_per_voxel)


# one below and exactly at each of the three limits (32- and 64-channel elements, the 8x output of the transposed kernel),
# a small volume and a huge one
VOXELS = sorted({1000, 1 << 40} | {v - d for v in (_first_over(128), _first_over(256), _first_over(1024)) for d in (0, 1)})


def _expected(rule, vox, ci, co, s2roll_on):
    element = vox * max(ci, co) * 4 < OFF32
    if rule == "never":
        return False
    if rule == "element":
        return element
    if rule == "t2roll":
        return vox * 64 * 4 < OFF32 and 8 * vox * 32 * 4 < OFF32
    if rule == "s2roll":
        return element or not s2roll_on
    return True


class _Shape:  # a stand-in with a tensor's shape (no 4 GiB allocation in a test)
    def __init__(self, *s):
        self.shape = torch.Size(s)


def _volume(vox, c):
    return _Shape(1, 1, 1, vox, c)


def _weight(mode, cin, cout):
    """the layer's weight in PyTorch's layout"""
    return _Shape(cin, cout, 3, 3, 3) if mode == DECONV_S2 else _Shape(cout, cin, 3, 3, 3)


class _Lib:
    def __init__(self, s2roll_on, split_ok=1):
        self.s2roll_on, self.split_ok = s2roll_on, split_ok

    def az_option(self, name):
        return {b"AZ_CONV_S2ROLL": int(self.s2roll_on)}[name]

    def az_conv3d_fwd_f16_split_ok(self, *a):
        return self.split_ok

    def az_conv3d_wgrad_f16_split_ok(self, *a):
        return 3 if self.split_ok else 0


@pytest.fixture
def launches(monkeypatch):
    """the pack and run functions of conv3d replaced by recorders: a list of (arithmetic, mode, ci, co) per launch"""
    log = []
    monkeypatch.setattr(conv3d, "_pack_f16", lambda *a, **k: ("image", "w_amax"))
    monkeypatch.setattr(conv3d, "_pack", lambda *a, **k: "image")
    monkeypatch.setattr(conv3d, "_run_f16", lambda x, pk, w_amax, mode, ci, co, *a, **k: log.append(("f16x3", mode, ci, co)))
    monkeypatch.setattr(conv3d, "_run_gather", lambda x, pk, mode, ci, co, *a, **k: log.append(("bf16x6", mode, ci, co)))
    return log


def _one(log):
    assert len(log) == 1, log
    return log.pop()


@pytest.mark.parametrize("s2roll_on", [True, False])
def test_one_rule_routes_forward_input_gradient_and_presplit(monkeypatch, launches, s2roll_on):
    monkeypatch.setattr(_lib, "lib", lambda: _Lib(s2roll_on))
    for ((op, ci, co), rule), vox in itertools.product(RULE.items(), VOXELS):
        want = _expected(rule, vox, ci, co, s2roll_on)
        operand = _volume(vox, ci)
        what = (op, ci, co, vox, s2roll_on)
        # (a) the predicate follows the table
        assert conv3d._f16_launch_ok(op, ci, co, operand) == want, what
        # (b) the launch as a layer's forward ...
        conv3d._conv(operand, _weight(op, ci, co), op, F16X3)
        assert _one(launches) == ("f16x3" if want else "bf16x6", op, ci, co), what
        # ... and as the input gradient of the layer of the dual map with the channel roles swapped
        mode, cin, cout = DUAL[op], co, ci
        conv3d._input_grad(operand, _weight(mode, cin, cout), mode, cin, cout, F16X3)
        assert _one(launches) == ("f16x3" if want else "bf16x6", op, ci, co), what
        # ... and as the reader of that layer's d(raw) (the library's own answer stubbed to yes)
        assert conv3d._presplit_ok(_volume(vox, cin), operand, mode, cin, cout, True, False) == want, what


@pytest.mark.parametrize("s2roll_on", [True, False])
@pytest.mark.parametrize("split_ok", [1, 0])
def test_presplit_gradients_only_reach_the_f16x3_input_gradient(monkeypatch, launches, s2roll_on, split_ok):
    """(c) whenever d(raw) may be written pre-split for a layer that needs its input gradient, _input_grad of that very
    tensor runs the f16x3 function -- the only one that reads such a tensor"""
    monkeypatch.setattr(_lib, "lib", lambda: _Lib(s2roll_on, split_ok))
    said_yes = 0
    for mode, cin, cout, vox, need_gw in itertools.product(DUAL, (16, 32, 64, 128), (16, 32, 64, 128), VOXELS, (False, True)):
        x, raw = _volume(vox, cin), _volume(vox, cout)
        if conv3d._presplit_ok(x, raw, mode, cin, cout, True, need_gw):
            said_yes += 1
            conv3d._input_grad(raw, _weight(mode, cin, cout), mode, cin, cout, F16X3)
            assert _one(launches)[0] == "f16x3", (mode, cin, cout, vox, need_gw, s2roll_on)
    assert (said_yes > 0) == bool(split_ok)  # (the loop did test something)
