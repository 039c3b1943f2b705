"""Autograd wrappers of the MFMA 3-D convolution family (include/azhip.h K4/K5).

Volumes are channels-last tensors [B, D, H, W, C] (C in {32, 64}); weights stay in
PyTorch's native layouts ([Cout,Cin,3,3,3] for Conv3d, [Cin,Cout,3,3,3] for
ConvTranspose3d) so the reference state-dict loads unchanged -- the kernels read a
packed copy made per call by az_conv3d_pack_weights (110-442 KB, L2 resident).

Every layer's three passes map onto the same gather kernel (mode 0/1/2 = stride-1
conv, stride-2 conv, stride-2 transposed conv) with differently packed weights:

    layer                 forward      input gradient            weight gradient
    Conv3d stride 1       mode 0       mode 0, flipped+swapped   wgrad(dy, x, 1)
    Conv3d stride 2       mode 1       mode 2, swapped           wgrad(dy, x, 2)
    ConvTranspose3d s2    mode 2       mode 1, as stored         wgrad(x, dy, 2)
"""
import collections
import os

import torch

from . import _lib, overlap, packing, profiler
from .amax import AMAX_SLOTS, ZEROS, absmax, debug_check, _get_amax, _set_amax, weight_amax
from .handover import slot_contribute, slot_leftover, slot_register, sum_parts
from .ops import _call, _chk, _p, _stream

CONV_S1, CONV_S2, DECONV_S2 = 0, 1, 2
FP32, BF16X6, F16X3 = 0, 1, 3
_PREC = {"fp32": FP32, "bf16x6": BF16X6, "f16x3": F16X3}
# "f16x3" (precision 3): operands scaled by a power of two from the tensor's largest magnitude and split into two fp16
# parts, three MFMAs per product, fp32 accumulation (include/azhip.h, az_roll_common.h; per-layer error against fp64 at
# bf16x6's level and below torch's fp32 convolution, tools/f16x3_probe.py).  It is used wherever an f16x3 kernel exists
# for the launch (_f16_launch_ok, _f16_wgrad_ok below); other shapes run on bf16x6.  As the arithmetic of the BACKWARD
# matrix kernels it is on by default with a bf16x6 forward; AZ_BWD_F16=0 (read once) keeps every gradient on the
# forward's arithmetic, for A/B runs.
_BWD_F16 = os.environ.get("AZ_BWD_F16", "1") != "0"
# Pre-split gradients (round 5; include/azhip.h "S2 format"): the BatchNorm-backward apply pass writes d(raw) as the two
# scaled fp16 parts its two readers -- the layer's f16x3 input- and weight-gradient kernels -- would otherwise compute
# while staging, wherever BOTH of them take such an operand (az_conv3d_*_split_ok).  AZ_PRESPLIT=0 (read once): fp32
# gradients everywhere, split by the consumers (round 4), for A/B runs.
PRESPLIT = os.environ.get("AZ_PRESPLIT", "1") != "0"
# include/azhip.h precision 2: the bf16x6 arithmetic on the depth-rolling 16x16x32 kernel (az_conv3d_roll.hip),
# which reads its own packed-weight layout.  Not an arithmetic a caller chooses: _layout() routes the stride-1
# layers with 32 output channels (the V0 layers and their input gradients) there.  AZ_CONV_ROLL=0 (read once)
# keeps them on az_conv3d_m128.hip for A/B runs.
BF16X6_R16 = 2
_ROLL = os.environ.get("AZ_CONV_ROLL", "1") != "0"


_OFF32 = 0xffffff00  # the depth-rolling kernels address ONE batch element through a 32-bit buffer offset


def _fits32(x, cin, cout):
    """the volume x ([B,D,H,W,C] tensor or LazyCostVolume) fits the 32-bit offsets of the depth-rolling kernels"""
    if isinstance(x, LazyCostVolume):
        return True
    _, d, h, w, _ = x.shape
    return d * h * w * max(cin, cout) * 4 < _OFF32


def _fits32_transposed(x, op_cin, op_cout):
    """transposed 64 -> 32 launches (the depth-rolling kernel of az_conv3d_t2roll.hip, 32-bit offsets): both the coarse
    input and the eight-times-larger fine output of a batch element must stay below 4 GiB"""
    if not (op_cin == 64 and op_cout == 32):
        return True
    _, d, h, w, _ = x.shape
    return d * h * w * 64 * 4 < _OFF32 and 8 * d * h * w * 32 * 4 < _OFF32


def _layout(precision, mode, op_cout, fits32=True):
    """precision code the C ABI is called with (packing and launch must agree)"""
    if precision == BF16X6 and mode == CONV_S1 and op_cout == 32 and _ROLL and fits32:
        return BF16X6_R16
    return precision


# ---- which launch a pass of a layer is, and whether the f16x3 kernels take it ------------------------------------------
# A LAUNCH is the operation actually run: its index map (mode), the channel counts of the operand it reads and of the
# result it writes, and the weight image (strides of the output- and input-channel index in the stored weight, flip).
def _fwd_launch(weight, mode):
    """(cin, cout, stride_out, stride_in) of a layer's forward launch from its weight in PyTorch's layout"""
    if mode == DECONV_S2:  # [Cin, Cout, 27]
        cin, cout = weight.shape[0], weight.shape[1]
        return cin, cout, 27, cout * 27
    cout, cin = weight.shape[0], weight.shape[1]
    return cin, cout, cin * 27, 27


def _dgrad_launch(mode, cin, cout):
    """(op mode, op cin, op cout, stride_out, stride_in, flip) of the launch that turns the gradient of a layer's output
    into that of its input: a forward launch cout -> cin of the dual map (module docstring)"""
    if mode == CONV_S1:    # flipped taps, channels swapped
        return CONV_S1, cout, cin, 27, cin * 27, True
    if mode == CONV_S2:    # transposed conv of dy with W[co][ci][k]
        return DECONV_S2, cout, cin, 27, cin * 27, False
    return CONV_S2, cout, cin, cout * 27, 27, False  # stride-2 conv of dy with Wt[ci][co][k]


def _f16_fwd_ok(mode, cin, cout):
    """shapes with an f16x3 forward kernel (operand `cin` channels -> `cout`)"""
    return cin in (32, 64) and cout in (32, 64)


def _f16_dgrad_ok(mode, cin, cout):
    """layers whose input gradient has an f16x3 kernel: it is a forward launch dy [cout] -> dx [cin] of the dual map"""
    return _f16_fwd_ok(*_dgrad_launch(mode, cin, cout)[:3])


def _f16_wgrad_ok(mode, cin, cout):
    return cin in (32, 64) and cout in (32, 64)


def _f16_launch_ok(op_mode, ci, co, operand):
    """THE routing rule of the f16x3 forward-type kernels: the launch (op_mode, ci -> co) reading `operand`
    ([B,D,H,W,ci]) runs on one of them; otherwise it runs on bf16x6.  A shape has a kernel (_f16_fwd_ok), and where that
    kernel addresses a batch element through 32-bit offsets the element must fit them (a batch element >= 4 GiB goes to
    the flat-address bf16x6 kernels).  _conv asks with the layer's forward launch, _input_grad and
    _presplit_ok with _dgrad_launch's: an answer that differed between them would hand pre-split pairs to a kernel
    that reads floats."""
    if not _f16_fwd_ok(op_mode, ci, co):
        return False
    if op_mode == DECONV_S2:  # az_conv3d_t2roll.hip (64 -> 32): the input and the eight-times-larger output
        return _fits32_transposed(operand, ci, co)
    if _fits32(operand, ci, co):
        return True
    if op_mode == CONV_S1:    # the two depth-rolling stride-1 kernels: az_conv3d_roll.hip (-> 32) and its 64 -> 64 form
        return not (co == 32 or ci == co == 64)
    # stride 2, 32 -> 64 (hourglass conv1 forward, conv6 input gradient): the depth-rolling kernel of az_conv3d_s2roll.hip
    # (AZ_CONV_S2ROLL=0: the gather kernel, flat addresses)
    return not (ci == 32 and co == 64 and _lib.lib().az_option(b"AZ_CONV_S2ROLL") != 0)


class Arith(collections.namedtuple("Arith", "conv wgrad sink bwd16", defaults=(None, False))):
    """Arithmetic of the MFMA kernels, passed with every call (no process-wide switch):
      fp32   -- v_mfma_f32_32x32x2_f32, bit-exact fp32 FMA chain (157 TFLOP/s peak)
      bf16x6 -- exact 3-way bf16 split of both operands, six bf16 MFMAs per product, fp32
                accumulate: fp32-class accuracy (measured ~1e-7 relative) at 2.7x the rate
    `conv` covers forward / input-gradient / transposed kernels, `wgrad` the weight gradients.
    `sink` (overlap.Sink or None) is not arithmetic but travels the same way, with every call: when set, the
    weight-gradient kernels of this forward/backward pass run on its side stream (overlap.py).
    `bwd16`: input and weight gradients on the f16x3 kernels where one exists for the shape (default with bf16x6;
    never with fp32, the exact mode)."""
    __slots__ = ()

    @classmethod
    def of(cls, conv="bf16x6", wgrad=None, bwd16=None):
        w = wgrad if wgrad is not None else conv
        if bwd16 is None:
            bwd16 = _BWD_F16 or conv == "f16x3"
        # (the weight-gradient kernels know fp32 and bf16x6; f16x3 reaches them through `bwd16`)
        return cls(_PREC[conv], BF16X6 if w == "f16x3" else _PREC[w], None, bool(bwd16) and conv != "fp32" and w != "fp32")

    @property
    def names(self):
        inv = {v: k for k, v in _PREC.items()}
        return inv[self.conv], ("f16x3" if self.bwd16 else inv[self.wgrad])


# the default is read ONCE from the environment and never mutated afterwards
DEFAULT_ARITH = Arith.of(os.environ.get("AZ_CONV_PRECISION", "f16x3"), os.environ.get("AZ_WGRAD_PRECISION"))


def _arith(a):
    if a is None:
        return DEFAULT_ARITH
    if isinstance(a, str):
        return Arith.of(a)
    return a


def _dims(x):
    b, d, h, w, c = x.shape
    return b, d, h, w, c


def _out_dims(mode, d, h, w):
    if mode == CONV_S1:
        return d, h, w
    if mode == CONV_S2:
        return (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return 2 * d, 2 * h, 2 * w


def _pack(weight, op_cin, op_cout, stride_out, stride_in, flip, precision, cache=False):
    w = _chk(weight.detach().contiguous(), "weight")

    def make():
        n = _lib.lib().az_conv3d_packed_floats(op_cin, op_cout, precision)
        packed = torch.empty(n, dtype=torch.float32, device=w.device)
        _call("az_conv3d_pack_weights", _p(packed), _p(w), op_cin, op_cout, stride_out, stride_in,
              int(flip), precision, _stream())
        packed.az_precision = precision  # the layout travels with the buffer: _run_gather launches what was packed
        return packed

    key = (packing.cache_key(weight), op_cin, op_cout, stride_out, stride_in, bool(flip), precision) if cache else None
    return packing.memo(packing.PACK_CACHE, key, make, (weight,), 256)


def eval_affine(bn, like, cache=False):
    """(scale, shift) of an eval-mode BatchNorm: gamma/sqrt(running_var+eps), beta - running_mean*scale."""
    c = bn.num_features
    src = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)

    def make():
        for t, name in zip(src[:4], ("weight", "bias", "running_mean", "running_var")):
            _chk(t, "BatchNorm " + name)
        scale, shift = like.new_empty(c), like.new_empty(c)
        _call("az_bn3d_eval_affine", _p(scale), _p(shift), _p(bn.weight.detach()), _p(bn.bias.detach()),
              _p(bn.running_mean), _p(bn.running_var), float(bn.eps), c, _stream())
        return scale, shift

    return packing.memo(packing.AFFINE_CACHE, (packing.cache_key(*src), float(bn.eps)) if cache else None, make, src, 512)


def _pack_forward(weight, mode, precision, cache=False, lazy=False, fits32=True):
    cin, cout, s_out, s_in = _fwd_launch(weight, mode)
    if not lazy:  # (the fused cost-volume operand, src = 1, stays on the 32x32x16 kernels)
        precision = _layout(precision, mode, cout, fits32)
    return _pack(weight, cin, cout, s_out, s_in, False, precision, cache), cin, cout


def _peak(precision):
    """MFMA roofline of the arithmetic in use, in fp32-equivalent TFLOP/s: the fp32 MFMA dense
    peak, or the bf16 dense peak divided by the six bf16 MFMAs one fp32 product costs."""
    if precision == F16X3:
        return _PEAK_F16
    return (157.3, "fp32 MFMA") if precision == FP32 else (2500.0 / 6.0, "bf16x6: bf16 MFMA peak / 6")


def _conv_flops(b, vox_out, cin, cout, mode):
    taps = 27.0 / 8.0 if mode == DECONV_S2 else 27.0
    return 2.0 * taps * cin * cout * b * vox_out


class LazyCostVolume:
    """The PSMNet concat cost volume as a recipe (left/right NHWC features + number of
    disparity planes) instead of a [B,d,h,w,64] tensor: the first convolution
    synthesises its operand on the fly (az_conv3d_fwd, src = 1)."""

    def __init__(self, feat_l_nhwc, feat_r_nhwc, ndisp):
        self.fl, self.fr, self.ndisp = _chk(feat_l_nhwc, "feat_l"), _chk(feat_r_nhwc, "feat_r"), int(ndisp)
        if self.fl.shape != self.fr.shape or self.fl.shape[-1] != 32:
            raise RuntimeError("fused cost volume expects two [B,h,w,32] feature maps")


def _run_gather(x, packed, mode, cin, cout, precision, scale=None, shift=None, residual=None, relu=False,
                stats=False, tag="conv3d"):
    if isinstance(x, LazyCostVolume):
        if stats or mode != CONV_S1 or cin != 64:
            raise RuntimeError("the fused cost-volume operand is only wired for the eval-mode dres0[0] conv")
        b, h, w, _ = x.fl.shape
        d = x.ndisp
        out = x.fl.new_empty(b, d, h, w, cout)
        with profiler.scope(f"{tag}_costvol_m0_{cin}_{cout}", flops=_conv_flops(b, d * h * w, cin, cout, mode),
                            peak=_peak(precision)):
            _call("az_conv3d_fwd", _p(out), _p(x.fl), _p(x.fr), _p(packed), _p(scale), _p(shift),
                  _p(residual), int(relu), mode, 1, getattr(packed, "az_precision", precision), b, cin, cout, d, h, w,
                  _stream())
        return out
    b, d, h, w, c = _dims(x)
    assert c == cin, (c, cin)
    precision = getattr(packed, "az_precision", precision)  # (BF16X6_R16 for the layers _layout() routes there)
    if mode == CONV_S2 and ((d % 2 and d != 1) or h % 2 or w % 2):
        raise RuntimeError("stride-2 layers need even D/H/W (as PSMNet's hourglass does; D = 1: a 2-D layer)")
    do, ho, wo = _out_dims(mode, d, h, w)
    out = x.new_empty(b, do, ho, wo, cout)
    flops = _conv_flops(b, do * ho * wo, cin, cout, mode)
    name = f"{tag}_m{mode}_{cin}_{cout}"
    if stats:
        ntiles = _lib.lib().az_conv3d_stats_tiles(mode, precision, b, cin, cout, d, h, w)
        if ntiles <= 0:
            raise RuntimeError(f"az_conv3d_stats_tiles: {ntiles}")
        part = x.new_empty(cout, ntiles, 2)
        cnt = x.new_empty(ntiles)
        with profiler.scope(name, flops=flops, peak=_peak(precision)):
            _call("az_conv3d_fwd_stats", _p(out), _p(part), _p(cnt), _p(x), None, _p(packed), mode, 0,
                  precision, b, cin, cout, d, h, w, _stream())
        return out, part, cnt, ntiles
    with profiler.scope(name, flops=flops, peak=_peak(precision)):
        _call("az_conv3d_fwd", _p(out), _p(x), None, _p(packed), _p(scale), _p(shift), _p(residual),
              int(relu), mode, 0, precision, b, cin, cout, d, h, w, _stream())
    return out


# ---- f16x3 (include/azhip.h, az_roll_common.h) ---------------------------------------------------------------------
_PEAK_F16 = (2500.0 / 3.0, "f16x3: fp16 MFMA peak / 3")


def _pack_f16(weight, op_cin, op_cout, stride_out, stride_in, flip, mode, cache=False):
    """`mode`: the index map the packed buffer will be launched with (it selects the kernel, hence the layout)"""
    w = _chk(weight.detach().contiguous(), "weight")

    def pack_now(packed, w_amax):
        _call("az_conv3d_pack_weights_f16", _p(packed), _p(w), _p(w_amax), op_cin, op_cout, stride_out, stride_in,
              int(flip), mode, _stream())

    def make():
        w_amax = weight_amax(weight, w)
        packed = torch.empty(_lib.lib().az_conv3d_packed_floats_f16(op_cin, op_cout), dtype=torch.float32, device=w.device)
        pack_now(packed, w_amax)
        return packed, w_amax

    if cache:
        key = (packing.cache_key(weight), op_cin, op_cout, stride_out, stride_in, bool(flip), F16X3, mode)
        hit = packing.memo(packing.PACK_CACHE, key, make, (weight,), 256)
        debug_check(w, hit[1])
        return hit
    kind = _lib.lib().az_conv3d_f16_layout(mode, op_cin, op_cout)
    if kind < 0:
        raise RuntimeError(f"az_conv3d_f16_layout({mode}, {op_cin}, {op_cout}): {kind}")
    hit = packing.planned_pack(weight, w, kind, op_cin, op_cout, op_cin, op_cout, stride_out, stride_in, 27, flip, pack_now)
    return hit if hit is not None else make()


def _is_split(t):
    """the tensor holds pre-split fp16 pairs, not floats (set by _ConvBN.backward on the d(raw) it asked az_bn3d_bwd to
    write that way; the amax attached to it is the producer's bound)"""
    return getattr(t, "az_split", False)


def _run_f16(x, packed, w_amax, mode, cin, cout, scale=None, shift=None, residual=None, relu=False, stats=False,
             tag="conv3d"):
    b, d, h, w, c = _dims(x)
    assert c == cin, (c, cin)
    do, ho, wo = _out_dims(mode, d, h, w)
    out = x.new_empty(b, do, ho, wo, cout)
    name = f"{tag}_m{mode}_{cin}_{cout}"
    flops = _conv_flops(b, do * ho * wo, cin, cout, mode)
    split = _is_split(x)
    x_amax = _get_amax(x) if split else absmax(x)
    if split and (stats or x_amax is None):
        raise RuntimeError("a pre-split tensor reached a launch that cannot read it")
    if stats:
        ntiles = _lib.lib().az_conv3d_stats_tiles_f16(mode, b, cin, cout, d, h, w)
        if ntiles <= 0:
            raise RuntimeError(f"az_conv3d_stats_tiles_f16: {ntiles}")
        part, cnt = x.new_empty(cout, ntiles, 2), x.new_empty(ntiles)
        with profiler.scope(name, flops=flops, peak=_PEAK_F16):
            _call("az_conv3d_fwd_stats_f16", _p(out), _p(part), _p(cnt), _p(x), _p(packed), _p(x_amax), _p(w_amax),
                  mode, b, cin, cout, d, h, w, _stream())
        return out, part, cnt, ntiles
    with profiler.scope(name, flops=flops, peak=_PEAK_F16):
        _call("az_conv3d_fwd_f16", _p(out), _p(x), _p(packed), _p(x_amax), _p(w_amax), int(split), _p(scale), _p(shift),
              _p(residual), int(relu), mode, b, cin, cout, d, h, w, _stream())
    return out


def _conv(x, weight, mode, precision, scale=None, shift=None, residual=None, relu=False, stats=False, cache=False,
          tag="conv3d"):
    """forward convolution of a layer from its weight in PyTorch's layout, on `precision` where a kernel for the shape
    exists (f16x3 falls back to bf16x6 otherwise); returns what _run_gather returns"""
    lazy = isinstance(x, LazyCostVolume)
    cin, cout, s_out, s_in = _fwd_launch(weight, mode)
    if precision == F16X3 and not lazy and _f16_launch_ok(mode, cin, cout, x):
        pk, w_amax = _pack_f16(weight, cin, cout, s_out, s_in, False, mode, cache)
        return _run_f16(x, pk, w_amax, mode, cin, cout, scale, shift, residual, relu, stats, tag)
    prec = BF16X6 if precision == F16X3 else precision
    packed, cin, cout = _pack_forward(weight, mode, prec, cache=cache, lazy=lazy, fits32=_fits32(x, cin, cout))
    return _run_gather(x, packed, mode, cin, cout, prec, scale, shift, residual, relu, stats, tag)


def _wgrad_f16(coarse, fine, stride, cm, cn, tag, sink=None, late_ok=True):
    """late_ok = False: the caller reads the result on the side stream right away (a slice / permute of it is the real
    gradient): no deferred epilogue"""
    b, dc, hc, wc, _ = _dims(coarse)
    _, df, hf, wf, _ = _dims(fine)
    gw = coarse.new_empty(cm, cn, 3, 3, 3)
    ws_bytes = _lib.lib().az_conv3d_wgrad_workspace(cm, cn)
    am_c, am_f = _get_amax(coarse), _get_amax(fine)
    mask = (1 if _is_split(coarse) else 0) | (2 if _is_split(fine) else 0)
    if (mask & 1 and am_c is None) or (mask & 2 and am_f is None):
        raise RuntimeError("a pre-split tensor without its producer's amax")
    with overlap.scope(sink, coarse, fine, gw, am_c, am_f):
        # on the side stream the epilogue is deferred: zeroed workspace from the pass's arena, unpack at the join (overlap.Sink)
        late = late_ok and sink is not None and sink.live and overlap.DEFER_UNPACK
        ws = sink.take_workspace(ws_bytes // 4) if late else coarse.new_empty(ws_bytes // 4)
        # (a pass over the tensor only when its producer attached none)
        am_c = am_c if mask & 1 else absmax(coarse)
        am_f = am_f if mask & 2 else absmax(fine)
        with profiler.scope(f"{tag}_wgrad_s{stride}_{cm}_{cn}", flops=2.0 * 27 * cm * cn * b * dc * hc * wc,
                            peak=_PEAK_F16):
            _call("az_conv3d_wgrad_f16", None if late else _p(gw), _p(ws), ws_bytes, _p(coarse), _p(fine), _p(am_c), _p(am_f),
                  mask, stride, b, cm, cn, dc, hc, wc, df, hf, wf, _stream())
        if late:
            sink.defer_unpack(gw, ws, cm, cn, cm, cn, 27)
        if sink is not None and sink.live:
            sink.keep.extend((am_c, am_f))
    return gw


def _weight_grad_f16(x, dy, mode, cin, cout, sink=None, late_ok=True):
    if mode == DECONV_S2:
        return _wgrad_f16(x, dy, 2, cin, cout, "deconv", sink, late_ok)
    return _wgrad_f16(dy, x, 1 if mode == CONV_S1 else 2, cout, cin, "conv", sink, late_ok)


def _wgrad(coarse, fine, stride, cm, cn, tag, precision, sink=None):
    b, dc, hc, wc, _ = _dims(coarse)
    _, df, hf, wf, _ = _dims(fine)
    gw = coarse.new_empty(cm, cn, 3, 3, 3)
    ws_bytes = _lib.lib().az_conv3d_wgrad_workspace(cm, cn)
    with overlap.scope(sink, coarse, fine, gw):  # (gw too: the engine may drop it before the join, overlap.py)
        ws = coarse.new_empty(ws_bytes // 4)
        with profiler.scope(f"{tag}_wgrad_s{stride}_{cm}_{cn}", flops=2.0 * 27 * cm * cn * b * dc * hc * wc,
                            peak=_peak(precision)):
            _call("az_conv3d_wgrad", _p(gw), _p(ws), ws_bytes, _p(coarse), _p(fine), stride, precision,
                  b, cm, cn, dc, hc, wc, df, hf, wf, _stream())
    return gw


def _input_grad(dy, weight, mode, cin, cout, precision, residual=None):
    """gradient of the layer's input from the gradient dy of its (raw) convolution output; `residual` (a tensor of the
    result's shape) is added in the kernel's epilogue: another consumer's gradient of the same tensor (handover.GradSlot)"""
    op, ci, co, s_out, s_in, flip = _dgrad_launch(mode, cin, cout)
    if precision == F16X3:
        if _f16_launch_ok(op, ci, co, dy):
            pk, w_amax = _pack_f16(weight, ci, co, s_out, s_in, flip, op)
            return _run_f16(dy, pk, w_amax, op, ci, co, residual=residual, tag="dgrad")
        precision = BF16X6
    pk = _pack(weight, ci, co, s_out, s_in, flip, _layout(precision, op, co, _fits32(dy, ci, co)))
    return _run_gather(dy, pk, op, ci, co, precision, residual=residual, tag="dgrad")


def _weight_grad(x, dy, mode, cin, cout, precision, sink=None, late_ok=True):
    if precision == F16X3:
        if _f16_wgrad_ok(mode, cin, cout):
            return _weight_grad_f16(x, dy, mode, cin, cout, sink, late_ok)
        precision = BF16X6
    if mode == DECONV_S2:
        return _wgrad(x, dy, 2, cin, cout, "deconv", precision, sink)
    return _wgrad(dy, x, 1 if mode == CONV_S1 else 2, cout, cin, "conv", precision, sink)


def _presplit_ok(x, raw, mode, cin, cout, need_gx, need_gw):
    """d(raw) of this layer may be written pre-split: every kernel that will read it -- the f16x3 input gradient (a forward
    launch of the dual map on d(raw)) and the f16x3 weight gradient -- stages such an operand by copy.  Asks the
    same questions as _input_grad (_f16_launch_ok of the same launch) and _weight_grad ask; the library answers for
    its own kernels (az_conv3d_*_split_ok)."""
    lib = _lib.lib()
    b, d, h, w, _ = raw.shape
    if need_gx:
        op, ci, co = _dgrad_launch(mode, cin, cout)[:3]
        if not _f16_launch_ok(op, ci, co, raw) or lib.az_conv3d_fwd_f16_split_ok(op, b, ci, co, d, h, w) != 1:
            return False
    if need_gw:
        if not _f16_wgrad_ok(mode, cin, cout):
            return False
        _, dx_, hx, wx, _ = x.shape
        if mode == DECONV_S2:   # coarse = x, fine = d(raw)
            ok, bit = lib.az_conv3d_wgrad_f16_split_ok(2, b, cin, cout, dx_, hx, wx, d, h, w), 2
        else:                   # coarse = d(raw), fine = x
            ok, bit = lib.az_conv3d_wgrad_f16_split_ok(1 if mode == CONV_S1 else 2, b, cout, cin, d, h, w, dx_, hx, wx), 1
        if not ok & bit:
            return False
    return bool(need_gx or need_gw)


class _ConvBN(torch.autograd.Function):
    """y = relu?( BN(conv(x, weight)) + residual ), one autograd node per convbn_3d unit."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, bn, mode, relu, arith, defer=None, x_slot=None, res_slot=None):
        ctx.x_slot, ctx.res_slot = x_slot, res_slot  # (registered by conv_bn, where autograd is on: handover.GradSlot)
        x = _chk(x, "x")  # (LazyCostVolume never reaches autograd: see conv_bn)
        if residual is not None:
            residual = _chk(residual, "residual")
        _chk(gamma, "gamma"), _chk(beta, "beta")  # (read through their pointers: a strided view of a parameter is refused)
        training = bn.training or not bn.track_running_stats
        eps = float(bn.eps)
        cin, cout = _fwd_launch(weight, mode)[:2]
        with torch.cuda.device(x.device):
            if not training:
                # eval-mode BatchNorm under autograd (fine-tuning with frozen statistics): the same
                # kernels, with the running-statistics affine map; backward below
                scale, shift = eval_affine(bn, x)
                raw = _conv(x, weight, mode, arith.conv)
                y = torch.empty_like(raw)
                y_amax = ZEROS.take(raw)
                _call("az_bn3d_apply", _p(y), _p(raw), _p(scale), _p(shift), _p(residual), int(relu),
                      raw.numel() // cout, cout, _p(y_amax), _stream())
                _set_amax(y, y_amax)
                # (1/sqrt(running_var + eps) from the statistics themselves: d gamma does not depend on gamma)
                ctx.save_for_backward(x, weight, gamma, raw, y if relu else None, bn.running_mean.clone(),
                                      scale, (bn.running_var + eps).rsqrt(), None)
                ctx.cfg = (mode, relu, residual is not None, cin, cout, arith, False)
                return y
            raw, part, cnt, ntiles = _conv(x, weight, mode, arith.conv, stats=True)
            scale, shift = x.new_empty(cout), x.new_empty(cout)
            mean, invstd = x.new_empty(cout), x.new_empty(cout)
            track = bn.track_running_stats and bn.running_mean is not None
            momentum = 0.1 if bn.momentum is None else float(bn.momentum)
            nbt = bn.num_batches_tracked if (track and bn.num_batches_tracked is not None) else None
            scratch = x.new_empty(int(_lib.lib().az_bn3d_finalize_scratch(cout))) if ntiles >= 4096 else None
            _call("az_bn3d_finalize", _p(mean), _p(invstd), _p(scale), _p(shift),
                  _p(bn.running_mean) if track else None, _p(bn.running_var) if track else None,
                  _p(part), _p(cnt), _p(gamma.detach()), _p(beta.detach()), ntiles, cout, eps,
                  momentum, _p(nbt), _p(scratch), scratch.numel() if scratch is not None else 0, _stream())
            if nbt is not None:  # the kernel wrote through raw pointers: tell the version counters (cache keys)
                packing.touched(nbt, bn.running_mean, bn.running_var)
            nvox = raw.numel() // cout
            if defer is not None and relu and residual is None:
                # the single consumer applies relu(raw * scale + shift) itself while it stages its input
                # (DeferredAffine): no apply pass, no second copy of the tensor; this node's output IS raw
                defer.scale, defer.shift = scale, shift
                y = raw
            else:
                y = torch.empty_like(raw)
                y_amax = ZEROS.take(raw)
                with profiler.scope(f"bn3d_apply_{cout}", bytes=4.0 * raw.numel() * (3 if residual is not None else 2),
                                    bound="hbm"):
                    _call("az_bn3d_apply", _p(y), _p(raw), _p(scale), _p(shift), _p(residual), int(relu),
                          nvox, cout, _p(y_amax), _stream())
                _set_amax(y, y_amax)
        # a ReLU layer without residual recomputes its mask from raw in backward (fma(raw, scale, shift) > 0)
        remask = relu and residual is None
        ctx.save_for_backward(x, weight, gamma, raw, y if (relu and not remask) else None, mean, invstd,
                              scale if remask else None, shift if remask else None)
        if arith.sink is not None and not arith.sink.owns(weight):  # see conv2d._leaf_sink
            arith = arith._replace(sink=None)
        ctx.cfg = (mode, relu, residual is not None, cin, cout, arith, True)
        # the f16x3 weight gradient scales its operand x by max |x|: keep what the forward pass knows of it
        ctx.x_amax = _get_amax(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, gamma, raw, y, mean, invstd, scale, shift = ctx.saved_tensors
        mode, relu, has_res, cin, cout, arith, training = ctx.cfg
        gy = _chk(gy.contiguous(), "grad_y")
        nvox = raw.numel() // cout
        with torch.cuda.device(gy.device):
            gy = slot_leftover(ctx, gy)
            if not training:
                # y = relu?(raw * s + t + res) with s = gamma * rinv, t = beta - running_mean * s (constants
                # of the running statistics): dz = gy * [y > 0]; d raw = dz * s; d gamma = sum dz (raw - rm) rinv;
                # d beta = sum dz.  A rarely used path (frozen-BN fine-tuning): plain tensor ops.
                # (the eval-mode forward saved running_mean's copy, the scale and 1/sqrt(running_var + eps) in these slots)
                rm, s_, rinv = mean, invstd, scale
                dz = gy * (y > 0).to(gy.dtype) if relu else gy
                dbeta = dz.sum(dim=(0, 1, 2, 3))
                dgamma = (dz * (raw - rm)).sum(dim=(0, 1, 2, 3)) * rinv
                dx_raw = (dz * s_).contiguous()
                g_res = dz if has_res else None
            else:
                lib = _lib.lib()
                dx_raw = torch.empty_like(raw)
                dz = torch.empty_like(raw) if (has_res and relu) else None
                dgamma, dbeta = gy.new_empty(cout), gy.new_empty(cout)
                coef = gy.new_empty(cout, 3)
                ws_bytes = lib.az_bn3d_bwd_workspace(nvox, cout)
                ws = gy.new_empty(ws_bytes // 4)
                # f16x3 gradients: max |dx_raw| (the operand scale) is taken by the kernel that writes dx_raw
                dx_amax = gy.new_empty(AMAX_SLOTS) if arith.bwd16 else None
                # ... and dx_raw itself is written pre-split where both of its readers stage such a tensor by copy
                split = arith.bwd16 and PRESPLIT and _presplit_ok(x, raw, mode, cin, cout, ctx.needs_input_grad[0],
                                                                  ctx.needs_input_grad[1])
                with profiler.scope(f"bn3d_bwd_{cout}", bytes=4.0 * raw.numel() * (7 if (relu and y is not None) else 5), bound="hbm"):
                    _call("az_bn3d_bwd", _p(dx_raw), _p(dz), _p(dgamma), _p(dbeta), _p(coef), _p(ws), ws_bytes,
                          _p(gy), _p(y), _p(raw), _p(mean), _p(invstd), _p(gamma.detach()), _p(scale), _p(shift),
                          int(relu), nvox, cout, _p(dx_amax), int(split), _stream())
                if dx_amax is not None:
                    _set_amax(dx_raw, dx_amax)
                if split:
                    dx_raw.az_split = True
                g_res = (dz if relu else gy) if has_res else None
            gx = gw = None
            # (the residual branch first: when this layer's own input is the same tensor's last consumer, it adds it)
            if has_res:
                g_res = slot_contribute(ctx.res_slot, plain=g_res)
            if ctx.needs_input_grad[0]:
                gx = slot_contribute(ctx.x_slot, make=lambda r: _input_grad(dx_raw, weight, mode, cin, cout,
                                                                             F16X3 if arith.bwd16 else arith.conv, r))
            if ctx.needs_input_grad[1]:
                if getattr(ctx, "x_amax", None) is not None and _get_amax(x) is None:
                    _set_amax(x, ctx.x_amax)
                gw = _weight_grad(x, dx_raw, mode, cin, cout, F16X3 if arith.bwd16 else arith.wgrad, arith.sink)
        return gx, gw, dgamma, dbeta, g_res, None, None, None, None, None, None, None


class DeferredAffine:
    """Filled by conv_bn(..., defer=this) in train mode: the returned tensor is the RAW convolution output and
    its one consumer must take relu(raw * scale + shift) (conv_logits(..., affine=this))."""

    def __init__(self):
        self.scale = self.shift = None

    @property
    def pending(self):
        return self.scale is not None


def conv_bn(x, conv, bn, mode, relu=False, residual=None, arith=None, defer=None):
    arith = _arith(arith)
    if isinstance(x, LazyCostVolume):  # inference: BN folded, operand synthesised in-kernel
        if torch.is_grad_enabled() or bn.training:
            raise RuntimeError("LazyCostVolume is an inference-only operand")
        with torch.cuda.device(x.fl.device):
            scale, shift = eval_affine(bn, x.fl, cache=True)
            return _conv(x, conv.weight, mode, arith.conv, scale, shift, residual, relu, cache=True)
    training = bn.training or not bn.track_running_stats
    if not training and not torch.is_grad_enabled():
        # inference: BatchNorm folded into the conv epilogue, packed weights / affine maps memoised
        x = _chk(x, "x")
        with torch.cuda.device(x.device):
            scale, shift = eval_affine(bn, x, cache=True)
            return _conv(x, conv.weight, mode, arith.conv, scale, shift,
                         _chk(residual, "residual") if residual is not None else None, relu, cache=True)
    w = arith.sink.weight(conv.weight) if arith.sink is not None else conv.weight
    x_slot = slot_register(x)
    res_slot = slot_register(residual) if residual is not None else None
    return _ConvBN.apply(x, w, bn.weight, bn.bias, residual, bn, mode, relu, arith, defer, x_slot, res_slot)


class _ConvLogits(torch.autograd.Function):
    """logits = Conv3d(32 -> 1)(x) + addend  (classifN[2] and the running cost sums)."""

    @staticmethod
    def forward(ctx, x, weight, addend, sink, scale=None, shift=None):
        ctx.sink = sink if (sink is not None and sink.owns(weight)) else None
        x = _chk(x, "x")
        w = _chk(weight.detach().contiguous(), "weight")
        b, d, h, wd, c = _dims(x)
        if c != 32 or tuple(w.shape) != (1, 32, 3, 3, 3):
            raise RuntimeError("classifier conv expects 32 -> 1 channels, 3x3x3")
        if addend is not None:
            addend = _chk(addend.contiguous(), "addend")
        out = x.new_empty(b, d, h, wd)
        with torch.cuda.device(x.device):
            with profiler.scope("conv3d_c1_fwd", bytes=4.0 * (x.numel() + out.numel()), bound="hbm"):
                _call("az_conv3d_c1_fwd", _p(out), _p(x), _p(w), _p(addend), _p(scale), _p(shift), b, d, h, wd, _stream())
        ctx.save_for_backward(x, w, scale, shift)
        ctx.has_add = addend is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, scale, shift = ctx.saved_tensors
        g = _chk(g.contiguous(), "grad_logits")
        b, d, h, wd, _ = _dims(x)
        gx = gw = None
        with torch.cuda.device(g.device):
            if ctx.needs_input_grad[0]:
                gx = torch.empty_like(x)
                with profiler.scope("conv3d_c1_dgrad", bytes=4.0 * (x.numel() + g.numel()), bound="hbm"):
                    _call("az_conv3d_c1_dgrad", _p(gx), _p(g), _p(w), b, d, h, wd, _stream())
            if ctx.needs_input_grad[1]:
                gw = torch.empty_like(w)
                # (scale / shift too: 32-float saved tensors that the engine frees right after this node -- the main
                #  stream's next small allocation would overwrite them before the queued side-stream kernel reads them)
                with overlap.scope(ctx.sink, x, g, gw, scale, shift), \
                        profiler.scope("conv3d_c1_wgrad", bytes=4.0 * (x.numel() + g.numel()), bound="hbm"):
                    _call("az_conv3d_c1_wgrad", _p(gw), _p(x), _p(g), _p(scale), _p(shift), b, d, h, wd, _stream())
        return gx, gw, (g if ctx.has_add else None), None, None, None


def conv_logits(x, conv, addend=None, sink=None, affine=None):
    """affine: a DeferredAffine filled by the conv_bn that produced x (x is then its raw output)."""
    sc, sh = (affine.scale, affine.shift) if (affine is not None and affine.pending) else (None, None)
    return _ConvLogits.apply(x, sink.weight(conv.weight) if sink is not None else conv.weight, addend, sink, sc, sh)


class _AddRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _chk(a, "a"), _chk(b, "b")
        y = torch.empty_like(a)
        y_amax = ZEROS.take(a)
        with torch.cuda.device(a.device):
            _call("az_add_relu", _p(y), _p(a), _p(b), 0, a.numel(), _p(y_amax), _stream())
        _set_amax(y, y_amax)
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _AddRelu.apply(a, b)


class _FanOut(torch.autograd.Function):
    """n aliases of x whose gradients are summed in ONE kernel pass (az_sum4) instead of autograd's
    n-1 pairwise adds: for a V0 tensor with four consumers that is 5 tensor passes instead of 9."""

    @staticmethod
    def forward(ctx, x, n):
        views = tuple(x.view_as(x) for _ in range(n))
        am = _get_amax(x)
        if am is not None:
            for v in views:
                _set_amax(v, am)
        return views

    @staticmethod
    def backward(ctx, *grads):
        gs = [_chk(g.contiguous(), "grad") for g in grads if g is not None]
        if not gs:
            return None, None
        with torch.cuda.device(gs[0].device):
            return sum_parts(gs), None


def fanout(x, n):
    """n views of x for n consumers (training); see _FanOut."""
    if not (torch.is_grad_enabled() and x.requires_grad) or x.numel() % 4:
        return (x,) * n
    return _FanOut.apply(x, n)


def conv_plain(x, weight, mode, arith=None):
    """Bare convolution (no BN), forward only -- used by parity tests and tools."""
    arith = _arith(arith)
    return _conv(_chk(x, "x"), weight, mode, arith.conv)
