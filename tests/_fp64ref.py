"""fp64 references and element-wise error checks of the stride-1, pad-1, 3x3x3 convolutions on the three matrix arithmetics
of include/azhip.h (shared by tests/test_conv_error_model_cpu.py and tests/test_gpu_conv3d_s1.py; a helper module, not a
conftest).

Operands are NCDHW float tensors (x: [B,cin,D,H,W], w: [cout,cin,3,3,3], dy: [B,cout,D,H,W]).  Every operation is one
bilinear map y = op(p, q) of two operands with K products per output:

    kind    p    q    y                                   K
    fwd     x    w    conv3d(x, w)                        27 cin
    dgrad   dy   w    conv_transpose3d(dy, w)             27 cout
    wgrad   x    dy   dW = conv3d_weight(x, dy)           B D H W

Checks per output, all element-wise:
  (a) |got - exact| <= the worst-case bound of the arithmetic (bound_a): sound, it cannot flake;
  (b) |got - split_reference| <= C[arith] 2^-24 (2 + sqrt(K / 32)) S, S = sum_k |p_k q_k|: split_reference is the fp64 value
      of exactly the products the arithmetic is defined to form, so what is left of a correct kernel is fp32 accumulation
      rounding -- a random walk.  This is the check that sees a wrong arithmetic (a dropped term, a mis-scaled part);
  (c) |got - split_reference| <= C2[arith] 2^-24 sqrt(K sum_k (p_k q_k)^2): the same random walk in the 2-norm of the
      products.  sqrt(K sum (p q)^2) >= S, so at small K (c) is about as loose as (b); for zero-mean operands it grows like
      K where S sqrt(K / 32) grows like K^1.5.  On a V0-sized weight gradient (K = 1.6e6) one 16-position column counted
      twice lands at 6 times (b)'s bound and at 600 times (c)'s (measured by tests/test_gpu_conv3d_s1.py).

Every function takes a geometry `geom`; None is the 3-D family above.  A Geom2d(kh, kw, dil, stride) is a 2-D convolution with
"same" padding dil (k - 1) / 2 (3x3 d1, 3x3 d2, 1x1, 3x5; stride 2 only for the 3x3 pad-1 layer of the patch route), operands
x: [B,cin,H,W], w: [cout,cin,kh,kw], dy: [B,cout,Ho,Wo], with K = kh kw cin (fwd), kh kw cout (dgrad), B Ho Wo (wgrad)
(tests/test_gpu_conv2d_fp64.py).

A Geom3d(stride=2, transposed, in_dhw) is one of the two strided 3x3x3 layer types of the hourglass (tests/test_gpu_conv3d_s2.py):
    transposed = False  Conv3d(stride 2, pad 1): x fine [B,cin,D,H,W], w [cout,cin,3,3,3], dy coarse [B,cout,Dc,Hc,Wc] with
                        Dc = (D - 1) / 2 + 1; in_dhw = the fine size where it is odd (the input gradient cannot know it)
    transposed = True   ConvTranspose3d(stride 2, pad 1, output_padding 1): x coarse [B,cin,Dc,Hc,Wc], w [cin,cout,3,3,3],
                        dy fine [B,cout,2Dc,2Hc,2Wc]
K is PER OUTPUT there -- a border output of the stride-2 forward has fewer than 27 cin real products, an output of the
transposed map 1, 2, 4 or 8 taps x channels by its parity, a weight-gradient tap the coarse positions whose fine tap lies
inside the volume -- so products() returns the count tensor op(kind, ones, ones) and the bounds take a tensor K.
"""
import collections
import functools
import math
import struct

import torch
import torch.nn.functional as F

U = 2.0 ** -24
KINDS = ("fwd", "dgrad", "wgrad")
ARITHS = ("f16x3", "bf16x6", "fp32")

# The constants of checks (b) and (c) per arithmetic, with the largest value of err / (2^-24 (2 + sqrt(K / 32)) S) and of
# err / (2^-24 sqrt(K sum (p q)^2)) measured on an MI355X over every case of tests/test_gpu_conv3d_s1.py, at default switches
# and behind each switch of its rows in tests/test_gpu_switches.py.  The maxima sit at the smallest K (a weight gradient of
# 9 positions), where the few roundings of the chained MFMAs, the flush and the unpack are not averaged out -- but for fp32 (c):
# a forward of K = 1728 on v_mfma_f32_32x32x2_f32, which rounds every 2 products instead of every 16 or 32.
#
# The 2-D family (tests/test_gpu_conv2d_fp64.py) uses the same constants; largest err / bound of checks (b) / (c) measured on an
# MI355X per arithmetic, kind and route (the maxima again sit at the smallest K: the 1 x 1 image and the 1x1 layers):
#                                              bf16x6 (b)  (c)     f16x3 (b)  (c)
#   fwd    roll NT 2 (plain / stats / epi)        0.13   0.23         0.13   0.25
#   fwd    roll NT 4 | roll64 (f16x3)             0.16   0.25         0.28   0.48   (roll64 + stats, 32 -> 64, (134, 9, 50), groups 2)
#   fwd    generic, all NW and geometries         0.16   0.24         0.20   0.29   (1x1, 64 -> 128, (3, 5, 47))
#   dgrad  roll NT 2 (+ residual)                 0.13   0.20         0.20   0.26
#   dgrad  roll NT 4 | roll64 (+ residual)        0.16   0.25         0.27   0.45   (64 -> 32, (131, 9, 50) and (13, 64, 80))
#   dgrad  generic, all NW and geometries         0.29   0.40         0.33   0.42   (1x1, 128 -> 32, (2, 13, 22))
#   wgrad  r16 AR 0 | AR 1                        0.30   0.39         0.41   0.51   ((1, 1, 1) image)
#   wgrad  w64                                      --     --         0.38   0.47   ((1, 1, 1) image)
#   wgrad  generic 3x3 d1 / 3x3 d2 / 3x5          0.07   0.19         0.11   0.29
#   wgrad  generic 1x1                            0.29   0.37         0.42   0.52   (128 -> 32, (1, 1, 1) image)
#   patch route (bf16x6 only)   fwd               0.31   0.36                        (3 -> 32, (2, 13, 22): K = 27)
#                               dgrad             0.15   0.11
#                               wgrad             0.20   0.27                        (6 -> 32, (1, 1, 1) image)
# The walking and segmented cases (batch segments of 3 images, 770 columns for 768 / 384 / 256 / 192 workgroups, 3 to 8 row
# segments, 770 items for 200 blocks) stay below 0.13 in (b) and 0.25 in (c) but for roll64 above; check (a) peaks at 0.41
# (f16x3 r16 AR 1, (1, 1, 1) image).
#
# The strided 3-D family (tests/test_gpu_conv3d_s2.py; K per output) uses the same constants; largest err / bound of checks
# (b) / (c) measured on an MI355X at default switches per arithmetic, kind and route (the maxima sit at the outputs of the
# smallest K: one tap x 32 channels of the transposed map, a weight-gradient tap that meets one coarse position):
#                                              f16x3 (b)  (c)     bf16x6 (b)  (c)     fp32 (b)  (c)
#   fwd    s2roll (plain / stats / epi)           0.19   0.50
#   fwd    s2roll seg > 1 (V0 -> V1, B = 1)       0.22   0.60
#   fwd    t2roll (plain / stats / epi)           0.34   0.48
#   fwd    t2roll seg > 1 | + ragged seg          0.35   0.50 | 0.36  0.51
#   fwd    t2 (plain / stats / epi)               0.43   0.50         0.31   0.41
#   fwd    gather mode 1 (plain / stats / epi)    0.06   0.21         0.20   0.44       0.32   0.44
#   fwd    gather mode 2 (plain / stats / epi)    0.64   0.85         0.36   0.44       0.92   0.59
#   dgrad  s2roll | presplit | seg > 1            0.22   0.57 | 0.17  0.53 | 0.23  0.64
#   dgrad  t2roll | presplit                      0.39   0.49 | 0.33  0.51
#   dgrad  t2roll seg > 1 | + ragged seg          0.34   0.49 | 0.44  0.63
#   dgrad  t2                                     0.58   0.66         0.45   0.57
#   dgrad  gather mode 1                          0.07   0.18         0.11   0.29       0.36   0.47
#   dgrad  gather mode 2                          0.76   0.95         0.49   0.58       0.70   0.48
#   wgrad  s2r16 mask 0 | 1 | 2                   0.45   0.56 | 0.14  0.22 | 0.14  0.25
#   wgrad  s2r16 walk, mask 0 | 1 | 2             0.05   0.24 | 0.04  0.20 | 0.05  0.22
#   wgrad  one kd per wave                        0.42   0.52         0.29   0.38       0.42   0.23
# Check (a) peaks at 0.40 (s2r16 mask 0 and the one-kd f16x3 weight gradient, a tap of one coarse position); the production-size
# weight gradients (K = 195 840) stay below 0.001 in (b) and 0.03 in (c).
#
# The 1-D correlation GEMM of az_corr1d.hip (tests/test_gpu_corr_fp64.py through tests/_corr_fp64ref.py: bf16x6 only, the fp32
# `* 1 / sqrt(C)` of its epilogue granted as a zero addend) uses the same constants; largest err / bound of checks (a) / (b) / (c)
# measured on an MI355X per contraction and route (<A_KFAST,B_KFAST> instantiation, staging of the k-fast operands), over seeded
# operands, per-channel powers of two 2^-8 .. 2^8 on one operand and an all-zero row / column:
#                                               (a)    (b)    (c)
#   volume  <F,F> (strided b32 staging)         0.36   0.64   0.66   ((3, 16, 70, 20, 20): K = 16, one block)
#   d fmap1 <T,T> 16-byte staging               0.26   0.64   0.60   ((3, 16, 70, 20, 20): K = 20)
#   d fmap1 <T,T> b32 staging                   0.17   0.40   0.32   ((1, 37, 2, 36, 31): K = 31)
#   d fmap1 <F,F> (W2 = 1)                      0.05   0.08   0.10
#   d fmap2 <F,T> 16-byte staging               0.18   0.45   0.56   ((3, 16, 70, 20, 20): K = 20)
#   d fmap2 <F,T> b32 staging                   0.20   0.41   0.40   ((1, 3, 1, 2, 5): K = 2)
#   d fmap2 <F,F> (H W1 = 1)                    0.07   0.15   0.19
# The maxima again sit at the smallest K with many outputs; the model's C = 256 volume stays below 0.14 in (b) and (c), and the
# 16-byte K tails beyond k = 64 ((1, 24, 2, 68, 100): K = 100 and 68) below 0.24.
#
# The one-part arithmetics of the ConvGRU update (bf16x1, f16x1: tests/test_gpu_gru_fp64.py) have their own constants, bounds and
# table of measured maxima in tests/_gru_fp64ref.py.
#
# The 32 -> 1 classifier convolutions of az_conv3d_c1.hip (VALU, fp32: tests/test_gpu_c1_fp64.py) use the fp32 constants with a
# rounding count of their own for check (a); their table of measured maxima is in tests/_c1_fp64ref.py.
C = {
    "f16x3": 2.0,   # measured max 1.17 (wide weight gradient, 64 -> 32, (1, 1, 3, 3))
    "bf16x6": 3.0,  # measured max 1.51 (r16 AR 0 weight gradient, 64 -> 64, (1, 1, 3, 3))
    "fp32": 2.0,    # measured max 0.90 (one-kd-per-wave weight gradient, 64 -> 32, (1, 1, 3, 3))
}
C2 = {
    "f16x3": 3.5,   # measured max 1.93 (wide weight gradient, 32 -> 64, (1, 1, 3, 3))
    "bf16x6": 5.0,  # measured max 2.67 (r16 AR 0 weight gradient, 32 -> 64, (1, 1, 3, 3))
    "fp32": 8.0,    # measured max 4.16 (gather forward, 64 -> 64, (1, 13, 25, 17))
}


class Geom2d(collections.namedtuple("Geom2d", "kh kw dil stride in_hw", defaults=(1, 1, None))):
    """a 2-D geometry; in_hw: (H, W) of x where the stride leaves it open (the input gradient of a stride-2 layer)"""

    @property
    def pad(self):
        return (self.dil * (self.kh - 1) // 2, self.dil * (self.kw - 1) // 2)


class Geom3d(collections.namedtuple("Geom3d", "stride transposed in_dhw", defaults=(2, False, None))):
    """a strided 3x3x3, pad-1 geometry (module docstring); in_dhw: (D, H, W) of the fine tensor of a stride-2 convolution where
    the coarse size leaves it open (odd fine sizes)"""

    def fine(self, coarse_dhw):
        return tuple(self.in_dhw) if self.in_dhw is not None else tuple(2 * n for n in coarse_dhw)


def zero_stuff(t, fine_dhw):
    """[B,C,Dc,Hc,Wc] -> [B,C,*fine_dhw] with t at the even positions and zeros between (and behind)"""
    z = t.new_zeros(tuple(t.shape[:2]) + tuple(fine_dhw))
    z[:, :, ::2, ::2, ::2] = t
    return z


# ---- fp64 operators ---------------------------------------------------------------------------------------------------
def _op2d(kind, p, q, g):
    st, dl = g.stride, g.dil
    if kind == "fwd":
        return F.conv2d(p, q, stride=st, padding=g.pad, dilation=dl)
    if kind == "dgrad":
        opad = (0, 0)
        if st > 1:  # the rows / columns of x a stride leaves without an output position of their own
            opad = tuple(n - ((m - 1) * st - 2 * pd + dl * (k - 1) + 1) for n, m, pd, k in
                         zip(g.in_hw, p.shape[2:], g.pad, (g.kh, g.kw)))
        return F.conv_transpose2d(p, q, stride=st, padding=g.pad, dilation=dl, output_padding=opad)
    return torch.nn.grad.conv2d_weight(p, (q.shape[1], p.shape[1], g.kh, g.kw), q, stride=st, padding=g.pad, dilation=dl)


def _op3d_strided(kind, p, q, g):
    assert g.stride == 2
    if g.transposed:  # y = conv_transpose3d(x, w): its input gradient is the stride-2 convolution of dy with the same weight
        if kind == "fwd":
            return F.conv_transpose3d(p, q, stride=2, padding=1, output_padding=1)
        if kind == "dgrad":
            return F.conv3d(p, q, stride=2, padding=1)
        # dW[ci][co][k] = sum_pos x[pos][ci] dy[2 pos - 1 + k][co]: the weight gradient of conv3d(dy -> x's shape)
        return torch.nn.grad.conv3d_weight(q, (p.shape[1], q.shape[1], 3, 3, 3), p, stride=2, padding=1)
    if kind == "fwd":
        return F.conv3d(p, q, stride=2, padding=1)
    if kind == "dgrad":  # the planes / rows / columns of x an odd fine size leaves without an output position of their own
        opad = tuple(n - (2 * m - 1) for n, m in zip(g.fine(p.shape[2:]), p.shape[2:]))
        return F.conv_transpose3d(p, q, stride=2, padding=1, output_padding=opad)
    return torch.nn.grad.conv3d_weight(p, (q.shape[1], p.shape[1], 3, 3, 3), q, stride=2, padding=1)


def op(kind, p, q, geom=None):
    """the fp64 operation (torch's convolutions; any device that has them)"""
    p, q = p.double(), q.double()
    if isinstance(geom, Geom3d):
        return _op3d_strided(kind, p, q, geom)
    if geom is not None:
        return _op2d(kind, p, q, geom)
    if kind == "fwd":
        return F.conv3d(p, q, padding=1)
    if kind == "dgrad":
        return F.conv_transpose3d(p, q, padding=1)
    return torch.nn.grad.conv3d_weight(p, (q.shape[1], p.shape[1], 3, 3, 3), q, padding=1)


def _neighbourhoods(xp, b, d, h, w):
    """[h*w, 27*C] rows of plane d of batch element b of the padded channels-last volume xp (tap-major, channel-minor)"""
    taps = [xp[b, d + kd, kh:kh + h, kw:kw + w, :] for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(taps, dim=2).reshape(h * w, -1)


def _op_gemm2d(kind, p, q, g):
    """stride-1 geometries: one matrix product per image over its [H W, kh kw C] neighbourhood rows"""
    assert g.stride == 1
    if kind == "dgrad":  # conv_transpose2d(dy, w) = conv2d(dy, w with taps flipped and channels swapped)
        kind, q = "fwd", q.transpose(0, 1).flip(2, 3)
    b, c, h, w = p.shape
    ph, pw = g.pad
    taps = g.kh * g.kw
    xp = F.pad(p.permute(0, 2, 3, 1), (0, 0, pw, pw, ph, ph))  # [B, H+2ph, W+2pw, C]

    def rows(bi):
        t = [xp[bi, i * g.dil:i * g.dil + h, j * g.dil:j * g.dil + w, :] for i in range(g.kh) for j in range(g.kw)]
        return torch.stack(t, dim=2).reshape(h * w, taps * c)

    if kind == "fwd":
        cout = q.shape[0]
        wm = q.permute(2, 3, 1, 0).reshape(taps * c, cout)
        y = torch.empty(b, h * w, cout, dtype=torch.float64, device=p.device)
        for bi in range(b):
            y[bi] = rows(bi) @ wm
        return y.reshape(b, h, w, cout).permute(0, 3, 1, 2)
    cout = q.shape[1]
    acc = torch.zeros(cout, taps * c, dtype=torch.float64, device=p.device)
    for bi in range(b):
        acc += q[bi].reshape(cout, h * w) @ rows(bi)
    return acc.reshape(cout, taps, c).permute(0, 2, 1).reshape(cout, c, g.kh, g.kw)


def op_gemm(kind, p, q, geom=None):
    """the same values as op(), as unfold + float64 matrix products over depth planes: no fp64 convolution of a vendor
    library is involved (the references of the large shapes are computed this way on the GPU)"""
    p, q = p.double(), q.double()
    if isinstance(geom, Geom3d):
        return _op_gemm3d_strided(kind, p, q, geom)
    if geom is not None:
        return _op_gemm2d(kind, p, q, geom)
    return _op_gemm3d(kind, p, q, 1)


def _op_gemm3d(kind, p, q, step):
    """the stride-1 plane GEMMs.  step = 2 keeps the neighbourhood rows of the even positions only: the forward at the even
    positions, and the weight gradient against a gradient q [B,cout,Dc,Hc,Wc] that sits at the even positions of p's volume
    (what its zero-stuffed image would give: the rows of the stuffed zeros add nothing)"""
    if kind == "dgrad":  # conv_transpose3d(dy, w) = conv3d(dy, w with taps flipped and channels swapped)
        kind, q = "fwd", q.transpose(0, 1).flip(2, 3, 4)
    b, c, d, h, w = p.shape
    do, ho, wo = [(n - 1) // step + 1 for n in (d, h, w)]
    xp = F.pad(p.permute(0, 2, 3, 4, 1), (0, 0, 1, 1, 1, 1, 1, 1))  # [B, D+2, H+2, W+2, C]

    def rows(bi, di):
        if step == 1:
            return _neighbourhoods(xp, bi, di, h, w)
        taps = [xp[bi, di * step + kd, kh:kh + h:step, kw:kw + w:step, :] for kd in range(3) for kh in range(3) for kw in range(3)]
        return torch.stack(taps, dim=2).reshape(ho * wo, -1)

    if kind == "fwd":
        cout = q.shape[0]
        wm = q.permute(2, 3, 4, 1, 0).reshape(27 * c, cout)  # [(tap, ci), co]
        y = torch.empty(b, do, ho * wo, cout, dtype=torch.float64, device=p.device)
        for bi in range(b):
            for di in range(do):
                y[bi, di] = rows(bi, di) @ wm
        return y.reshape(b, do, ho, wo, cout).permute(0, 4, 1, 2, 3)
    cout = q.shape[1]
    assert tuple(q.shape[2:]) == (do, ho, wo), (q.shape, (do, ho, wo))
    g = torch.zeros(cout, 27 * c, dtype=torch.float64, device=p.device)
    for bi in range(b):
        for di in range(do):
            g += q[bi, :, di].reshape(cout, ho * wo) @ rows(bi, di)
    return g.reshape(cout, 27, c).permute(0, 2, 1).reshape(cout, c, 3, 3, 3)


def _op_gemm3d_strided(kind, p, q, g):
    """the strided maps from the stride-1 plane GEMMs: a stride-2 convolution = the stride-1 result at the even positions; a
    transposed one (and the input gradient of a stride-2 one) = the stride-1 convolution of the zero-stuffed operand with the
    weight flipped and channel-swapped; the weight gradients = the stride-1 weight gradient with the coarse operand at the even
    positions"""
    assert g.stride == 2
    if kind == "wgrad":  # p = x, q = dy; the result is [coarse channels, fine channels, 3, 3, 3] for both layer types
        return _op_gemm3d("wgrad", q, p, 2) if g.transposed else _op_gemm3d("wgrad", p, q, 2)
    if (kind == "fwd") != g.transposed:  # the stride-2 convolution of p (a transposed layer's input gradient reads w as stored)
        return _op_gemm3d("fwd", p, q, 2)
    return _op_gemm3d("dgrad", zero_stuff(p, g.fine(p.shape[2:])), q, 1)


def products(kind, p, q, geom=None):
    """K: products per output (a strided 3-D geometry: the count tensor op(kind, ones, ones), broadcast over the channels)"""
    if isinstance(geom, Geom3d):
        one_p = torch.ones((p.shape[0], 1) + tuple(p.shape[2:]), dtype=torch.float64)
        one_q = torch.ones((q.shape[0] if kind == "wgrad" else 1, 1) + tuple(q.shape[2:]), dtype=torch.float64)
        return op(kind, one_p, one_q, geom) * (1 if kind == "wgrad" else p.shape[1])
    if geom is not None:
        return q.shape[0] * q.shape[2] * q.shape[3] if kind == "wgrad" else geom.kh * geom.kw * p.shape[1]
    if kind == "wgrad":
        b, _, d, h, w = p.shape
        return b * d * h * w
    return 27 * p.shape[1]


def exact(kind, p, q, gemm=False, geom=None):
    """fp64 result and the per-output magnitude sums: S = sum |p_k q_k|, Q2 = sum (p_k q_k)^2, sum_q = sum |q_k| and
    sum_p = sum |p_k| (the sums the f16x3 amax term multiplies with the amax of p and of q).  (Padding stays zero in the
    ones.)"""
    f = functools.partial(op_gemm if gemm else op, geom=geom)
    p, q = p.double(), q.double()
    ap, aq = p.abs(), q.abs()
    return {"y": f(kind, p, q), "S": f(kind, ap, aq), "Q2": f(kind, p * p, q * q), "sum_q": f(kind, torch.ones_like(p), aq),
            "sum_p": f(kind, ap, torch.ones_like(q))}


# ---- the operand splits of the arithmetics ------------------------------------------------------------------------------
def f16_scale_exp(amax):
    """az_roll_common.h az_f16_scale_exp: k with 2^k amax in [2^14, 2^15), clamped to normal floats"""
    e = ((struct.unpack("<I", struct.pack("<f", float(amax)))[0] >> 23) & 0xFF) - 127
    return min(max(14 - e, -126), 127)


def amax_of(t):
    """largest finite magnitude, as the fp32 value the kernels see"""
    t = t.float()
    fin = t[torch.isfinite(t)]
    return float(fin.abs().max()) if fin.numel() else 0.0


def split_parts(t, arith, amax=None):
    """the parts the arithmetic multiplies, as unscaled fp64 tensors whose sum is the operand up to the split error:
    f16x3  -- x 2^k split into hi = fp16(x), lo = fp16(x - hi), both round-to-nearest (az_split2_f16_pair), k from amax;
    bf16x6 -- hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (az_split3_pair);
    fp32   -- the fp32 value itself"""
    t = t.float()
    if arith == "f16x3":
        k = f16_scale_exp(amax_of(t) if amax is None else amax)
        s = t * (2.0 ** k)
        hi = s.half()
        lo = (s - hi.float()).half()
        return [hi.double() * 2.0 ** -k, lo.double() * 2.0 ** -k]
    if arith == "bf16x6":
        hi = t.bfloat16()
        r = t - hi.float()
        mid = r.bfloat16()
        lo = (r - mid.float()).bfloat16()
        return [hi.double(), mid.double(), lo.double()]
    return [t.double()]


def split_reference(kind, p, q, arith, parts_p=None, parts_q=None, gemm=False, geom=None):
    """fp64 value of exactly the products the arithmetic forms:
    f16x3  -- hi*hi + hi*lo + lo*hi (lo*lo dropped);
    bf16x6 -- the six products of az_conv3d_wgrad16.hip's chain: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi (mid*lo,
              lo*mid, lo*lo dropped);
    fp32   -- the fp32 operands' exact bilinear form.
    parts_p / parts_q: parts already split (a pre-split tensor decoded from its bits) in place of split_parts().
    The 2-D kernels form the same sets: az_mfma6 / az_mfma6_now / r16_step of az_common.h and az_roll_common.h multiply hi*hi,
    hi*mid, mid*hi, mid*mid, hi*lo, lo*hi; az_mfma3_* / r16_step3 / r16_chain9 hi*hi, hi*lo, lo*hi."""
    f = functools.partial(op_gemm if gemm else op, geom=geom)
    pp = parts_p if parts_p is not None else split_parts(p, arith)
    qq = parts_q if parts_q is not None else split_parts(q, arith)
    if arith == "f16x3":
        return f(kind, pp[0], qq[0] + qq[1]) + f(kind, pp[1], qq[0])
    if arith == "bf16x6":
        return f(kind, pp[0], qq[0] + qq[1] + qq[2]) + f(kind, pp[1], qq[0] + qq[1]) + f(kind, pp[2], qq[0])
    return f(kind, pp[0], qq[0])


# ---- the two checks -----------------------------------------------------------------------------------------------------
def rounding_count(arith, K, blocks=None):
    """fp32 roundings an output may see in the worst case: every MFMA rounds the accumulator it is chained into (f16x3: 3
    per 16-deep block of v_mfma_*_f16, bf16x6: 6 per 16-deep block, fp32: v_mfma_f32_32x32x2_f32 rounds each of its 2
    products and adds), plus one fp32 add per block for block sums and partial-sum flushes, plus 3 for the epilogue.

    The 2-D kernels, read against this count:
      * az_conv2d.hip (forward / input gradient): per tap and 16-channel chunk one 16-deep block of 3 / 6
        v_mfma_f32_32x32x16 chained from ZERO in a block temporary (az_mfma6_step / _now, az_mfma3_*) and one fp32 add of the
        temporary into the accumulator -- its acc[0..3] are four M tiles, not partial sums of one output.  kh kw cin / 16
        blocks = ceil(K / 16) exactly (cin % 16 == 0; the patch route's K = 9 cin is padded with zero products to Kp = 32 / 64:
        ceil(27 / 16) = 32 / 16, ceil(54 / 16) = 64 / 16), so chain + blocks covers it.
      * az_conv2d_roll.hip: 32-deep blocks (r16_step / r16_step3: 6 / 3 v_mfma_f32_16x16x32 from zero + one add; roll64's
        r16_chain9: nine MFMAs over three 32-deep blocks + one add): half as many chain roundings as counted, and at most as
        many adds.
      * the weight gradients: their K blocks are not K / 16 consecutive positions but (image, row or row pair, 16-position
        chunk) pieces -- az_conv2d_wgrad.hip one 16-deep block per output row and chunk, az_conv2d_wgrad16.hip one 32-deep
        block per PAIR of rows and chunk -- so a ragged W (W = 47: three chunks, the last 15 / 16 full) gives an output up to
        B H ceil(W / 16) blocks with non-zero products where ceil(B H W / 16) would count fewer.  `blocks` carries that number
        (wgrad_blocks_2d); every block is 3 / 6 MFMAs chained into the running accumulator (no temporary there).  The flushes:
        one atomicAdd per workgroup and output, at most one workgroup per column = (image, chunk, row segment) <= B ceil(W / 16)
        H, within the `+ blocks` adds; the unpack copies.

    The strided 3-D kernels (K is a tensor there: an MFMA whose products are all padding adds an exact zero and rounds nothing,
    so the count of an output follows its own K):
      * az_conv3d_s2roll.hip: per (kd, kh, kw) tap one 32-deep block (cin = 32) of 3 v_mfma_f32_16x16x32 chained into the running
        accumulator (mul4: w_hi x_hi, w_hi x_lo, w_lo x_hi), no temporary and no add; the plane-to-plane move acc[0] = acc[1]
        is a copy.  3 per 32 products where 3 per 16 + 1 are counted.
      * az_conv3d_t2roll.hip: a chain = the one or two ow taps of one (kd group, phase, row offset oh, 32-channel chunk): 3 or 6
        v_mfma_f32_16x16x32 from ZERO in a temporary + one VALU add per chain and tile into the phase accumulator; the carried
        kd = 2 set is a register copy (rotate).  An output of parity (1, 1, 1), 64 channels: 8 chains of 6 + 8 adds = 56
        where 3 * 32 + 32 are counted.
      * az_conv3d_t2.hip and the mode-1 / mode-2 gather kernel of az_conv3d.hip: per tap and 16-channel chunk (t2) / per tap
        and 32-channel chunk as two 16-deep blocks (gather f16x3: 6 MFMAs from zero + one add; bf16x6: az_mfma6 / _now) -- at
        most 3 / 6 per 16 products + one add per block, exactly what is counted; fp32: one rounding per product and add.
      * az_conv3d_wgrad16s2.hip: a step = 32 positions = 4 coarse rows x 8 positions of one (image, coarse plane, 8-position
        chunk) column, 3 v_mfma_f32_16x16x32 chained into the running accumulator.  Ragged rows and chunks make more steps than
        ceil(K / 32): B Dc ceil(Hc / 4) ceil(Wc / 8) (wgrad_blocks_s2(dy, 4, 8)), passed as `blocks`; the flush is one
        atomicAdd per persistent workgroup <= the columns B Dc ceil(Wc / 8), within the `+ blocks` adds; o_scale is a power of
        two; the unpack copies.
      * the stride-2 instantiations of az_conv3d_wgrad.hip (one kd per wave): one 16-position block per coarse row and
        16-position chunk, 3 / 6 MFMAs chained into the accumulator (fp32: 2 roundings per position): B Dc Hc ceil(Wc / 16)
        blocks (wgrad_blocks_s2(dy, 1, 16)); one atomicAdd per wave <= the (image, plane, row segment, chunk) items."""
    if torch.is_tensor(K):  # per-output K (a strided geometry): the same count, element-wise
        kb = torch.ceil(K / 16.0)
        blocks = kb if blocks is None else kb.clamp_min(float(blocks))
    else:
        blocks = math.ceil(K / 16) if blocks is None else max(blocks, math.ceil(K / 16))
    chain = {"f16x3": 3 * blocks, "bf16x6": 6 * blocks, "fp32": 2 * K}[arith]
    return chain + blocks + 3


def wgrad_blocks_2d(dy):
    """K blocks with non-zero products an output of a 2-D weight gradient may see (rounding_count): B H ceil(W / 16) for
    a gradient dy [B, C, H, W]"""
    b, _, h, w = dy.shape
    return b * h * ((w + 15) // 16)


def wgrad_blocks_s2(coarse, rows, chunk):
    """K blocks an output of a stride-2 / transposed weight gradient may see (rounding_count): B Dc ceil(Hc / rows)
    ceil(Wc / chunk) for a coarse operand [B, C, Dc, Hc, Wc] -- (4, 8): az_conv3d_wgrad16s2.hip, (1, 16): az_conv3d_wgrad.hip"""
    b, _, d, h, w = coarse.shape
    return b * d * ((h + rows - 1) // rows) * ((w + chunk - 1) // chunk)


def bound_a(arith, K, ex, amax_p, amax_q, blocks=None):
    """the worst-case bound (check a).  f16x3: include/azhip.h "CONTRACT of a caller-supplied amax",
        [3 * 2^-22 + n * 2^-24] * S + 2^-38 * (A_p * sum |q| + A_q * sum |p|)
    (3 * 2^-22: the two-part split of both operands and the dropped lo*lo; 2^-38 A: the fp16 subnormal spacing of `lo`),
    with n = rounding_count(): the header's K / 32 + 3 counts one add per 32-deep block sum, the kernels that chain their
    three MFMAs into the running accumulator round up to 3 K / 16 times.
    bf16x6: 5 * 2^-24 * S for the split (hi + mid + lo = x up to 2^-24 |x| per operand, the dropped mid*lo and lo*mid up to
    2^-24 |x y| each) + n * 2^-24 * S.  fp32: n * 2^-24 * S (the operands are exact)."""
    rep = {"f16x3": 12.0, "bf16x6": 5.0, "fp32": 0.0}[arith]
    lim = (rep + rounding_count(arith, K, blocks)) * U * ex["S"]
    if arith == "f16x3":
        lim = lim + 2.0 ** -38 * (amax_p * ex["sum_q"] + amax_q * ex["sum_p"])
    return lim


def bound_b(arith, K, ex):
    """the random-walk accumulation bound against split_reference (check b)"""
    root = (K / 32.0).sqrt() if torch.is_tensor(K) else math.sqrt(K / 32.0)
    return C[arith] * U * (2.0 + root) * ex["S"]


def bound_c(arith, K, ex):
    """the random-walk bound in the 2-norm of the products (check c)"""
    return C2[arith] * U * (K * ex["Q2"]).sqrt()


def _ratio(err, lim):
    """max err / lim; an output with lim = 0 (every product is zero: padding) must be exactly zero"""
    pos = lim > 0
    if bool((err[~pos] != 0).any()):
        return float("inf")
    return float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0


def check(got, arith, K, ex, sref, amax_p=0.0, amax_q=0.0, addend=None, blocks=None, epilogue=None):
    """the three checks for every output; returns (ratio a, ratio b, ratio c), the largest err / bound of each (<= 1
    passes).
    addend: a tensor the kernel added in fp32 after the sum (the residual of the gradient hand-over): it is added to both
    references, and one more rounding of the total is allowed
    blocks: rounding_count's block count where ceil(K / 16) is not it (2-D weight gradients)
    epilogue: (scale [C], shift [C], res or None, relu) of the fused relu?(conv * scale + shift + res) on dim 1: applied in
    fp64 to both references; the three bounds scale with |scale|, and 3 2^-24 (|conv scale| + |shift| + |res|) is allowed
    for its three roundings (ReLU does not increase a difference)"""
    got = got.double().to(ex["y"].device)
    y, sr = ex["y"], sref
    if torch.is_tensor(K):
        K = K.double().to(y.device)
    la, lb, lc = bound_a(arith, K, ex, amax_p, amax_q, blocks), bound_b(arith, K, ex), bound_c(arith, K, ex)
    if addend is not None:
        a = addend.double().to(y.device)
        y, sr = y + a, sr + a
        la, lb, lc = la + U * y.abs(), lb + U * y.abs(), lc + U * y.abs()
    if epilogue is not None:
        scale, shift, res, relu = epilogue
        bc = (lambda t: t.double().to(y.device).reshape(1, -1, *([1] * (y.dim() - 2))))
        sc, sh = bc(scale), bc(shift)
        r = res.double().to(y.device) if res is not None else torch.zeros_like(y)
        extra = 3.0 * U * ((y * sc).abs() + sh.abs() + r.abs())
        la, lb, lc = la * sc.abs() + extra, lb * sc.abs() + extra, lc * sc.abs() + extra
        y, sr = y * sc + sh + r, sr * sc + sh + r
        if relu:
            y, sr = y.clamp_min(0.0), sr.clamp_min(0.0)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf"), float("inf")
    eb = (got - sr).abs()
    return _ratio((got - y).abs(), la), _ratio(eb, lb), _ratio(eb, lc)
