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
"""
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


# ---- fp64 operators ---------------------------------------------------------------------------------------------------
def op(kind, p, q):
    """the fp64 operation (torch's convolutions; any device that has them)"""
    p, q = p.double(), q.double()
    if kind == "fwd":
        return F.conv3d(p, q, padding=1)
    if kind == "dgrad":
        return F.conv_transpose3d(p, q, padding=1)
    return torch.nn.grad.conv3d_weight(p, (q.shape[1], p.shape[1], 3, 3, 3), q, padding=1)


def _neighbourhoods(xp, b, d, h, w):
    """[h*w, 27*C] rows of plane d of batch element b of the padded channels-last volume xp (tap-major, channel-minor)"""
    taps = [xp[b, d + kd, kh:kh + h, kw:kw + w, :] for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(taps, dim=2).reshape(h * w, -1)


def op_gemm(kind, p, q):
    """the same values as op(), as unfold + float64 matrix products over depth planes: no fp64 convolution of a vendor
    library is involved (the references of the large shapes are computed this way on the GPU)"""
    p, q = p.double(), q.double()
    if kind == "dgrad":  # conv_transpose3d(dy, w) = conv3d(dy, w with taps flipped and channels swapped)
        kind, q = "fwd", q.transpose(0, 1).flip(2, 3, 4)
    b, c, d, h, w = p.shape
    xp = F.pad(p.permute(0, 2, 3, 4, 1), (0, 0, 1, 1, 1, 1, 1, 1))  # [B, D+2, H+2, W+2, C]
    if kind == "fwd":
        cout = q.shape[0]
        wm = q.permute(2, 3, 4, 1, 0).reshape(27 * c, cout)  # [(tap, ci), co]
        y = torch.empty(b, d, h * w, cout, dtype=torch.float64, device=p.device)
        for bi in range(b):
            for di in range(d):
                y[bi, di] = _neighbourhoods(xp, bi, di, h, w) @ wm
        return y.reshape(b, d, h, w, cout).permute(0, 4, 1, 2, 3)
    cout = q.shape[1]
    g = torch.zeros(cout, 27 * c, dtype=torch.float64, device=p.device)
    for bi in range(b):
        for di in range(d):
            g += q[bi, :, di].reshape(cout, h * w) @ _neighbourhoods(xp, bi, di, h, w)
    return g.reshape(cout, 27, c).permute(0, 2, 1).reshape(cout, c, 3, 3, 3)


def products(kind, p, q):
    """K: products per output"""
    if kind == "wgrad":
        b, _, d, h, w = p.shape
        return b * d * h * w
    return 27 * p.shape[1]


def exact(kind, p, q, gemm=False):
    """fp64 result and the per-output magnitude sums: S = sum |p_k q_k|, Q2 = sum (p_k q_k)^2, sum_q = sum |q_k| and
    sum_p = sum |p_k| (the sums the f16x3 amax term multiplies with the amax of p and of q).  (Padding stays zero in the
    ones.)"""
    f = op_gemm if gemm else op
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


def split_reference(kind, p, q, arith, parts_p=None, parts_q=None, gemm=False):
    """fp64 value of exactly the products the arithmetic forms:
    f16x3  -- hi*hi + hi*lo + lo*hi (lo*lo dropped);
    bf16x6 -- the six products of az_conv3d_wgrad16.hip's chain: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi (mid*lo,
              lo*mid, lo*lo dropped);
    fp32   -- the fp32 operands' exact bilinear form.
    parts_p / parts_q: parts already split (a pre-split tensor decoded from its bits) in place of split_parts()"""
    f = op_gemm if gemm else op
    pp = parts_p if parts_p is not None else split_parts(p, arith)
    qq = parts_q if parts_q is not None else split_parts(q, arith)
    if arith == "f16x3":
        return f(kind, pp[0], qq[0] + qq[1]) + f(kind, pp[1], qq[0])
    if arith == "bf16x6":
        return f(kind, pp[0], qq[0] + qq[1] + qq[2]) + f(kind, pp[1], qq[0] + qq[1]) + f(kind, pp[2], qq[0])
    return f(kind, pp[0], qq[0])


# ---- the two checks -----------------------------------------------------------------------------------------------------
def rounding_count(arith, K):
    """fp32 roundings an output may see in the worst case: every MFMA rounds the accumulator it is chained into (f16x3: 3
    per 16-deep block of v_mfma_*_f16, bf16x6: 6 per 16-deep block, fp32: v_mfma_f32_32x32x2_f32 rounds each of its 2
    products and adds), plus one fp32 add per block for block sums and partial-sum flushes, plus 3 for the epilogue"""
    blocks = math.ceil(K / 16)
    chain = {"f16x3": 3 * blocks, "bf16x6": 6 * blocks, "fp32": 2 * K}[arith]
    return chain + blocks + 3


def bound_a(arith, K, ex, amax_p, amax_q):
    """the worst-case bound (check a).  f16x3: include/azhip.h "CONTRACT of a caller-supplied amax",
        [3 * 2^-22 + n * 2^-24] * S + 2^-38 * (A_p * sum |q| + A_q * sum |p|)
    (3 * 2^-22: the two-part split of both operands and the dropped lo*lo; 2^-38 A: the fp16 subnormal spacing of `lo`),
    with n = rounding_count(): the header's K / 32 + 3 counts one add per 32-deep block sum, the kernels that chain their
    three MFMAs into the running accumulator round up to 3 K / 16 times.
    bf16x6: 5 * 2^-24 * S for the split (hi + mid + lo = x up to 2^-24 |x| per operand, the dropped mid*lo and lo*mid up to
    2^-24 |x y| each) + n * 2^-24 * S.  fp32: n * 2^-24 * S (the operands are exact)."""
    rep = {"f16x3": 12.0, "bf16x6": 5.0, "fp32": 0.0}[arith]
    lim = (rep + rounding_count(arith, K)) * U * ex["S"]
    if arith == "f16x3":
        lim = lim + 2.0 ** -38 * (amax_p * ex["sum_q"] + amax_q * ex["sum_p"])
    return lim


def bound_b(arith, K, ex):
    """the random-walk accumulation bound against split_reference (check b)"""
    return C[arith] * U * (2.0 + math.sqrt(K / 32.0)) * ex["S"]


def bound_c(arith, K, ex):
    """the random-walk bound in the 2-norm of the products (check c)"""
    return C2[arith] * U * (K * ex["Q2"]).sqrt()


def _ratio(err, lim):
    """max err / lim; an output with lim = 0 (every product is zero: padding) must be exactly zero"""
    pos = lim > 0
    if bool((err[~pos] != 0).any()):
        return float("inf")
    return float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0


def check(got, arith, K, ex, sref, amax_p=0.0, amax_q=0.0, addend=None):
    """the three checks for every output; returns (ratio a, ratio b, ratio c), the largest err / bound of each (<= 1
    passes).
    addend: a tensor the kernel added in fp32 after the sum (the residual of the gradient hand-over): it is added to both
    references, and one more rounding of the total is allowed"""
    got = got.double().to(ex["y"].device)
    y, sr = ex["y"], sref
    la, lb, lc = bound_a(arith, K, ex, amax_p, amax_q), bound_b(arith, K, ex), bound_c(arith, K, ex)
    if addend is not None:
        a = addend.double().to(y.device)
        y, sr = y + a, sr + a
        la, lb, lc = la + U * y.abs(), lb + U * y.abs(), lc + U * y.abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf"), float("inf")
    eb = (got - sr).abs()
    return _ratio((got - y).abs(), la), _ratio(eb, lb), _ratio(eb, lc)
