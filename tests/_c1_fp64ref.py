"""fp64 references, launch plan and element-wise error bounds of the 32 -> 1 classifier convolutions of az_conv3d_c1.hip
(az_conv3d_c1_fwd / _dgrad / _wgrad), shared by tests/test_c1_error_model_cpu.py and tests/test_gpu_c1_fp64.py (a helper
module, not a conftest).

The three operations are the 3-D stride-1 family of tests/_fp64ref.py (geom = None) with cout = 1 on the fp32 arithmetic:
    kind    p                q    y                                K = products per output
    fwd     x [B,32,D,H,W]   w    conv3d(x, w)      [B,1,D,H,W]    27 * 32 = 864
    dgrad   dy [B,1,D,H,W]   w    conv_transpose3d  [B,32,D,H,W]   27
    wgrad   x                dy   dW                [1,32,3,3,3]   B D H W
R.exact gives y, S = sum |p_k q_k| and Q2 = sum (p_k q_k)^2; the operands are exact in fp32, so the split reference of
check (b) is y itself.  With in_scale / in_shift the operand x is relu(raw * scale + shift), taken in fp64 (operand()).

Check (a), sound: COUNTED from the kernels' code.  U = 2^-24 is the unit roundoff of one fp32 operation, and a sum whose every
term passes through at most n roundings is off by at most gamma_n S, gamma_n = n U / (1 - n U), whatever the order of the
additions (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  An FMA rounds once.
  forward   a lane owns a channel pair of 8 voxels: per channel one accumulator chained through the 27 FMAs of the three
            staged planes (a_next on plane od - 1 with the kd = 0 taps, then as a_cur on plane od, then as a_prev on plane
            od + 1: 9 each, order kd, kh, kw); one add joins the two channels of the pair; four DPP adds (quad_perm xor 1,
            xor 2, row_half_mirror, row_mirror) join the 16 pairs:                                       n = 27 + 1 + 4 = 32
            `+ addend` is one more rounding, of the total: U |y + addend|.
  dgrad     one accumulator per channel and voxel, 27 FMAs (kd, kh, kw), nothing else:                 n = 27
  wgrad     one accumulator per (lane, channel, tap): 16 FMAs per item (4 passes x 4 voxels) x items = ceil(ntiles / grid) items
            of the workgroup's strided list; three __shfl_xor adds over the 8 lanes of a wave that share a channel quad; an LDS
            atomic per wave (4); a global atomic per workgroup (grid), the last two in any order:
                                                                                   n = 16 items + 3 + 4 + grid   (wgrad_roundings)
The fused operand is rounded once by fmaf before the ReLU, which is 1-Lipschitz: each product moves by at most
U |raw scale + shift| |q|, so U op(|raw scale + shift|, |q|) -- the PRE-ReLU magnitude -- is added to all three bounds
(operand_grant).  SECOND = 1 + 2^-16 covers the products of two roundings that these first-order terms drop.  No constant of
check (a) is fitted to GPU output.

Checks (b) and (c) are R.bound_b / R.bound_c of the fp32 arithmetic with the project's constants C["fp32"] = 2.0 and
C2["fp32"] = 8.0.

Every check is a ratio err / bound <= 1 over every element through R._ratio (an exact zero where the bound is zero); a
non-finite output gives inf.

Largest ratio err / bound measured on an MI355X over every case of tests/test_gpu_c1_fp64.py (test_zz_largest_ratios prints it),
per kernel and launch regime; the constants of (b) and (c) are the shared ones, unchanged:
    kernel, regime                                               (a)      (b)      (c)
    fwd    dseg = 1                                              0.017    0.037    0.038   ((3, 5, 11, 65) + addend)
    fwd    dseg >= 2, whole segments                             0.017    0.038    0.051   ((1, 48, 16, 240) + addend)
    fwd    dseg >= 2, ragged last segment                        0.017    0.038    0.052   ((1, 20, 64, 160) + addend)
    fwd    dseg = D, one segment                                 0.018    0.039    0.044   ((768, 3, 8, 16) + addend)
    fwd    fused affine, dseg = 1                                0.021    0.043    0.035   ((1, 4, 8, 33))
    fwd    fused affine, dseg >= 2 (ragged or not), dseg = D     0.027    0.056    0.040   ((1, 2050, 3, 5) and (768, 3, 8, 16) + addend)
    dgrad  (one regime: a workgroup per plane tile)              0.177    0.817    0.448   ((1, 20, 64, 160))
    wgrad  one item per workgroup                                0.038    0.207    0.113   ((1, 1, 1, 1): K = 1)
    wgrad  walking workgroups (ntiles > 2048)                    0.0003   0.010    0.045   ((1, 2050, 3, 5): 2087 roundings counted)
    wgrad  fused affine, one item | walking                      0.014    0.029    0.023 | 0.0005  0.014  0.050
    wgrad  operands embedded in 1e4, one item | walking          0.016    0.034    0.033 | 0.0005  0.016  0.060
    through conv3d.conv_logits: fwd | x.grad | weight.grad       0.023    0.047    0.033 | 0.164  0.759  0.398 | 0.0003  0.001  0.008
Two runs of the weight gradient differed by at most 0.001 of the order bound 2 gamma_(4 + grid) S and were bit-identical at none
of the four shapes tried; forward and input gradient are bit-identical.  The input gradient stands closest to its bounds: K = 27
leaves (b) only 2 (2 + sqrt(27 / 32)) U S = 5.8 U S for a chain of 27 roundings, and its ratio is the maximum over up to 9.4
million outputs -- it rises with their number, from 0.15 at 32 outputs to 0.82 at 6.5 million, as the maximum of a random
walk's end point does, and the fp32 emulation of tests/test_c1_error_model_cpu.py stands at the same values (0.48 at
(2, 5, 7, 13), where the kernel gives 0.49).  The walking weight gradient, the long single-lane chain, is far inside all three.
"""
import functools

import torch

from tests import _fp64ref as R

U = R.U
SECOND = 1.0 + 2.0 ** -16
ARITH = "fp32"
N_FWD, N_DGRAD = 32, 27
FWD_SLOTS, WGRAD_MAX_GRID = 768, 2048


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the launch plan, restated (the library's answer, az_conv3d_c1_plan, is compared with it) ---------------------------------
def fwd_dseg(patches, D):
    """az_launch_math.h az_c1_fwd_dseg"""
    best, best_cost = 1, None
    for nseg in range(1, D + 1):
        dseg = -(-D // nseg)
        cost = -(-(patches * -(-D // dseg)) // FWD_SLOTS) * (dseg + 2)
        if best_cost is None or cost < best_cost:
            best, best_cost = dseg, cost
    return best


@functools.lru_cache(maxsize=None)
def plan(shape):
    """(forward dseg, forward workgroups, weight-gradient ntiles, weight-gradient grid) of a shape (B, D, H, W)"""
    b, d, h, w = shape
    patches = b * -(-h // 8) * -(-w // 16)
    dseg = fwd_dseg(patches, d)
    ntiles = b * d * -(-h // 8) * -(-w // 32)
    return dseg, patches * -(-d // dseg), ntiles, min(ntiles, WGRAD_MAX_GRID)


def segments(shape):
    """(number of forward depth segments, planes of the last one)"""
    dseg, d = plan(shape)[0], shape[1]
    nseg = -(-d // dseg)
    return nseg, d - (nseg - 1) * dseg


def wgrad_roundings(shape):
    _, _, ntiles, grid = plan(shape)
    return 16 * -(-ntiles // grid) + 3 + 4 + grid


def wgrad_order_roundings(shape):
    """the roundings of a weight gradient whose ORDER is not fixed (the LDS and the global atomics): two runs differ by at most
    2 gamma of this count times S"""
    return 4 + plan(shape)[3]


def roundings(kind, shape):
    return {"fwd": N_FWD, "dgrad": N_DGRAD}[kind] if kind != "wgrad" else wgrad_roundings(shape)


# ---- operands in the reference's layout ------------------------------------------------------------------------------------------
def operand(raw, scale=None, shift=None):
    """the fp64 activation operand [B,32,D,H,W] and its pre-ReLU magnitude (None without the affine)"""
    raw = raw.double()
    if scale is None:
        return raw, None
    pre = raw * scale.double().to(raw.device).view(1, -1, 1, 1, 1) + shift.double().to(raw.device).view(1, -1, 1, 1, 1)
    return pre.clamp_min(0.0), pre.abs()


def operand_grant(kind, pre_abs, q, gemm=False):
    """U op(|raw scale + shift|, |q|): the one rounding of the fused operand"""
    f = R.op_gemm if gemm else R.op
    return U * f(kind, pre_abs, q.double().abs())


def check(got, kind, shape, ex, addend=None, grant=None, n=None):
    """(ratio a, ratio b, ratio c) of an output in the reference's layout; ex = R.exact(kind, p, q); addend: added in fp32
    after the sum; grant: operand_grant of a fused operand; n: the rounding count where roundings(kind, shape) is not it"""
    y = ex["y"]
    got = got.double().to(y.device)
    K = 864 if kind == "fwd" else 27 if kind == "dgrad" else shape[0] * shape[1] * shape[2] * shape[3]
    n = roundings(kind, shape) if n is None else n
    la, lb, lc = SECOND * gamma(n) * ex["S"], R.bound_b(ARITH, K, ex), R.bound_c(ARITH, K, ex)
    if grant is not None:
        g = SECOND * grant.to(y.device)
        la, lb, lc = la + g, lb + g, lc + g
    if addend is not None:
        y = y + addend.double().to(y.device)
        la, lb, lc = la + SECOND * U * (y.abs() + la), lb + U * y.abs(), lc + U * y.abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf"), float("inf")
    err = (got - y).abs()
    return R._ratio(err, la), R._ratio(err, lb), R._ratio(err, lc)


def order_ratio(a, b, shape, ex):
    """two runs of the weight gradient: |a - b| over the smaller of 2 gamma_(4 + grid) S (sound: only the atomics' order differs)
    and the bound of check (a) itself"""
    lim = SECOND * min(2.0 * gamma(wgrad_order_roundings(shape)), gamma(wgrad_roundings(shape))) * ex["S"]
    if not (bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())):
        return float("inf")
    return R._ratio((a.double() - b.double()).abs().to(lim.device), lim)


def affine_pair(seed, positive_quad=0):
    """per-channel (scale, shift) of the fused BatchNorm + ReLU for operands in [-1, 1]: scales of both signs and of magnitude
    0.5 .. 1.5; shifts of both signs -- channels 8 .. 11 at <= -2 (|raw scale| <= 1.5: clamped everywhere), channels 12 .. 15 at
    >= 2 (never clamped), the channel quad `positive_quad` at +0.75 (an affine applied to padding would put relu(shift) there)"""
    from tests._weights import seeded
    scale = seeded((32,), seed, 0.5, 1.5) * torch.where(torch.arange(32) % 3 == 0, -1.0, 1.0)
    shift = seeded((32,), seed + 1, -0.5, 0.5)
    shift[8:12] = -2.0 - shift[8:12].abs()
    shift[12:16] = 2.0 + shift[12:16].abs()
    shift[4 * positive_quad:4 * positive_quad + 4] = 0.75
    return scale, shift
