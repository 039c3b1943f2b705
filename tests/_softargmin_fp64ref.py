"""fp64 reference of the soft-argmin head -- K6 az_softargmin.hip: trilinear x4 upsample, softmax over D = 4d, expectation, and
its vector-Jacobian product -- shared by tests/test_softargmin_error_model_cpu.py and tests/test_gpu_softargmin_fp64.py (a helper
module, not a conftest).

The reference is closed form: align_corners=False at an exact x4 scale makes destination 4q + r read cells (q - 1, q) with upper
weight .625 / .875 for r = 0, 1 and (q, q + 1) with upper weight .125 / .375 for r = 2, 3, indices clamped; axis_matrix(n) is
that map as a [4n, n] matrix, and the head is three such matrices applied to the logits, a softmax and a dot product with D, all
in fp64.  The gradient is d out / d u_D = p_D (D - out) folded back through the transposed matrices.

The bounds COUNT the kernel's fp32 roundings.  U = 2^-24 is the unit roundoff of one operation; a multiply-add contracted into
an FMA only removes a rounding, so the counts hold with and without contraction.  The hardware exp2 is taken at the 1 ulp the
kernel's comments state: relative 2^-23 = 2 U, plus TINY = 2^-126 absolute (it flushes denormals).  Relative errors are composed
as products, not sums, because on the `spike` set they reach 1e-3.

Per pixel (um = the trilinear form of |logits|, vm its bilinear part per plane, x_D = u_D - M):
  plane value  v_k = wy0 (wx0 a + wx1 b) + wy1 (...): the weights and 1 - w are exact; a product (1) and the add (1) per lerp:
               |err| <= K_PLANE U vm,  K_PLANE = 4
  shift        M = the largest of v_0, v_(d-1) and .875 v_k + .125 v_(k+1), .125 v_k + .875 v_(k+1) (product, add: 2 more):
               |M - M_ref| <= K_SHIFT U max_D um,  K_SHIFT = 6       (|max x_i - max y_i| <= max |x_i - y_i|)
  forward      argument of exp2 = lerp_D((v_k - M) log2 e): the plane (4 U um), the subtraction (1), the product with the
               rounded constant (2), the lerp (2), the last three relative to am_D = lerp_D |v_k - M| -- NOT to |x_D|: a plane
               may tower over M (only upsampled levels are below it) and the lerp then cancels:
               eta_D = 4 U um_D + 5 U am_D,   e_D = exp(x_D) (1 + rel_D),  rel_D = expm1(eta_D) (1 + 2 U) + 2 U
  s            a chain of CH adds of positive terms (d + 3 in the four-accumulator templates, 4 d in the generic loop):
               |s - sum exp(u_D - M_got)| <= (sum p_D rel_D + CH U (1 + max rel)) s     against the kernel's OWN shift M_got
  out = t / s  t and s share every e_D, so the common part of rel_D cancels: N - out S = sum e_D rel_D (D - out) + the adds;
               |err| <= (sum p_D rel_D |D - out| + (1 + max rel) (2 CH + 3) U out) / (1 - eps_s) + U out
  backward     gu_D = (g / s) exp2((u_D - M) log2 e) (D - pred): u_D = lerp_D v_k (4 + 2 roundings relative to um_D), u_D - M
               (1) and the product with the constant (2) relative to |x_D|:  eta'_D = 6 U um_D + 3 U |x_D|; g / s carries the
               error of the saved (or recomputed) s and the division (1); D - pred the forward bound of pred and the
               subtraction; the two products and the sum of the doubled end terms: K_GU = 4
  fold         every (pixel, D) contribution then passes through: the D-lerp product and <= 9 adds into the plane's
               accumulator (K_FOLD = 10); the x-share product, two quad adds and the two +-4-lane adds (K_X = 5); the row-share
               product (K_Y = 1); the sum of the four waves' images (K_FLUSH = 4); and the global float atomics: a cell is inside
               the 3 x 18 window of at most 3 tile rows or aliased halo rows times 3 tile columns or aliased halo columns
               (K_ATOM = 9), in any order.  Each is granted U times the SUM OF ABSOLUTE contributions to the cell.

Every check is a ratio err / bound <= 1.0 over every element (ratio()); a non-finite output has ratio inf.  No constant here is
fitted to GPU output.

Largest ratio err / bound measured on an MI355X over every case of tests/test_gpu_softargmin_fp64.py
(test_zz_largest_ratios prints it per input set), d == 48 / d == 16 / generic depth:
    check                                   plain                 wide                  flat     spike
    forward                                 0.06 / 0.09 / 0.12    0.09 / 0.11 / 0.33    0 exact  0 exact
    saved M                                 0.35 / 0.32 / 0.45    0.41 / 0.27 / 0.43    0 exact  0 exact
    saved s (against the kernel's own M)    0.14 / 0.18 / 0.26    0.12 / 0.14 / 0.38    0 exact  <= 0.01
    backward, saved statistics              0.03 / 0.05 / 0.05    0.03 / 0.04 / 0.03    <= 0.02  <= 0.001
    backward, recompute                     0.03 / 0.05 / 0.05    0.03 / 0.04 / 0.03    <= 0.02  <= 0.001
    backward through ops.softargmin         -                     0.03 / 0.04 / 0.03
No ratio exceeds 0.5.  The bounds are worst cases: with logits of magnitude 10 to 400 the counted error of the exponent's
argument (about 100 U at |logit| = 15) outweighs every other term, and it is granted with the same sign in every term.  A pixel's
output sums 4 d such terms and a gradient cell those of up to 8 x 8 pixels, so the measured ratios fall as the sums grow --
as the ratios of the reprojection kernels fall with their window.  What the checks still reject is listed, mutant by mutant,
in tests/test_softargmin_error_model_cpu.py.  Before its dead lanes were given a shift of their own, the backward kernel
failed every `wide` case of the saved-statistics path at the seven shapes with 4 w % 64 != 0 -- a NaN in column w - 1 of
grad_logits and nowhere else -- and passed the recompute path and every other set.
"""
import functools

import numpy as np

from tests._reproj_fp64ref import ratio  # noqa: F401  (the one definition of a check)

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16
TINY = 2.0 ** -126
EXP_REL = 2.0 * U          # 1 ulp of the hardware exp2
K_PLANE, K_SHIFT, K_GU = 4.0, 6.0, 4.0
K_FOLD, K_X, K_Y, K_FLUSH, K_ATOM = 10.0, 5.0, 1.0, 4.0, 9.0
K_SUM = K_FOLD + K_X + K_Y + K_FLUSH + K_ATOM
PHASE_W1 = (0.625, 0.875, 0.125, 0.375)
MAX_D = 82                 # the largest depth sa_check admits: (54 + 144) d floats of LDS <= 64 KiB


def axis_matrix(n):
    """[4n, n]: PyTorch's linear x4 upsampling, align_corners=False, as a matrix"""
    A = np.zeros((4 * n, n))
    dst = np.arange(4 * n)
    q, r = dst >> 2, dst & 3
    lo = np.where(r < 2, q - 1, q)
    w1 = np.array(PHASE_W1)[r]
    np.add.at(A, (dst, np.clip(lo, 0, n - 1)), 1.0 - w1)
    np.add.at(A, (dst, np.clip(lo + 1, 0, n - 1)), w1)
    return A


def chain(d):
    """adds on the longest chain of the forward sums: four accumulators and three joining adds, or the generic loop"""
    return d + 3 if d in (48, 16) else 4 * d


def route(d):
    return "d == 48 registers" if d == 48 else "d == 16 registers" if d == 16 else "generic depth"


def _comp(*rels):
    out = 1.0
    for r in rels:
        out = out * (1.0 + r)
    return out - 1.0


def head(logits, gout=None):
    """logits [B,d,h,w] (, gout [B,4h,4w]) -> dict of fp64 arrays:
        out, M, s [B,H,W]; p, u [B,D,H,W]; M_bound, out_bound, eps_s; and with gout: grad, grad_bound [B,d,h,w]"""
    x = np.asarray(logits, dtype=np.float64)
    B, d, h, w = x.shape
    Ad, Ah, Aw = axis_matrix(d), axis_matrix(h), axis_matrix(w)
    D = np.arange(4 * d, dtype=np.float64)[None, :, None, None]
    plane = lambda t: np.einsum("Yy,byX->bYX", Ah, np.einsum("Xx,byx->byX", Aw, t.reshape(B * d, h, w))).reshape(B, d, 4 * h, 4 * w)
    depth = lambda t: np.einsum("Dk,bkYX->bDYX", Ad, t)
    v = plane(x)
    u = depth(v)
    um = depth(plane(np.abs(x)))
    M = u.max(1)
    e = np.exp(u - M[:, None])
    s = e.sum(1)
    p = e / s[:, None]
    out = (p * D).sum(1)
    # ---- forward bounds
    M_bound = K_SHIFT * U * SECOND * um.max(1)
    am = depth(np.abs(v - M[:, None])) + M_bound[:, None]
    ax = np.abs(u - M[:, None]) + M_bound[:, None]
    rel_f = np.expm1(SECOND * U * (K_PLANE * um + 5.0 * am)) * (1.0 + EXP_REL) + EXP_REL
    relmax = rel_f.max(1)
    CH = float(chain(d))
    eps_s = (p * rel_f).sum(1) + CH * U * (1.0 + relmax) + 4 * d * TINY
    dev = np.abs(D - out[:, None])
    num = (p * rel_f * dev).sum(1) + (1.0 + relmax) * (2 * CH + 3) * U * out + 16.0 * d * d * TINY
    out_bound = SECOND * (num / (1.0 - eps_s) + U * (out + num))
    res = dict(out=out, M=M, s=s, p=p, u=u, M_bound=M_bound, out_bound=out_bound, eps_s=eps_s * SECOND)
    if gout is None:
        return res
    # ---- the vector-Jacobian product and its bound
    g = np.asarray(gout, dtype=np.float64).reshape(B, 1, 4 * h, 4 * w)
    gu = g * p * (D - out[:, None])
    rel_b = np.expm1(SECOND * U * (6.0 * um + 3.0 * ax)) * (1.0 + EXP_REL) + EXP_REL
    rel_g = (eps_s / (1.0 - eps_s))[:, None] + U
    R = _comp(rel_g, rel_b, K_GU * U)
    err = np.abs(gu) * R + np.abs(g) * p * out_bound[:, None] * (1.0 + R) + 2.0 * np.abs(g) * TINY * (dev + out_bound[:, None])
    back = lambda t: np.einsum("Xx,bkyX->bkyx", Aw, np.einsum("Yy,bkYX->bkyX", Ah, np.einsum("Dk,bDYX->bkYX", Ad, t)))
    res["grad"] = back(gu)
    res["grad_bound"] = SECOND * back(err + K_SUM * U * (np.abs(gu) + err)) + TINY
    return res


def s_at(ref, M_got):
    """sum_D exp(u_D - M_got): the normaliser that belongs to the kernel's own shift"""
    return np.exp(ref["u"] - np.asarray(M_got, dtype=np.float64)[:, None]).sum(1)


def check_stats(ref, stats):
    """stats [B,H,W,2] as az_softargmin_fwd saves them -> (ratio of M, ratio of s)"""
    stats = np.asarray(stats)
    M_got, s_got = stats[..., 0], stats[..., 1]
    rM = ratio(M_got, ref["M"], ref["M_bound"])
    if not np.isfinite(rM):
        return rM, np.inf
    want = s_at(ref, M_got)
    return rM, ratio(s_got, want, ref["eps_s"] * want * (1.0 + U))


# ---- the cases, shared by the CPU model and the GPU sweep -----------------------------------------------------------------------
SHAPES = [(3, 1, 3, 1), (1, 2, 1, 3), (1, 5, 4, 15), (3, 7, 3, 16), (3, 16, 1, 17), (1, 48, 3, 21), (1, 3, 2, 33), (1, 82, 1, 3)]
SETS = ("plain", "flat", "spike", "wide")
FLAT = 0.75        # a short mantissa: every lerp of it and every partial sum of exp2(0) is exact
SPIKE = 4000.0
RAMP = 125.0
WANT = {"d == 48", "d == 16", "d == 1", "d == 2", "odd generic d", "d == 82", "w == 1", "w == 3", "4w % 64 == 0",
        "one live quad in the last tile", "exactly one dead quad", "multi-tile width with dead lanes", "h == 1", "h >= 3",
        "b == 1", "b == 3", "dead lanes in a later batch"}


def dead_lanes(w):
    return (4 * w) % 64 != 0


def features(shapes=None):
    """what the shape list reaches"""
    feats = set()
    for b, d, h, w in (SHAPES if shapes is None else shapes):
        assert d <= MAX_D
        feats |= {n for n, on in (
            ("d == 48", d == 48), ("d == 16", d == 16), ("d == 1", d == 1), ("d == 2", d == 2), ("d == 82", d == MAX_D),
            ("odd generic d", d % 2 == 1 and d > 1 and d not in (48, 16)), ("w == 1", w == 1), ("w == 3", w == 3),
            ("4w % 64 == 0", not dead_lanes(w)), ("one live quad in the last tile", w % 16 == 1 and w > 16),
            ("exactly one dead quad", w % 16 == 15), ("multi-tile width with dead lanes", w > 16 and w % 16 > 1),
            ("h == 1", h == 1), ("h >= 3", h >= 3), ("b == 1", b == 1), ("b == 3", b == 3),
            ("dead lanes in a later batch", b >= 2 and dead_lanes(w))) if on}
    return feats


def spike_plane(d):
    return d // 2


def _seed(shape, which):
    return 6100 + 17 * SETS.index(which) + sum(p * s for p, s in zip((7, 3, 5, 11), shape))


@functools.lru_cache(maxsize=None)
def inputs(shape, which):
    """(logits [b,d,h,w], gout [b,4h,4w]) float32, read-only"""
    b, d, h, w = shape
    rng = np.random.default_rng(_seed(shape, which))
    if which == "plain":
        lg = 5.0 * rng.standard_normal(shape)
    elif which == "flat":
        lg = np.full(shape, FLAT)
    elif which == "spike":
        lg = np.zeros(shape)
        lg[:, spike_plane(d)] = SPIKE
    else:
        bb, yy, xx = np.arange(b)[:, None, None, None], np.arange(h)[None, None, :, None], np.arange(w)[None, None, None, :]
        lg = 1.5 * rng.standard_normal(shape) + RAMP * (bb + yy / max(h - 1, 1) + xx / max(w - 1, 1))
    lg = lg.astype(np.float32)
    gout = rng.standard_normal((b, 4 * h, 4 * w)).astype(np.float32)
    lg.setflags(write=False)
    gout.setflags(write=False)
    return lg, gout


@functools.lru_cache(maxsize=None)
def reference(shape, which):
    lg, gout = inputs(shape, which)
    ref = head(lg, gout)
    if which == "wide" and dead_lanes(shape[3]):
        # what arms the dead lanes of the backward pass: in some batch every logit of the right-edge column lies more than
        # 100 above the shift of pixel (0, 0, 0) of batch 0, so exp(v - M) of a lane that reads that shift overflows
        excess = lg[:, :, :, -1].astype(np.float64).min(axis=(1, 2)).max() - ref["M"][0, 0, 0]
        assert excess > 100.0, (shape, excess)
    for t in ref.values():
        if isinstance(t, np.ndarray):
            t.setflags(write=False)
    return ref


# ---- the checks, one place for the CPU model and the GPU sweep ------------------------------------------------------------------
def check_forward(shape, which, out, stats=None):
    """out [b,4h,4w] (, stats [b,4h,4w,2]) -> dict of ratios; the exact properties (d == 1: 1.5; flat: (D - 1) / 2) are part of
    `forward`: a violation is ratio inf"""
    b, d, h, w = shape
    ref = reference(shape, which)
    out = np.asarray(out).reshape(b, 4 * h, 4 * w)
    r = {"forward": ratio(out, ref["out"], ref["out_bound"])}
    if d == 1 and not np.all(out == 1.5):
        r["forward"] = np.inf
    if which == "flat" and not np.all(out == (4 * d - 1) / 2.0):
        r["forward"] = np.inf
    if stats is not None:
        r["stats M"], r["stats s"] = check_stats(ref, np.asarray(stats).reshape(b, 4 * h, 4 * w, 2))
    return r


def check_backward(shape, which, grad):
    ref = reference(shape, which)
    return ratio(np.asarray(grad).reshape(shape), ref["grad"], ref["grad_bound"])
