"""fp64 references of the RAFT-Stereo 1-D correlation block (activezero_amd/csrc/az_corr1d.hip), shared by
tests/test_corr_error_model_cpu.py and tests/test_gpu_corr_fp64.py (a helper module, not a conftest).

The three dense contractions are one strided batched bf16x6 GEMM, bgemm_x6_kernel.  Each is a bilinear map y = s op(p, q) of two
operands with K products per output; s is the fp32 value the kernel forms, 1 / sqrtf(C):

    kind   p             q             y                                               K    M    N
    vol    f1 [B,C,H,W1] f2 [B,C,H,W2] vol[b,h,m,n] = s sum_c f1[b,c,h,m] f2[b,c,h,n]  C    W1   W2
    df1    G [B,H,W1,W2] f2            df1[b,c,h,m] = s sum_n G[b,h,m,n] f2[b,c,h,n]   W2   W1   C
    df2    G             f1            df2[b,c,h,n] = s sum_m G[b,h,m,n] f1[b,c,h,m]   W1   W2   C

The checks are (a), (b), (c) of tests/_fp64ref.py with its bf16x6 constants; the kernel forms the six products of az_mfma6_now
(hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi) from zero per 16-deep block and adds the block to the accumulator: exactly
rounding_count's model.  The `* scale` of the epilogue is one more rounding of the total, granted through a zero `addend`.

The pyramid lookup (lookup_fwd_kernel / lookup_bwd_kernel) is referenced in two steps: the sampling coordinate in numpy float32,
step by step as lookup_x computes it (no fast-math, fp contract(off): bit for bit), then the linear interpolation in fp64.
"""
import numpy as np
import torch

from tests import _fp64ref as R

KINDS = ("vol", "df1", "df2")
ARITH = "bf16x6"
_EQ = {"vol": "bchm,bchn->bhmn", "df1": "bhmn,bchn->bchm", "df2": "bhmn,bchm->bchn"}
U = R.U


def scale(c):
    """the kernel's 1.0f / sqrtf((float)C), as a Python float holding the fp32 value"""
    return float(np.float32(1.0) / np.sqrt(np.float32(c)))


def op(kind, p, q):
    """the unscaled fp64 contraction"""
    return torch.einsum(_EQ[kind], p.double(), q.double())


def dims(kind, shape):
    """(M, N, K) of the GEMM a contraction is, for shape = (B, C, H, W1, W2)"""
    _, c, _, w1, w2 = shape
    return {"vol": (w1, w2, c), "df1": (w1, c, w2), "df2": (w2, c, w1)}[kind]


def operands(kind, f1, f2, g):
    return {"vol": (f1, f2), "df1": (g, f2), "df2": (g, f1)}[kind]


def exact(kind, p, q, c):
    """fp64 result y and the per-output sums S = sum |p_k q_k| (both times s) and Q2 = sum (p_k q_k)^2 (times s^2)"""
    s = scale(c)
    p, q = p.double(), q.double()
    return {"y": op(kind, p, q) * s, "S": op(kind, p.abs(), q.abs()) * s, "Q2": op(kind, p * p, q * q) * (s * s)}


def split_reference(kind, p, q, c):
    """s times the fp64 value of exactly the six products az_mfma6_now forms (mid*lo, lo*mid, lo*lo dropped)"""
    pp, qq = R.split_parts(p, ARITH), R.split_parts(q, ARITH)
    y = op(kind, pp[0], qq[0] + qq[1] + qq[2]) + op(kind, pp[1], qq[0] + qq[1]) + op(kind, pp[2], qq[0])
    return y * scale(c)


def check(got, kind, shape, ex, sref):
    """(ratio a, ratio b, ratio c) of tests/_fp64ref.py's checks, constants unchanged"""
    return R.check(got, ARITH, dims(kind, shape)[2], ex, sref, addend=torch.zeros_like(ex["y"]))


# ---- the lookup -----------------------------------------------------------------------------------------------------------------
def lookup_ix(coord, w_level, radius, level):
    """lookup_x of az_corr1d.hip in numpy float32, one rounding per operation: coord [...] (channel 0 of the coordinates) ->
    the sampling position ix [..., 2 radius + 1] in pixels of the level"""
    f = np.float32
    c = np.asarray(coord, dtype=np.float32)[..., None]
    inv = f(1.0) / f(1 << level)
    dx = (np.arange(2 * radius + 1) - radius).astype(np.float32)
    wm1 = f(w_level - 1)
    with np.errstate(all="ignore"):
        x = c * inv + dx
        gx = f(2.0) * x / wm1 - f(1.0)
        ix = ((gx + f(1.0)) / f(2.0)) * wm1
    assert ix.dtype == np.float32
    return ix


def lookup_taps(ix, w_level):
    """(x0, w, in0, in1): the left tap's column (clamped as the kernel clamps it), the fp32 weight of the right tap as fp64,
    and which of the two taps lie inside the row"""
    fx = np.floor(ix)
    x0 = np.clip(fx, np.float32(-2.0), np.float32(w_level + 1.0)).astype(np.int64)
    w = (ix - fx).astype(np.float64)  # (exact in fp32: ix and floor(ix) are less than one apart or ix is an integer)
    return x0, w, (x0 >= 0) & (x0 < w_level), (x0 + 1 >= 0) & (x0 + 1 < w_level)


def lookup_fwd(pyr, coord, radius, level):
    """pyr [B,H,W1,Wl], coord [B,H,W1] -> (ref [B,taps,H,W1] fp64, mag = |a| (1 - w) + |b| w, integer = ix is a column of the row)"""
    pyr = np.asarray(pyr, dtype=np.float64)
    wl = pyr.shape[-1]
    ix = lookup_ix(coord, wl, radius, level)
    x0, w, in0, in1 = lookup_taps(ix, wl)
    a = np.where(in0, np.take_along_axis(pyr, np.clip(x0, 0, wl - 1), -1), 0.0)
    b = np.where(in1, np.take_along_axis(pyr, np.clip(x0 + 1, 0, wl - 1), -1), 0.0)
    ref = a * (1.0 - w) + b * w
    mag = np.abs(a) * (1.0 - w) + np.abs(b) * w
    integer = (w == 0.0) & in0
    to = (lambda t: np.ascontiguousarray(np.moveaxis(t, -1, 1)))
    return to(ref), to(mag), to(integer)


def lookup_bwd(gout, coord, w_level, radius, level):
    """gout [B,taps,H,W1] (the taps' channels only), coord [B,H,W1] -> (the fp64 scatter [B,H,W1,Wl] of the same weights,
    sum |contribution| per element, number of contributions per element)"""
    g = np.moveaxis(np.asarray(gout, dtype=np.float64), 1, -1)  # [B,H,W1,taps]
    ix = lookup_ix(coord, w_level, radius, level)
    x0, w, in0, in1 = lookup_taps(ix, w_level)
    ref = np.zeros(g.shape[:-1] + (w_level,))
    mag, cnt = np.zeros_like(ref), np.zeros_like(ref)
    for k in range(g.shape[-1]):  # (one tap at a time: the two columns of a tap differ, so a plain fancy-index add is exact)
        for col, wt, inside in ((x0[..., k], 1.0 - w[..., k], in0[..., k]), (x0[..., k] + 1, w[..., k], in1[..., k])):
            idx = np.nonzero(inside)
            c = g[..., k][idx] * wt[idx]
            at = idx + (col[idx],)
            ref[at] += c
            mag[at] += np.abs(c)
            cnt[at] += 1.0
    return ref, mag, cnt
