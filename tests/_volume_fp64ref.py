"""fp64 references and rounding-count bounds of the three kernel files between PSMNet's feature extractor and its 3-D aggregation
-- K3 az_cost_volume.hip (both layouts, forward and backward), K3+K4 factored az_costconv.hip (assemble and merge, forward and
backward) and az_spp.hip (forward and backward) -- shared by tests/test_volume_error_model_cpu.py and
tests/test_gpu_volume_fp64.py (a helper module, not a conftest).  numpy only.

U = 2^-24, gamma(n) = n U / (1 - n U).  Every check is ratio() = |got - ref64| / bound <= 1.0 over every element (a zero bound
demands got == ref exactly; a non-finite output is inf), or same_bits() on int32 views where the operation is a copy or one
correctly rounded add.  The bounds COUNT the kernel's own fp32 roundings from its source; a product contracted into an FMA only
removes a rounding.  No bound is scaled to a measurement.

  K3 forward        a pure copy: bit equality with the header's definition, the region x < i the bit pattern +0.0.
  K3 backward       grad_l[x] sums n = min(d-1, x) + 1 terms, grad_r[x] n = min(d-1, w-1-x) + 1, in-order fp32 adds from 0.f
                    (0 + t is exact): gamma(n-1) sum|terms|; n = 1 is bit-equal.
  assemble forward  one correctly rounded add f + g: bit-equal to numpy's float32 add; +0.0 where x - d < -2.  asm_map(D, W)
                    is the index rule of include/azhip.h per (d, x): which F_bulk / F_edge block and which G block is read.
  assemble backward the transpose of asm_map by np.add.at in fp64.  dF_edge: single copies and zeros, bit-equal.  dF_bulk, dG:
                    gamma(n-1) sum|terms|, n = the number of planes the slot receives.
  merge             the header's two einsums in fp64 with any float masks; gamma(n) sum|products|: forward n = 3 (K_L), 9 (K_R);
                    backward n = ncls 5 (K_L), ncls 2 5 (K_R).
  SPP forward       positions by the kernel's and ATen's fp32 recipe (spp_positions), the four-tap expression in fp64 from those
                    fp32 weights; gamma(4) (|h0| (|w0 x00| + |w1 x01|) + |h1| (|w0 x10| + |w1 x11|)).  (hipcc contracts the
                    expression into FMAs: at most 4 roundings lie on any path from a tap to the result.  An un-contracted fp32
                    evaluation has 5 on its longest path; the CPU emulation here is un-contracted and stays below 1.)
  SPP backward      np.add.at of the forward's fp32 weights in fp64, separable (wy (x) wx); gamma(N) sum |wy| |wx| |g| with
                    N = spp_roundings(): per pass  ceil(window / npl) + log2(npl) + 1,  the two passes added:
                      ceil(window / npl)  the longest per-lane FMA chain (one rounding per FMA, the first onto 0.f included);
                                          window = hi - lo + 1 of the kernel's own spp_window (restated here in fp32), the
                                          longest over the source indices of that axis; npl = 256 / (C / 4) lanes walk it
                      log2(npl)           the adds of the LDS tree
                      + 1                 spp_weight's own add l0 + l1 where both taps land on the last source index: a count
                                          of the chain and the tree alone leaves it out; it is one more rounding of the
                                          weight against the reference's exact l0 + l1, so it belongs to the count
                    The second pass reads the first's rounded result, so the relative errors compose: the counts add.

Input sets (seeded, read-only, the same arrays on the CPU and the GPU):
  plain     normal values
  exact     integer-valued floats in [-64, 64]: every sum is exact in fp32, the kernel must equal the fp64 reference bit for
            bit -- the index check no tolerance can blur (the SPP weights are not integers: SPP has no such set; its bit-exact
            cases are the same-size and the 1 x 1-source copies)
  bits      K3 forward only: -0.0, +-inf, a NaN with a payload, FLT_MAX among ordinary values (no subnormals)
  embedded  plain operands whose unused neighbours hold +-1e4: the other channels of a wider SPP row; for the merge kernels the
            other half of the [32][64] weight (embedded_l: K_L's operand is plain and K_R's half is +-1e4; embedded_r the
            reverse) and of the incoming gradients

Largest ratio err / bound measured on an MI355X over every case of tests/test_gpu_volume_fp64.py (test_zz_largest_ratios
prints them):
    check                          plain            exact     embedded (_l / _r)
    K3 backward, NCDHW / NDHWC     1.000 / 1.000    0 exact   -          (through ops.cost_volume*: 0.91 / 1.00)
    assemble backward dF_bulk, dG  1.000, 1.000     0 exact   -          (through costconv._Assemble: 1.00)
    merge forward  K_L / K_R       0.85 / 0.43      0 exact   0.83 / 0.29,  0.58 / 0.40
    merge backward K_L / K_R       0.58 / 0.37      0 exact   0.46 / 0.27,  0.30 / 0.29
    SPP forward                    0.84             -         0.84       (CPU emulation 0.86; through spp_concat 0.58)
    SPP backward                   0.16             -         0.16
K3 forward, assemble forward, dF_edge and the SPP copies are bit-equal in every case, and so is every `exact` case.  The 1.000
of the in-order sums is a two-term sum: fl(a + b) against gamma(1) (|a| + |b|) is sharp when a and b have one sign.
Before spp_src forbade the contraction of scale * dst - i0 into an FMA (the compiler fused it in the backward kernels only), the
SPP backward measured 1.364 at (13, 8) -> (22, 14) -- the value the CPU file's emulation of that FMA gives -- and passed every
other case."""
import functools
import math

import numpy as np

U = 2.0 ** -24
F32 = np.float32
BIG = 1.0e4
SPECIALS = (0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x7F7FFFFF)  # -0.0, +inf, -inf, a NaN with a payload, FLT_MAX


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def ratio(got, ref, bound):
    """the largest err / bound over every element; got == ref demanded where the bound is zero; inf for a non-finite output"""
    got, ref, bound = (np.asarray(t, dtype=np.float64) for t in (got, ref, bound))
    got, ref, bound = np.broadcast_arrays(got, ref, bound)
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def bit_ratio(got, ref):
    """0.0 for the same bits, inf otherwise: a bit-equality check in the currency of the ratios"""
    return 0.0 if same_bits(got, ref) else np.inf


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def values(shape, which, seed):
    """float32 array of `shape` from the set `which`"""
    rng = np.random.default_rng(seed)
    if which == "exact":
        return rng.integers(-64, 65, size=shape).astype(F32)
    a = rng.standard_normal(shape).astype(F32)
    if which == "bits":
        flat = a.reshape(-1).view(np.uint32)
        at = np.arange(0, flat.size, 3)
        flat[at] = np.array(SPECIALS, dtype=np.uint32)[np.arange(at.size) % len(SPECIALS)]
    elif which == "big":
        a = (BIG * np.where(a >= 0, 1.0, -1.0)).astype(F32)
    return a


# ==== K3: the concat cost volume ==================================================================================================
# (B, C, h, w), d.  NCDHW: feat [B,C,h,w], cost [B,2C,d,h,w].  NDHWC: feat [B,h,w,C], cost [B,d,h,w,2C].
K3_NCDHW = [((2, 3, 2, 7), 5),      # scalar path, odd C
            ((1, 2, 3, 8), 3),      # float4 path
            ((1, 1, 1, 260), 6),    # w4 = 65 > 64 lanes; w > 256: the staging loop laps
            ((1, 1, 2, 261), 9),    # scalar path, the x loop past 64, d no multiple of 4 (waves get unequal shares)
            ((1, 2, 1, 5), 9),      # d > w: all-zero planes
            ((1, 1, 1, 1), 1)]
K3_NCDHW_WALK = ((1, 32, 68, 244), 3)   # backward: 1 061 888 items > 4096 x 256 threads
K3_NDHWC = [((1, 4, 2, 5), 3),
            ((2, 32, 3, 9), 12),
            ((1, 8, 1, 40), 4),         # w * per = 40 * 4 = 160 float4 of a row: one lap of the 256 threads
            ((1, 16, 1, 40), 4)]        # w * per = 40 * 8 = 320 > 256: the in-row loop laps
K3_NDHWC_FWD_WALK = ((2, 4, 64, 3), 65)     # 8320 rows > 8192 blocks
K3_NDHWC_BWD_WALK = ((1, 32, 260, 254), 2)  # 1 056 640 items
GRID_CAP = 4096 * 256


def k3_shapes(case, layout):
    (b, c, h, w), d = case
    return ((b, c, h, w), (b, 2 * c, d, h, w)) if layout == "ncdhw" else ((b, h, w, c), (b, d, h, w, 2 * c))


def _k3_seed(case, layout, which):
    (b, c, h, w), d = case
    return 9100 + 13 * b + 7 * c + 5 * h + 3 * w + 11 * d + (500 if layout == "ndhwc" else 0) + 37 * len(which)


@functools.lru_cache(maxsize=None)
def k3_inputs(case, layout, which):
    """(feat_l, feat_r, grad_cost); grad_cost is `plain` on the `bits` set"""
    fs, cs = k3_shapes(case, layout)
    s = _k3_seed(case, layout, which)
    return _ro(values(fs, which, s), values(fs, which, s + 1), values(cs, "plain" if which == "bits" else which, s + 2))


def k3_forward_ref(fl, fr, d, layout):
    """the header's definition as slice copies of the bit patterns: cost[.., i, .., x] = L[x] | R[x - i] for x >= i, else +0.0"""
    L, R = bits(fl), bits(fr)
    if layout == "ncdhw":
        b, c, h, w = L.shape
        cost = np.zeros((b, 2 * c, d, h, w), dtype=np.int32)
        for i in range(min(d, w)):
            cost[:, :c, i, :, i:] = L[:, :, :, i:]
            cost[:, c:, i, :, i:] = R[:, :, :, :w - i]
    else:
        b, h, w, c = L.shape
        cost = np.zeros((b, d, h, w, 2 * c), dtype=np.int32)
        for i in range(min(d, w)):
            cost[:, i, :, i:, :c] = L[:, :, i:, :]
            cost[:, i, :, i:, c:] = R[:, :, :w - i, :]
    return cost.view(F32)


def k3_backward_ref(g, d, layout):
    """(grad_l, grad_r, bound_l, bound_r) in fp64: grad_l[x] = sum_{i <= min(d-1, x)} g[c, i, y, x], grad_r[x] =
    sum_{i <= min(d-1, w-1-x)} g[C + c, i, y, x + i]; bound = gamma(n - 1) sum |terms|"""
    g = np.asarray(g)
    if layout == "ncdhw":
        b, c2, _, h, w = g.shape
        c = c2 // 2
        shape, xs = (b, c, h, w), (None, None, None, slice(None))
        left = lambda i: g[:, :c, i, :, i:]
        right = lambda i: g[:, c:, i, :, i:]
        cut = lambda t, lo, hi: t[:, :, :, lo:hi]
    else:
        b, _, h, w, c2 = g.shape
        c = c2 // 2
        shape, xs = (b, h, w, c), (None, None, slice(None), None)
        left = lambda i: g[:, i, :, i:, :c]
        right = lambda i: g[:, i, :, i:, c:]
        cut = lambda t, lo, hi: t[:, :, lo:hi, :]
    gl, gr, al, ar = (np.zeros(shape) for _ in range(4))
    for i in range(min(d, w)):
        t = left(i).astype(np.float64)
        cut(gl, i, w)[...] += t
        cut(al, i, w)[...] += np.abs(t)
        t = right(i).astype(np.float64)
        cut(gr, 0, w - i)[...] += t
        cut(ar, 0, w - i)[...] += np.abs(t)
    x = np.arange(w)
    nl, nr = np.minimum(d - 1, x) + 1, np.minimum(d - 1, w - 1 - x) + 1
    return gl, gr, gamma(nl - 1)[xs] * al, gamma(nr - 1)[xs] * ar


# ==== K3+K4 factored: assemble ====================================================================================================
# (B, H, W, D)
ASM_SHAPES = [(2, 3, 9, 1), (2, 3, 9, 2), (2, 3, 9, 3), (2, 3, 9, 5),
              (1, 2, 4, 8),                                  # D > W: XE = W
              (1, 2, 1, 3), (1, 2, 2, 2), (1, 2, 3, 1)]      # W <= 3: x = W - 1 coincides with the edge columns
ASM_FWD_WALK = (1, 130, 254, 4)    # 1 056 640 items
ASM_BWD_WALK = (1, 520, 254, 2)    # grad_f 1 056 640 items, grad_g 1 064 960


def num_classes(D):
    return min(D, 3)


def edge_width(D, W):
    return min(W, D + 1)


def depth_class(d, D):
    """first / middle / last plane; D = 2: first, last; D = 1: the only plane"""
    if D == 1 or d == 0:
        return 0
    if d == D - 1:
        return 1 if D == 2 else 2
    return 1


@functools.lru_cache(maxsize=None)
def asm_map(D, W):
    """include/azhip.h: out[b,d,y,x,:] = F[c(d), min(x-d, 2)][y, x] + G[c(d), x = W-1][y, x - d] for x - d >= -2, else 0.
    Per (d, x), as [D, W] integer arrays: valid; f_bulk = block of F_bulk's [W * NC] row-major (x, class) blocks, or -1;
    f_edge = block of F_edge's [XE * NC * 4] (x, class, delta + 2) blocks, or -1; g = block of G's [(W+2) * NC * 2]
    (x - d + 2, class, x = W-1) blocks.  (b, y and the 32 channels of a block pass straight through.)"""
    nc, xe = num_classes(D), edge_width(D, W)
    valid = np.zeros((D, W), dtype=bool)
    f_bulk, f_edge, gb = (np.full((D, W), -1, dtype=np.int64) for _ in range(3))
    for d in range(D):
        c = depth_class(d, D)
        for x in range(W):
            delta = x - d
            if delta < -2:
                continue
            valid[d, x] = True
            if delta >= 2:
                f_bulk[d, x] = x * nc + c
            else:
                assert x < xe
                f_edge[d, x] = (x * nc + c) * 4 + (delta + 2)
            gb[d, x] = ((delta + 2) * nc + c) * 2 + (1 if x == W - 1 else 0)
    return _ro(valid, f_bulk, f_edge, gb)


def asm_shapes(shape):
    B, H, W, D = shape
    nc, xe = num_classes(D), edge_width(D, W)
    return (B, H, W, nc * 32), (B, H, xe, nc * 128), (B, H, W + 2, nc * 64), (B, D, H, W, 32)


@functools.lru_cache(maxsize=None)
def asm_inputs(shape, which):
    """(F_bulk, F_edge, G, grad_out): independent operands, every slot its own values"""
    s = 9700 + sum(p * q for p, q in zip((3, 5, 7, 11), shape)) + 37 * len(which)
    return _ro(*(values(sh, which, s + k) for k, sh in enumerate(asm_shapes(shape))))


def asm_forward_ref(fb, fe, g, D):
    B, H, W, _ = fb.shape
    valid, f_bulk, f_edge, gb = asm_map(D, W)
    Fb, Fe, G = (t.reshape(B, H, -1, 32) for t in (fb, fe, g))
    out = np.zeros((B, D, H, W, 32), dtype=F32)
    for d, x in zip(*np.nonzero(valid)):
        f = Fb[:, :, f_bulk[d, x]] if f_bulk[d, x] >= 0 else Fe[:, :, f_edge[d, x]]
        out[:, d, :, x] = f + G[:, :, gb[d, x]]        # float32 + float32: one correctly rounded add
    return out


def asm_backward_ref(gy, D):
    """{name: (ref, bound)} of dF_bulk, dF_edge, dG: the transpose of asm_map by np.add.at in fp64"""
    B, _, H, W, _ = gy.shape
    valid, f_bulk, f_edge, gb = asm_map(D, W)
    shapes = asm_shapes((B, H, W, D))
    pay = np.moveaxis(np.asarray(gy, dtype=np.float64), (1, 3), (0, 1)).reshape(D * W, B, H, 32)   # [(d, x), b, y, 32]
    res = {}
    for name, idx, shp in (("dF_bulk", f_bulk, shapes[0]), ("dF_edge", f_edge, shapes[1]), ("dG", gb, shapes[2])):
        nblk = shp[2] * shp[3] // 32
        on = (idx.reshape(-1) >= 0) & valid.reshape(-1)
        at = idx.reshape(-1)[on]
        tot, ab, cnt = np.zeros((nblk, B, H, 32)), np.zeros((nblk, B, H, 32)), np.zeros(nblk)
        np.add.at(tot, at, pay[on])
        np.add.at(ab, at, np.abs(pay[on]))
        np.add.at(cnt, at, 1.0)
        back = lambda t: np.moveaxis(t, 0, 2).reshape(shp)
        res[name] = (back(tot), back(gamma(np.maximum(cnt - 1, 0))[:, None, None, None] * ab))
        if name == "dF_edge":
            assert cnt.max(initial=0) <= 1
    return res


# ==== K3+K4 factored: merge =======================================================================================================
MERGE_SETS = ("plain", "exact", "embedded_l", "embedded_r")


@functools.lru_cache(maxsize=None)
def merge_inputs(ncls, which):
    """(weight [32,64,3,3,3], ml [ncls,5,3,3], mr [ncls,2,3,3,5], gkl [ncls,5,32,32,3,3], gkr [ncls,2,32,32,3,5]) with random
    float masks (integers in [-3, 3] on `exact`)"""
    s = 9900 + 17 * ncls + 37 * len(which) + (1 if which.endswith("_r") else 0)
    kind = "exact" if which == "exact" else "plain"
    w = values((32, 64, 3, 3, 3), kind, s)
    gkl, gkr = values((ncls, 5, 32, 32, 3, 3), kind, s + 1), values((ncls, 2, 32, 32, 3, 5), kind, s + 2)
    if which == "embedded_l":
        w[:, 32:] = values((32, 32, 3, 3, 3), "big", s + 3)
        gkr = values(gkr.shape, "big", s + 4)
    elif which == "embedded_r":
        w[:, :32] = values((32, 32, 3, 3, 3), "big", s + 3)
        gkl = values(gkl.shape, "big", s + 4)
    if which == "exact":
        rng = np.random.default_rng(s + 5)
        ml, mr = (rng.integers(-3, 4, size=sh).astype(F32) for sh in ((ncls, 5, 3, 3), (ncls, 2, 3, 3, 5)))
    else:
        ml, mr = values((ncls, 5, 3, 3), "plain", s + 5), values((ncls, 2, 3, 3, 5), "plain", s + 6)
    return _ro(w, ml, mr, gkl, gkr)


def merge_forward_ref(w, ml, mr):
    """{kl, kr: (ref, bound)}: kl[c,e,o,i,h,w] = sum_d W[o,i,d,h,w] ML[c,e,d,w]; kr[c,e,o,i,h,j] = sum_{d,w} W[o,32+i,d,h,w]
    MR[c,e,d,w,j]"""
    w, ml, mr = (np.asarray(t, dtype=np.float64) for t in (w, ml, mr))
    kl = lambda a, m: np.einsum("oidhw,cedw->ceoihw", a[:, :32], m)
    kr = lambda a, m: np.einsum("oidhw,cedwj->ceoihj", a[:, 32:], m)
    return {"kl": (kl(w, ml), gamma(3) * kl(np.abs(w), np.abs(ml))), "kr": (kr(w, mr), gamma(9) * kr(np.abs(w), np.abs(mr)))}


def merge_backward_ref(gkl, gkr, ml, mr):
    """(grad_weight [32,64,3,3,3], bound): the adjoint of the two einsums"""
    gkl, gkr, ml, mr = (np.asarray(t, dtype=np.float64) for t in (gkl, gkr, ml, mr))
    ncls = ml.shape[0]
    left = lambda g, m: np.einsum("ceoihw,cedw->oidhw", g, m)
    right = lambda g, m: np.einsum("ceoihj,cedwj->oidhw", g, m)
    ref = np.concatenate([left(gkl, ml), right(gkr, mr)], axis=1)
    bound = np.concatenate([gamma(ncls * 5) * left(np.abs(gkl), np.abs(ml)),
                            gamma(ncls * 2 * 5) * right(np.abs(gkr), np.abs(mr))], axis=1)
    return ref, bound


# ==== SPP branch upsampling =======================================================================================================
# (hs, ws), (H, W), B, C
SPP_PRODUCTION = [((2, 3), (136, 240)), ((4, 7), (136, 240)), ((8, 15), (136, 240)), ((17, 30), (136, 240))]
SPP_PAIRS = [((1, 1), (8, 8)),       # a 1 x 1 source: a bit copy
             ((3, 5), (3, 5)),       # scale exactly 1: a bit copy
             ((5, 4), (17, 9)),
             ((1, 6), (1, 23)),
             ((6, 1), (23, 1)),
             ((4, 3), (1, 7)),       # H == 1 with hs > 1: scale 0 on a source with more than one row
             ((9, 8), (4, 3)),       # downsampling
             ((2, 2), (7, 300)),     # a long window: several laps per lane
             ((13, 8), (22, 14))]    # fl(scale (out-1)) > in-1 on both axes: l1 > 0 where both taps land on the last index
SPP_CHANNELS = (4, 8, 16, 32, 64)    # npl = 256, 128, 64, 32, 16
SPP_CASES = ([(s, d, 1, 32) for s, d in SPP_PRODUCTION] + [(s, d, 2, 32) for s, d in SPP_PAIRS]
             + [((5, 4), (17, 9), 2, c) for c in SPP_CHANNELS if c != 32])
SPP_COPIES = {((1, 1), (8, 8)), ((3, 5), (3, 5))}


def spp_scale(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)


def spp_positions(n_in, n_out):
    """(i0, ip, l0, l1) per destination index: the kernel's and ATen's fp32 recipe (area_pixel_compute_scale with
    align_corners=True): scale = fl(in-1)/fl(out-1), src = fl(scale dst), i0 = min(int(src), in-1), ip = i0 < in-1,
    l1 = fl(src - i0), l0 = fl(1 - l1)"""
    src = (spp_scale(n_in, n_out) * np.arange(n_out, dtype=F32)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    ip = (i0 < n_in - 1).astype(np.int64)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1.0) - l1).astype(F32)
    return i0, ip, l0, l1


def spp_forward_ref(x, H, W, positions=spp_positions):
    """x rows [B,hs,ws,C] -> (ref, bound) [B,H,W,C]: h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11) in fp64 from the fp32 weights"""
    x = np.asarray(x, dtype=np.float64)
    _, hs, ws, _ = x.shape
    y0, yp, h0, h1 = positions(hs, H)
    x0, xp, w0, w1 = positions(ws, W)
    h0, h1 = (t.astype(np.float64)[None, :, None, None] for t in (h0, h1))
    w0, w1 = (t.astype(np.float64)[None, None, :, None] for t in (w0, w1))
    tap = lambda yy, xx: x[:, yy][:, :, xx]
    x00, x01, x10, x11 = tap(y0, x0), tap(y0, x0 + xp), tap(y0 + yp, x0), tap(y0 + yp, x0 + xp)
    ref = h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11)
    mag = np.abs(h0) * (np.abs(w0 * x00) + np.abs(w1 * x01)) + np.abs(h1) * (np.abs(w0 * x10) + np.abs(w1 * x11))
    return ref, gamma(4) * mag


def spp_matrix(n_in, n_out):
    """[n_out, n_in] fp64: the forward's fp32 weights scattered by np.add.at (both taps land on the last source index there)"""
    i0, ip, l0, l1 = spp_positions(n_in, n_out)
    A = np.zeros((n_out, n_in))
    dst = np.arange(n_out)
    np.add.at(A, (dst, i0), l0.astype(np.float64))
    np.add.at(A, (dst, i0 + ip), l1.astype(np.float64))
    return A


def spp_window(n_in, n_out, i):
    """the kernel's spp_window in fp32: the destination indices [lo, hi] that may touch source index i"""
    scale = spp_scale(n_in, n_out)
    if not scale > 0:
        return 0, n_out - 1
    lo = max(0, int(np.floor(F32(i - 1) / scale)) - 1)
    hi = min(n_out - 1, int(np.ceil(F32(i + 1) / scale)) + 1)
    return lo, hi


def spp_roundings(hs, ws, H, W, C):
    """N of the backward bound (module docstring): per pass ceil(window / npl) + log2(npl) + 1, the two passes added"""
    npl = 256 // (C // 4)
    n = 0
    for n_in, n_out in ((ws, W), (hs, H)):
        window = max(hi - lo + 1 for lo, hi in (spp_window(n_in, n_out, i) for i in range(n_in)))
        n += math.ceil(window / npl) + int(math.log2(npl)) + 1
    return n


def spp_backward_ref(g, hs, ws):
    """g rows [B,H,W,C] -> (ref, bound) [B,hs,ws,C]"""
    g = np.asarray(g, dtype=np.float64)
    _, H, W, C = g.shape
    Ay, Ax = spp_matrix(hs, H), spp_matrix(ws, W)
    back = lambda t: np.einsum("yi,byjc->bijc", Ay, np.einsum("xj,byxc->byjc", Ax, t))
    return back(g), gamma(spp_roundings(hs, ws, H, W, C)) * np.einsum("yi,byjc->bijc", np.abs(Ay),
                                                                     np.einsum("xj,byxc->byjc", np.abs(Ax), np.abs(g)))


@functools.lru_cache(maxsize=None)
def spp_inputs(case):
    """(x rows [B,hs,ws,C], grad_out rows [B,H,W,C]) plain"""
    (hs, ws), (H, W), B, C = case
    s = 9300 + 3 * hs + 5 * ws + 7 * H + 11 * W + 13 * B + 17 * C
    return _ro(values((B, hs, ws, C), "plain", s), values((B, H, W, C), "plain", s + 1))


def spp_embed(a, cstride, at, seed):
    """rows [.., C] -> rows [.., cstride] holding `a` at channel `at` and +-1e4 in every other channel"""
    wide = values(a.shape[:-1] + (cstride,), "big", seed)
    wide[..., at:at + a.shape[-1]] = a
    return wide


# ==== the cached references and the checks, one place for the CPU model and the GPU sweep =======================================
@functools.lru_cache(maxsize=None)
def k3_reference(case, layout, which):
    fl, fr, g = k3_inputs(case, layout, which)
    d = case[1]
    gl, gr, bl, br = k3_backward_ref(g, d, layout)
    return dict(cost=_ro(k3_forward_ref(fl, fr, d, layout)), gl=_ro(gl), gr=_ro(gr), bl=_ro(bl), br=_ro(br))


def k3_check_forward(case, layout, which, cost):
    return bit_ratio(cost, k3_reference(case, layout, which)["cost"])


def k3_check_backward(case, layout, which, gl, gr):
    ref = k3_reference(case, layout, which)
    r = max(ratio(gl, ref["gl"], ref["bl"]), ratio(gr, ref["gr"], ref["br"]))
    if which == "exact" and not (same_bits(gl, ref["gl"].astype(F32) + F32(0)) and same_bits(gr, ref["gr"].astype(F32) + F32(0))):
        return np.inf       # (+ 0: a sum that starts at 0.f never returns -0.0)
    return r


@functools.lru_cache(maxsize=None)
def asm_reference(shape, which):
    fb, fe, g, gy = asm_inputs(shape, which)
    res = dict(out=_ro(asm_forward_ref(fb, fe, g, shape[3])))
    for k, (ref, bound) in asm_backward_ref(gy, shape[3]).items():
        res[k] = (_ro(ref), _ro(bound))
    return res


def asm_check_forward(shape, which, out):
    return bit_ratio(out, asm_reference(shape, which)["out"])


def asm_check_backward(shape, which, dfb, dfe, dg):
    """{dF_bulk, dF_edge, dG: ratio}; dF_edge by its bits (copies and +0.0), everything by its bits on `exact`"""
    ref = asm_reference(shape, which)
    r = {k: ratio(got, *ref[k]) for k, got in (("dF_bulk", dfb), ("dF_edge", dfe), ("dG", dg))}
    exact = ("dF_bulk", "dF_edge", "dG") if which == "exact" else ("dF_edge",)
    for k, got in (("dF_bulk", dfb), ("dF_edge", dfe), ("dG", dg)):
        if k in exact and not same_bits(got, ref[k][0].astype(F32) + F32(0)):
            r[k] = np.inf
    return r


def merge_check_forward(w, ml, mr, kl, kr, exact=False):
    ref = merge_forward_ref(w, ml, mr)
    r = {"kl": ratio(kl, *ref["kl"]), "kr": ratio(kr, *ref["kr"])}
    if exact and not (same_bits(kl, ref["kl"][0].astype(F32) + F32(0)) and same_bits(kr, ref["kr"][0].astype(F32) + F32(0))):
        return {"kl": np.inf, "kr": np.inf}
    return r


def merge_check_backward(gkl, gkr, ml, mr, gw, exact=False):
    ref, bound = merge_backward_ref(gkl, gkr, ml, mr)
    gw = np.asarray(gw).reshape(32, 64, 3, 3, 3)
    if exact and not same_bits(gw, ref.astype(F32) + F32(0)):
        return {"kl": np.inf, "kr": np.inf}
    return {"kl": ratio(gw[:, :32], ref[:, :32], bound[:, :32]), "kr": ratio(gw[:, 32:], ref[:, 32:], bound[:, 32:])}


@functools.lru_cache(maxsize=None)
def spp_reference(case):
    (hs, ws), (H, W), _, _ = case
    x, g = spp_inputs(case)
    return dict(fwd=_ro(*spp_forward_ref(x, H, W)), bwd=_ro(*spp_backward_ref(g, hs, ws)))


def spp_check_forward(case, out):
    r = ratio(out, *spp_reference(case)["fwd"])
    if (case[0], case[1]) in SPP_COPIES:       # scale 1 or a 1 x 1 source: the rows themselves
        x = spp_inputs(case)[0]
        want = x if case[0] == case[1] else np.broadcast_to(x, np.asarray(out).shape)
        return r if same_bits(out, want) else np.inf
    return r


def spp_check_backward(case, gin):
    r = ratio(gin, *spp_reference(case)["bwd"])
    if case[0] == case[1] and not same_bits(gin, spp_inputs(case)[1]):
        return np.inf
    return r
