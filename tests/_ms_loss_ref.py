"""What tests/test_gpu_ms_loss.py holds K29 to (numpy only): az_ms_loss_fwd / _bwd (csrc/az_ms_loss.hip) and
ops.multiscale_disp_loss restated per pixel in float32, in the kernel's own order of operations, with the rules a result is
compared by and the inputs of the comparison.  tests/test_ms_loss_error_model_cpu.py proves on the CPU that the rules
reject every wrong kernel of its list on these inputs.

The computation.  gt and mask are [B,1,H,W]; prediction k is [B,1,H >> s_k,W >> s_k] and its pixel (b, y, x) meets the
full-resolution pixel (b, y << s_k, x << s_k); valid: mask byte != 0 there, or lo < gt < hi without a mask.
  forward   term = (0.5f d) d if d < 1 else d - 0.5f, d = |p - g|, float32; acc[2k] = sum of the terms, acc[2k+1] = count
  backward  g_k = valid ? (w_k s_k) clamp_keep_nan(p - g, -1, 1) : 0,  s_k = gloss / float32(count_k)
  wrapper   loss = float32(sum_k w_k acc[2k] / acc[2k+1]) in fp64; scale_means[k] = float32(acc[2k] / acc[2k+1])

Rules: tests/_reduce_ref.py's, unchanged.  None is fitted to GPU output; every element of every case takes part.
  * counts are exact integers;
  * gradients equal the restatement as values (np.array_equal, NaN in the same places): every operation in them is one
    rounding -- p - g, gloss / count, w s, (w s) clamp -- and there is no multiply-add to contract; a prediction whose
    gradient was not asked for has None;
  * sums against math.fsum of the float32 terms within m 2^-52 sum|term| (check_sum);
  * the wrapper's scalar and per-scale means within scalar_bound.

Launch constants the sizes are built around (tests/test_ms_loss_error_model_cpu.py reads the source and fails when one
moves):
  BLOCK = 256      `#define MS_BLOCK 256`
  GRID_CAP = 1024  `#define MS_GRID_CAP 1024`: workgroups per prediction, forward and backward; a prediction of more than
                   GRID_CAP * BLOCK pixels is walked in passes

The golden bounds (tests/golden/g17_ms_loss.npz: the reference's dispnet_disp and default_disp evaluated in fp64 on the
float32 inputs cast to double).
  loss and per-scale means: |got - ref64| <= 5 * 2^-24 |ref64|
  gradients:                |got - ref64| <= 4 * 2^-24 |ref64| + one float32 ulp of w_k / count_k
Derivation.  The terms are non-negative, so a relative error of every term passes through sum and mean unchanged.  A term
errs by at most 3 * 2^-24 relative: in the quadratic branch the subtraction p - g rounds once (2^-24 of d), the square
doubles that, and the products add one rounding that matters ((0.5f d) is exact); in the linear branch the subtraction's
2^-24 d and the rounding of d - 0.5f, 2^-24 (d - 0.5), make (2 d - 0.5) 2^-24 on a term d - 0.5 >= 0.5, which is 3 * 2^-24
relative at d = 1 and tends to 2 * 2^-24 for large d.  The fp64 summation and the weighted sum add nothing visible at this
scale (m 2^-52); the final float32 rounding adds 2^-24; one more unit is slack for the float32 cast of the count inside
s_k, which only the gradients see: 5 in all.  A gradient is (w s) c with c = clamp(p - g): the subtraction (2^-24 |d|,
which the clamp passes on or removes), the division gloss / count, w s and the last product round once each, 4 * 2^-24
relative; where the clamp's argument is within rounding of +-1 the fp64 reference may sit on the other branch, by less
than 2^-24 |w s|, and a pixel with |ref| tiny keeps an absolute floor: one float32 ulp of w_k / count_k covers both.

Measured on an MI355X (largest err / bound over all cases, which tests/test_gpu_ms_loss.py prints; every count and every
gradient element: equal):
  acc[2k]  7.7e-05 at scale 0 (up to 262 437 terms; the bound is a worst case over orders), 0 at every coarser scale (so few
           terms of so few binades that fp64 adds them exactly)
  the wrapper's loss and scale_means: at most 0.991 of scalar_bound (1 x 64 x 128: a value just above a power of two, where
           one float32 rounding is the whole bound)
  golden, dispnet_disp (mask and range forms alike): loss 0.056, means 0.023 .. 0.160, gradients 0.057 .. 0.242
  golden, default_disp: loss 0.040, mean 0.040, gradient 0.253
  (the restatement itself gives the same golden ratios on the CPU: tests/test_ms_loss_error_model_cpu.py prints them)
"""
import math

import numpy as np

from tests import _reduce_ref as R
from tests._reduce_ref import down, fsum, scalar_bound, sum_bound, up  # noqa: F401  (the rules' own helpers)

F32 = np.float32
BLOCK, GRID_CAP, MS_LOSS_MAX = 256, 1024, 8
N_BIG = GRID_CAP * BLOCK + BLOCK + 37  # a second pass that only some workgroups take
DISPNET_WEIGHTS = (1.0, 1.0, 1.0, 0.8, 0.6, 0.4, 0.2)
GLOSS = 1.75
# (B, H, W), shifts
SHAPES = (((2, 70, 200), tuple(range(7))),     # down to 1 x 3
          ((2, 127, 65), tuple(range(7))),     # down to 1 x 1
          ((1, 64, 128), tuple(range(7))),     # exact powers of two
          ((3, 7, 33), (0, 1, 2)))             # per image 231, 48, 8 pixels: batch boundaries inside a block
FLAT_SHAPES = tuple(((1, 1, n), (0,)) for n in R.FLAT)
BIG_SHAPE = ((1, 1, N_BIG), (0,))


# ---- geometry ----------------------------------------------------------------------------------------------------------
def scale_size(H, W, s, defect=None):
    """(h, w) of scale s: floor, H >> s"""
    if defect == "ceil_size":
        return -(-H // (1 << s)), -(-W // (1 << s))
    return H >> s, W >> s


def src_index(B, H, W, s, h, w, defect=None):
    """flat index into [B,1,H,W] of the pixel that flat pixel i of a [B,1,h,w] prediction meets"""
    i = np.arange(B * h * w, dtype=np.int64)
    b, r = i // (h * w), i % (h * w)
    y, x = r // w, r % w
    sy, sx = y << s, x << s
    if defect == "src_plus1":  # dst * 2^s + 1 (kept inside the map, as a clamped read would be)
        sy, sx = np.minimum(sy + 1, H - 1), np.minimum(sx + 1, W - 1)
    if defect == "ceil_size":  # sizes by ceil: the last row / column reads past the map; clamped
        sy, sx = np.minimum(sy, H - 1), np.minimum(sx, W - 1)
    stride_b = h * w if defect == "batch_stride_hw" else H * W
    return np.minimum(b * stride_b + sy * W + sx, B * H * W - 1)


def _covered(n, defect):
    """the pixels of ONE prediction a launch visits: all -- or, for the mutants, not the last n % 256 / only the first pass"""
    i = np.arange(n)
    if defect == "tail":
        return i < n - n % BLOCK
    if defect == "one_pass":
        return i < GRID_CAP * BLOCK
    return np.ones(n, dtype=bool)


def _valid(gt, mask, lo, hi, src, own, defect=None):
    """ms_valid at the strided pixel (mutant: the mask byte at the prediction's own flat index)"""
    g = gt.ravel()[src]
    if mask is None:
        return R.k12_valid(g, None, lo, hi)
    m = mask.ravel().view(np.uint8) if mask.dtype == np.bool_ else mask.ravel()
    return m[own if defect == "mask_own_index" else src] != 0


def _geometry(preds, shifts, gt, defect):
    B, _, H, W = gt.shape
    for p, s in zip(preds, shifts):
        h, w = p.shape[2], p.shape[3]
        if defect == "ceil_size":  # the kernel takes the prediction for [B,1,ceil,ceil] and walks it with that row length
            h, w = scale_size(H, W, s, defect)
        yield p.ravel(), src_index(B, H, W, s, h, w, defect)[:p.size], np.arange(p.size)


# ---- the kernels -------------------------------------------------------------------------------------------------------
def ms_fwd(preds, shifts, gt, mask, lo, hi, defect=None):
    """[(float32 terms over prediction k's valid pixels, count)]"""
    out = []
    for p, src, own in _geometry(preds, shifts, gt, defect):
        ok = _valid(gt, mask, lo, hi, src, own, defect) & _covered(p.size, defect)
        with np.errstate(invalid="ignore", over="ignore"):
            terms = R.smooth_l1(np.abs(p[ok] - gt.ravel()[src][ok]))
        out.append((terms, int(ok.sum())))
    if defect == "shared_count":  # one count for all scales: scale 0's
        out = [(t, out[0][1]) for t, _ in out]
    return out


def ms_fwd_acc(preds, shifts, gt, mask, lo, hi, defect=None):
    """acc [nd, 2] of a kernel that sums exactly"""
    return np.array([[fsum(t), float(c)] for t, c in ms_fwd(preds, shifts, gt, mask, lo, hi, defect)]).reshape(-1, 2)


def ms_bwd(preds, shifts, weights, gt, mask, lo, hi, gloss, counts, need=None, defect=None):
    """[g_k float32 or None]: s = gloss / float32(count_k); (w_k s) clamp(p - g, -1, 1) on valid pixels, 0 elsewhere; pixels a
    mutant does not visit keep the NaN the output buffer was filled with"""
    need = [True] * len(preds) if need is None else need
    if defect == "weights_reversed":
        weights = weights[::-1]
    out = []
    for k, (p, src, own) in enumerate(_geometry(preds, shifts, gt, defect)):
        if not need[k]:
            out.append(None)
            continue
        ok = _valid(gt, mask, lo, hi, src, own, defect)
        seen = _covered(p.size, defect)
        with np.errstate(all="ignore"):
            s = F32(gloss) / F32(counts[0 if defect == "shared_count" else k])
            c = R.clamp1(p - gt.ravel()[src], "clamp_fmin" if defect == "clamp_fmin" else None)
            if defect == "mul_order":
                v = F32(weights[k]) * (s * c)
            else:
                v = (F32(weights[k]) * s) * c
            if defect == "empty_mul":  # the mask multiplied in: inf * 0 = NaN on an empty scale
                v = (v * ok.astype(F32)).astype(F32)
            else:
                v = np.where(ok, v, F32(0)).astype(F32)
        out.append(np.where(seen, v, F32(np.nan)).reshape(preds[k].shape))
    return out


def ms_scalars(preds, shifts, weights, gt, mask, lo, hi):
    """(loss in fp64 from the exact sums, its bound, [mean_k], [bound of mean_k]); an empty scale: NaN, as 0 / 0"""
    loss = prop = 0.0
    means, bounds = [], []
    for w, (terms, count) in zip(weights, ms_fwd(preds, shifts, gt, mask, lo, hi)):
        if count == 0:
            means.append(math.nan), bounds.append(0.0)
            loss = math.nan
            continue
        m = fsum(terms) / count
        means.append(m), bounds.append(scalar_bound(m, sum_bound(terms) / count))
        loss += w * m
        prop += w * sum_bound(terms) / count
    return loss, (scalar_bound(loss, prop) if math.isfinite(loss) else 0.0), means, bounds


# ---- the rules ---------------------------------------------------------------------------------------------------------
def check_fwd(acc, preds, shifts, gt, mask, lo, hi, what="az_ms_loss_fwd"):
    """{accumulator: err / bound}; counts exact"""
    acc = np.asarray(acc, dtype=np.float64).reshape(-1, 2)
    want = ms_fwd(preds, shifts, gt, mask, lo, hi)
    assert acc.shape[0] == len(want), f"{what}: {acc.shape[0]} accumulator pairs for {len(want)} predictions"
    out = {}
    for k, (terms, count) in enumerate(want):
        R._same_int(acc[k, 1], count, f"{what} acc[{2 * k + 1}] (count of scale {shifts[k]})")
        out[f"acc[{2 * k}]"] = R.check_sum(float(acc[k, 0]), terms, f"{what} acc[{2 * k}]")
    return out


def check_bwd(grads, preds, shifts, weights, gt, mask, lo, hi, gloss, counts, need=None, what="az_ms_loss_bwd"):
    want = ms_bwd(preds, shifts, weights, gt, mask, lo, hi, gloss, counts, need)
    assert len(grads) == len(want), what
    n = 0
    for k, (g, wnt) in enumerate(zip(grads, want)):
        if wnt is None:
            assert g is None, f"{what}: prediction {k} needs no gradient but got one"
            continue
        assert g is not None, f"{what}: prediction {k} needs a gradient, got None"
        n += R.check_grad(g, wnt, f"{what} g_pred[{k}]")
    return n


def _check_scalar(got, want, bound, what):
    got = float(got)
    if not math.isfinite(want):
        if not ((math.isnan(got) and math.isnan(want)) or got == want):
            raise AssertionError(f"{what}: got {got}, {want} expected")
        return 0.0
    return R._ratio(abs(got - want), bound, what)


def check_scalars(loss, means, preds, shifts, weights, gt, mask, lo, hi, what="multiscale_disp_loss"):
    """largest err / bound of the scalar and the per-scale means"""
    want, bound, wm, wb = ms_scalars(preds, shifts, weights, gt, mask, lo, hi)
    r = [_check_scalar(loss, want, bound, f"{what} loss")]
    means = np.asarray(means, dtype=np.float64).ravel()
    assert means.size == len(wm), what
    r += [_check_scalar(m, a, b, f"{what} scale_means[{k}]") for k, (m, a, b) in enumerate(zip(means, wm, wb))]
    return max(r)


def golden_scalar_ratio(got, ref64, what):
    """|got - ref64| / (5 * 2^-24 |ref64|); AssertionError above 1"""
    return R._ratio(abs(float(got) - float(ref64)), 5 * 2.0 ** -24 * abs(float(ref64)), what)


def golden_grad_ratio(got, ref64, weight, count, what):
    """largest |got - ref64| / (4 * 2^-24 |ref64| + ulp32(w / count)) over the map; AssertionError above 1"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, what
    ulp = float(np.spacing(F32(weight / count)))
    ratio = np.abs(got - ref64) / (4 * 2.0 ** -24 * np.abs(ref64) + ulp)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(np.argmax(ratio))
        raise AssertionError(f"{what}: err / bound {worst:.4g} at {i}: got {got.ravel()[i]!r}, fp64 {ref64.ravel()[i]!r}")
    return worst


# ---- inputs ------------------------------------------------------------------------------------------------------------
def special_positions(n, per_image):
    """flat pixels of one prediction where kernels go wrong: 0 and n - 1, both sides of every block boundary that exists up
    to 512, of the end of the first pass and of every batch boundary"""
    pos = {0, n - 1}
    pos |= {p for p in (BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, GRID_CAP * BLOCK - 1, GRID_CAP * BLOCK) if p < n}
    for b in range(1, n // per_image):
        pos |= {b * per_image - 1, b * per_image}
    return sorted(pos)


# with g = 1.5: d exactly 1 (p = 0.5, 2.5), up(1), down(1), just over 1 from above, and 0
EDGE_PREDS = (F32(0.5), F32(0.5) - F32(2.0 ** -23), F32(0.5) + F32(2.0 ** -24), F32(2.5), F32(2.5) + F32(2.0 ** -22), F32(1.5))
# ground truths on and beside lo / hi of R.RANGES, the neighbours of 0, negative, inf, NaN: (value, mask byte)
EDGE_GTS = tuple((F32(g), 1) for g in (1, down(1), up(1), 192, down(192), up(192), 0, -0.0, 2.0 ** -126, 1e-45, -3)) + \
    ((F32(np.inf), 0), (F32(np.nan), 0))


def ms_case(shape, shifts, seed, only_scale0=False, nonfinite_preds=False):
    """dict preds [nd], gt, mask (uint8), shifts, weights, shape.  Bulk: gt in [1.5, 100), predictions within 2.5 of the pixel
    they meet, mask bytes 0 / 1 (70 % valid).  Then, scale after scale, the ground truths of EDGE_GTS on pixels that scale
    reads; mask bytes 2 and 255; and at every special position of every prediction a valid pixel (g = 1.5, bytes 1 / 2 /
    255 in turn) whose prediction runs through EDGE_PREDS.  only_scale0: every pixel with even y and even x is invalid
    under the mask and under both ranges (gt = 0), so that scales >= 1 are empty.  nonfinite_preds: NaN / +inf / -inf
    predictions on valid pixels of every prediction (backward only: they make the forward sums NaN / inf)"""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    n = B * H * W
    gt = rng.uniform(1.5, 100.0, n).astype(F32)
    mask = (rng.uniform(0, 1, n) > 0.3).astype(np.uint8)
    geo = []
    for s in shifts:
        h, w = scale_size(H, W, s)
        geo.append((h, w, src_index(B, H, W, s, h, w)))
    taken = set()
    for j, (g, m) in enumerate(EDGE_GTS):  # edge ground truths, on pixels the scales read in turn
        h, w, src = geo[j % len(geo)]
        q = int(src[(3 + 7 * j) % src.size])
        if q not in taken:
            gt[q], mask[q] = g, m
            taken.add(q)
    for j, byte in enumerate((2, 255, 0)):
        q = int(geo[j % len(geo)][2][(5 + 11 * j) % geo[j % len(geo)][2].size])
        if q not in taken:
            gt[q], mask[q] = F32(7.25), byte
            taken.add(q)
    special = []
    r = 0
    for k, (h, w, src) in enumerate(geo):
        pos = special_positions(src.size, h * w)
        if nonfinite_preds:
            pos = sorted(set(pos) | {q for q in (2, 3, 4) if q < src.size})
        for i in pos:
            gt[src[i]], mask[src[i]] = F32(1.5), (1, 2, 255)[r % 3]
            special.append((k, i, r))
            r += 1
    if only_scale0:
        g2, m2 = gt.reshape(B, H, W), mask.reshape(B, H, W)
        g2[:, ::2, ::2], m2[:, ::2, ::2] = F32(0), 0
    preds = []
    for k, (h, w, src) in enumerate(geo):
        with np.errstate(invalid="ignore"):
            p = (gt[src] + rng.uniform(-2.5, 2.5, src.size).astype(F32)).astype(F32)
        p[~np.isfinite(p)] = F32(5)
        preds.append(p)
    for k, i, r in special:
        preds[k][i] = EDGE_PREDS[r % len(EDGE_PREDS)]
    if nonfinite_preds:
        for k, (h, w, src) in enumerate(geo):
            for q, bad in zip((2, 3, 4), (F32(np.nan), F32(np.inf), F32(-np.inf))):
                if q < src.size and q not in special_positions(src.size, h * w):
                    preds[k][q] = bad
    weights = DISPNET_WEIGHTS[:len(shifts)]
    return dict(preds=[p.reshape(B, 1, h, w) for p, (h, w, _) in zip(preds, geo)], gt=gt.reshape(B, 1, H, W),
                mask=mask.reshape(B, 1, H, W), shifts=tuple(shifts), weights=tuple(weights), shape=shape,
                name="x".join(map(str, shape)) + f" scales {shifts[0]}..{shifts[-1]}" + (" only scale 0 valid" if only_scale0 else ""))


_CASES = {}


def all_cases(nonfinite_preds=False):
    """every case, smallest first, built once and never written to"""
    if nonfinite_preds not in _CASES:
        out = [ms_case(shape, shifts, 7500 + k, nonfinite_preds=nonfinite_preds)
               for k, (shape, shifts) in enumerate(FLAT_SHAPES + SHAPES[::-1] + (BIG_SHAPE,))]
        out.insert(len(FLAT_SHAPES), ms_case((2, 24, 40), (0, 1, 2, 3), 7590, only_scale0=True, nonfinite_preds=nonfinite_preds))
        for c in out:
            for a in c["preds"] + [c["gt"], c["mask"]]:
                a.setflags(write=False)
        _CASES[nonfinite_preds] = out
    return _CASES[nonfinite_preds]


def modes(case):
    """(name, mask, lo, hi): the byte mask, the same mask as bool, then the in-kernel range rule under each of R.RANGES"""
    yield "byte mask", case["mask"], 0.0, math.inf
    yield "bool mask", case["mask"] != 0, 0.0, math.inf
    for lo, hi in R.RANGES:
        yield f"range ({lo:g}, {hi:g})", None, lo, hi
