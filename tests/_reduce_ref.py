"""What tests/test_gpu_reduce_exact.py holds the reductions to (numpy only): the kernels that turn a whole map into a few
numbers -- K12 az_disp_loss_fwd / _bwd and az_disp_metrics (csrc/az_disp_loss.hip), K16 az_seq_loss_fwd / _bwd
(csrc/az_convex_up.hip), az_absmax and az_absmax_multi (csrc/az_absmax.hip) -- restated per pixel in float32, in the
kernel's own order of operations, together with the rules a result is compared by and the inputs of the comparison.
tests/test_reduce_error_model_cpu.py proves on the CPU that the rules reject every wrong kernel of its list on these inputs.

Rules.  None is fitted to GPU output; every element of every case takes part.
  * Counts (acc4[3], acc8[1, 2, 4, 5, 6, 7], acc3[1], acc3[2]) are exact integers: every term is 0.0 or 1.0 and a map has
    far fewer than 2^53 pixels.
  * Gradients equal the restatement as values (np.array_equal, NaN in the same places): every operation in them is one
    rounding, w * s, (w s) * clamp, weight * gloss, (.) / count -- there is no multiply-add to contract.
  * Sums (acc4[0..2], acc8[0], acc3[0]) against math.fsum of the float32 terms.  The kernel adds m float32 terms in fp64
    in an unspecified order (lane, wave, LDS, one atomic per block).  m - 1 additions, each rounded once, give in first
    order |err| <= (m - 1) 2^-53 sum|term|; the tolerance is twice that, m 2^-52 sum|term|, for the higher-order part
    ((1 + u)^(m-1) - 1 <= 2 (m - 1) u while m u < 1, and m < 2^21 here).  A sum of zeros must be 0.
  * acc8[3], the clipped millimetre error, is the one sum whose TERM the compiler may evaluate in more than one way:
    |zg * 1000 - zp * 1000| may become fma(zg, 1000, -(zp * 1000)) under hipcc's default contraction.  It is compared with
    the fp64 evaluation of the float32 inputs (zp as restated), each term granted 3 * 2^-24 (|1000 zg| + |1000 zp|) -- two
    product roundings and the subtraction's, of which a fused operation only removes one; the clip to [0, 100] is
    1-Lipschitz, so the bound passes through it -- plus the summation term above.
  * The wrappers' scalars (ops.disp_loss, ops.sequence_loss, the dict of compute_err_metric) are within one float32
    rounding, 2^-24 relative, of the fp64 formula on the exact accumulators, plus what the formula makes of the
    accumulators' own bounds (scalar_bound).
  * absmax: max(am[::AZ_AMAX_STRIDE]) equals the restatement bit for bit.

Launch constants the sizes are built around, each beside the line it restates (tests/test_reduce_error_model_cpu.py reads
the sources and fails when one moves):
  BLOCK = 256            `#define DL_BLOCK 256` (az_disp_loss.hip), `#define SL_BLOCK 256` (az_convex_up.hip),
                         `__launch_bounds__(256)` of absmax_kernel
  RED_CAP = 1024 blocks  `return g > 1024u ? 1024u : g;` in dl_reduce_grid and sl_reduce_grid: the reductions
  EW_CAP = 4096 blocks   `if (g > 256LL * 16) g = 256LL * 16;` in az_grid_for (az_common.h): the backward kernels, absmax
  ABSMAX_VEC = 4         `const long long n4 = n >> 2;` in absmax_kernel: four floats per work item, the `n & 3` tail by
                         the first `n & 3` threads of block 0

Measured on an MI355X (largest err / bound over all cases of tests/test_gpu_reduce_exact.py, which prints them; every
count, every gradient element and every absmax: equal):
  acc4[0] 6.18e-05   acc4[1] 5.70e-05   acc4[2] 5.23e-05   (az_disp_loss_fwd: m up to 1 048 864 terms; the bound is a worst
                                                            case over orders, a real order errs like sqrt(m), not like m)
  acc8[0] 0          acc3[0] 0          (|dg - dp| and |p - t| span so few binades that fp64 adds a million of them exactly)
  acc8[3] 4.28e-02   (the millimetre terms: the per-term allowance for the contracted multiply-add is what is used)
  the wrappers' scalars: inside scalar_bound in every case
  a weight tensor with one inf / NaN: the other output channels within 0.030 (Conv3d 32 -> 32) and 0.024 (Conv2d 64 -> 64) of
  the f16x3 contract bound, the same figures as with finite weights (0.030, 0.026); before the weights' amax came from
  az_absmax_multi those channels were exact zeros, 1.4e5 times the bound
"""
import math

import numpy as np

F32 = np.float32
BLOCK, RED_CAP, EW_CAP, ABSMAX_VEC = 256, 1024, 4096, 4
AMAX_SLOTS, AMAX_STRIDE = 16, 64  # include/azhip.h AZ_AMAX_SLOTS / AZ_AMAX_STRIDE (checked against _lib.CONST by the tests)
AMAX_FLOATS = AMAX_SLOTS * AMAX_STRIDE
U = 2.0 ** -53

FLAT = (1, 63, 64, 65, 255, 256, 257, 1000)
N_RED = RED_CAP * BLOCK + BLOCK + 37   # a second reduction pass that only some blocks take
N_EW = EW_CAP * BLOCK + BLOCK + 37     # the same for the backward kernels
SHAPED = ((3, 1, 7, 33), (2, 1, 24, 40))  # per_batch 231: batch boundaries inside blocks
MAP_SHAPES = tuple((1, 1, 1, n) for n in FLAT) + SHAPED + ((1, 1, 1, N_RED), (1, 1, 1, N_EW))
ABSMAX_N = (1, 2, 3, 4, 5, 7, 1021, ABSMAX_VEC * EW_CAP * BLOCK + ABSMAX_VEC * 300 + 3)
LOSS_WEIGHTS = (1.0, 0.7, 0.5)  # pred3, pred2, pred1 (ops._DispLoss.WEIGHTS)
RANGES = ((0.0, math.inf), (1.0, 192.0))  # (lo, hi) of the in-kernel range mask: the default and a bounded one
FB = (24.75, 3.0, 101.5)  # focal * baseline per batch element: clearly different

def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def fsum(terms):
    """exact sum of float32 / float64 terms, correctly rounded; NaN / inf by class"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    if not np.isfinite(t).all():
        with np.errstate(invalid="ignore"):
            return float(t.sum())
    return math.fsum(t.tolist())


def sum_bound(terms, calls=1):
    """m 2^-52 sum|term| for the term list taken `calls` times"""
    t = np.abs(np.asarray(terms, dtype=np.float64).ravel())
    return calls * t.size * 2.0 * U * calls * math.fsum(t.tolist())


def _covered(n, defect, cap):
    """the pixels a launch visits: all -- or, for the mutants, not the last n % 256 / only the first pass of `cap` blocks"""
    i = np.arange(n)
    if defect == "tail":
        return i < n - n % BLOCK
    if defect == "one_pass":
        return i < cap * BLOCK
    return np.ones(n, dtype=bool)


# ---- K12 ---------------------------------------------------------------------------------------------------------------
def k12_valid(gt, mask, lo, hi, defect=None):
    """dl_valid: mask[i] != 0, or lo < gt < hi when there is no mask"""
    if mask is not None:
        return (mask == 1) if defect == "mask_eq1" else (mask != 0)
    with np.errstate(invalid="ignore"):
        a = gt >= F32(lo) if defect == "lo_incl" else gt > F32(lo)
        b = gt <= F32(hi) if defect == "hi_incl" else gt < F32(hi)
    return a & b


def smooth_l1(d, defect=None):
    """(0.5f d) d if d < 1 else d - 0.5f, float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        quad = (d <= F32(1)) if defect == "branch_le" else (d < F32(1))
        return np.where(quad, (F32(0.5) * d) * d, d - F32(0.5)).astype(F32)


def k12_fwd(preds, gt, mask, lo, hi, defect=None):
    """(terms of pred3, pred2, pred1 over the valid pixels [3][count] float32, count)"""
    gt = gt.ravel()
    ok = k12_valid(gt, None if mask is None else mask.ravel(), lo, hi, defect) & _covered(gt.size, defect, RED_CAP)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = [smooth_l1(np.abs(p.ravel()[ok] - gt[ok]), defect) for p in preds]
    return terms, int(ok.sum())


def k12_fwd_acc(preds, gt, mask, lo, hi, defect=None):
    """acc4 of a kernel that sums exactly"""
    terms, count = k12_fwd(preds, gt, mask, lo, hi, defect)
    return np.array([fsum(t) for t in terms] + [float(count)])


def clamp1(d, defect=None):
    """clamp(d, -1, 1) that keeps NaN (np.minimum / np.maximum propagate it; fmin / fmax, the mutant, drop it)"""
    if defect == "clamp_fmin":
        return np.fmin(np.fmax(d, F32(-1)), F32(1))
    return np.minimum(np.maximum(d, F32(-1)), F32(1))


def k12_bwd(preds, gt, mask, lo, hi, gloss, count, weights=LOSS_WEIGHTS, defect=None):
    """[g3, g2, g1] float32 maps: s = gloss / float32(count); (w_k s) clamp(p_k - g, -1, 1) on valid pixels, 0 elsewhere;
    pixels a mutant does not visit keep the NaN the output buffer was filled with"""
    g = gt.ravel()
    ok = k12_valid(g, None if mask is None else mask.ravel(), lo, hi, defect)
    seen = _covered(g.size, defect, EW_CAP)
    with np.errstate(all="ignore"):
        s = F32(gloss) / F32(count)
        out = []
        for w, p in zip(weights, preds):
            v = (F32(w) * s) * clamp1(p.ravel() - g, defect)
            v = np.where(ok, v, F32(0)).astype(F32)
            out.append(np.where(seen, v, F32(np.nan)).reshape(gt.shape))
    return out


THRESHOLDS = (F32(1), F32(2), F32(2e-3), F32(4e-3), F32(8e-3))  # the float32 constants 1.f, 2.f, 2e-3f, 4e-3f, 8e-3f


def k12_metrics(dg, zg, dp, zp, fb, mask, per_batch, defect=None):
    """dict: dd (float32 terms), mm64 (fp64 millimetre terms), mm_tol (per-term allowance), counts [#dd>1, #dd>2, #dz>2e-3,
    #dz>4e-3, #dz>8e-3, count], over the masked pixels"""
    dg, zg, dp, m = dg.ravel(), zg.ravel(), dp.ravel(), mask.ravel()
    n = dg.size
    ok = ((m == 1) if defect == "mask_eq1" else (m != 0)) & _covered(n, defect, RED_CAP)
    i = np.arange(n)[ok]
    dgv, zgv, dpv = dg[ok], zg[ok], dp[ok]
    with np.errstate(all="ignore"):
        dd = np.abs(dgv - dpv)
        if zp is not None:
            zpv = zp.ravel()[ok]
        else:
            fb = np.asarray(fb, dtype=F32)
            b = i // per_batch
            if defect == "fb0":
                b = np.zeros_like(b)
            elif defect == "fb_block":
                b = np.minimum((i + (BLOCK - 1)) // per_batch, fb.size - 1)
            zpv = (fb[b] / dpv).astype(F32)  # IEEE float32 division
        dz = np.abs(zgv - zpv)
        z64, p64 = zgv.astype(np.float64) * 1000.0, zpv.astype(np.float64) * 1000.0
        mm64 = np.minimum(np.maximum(np.abs(z64 - p64), 0.0), 100.0)
        mm_tol = 3.0 * 2.0 ** -24 * (np.abs(z64) + np.abs(p64))
    cmp = [(lambda a, t: a >= t) if defect == f"ge{k}" else (lambda a, t: a > t) for k in range(5)]
    counts = [int(cmp[0](dd, THRESHOLDS[0]).sum()), int(cmp[1](dd, THRESHOLDS[1]).sum()),
              int(cmp[2](dz, THRESHOLDS[2]).sum()), int(cmp[3](dz, THRESHOLDS[3]).sum()),
              int(cmp[4](dz, THRESHOLDS[4]).sum()), int(ok.sum())]
    return dict(dd=dd, mm64=mm64, mm_tol=mm_tol, counts=counts)


def k12_metrics_acc(*args, **kw):
    """acc8 of a kernel that sums exactly (its millimetre terms evaluated in fp64)"""
    r = k12_metrics(*args, **kw)
    c = r["counts"]
    return np.array([fsum(r["dd"]), c[0], c[1], fsum(r["mm64"]), c[2], c[3], c[4], c[5]], dtype=np.float64)


# ---- K16 ---------------------------------------------------------------------------------------------------------------
def k16_valid(gt, valid, max_flow, defect=None):
    """sl_valid: float32(valid) >= 0.5 and |gt| < max_flow (valid: float32, uint8 or bool map)"""
    v = valid.ravel().astype(F32)
    with np.errstate(invalid="ignore"):
        a = v > F32(0.5) if defect == "valid_gt" else v >= F32(0.5)
        b = np.abs(gt) <= F32(max_flow) if defect == "flow_le" else np.abs(gt) < F32(max_flow)
    return a & b


def k16_fwd(pred, gt, valid, max_flow, tsign, defect=None):
    """(terms |p - tsign g| over the valid pixels, count, number of non-finite predictions over ALL pixels)"""
    p, g = pred.ravel(), gt.ravel()
    seen = _covered(g.size, defect, RED_CAP)
    ok = k16_valid(g, valid, max_flow, defect) & seen
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.abs(p[ok] - F32(tsign) * g[ok])
    bad = ~np.isfinite(p) & seen
    if defect == "nonfinite_valid":
        bad &= ok
    return terms, int(ok.sum()), int(bad.sum())


def k16_fwd_acc(*args, **kw):
    terms, count, bad = k16_fwd(*args, **kw)
    return np.array([fsum(terms), float(count), float(bad)])


def k16_bwd(pred, gt, valid, max_flow, tsign, gloss, count, weight, defect=None):
    """s = (float32(weight) gloss) / float32(count); +s / -s by the sign of d = p - tsign g, 0 * d for d == 0 (NaN stays NaN),
    0 on invalid pixels"""
    p, g = pred.ravel(), gt.ravel()
    ok = k16_valid(g, valid, max_flow, defect)
    seen = _covered(g.size, defect, EW_CAP)
    with np.errstate(all="ignore"):
        s = (F32(weight) * F32(gloss)) / F32(count)
        d = p - F32(tsign) * g
        zero = np.full_like(d, s) if defect == "sign0" else F32(0) * d
        sg = np.where(d > 0, s, np.where(d < 0, -s, zero)).astype(F32)
    out = np.where(ok, sg, F32(0)).astype(F32)
    return np.where(seen, out, F32(np.nan)).reshape(gt.shape)


# ---- absmax ------------------------------------------------------------------------------------------------------------
def finite_abs_bits(x, defect=None):
    """az_finite_abs_bits: bits(x) & 0x7fffffff, 0 for inf / NaN"""
    x = np.ascontiguousarray(x, dtype=F32).ravel()
    if defect == "signed":  # max of the signed values: a negative element never wins
        with np.errstate(invalid="ignore"):
            x = np.where(x > 0, x, F32(0))
    b = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return b if defect == "keep_inf" else np.where(b < np.uint32(0x7F800000), b, np.uint32(0))


def absmax_bits(x):
    """the largest finite |x| as a bit pattern, 0 when there is none"""
    b = finite_abs_bits(x)
    return int(b.max()) if b.size else 0


def absmax_array(x, defect=None):
    """the amax array az_absmax leaves, as uint32 [AMAX_FLOATS]: work item i = floats 4i..4i+3 goes to block
    (i / 256) mod grid, grid = min(ceil(ceil(n / 4) / 256), EW_CAP); a block's maximum lands in slot block & 15; the n & 3
    tail belongs to block 0"""
    b = finite_abs_bits(x, defect)
    n = b.size
    n4 = n // ABSMAX_VEC
    grid = min(max(((n + 3) // 4 + BLOCK - 1) // BLOCK, 1), EW_CAP)
    out = np.zeros(AMAX_FLOATS, dtype=np.uint32)
    if n4:
        item = b[:4 * n4].reshape(n4, 4).max(axis=1)
        slot = ((np.arange(n4) // BLOCK) % grid) & (AMAX_SLOTS - 1)
        for k in range(AMAX_SLOTS):
            sel = item[slot == k]
            if sel.size:
                out[k * AMAX_STRIDE] = sel.max()
    if n & 3 and defect != "no_tail":
        out[0] = max(out[0], b[4 * n4:].max())
    return out


def amax_read(arr, defect=None):
    """what a reader of an amax array takes: the largest slot (uint32 view)"""
    arr = np.asarray(arr).view(np.uint32)
    return int(arr[0]) if defect == "slot0" else int(arr[::AMAX_STRIDE].max())


# ---- the rules ---------------------------------------------------------------------------------------------------------
def _ratio(err, bound, what):
    """err / bound, 0 / 0 = 0; AssertionError when the bound is missed"""
    if not (err <= bound):
        raise AssertionError(f"{what}: |err| {err:.6g} > bound {bound:.6g}")
    return err / bound if bound > 0 else 0.0


def _same_int(got, want, what):
    if not (float(got) == float(want)):
        raise AssertionError(f"{what}: got {got!r}, exactly {want} expected")


def check_sum(got, terms, what, calls=1, extra=0.0):
    """got against fsum(terms) * calls within sum_bound (+ extra, the terms' own allowance); returns err / bound"""
    want = calls * fsum(terms)
    if not math.isfinite(want):
        same = (math.isnan(got) and math.isnan(want)) or got == want
        if not same:
            raise AssertionError(f"{what}: got {got}, {want} expected")
        return 0.0
    return _ratio(abs(float(got) - want), sum_bound(terms, calls) + calls * extra, what)


def check_k12_fwd(acc4, preds, gt, mask, lo, hi, calls=1, what="az_disp_loss_fwd"):
    """{accumulator: err / bound or the count compared}"""
    terms, count = k12_fwd(preds, gt, mask, lo, hi)
    _same_int(acc4[3], calls * count, f"{what} acc4[3] (count)")
    out = {f"acc4[{k}]": check_sum(acc4[k], terms[k], f"{what} acc4[{k}]", calls) for k in range(3)}
    out["count"] = calls * count
    return out


def check_grad(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        i = int(np.flatnonzero(bad.ravel())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from the restatement; the first at {i}: "
                             f"got {got.ravel()[i]!r}, {want.ravel()[i]!r} expected")
    return int(got.size)


def check_k12_bwd(grads, preds, gt, mask, lo, hi, gloss, count, what="az_disp_loss_bwd"):
    want = k12_bwd(preds, gt, mask, lo, hi, gloss, count)
    return {f"g_pred{3 - k}": check_grad(grads[k], want[k], f"{what} g_pred{3 - k}") for k in range(3)}


def check_k12_metrics(acc8, dg, zg, dp, zp, fb, mask, per_batch, calls=1, what="az_disp_metrics"):
    r = k12_metrics(dg, zg, dp, zp, fb, mask, per_batch)
    for slot, c, name in zip((1, 2, 4, 5, 6, 7), r["counts"], ("dd>1", "dd>2", "dz>2e-3", "dz>4e-3", "dz>8e-3", "count")):
        _same_int(acc8[slot], calls * c, f"{what} acc8[{slot}] (#{name})")
    out = {"acc8[0]": check_sum(acc8[0], r["dd"], f"{what} acc8[0]", calls),
           "acc8[3]": check_sum(acc8[3], r["mm64"], f"{what} acc8[3]", calls, extra=fsum(r["mm_tol"]))}
    out["counts"] = [calls * c for c in r["counts"]]
    return out


def check_k16_fwd(acc3, pred, gt, valid, max_flow, tsign, calls=1, what="az_seq_loss_fwd"):
    terms, count, bad = k16_fwd(pred, gt, valid, max_flow, tsign)
    _same_int(acc3[1], calls * count, f"{what} acc3[1] (count)")
    _same_int(acc3[2], calls * bad, f"{what} acc3[2] (non-finite predictions)")
    return {"acc3[0]": check_sum(acc3[0], terms, f"{what} acc3[0]", calls), "count": calls * count, "nonfinite": calls * bad}


def check_k16_bwd(grad, pred, gt, valid, max_flow, tsign, gloss, count, weight, what="az_seq_loss_bwd"):
    return {"g_pred": check_grad(grad, k16_bwd(pred, gt, valid, max_flow, tsign, gloss, count, weight), f"{what} g_pred")}


def check_absmax(arr, x, what="az_absmax", defect=None):
    got, want = amax_read(arr, defect), absmax_bits(x)
    if got != want:
        raise AssertionError(f"{what}: largest slot 0x{got:08x}, 0x{want:08x} expected")
    return want


def scalar_bound(value, propagated):
    """a float32 scalar made from exact fp64 accumulators by a short fp64 formula: one float32 rounding, the formula's own
    fp64 roundings (16 of them cover every formula here), and what it makes of the accumulators' bounds"""
    return (2.0 ** -24 + 16 * U) * abs(value) + propagated


def disp_loss_scalar(preds, gt, mask, lo, hi):
    """(loss in fp64 from the exact sums, bound for ops.disp_loss)"""
    terms, count = k12_fwd(preds, gt, mask, lo, hi)
    if count == 0:
        return math.nan, 0.0
    loss = sum(w * fsum(t) for w, t in zip(LOSS_WEIGHTS, terms)) / count
    return loss, scalar_bound(loss, sum(w * sum_bound(t) for w, t in zip(LOSS_WEIGHTS, terms)) / count)


def seq_loss_scalar(preds, gt, valid, max_flow, tsign, weights):
    loss = prop = 0.0
    for w, p in zip(weights, preds):
        terms, count, _ = k16_fwd(p, gt, valid, max_flow, tsign)
        if count == 0:
            return math.nan, 0.0
        loss += w * fsum(terms) / count
        prop += w * sum_bound(terms) / count
    return loss, scalar_bound(loss, prop)


METRIC_KEYS = ("epe", "bad1", "bad2", "depth_abs_err", "depth_err2", "depth_err4", "depth_err8")


def metrics_scalars(dg, zg, dp, zp, fb, mask, per_batch):
    """{key: (value, bound)} of compute_err_metric"""
    r = k12_metrics(dg, zg, dp, zp, fb, mask, per_batch)
    c = r["counts"]
    n = c[5]
    vals = (fsum(r["dd"]), c[0], c[1], fsum(r["mm64"]), c[2], c[3], c[4])
    props = (sum_bound(r["dd"]), 0.0, 0.0, sum_bound(r["mm64"]) + fsum(r["mm_tol"]), 0.0, 0.0, 0.0)
    return {k: (v / n, scalar_bound(v / n, p / n)) for k, v, p in zip(METRIC_KEYS, vals, props)}


# ---- inputs ------------------------------------------------------------------------------------------------------------
def special_positions(n, per_batch):
    """index 0 and n - 1, the last index of the first pass and the first of the second (both caps), both sides of every
    batch boundary"""
    pos = {0, n - 1}
    for cap in (RED_CAP, EW_CAP):
        pos |= {p for p in (cap * BLOCK - 1, cap * BLOCK) if p < n}
    for b in range(1, n // per_batch):
        pos |= {b * per_batch - 1, b * per_batch}
    return sorted(pos)


def _place(n, per_batch, kinds, anywhere):
    """[(index, kind)]: every kind once in a run from index 1 on (as far as the map reaches), then -- overriding -- a kind of
    `anywhere` (valid pixels) at every special position and, rotating on, at its free neighbours"""
    at = {1 + j: k for j, k in enumerate(kinds) if 1 + j < n}
    r = 0
    for p in special_positions(n, per_batch):
        for q in (p, p - 1, p + 1, p - 2, p + 2):
            if 0 <= q < n and (q == p or q not in at):
                at[q] = anywhere[r % len(anywhere)]
                r += 1
    return sorted(at.items())


def _shape(shape):
    b = shape[0]
    n = int(np.prod(shape))
    return b, n, n // b


def loss_case(shape, seed, nonfinite_preds=False):
    """K12 loss inputs: dict preds [p3, p2, p1], gt, mask (uint8), shape, n, per_batch.  Bulk: gt in [1.5, 100), predictions
    within 2.5 of it, mask bytes 0 / 1.  Special pixels: d exactly 0, exactly 1 and the float32 neighbours of 1 in each
    head; mask bytes 2 and 255; gt on lo / hi of RANGES and beside them, 0, -0, the smallest normal and the smallest
    subnormal (the neighbours of lo = 0), +inf, NaN, negative.  nonfinite_preds: NaN / +inf / -inf predictions on valid
    pixels (backward only: they make every forward sum NaN)"""
    b, n, pb = _shape(shape)
    rng = np.random.default_rng(seed)
    gt = rng.uniform(1.5, 100.0, n).astype(F32)
    preds = [(gt + rng.uniform(-2.5, 2.5, n).astype(F32)).astype(F32) for _ in range(3)]
    mask = (rng.uniform(0, 1, n) > 0.3).astype(np.uint8)
    # g = 1.5: p = 0.5 -> d = 1; 0.5 - 2^-23 -> 1 + 2^-23 = up(1); 0.5 + 2^-24 -> 1 - 2^-24 = down(1); 2.5 -> +1; 1.5 -> 0
    edge = (F32(0.5), F32(0.5) - F32(2.0 ** -23), F32(0.5) + F32(2.0 ** -24), F32(2.5), F32(2.5) + F32(2.0 ** -22), F32(1.5))
    others = (F32(1.75), F32(-1.5))
    valid_kinds = []
    for h in range(3):
        for e in edge:
            ps = [others[0], others[1]]
            ps.insert(h, e)
            valid_kinds.append((F32(1.5), ps, 1))
    valid_kinds += [(F32(7.25), [F32(7.0), F32(9.5), F32(7.25)], 2), (F32(40.0), [F32(40.5), F32(38.0), F32(41.0)], 255)]
    kinds = list(valid_kinds) + [(F32(7.25), [F32(7.0), F32(9.5), F32(7.25)], 0)]
    for g in (F32(1), down(1), up(1), F32(192), down(192), up(192), F32(0), F32(-0.0), F32(2.0 ** -126), F32(1e-45), F32(-3)):
        kinds.append((g, [g + F32(0.25), g - F32(3), g + F32(1)], 1))
    for g in (F32(np.inf), F32(np.nan)):
        kinds.append((g, [F32(5), F32(6), F32(7)], 0))
    if nonfinite_preds:
        for h in range(3):
            for bad in (F32(np.nan), F32(np.inf), F32(-np.inf)):
                ps = [F32(3), F32(4)]
                ps.insert(h, bad)
                kinds.append((F32(2.5), ps, 1))
    for i, (g, ps, m) in _place(n, pb, kinds, valid_kinds):
        gt[i], mask[i] = g, m
        for h in range(3):
            preds[h][i] = ps[h]
    return dict(preds=[p.reshape(shape) for p in preds], gt=gt.reshape(shape), mask=mask.reshape(shape), shape=shape, n=n,
                per_batch=pb, name=f"{'x'.join(map(str, shape))}")


def metrics_case(shape, seed):
    """az_disp_metrics inputs: dg, zg, dp, zp (the explicit depth_pred), fb [B], mask.  Special pixels: dd exactly 1 and 2
    and their float32 neighbours; with zp = 0 a dz exactly 2e-3f, 4e-3f, 8e-3f and their neighbours, and a millimetre error
    just under, at and over 100; mask bytes 2 and 255; on both sides of every batch boundary zg = fb[b] / dp exactly, so
    that any other fb puts the pixel over every depth threshold"""
    b, n, pb = _shape(shape)
    rng = np.random.default_rng(seed)
    fb = np.array([FB[i % 3] for i in range(b)], dtype=F32)
    dg = rng.uniform(4.0, 100.0, n).astype(F32)
    dp = np.maximum(dg + rng.uniform(-3.0, 3.0, n).astype(F32), F32(0.5)).astype(F32)
    zg = ((fb[np.arange(n) // pb] / dg) * rng.uniform(0.99, 1.01, n).astype(F32)).astype(F32)
    zp = (zg + rng.uniform(-0.012, 0.012, n).astype(F32)).astype(F32)
    mask = (rng.uniform(0, 1, n) > 0.3).astype(np.uint8)
    h = F32(0.5)
    dd_edges = ((F32(1.5), h), (F32(1.5) + F32(2.0 ** -23), h), (F32(1.5), h + F32(2.0 ** -24)),
                (F32(2.5), h), (F32(2.5) + F32(2.0 ** -22), h), (F32(2.5), h + F32(2.0 ** -23)))
    valid_kinds = [(a, F32(0.7), p, F32(0.7015), 1) for a, p in dd_edges]
    for c in THRESHOLDS[2:]:
        valid_kinds += [(F32(30), z, F32(29.5), F32(0), 1) for z in (c, down(c), up(c))]
    valid_kinds += [(F32(30), z, F32(29.5), F32(0), 1) for z in (down(0.1), F32(0.1), up(0.1), F32(0.0999), F32(0.1001))]
    valid_kinds += [(F32(12), F32(0.9), F32(11), F32(0.905), 2), (F32(13), F32(0.8), F32(15), F32(0.79), 255)]
    kinds = valid_kinds + [(F32(12), F32(0.9), F32(11), F32(0.905), 0)]
    for i, (a, z, p, q, m) in _place(n, pb, kinds, valid_kinds):
        dg[i], zg[i], dp[i], zp[i], mask[i] = a, z, p, q, m
    for bb in range(1, b):  # both sides of every batch boundary: the depth is right under this element's fb only
        for i in (bb * pb - 1, bb * pb):
            dp[i], mask[i] = F32(8 + bb), 1
            dg[i] = dp[i] + F32(0.25)
            zg[i] = fb[i // pb] / dp[i]
            zp[i] = zg[i]
    s = lambda a: a.reshape(shape)
    return dict(dg=s(dg), zg=s(zg), dp=s(dp), zp=s(zp), fb=fb, mask=s(mask), shape=shape, n=n, per_batch=pb, B=b,
                name=f"{'x'.join(map(str, shape))}")


MAX_FLOW = 700.0


def seq_case(shape, seed, n_pred=2, nonfinite_preds=False):
    """K16 inputs: preds (offsets from the target, so that one set serves both tsign: pred = tsign gt + off), gt, valid as
    float32 / uint8 / bool maps.  Special pixels: valid exactly 0.5 and its neighbours (bytes 1, 0, 2), 0 and 1 (bytes 0 and
    255); |gt| exactly max_flow and beside it, both signs; pred == target on a valid pixel; NaN / +inf / -inf predictions
    on pixels that valid or gt make invalid.  nonfinite_preds: the same on valid pixels (backward only)"""
    b, n, pb = _shape(shape)
    rng = np.random.default_rng(seed)
    gt = rng.uniform(-40.0, 820.0, n).astype(F32)
    offs = [rng.uniform(-3.0, 3.0, n).astype(F32) for _ in range(n_pred)]
    vf = (rng.uniform(0, 1, n) > 0.1).astype(F32)
    vu = vf.astype(np.uint8)
    mf = F32(MAX_FLOW)
    # (gt, offset or None = keep the bulk's, non-finite prediction or None, valid as float, valid as byte)
    valid_kinds = [(F32(33.5), F32(0), None, F32(1), 1), (F32(-20.25), F32(1.5), None, F32(0.5), 1),
                   (F32(100), F32(-2), None, up(0.5), 2), (F32(5), F32(0.75), None, F32(1), 255),
                   (down(mf), F32(0.5), None, F32(1), 1), (-down(mf), F32(0), None, F32(1), 1)]
    kinds = list(valid_kinds) + [(F32(50), F32(1), None, down(0.5), 0), (F32(50), F32(1), None, F32(0), 0)]
    kinds += [(g, F32(0.5), None, F32(1), 1) for g in (mf, -mf, up(mf), -up(mf))]
    kinds += [(F32(50), None, bad, F32(0), 0) for bad in (F32(np.nan), F32(np.inf), F32(-np.inf))]
    kinds += [(mf, None, F32(np.nan), F32(1), 1), (F32(900), None, F32(np.inf), F32(1), 255)]
    if nonfinite_preds:
        kinds += [(F32(50), None, bad, F32(1), 1) for bad in (F32(np.nan), F32(np.inf), F32(-np.inf))]
    bad_at = {}
    for i, (g, off, bad, f, u) in _place(n, pb, kinds, valid_kinds):
        gt[i], vf[i], vu[i] = g, f, u
        if off is not None:
            for o in offs:
                o[i] = off
        if bad is not None:
            bad_at[i] = bad
    s = lambda a: a.reshape(shape)

    def preds(tsign):
        out = []
        for o in offs:
            p = (F32(tsign) * gt + o).astype(F32)
            for i, bad in bad_at.items():
                p[i] = bad
            out.append(s(p))
        return out

    return dict(preds=preds, gt=s(gt), valid_f32=s(vf), valid_u8=s(vu), valid_bool=s(vu != 0), shape=shape, n=n, per_batch=pb,
                name=f"{'x'.join(map(str, shape))}")


def absmax_cases(n, seed=7100):
    """(name, x float32 [n]) for one length: the maximum at index 0, in the last full float4, in each position of the tail,
    at the first element of the second pass; a negative maximum; a subnormal as the only non-zero value; FLT_MAX beside an
    inf and a NaN; nothing finite; only -0.0"""
    rng = np.random.default_rng(seed + n % 1000)
    base = rng.uniform(-1.0, 1.0, n).astype(F32)
    base[np.abs(base) < 2.0 ** -100] = F32(0.25)
    n4 = n // ABSMAX_VEC
    spots = {"index 0": 0}
    if n4:
        spots["last full float4"] = 4 * (n4 - 1) + min(2, 4 * n4 - 1)
    for t in range(n & 3):
        spots[f"tail position {t}"] = 4 * n4 + t
    if n > ABSMAX_VEC * EW_CAP * BLOCK:
        spots["first element of the second pass"] = ABSMAX_VEC * EW_CAP * BLOCK
        spots["last element of the first pass"] = ABSMAX_VEC * EW_CAP * BLOCK - 1
    for name, i in spots.items():
        for sign, sname in ((1, ""), (-1, ", negative")):
            if sign < 0 and name not in ("index 0", "last full float4", f"tail position {(n & 3) - 1}"):
                continue
            x = base.copy()
            x[i] = F32(sign * 3.5)
            yield f"n={n}: maximum at {name}{sname}", x
    i = max(spots.values())
    x = np.zeros(n, dtype=F32)
    x[i] = F32(1e-40)
    yield f"n={n}: a subnormal the only non-zero value", x
    x = base.copy()
    x[i] = np.finfo(F32).max
    if n >= 3:
        a, b = [j for j in (0, n // 2, 1, n - 1) if j != i][:2]
        x[a], x[b] = F32(np.inf), F32(np.nan)
    yield f"n={n}: FLT_MAX beside an inf and a NaN", x
    x = np.full(n, np.nan, dtype=F32)
    x[::2] = F32(np.inf)
    x[::3] = F32(-np.inf)
    yield f"n={n}: nothing finite", x
    yield f"n={n}: only -0.0", np.full(n, -0.0, dtype=F32)


def map_cases(make, seed, **kw):
    """make(shape, seed, ...) for every shape of MAP_SHAPES, smallest maps first"""
    for k, shape in enumerate(MAP_SHAPES):
        yield make(shape, seed + k, **kw)


def loss_modes(case):
    """(name, mask, lo, hi): the explicit mask, then the in-kernel range mask under each of RANGES"""
    yield "mask", case["mask"], 0.0, math.inf
    for lo, hi in RANGES:
        yield f"range ({lo:g}, {hi:g})", None, lo, hi
