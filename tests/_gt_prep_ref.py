"""Restatements the K18 (az_gt_from_right) and K19 (az_error_img) kernels are compared with, bit for bit.  Test
infrastructure: CPU torch and numpy only, never the product path.

K18 is the operator chain itself, composed from CPU torch and the committed scatter oracle: F.interpolate(mode="nearest"),
.type(torch.int), oracle.warp_oracle.apply_disparity_cu_oracle, the two compares.  The chain has no defined answer for a
disparity that cannot be cast or that the reference's sign assertion refuses (<= -1, NaN, +-inf), nor a portable one for a
float beyond the int range; the entry point's contract says such a pixel lands nowhere, and so does a disparity >= W in
the chain.  They are therefore given the shift W before the cast -- the landing rule of the chain then drops them -- and
the first kind is counted.

K19 restates the two image functions in numpy on whole arrays, with the colour tables as data.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.warp_oracle import apply_disparity_cu_oracle


def resize_nearest(t, scale_factor=None, size=None):
    if size is not None:
        return F.interpolate(t, size, mode="nearest", recompute_scale_factor=False)
    return F.interpolate(t, scale_factor=scale_factor, mode="nearest", recompute_scale_factor=False)


def gt_from_right(disp_r, extra=None, keep=None, scale_factor=0.5, size=None, lo=0.0, hi=float("inf")):
    """CPU tensors in -> (disp_l, extra_l or None, keep_s or None, mask bool, stats int32 [2])"""
    kw = dict(size=size) if size is not None else dict(scale_factor=scale_factor)
    d = resize_nearest(disp_r, **kw)
    w = d.shape[-1]
    refused = ~torch.isfinite(d) | (d <= -1)
    nowhere = refused | (d >= w)
    shift = torch.where(nowhere, torch.full_like(d, float(w)), d).type(torch.int)
    src = d if extra is None else torch.cat([d, resize_nearest(extra, **kw)], 1)
    # the oracle moves values through numpy float32 arrays: bits are kept, NaN payloads included
    warped = apply_disparity_cu_oracle(src.contiguous(), shift.contiguous())
    disp_l = warped[:, :1].contiguous()
    extra_l = None if extra is None else warped[:, 1:].contiguous()
    keep_s = None if keep is None else resize_nearest(keep, **kw)
    mask = (disp_l < hi) * (disp_l > lo)
    stats = torch.tensor([int(refused.sum()), int(mask.sum())], dtype=torch.int32)
    return disp_l, extra_l, keep_s, mask, stats


# ---- K19 ----------------------------------------------------------------------------------------------------------
# the eleven classes: lower bounds (the upper bound of class i is the lower bound of class i + 1, the last one is open
# towards +inf, itself excluded) and the 0..255 colours, shared by both kinds
DISP_LOWER = [0, 0.00001, 0.1875 / 3.0, 0.375 / 3.0, 0.75 / 3.0, 1.5 / 3.0, 3 / 3.0, 6 / 3.0, 12 / 3.0, 24 / 3.0, 48 / 3.0]
DEPTH_LOWER = [0, 0.00001] + [2000.0 / 2 ** k for k in range(10, 1, -1)]
RGB = [(0, 0, 0), (49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144),
       (253, 174, 97), (244, 109, 67), (215, 48, 39), (165, 0, 38)]


def bounds(kind):
    """float32 [12]: lower bounds of the eleven classes, then +inf"""
    return np.array((DISP_LOWER if kind == "disp" else DEPTH_LOWER) + [np.inf], dtype=np.float32)


def colours():
    """float32 [11,3], each component divided by 255 in float32"""
    return np.array(RGB, dtype=np.float32) / np.float32(255.0)


def scaled_error(est, gt, kind, abs_thres, rel_thres=0.05):
    """float32 [B,H,W]: the quantity that is classified (before the mask)"""
    est, gt = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    with np.errstate(all="ignore"):
        e = np.abs(gt - est)
        if kind == "disp":
            return np.minimum(e / np.float32(abs_thres), (e / gt) / np.float32(rel_thres))
        return e / np.float32(abs_thres)


def classes(e, kind):
    """int [..]: the class of every element, -1 where none matches"""
    b = bounds(kind)
    cls = np.full(e.shape, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(11):
            cls[(e >= b[i]) & (e < b[i + 1])] = i
    return cls


def error_img(est, gt, mask, kind="disp", abs_thres=None, rel_thres=0.05):
    """numpy [B,H,W] x3 -> float32 [B,H,W,3]"""
    if abs_thres is None:
        abs_thres = 3.0 if kind == "disp" else 1.0
    mask = np.asarray(mask).astype(bool)
    cls = classes(scaled_error(est, gt, kind, abs_thres, rel_thres), kind)
    cls[~mask] = -1
    col = colours()
    img = np.zeros(cls.shape + (3,), dtype=np.float32)
    img[cls >= 0] = col[cls[cls >= 0]]
    for i in range(11):  # the legend; numpy slices clip it to the image
        img[:, :10, 20 * i:20 * i + 20, :] = col[i]
    return img


def on_the_bound(kind):
    """(est, gt) float32 [10] x2 whose scaled error IS the inner bound i + 1, exactly: est = 0 and gt = the bound (depth,
    abs_thres 1) or the float nearest 3 * bound whose third rounds to the bound (disp, abs_thres 3; every float32 has one
    because a third of the spacing of 3 b is below the spacing of b; the relative quotient is 20 and loses the minimum)"""
    b = bounds(kind)[1:11]
    if kind == "depth":
        return np.zeros(10, np.float32), b.copy()
    gt = np.empty(10, np.float32)
    for i, v in enumerate(b):
        g = np.float32(np.float32(3.0) * v)
        cands = [g, np.nextafter(g, np.float32(0)), np.nextafter(g, np.float32(np.inf))]
        gt[i] = next(c for c in cands if np.float32(c / np.float32(3.0)) == v)
    return np.zeros(10, np.float32), gt


# (est, gt): gt = 0 with an error, gt = 0 = est, est = gt, est = NaN, est = +inf, gt = NaN, a negative quotient
HOSTILE = [(2.0, 0.0), (0.0, 0.0), (33.0, 33.0), (np.nan, 40.0), (np.inf, 40.0), (40.0, np.nan), (-18.0, -20.0)]


def error_case(seed, b, h, w, kind="disp"):
    """est, gt, mask (float32, float32, bool; [b,h,w]) with every class populated, pixels exactly on the ten inner bounds,
    the hostile pixels, and the mask off on about a fifth of the image.
    Generator: rng = default_rng(seed); gt = uniform(5, 60) (the absolute quotient is the smaller one); every pixel draws
    a class uniformly and a scaled error inside it -- uniform(0, 0.9e-5) in class 0, log-uniform over the class with a
    margin of 2^0.05 at either end elsewhere (class 10: up to 8 times its lower bound) -- est = gt +- error * abs_thres;
    then the last 17 pixels of every image that has them take on_the_bound() and HOSTILE, under the mask."""
    rng = np.random.default_rng(seed)
    bd = bounds(kind).astype(np.float64)
    thres = 3.0 if kind == "disp" else 1.0
    gt = rng.uniform(5, 60, (b, h, w)).astype(np.float32)
    cls = rng.integers(0, 11, (b, h, w))
    lo, hi = np.log2(np.maximum(bd[cls], 2.0 ** -40)), np.log2(np.where(cls == 10, 8 * bd[10], bd[np.minimum(cls + 1, 10)]))
    e = 2.0 ** rng.uniform(lo + 0.05, hi - 0.05)
    e = np.where(cls == 0, rng.uniform(0, 0.9e-5, (b, h, w)), e)
    est = (gt + e * thres * rng.choice([-1.0, 1.0], (b, h, w))).astype(np.float32)
    mask = rng.random((b, h, w)) >= 0.2
    be, bg = on_the_bound(kind)
    special = list(zip(be, bg)) + HOSTILE
    fe, fg, fm = est.reshape(b, -1), gt.reshape(b, -1), mask.reshape(b, -1)
    if h * w >= len(special):
        for k, (pe, pg) in enumerate(special):
            fe[:, h * w - 1 - k], fg[:, h * w - 1 - k], fm[:, h * w - 1 - k] = pe, pg, True
    return est, gt, mask


def special_pixels(h, w):
    """flat indices of error_case's on-the-bound pixels (bound 1 .. 10) and of its HOSTILE pixels"""
    return [h * w - 1 - k for k in range(10)], [h * w - 11 - k for k in range(len(HOSTILE))]
