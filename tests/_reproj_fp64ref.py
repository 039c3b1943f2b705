"""fp64 references of the reprojection-loss kernels -- K7 az_warp_gather.hip (apply_disparity), K8 az_patch_reproj.hip
(get_reproj_error_patch and its Fold visualisation), K9 az_lcn.hip (local_contrast_norm) -- shared by
tests/test_reproj_error_model_cpu.py and tests/test_gpu_reproj_fp64.py (a helper module, not a conftest).

The recipe is the one of tests/_corr_fp64ref.py's lookup: the sampling coordinate is restated in numpy float32, one rounding per
operation, exactly as make_taps / pr_geom compute it (fp contract(off), no fast-math: bit for bit; the one fused operation is
the upper half of the linspace, linspace01 below), and everything after the coordinate is done in fp64 on the fp32 weights tx = ix - floor(ix), ty = iy - floor(iy).  That keeps the floor's discontinuity
out of the comparison; what is left is the rounding of a handful of fp32 operations, bounded below by COUNTING them.  U = 2^-24
is the unit roundoff of one fp32 operation (round to nearest; division and square root are correctly rounded).  Contraction of
a product and an add into an FMA only removes roundings, so the bounds hold either way.  SECOND = 1 + 2^-16 covers the products
of two roundings that a first-order count drops ((1 + U)^m - 1 <= m U (1 + m U) and m U < 2^-10 for every count below but the
k = 113 window, whose sums of zeros are exact and are not counted).

Every check is a ratio err / bound that must be <= 1.0 (ratio()); where the bound is zero the output must be exactly zero; a
non-finite output has ratio inf.  Nothing is excluded: every element of every output is checked.

K7 forward, out = nw (1-tx)(1-ty) + ne tx (1-ty) + sw (1-tx) ty + se tx ty:
    a term carries 1 - tx (1), 1 - ty (1), the weight product (1), the tap product (1); the sum of four terms, begun from
    zero, three adds: 7 roundings.                                                     |err| <= K7_FWD U mag,  K7_FWD = 7
    mag = sum |tap| weight.
K7 grad_disp, gix = sum_c g ((ne - nw) wy0 + (se - sw) wy1):
    ne - nw (1), wy0 = 1 - ty (1), the product (1), the inner add (1), times g (1): 5, and C - 1 adds over the channels.
                                                                                       |err| <= (C + K7_GD) U mag,  K7_GD = 4
    mag = sum_c |g| (|ne - nw| wy0 + |se - sw| wy1).
K7 grad_img, the scatter of g wx wy: 1 - tx (1), g wx (1), 1 - ty (1), times wy (1): 4 per contribution, and cnt - 1 float
    atomic adds in any order, each rounding a partial sum of magnitude <= mag.         |err| <= (cnt + K7_GI) U mag,  K7_GI = 3
K8 per tap, warped = wy0 (wx0 a0 + wx1 b0) + wy1 (wx0 a1 + wx1 b1), diff = warped - l:
    horizontal lerp: 1 - tx (1), wx0 a (1), wx1 b (1), the add (1): its first term carries 3, its second 2: 3;
    vertical lerp: 1 - ty (1), the product (1), the add (1): 3 more.                   |warped err| <= K8_W U wm,  K8_W = 6
    wm = the same bilinear form of |R0|.  The subtraction adds U |diff|: e = K8_W U wm + U |diff|.
    Forward: diff^2 (1) then a sequential fp32 sum of n = C ps^2 non-negative terms (n - 1 adds, granted as n):
                      |err| <= sum (2 |diff| e + e^2 + U diff^2) + n U sum diff^2
    Backward: dW = wy0 (dwx0 a0 + dwx1 b0) + wy1 (...), dwx = -+1 or 0: the inner add (1), 1 - ty (1), the product (1), the
    outer add (1): |dW err| <= K8_DW U dm, K8_DW = 4, dm the form of absolute values.  The term diff dW (1), summed over n
    terms (n), the per-channel results added into grad_disp by the tiled kernel (C), bwd_scale = (float)(gloss 2 / acc[1]) *
    sign: one rounding from fp64 (1), the product with it (1):
                      |err| <= |scale| (sum (e |dW| + K8_DW U |diff| dm + K8_DW U e dm + U |diff dW|) + (n + C + 2) U sum |diff dW|)
Fold, vis = sum_{u,v} warped_(u,v)(y - u, x - v): K8_W per term and ps^2 - 1 adds (granted as ps^2):
                      |err| <= (K8_W + ps^2) U sum wm
K9, n = k^2, nz = the number of non-zero pixels of the window (adding a zero is exact):
    mean = sum / n: nz - 1 adds (granted as nz) of partial sums <= sum |x|, the division (1):
                      em = (nz U sum |x|) / n + U |mean|
    d = x - mean (1): ed = em + U |d|;  ss = sum d^2: the square (1) and n - 1 adds (granted as n):
                      ess = sum (2 |d| ed + ed^2) + (n + 1) U sum (|d| + ed)^2
    var = ss / n (1), sd = sqrt(var) (1); |sqrt(a + t) - sqrt(a)| <= min(sqrt |t|, |t| / sqrt a):
                      ev = ess / n + U var,   esd = min(sqrt ev, ev / sd) + U (sd + sqrt ev)
    normed = (x - mean) / (sd + eps): numerator ed, denominator eden = esd + U (sd + eps + esd), the quotient (1):
                      |err| <= ed / (den - eden) + |d| eden / (den (den - eden)) + U (|q| + that)
    and no bound at all (inf) where eden >= den: there the kernel's own std is not known to one part in one.

Largest ratio err / bound measured on an MI355X over every case of tests/test_gpu_reproj_fp64.py (test_zz_largest_ratios), at
default switches and, for K8, under AZ_PATCH_TILED=0 (tests/test_gpu_switches.py):
    kernel, route                            check                 largest ratio
    K7  one launch pass                      forward / grad_disp / grad_img      0.33 / 0.44 / 0.54
    K7  grid-stride (1025 x 1024)            forward / grad_disp / grad_img      0.48 / 0.64 / 0.54
    K7  through autograd                     forward / grad_disp / grad_img      0.15 / 0.14 / 0.32
    K8  tiled PSM 5, one-row bands           per pixel / full / grad_disp        0.20 / 0.07 / 0.11
    K8  tiled PSM 5, multi-row bands         per pixel / full / grad_disp        0.37 / 0.00 / 0.40   (ps = 1 and 3: few terms)
    K8  tiled PSM 11, one-row bands          per pixel / full / grad_disp        0.09 / 0.02 / 0.07
    K8  tiled PSM 15, one-row bands          per pixel / full / grad_disp        0.06 / 0.01 / 0.05   (W = 1244, 1245 among them)
    K8  tiled PSM 15, multi-row bands        per pixel / full / grad_disp        0.04 / 0.00 / 0.04
    K8  per-pixel by width (W = 1245, 1246)  per pixel / full / grad_disp        0.02 / 0.00 / 0.02
    K8  per-pixel, AZ_PATCH_TILED=0          per pixel / full / grad_disp        0.37 / 0.10 / 0.40   (every K8 case, 1025 x 1024 too)
    K8  Fold                                 vis                                 0.16
    K8  through autograd                     loss / grad_disp / vis              0.01 / 0.02 / 0.06   (0.02 / 0.04 / 0.06 per-pixel)
    K9  full 16 x 16 tiles                   std / normed                        0.10 / 0.35
    K9  partial tiles                        std / normed                        0.16 / 0.20
The bounds are worst cases: a sum of n terms is granted n U times its magnitude, so the ratios fall as ps and k grow; what the
checks still reject at those sizes is listed, mutant by mutant, in tests/test_reproj_error_model_cpu.py.  Before the restated
linspace took its upper half as one fused multiply-add (linspace01 below) the same run stood at ratios of 1.1 to 320 and at
non-zero outputs where the reference had every tap outside, at sizes from 10 up whose step 1 / (n - 1) is inexact: the
restatement was the side that differed from torch's linspace, not the kernels.
"""
import functools

import numpy as np

from tests._weights import seeded

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16
K7_FWD, K7_GD, K7_GI = 7.0, 4.0, 3.0
K8_W, K8_DW = 6.0, 4.0
F32 = np.float32


def ratio(got, ref, bound):
    """the largest err / bound over every element; exact zero demanded where the bound is zero; inf for a non-finite output"""
    got, ref, bound = (np.asarray(t, dtype=np.float64) for t in (got, ref, bound))
    got, ref, bound = np.broadcast_arrays(got, ref, bound)
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(got == 0, 0.0, np.inf))
        r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


# ---- the coordinate -------------------------------------------------------------------------------------------------------------
def linspace01(n):
    """torch.linspace(0, 1, n) as linspace01 of the kernels forms it in fp32: step i in the lower half, and in the upper half
    the ONE fused multiply-add fma(-step, n - 1 - i, 1) -- what torch's CPU kernel computes.  The product of a 24-bit step and
    an integer below 2^20 and its difference from 1 are exact in fp64, so rounding the fp64 value once is the fma."""
    assert 2 <= n < 2 ** 20
    i = np.arange(n)
    step = F32(1.0) / F32(n - 1)
    lo = step * i.astype(np.float32)
    assert step.dtype == lo.dtype == np.float32
    hi = (1.0 - np.float64(step) * (n - 1 - i).astype(np.float64)).astype(np.float32)
    return np.where(i < n // 2, lo, hi)


def unnormalise(g, size):
    """2 g - 1, then ((n + 1) size - 1) / 2, one fp32 rounding per operation"""
    n = F32(2.0) * g
    assert n.dtype == np.float32
    n = n - F32(1.0)
    assert n.dtype == np.float32
    p = n + F32(1.0)
    assert p.dtype == np.float32
    p = p * F32(size)
    assert p.dtype == np.float32
    p = p - F32(1.0)
    assert p.dtype == np.float32
    p = p / F32(2.0)
    assert p.dtype == np.float32
    return p


def pixel_coords(disp, H, W):
    """(ix [..., H, W], iy [H]) in fp32 as make_taps / pr_geom compute them; disp [..., H, W] float32"""
    disp = np.asarray(disp)
    assert disp.dtype == np.float32 and disp.shape[-2:] == (H, W)
    with np.errstate(all="ignore"):
        q = disp / F32(W)
        assert q.dtype == np.float32
        gx = linspace01(W) + q
        assert gx.dtype == np.float32
        return unnormalise(gx, W), unnormalise(linspace01(H), H)


def taps(p, size):
    """(the north-west tap, clamped to [-2, size + 1] before the int conversion as the kernels clamp it (fmaxf / fminf drop a
    NaN); the fp32 weight p - floor(p) as fp64 -- exact in fp32)"""
    with np.errstate(all="ignore"):
        fl = np.floor(p)
        assert fl.dtype == np.float32
        c = np.fmin(np.fmax(fl, F32(-2.0)), F32(size) + F32(1.0))
        assert c.dtype == np.float32
        t = p - fl
        assert t.dtype == np.float32
    return c.astype(np.int64), t.astype(np.float64)


def coords(disp, H, W):
    """x0, y0, tx, ty, vx0, vx1, vy0, vy1, each broadcast to disp's shape"""
    ix, iy = pixel_coords(disp, H, W)
    x0, tx = taps(ix, W)
    y0, ty = taps(iy, H)
    y0, ty = (np.broadcast_to(t[:, None], x0.shape) for t in (y0, ty))
    return x0, y0, tx, ty, (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W), (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)


def _pad(img, p, dtype=np.float64):
    return np.pad(np.asarray(img, dtype=dtype), ((0, 0), (0, 0), (p, p), (p, p)))


# ---- K7 -------------------------------------------------------------------------------------------------------------------------
def _corners(img, disp):
    """the four taps [B,C,H,W] (zero where outside) and the geometry"""
    img = np.asarray(img, dtype=np.float64)
    B, C, H, W = img.shape
    x0, y0, tx, ty, vx0, vx1, vy0, vy1 = coords(np.asarray(disp).reshape(B, H, W), H, W)
    P = _pad(img, 3)
    bb = np.arange(B)[:, None, None, None]
    cc = np.arange(C)[None, :, None, None]
    g = lambda a, b: P[bb, cc, (y0 + a + 3)[:, None], (x0 + b + 3)[:, None]]
    val = lambda vy, vx: (vy & vx)[:, None]
    nw, ne = np.where(val(vy0, vx0), g(0, 0), 0.0), np.where(val(vy0, vx1), g(0, 1), 0.0)
    sw, se = np.where(val(vy1, vx0), g(1, 0), 0.0), np.where(val(vy1, vx1), g(1, 1), 0.0)
    return (nw, ne, sw, se), (x0, y0, tx[:, None], ty[:, None], vx0, vx1, vy0, vy1)


def warp_fwd(img, disp):
    """(ref [B,C,H,W], mag = sum |tap| weight)"""
    (nw, ne, sw, se), (_, _, tx, ty, *_) = _corners(img, disp)
    w = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
    ref = sum(t * k for t, k in zip((nw, ne, sw, se), w))
    mag = sum(np.abs(t) * k for t, k in zip((nw, ne, sw, se), w))
    return ref, mag


def warp_fwd_bound(mag):
    return K7_FWD * U * SECOND * mag


def warp_bwd(gout, img, disp):
    """((gdisp_ref [B,H,W], gdisp_mag), (gimg_ref [B,C,H,W], gimg_mag, gimg_cnt))"""
    g = np.asarray(gout, dtype=np.float64)
    B, C, H, W = g.shape
    (nw, ne, sw, se), (x0, y0, tx, ty, vx0, vx1, vy0, vy1) = _corners(img, disp)
    gd = (g * ((ne - nw) * (1 - ty) + (se - sw) * ty)).sum(1)
    gd_mag = (np.abs(g) * (np.abs(ne - nw) * (1 - ty) + np.abs(se - sw) * ty)).sum(1)
    ref = np.zeros((B, C, H + 6, W + 6))
    mag, cnt = np.zeros_like(ref), np.zeros_like(ref)
    bb = np.broadcast_to(np.arange(B)[:, None, None], x0.shape)
    tx, ty = tx[:, 0], ty[:, 0]
    for a, b, vy, vx, w in ((0, 0, vy0, vx0, (1 - tx) * (1 - ty)), (0, 1, vy0, vx1, tx * (1 - ty)),
                            (1, 0, vy1, vx0, (1 - tx) * ty), (1, 1, vy1, vx1, tx * ty)):
        ok = vy & vx
        for c in range(C):
            con = (g[:, c] * w)[ok]
            at = (bb[ok], c, (y0 + a + 3)[ok], (x0 + b + 3)[ok])
            np.add.at(ref, at, con)
            np.add.at(mag, at, np.abs(con))
            np.add.at(cnt, at, 1.0)
    crop = lambda t: t[:, :, 3:-3, 3:-3]
    return (gd, gd_mag), (crop(ref), crop(mag), crop(cnt))


def warp_gdisp_bound(mag, C):
    return (C + K7_GD) * U * SECOND * mag


def warp_gimg_bound(mag, cnt):
    return (cnt + K7_GI) * U * SECOND * mag


# ---- K8 -------------------------------------------------------------------------------------------------------------------------
def all_pixels(B, H, W):
    b, i, j = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    return b.ravel(), i.ravel(), j.ravel()


def patch_pixel(L, R, disp, ps, sign, pix=None):
    """per pixel of `pix` = (b, i, j) index arrays (every pixel, in C order, if None):
        ssd, fwd_bound     the fp64 sum over (c, u, v) of diff^2 and the bound of the kernel's fp32 value of it
        g, g_abs, g_bound  sum diff dW, sum |diff dW| and the bound of the fp32 value of sum diff dW times a |scale| of one
                           (K8 backward: times |scale|, see patch_grad)
        sum_abs_diff, sum_wm   the bound's ingredients: sum |diff| and the bilinear magnitude of |R0|, summed over the taps
    R0 and L are zero-padded by ps / 2 (Unfold's padding); a corner weight is zero when the corner (y0 + a, x0 + b) itself is
    outside the image (grid_sample's padding), and d wx / d ix = -+1 under the same validity."""
    L64 = np.asarray(L, dtype=np.float64)
    B, C, H, W = L64.shape
    r = ps // 2
    d = (F32(sign) * np.asarray(disp, dtype=np.float32).reshape(B, H, W)).astype(np.float32)
    bb, ii, jj = all_pixels(B, H, W) if pix is None else pix
    x0, y0, tx, ty, vx0, vx1, vy0, vy1 = (t[bb, ii, jj] for t in coords(d, H, W))
    wx0, wx1, wy0, wy1 = np.where(vx0, 1 - tx, 0.0), np.where(vx1, tx, 0.0), np.where(vy0, 1 - ty, 0.0), np.where(vy1, ty, 0.0)
    dx0, dx1 = np.where(vx0, -1.0, 0.0), np.where(vx1, 1.0, 0.0)
    P = r + 3
    Rp, Lp = _pad(R, P), _pad(L64, r)
    z = np.zeros(len(bb))
    out = {k: z.copy() for k in ("ssd", "fb", "g", "g_abs", "gb", "sum_abs_diff", "sum_wm")}
    for c in range(C):
        for u in range(-r, r + 1):
            for v in range(-r, r + 1):
                a0, b0 = Rp[bb, c, y0 + u + P, x0 + v + P], Rp[bb, c, y0 + u + P, x0 + v + 1 + P]
                a1, b1 = Rp[bb, c, y0 + u + 1 + P, x0 + v + P], Rp[bb, c, y0 + u + 1 + P, x0 + v + 1 + P]
                warped = wy0 * (wx0 * a0 + wx1 * b0) + wy1 * (wx0 * a1 + wx1 * b1)
                wm = wy0 * (wx0 * np.abs(a0) + wx1 * np.abs(b0)) + wy1 * (wx0 * np.abs(a1) + wx1 * np.abs(b1))
                diff = warped - Lp[bb, c, ii + u + r, jj + v + r]
                ad = np.abs(diff)
                e = K8_W * U * wm + U * ad
                out["ssd"] += diff * diff
                out["fb"] += 2 * ad * e + e * e + U * diff * diff
                dW = wy0 * (dx0 * a0 + dx1 * b0) + wy1 * (dx0 * a1 + dx1 * b1)
                dm = wy0 * (np.abs(dx0 * a0) + np.abs(dx1 * b0)) + wy1 * (np.abs(dx0 * a1) + np.abs(dx1 * b1))
                out["g"] += diff * dW
                out["g_abs"] += np.abs(diff * dW)
                out["gb"] += e * np.abs(dW) + K8_DW * U * ad * dm + K8_DW * U * e * dm + U * np.abs(diff * dW)
                out["sum_abs_diff"] += ad
                out["sum_wm"] += wm
    n = C * ps * ps
    out["fwd_bound"] = SECOND * (out.pop("fb") + n * U * out["ssd"])
    out["g_bound"] = SECOND * (out.pop("gb") + (n + C + 2) * U * out["g_abs"])
    return out


def patch_grad(pp, gloss, count, C, ps, sign):
    """(ref, bound) of grad_disp at the pixels of pp = patch_pixel(...): gloss 2 / (count C ps^2) sign sum diff dW"""
    scale = float(gloss) * 2.0 / (count * C * ps * ps) * sign
    return pp["g"] * scale, pp["g_bound"] * abs(scale)


def patch_vis(R, disp, ps, sign):
    """the Fold: (vis [B,C,H,W] = sum_{u,v} warped_(u,v)(y - u, x - v), its magnitude); bound (K8_W + ps^2) U mag"""
    R64 = np.asarray(R, dtype=np.float64)
    B, C, H, W = R64.shape
    r = ps // 2
    d = (F32(sign) * np.asarray(disp, dtype=np.float32).reshape(B, H, W)).astype(np.float32)
    x0, y0, tx, ty, vx0, vx1, vy0, vy1 = (t[:, None] for t in coords(d, H, W))
    wx0, wx1, wy0, wy1 = np.where(vx0, 1 - tx, 0.0), np.where(vx1, tx, 0.0), np.where(vy0, 1 - ty, 0.0), np.where(vy1, ty, 0.0)
    P = r + 3
    Rp, aRp = _pad(R64, P), np.abs(_pad(R64, P))
    bb = np.arange(B)[:, None, None, None]
    cc = np.arange(C)[None, :, None, None]
    vis, mag = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    for u in range(-r, r + 1):
        for v in range(-r, r + 1):
            f = lambda S: (wy0 * (wx0 * S[bb, cc, y0 + u + P, x0 + v + P] + wx1 * S[bb, cc, y0 + u + P, x0 + v + 1 + P]) +
                           wy1 * (wx0 * S[bb, cc, y0 + u + 1 + P, x0 + v + P] + wx1 * S[bb, cc, y0 + u + 1 + P, x0 + v + 1 + P]))
            ys, xs = slice(max(u, 0), H + min(u, 0)), slice(max(v, 0), W + min(v, 0))      # y = i + u, x = j + v inside
            yi, xi = slice(max(-u, 0), H + min(-u, 0)), slice(max(-v, 0), W + min(-v, 0))
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            vis[:, :, ys, xs] += f(Rp)[:, :, yi, xi]
            mag[:, :, ys, xs] += f(aRp)[:, :, yi, xi]
    return vis, mag


def vis_bound(mag, ps):
    return (K8_W + ps * ps) * U * SECOND * mag


# ---- K9 -------------------------------------------------------------------------------------------------------------------------
def lcn(img, k, eps):
    """img [B,H,W] -> dict: mean, sd (two-pass population std), normed, the bounds sd_bound and normed_bound, and what they are
    made of: sum_abs (sum |x| of the window), sum_d2, inv_den = 1 / (sd + eps); eps is the fp32 value the kernel receives"""
    x = np.asarray(img, dtype=np.float64)
    B, H, W = x.shape
    r, n = k // 2, float(k * k)
    eps = float(F32(eps))
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (r, r), (r, r))), (k, k), axis=(1, 2))   # [B,H,W,k,k]
    mean = win.sum((-1, -2)) / n
    d = win - mean[..., None, None]
    sum_d2 = (d * d).sum((-1, -2))
    sd = np.sqrt(sum_d2 / n)
    den = sd + eps
    dc = x - mean
    normed = dc / den
    sum_abs, nz = np.abs(win).sum((-1, -2)), (win != 0).sum((-1, -2))
    em = nz * U * sum_abs / n + U * np.abs(mean)
    ed = em[..., None, None] + U * np.abs(d)
    ess = (2 * np.abs(d) * ed + ed * ed).sum((-1, -2)) + (n + 1) * U * ((np.abs(d) + ed) ** 2).sum((-1, -2))
    ev = ess / n + U * sum_d2 / n
    with np.errstate(all="ignore"):
        esd = np.minimum(np.sqrt(ev), np.where(sd > 0, ev / np.where(sd > 0, sd, 1.0), np.inf)) + U * (sd + np.sqrt(ev))
        eden = esd + U * (den + esd)
        edc = em + U * np.abs(dc)
        first = edc / (den - eden) + np.abs(dc) * eden / (den * (den - eden))
        nb = np.where(eden < den, first + U * (np.abs(normed) + first), np.inf)
    return {"mean": mean, "sd": sd, "normed": normed, "sd_bound": SECOND * esd, "normed_bound": SECOND * nb,
            "sum_abs": sum_abs, "sum_d2": sum_d2, "inv_den": 1.0 / den}


# ---- the dispatch of az_patch_reproj.hip, restated once -------------------------------------------------------------------------
PR_K = {"fwd": 4, "bwd": 2}
LDS_LIMIT = 158 * 1024
GRID_THREADS = 256 * 16 * 256   # az_grid_for's cap: beyond it a thread walks more than one element


def pr_band_rows(B, H, W, ps, pr_k):
    """pr_band_rows of az_patch_reproj.hip: (rows per band or 0, the dynamic LDS bytes of that launch)"""
    r = ps // 2
    RS, LS = W + 2 * (r + 3), W + 2 * r + pr_k
    best, best_eff, lds = 0, 0.0, 0
    for tr in range(1, min(32, H) + 1):
        need = ((tr + 2 * r + 2) * RS + (tr + 2 * r) * LS) * 4
        if need > LDS_LIMIT:
            break
        blocks = B * ((H + tr - 1) // tr)
        rounds = (blocks + 255) // 256
        eff = float(B * H) / float(rounds * 256) / (tr + 0.15 * (2 * tr + 4 * r + 2))
        if eff > best_eff:
            best_eff, best, lds = eff, tr, need
    return best, lds


def psm(ps):
    return 5 if ps <= 5 else 11 if ps <= 11 else 15


def k8_route(shape, which, tiled_enabled=True):
    """the launch of `which` in ("fwd", "bwd") for shape = (B, C, H, W, ps): dict(tiled, psm, k, tr, nbands, last, lds)"""
    B, C, H, W, ps = shape
    k = PR_K[which]
    tr, lds = pr_band_rows(B, H, W, ps, k)
    tiled = bool(tiled_enabled) and tr > 0
    if not tiled:
        return dict(tiled=False, psm=None, k=1, tr=0, nbands=0, last=0, lds=0)
    nbands = (H + tr - 1) // tr
    return dict(tiled=True, psm=psm(ps), k=k, tr=tr, nbands=nbands, last=H - (nbands - 1) * tr, lds=lds)


def k8_chain(shape, tiled_enabled=True):
    """the number of fp32 adds on the longest chain of the forward's partial sums: a thread's own items, then six shuffle steps"""
    B, C, H, W, ps = shape
    rt = k8_route(shape, "fwd", tiled_enabled)
    if rt["tiled"]:
        groups = (W + 3) // 4
        return C * 4 * (-(-rt["tr"] * groups // 512)) + 6
    total = B * H * W
    threads = min(-(-total // 256) * 256, GRID_THREADS)
    return -(-total // threads) + 6


def k8_route_features(shapes, tiled_enabled=True):
    """the branches of K8's dispatch that a list of shapes reaches"""
    feats = set()
    for s in shapes:
        B, C, H, W, ps = s
        f, b = k8_route(s, "fwd", tiled_enabled), k8_route(s, "bwd", tiled_enabled)
        for rt in (f, b):
            if rt["tiled"]:
                feats.add(f"PSM {rt['psm']} " + ("ps == PSM" if ps == rt["psm"] else "ps < PSM"))
                feats.add("tr == 1" if rt["tr"] == 1 else "tr >= 2 full last band" if rt["last"] == rt["tr"] else
                          "tr >= 2 partial last band")
                if pr_band_rows(B, H, W + 1, ps, rt["k"])[0] == 0:
                    feats.add("tiled at the last width that fits")
            else:
                feats.add("per-pixel by width" if tiled_enabled else "per-pixel by switch")
        if f["tiled"] != b["tiled"]:
            feats.add("forward and backward on different routes")
        feats |= {n for n, on in (("W % 4 != 0", W % 4 != 0), ("W % 2 != 0", W % 2 != 0), ("C > 1", C > 1),
                                  ("window larger than the image", ps > H and ps > W)) if on}
    return feats


K8_WANT = {f"PSM {p} {q}" for p in (5, 11, 15) for q in ("ps < PSM", "ps == PSM")} | {
    "tr == 1", "tr >= 2 full last band", "tr >= 2 partial last band", "W % 4 != 0", "W % 2 != 0", "C > 1",
    "window larger than the image", "tiled at the last width that fits", "per-pixel by width",
    "forward and backward on different routes"}


# ---- the cases, shared by the CPU model and the GPU sweep -----------------------------------------------------------------------
K7_SHAPES = [(1, 1, 2, 2), (2, 3, 5, 8), (1, 2, 33, 65), (1, 121, 4, 6), (1, 1, 1025, 1024)]
K8_SMALL = [(1, 1, 2, 2, 1), (1, 1, 5, 9, 3), (2, 2, 6, 7, 5), (1, 1, 9, 13, 7), (1, 1, 8, 10, 9), (1, 1, 12, 14, 11),
            (1, 1, 16, 18, 13), (1, 1, 16, 17, 15), (1, 1, 3, 4, 15)]
K8_BANDS = [(3, 1, 87, 7, 3), (1, 1, 700, 6, 15), (3, 1, 300, 5, 13), (1, 1, 1025, 3, 1)]
K8_LDS = [(1, 1, 2, 1244, 15), (1, 1, 2, 1245, 15), (1, 1, 2, 1246, 15)]
K8_SHAPES = K8_SMALL + K8_BANDS + K8_LDS
K8_STRIDE_CASE = (1, 1, 1025, 1024, 1)   # tiled by default, the per-pixel kernel's grid-stride loop under AZ_PATCH_TILED=0
K9_SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 9), (2, 1, 16, 16, 3), (1, 3, 17, 33, 5), (1, 1, 31, 15, 9), (1, 1, 20, 40, 11),
             (1, 1, 5, 7, 113)]
K9_SETS = ("seeded", "flat", "constant", "offset", "tiny")
SETS = ("seeded", "binary", "zero")
CLASSES = ("inside", "on a column", "x0 = -1", "x0 = W - 1", "x0 = W", "only the right tap", "only the left tap", "both out",
           "clamped low", "clamped high")


def _seed(shape, extra):
    return 9100 + 131 * extra + sum(p * s for p, s in zip((7, 3, 5, 11, 13), shape))


def image(shape4, which, seed):
    """[B,C,H,W] float32: seeded normal values, or 0/1 at density 0.25 as the IR patterns are"""
    rng = np.random.default_rng(seed)
    if which == "binary":
        return (rng.uniform(size=shape4) < 0.25).astype(np.float32)
    return rng.standard_normal(shape4).astype(np.float32)


def classes_of(disp, H, W):
    """which classes of sampling position a field holds, read from the restated coordinates"""
    ix, _ = pixel_coords(disp, H, W)
    x0, _, tx, _, vx0, vx1, _, _ = coords(disp, H, W)
    with np.errstate(all="ignore"):
        lo, hi = np.floor(ix) < -2, np.floor(ix) > W + 1
    return {n for n, m in zip(CLASSES, (vx0 & vx1 & (tx > 0), vx0 & (tx == 0), x0 == -1, x0 == W - 1, x0 == W, ~vx0 & vx1,
                                        vx0 & ~vx1, ~vx0 & ~vx1, lo, hi)) if m.any()}


@functools.lru_cache(maxsize=None)
def disparity(B, H, W, seed):
    """[B,H,W] float32 holding every class of sampling position in every row that is long enough (in a rotated order), as
    lookup_coords of the correlation test builds its coordinates: for the column j of a pixel, the disparity that puts ix at
    the wanted place; `on a column` is searched among the neighbouring floats until tx == 0"""
    f = F32
    targets = [f(0.5 * W - 0.25), f(0.0), f(W - 1.0), f(-1.0), f(W), f(-0.5), f(W - 0.5), f(W + 0.25), f(1e6), f(-1e6), f(-1.5),
               np.nextafter(f(0.0), f(-np.inf)), np.nextafter(f(0.0), f(np.inf)), np.nextafter(f(-1.0), f(-np.inf)),
               np.nextafter(f(-1.0), f(np.inf)), np.nextafter(f(W - 1.0), f(-np.inf)), np.nextafter(f(W - 1.0), f(np.inf)),
               np.nextafter(f(W), f(-np.inf)), np.nextafter(f(W), f(np.inf)), f(W + 5.0), f(-(W + 5.0)), f(1.0),
               f(W - 2.0), f(0.25), f(W - 1.25)]
    rng = np.random.default_rng(seed)
    n = B * H * W
    t = np.empty(n, dtype=np.float32)
    pos = np.arange(n)
    row = pos // W
    sel = ((pos + 5 * row) if W >= len(targets) + 8 else pos) % (len(targets) + 8)   # a short row holds a part of the cycle
    t[:] = rng.uniform(-3.0, W + 2.0, size=n).astype(np.float32)
    for k, v in enumerate(targets):
        t[sel == k] = v
    j = (pos % W).astype(np.float64)
    base = j * W / (W - 1) - 0.5
    d = (t.astype(np.float64) - base).astype(np.float32).reshape(B, H, W)
    want_int = np.isin(sel, (1, 2, 3, 4, 21)).reshape(B, H, W)
    best = d.copy()
    found = np.zeros(d.shape, dtype=bool)
    up, dn = d.copy(), d.copy()
    for step in range(9):
        for cand in ((d,) if step == 0 else (up, dn)):
            _, _, tx, *_ = coords(cand, H, W)
            hit = want_int & ~found & (tx == 0)
            best[hit] = cand[hit]
            found |= hit
        up, dn = np.nextafter(up, f(np.inf)), np.nextafter(dn, f(-np.inf))
    return best


def k7_inputs(shape, which):
    B, C, H, W = shape
    s = _seed(shape + (0,), SETS.index(which))
    img = np.zeros(shape, dtype=np.float32) if which == "zero" else image(shape, which, s)
    return img, disparity(B, H, W, s + 1), image(shape, "seeded", s + 2)     # img, disp, grad_out


def k8_inputs(shape, which):
    B, C, H, W, ps = shape
    s = _seed(shape, 10 + SETS.index(which))
    L = image((B, C, H, W), "binary" if which == "binary" else "seeded", s)
    R = np.zeros((B, C, H, W), dtype=np.float32) if which == "zero" else image((B, C, H, W), which, s + 1)
    return L, R, disparity(B, H, W, s + 2)


def k8_mask(shape, kind):
    B, C, H, W, ps = shape
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((B, H, W), dtype=np.uint8)
    m = (np.random.default_rng(_seed(shape, 20)).uniform(size=(B, H, W)) < 0.8).astype(np.uint8)
    m.flat[0] = 0          # at least one masked pixel, at least one live one
    m.flat[-1] = 1
    return m


def k8_sample(shape, tiled_enabled=True):
    """the pixels whose forward value is checked one launch each: all of a small shape; of a larger one every pixel (the first
    and last PR_K + 1 columns where the row is long) of the first and last row of the first, a middle and the last band, and
    64 seeded pixels"""
    B, C, H, W, ps = shape
    if B * H * W <= 320:
        return all_pixels(B, H, W)
    rt = k8_route(shape, "fwd", tiled_enabled)
    tr = max(rt["tr"], 1)
    nb = (H + tr - 1) // tr
    rows = sorted({min(H - 1, b * tr + o) for b in (0, nb // 2, nb - 1) for o in (0, tr - 1)} | {H - 1})
    cols = list(range(W)) if W <= 32 else list(range(5)) + list(range(W - 5, W))
    px = {(B - 1 if i else 0, y, x) for i, y in enumerate(rows) for x in cols}
    rng = np.random.default_rng(_seed(shape, 30))
    px |= {(int(rng.integers(B)), int(rng.integers(H)), int(rng.integers(W))) for _ in range(64)}
    b, i, j = (np.array(t) for t in zip(*sorted(px)))
    return b, i, j


def k9_input(shape, which):
    """[B,C,H,W] float32; channels past the first hold NaN and must never be read"""
    B, C, H, W, k = shape
    s = _seed(shape, 40 + K9_SETS.index(which))
    x = seeded((B, 1, H, W), s).numpy()
    if which == "flat":        # a block of one short-mantissa value (every partial sum of it is exact) in a seeded image
        x[:, :, : (H + 1) // 2 + k // 2, : (W + 1) // 2 + k // 2] = 0.75
    elif which == "constant":
        x[:] = 0.75
    elif which == "offset":
        x = (F32(1000.0) + F32(1e-3) * x).astype(np.float32)
    elif which == "tiny":
        x = (F32(1e-6) * x).astype(np.float32)
    full = np.full((B, C, H, W), np.nan, dtype=np.float32)
    full[:, :1] = x
    return full


def k9_flat_inside(shape):
    """[H,W] bool: the pixels of the `flat` set whose whole window lies inside the flat block"""
    B, C, H, W, k = shape
    r = k // 2
    hb, wb = min(H, (H + 1) // 2 + r), min(W, (W + 1) // 2 + r)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (y - r >= 0) & (y + r < hb) & (x - r >= 0) & (x + r < wb)


# ---- the checks of K8, one place for the CPU model and the GPU sweep ------------------------------------------------------------
def k8_check_pixels(acc, pp, C, ps):
    """acc [N,2] of N launches whose mask selects one pixel each: ratio of acc[:,0] against the pixel's bound; acc[:,1] exact"""
    acc = np.asarray(acc, dtype=np.float64)
    if not np.array_equal(acc[:, 1], np.full(len(acc), float(C * ps * ps))):
        return np.inf
    return ratio(acc[:, 0], pp["ssd"], pp["fwd_bound"])


def k8_check_full(acc, pp, mask, shape, tiled_enabled=True):
    """acc [2] of one launch over the whole image, pp = patch_pixel over every pixel: acc[1] == count C ps^2 exactly, acc[0]
    within the sum of the pixels' bounds plus the fp32 accumulation of the partial sums (non-negative terms: magnitude sum ref)"""
    B, C, H, W, ps = shape
    live = np.ones(B * H * W, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if float(acc[1]) != float(live.sum()) * C * ps * ps:
        return np.inf
    ref = pp["ssd"][live].sum()
    bound = pp["fwd_bound"][live].sum() + SECOND * k8_chain(shape, tiled_enabled) * U * ref
    return ratio(acc[0], ref, bound)


def k8_check_grad(got, pp, mask, gloss, shape, sign):
    """every element of grad_disp [B,H,W]; masked elements (all of them under an all-zero mask) are +0 bit for bit"""
    B, C, H, W, ps = shape
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    live = np.ones(B * H * W, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if np.any(got[~live].view(np.uint32) != 0):
        return np.inf
    if not live.any():
        return 0.0
    ref, bound = patch_grad(pp, gloss, float(live.sum()), C, ps, sign)
    return ratio(got[live], ref[live], bound[live])
