"""CPU: what says that the element-wise sweep of tests/test_gpu_reproj_fp64.py would notice a defect.

A numpy-float32 emulation of each of K7 (az_warp_gather.hip), K8 (az_patch_reproj.hip) and K9 (az_lcn.hip) -- the kernels'
operation order, per-pixel fp32 accumulation, an arbitrary fixed order for the grad_img scatter -- passes every check of
tests/_reproj_fp64ref.py at every shape of the GPU file (for the widest and the million-pixel shapes on a strided sample of the
pixels), and each mutant of the emulation fails at least one check at every shape its class applies to.  No mutant kernel is
built or run.  The references themselves are pinned against float64 torch (grid_sample, unfold, fold) and the oracle, the fp32
coordinate against the oracle's closed form, and the invariant the tiled kernel's LDS row index rests on (floor(iy) is i - 1 or
i) is swept over every height to 4096.

Two mutants of the list cannot be rejected everywhere, and the reason is arithmetic, not the checks:
  * K7 "clamp dropped" at disp = +-1e6: floor(ix) fits an int, so the unclamped tap is out of range exactly as the clamped one
    is; the emulation's outputs are the same bits (asserted).  The clamp only guards the conversion of values beyond 2^31.
  * K9 "divisor k^2 - 1" at k = 113: it changes std by 4e-5 of itself, below the counted bound of 12 769-term fp32 sums.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reprojection_oracle as O
from tests import _reproj_fp64ref as RP

f32 = np.float32


# ---- K7 in fp32 -----------------------------------------------------------------------------------------------------------------
def emu_k7(img, disp, gout, mut=None):
    img, gout = np.asarray(img, dtype=np.float32), np.asarray(gout, dtype=np.float32)
    B, C, H, W = img.shape
    ix, iy = RP.pixel_coords(disp, H, W)
    with np.errstate(all="ignore"):
        fx, fy = np.floor(ix), np.floor(iy)
        if mut == "noclamp":
            x0 = fx.astype(np.int64)
        else:
            x0 = np.fmin(np.fmax(fx, f32(-2)), f32(W) + f32(1)).astype(np.int64)
        y0 = np.fmin(np.fmax(fy, f32(-2)), f32(H) + f32(1)).astype(np.int64)
        tx, ty = ix - fx, np.broadcast_to((iy - fy)[:, None], ix.shape)
    y0 = np.broadcast_to(y0[:, None], x0.shape)
    if mut == "shift":
        x0 = x0 + 1
    vx0, vx1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    vy0, vy1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    if mut == "novx1":
        vx1 = np.ones_like(vx1)
    wx0, wy0 = f32(1) - tx, f32(1) - ty
    w = {(0, 0): wx0 * wy0, (0, 1): tx * wy0, (1, 0): wx0 * ty, (1, 1): tx * ty}
    val = {(0, 0): vy0 & vx0, (0, 1): vy0 & vx1, (1, 0): vy1 & vx0, (1, 1): vy1 & vx1}
    flat = img.reshape(B, C, H * W)
    bb = np.arange(B)[:, None, None]
    o00 = y0 * W + x0
    tap = {k: np.where(val[k][:, None], flat[bb[:, None], np.arange(C)[None, :, None, None],
                                               np.clip(o00 + k[0] * W + k[1], 0, H * W - 1)[:, None]], f32(0)) for k in w}
    out = np.zeros((B, C, H, W), dtype=np.float32)
    for k in ((0, 0), (0, 1), (1, 0), (1, 1)):
        out = np.where(val[k][:, None], out + tap[k] * w[k][:, None], out)
    assert out.dtype == np.float32
    inner = (tap[0, 1] - tap[0, 0]) * wy0[:, None] + (tap[1, 1] - tap[1, 0]) * ty[:, None]
    if mut == "nowy":
        inner = (tap[0, 1] - tap[0, 0]) + (tap[1, 1] - tap[1, 0])
    gd = np.zeros((B, H, W), dtype=np.float32)
    for c in range(C):
        gd = gd + gout[:, c] * inner[:, c]
    gi = np.zeros((B, C, H * W), dtype=np.float32)
    gw = {(0, 0): (wx0, wy0), (0, 1): (tx, wy0), (1, 0): (wx0, ty), (1, 1): (tx, ty)}
    if mut == "transposed":
        gw[0, 1], gw[1, 0] = gw[1, 0], gw[0, 1]
    bfull = np.broadcast_to(bb, x0.shape)
    for k, (a, b) in gw.items():
        ok = val[k]
        for c in range(C):
            np.add.at(gi, (bfull[ok], c, np.clip(o00 + k[0] * W + k[1], 0, H * W - 1)[ok]), (gout[:, c] * a * b)[ok])
    assert gd.dtype == gi.dtype == np.float32
    return out, gd, gi.reshape(B, C, H, W)


@functools.lru_cache(maxsize=None)
def k7_reference(shape, which):
    img, disp, gout = RP.k7_inputs(shape, which)
    return RP.warp_fwd(img, disp), RP.warp_bwd(gout, img, disp)


def k7_ratios(shape, which, outs):
    out, gd, gi = outs
    (ref, mag), ((gdr, gdm), (gir, gim, gic)) = k7_reference(shape, which)
    return {"fwd": RP.ratio(out, ref, RP.warp_fwd_bound(mag)), "gdisp": RP.ratio(gd, gdr, RP.warp_gdisp_bound(gdm, shape[1])),
            "gimg": RP.ratio(gi, gir, RP.warp_gimg_bound(gim, gic))}


@pytest.mark.parametrize("shape", RP.K7_SHAPES, ids=str)
@pytest.mark.parametrize("which", RP.SETS)
def test_k7_emulation_is_within_every_bound(shape, which):
    r = k7_ratios(shape, which, emu_k7(*RP.k7_inputs(shape, which)))
    print(shape, which, r)
    assert max(r.values()) <= 1.0, r
    if which == "zero":
        out, gd, _ = emu_k7(*RP.k7_inputs(shape, which))
        assert not out.any() and not gd.any()


K7_MUTANTS = {"shift": "fwd", "novx1": "fwd", "nowy": "gdisp", "transposed": "gimg"}


@pytest.mark.parametrize("shape", RP.K7_SHAPES[:4], ids=str)
@pytest.mark.parametrize("mut", sorted(K7_MUTANTS))
def test_k7_mutant_is_rejected(shape, mut):
    r = k7_ratios(shape, "seeded", emu_k7(*RP.k7_inputs(shape, "seeded"), mut=mut))
    assert max(r.values()) > 1.0, (mut, r)


def test_k7_clamp_mutant_is_the_same_bits_at_a_million():
    """+-1e6 fits an int: without the clamp the taps are as far out of range as with it (module docstring)"""
    for shape in RP.K7_SHAPES[1:4]:
        args = RP.k7_inputs(shape, "seeded")
        assert np.abs(args[1]).max() >= 9e5
        for a, b in zip(emu_k7(*args), emu_k7(*args, mut="noclamp")):
            assert np.array_equal(a, b)


def test_k7_fields_hold_every_class():
    for B, C, H, W in RP.K7_SHAPES[1:]:
        got = RP.classes_of(RP.k7_inputs((B, C, H, W), "seeded")[1], H, W)
        assert got == set(RP.CLASSES), set(RP.CLASSES) - got


# ---- K8 in fp32 -----------------------------------------------------------------------------------------------------------------
def emu_k8(L, R, disp, ps, sign, pix, mut=None, tr=1, K=4):
    """per pixel of pix: (the fp32 sum of squares over (c, u, v), [the fp32 sum diff dW of each channel])"""
    L, R = np.asarray(L, dtype=np.float32), np.asarray(R, dtype=np.float32)
    B, C, H, W = L.shape
    r = ps // 2
    bb, ii, jj = pix
    d = (f32(sign) * np.asarray(disp, dtype=np.float32).reshape(B, H, W)).astype(np.float32)
    if mut == "neighbour":
        d = d[:, :, np.minimum(np.arange(W) + 1, W - 1)]
    ix, iy = RP.pixel_coords(d, H, W)
    ix, irow = ix[bb, ii, jj], ((ii // tr) * tr if mut == "bandrow" else ii)
    with np.errstate(all="ignore"):
        fx, fy = np.floor(ix), np.floor(iy)
        x0 = np.fmin(np.fmax(fx, f32(-2)), f32(W) + f32(1)).astype(np.int64)
        y0 = np.fmin(np.fmax(fy, f32(-2)), f32(H) + f32(1)).astype(np.int64)[irow]
        tx, ty = ix - fx, (iy - fy)[ii]
    vx0, vx1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    vy0, vy1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    if mut == "corners":
        vx0 = vx1 = vy0 = vy1 = np.ones_like(vx0)
    z, one = f32(0), f32(1)
    wx0, wx1, wy0, wy1 = np.where(vx0, one - tx, z), np.where(vx1, tx, z), np.where(vy0, one - ty, z), np.where(vy1, ty, z)
    dx0, dx1 = np.where(vx0, -one, z), np.where(vx1, one, z)

    def ld(img, c, y, x):
        if mut == "edge":
            return img[bb, c, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        return np.where(ok, img[bb, c, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], z)

    pixs = np.zeros(len(bb), dtype=np.float32)
    gch = []
    for c in range(C):
        g = np.zeros(len(bb), dtype=np.float32)
        for u in range(-r, r + 1):
            for v in range(-r, r + 1):
                a0, b0 = ld(R, c, y0 + u, x0 + v), ld(R, c, y0 + u, x0 + v + 1)
                a1, b1 = ld(R, c, y0 + u + 1, x0 + v), ld(R, c, y0 + u + 1, x0 + v + 1)
                warped = wy0 * (wx0 * a0 + wx1 * b0) + wy1 * (wx0 * a1 + wx1 * b1)
                lrow = ii + u + (1 if mut == "urow" else 0)
                lcol = jj + v + (jj % K if mut == "lcol" else 0)
                diff = warped - ld(L, c, lrow, lcol)
                pixs = pixs + diff * diff
                g = g + diff * (wy0 * (dx0 * a0 + dx1 * b0) + wy1 * (dx0 * a1 + dx1 * b1))
        gch.append(g)
    assert pixs.dtype == np.float32 and all(g.dtype == np.float32 for g in gch)
    return pixs, gch


def k8_outputs(shape, pixs, gch, mask, gloss, sign, mut=None):
    """the emulated launch over every pixel: (acc [2], grad_disp [B H W]); a dropped pixel's gradient stays unwritten (NaN)"""
    B, C, H, W, ps = shape
    n = B * H * W
    live = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    jj, ii = np.arange(n) % W, (np.arange(n) // W) % H
    done_f, done_b = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    if mut == "dropgroup":
        done_f, done_b = jj < (W // 4) * 4, jj < (W // 2) * 2
    if mut == "dropband":
        rf, rb = RP.k8_route(shape, "fwd"), RP.k8_route(shape, "bwd")
        done_f = ii < (rf["nbands"] - (rf["last"] < rf["tr"])) * rf["tr"]
        done_b = ii < (rb["nbands"] - (rb["last"] < rb["tr"])) * rb["tr"]
    summed = done_f if mut == "masked" else live & done_f
    count = float((live & done_f).sum())
    acc = np.array([pixs[summed].astype(np.float64).sum(), count * (1 if mut == "count" else C * ps * ps)])
    true_acc1 = float(live.sum()) * C * ps * ps
    with np.errstate(all="ignore"):
        scale = f32(np.float64(gloss) * 2.0 / np.float64(true_acc1)) * (f32(1) if mut == "nosign" else f32(sign))
    grad = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):   # (an all-zero mask: the scale is inf or NaN, and no live pixel takes it)
        for c, g in enumerate(gch):
            gv = g * scale
            grad = gv if (c == 0 or mut == "overwrite") else grad + gv
    grad = np.where(live, grad, f32(0))
    grad = np.where(done_b, grad, f32(np.nan))
    return acc, grad.astype(np.float32)


def strided(shape):
    """every pixel, or for the widest and the million-pixel shapes every 7th (the emulation only)"""
    B, C, H, W, ps = shape
    b, i, j = RP.all_pixels(B, H, W)
    step = 7 if B * H * W * ps * ps > 300000 else 1
    return b[::step], i[::step], j[::step]


@functools.lru_cache(maxsize=None)
def k8_reference(shape, which, sign, full):
    L, R, disp = RP.k8_inputs(shape, which)
    return RP.patch_pixel(L, R, disp, shape[4], sign, None if full else strided(shape))


ALL_K8 = RP.K8_SHAPES + [RP.K8_STRIDE_CASE]


@pytest.mark.parametrize("shape", ALL_K8, ids=str)
@pytest.mark.parametrize("which,sign", [("seeded", -1.0), ("seeded", 1.0), ("binary", -1.0), ("zero", -1.0)])
def test_k8_emulation_is_within_every_bound(shape, which, sign):
    B, C, H, W, ps = shape
    L, R, disp = RP.k8_inputs(shape, which)
    pix = strided(shape)
    full = len(pix[0]) == B * H * W
    pp = k8_reference(shape, which, sign, full)
    pixs, gch = emu_k8(L, R, disp, ps, sign, pix)
    rs = {"pixel": RP.k8_check_pixels(np.stack([pixs, np.full(len(pixs), C * ps * ps)], 1), pp, C, ps)}
    if which == "zero":   # the per-pixel value is sum L^2, and no gradient flows
        assert not any(g.any() for g in gch)
    if full:
        for mk in ("none", "random", "zero"):
            mask = RP.k8_mask(shape, mk)
            for gloss in (1.0, 3.0, -0.5):
                acc, grad = k8_outputs(shape, pixs, gch, mask, gloss, sign)
                rs[f"full {mk}"] = RP.k8_check_full(acc, pp, mask, shape)
                rs[f"grad {mk} {gloss}"] = RP.k8_check_grad(grad, pp, mask, gloss, shape, sign)
            if mk == "zero":
                assert acc[0] == 0 and acc[1] == 0 and not grad.view(np.uint32).any()
    else:   # the gradient on the sample, under no mask
        n = float(B * H * W)
        ref, bound = RP.patch_grad(pp, 3.0, n, C, ps, sign)
        scale = f32(3.0 * 2.0 / (n * C * ps * ps)) * f32(sign)
        rs["grad sample"] = RP.ratio(sum(g * scale for g in gch), ref, bound)
    print(shape, which, sign, rs)
    assert max(rs.values()) <= 1.0, rs


# mutant -> the shapes its class applies to
def _partial_band(s):
    return any(0 < RP.k8_route(s, w)["last"] < RP.k8_route(s, w)["tr"] for w in ("fwd", "bwd"))


K8_MUTANTS = {
    "neighbour": lambda s: True,
    "urow": lambda s: True,
    "lcol": lambda s: True,                                     # every shape has a pixel with j % PR_K != 0
    "bandrow": lambda s: RP.k8_route(s, "fwd")["tr"] > 1,
    "corners": lambda s: s[4] > 1,                               # at ps = 1 a tap is the corner itself: outside, hence zero
    "edge": lambda s: s[4] > 1,                                  # ps = 1 reads no padding
    "dropgroup": lambda s: s[3] % 2 != 0 or s[3] % 4 != 0,
    "dropband": _partial_band,
    "count": lambda s: s[1] * s[4] * s[4] > 1,
    "masked": lambda s: True,
    "nosign": lambda s: True,
    "overwrite": lambda s: s[1] > 1,
}
_MUT_SHAPES = RP.K8_SMALL + RP.K8_BANDS   # (the widest shapes repeat (1,1,16,17,15)'s classes at 80 times the cost)


@pytest.mark.parametrize("shape", _MUT_SHAPES, ids=str)
def test_k8_mutants_are_rejected(shape):
    B, C, H, W, ps = shape
    sign, gloss, which = -1.0, 3.0, "seeded"
    L, R, disp = RP.k8_inputs(shape, which)
    pix = RP.all_pixels(B, H, W)
    pp = k8_reference(shape, which, sign, True)
    mask = RP.k8_mask(shape, "random")
    base = emu_k8(L, R, disp, ps, sign, pix)
    tr = RP.k8_route(shape, "fwd")["tr"]
    applied = 0
    for mut, applies in K8_MUTANTS.items():
        if not applies(shape):
            continue
        if mut == "nosign" and not pp["g"][mask.reshape(-1) != 0].any():
            continue   # (the four pixels of the 2 x 2 image: every live pixel samples outside, no gradient to mis-sign)
        applied += 1
        kernel_level = mut in ("neighbour", "urow", "lcol", "bandrow", "corners", "edge")
        pixs, gch = emu_k8(L, R, disp, ps, sign, pix, mut=mut, tr=tr) if kernel_level else base
        acc, grad = k8_outputs(shape, pixs, gch, mask, gloss, sign, mut=mut)
        rs = [RP.k8_check_pixels(np.stack([pixs, np.full(len(pixs), C * ps * ps)], 1), pp, C, ps),
              RP.k8_check_full(acc, pp, mask, shape), RP.k8_check_grad(grad, pp, mask, gloss, shape, sign)]
        assert max(rs) > 1.0, (mut, rs)
    assert applied >= 5


def test_k8_fields_hold_every_class():
    for s in RP.K8_SHAPES[1:]:
        if s[0] * s[2] * s[3] < 64:
            continue
        got = RP.classes_of(RP.k8_inputs(s, "seeded")[2], s[2], s[3])
        assert got == set(RP.CLASSES), (s, set(RP.CLASSES) - got)


# ---- the Fold -------------------------------------------------------------------------------------------------------------------
def emu_vis(R, disp, ps, sign, mut=None):
    R = np.asarray(R, dtype=np.float32)
    B, C, H, W = R.shape
    r = ps // 2
    vis = np.zeros((B, C, H, W), dtype=np.float32)
    bb, ii, jj = RP.all_pixels(B, H, W)
    d = (f32(sign) * np.asarray(disp, dtype=np.float32).reshape(B, H, W)).astype(np.float32)
    x0, y0, tx, ty, vx0, vx1, vy0, vy1 = (t[bb, ii, jj] for t in RP.coords(d, H, W))
    tx, ty = tx.astype(np.float32), ty.astype(np.float32)
    z, one = f32(0), f32(1)
    wx0, wx1, wy0, wy1 = np.where(vx0, one - tx, z), np.where(vx1, tx, z), np.where(vy0, one - ty, z), np.where(vy1, ty, z)
    Rp = np.pad(R, ((0, 0), (0, 0), (r + 3, r + 3), (r + 3, r + 3)))
    P = r + 3
    for c in range(C):
        for u in range(-r, r + 1):
            for v in range(-r, r + 1):
                top = wx0 * Rp[bb, c, y0 + u + P, x0 + v + P] + wx1 * Rp[bb, c, y0 + u + P, x0 + v + 1 + P]
                bot = wx0 * Rp[bb, c, y0 + u + 1 + P, x0 + v + P] + wx1 * Rp[bb, c, y0 + u + 1 + P, x0 + v + 1 + P]
                val = wy0 * top + wy1 * bot
                y, x = (ii - u if mut == "plus" else ii + u), jj + v      # (mutant: y + u instead of y - u)
                ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
                np.add.at(vis, (bb[ok], c, y[ok], x[ok]), val[ok])
    assert vis.dtype == np.float32
    return vis


@pytest.mark.parametrize("shape", RP.K8_SMALL + [RP.K8_BANDS[0]], ids=str)
def test_fold_emulation_and_mutant(shape):
    B, C, H, W, ps = shape
    L, R, disp = RP.k8_inputs(shape, "seeded")
    ref, mag = RP.patch_vis(R, disp, ps, -1.0)
    assert RP.ratio(emu_vis(R, disp, ps, -1.0), ref, RP.vis_bound(mag, ps)) <= 1.0
    if ps > 1:
        assert RP.ratio(emu_vis(R, disp, ps, -1.0, mut="plus"), ref, RP.vis_bound(mag, ps)) > 1.0


# ---- K9 in fp32 -----------------------------------------------------------------------------------------------------------------
def emu_k9(img, k, eps, mut=None):
    x = np.asarray(img, dtype=np.float32)
    B, H, W = x.shape
    r = k // 2
    xp = np.pad(x, ((0, 0), (r, r + 1), (r, r + 1)), mode="edge" if mut == "edge" else "constant")
    n = f32(k * k)
    s = 1 if mut == "shift" else 0
    win = lambda u, v: xp[:, u:u + H, v + s:v + s + W]
    tot, sq = np.zeros_like(x), np.zeros_like(x)
    for u in range(k):
        for v in range(k):
            tot = tot + win(u, v)
            sq = sq + win(u, v) * win(u, v)
    mean = tot / n
    ss = np.zeros_like(x)
    for u in range(k):
        for v in range(k):
            dd = win(u, v) - mean
            ss = ss + dd * dd
    with np.errstate(all="ignore"):
        var = ss / (n - f32(1) if mut == "nm1" else n)
        if mut == "onepass":
            var = np.maximum(sq / n - mean * mean, f32(0))
        e = f32(eps)
        sd = np.sqrt(var + e) if mut == "epsroot" else np.sqrt(var)
        normed = (x - mean) / (sd if mut == "epsroot" else sd + e)
    assert normed.dtype == sd.dtype == np.float32
    return normed, sd


@functools.lru_cache(maxsize=None)
def k9_reference(shape, which):
    return RP.lcn(RP.k9_input(shape, which)[:, 0], shape[4], 1e-5)


def k9_ratios(shape, which, outs):
    ref = k9_reference(shape, which)
    return {"std": RP.ratio(outs[1], ref["sd"], ref["sd_bound"]), "normed": RP.ratio(outs[0], ref["normed"], ref["normed_bound"])}


@pytest.mark.parametrize("shape", RP.K9_SHAPES, ids=str)
@pytest.mark.parametrize("which", RP.K9_SETS)
def test_k9_emulation_is_within_every_bound(shape, which):
    normed, sd = emu_k9(RP.k9_input(shape, which)[:, 0], shape[4], 1e-5)
    r = k9_ratios(shape, which, (normed, sd))
    print(shape, which, r)
    assert max(r.values()) <= 1.0, r
    if shape[4] == 1:
        assert not sd.any() and not normed.any()
    if which == "flat":
        inside = RP.k9_flat_inside(shape)
        assert not sd[:, inside].any() and not normed[:, inside].any()


# mutant -> the shapes its class applies to (k = 1 has no window; at 5x7, k = 113 every window holds the whole image)
K9_MUTANTS = {
    "onepass": lambda s: 1 < s[4] <= min(s[2], s[3]),          # (a window that is mostly padding does not cancel)
    "nm1": lambda s: 1 <= s[4] < 113,       # (k = 1 divides by zero: rejected as non-finite)
    "shift": lambda s: s[4] < 113 and s[2] * s[3] > 1,
    "edge": lambda s: s[4] > 1,
    "epsroot": lambda s: s[4] > 1,
}


@pytest.mark.parametrize("shape", RP.K9_SHAPES, ids=str)
@pytest.mark.parametrize("mut", sorted(K9_MUTANTS))
def test_k9_mutant_is_rejected_on_some_input_set(shape, mut):
    if not K9_MUTANTS[mut](shape):
        return
    worst = {w: max(k9_ratios(shape, w, emu_k9(RP.k9_input(shape, w)[:, 0], shape[4], 1e-5, mut=mut)).values()) for w in RP.K9_SETS}
    assert max(worst.values()) > 1.0, worst
    if mut == "onepass":
        assert worst["offset"] > 1.0, worst


# ---- the references, pinned -----------------------------------------------------------------------------------------------------
def _grid64(disp, H, W):
    """the float64 grid that makes F.grid_sample sample at the fp32 (ix, iy)"""
    x0, y0, tx, ty, *_ = RP.coords(disp, H, W)   # floor + weight: a tiny negative ix has ix - floor(ix) == 1.0f, column 0 exactly
    with np.errstate(all="ignore"):
        ix = np.where(np.abs(x0) < W + 1, x0 + tx, np.float64(4.0 * W) * np.sign(x0))   # (clamped taps: anywhere far outside)
    gx = (2.0 * ix + 1.0) / W - 1.0
    gy = (2.0 * (y0 + ty) + 1.0) / H - 1.0
    return torch.from_numpy(np.stack([gx, gy], -1))


@pytest.mark.parametrize("shape", RP.K7_SHAPES[:4], ids=str)
def test_warp_reference_is_grid_sample_in_float64(shape):
    img, disp, gout = RP.k7_inputs(shape, "seeded")
    B, C, H, W = shape
    t = torch.from_numpy(img).double().requires_grad_()
    out = F.grid_sample(t, _grid64(disp, H, W), mode="bilinear", padding_mode="zeros", align_corners=False)
    ref, _ = RP.warp_fwd(img, disp)
    assert np.abs(out.detach().numpy() - ref).max() <= 1e-12
    (gi,) = torch.autograd.grad(out, t, torch.from_numpy(gout).double())
    _, (gir, _, _) = RP.warp_bwd(gout, img, disp)
    assert np.abs(gi.numpy() - gir).max() <= 1e-12


@pytest.mark.parametrize("shape", RP.K7_SHAPES[:4], ids=str)
def test_fp32_coordinates_are_the_oracles_within_nine_roundings(shape):
    """in units of U (W + |disp| + 1): the division (1), the linspace's step, product and subtraction (3), the sum (1),
    2 g - 1 (1), + 1 (1), times W (1), - 1 (1): 9; the halving and the doubling are exact"""
    B, C, H, W = shape
    disp = RP.k7_inputs(shape, "seeded")[1]
    ix, iy = RP.pixel_coords(disp, H, W)
    px, py = O.sample_coords(H, W, torch.from_numpy(disp)[:, None])
    assert bool((np.abs(ix - px.numpy()) <= 9 * RP.U * (W + np.abs(disp.astype(np.float64)) + 1)).all())
    assert bool((np.abs(iy[None, :, None] - py.numpy()) <= 9 * RP.U * (H + 1)).all())


@pytest.mark.parametrize("shape", RP.K8_SMALL + [RP.K8_BANDS[0]], ids=str)
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_patch_reference_is_unfold_grid_sample_fold_in_float64(shape, sign):
    B, C, H, W, ps = shape
    L, R, disp = RP.k8_inputs(shape, "seeded")
    r = ps // 2
    d = (f32(sign) * disp).astype(np.float32)
    grid = _grid64(d, H, W).requires_grad_()
    tl = F.unfold(torch.from_numpy(L).double(), ps, padding=r).reshape(B, C * ps * ps, H, W)
    tr_ = F.unfold(torch.from_numpy(R).double(), ps, padding=r).reshape(B, C * ps * ps, H, W)
    warped = F.grid_sample(tr_, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    ssd = ((warped - tl) ** 2).sum(1)
    pp = RP.patch_pixel(L, R, disp, ps, sign)
    tol = lambda ref: 1e-12 * (1.0 + np.abs(ref))
    got = ssd.detach().numpy().reshape(-1)
    assert bool((np.abs(got - pp["ssd"]) <= tol(pp["ssd"])).all())
    (gg,) = torch.autograd.grad(0.5 * ssd.sum(), grid)
    gx = gg[..., 0].numpy().reshape(-1) * 2.0 / W       # d ix / d grid_x = W / 2
    tx = RP.coords(d, H, W)[2].reshape(-1)
    off = (tx != 0) & (tx != 1)                           # on a column the derivative is one-sided: the side is the floor's
    assert bool((np.abs(gx - pp["g"])[off] <= 1e-11 * (1.0 + pp["g_abs"][off])).all())
    vis = F.fold(warped.detach().reshape(B, C * ps * ps, H * W), (H + ps - 1, W + ps - 1), ps)
    if ps > 1:
        vis = vis[:, :, r:-r, r:-r]
    ref, mag = RP.patch_vis(R, disp, ps, sign)
    assert bool((np.abs(vis.numpy() - ref) <= 1e-12 * (1.0 + mag)).all())


@pytest.mark.parametrize("shape", RP.K9_SHAPES, ids=str)
def test_lcn_reference_is_the_oracle_in_float64(shape):
    x = RP.k9_input(shape, "seeded")[:, :1]
    ref = RP.lcn(x[:, 0], shape[4], 1e-5)
    normed, std = O.local_contrast_norm(torch.from_numpy(x).double(), shape[4], float(f32(1e-5)))
    assert np.abs(std[:, 0].numpy() - ref["sd"]).max() <= 1e-12
    assert bool((np.abs(normed[:, 0].numpy() - ref["normed"]) <= 1e-9 * (1 + np.abs(ref["normed"]))).all())


# ---- the row invariant and the dispatch -----------------------------------------------------------------------------------------
def test_floor_of_iy_is_the_row_or_the_row_above():
    """the tiled kernel's LDS row index y0 + t - ra rests on it"""
    for H in range(2, 4097):
        y0, _ = RP.taps(RP.unnormalise(RP.linspace01(H), H), H)
        i = np.arange(H)
        assert bool(((y0 == i - 1) | (y0 == i)).all()), H


def test_the_shape_list_reaches_every_route():
    feats = RP.k8_route_features(RP.K8_SHAPES)
    assert RP.K8_WANT <= feats, RP.K8_WANT - feats
    # what the issue states about the shapes, as the restated rule gives it
    bands = [(RP.k8_route(s, "fwd")["tr"], RP.k8_route(s, "fwd")["last"]) for s in RP.K8_BANDS]
    print("band heights and last bands:", bands)
    assert bands == [(2, 1), (3, 1), (4, 4), (5, 5)]
    lds = [(RP.k8_route(s, "fwd")["tiled"], RP.k8_route(s, "bwd")["tiled"]) for s in RP.K8_LDS]
    assert lds == [(True, True), (False, True), (False, False)]
    assert max(RP.k8_route(s, w)["lds"] for s in RP.K8_LDS for w in ("fwd", "bwd")) == 161680 <= 159 * 1024   # (the backward at W = 1245; the forward at W = 1244 asks for 161 672)
    assert RP.k8_route(RP.K8_LDS[0], "fwd")["lds"] == 161672
    assert all(RP.k8_route(s, "fwd")["tr"] == 1 for s in RP.K8_SMALL)
    assert RP.k8_route(RP.K8_STRIDE_CASE, "fwd")["tiled"] and 1025 * 1024 > RP.GRID_THREADS
    off = RP.k8_route_features(RP.K8_SHAPES + [RP.K8_STRIDE_CASE], tiled_enabled=False)
    assert "per-pixel by switch" in off and not any(f.startswith("PSM") or f.startswith("tr") for f in off)
    # K7 and K9: the grid-stride case and a partial 16 x 16 tile on both axes
    assert any(b * h * w > RP.GRID_THREADS for b, c, h, w in RP.K7_SHAPES)
    assert any(h % 16 and w % 16 and h > 16 and w > 16 for b, c, h, w, k in RP.K9_SHAPES)
