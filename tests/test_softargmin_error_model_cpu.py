"""CPU: what says that the element-wise sweep of tests/test_gpu_softargmin_fp64.py would notice a defect.

A numpy-float32 emulation of K6 (az_softargmin.hip) -- the tile load with clamped indices, the kernel's phase weights and
operation order, its shift rule, the four accumulator pairs of the register-resident depths and the single pair of the generic
loop, the backward pass' D-lerp fold, the quad and +-4-lane reduction (as plain sums), the per-wave row shares, the sum of the
four waves' images, the clamped flush (in one fixed order) and the dead lanes of a last tile narrower than 64 pixels -- passes
every check of tests/_softargmin_fp64ref.py at every shape and input set of the GPU file, on the saved-statistics and on the
recompute path.  Each mutant of the emulation fails at least one check at every shape its class applies to.  No mutant kernel is
built or run.  The closed-form reference itself is pinned against float64 F.interpolate + softmax + autograd and against
oracle.psmnet_oracle.soft_argmin_head.

Where a mutant cannot be rejected, the reason is arithmetic, not the checks:
  * a swapped phase weight or a border cell read as zero needs two different cells (phase) or any cell (border) on that axis:
    the phase mutants apply where the axis is longer than one (the D-axis one from d == 2), the border ones everywhere;
  * "index" (4k + 1 + m) and "fold" (the D-lerp weights swapped in the backward pass) live in the loop over plane pairs, which
    d == 1 never enters; at d == 1 the output is the constant 1.5 and the gradient identically zero, so no mutant of the
    backward pass alone ("rows", "halo_l", "halo_r") can show there either: every share is a multiple of zero;
  * "planemax" needs an upsampled maximum below the plane maximum: an interior spike plane, d >= 3; at d == 2 the spike is the
    end plane, whose value IS an upsampled level, and at d == 1 there is nothing else -- there the outputs are the same bits;
  * "rows" (wy1 and 1 - wy1 swapped) is invisible at h == 1, where all three tile rows alias row 0;
  * "halo_r" drops what quad 15 of a wave sends to tile column 17; a tile narrower than 64 pixels has no live quad 15, so it
    applies from w == 16 on; "halo_l" (quad 0 to tile column 0, which is cell -1 in the first tile) applies everywhere;
  * "stats_s" (one end term missing from the saved s) is invisible on `spike`, where that term is exp(-2000) = 0, and on
    `plain` its weight p_D can fall below what a sequential fp32 sum of 328 terms is granted (d == 82: ratio 0.99); it is
    searched on `flat`, where the term is exactly 1 / D of s, by the check of the saved s;
  * "dead_old" is the backward kernel as it stood before its dead lanes were given a shift of their own: they read the
    statistics of pixel (0, 0, 0) of batch 0.  It is rejected on `wide` at every width with dead lanes (a NaN in column
    w - 1); on the other sets it only multiplies finite numbers by zero and is the same bits as the fixed kernel.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import psmnet_oracle as po
from tests import _softargmin_fp64ref as SA

f32 = np.float32
L2E = f32(1.4426950408889634)
LAM1 = np.array(SA.PHASE_W1, dtype=np.float32)            # upper weight per phase r (sa_axis)
LAM1_SWAPPED = np.array((0.875, 0.625, 0.375, 0.125), dtype=np.float32)
W1 = np.array((0.125, 0.375, 0.625, 0.875), dtype=np.float32)       # D-lerp: 0.125 + 0.25 m
W1_SWAPPED = np.array((0.375, 0.125, 0.875, 0.625), dtype=np.float32)


def fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def exp2(x):
    with np.errstate(all="ignore"):
        r = np.exp2(x.astype(np.float32))
    assert r.dtype == np.float32
    return r


def sa_axis(dst, base, swapped=False):
    q, r = dst >> 2, dst & 3
    return np.where(r < 2, q - 1, q) - base, (LAM1_SWAPPED if swapped else LAM1)[r]


class Tiles:
    """the launch geometry and the plane values of every thread: N = b * h * tiles_x blocks of 4 waves x 64 lanes"""

    def __init__(self, logits, mut=None):
        lg = np.asarray(logits, dtype=np.float32)
        b, d, h, w = lg.shape
        self.shape, self.tiles_x = lg.shape, (4 * w + 63) // 64
        N = b * h * self.tiles_x
        self.bi, ty, tx = np.unravel_index(np.arange(N), (b, h, self.tiles_x))
        tid = np.arange(256)
        self.Y, self.X = ty[:, None] * 4 + (tid >> 6)[None], tx[:, None] * 64 + (tid & 63)[None]
        self.live = self.X < 4 * w
        ybase, xbase = ty - 1, tx * 16 - 1
        cy, cx = ybase[:, None] + np.arange(3)[None], xbase[:, None] + np.arange(18)[None]
        self.gy, self.gx = np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)
        tile = lg.transpose(0, 2, 3, 1)[self.bi[:, None, None], self.gy[:, :, None], self.gx[:, None, :]]   # sa_load_tile, [N,3,18,d]
        if mut == "zero_y":
            tile = np.where(((cy < 0) | (cy >= h))[:, :, None, None], f32(0), tile)
        if mut == "zero_x":
            tile = np.where(((cx < 0) | (cx >= w))[:, None, :, None], f32(0), tile)
        self.ly0, self.wy1 = sa_axis(self.Y, ybase[:, None], mut == "phase_y")
        self.lx0, self.wx1 = sa_axis(self.X, xbase[:, None], mut == "phase_x")
        assert self.ly0.min() >= 0 and self.ly0.max() <= 1 and self.lx0.min() >= 0 and self.lx0.max() <= 16
        nn = np.arange(N)[:, None]
        a00, a01 = tile[nn, self.ly0, self.lx0], tile[nn, self.ly0, self.lx0 + 1]
        a10, a11 = tile[nn, self.ly0 + 1, self.lx0], tile[nn, self.ly0 + 1, self.lx0 + 1]
        wx1, wy1 = self.wx1[..., None], self.wy1[..., None]
        wx0, wy0 = f32(1) - wx1, f32(1) - wy1
        self.V = wy0 * (wx0 * a00 + wx1 * a01) + wy1 * (wx0 * a10 + wx1 * a11)                              # sa_plane, [N,256,d]
        assert self.V.dtype == np.float32


def emu_stats(V, mut=None):
    """sa_stats: (M, s, t, s as saved) of every thread; V [..., d]"""
    d = V.shape[-1]
    planes = d in (48, 16)
    w1s = W1_SWAPPED if mut == "phase_d" else W1
    if mut == "planemax":
        M = V.max(-1)
    else:
        M = np.maximum(V[..., 0], V[..., -1])
        if d > 1:
            a, c = V[..., :-1], V[..., 1:]
            M = np.maximum(M, np.maximum(f32(0.875) * a + f32(0.125) * c, f32(0.125) * a + f32(0.875) * c).max(-1))
    Vp = (V - M[..., None]) * L2E
    z = (f32(0) - M) * L2E                       # plane -1 / plane d read as zero (mutant "zero_d")
    assert Vp.dtype == np.float32
    sa = [np.zeros(M.shape, dtype=np.float32) for _ in range(4)]
    ta = [np.zeros(M.shape, dtype=np.float32) for _ in range(4)]
    slot = (lambda m: m) if planes else (lambda m: 0)
    # D = 0, 1
    if mut == "zero_d":
        e0, e1 = exp2(f32(0.375) * z + f32(0.625) * Vp[..., 0]), exp2(f32(0.125) * z + f32(0.875) * Vp[..., 0])
        sa[0] = sa[0] + (e0 + e1)
        ta[0] = ta[0] + e1
    else:
        e = exp2(Vp[..., 0])
        sa[0] = sa[0] + (e if mut == "once" else e + e)
        ta[0] = ta[0] + e
    for k in range(d - 1):
        for m in range(4):
            e = exp2((f32(1) - w1s[m]) * Vp[..., k] + w1s[m] * Vp[..., k + 1])
            i = slot(m)
            sa[i] = sa[i] + e
            ta[i] = fma(f32(4 * k + (1 if mut == "index" else 2) + m), e, ta[i])
    # D = 4d - 2, 4d - 1
    i = 1 if planes else 0
    if mut == "zero_d":
        e0, e1 = exp2(f32(0.875) * Vp[..., -1] + f32(0.125) * z), exp2(f32(0.625) * Vp[..., -1] + f32(0.375) * z)
        sa[i] = sa[i] + (e0 + e1)
        ta[i] = ta[i] + (f32(4 * d - 2) * e0 + f32(4 * d - 1) * e1)
        e = e1
    else:
        e = exp2(Vp[..., -1])
        sa[i] = sa[i] + (e if mut == "once" else e + e)
        ta[i] = ta[i] + (f32(4 * d - 2) * e + f32(4 * d - 1) * e)
    s = (sa[0] + sa[1]) + (sa[2] + sa[3])
    t = (ta[0] + ta[1]) + (ta[2] + ta[3])
    assert s.dtype == t.dtype == np.float32
    return M, s, t, ((s - e).astype(np.float32) if mut == "stats_s" else s)


def emu_fwd(logits, mut=None):
    """(out [b,4h,4w], stats [b,4h,4w,2])"""
    T = Tiles(logits, mut)
    b, d, h, w = T.shape
    with np.errstate(all="ignore"):
        M, s, t, s_saved = emu_stats(T.V, mut)
        val = t / s
    out, stats = np.full((b, 4 * h, 4 * w), np.nan, dtype=np.float32), np.full((b, 4 * h, 4 * w, 2), np.nan, dtype=np.float32)
    at = (np.broadcast_to(T.bi[:, None], T.X.shape)[T.live], T.Y[T.live], T.X[T.live])
    out[at] = val[T.live]
    stats[at + (0,)] = M[T.live]
    stats[at + (1,)] = s_saved[T.live]
    assert not np.isnan(stats[..., 0]).any()      # every pixel has exactly one thread
    return out, stats


def exp_fast(x):
    with np.errstate(all="ignore"):
        return exp2(x * L2E)


def emu_bwd(logits, gout, stats=None, fwd_out=None, mut=None):
    """softargmin_bwd_kernel: grad_logits [b,d,h,w]; stats / fwd_out None: the recompute path"""
    T = Tiles(logits, mut)
    b, d, h, w = T.shape
    gout = np.asarray(gout, dtype=np.float32).reshape(b, 4 * h, 4 * w)
    N, live = len(T.bi), T.live
    bb = np.broadcast_to(T.bi[:, None], T.X.shape)
    Xc = np.where(live, T.X, 0)
    with np.errstate(all="ignore"):
        if stats is not None:
            if mut == "dead_old":      # a dead lane reads element 0: pixel (0, 0, 0) of batch 0
                pix = (np.where(live, bb, 0), np.where(live, T.Y, 0), Xc)
                M, s, pred = stats[pix + (0,)], stats[pix + (1,)], fwd_out[pix]
            else:                      # ... or owns a shift that makes every term of it exp2(-inf) = 0
                M = np.where(live, stats[bb, T.Y, Xc, 0], f32(np.inf))
                s = np.where(live, stats[bb, T.Y, Xc, 1], f32(1))
                pred = np.where(live, fwd_out[bb, T.Y, Xc], f32(0))
        else:
            M, s, t, _ = emu_stats(T.V, mut)
            pred = t / s
        g = np.where(live, gout[bb, T.Y, Xc] / s, f32(0)).astype(np.float32)
        r = np.arange(256) & 3
        wx0 = f32(1) - T.wx1
        zero = np.zeros_like(wx0)
        f_m1, f_0, f_p1 = np.where(r < 2, wx0, zero), np.where(r < 2, T.wx1, wx0), np.where(r < 2, zero, T.wx1)
        w1s = W1_SWAPPED if mut == "phase_d" else W1
        V = T.V
        v0 = V[..., 0]
        acc0 = g * exp_fast(v0 - M) * ((f32(0) - pred) + (f32(1) - pred))
        VAL = np.zeros((N, d, 4, 18), dtype=np.float32)
        for k in range(d):
            acc1 = np.zeros_like(acc0)
            if k + 1 < d:
                v1 = V[..., k + 1]
                for m in range(4):
                    w1 = w1s[m]
                    u = (f32(1) - w1) * v0 + w1 * v1
                    gu = g * exp_fast(u - M) * (f32(4 * k + 2 + m) - pred)
                    a, c = ((f32(1) - w1), w1) if mut != "fold" else (w1, (f32(1) - w1))
                    acc0 = acc0 + a * gu
                    acc1 = acc1 + c * gu
                v0 = v1
            else:
                acc0 = acc0 + g * exp_fast(v0 - M) * ((f32(4 * d - 2) - pred) + (f32(4 * d - 1) - pred))
            quad = lambda t: (lambda q: (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))(t.reshape(N, 4, 16, 4))
            s_m1, s_0, s_p1 = quad(f_m1 * acc0), quad(f_0 * acc0), quad(f_p1 * acc0)                        # [N,4,16]
            cell = s_0.copy()
            cell[..., 1:] = cell[..., 1:] + s_p1[..., :-1]          # from_left
            cell[..., :-1] = cell[..., :-1] + s_m1[..., 1:]         # from_right
            VAL[:, k, :, 1:17] = cell
            VAL[:, k, :, 0] = f32(0) if mut == "halo_l" else s_m1[..., 0]
            VAL[:, k, :, 17] = f32(0) if mut == "halo_r" else s_p1[..., 15]
            acc0 = acc1
        assert VAL.dtype == np.float32 and acc0.dtype == np.float32
        # the row shares of each wave (its lanes share Y) and the flush: waves in a fixed order, then the clamped global add
        wy1, ly0 = T.wy1[:, ::64], T.ly0[:, ::64]                   # [N,4]
        lo, hi = (f32(1) - wy1, wy1) if mut != "rows" else (wy1, f32(1) - wy1)
        G = np.zeros((N, d, 3, 18), dtype=np.float32)
        nn = np.arange(N)
        for wv in range(4):
            G[nn, :, ly0[:, wv]] += lo[:, wv, None, None] * VAL[:, :, wv]
            G[nn, :, ly0[:, wv] + 1] += hi[:, wv, None, None] * VAL[:, :, wv]
        gl = np.zeros((b, d, h, w), dtype=np.float32)
        np.add.at(gl, (T.bi[:, None, None, None], np.arange(d)[None, :, None, None], T.gy[:, None, :, None], T.gx[:, None, None, :]), G)
    assert gl.dtype == np.float32
    return gl


def run(shape, which, mut=None):
    """every output of the emulation; the backward pass reads what ITS forward saved, as the autograd function does"""
    lg, gout = SA.inputs(shape, which)
    out, stats = emu_fwd(lg, mut)
    return dict(out=out, stats=stats, saved=emu_bwd(lg, gout, stats, out, mut), recompute=emu_bwd(lg, gout, None, None, mut))


def ratios(shape, which, res):
    r = SA.check_forward(shape, which, res["out"], res["stats"])
    r["backward saved"] = SA.check_backward(shape, which, res["saved"])
    r["backward recompute"] = SA.check_backward(shape, which, res["recompute"])
    return r


@functools.lru_cache(maxsize=None)
def clean(shape, which):
    return run(shape, which)


# ---- the emulation passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SA.SHAPES, ids=str)
@pytest.mark.parametrize("which", SA.SETS)
def test_emulation_is_within_every_bound(shape, which):
    res = clean(shape, which)
    r = ratios(shape, which, res)
    print(shape, which, r)
    assert max(r.values()) <= 1.0, r
    if which in ("spike", "wide"):
        assert all(np.isfinite(t).all() for t in res.values())


def test_shape_list_reaches_every_feature():
    assert SA.WANT <= SA.features(), SA.WANT - SA.features()
    assert SA.features([(1, 4, 2, 16)]) == {"4w % 64 == 0", "b == 1"}
    for shape in SA.SHAPES:      # the hazard of the dead lanes is armed wherever there are dead lanes (asserted inside)
        SA.reference(shape, "wide")


def test_flat_gradient_sums_to_zero_per_pixel():
    """sum_D p_D (D - out) = 0: the planes' gradients of every cell cancel, in the reference and within the bounds"""
    for shape in SA.SHAPES:
        for which in SA.SETS:
            ref = SA.reference(shape, which)
            assert np.all(np.abs(ref["grad"].sum(1)) <= ref["grad_bound"].sum(1))
        assert np.all(np.abs(clean(shape, "flat")["saved"].astype(np.float64).sum(1)) <= SA.reference(shape, "flat")["grad_bound"].sum(1))


# ---- the reference is pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SA.SHAPES, ids=str)
def test_reference_against_float64_torch_and_the_oracle(shape):
    b, d, h, w = shape
    for which in ("plain", "wide"):
        lg, gout = SA.inputs(shape, which)
        ref = SA.reference(shape, which)
        x = torch.from_numpy(lg.astype(np.float64)).view(b, 1, d, h, w).requires_grad_()
        up = F.interpolate(x, scale_factor=4, mode="trilinear", align_corners=False)
        assert tuple(up.shape) == (b, 1, 4 * d, 4 * h, 4 * w)
        assert np.abs(up.detach().numpy()[:, 0] - ref["u"]).max() <= 1e-12 * max(1.0, np.abs(lg).max())
        prob = torch.softmax(up[:, 0], dim=1)
        out = (prob * torch.arange(4 * d, dtype=torch.float64).view(1, -1, 1, 1)).sum(1)
        (grad,) = torch.autograd.grad(out, x, torch.from_numpy(gout.astype(np.float64)))
        scale = max(1.0, float(np.abs(ref["grad"]).max()))
        assert np.abs(out.detach().numpy() - ref["out"]).max() <= 1e-10 * 4 * d
        assert np.abs(grad.numpy()[:, 0] - ref["grad"]).max() <= 1e-10 * scale
        orc = po.soft_argmin_head(x.detach(), 4 * d, 4 * h, 4 * w)
        assert np.abs(orc.numpy()[:, 0] - ref["out"]).max() <= 1e-10 * 4 * d
        lse = torch.logsumexp(up[:, 0].detach(), dim=1).numpy()            # M + log s does not depend on the shift
        assert np.abs(ref["M"] + np.log(ref["s"]) - lse).max() <= 1e-10 * max(1.0, np.abs(lse).max())


def test_closed_form_special_cases():
    for shape in SA.SHAPES:
        b, d, h, w = shape
        assert np.abs(SA.reference(shape, "flat")["out"] - (4 * d - 1) / 2).max() <= 1e-12 * d
        if d == 1:
            for which in SA.SETS:
                assert np.abs(SA.reference(shape, which)["out"] - 1.5).max() <= 1e-12
        if d >= 3:
            assert np.abs(SA.reference(shape, "spike")["out"] - (4 * SA.spike_plane(d) + 1.5)).max() <= 1e-9


# ---- the mutants are rejected -------------------------------------------------------------------------------------------------------
MUTANTS = {     # name -> (the shapes its class applies to, the input sets searched for a failing check)
    "phase_x": (lambda b, d, h, w: w > 1, ("plain",)),
    "phase_y": (lambda b, d, h, w: h > 1, ("plain",)),
    "phase_d": (lambda b, d, h, w: d > 1, ("plain",)),
    "zero_x": (lambda b, d, h, w: True, ("plain",)),
    "zero_y": (lambda b, d, h, w: True, ("plain",)),
    "zero_d": (lambda b, d, h, w: True, ("plain",)),
    "once": (lambda b, d, h, w: True, ("plain",)),
    "index": (lambda b, d, h, w: d > 1, ("plain",)),
    "planemax": (lambda b, d, h, w: d >= 3, ("spike",)),
    "fold": (lambda b, d, h, w: d > 1, ("plain",)),
    "rows": (lambda b, d, h, w: h > 1 and d > 1, ("plain",)),
    "halo_l": (lambda b, d, h, w: d > 1, ("plain",)),
    "halo_r": (lambda b, d, h, w: w >= 16 and d > 1, ("plain",)),
    "stats_s": (lambda b, d, h, w: True, ("flat",)),
    "dead_old": (lambda b, d, h, w: SA.dead_lanes(w), ("wide",)),
}
_MUTANT_CASES = [(m, s) for m in MUTANTS for s in SA.SHAPES if MUTANTS[m][0](*s)]


@pytest.mark.parametrize("mut,shape", _MUTANT_CASES, ids=[f"{m}-{s}" for m, s in _MUTANT_CASES])
def test_mutant_is_rejected(mut, shape):
    """on EVERY set listed for it: a set on which the mutant is only sometimes visible is not listed"""
    for which in MUTANTS[mut][1]:
        r = ratios(shape, which, run(shape, which, mut))
        assert max(r.values()) > 1.0, (mut, shape, which, r)


def test_every_mutant_class_is_exercised():
    for m, (applies, _) in MUTANTS.items():
        assert sum(applies(*s) for s in SA.SHAPES) >= 2, m


@pytest.mark.parametrize("shape", [s for s in SA.SHAPES if SA.dead_lanes(s[3])], ids=str)
def test_dead_lane_mutant_is_a_nan_in_the_last_column(shape):
    """the defect itself: on `wide` the old dead lanes put a NaN into column w - 1 of the saved-statistics gradient and nowhere
    else; the recompute path is immune; on `plain` the mutant is the same bits as the fixed emulation"""
    bad = run(shape, "wide", "dead_old")
    nan = np.isnan(bad["saved"])
    assert nan[..., -1].any() and not nan[..., :-1].any()
    assert np.isfinite(bad["recompute"]).all() and np.array_equal(bad["recompute"], clean(shape, "wide")["recompute"])
    assert np.array_equal(run(shape, "plain", "dead_old")["saved"], clean(shape, "plain")["saved"])


def test_planemax_mutant_is_the_same_bits_without_an_interior_spike():
    for shape in SA.SHAPES:
        if shape[1] <= 2:
            a, c = emu_fwd(SA.inputs(shape, "spike")[0]), emu_fwd(SA.inputs(shape, "spike")[0], "planemax")
            assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


# ---- what the entry points refuse, on the host ------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    """sa_check and the pointer rules run before the first HIP call: safe without a GPU.  d == 83 does not fit the backward
    kernel's LDS; d == 82 (in the shape list) is the last depth that does"""
    from activezero_amd import _lib, build
    build.build()
    lib = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, EUNSUPPORTED = _lib.CONST["AZ_EINVAL"], _lib.CONST["AZ_EUNSUPPORTED"]
    assert (54 + 144) * 4 * SA.MAX_D <= 64 * 1024 < (54 + 144) * 4 * (SA.MAX_D + 1)
    assert lib.az_softargmin_fwd(p, p, p, 1, SA.MAX_D + 1, 1, 3, None) == EUNSUPPORTED
    assert lib.az_softargmin_bwd(p, p, p, None, None, 1, SA.MAX_D + 1, 1, 3, None) == EUNSUPPORTED
    assert lib.az_softargmin_bwd(p, p, p, p, p, 1, SA.MAX_D + 1, 1, 3, None) == EUNSUPPORTED
    assert lib.az_softargmin_bwd(p, p, p, p, None, 1, 4, 1, 3, None) == EINVAL
    assert lib.az_softargmin_bwd(p, p, p, None, p, 1, 4, 1, 3, None) == EINVAL
    assert lib.az_softargmin_fwd(p, None, p, 1, 0, 1, 3, None) == EINVAL
