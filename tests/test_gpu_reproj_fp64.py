"""GPU: the reprojection-loss kernels -- K7 az_warp_gather.hip, K8 az_patch_reproj.hip (forward, backward, Fold), K9 az_lcn.hip --
against fp64, element-wise and per route.

The kernels are called through the C ABI; every output lies inside a larger buffer filled with a NaN sentinel: every output
element must be written, nothing around the output may be (grad_img is accumulated into: it starts as zeros between the
guards).  The references are those of tests/_reproj_fp64ref.py: the kernels' own fp32 sampling coordinate restated step by step,
fp64 after it, and bounds that count the roundings of the kernel's expression.  Every check is a ratio err / bound <= 1.0 over
every element; tests/test_reproj_error_model_cpu.py shows that these checks reject the defects they are meant to see.

K8's forward leaves the GPU as two numbers, so a pixel's value is seen through a launch whose mask selects that pixel alone:
acc[0] is its sum of squares, acc[1] exactly C ps^2 -- every pixel of the small shapes; of the larger ones the first and last
row of the first, a middle and the last band, and 64 seeded pixels.  test_every_route restates the dispatch (PSM from ps, PR_K 4
forward / 2 backward, band rows from pr_band_rows, tiled or per-pixel from that and AZ_PATCH_TILED) and asserts that the shape
list reaches every branch; under AZ_PATCH_TILED=0 (tests/test_gpu_switches.py) that every K8 case is per-pixel."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, ops  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from activezero_amd.utils import reprojection  # noqa: E402
from tests import _reproj_fp64ref as RP  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x7FC0BEEF  # a NaN with a payload no arithmetic produces
GUARD = 4096
WORST = {}  # (kernel, route, check) -> largest ratio
K8_ALL = RP.K8_SHAPES + [RP.K8_STRIDE_CASE]


@functools.lru_cache(maxsize=None)
def tiled_enabled():
    return _lib.lib().az_option(b"AZ_PATCH_TILED") != 0


def note(kernel, route, check, r, capsys, what=""):
    key = (kernel, route, check)
    WORST[key] = max(WORST.get(key, 0.0), r)
    with capsys.disabled():
        print(f"\nreproj {kernel} {route} {check} {what}: {r:.4f}")
    return r


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """a float32 output of `shape` inside a buffer of NaN sentinels (GUARD elements before and after it), 16-byte aligned as a
    tensor of its own would be; zero=True: an output that is accumulated into starts as zeros"""

    def __init__(self, shape, zero=False):
        n = int(np.prod(shape))
        self.n, self.zero = n, zero
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        if zero:
            self.buf[GUARD:GUARD + n] = 0
        self.out = self.buf[GUARD:GUARD + n].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 0

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())

    def settle(self):
        """the guards are untouched and every output element was written; returns the output as numpy"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all()), "guard band written"
        inner = self.buf[GUARD:GUARD + self.n]
        if not self.zero:
            assert not bool((inner == SENTINEL).any()), f"{int((inner == SENTINEL).sum())} output elements not written"
        return self.out.cpu().numpy()


# ---- route coverage -------------------------------------------------------------------------------------------------------------
def k8_label(shape, which):
    rt = RP.k8_route(shape, which, tiled_enabled())
    if not rt["tiled"]:
        return "per-pixel"
    return f"tiled PSM {rt['psm']} " + ("one-row bands" if rt["tr"] == 1 else "multi-row bands")


def test_every_route(capsys):
    on = tiled_enabled()
    feats = RP.k8_route_features(K8_ALL, on)
    with capsys.disabled():
        print()
        for s in K8_ALL:
            print(f"K8 {s}: fwd {RP.k8_route(s, 'fwd', on)} bwd {RP.k8_route(s, 'bwd', on)}")
        print("reached:", sorted(feats))
    if on:
        assert RP.K8_WANT <= feats, RP.K8_WANT - feats
    else:
        assert "per-pixel by switch" in feats and not any(f.startswith(("PSM", "tr ")) for f in feats)
        assert all(k8_label(s, w) == "per-pixel" for s in K8_ALL for w in ("fwd", "bwd"))
        assert RP.K8_STRIDE_CASE[2] * RP.K8_STRIDE_CASE[3] > RP.GRID_THREADS          # the per-pixel kernel's grid-stride loop
    assert {"W % 4 != 0", "W % 2 != 0", "C > 1", "window larger than the image"} <= feats
    assert any(b * h * w > RP.GRID_THREADS for b, c, h, w in RP.K7_SHAPES)             # K7's grid-stride loop
    assert any(h % 16 and w % 16 and h > 16 and w > 16 for b, c, h, w, k in RP.K9_SHAPES)  # K9: a partial tile on both axes


# ---- K7 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k7_reference(shape, which):
    img, disp, gout = RP.k7_inputs(shape, which)
    return RP.warp_fwd(img, disp), RP.warp_bwd(gout, img, disp)


def k7_route(shape):
    return "grid-stride" if shape[0] * shape[2] * shape[3] > RP.GRID_THREADS else "one pass"


@pytest.mark.parametrize("shape", RP.K7_SHAPES, ids=str)
@pytest.mark.parametrize("which", RP.SETS)
def test_k7_forward_and_gradients(shape, which, capsys):
    B, C, H, W = shape
    img, disp, gout = RP.k7_inputs(shape, which)
    if B * H * W >= 40:
        assert RP.classes_of(disp, H, W) == set(RP.CLASSES)
    (ref, mag), ((gdr, gdm), (gir, gim, gic)) = k7_reference(shape, which)
    img_d, disp_d, gout_d = dev(img), dev(disp), dev(gout)
    out, gd, gi, gd0 = Guarded(shape), Guarded((B, H, W)), Guarded(shape, zero=True), Guarded((B, H, W))
    with torch.cuda.device(DEV):
        _call("az_warp_gather_fwd", _p(out.out), _p(img_d), _p(disp_d), B, C, H, W, _stream())
        _call("az_warp_gather_bwd", _p(gd.out), _p(gi.out), _p(gout_d), _p(img_d), _p(disp_d), B, C, H, W, _stream())
        _call("az_warp_gather_bwd", _p(gd0.out), None, _p(gout_d), _p(img_d), _p(disp_d), B, C, H, W, _stream())
    out, gd, gi, gd0 = out.settle(), gd.settle(), gi.settle(), gd0.settle()
    rt = k7_route(shape)
    rs = [note("K7", rt, "forward", RP.ratio(out, ref, RP.warp_fwd_bound(mag)), capsys, f"{shape} {which}"),
          note("K7", rt, "grad_disp", RP.ratio(gd, gdr, RP.warp_gdisp_bound(gdm, C)), capsys, f"{shape} {which}"),
          note("K7", rt, "grad_img", RP.ratio(gi, gir, RP.warp_gimg_bound(gim, gic)), capsys, f"{shape} {which}")]
    assert np.array_equal(gd.view(np.uint32), gd0.view(np.uint32))   # grad_disp: the same bits with and without grad_img
    if which == "zero":
        assert not out.any() and not gd.any()
    assert max(rs) <= 1.0, rs


def test_k7_refuses_a_single_row_or_column():
    code = _lib.CONST["AZ_EINVAL"]
    lib = _lib.lib()
    src = dev(np.ones(64, dtype=np.float32))
    for H, W in ((1, 8), (8, 1)):
        outs = [Guarded((1, 1, H, W)) for _ in range(3)]
        with torch.cuda.device(DEV):
            assert lib.az_warp_gather_fwd(_p(outs[0].out), _p(src), _p(src), 1, 1, H, W, _stream()) == code
            assert lib.az_warp_gather_bwd(_p(outs[1].out), _p(outs[2].out), _p(src), _p(src), _p(src), 1, 1, H, W, _stream()) == code
        assert all(o.untouched() for o in outs)


def test_k7_through_autograd(capsys):
    shape, which = (2, 3, 5, 8), "seeded"
    B, C, H, W = shape
    img, disp, gout = RP.k7_inputs(shape, which)
    (ref, mag), ((gdr, gdm), (gir, gim, gic)) = k7_reference(shape, which)
    rs = []
    for img_grad in (False, True):
        x, d = dev(img).requires_grad_(img_grad), dev(disp).view(B, 1, H, W).requires_grad_()
        out = reprojection.apply_disparity(x, d)
        out.backward(dev(gout))
        rs.append(note("K7", "autograd", "forward", RP.ratio(out.detach().cpu().numpy(), ref, RP.warp_fwd_bound(mag)), capsys))
        rs.append(note("K7", "autograd", "grad_disp", RP.ratio(d.grad.cpu().numpy()[:, 0], gdr, RP.warp_gdisp_bound(gdm, C)), capsys))
        if img_grad:
            rs.append(note("K7", "autograd", "grad_img", RP.ratio(x.grad.cpu().numpy(), gir, RP.warp_gimg_bound(gim, gic)), capsys))
        else:
            assert x.grad is None
    assert max(rs) <= 1.0, rs


# ---- K8 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k8_reference(shape, which, sign):
    L, R, disp = RP.k8_inputs(shape, which)
    return RP.patch_pixel(L, R, disp, shape[4], sign)


@functools.lru_cache(maxsize=None)
def k8_device(shape, which):
    return tuple(dev(t) for t in RP.k8_inputs(shape, which))


def k8_fwd(shape, L, R, disp, mask, sign, acc=None):
    B, C, H, W, ps = shape
    acc = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV) if acc is None else acc
    with torch.cuda.device(DEV):
        _call("az_patch_reproj_fwd", _p(acc), _p(L), _p(R), _p(disp), _p(mask), B, C, H, W, ps, float(sign), _stream())
    return acc


def k8_bwd(shape, L, R, disp, mask, sign, acc, gloss):
    B, C, H, W, ps = shape
    g = Guarded((B, H, W))
    gl = torch.tensor([gloss], dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _call("az_patch_reproj_bwd", _p(g.out), _p(gl), _p(acc), _p(L), _p(R), _p(disp), _p(mask), B, C, H, W, ps, float(sign),
              _stream())
    return g.settle()


_PIXEL_CASES = [(s, w, sg) for s in K8_ALL for w, sg in (("seeded", -1.0), ("seeded", 1.0), ("binary", -1.0), ("zero", -1.0))]


@pytest.mark.parametrize("shape,which,sign", _PIXEL_CASES, ids=[f"{s}-{w}-{sg:+.0f}" for s, w, sg in _PIXEL_CASES])
def test_k8_forward_per_pixel(shape, which, sign, capsys):
    """one launch per pixel, each with a mask that selects that pixel and an acc slot of its own; one synchronisation"""
    B, C, H, W, ps = shape
    L, R, disp = k8_device(shape, which)
    if sign > 0 and B * H * W >= 40:
        assert RP.classes_of(RP.k8_inputs(shape, which)[2], H, W) == set(RP.CLASSES)
    bb, ii, jj = RP.k8_sample(shape, tiled_enabled())
    n, npix = len(bb), B * H * W
    flat = (bb * H + ii) * W + jj
    masks = torch.zeros((n, npix), dtype=torch.uint8, device=DEV)
    masks[torch.arange(n, device=DEV), dev(flat)] = 1
    acc = torch.full((n, 2), float("nan"), dtype=torch.float64, device=DEV)
    lib = _lib.lib()
    with torch.cuda.device(DEV):
        s = _stream()
        for k in range(n):
            code = lib.az_patch_reproj_fwd(acc.data_ptr() + 16 * k, _p(L), _p(R), _p(disp), masks.data_ptr() + npix * k,
                                           B, C, H, W, ps, float(sign), s)
            assert code == 0, code
    torch.cuda.synchronize()
    pp = {k: v[flat] for k, v in k8_reference(shape, which, sign).items()}
    r = note("K8", k8_label(shape, "fwd"), "forward, per pixel", RP.k8_check_pixels(acc.cpu().numpy(), pp, C, ps), capsys,
             f"{shape} {which} {sign:+.0f} ({n} pixels)")
    assert r <= 1.0


_FULL_CASES = [(s, w, sg) for s in K8_ALL for w, sg in (("seeded", -1.0), ("seeded", 1.0), ("binary", -1.0), ("zero", 1.0))]


@pytest.mark.parametrize("shape,which,sign", _FULL_CASES, ids=[f"{s}-{w}-{sg:+.0f}" for s, w, sg in _FULL_CASES])
def test_k8_full_forward_and_backward(shape, which, sign, capsys):
    B, C, H, W, ps = shape
    L, R, disp = k8_device(shape, which)
    pp = k8_reference(shape, which, sign)
    rs = []
    for mk in ("none", "random", "zero"):
        mask = RP.k8_mask(shape, mk)
        mask_d = None if mask is None else dev(mask)
        acc = k8_fwd(shape, L, R, disp, mask_d, sign)
        acc_h = acc.cpu().numpy()
        what = f"{shape} {which} {sign:+.0f} mask {mk}"
        rs.append(note("K8", k8_label(shape, "fwd"), "forward, full", RP.k8_check_full(acc_h, pp, mask, shape, tiled_enabled()),
                       capsys, what))
        for gloss in (1.0, 3.0, -0.5):
            grad = k8_bwd(shape, L, R, disp, mask_d, sign, acc, gloss)
            rs.append(note("K8", k8_label(shape, "bwd"), "grad_disp", RP.k8_check_grad(grad, pp, mask, gloss, shape, sign), capsys,
                           f"{what} gloss {gloss}"))
            if mk == "zero":
                assert acc_h[0] == 0 and acc_h[1] == 0 and not grad.view(np.uint32).any()
            if which == "zero":
                assert not grad.any()
    assert max(rs) <= 1.0, rs


@pytest.mark.parametrize("shape", [(2, 2, 6, 7, 5), (1, 1, 16, 17, 15), (3, 1, 87, 7, 3), (1, 1, 2, 1245, 15)], ids=str)
def test_k8_disparities_under_masked_pixels_do_not_matter(shape):
    B, C, H, W, ps = shape
    L, R, disp = k8_device(shape, "seeded")
    mask = RP.k8_mask(shape, "random")
    dead = np.flatnonzero(mask.reshape(-1) == 0)
    assert len(dead) >= 5
    clean = RP.k8_inputs(shape, "seeded")[2].copy().reshape(-1)
    clean[dead] = 0.0
    wild = clean.copy()
    wild[dead] = np.resize(np.array([1e30, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32), len(dead))
    mask_d = dev(mask)
    got = []
    for d in (clean, wild):
        d_d = dev(d.reshape(B, H, W))
        acc = k8_fwd(shape, L, R, d_d, mask_d, -1.0)
        got.append((acc.cpu().numpy(), k8_bwd(shape, L, R, d_d, mask_d, -1.0, acc, 3.0)))
    assert np.array_equal(got[0][0], got[1][0]) and np.isfinite(got[0][0]).all()
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    assert not got[1][1].reshape(-1)[dead].view(np.uint32).any()     # +0 bit for bit


@pytest.mark.parametrize("shape", RP.K8_SMALL + [RP.K8_BANDS[0]], ids=str)
def test_k8_fold(shape, capsys):
    B, C, H, W, ps = shape
    rs = []
    for which, sign in (("seeded", -1.0), ("seeded", 1.0), ("zero", -1.0)):
        _, R, disp = k8_device(shape, which)
        vis = Guarded((B, C, H, W))
        with torch.cuda.device(DEV):
            _call("az_patch_reproj_vis", _p(vis.out), _p(R), _p(disp), B, C, H, W, ps, float(sign), _stream())
        got = vis.settle()
        ref, mag = RP.patch_vis(RP.k8_inputs(shape, which)[1], RP.k8_inputs(shape, which)[2], ps, sign)
        rs.append(note("K8", "fold", "vis", RP.ratio(got, ref, RP.vis_bound(mag, ps)), capsys, f"{shape} {which} {sign:+.0f}"))
        if which == "zero":
            assert not got.any()
    assert max(rs) <= 1.0, rs


def test_k8_through_autograd(capsys):
    shape, which = (2, 2, 6, 7, 5), "seeded"
    B, C, H, W, ps = shape
    L, R, disp = k8_device(shape, which)
    mask = RP.k8_mask(shape, "random")
    pp = k8_reference(shape, which, -1.0)
    d = disp.view(B, 1, H, W).clone().requires_grad_()
    loss, vis, mask_out = reprojection.get_reproj_error_patch(L, R, d, dev(mask).view(B, 1, H, W).bool(), ps)
    (3 * loss).backward()
    live = mask.reshape(-1) != 0
    n = float(live.sum()) * C * ps * ps
    ref = pp["ssd"][live].sum() / n
    bound = (pp["fwd_bound"][live].sum() + RP.SECOND * RP.k8_chain(shape, tiled_enabled()) * RP.U * pp["ssd"][live].sum()) / n
    rs = [note("K8", "autograd", "loss", RP.ratio(float(loss.detach()), ref, bound + RP.U * ref), capsys),
          note("K8", "autograd", "grad_disp", RP.k8_check_grad(d.grad.cpu().numpy(), pp, mask, 3.0, shape, -1.0), capsys)]
    vref, vmag = RP.patch_vis(RP.k8_inputs(shape, which)[1], RP.k8_inputs(shape, which)[2], ps, -1.0)
    rs.append(note("K8", "autograd", "vis", RP.ratio(vis.cpu().numpy(), vref, RP.vis_bound(vmag, ps)), capsys))
    assert tuple(mask_out.shape) == (B, C, H, W) and np.array_equal(mask_out.cpu().numpy()[:, 0].reshape(-1) != 0, live)
    assert max(rs) <= 1.0, rs


# ---- K9 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k9_reference(shape, which):
    return RP.lcn(RP.k9_input(shape, which)[:, 0], shape[4], 1e-5)


@pytest.mark.parametrize("shape", RP.K9_SHAPES, ids=str)
@pytest.mark.parametrize("which", RP.K9_SETS)
def test_k9(shape, which, capsys):
    """through ops.local_contrast_norm: the batch stride is C H W, and the channels past the first (NaN here) are never read"""
    B, C, H, W, k = shape
    normed, sd = ops.local_contrast_norm(dev(RP.k9_input(shape, which)), k, 1e-5)
    assert tuple(normed.shape) == tuple(sd.shape) == (B, 1, H, W)
    normed, sd = normed.cpu().numpy()[:, 0], sd.cpu().numpy()[:, 0]
    ref = k9_reference(shape, which)
    rt = "partial tiles" if (H % 16 or W % 16) else "full tiles"
    rs = [note("K9", rt, "std", RP.ratio(sd, ref["sd"], ref["sd_bound"]), capsys, f"{shape} {which}"),
          note("K9", rt, "normed", RP.ratio(normed, ref["normed"], ref["normed_bound"]), capsys, f"{shape} {which}")]
    if k == 1:
        assert not sd.any() and not normed.any()
    if which == "flat":
        inside = RP.k9_flat_inside(shape)
        assert not sd[:, inside].any() and not normed[:, inside].any()
    assert max(rs) <= 1.0, rs


def test_k9_refuses_a_window_that_does_not_fit():
    src = dev(np.ones((5, 7), dtype=np.float32))
    outs = [Guarded((5, 7)) for _ in range(2)]
    with torch.cuda.device(DEV):
        code = _lib.lib().az_lcn(_p(outs[0].out), _p(outs[1].out), _p(src), 1, 5, 7, 115, 1e-5, 35, _stream())
    assert code == _lib.CONST["AZ_EUNSUPPORTED"]
    assert all(o.untouched() for o in outs)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_zz_largest_ratios(capsys):
    """the table of tests/_reproj_fp64ref.py: the largest ratio of each check per kernel and route over the cases run"""
    with capsys.disabled():
        print()
        for (kernel, route, check), w in sorted(WORST.items()):
            print(f"reproj worst {kernel:3s} {route:32s} {check:20s} {w:.2f}")
    assert all(w <= 1.0 for w in WORST.values())
