"""CPU (no GPU): what the checks of tests/_volume_fp64ref.py accept and what they reject.

Emulations: for each kernel of az_cost_volume.hip, az_costconv.hip and az_spp.hip an fp32 numpy restatement of its index
arithmetic on FLAT buffers (as the kernel addresses them) and of its summation order.  Each passes its check, ratio <= 1.0, on
every shape of the GPU sweep that is small enough for the CPU.

Mutants: the same emulations with one listed defect each.  Every one must fail its check (ratio > 1.0, or other bits where the
check is bit equality) on a shape of the sweep -- but for the doubled tap counted once, which shows only where the last
position rounds above the last index by more than the bound of a short tree: that test finds such a pair itself.

Pins: the closed-form references against the oracle, torch's conv3d of the materialised volume and torch's own fp64
interpolation and autograd."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _volume_fp64ref as V

F32 = np.float32


def fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in fp64"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def take(flat, idx):
    """a flat load; an address outside the buffer (a mutant's) reads the nearest end"""
    return np.take(flat, idx, mode="clip")


# ==== K3 ==========================================================================================================================
def emu_k3_fwd(fl, fr, d, layout, strict=False, shift=True):
    L, R = V.bits(fl), V.bits(fr)
    w = L.shape[3] if layout == "ncdhw" else L.shape[2]
    ax = 3 if layout == "ncdhw" else 2
    x = np.arange(w)
    planes = []
    for i in range(d):
        on = (x > i) if strict else (x >= i)
        src = np.clip(x - i if shift else x, 0, w - 1)
        on = on.reshape([-1 if a == ax else 1 for a in range(4)])
        halves = [np.where(on, L, 0), np.where(on, np.take(R, src, axis=ax), 0)]
        planes.append(np.concatenate(halves, axis=1 if layout == "ncdhw" else 3))
    return np.stack(planes, axis=2 if layout == "ncdhw" else 1).view(F32)


def emu_k3_bwd(g, d, layout, lim=-1, edge=-1, shifted=True):
    """in-order fp32 sums over flat addresses; lim / edge: the limits min(d + lim, x) and min(d + lim, w + edge - x)"""
    g = np.asarray(g)
    if layout == "ncdhw":
        b, c2, _, h, w = g.shape
        c = c2 // 2
        B, C2, Y, X = np.meshgrid(np.arange(b), np.arange(c2), np.arange(h), np.arange(w), indexing="ij")
        addr = lambda i, xx: ((B * c2 + C2) * d + i) * h * w + Y * w + xx
    else:
        b, _, h, w, c2 = g.shape
        c = c2 // 2
        B, Y, X, C2 = np.meshgrid(np.arange(b), np.arange(h), np.arange(w), np.arange(c2), indexing="ij")
        addr = lambda i, xx: ((((B * d + i) * h + Y) * w) + xx) * c2 + C2
    flat = g.reshape(-1)
    right = C2 >= c
    last = np.where(right, np.minimum(d + lim, w + edge - X), np.minimum(d + lim, X))
    acc = np.zeros(B.shape, dtype=F32)
    for i in range(int(last.max()) + 1):
        t = take(flat, addr(i, np.where(right & shifted, X + i, X)))
        acc = np.where(i <= last, acc + t, acc)
    halves = np.split(acc, 2, axis=1 if layout == "ncdhw" else 3)
    return halves[0], halves[1]


K3_CPU = [(c, "ncdhw") for c in V.K3_NCDHW] + [(c, "ndhwc") for c in V.K3_NDHWC + [V.K3_NDHWC_FWD_WALK]]


@pytest.mark.parametrize("case,layout", K3_CPU, ids=str)
@pytest.mark.parametrize("which", ["plain", "exact", "bits"])
def test_k3_emulation_passes(case, layout, which):
    fl, fr, g = V.k3_inputs(case, layout, which)
    assert V.k3_check_forward(case, layout, which, emu_k3_fwd(fl, fr, case[1], layout)) == 0.0
    if which != "bits":
        assert V.k3_check_backward(case, layout, which, *emu_k3_bwd(g, case[1], layout)) <= 1.0


def test_k3_zero_region_is_plus_zero_and_specials_survive():
    case = V.K3_NCDHW[0]
    fl, fr, _ = V.k3_inputs(case, "ncdhw", "bits")
    ref = V.bits(V.k3_reference(case, "ncdhw", "bits")["cost"])
    (b, c, h, w), d = case
    for i in range(d):
        assert not ref[:, :, i, :, :i].any()
    assert set(np.unique(V.bits(fl)).tolist()) <= set(np.unique(ref).tolist()) | {0}
    assert {np.int32(np.uint32(s).astype(np.int32)) for s in V.SPECIALS} <= set(np.unique(ref).tolist())


K3_MUTANTS = {
    "mask x > i": dict(fwd=dict(strict=True)),
    "right half not shifted": dict(fwd=dict(shift=False)),
    "gradient limits d": dict(bwd=dict(lim=0)),
    "gradient limits w - x": dict(bwd=dict(edge=0)),
    "right gradient reads column x": dict(bwd=dict(shifted=False)),
}


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
@pytest.mark.parametrize("name", K3_MUTANTS)
@pytest.mark.parametrize("which", ["plain", "exact"])
def test_k3_mutant_fails(name, layout, which):
    case = V.K3_NCDHW[0] if layout == "ncdhw" else V.K3_NDHWC[0]
    fl, fr, g = V.k3_inputs(case, layout, which)
    m = K3_MUTANTS[name]
    if "fwd" in m:
        assert V.k3_check_forward(case, layout, which, emu_k3_fwd(fl, fr, case[1], layout, **m["fwd"])) > 1.0
    else:
        assert V.k3_check_backward(case, layout, which, *emu_k3_bwd(g, case[1], layout, **m["bwd"])) > 1.0


@pytest.mark.parametrize("case", V.K3_NCDHW[:2] + [V.K3_NCDHW[4]], ids=str)
def test_k3_reference_is_the_oracle(case):
    from oracle import psmnet_oracle as po
    (b, c, h, w), d = case
    fl, fr, g = V.k3_inputs(case, "ncdhw", "plain")
    ref = V.k3_reference(case, "ncdhw", "plain")
    tl, tr = (torch.from_numpy(t.copy()).double().requires_grad_() for t in (fl, fr))
    vol = po.build_cost_volume(tl, tr, d)
    assert np.array_equal(vol.detach().numpy(), ref["cost"].astype(np.float64))
    vol.backward(torch.from_numpy(g.copy()).double())
    assert np.allclose(tl.grad.numpy(), ref["gl"], rtol=1e-14, atol=1e-14) and np.allclose(tr.grad.numpy(), ref["gr"], rtol=1e-14, atol=1e-14)
    # the channels-last reference is the same volume, permuted
    cl = lambda t: np.ascontiguousarray(np.moveaxis(t, 1, -1))
    assert V.same_bits(V.k3_forward_ref(cl(fl), cl(fr), d, "ndhwc"), cl(ref["cost"]))
    gl, gr, bl, br = V.k3_backward_ref(cl(g), d, "ndhwc")
    assert np.array_equal(gl, cl(ref["gl"])) and np.array_equal(br, cl(ref["br"]))


# ==== assemble ====================================================================================================================
def kernel_class(d, D):
    return np.where((D == 1) | (d == 0), 0, np.where(d == D - 1, 1 if D == 2 else 2, 1))


def class_wrong_at_2(d, D):        # the D == 2 special case forgotten: the last of two planes becomes class 2
    return np.where((D == 1) | (d == 0), 0, np.where(d == D - 1, 2, 1))


def class_wrong_at_3(d, D):        # the last plane taken for a middle one when there is a middle one
    return np.where((D == 1) | (d == 0), 0, np.where((d == D - 1) & (D == 2), 1, 1))


def emu_asm_fwd(fb, fe, g, D, cut=-2, cls=kernel_class, use_xb=True, slot=2, fe_stride=None, g_stride=None):
    B, H, W, _ = fb.shape
    nc, xe = V.num_classes(D), V.edge_width(D, W)
    fe_stride = xe if fe_stride is None else fe_stride
    g_stride = W + 2 if g_stride is None else g_stride
    b, d, y, x, c = np.meshgrid(np.arange(B), np.arange(D), np.arange(H), np.arange(W), np.arange(32), indexing="ij")
    delta = x - d
    k = cls(d, D)
    f = np.where(delta >= 2, take(fb.reshape(-1), ((b * H + y) * W + x) * (nc * 32) + k * 32 + c),
                 take(fe.reshape(-1), ((b * H + y) * fe_stride + x) * (nc * 128) + (k * 4 + delta + slot) * 32 + c))
    xb = (x == W - 1) & use_xb
    gg = take(g.reshape(-1), ((b * H + y) * g_stride + delta + 2) * (nc * 64) + (k * 2 + xb) * 32 + c)
    return np.where(delta >= cut, f + gg, F32(0))


def emu_asm_bwd(gy, D, dmax=-2, d_lo_zero=False):
    B, _, H, W, _ = gy.shape
    nc, xe = V.num_classes(D), V.edge_width(D, W)
    flat = np.asarray(gy).reshape(-1)
    at = lambda b, d, y, x, c: (((b * D + d) * H + y) * W + x) * 32 + c
    # grad_f
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(32), indexing="ij")
    bulk = np.zeros((B, H, W, nc, 32), dtype=F32)
    for d in range(D):
        k = int(kernel_class(np.int64(d), D))
        t = take(flat, at(b, d, y, x, c))
        bulk[:, :, :, k] = np.where(d <= np.minimum(D - 1, x + dmax), bulk[:, :, :, k] + t, bulk[:, :, :, k])
    edge = np.full((B, H, xe, nc, 4, 32), np.nan, dtype=F32)
    for k in range(nc):
        for dl in range(4):
            d = x - (dl - 2)
            on = (d >= 0) & (d < D) & (kernel_class(np.clip(d, 0, D - 1), D) == k)
            edge[:, :, :, k, dl] = np.where(on, take(flat, at(b, d, y, x, c)), F32(0))[:, :, :xe]
    # grad_g
    b, y, t_, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W + 2), np.arange(32), indexing="ij")
    u = t_ - 2
    lo, hi = (0 if d_lo_zero else np.maximum(0, -u)), np.minimum(D - 1, W - 1 - u)
    acc = np.zeros((B, H, W + 2, nc, 2, 32), dtype=F32)
    for d in range(D):
        x = u + d
        k = int(kernel_class(np.int64(d), D))
        v = take(flat, at(b, d, y, x, c))
        for e in range(2):
            on = (d >= lo) & (d <= hi) & ((x == W - 1) == bool(e))
            acc[:, :, :, k, e] = np.where(on, acc[:, :, :, k, e] + v, acc[:, :, :, k, e])
    return bulk.reshape(B, H, W, nc * 32), edge.reshape(B, H, xe, nc * 128), acc.reshape(B, H, W + 2, nc * 64)


@pytest.mark.parametrize("shape", V.ASM_SHAPES, ids=str)
@pytest.mark.parametrize("which", ["plain", "exact"])
def test_assemble_emulation_passes(shape, which):
    fb, fe, g, gy = V.asm_inputs(shape, which)
    assert V.asm_check_forward(shape, which, emu_asm_fwd(fb, fe, g, shape[3])) == 0.0
    r = V.asm_check_backward(shape, which, *emu_asm_bwd(gy, shape[3]))
    assert max(r.values()) <= 1.0, r


ASM_FWD_MUTANTS = {
    "cut at delta >= -1": (dict(cut=-1), (2, 3, 9, 5)),
    "class of the last plane at D = 2": (dict(cls=class_wrong_at_2), (2, 3, 9, 2)),
    "class of the last plane at D = 3": (dict(cls=class_wrong_at_3), (2, 3, 9, 3)),
    "xb ignored": (dict(use_xb=False), (2, 3, 9, 3)),
    "edge slot off by one": (dict(slot=1), (2, 3, 9, 3)),
    "F_edge row stride W": (dict(fe_stride=9), (2, 3, 9, 3)),
    "G row stride W": (dict(g_stride=9), (2, 3, 9, 3)),
}


@pytest.mark.parametrize("name", ASM_FWD_MUTANTS)
@pytest.mark.parametrize("which", ["plain", "exact"])
def test_assemble_forward_mutant_fails(name, which):
    opts, shape = ASM_FWD_MUTANTS[name]
    fb, fe, g, _ = V.asm_inputs(shape, which)
    assert V.asm_check_forward(shape, which, emu_asm_fwd(fb, fe, g, shape[3], **opts)) > 1.0


@pytest.mark.parametrize("opts,victim", [(dict(dmax=-1), "dF_bulk"), (dict(d_lo_zero=True), "dG")], ids=str)
@pytest.mark.parametrize("which", ["plain", "exact"])
def test_assemble_backward_mutant_fails(opts, victim, which):
    shape = (2, 3, 9, 3)
    r = V.asm_check_backward(shape, which, *emu_asm_bwd(V.asm_inputs(shape, which)[3], shape[3], **opts))
    assert r[victim] > 1.0, r


def test_assemble_reference_demands_every_element():
    """an element the kernel never wrote (a NaN sentinel on the GPU) fails each of the three checks"""
    shape = (1, 2, 4, 8)
    outs = [t.copy() for t in emu_asm_bwd(V.asm_inputs(shape, "plain")[3], shape[3])]
    for k, name in enumerate(("dF_bulk", "dF_edge", "dG")):
        bad = [t.copy() for t in outs]
        bad[k].reshape(-1)[-1] = np.nan
        assert V.asm_check_backward(shape, "plain", *bad)[name] == np.inf


@pytest.mark.parametrize("dims", [(1, 4, 9, 4), (2, 3, 7, 3), (1, 3, 6, 2), (1, 2, 5, 1), (1, 3, 4, 7)], ids=str)
def test_assemble_map_is_conv3d_of_the_volume(dims):
    """as tests/test_costconv_cpu.py, with asm_map in the place of its _assemble"""
    from activezero_amd import costconv
    from oracle import psmnet_oracle as po
    from tests._weights import seeded
    b, h, w, nd = dims
    fl, fr = seeded((b, 32, h, w), 1), seeded((b, 32, h, w), 2)
    wt = seeded((32, 64, 3, 3, 3), 3, -0.1, 0.1)
    ref = F.conv3d(po.build_cost_volume(fl, fr, nd), wt, padding=1)
    kb, ke, kr = costconv._merged_kernels(wt, nd)
    xe = V.edge_width(nd, w)
    rows = lambda t: np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())
    fb = rows(F.conv2d(fl, kb, padding=1))
    fe = rows(F.conv2d(fl[..., :min(w, xe + 1)], ke, padding=1)[..., :xe])
    g = rows(F.conv2d(F.pad(fr, (2, 0)), kr, padding=(1, 2)))
    assert tuple(t.shape for t in (fb, fe, g)) == V.asm_shapes((b, h, w, nd))[:3]
    out = torch.from_numpy(V.asm_forward_ref(fb, fe, g, nd)).permute(0, 4, 1, 2, 3)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5), float((out - ref).abs().max())


# ==== merge =======================================================================================================================
def emu_merge_fwd(w, ml, mr, transposed=False, offset=32 * 27, so=64 * 27):
    ncls = ml.shape[0]
    wf = np.asarray(w).reshape(-1)
    outs = []
    for J, m, nce, off in ((0, ml, ncls * 5, 0), (5, mr, ncls * 2, offset)):
        L = J or 3
        mf = np.asarray(m).reshape(-1)
        ce, o, i, h, l = np.meshgrid(np.arange(nce), np.arange(32), np.arange(32), np.arange(3), np.arange(L), indexing="ij")
        base = off + o * so + i * 27 + h * 3
        acc = np.zeros(ce.shape, dtype=F32)
        for d in range(3):
            if J:
                for x in range(3):
                    mi = ((ce * 3 + x) * 3 + d) if transposed else ((ce * 3 + d) * 3 + x)
                    acc = acc + take(wf, base + d * 9 + x) * take(mf, mi * J + l)
            else:
                mi = ((ce * 3 + l) * 3 + d) if transposed else ((ce * 3 + d) * 3 + l)
                acc = acc + take(wf, base + d * 9 + l) * take(mf, mi)
        outs.append(acc)
    return outs[0].reshape(ncls, 5, 32, 32, 3, 3), outs[1].reshape(ncls, 2, 32, 32, 3, 5)


def emu_merge_bwd(gkl, gkr, ml, mr, transposed=False, offset=32 * 27, so=64 * 27):
    ncls = ml.shape[0]
    gw = np.full(32 * 64 * 27, np.nan, dtype=F32)
    o, i, d, h, x = np.meshgrid(np.arange(32), np.arange(32), np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    for J, g, m, nce, off in ((0, gkl, ml, ncls * 5, 0), (5, gkr, mr, ncls * 2, offset)):
        L = J or 3
        gf, mf = np.asarray(g).reshape(-1), np.asarray(m).reshape(-1)
        acc = np.zeros(o.shape, dtype=F32)
        for ce in range(nce):
            gb = (((ce * 32 + o) * 32 + i) * 3 + h) * L
            mi = ((ce * 3 + x) * 3 + d) if transposed else ((ce * 3 + d) * 3 + x)
            if J:
                for l in range(J):
                    acc = acc + take(gf, gb + l) * take(mf, mi * J + l)
            else:
                acc = acc + take(gf, gb + x) * take(mf, mi)
        at = off + o * so + i * 27 + d * 9 + h * 3 + x
        ok = at < gw.size
        gw[at[ok]] = acc[ok]
    return gw.reshape(32, 64, 3, 3, 3)


def production_masks(ncls):
    from activezero_amd import costconv
    ml, mr = costconv._masks("cpu", {1: 1, 2: 2, 3: 5}[ncls])
    return ml.numpy(), mr.numpy()


def merge_operands(ncls, which, masks):
    w, ml, mr, gkl, gkr = V.merge_inputs(ncls, which)
    if masks == "production":
        ml, mr = production_masks(ncls)
    return w, ml, mr, gkl, gkr


@pytest.mark.parametrize("ncls", [1, 2, 3])
@pytest.mark.parametrize("which", V.MERGE_SETS)
@pytest.mark.parametrize("masks", ["float", "production"])
def test_merge_emulation_passes(ncls, which, masks):
    w, ml, mr, gkl, gkr = merge_operands(ncls, which, masks)
    exact = which == "exact"
    r = V.merge_check_forward(w, ml, mr, *emu_merge_fwd(w, ml, mr), exact=exact)
    assert max(r.values()) <= 1.0, r
    r = V.merge_check_backward(gkl, gkr, ml, mr, emu_merge_bwd(gkl, gkr, ml, mr), exact=exact)
    assert max(r.values()) <= 1.0, r


MERGE_MUTANTS = {"mask indices (d, w) transposed": dict(transposed=True), "K_R slice offset missing": dict(offset=0),
                 "o stride 32 * 27": dict(so=32 * 27)}


@pytest.mark.parametrize("name", MERGE_MUTANTS)
@pytest.mark.parametrize("which", ["plain", "exact"])
@pytest.mark.parametrize("ncls", [1, 3])
def test_merge_mutant_fails(name, which, ncls):
    w, ml, mr, gkl, gkr = V.merge_inputs(ncls, which)
    opts = MERGE_MUTANTS[name]
    assert max(V.merge_check_forward(w, ml, mr, *emu_merge_fwd(w, ml, mr, **opts), exact=which == "exact").values()) > 1.0
    assert max(V.merge_check_backward(gkl, gkr, ml, mr, emu_merge_bwd(gkl, gkr, ml, mr, **opts), exact=which == "exact").values()) > 1.0


def test_production_masks_hide_the_transposed_mask_where_they_are_symmetric():
    """why the sweep uses float masks: with the production 0/1 masks the transposed K_L index survives wherever ML[c, e] is a
    symmetric matrix -- the bulk variant (all ones) of the middle class among them"""
    ml, _ = production_masks(3)
    assert np.array_equal(ml[1, 4], ml[1, 4].T)


# ==== SPP =========================================================================================================================
def positions_half_pixel(n_in, n_out):     # align_corners=False
    src = np.maximum((np.arange(n_out, dtype=F32) + F32(0.5)) * F32(n_in / n_out) - F32(0.5), F32(0)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, (i0 < n_in - 1).astype(np.int64), (F32(1) - l1).astype(F32), l1


def positions_fp64(n_in, n_out):           # the scale and the positions in fp64, rounded at the end
    src = (n_in - 1) / (n_out - 1) * np.arange(n_out) if n_out > 1 else np.zeros(n_out)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = src - i0
    return i0, (i0 < n_in - 1).astype(np.int64), (1.0 - l1).astype(F32), l1.astype(F32)


def positions_swapped(n_in, n_out):
    i0, ip, l0, l1 = V.spp_positions(n_in, n_out)
    return i0, ip, l1, l0


def positions_unclamped(n_in, n_out):
    i0, ip, l0, l1 = V.spp_positions(n_in, n_out)
    return i0, np.ones_like(ip), l0, l1


def emu_spp_fwd(x, H, W, positions=V.spp_positions):
    B, hs, ws, C = x.shape
    y0, yp, h0, h1 = positions(hs, H)
    x0, xp, w0, w1 = positions(ws, W)
    flat = np.asarray(x).reshape(-1)
    b, yy, xx, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    tap = lambda r, q: take(flat, ((b * hs + r) * ws + q) * C + c)
    r0, q0 = y0[yy], x0[xx]
    r1, q1 = r0 + yp[yy], q0 + xp[xx]
    h0, h1, w0, w1 = h0[yy], h1[yy], w0[xx], w1[xx]
    return h0 * (w0 * tap(r0, q0) + w1 * tap(r0, q1)) + h1 * (w0 * tap(r1, q0) + w1 * tap(r1, q1))


def positions_contracted(n_in, n_out):     # l1 = fma(scale, dst, -i0): the position is not rounded before the subtraction
    i0, ip, _, _ = V.spp_positions(n_in, n_out)
    l1 = fma(V.spp_scale(n_in, n_out), np.arange(n_out, dtype=F32), -i0.astype(F32))
    return i0, ip, (F32(1) - l1).astype(F32), l1


def emu_spp_pass(g, n_in, n_out, npl, once=False, positions=V.spp_positions):
    """one separable pass along axis 0 of g [n_out, M] -> [n_in, M]: npl lanes walk the kernel's window in laps of FMAs, then
    the LDS tree"""
    i0, ip, l0, l1 = positions(n_in, n_out)
    out = np.empty((n_in, g.shape[1]), dtype=F32)
    for i in range(n_in):
        lo, hi = V.spp_window(n_in, n_out, i)
        dst = np.arange(lo, hi + 1)
        a, b = np.where(i0[dst] == i, l0[dst], F32(0)), np.where(i0[dst] + ip[dst] == i, l1[dst], F32(0))
        wt = np.where(i0[dst] == i, a, b) if once else (a + b).astype(F32)
        laps = math.ceil(dst.size / npl)
        wt = np.concatenate([wt, np.zeros(laps * npl - dst.size, dtype=F32)]).reshape(laps, npl)
        v = np.concatenate([g[dst], np.zeros((laps * npl - dst.size, g.shape[1]), dtype=F32)]).reshape(laps, npl, -1)
        acc = np.zeros((npl, g.shape[1]), dtype=F32)
        for lap in range(laps):
            acc = fma(wt[lap][:, None], v[lap], acc)
        s = npl >> 1
        while s > 0:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s >>= 1
        out[i] = acc[0]
    return out


def emu_spp_bwd(g, hs, ws, once=False, positions=V.spp_positions):
    B, H, W, C = g.shape
    npl = 256 // (C // 4)
    t = emu_spp_pass(np.moveaxis(np.asarray(g), 2, 0).reshape(W, -1), ws, W, npl, once, positions).reshape(ws, B, H, C)    # [j, b, y, c]
    t = emu_spp_pass(np.moveaxis(t, 2, 0).reshape(H, -1), hs, H, npl, once, positions).reshape(hs, ws, B, C)               # [i, j, b, c]
    return np.ascontiguousarray(np.moveaxis(t, 2, 0))


@pytest.mark.parametrize("case", V.SPP_CASES, ids=str)
def test_spp_emulation_passes(case):
    (hs, ws), (H, W), _, _ = case
    x, g = V.spp_inputs(case)
    rf = V.spp_check_forward(case, emu_spp_fwd(x, H, W))
    rb = V.spp_check_backward(case, emu_spp_bwd(g, hs, ws))
    assert rf <= 1.0 and rb <= 1.0, (rf, rb)     # (forward: 0.86 at most, at (2, 3) -> (136, 240))


@pytest.mark.parametrize("name,positions", [("align_corners=False", positions_half_pixel), ("scale in fp64", positions_fp64),
                                            ("l0 and l1 swapped", positions_swapped), ("ip not clamped", positions_unclamped)])
def test_spp_forward_mutant_fails(name, positions):
    # (17, 30) -> (136, 240) has the real scales.  An unclamped ip multiplies what lies past the last row or column by l1,
    # which is 0 there unless the last position rounds ABOVE in - 1: (13, 8) -> (22, 14) is the case of the sweep where it does
    # (on the GPU the tap past the buffer's end would also be an out-of-bounds read)
    case = ((13, 8), (22, 14), 2, 32) if name == "ip not clamped" else V.SPP_CASES[3]
    assert case in V.SPP_CASES
    assert V.spp_check_forward(case, emu_spp_fwd(V.spp_inputs(case)[0], *case[1], positions=positions)) > 1.0
    if name in ("align_corners=False", "l0 and l1 swapped"):
        small = ((5, 4), (17, 9), 2, 32)
        assert V.spp_check_forward(small, emu_spp_fwd(V.spp_inputs(small)[0], 17, 9, positions=positions)) > 1.0


@functools.lru_cache(maxsize=None)
def pair_with_a_doubled_tap():
    """(n_in, n_out) whose last destination lands ABOVE the last source index in fp32, so that l1 > 0 falls on the index l0
    falls on; the largest such l1 among small sizes"""
    best = None
    for n_in in range(17, 64):
        for n_out in range(n_in + 1, 4 * n_in):
            i0, ip, l0, l1 = V.spp_positions(n_in, n_out)
            if ip[-1] == 0 and l1[-1] > 0 and (best is None or l1[-1] > best[0]):
                best = (float(l1[-1]), n_in, n_out)
    return best


def test_spp_backward_mutant_doubled_tap_counted_once_fails():
    """the check is the sweep's; the gradient is a single 1 at the last pixel, so that the dropped tap is the whole error"""
    l1, n_in, n_out = pair_with_a_doubled_tap()
    C = 64
    g = np.zeros((1, n_out, n_out, C), dtype=F32)
    g[0, -1, -1] = 1.0
    ref, bound = V.spp_backward_ref(g, n_in, n_in)
    assert V.ratio(emu_spp_bwd(g, n_in, n_in), ref, bound) <= 1.0
    assert V.ratio(emu_spp_bwd(g, n_in, n_in, once=True), ref, bound) > 1.0, (l1, n_in, n_out)


def test_spp_backward_mutant_contracted_position_fails():
    """the defect this sweep found on the GPU: the compiler fused scale * dst - i0 of the backward kernels (not of the forward)
    into one FMA.  (13, 8) -> (22, 14) has positions up to 12 -- half an ulp of them is 4.8e-7 of weight -- and a short tree"""
    case = ((13, 8), (22, 14), 2, 32)
    assert case in V.SPP_CASES
    r = V.spp_check_backward(case, emu_spp_bwd(V.spp_inputs(case)[1], 13, 8, positions=positions_contracted))
    assert r > 1.0, r      # 1.364, which is also what the GPU measured before spp_src forbade the contraction


@pytest.mark.parametrize("case", V.SPP_CASES[:4] + V.SPP_CASES[6:13], ids=str)
def test_spp_reference_is_torch_fp64_within_the_position_rounding(case):
    (hs, ws), (H, W), _, _ = case
    x, g = V.spp_inputs(case)
    ref, _ = V.spp_reference(case)["fwd"]
    gref, _ = V.spp_reference(case)["bwd"]
    t = torch.from_numpy(x.copy()).double().permute(0, 3, 1, 2).requires_grad_()
    out = F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
    out.backward(torch.from_numpy(g.copy()).double().permute(0, 3, 1, 2))
    assert np.abs(out.detach().permute(0, 2, 3, 1).numpy() - ref).max() <= 1e-5 * np.abs(x).max()
    tg = t.grad.permute(0, 2, 3, 1).numpy()
    assert np.abs(tg - gref).max() <= 1e-5 * np.abs(tg).max()


def test_spp_rounding_count_formula():
    # (5, 4) -> (17, 9), C = 32: npl = 32, both windows shorter than 32: 1 + 5 + 1 per pass
    assert V.spp_roundings(5, 4, 17, 9, 32) == 14
    # (2, 2) -> (7, 300), C = 32: the x window is all 300 columns: ceil(300 / 32) = 10 laps
    assert V.spp_roundings(2, 2, 7, 300, 32) == (10 + 5 + 1) + (1 + 5 + 1)
    assert V.spp_roundings(5, 4, 17, 9, 4) == 2 * (1 + 8 + 1) and V.spp_roundings(5, 4, 17, 9, 64) == 2 * (1 + 4 + 1)
