"""GPU: the kernels between PSMNet's feature extractor and its 3-D aggregation -- K3 az_cost_volume.hip (both layouts), the
assemble and merge kernels of az_costconv.hip and az_spp.hip, forward and backward -- against fp64, element-wise.

The kernels are called through the C ABI; every output lies inside a larger buffer filled with a NaN sentinel: every output
element must be written, nothing around it may be.  The references, the bounds and the cases are those of
tests/_volume_fp64ref.py: closed-form fp64 (bit patterns where the operation is a copy or one correctly rounded add) and bounds
that count the kernel's roundings.  Every check is a ratio err / bound <= 1.0 over every element;
tests/test_volume_error_model_cpu.py shows that these checks reject the defects they are meant to see.  Every forward runs
twice and must return the same bits.  Then the refusals (return code, nothing written), the size queries, the alignment
contract and one case per torch-facing wrapper."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, costconv, ops  # noqa: E402
from activezero_amd.nets.psmnet import psmnet_submodule_3 as sub  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _volume_fp64ref as V  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x7FC0BEEF  # a NaN with a payload no arithmetic produces
GUARD = 4096
WORST = {}  # (kernel, input set) -> largest ratio
CODE = _lib.CONST


def note(kernel, case, which, r, capsys):
    WORST[(kernel, which)] = max(WORST.get((kernel, which), 0.0), r)
    with capsys.disabled():
        print(f"\nvolume {kernel} {case} {which}: {r:.4f}")
    return r


def dev(a, skew=0):
    """a device copy of the (read-only) array; skew: its first element lies that many floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + skew, dtype=torch.float32, device=DEV)
    t = buf[skew:].view(a.shape)
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4 * skew
    return t


class Guarded:
    """a float32 output of `shape` inside a buffer of NaN sentinels (GUARD elements before and after it), 16-byte aligned as a
    tensor of its own would be, or `skew` floats past that"""

    def __init__(self, shape, skew=0):
        n = int(np.prod(shape))
        self.n, self.lo = n, GUARD + skew
        self.buf = torch.full((GUARD + skew + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.out = self.buf[self.lo:self.lo + n].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 4 * skew

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())

    def raw(self):
        """the guards are untouched; returns the int32 bits of the inner region"""
        torch.cuda.synchronize()
        assert bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all()), "guard band written"
        return self.buf[self.lo:self.lo + self.n].cpu().numpy().reshape(tuple(self.out.shape))

    def settle(self):
        """the guards are untouched and every output element was written; returns the output as numpy"""
        inner = self.raw()
        assert not (inner == SENTINEL).any(), f"{int((inner == SENTINEL).sum())} output elements not written"
        return inner.view(np.float32)


def call(name, *args):
    with torch.cuda.device(DEV):
        _call(name, *args, _stream())


def twice(run):
    """a forward, run twice into fresh guarded buffers: the same bits"""
    a, b = run(), run()
    if isinstance(a, tuple):
        assert all(V.same_bits(p, q) for p, q in zip(a, b)), "two runs differ"
    else:
        assert V.same_bits(a, b), "two runs differ"
    return a


# ==== K3 ==========================================================================================================================
def k3_forward(case, layout, fl, fr, skew=0):
    (b, c, h, w), d = case
    cost = Guarded(V.k3_shapes(case, layout)[1], skew)
    call("az_cost_volume_fwd" if layout == "ncdhw" else "az_cost_volume_fwd_ndhwc", _p(cost.out), _p(fl), _p(fr), b, c, d, h, w)
    return cost.settle()


def k3_backward(case, layout, g):
    (b, c, h, w), d = case
    fs = V.k3_shapes(case, layout)[0]
    gl, gr = Guarded(fs), Guarded(fs)
    call("az_cost_volume_bwd" if layout == "ncdhw" else "az_cost_volume_bwd_ndhwc", _p(gl.out), _p(gr.out), _p(g), b, c, d, h, w)
    return gl.settle(), gr.settle()


K3_CASES = ([(c, "ncdhw", s) for c in V.K3_NCDHW for s in ("plain", "exact", "bits")]
            + [(V.K3_NCDHW_WALK, "ncdhw", s) for s in ("plain", "exact")]
            + [(c, "ndhwc", s) for c in V.K3_NDHWC for s in ("plain", "exact", "bits")]
            + [(c, "ndhwc", s) for c in (V.K3_NDHWC_FWD_WALK, V.K3_NDHWC_BWD_WALK) for s in ("plain", "exact")])


def test_k3_walk_cases_walk():
    (b, c, h, w), d = V.K3_NCDHW_WALK
    assert b * 2 * c * h * w > V.GRID_CAP
    (b, c, h, w), d = V.K3_NDHWC_BWD_WALK
    assert b * h * w * (2 * c // 4) > V.GRID_CAP
    (b, c, h, w), d = V.K3_NDHWC_FWD_WALK
    assert b * d * h > 8192
    assert any(w * (2 * c // 4) > 256 for (_, c, _, w), _ in V.K3_NDHWC)


@pytest.mark.parametrize("case,layout,which", K3_CASES, ids=str)
def test_k3_forward_bits_and_backward(case, layout, which, capsys):
    fl, fr, g = (dev(t) for t in V.k3_inputs(case, layout, which))
    cost = twice(lambda: k3_forward(case, layout, fl, fr))
    assert note(f"K3 forward {layout}", case, which, V.k3_check_forward(case, layout, which, cost), capsys) == 0.0
    if which != "bits":
        r = note(f"K3 backward {layout}", case, which, V.k3_check_backward(case, layout, which, *k3_backward(case, layout, g)), capsys)
        assert r <= 1.0


def test_k3_ncdhw_takes_no_alignment(capsys):
    """w = 8 with cost (and the feature maps) one float past a 16-byte boundary: the scalar path, the same bits"""
    case = V.K3_NCDHW[1]
    assert case[0][3] == 8
    fl, fr, g = V.k3_inputs(case, "ncdhw", "bits")
    cost = k3_forward(case, "ncdhw", dev(fl, 1), dev(fr, 1), skew=1)
    assert V.k3_check_forward(case, "ncdhw", "bits", cost) == 0.0
    (b, c, h, w), d = case
    gl, gr = Guarded((b, c, h, w), 1), Guarded((b, c, h, w), 3)
    call("az_cost_volume_bwd", _p(gl.out), _p(gr.out), _p(dev(g, 1)), b, c, d, h, w)
    assert V.k3_check_backward(case, "ncdhw", "bits", gl.settle(), gr.settle()) <= 1.0


# ==== assemble ====================================================================================================================
def asm_forward(shape, fb, fe, g):
    B, H, W, D = shape
    out = Guarded(V.asm_shapes(shape)[3])
    call("az_costconv_assemble_fwd", _p(out.out), _p(fb), _p(fe), _p(g), B, D, H, W)
    return out.settle()


def asm_backward(shape, gy):
    B, H, W, D = shape
    outs = [Guarded(s) for s in V.asm_shapes(shape)[:3]]
    call("az_costconv_assemble_bwd", *(_p(o.out) for o in outs), _p(gy), B, D, H, W)
    return [o.settle() for o in outs]


def test_assemble_walk_cases_walk():
    B, H, W, D = V.ASM_FWD_WALK
    assert B * D * H * W * 8 > V.GRID_CAP
    B, H, W, D = V.ASM_BWD_WALK
    assert B * H * W * 8 > V.GRID_CAP and B * H * (W + 2) * 8 > V.GRID_CAP


@pytest.mark.parametrize("shape", V.ASM_SHAPES + [V.ASM_FWD_WALK, V.ASM_BWD_WALK], ids=str)
@pytest.mark.parametrize("which", ["plain", "exact"])
def test_assemble_forward_bits_and_backward(shape, which, capsys):
    fb, fe, g, gy = (dev(t) for t in V.asm_inputs(shape, which))
    out = twice(lambda: asm_forward(shape, fb, fe, g))
    assert note("assemble forward", shape, which, V.asm_check_forward(shape, which, out), capsys) == 0.0
    rs = V.asm_check_backward(shape, which, *asm_backward(shape, gy))
    for k, r in rs.items():
        note(f"assemble backward {k}", shape, which, r, capsys)
    assert rs["dF_edge"] == 0.0 and max(rs.values()) <= 1.0, rs


# ==== merge =======================================================================================================================
def production_masks(ncls):
    ml, mr = costconv._masks("cpu", {1: 1, 2: 2, 3: 5}[ncls])
    return ml.numpy(), mr.numpy()


def merge_forward(ncls, w, ml, mr):
    kl, kr = Guarded((ncls, 5, 32, 32, 3, 3)), Guarded((ncls, 2, 32, 32, 3, 5))
    call("az_costconv_merge_fwd", _p(kl.out), _p(kr.out), _p(w), _p(ml), _p(mr), ncls)
    return kl.settle(), kr.settle()


@pytest.mark.parametrize("ncls", [1, 2, 3])
@pytest.mark.parametrize("which", V.MERGE_SETS)
@pytest.mark.parametrize("masks", ["float", "production"])
def test_merge_forward_and_backward(ncls, which, masks, capsys):
    w, ml, mr, gkl, gkr = V.merge_inputs(ncls, which)      # the weight is the full [32][64][27] tensor: both halves in place
    if masks == "production":
        ml, mr = production_masks(ncls)
    exact = which == "exact"
    dw, dml, dmr, dgkl, dgkr = (dev(t) for t in (w, ml, mr, gkl, gkr))
    kl, kr = twice(lambda: merge_forward(ncls, dw, dml, dmr))
    rs = V.merge_check_forward(w, ml, mr, kl, kr, exact=exact)
    gw = Guarded((32, 64, 3, 3, 3))
    call("az_costconv_merge_bwd", _p(gw.out), _p(dgkl), _p(dgkr), _p(dml), _p(dmr), ncls)
    rb = V.merge_check_backward(gkl, gkr, ml, mr, gw.settle(), exact=exact)     # settle: all 32 * 64 * 27 elements written
    for k in ("kl", "kr"):
        note(f"merge forward {k}", (ncls, masks), which, rs[k], capsys)
        note(f"merge backward {k}", (ncls, masks), which, rb[k], capsys)
    assert max(rs.values()) <= 1.0 and max(rb.values()) <= 1.0, (rs, rb)
    if exact:
        assert max(rs.values()) == 0.0 and max(rb.values()) == 0.0


# ==== SPP =========================================================================================================================
WIDE, AT = 96, 40     # the slot inside a wider row


def spp_forward(case, x, cstride, at):
    (hs, ws), (H, W), B, C = case
    out = Guarded((B, H, W, cstride))
    call("az_spp_upsample_fwd", _p(out.out.view(-1)[at:]), _p(x), B, hs, ws, H, W, C, cstride)
    raw = out.raw()
    slot = raw[..., at:at + C]
    assert not (slot == SENTINEL).any(), "slot elements not written"
    rest = np.delete(raw, np.s_[at:at + C], axis=3)
    assert (rest == SENTINEL).all(), "a channel outside the slot was written"
    return np.ascontiguousarray(slot).view(np.float32)


def spp_backward(case, gout, cstride, at):
    (hs, ws), (H, W), B, C = case
    gin = Guarded((B, hs, ws, C))
    nbytes = _lib.lib().az_spp_upsample_bwd_workspace(B, ws, H, C)
    assert nbytes == B * H * ws * C * 4
    wsp = Guarded((nbytes // 4,))
    call("az_spp_upsample_bwd", _p(gin.out), _p(wsp.out), nbytes, _p(gout.view(-1)[at:]), B, hs, ws, H, W, C, cstride)
    wsp.raw()      # the workspace's guards
    return gin.settle()


@pytest.mark.parametrize("case", V.SPP_CASES, ids=str)
def test_spp_forward_and_backward(case, capsys):
    (hs, ws), (H, W), B, C = case
    x, g = V.spp_inputs(case)
    dx = dev(x)
    layouts = [(C, 0)] + ([(WIDE, AT)] if AT + C <= WIDE else [])      # out_cstride == C, and the slot inside a wider row
    for cstride, at in layouts:
        which = "plain" if cstride == C else "embedded"
        out = twice(lambda: spp_forward(case, dx, cstride, at))
        rf = note("SPP forward", case, which, V.spp_check_forward(case, out), capsys)
        gout = dev(g if cstride == C else V.spp_embed(g, cstride, at, 77))     # the neighbours hold +-1e4
        rb = note("SPP backward", case, which, V.spp_check_backward(case, spp_backward(case, gout, cstride, at)), capsys)
        assert rf <= 1.0 and rb <= 1.0, (rf, rb)
        if (case[0], case[1]) in V.SPP_COPIES:
            assert rf == 0.0


def test_spp_case_list_reaches_every_tree_depth():
    assert {c[3] for c in V.SPP_CASES} == set(V.SPP_CHANNELS)
    assert any(AT + c[3] <= WIDE for c in V.SPP_CASES)


# ==== refusals: the return code, and nothing written ==============================================================================
def refused(name, want, args, outs):
    with torch.cuda.device(DEV):
        got = getattr(_lib.lib(), name)(*args, _stream())
    assert got == CODE[want], (name, got, want)
    assert all(o.untouched() for o in outs), name


def variants(ptrs, dims):
    """(code, ptrs, dims): each pointer NULL in turn, each dimension 0 and -1 in turn"""
    for k in range(len(ptrs)):
        yield "AZ_ENULL", ptrs[:k] + [None] + ptrs[k + 1:], dims
    for k in range(len(dims)):
        for bad in (0, -1):
            yield "AZ_EINVAL", ptrs, dims[:k] + [bad] + dims[k + 1:]


def skewed(ptrs):
    """each pointer one float past its 16-byte boundary in turn (every buffer here has room behind it)"""
    for k in range(len(ptrs)):
        yield ptrs[:k] + [ptrs[k] + 4] + ptrs[k + 1:]


def test_k3_refusals():
    case = ((1, 4, 2, 5), 3)
    (b, c, h, w), d = case
    dims = [b, c, d, h, w]
    for layout, fwd, bwd in (("ncdhw", "az_cost_volume_fwd", "az_cost_volume_bwd"), ("ndhwc", "az_cost_volume_fwd_ndhwc", "az_cost_volume_bwd_ndhwc")):
        fs, cs = V.k3_shapes(case, layout)
        cost, gl, gr = Guarded(cs), Guarded(fs), Guarded(fs)
        outs = [cost, gl, gr]
        fwd_ptrs, bwd_ptrs = [_p(cost.out), _p(gl.out), _p(gr.out)], [_p(gl.out), _p(gr.out), _p(cost.out)]
        for name, ptrs in ((fwd, fwd_ptrs), (bwd, bwd_ptrs)):
            for code, p, dm in variants(ptrs, dims):
                refused(name, code, p + dm, outs)
            if layout == "ndhwc":
                refused(name, "AZ_EUNSUPPORTED", ptrs + [b, 6, d, h, w], outs)       # C % 4
                for p in skewed(ptrs):
                    refused(name, "AZ_EINVAL", p + dims, outs)                         # the float4 lanes' alignment
        if layout == "ncdhw":
            refused(fwd, "AZ_EUNSUPPORTED", fwd_ptrs + [1, 1, 1, 1, 16385], outs)      # a row of more than 64 KiB of LDS


def test_assemble_refusals():
    shape = (1, 2, 4, 3)
    B, H, W, D = shape
    bufs = [Guarded(s) for s in V.asm_shapes(shape)]
    fwd = [_p(bufs[3].out), _p(bufs[0].out), _p(bufs[1].out), _p(bufs[2].out)]
    bwd = [_p(bufs[0].out), _p(bufs[1].out), _p(bufs[2].out), _p(bufs[3].out)]
    for name, ptrs in (("az_costconv_assemble_fwd", fwd), ("az_costconv_assemble_bwd", bwd)):
        for code, p, dm in variants(ptrs, [B, D, H, W]):
            refused(name, code, p + dm, bufs)
        for p in skewed(ptrs):
            refused(name, "AZ_EINVAL", p + [B, D, H, W], bufs)


def test_merge_refusals():
    kl, kr, gw = Guarded((3, 5, 32, 32, 3, 3)), Guarded((3, 2, 32, 32, 3, 5)), Guarded((32, 64, 27))
    ml, mr = Guarded((3, 5, 3, 3)), Guarded((3, 2, 3, 3, 5))
    bufs = [kl, kr, gw, ml, mr]
    fwd = [_p(kl.out), _p(kr.out), _p(gw.out), _p(ml.out), _p(mr.out)]
    bwd = [_p(gw.out), _p(kl.out), _p(kr.out), _p(ml.out), _p(mr.out)]
    for name, ptrs in (("az_costconv_merge_fwd", fwd), ("az_costconv_merge_bwd", bwd)):
        for k in range(5):
            refused(name, "AZ_ENULL", ptrs[:k] + [None] + ptrs[k + 1:] + [3], bufs)
        for ncls in (0, 4, -1):
            refused(name, "AZ_EINVAL", ptrs + [ncls], bufs)


def test_spp_refusals():
    B, hs, ws, H, W, C = 2, 3, 2, 5, 4, 32
    out, x, gin = Guarded((B, H, W, 128)), Guarded((B, hs, ws, 128)), Guarded((B, hs, ws, 128))
    nbytes = _lib.lib().az_spp_upsample_bwd_workspace(B, ws, H, 128)
    wsp = Guarded((nbytes // 4,))
    bufs = [out, x, gin, wsp]
    dims = [B, hs, ws, H, W]
    fwd_ptrs = [_p(out.out), _p(x.out)]
    fwd = lambda p, dm, c, cs: p + dm + [c, cs]
    bwd = lambda p, dm, c, cs, nb=nbytes: [p[0], p[1], nb, p[2]] + dm + [c, cs]
    bwd_ptrs = [_p(gin.out), _p(wsp.out), _p(out.out)]
    for name, ptrs, pack in (("az_spp_upsample_fwd", fwd_ptrs, fwd), ("az_spp_upsample_bwd", bwd_ptrs, bwd)):
        for code, p, dm in variants(ptrs, dims):
            refused(name, code, pack(p, dm, C, C), bufs)
        for c, code in ((0, "AZ_EINVAL"), (-4, "AZ_EINVAL"), (6, "AZ_EINVAL"), (48, "AZ_EUNSUPPORTED"), (128, "AZ_EUNSUPPORTED")):
            refused(name, code, pack(ptrs, dims, c, 128), bufs)
        refused(name, "AZ_EINVAL", pack(ptrs, dims, C, C - 4), bufs)      # out_cstride < C
        refused(name, "AZ_EINVAL", pack(ptrs, dims, C, C + 2), bufs)      # out_cstride % 4
        for p in skewed(ptrs):
            refused(name, "AZ_EINVAL", pack(p, dims, C, C), bufs)
    need = _lib.lib().az_spp_upsample_bwd_workspace(B, ws, H, C)
    refused("az_spp_upsample_bwd", "AZ_EWORKSPACE", bwd(bwd_ptrs, dims, C, C, need - 1), bufs)


def test_size_queries():
    lib = _lib.lib()
    for D in range(1, 7):
        assert lib.az_costconv_num_classes(D) == min(D, 3) == V.num_classes(D) == costconv.num_classes(D)
        for W in range(1, 7):
            assert lib.az_costconv_edge_width(D, W) == min(W, D + 1) == V.edge_width(D, W)
    assert lib.az_costconv_num_classes(0) == CODE["AZ_EINVAL"] and lib.az_costconv_num_classes(-1) == CODE["AZ_EINVAL"]
    for B, ws, H, C in ((1, 1, 1, 4), (2, 3, 5, 32), (4, 30, 136, 32), (3, 7, 2, 64)):
        assert lib.az_spp_upsample_bwd_workspace(B, ws, H, C) == 4 * B * H * ws * C
    for bad in ((0, 3, 5, 32), (2, 0, 5, 32), (2, 3, -1, 32), (2, 3, 5, 0)):
        assert lib.az_spp_upsample_bwd_workspace(*bad) == CODE["AZ_EINVAL"]


# ==== the torch-facing wrappers, one case each against the same references ======================================================
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_wiring_cost_volume_with_a_non_contiguous_input(layout, capsys):
    case, which = (V.K3_NCDHW[0], "plain") if layout == "ncdhw" else (V.K3_NDHWC[1], "plain")
    fl, fr, g = V.k3_inputs(case, layout, which)
    # leaves whose views with the last two axes swapped are the operands: equal values, not contiguous
    bl, br = (dev(np.swapaxes(t, -1, -2)).requires_grad_() for t in (fl, fr))
    xl, xr = bl.transpose(-1, -2), br.transpose(-1, -2)
    assert not xl.is_contiguous()
    fn = ops.cost_volume if layout == "ncdhw" else ops.cost_volume_ndhwc
    cost = fn(xl, xr, case[1])
    assert V.k3_check_forward(case, layout, which, cost.detach().cpu().numpy()) == 0.0
    cost.backward(dev(g))
    gl, gr = (np.swapaxes(t.grad.cpu().numpy(), -1, -2) for t in (bl, br))
    assert note(f"K3 backward {layout}", case, "autograd", V.k3_check_backward(case, layout, which, gl, gr), capsys) <= 1.0


def test_wiring_assemble_node(capsys):
    shape, which = (2, 3, 9, 5), "plain"
    fb, fe, g, gy = (dev(t) for t in V.asm_inputs(shape, which))
    for t in (fb, fe, g):
        t.requires_grad_()
    out = costconv._Assemble.apply(fb, fe, g, shape[3])
    assert V.asm_check_forward(shape, which, out.detach().cpu().numpy()) == 0.0
    out.backward(gy)
    grads = [t.grad for t in (fb, fe, g)]
    assert [tuple(t.shape) for t in grads] == list(V.asm_shapes(shape)[:3])
    rs = V.asm_check_backward(shape, which, *(t.cpu().numpy() for t in grads))
    assert note("assemble backward", shape, "autograd", max(rs.values()), capsys) <= 1.0


def test_wiring_spp_concat_slots_and_needs_input_grad(capsys):
    B, h, w = 2, 17, 9
    sizes = [(5, 4), (1, 1), (3, 5), (9, 8)]
    cl = lambda a: dev(a).permute(0, 3, 1, 2)       # rows [B,h,w,C] -> an image in channels_last memory
    raw_r, skip_r = V.values((B, h, w, 64), "plain", 501), V.values((B, h, w, 128), "plain", 502)
    br_r = [V.values((B, hs, ws, 32), "plain", 503 + k) for k, (hs, ws) in enumerate(sizes)]
    cot_r = V.values((B, h, w, 320), "plain", 510)
    raw, skip = cl(raw_r).requires_grad_(), cl(skip_r)                   # skip and branch 2 take no gradient
    br = [cl(t) for t in br_r]
    for k in (0, 1, 3):
        br[k].requires_grad_()
    y = sub.spp_concat(raw, skip, br)
    assert tuple(y.shape) == (B, 320, h, w) and y.is_contiguous(memory_format=torch.channels_last)
    rows = y.detach().permute(0, 2, 3, 1).cpu().numpy()
    assert V.same_bits(rows[..., :64], raw_r) and V.same_bits(rows[..., 64:192], skip_r)
    y.backward(cl(cot_r))
    assert skip.grad is None and br[2].grad is None
    assert V.same_bits(raw.grad.permute(0, 2, 3, 1).cpu().numpy(), cot_r[..., :64])
    worst = 0.0
    for k, (t, (hs, ws)) in enumerate(zip(br_r, sizes)):
        at = 192 + 32 * k
        worst = max(worst, V.ratio(rows[..., at:at + 32], *V.spp_forward_ref(t, h, w)))
        if k != 2:
            got = br[k].grad.permute(0, 2, 3, 1).cpu().numpy()
            worst = max(worst, V.ratio(got, *V.spp_backward_ref(cot_r[..., at:at + 32], hs, ws)))
    assert note("SPP", (B, h, w), "spp_concat", worst, capsys) <= 1.0


def test_zz_largest_ratios(capsys):
    """the largest ratio of each check per kernel and input set over the cases run"""
    with capsys.disabled():
        print()
        for (kernel, which), r in sorted(WORST.items()):
            print(f"volume worst {kernel:28s} {which:11s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
