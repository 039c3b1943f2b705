"""CPU: the two element-wise checks of tests/_fp64ref.py are sharp enough to catch a subtly wrong stride-1 convolution.

A pure-torch emulation of the f16x3 and bf16x6 arithmetic (operands split as the kernels split them, the defined products
summed exactly per 32-deep K block, the block sums accumulated in fp32) passes checks (a), (b) and (c) at the small shapes of
tests/test_gpu_conv3d_s1.py; each mutant of it -- one defect of a class a kernel could have -- fails at least one check at
every one of those shapes its class applies to.  This is what says that the GPU sweep would fail on such a kernel; no mutant
kernel is built or run."""
import pytest
import torch
import torch.nn.functional as F

from tests import _fp64ref as R
from tests._weights import seeded

SHAPES = [(1, 1, 1, 1), (1, 1, 3, 3), (1, 5, 7, 19), (2, 4, 9, 16), (1, 3, 2, 15), (3, 2, 5, 33), (1, 13, 25, 17)]
TERMS = {"f16x3": [(0, 0), (0, 1), (1, 0)], "bf16x6": [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], "fp32": [(0, 0)]}


def operands(kind, shape, cin=32, cout=32, seed=7000):
    b, d, h, w = shape
    x = seeded((b, cin, d, h, w), seed)
    wt = seeded((cout, cin, 3, 3, 3), seed + 1, -0.2, 0.2)
    dy = seeded((b, cout, d, h, w), seed + 2) * 1e-3
    return {"fwd": (x, wt), "dgrad": (dy, wt), "wgrad": (x, dy)}[kind]


def unfold(t, w_edge=False):
    """[B,C,D,H,W] (fp64) -> [B*D*H*W, 27*C] neighbourhoods (tap-major).  w_edge: the kw = 2 tap of the last column reads
    the column itself instead of the zero padding (a tap shifted by one at the W edge)"""
    b, c, d, h, w = t.shape
    xp = F.pad(t.permute(0, 2, 3, 4, 1), (0, 0, 1, 1, 1, 1, 1, 1))
    if w_edge:
        xp[:, :, :, w + 1, :] = xp[:, :, :, w, :]
    return torch.cat([R._neighbourhoods(xp, bi, di, h, w) for bi in range(b) for di in range(d)])


def position_weights(shape, mutant):
    """per coarse position (b, d, h, w order) how often the r16 weight-gradient kernel's K blocks count it"""
    b, d, h, w = shape
    m = torch.ones(b, d, h, w, dtype=torch.float64)
    if mutant == "odd_h_tail":      # K block = two adjacent rows x 16 positions: the last, half-empty pair of an odd H dropped
        m[:, :, h - 1, :] = 0.0
    if mutant == "column_twice":    # one (batch, depth, 16-position chunk) column walked by two workgroups
        c0 = 16 * ((w - 1) // 16)
        m[0, d - 1, :, c0:] = 2.0
    return m.reshape(-1)


def emulate(kind, p, q, arith, mutant=None):
    """the kernel's result in the emulated arithmetic (NCDHW / weight layout, fp32)"""
    terms = list(TERMS[arith])
    if mutant == "hilo_dropped":
        terms.remove((0, 1))
    if mutant == "f16x1":
        terms = [(0, 0)]
    pp, qq = R.split_parts(p, arith), R.split_parts(q, arith)
    if mutant == "lo_scale":        # the lo parts of one operand scaled by 2^(k+1) instead of 2^k
        pp[1] = pp[1] * 2.0
    edge = mutant == "w_edge"
    if kind == "dgrad":
        qq = [t.transpose(0, 1).flip(2, 3, 4) for t in qq]
    if kind in ("fwd", "dgrad"):
        b, _, d, h, w = p.shape
        cout = qq[0].shape[0]
        a = [unfold(t, edge) for t in pp]                                          # [N, K]
        bm = [t.permute(2, 3, 4, 1, 0).reshape(-1, cout) for t in qq]              # [K, cout]
    else:
        b, _, d, h, w = p.shape
        cout = qq[0].shape[1]
        pw = position_weights((b, d, h, w), mutant)
        a = [(t.permute(1, 0, 2, 3, 4).reshape(cout, -1) * pw) for t in qq]      # dy^T [cout, K]
        bm = [unfold(t, edge) for t in pp]                                         # [K, 27 cin]
    K = a[0].shape[1]
    acc = torch.zeros(a[0].shape[0], bm[0].shape[1], dtype=torch.float32)
    for k0 in range(0, K, 32):
        blk = sum(a[i][:, k0:k0 + 32] @ bm[j][k0:k0 + 32] for (i, j) in
                  (terms if kind == "wgrad" else [(j, i) for (i, j) in terms]))
        acc = acc + blk.float()  # (one fp32 rounding of the exact block sum, one fp32 add)
    if kind == "wgrad":
        cin = p.shape[1]
        return acc.reshape(cout, 27, cin).permute(0, 2, 1).reshape(cout, cin, 3, 3, 3)
    return acc.reshape(b, d, h, w, cout).permute(0, 4, 1, 2, 3)


def ratios(kind, shape, arith, mutant=None):
    p, q = operands(kind, shape)
    got = emulate(kind, p, q, arith, mutant)
    ex = R.exact(kind, p, q)
    sref = R.split_reference(kind, p, q, arith)
    return R.check(got, arith, R.products(kind, p, q), ex, sref, R.amax_of(p), R.amax_of(q))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "fp32"])
def test_emulated_arithmetic_passes_both_checks(arith, kind, shape, capsys):
    r = ratios(kind, shape, arith)
    with capsys.disabled():
        print(f"\nemulated {arith} {kind} {shape}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")
    assert max(r) <= 1.0, r


# (mutant, arithmetic, kinds, shapes it applies to)
_ODD_H = [s for s in SHAPES if s[2] % 2]
# (a V0-deep weight gradient, K = 42 240 positions, the 32 x 32 walk shape of the GPU test: check (c) must see one column)
_LARGE = [(1, 24, 5, 352)]
MUTANTS = [
    ("hilo_dropped", "f16x3", R.KINDS, SHAPES),
    ("f16x1", "f16x3", R.KINDS, SHAPES),
    ("lo_scale", "f16x3", R.KINDS, SHAPES),
    ("odd_h_tail", "f16x3", ("wgrad",), _ODD_H + _LARGE),
    ("odd_h_tail", "bf16x6", ("wgrad",), _ODD_H),
    ("column_twice", "f16x3", ("wgrad",), SHAPES + _LARGE),
    ("column_twice", "bf16x6", ("wgrad",), SHAPES),
    ("w_edge", "f16x3", R.KINDS, SHAPES),
    ("w_edge", "bf16x6", R.KINDS, SHAPES),
]
_CASES = [(m, a, k, s) for (m, a, kinds, shapes) in MUTANTS for k in kinds for s in shapes]


@pytest.mark.parametrize("mutant,arith,kind,shape", _CASES, ids=[f"{m}-{a}-{k}-{s}" for (m, a, k, s) in _CASES])
def test_mutant_fails_a_check(mutant, arith, kind, shape, capsys):
    r = ratios(kind, shape, arith, mutant)
    with capsys.disabled():
        print(f"\nmutant {mutant} {arith} {kind} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert max(r) > 1.0, r


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 1, 1)])
def test_gemm_reference_is_the_convolution(kind, shape):
    """op_gemm (the references of the GPU test's large shapes) computes what torch's fp64 convolutions compute"""
    p, q = operands(kind, shape, cin=32, cout=64)
    want, got = R.op(kind, p, q), R.op_gemm(kind, p, q)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_split_parts_are_the_documented_splits():
    t = seeded((4096,), 7100) * 3.0
    t[:3] = torch.tensor([0.0, 2.0 ** -30, -3.0])
    k = R.f16_scale_exp(R.amax_of(t))
    assert 2.0 ** 14 <= 2.0 ** k * R.amax_of(t) < 2.0 ** 15
    hi, lo = R.split_parts(t, "f16x3")
    am = R.amax_of(t)
    # hi + lo = x up to 2^-22 |x|, and 2^-39 of the amax for elements in fp16's subnormal range
    assert bool(((hi + lo - t.double()).abs() <= 2.0 ** -22 * t.double().abs() + 2.0 ** -39 * am).all())
    parts = R.split_parts(t, "bf16x6")
    assert bool(((sum(parts) - t.double()).abs() <= 2.0 ** -24 * t.double().abs()).all())
    assert R.split_parts(t, "fp32")[0].equal(t.double())


# ---- the 2-D family (tests/test_gpu_conv2d_fp64.py) ----------------------------------------------------------------------------
G33, G33D2, G11, G35 = R.Geom2d(3, 3, 1), R.Geom2d(3, 3, 2), R.Geom2d(1, 1, 1), R.Geom2d(3, 5, 1)
SHAPES2D = [(2, 13, 22), (1, 16, 32), (3, 5, 47), (2, 37, 53), (1, 1, 1)]  # the small shapes of the GPU file
GEOMS2D = [(G33, SHAPES2D), (G33D2, [(2, 13, 22), (1, 1, 1)]), (G11, [(3, 5, 47), (1, 1, 1)]), (G35, [(2, 13, 22), (1, 1, 1)])]
SEG_LEN = 3  # images per batch segment of the emulated walk (the GPU file's walking cases have seg_len 3)


def operands2d(kind, shape, geom, cin=32, cout=32, seed=7600):
    b, h, w = shape
    x = seeded((b, cin, h, w), seed)
    wt = seeded((cout, cin, geom.kh, geom.kw), seed + 1, -0.2, 0.2)
    dy = seeded((b, cout, h, w), seed + 2) * 1e-3
    return {"fwd": (x, wt), "dgrad": (dy, wt), "wgrad": (x, dy)}[kind]


def seam_row(h):
    """first row of the second row segment of a weight gradient split into two even-length segments (az_c2w16_plan)"""
    rows = (h + 1) // 2
    return rows + (rows & 1)


def halo_row(h):
    """an output row whose kh = 0 tap lies in the halo of its 8-row patch (the first row of the second patch row, else row 1)"""
    return 8 if h > 8 else 1


def unfold2d(t, geom, mutant=None):
    """[B,C,H,W] (fp64) -> [B*H*W, kh*kw*C] neighbourhoods (tap-major).
    w_edge: the taps right of the last image column read that column instead of the zero padding;
    halo_prev: the row above output row halo_row(H) of every image but the first is read from the previous image of the walk"""
    b, c, h, w = t.shape
    ph, pw = geom.pad
    xp = F.pad(t.permute(0, 2, 3, 1), (0, 0, pw, pw, ph, ph))
    if mutant == "w_edge" and pw:
        xp[:, :, w + pw:, :] = xp[:, :, w + pw - 1:w + pw, :]
    out = []
    for bi in range(b):
        img = xp[bi]
        taps = []
        for i in range(geom.kh):
            for j in range(geom.kw):
                v = img[i * geom.dil:i * geom.dil + h, j * geom.dil:j * geom.dil + w, :].clone()
                if mutant == "halo_prev" and bi > 0 and i == 0 and ph:
                    r = halo_row(h)
                    v[r] = xp[bi - 1][i * geom.dil + r, j * geom.dil:j * geom.dil + w, :]
                taps.append(v)
        out.append(torch.stack(taps, dim=2).reshape(h * w, -1))
    return torch.cat(out)


def position_weights2d(shape, mutant):
    """per position (b, h, w order) how often the weight-gradient kernels' K blocks count it"""
    b, h, w = shape
    m = torch.ones(b, h, w, dtype=torch.float64)
    if mutant == "seam_row_twice":    # the first row of the second row segment also counted by the first segment
        m[:, seam_row(h), :] = 2.0
    if mutant == "seam_row_dropped":  # ... or by neither
        m[:, seam_row(h), :] = 0.0
    if mutant == "column_twice":      # one (image, 16-position chunk) column walked by two workgroups
        m[b - 1, :, 16 * ((w - 1) // 16):] = 2.0
    return m.reshape(-1)


def emulate2d(kind, p, q, arith, geom, mutant=None):
    """the 2-D kernels' result in the emulated arithmetic (NCHW / weight layout, fp32): exact sums of the defined products
    per 32-deep K block, fp32 accumulation of the block sums"""
    terms = list(TERMS[arith])
    if mutant == "hilo_dropped":
        terms.remove((0, 1))
    pp, qq = R.split_parts(p, arith), R.split_parts(q, arith)
    if mutant == "lo_scale":
        pp[1] = pp[1] * 2.0
    if kind == "dgrad":
        qq = [t.transpose(0, 1).flip(2, 3) for t in qq]
    b, _, h, w = p.shape
    if kind in ("fwd", "dgrad"):
        cout = qq[0].shape[0]
        a = [unfold2d(t, geom, mutant) for t in pp]
        bm = [t.permute(2, 3, 1, 0).reshape(-1, cout) for t in qq]
    else:
        cout = qq[0].shape[1]
        pw = position_weights2d((b, h, w), mutant)
        a = [(t.permute(1, 0, 2, 3).reshape(cout, -1) * pw) for t in qq]
        bm = [unfold2d(t, geom, mutant) for t in pp]
    K = a[0].shape[1]
    acc = torch.zeros(a[0].shape[0], bm[0].shape[1], dtype=torch.float32)
    for k0 in range(0, K, 32):
        blk = sum(a[i][:, k0:k0 + 32] @ bm[j][k0:k0 + 32] for (i, j) in
                  (terms if kind == "wgrad" else [(j, i) for (i, j) in terms]))
        acc = acc + blk.float()
    if kind == "wgrad":
        cin = p.shape[1]
        return acc.reshape(cout, geom.kh * geom.kw, cin).permute(0, 2, 1).reshape(cout, cin, geom.kh, geom.kw)
    y = acc.reshape(b, h, w, cout).permute(0, 3, 1, 2).clone()
    if mutant == "last_image_skipped":  # the last image of a ragged batch segment never multiplied: its output stays as
        y[b - 1] = 0.0                  # the buffer was (zero here)
    return y


def ratios2d(kind, shape, arith, geom, mutant=None):
    p, q = operands2d(kind, shape, geom)
    got = emulate2d(kind, p, q, arith, geom, mutant)
    ex = R.exact(kind, p, q, geom=geom)
    sref = R.split_reference(kind, p, q, arith, geom=geom)
    blocks = R.wgrad_blocks_2d(q) if kind == "wgrad" else None
    return R.check(got, arith, R.products(kind, p, q, geom), ex, sref, R.amax_of(p), R.amax_of(q), blocks=blocks)


_EMU2D = [(g, s) for (g, shapes) in GEOMS2D for s in shapes]


@pytest.mark.parametrize("geom,shape", _EMU2D, ids=[f"{g.kh}x{g.kw}d{g.dil}-{s}" for (g, s) in _EMU2D])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("arith", ["f16x3", "bf16x6"])
def test_emulated_2d_arithmetic_passes_the_checks(arith, kind, geom, shape, capsys):
    r = ratios2d(kind, shape, arith, geom)
    with capsys.disabled():
        print(f"\nemulated 2-D {arith} {kind} {tuple(geom[:3])} {shape}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")
    assert max(r) <= 1.0, r


_SEAM = [s for s in SHAPES2D if s[1] >= 3]                 # a second row segment exists
_RAGGED = [s for s in SHAPES2D if s[0] % SEG_LEN]          # the last batch segment is shorter than SEG_LEN
_HALO = [s for s in SHAPES2D if s[0] >= 2 and s[1] >= 2]   # a previous image and a row above
_WIDE = [s for s in SHAPES2D if s != (1, 1, 1)]
ARITHS2D = ("f16x3", "bf16x6")
MUTANTS2D = [  # (mutant, kinds, geometry, shapes it applies to)
    ("seam_row_twice", ("wgrad",), G33, _SEAM),
    ("seam_row_dropped", ("wgrad",), G33, _SEAM),
    ("column_twice", ("wgrad",), G33, SHAPES2D),
    ("last_image_skipped", ("fwd",), G33, _RAGGED),
    ("halo_prev", ("fwd", "dgrad"), G33, _HALO),
    ("hilo_dropped", R.KINDS, G33, SHAPES2D),
    ("lo_scale", R.KINDS, G33, SHAPES2D),
    ("w_edge", R.KINDS, G33, SHAPES2D),
    ("w_edge", R.KINDS, G35, [(2, 13, 22), (1, 1, 1)]),
    ("w_edge", R.KINDS, G33D2, [(2, 13, 22), (1, 1, 1)]),
    ("hilo_dropped", R.KINDS, G11, [(3, 5, 47), (1, 1, 1)]),
]
_CASES2D = [(m, a, k, g, s) for (m, kinds, g, shapes) in MUTANTS2D for a in ARITHS2D for k in kinds for s in shapes]


@pytest.mark.parametrize("mutant,arith,kind,geom,shape", _CASES2D,
                         ids=[f"{m}-{a}-{k}-{g.kh}x{g.kw}d{g.dil}-{s}" for (m, a, k, g, s) in _CASES2D])
def test_2d_mutant_fails_a_check(mutant, arith, kind, geom, shape, capsys):
    r = ratios2d(kind, shape, arith, geom, mutant)
    with capsys.disabled():
        print(f"\n2-D mutant {mutant} {arith} {kind} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert max(r) > 1.0, r


# the patch route of firstconv.0: 3x3, stride 2, pad 1 on a 3- / 6-channel image as patches [.., Kp] x a 1x1 layer on Kp
# channels of which 9 cin are real; the reference is the stride-2 convolution with K = 9 cin
def patch_rows(x, kp, pad_value=0.0):
    """az_im2col_s2k3: [B,C,H,W] -> [B,Ho,Wo,Kp], patches[.., t C + c] = x[2 oy - 1 + t / 3, 2 ox - 1 + t % 3, c]"""
    b, c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = F.pad(x, (1, 2, 1, 2))
    taps = [xp[:, :, i:i + 2 * ho:2, j:j + 2 * wo:2] for i in range(3) for j in range(3)]  # each [B,C,Ho,Wo]
    pt = torch.stack(taps, dim=1).reshape(b, 9 * c, ho, wo).permute(0, 2, 3, 1)
    out = torch.full((b, ho, wo, kp), pad_value, dtype=x.dtype)
    out[..., :9 * c] = pt
    return out


@pytest.mark.parametrize("cin,kp", [(3, 32), (6, 64)])
@pytest.mark.parametrize("shape", [(2, 13, 22), (1, 16, 32), (1, 1, 1)])
@pytest.mark.parametrize("mutant", [None, "pad_channel"])
def test_patch_route_forward_emulation_and_its_pad_channel_mutant(cin, kp, shape, mutant, capsys):
    """bf16x6, as the code routes it.  pad_channel: the channels [9 cin, Kp) of the patches and of the packed weights are read
    as what lies next to them (non-zero) instead of zero"""
    b, h, w = shape
    cout = 32
    geom = R.Geom2d(3, 3, 1, 2)
    x = seeded((b, cin, h, w), 7700)
    wt = seeded((cout, cin, 3, 3), 7701, -0.2, 0.2)
    pr = patch_rows(x, kp)
    w2 = torch.zeros(cout, kp)
    w2[:, :9 * cin] = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    if mutant:
        n = kp - 9 * cin  # (copies of the centre tap's channels: the tap no image edge zeroes)
        pr[..., 9 * cin:] = pr[..., 4 * cin:4 * cin + n]
        w2[:, 9 * cin:] = w2[:, 4 * cin:4 * cin + n]
    pp, qq = R.split_parts(pr.reshape(-1, kp), "bf16x6"), R.split_parts(w2, "bf16x6")
    acc = torch.zeros(pp[0].shape[0], cout, dtype=torch.float32)
    for k0 in range(0, kp, 16):
        acc = acc + sum(pp[i][:, k0:k0 + 16] @ qq[j][:, k0:k0 + 16].t() for (j, i) in TERMS["bf16x6"]).float()
    got = acc.reshape(b, pr.shape[1], pr.shape[2], cout).permute(0, 3, 1, 2)
    ex = R.exact("fwd", x, wt, geom=geom)
    assert got.shape == ex["y"].shape
    sref = R.split_reference("fwd", x, wt, "bf16x6", geom=geom)
    r = R.check(got, "bf16x6", R.products("fwd", x, wt, geom), ex, sref)
    with capsys.disabled():
        print(f"\npatch route {mutant} cin {cin} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert (max(r) > 1.0) if mutant else (max(r) <= 1.0), r


@pytest.mark.parametrize("geom", [G33, G33D2, G11, G35, R.Geom2d(3, 3, 1, 2, (7, 10)), R.Geom2d(3, 3, 1, 2, (8, 9))])
@pytest.mark.parametrize("kind", R.KINDS)
def test_2d_references_agree_with_a_direct_sum(kind, geom):
    """op (torch's fp64 convolutions) against a tap-by-tap sum written here, and op_gemm against op at stride 1"""
    b, cin, cout = 2, 3, 4
    h, w = geom.in_hw or (7, 10)
    st = geom.stride
    ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
    x, wt, dy = seeded((b, cin, h, w), 7800).double(), seeded((cout, cin, geom.kh, geom.kw), 7801).double(), seeded((b, cout, ho, wo), 7802).double()
    ph, pw = geom.pad
    xp = F.pad(x, (pw, pw + st, ph, ph + st))
    win = {(i, j): xp[:, :, i * geom.dil:i * geom.dil + st * ho:st, j * geom.dil:j * geom.dil + st * wo:st]
           for i in range(geom.kh) for j in range(geom.kw)}  # x at (st oy - ph + i dil, st ox - pw + j dil): [B,cin,Ho,Wo]
    if kind == "fwd":
        want = sum(torch.einsum("bchw,oc->bohw", win[i, j], wt[:, :, i, j]) for (i, j) in win)
        p, q = x, wt
    elif kind == "wgrad":
        want = torch.stack([torch.stack([torch.einsum("bchw,bohw->oc", win[i, j], dy) for j in range(geom.kw)], -1)
                            for i in range(geom.kh)], -2)
        p, q = x, dy
    else:  # the adjoint of the forward: <fwd(x), dy> = <x, dgrad(dy)> for every x; taken from autograd of the direct sum
        xr = x.clone().requires_grad_(True)
        xpr = F.pad(xr, (pw, pw + st, ph, ph + st))
        y = sum(torch.einsum("bchw,oc->bohw", xpr[:, :, i * geom.dil:i * geom.dil + st * ho:st, j * geom.dil:j * geom.dil + st * wo:st],
                             wt[:, :, i, j]) for (i, j) in win)
        want, = torch.autograd.grad(y, xr, dy)
        p, q = dy, wt
    got = R.op(kind, p, q, geom)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    if st == 1:
        assert float((R.op_gemm(kind, p, q, geom) - want).abs().max()) <= 1e-13 * float(want.abs().max())


# ---- the strided 3-D family (tests/test_gpu_conv3d_s2.py) -----------------------------------------------------------------------
S2, T2 = R.Geom3d(2, False), R.Geom3d(2, True)
S2_FINE = [(1, 2, 2, 2), (1, 1, 6, 10), (1, 4, 6, 10), (2, 6, 8, 20), (1, 2, 10, 34), (3, 4, 18, 30), (1, 14, 50, 34)]
S2_ODD = [(1, 7, 33, 65), (1, 3, 7, 13)]                    # fine sizes: forward and weight gradient only
T2_COARSE = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 4, 17), (1, 1, 5, 9), (3, 2, 9, 15), (1, 7, 25, 17)]
T_SEG_LEN = 2  # coarse planes per depth segment of the emulated transposed walk (the seam mutant)


def coarse_of(fine):
    return (fine[0],) + tuple((n - 1) // 2 + 1 for n in fine[1:])


def geom_of(transposed, shape):
    """the geometry of a case: shape = the fine size of a stride-2 layer / the coarse size of a transposed one"""
    if transposed:
        return T2
    return R.Geom3d(2, False, shape[1:]) if any(n % 2 for n in shape[1:]) else S2


def operands_s2(kind, transposed, shape, cin=32, cout=32, seed=7900):
    """x: the layer's input (fine for a stride-2 layer, coarse for a transposed one), dy: the gradient of its output"""
    b = shape[0]
    out = tuple(2 * n for n in shape[1:]) if transposed else coarse_of(shape)[1:]
    x = seeded((b, cin) + tuple(shape[1:]), seed)
    wt = seeded(((cin, cout) if transposed else (cout, cin)) + (3, 3, 3), seed + 1, -0.2, 0.2)
    dy = seeded((b, cout) + out, seed + 2) * 1e-3
    return {"fwd": (x, wt), "dgrad": (dy, wt), "wgrad": (x, dy)}[kind]


def rows3(t, step, edit=None):
    """[B,C,D,H,W] (fp64) -> [B,Do,Ho,Wo,27,C]: the 27-tap neighbourhoods of the positions ::step; edit(xp) may change the
    zero-padded channels-last volume [B,D+2,H+2,W+2,C] first"""
    b, c, d, h, w = t.shape
    xp = F.pad(t.permute(0, 2, 3, 4, 1), (0, 0, 1, 1, 1, 1, 1, 1)).clone()
    if edit is not None:
        edit(xp)
    taps = [xp[:, kd:kd + d:step, kh:kh + h:step, kw:kw + w:step, :] for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(taps, dim=4)


def _tap(kd, kh, kw):
    return (kd * 3 + kh) * 3 + kw


def emulate_s2(kind, p, q, arith, geom, mutant=None):
    """the strided kernels' result in the emulated arithmetic: the defined products summed exactly per 32-deep K block (one tap x
    32 channels of a convolution launch, 32 positions of a weight gradient), the block sums accumulated in fp32"""
    terms = list(TERMS[arith])
    if mutant == "lohi_dropped":
        terms.remove((1, 0))
    pp, qq = R.split_parts(p, arith), R.split_parts(q, arith)
    if kind == "wgrad":
        cp, fp_ = (pp, qq) if geom.transposed else (qq, pp)  # coarse = x of a transposed layer, dy of a stride-2 one
        b, cm, dc, hc, wc = cp[0].shape
        cn = fp_[0].shape[1]
        m = torch.ones(b, dc, hc, wc, dtype=torch.float64)
        if mutant == "chunk_twice":      # the ragged last 8-position chunk of every row counted twice
            m[..., 8 * ((wc - 1) // 8):] = 2.0
        if mutant == "rowgroup_skipped":  # the ragged last 4-row group of every plane skipped
            m[:, :, 4 * ((hc - 1) // 4):, :] = 0.0
        if mutant == "odd_tail_dropped":  # the last coarse plane / row / column (the one an odd fine size adds) dropped
            m[:, dc - 1], m[:, :, hc - 1], m[..., wc - 1] = 0.0, 0.0, 0.0
        a = [t.permute(1, 0, 2, 3, 4).reshape(cm, -1) * m.reshape(-1) for t in cp]
        rows = [rows3(t, 2) for t in fp_]                        # [B,Dc,Hc,Wc,27,cn]
        assert rows[0].shape[1:4] == (dc, hc, wc)
        if mutant == "kw1_images_swapped":  # tap kw = 1 reads the odd-position image (what kw = 0 reads) instead of the even one
            for r in rows:
                for kd in range(3):
                    for kh in range(3):
                        r[..., _tap(kd, kh, 1), :] = r[..., _tap(kd, kh, 0), :]
        bm = [r.reshape(-1, 27 * cn) for r in rows]
        K = a[0].shape[1]
        acc = torch.zeros(cm, 27 * cn, dtype=torch.float32)
        for k0 in range(0, K, 32):
            acc = acc + sum(a[i][:, k0:k0 + 32] @ bm[j][k0:k0 + 32] for (i, j) in terms).float()
        return acc.reshape(cm, 27, cn).permute(0, 2, 1).reshape(cm, cn, 3, 3, 3)
    if (kind == "fwd") != geom.transposed:  # a mode-1 launch: the stride-2 convolution of p
        rows = [rows3(t, 2) for t in pp]
        wq = qq
    else:                                   # a mode-2 launch: the transposed convolution of p
        fine = geom.fine(p.shape[2:])
        dc = p.shape[2]

        def edit(xp):
            if mutant == "zero_plane_next_batch":  # behind the last coarse plane: the first plane of the next batch element
                xp[:-1, 2 * dc + 1] = xp[1:, 1].clone()

        rows = [rows3(R.zero_stuff(t, fine), 1, edit) for t in pp]
        wq = [t.transpose(0, 1).flip(2, 3, 4) for t in qq]
        od = torch.arange(rows[0].shape[1])
        odd_w = torch.arange(rows[0].shape[3]) % 2 == 1
        for r in rows:
            if mutant == "phase_dropped":          # the (pd, ph, pw) = (0, 0, 1) phase never multiplied
                r[:, 0::2, 0::2, 1::2] = 0.0
            if mutant == "phase_neighbour_tap":    # the pw = 1 phases read their two kw taps the other way round
                sw = r[:, :, :, odd_w].clone()
                for kd in range(3):
                    for kh in range(3):
                        sw[..., [_tap(kd, kh, 0), _tap(kd, kh, 2)], :] = sw[..., [_tap(kd, kh, 2), _tap(kd, kh, 0)], :]
                r[:, :, :, odd_w] = sw
            if mutant == "seam_carry_lost":        # fine plane 2 z + 1 of the last plane z of a segment loses coarse z's kd = 2 taps
                seam = (od % 2 == 1) & (((od - 1) // 2 + 1) % T_SEG_LEN == 0) & ((od - 1) // 2 + 1 < dc)
                r[:, seam, :, :, :9] = 0.0         # (the flipped image's kd' = 0 = the layer's kd = 2)
    b, do, ho, wo = rows[0].shape[:4]
    cout = wq[0].shape[0]
    a = [r.reshape(b * do * ho * wo, -1) for r in rows]
    bm = [t.permute(2, 3, 4, 1, 0).reshape(-1, cout) for t in wq]
    acc = torch.zeros(a[0].shape[0], cout, dtype=torch.float32)
    for k0 in range(0, a[0].shape[1], 32):
        acc = acc + sum(a[i][:, k0:k0 + 32] @ bm[j][k0:k0 + 32] for (i, j) in terms).float()
    y = acc.reshape(b, do, ho, wo, cout).permute(0, 4, 1, 2, 3).clone()
    if mutant == "odd_tail_dropped":
        y[:, :, do - 1], y[:, :, :, ho - 1], y[..., wo - 1] = 0.0, 0.0, 0.0
    return y


def ratios_s2(kind, transposed, shape, arith, mutant=None):
    geom = geom_of(transposed, shape)
    p, q = operands_s2(kind, transposed, shape)
    got = emulate_s2(kind, p, q, arith, geom, mutant)
    ex = R.exact(kind, p, q, geom=geom)
    assert got.shape == ex["y"].shape, (got.shape, ex["y"].shape)
    sref = R.split_reference(kind, p, q, arith, geom=geom)
    blocks = None
    if kind == "wgrad":
        blocks = R.wgrad_blocks_s2(p if transposed else q, 4, 8)
    return R.check(got, arith, R.products(kind, p, q, geom), ex, sref, R.amax_of(p), R.amax_of(q), blocks=blocks)


_EMU_S2 = [(False, s, k) for s in S2_FINE for k in R.KINDS] + [(False, s, k) for s in S2_ODD for k in ("fwd", "wgrad")]
_EMU_S2 += [(True, s, k) for s in T2_COARSE for k in R.KINDS]


@pytest.mark.parametrize("transposed,shape,kind", _EMU_S2, ids=[f"{'t2' if t else 's2'}-{k}-{s}" for (t, s, k) in _EMU_S2])
@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "fp32"])
def test_emulated_strided_arithmetic_passes_the_checks(arith, transposed, shape, kind, capsys):
    r = ratios_s2(kind, transposed, shape, arith)
    with capsys.disabled():
        print(f"\nemulated {'transposed' if transposed else 'stride-2'} {arith} {kind} {shape}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")
    assert max(r) <= 1.0, r


# the launches of the transposed map: the forward of a transposed layer (shape = coarse) and the input gradient of a stride-2
# one (shape = fine)
_MODE2 = [(True, s, "fwd") for s in T2_COARSE] + [(False, s, "dgrad") for s in S2_FINE]


def _coarse_dhw(transposed, shape):
    return shape[1:] if transposed else coarse_of(shape)[1:]


_WG = [(t, s, "wgrad") for t, shapes in ((False, S2_FINE + S2_ODD), (True, T2_COARSE)) for s in shapes]
MUTANTS_S2 = [  # (mutant, arithmetics, cases (transposed, shape, kind) it applies to)
    ("phase_dropped", R.ARITHS, _MODE2),
    ("phase_neighbour_tap", R.ARITHS, _MODE2),
    ("seam_carry_lost", R.ARITHS, [c for c in _MODE2 if _coarse_dhw(c[0], c[1])[0] > T_SEG_LEN]),
    ("zero_plane_next_batch", R.ARITHS, [c for c in _MODE2 if c[1][0] >= 2]),
    ("odd_tail_dropped", R.ARITHS, [(False, s, k) for s in S2_ODD for k in ("fwd", "wgrad")]),
    ("kw1_images_swapped", R.ARITHS, [c for c in _WG if not c[0]] + [c for c in _WG if c[0]]),
    ("chunk_twice", R.ARITHS, [c for c in _WG if _coarse_dhw(c[0], c[1])[2] % 8]),
    ("rowgroup_skipped", R.ARITHS, [c for c in _WG if _coarse_dhw(c[0], c[1])[1] % 4]),
    ("lohi_dropped", ("f16x3",), [(t, s, k) for (t, s, k) in _EMU_S2]),
]
_CASES_S2 = [(m, a, t, s, k) for (m, ariths, cases) in MUTANTS_S2 for a in ariths for (t, s, k) in cases]


@pytest.mark.parametrize("mutant,arith,transposed,shape,kind", _CASES_S2,
                         ids=[f"{m}-{a}-{'t2' if t else 's2'}-{k}-{s}" for (m, a, t, s, k) in _CASES_S2])
def test_strided_mutant_fails_a_check(mutant, arith, transposed, shape, kind, capsys):
    r = ratios_s2(kind, transposed, shape, arith, mutant)
    with capsys.disabled():
        print(f"\nstrided mutant {mutant} {arith} {kind} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert max(r) > 1.0, r


_AGREE = [(False, (2, 4, 6, 10)), (False, (1, 7, 5, 9)), (False, (1, 1, 6, 10)), (True, (2, 3, 4, 5)), (True, (1, 1, 3, 5))]


@pytest.mark.parametrize("transposed,shape", _AGREE, ids=[f"{'t2' if t else 's2'}-{s}" for (t, s) in _AGREE])
@pytest.mark.parametrize("kind", R.KINDS)
def test_strided_gemm_reference_is_the_convolution(kind, transposed, shape):
    """op_gemm on the strided geometries (an odd fine size and D = 1 among them) computes what torch's fp64 convolutions do"""
    geom = geom_of(transposed, shape)
    p, q = operands_s2(kind, transposed, shape, cin=32, cout=64)
    want, got = R.op(kind, p, q, geom), R.op_gemm(kind, p, q, geom)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("transposed,fine", [(False, (4, 6, 8)), (False, (5, 7, 3)), (True, (4, 6, 8))])
def test_strided_references_agree_with_a_direct_sum(transposed, fine):
    """op on the strided geometries against a seven-loop sum over (b, co, ci, coarse position, tap) written here: with
    f = 2 c - 1 + k,  stride-2: y[b,co,c] += x[b,ci,f] w[co,ci,k];  transposed: y[b,co,f] += x[b,ci,c] w[ci,co,k]"""
    b, cin, cout = 2, 2, 3
    coarse = tuple((n - 1) // 2 + 1 for n in fine)
    geom = R.Geom3d(2, transposed, None if transposed else fine)
    xs, ys = (coarse, fine) if transposed else (fine, coarse)
    x, dy = seeded((b, cin) + xs, 7990).double(), seeded((b, cout) + ys, 7992).double()
    wt = seeded(((cin, cout) if transposed else (cout, cin)) + (3, 3, 3), 7991).double()
    y, dx, dw = torch.zeros_like(dy), torch.zeros_like(x), torch.zeros_like(wt)
    K = {k: torch.zeros_like(t) for k, t in (("fwd", dy), ("dgrad", x), ("wgrad", wt))}
    for bi in range(b):
        for co in range(cout):
            for ci in range(cin):
                for c in [(i, j, l) for i in range(coarse[0]) for j in range(coarse[1]) for l in range(coarse[2])]:
                    for k in [(i, j, l) for i in range(3) for j in range(3) for l in range(3)]:
                        f = tuple(2 * ci_ - 1 + ki for ci_, ki in zip(c, k))
                        if any(v < 0 or v >= n for v, n in zip(f, fine)):
                            continue
                        xi, yi = ((bi, ci) + c, (bi, co) + f) if transposed else ((bi, ci) + f, (bi, co) + c)
                        wi = ((ci, co) if transposed else (co, ci)) + k
                        y[yi] += x[xi] * wt[wi]
                        dx[xi] += dy[yi] * wt[wi]
                        dw[wi] += x[xi] * dy[yi]
                        K["fwd"][yi] += 1
                        K["dgrad"][xi] += 1
                        K["wgrad"][wi] += 1
    for kind, (p, q), want in (("fwd", (x, wt), y), ("dgrad", (dy, wt), dx), ("wgrad", (x, dy), dw)):
        got = R.op(kind, p, q, geom)
        assert got.shape == want.shape, kind
        assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max()), kind
        assert float((R.op_gemm(kind, p, q, geom) - want).abs().max()) <= 1e-13 * float(want.abs().max()), kind
        assert torch.equal(R.products(kind, p, q, geom).expand_as(want), K[kind]), kind  # the count tensor: products per output
