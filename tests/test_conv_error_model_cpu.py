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
