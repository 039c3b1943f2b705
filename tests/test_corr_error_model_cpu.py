"""CPU: the element-wise checks of tests/_corr_fp64ref.py are sharp enough to catch a subtly wrong correlation GEMM.

A pure-torch emulation of bgemm_x6_kernel (operands split as az_split3_bf16x4 splits them, the six products of az_mfma6_now summed
exactly per 16-deep K block, the block sums accumulated in fp32, the fp32 `* scale` of the epilogue) passes checks (a), (b) and
(c) at every GEMM shape of tests/test_gpu_corr_fp64.py for the volume and both gradients; each mutant of it -- one defect of a
class the kernel could have -- fails at least one check at every one of those shapes its class applies to.  This is what says
that the GPU sweep would fail on such a kernel; no mutant kernel is built or run.  The references themselves are pinned: the
einsums to a direct triple loop, the lookup reference to F.grid_sample(align_corners=True) as RAFT's bilinear_sampler calls it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _corr_fp64ref as CR
from tests import _fp64ref as R
from tests._weights import seeded

# (B, C, H, W1, W2): the GEMM shapes of tests/test_gpu_corr_fp64.py
SHAPES = [(1, 1, 1, 1, 1), (1, 3, 1, 2, 5), (2, 256, 3, 60, 60), (1, 40, 2, 65, 128), (1, 37, 2, 36, 31), (2, 32, 5, 130, 70),
          (1, 72, 2, 44, 52), (1, 24, 2, 68, 100), (3, 16, 70, 20, 20)]
# (part of A, part of B) of the six products; A is the kernel's first operand (f1 for the volume, G for the gradients)
TERMS = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]


def inputs(shape, seed=8100):
    b, c, h, w1, w2 = shape
    return seeded((b, c, h, w1), seed), seeded((b, c, h, w2), seed + 1), seeded((b, h, w1, w2), seed + 2)


def as_gemm(kind, t, which, mutant=None):
    """operand `which` (0: A [B,H,M,K], 1: B [B,H,N,K]) of the GEMM a contraction is, from the tensor as stored"""
    if which == 1 or kind == "vol":      # a feature map [B,C,H,W]: vol -> [B,H,W,C] (k = c); a gradient's B -> [B,H,C,W] (k = w)
        return t.permute(0, 2, 3, 1) if kind == "vol" else t.permute(0, 2, 1, 3)
    if mutant == "pitch_swapped":        # G [B,H,W1,W2] addressed as m W1 + n instead of m W2 + n, inside its (b, h) slab
        b, h, w1, w2 = t.shape
        idx = (torch.arange(w1)[:, None] * w1 + torch.arange(w2)[None, :]) % (w1 * w2)
        t = t.reshape(b, h, w1 * w2)[:, :, idx]
    return t if kind == "df1" else t.transpose(2, 3)  # df1: m = w1, k = w2; df2: m = w2, k = w1


def emulate(kind, p, q, c, mutant=None):
    """the kernel's result in the emulated arithmetic, in the layout of the kernel's output (fp32)"""
    terms = list(TERMS)
    if mutant == "lohi_dropped":
        terms.remove((2, 0))
    if mutant == "hi_only":
        terms = [(0, 0)]
    a = [as_gemm(kind, t, 0, mutant) for t in R.split_parts(p, CR.ARITH)]
    bm = [as_gemm(kind, t, 1) for t in R.split_parts(q, CR.ARITH)]
    if mutant == "next_slab":            # operand A of slab h read from slab h + 1 (the last one from the first)
        a = [t.roll(-1, 1) for t in a]
    k = a[0].shape[-1]
    kend = k
    if mutant == "chunk_tail_dropped":   # the last, partial 32-chunk of K never staged
        kend = k - k % 32
    if mutant == "group_tail_dropped":   # the `kk + 4 < K` predicate of the second 16-byte load applied to the whole 8-group:
        kend = k - k % 8                 # the last group, whose second four lies beyond K, contributes nothing
    acc = torch.zeros(a[0].shape[:3] + (bm[0].shape[2],), dtype=torch.float32)
    for k0 in range(0, kend, 16):
        k1 = min(k0 + 16, kend)
        blk = sum(torch.einsum("bhmk,bhnk->bhmn", a[i][..., k0:k1], bm[j][..., k0:k1]) for (i, j) in terms)
        acc = acc + blk.float()          # (one fp32 rounding of the exact block sum, one fp32 add)
    s = np.float32(1.0) / np.float32(c) if mutant == "scale_1_over_c" else np.float32(CR.scale(c))
    y = acc * torch.tensor(s, dtype=torch.float32)
    if mutant == "last_row_copied":      # the one row of the last M tile's wave written from the row before
        y[:, :, -1, :] = y[:, :, -2, :]
    return y if kind == "vol" else y.permute(0, 3, 1, 2)  # [B,H,M,N] -> [B,C = N,H,M]


def ratios(kind, shape, mutant=None):
    p, q = CR.operands(kind, *inputs(shape))
    c = shape[1]
    got = emulate(kind, p, q, c, mutant)
    ex = CR.exact(kind, p, q, c)
    assert got.shape == ex["y"].shape
    return CR.check(got, kind, shape, ex, CR.split_reference(kind, p, q, c))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", CR.KINDS)
def test_emulated_gemm_passes_the_checks(kind, shape, capsys):
    r = ratios(kind, shape)
    with capsys.disabled():
        print(f"\nemulated corr {kind} {shape}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")
    assert max(r) <= 1.0, r


def _outputs(kind, s):
    m, n, _ = CR.dims(kind, s)
    return s[0] * s[2] * m * n


# (mutant, applies(kind, shape))
MUTANTS = [
    ("lohi_dropped", lambda k, s: _outputs(k, s) > 1),
    ("hi_only", lambda k, s: True),
    ("chunk_tail_dropped", lambda k, s: CR.dims(k, s)[2] % 32 != 0),
    ("group_tail_dropped", lambda k, s: 1 <= CR.dims(k, s)[2] % 8 <= 4),
    ("last_row_copied", lambda k, s: CR.dims(k, s)[0] % 64 in (1, 33) and CR.dims(k, s)[0] > 1),
    ("scale_1_over_c", lambda k, s: s[1] > 1),
    ("next_slab", lambda k, s: s[2] > 1),
    ("pitch_swapped", lambda k, s: k != "vol" and s[3] != s[4]),
]
_CASES = [(m, k, s) for (m, applies) in MUTANTS for k in CR.KINDS for s in SHAPES if applies(k, s)]


def test_every_mutant_has_cases():
    assert {m for (m, _, _) in _CASES} == {m for (m, _) in MUTANTS}


@pytest.mark.parametrize("mutant,kind,shape", _CASES, ids=[f"{m}-{k}-{s}" for (m, k, s) in _CASES])
def test_mutant_fails_a_check(mutant, kind, shape, capsys):
    r = ratios(kind, shape, mutant)
    with capsys.disabled():
        print(f"\ncorr mutant {mutant} {kind} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert max(r) > 1.0, r


def test_references_agree_with_a_direct_sum():
    """the three einsums against a triple loop written here, and the scale against its definition"""
    b, c, h, w1, w2 = 2, 3, 2, 4, 5
    f1, f2, g = (t.double() for t in inputs((b, c, h, w1, w2), 8200))
    vol, df1, df2 = torch.zeros(b, h, w1, w2, dtype=torch.float64), torch.zeros_like(f1), torch.zeros_like(f2)
    for bi in range(b):
        for hi in range(h):
            for ci in range(c):
                for m in range(w1):
                    for n in range(w2):
                        vol[bi, hi, m, n] += f1[bi, ci, hi, m] * f2[bi, ci, hi, n]
                        df1[bi, ci, hi, m] += g[bi, hi, m, n] * f2[bi, ci, hi, n]
                        df2[bi, ci, hi, n] += g[bi, hi, m, n] * f1[bi, ci, hi, m]
    s = CR.scale(c)
    assert float(np.float32(s)) == s and abs(s - 1.0 / np.sqrt(3.0)) <= 2.0 ** -24  # an fp32 value, two roundings from exact
    for kind, want in (("vol", vol), ("df1", df1), ("df2", df2)):
        p, q = CR.operands(kind, f1, f2, g)
        ex = CR.exact(kind, p, q, c)
        assert ex["y"].shape == want.shape, kind
        assert float((ex["y"] - want * s).abs().max()) <= 1e-13 * float(want.abs().max()), kind
        assert bool((ex["S"] >= ex["y"].abs() * (1 - 1e-13)).all()) and bool((ex["Q2"] > 0).all())
        # the volume's gradients are its adjoints: <vol(f1, f2), G> = <f1, df1(G, f2)> = <f2, df2(G, f1)>
    dot = float((vol * g).sum())
    assert abs(float((f1 * df1).sum()) - dot) <= 1e-12 * abs(dot) and abs(float((f2 * df2).sum()) - dot) <= 1e-12 * abs(dot)


def _grid_sample_lookup(pyr, coord, radius, level):
    """one level of tests/test_gpu_raft_corr.py's _torch_reference: pyr [B,H,W1,Wl], coord [B,H,W1] -> [B,taps,H,W1] (fp32)"""
    b, h, w1, wl = pyr.shape
    r = radius
    dx = torch.linspace(-r, r, 2 * r + 1).view(1, 1, 2 * r + 1, 1)
    x0 = dx + coord.reshape(b * h * w1, 1, 1, 1) / 2 ** level
    grid = torch.cat([2 * x0 / (wl - 1) - 1, torch.zeros_like(x0)], -1)
    out = F.grid_sample(pyr.reshape(b * h * w1, 1, 1, wl), grid, align_corners=True)
    return out.view(b, h, w1, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("radius", [0, 4])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("wl", [9, 17, 33])
def test_lookup_reference_is_grid_sample(wl, level, radius):
    """W_level - 1 a power of two and coordinates multiples of 1/8: every step of both coordinate chains is exact, so the two
    may differ by the rounding of the interpolation only -- 1 - w, two products and an add: 4 2^-24 (|a| (1 - w) + |b| w)"""
    b, h, w1 = 2, 3, 37
    pyr = seeded((b, h, w1, wl), 8300 + wl)
    span = float((wl + 6) * 2 ** level)
    coord = torch.round(seeded((b, h, w1), 8301 + level, -3.0 * 2 ** level, span) * 8.0) / 8.0
    coord.view(-1)[:6] = torch.tensor([0.0, -1.0, wl - 1.0, float(wl), 0.125, wl - 1.125]) * 2 ** level
    ref, mag, integer = CR.lookup_fwd(pyr.numpy(), coord.numpy(), radius, level)
    ix = CR.lookup_ix(coord.numpy(), wl, radius, level).astype(np.float64)
    want_ix = coord.double().numpy()[..., None] / 2 ** level + (np.arange(2 * radius + 1) - radius)
    assert np.array_equal(ix, want_ix)  # the fp32 chain was exact
    got = _grid_sample_lookup(pyr, coord, radius, level).double().numpy()
    assert got.shape == ref.shape
    assert bool((np.abs(got - ref) <= 4.0 * R.U * mag).all()), float(np.abs(got - ref).max())
    assert np.array_equal(got[integer], ref[integer])
    assert integer.any() and (mag == 0).any() and ((mag > 0) & ~integer).any()  # inside, outside and between columns


def test_lookup_scatter_is_the_adjoint_of_the_lookup():
    """lookup_bwd's fp64 scatter against the definition: <lookup(pyr), g> = <pyr, scatter(g)>, and its counts"""
    b, h, w1, wl, radius, level = 2, 2, 11, 9, 4, 1
    pyr, g = seeded((b, h, w1, wl), 8400).numpy(), seeded((b, 2 * radius + 1, h, w1), 8401).numpy()
    coord = seeded((b, h, w1), 8402, -6.0, 2.0 * wl + 6.0).numpy()
    ref, _, _ = CR.lookup_fwd(pyr, coord, radius, level)
    sc, mag, cnt = CR.lookup_bwd(g, coord, wl, radius, level)
    lhs, rhs = float((ref * g.astype(np.float64)).sum()), float((pyr.astype(np.float64) * sc).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(mag.sum())
    assert bool((np.abs(sc) <= mag * (1 + 1e-15)).all()) and bool((mag[cnt == 0] == 0).all())
    assert cnt.max() <= 2 * (2 * radius + 1) and cnt.sum() > 0
