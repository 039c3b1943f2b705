"""GPU: the RAFT-Stereo 1-D correlation block of az_corr1d.hip against fp64, element-wise and per route.

The GEMM (bgemm_x6_kernel: the volume, d/d fmap1, d/d fmap2) is called through the C ABI with W1 != W2, dense cotangents and
outputs that lie inside a larger buffer filled with a NaN sentinel: every output element must be written, nothing around the
output may be.  Each case runs checks (a), (b), (c) of tests/_fp64ref.py through tests/_corr_fp64ref.py with the bf16x6
constants unchanged; tests/test_corr_error_model_cpu.py shows that those checks reject the defects they are meant to see.
test_every_route restates the kernel's routing rule (the <A_KFAST,B_KFAST> instantiation from the strides, 16-byte staging from
the divisibility of the contracted width, float4 stores from sDm and the row's alignment) and asserts that the shape list
reaches every branch, K tails beyond k = 64 on both staging paths among them.

The pool and lookup kernels are called on their own, on plain random pyramids: the pool bit-exact against numpy fp32, the lookup
against an fp64 interpolation at the kernel's own fp32 coordinate (tests/_corr_fp64ref.py lookup_ix), the scatter of its
gradient against the fp64 scatter of the same weights."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib  # noqa: E402
from activezero_amd.nets.raft.corr import CorrBlock1D  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _corr_fp64ref as CR  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = torch.device("cuda:0")
# (B, C, H, W1, W2): the smallest shapes that reach each branch of the kernel (test_every_route)
SHAPES = [(1, 1, 1, 1, 1), (1, 3, 1, 2, 5), (2, 256, 3, 60, 60), (1, 40, 2, 65, 128), (1, 37, 2, 36, 31), (2, 32, 5, 130, 70),
          (1, 72, 2, 44, 52), (1, 24, 2, 68, 100), (3, 16, 70, 20, 20)]
TOO_MANY_SLABS = (1, 1, 65536, 1, 1)
SETS = ("seeded", "pow2", "zero")
SENTINEL = 0x7FC0BEEF  # a NaN with a payload no arithmetic produces
WORST = {}  # (kind, route) -> [max ratio a, b, c]


# ---- the routing rule of az_corr1d.hip, restated once -----------------------------------------------------------------------------
def gemm_args(kind, shape):
    """element strides of the launch as az_corr1d_volume / az_corr1d_volume_bwd set them"""
    b, c, h, w1, w2 = shape
    m, n, k = CR.dims(kind, shape)
    if kind == "vol":
        a = dict(sk=h * w1, sr=1, b0=c * h * w1, b1=w1)
        bb = dict(sk=h * w2, sr=1, b0=c * h * w2, b1=w2)
        d = dict(sm=w2, sn=1, b0=h * w1 * w2, b1=w1 * w2)
    elif kind == "df1":
        a = dict(sk=1, sr=w2, b0=h * w1 * w2, b1=w1 * w2)
        bb = dict(sk=1, sr=h * w2, b0=c * h * w2, b1=w2)
        d = dict(sm=1, sn=h * w1, b0=c * h * w1, b1=w1)
    else:
        a = dict(sk=w2, sr=1, b0=h * w1 * w2, b1=w1 * w2)
        bb = dict(sk=1, sr=h * w1, b0=c * h * w1, b1=w1)
        d = dict(sm=1, sn=h * w2, b0=c * h * w2, b1=w2)
    return m, n, k, a, bb, d


def route(kind, shape):
    """(label, features) of a launch whose output starts at a 16-byte aligned address"""
    b, _, h, _, _ = shape
    m, n, k, a, bb, d = gemm_args(kind, shape)
    kfast = [o["sk"] == 1 and o["sr"] != 1 for o in (a, bb)]                        # launch_gemm: ak, bk
    vec = [kf and o["sr"] % 4 == 0 and o["b0"] % 4 == 0 and o["b1"] % 4 == 0 and k % 4 == 0 for kf, o in zip(kfast, (a, bb))]
    pair = "<%s,%s>" % tuple("T" if kf else "F" for kf in kfast)
    if any(kfast):
        assert len({v for v, kf in zip(vec, kfast) if kf}) == 1  # the k-fast operands of a launch stage the same way
        staging = "vector" if any(vec) else "scalar"
        assert (staging == "vector") == (k % 4 == 0)             # "vector staging from W % 4"
    else:
        staging = "strided"
    feats = {pair if staging == "strided" else f"{pair} {staging}"}
    if d["sm"] != 1 or m < 4:
        store = "scalar"
    else:  # float4 where the four rows exist and the address is aligned: per (b, h, n)
        res = {(bi * d["b0"] + hi * d["b1"] + ni * d["sn"]) % 4 for bi in range(b) for hi in range(h) for ni in range(n)}
        store = "float4" if res == {0} else "mixed" if 0 in res else "scalar"
    feats.add(f"store {store}")
    feats |= {f for f, on in (
        ("partial M tile", m % 64 != 0), ("partial N tile", n % 64 != 0),
        ("empty wave", 1 <= m % 64 <= 32 or 1 <= n % 64 <= 32),
        ("K < 32", k < 32), ("K % 32 in 1..7", 1 <= k % 32 <= 7), ("K % 8 in 5..7", 5 <= k % 8 <= 7),
        ("K % 8 in 1..4 vector", staging == "vector" and 1 <= k % 8 <= 4),
        ("K tail past 64 vector", staging == "vector" and k > 64 and k % 32 != 0),
        ("K tail past 64 scalar", staging == "scalar" and k > 64 and k % 32 != 0),
        ("many slabs", b * h > 128)) if on}
    return f"{pair} {staging}", feats


def test_every_route():
    reached = set()
    for s in SHAPES:
        for kind in CR.KINDS:
            label, feats = route(kind, s)
            print(f"{kind} {s}: {sorted(feats)}")
            reached |= feats
            if kind == "vol":
                assert label == "<F,F> strided" and "store scalar" in feats
    want = {"<F,F>", "<T,T> vector", "<T,T> scalar", "<F,T> vector", "<F,T> scalar", "store float4", "store scalar", "store mixed",
            "partial M tile", "partial N tile", "empty wave", "K < 32", "K % 32 in 1..7", "K % 8 in 1..4 vector", "K % 8 in 5..7",
            "K tail past 64 vector", "K tail past 64 scalar", "many slabs"}
    assert want <= reached, want - reached
    # <T,F> needs ak (W2 != 1) and !bk (H W2 == 1): no shape of the C ABI reaches it
    assert not any(f.startswith("<T,F>") for f in reached)
    assert route("df1", (1, 1, 1, 1, 1))[0] == route("df2", (1, 1, 1, 1, 1))[0] == "<F,F> strided"


# ---- operands and references ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(shape, which):
    b, c, h, w1, w2 = shape
    seed = 8500 + 1000 * SETS.index(which) + 7 * b + 3 * c + 5 * h + 11 * w1 + 13 * w2
    f1, f2, g = seeded((b, c, h, w1), seed), seeded((b, c, h, w2), seed + 1), seeded((b, h, w1, w2), seed + 2)
    if which == "pow2":   # per-channel powers of two from 2^-8 to 2^8 on one operand of each contraction: f1 (the volume's
        f1 = f1 * (2.0 ** ((torch.arange(c) * 5) % 17 - 8)).view(1, c, 1, 1)   # and d f2's), G along w2 (d f1's K axis)
        g = g * (2.0 ** ((torch.arange(w2) * 7) % 17 - 8)).view(1, 1, 1, w2)
    if which == "zero":   # an all-zero row of f1 and G and an all-zero column of G: their outputs are exactly zero
        f1[:, :, :, w1 // 2] = 0.0
        g[:, :, w1 // 2, :] = 0.0
        g[:, :, :, w2 // 3] = 0.0
    return f1, f2, g


@functools.lru_cache(maxsize=None)
def reference(kind, shape, which):
    p, q = CR.operands(kind, *inputs(shape, which))
    return CR.exact(kind, p, q, shape[1]), CR.split_reference(kind, p, q, shape[1])


def verdict(got, kind, shape, which, label, capsys):
    ex, sref = reference(kind, shape, which)
    assert tuple(got.shape) == tuple(ex["y"].shape)
    if which == "zero":
        z = got[:, :, shape[3] // 2, :] if kind == "vol" else got[..., shape[3] // 2] if kind == "df1" else got[..., shape[4] // 3]
        assert not bool(z.any())
    r = CR.check(got.cpu(), kind, shape, ex, sref)
    rt = route(kind, shape)[0]
    w = WORST.setdefault((kind, rt), [0.0, 0.0, 0.0])
    w[:] = [max(u, v) for u, v in zip(w, r)]
    with capsys.disabled():
        print(f"\ncorr {kind} {rt} {shape} {which} {label}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")
    return r


# ---- outputs inside a sentinel-filled buffer --------------------------------------------------------------------------------------
class Guarded:
    """an output tensor of `shape` inside a buffer of NaN sentinels, with a guard band of one tile row (64 x the widest pitch
    of the launch) before and after it; the output starts 16-byte aligned, as a tensor of its own would"""

    def __init__(self, shape, pitch):
        n = int(np.prod(shape))
        self.g = -(-64 * pitch // 4) * 4
        self.buf = torch.full((self.g + n + self.g,), SENTINEL, dtype=torch.int32, device=DEV)
        self.out = self.buf[self.g:self.g + n].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 0

    def settle(self):
        """the guards are untouched and every output element was written; returns the output"""
        torch.cuda.synchronize()
        g = self.g
        assert bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all()), "guard band written"
        inner = self.buf[g:-g]
        assert not bool((inner == SENTINEL).any()), f"{int((inner == SENTINEL).sum())} output elements not written"
        return self.out


def pitch(shape):
    _, _, h, w1, w2 = shape
    return h * max(w1, w2)


def run_volume(shape, f1, f2):
    b, c, h, w1, w2 = shape
    o = Guarded((b, h, w1, w2), pitch(shape))
    with torch.cuda.device(DEV):
        _call("az_corr1d_volume", _p(o.out), _p(f1), _p(f2), b, c, h, w1, w2, _stream())
    return o.settle()


def run_bwd(shape, f1, f2, g, want1=True, want2=True):
    b, c, h, w1, w2 = shape
    o1 = Guarded((b, c, h, w1), pitch(shape)) if want1 else None
    o2 = Guarded((b, c, h, w2), pitch(shape)) if want2 else None
    with torch.cuda.device(DEV):
        _call("az_corr1d_volume_bwd", _p(o1.out) if o1 else None, _p(o2.out) if o2 else None, _p(g), _p(f1), _p(f2),
              b, c, h, w1, w2, _stream())
    return (o1.settle() if o1 else None), (o2.settle() if o2 else None)


_IDS = [f"{s}-{w}" for s in SHAPES for w in SETS]
_CASES = [(s, w) for s in SHAPES for w in SETS]


@pytest.mark.parametrize("shape,which", _CASES, ids=_IDS)
def test_volume(shape, which, capsys):
    f1, f2, _ = (t.to(DEV) for t in inputs(shape, which))
    r = verdict(run_volume(shape, f1, f2), "vol", shape, which, "", capsys)
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("shape,which", _CASES, ids=_IDS)
def test_gradients(shape, which, capsys):
    """both gradients in one call, and each alone with the other pointer null: the same bits"""
    f1, f2, g = (t.to(DEV) for t in inputs(shape, which))
    g1, g2 = run_bwd(shape, f1, f2, g)
    r1 = verdict(g1, "df1", shape, which, "", capsys)
    r2 = verdict(g2, "df2", shape, which, "", capsys)
    a1, none2 = run_bwd(shape, f1, f2, g, want2=False)
    none1, a2 = run_bwd(shape, f1, f2, g, want1=False)
    assert none1 is None and none2 is None
    assert torch.equal(a1, g1) and torch.equal(a2, g2)
    assert max(r1) <= 1.0 and max(r2) <= 1.0, (r1, r2)


def test_autograd_with_a_dense_cotangent(capsys):
    """CorrBlock1D.corr and its backward: the cotangent is a dense tensor, not the pooled-back scatter of a lookup"""
    shape, which = (1, 37, 2, 36, 31), "seeded"
    f1, f2, g = inputs(shape, which)
    x1, x2 = f1.to(DEV).requires_grad_(), f2.to(DEV).requires_grad_()
    vol = CorrBlock1D.corr(x1, x2)
    b, c, h, w1, w2 = shape
    assert tuple(vol.shape) == (b, h, w1, 1, w2)
    g1, g2 = torch.autograd.grad(vol, (x1, x2), g.to(DEV).view(b, h, w1, 1, w2))
    rs = [verdict(vol.detach().view(b, h, w1, w2), "vol", shape, which, "autograd", capsys),
          verdict(g1, "df1", shape, which, "autograd", capsys), verdict(g2, "df2", shape, which, "autograd", capsys)]
    assert max(max(r) for r in rs) <= 1.0, rs


def test_too_many_slabs_is_refused_before_any_launch():
    b, c, h, w1, w2 = TOO_MANY_SLABS
    f = seeded((b, c, h, w1), 8490).to(DEV)
    g = seeded((b, h, w1, w2), 8491).to(DEV)
    outs = [torch.full((h,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)]
    lib, code = _lib.lib(), _lib.CONST["AZ_EUNSUPPORTED"]
    with torch.cuda.device(DEV):
        assert lib.az_corr1d_volume(_p(outs[0]), _p(f), _p(f), b, c, h, w1, w2, _stream()) == code
        assert lib.az_corr1d_volume_bwd(_p(outs[1]), _p(outs[2]), _p(g), _p(f), _p(f), b, c, h, w1, w2, _stream()) == code
        with pytest.raises(RuntimeError, match="az_corr1d_volume failed"):
            _call("az_corr1d_volume", _p(outs[0]), _p(f), _p(f), b, c, h, w1, w2, _stream())
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


def test_zz_largest_ratios_per_route(capsys):
    """the table of tests/_fp64ref.py: the largest ratio of each check per contraction and route over the cases run"""
    with capsys.disabled():
        print()
        for (kind, rt), w in sorted(WORST.items()):
            print(f"corr worst {kind:4s} {rt:14s} (a) {w[0]:.2f} (b) {w[1]:.2f} (c) {w[2]:.2f}")
    assert all(max(w) <= 1.0 for w in WORST.values())


# ---- the pool ---------------------------------------------------------------------------------------------------------------------
GRID_THREADS = 256 * 16 * 256  # az_grid_for's cap: beyond it a thread walks more than one element


@pytest.mark.parametrize("w", [2, 3, 75, 240])
@pytest.mark.parametrize("many", [False, True], ids=["one-pass", "grid-stride"])
def test_pool_and_its_gradient_are_bit_exact(w, many):
    rows = GRID_THREADS // (w // 2) + 3 if many else 7
    assert (rows * (w // 2) > GRID_THREADS) == many
    wd = w // 2
    src = seeded((rows, w), 8600 + w)
    gd = seeded((rows, wd), 8601 + w)
    dst = torch.full((rows, wd), float("nan"), device=DEV)
    gs = torch.full((rows, w), float("nan"), device=DEV)
    src_d, gd_d = src.to(DEV), gd.to(DEV)  # (named: the kernels read them after the call returns)
    with torch.cuda.device(DEV):
        _call("az_corr1d_pool", _p(dst), _p(src_d), rows, w, _stream())
        _call("az_corr1d_pool_bwd", _p(gs), _p(gd_d), rows, w, _stream())
    a = src.numpy()
    want = (a[:, 0:2 * wd:2] + a[:, 1:2 * wd:2]) * np.float32(0.5)
    assert want.dtype == np.float32 and np.array_equal(dst.cpu().numpy(), want)
    wg = np.zeros((rows, w), dtype=np.float32)
    wg[:, :2 * wd] = np.repeat(np.float32(0.5) * gd.numpy(), 2, axis=1)
    got = gs.cpu().numpy()
    assert np.array_equal(got, wg)
    if w % 2:  # the odd last column is written, as zero, over the NaN the buffer held
        assert not np.any(got[:, -1]) and not np.isnan(got).any()


# ---- the lookup -------------------------------------------------------------------------------------------------------------------
LB, LH = 2, 3
CH_OFF, CH_EXTRA = 5, 3  # the taps sit at channels [5, 5 + taps) of 5 + taps + 3


def lookup_coords(wl, level, seed):
    """[B,2,H,W1] coordinates: channel 0 holds every class of sampling position of a row of wl columns (in level pixels: the
    integers, exactly -1, 0, wl - 1 and wl, just inside and just outside each end, +-1e6, and positions in between), scaled by
    2^level (exact); channel 1 is NaN and must never be read"""
    f = np.float32
    cls = [f(v) for v in range(-2, min(wl, 12) + 2)] + [f(wl - 2), f(wl - 1), f(wl), f(wl + 1)]
    for edge in (f(-1.0), f(0.0), f(wl - 1), f(wl)):
        cls += [np.nextafter(edge, f(-np.inf)), np.nextafter(edge, f(np.inf)), edge - f(2.0 ** -10), edge + f(2.0 ** -10)]
    cls += [f(1e6), f(-1e6), f(0.5), f(wl - 1.5), f(0.25), f(wl / 2.0 + 0.375)]
    rnd = seeded((LB * LH * 48,), seed, -7.0, wl + 6.0).numpy()
    w1 = len(cls) + 48
    c0 = np.empty((LB, LH, w1), dtype=np.float32)
    for i in range(LB * LH):  # every (b, h) row holds every class, in a rotated order
        c0[i // LH, i % LH] = np.roll(np.concatenate([np.array(cls, dtype=np.float32), rnd[48 * i:48 * i + 48]]), 5 * i)
    c0 = c0 * f(2 ** level)
    assert np.isfinite(c0).all()
    coords = np.full((LB, 2, LH, w1), np.nan, dtype=np.float32)
    coords[:, 0] = c0
    return coords, c0, w1


_LOOKUPS = [(wl, r, lvl) for wl in (2, 9, 37, 240) for r in (0, 4) for lvl in range(4)]


@pytest.mark.parametrize("wl,radius,level", _LOOKUPS)
def test_lookup_forward(wl, radius, level):
    coords, c0, w1 = lookup_coords(wl, level, 8700 + wl)
    taps = 2 * radius + 1
    total = CH_OFF + taps + CH_EXTRA
    pyr = seeded((LB, LH, w1, wl), 8701 + wl + level)
    out = torch.full((LB, total, LH, w1), SENTINEL, dtype=torch.int32, device=DEV)
    pyr_d, coords_d = pyr.to(DEV), torch.from_numpy(coords).to(DEV)
    with torch.cuda.device(DEV):
        _call("az_corr1d_lookup_fwd", _p(out), _p(pyr_d), _p(coords_d), LB, LH, w1, wl, radius, level, CH_OFF, total, _stream())
    torch.cuda.synchronize()
    assert bool((out[:, :CH_OFF] == SENTINEL).all()) and bool((out[:, CH_OFF + taps:] == SENTINEL).all())
    got = out[:, CH_OFF:CH_OFF + taps].contiguous().view(torch.float32).cpu().numpy().astype(np.float64)
    ref, mag, integer = CR.lookup_fwd(pyr.numpy(), c0, radius, level)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    assert bool((err <= 4.0 * CR.U * mag).all()), float((err / np.maximum(4.0 * CR.U * mag, 1e-300)).max())
    assert np.array_equal(got[integer], ref[integer])
    assert integer.any() and (mag == 0).any() and ((mag > 0) & ~integer).any()  # on a column, outside the row, between columns


@pytest.mark.parametrize("wl,radius,level", _LOOKUPS)
def test_lookup_backward_and_accumulating_backward(wl, radius, level):
    coords, c0, w1 = lookup_coords(wl, level, 8800 + wl)
    taps = 2 * radius + 1
    total = CH_OFF + taps + CH_EXTRA
    gout = torch.full((LB, total, LH, w1), float("nan"))
    gout[:, CH_OFF:CH_OFF + taps] = seeded((LB, taps, LH, w1), 8801 + wl + level)
    init = seeded((LB, LH, w1, wl), 8802 + wl + level)
    plain = torch.full((LB, LH, w1, wl), float("nan"), device=DEV)
    acc = init.clone().to(DEV)
    cd, gd = torch.from_numpy(coords).to(DEV), gout.to(DEV)
    with torch.cuda.device(DEV):
        _call("az_corr1d_lookup_bwd", _p(plain), _p(gd), _p(cd), LB, LH, w1, wl, radius, level, CH_OFF, total, _stream())
        _call("az_corr1d_lookup_bwd_acc", _p(acc), _p(gd), _p(cd), LB, LH, w1, wl, radius, level, CH_OFF, total, _stream())
    ref, mag, cnt = CR.lookup_bwd(gout[:, CH_OFF:CH_OFF + taps].numpy(), c0, wl, radius, level)
    got = plain.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert bool((np.abs(got - ref) <= (cnt + 2.0) * CR.U * mag).all())
    assert not got[cnt == 0].any() and (cnt == 0).any() and bool((cnt >= 2).any()) == (radius > 0)
    i64 = init.numpy().astype(np.float64)  # what the buffer held is one more contribution to every element
    got = acc.cpu().numpy().astype(np.float64)
    assert bool((np.abs(got - (ref + i64)) <= (cnt + 3.0) * CR.U * (mag + np.abs(i64))).all())
    assert np.array_equal(got[cnt == 0], i64[cnt == 0])
