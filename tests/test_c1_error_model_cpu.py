"""CPU: the checks of tests/_c1_fp64ref.py are sharp enough to catch a subtly wrong 32 -> 1 classifier convolution.

A plain fp32 emulation of the summation order of each kernel of az_conv3d_c1.hip (every FMA and add rounded to fp32 where the
kernel rounds; the forward's depth segments, the weight gradient's strided work lists, lane chains, shuffles and atomics in block
order) passes checks (a), (b) and (c); each mutant of it -- one defect of a class such a kernel could have -- fails at least one
check.  That is what says the GPU sweep (tests/test_gpu_c1_fp64.py) would fail on such a kernel; no mutant kernel is built or
run.  REJECTED_BY records, per mutant, the checks that must reject it, and the test asserts each of them.  Every mutant is
rejected by all three checks.  The narrowest are the weight-gradient walk defects at K = 30 750 positions (ntiles = 2050 for
2048 workgroups), which move a cell by about one tile's share of the sum: one tile counted twice stands at 5.6 x the bound of
(a), 177 x (b), 909 x (c); the two items beyond the grid dropped at 11.6 / 367 / 1662 -- the worst-case bound (a) of 2087 roundings
is the loosest there, the 2-norm bound (c) the sharpest."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import _c1_fp64ref as C1
from tests import _fp64ref as R
from tests._weights import seeded

NAN = float("nan")
SHAPES = [(1, 1, 1, 1), (1, 2, 1, 47), (2, 5, 7, 13), (1, 4, 8, 33)]
SEG_SHAPE, SEG_DSEG = (2, 5, 7, 13), 2          # forced segments [0, 2) [2, 4) [4, 5): the emulation's result does not depend on them
WALK_SHAPE = (1, 2050, 3, 5)                    # ntiles = 2050 > grid = 2048, K = 30 750


def f32(t):
    return t.float().double()


def fma(a, b, c):
    """fp32 fma of fp32 values held in fp64: the product is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return f32(a * b + c)


@pytest.fixture(scope="module")
def operands():
    cache = {}

    def get(shape):
        if shape not in cache:
            b, d, h, w = shape
            seed = 9100 + 7 * b + 3 * d + 5 * h + w
            cache[shape] = dict(x=seeded((b, 32, d, h, w), seed), w=seeded((1, 32, 3, 3, 3), seed + 1, -0.3, 0.3),
                                dy=seeded((b, 1, d, h, w), seed + 2) * 1e-3, addend=seeded((b, 1, d, h, w), seed + 3),
                                affine=C1.affine_pair(seed + 4))
        return cache[shape]
    return get


# ---- the emulations -----------------------------------------------------------------------------------------------------------------
def staged(x, affine, mutant):
    """the zero-padded operand [B, D+2, H+2, W+2, 32] as the kernels stage it (fp32 values in fp64)"""
    t = x.double().permute(0, 2, 3, 4, 1)
    pad = lambda u: F.pad(u, (0, 0, 1, 1, 1, 1, 1, 1))
    if affine is None:
        return pad(t)
    sc, sh = affine[0].double(), affine[1].double()
    act = (lambda u: u) if mutant == "affine_no_relu" else (lambda u: u.clamp_min(0.0))
    if mutant == "affine_on_padding":
        return act(fma(pad(t), sc, sh))
    return pad(act(fma(t, sc, sh)))


def emulate_fwd(x, wt, addend=None, affine=None, dseg=1, mutant=None):
    b, _, d, h, w = x.shape
    xp = staged(x, affine, mutant)
    wv = wt.double().reshape(32, 3, 3, 3).clone()
    if mutant == "tap_dropped":
        wv[5, 1, 2, 0] = 0.0
    if mutant == "kd_swapped":
        wv = wv.flip(1)
    acc = torch.zeros(b, d, h, w, 32, dtype=torch.float64)
    seg_first = torch.arange(d) % dseg == 0
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                src = xp[:, kd:kd + d, kh:kh + h, kw:kw + w, :]
                if mutant == "halo_zero" and kd == 0:  # plane d0 - 1 of every segment but the first is read as zero
                    src = src.clone()
                    src[:, seg_first & (torch.arange(d) > 0)] = 0.0
                acc = fma(src, wv[:, kd, kh, kw], acc)
    v = f32(acc[..., 0::2] + acc[..., 1::2])                    # the lane's channel pair
    for _ in range(4):                                        # quad_perm xor 1, xor 2, row_half_mirror, row_mirror
        v = f32(v[..., 0::2] + v[..., 1::2])
    out = v[..., 0]
    if addend is not None:
        plus = f32(out + addend.double()[:, 0])
        if mutant == "addend_skipped":
            plus[:, d - 1] = out[:, d - 1]
        out = plus
    if mutant == "ragged_unwritten" and d % dseg:
        out[:, d - 1] = NAN
    return out.float().unsqueeze(1)


def emulate_dgrad(dy, wt, mutant=None):
    b, _, d, h, w = dy.shape
    gp = F.pad(dy.double()[:, 0], (1, 1, 1, 1, 1, 1))
    wv = wt.double().reshape(32, 3, 3, 3)
    acc = torch.zeros(b, d, h, w, 32, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):  # gin[v] += gout[v + 1 - k] w[k]
                g = gp[:, 2 - kd:2 - kd + d, 2 - kh:2 - kh + h, 2 - kw:2 - kw + w]
                acc = fma(g.unsqueeze(-1), wv[:, kd, kh, kw], acc)
    if mutant == "x_tail":  # tx0 + lx0 + j < W - 1: the last column is never stored
        acc[:, :, :, w - 1] = NAN
    return acc.float().permute(0, 4, 1, 2, 3)


def emulate_wgrad(x, dy, affine=None, grid=None, mutant=None):
    """blocks walk items blk, blk + grid, ...; lane (wave = grp >> 3, grp & 7) of channel c chains 16 FMAs per item and tap"""
    b, _, d, h, w = x.shape
    ty_n, tx_n = -(-h // 8), -(-w // 32)
    ntiles = b * d * ty_n * tx_n
    grid = min(ntiles, C1.WGRAD_MAX_GRID) if grid is None else grid
    xs = staged(x, affine, mutant)[:, 1:-1, 1:-1, 1:-1]        # [B, D, H, W, 32] (the weight gradient reads no padding of x)
    xs = F.pad(xs, (0, 0, 0, 32 * tx_n - w, 0, 8 * ty_n - h))  # tiles read zeros beyond H, W
    if mutant == "ih_tail":                                    # ih < H - 1
        xs[:, :, h - 1] = 0.0
    gp = F.pad(dy.double()[:, 0], (1, 1 + 32 * tx_n - w, 1, 1 + 8 * ty_n - h, 1, 1))
    lists = [list(range(blk, ntiles, grid)) for blk in range(grid)]
    if mutant == "no_walk":
        lists = [l[:1] for l in lists]
    if mutant == "tile_twice":
        lists[grid // 2] = lists[grid // 2] + lists[grid // 2][:1]
    steps = max(len(l) for l in lists)
    item = torch.tensor([l + [-1] * (steps - len(l)) for l in lists])      # [grid, steps]
    live = (item >= 0).double()
    r = item.clamp_min(0)
    tx0, r = (r % tx_n) * 32, r // tx_n
    ty0, r = (r % ty_n) * 8, r // ty_n
    od, bi = r % d, r // d
    # only the lanes that ever hold a voxel inside the volume: the others add exact zeros
    gr_n, gc_n, p_n = min(4, h), min(8, -(-min(32, w) // 4)), -(-min(8, h) // 4)
    gr, gc = torch.arange(gr_n).view(1, -1, 1), torch.arange(gc_n).view(1, 1, -1)
    acc = torch.zeros(grid, gr_n, gc_n, 32, 27, dtype=torch.float64)
    for s in range(steps):
        B_, D_ = bi[:, s].view(-1, 1, 1), od[:, s].view(-1, 1, 1)
        for p in range(p_n):
            ih = ty0[:, s].view(-1, 1, 1) + 4 * p + gr
            for j in range(4):
                iw = tx0[:, s].view(-1, 1, 1) + 4 * gc + j
                xv = xs[B_, D_, ih, iw] * live[:, s].view(-1, 1, 1, 1)                       # [grid, gr, gc, 32]
                taps = [gp[B_, D_ + 2 - kd, ih + 2 - kh, iw + 2 - kw] for kd in range(3) for kh in range(3) for kw in range(3)]
                gv = torch.stack(taps, dim=-1)                                               # [grid, gr, gc, 27]
                acc = fma(gv.unsqueeze(-2), xv.unsqueeze(-1), acc)
    v = F.pad(acc, (0, 0, 0, 0, 0, 8 - gc_n))                  # the 8 lanes of a wave that share a channel quad
    for _ in range(3):                                         # __shfl_xor 8, 16, 32
        v = f32(v[:, :, 0::2] + v[:, :, 1::2])
    v = v[:, :, 0]                                             # [grid, waves, 32, 27]
    if mutant == "wave_lost":
        v[:, 0] = 0.0
    red = torch.zeros(grid, 32, 27, dtype=torch.float64)
    for wv in range(gr_n):                                     # LDS atomics, wave after wave
        red = f32(red + v[:, wv])
    gw = torch.zeros(32, 27, dtype=torch.float64)
    for blk in range(grid):                                    # global atomics, block after block
        gw = f32(gw + red[blk])
    return gw.float().reshape(1, 32, 3, 3, 3)


# ---- the verdicts -------------------------------------------------------------------------------------------------------------------
def verdict_fwd(o, shape, got, addend=False, affine=False):
    p, pre = C1.operand(o["x"], *(o["affine"] if affine else (None, None)))
    ex = R.exact("fwd", p, o["w"])
    grant = C1.operand_grant("fwd", pre, o["w"]) if affine else None
    return C1.check(got, "fwd", shape, ex, addend=o["addend"] if addend else None, grant=grant)


def verdict_wgrad(o, shape, got, affine=False):
    p, pre = C1.operand(o["x"], *(o["affine"] if affine else (None, None)))
    ex = R.exact("wgrad", p, o["dy"])
    grant = C1.operand_grant("wgrad", pre, o["dy"]) if affine else None
    return C1.check(got, "wgrad", shape, ex, grant=grant)


def show(capsys, label, r):
    with capsys.disabled():
        print(f"\n{label}: (a) {r[0]:.4g} (b) {r[1]:.4g} (c) {r[2]:.4g}")


@pytest.mark.parametrize("shape", SHAPES + [WALK_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_emulated_kernels_pass_all_checks(shape, operands, capsys):
    o = operands(shape)
    aff = o["affine"]
    walk = shape == WALK_SHAPE
    if walk:
        assert C1.plan(shape)[2:] == (2050, 2048)
    runs = [("wgrad", verdict_wgrad(o, shape, emulate_wgrad(o["x"], o["dy"]))),
            ("wgrad affine", verdict_wgrad(o, shape, emulate_wgrad(o["x"], o["dy"], affine=aff), affine=True))]
    if not walk:
        runs += [("fwd", verdict_fwd(o, shape, emulate_fwd(o["x"], o["w"]))),
                 ("fwd addend affine", verdict_fwd(o, shape, emulate_fwd(o["x"], o["w"], o["addend"], aff), addend=True, affine=True)),
                 ("dgrad", C1.check(emulate_dgrad(o["dy"], o["w"]), "dgrad", shape, R.exact("dgrad", o["dy"], o["w"])))]
    if shape == SEG_SHAPE:
        seg = emulate_fwd(o["x"], o["w"], o["addend"], aff, dseg=SEG_DSEG)
        assert torch.equal(seg, emulate_fwd(o["x"], o["w"], o["addend"], aff))
    for label, r in runs:
        show(capsys, f"emulated {label} {shape}", r)
        assert max(r) <= 1.0, (label, r)


# mutant -> (kind, shape, emulation keywords, verdict keywords, the checks that reject it)
ABC = (0, 1, 2)
REJECTED_BY = {
    "tap_dropped":       ("fwd", (1, 4, 8, 33), {}, {}, ABC),
    "kd_swapped":        ("fwd", (1, 4, 8, 33), {}, {}, ABC),
    "halo_zero":         ("fwd", SEG_SHAPE, dict(dseg=SEG_DSEG), {}, ABC),
    "ragged_unwritten":  ("fwd", SEG_SHAPE, dict(dseg=SEG_DSEG), {}, ABC),
    "affine_on_padding": ("fwd", (2, 5, 7, 13), dict(affine=True), dict(affine=True), ABC),
    "affine_no_relu":    ("fwd", (2, 5, 7, 13), dict(affine=True), dict(affine=True), ABC),
    "addend_skipped":    ("fwd", (1, 4, 8, 33), dict(addend=True), dict(addend=True), ABC),
    "x_tail":            ("dgrad", (1, 4, 8, 33), {}, {}, ABC),
    "tile_twice":        ("wgrad", WALK_SHAPE, {}, {}, ABC),
    "no_walk":           ("wgrad", WALK_SHAPE, {}, {}, ABC),
    "ih_tail":           ("wgrad", (2, 5, 7, 13), {}, {}, ABC),
    "wave_lost":         ("wgrad", (2, 5, 7, 13), {}, {}, ABC),
}
# further (mutant, shape) pairs: the weight gradient's fused operand, and the tile defects at a tiny K
ALSO = [("affine_on_padding", "wgrad", (2, 5, 7, 13), dict(affine=True), dict(affine=True), ()),  # the weight gradient reads no padding
        ("affine_no_relu", "wgrad", (2, 5, 7, 13), dict(affine=True), dict(affine=True), ABC),
        ("tile_twice", "wgrad", (1, 2, 1, 47), {}, {}, ABC),
        ("ih_tail", "wgrad", WALK_SHAPE, {}, {}, ABC)]
CASES = [(m,) + v for m, v in REJECTED_BY.items()] + ALSO


@pytest.mark.parametrize("mutant,kind,shape,ekw,vkw,rejecting", CASES, ids=[f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}" for c in CASES])
def test_mutants_are_rejected(mutant, kind, shape, ekw, vkw, rejecting, operands, capsys):
    o = operands(shape)
    ekw = dict(ekw)
    if ekw.pop("affine", False):
        ekw["affine"] = o["affine"]
    if kind == "fwd":
        if ekw.pop("addend", False):
            ekw["addend"] = o["addend"]
        r = verdict_fwd(o, shape, emulate_fwd(o["x"], o["w"], mutant=mutant, **ekw), **vkw)
    elif kind == "dgrad":
        r = C1.check(emulate_dgrad(o["dy"], o["w"], mutant=mutant), "dgrad", shape, R.exact("dgrad", o["dy"], o["w"]))
    else:
        r = verdict_wgrad(o, shape, emulate_wgrad(o["x"], o["dy"], mutant=mutant, **ekw), **vkw)
    show(capsys, f"mutant {mutant} {kind} {shape}", r)
    for i in range(3):
        if i in rejecting:
            assert r[i] > 1.0, (mutant, "abc"[i], r)
    if not rejecting:  # (a defect this kernel cannot have: its emulation is the correct one)
        assert max(r) <= 1.0, r


def test_the_restated_plan_is_the_library_s():
    """tests/_c1_fp64ref.py plan() against az_conv3d_c1_plan (host arithmetic only: no GPU is touched), with the refusals"""
    from activezero_amd import _lib, build
    build.build()
    lib = _lib.lib()
    out = (ctypes.c_longlong * 4)()
    shapes = [(b, d, h, w) for b in (1, 2, 3, 5) for d in (1, 2, 7, 20, 48, 97) for h in (1, 8, 9, 40, 64) for w in (1, 16, 17, 47, 130, 240)]
    shapes += [(1, 2050, 3, 5), (768, 3, 8, 16), (1, 48, 136, 240), (4, 48, 136, 240), (65535, 1, 1, 1), (1, 65535, 1, 1)]
    for s in shapes:
        assert lib.az_conv3d_c1_plan(out, *s) == 0 and tuple(out) == C1.plan(s), (s, tuple(out), C1.plan(s))
    einval, enull, eunsup = _lib.CONST["AZ_EINVAL"], _lib.CONST["AZ_ENULL"], _lib.CONST["AZ_EUNSUPPORTED"]
    assert [lib.az_conv3d_c1_plan(out, *s) for s in [(0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, -1)]] == [einval] * 4
    assert [lib.az_conv3d_c1_plan(out, *s) for s in [(65536, 3, 4, 5), (2, 65536, 4, 5)]] == [eunsup] * 2
    assert lib.az_conv3d_c1_plan(None, 2, 3, 4, 5) == enull
