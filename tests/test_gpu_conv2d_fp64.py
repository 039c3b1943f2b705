"""GPU: the 2-D convolution family -- forward, input gradient and weight gradient -- against fp64, element-wise, on every route
a layer of the feature extractor or of the factored cost-volume convolution can take, in both arithmetics (bf16x6, and f16x3:
the default of the training step): the batch-walking kernels of az_conv2d_roll.hip (NT 2 / NT 4 and the f16x3 64-channel
conv2d_roll64_kernel; plain, with the residual of the gradient hand-over, with the affine + ReLU epilogue, with BatchNorm
partials) including walks of three images with a shorter last segment, the generic conv2d_same_kernel of az_conv2d.hip with
every NW and geometry and with pixel strides wider than the channel counts, the patch route of firstconv.0 (az_im2col_s2k3 + a
1x1 layer on zero-padded channels + az_col2im_s2k3), and the weight gradients of az_conv2d_wgrad16.hip (AR 0, AR 1, w64) and
az_conv2d_wgrad.hip (MT x NT, 3x3 d2, 1x1, the three launches of 3x5) with row segments, column walks and work lists longer than
the grid, and the accumulate-only launch + unpack.

Each case asserts the route it takes from the library's own answers (conv2d._roll_ok, az_conv2d_wgrad_plan,
az_conv2d_roll_stats_rows) before it launches, prints the plan that shows what it walked, and runs the checks of
tests/_fp64ref.py (a), (b), (c) per output.  tests/test_conv_error_model_cpu.py shows that the checks reject the defects they are
meant to see; tests/test_gpu_switches.py runs this file again behind AZ_CONV2D_ROLL=0 and AZ_CONV2D_WGRAD_R16=0."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, amax, conv2d, overlap  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _fp64ref as R  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = torch.device("cuda:0")
ARITHS = ("bf16x6", "f16x3")
PAIRS = [(32, 32), (32, 64), (64, 32), (64, 64)]
G33, G33D2, G11, G35 = R.Geom2d(3, 3, 1), R.Geom2d(3, 3, 2), R.Geom2d(1, 1, 1), R.Geom2d(3, 5, 1)
SMALL = [(2, 13, 22), (1, 16, 32), (3, 5, 47), (2, 37, 53), (1, 1, 1)]
# batch walks of az_c2r_segments (asserted through az_conv2d_roll_stats_rows): seg_len 3 with a last segment of 2; seg_len 2 / 1
WALK3, WALK2, WALK3_G2 = (131, 9, 50), (13, 64, 80), (134, 9, 50)
# weight-gradient plans (asserted through az_conv2d_wgrad_plan): 770 columns for at most 768 workgroups per tile; row segments
# with an odd H and a shorter last segment for 768 / 384 / 192 and 256 slots per tile
COLWALK = (1, 3, 12320)
ROWSEG = {(32, 32): [(4, 47, 300)], (32, 64): [(5, 47, 150)], (64, 32): [(5, 47, 150)], (64, 64): [(3, 47, 150), (2, 24, 400)]}
LARGE = {WALK3, WALK2, WALK3_G2, COLWALK, (4, 47, 300), (5, 47, 150), (3, 47, 150), (2, 24, 400)}  # fp64 GEMMs on the GPU
K_R16_AR0, K_R16_AR1, K_W64, K_GENERIC = (_lib.CONST[f"AZ_C2W_KERNEL_{n}"] for n in ("R16_AR0", "R16_AR1", "W64", "GENERIC"))
WORST = {}  # (arith, kind) -> [max ratio a, b, c] over the cases run


def lib():
    return _lib.lib()


def opt(name):
    return lib().az_option(name.encode())


def rows(t):
    """[B,C,H,W] -> contiguous [B,H,W,C] rows on the GPU"""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(r):
    return r.detach().permute(0, 3, 1, 2)


def gname(g):
    return f"{g.kh}x{g.kw}d{g.dil}"


# ---- routes --------------------------------------------------------------------------------------------------------------------
def batch_walk(groups, b, h, w, cin, cout):
    """(segments per group, images per segment, images of the last segment) of the batch-walking kernels"""
    nrows = int(lib().az_conv2d_roll_stats_rows(groups, b, h, w, cin, cout))
    assert nrows > 0, nrows
    per = 4 * ((h + 7) // 8) * ((w + 15) // 16)
    assert nrows % per == 0
    nseg, n = nrows // per, b // groups
    seg_len = (n + nseg - 1) // nseg
    assert (nseg - 1) * seg_len < n <= nseg * seg_len
    return nseg, seg_len, n - (nseg - 1) * seg_len


def route_conv(ci, co, arith, shape, geom, variant="plain", cx=None, res_c=None, groups=1, force_roll=False):
    """the kernel a stride-1 launch ci -> co takes (ci, co: the LAUNCH's channels -- an input gradient is a forward of dy with
    the roles swapped), asserted against the wrapper's and the library's answers.  variant: plain / res / epi / stats"""
    b, h, w = shape
    xr = torch.empty(b, h, w, cx or ci, device="meta")
    res = torch.empty(b, h, w, res_c or co, device="meta") if variant in ("res", "epi") else None
    roll = conv2d._roll_ok(xr, ci, co, geom.kh, geom.kw, geom.dil, res)
    fits = geom == G33 and ci in (32, 64) and co in (32, 64) and cx in (None, ci) and res_c in (None, co)
    assert roll == (conv2d._ROLL2D and fits), (roll, conv2d._ROLL2D, fits)
    if roll or (force_roll and fits):  # (force_roll: the C ABI of the kernel, whatever the wrapper's switch says)
        kern = "roll64" if (arith == "f16x3" and co == 64) else ("roll NT4" if co == 64 else "roll NT2")
        nseg, seg_len, last = batch_walk(groups, b, h, w, ci, co)
        name = f"{kern} {arith} {variant}"
        if seg_len >= 3 and last < seg_len:
            name += " ragged-walk"
        return name + f" [nseg {nseg} seg_len {seg_len} last {last}]"
    nt = co // 32
    nw = 4 if nt % 4 == 0 else 3 if nt % 3 == 0 else 2 if nt % 2 == 0 else 1  # az_conv2d.hip dispatch_nw
    name = f"generic NW{nw} {gname(geom)} {arith} {variant}"
    if cx not in (None, ci):
        name += " in-stride"
    if res_c not in (None, co):
        name += " res-stride"
    return name


def wgrad_plan(arith, shape, cm, cn, geom):
    plan = (ctypes.c_longlong * 8)()
    rc = lib().az_conv2d_wgrad_plan(plan, int(arith == "f16x3"), *shape, cm, cn, geom.kh, geom.kw, geom.dil)
    assert rc == 0, rc
    return list(plan)


def route_wgrad(cin, cout, arith, shape, geom):
    """the kernel and plan of a weight gradient (coarse = dy: cm = cout, fine = x: cn = cin), from the library's plan query"""
    b, h, w = shape
    p = wgrad_plan(arith, shape, cout, cin, geom)
    r16 = geom == G33 and cin in (32, 64) and cout in (32, 64) and opt("AZ_CONV2D_WGRAD_R16")
    if r16:
        want = K_W64 if (arith == "f16x3" and cin == cout == 64) else (K_R16_AR1 if arith == "f16x3" else K_R16_AR0)
        assert p[0] == want, (p, want)
        _, seg_rows, nrseg, ncols, wgs, slots = p[:6]
        assert seg_rows % 2 == 0 and (nrseg - 1) * seg_rows < h <= nrseg * seg_rows and 1 <= wgs <= min(slots, ncols)
        assert ncols == b * ((w + 15) // 16) * nrseg
        name = {K_R16_AR0: "r16 AR0", K_R16_AR1: "r16 AR1", K_W64: "w64"}[p[0]]
        if nrseg >= 2 and h % 2 and h - (nrseg - 1) * seg_rows < seg_rows:
            name += " odd-seg"
        if ncols > wgs and ncols % wgs:
            name += " colwalk"
        return name + f" [seg_rows {seg_rows} nrseg {nrseg} last {h - (nrseg - 1) * seg_rows} ncols/wgs {ncols}/{wgs}]"
    assert p[0] == K_GENERIC, p
    _, mt, nt, blocks, hseg_rows, nhseg, nitems, launches = p
    assert (mt, nt) == (2 if cout % 64 == 0 else 1, 2 if cin % 64 == 0 else 1)
    assert (nhseg - 1) * hseg_rows < h <= nhseg * hseg_rows and nitems == b * ((w + 15) // 16) * nhseg and blocks % 8 == 0
    assert launches == (3 if geom == G35 else 1)
    name = f"generic {mt}x{nt} {gname(geom)} {arith}"
    if nitems > blocks:
        name += " items"
    if nhseg >= 2:
        name += " hseg"
    return name + f" [blocks {blocks} hseg_rows {hseg_rows} nhseg {nhseg} nitems {nitems}]"


# ---- operands, references, records ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def operands(cin, cout, shape, geom):
    b, h, w = shape
    seed = 7900 + 97 * (cin // 32) + 13 * (cout // 32) + 7 * b + 3 * h + w + 31 * geom.kw + geom.dil
    x = seeded((b, cin, h, w), seed)
    wt = seeded((cout, cin, geom.kh, geom.kw), seed + 1, -0.2, 0.2)
    dy = seeded((b, cout, h, w), seed + 2) * 1e-3
    return x, wt, dy


def pq(kind, x, wt, dy):
    return {"fwd": (x, wt), "dgrad": (dy, wt), "wgrad": (x, dy)}[kind]


def where(shape):
    return (DEV, True) if shape in LARGE else ("cpu", False)


@functools.lru_cache(maxsize=8)
def reference(kind, cin, cout, shape, geom):
    """fp64 result and magnitude sums, shared by the arithmetics and variants (large shapes: fp64 GEMMs on the GPU)"""
    p, q = pq(kind, *operands(cin, cout, shape, geom))
    dev, gemm = where(shape)
    return R.exact(kind, p.to(dev), q.to(dev), gemm=gemm, geom=geom)


def verdict(got, kind, cin, cout, shape, geom, arith, **kw):
    p, q = pq(kind, *operands(cin, cout, shape, geom))
    dev, gemm = where(shape)
    sref = R.split_reference(kind, p.to(dev), q.to(dev), arith, gemm=gemm, geom=geom)
    blocks = R.wgrad_blocks_2d(q) if kind == "wgrad" else None
    return R.check(got, arith, R.products(kind, p, q, geom), reference(kind, cin, cout, shape, geom), sref, R.amax_of(p),
                   R.amax_of(q), blocks=blocks, **kw)


def record(arith, kind, label, r, capsys):
    w = WORST.setdefault((arith, kind), [0.0, 0.0, 0.0, ""])
    if r[1] > w[1]:
        w[3] = label
    w[:3] = [max(u, v) for u, v in zip(w, r)]
    with capsys.disabled():
        print(f"\n{label}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")


# ---- launches through the entry points the network uses ------------------------------------------------------------------------
def run_conv(kind, cin, cout, arith, geom, src, wt, res=None):
    """forward (src = x rows) or input gradient (src = dy rows) through conv2d._run_same; NCHW result"""
    ci, co, flip = (cin, cout, False) if kind == "fwd" else (cout, cin, True)
    with torch.no_grad():
        return nchw(conv2d._run_same(src, src, wt, ci, co, geom.kh, geom.kw, geom.dil, flip, arith == "f16x3", res=res))


def launch(k, xr, wd, cin, cout, x_amax=None, **epilogue):
    """a 3x3 d1 layer's forward on the kernel of row k of conv2d.KERNELS, whatever conv2d._run_same would route it to"""
    with torch.no_grad():
        pk, w_am = conv2d._pack_image(k, wd, cin, cout, cin * 9, 9)
        return conv2d._launch(k, xr, pk, cin, cout, amax=(x_amax if x_amax is not None else amax.absmax(xr), w_am) if k.amax else None,
                              **epilogue)


def run_wgrad(cin, cout, arith, geom, xr, gr):
    with torch.no_grad():
        return conv2d._wgrad(gr, xr, cout, cin, cout, cin, geom.kh, geom.kw, geom.dil,
                             amax=(None, None) if arith == "f16x3" else None)


# (cin, cout, geometry, shape) of the forward / input-gradient sweep: the roll family at every pair and small shape and on the
# batch walks; the generic kernel with every NW (cout 128, 96, 64, 32 and 160 -- cin 128, so that the roll kernel does not take
# it -- and the input gradients' 128 -> NW 4) and every geometry
CONV = [(ci, co, G33, s) for (ci, co) in PAIRS for s in SMALL + [WALK3]]
CONV += [(64, 32, G33, WALK2), (32, 64, G33, WALK2)]
CONV += [(128, 128, G33, (2, 13, 22)), (128, 96, G33, (3, 5, 47)), (128, 64, G33, (2, 37, 53)), (128, 32, G33, (1, 16, 32)),
         (128, 160, G33, (1, 1, 1)), (128, 128, G33D2, (2, 37, 53)), (128, 128, G33D2, (1, 1, 1)), (64, 128, G11, (3, 5, 47)),
         (128, 32, G11, (2, 13, 22)), (32, 192, G35, (2, 13, 22)), (32, 192, G35, (1, 1, 1))]
CONV_CASES = [(ci, co, g, s, k, a) for (ci, co, g, s) in CONV for k in ("fwd", "dgrad") for a in ARITHS]
# (cin, cout, geometry, shape) of the weight-gradient sweep: r16 / w64 at every pair, small shape and plan shape; the generic
# kernel's four MT x NT at a small shape, with row segments and with more items than blocks, and its other geometries
WGRAD = [(ci, co, G33, s) for (ci, co) in PAIRS for s in SMALL + [COLWALK] + ROWSEG[(ci, co)]]
WGRAD += [(ci, co, G33, s) for (ci, co) in [(128, 64), (96, 64), (64, 96), (96, 96)] for s in [(2, 13, 22), (3, 47, 150)]]
WGRAD += [(128, 64, G33, COLWALK), (96, 96, G33, COLWALK)]
WGRAD += [(128, 128, G33D2, (2, 37, 53)), (64, 128, G11, (3, 5, 47)), (128, 32, G11, (1, 1, 1)), (32, 192, G35, (2, 13, 22)),
          (32, 192, G35, (3, 47, 150))]
WGRAD_CASES = [(ci, co, g, s, a) for (ci, co, g, s) in WGRAD for a in ARITHS]
RESIDUAL = [(ci, co, G33, s, a) for (ci, co) in PAIRS for s in [(2, 13, 22), (3, 5, 47), WALK3] for a in ARITHS]
RESIDUAL += [(128, 128, G33, (2, 13, 22), a) for a in ARITHS]
EPILOGUE = [(ci, co, s) for (ci, co) in PAIRS for s in [(2, 37, 53), WALK3]]  # bf16x6 affine + ReLU (+ residual)
STATS = [(ci, co, s, g, a) for (ci, co) in PAIRS for (s, g) in [(WALK3_G2, 2), (WALK3, 1)] for a in ARITHS]
STRIDED = [(a, k) for a in ARITHS for k in ("in", "res")]
PATCH = [(c, s) for c in (3, 6) for s in [(2, 13, 22), (1, 16, 32), (3, 5, 47), (1, 1, 1)]]


def all_routes():
    names = []
    for (ci, co, g, s, k, a) in CONV_CASES:
        names.append(route_conv(*((ci, co) if k == "fwd" else (co, ci)), a, s, g))
    for (ci, co, g, s, a) in RESIDUAL:
        names.append(route_conv(co, ci, a, s, g, "res"))
    for (ci, co, s) in EPILOGUE:
        names.append(route_conv(ci, co, "bf16x6", s, G33, "epi", force_roll=True))
    for (ci, co, s, grp, a) in STATS:
        names.append(route_conv(ci, co, a, s, G33, "stats", groups=grp, force_roll=True))
    for (a, k) in STRIDED:
        names.append(route_conv(64, 64, a, (2, 13, 22), G33, "res" if k == "res" else "plain",
                                cx=96 if k == "in" else None, res_c=96 if k == "res" else None))
    names += ["patch route bf16x6"] * bool(PATCH)
    for (ci, co, g, s, a) in WGRAD_CASES:
        names.append("wgrad " + route_wgrad(ci, co, a, s, g))
    return names


def test_every_route_of_the_family_is_swept():
    """the cases of this file together take every route the current switches leave to this family, the walking ones included"""
    names = all_routes()
    want = []
    if conv2d._ROLL2D:
        for kern in ("roll NT2 bf16x6", "roll NT4 bf16x6", "roll NT2 f16x3", "roll64 f16x3"):
            want += [(kern, "plain", "ragged-walk"), (kern, "res", "ragged-walk")]
    for kern in ("roll NT2 bf16x6", "roll NT4 bf16x6", "roll NT2 f16x3", "roll64 f16x3"):  # (through the C ABI)
        want += [(kern, "stats", "ragged-walk")]
    want += [("roll NT2 bf16x6", "epi", "ragged-walk"), ("roll NT4 bf16x6", "epi", "ragged-walk")]
    for a in ARITHS:
        want += [(f"generic NW{n}", a) for n in (1, 2, 3, 4)]
        want += [("generic", gname(g), a, "plain") for g in (G33, G33D2, G11, G35)]
        want += [("generic", a, "in-stride"), ("generic", a, "res-stride"), ("generic", a, " res")]
    want += [("patch route",)]
    if opt("AZ_CONV2D_WGRAD_R16"):
        for kern in ("r16 AR0", "r16 AR1", "w64"):
            want += [("wgrad", kern, "odd-seg"), ("wgrad", kern, "colwalk")]
    for a in ARITHS:
        want += [("wgrad generic", f"{m}x{n} 3x3d1", a) for m in (1, 2) for n in (1, 2)]
        want += [("wgrad generic", gname(g), a) for g in (G33D2, G11, G35)]
        want += [("wgrad generic", a, " items"), ("wgrad generic", a, " hseg")]
    missing = [w for w in want if not any(all(part in n for part in w) for n in names)]
    assert not missing, (missing, sorted(set(names)))


@pytest.mark.parametrize("cin,cout,geom,shape,kind,arith", CONV_CASES,
                         ids=[f"{k}-{ci}x{co}-{gname(g)}-{'x'.join(map(str, s))}-{a}" for (ci, co, g, s, k, a) in CONV_CASES])
def test_conv_vs_fp64(cin, cout, geom, shape, kind, arith, capsys):
    x, wt, dy = operands(cin, cout, shape, geom)
    name = route_conv(*((cin, cout) if kind == "fwd" else (cout, cin)), arith, shape, geom)
    got = run_conv(kind, cin, cout, arith, geom, rows(x if kind == "fwd" else dy), wt.to(DEV))
    r = verdict(got, kind, cin, cout, shape, geom, arith)
    record(arith, kind, f"{kind} {cin}->{cout} {gname(geom)} {shape} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("cin,cout,geom,shape,arith", RESIDUAL,
                         ids=[f"{ci}x{co}-{'x'.join(map(str, s))}-{a}" for (ci, co, g, s, a) in RESIDUAL])
def test_dgrad_residual_handover(cin, cout, geom, shape, arith, capsys):
    """dx = conv_transpose(dy) + the shortcut's gradient, added in the input-gradient launch (flipped packing)"""
    _, wt, dy = operands(cin, cout, shape, geom)
    res = seeded((shape[0], cin) + shape[1:], 7950) * 1e-2
    name = route_conv(cout, cin, arith, shape, geom, "res")
    got = run_conv("dgrad", cin, cout, arith, geom, rows(dy), wt.to(DEV), res=rows(res))
    r = verdict(got, "dgrad", cin, cout, shape, geom, arith, addend=res)
    record(arith, "dgrad", f"dgrad+residual {cin}->{cout} {shape} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("cin,cout,shape", EPILOGUE, ids=[f"{ci}x{co}-{'x'.join(map(str, s))}" for (ci, co, s) in EPILOGUE])
def test_roll_affine_relu_epilogue_bf16x6(cin, cout, shape, capsys):
    """relu(conv * scale + shift + res) of az_conv2d_roll_fwd (bf16x6; the f16x3 entry point is launched without scale / shift)"""
    x, wt, _ = operands(cin, cout, shape, G33)
    b, h, w = shape
    sc, sh = seeded((cout,), 7960) * 0.5 + 1.0, seeded((cout,), 7961) * 0.3
    sc[::5] *= -1.0
    res = seeded((b, cout, h, w), 7962) * 0.5
    name = route_conv(cin, cout, "bf16x6", shape, G33, "epi", force_roll=True)
    got = nchw(launch(conv2d.ROLL_X6, rows(x), wt.to(DEV), cin, cout, scale=sc.to(DEV), shift=sh.to(DEV), res=rows(res), relu=True))
    r = verdict(got, "fwd", cin, cout, shape, G33, "bf16x6", epilogue=(sc, sh, res, True))
    record("bf16x6", "fwd", f"fwd affine+relu+res {cin}->{cout} {shape} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("arith,which", STRIDED, ids=[f"{a}-{k}-stride" for (a, k) in STRIDED])
def test_generic_kernel_with_wide_pixel_strides(arith, which, capsys):
    """the input read as the first 64 channels of a 96-channel tensor (as costconv.py passes it) / the residual likewise; the
    other 32 channels hold large values that must not be read"""
    cin = cout = 64
    shape, geom = (2, 13, 22), G33
    b, h, w = shape
    x, wt, _ = operands(cin, cout, shape, geom)
    junk = torch.full((b, h, w, 32), 1.0e4, device=DEV)
    xr, res, rr = rows(x), None, None
    if which == "in":
        xr = torch.cat([xr, junk], dim=-1).contiguous()
    else:
        res = seeded((b, cout, h, w), 7970) * 0.5
        rr = torch.cat([rows(res), junk], dim=-1).contiguous()
    name = route_conv(cin, cout, arith, shape, geom, "res" if res is not None else "plain", cx=xr.shape[-1],
                      res_c=rr.shape[-1] if rr is not None else None)
    assert "generic" in name
    k = conv2d.KERNELS[f"gather {arith}"]
    out = launch(k, xr, wt.to(DEV), cin, cout, x_amax=amax.absmax(rows(x)) if k.amax else None, res=rr)
    r = verdict(nchw(out), "fwd", cin, cout, shape, geom, arith, addend=res)
    record(arith, "fwd", f"fwd {which}-stride 96 {cin}->{cout} {shape} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("cin,cout,shape,groups,arith", STATS,
                         ids=[f"{ci}x{co}-{'x'.join(map(str, s))}-g{g}-{a}" for (ci, co, s, g, a) in STATS])
def test_roll_stats_partials_on_a_batch_walk(cin, cout, shape, groups, arith, capsys):
    """the BatchNorm partials of the walking kernels with seg_len > 1 (one row per wave quarter and segment) and two statistic
    groups: every row written, counts exact, mean and variance within the tolerances of tests/test_gpu_conv2d_roll.py"""
    x, wt, _ = operands(cin, cout, shape, G33)
    b, h, w = shape
    name = route_conv(cin, cout, arith, shape, G33, "stats", groups=groups, force_roll=True)
    assert "ragged-walk" in name, name
    xr, wd = rows(x), wt.to(DEV)
    nrows = int(lib().az_conv2d_roll_stats_rows(groups, b, h, w, cin, cout))
    part = torch.full((groups, cout, nrows, 2), float("nan"), device=DEV)
    cnt = torch.full((groups, nrows), float("nan"), device=DEV)
    out = torch.empty(b, h, w, cout, device=DEV)
    k = conv2d.KERNELS[f"roll {arith}"]
    pk, w_am = conv2d._pack_image(k, wd, cin, cout, cin * 9, 9)
    am = (_p(amax.absmax(xr)), _p(w_am)) if k.amax else ()
    _call(k.stats[0], _p(out), _p(part), _p(cnt), _p(xr), _p(pk), *am, groups, b, h, w, cin, cout, _stream())
    torch.cuda.synchronize()
    r = verdict(nchw(out), "fwd", cin, cout, shape, G33, arith)
    record(arith, "fwd", f"fwd+stats {cin}->{cout} {shape} groups {groups} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)
    assert not torch.isnan(part).any() and not torch.isnan(cnt).any()
    n = cnt.double().sum(1)
    assert torch.equal(n.cpu(), torch.full((groups,), float(b // groups * h * w), dtype=torch.float64))
    mean = part[..., 0].double().sum(2) / n[:, None]
    tile_mean = part[..., 0].double() / cnt.double().clamp_min(1.0)[:, None, :]
    m2 = part[..., 1].double().sum(2) + (cnt.double()[:, None, :] * (tile_mean - mean[:, :, None]) ** 2).sum(2)
    ref = reference("fwd", cin, cout, shape, G33)["y"].to(DEV).permute(0, 2, 3, 1)
    rg = ref.reshape(groups, b // groups, h, w, cout)
    mean_ref, var_ref = rg.mean(dim=(1, 2, 3)), rg.var(dim=(1, 2, 3), unbiased=False)
    assert float(((mean - mean_ref).abs() / var_ref.sqrt()).max()) <= 1e-5
    assert float((m2 / n[:, None] / var_ref - 1).abs().max()) <= 1e-4


# ---- the patch route of firstconv.0 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,shape", PATCH, ids=[f"c{c}-{'x'.join(map(str, s))}" for (c, s) in PATCH])
def test_patch_route_vs_stride2_fp64(cin, shape, capsys):
    """3x3, stride 2, pad 1 on a 3- / 6-channel image -> 32 (bf16x6, as conv2d.conv routes it): az_im2col_s2k3 + a 1x1 layer on
    Kp = 32 / 64 channels of which 27 / 54 are real, its flipped 1x1 + az_col2im_s2k3, and the 1x1 weight gradient with
    cn_real < cn -- against the stride-2 convolution with K = 9 cin: what a pad channel contributes shows in check (b)"""
    b, h, w = shape
    cout = 32
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    geom = R.Geom2d(3, 3, 1, 2, (h, w))
    x = seeded((b, cin, h, w), 7980 + cin)
    wt = seeded((cout, cin, 3, 3), 7981, -0.2, 0.2)
    dy = seeded((b, cout, ho, wo), 7982) * 1e-3
    kp = conv2d._up(9 * cin, 32)
    assert kp == {3: 32, 6: 64}[cin] and wgrad_plan("bf16x6", (b, ho, wo), cout, kp, G11)[0] == K_GENERIC
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = wt.to(DEV).requires_grad_(True)
    y = conv2d._ConvS2Patches.apply(xg, wg, None, None, None)
    gx, gw = torch.autograd.grad(y, (xg, wg), dy.to(DEV).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    for kind, got in (("fwd", y.detach()), ("dgrad", gx), ("wgrad", gw)):
        p, q = pq(kind, x, wt, dy)
        ex = R.exact(kind, p, q, geom=geom)
        assert got.shape == ex["y"].shape
        sref = R.split_reference(kind, p, q, "bf16x6", geom=geom)
        r = R.check(got, "bf16x6", R.products(kind, p, q, geom), ex, sref, blocks=R.wgrad_blocks_2d(dy) if kind == "wgrad" else None)
        record("bf16x6", kind, f"{kind} patch route {cin}->{cout} {shape} [patch route bf16x6, Kp {kp}]", r, capsys)
        assert max(r) <= 1.0, (kind, r)


# ---- weight gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,geom,shape,arith", WGRAD_CASES,
                         ids=[f"{ci}x{co}-{gname(g)}-{'x'.join(map(str, s))}-{a}" for (ci, co, g, s, a) in WGRAD_CASES])
def test_wgrad_vs_fp64(cin, cout, geom, shape, arith, capsys):
    x, _, dy = operands(cin, cout, shape, geom)
    name = route_wgrad(cin, cout, arith, shape, geom)
    got = run_wgrad(cin, cout, arith, geom, rows(x), rows(dy))
    r = verdict(got, "wgrad", cin, cout, shape, geom, arith)
    record(arith, "wgrad", f"wgrad {cin}->{cout} {gname(geom)} {shape} [{name}]", r, capsys)
    assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("arith", ARITHS)
def test_accumulate_only_into_one_arena_then_unpack(arith, capsys):
    """grad_w = NULL launches (r16 / w64, a generic 3x3 and the three launches of 3x5) accumulate into slices of one zeroed
    arena, one az_wgrad_unpack_multi (overlap.Sink) writes the gradients; the words behind the arena stay untouched"""
    layers = [(32, 64, G33, (2, 13, 22)), (64, 64, G33, (3, 5, 47)), (96, 64, G33, (2, 13, 22)), (32, 64, G35, (1, 16, 32))]
    sizes = [(lib().az_conv2d_wgrad_workspace(co, ci, g.kh, g.kw) // 4 + 63) & ~63 for (ci, co, g, _) in layers]
    guard = 4096
    arena = torch.zeros(sum(sizes) + guard, device=DEV)
    sink = overlap.Sink(DEV)
    grads, keep, off = [], [], 0
    for (ci, co, g, shape), n in zip(layers, sizes):
        b, h, w = shape
        x, _, dy = operands(ci, co, shape, g)
        xr, gr = rows(x), rows(dy)
        ws = arena[off:off + n]
        off += n
        gw = torch.full((co, ci, g.kh, g.kw), float("nan"), device=DEV)
        route_wgrad(ci, co, arith, shape, g)
        if arith == "f16x3":
            am_g, am_x = amax.absmax(gr), amax.absmax(xr)
            keep += [am_g, am_x]
            _call("az_conv2d_wgrad_f16", None, _p(ws), n * 4, _p(gr), _p(xr), _p(am_g), _p(am_x), b, h, w, co, ci, co, ci, co, ci,
                  g.kh, g.kw, g.dil, _stream())
        else:
            _call("az_conv2d_wgrad", None, _p(ws), n * 4, _p(gr), _p(xr), b, h, w, co, ci, co, ci, co, ci, g.kh, g.kw, g.dil,
                  _stream())
        sink.defer_unpack(gw, ws, co, ci, co, ci, g.kh * g.kw)
        grads.append(gw)
        keep += [xr, gr]
    sink.stream.wait_stream(torch.cuda.current_stream())
    sink._flush_pending()
    torch.cuda.current_stream().wait_stream(sink.stream)
    torch.cuda.synchronize()
    assert float(arena[off:].abs().max()) == 0.0, "a launch wrote past its workspace"
    for (ci, co, g, shape), gw in zip(layers, grads):
        r = verdict(gw, "wgrad", ci, co, shape, g, arith)
        record(arith, "wgrad", f"wgrad accumulate-only + unpack {ci}->{co} {gname(g)} {shape}", r, capsys)
        assert max(r) <= 1.0, (ci, co, shape, r)


def test_worst_ratios_of_this_run(capsys):
    """the last test of the module: the largest ratio of each check per arithmetic and kind over the cases this run executed"""
    with capsys.disabled():
        print("\nworst err / bound per arithmetic and kind:  check (a)  check (b)  check (c)   [case of the largest (b)]")
        for (a, k), r in sorted(WORST.items()):
            print(f"  {a:7s} {k:6s}  " + "  ".join(f"{v:9.4f}" for v in r[:3]) + f"   {r[3]}")
    assert all(max(r[:3]) <= 1.0 for r in WORST.values())
