"""GPU: the strided half of the hourglass -- the stride-2 3x3x3 convolutions (conv1 / conv3) and the stride-2 transposed ones
(conv5 / conv6): forward, input gradient and weight gradient against fp64, element-wise, on every route a layer of this family
can take: the depth-rolling kernels az_conv3d_s2roll.hip (mode 1, 32 -> 64) and az_conv3d_t2roll.hip (mode 2, 64 -> 32) with
one-plane, multi-plane and ragged depth segments and pre-split inputs, az_conv3d_t2.hip, the mode-1 / mode-2 paths of the gather
kernel of az_conv3d.hip in all three arithmetics, the stride-2 weight gradient of az_conv3d_wgrad16s2.hip (split masks 0-2, its
column walk) and the stride-2 instantiations of the one-kd-per-wave kernels of az_conv3d_wgrad.hip.

A layer is (transposed, cin, cout); `shape` is (B, D, H, W) of its INPUT x: the fine size of a stride-2 layer, the coarse size of
a transposed one.  Each case asserts the route it takes before it launches and runs the checks of tests/_fp64ref.py with the
per-output product count K of the strided maps; it prints the three ratios (<= 1 passes), and the module prints the largest of
each per arithmetic, kind and route.  tests/test_conv_error_model_cpu.py shows that the checks reject the defects they are meant
to see.  tests/test_gpu_switches.py runs this file again behind the switches that change its routes.

Odd fine sizes: a stride-2 layer's forward and weight gradient take them (az_conv3d_s2roll.hip, the gather kernel -- whose
staging pads by comparing every fine coordinate with the size -- and both weight-gradient kernels); the bf16x6 / fp32 wrapper
refuses them but for D = 1 (conv3d._run_gather), and no input gradient exists for them, D = 1 included: a mode-2 launch writes
2 Dc planes / rows / columns, whatever the fine size was."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, amax, conv3d, overlap  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _fp64ref as R  # noqa: E402
from tests._weights import seeded  # noqa: E402
from tests.test_gpu_conv3d_s1 import (LAYOUT_GATHER, LAYOUT_ROLL, _sample_points, _sampled_reference, _split_operand, cl,  # noqa: E402
                                      ncdhw, r16_workgroups)

DEV = torch.device("cuda:0")
PAIRS = [(32, 32), (32, 64), (64, 32), (64, 64)]
S2_FINE = [(1, 2, 2, 2), (1, 1, 6, 10), (1, 4, 6, 10), (2, 6, 8, 20), (1, 2, 10, 34), (3, 4, 18, 30), (1, 14, 50, 34)]
S2_ODD = [(1, 7, 33, 65), (1, 3, 7, 13)]
T2_COARSE = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 4, 17), (1, 1, 5, 9), (3, 2, 9, 15), (1, 7, 25, 17)]
# the column walk of az_conv3d_wgrad16s2.hip by the fine channel count: ncols = B Dc ceil(Wc / 8) = 264 > 256, 132 > 128
WALK_COARSE = {32: (1, 12, 3, 176), 64: (1, 6, 3, 176)}
# patches * Di = 10 * 2 * 2 * 7 = 280 > 256: az_t2roll_segments gives 4 segments of 2 coarse planes, the last of 1
SEG_COARSE = (10, 7, 16, 32)
PREC = {"f16x3": conv3d.F16X3, "bf16x6": conv3d.BF16X6, "fp32": conv3d.FP32}
WORST = {}  # (arith, kind, route) -> [max ratio a, b, c] over the cases run


def lib():
    return _lib.lib()


def opt(name):
    return lib().az_option(name.encode())


def mode_of(transposed):
    return conv3d.DECONV_S2 if transposed else conv3d.CONV_S2


def out_dims(transposed, dhw):
    return tuple(2 * n for n in dhw) if transposed else tuple((n - 1) // 2 + 1 for n in dhw)


def geom_of(transposed, shape):
    if transposed:
        return R.Geom3d(2, True)
    return R.Geom3d(2, False, tuple(shape[1:]) if any(n % 2 for n in shape[1:]) else None)


def coarse_shape(transposed, shape):
    return shape if transposed else (shape[0],) + out_dims(False, shape[1:])


def fine_of(coarse):
    return (coarse[0],) + tuple(2 * n for n in coarse[1:])


# ---- Python mirrors of az_launch_math.h -----------------------------------------------------------------------------------------
def t2roll_segments(patches, di):
    """az_t2roll_segments -> (nseg, seg_len)"""
    best, nseg, seg_len = -1, 1, di
    for n in range(1, di + 1):
        ln = (di + n - 1) // n
        if (di + ln - 1) // ln != n:
            continue
        cost = ((patches * n + 255) // 256) * (ln * 4 + 2) + 1
        if best < 0 or cost < best:
            best, nseg, seg_len = cost, n, ln
    return nseg, seg_len


def s2roll_segments(patches, do, forced, slots=512):
    """az_s2roll_segments -> (nseg, seg_len)"""
    if forced > 0:
        seg_len = min(forced, do)
        return (do + seg_len - 1) // seg_len, seg_len
    best, nseg, seg_len = -1, 1, do
    for n in range(1, do + 1):
        ln = (do + n - 1) // n
        if (do + ln - 1) // ln != n:
            continue
        cost = ((patches * n + slots - 1) // slots) * (27 * ln + 4 * (2 * ln + 1) + 4)
        if best < 0 or cost < best:
            best, nseg, seg_len = cost, n, ln
    return nseg, seg_len


def _segs(name, depth, seg_len):
    return name + (" seg>1" if seg_len > 1 else "") + (" ragged seg" if depth % seg_len else "")


def route(kind, transposed, cin, cout, arith, shape, split_mask=0):
    """the kernel this call takes, asserted against the library's and the wrapper's own routing answers"""
    mode = mode_of(transposed)
    if kind in ("fwd", "dgrad"):
        if kind == "fwd":
            op, ci, co, dims = mode, cin, cout, shape
        else:  # a forward launch of the dual map on dy
            op, ci, co = conv3d._dgrad_launch(mode, cin, cout)[:3]
            dims = (shape[0],) + out_dims(transposed, shape[1:])
        b, d, h, w = dims
        operand = torch.empty(b, d, h, w, ci, device="meta")
        do, ho, wo = conv3d._out_dims(op, d, h, w)
        if arith == "f16x3":
            assert conv3d._f16_launch_ok(op, ci, co, operand)  # (no flat-address fallback at these sizes)
            lay = lib().az_conv3d_f16_layout(op, ci, co)
            if op == conv3d.CONV_S2 and (ci, co) == (32, 64) and opt("AZ_CONV_S2ROLL"):
                assert lay == LAYOUT_ROLL, lay
                _, seg_len = s2roll_segments(b * ((ho + 7) // 8) * ((wo + 15) // 16), do, opt("AZ_S2ROLL_SEGLEN"))
                name, depth = "s2roll f16x3", do
            elif op == conv3d.DECONV_S2 and (ci, co) == (64, 32) and opt("AZ_CONV_T2ROLL"):
                assert lay == LAYOUT_ROLL, lay
                _, seg_len = t2roll_segments(b * ((h + 7) // 8) * ((w + 15) // 16), d)
                name, depth = "t2roll f16x3", d
            else:
                assert lay == LAYOUT_GATHER, lay
                assert lib().az_conv3d_fwd_f16_split_ok(op, b, ci, co, d, h, w) == 0 and not split_mask
                return "t2 f16x3" if (op == conv3d.DECONV_S2 and co == 32) else f"gather m{op} f16x3"
            if split_mask:
                assert lib().az_conv3d_fwd_f16_split_ok(op, b, ci, co, d, h, w) == 1
                name += " presplit"
            return _segs(name, depth, seg_len)
        assert not split_mask
        assert conv3d._layout(PREC[arith], op, co) == PREC[arith]
        if arith == "bf16x6" and op == conv3d.DECONV_S2 and co == 32:
            return "t2 bf16x6"
        return f"gather m{op} {arith}"
    b, dc, hc, wc = coarse_shape(transposed, shape)
    df, hf, wf = out_dims(True, shape[1:]) if transposed else shape[1:]
    cm, cn = (cin, cout) if transposed else (cout, cin)  # coarse = x of a transposed layer, dy of a stride-2 one
    if arith != "f16x3":
        assert split_mask == 0
        return f"one-kd {arith}"
    assert conv3d._f16_wgrad_ok(mode, cin, cout)
    ok = lib().az_conv3d_wgrad_f16_split_ok(2, b, cm, cn, dc, hc, wc, df, hf, wf)
    if not (opt("AZ_WGRAD_S2R16") and cm == 64):
        assert ok == 0 and split_mask == 0
        return "one-kd f16x3"
    assert ok == 3  # (either operand; both at once: AZ_EUNSUPPORTED)
    ntiles = cn // 32
    ncols = b * dc * ((wc + 7) // 8)
    wgs = r16_workgroups(ncols, 256 // ntiles, ntiles, 0)
    return f"s2r16 mask {split_mask}" + (" walk" if ncols > wgs else "")


def wgrad_blocks(name, coarse):
    return R.wgrad_blocks_s2(coarse, 4, 8) if name.startswith("s2r16") else R.wgrad_blocks_s2(coarse, 1, 16)


def run(kind, transposed, cin, cout, arith, x, wt, dy, residual=None, **epi):
    """x, wt, dy on the GPU (channels-last volumes); the result in NCDHW / weight layout"""
    prec, mode = PREC[arith], mode_of(transposed)
    with torch.no_grad():
        if kind == "fwd":
            return ncdhw(conv3d._conv(x, wt, mode, prec, residual=residual, **epi))
        if kind == "dgrad":
            return ncdhw(conv3d._input_grad(dy, wt, mode, cin, cout, prec, residual=residual))
        return conv3d._weight_grad(x, dy, mode, cin, cout, prec)


@functools.lru_cache(maxsize=16)
def operands(transposed, cin, cout, shape):
    b, d, h, w = shape
    seed = 8100 + 1000 * int(transposed) + 97 * (cin // 32) + 13 * (cout // 32) + 7 * b + 5 * d + 3 * h + w
    x = seeded((b, cin, d, h, w), seed)
    wt = seeded(((cin, cout) if transposed else (cout, cin)) + (3, 3, 3), seed + 1, -0.2, 0.2)
    dy = seeded((b, cout) + out_dims(transposed, (d, h, w)), seed + 2) * 1e-3
    return x, wt, dy


def pq(kind, x, wt, dy):
    return {"fwd": (x, wt), "dgrad": (dy, wt), "wgrad": (x, dy)}[kind]


def is_large(transposed, shape):
    """shapes whose references are fp64 GEMMs on the GPU"""
    c = coarse_shape(transposed, shape)
    return c in WALK_COARSE.values() or c == SEG_COARSE


@functools.lru_cache(maxsize=16)
def reference(kind, transposed, cin, cout, shape):
    """fp64 result and magnitude sums, shared by the three arithmetics"""
    p, q = pq(kind, *operands(transposed, cin, cout, shape))
    gemm = is_large(transposed, shape)
    if gemm:
        p, q = p.to(DEV), q.to(DEV)
    return R.exact(kind, p, q, gemm=gemm, geom=geom_of(transposed, shape))


def verdict(got, kind, transposed, cin, cout, shape, arith, name, p=None, q=None, parts_p=None, parts_q=None, amax_p=None,
            amax_q=None, ex=None, **kw):
    """the three ratios of a result against the references of a case (p / q: operands that replace the case's own)"""
    geom = geom_of(transposed, shape)
    gemm = is_large(transposed, shape)
    dev = DEV if gemm else "cpu"
    if p is None:
        p, q = pq(kind, *operands(transposed, cin, cout, shape))
        ex = reference(kind, transposed, cin, cout, shape)
    elif ex is None:
        ex = R.exact(kind, p.to(dev), q.to(dev), gemm=gemm, geom=geom)
    mv = (lambda ps: None if ps is None else [t.to(dev) for t in ps])
    sref = R.split_reference(kind, p.to(dev), q.to(dev), arith, parts_p=mv(parts_p), parts_q=mv(parts_q), gemm=gemm, geom=geom)
    blocks = None
    if kind == "wgrad":
        blocks = wgrad_blocks(name, p if transposed else q)
    return R.check(got, arith, R.products(kind, p, q, geom), ex, sref, R.amax_of(p) if amax_p is None else amax_p,
                   R.amax_of(q) if amax_q is None else amax_q, blocks=blocks, **kw)


def record(arith, kind, name, label, r, capsys):
    w = WORST.setdefault((arith, kind, name), [0.0, 0.0, 0.0])
    w[:] = [max(u, v) for u, v in zip(w, r)]
    with capsys.disabled():
        print(f"\n{label} [{name}]: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}")


def tag(transposed, kind, cin, cout, shape, arith):
    return f"{'t2' if transposed else 's2'}-{kind}-{cin}x{cout}-{'x'.join(map(str, shape))}-{arith}"


def _walk_shape(transposed, cin, cout):
    """the input shape of a layer whose weight gradient walks its columns (None: a 32-channel coarse operand, no s2r16)"""
    cm, cn = (cin, cout) if transposed else (cout, cin)
    if cm != 64:
        return None
    c = WALK_COARSE[cn]
    return c if transposed else fine_of(c)


def _cases():
    out = []
    for (ci, co) in PAIRS:
        for t, shapes in ((False, S2_FINE), (True, T2_COARSE)):
            for s in shapes:
                # (a fine depth of 1 is an odd fine size: forward and weight gradient only, see the module docstring)
                out += [(t, ci, co, s, k, a) for k in R.KINDS for a in R.ARITHS if t or k != "dgrad" or not any(n % 2 for n in s[1:])]
            ws = _walk_shape(t, ci, co)
            if ws is not None:
                out += [(t, ci, co, ws, "wgrad", a) for a in R.ARITHS]
        for s in S2_ODD:  # (the bf16x6 / fp32 forward wrapper refuses odd sizes; a mode-2 launch cannot write them)
            out += [(False, ci, co, s, "fwd", "f16x3")] + [(False, ci, co, s, "wgrad", a) for a in R.ARITHS]
    return out


CASES = _cases()


@pytest.mark.parametrize("transposed,cin,cout,shape,kind,arith", CASES, ids=[tag(t, k, ci, co, s, a) for (t, ci, co, s, k, a) in CASES])
def test_strided_vs_fp64(transposed, cin, cout, shape, kind, arith, capsys):
    x, wt, dy = operands(transposed, cin, cout, shape)
    name = route(kind, transposed, cin, cout, arith, shape)
    got = run(kind, transposed, cin, cout, arith, cl(x), wt.to(DEV), cl(dy))
    r = verdict(got, kind, transposed, cin, cout, shape, arith, name)
    record(arith, kind, name, tag(transposed, kind, cin, cout, shape, arith), r, capsys)
    assert max(r) <= 1.0, (name, r)


# ---- t2roll with seg_len >= 2 and a ragged last segment: the carried kd = 2 accumulators across stages and segment seams ---------
SEG = [(True, 64, 32, SEG_COARSE, "fwd"), (False, 32, 64, fine_of(SEG_COARSE), "dgrad")]


@pytest.mark.parametrize("transposed,cin,cout,shape,kind", SEG, ids=[tag(t, k, ci, co, s, "f16x3") + "-seg" for (t, ci, co, s, k) in SEG])
def test_t2roll_carried_accumulators_across_segments(transposed, cin, cout, shape, kind, capsys):
    b, di, hi, wi = SEG_COARSE
    nseg, seg_len = t2roll_segments(b * ((hi + 7) // 8) * ((wi + 15) // 16), di)
    assert seg_len >= 2 and di % seg_len != 0 and nseg >= 2, (nseg, seg_len)
    name = route(kind, transposed, cin, cout, "f16x3", shape)
    if opt("AZ_CONV_T2ROLL"):
        assert "t2roll" in name and "seg>1" in name and "ragged seg" in name, name
    x, wt, dy = operands(transposed, cin, cout, shape)
    got = run(kind, transposed, cin, cout, "f16x3", cl(x), wt.to(DEV), cl(dy))
    r = verdict(got, kind, transposed, cin, cout, shape, "f16x3", name)
    record("f16x3", kind, name, tag(transposed, kind, cin, cout, shape, "f16x3"), r, capsys)
    assert max(r) <= 1.0, (name, r)


# ---- the gradient hand-over -------------------------------------------------------------------------------------------------------
RESIDUAL = [(t, ci, co, s, a) for (ci, co) in PAIRS for t, shapes in ((False, [(2, 6, 8, 20), (3, 4, 18, 30)]), (True, [(2, 3, 4, 17), (3, 2, 9, 15)]))
            for s in shapes for a in R.ARITHS]


@pytest.mark.parametrize("transposed,cin,cout,shape,arith", RESIDUAL, ids=[tag(t, "dgrad", ci, co, s, a) for (t, ci, co, s, a) in RESIDUAL])
def test_dgrad_residual_handover(transposed, cin, cout, shape, arith, capsys):
    """the gradient hand-over epilogue: dx = dgrad(dy) + residual, added in the input-gradient kernel"""
    x, wt, dy = operands(transposed, cin, cout, shape)
    res = seeded(tuple(x.shape), 8400) * 1e-2
    name = route("dgrad", transposed, cin, cout, arith, shape)
    got = run("dgrad", transposed, cin, cout, arith, None, wt.to(DEV), cl(dy), residual=cl(res))
    r = verdict(got, "dgrad", transposed, cin, cout, shape, arith, name, addend=res)
    record(arith, "dgrad", name, "residual " + tag(transposed, "dgrad", cin, cout, shape, arith), r, capsys)
    assert max(r) <= 1.0, (name, r)


# ---- the forward epilogues on every forward route ------------------------------------------------------------------------------------
EPILOGUE = [(t, ci, co, s, a) for (ci, co) in PAIRS for t, shapes in ((False, [(2, 6, 8, 20), (1, 14, 50, 34)]), (True, [(2, 3, 4, 17), (1, 7, 25, 17)]))
            for s in shapes for a in R.ARITHS]


@pytest.mark.parametrize("transposed,cin,cout,shape,arith", EPILOGUE, ids=[tag(t, "fwd", ci, co, s, a) for (t, ci, co, s, a) in EPILOGUE])
def test_forward_affine_residual_relu_epilogue(transposed, cin, cout, shape, arith, capsys):
    """relu(conv * scale + shift + res) in the kernel's epilogue"""
    x, wt, dy = operands(transposed, cin, cout, shape)
    sc, sh = seeded((cout,), 8410) * 0.5 + 1.0, seeded((cout,), 8411) * 0.3
    sc[::5] *= -1.0
    res = seeded(tuple(dy.shape), 8412) * 0.5
    name = route("fwd", transposed, cin, cout, arith, shape)
    got = run("fwd", transposed, cin, cout, arith, cl(x), wt.to(DEV), None, scale=sc.to(DEV), shift=sh.to(DEV), residual=cl(res),
              relu=True)
    r = verdict(got, "fwd", transposed, cin, cout, shape, arith, name, epilogue=(sc, sh, res, True))
    record(arith, "fwd", name + " epi", "epilogue " + tag(transposed, "fwd", cin, cout, shape, arith), r, capsys)
    assert max(r) <= 1.0, (name, r)
    assert float(got.min()) >= 0.0


@pytest.mark.parametrize("transposed,cin,cout,shape,arith", EPILOGUE, ids=[tag(t, "fwd", ci, co, s, a) for (t, ci, co, s, a) in EPILOGUE])
def test_forward_batchnorm_partials(transposed, cin, cout, shape, arith, capsys):
    """the BatchNorm-partials launch: its raw output through the three checks, its partials merged by Chan's rule (as
    az_bn3d_finalize) to the moments of that output, every output voxel counted once"""
    x, wt, _ = operands(transposed, cin, cout, shape)
    name = route("fwd", transposed, cin, cout, arith, shape)
    with torch.no_grad():
        raw, part, cnt, ntiles = conv3d._conv(cl(x), wt.to(DEV), mode_of(transposed), PREC[arith], stats=True)
    r = verdict(ncdhw(raw), "fwd", transposed, cin, cout, shape, arith, name)
    record(arith, "fwd", name + " stats", "stats " + tag(transposed, "fwd", cin, cout, shape, arith), r, capsys)
    assert max(r) <= 1.0, (name, r)
    part, cnt = part.double().cpu(), cnt.double().cpu()
    assert tuple(part.shape) == (cout, ntiles, 2)
    vox = raw.numel() // cout
    assert float(cnt.sum()) == vox  # every output voxel counted once
    y = raw.double().reshape(-1, cout).cpu()
    mean = part[:, :, 0].sum(1) / vox
    torch.testing.assert_close(mean, y.mean(0), rtol=1e-5, atol=1e-6)
    live = cnt > 0
    tile_mean = torch.where(live, part[:, :, 0] / cnt.clamp_min(1.0), torch.zeros_like(part[:, :, 0]))
    m2 = (part[:, :, 1] + cnt * (tile_mean - mean[:, None]) ** 2 * live).sum(1)
    torch.testing.assert_close(m2 / vox, y.var(0, unbiased=False), rtol=2e-4, atol=1e-7)


# ---- pre-split operands (include/azhip.h "S2 format") ---------------------------------------------------------------------------------
# the layers whose input-gradient launch stages a pre-split input: conv1 (t2roll, dy coarse 64 channels) and conv6 (s2roll)
PRESPLIT_DGRAD = [(False, 32, 64, s) for s in [(2, 6, 8, 20), (3, 4, 18, 30), (1, 14, 50, 34)]]
PRESPLIT_DGRAD += [(True, 64, 32, s) for s in [(2, 3, 4, 17), (3, 2, 9, 15), (1, 7, 25, 17)]]


def _dgrad_on_roll(transposed):
    return bool(opt("AZ_CONV_S2ROLL") if transposed else opt("AZ_CONV_T2ROLL"))


@pytest.mark.parametrize("transposed,cin,cout,shape", PRESPLIT_DGRAD,
                         ids=[tag(t, "dgrad", ci, co, s, "f16x3") + "-presplit" for (t, ci, co, s) in PRESPLIT_DGRAD])
def test_dgrad_presplit_operand_vs_fp64(transposed, cin, cout, shape, capsys):
    if not conv3d.PRESPLIT or not _dgrad_on_roll(transposed):
        pytest.skip("AZ_PRESPLIT=0 / the rolling kernel is switched off: the launch reads floats only")
    _, wt, dy = operands(transposed, cin, cout, shape)
    split, plain, parts_dy, am_dy = _split_operand(cl(dy), 8430)
    dyv = ncdhw(plain).cpu()
    name = route("dgrad", transposed, cin, cout, "f16x3", shape, split_mask=1)
    assert "presplit" in name
    with torch.no_grad():
        got = ncdhw(conv3d._input_grad(split, wt.to(DEV), mode_of(transposed), cin, cout, conv3d.F16X3))
    r = verdict(got, "dgrad", transposed, cin, cout, shape, "f16x3", name, p=dyv, q=wt, parts_p=parts_dy, amax_p=am_dy)
    record("f16x3", "dgrad", name, tag(transposed, "dgrad", cin, cout, shape, "f16x3"), r, capsys)
    assert max(r) <= 1.0, (name, r)


def _presplit_wgrad_cases():
    out = []
    for (t, ci, co) in [(False, 32, 64), (False, 64, 64), (True, 64, 32), (True, 64, 64)]:  # coarse 64 channels: s2r16
        small = [(2, 3, 4, 17), (3, 2, 9, 15)] if t else [(2, 6, 8, 20), (3, 4, 18, 30)]
        out += [(t, ci, co, s, m) for s in small + [_walk_shape(t, ci, co)] for m in (1, 2)]
    return out


PRESPLIT_WGRAD = _presplit_wgrad_cases()


def _wgrad_f16_operands(transposed, x, dy):
    """(coarse, fine, cm, cn, tag) as conv3d._weight_grad_f16 passes them"""
    return (x, dy) if transposed else (dy, x)


@pytest.mark.parametrize("transposed,cin,cout,shape,mask", PRESPLIT_WGRAD,
                         ids=[tag(t, "wgrad", ci, co, s, "f16x3") + f"-mask{m}" for (t, ci, co, s, m) in PRESPLIT_WGRAD])
def test_wgrad_presplit_operands_vs_fp64(transposed, cin, cout, shape, mask, capsys):
    if not conv3d.PRESPLIT or not opt("AZ_WGRAD_S2R16"):
        pytest.skip("AZ_PRESPLIT=0 / AZ_WGRAD_S2R16=0: the one-kd-per-wave kernels read floats only")
    x, wt, dy = operands(transposed, cin, cout, shape)
    xg, dg = cl(x), cl(dy)
    parts_x = parts_dy = None
    am_x, am_dy = R.amax_of(x), R.amax_of(dy)
    x_is_coarse = transposed
    if bool(mask & 1) == x_is_coarse:  # the pre-split operand is x
        xg, plain, parts_x, am_x = _split_operand(xg, 8420)
        x = ncdhw(plain).cpu()
    else:
        dg, plain, parts_dy, am_dy = _split_operand(dg, 8410)
        dy = ncdhw(plain).cpu()
    name = route("wgrad", transposed, cin, cout, "f16x3", shape, split_mask=mask)
    coarse, fine = _wgrad_f16_operands(transposed, xg, dg)
    cm, cn = (cin, cout) if transposed else (cout, cin)
    with torch.no_grad():
        got = conv3d._wgrad_f16(coarse, fine, 2, cm, cn, "deconv" if transposed else "conv")
    r = verdict(got, "wgrad", transposed, cin, cout, shape, "f16x3", name, p=x, q=dy, parts_p=parts_x, parts_q=parts_dy,
                amax_p=am_x, amax_q=am_dy)
    record("f16x3", "wgrad", name, tag(transposed, "wgrad", cin, cout, shape, "f16x3"), r, capsys)
    assert max(r) <= 1.0, (name, r)


def test_wgrad_with_both_operands_presplit_is_refused():
    """split mask 3 on the stride-2 kernel: AZ_EUNSUPPORTED through _call, nothing launched (the workspace stays as it was)"""
    b, dc, hc, wc = 1, 2, 3, 5
    coarse, fine = torch.zeros(b, dc, hc, wc, 64, device=DEV), torch.zeros(b, 2 * dc, 2 * hc, 2 * wc, 32, device=DEV)
    am = torch.ones(amax.AMAX_SLOTS, device=DEV)
    n = lib().az_conv3d_wgrad_workspace(64, 32) // 4
    ws = torch.full((n,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        _call("az_conv3d_wgrad_f16", None, _p(ws), n * 4, _p(coarse), _p(fine), _p(am), _p(am), 3, 2, b, 64, 32, dc, hc, wc,
              2 * dc, 2 * hc, 2 * wc, _stream())
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all())


# ---- accumulate-only weight gradients + one unpack of the pass (overlap.Sink) ----------------------------------------------------------
def test_accumulate_only_into_one_arena_then_unpack(capsys):
    layers = [(False, 32, 64, (2, 6, 8, 20)), (True, 64, 32, (3, 2, 9, 15))]  # (transposed, cin, cout, shape)
    dims = [((ci, co) if t else (co, ci)) for (t, ci, co, _) in layers]      # (cm, cn)
    sizes = [(lib().az_conv3d_wgrad_workspace(cm, cn) // 4 + 63) & ~63 for (cm, cn) in dims]
    guard = 4096
    arena = torch.zeros(sum(sizes) + guard, device=DEV)
    sink = overlap.Sink(DEV)
    grads, keep, off, names = [], [], 0, []
    for (t, ci, co, shape), (cm, cn), n in zip(layers, dims, sizes):
        x, wt, dy = operands(t, ci, co, shape)
        coarse, fine = _wgrad_f16_operands(t, cl(x), cl(dy))
        am_c, am_f = amax.absmax(coarse), amax.absmax(fine)
        ws = arena[off:off + n]
        off += n
        gw = torch.full((cm, cn, 3, 3, 3), float("nan"), device=DEV)
        names.append(route("wgrad", t, ci, co, "f16x3", shape))
        _call("az_conv3d_wgrad_f16", None, _p(ws), n * 4, _p(coarse), _p(fine), _p(am_c), _p(am_f), 0, 2, coarse.shape[0], cm, cn,
              *coarse.shape[1:4], *fine.shape[1:4], _stream())
        sink.defer_unpack(gw, ws, cm, cn, cm, cn, 27)
        grads.append(gw)
        keep += [coarse, fine, am_c, am_f]
    sink.stream.wait_stream(torch.cuda.current_stream())
    sink._flush_pending()
    torch.cuda.current_stream().wait_stream(sink.stream)
    torch.cuda.synchronize()
    assert float(arena[off:].abs().max()) == 0.0, "a launch wrote past its workspace"
    for (t, ci, co, shape), gw, name in zip(layers, grads, names):
        r = verdict(gw, "wgrad", t, ci, co, shape, "f16x3", name)
        record("f16x3", "wgrad", name, "accumulate-only + unpack " + tag(t, "wgrad", ci, co, shape, "f16x3"), r, capsys)
        assert max(r) <= 1.0, (t, ci, co, shape, r)


# ---- one production-size layer pair: B = 1, V0 <-> V1, f16x3 ----------------------------------------------------------------------------
FULL_FINE = (1, 48, 136, 240)


def _stuffed_cl(t_cl, fine_dhw):
    z = torch.zeros((t_cl.shape[0],) + tuple(fine_dhw) + (t_cl.shape[-1],), device=t_cl.device)
    z[:, ::2, ::2, ::2, :] = t_cl
    return z


@pytest.mark.parametrize("transposed", [False, True], ids=["s2-32x64-V0toV1-f16x3", "t2-64x32-V1toV0-f16x3"])
def test_full_size_layer_f16x3(transposed, capsys):
    """the weight gradient at its production size element-wise against fp64 GEMMs; forward and input gradient at sampled
    outputs (the faces and 4096 random voxels), each from its own neighbourhood"""
    cin, cout = (64, 32) if transposed else (32, 64)
    fine, coarse = FULL_FINE, coarse_shape(False, FULL_FINE)
    shape = coarse if transposed else fine
    g = torch.Generator(device=DEV).manual_seed(8500 + int(transposed))
    rnd = (lambda *s: torch.rand(*s, generator=g, device=DEV) * 2 - 1)
    x = rnd(*shape, cin)
    dy = rnd(shape[0], *out_dims(transposed, shape[1:]), cout) * 1e-3
    wt = rnd(*((cin, cout) if transposed else (cout, cin)), 3, 3, 3) * 0.2
    geom = geom_of(transposed, shape)
    for kind in R.KINDS:
        name = route(kind, transposed, cin, cout, "f16x3", shape)
        got = run(kind, transposed, cin, cout, "f16x3", x, wt, dy)
        if kind == "wgrad":
            p, q = ncdhw(x), ncdhw(dy)
            ex = R.exact("wgrad", p, q, gemm=True, geom=geom)
            sref = R.split_reference("wgrad", p, q, "f16x3", gemm=True, geom=geom)
            r = R.check(got, "f16x3", R.products("wgrad", p, q, geom), ex, sref, R.amax_of(x), R.amax_of(dy),
                        blocks=wgrad_blocks(name, p if transposed else q))
        else:
            src = x if kind == "fwd" else dy
            mode1 = (kind == "fwd") != transposed
            od = coarse[1:] if mode1 else fine[1:]
            pts = _sample_points(1, *od, 4096, 8501)
            if mode1:  # the stride-2 convolution at coarse voxel c = the 27-tap neighbourhood of fine voxel 2 c
                ref = _sampled_reference(src, wt, pts * torch.tensor([1, 2, 2, 2], device=DEV))
            else:      # the transposed map = the stride-1 convolution of the zero-stuffed operand with the flipped weight
                ref = _sampled_reference(_stuffed_cl(src, fine[1:]), wt.transpose(0, 1).flip(2, 3, 4), pts,
                                         ones_cl=_stuffed_cl(torch.ones_like(src), fine[1:]))
            sref = ref.pop("sref")
            meta = (lambda t: torch.empty(t.shape, device="meta"))
            kt = R.products(kind, meta(ncdhw(src)), meta(wt), geom).to(DEV)
            kt = kt[pts[:, 0], 0, pts[:, 1], pts[:, 2], pts[:, 3]][:, None]
            sel = got.permute(0, 2, 3, 4, 1)[pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]]
            r = R.check(sel, "f16x3", kt, ref, sref, R.amax_of(src), R.amax_of(wt))
        record("f16x3", kind, name, f"full size {tag(transposed, kind, cin, cout, shape, 'f16x3')}", r, capsys)
        assert max(r) <= 1.0, (kind, name, r)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_route_of_the_family_is_swept():
    """the cases of this file together take every route the current switches leave to this family, and the mirrors of the launch
    arithmetic say that the cases named for a regime are in it"""
    names = {route(k, t, ci, co, a, s) for (t, ci, co, s, k, a) in CASES}
    names |= {route(k, t, ci, co, "f16x3", s) for (t, ci, co, s, k) in SEG}
    names |= {route("wgrad", t, ci, co, "f16x3", s, m) for (t, ci, co, s, m) in PRESPLIT_WGRAD
              if conv3d.PRESPLIT and opt("AZ_WGRAD_S2R16")}
    names |= {route("dgrad", t, ci, co, "f16x3", s, 1) for (t, ci, co, s) in PRESPLIT_DGRAD if conv3d.PRESPLIT and _dgrad_on_roll(t)}
    want = [["t2 f16x3"], ["gather m1 f16x3"], ["gather m2 f16x3"], ["t2 bf16x6"], ["gather m1 bf16x6"], ["gather m2 bf16x6"],
            ["gather m1 fp32"], ["gather m2 fp32"], ["one-kd f16x3"], ["one-kd bf16x6"], ["one-kd fp32"]]
    if opt("AZ_CONV_S2ROLL"):
        want += [["s2roll f16x3"]] + ([["s2roll f16x3", "presplit"]] if conv3d.PRESPLIT else [])
        if opt("AZ_S2ROLL_SEGLEN") > 1:  # the forced segment lengths of tests/test_gpu_switches.py: multi-plane and ragged
            want += [["s2roll f16x3", "seg>1", "ragged seg"]]
    if opt("AZ_CONV_T2ROLL"):
        want += [["t2roll f16x3"], ["t2roll f16x3", "seg>1", "ragged seg"]] + ([["t2roll f16x3", "presplit"]] if conv3d.PRESPLIT else [])
    if opt("AZ_WGRAD_S2R16"):
        want += [["s2r16 mask 0"], ["s2r16 mask 0", "walk"]]
        want += [["s2r16 mask 1"], ["s2r16 mask 2"], ["s2r16 mask 1", "walk"], ["s2r16 mask 2", "walk"]] if conv3d.PRESPLIT else []
    missing = [w for w in want if not any(all(tok in r for tok in w) for r in names)]
    assert not missing, (missing, sorted(names))
    # both walk shapes have more columns than persistent workgroups
    for cn, (b, dc, hc, wc) in WALK_COARSE.items():
        ncols, ntiles = b * dc * ((wc + 7) // 8), cn // 32
        assert ncols > r16_workgroups(ncols, 256 // ntiles, ntiles, 0), (cn, ncols)


def test_print_the_worst_ratios(capsys):
    """last in the file: the largest ratio of each check per arithmetic, kind and route over the cases this run executed"""
    with capsys.disabled():
        print("\nworst err / bound per arithmetic, kind and route:  check (a)  check (b)  check (c)")
        for (a, k, n), r in sorted(WORST.items()):
            print(f"  {a:7s} {k:6s} {n:42s}  " + "  ".join(f"{v:9.4f}" for v in r))
    assert all(max(r) <= 1.0 for r in WORST.values())
