"""GPU: the RAFT-Stereo ConvGRU update element-wise against fp64 -- the one-part convolutions conv2d_same_kernel<NW, 3, 3, 1,
PARTS = 1, STATS = false, H1> (az_conv2d_bf16_fwd, az_conv2d_h1_fwd: forward and, on the flipped packing, input gradient),
conv2d_wgrad_kernel<MT, NT, 3, 3, 1, AR = 2 | 3> (az_conv2d_wgrad_bf16, az_conv2d_wgrad_h1), the three packers, the sigmoid /
tanh / GRU-combine epilogues, the five gate kernels of az_gru_gates.hip with the amax arrays they write, and the wiring of those
arrays through nets/raft/gru.py.

Every launch goes through the C ABI (ops._call); every output sits between NaN sentinel bands, with NaN spare channels where the
pixel stride is wider than the channel count, and both must be untouched afterwards.  Each case names the instantiation it
reaches (NW from cout / 32 as dispatch_nw picks it, H1, MT x NT, AR, the plan numbers of the walking weight gradients) and runs
the checks of tests/_gru_fp64ref.py; tests/test_gru_error_model_cpu.py shows that those checks reject the defects they are meant
to see.  The last test prints the largest ratios per route."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _fp64ref as R  # noqa: E402
from tests import _gru_fp64ref as G  # noqa: E402
from tests._weights import seeded  # noqa: E402
from tests.test_gru_error_model_cpu import gate_inputs  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
BAND = 1024  # floats of a sentinel band
AMAX_FLOATS, AMAX_STRIDE = _lib.CONST["AZ_AMAX_FLOATS"], _lib.CONST["AZ_AMAX_STRIDE"]
SMALL = [(1, 1, 1), (2, 13, 22), (1, 16, 32), (3, 5, 47), (2, 37, 53)]
PROD_IMAGE = (1, 9, 17)
# launch channels (cin -> cout) and the NW dispatch_nw gives them
NW_PAIRS = [(16, 32, 1), (48, 64, 2), (32, 96, 3), (64, 128, 4)]
PAIRS = NW_PAIRS + [(144, 160, 1)]
PROD_PAIRS = [(384, 256, 4), (256, 384, 4)]
# weight gradients: (cm, cn) = (channels of dy, channels of x) and the MT x NT dispatch_tiles gives them
WG_PAIRS = [(32, 96, 1, 1), (64, 96, 2, 1), (32, 128, 1, 2), (128, 128, 2, 2), (64, 64, 2, 2)]
WG_PROD = [(256, 384, 2, 2), (128, 384, 2, 2)]
ROWSEG = (32, 96, (1, 2, 1))       # the smallest image whose plan has nhseg > 1
COLWALK = (128, 128, (129, 1, 1))  # the smallest image whose plan has nitems > blocks_per_combo ...
COLWALK_W = (128, 128, (5, 1, 401))  # ... and the smallest of at most five images, whose rows hold 26 chunks
WORST = {}  # (arith, kind, instantiation) -> [a, b, c, a with the specified eps, case of the largest (b)]
EXTRA = {}  # activation / gate maxima


def lib():
    return _lib.lib()


def sid(s):
    return "x".join(map(str, s))


def rows(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def guarded(n):
    """(whole buffer, the n floats between two NaN bands)"""
    whole = torch.full((n + 2 * BAND,), NAN, device=DEV)
    return whole, whole[BAND:BAND + n]


def bands_intact(whole, n):
    return bool(torch.isnan(whole[:BAND]).all()) and bool(torch.isnan(whole[BAND + n:]).all())


def amax_array(value, slot=3):
    """an amax array holding `value` (any slot: readers take the largest)"""
    a = torch.zeros(AMAX_FLOATS, device=DEV)
    if value is not None:
        a[slot * AMAX_STRIDE] = value
    return a


def amax_read(a):
    return float(a[::AMAX_STRIDE].max())


def nw_of(cout):
    nt = cout // 32
    return 4 if nt % 4 == 0 else 3 if nt % 3 == 0 else 2 if nt % 2 == 0 else 1  # az_conv2d.hip dispatch_nw


def where(shape):
    """fp64 references of the larger cases: GEMMs on the GPU"""
    return (DEV, True) if shape[0] * shape[1] * shape[2] >= 1000 else ("cpu", False)


# ---- operands and references ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def conv_operands(kind, cin, cout, shape, in_scale):
    """(p, q) of a LAUNCH cin -> cout: fwd: x [B,cin,H,W], w [cout,cin,3,3]; dgrad: dy [B,cin,H,W] and the weight [cin,cout,3,3]
    of the layer whose input gradient it is.  in_scale: factor on the activation operand"""
    b, h, w = shape
    seed = 8400 + 89 * (cin // 16) + 17 * (cout // 32) + 7 * b + 3 * h + w + (1000 if kind == "dgrad" else 0)
    src = seeded((b, cin, h, w), seed) * in_scale
    wt = seeded((cout, cin, 3, 3) if kind == "fwd" else (cin, cout, 3, 3), seed + 1, -0.2, 0.2)
    return src, wt


@functools.lru_cache(maxsize=4)
def wgrad_operands(cm, cn, shape):
    b, h, w = shape
    seed = 8600 + 89 * (cm // 32) + 17 * (cn // 32) + 7 * b + 3 * h + w
    return seeded((b, cn, h, w), seed), seeded((b, cm, h, w), seed + 2) * 1e-3  # x, dy


@functools.lru_cache(maxsize=4)
def reference(kind, a, b, shape, in_scale=1.0):
    p, q = wgrad_operands(a, b, shape) if kind == "wgrad" else conv_operands(kind, a, b, shape, in_scale)
    dev, gemm = where(shape)
    return R.exact(kind, p.to(dev), q.to(dev), gemm=gemm, geom=G.G33)


def verdict(got, kind, a, b, shape, arith, amax_p=None, amax_q=None, in_scale=1.0, epilogue=None, crop=None):
    """crop = (cm_real, cn_real): the weight gradient was unpacked without its padding channels"""
    p, q = wgrad_operands(a, b, shape) if kind == "wgrad" else conv_operands(kind, a, b, shape, in_scale)
    dev, gemm = where(shape)
    ex = reference(kind, a, b, shape, in_scale)
    sref = G.split_reference(kind, p.to(dev), q.to(dev), arith, amax_p, amax_q, gemm=gemm)
    K = R.products(kind, p, q, G.G33)
    blocks = R.wgrad_blocks_2d(q) if kind == "wgrad" else None
    if crop is not None:
        ex, sref = {k: v[:crop[0], :crop[1]] for k, v in ex.items()}, sref[:crop[0], :crop[1]]
    r = G.check(got, arith, K, ex, sref, amax_p, amax_q, blocks=blocks, epilogue=epilogue)
    spec = G.check(got, arith, K, ex, sref, amax_p, amax_q, blocks=blocks, epilogue=epilogue, eps=G.EPS_SPECIFIED[arith])[0]
    return r + (spec,)


def record(arith, kind, inst, label, r, capsys):
    w = WORST.setdefault((arith, kind, inst), [0.0, 0.0, 0.0, 0.0, ""])
    if r[1] > w[1]:
        w[4] = label
    w[:4] = [max(u, v) for u, v in zip(w, r)]
    with capsys.disabled():
        print(f"\n{label}: (a) {r[0]:.4f} (b) {r[1]:.4f} (c) {r[2]:.4f}   (a) with the specified eps {r[3]:.4f}")


# ---- launches through the C ABI ----------------------------------------------------------------------------------------------------
def pack(arith, kind, wt, cin, cout, w_amax=None):
    """the packed image of a launch cin -> cout (kind dgrad: the flipped image of the layer weight [cin, cout, 3, 3]) between
    sentinel bands; w_amax: an amax array (f16x1 only)"""
    n = 9 * cin * cout // 2
    whole, pk = guarded(n)
    w = wt.to(DEV).contiguous()
    so, si, flip = (cin * 9, 9, 0) if kind == "fwd" else (9, cout * 9, 1)
    if arith == "f16x1":
        _call("az_conv2d_pack_weights_h1", _p(pk), _p(w), _p(w_amax), cin, cout, so, si, flip, _stream())
    else:
        assert w_amax is None
        _call("az_conv2d_pack_weights_bf16_flipped" if flip else "az_conv2d_pack_weights_bf16", _p(pk), _p(w), cin, cout, so, si, 3, 3,
              _stream())
    torch.cuda.synchronize()
    assert bands_intact(whole, n)
    return pk


def conv_call(arith, out, src, pk, cin, cout, shape, bias=None, res=None, act=0, gz=None, gh=None, in_amax=None, w_amax=None,
              in_cs=None, out_cs=None, res_cs=None, gz_cs=None, gh_cs=None):
    b, h, w = shape
    tail = (_p(bias), _p(res), _p(gz), _p(gh), act, b, h, w, cin, cout, in_cs or src.shape[-1], out_cs or cout,
            res_cs if res_cs is not None else (res.shape[-1] if res is not None else 0),
            gz_cs if gz_cs is not None else (gz.shape[-1] if gz is not None else 0),
            gh_cs if gh_cs is not None else (gh.shape[-1] if gh is not None else 0), _stream())
    if arith == "f16x1":
        _call("az_conv2d_h1_fwd", _p(out), _p(src), _p(pk), _p(in_amax), _p(w_amax), *tail)
    else:
        assert in_amax is None and w_amax is None
        _call("az_conv2d_bf16_fwd", _p(out), _p(src), _p(pk), *tail)


def run_conv(arith, src, pk, cin, cout, shape, out_cs=None, **kw):
    """the launch into a guarded buffer; NCHW result [B,cout,H,W] after the sentinel checks"""
    b, h, w = shape
    out_cs = out_cs or cout
    n = b * h * w * out_cs
    whole, flat = guarded(n)
    conv_call(arith, flat, src, pk, cin, cout, shape, out_cs=out_cs, **kw)
    torch.cuda.synchronize()
    out = flat.view(b, h, w, out_cs)
    assert bands_intact(whole, n), "a launch wrote outside its output"
    assert bool(torch.isnan(out[..., cout:]).all()), "a launch wrote the spare channels of a wide pixel stride"
    assert not bool(torch.isnan(out[..., :cout]).any()), "an output was not written"
    return out[..., :cout].permute(0, 3, 1, 2)


def run_wgrad(arith, xr, gr, cm, cn, shape, go_amax=None, in_amax=None, cm_real=None, cn_real=None):
    b, h, w = shape
    cm_real, cn_real = cm_real or cm, cn_real or cn
    ws_bytes = lib().az_conv2d_wgrad_workspace(cm, cn, 3, 3)
    ws_whole, ws = guarded(ws_bytes // 4)
    n = cm_real * cn_real * 9
    whole, gw = guarded(n)
    if arith == "f16x1":
        _call("az_conv2d_wgrad_h1", _p(gw), _p(ws), ws_bytes, _p(gr), _p(xr), _p(go_amax), _p(in_amax), b, h, w, cm, cn, cm_real,
              cn_real, gr.shape[-1], xr.shape[-1], _stream())
    else:
        _call("az_conv2d_wgrad_bf16", _p(gw), _p(ws), ws_bytes, _p(gr), _p(xr), b, h, w, cm, cn, cm_real, cn_real, gr.shape[-1],
              xr.shape[-1], _stream())
    torch.cuda.synchronize()
    assert bands_intact(whole, n) and bands_intact(ws_whole, ws_bytes // 4), "a launch wrote outside its output / workspace"
    assert not bool(torch.isnan(gw).any())
    return gw.view(cm_real, cn_real, 3, 3)


def wgrad_route(cm, cn, mt, nt, arith, shape):
    """MT x NT restated from dispatch_tiles and -- for pairs the r16 kernels do not own -- confirmed with the plan the library
    answers for the generic kernel; the one-part launches never go to r16, so (64, 64) runs the generic 2 x 2 kernel too"""
    assert (mt, nt) == (2 if cm % 64 == 0 else 1, 2 if cn % 64 == 0 else 1)
    name = f"generic {mt}x{nt} AR{3 if arith == 'f16x1' else 2}"
    plan = None
    if not (cm in (32, 64) and cn in (32, 64)):
        plan = (ctypes.c_longlong * 8)()
        assert lib().az_conv2d_wgrad_plan(plan, 0, *shape, cm, cn, 3, 3, 1) == 0
        plan = list(plan)
        assert plan[0] == _lib.CONST["AZ_C2W_KERNEL_GENERIC"] and (plan[1], plan[2]) == (mt, nt), plan
        name += f" [blocks {plan[3]} hseg_rows {plan[4]} nhseg {plan[5]} nitems {plan[6]}]"
    return name, plan


# ---- forward and input gradient ------------------------------------------------------------------------------------------------------
CONV_CASES = [(ci, co, nw, s, k, a) for (ci, co, nw) in PAIRS for s in SMALL for k in ("fwd", "dgrad") for a in G.ARITHS]
CONV_CASES += [(ci, co, nw, PROD_IMAGE, k, a) for (ci, co, nw) in PROD_PAIRS for k in ("fwd", "dgrad") for a in G.ARITHS]


@pytest.mark.parametrize("cin,cout,nw,shape,kind,arith", CONV_CASES,
                         ids=[f"{k}-{ci}x{co}-{sid(s)}-{a}" for (ci, co, nw, s, k, a) in CONV_CASES])
def test_conv_vs_fp64(cin, cout, nw, shape, kind, arith, capsys):
    assert nw_of(cout) == nw
    in_scale = 1.0 if kind == "fwd" else 1e-3
    src, wt = conv_operands(kind, cin, cout, shape, in_scale)
    got = run_conv(arith, rows(src), pack(arith, kind, wt, cin, cout), cin, cout, shape)
    r = verdict(got, kind, cin, cout, shape, arith, in_scale=in_scale)
    inst = f"NW{nw}{' H1' if arith == 'f16x1' else ''}"
    record(arith, kind, f"NW{nw}", f"{kind} {cin}->{cout} {shape} [{inst} plain]", r, capsys)
    assert max(r[:3]) <= 1.0, (inst, r)


VARIANTS = [(ci, co, nw, s, v, a) for (ci, co, nw) in NW_PAIRS for s in [(2, 13, 22), (3, 5, 47)]
            for v in ("bias-res", "in-stride", "out-stride") for a in G.ARITHS]


@pytest.mark.parametrize("cin,cout,nw,shape,variant,arith", VARIANTS,
                         ids=[f"{v}-{ci}x{co}-{sid(s)}-{a}" for (ci, co, nw, s, v, a) in VARIANTS])
def test_conv_variants_vs_fp64(cin, cout, nw, shape, variant, arith, capsys):
    """bias + residual read at res_cs = cout + 8 (ReLU at one of the two images), the input at in_cs = cin + 4, the output at
    out_cs = cout + 4; the channels next to the operands hold large values that must not be read"""
    assert nw_of(cout) == nw
    b, h, w = shape
    src, wt = conv_operands("fwd", cin, cout, shape, 1.0)
    xr, kw, epi = rows(src), {}, None
    if variant == "bias-res":
        bias, res = seeded((cout,), 8501), seeded((b, cout, h, w), 8502) * 0.5
        relu = shape == (3, 5, 47)
        rr = torch.cat([rows(res), torch.full((b, h, w, 8), 1.0e4, device=DEV)], -1).contiguous()
        kw = dict(bias=bias.to(DEV), res=rr, act=int(relu))
        epi = (torch.ones(cout), bias, res, relu)
    elif variant == "in-stride":
        xr = torch.cat([xr, torch.full((b, h, w, 4), 1.0e4, device=DEV)], -1).contiguous()
    else:
        kw = dict(out_cs=cout + 4)
    got = run_conv(arith, xr, pack(arith, "fwd", wt, cin, cout), cin, cout, shape, **kw)
    r = verdict(got, "fwd", cin, cout, shape, arith, epilogue=epi)
    inst = f"NW{nw}{' H1' if arith == 'f16x1' else ''}"
    record(arith, "fwd", f"NW{nw}", f"fwd {cin}->{cout} {shape} [{inst} {variant}]", r, capsys)
    assert max(r[:3]) <= 1.0, (inst, variant, r)


# f16x1 operand scales: (name, kind, factor on the activation operand, in_amax given, w_amax given)
AMAX_COMBOS = [("none", "fwd", 1.0, False, False), ("in-tiny", "dgrad", None, True, False), ("in-large", "fwd", 1000.0, True, False),
               ("w", "fwd", 1.0, False, True), ("both", "fwd", 1.0, True, True), ("both-tiny", "dgrad", None, True, True)]
AMAX_CASES = [(ci, co, nw, c) for (ci, co, nw) in NW_PAIRS for c in AMAX_COMBOS]


@pytest.mark.parametrize("cin,cout,nw,combo", AMAX_CASES, ids=[f"{c[0]}-{ci}x{co}" for (ci, co, nw, c) in AMAX_CASES])
def test_h1_operand_scales_vs_fp64(cin, cout, nw, combo, capsys):
    """az_conv2d_h1_fwd with no amax, in_amax only (|in| <= 2^-22, the gradient case, and |in| near 2^10), w_amax only (the image
    packed with it) and both: the reference rounds each operand with the k its array gives, k = 0 without one"""
    name, kind, in_scale, with_in, with_w = combo
    shape = (3, 5, 47)
    if in_scale is None:
        in_scale = 2.0 ** -22
    src, wt = conv_operands(kind, cin, cout, shape, in_scale)
    am_in, am_w = (R.amax_of(src) if with_in else None), (R.amax_of(wt) if with_w else None)
    if name.endswith("tiny"):
        assert am_in <= 2.0 ** -22
    if name == "in-large":
        assert 2.0 ** 9 <= am_in < 2.0 ** 10
    a_in, a_w = (amax_array(am_in) if with_in else None), (amax_array(am_w, slot=11) if with_w else None)
    got = run_conv("f16x1", rows(src), pack("f16x1", kind, wt, cin, cout, a_w), cin, cout, shape, in_amax=a_in, w_amax=a_w)
    r = verdict(got, kind, cin, cout, shape, "f16x1", am_in, am_w, in_scale=in_scale)
    record("f16x1", kind, f"NW{nw}", f"{kind} {cin}->{cout} {shape} [NW{nw} H1 amax {name}]", r, capsys)
    assert max(r[:3]) <= 1.0, (name, r)


ACT_CASES = [(ci, co, nw, s, a) for (ci, co, nw) in NW_PAIRS for s in [(2, 13, 22), (3, 5, 47)] for a in G.ARITHS]


@pytest.mark.parametrize("cin,cout,nw,shape,arith", ACT_CASES, ids=[f"{ci}x{co}-{sid(s)}-{a}" for (ci, co, nw, s, a) in ACT_CASES])
def test_gate_activations_vs_fp64_of_the_pre_activation(cin, cout, nw, shape, arith, capsys):
    """act 0 first (its output y0 is checked against fp64 like any other); act 1 = max(y0, 0) to the bit; act 2 / 3 / 4 = the
    fp64 sigmoid / tanh / (1 - z) h + z tanh of y0 within act_check's allowance, with z read as the first half of a zr-shaped
    tensor (gz_cs = 2 cout) and h at gh_cs = cout; a few pixels are driven to +-100 by the residual and must stay finite"""
    b, h, w = shape
    src, wt = conv_operands("fwd", cin, cout, shape, 1.0)
    bias, res = seeded((cout,), 8511), seeded((b, cout, h, w), 8512) * 2.0
    res[0, :, 0, 0], res[-1, :, h - 1, w - 1], res[0, ::2, h // 2, w // 2] = 100.0, -100.0, -100.0
    zr = torch.sigmoid(seeded((b, h, w, 2 * cout), 8513) * 3.0).to(DEV)
    zr[..., cout:] = 1.0e4  # (the r half: not read)
    hp = torch.tanh(seeded((b, h, w, cout), 8514) * 2.0).to(DEV)
    xr, pk, rr = rows(src), pack(arith, "fwd", wt, cin, cout), rows(res)
    run = lambda act, **kw: run_conv(arith, xr, pk, cin, cout, shape, bias=bias.to(DEV), res=rr, act=act, **kw)
    y0 = run(G.ACT_NONE)
    r = verdict(y0, "fwd", cin, cout, shape, arith, epilogue=(torch.ones(cout), bias, res, False))
    inst = f"NW{nw}{' H1' if arith == 'f16x1' else ''}"
    record(arith, "fwd", f"NW{nw}", f"fwd {cin}->{cout} {shape} [{inst} bias + residual to +-100]", r, capsys)
    assert max(r[:3]) <= 1.0, r
    assert float(y0.abs().max()) > 90.0
    assert torch.equal(run(G.ACT_RELU), y0.clamp_min(0.0))
    z, hh = zr[..., :cout].permute(0, 3, 1, 2), hp.permute(0, 3, 1, 2)
    for act, name, kw in ((G.ACT_SIGMOID, "sigmoid", {}), (G.ACT_TANH, "tanh", {}), (G.ACT_GRU, "combine", dict(gz=zr, gh=hp))):
        got = run(act, **kw)
        ratio, err = G.act_check(got, y0, act, z, hh)
        e = EXTRA.setdefault(f"act {name} {arith}", [0.0, 0.0])
        e[:] = [max(e[0], ratio), max(e[1], err)]
        with capsys.disabled():
            print(f"  {name} [{inst}] {shape}: err / allowance {ratio:.4f}, max |err| {err:.3e}")
        assert ratio <= 1.0, (name, ratio, err)


@pytest.mark.parametrize("arith", G.ARITHS)
def test_conv_refusals(arith):
    shape, cin, cout = (1, 4, 5), 16, 32
    b, h, w = shape
    xr = torch.zeros(b, h, w, 64, device=DEV)
    pk, out, res = torch.zeros(9 * 64 * 64, device=DEV), torch.zeros(b, h, w, 64, device=DEV), torch.zeros(b, h, w, 64, device=DEV)
    conv_call(arith, out, xr, pk, cin, cout, shape, in_cs=64, out_cs=64)  # (the base launch is accepted)
    bad = [dict(cin=24), dict(cout=48), dict(in_cs=18), dict(res=res, res_cs=cout - 4), dict(act=G.ACT_GRU),
           dict(act=G.ACT_GRU, gz=res, gh=res, gz_cs=cout - 4, gh_cs=64)]
    for kw in bad:
        args = dict(cin=cin, cout=cout, in_cs=64, out_cs=64)
        args.update(kw)
        ci, co = args.pop("cin"), args.pop("cout")
        with pytest.raises(RuntimeError):
            conv_call(arith, out, xr, pk, ci, co, shape, **args)
    torch.cuda.synchronize()


# ---- the packers ------------------------------------------------------------------------------------------------------------------
def decode_expected(w_launch, cin, cout):
    """[cout, cin, 9] launch-view weights -> the packed order [tap][cin / 16][cout / 32][64 lanes][8]: element co = 32 n + (lane &
    31), ci = 16 cc + 8 (lane >> 5) + j"""
    v = w_launch.reshape(cout // 32, 32, cin // 16, 2, 8, 9)  # n, lane & 31, cc, lane >> 5, j, tap
    return v.permute(5, 2, 0, 3, 1, 4).reshape(9, cin // 16, cout // 32, 64, 8)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("cin,cout", [(16, 32), (48, 64), (96, 64), (64, 96)])
def test_packed_images_bit_for_bit(cin, cout, flip):
    """the three packers against torch's .bfloat16() / .half() of the (scaled) weight, decoded on the host; (96, 64) is the
    concatenated (wz, wr) weight [2 x 32, 96, 3, 3] of a hidden 32, input 64 GRU as gru.py builds it, (64, 96) flipped its input gradient's"""
    kind = "dgrad" if flip else "fwd"
    lc, li = (cin, cout) if flip else (cout, cin)  # the layer's [out, in]
    if (lc, li) == (64, 96):
        wt = torch.cat([seeded((lc // 2, li, 3, 3), 8521, -0.2, 0.2), seeded((lc // 2, li, 3, 3), 8522, -0.2, 0.2)], 0)
    else:
        wt = seeded((lc, li, 3, 3), 8520, -0.2, 0.2)
    wt[0, 0, 0, 0], wt[1, 0, 0, 1] = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8  # bf16 ties: to even
    launch = (wt.permute(1, 0, 2, 3).flip(2, 3) if flip else wt).reshape(cout, cin, 9)
    want = decode_expected(launch, cin, cout)
    bits = lambda pk: pk.view(torch.int16).view(9, cin // 16, cout // 32, 64, 8).cpu()
    assert torch.equal(bits(pack("bf16x1", kind, wt, cin, cout)), want.bfloat16().view(torch.int16))
    assert torch.equal(bits(pack("f16x1", kind, wt, cin, cout)), want.half().view(torch.int16))
    am = R.amax_of(wt)
    k = R.f16_scale_exp(am)
    assert 2.0 ** 14 <= am * 2.0 ** k < 2.0 ** 15
    assert torch.equal(bits(pack("f16x1", kind, wt, cin, cout, amax_array(am, slot=7))), (want * 2.0 ** k).half().view(torch.int16))


# ---- weight gradients ----------------------------------------------------------------------------------------------------------------
WG = [(cm, cn, mt, nt, s) for (cm, cn, mt, nt) in WG_PAIRS for s in SMALL] + [(cm, cn, mt, nt, PROD_IMAGE) for (cm, cn, mt, nt) in WG_PROD]
WG += [(32, 96, 1, 1, ROWSEG[2]), (128, 128, 2, 2, COLWALK[2]), (128, 128, 2, 2, COLWALK_W[2])]
WG_CASES = [(cm, cn, mt, nt, s, a) for (cm, cn, mt, nt, s) in WG for a in G.ARITHS]


def wgrad_case(cm, cn, mt, nt, shape, arith, mode, capsys, label=""):
    """mode (f16x1): "go" = go_amax only, as gru.py calls it; "both"; "none" """
    x, dy = wgrad_operands(cm, cn, shape)
    name, plan = wgrad_route(cm, cn, mt, nt, arith, shape)
    am_g = R.amax_of(dy) if (arith == "f16x1" and mode in ("go", "both")) else None
    am_x = R.amax_of(x) if (arith == "f16x1" and mode == "both") else None
    got = run_wgrad(arith, rows(x), rows(dy), cm, cn, shape, amax_array(am_g) if am_g else None, amax_array(am_x, slot=9) if am_x else None)
    r = verdict(got, "wgrad", cm, cn, shape, arith, am_x, am_g)
    record(arith, "wgrad", f"{mt}x{nt}", f"wgrad dy {cm} x {cn} {shape} [{name}{label}{' amax ' + mode if arith == 'f16x1' else ''}]", r, capsys)
    assert max(r[:3]) <= 1.0, (name, r)
    return plan


@pytest.mark.parametrize("cm,cn,mt,nt,shape,arith", WG_CASES, ids=[f"{cm}x{cn}-{sid(s)}-{a}" for (cm, cn, mt, nt, s, a) in WG_CASES])
def test_wgrad_vs_fp64(cm, cn, mt, nt, shape, arith, capsys):
    plan = wgrad_case(cm, cn, mt, nt, shape, arith, "go", capsys)
    if (cm, cn, shape) == ROWSEG:
        assert plan[5] > 1, plan                # row segments
    if (cm, cn, shape) in (COLWALK, COLWALK_W):
        assert plan[6] > plan[3], plan          # more items than blocks per combo: blocks walk their list


@pytest.mark.parametrize("mode", ["both", "none"])
@pytest.mark.parametrize("cm,cn,mt,nt", WG_PAIRS[:4])
def test_wgrad_h1_with_both_and_with_no_amax(cm, cn, mt, nt, mode, capsys):
    wgrad_case(cm, cn, mt, nt, (3, 5, 47), "f16x1", mode, capsys)


@pytest.mark.parametrize("arith", G.ARITHS)
@pytest.mark.parametrize("which", ["strides", "real"])
def test_wgrad_wide_strides_and_channel_padding(which, arith, capsys):
    """go_cstride / in_cstride wider than the channel counts (the spare channels hold large values that must not be read);
    cm_real < cm and cn_real < cn: the unpack drops the padding channels"""
    cm, cn, shape = 64, 96, (2, 13, 22)
    b, h, w = shape
    x, dy = wgrad_operands(cm, cn, shape)
    name, _ = wgrad_route(cm, cn, 2, 1, arith, shape)
    am_g = R.amax_of(dy) if arith == "f16x1" else None
    a_g = amax_array(am_g) if am_g else None
    xr, gr = rows(x), rows(dy)
    if which == "strides":
        junk = lambda n: torch.full((b, h, w, n), 1.0e4, device=DEV)
        got = run_wgrad(arith, torch.cat([xr, junk(4)], -1).contiguous(), torch.cat([gr, junk(8)], -1).contiguous(), cm, cn, shape, a_g)
    else:
        got = run_wgrad(arith, xr, gr, cm, cn, shape, a_g, cm_real=cm - 3, cn_real=cn - 5)
        assert got.shape == (cm - 3, cn - 5, 3, 3)
    r = verdict(got, "wgrad", cm, cn, shape, arith, None, am_g, crop=(cm - 3, cn - 5) if which == "real" else None)
    record(arith, "wgrad", "2x1", f"wgrad dy {cm} x {cn} {shape} [{name} {which}]", r, capsys)
    assert max(r[:3]) <= 1.0, r


# ---- the gate kernels ----------------------------------------------------------------------------------------------------------------
GATE_SHAPES = [(1, 4, 0), (77, 36, 20), (4099, 128, 256), (33001, 128, 4)]  # the last: more float4s than the 4096 x 256 grid


def gate_buf(npix, c):
    whole, flat = guarded(npix * c)
    return whole, flat.view(npix, c)


def gate_record(name, ratio, capsys, note=""):
    EXTRA[f"gate {name}"] = [max(EXTRA.get(f"gate {name}", [0.0])[0], ratio)]
    with capsys.disabled():
        print(f"  {name}{note}: err / bound {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("shape", GATE_SHAPES, ids=sid)
def test_gru_forward_gates_vs_fp64(shape, capsys):
    npix, hid, inp = shape
    zr, q, hx, _, _, _ = [t.to(DEV) for t in gate_inputs(npix, hid, inp)]
    if npix * hid // 4 > 4096 * 256:
        assert shape == GATE_SHAPES[-1]
    w1, rhx = gate_buf(npix, hid + inp)
    _call("az_gru_rh", _p(rhx), _p(zr), _p(hx), npix, hid, inp, _stream())
    w2, hn = gate_buf(npix, hid)
    _call("az_gru_out", _p(hn), _p(zr), _p(q), _p(hx), npix, hid, inp, _stream())
    torch.cuda.synchronize()
    assert bands_intact(w1, rhx.numel()) and bands_intact(w2, hn.numel())
    gate_record("rh", G.gate_ratio(rhx, G.gru_rh(zr, hx, hid)), capsys, f" {shape}")
    assert torch.equal(rhx[:, hid:], hx[:, hid:])
    gate_record("out", G.gate_ratio(hn, G.gru_out(zr, q, hx, hid)), capsys, f" {shape}")


def run_bwd12(t, shape, with_amax):
    """az_gru_bwd1 then az_gru_bwd2 into the same dzr / dh_acc / amax array; returns the outputs after each"""
    npix, hid, inp = shape
    zr, q, hx, g, d_rhx, _ = t
    bufs = {k: gate_buf(npix, c) for k, c in (("dq", hid), ("dzr", 2 * hid), ("dh_acc", hid))}
    am_q, am_z = (amax_array(None), amax_array(None)) if with_amax else (None, None)
    o = {n: b[1] for n, b in bufs.items()}
    _call("az_gru_bwd1", _p(o["dq"]), _p(o["dzr"]), _p(o["dh_acc"]), _p(g), _p(zr), _p(q), _p(hx), npix, hid, inp, _p(am_q), _p(am_z), _stream())
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in o.items()}
    first["am_q"], first["am_z"] = (amax_read(am_q), amax_read(am_z)) if with_amax else (None, None)
    _call("az_gru_bwd2", _p(o["dzr"]), _p(o["dh_acc"]), _p(d_rhx), _p(zr), _p(hx), npix, hid, inp, _p(am_z), _stream())
    torch.cuda.synchronize()
    for k, (whole, v) in bufs.items():
        assert bands_intact(whole, v.numel()), k
    o["am_q"], o["am_z"] = (amax_read(am_q), amax_read(am_z)) if with_amax else (None, None)
    return first, o


@pytest.mark.parametrize("orient", ["z", "r"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=sid)
def test_gru_backward_gates_and_their_amax_vs_fp64(shape, orient, capsys):
    """bwd1 and bwd2 with and without amax arrays (bit-identical outputs), against fp64; am_q = the largest finite |dq_pre| and
    am_z = the largest finite |dzr| over BOTH halves, bit for bit, with the maximum in the z half (large g) and in the r half
    (large d_rhx: only bwd2 can supply it); one inf planted in g is ignored by the amax and changes no other output"""
    npix, hid, inp = shape
    t = [x.to(DEV) for x in gate_inputs(npix, hid, inp, orient)]
    zr, q, hx, g, d_rhx, d_hx = t
    f_am, o_am = run_bwd12(t, shape, True)
    f_no, o_no = run_bwd12(t, shape, False)
    for k in ("dq", "dzr", "dh_acc"):
        assert torch.equal(o_am[k], o_no[k]) and torch.equal(f_am[k].nan_to_num(7.0), f_no[k].nan_to_num(7.0)), k
    assert bool(torch.isnan(f_am["dzr"][:, hid:]).all()), "bwd1 wrote the r half of dzr"
    assert torch.equal(o_am["dzr"][:, :hid], f_am["dzr"][:, :hid]), "bwd2 changed the z half of dzr"
    assert torch.equal(o_am["dq"], f_am["dq"])
    b1 = G.gru_bwd1(g, zr, q, hx, hid)
    note = f" {shape} max in {orient}"
    gate_record("bwd1 dq_pre", G.gate_ratio(f_am["dq"], b1["dq"]), capsys, note)
    gate_record("bwd1 dz", G.gate_ratio(f_am["dzr"][:, :hid], b1["dz"]), capsys, note)
    gate_record("bwd1 dh_acc", G.gate_ratio(f_am["dh_acc"], b1["dh_acc"]), capsys, note)
    b2 = G.gru_bwd2(f_am["dh_acc"], d_rhx, zr, hx, hid)
    gate_record("bwd2 dr", G.gate_ratio(o_am["dzr"][:, hid:], b2["dr"]), capsys, note)
    gate_record("bwd2 dh_acc", G.gate_ratio(o_am["dh_acc"], b2["dh_acc"]), capsys, note)
    # the amax arrays: bit for bit the largest finite magnitude of the kernel's own output (= the fp64 value rounded to fp32 up
    # to the bound just checked)
    assert f_am["am_q"] == R.amax_of(f_am["dq"]) and o_am["am_q"] == f_am["am_q"]
    assert f_am["am_z"] == R.amax_of(f_am["dzr"][:, :hid])
    assert o_am["am_z"] == R.amax_of(o_am["dzr"])
    am_zh, am_rh = R.amax_of(o_am["dzr"][:, :hid]), R.amax_of(o_am["dzr"][:, hid:])
    assert (am_zh > am_rh) if orient == "z" else (am_rh > am_zh), (am_zh, am_rh)
    # one inf in g
    gi = g.clone()
    gi[npix // 2, hid // 2] = float("inf")
    _, o_inf = run_bwd12([zr, q, hx, gi, d_rhx, d_hx], shape, True)
    # (the amax stays the largest FINITE magnitude: that of the run before unless the planted element held it)
    assert o_inf["am_q"] == R.amax_of(o_inf["dq"]) <= o_am["am_q"] and o_inf["am_z"] == R.amax_of(o_inf["dzr"]) <= o_am["am_z"]
    hit = torch.zeros(npix, hid, dtype=torch.bool, device=DEV)
    hit[npix // 2, hid // 2] = True
    assert torch.equal(o_inf["dq"][~hit], o_am["dq"][~hit]) and torch.equal(o_inf["dh_acc"][~hit], o_am["dh_acc"][~hit])
    assert torch.equal(o_inf["dzr"][:, hid:], o_am["dzr"][:, hid:]) and torch.equal(o_inf["dzr"][:, :hid][~hit], o_am["dzr"][:, :hid][~hit])
    assert not bool(torch.isfinite(o_inf["dh_acc"][hit]).any())


@pytest.mark.parametrize("shape", GATE_SHAPES[1:], ids=sid)
def test_gru_bwd3_vs_fp64(shape, capsys):
    npix, hid, inp = shape
    _, _, _, g, d_rhx, d_hx = [x.to(DEV) for x in gate_inputs(npix, hid, inp)]
    dh_acc = g
    w1, dh = gate_buf(npix, hid)
    w2, dx = gate_buf(npix, inp)
    _call("az_gru_bwd3", _p(dh), _p(dx), _p(dh_acc), _p(d_rhx), _p(d_hx), npix, hid, inp, _stream())
    torch.cuda.synchronize()
    assert bands_intact(w1, dh.numel()) and bands_intact(w2, dx.numel())
    b3 = G.gru_bwd3(dh_acc, d_rhx, d_hx, hid)
    gate_record("bwd3 dh", G.gate_ratio(dh, b3["dh"]), capsys, f" {shape}")
    gate_record("bwd3 dx", G.gate_ratio(dx, b3["dx"]), capsys, f" {shape}")


def test_gate_refusals():
    npix, hid = 5, 8
    t = torch.zeros(npix, 4 * hid, device=DEV)
    am = amax_array(None)
    with pytest.raises(RuntimeError):  # inp = 0: bwd3 has no dx to write
        _call("az_gru_bwd3", _p(t), _p(t), _p(t), _p(t), _p(t), npix, hid, 0, _stream())
    for a, b in ((am, None), (None, am)):  # one NULL of the amax pair
        with pytest.raises(RuntimeError):
            _call("az_gru_bwd1", _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), npix, hid, 4, _p(a), _p(b), _stream())
    with pytest.raises(RuntimeError):  # channels: multiples of 4
        _call("az_gru_rh", _p(t), _p(t), _p(t), npix, 6, 4, _stream())
    torch.cuda.synchronize()


# ---- the wiring of the scales through nets/raft/gru.py --------------------------------------------------------------------------------
def test_f16x1_gradient_scales_follow_the_cotangent():
    """ConvGRU under train_arithmetic "f16x1" with cotangents g and 2^-30 g: the amax scale tracks the operand's exponent and the
    gates are exact under powers of two, so every gradient that does not pass through float atomics (state, the three context terms,
    the inputs) is bit-identical after multiplication by 2^30; weight and bias gradients agree to the run-to-run tolerance of
    test_gru_update_with_assembled_rows_equals_the_slice_assignments.  A lost or swapped amax flushes the small run to zero."""
    from activezero_amd.nets.raft.gru import ConvGRU
    from tests.test_gpu_raft_gru import _inputs
    b, c, cx, h, w = 2, 32, (36, 60), 21, 35
    hid, ctx, xs = _inputs(b, c, cx, h, w, 79)
    cot = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(4))
    res = []
    for s in (1.0, 2.0 ** -30):
        torch.manual_seed(11)
        mod = ConvGRU(c, sum(cx)).cuda()
        assert mod.train_arithmetic == "f16x1"
        leaves = [t.clone().cuda().requires_grad_(True) for t in [hid] + ctx + xs]
        out = mod(leaves[0], *leaves[1:4], *leaves[4:])
        (out * (cot * s).cuda()).sum().backward()
        res.append([t.grad * (1.0 / s) for t in leaves] + [p.grad * (1.0 / s) for p in mod.parameters()])
    for i, (a, bb) in enumerate(zip(*res)):
        assert float(a.abs().max()) > 0.0, i
        if i < 6:
            assert torch.equal(a.contiguous(), bb.contiguous()), i
        else:
            torch.testing.assert_close(bb, a, rtol=1e-5, atol=1e-6 * float(a.abs().max()))


def test_zz_largest_ratios(capsys):
    """the last test of the module: the largest ratio of each check per arithmetic, kind and instantiation over the cases run"""
    with capsys.disabled():
        print("\nlargest err / bound:  (a)  (b)  (c)  (a) with the specified eps   [case of the largest (b)]")
        for (a, k, inst), r in sorted(WORST.items()):
            print(f"  {a:7s} {k:6s} {inst:4s} " + "  ".join(f"{v:7.4f}" for v in r[:4]) + f"   {r[4]}")
        for k, v in sorted(EXTRA.items()):
            print(f"  {k}: " + "  ".join(f"{x:.4g}" for x in v))
    assert all(max(r[:3]) <= 1.0 for r in WORST.values())
