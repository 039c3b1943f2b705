"""CPU: the checks of tests/_gru_fp64ref.py are sharp enough to catch a subtly wrong one-part convolution or gate kernel of the
RAFT-Stereo ConvGRU update.

A pure-torch emulation of the bf16x1 and f16x1 arithmetic (operands rounded once as the kernels round them, each 16-deep K block
summed exactly and chained into an fp32 accumulator, the amax scale applied and undone) passes checks (a), (b) and (c) for the
forward, the input gradient and the weight gradient at the small shapes of tests/test_gpu_gru_fp64.py; each mutant of it -- one
defect of a class a kernel could have -- fails at least one check at every one of those shapes its class applies to.  A float32
emulation of the five gate kernels passes their counted bounds and its mutants do not.  The fp64 references themselves are pinned
to torch.nn.functional.conv2d / torch.nn.grad.conv2d_weight and to autograd of the reference's 22 lines as
tests/test_gpu_raft_gru.py restates them.  No mutant kernel is built or run."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import _fp64ref as R
from tests import _gru_fp64ref as G
from tests._weights import seeded
from tests.test_conv_error_model_cpu import unfold2d
from tests.test_gpu_raft_gru import _reference_gru

SHAPES = [(1, 1, 1), (2, 13, 22), (1, 16, 32), (3, 5, 47), (2, 37, 53)]  # the SMALL list of the GPU file
CIN = COUT = 32
GRAD_MAX = 2.0 ** -22  # |dy| of the "gradient" operand sets: far below fp16's range without the amax scale
# operand sets: (arithmetic, dy scaled to GRAD_MAX and given an amax)
SETS = [("bf16x1", False), ("f16x1", False), ("f16x1", True)]


def operands(kind, shape, small_grad, seed=8100):
    """(p, q, amax_p, amax_q): amax = None where the launch has no amax array (bf16x1; every f16x1 operand but a scaled dy)"""
    b, h, w = shape
    x = seeded((b, CIN, h, w), seed)
    wt = seeded((COUT, CIN, 3, 3), seed + 1, -0.2, 0.2)
    dy = seeded((b, COUT, h, w), seed + 2) * (GRAD_MAX if small_grad else 1e-3)
    am = R.amax_of(dy) if small_grad else None
    return {"fwd": (x, wt, None, None), "dgrad": (dy, wt, am, None), "wgrad": (x, dy, None, am)}[kind]


def rounded(t, arith, amax, mutant, is_grad):
    """(the fp16 / bf16 value the emulated kernel multiplies, as fp64; the exponent k it was scaled by)"""
    t = t.float()
    if mutant == "wrong_format":
        arith = "f16x1" if arith == "bf16x1" else "bf16x1"
    if arith == "bf16x1":
        if mutant == "bf16_trunc":
            return (t.view(torch.int32) & -65536).view(torch.float32).double(), 0
        return t.bfloat16().double(), 0
    k = G.scale_exp(arith, amax)
    if mutant == "amax_ignored" and is_grad:
        k = 0
    return (t * 2.0 ** k).half().double(), k


def emulate(kind, p, q, arith, amax_p=None, amax_q=None, mutant=None):
    """the kernels' result in the emulated arithmetic (NCHW / weight layout, fp32): the products of the rounded, scaled operands
    summed exactly per 16-deep block -- one (tap, 16-channel chunk) of a convolution launch, one (image, row, 16-position chunk) of
    a weight gradient -- each block chained into the fp32 accumulator with one rounding, the scales undone once at the end"""
    pr, kp = rounded(p, arith, amax_p, mutant, kind == "dgrad")
    qr, kq = rounded(q, arith, amax_q, mutant, kind == "wgrad")
    b, _, h, w = p.shape
    edge = "w_edge" if mutant == "w_edge" else None
    if kind in ("fwd", "dgrad"):
        if kind == "dgrad":
            qr = qr.transpose(0, 1) if mutant == "taps_not_flipped" else qr.transpose(0, 1).flip(2, 3)
        cout, c = qr.shape[0], qr.shape[1]
        a = unfold2d(pr, G.G33, edge)                         # [N, 9 C], tap-major
        bm = qr.permute(2, 3, 1, 0).reshape(-1, cout)         # [9 C, cout]
        if mutant == "chunk_dropped":                         # the second 16-channel chunk never multiplied
            a = a.reshape(-1, 9, c).clone()
            a[:, :, 16:32] = 0.0
            a = a.reshape(-1, 9 * c)
    else:
        cout, cin = qr.shape[1], pr.shape[1]
        m = torch.ones(b, h, w, dtype=torch.float64)
        seam = (h + 1) // 2                                   # two row segments: rows [0, seam) and [seam, h)
        if mutant == "row_twice":                             # the first row of the second segment also counted by the first
            m[:, min(seam, h - 1), :] = 2.0
        if mutant == "seg_last_row_dropped":
            m[:, seam - 1, :] = 0.0
        wp = (w + 15) // 16 * 16                              # K blocks are (image, row, 16-position chunk): pad the rows
        a = F.pad(qr * m.unsqueeze(1), (0, wp - w)).permute(1, 0, 2, 3).reshape(cout, -1)
        bm = F.pad(unfold2d(pr, G.G33, edge).reshape(b, h, w, 9 * cin), (0, 0, 0, wp - w)).reshape(-1, 9 * cin)
    acc = torch.zeros(a.shape[0], bm.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 16):
        acc = (acc.double() + a[:, k0:k0 + 16] @ bm[k0:k0 + 16]).float()  # one MFMA: exact block sum, one rounding
    acc = acc * 2.0 ** -(kp + kq + (1 if mutant == "scale_off_by_one" else 0))
    if kind == "wgrad":
        return acc.reshape(cout, 9, cin).permute(0, 2, 1).reshape(cout, cin, 3, 3)
    return acc.reshape(b, h, w, cout).permute(0, 3, 1, 2)


def ratios(kind, shape, arith, small_grad, mutant=None):
    p, q, amp, amq = operands(kind, shape, small_grad)
    got = emulate(kind, p, q, arith, amp, amq, mutant)
    ex = R.exact(kind, p, q, geom=G.G33)
    sref = G.split_reference(kind, p, q, arith, amp, amq)
    blocks = R.wgrad_blocks_2d(q) if kind == "wgrad" else None
    K = R.products(kind, p, q, G.G33)
    r = G.check(got, arith, K, ex, sref, amp, amq, blocks=blocks)
    # the arithmetic alone (no accumulation error) against bound (a), and against (a) in the form the sweep was specified with
    r_split = G.check(sref, arith, K, ex, sref, amp, amq, blocks=blocks)[0]
    r_spec = G.check(sref, arith, K, ex, sref, amp, amq, blocks=blocks, eps=G.EPS_SPECIFIED[arith])[0]
    return r, (r_split, r_spec)


def _sid(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("arith,small_grad", SETS, ids=[f"{a}{'-grad' if g else ''}" for a, g in SETS])
def test_emulated_arithmetic_passes_the_checks(arith, small_grad, kind, shape, capsys):
    r, (r_split, r_spec) = ratios(kind, shape, arith, small_grad)
    with capsys.disabled():
        print(f"\nemulated {arith}{' (|dy| <= 2^-22, amax)' if small_grad else ''} {kind} {shape}: (a) {r[0]:.4f} (b) {r[1]:.4f} "
              f"(c) {r[2]:.4f}   split reference alone: (a) {r_split:.4f}, (a) with the specified eps {r_spec:.4f}")
    assert max(r) <= 1.0, r
    # the unit roundoff is what makes (a) sound: the specified half of it fails on the exact arithmetic where an output is ONE product
    assert r_split <= 1.0 and (r_spec <= 1.0 or R.products(kind, *operands(kind, shape, small_grad)[:2], G.G33) == 1), (r_split, r_spec)


_WIDE = [s for s in SHAPES if s != (1, 1, 1)]
_BOTH = [("bf16x1", False), ("f16x1", False)]
_GRAD = [("f16x1", True)]
MUTANTS = [  # (mutant, operand sets, kinds, shapes it applies to)
    ("bf16_trunc", [("bf16x1", False)], R.KINDS, SHAPES),
    ("wrong_format", _BOTH, R.KINDS, SHAPES),
    ("amax_ignored", _GRAD, ("dgrad", "wgrad"), SHAPES),
    ("scale_off_by_one", _GRAD, ("dgrad", "wgrad"), SHAPES),
    ("chunk_dropped", _BOTH, ("fwd", "dgrad"), SHAPES),
    ("taps_not_flipped", _BOTH, ("dgrad",), _WIDE),  # (a 1 x 1 image meets the centre tap only)
    ("w_edge", _BOTH, R.KINDS, SHAPES),
    ("row_twice", _BOTH, ("wgrad",), SHAPES),
    ("seg_last_row_dropped", _BOTH, ("wgrad",), SHAPES),
]
_CASES = [(m, a, g, k, s) for (m, sets, kinds, shapes) in MUTANTS for (a, g) in sets for k in kinds for s in shapes]


@pytest.mark.parametrize("mutant,arith,small_grad,kind,shape", _CASES, ids=[f"{m}-{a}-{k}-{_sid(s)}" for (m, a, g, k, s) in _CASES])
def test_convolution_mutant_fails_a_check(mutant, arith, small_grad, kind, shape, capsys):
    r, _ = ratios(kind, shape, arith, small_grad, mutant)
    with capsys.disabled():
        print(f"\nmutant {mutant} {arith} {kind} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert max(r) > 1.0, r


# ---- epilogues ----------------------------------------------------------------------------------------------------------------------
def epilogue32(conv, bias, res, act, z=None, h=None, mutant=None):
    """the kernel's epilogue in float32: act(conv + bias + res), act 4 = (1 - z) h + z tanh(.)"""
    bb = bias.float().view(1, -1, 1, 1)
    late_b, late_r = mutant == "bias_after_act", mutant == "res_after_act"
    y = conv.float()
    if not late_b:
        y = y + bb
    if not late_r:
        y = y + res.float()
    if act == G.ACT_RELU:
        y = y.clamp_min(0.0)
    elif act == G.ACT_SIGMOID:
        y = torch.sigmoid(y)
    elif act >= G.ACT_TANH:
        y = torch.tanh(y)
    if late_b:
        y = y + bb
    if late_r:
        y = y + res.float()
    if act == G.ACT_GRU:
        y = z * h + (1.0 - z) * y if mutant == "gru_swapped" else (1.0 - z) * h + z * y
    return y


def _epi_inputs(shape):
    b, h, w = shape
    bias = seeded((COUT,), 8200)
    res = seeded((b, COUT, h, w), 8201) * 0.5
    z = torch.sigmoid(seeded((b, COUT, h, w), 8202) * 3.0)
    hp = torch.tanh(seeded((b, COUT, h, w), 8203) * 2.0)
    return bias, res, z, hp


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("arith", G.ARITHS)
@pytest.mark.parametrize("mutant", [None, "bias_after_act", "res_after_act"])
def test_relu_epilogue_and_its_order_mutants(mutant, arith, shape, capsys):
    """act 0 / 1 through check()'s epilogue: bias and residual enter BEFORE the activation"""
    p, q, _, _ = operands("fwd", shape, False)
    bias, res, _, _ = _epi_inputs(shape)
    got = epilogue32(emulate("fwd", p, q, arith), bias, res, G.ACT_RELU, mutant=mutant)
    ex = R.exact("fwd", p, q, geom=G.G33)
    r = G.check(got, arith, R.products("fwd", p, q, G.G33), ex, G.split_reference("fwd", p, q, arith),
                epilogue=(torch.ones(COUT), bias, res, True))
    with capsys.disabled():
        print(f"\nrelu epilogue {mutant} {arith} {shape}: (a) {r[0]:.3g} (b) {r[1]:.3g} (c) {r[2]:.3g}")
    assert (max(r) > 1.0) if mutant else (max(r) <= 1.0), r


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("act,mutant", [(G.ACT_SIGMOID, None), (G.ACT_TANH, None), (G.ACT_GRU, None), (G.ACT_SIGMOID, "bias_after_act"),
                                        (G.ACT_TANH, "res_after_act"), (G.ACT_GRU, "res_after_act"), (G.ACT_GRU, "gru_swapped")])
def test_gate_activations_against_the_pre_activation(act, mutant, shape, capsys):
    """act 2 / 3 / 4 against the fp64 function of the act 0 output y0 of the same (emulated) launch"""
    p, q, _, _ = operands("fwd", shape, False)
    bias, res, z, hp = _epi_inputs(shape)
    conv = emulate("fwd", p, q, "bf16x1")
    y0 = epilogue32(conv, bias, res, G.ACT_NONE)
    got = epilogue32(conv, bias, res, act, z, hp, mutant)
    ratio, err = G.act_check(got, y0, act, z, hp)
    with capsys.disabled():
        print(f"\nact {act} {mutant} {shape}: err / allowance {ratio:.3g}, max |err| {err:.3g}")
    assert (ratio > 1.0) if mutant else (ratio <= 1.0), (ratio, err)


# ---- the gate kernels -------------------------------------------------------------------------------------------------------------
def gate_inputs(npix, hid, inp, orient="z", seed=8300):
    """fp32 rows of one update's backward.  orient: which half of dzr holds its maximum -- "z": a large g; "r": a large d_rhx"""
    zr = torch.sigmoid(seeded((npix, 2 * hid), seed) * 3.0)
    q = torch.tanh(seeded((npix, hid), seed + 1) * 2.5)
    hx = seeded((npix, hid + inp), seed + 2)
    hx[:, :hid] = torch.tanh(hx[:, :hid] * 2.0)
    g = seeded((npix, hid), seed + 3) * (3.0 if orient == "z" else 1e-3)
    d_rhx = seeded((npix, hid + inp), seed + 4) * (1e-3 if orient == "z" else 3.0)
    d_hx = seeded((npix, hid + inp), seed + 5) * 0.1
    return zr, q, hx, g, d_rhx, d_hx


def gates32(zr, q, hx, g, d_rhx, d_hx, hid, mutant=None):
    """float32 emulation of the five kernels, in their expression order; returns every output and the two amax values"""
    z, r, h = zr[:, :hid], zr[:, hid:], hx[:, :hid]
    o = {}
    o["rhx"] = hx.clone()
    o["rhx"][:, :hid] = (z if mutant == "r_from_z_half" else r) * h
    o["hn"] = (1.0 - z) * h + z * q
    gate = g * z
    o["dq"] = gate * ((1.0 - q) if mutant == "one_minus_q" else (1.0 - q * q))
    o["dz"] = g * (q - h) * z * (1.0 - z)
    acc1 = g * (1.0 - z)
    d = d_rhx[:, :hid]
    o["dr"] = d * h * r * (1.0 - r)
    o["dh_acc"] = d * r if mutant == "dh_acc_overwritten" else acc1 + d * r
    o["dh_acc1"] = acc1
    o["dh"] = o["dh_acc"] + d_hx[:, :hid]
    o["dx"] = d_rhx[:, hid:] + (d_hx[:, :d_hx.shape[1] - hid] if mutant == "dx_at_dh_offset" else d_hx[:, hid:])
    o["am_q"] = R.amax_of(z * (1.0 - q * q)) if mutant == "amax_before_g" else R.amax_of(o["dq"])
    o["am_z"] = R.amax_of(o["dz"]) if mutant == "bwd2_amax_missing" else max(R.amax_of(o["dz"]), R.amax_of(o["dr"]))
    return o


def gate_verdict(o, zr, q, hx, g, d_rhx, d_hx, hid):
    """largest ratio of every output against its fp64 reference; the amax values against amax_of of the fp32 outputs"""
    r = {"rhx": G.gate_ratio(o["rhx"], G.gru_rh(zr, hx, hid)), "hn": G.gate_ratio(o["hn"], G.gru_out(zr, q, hx, hid))}
    b1 = G.gru_bwd1(g, zr, q, hx, hid)
    r.update(dq=G.gate_ratio(o["dq"], b1["dq"]), dz=G.gate_ratio(o["dz"], b1["dz"]), dh_acc1=G.gate_ratio(o["dh_acc1"], b1["dh_acc"]))
    b2 = G.gru_bwd2(o["dh_acc1"], d_rhx, zr, hx, hid)
    r.update(dr=G.gate_ratio(o["dr"], b2["dr"]), dh_acc=G.gate_ratio(o["dh_acc"], b2["dh_acc"]))
    b3 = G.gru_bwd3(o["dh_acc"], d_rhx, d_hx, hid)
    r.update(dh=G.gate_ratio(o["dh"], b3["dh"]), dx=G.gate_ratio(o["dx"], b3["dx"]))
    amax_ok = o["am_q"] == R.amax_of(o["dq"]) and o["am_z"] == R.amax_of(torch.cat([o["dz"], o["dr"]], 1))
    return r, amax_ok


GATE_SHAPES = [(1, 4, 4), (77, 36, 20), (4099, 128, 256)]


@pytest.mark.parametrize("orient", ["z", "r"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=_sid)
def test_emulated_gates_pass_the_counted_bounds(shape, orient, capsys):
    npix, hid, inp = shape
    t = gate_inputs(npix, hid, inp, orient)
    r, amax_ok = gate_verdict(gates32(*t, hid), *t, hid)
    with capsys.disabled():
        print(f"\nemulated gates {shape} max in {orient} half: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0 and amax_ok, (r, amax_ok)
    dz, dr = R.amax_of(gates32(*t, hid)["dz"]), R.amax_of(gates32(*t, hid)["dr"])
    assert (dz > dr) if orient == "z" else (dr > dz)  # the orientation is what it says


GATE_MUTANTS = [("r_from_z_half", "rhx", ("z", "r")), ("one_minus_q", "dq", ("z", "r")), ("dh_acc_overwritten", "dh_acc", ("z", "r")),
                ("dx_at_dh_offset", "dx", ("z", "r")), ("bwd2_amax_missing", "amax", ("r",)), ("amax_before_g", "amax", ("z", "r"))]
_GCASES = [(m, what, s, o) for (m, what, orients) in GATE_MUTANTS for s in GATE_SHAPES for o in orients]


@pytest.mark.parametrize("mutant,what,shape,orient", _GCASES, ids=[f"{m}-{_sid(s)}-{o}" for (m, w, s, o) in _GCASES])
def test_gate_mutant_is_seen(mutant, what, shape, orient):
    npix, hid, inp = shape
    t = gate_inputs(npix, hid, inp, orient)
    r, amax_ok = gate_verdict(gates32(*t, hid, mutant=mutant), *t, hid)
    if what == "amax":
        assert not amax_ok
    else:
        assert r[what] > 1.0, (what, r)


# ---- the references themselves ------------------------------------------------------------------------------------------------------
def test_round_operand_is_the_documented_rounding():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 2.0 ** -30, 3.0 * 2.0 ** -26, 1000.5])
    bf = G.round_operand(t, "bf16x1")  # ties to even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6; above a tie: away
    assert bf.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 2.0 ** -30, 3.0 * 2.0 ** -26, 1000.0]
    assert torch.equal(bf, t.bfloat16().double())
    h0 = G.round_operand(t, "f16x1")   # no amax: k = 0, fp16 as it is -- 2^-30 is below half the smallest subnormal
    assert torch.equal(h0, t.half().double()) and h0[4] == 0.0 and h0[5] == 2.0 ** -24 and h0[6] == 1000.5
    hk = G.round_operand(t[4:6], "f16x1", amax=3.0 * 2.0 ** -26)  # k = 14 + 25: both exact
    assert R.f16_scale_exp(3.0 * 2.0 ** -26) == 39 and torch.equal(hk, t[4:6].double())
    assert G.scale_exp("f16x1", None) == 0 and G.scale_exp("bf16x1", 5.0) == 0 and G.scale_exp("f16x1", 1.0) == 14


@pytest.mark.parametrize("arith,small_grad", SETS, ids=[f"{a}{'-grad' if g else ''}" for a, g in SETS])
def test_split_reference_is_torchs_fp64_convolution_of_the_rounded_operands(arith, small_grad):
    shape = (2, 5, 7)
    for kind in R.KINDS:
        p, q, amp, amq = operands(kind, shape, small_grad)
        rp, rq = G.round_operand(p, arith, amp), G.round_operand(q, arith, amq)
        if kind == "fwd":
            want = F.conv2d(rp, rq, padding=1)
        elif kind == "wgrad":
            want = torch.nn.grad.conv2d_weight(rp, (COUT, CIN, 3, 3), rq, padding=1)
        else:  # the adjoint of the forward, from autograd
            xr = torch.zeros(shape[0], CIN, *shape[1:], dtype=torch.float64, requires_grad=True)
            want, = torch.autograd.grad(F.conv2d(xr, rq, padding=1), xr, rp)
        for gemm in (False, True):
            got = G.split_reference(kind, p, q, arith, amp, amq, gemm=gemm)
            assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-13 * float(want.abs().max()), (kind, gemm)
        assert float((want - R.exact(kind, p, q, geom=G.G33)["y"]).abs().max()) > 0.0  # (the rounding is not a no-op)


def test_gate_references_are_autograd_of_the_reference_lines():
    """forward and backward of one update assembled from the five fp64 gate references and fp64 convolutions, against
    _reference_gru (update.py:32-41) and its autograd gradients"""
    torch.manual_seed(3)
    b, hid, inp, hh, ww = 2, 4, 8, 5, 6
    mod = nn.Module()
    for name in ("convz", "convr", "convq"):
        setattr(mod, name, nn.Conv2d(hid + inp, hid, 3, padding=1))
    mod.double()
    h = torch.tanh(torch.randn(b, hid, hh, ww, dtype=torch.float64)).requires_grad_(True)
    x = torch.randn(b, inp, hh, ww, dtype=torch.float64, requires_grad=True)
    cz, cr, cq = [torch.randn(b, hid, hh, ww, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    cot = torch.randn(b, hid, hh, ww, dtype=torch.float64)
    out = _reference_gru(mod, h, cz, cr, cq, x)
    gh, gx, gcz, gcr, gcq = torch.autograd.grad(out, (h, x, cz, cr, cq), cot)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(b * hh * ww, -1)
    img = lambda t: t.reshape(b, hh, ww, -1).permute(0, 3, 1, 2)
    with torch.no_grad():
        wzr, bzr = torch.cat([mod.convz.weight, mod.convr.weight]), torch.cat([mod.convz.bias, mod.convr.bias])
        hx = torch.cat([h, x], 1)
        zr = rows(torch.sigmoid(F.conv2d(hx, wzr, bzr, padding=1) + torch.cat([cz, cr], 1)))
        rhx = G.gru_rh(zr, rows(hx), hid)[0]
        q = rows(torch.tanh(F.conv2d(img(rhx), mod.convq.weight, mod.convq.bias, padding=1) + cq))
        hn = G.gru_out(zr, q, rows(hx), hid)[0]
        assert float((img(hn) - out).abs().max()) <= 1e-14
        b1 = G.gru_bwd1(rows(cot), zr, q, rows(hx), hid)
        dq = b1["dq"][0]
        d_rhx = rows(F.conv_transpose2d(img(dq), mod.convq.weight, padding=1))
        b2 = G.gru_bwd2(b1["dh_acc"][0], d_rhx, zr, rows(hx), hid)
        dzr = torch.cat([b1["dz"][0], b2["dr"][0]], 1)
        d_hx = rows(F.conv_transpose2d(img(dzr), wzr, padding=1))
        b3 = G.gru_bwd3(b2["dh_acc"][0], d_rhx, d_hx, hid)
    for got, want in ((img(b3["dh"][0]), gh), (img(b3["dx"][0]), gx), (img(dzr[:, :hid]), gcz), (img(dzr[:, hid:]), gcr), (img(dq), gcq)):
        assert float((got - want).abs().max()) <= 1e-13 * max(float(want.abs().max()), 1.0)
