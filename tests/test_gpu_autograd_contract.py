"""Every hand-written autograd node of the PSMNet and RAFT-Stereo paths under the configurations the models never produce: partial
requires_grad, unused outputs, strided / offset cotangents, replayed and pruned backward passes -- each gradient against
the CPU fp64 autograd of a plain torch composition (tests/_autograd_contract.py holds the harness, its rules and the table
of determinism classes and nullable kernel pointers; tests/test_autograd_contract_cpu.py proves that each check can fail).

Shapes are the minima of the per-kernel tests.  ReLU layers: the inputs' seed is the first one for which no fp64
pre-activation lies within 1e-5 of zero (relative to the median magnitude), so that no rounding of a correct kernel can flip a mask
bit -- decided on the CPU, from the reference alone."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import agg3d, conv3d, costconv, ops, torch_ops  # noqa: E402,F401  (torch_ops registers torch.ops.azhip)
from activezero_amd import handover as handover_mod  # noqa: E402
from activezero_amd.nets.psmnet import psmnet_3  # noqa: E402
from activezero_amd.nets.psmnet import psmnet_submodule_3 as sub3  # noqa: E402
from oracle import psmnet_oracle as po  # noqa: E402
from oracle import reprojection_oracle as ro  # noqa: E402
from activezero_amd.nets.raft import corr as raft_corr  # noqa: E402
from activezero_amd.nets.raft import gru as raft_gru  # noqa: E402
from oracle.raft_gru_oracle import ConvGRUOracle  # noqa: E402
from tests import _autograd_contract as H  # noqa: E402
from tests import _raft_head_ref as rh  # noqa: E402
from tests import _fp64ref as R64  # noqa: E402
from tests import _gru_fp64ref as GR  # noqa: E402
from tests import _reduce_ref as RD  # noqa: E402
from tests import _reproj_fp64ref as RP  # noqa: E402
from tests import _softargmin_fp64ref as SA  # noqa: E402
from tests import _volume_fp64ref as V  # noqa: E402
from activezero_amd import overlap  # noqa: E402
import numpy as np  # noqa: E402
from tests._weights import procedural_tensor, seeded  # noqa: E402
from tests.test_gpu_conv3d import _fork_net  # noqa: E402
from tests.test_gpu_raft_corr import _torch_reference as _corr_reference  # noqa: E402

DEV = "cuda:0"
EPS = 1e-5
RELU_MARGIN = 1e-5
# what the wrappers REFUSE (H.Node.refuses), as measured by H.check_input_forms: a `_chk` without `.contiguous()` refuses the
# forms that are not dense-contiguous; the library refuses (AZ_EINVAL) a pointer that is not 16-byte aligned where a kernel
# loads float4 unconditionally -- az_absmax on the operands of the f16x3 / one-part convolutions, az_cost_volume_fwd_ndhwc,
# az_spp_upsample_fwd, az_costconv_assemble_fwd; BatchNorm's gamma and beta are read through their pointers.
STRIDED, UNALIGNED, PARAM = H.NOT_DENSE, ("offset1",), ("slice",)


def _bn_refusals(weights=("weight",), affine=("gamma", "beta"), x=STRIDED + UNALIGNED, extra=None):
    r = {"x": x, **{k: UNALIGNED for k in weights}, **{k: PARAM for k in affine}}
    r.update(extra or {})
    return {k: v for k, v in r.items() if v}


def _plant(unit, weight, gamma, beta, rm=None, rv=None):
    """the node's inputs in place of the container's parameters (plain leaves whose requires_grad the harness chose)"""
    for m, name, t in ((unit[0], "weight", weight), (unit[1], "weight", gamma), (unit[1], "bias", beta)):
        del m._parameters[name]
        setattr(m, name, t)
    if rm is not None:
        unit[1].running_mean.copy_(rm)
        unit[1].running_var.copy_(rv)
    return unit


def _bn_params(tag, c, special):
    gamma, beta = procedural_tensor(tag + ".weight", (c,)), procedural_tensor(tag + ".bias", (c,))
    rm, rv = procedural_tensor(tag + ".running_mean", (c,)), procedural_tensor(tag + ".running_var", (c,))
    if special:  # the channels an eval-mode backward can get wrong: gamma == 0, gamma < 0, a running_var of eps' size
        gamma[3], gamma[5], rv[7] = 0.0, -0.8, 4e-5
    return gamma, beta, rm, rv


def _safe_seed(base, pre_of):
    """first seed whose fp64 ReLU arguments all keep RELU_MARGIN away from zero"""
    for seed in range(base, base + 64):
        pre = pre_of(seed)
        if float(pre.abs().min()) > RELU_MARGIN * float(pre.abs().median()):
            return seed
    raise AssertionError("no seed keeps the ReLU arguments away from zero")


# ---- conv_bn: 3-D convolution + BatchNorm3d (+ residual) (+ ReLU) -----------------------------------------------------------
def _ref_bn(z, i, train, groups=1):
    rm, rv = i["rm"].clone(), i["rv"].clone()
    if groups == 1:
        return F.batch_norm(z, rm, rv, i["gamma"], i["beta"], train, 0.1, EPS)
    return torch.cat([F.batch_norm(p, rm, rv, i["gamma"], i["beta"], train, 0.1, EPS) for p in z.chunk(groups)])


def _convbn_node(mode, cin, cout, xshape, relu, res, train, arith):
    name = f"conv_bn m{mode} {cin}->{cout} {'train' if train else 'eval'}{' relu' if relu else ''}{' res' if res else ''} {arith}"
    wshape = (cin, cout, 3, 3, 3) if mode == conv3d.DECONV_S2 else (cout, cin, 3, 3, 3)
    stride = 1 if mode == conv3d.CONV_S1 else 2

    def pre(i):  # the ReLU's argument, channels-last like the product's tensors
        x = i["x"].permute(0, 4, 1, 2, 3)
        if mode == conv3d.DECONV_S2:
            z = F.conv_transpose3d(x, i["weight"], stride=2, padding=1, output_padding=1)
        else:
            z = F.conv3d(x, i["weight"], stride=stride, padding=1)
        z = _ref_bn(z, i, train).permute(0, 2, 3, 4, 1)
        return z + i["residual"] if res else z

    def build(seed):
        gamma, beta, rm, rv = _bn_params(name, cout, special=not train)
        i = {"x": seeded(xshape, seed), "weight": procedural_tensor(name + ".w", wshape), "gamma": gamma, "beta": beta,
             "rm": rm, "rv": rv}
        if res:
            b, d, h, w, _ = xshape
            out = {S1: (d, h, w), S2: ((d + 1) // 2, (h + 1) // 2, (w + 1) // 2), T2: (2 * d, 2 * h, 2 * w)}[mode]
            i["residual"] = seeded((b,) + out + (cout,), seed + 500)
        return i

    cache = {}

    def make(device):
        if "seed" not in cache:
            dbl = lambda i: {k: v.double() for k, v in i.items()}
            with torch.no_grad():
                cache["seed"] = _safe_seed(4000, lambda s: pre(dbl(build(s)))) if relu else 4000
        return {k: v.to(device) for k, v in build(cache["seed"]).items()}

    def call(i):
        unit = psmnet_3._up_unit(cin, cout) if mode == conv3d.DECONV_S2 else psmnet_3.convbn_3d(cin, cout, 3, stride, 1)
        unit = _plant(unit.to(DEV).train(train), i["weight"], i["gamma"], i["beta"], i["rm"], i["rv"])
        fn = agg3d.deconv_bn if mode == conv3d.DECONV_S2 else agg3d.conv_bn
        return fn(i["x"], unit, relu=relu, add=i.get("residual"), arith=conv3d.Arith.of(arith))

    diff = ("x", "weight", "gamma", "beta") + (("residual",) if res else ())
    return H.Node(name, make, call, diff, lambda i: F.relu(pre(i)) if relu else pre(i), atomic=("weight",),
                  refuses=_bn_refusals(extra={"residual": STRIDED}))


S1, S2, T2 = conv3d.CONV_S1, conv3d.CONV_S2, conv3d.DECONV_S2
V32, V32_FINE, V64 = (1, 4, 8, 16, 32), (1, 8, 16, 32, 32), (1, 4, 8, 16, 64)
CONVBN = [
    _convbn_node(S1, 32, 32, V32, True, True, True, "f16x3"),
    _convbn_node(S1, 32, 32, V32, True, False, True, "f16x3"),
    _convbn_node(S1, 32, 32, V32, False, True, True, "f16x3"),
    _convbn_node(S1, 32, 32, V32, False, False, True, "f16x3"),
    _convbn_node(S1, 32, 32, V32, True, True, True, "bf16x6"),
    _convbn_node(S2, 32, 64, V32_FINE, True, False, True, "f16x3"),
    _convbn_node(T2, 64, 32, V64, True, True, True, "f16x3"),
    _convbn_node(S1, 32, 32, V32, True, True, False, "f16x3"),
    _convbn_node(S1, 32, 32, V32, False, False, False, "f16x3"),
    _convbn_node(S2, 32, 64, V32_FINE, True, False, False, "f16x3"),
    _convbn_node(T2, 64, 32, V64, False, True, False, "f16x3"),
]


# ---- _convbn_unit: 2-D convolution (conv2d.py) + bn_act (bn2d.py) ------------------------------------------------------------
def _unit2d_node(cin, cout, stride, relu, res, train, groups, skip=False):
    name = (f"convbn_unit {cin}->{cout} s{stride} {'train' if train else 'eval'} g{groups}{' relu' if relu else ''}"
            f"{' res' if res else ''}{' skip' if skip else ''}")
    xshape = (2, cin, 8, 12)

    def pre(i):
        z = _ref_bn(F.conv2d(i["x"], i["weight"], stride=stride, padding=1), i, train, groups)
        return z + i["residual"] if res else z

    def build(seed):
        gamma, beta, rm, rv = _bn_params(name, cout, special=not train)
        i = {"x": seeded(xshape, seed), "weight": procedural_tensor(name + ".w", (cout, cin, 3, 3)), "gamma": gamma,
             "beta": beta, "rm": rm, "rv": rv}
        if res:
            i["residual"] = seeded((2, cout, 8 // stride, 12 // stride), seed + 500)
        return i

    cache = {}

    def make(device):
        if "seed" not in cache:
            dbl = lambda i: {k: v.double() for k, v in i.items()}
            with torch.no_grad():
                cache["seed"] = _safe_seed(4100, lambda s: pre(dbl(build(s)))) if relu else 4100
        i = {k: v.to(device) for k, v in build(cache["seed"]).items()}
        for k in ("x", "residual"):  # the extractor's activations live in channels_last memory
            if k in i and device != "cpu":
                i[k] = i[k].contiguous(memory_format=torch.channels_last)
        return i

    def call(i):
        unit = _plant(sub3.convbn(cin, cout, 3, stride, 1, 1).to(DEV).train(train), i["weight"], i["gamma"], i["beta"],
                      i["rm"], i["rv"])
        return sub3._convbn_unit(i["x"], unit, relu=relu, residual=i.get("residual"), groups=groups, skip=skip,
                                 arith=conv3d.Arith.of("f16x3"))

    def ref(i):
        y = F.relu(pre(i)) if relu else pre(i)
        return (y, i["x"] * 1.0) if skip else y

    diff = ("x", "weight", "gamma", "beta") + (("residual",) if res else ())
    # stride 1: az_absmax of x and of the weight; the stride-2 volume route packs its weight first; the 3-channel patches
    # route reads neither through a float4
    refuses = _bn_refusals(x=UNALIGNED) if stride == 1 else _bn_refusals((), x=UNALIGNED if cin == 32 else ())
    return H.Node(name, make, call, diff, ref, atomic=("weight",), refuses=refuses)


UNIT2D = [
    _unit2d_node(32, 32, 1, True, False, True, 1),
    _unit2d_node(32, 32, 1, False, True, True, 2),
    _unit2d_node(64, 64, 1, True, True, True, 2),
    _unit2d_node(32, 64, 2, True, False, True, 1),       # _ConvS2Vol: Partials stay empty, bn_act takes its own statistics
    _unit2d_node(3, 32, 2, True, False, True, 2),        # _ConvS2Patches, the 3-channel first layer (no sink: no token)
    _unit2d_node(32, 32, 1, True, True, False, 1),
    _unit2d_node(64, 64, 1, False, False, False, 2),
]
UNIT2D_SKIP = _unit2d_node(32, 32, 1, True, False, True, 1, skip=True)


# ---- conv_logits, add, fanout ---------------------------------------------------------------------------------------------------
def _logits_node(addend):
    shape = (1, 3, 5, 7)

    def make(device):
        i = {"x": seeded(shape + (32,), 4201), "weight": procedural_tensor("contract.c1.w", (1, 32, 3, 3, 3))}
        if addend:
            i["addend"] = seeded(shape, 4202)
        return {k: v.to(device) for k, v in i.items()}

    def call(i):
        conv = nn.Conv3d(32, 1, 3, padding=1, bias=False).to(DEV)
        del conv._parameters["weight"]
        conv.weight = i["weight"]
        return agg3d.conv_logits(i["x"], conv, add=i.get("addend"))

    def ref(i):
        y = F.conv3d(i["x"].permute(0, 4, 1, 2, 3), i["weight"], padding=1)[:, 0]
        return y + i["addend"] if addend else y

    return H.Node(f"conv_logits{' +addend' if addend else ''}", make, call, ("x", "weight") + (("addend",) if addend else ()),
                  ref, atomic=("weight",), refuses={"x": STRIDED})


def _deferred_node():
    """conv_bn(defer=...) -> conv_logits(affine=...): the train-mode classifier head, whose BatchNorm + ReLU is applied by
    the 32 -> 1 convolution while it stages its operand (the pending DeferredAffine)"""
    name = "conv_bn defer -> conv_logits affine"

    def pre(i):
        return _ref_bn(F.conv3d(i["x"].permute(0, 4, 1, 2, 3), i["weight"], padding=1), i, True)

    def build(seed):
        gamma, beta, rm, rv = _bn_params(name, 32, False)
        return {"x": seeded(V32, seed), "weight": procedural_tensor(name + ".w", (32, 32, 3, 3, 3)), "gamma": gamma, "beta": beta,
                "rm": rm, "rv": rv, "w1": procedural_tensor(name + ".w1", (1, 32, 3, 3, 3)), "addend": seeded(V32[:4], seed + 7)}

    cache = {}

    def make(device):
        if "seed" not in cache:
            with torch.no_grad():
                cache["seed"] = _safe_seed(4300, lambda s: pre({k: v.double() for k, v in build(s).items()}))
        return {k: v.to(device) for k, v in build(cache["seed"]).items()}

    def call(i):
        unit = _plant(psmnet_3.convbn_3d(32, 32, 3, 1, 1).to(DEV).train(), i["weight"], i["gamma"], i["beta"], i["rm"], i["rv"])
        conv = nn.Conv3d(32, 1, 3, padding=1, bias=False).to(DEV)
        del conv._parameters["weight"]
        conv.weight = i["w1"]
        defer = conv3d.DeferredAffine()
        t = agg3d.conv_bn(i["x"], unit, relu=True, arith=conv3d.Arith.of("f16x3"), defer=defer)
        assert defer.pending
        return agg3d.conv_logits(t, conv, add=i["addend"], affine=defer)

    return H.Node(name, make, call, ("x", "weight", "gamma", "beta", "w1", "addend"),
                  lambda i: F.conv3d(F.relu(pre(i)), i["w1"], padding=1)[:, 0] + i["addend"], atomic=("weight", "w1"),
                  refuses=_bn_refusals())


ADD = H.Node("add", lambda dev: {"a": seeded(V32, 4401).to(dev), "b": seeded(V32, 4402).to(dev)},
             lambda i: agg3d.add(i["a"], i["b"]), ("a", "b"), lambda i: i["a"] + i["b"], refuses={"a": STRIDED, "b": STRIDED})


def _fanout_node(n):
    return H.Node(f"fanout n={n}", lambda dev: {"x": seeded(V32, 4500 + n).to(dev)}, lambda i: agg3d.fanout(i["x"], n), ("x",),
                  lambda i: tuple(i["x"] * 1.0 for _ in range(n)))



# ---- the element-wise error models of the single-launch nodes (tests/_*_fp64ref.py, tests/_reduce_ref.py), fed with this
# ---- file's inputs and cotangents: (reference, bound) per element, ratio = the largest error / bound
def _cached(fn):
    memo = {}
    return lambda i, cots, got, key: fn(i, cots, got, memo.setdefault(key, {}))


def _np(t):
    return t.detach().cpu().numpy()


def _cv_elementwise(layout):
    def f(i, cots, got, memo):
        if "ref" not in memo:
            memo["ref"] = V.k3_backward_ref(_np(cots[0]), 4, layout)
        gl, gr, bl, br = memo["ref"]
        return {k: V.ratio(got[k], r, b) for k, r, b in (("fl", gl, bl), ("fr", gr, br)) if k in got}
    return _cached(f)


@_cached
def _softargmin_elementwise(i, cots, got, memo):
    if "ref" not in memo:
        memo["ref"] = SA.head(_np(i["logits"]), _np(cots[0])[:, 0])
    return {"logits": SA.ratio(got["logits"], memo["ref"]["grad"], memo["ref"]["grad_bound"])} if "logits" in got else {}


@_cached
def _warp_elementwise(i, cots, got, memo):
    if "ref" not in memo:
        memo["ref"] = RP.warp_bwd(_np(cots[0]), _np(i["img"]), _np(i["disp"]))
    (gd, gd_mag), (gi, gi_mag, cnt) = memo["ref"]
    out = {}
    if "disp" in got:
        out["disp"] = RP.ratio(got["disp"][:, 0], gd, RP.warp_gdisp_bound(gd_mag, i["img"].shape[1]))
    if "img" in got:
        out["img"] = RP.ratio(got["img"], gi, RP.warp_gimg_bound(gi_mag, cnt))
    return out


@_cached
def _reproj_elementwise(i, cots, got, memo):
    if "pp" not in memo:
        memo["pp"] = RP.patch_pixel(_np(i["l"]), _np(i["r"]), _np(i["disp"]), 3, -1.0)
    mask = _np(i["mask"]).astype(np.uint8)[:, 0] if "mask" in i else None
    return {"disp": RP.k8_check_grad(got["disp"], memo["pp"], mask, float(cots[0]), tuple(i["l"].shape) + (3,), -1.0)}


def _exact(got, want):
    return V.ratio(got, want, np.zeros_like(want))


@_cached
def _disp_loss_elementwise(i, cots, got, memo):
    preds, gt, mask = [_np(i[k]) for k in ("p3", "p2", "p1")], _np(i["gt"]), _np(i["mask"]).astype(np.uint8)
    count = RD.k12_fwd(preds, gt, mask, 0.0, float("inf"))[1]
    want = RD.k12_bwd(preds, gt, mask, 0.0, float("inf"), float(cots[0]), count)
    return {k: _exact(got[k], w) for k, w in zip(("p3", "p2", "p1"), want) if k in got}


@_cached
def _seq_loss_elementwise(i, cots, got, memo):
    gt, valid = _np(i["gt"]), _np(i["valid"])
    out = {}
    for k, w in enumerate(rh.sequence_weights(3)):
        pred = _np(i[f"q{k}"])
        count = RD.k16_fwd(pred, gt, valid, 700.0, -1)[1]
        if f"q{k}" in got:
            out[f"q{k}"] = _exact(got[f"q{k}"], RD.k16_bwd(pred, gt, valid, 700.0, -1, float(cots[0]), count, w))
    return out


@_cached
def _spp_elementwise(i, cots, got, memo):
    g = np.ascontiguousarray(np.moveaxis(_np(cots[0]), 1, -1))  # rows [B,H,W,320]
    out = {k: _exact(np.moveaxis(got[k], 1, -1), g[..., at:at + c]) for k, at, c in (("raw", 0, 64), ("skip", 64, 128)) if k in got}
    for k in range(4):
        name = f"b{k}"
        if name in got:
            if name not in memo:
                memo[name] = V.spp_backward_ref(g[..., 192 + 32 * k:224 + 32 * k], *i[name].shape[2:])
            out[name] = V.ratio(np.moveaxis(got[name], 1, -1), *memo[name])
    return out


# ---- ops.py --------------------------------------------------------------------------------------------------------------------
def _ops_nodes():
    fshape = (1, 8, 5, 12)
    feats = lambda dev: {"fl": seeded(fshape, 4601).to(dev), "fr": seeded(fshape, 4602).to(dev)}
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    yield H.Node("cost_volume", feats, lambda i: ops.cost_volume(i["fl"], i["fr"], 4), ("fl", "fr"),
                 lambda i: po.build_cost_volume(i["fl"], i["fr"], 4), elementwise=_cv_elementwise("ncdhw"))
    yield H.Node("cost_volume_ndhwc", lambda dev: {k: nhwc(v) for k, v in feats(dev).items()},
                 lambda i: ops.cost_volume_ndhwc(i["fl"], i["fr"], 4), ("fl", "fr"),
                 lambda i: po.build_cost_volume(i["fl"].permute(0, 3, 1, 2), i["fr"].permute(0, 3, 1, 2), 4).permute(0, 2, 3, 4, 1),
                 elementwise=_cv_elementwise("ndhwc"), refuses={"fl": UNALIGNED, "fr": UNALIGNED})
    yield H.Node("softargmin", lambda dev: {"logits": seeded((1, 6, 3, 5), 4610, -3.0, 3.0).to(dev)},
                 lambda i: ops.softargmin(i["logits"]), ("logits",),
                 lambda i: po.soft_argmin_head(i["logits"][:, None], 24, 12, 20), atomic=("logits",),
                 elementwise=_softargmin_elementwise)
    yield H.Node("warp_gather", lambda dev: {"img": seeded((2, 3, 6, 17), 4620).to(dev),
                                             "disp": seeded((2, 1, 6, 17), 4621, -3.0, 3.0).to(dev)},
                 lambda i: ops.warp_gather(i["img"], i["disp"]), ("img", "disp"),
                 lambda i: ro.apply_disparity(i["img"], i["disp"]), atomic=("img",), elementwise=_warp_elementwise)

    def loss_inputs(dev):
        gt = seeded((2, 1, 5, 9), 4630, 0.0, 40.0)
        i = {f"p{k}": gt + seeded((2, 1, 5, 9), 4630 + k, -2.5, 2.5) for k in (3, 2, 1)}
        i["gt"], i["mask"] = gt, seeded((2, 1, 5, 9), 4634) > -0.6
        return {k: v.to(dev) for k, v in i.items()}

    yield H.Node("disp_loss", loss_inputs, lambda i: ops.disp_loss(i["p3"], i["p2"], i["p1"], i["gt"], i["mask"]),
                 ("p3", "p2", "p1"), lambda i: po.psmnet_disp_loss((i["p3"], i["p2"], i["p1"]), i["gt"], i["mask"]),
                 images=False, elementwise=_disp_loss_elementwise)

    for with_mask in (False, True):
        def reproj_inputs(dev, with_mask=with_mask):
            i = {"l": seeded((2, 1, 6, 17), 4640, 0.0, 1.0), "r": seeded((2, 1, 6, 17), 4641, 0.0, 1.0),
                 "disp": seeded((2, 1, 6, 17), 4642, 0.0, 3.0)}
            if with_mask:
                i["mask"] = seeded((2, 1, 6, 17), 4643) > -0.5
            return {k: v.to(dev) for k, v in i.items()}

        yield H.Node(f"patch_reprojection ps 3{' mask' if with_mask else ''}", reproj_inputs,
                     lambda i: ops.patch_reprojection(i["l"], i["r"], i["disp"], i.get("mask"), ps=3, want_vis=False)[0],
                     ("disp",), lambda i: ro.get_reproj_error_patch(i["l"], i["r"], i["disp"], i.get("mask"), ps=3)[0],
                     images=False, elementwise=_reproj_elementwise)

    yield H.Node("convex_upsample fp32 mask",
                 lambda dev: {"flow": seeded((1, 2, 5, 7), 4650, -4.0, 4.0).to(dev), "mask": rh.make_mask_logits((1, 144, 5, 7), 4651).to(dev)},
                 lambda i: ops.convex_upsample(i["flow"], i["mask"], 4), ("flow", "mask"),
                 lambda i: rh.convex_upsample(i["flow"], i["mask"], 4))

    # the mask as the fp16 tensor RAFT's autocast hands over: its gradient is fp16 too, so both references are rounded to fp16
    yield H.Node("convex_upsample fp16 mask",
                 lambda dev: {"flow": seeded((1, 2, 5, 7), 4650, -4.0, 4.0).to(dev),
                              "mask": rh.make_mask_logits((1, 144, 5, 7), 4651).half().to(dev)},
                 lambda i: ops.convex_upsample(i["flow"], i["mask"], 4), ("flow", "mask"),
                 lambda i: rh.convex_upsample(i["flow"], i["mask"].to(i["flow"].dtype), 4), half=("mask",))

    def seq_inputs(dev):
        gt = seeded((2, 1, 5, 9), 4660, -40.0, 0.0)
        i = {f"q{k}": -gt + seeded((2, 1, 5, 9), 4661 + k, -2.5, 2.5) for k in range(3)}
        i["gt"], i["valid"] = gt, (seeded((2, 1, 5, 9), 4665) > -0.6).float()
        return {k: v.to(dev) for k, v in i.items()}

    yield H.Node("sequence_loss n=3", seq_inputs, lambda i: ops.sequence_loss([i["q0"], i["q1"], i["q2"]], i["gt"], i["valid"]),
                 ("q0", "q1", "q2"), lambda i: rh.sequence_loss([i["q0"], i["q1"], i["q2"]], i["gt"], i["valid"]),
                 images=False, elementwise=_seq_loss_elementwise)

    # K29: three scales of one ground truth (ops.multiscale_disp_loss); the reference is utils/disp_losses.py's formula
    MS_SHIFTS, MS_WEIGHTS = (0, 1, 2), (1.0, 0.7, 0.5)

    def ms_inputs(dev):
        gt = seeded((2, 1, 9, 13), 4636, 0.0, 40.0)
        i = {"gt": gt, "mask": seeded((2, 1, 9, 13), 4637) > -0.6}
        for k, s in enumerate(MS_SHIFTS):
            at = gt[:, :, ::1 << s, ::1 << s][:, :, :9 >> s, :13 >> s]
            i[f"p{k}"] = at + seeded(tuple(at.shape), 4638 + k, -2.5, 2.5)
        return {k: v.to(dev) for k, v in i.items()}

    def ms_ref(i):
        total = 0.0
        for k, (s, wt) in enumerate(zip(MS_SHIFTS, MS_WEIGHTS)):
            p = i[f"p{k}"]
            pick = lambda t: t[:, :, ::1 << s, ::1 << s][:, :, :p.shape[2], :p.shape[3]]
            m = pick(i["mask"])
            total = total + wt * F.smooth_l1_loss(p[m], pick(i["gt"])[m], reduction="mean")
        return total

    yield H.Node("multiscale_disp_loss", ms_inputs,
                 lambda i: ops.multiscale_disp_loss([i["p0"], i["p1"], i["p2"]], i["gt"], i["mask"], MS_SHIFTS, MS_WEIGHTS),
                 ("p0", "p1", "p2"), ms_ref, images=False)

    def spp_inputs(dev):
        i = {"raw": seeded((1, 64, 8, 12), 4670), "skip": seeded((1, 128, 8, 12), 4671)}
        for k, hw in enumerate(((1, 1), (2, 3), (3, 5), (4, 6))):
            i[f"b{k}"] = seeded((1, 32) + hw, 4672 + k)
        return {k: (v.to(dev).contiguous(memory_format=torch.channels_last) if dev != "cpu" else v) for k, v in i.items()}

    branches = lambda i: [i[f"b{k}"] for k in range(4)]
    yield H.Node("spp_concat", spp_inputs, lambda i: sub3.spp_concat(i["raw"], i["skip"], branches(i)),
                 ("raw", "skip", "b0", "b1", "b2", "b3"),
                 lambda i: torch.cat([i["raw"], i["skip"]] + [F.interpolate(t, size=(8, 12), mode="bilinear", align_corners=True)
                                                              for t in branches(i)], 1), elementwise=_spp_elementwise,
                 refuses={f"b{k}": UNALIGNED for k in range(4)})

    # costconv._Merge and _Assemble, through the fused cost-volume convolution that owns them
    yield H.Node("costvol_conv", lambda dev: {"fl": seeded((2, 32, 6, 12), 4690).to(dev), "fr": seeded((2, 32, 6, 12), 4691).to(dev),
                                              "weight": seeded((32, 64, 3, 3, 3), 4692, -0.1, 0.1).to(dev)},
                 lambda i: costconv.costvol_conv(i["fl"], i["fr"], 3, i["weight"]), ("fl", "fr", "weight"),
                 lambda i: F.conv3d(po.build_cost_volume(i["fl"], i["fr"], 3), i["weight"], padding=1).permute(0, 2, 3, 4, 1),
                 atomic=("weight",))
    # the autograd formulas registered for the torch.ops.azhip operators (torch_ops.py)
    yield H.Node("torch.ops.azhip.warp_gather", lambda dev: {"img": seeded((2, 3, 6, 17), 4620).to(dev),
                                                             "disp": seeded((2, 1, 6, 17), 4621, -3.0, 3.0).to(dev)},
                 lambda i: torch.ops.azhip.warp_gather(i["img"], i["disp"]), ("img", "disp"),
                 lambda i: ro.apply_disparity(i["img"], i["disp"]), atomic=("img",), elementwise=_warp_elementwise)
    yield H.Node("torch.ops.azhip.conv3d", lambda dev: {"x": seeded(V32, 4695).to(dev),
                                                        "weight": procedural_tensor("contract.op.w", (32, 32, 3, 3, 3)).to(dev)},
                 lambda i: torch.ops.azhip.conv3d(i["x"], i["weight"], S1), ("x", "weight"),
                 lambda i: F.conv3d(i["x"].permute(0, 4, 1, 2, 3), i["weight"], padding=1).permute(0, 2, 3, 4, 1),
                 atomic=("weight",), refuses={"x": UNALIGNED, "weight": UNALIGNED})


# ---- costconv._Assemble and _Merge, called directly: each backward is one launch with an element-wise model ------------------
ASM = (2, 6, 12, 3)  # B, H, W, D


def _assemble_ref(i):
    fb, fe, g = i["fb"], i["fe"], i["g"]
    B, H, W, D = ASM
    valid, f_bulk, f_edge, gb = V.asm_map(D, W)
    Fb, Fe, G = (t.reshape(B, H, -1, 32) for t in (fb, fe, g))
    cols = []
    for d in range(D):
        row = []
        for x in range(W):
            if not valid[d, x]:
                row.append(torch.zeros(B, H, 32, dtype=fb.dtype))
            else:
                f = Fb[:, :, int(f_bulk[d, x])] if f_bulk[d, x] >= 0 else Fe[:, :, int(f_edge[d, x])]
                row.append(f + G[:, :, int(gb[d, x])])
        cols.append(torch.stack(row, 2))
    return torch.stack(cols, 1)


@_cached
def _assemble_elementwise(i, cots, got, memo):
    if "ref" not in memo:
        memo["ref"] = V.asm_backward_ref(_np(cots[0]), ASM[3])
    return {k: V.ratio(got[k], *memo["ref"][n]) for k, n in (("fb", "dF_bulk"), ("fe", "dF_edge"), ("g", "dG")) if k in got}


ASSEMBLE = H.Node("costconv._Assemble", lambda dev: {k: seeded(sh, 4900 + j).to(dev)
                                                     for j, (k, sh) in enumerate(zip(("fb", "fe", "g"), V.asm_shapes(ASM)))},
                  lambda i: costconv._Assemble.apply(i["fb"], i["fe"], i["g"], ASM[3]), ("fb", "fe", "g"), _assemble_ref,
                  elementwise=_assemble_elementwise, refuses={k: STRIDED + UNALIGNED for k in ("fb", "fe", "g")})


def _merge_masks(dev):
    return tuple(m.to(dev) for m in costconv._masks(torch.device("cpu"), ASM[3]))


@_cached
def _merge_elementwise(i, cots, got, memo):
    ml, mr = (_np(m) for m in _merge_masks("cpu"))
    ncls = ml.shape[0]
    gkl = _np(cots[0]) if 0 in cots else np.zeros((ncls, 5, 32, 32, 3, 3), np.float32)
    gkr = _np(cots[1]) if 1 in cots else np.zeros((ncls, 2, 32, 32, 3, 5), np.float32)
    return {"weight": V.ratio(got["weight"], *V.merge_backward_ref(gkl, gkr, ml, mr))}


def _merge_call(i):
    ml, mr = _merge_masks(i["weight"].device)
    return costconv._Merge.apply(i["weight"], ml.contiguous(), mr.contiguous(), ml.shape[0])


def _merge_ref(i):
    ml, mr = (m.to(i["weight"].dtype) for m in _merge_masks("cpu"))
    return (torch.einsum("oidhw,cedw->ceoihw", i["weight"][:, :32], ml), torch.einsum("oidhw,cedwj->ceoihj", i["weight"][:, 32:], mr))


MERGE = H.Node("costconv._Merge", lambda dev: {"weight": seeded((32, 64, 3, 3, 3), 4910, -0.1, 0.1).to(dev)}, _merge_call,
               ("weight",), _merge_ref, images=False, elementwise=_merge_elementwise)


# ---- BasicBlock: the skip route (conv2d._ConvSame with its second output) and the downsample route ----------------------------
def _block_node(down):
    cin, cout, stride = (32, 64, 2) if down else (32, 32, 1)
    name = f"BasicBlock {cin}->{cout}{' downsample' if down else ' skip'}"
    units = ("1", "2") + (("d",) if down else ())

    def build(seed):
        i = {"x": seeded((2, cin, 8, 12), seed)}
        for u in units:
            k = 1 if u == "d" else 3
            i["w" + u] = procedural_tensor(f"{name}.w{u}", (cout, cin if u != "2" else cout, k, k))
            i["g" + u], i["b" + u] = _bn_params(f"{name}.bn{u}", cout, False)[:2]
        return i

    def bn(z, i, u):
        return torch.cat([F.batch_norm(p, None, None, i["g" + u], i["b" + u], True, 0.1, EPS) for p in z.chunk(2)])

    def pre(i):
        return bn(F.conv2d(i["x"], i["w1"], stride=stride, padding=1), i, "1")

    def ref(i):
        short = bn(F.conv2d(i["x"], i["wd"], stride=2), i, "d") if down else i["x"]
        return bn(F.conv2d(F.relu(pre(i)), i["w2"], padding=1), i, "2") + short

    cache = {}

    def make(device):
        if "seed" not in cache:
            with torch.no_grad():
                cache["seed"] = _safe_seed(4950, lambda s: pre({k: v.double() for k, v in build(s).items()}))
        i = {k: v.to(device) for k, v in build(cache["seed"]).items()}
        if device != "cpu":
            i["x"] = i["x"].contiguous(memory_format=torch.channels_last)
        return i

    def call(i):
        ds = sub3.convbn(cin, cout, 1, 2, 0, 1) if down else None
        blk = sub3.BasicBlock(cin, cout, stride, ds, 1, 1).to(DEV).train()
        _plant(blk.conv1[0], i["w1"], i["g1"], i["b1"])
        _plant(blk.conv2, i["w2"], i["g2"], i["b2"])
        if down:
            _plant(blk.downsample, i["wd"], i["gd"], i["bd"])
        return blk(i["x"], groups=2, arith=conv3d.Arith.of("f16x3"))

    diff = ["x"] + [p + u for u in units for p in ("w", "g", "b")]
    return H.Node(name, make, call, diff, ref, atomic=["w" + u for u in units],
                  refuses=_bn_refusals(("w2", "wd") if down else ("w1", "w2"), [p + u for u in units for p in ("g", "b")], UNALIGNED))


BLOCKS = [_block_node(False), _block_node(True)]


# ---- RAFT: three lookups reading one correlation pyramid (corr._Volume, _Pool, _Lookup and its _LevelSums) ----------------
LAST_BLOCK = []


def _corr_node():
    b, c, h, w = 2, 64, 3, 75

    def make(dev):
        i = {"f1": seeded((b, c, h, w), 4680), "f2": seeded((b, c, h, w), 4681)}
        base = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")[::-1], 0).float()[None].repeat(b, 1, 1, 1)
        for k in range(3):
            i[f"c{k}"] = base.clone()
            i[f"c{k}"][:, 0] -= seeded((b, h, w), 4682 + k, -3.0, 0.6 * w)  # includes far out-of-range lookups
        return {k: v.to(dev) for k, v in i.items()}

    def call(i):
        blk = raft_corr.CorrBlock1D(i["f1"], i["f2"])
        LAST_BLOCK[:] = [blk]
        return tuple(blk(i[f"c{k}"]) for k in range(3))

    def dirty(outs):
        sums = LAST_BLOCK[0]._sums
        return [] if (sums.task is None and all(t is None for t in sums.bufs)) else ["_LevelSums keeps its buffers"]

    return H.Node("CorrBlock1D x3 lookups", make, call, ("f1", "f2"),
                  lambda i: tuple(_corr_reference(i["f1"], i["f2"], i[f"c{k}"].to(i["f1"].dtype))[0] for k in range(3)),
                  atomic=("f1", "f2"), dirty=dirty)


CORR = _corr_node()


# ---- RAFT: the ConvGRU update, one fused node per operand format and the operator form -----------------------------------------
def _gru_node(arithmetic):
    names = ("wz", "wr", "wq", "bz", "br", "bq")
    shape = lambda c: (1, c, 6, 10)

    def make(dev):
        i = {"h": seeded(shape(32), 4800), "cz": seeded(shape(32), 4801), "cr": seeded(shape(32), 4802),
             "cq": seeded(shape(32), 4803), "x0": seeded(shape(12), 4804), "x1": seeded(shape(20), 4805)}
        for k, n in enumerate(names[:3]):
            i[n] = procedural_tensor(f"contract.gru.{n}", (32, 64, 3, 3))
            i[names[3 + k]] = seeded((32,), 4810 + k, -0.2, 0.2)
        i = {k: v.to(dev) for k, v in i.items()}
        if dev != "cpu":  # (x0 stays a dense NCHW image: gru._assemble's other route)
            for k in ("h", "cz", "cr", "cq", "x1"):
                i[k] = i[k].contiguous(memory_format=torch.channels_last)
        return i

    def plant(mod, i, as_parameters):
        for conv, w, b in ((mod.convz, "wz", "bz"), (mod.convr, "wr", "br"), (mod.convq, "wq", "bq")):
            for attr, k in (("weight", w), ("bias", b)):
                if as_parameters:  # ConvGRU.forward asks its parameters whether autograd is wanted: the leaves are Parameters
                    i[k] = nn.Parameter(i[k].detach(), requires_grad=i[k].requires_grad)
                    setattr(conv, attr, i[k])
                else:
                    del conv._parameters[attr]
                    setattr(conv, attr, i[k])
        return mod

    def call(i):
        mod = raft_gru.ConvGRU(32, 32).to(DEV)
        mod.train_arithmetic = arithmetic
        return plant(mod, i, True)(i["h"], i["cz"], i["cr"], i["cq"], i["x0"], i["x1"])

    def ref(i):
        mod = plant(ConvGRUOracle(32, 32).to(i["h"].dtype), i, False)
        return mod(i["h"], i["cz"], i["cr"], i["cq"], i["x0"], i["x1"])

    def vjp(i, cots):
        """the step's forward and backward chained in fp64 from the pieces of tests/_gru_fp64ref.py, with the operand rounding
        of every convolution launch (and the power-of-two amax scaling of the f16x1 gradient operands, gru.py:289-297) in it"""
        arith, c = ("f16x1" if arithmetic == "f16x1" else "bf16x1"), 32
        col = lambda *ks: torch.cat([i[k] for k in ks]).double().view(1, -1, 1, 1)
        hx = torch.cat([i["h"], i["x0"], i["x1"]], 1).contiguous()
        wzr = torch.cat([i["wz"], i["wr"]], 0)
        zr = torch.sigmoid(GR.split_reference("fwd", hx, wzr, arith) + col("bz", "br") + torch.cat([i["cz"], i["cr"]], 1).double())
        rhx = GR.gru_rh(zr, hx, c)[0]
        q = torch.tanh(GR.split_reference("fwd", rhx, i["wq"], arith) + col("bq") + i["cq"].double())
        b1 = GR.gru_bwd1(cots[0], zr, q, hx, c)
        dq = b1["dq"][0]
        am_q = R64.amax_of(dq)
        d_rhx = GR.split_reference("dgrad", dq, i["wq"], arith, amax_p=am_q)
        b2 = GR.gru_bwd2(b1["dh_acc"][0], d_rhx, zr, hx, c)
        dzr = torch.cat([b1["dz"][0], b2["dr"][0]], 1)
        am_z = R64.amax_of(dzr)
        d_hx = GR.split_reference("dgrad", dzr, wzr, arith, amax_p=am_z)
        b3 = GR.gru_bwd3(b2["dh_acc"][0], d_rhx, d_hx, c)
        gwzr = GR.split_reference("wgrad", hx, dzr, arith, amax_q=am_z)
        dx, gbzr = b3["dx"][0], dzr.sum(dim=(0, 2, 3))
        return {"h": b3["dh"][0], "cz": dzr[:, :c], "cr": dzr[:, c:], "cq": dq, "x0": dx[:, :12], "x1": dx[:, 12:],
                "wz": gwzr[:c], "wr": gwzr[c:], "wq": GR.split_reference("wgrad", rhx, dq, arith, amax_q=am_q),
                "bz": gbzr[:c], "br": gbzr[c:], "bq": dq.sum(dim=(0, 2, 3))}

    # (operator form: h collects three gradients that the engine sums in its own order)
    atomic = names[:3] + (("h",) if arithmetic == "bf16_ops" else ())
    return H.Node(f"ConvGRU {arithmetic}", make, call, ("h", "cz", "cr", "cq", "x0", "x1") + names, ref, atomic=atomic,
                  vjp=vjp)

# gru._Conv3x3Bf16 called directly: its input and weight gradients are one launch each, held to the one-part model of
# tests/_gru_fp64ref.py (the operand rounding is in split_reference, not in a tolerance); the bias gradient is a torch sum
@_cached
def _conv_bf16_elementwise(i, cots, got, memo):
    dy, out = cots[0], {}
    for name, kind, p, q in (("x", "dgrad", dy, i["w"]), ("w", "wgrad", i["x"], dy)):
        if name in got:
            if name not in memo:
                memo[name] = (R64.exact(kind, p, q, gemm=False, geom=GR.G33), GR.split_reference(kind, p, q, "bf16x1"),
                              R64.products(kind, p, q, GR.G33), R64.wgrad_blocks_2d(q) if kind == "wgrad" else None)
            ex, sref, K, blocks = memo[name]
            out[name] = max(GR.check(torch.from_numpy(np.ascontiguousarray(got[name])), "bf16x1", K, ex, sref, blocks=blocks))
    return out


CONV_BF16 = H.Node("gru._Conv3x3Bf16 64->32",
                   lambda dev: {"x": seeded((1, 64, 6, 10), 4820).to(dev), "w": seeded((32, 64, 3, 3), 4821, -0.2, 0.2).to(dev),
                                "bias": seeded((32,), 4822, -0.2, 0.2).to(dev)},
                   lambda i: raft_gru._Conv3x3Bf16.apply(i["x"], i["w"], i["bias"]), ("x", "w", "bias"),
                   lambda i: F.conv2d(i["x"], i["w"], i["bias"], padding=1), atomic=("w",), elementwise=_conv_bf16_elementwise)


GRU = [_gru_node("f16x1"), _gru_node("bf16"), _gru_node("bf16_ops")]
OPS = list(_ops_nodes())
SINGLE = CONVBN + UNIT2D + [_logits_node(False), _logits_node(True), _deferred_node(), ADD] + OPS + GRU + BLOCKS + [ASSEMBLE, CONV_BF16]
MULTI = [(UNIT2D_SKIP, 2), (_fanout_node(2), 2), (_fanout_node(4), 4), (MERGE, 2)]
ALL = SINGLE + [n for n, _ in MULTI]
ids = lambda nodes: [str(n).replace(" ", "_") for n in nodes]


def record(capsys, node, check, *args):
    """run one check of the harness and print the node's worst error / bound per configuration family, pass or fail"""
    report = H.Report()
    try:
        check(node, DEV, report, *args)
    finally:
        with capsys.disabled():
            print("".join("\n" + line for line in report.lines()), end="")


@pytest.mark.parametrize("node", ALL, ids=ids(ALL))
def test_flag_subsets(node, capsys):
    record(capsys, node, H.check_flags)


@pytest.mark.parametrize("node", ALL, ids=ids(ALL))
def test_cotangent_forms(node, capsys):
    record(capsys, node, H.check_forms)


@pytest.mark.parametrize("node", ALL, ids=ids(ALL))
def test_replay(node, capsys):
    record(capsys, node, H.check_replay)


@pytest.mark.parametrize("node,n_out", MULTI, ids=ids([n for n, _ in MULTI]))
def test_unused_outputs(node, n_out, capsys):
    record(capsys, node, H.check_unused, n_out)


EVAL = [n for n in CONVBN + UNIT2D if " eval" in str(n)]


@pytest.mark.parametrize("node", EVAL, ids=ids(EVAL))
def test_eval_mode_dgamma_of_the_special_channels(node, capsys):
    """frozen statistics: d gamma = sum dz (x - running_mean) / sqrt(running_var + eps) does not depend on gamma.  The same
    per-tensor rule on each special channel alone (gamma == 0, gamma < 0, running_var of eps' size), where the whole-tensor
    norm, which the small-variance channel dominates, cannot hide it"""
    g64, g32 = H.reference(node)
    got = H.run(node, DEV, ("gamma",))["gamma"]
    for ch in (3, 5, 7):
        r = H.ratio(got[ch:ch + 1], g64["gamma"][ch:ch + 1], g32["gamma"][ch:ch + 1])
        with capsys.disabled():
            print(f"\n{node} [channel {ch} of d/dgamma alone]: error/bound {r:.4f}", end="")
        assert r <= 1.0, f"{node}: d/dgamma[{ch}] misses the fp64 rule, error/bound {r:.3f}"


@pytest.fixture(params=[True, False], ids=["acc", "per_lookup"])
def lookup_acc(request, monkeypatch):
    monkeypatch.setattr(raft_corr, "LOOKUP_ACC", request.param)
    return request.param


def test_corr_flag_subsets(lookup_acc, capsys):
    record(capsys, CORR, H.check_flags)


def test_corr_unused_outputs(lookup_acc, capsys):
    record(capsys, CORR, H.check_unused, 3)


def test_corr_cotangent_forms(lookup_acc, capsys):
    record(capsys, CORR, H.check_forms)


def test_corr_replay_releases_the_level_sums(lookup_acc, capsys):
    record(capsys, CORR, H.check_replay)


def test_corr_pruned_pass_then_full_pass(lookup_acc, capsys):
    record(capsys, CORR, H.check_pruned_then_full, (1,))


# ---- the first layer with the pass's weight-gradient sink: the token slot of _ConvS2Patches, and the sink closed afterwards -------
FIRST = _unit2d_node(3, 32, 2, True, False, True, 2)


@pytest.mark.parametrize("need_x", [True, False], ids=["x_and_parameters", "parameters_only"])
def test_first_layer_token_and_the_sink_is_closed(need_x, capsys):
    """conv2d._ConvS2Patches takes the sink's token as its fourth input (needs_input_grad[3]) and its gradient is what makes
    overlap._Tail join the side stream after every weight-gradient launch: with an armed overlap.Sink, as the models run it,
    every gradient against fp64, the non-atomic ones equal to the sink-less run, and no sink left open after backward"""
    i = H.leaves(FIRST, DEV, ("x",) if need_x else ())
    unit = sub3.convbn(3, 32, 3, 2, 1, 1).to(DEV).train()
    with torch.no_grad():
        for p, k in ((unit[0].weight, "weight"), (unit[1].weight, "gamma"), (unit[1].bias, "beta")):
            p.copy_(i[k])
    sink = overlap.begin(unit, i["x"])
    assert sink is not None and sink.token.requires_grad
    y = sub3._convbn_unit(i["x"], unit, relu=True, groups=2, arith=conv3d.Arith.of("f16x3")._replace(sink=sink))
    assert sink.armed and sink.live
    cot = H.cot_values(y.shape, 0).to(DEV)
    y.backward(cot)
    assert sink.joined and not sink.live and not sink.pending and not sink.keep and sink.arena is None
    torch.cuda.synchronize()
    grads = {"x": i["x"].grad, "weight": unit[0].weight.grad, "gamma": unit[1].weight.grad, "beta": unit[1].bias.grad}
    need = (("x",) if need_x else ()) + ("weight", "gamma", "beta")
    report = H.Report()
    try:
        H.check_fp64(FIRST, grads, need, None, "random", report, "armed sink")
    finally:
        with capsys.disabled():
            print("".join("\n" + line for line in report.lines()), end="")
    H.same(FIRST, grads, H.run(FIRST, DEV, need), need, "armed sink vs no sink")


LAST_SINK = []


def _first_sink_node():
    """the first layer as the models run it: an armed overlap.Sink whose token is the fourth input of conv2d._ConvS2Patches and
    whose _Gate aliases stand for the weight; `dirty` asks that the pass's sink is joined and empty after every backward"""
    def call(i):
        unit = _plant(sub3.convbn(3, 32, 3, 2, 1, 1).to(DEV).train(), i["weight"], i["gamma"], i["beta"], i["rm"], i["rv"])
        sink = overlap.begin(unit, i["x"])
        assert sink is not None and sink.token.requires_grad
        LAST_SINK[:] = [sink]
        y = sub3._convbn_unit(i["x"], unit, relu=True, groups=2, arith=conv3d.Arith.of("f16x3")._replace(sink=sink))
        assert sink.armed and sink.live
        return y

    def dirty(outs):
        k = LAST_SINK[0]
        return [] if (k.joined and not k.live and not k.pending and not k.keep and k.arena is None) else ["the sink is still open"]

    return H.Node("convbn_unit 3->32 s2 train g2 relu, armed sink", FIRST.make, call, FIRST.diff, FIRST.ref, atomic=("weight",),
                  dirty=dirty, refuses=FIRST.refuses)


FIRST_SINK = _first_sink_node()


# ---- several consumers of one tensor: handover.GradSlot --------------------------------------------------------------------------
def _fork_node():
    names = [f"{p}{k}" for k in range(4) for p in ("w", "g", "b")]

    def build(seed):
        i = {"x": seeded(V32, seed)}
        for k in range(4):
            i[f"w{k}"] = procedural_tensor(f"contract.fork{k}.w", (32, 32, 3, 3, 3))
            i[f"g{k}"], i[f"b{k}"] = _bn_params(f"contract.fork{k}", 32, False)[:2]
        return i

    def bn(z, i, k):
        return F.batch_norm(z, None, None, i[f"g{k}"], i[f"b{k}"], True, 0.1, EPS)

    def pres(i):  # the three ReLU arguments of the net
        x = i["x"].permute(0, 4, 1, 2, 3)
        pt = bn(F.conv3d(x, i["w0"], padding=1), i, 0)
        t = F.relu(pt)
        pu = bn(F.conv3d(t, i["w1"], padding=1), i, 1)
        pw = bn(F.conv3d(t, i["w3"], padding=1), i, 3)
        v = bn(F.conv3d(F.relu(pu), i["w2"], padding=1), i, 2) + t
        return pt, pu, pw, v

    def ref(i):
        pt, pu, pw, v = pres(i)
        return tuple(o.permute(0, 2, 3, 4, 1) for o in (v, F.relu(pw), F.relu(pt)))

    cache = {}

    def make(device):
        if "seed" not in cache:
            with torch.no_grad():
                cache["seed"] = _safe_seed(4700, lambda s: torch.cat(
                    [p.flatten() / p.abs().median() for p in pres({k: v.double() for k, v in build(s).items()})[:3]]))
        return {k: v.to(device) for k, v in build(cache["seed"]).items()}

    def call(i):
        units = [_plant(psmnet_3.convbn_3d(32, 32, 3, 1, 1).to(DEV).train(), i[f"w{k}"], i[f"g{k}"], i[f"b{k}"])
                 for k in range(4)]
        return _fork_net(i["x"], units, conv3d.Arith.of("f16x3"))

    return H.Node("fork net", make, call, ["x"] + names, ref, atomic=[f"w{k}" for k in range(4)], dirty=H.slot_complaints,
                  refuses=_bn_refusals([f"w{k}" for k in range(4)], [f"{p}{k}" for k in range(4) for p in ("g", "b")]))


FORK = _fork_node()


@pytest.fixture(params=[True, False], ids=["handover", "engine"])
def handover(request, monkeypatch):
    monkeypatch.setattr(handover_mod, "_HANDOVER", request.param)
    return request.param


def test_fork_flag_subsets(handover, capsys):
    record(capsys, FORK, H.check_flags)


def test_fork_unused_outputs(handover, capsys):
    record(capsys, FORK, H.check_unused, 3)


def test_fork_cotangent_forms(handover, capsys):
    record(capsys, FORK, H.check_forms)


def test_fork_replay_leaves_the_slots_clean(handover, capsys):
    record(capsys, FORK, H.check_replay)


def test_fork_pruned_pass_then_full_pass(handover, capsys):
    """"first_only" then "all" (test_gpu_conv3d.py): the consumers that the engine pruned must leave nothing behind"""
    record(capsys, FORK, H.check_pruned_then_full, (0,))


def test_the_slots_are_there_to_be_checked(monkeypatch):
    monkeypatch.setattr(handover_mod, "_HANDOVER", True)
    outs = FORK.call(H.leaves(FORK, DEV, FORK.diff))
    slot = getattr(outs[2], "az_gslot", None)
    assert slot is not None and slot.expect == 3 and not H.slot_complaints(outs)
    slot.left -= 1
    assert H.slot_complaints(outs)


# ---- the memory form of the INPUTS: strides, storage offsets, alignment (H.check_input_forms) ---------------------------------
def _sum_parts_node(n):
    """handover.sum_parts is no autograd node: a plain sum of n gradients of one tensor, whose first part arrives in the other
    memory format (a plain torch consumer may hand back such a gradient)"""
    def make(dev):
        i = {f"p{k}": seeded(V32, 4960 + k).to(dev) for k in range(n)}
        i["p0"] = H.input_form(i["p0"], "format", dev)
        return i

    return H.Node(f"sum_parts n={n}", make, lambda i: handover_mod.sum_parts([i[f"p{k}"] for k in range(n)]), (),
                  lambda i: sum(i[f"p{k}"] for k in range(n)))


SUM_PARTS = [_sum_parts_node(n) for n in (2, 4, 5)]
INPUT_NODES = ALL + [CORR, FORK, FIRST_SINK] + SUM_PARTS


@pytest.mark.parametrize("node", INPUT_NODES, ids=ids(INPUT_NODES))
def test_input_forms(node, capsys):
    record(capsys, node, H.check_input_forms)


@pytest.mark.parametrize("node", SUM_PARTS, ids=ids(SUM_PARTS))
def test_sum_parts_with_the_first_part_in_the_other_format(node):
    """the sum has the parts' logical shape and, read logically, their sum's values (fp64 rule): before its fix sum_parts
    allocated the result *_like the first part and az_sum4 wrote it linearly, a permuted sum"""
    i = node.make(DEV)
    assert not i["p0"].is_contiguous()
    out = node.call(i)
    o64, o32 = H.out_reference(node)
    assert out.shape == o64[0].shape and H.ratio(out, o64[0], o32[0]) <= 1.0
