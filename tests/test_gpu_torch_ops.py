"""GPU: the dispatcher boundary (activezero_amd/torch_ops.py).  torch.library.opcheck on every `azhip::` overload
-- schema, autograd registration, fake against real metadata (shapes, strides, dtypes), and aot_dispatch with symbolic
sizes -- on contiguous samples, on the other memory format and on slices of a NaN-filled buffer; the registered autograd
formulas as contract Nodes (tests/_autograd_contract.py: flag subsets, cotangent forms, replay, input forms) against fp64;
warp_scatter and local_contrast_norm bit-equal to the ops wrappers.

Mismatched sizes are NOT passed to the GPU here: the checks that refuse them are shared by the fake and the CUDA
implementations and are exercised on the meta device (tests/test_torch_ops_cpu.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from activezero_amd import conv3d, ops, torch_ops  # noqa: E402,F401  (torch_ops registers torch.ops.azhip)
from oracle import psmnet_oracle as po  # noqa: E402
from oracle import reprojection_oracle as ro  # noqa: E402
from tests import _autograd_contract as H  # noqa: E402
from tests._weights import procedural_tensor, seeded  # noqa: E402
from tests.test_gpu_autograd_contract import (DEV, OPS, V32, V32_FINE, V64, _cv_elementwise, _reproj_elementwise,  # noqa: E402
                                              _safe_seed, _softargmin_elementwise, ids, record)

AZ = torch.ops.azhip
S1, S2, T2 = conv3d.CONV_S1, conv3d.CONV_S2, conv3d.DECONV_S2


# ---- contract Nodes of the registered autograd formulas -----------------------------------------------------------------------
def _softargmin_node(five):
    shape = (1, 1, 6, 3, 5) if five else (1, 6, 3, 5)
    four = (lambda t: t[:, 0]) if five else (lambda t: t)

    def elementwise(i, cots, got, key):
        got4 = {k: four(v) for k, v in got.items()}
        return _softargmin_elementwise({"logits": four(i["logits"])}, cots, got4, key)

    return H.Node(f"azhip.softargmin {len(shape)}-D", lambda dev: {"logits": seeded(shape, 4610, -3.0, 3.0).to(dev)},
                  lambda i: AZ.softargmin(i["logits"]), ("logits",),
                  lambda i: po.soft_argmin_head(four(i["logits"])[:, None], 24, 12, 20), atomic=("logits",), elementwise=elementwise)


def _conv3d_node(mode, cin, cout, xshape):
    wshape = (cin, cout, 3, 3, 3) if mode == T2 else (cout, cin, 3, 3, 3)

    def ref(i):
        x = i["x"].permute(0, 4, 1, 2, 3)
        if mode == T2:
            return F.conv_transpose3d(x, i["weight"], stride=2, padding=1, output_padding=1).permute(0, 2, 3, 4, 1)
        return F.conv3d(x, i["weight"], stride=1 if mode == S1 else 2, padding=1).permute(0, 2, 3, 4, 1)

    return H.Node(f"azhip.conv3d m{mode} {cin}->{cout}",
                  lambda dev: {"x": seeded(xshape, 4695 + mode).to(dev), "weight": procedural_tensor(f"ops.conv3d.m{mode}.w", wshape).to(dev)},
                  lambda i: AZ.conv3d(i["x"], i["weight"], mode), ("x", "weight"), ref, atomic=("weight",),
                  refuses={"x": ("offset1",), "weight": ("offset1",)})   # az_absmax loads float4: AZ_EINVAL off 16 bytes


def _bn3d_node(res, relu):
    """y = relu?(raw * scale + shift (+ residual)) with some ReLU arguments EXACTLY 0 (raw, shift and residual are 0 there:
    the derivative there is 0 on both sides, F.relu's and the formula's y > 0) and every other one away from 0"""
    shape, c = (1, 3, 4, 5, 32), 32

    def build(seed):
        i = {"raw": seeded(shape, seed), "scale": seeded((c,), seed + 1, 0.5, 1.5), "shift": seeded((c,), seed + 2, -0.3, 0.3)}
        i["scale"][3], i["scale"][5], i["shift"][2] = 0.0, -0.8, 0.0
        i["raw"][:, :, ::2, ::3, 2] = 0.0
        if res:
            i["residual"] = seeded(shape, seed + 3)
            i["residual"][:, :, ::2, ::3, 2] = 0.0
        return i

    def pre(i):
        z = i["raw"] * i["scale"] + i["shift"]
        return z + i["residual"] if res else z

    cache = {}

    def nonzero_pre(seed):
        z = pre({k: v.double() for k, v in build(seed).items()})
        assert int((z == 0).sum()) >= 6   # (channel 3, scale 0 and shift != 0, is away from 0; the planted ones are exact)
        return z[z != 0]

    def make(device):
        if "seed" not in cache:
            with torch.no_grad():
                cache["seed"] = _safe_seed(4980, nonzero_pre) if relu else 4980
        return {k: v.to(device) for k, v in build(cache["seed"]).items()}

    return H.Node(f"azhip.bn3d{' res' if res else ''}{' relu' if relu else ''}", make,
                  lambda i: AZ.bn3d(i["raw"], i["scale"], i["shift"], i.get("residual"), relu),
                  ("raw", "scale", "shift") + (("residual",) if res else ()), lambda i: F.relu(pre(i)) if relu else pre(i))


def _reproj_node(with_mask):
    def make(dev):
        i = {"l": seeded((2, 1, 6, 17), 4640, 0.0, 1.0), "r": seeded((2, 1, 6, 17), 4641, 0.0, 1.0),
             "disp": seeded((2, 1, 6, 17), 4642, 0.0, 3.0)}
        if with_mask:
            i["mask"] = seeded((2, 1, 6, 17), 4643) > -0.5
        return {k: v.to(dev) for k, v in i.items()}

    return H.Node(f"azhip.patch_reproj ps 3{' mask' if with_mask else ''}", make,
                  lambda i: AZ.patch_reproj(i["l"], i["r"], i["disp"], i.get("mask"), 3), ("disp",),
                  lambda i: ro.get_reproj_error_patch(i["l"], i["r"], i["disp"], i.get("mask"), ps=3)[0], images=False,
                  elementwise=_reproj_elementwise)


FEATS = lambda dev: {"fl": seeded((1, 8, 5, 12), 4601).to(dev), "fr": seeded((1, 8, 5, 12), 4602).to(dev)}
NODES = [
    H.Node("azhip.cost_volume", FEATS, lambda i: AZ.cost_volume(i["fl"], i["fr"], 4), ("fl", "fr"),
           lambda i: po.build_cost_volume(i["fl"], i["fr"], 4), elementwise=_cv_elementwise("ncdhw")),
    _softargmin_node(False), _softargmin_node(True),
    _conv3d_node(S1, 32, 32, V32), _conv3d_node(S2, 32, 64, V32_FINE), _conv3d_node(T2, 64, 32, V64),
    _bn3d_node(False, False), _bn3d_node(False, True), _bn3d_node(True, False), _bn3d_node(True, True),
    _reproj_node(False), _reproj_node(True),
]


@pytest.mark.parametrize("node", NODES, ids=ids(NODES))
def test_flag_subsets(node, capsys):
    record(capsys, node, H.check_flags)


@pytest.mark.parametrize("node", NODES, ids=ids(NODES))
def test_cotangent_forms(node, capsys):
    record(capsys, node, H.check_forms)


@pytest.mark.parametrize("node", NODES, ids=ids(NODES))
def test_replay(node, capsys):
    record(capsys, node, H.check_replay)


@pytest.mark.parametrize("node", NODES, ids=ids(NODES))
def test_input_forms(node, capsys):
    record(capsys, node, H.check_input_forms)


def _warp_node():
    return next(n for n in OPS if str(n) == "torch.ops.azhip.warp_gather")


def test_warp_gather_with_img_channels_last_and_disp_transposed():
    """the defect of _warp_gather_bwd (gradients allocated *_like the caller's permuted tensors, written linearly) in the
    very arrangement that showed it: both gradients equal to / within the atomic rule of the fresh run's, read logically"""
    node = _warp_node()
    fresh = H.run_inputs(node, DEV, {})[1]
    got = H.run_inputs(node, DEV, {"img": "format", "disp": "transposed"})[1]
    assert got["disp"].shape == fresh["disp"].shape and torch.equal(got["disp"].contiguous(), fresh["disp"])
    H.check_fp64(node, got, ("img", "disp"), None, "random", H.Report(), "img format, disp transposed")


# ---- forward-only operators against the ops wrappers --------------------------------------------------------------------------
def test_warp_scatter_and_lcn_are_bit_equal_to_the_wrappers():
    img = seeded((2, 3, 9, 17), 5101).to(DEV)
    disp = (seeded((2, 1, 9, 17), 5102, -4.0, 4.0).round().to(torch.int32)).to(DEV)
    for sign in (1, -1):
        assert torch.equal(AZ.warp_scatter(img, disp, sign), ops.warp_scatter(img, disp, sign))
    gray = seeded((2, 1, 13, 21), 5103, 0.0, 1.0).to(DEV)
    for k in (3, 9):
        a, b = AZ.local_contrast_norm(gray, k, 1e-5), ops.local_contrast_norm(gray, k, 1e-5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the operator form takes any strides (it copies); the wrapper refuses them
    cl = H.input_form(gray, "slice", DEV)
    a = AZ.local_contrast_norm(cl, 9, 1e-5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError):
        ops.local_contrast_norm(cl, 9, 1e-5)
    with pytest.raises(RuntimeError):
        AZ.warp_scatter(H.input_form(img, "format", DEV), disp, 1)


# ---- torch.library.opcheck on all fifteen overloads ------------------------------------------------------------------------------
UTILS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic")
SAMPLE_FORMS = ("fresh", "format", "slice")
REFUSES_STRIDES = {"warp_scatter"}   # ops.warp_scatter checks without copying: non-contiguous samples must raise


def _g64max(node, name):
    return float(H.reference(node)[0][name].abs().max())


def _samples():
    """{overload: (args builder(form) -> tuple, atol or None)}; the tensors of a sample are all in one form"""
    def f(t, form):
        if form == "fresh" or not isinstance(t, torch.Tensor):
            return t
        out = H.input_form(t, form, DEV)
        return t if out is None else out

    sa, wg, c3 = NODES[1], _warp_node(), NODES[3]
    logits = seeded((1, 6, 3, 5), 4610, -3.0, 3.0).to(DEV)
    disp, stats = AZ.softargmin_fwd(logits)
    g_sa = H.cot_values((1, 1, 12, 20), 0).to(DEV)
    img, dsp = seeded((2, 3, 6, 17), 4620).to(DEV), seeded((2, 1, 6, 17), 4621, -3.0, 3.0).to(DEV)
    g_wg = H.cot_values((2, 3, 6, 17), 0).to(DEV)
    x, w = seeded(V32, 4695).to(DEV), procedural_tensor("ops.conv3d.m0.w", (32, 32, 3, 3, 3)).to(DEV)
    g_c3 = H.cot_values(V32, 0).to(DEV)
    fl, fr = FEATS(DEV)["fl"], FEATS(DEV)["fr"]
    l, r, d, m = (_reproj_node(True).make(DEV)[k] for k in ("l", "r", "disp", "mask"))
    bn = _bn3d_node(True, True).make(DEV)
    idisp = seeded((2, 1, 6, 17), 5102, -4.0, 4.0).round().to(torch.int32).to(DEV)
    floor_sa = H.RULE_FLOOR * _g64max(sa, "logits")
    floor_wg = H.RULE_FLOOR * _g64max(wg, "img")
    floor_c3 = H.RULE_FLOOR * _g64max(c3, "weight")
    # a leaf WITHOUT a copy (clone() of a view that is not dense is contiguous: it would undo the slice), as H.run_inputs does
    grad = lambda t: t.detach().requires_grad_()
    return {
        "warp_scatter": (lambda s: (f(img, s), f(idisp, s), 1), None),
        "cost_volume": (lambda s: (grad(f(fl, s)), grad(f(fr, s)), 4), None),
        "cost_volume_bwd": (lambda s: (f(H.cot_values((1, 16, 4, 5, 12), 0).to(DEV), s), 4), None),
        "softargmin_fwd": (lambda s: (grad(f(logits, s)),), floor_sa),
        "softargmin_bwd": (lambda s: (f(g_sa, s), f(logits, s), f(stats, s), f(disp, s)), floor_sa),
        "softargmin": (lambda s: (grad(f(logits, s)),), floor_sa),
        "warp_gather": (lambda s: (grad(f(img, s)), grad(f(dsp, s))), floor_wg),
        "warp_gather_bwd": (lambda s: (f(g_wg, s), f(img, s), f(dsp, s), True), floor_wg),
        "local_contrast_norm": (lambda s: (f(img[:, :1].contiguous(), s), 3, 1e-5), None),
        "conv3d": (lambda s: (grad(f(x, s)), grad(f(w, s)), S1), floor_c3),
        "conv3d_input_grad": (lambda s: (f(g_c3, s), f(w, s), S1), None),
        "conv3d_weight_grad": (lambda s: (f(x, s), f(g_c3, s), f(w, s), S1), floor_c3),
        "bn3d": (lambda s: (grad(f(bn["raw"], s)), grad(f(bn["scale"], s)), grad(f(bn["shift"], s)), grad(f(bn["residual"], s)), True), None),
        "patch_reproj": (lambda s: (f(l, s), f(r, s), grad(f(d, s)), f(m, s), 3), None),
        "patch_reproj_bwd": (lambda s: (torch.tensor(0.75, device=DEV), f(l, s), f(r, s), f(d, s), f(m, s), 3), None),
    }


OVERLOADS = ("warp_scatter", "cost_volume", "softargmin", "softargmin_fwd", "softargmin_bwd", "warp_gather", "warp_gather_bwd",
             "local_contrast_norm", "cost_volume_bwd", "conv3d", "conv3d_input_grad", "conv3d_weight_grad", "bn3d", "patch_reproj",
             "patch_reproj_bwd")
_SAMPLES = {}


@pytest.mark.parametrize("form", SAMPLE_FORMS)
@pytest.mark.parametrize("name", OVERLOADS)
def test_opcheck(name, form):
    """float-atomic gradients (softargmin_bwd, warp_gather's grad_img, conv3d_weight_grad) differ between two runs of the
    same kernel, which is what aot_dispatch compares: atol = RULE_FLOOR * max|g64| from the CPU fp64 reference, rtol = 0 --
    the project's floor, not fitted to the code under test.  Everything else: opcheck's own defaults."""
    if not _SAMPLES:
        _SAMPLES.update(_samples())
    build, atol = _SAMPLES[name]
    op = getattr(AZ, name).default
    if form != "fresh" and name in REFUSES_STRIDES:
        with pytest.raises(RuntimeError):
            op(*build(form))
        return
    kw = {} if atol is None else {"atol": atol, "rtol": 0.0}
    args = build(form)
    if form == "slice":   # every tensor of the sample really is one (a scalar has no form)
        assert all(not a.is_contiguous() for a in args if isinstance(a, torch.Tensor) and a.dim() > 0)
        assert all(a.is_leaf for a in args if isinstance(a, torch.Tensor) and a.requires_grad)
    torch.library.opcheck(op, args, test_utils=UTILS, **kw)
