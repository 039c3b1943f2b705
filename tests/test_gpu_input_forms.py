"""GPU: the memory form of the INPUTS of every public entry point that has no autograd node (the nodes are covered by
tests/test_gpu_autograd_contract.py::test_input_forms).  One table, `(name, make inputs, call)`; every tensor input in every
form of tests/_autograd_contract.py's INPUT_FORMS -- the other memory format, the last two dimensions swapped in memory,
a slice of a larger NaN-filled buffer, contiguous views at storage offsets 12 and 1 -- alone, then all inputs together in
`format` and in `offset1`.  The rule:

  * either the call raises RuntimeError or TypeError (a refusal is a pass; FusedAdam raises ValueError for a parameter,
    torch.optim's convention, which tests/test_optim_cpu.py holds it to),
  * or every result equals the result on `.contiguous().clone()` inputs: integer, byte and element-wise float outputs
    exactly (NaN in the same places); the outputs an entry names as REDUCTIONS (fp64 accumulators of non-negative float32
    terms added in an unspecified order, and the float32 scalars made of them) within the rule of tests/_reduce_ref.py:
    each of two runs is within m 2^-52 sum|term| of the exact sum, so two runs differ by at most 2 m 2^-52 |sum| (the
    terms are >= 0, so sum|term| is the sum), m the number of elements of the largest input; a float32 scalar adds one
    rounding of its own, 2^-23 relative between two of them.

The two optimizer entries take the FIRST step, from zero moments.  For a parameter or gradient one float past 16-byte alignment
the Adam kernels (az_optim.hip) take their element-wise branches: adam_multi_kernel then fuses the other product of
v = b2 v + ((1 - b2) g) g than its float4 branch (equal bits from v = 0, one rounding apart from any other state, which
tests/_adam_ref.py's `misaligned` tensor covers under its own rule), and grad_sumsq_multi_kernel adds a thread's four squares
in another order (the clip coefficient came out bit-equal on these inputs).  All of it is held to equality here.

A silent wrong answer is the only failure this file hunts.  Shapes: the smallest of each entry's own test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import amax, ops  # noqa: E402
from activezero_amd import optim as az_optim  # noqa: E402
from activezero_amd.datasets import dataset_utils_gpu as du  # noqa: E402
from tests import _autograd_contract as H  # noqa: E402
from tests import _raft_head_ref as rh  # noqa: E402
from tests._weights import seeded  # noqa: E402

DEV = "cuda:0"
MAP = (2, 1, 7, 33)


def _maps():
    gt = seeded(MAP, 6001, 0.5, 40.0)
    return {"disp_gt": gt, "depth_gt": seeded(MAP, 6002, 0.2, 1.5), "disp_pred": gt + seeded(MAP, 6003, -2.5, 2.5),
            "mask": seeded(MAP, 6004) > -0.6, "fb": seeded((2,), 6005, 20.0, 40.0)}


def _metrics_inputs():
    return _maps()


def _obj_inputs():
    i = _maps()
    i["label"] = (seeded(MAP, 6006, 0.0, 2.999)).to(torch.int32)
    return i


def _eval_mask_inputs():
    return {"disp_l": seeded((2, 1, 5, 7), 6010, -10.0, 250.0), "depth_l": seeded((2, 1, 5, 7), 6011, -0.2, 2.0),
            "robot": (seeded((2, 3, 4), 6012) > 0.5).float(), "realsense": seeded((2, 1, 10, 14), 6013, -0.5, 1.5)}


def _gt_inputs():
    return {"disp_r": seeded((2, 1, 8, 14), 6020, 2.0, 6.0), "extra": seeded((2, 2, 8, 14), 6021), "keep": seeded((2, 1, 8, 14), 6022)}


def _result_inputs():
    i = _maps()
    return {"pred": i["disp_pred"].abs() + 0.5, "gt_disp": i["disp_gt"], "gt_depth": i["depth_gt"], "mask": i["mask"], "fb": i["fb"]}


def _depth_inputs():
    mm = lambda s: seeded((2, 6, 10), s, -200.0, 1500.0).clamp(min=0).to(torch.int32)  # noqa: E731  (zeros: no measurement)
    return {"l": mm(6030), "r": mm(6031), "focal": seeded((2,), 6032, 400.0, 450.0).double(), "origin": torch.tensor([[1, 2], [0, 3]], dtype=torch.int32)}


def _seq_inputs():
    gt = seeded((2, 1, 5, 9), 4660, -40.0, 0.0)
    i = {f"q{k}": -gt + seeded((2, 1, 5, 9), 4661 + k, -2.5, 2.5) for k in range(3)}
    i["gt"], i["valid"] = gt, (seeded((2, 1, 5, 9), 4665) > -0.6).float()
    return i


def _ir_inputs():
    return {"img_ir": seeded((2, 16, 20), 6040, 0.0, 1.0), "img": seeded((2, 16, 20), 6041, 0.0, 1.0)}


def _adam_inputs():
    return {"param": seeded((4, 3, 3, 5), 6050), "grad": seeded((4, 3, 3, 5), 6051)}


ADAM = dict(lr=1e-2, weight_decay=0.01)


def _adam_step(cls, **kw):
    def call(i):
        keep = i["param"].clone()   # (the step writes the parameter in place: the Parameter shares the input's memory)
        p = torch.nn.Parameter(i["param"])
        assert p.data_ptr() == i["param"].data_ptr() and p.stride() == i["param"].stride()
        try:
            opt = cls([p], **ADAM, **kw)
            p.grad = i["grad"]
            opt.step()
            st = opt.state[p]
            return p.detach().clone(), st["exp_avg"], st["exp_avg_sq"], st["step"]
        finally:
            with torch.no_grad():
                i["param"].copy_(keep)
    return call


def _no_grad(fn):
    def call(i):
        with torch.no_grad():
            return fn(i)
    return call


# (name, make() -> {input: CPU tensor}, call(inputs on the device) -> tensors, m of the reduction outputs or None, refusals)
REFUSAL = (RuntimeError, TypeError)
TABLE = [
    ("warp_scatter", lambda: {"img": seeded((2, 3, 9, 17), 5101), "disp": seeded((2, 1, 9, 17), 5102, -4.0, 4.0).round().to(torch.int32)},
     lambda i: ops.warp_scatter(i["img"], i["disp"], 1), None),
    ("local_contrast_norm", lambda: {"image": seeded((2, 1, 13, 21), 5103, 0.0, 1.0)}, lambda i: ops.local_contrast_norm(i["image"], 9), None),
    ("disp_metrics", _metrics_inputs,
     lambda i: ops.disp_metrics(i["disp_gt"], i["depth_gt"], i["disp_pred"], i["mask"], i["fb"]), 2 * 7 * 33),
    ("disp_metrics depth_pred", _metrics_inputs,
     lambda i: ops.disp_metrics(i["disp_gt"], i["depth_gt"], i["disp_pred"], i["mask"], depth_pred=i["depth_gt"] * 1.01), 2 * 7 * 33),
    ("obj_metrics", _obj_inputs,
     lambda i: ops.obj_metrics(i["disp_gt"], i["depth_gt"], i["disp_pred"], i["mask"], i["label"], 3, i["fb"]), 2 * 7 * 33),
    ("eval_mask", _eval_mask_inputs,
     lambda i: ops.eval_mask(i["disp_l"], i["depth_l"], 192, True, i["robot"], i["realsense"]), None),
    ("eval_mask float64 maps", _eval_mask_inputs,
     lambda i: ops.eval_mask(i["disp_l"], i["depth_l"], 192, False, i["robot"].double(), i["realsense"].double()), None),
    ("gt_from_right", _gt_inputs, lambda i: ops.gt_from_right(i["disp_r"], i["extra"], i["keep"], lo=0.0, hi=3.0), None),
    ("error_img disp", _maps, lambda i: ops.error_img(i["disp_pred"], i["disp_gt"], i["mask"]), None),
    ("error_img depth channels-last", _maps,
     lambda i: ops.error_img(i["depth_gt"] * 1.3, i["depth_gt"], i["mask"], kind="depth", channels_first=False), None),
    ("result_images", _result_inputs,
     lambda i: ops.result_images(i["pred"], i["gt_disp"], i["gt_depth"], i["mask"], i["fb"], 192, return_flags=True), None),
    ("depth_labels", _depth_inputs, lambda i: ops.depth_labels(i["l"], i["r"], i["focal"], 0.055), None),
    ("depth_labels window", _depth_inputs,
     lambda i: ops.depth_labels(i["l"], i["r"], i["focal"], 0.055, origin=i["origin"], window=(4, 6)), None),
    ("test_images float", lambda: {"src": seeded((2, 3, 6, 9), 6060), "second": seeded((1, 3, 6, 9), 6061)},
     lambda i: ops.test_images(i["src"], i["second"], size=(8, 12), pad=(1, 2)), None),
    ("test_images uint8", lambda: {"src": seeded((2, 6, 9), 6062, 0.0, 255.0).to(torch.uint8), "second": seeded((1, 6, 9), 6063, 0.0, 255.0).to(torch.uint8)},
     lambda i: ops.test_images(i["src"], i["second"], size=(8, 12), pad=(1, 2)), None),
    ("convex_upsample fp32 mask", lambda: {"flow": seeded((1, 2, 5, 7), 4650, -4.0, 4.0), "mask": rh.make_mask_logits((1, 144, 5, 7), 4651)},
     _no_grad(lambda i: ops.convex_upsample(i["flow"], i["mask"], 4)), None),
    ("convex_upsample fp16 mask", lambda: {"flow": seeded((1, 2, 5, 7), 4650, -4.0, 4.0), "mask": rh.make_mask_logits((1, 144, 5, 7), 4651).half()},
     _no_grad(lambda i: ops.convex_upsample(i["flow"], i["mask"], 4)), None),
    ("sequence_loss", _seq_inputs, _no_grad(lambda i: ops.sequence_loss([i["q0"], i["q1"], i["q2"]], i["gt"], i["valid"])), 2 * 5 * 9),
    ("get_ir_pattern", _ir_inputs, lambda i: du.get_ir_pattern(i["img_ir"], i["img"]), None),
    ("get_smoothed_ir_pattern", _ir_inputs, lambda i: du.get_smoothed_ir_pattern(i["img_ir"], i["img"], ks=5), None),
    ("get_smoothed_ir_pattern2", _ir_inputs, lambda i: du.get_smoothed_ir_pattern2(i["img_ir"], i["img"], ks=5), None),
    ("get_temporal_ir_pattern float", lambda: {"stack": seeded((2, 4, 16, 20), 6070, 0.0, 255.0).round()},
     lambda i: du.get_temporal_ir_pattern(i["stack"], ks=5), None),
    ("get_temporal_ir_pattern uint8", lambda: {"stack": seeded((2, 4, 16, 20), 6070, 0.0, 255.0).to(torch.uint8)},
     lambda i: du.get_temporal_ir_pattern(i["stack"], ks=5), None),
    ("augment_images float", lambda: {"grey": seeded((2, 12, 16), 6080, 0.0, 1.0), "sigma": seeded((2,), 6081, 0.5, 2.0)},
     lambda i: du.augment_images(i["grey"], i["sigma"], 1.1, 0.9, 1.0, kernel_size=5), None),
    ("augment_images uint8", lambda: {"grey": seeded((2, 12, 16), 6082, 0.0, 255.0).to(torch.uint8)},
     lambda i: du.augment_images(i["grey"], 1.0, 1.2, 0.85, 0.0, kernel_size=5), None),
    ("resize_bilinear", lambda: {"grey": seeded((2, 12, 18), 6090, 0.0, 255.0).to(torch.uint8)},
     lambda i: (du.resize_bilinear(i["grey"], (6, 9)), du.resize_bilinear(i["grey"], (6, 9), crop=(1, 2, 4, 5), dtype=torch.float32)), None),
    ("amax", lambda: {"t": seeded((2, 3, 5, 7, 32), 6100, -3.0, 3.0)}, lambda i: amax.absmax(i["t"]).max(), None),
    ("FusedAdam clipped", _adam_inputs, _adam_step(az_optim.FusedAdam, max_grad_norm=1.0), None),
    ("FusedAdamW", _adam_inputs, _adam_step(az_optim.FusedAdamW), None),
]
REFUSALS = {"FusedAdam clipped": REFUSAL + (ValueError,), "FusedAdamW": REFUSAL + (ValueError,)}


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _flat(o)]
    assert out is None, type(out)
    return []


def _same(name, config, got, want, m):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want), f"{name} [{config}]: {len(got)} results, {len(want)} on contiguous inputs"
    for j, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{name} [{config}]: result {j} is {tuple(a.shape)} {a.dtype}, not {tuple(b.shape)} {b.dtype}"
        a, b = a.contiguous(), b.contiguous()
        reduction = m is not None and (a.dtype == torch.float64 or (a.dim() == 0 and a.is_floating_point()))
        if not a.is_floating_point():
            assert torch.equal(a, b), f"{name} [{config}]: result {j} differs in {int((a != b).sum())} places"
        elif not reduction:
            ok = torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True)
            assert ok, f"{name} [{config}]: result {j} differs, max {float((a.double() - b.double()).abs().nan_to_num(float('inf')).max()):.3e}"
        else:
            a64, b64 = a.double(), b.double()
            rel = 2.0 * m * 2.0 ** -52 + (2.0 ** -23 if a.dtype != torch.float64 else 0.0)
            bound = rel * torch.maximum(a64.abs(), b64.abs())
            assert bool(((a64 - b64).abs() <= bound).all()) and torch.equal(a64.isnan(), b64.isnan()), (
                f"{name} [{config}]: reduction {j} differs by {float((a64 - b64).abs().max()):.3e}, bound {float(bound.max()):.3e}")


@pytest.mark.parametrize("entry", TABLE, ids=[e[0].replace(" ", "_") for e in TABLE])
def test_every_input_form_is_refused_or_gives_the_contiguous_result(entry, capsys):
    name, make, call, m = entry
    refusal = REFUSALS.get(name, REFUSAL)
    base = {k: v.to(DEV).contiguous().clone() for k, v in make().items()}
    want = call(base)
    again = call({k: v.clone() for k, v in base.items()})
    _same(name, "the same inputs again", again, want, m)
    plans = [({k: form}, f"{k}/{form}") for k in base for form in H.INPUT_FORMS]
    plans += [({k: "format" for k in base}, "all/format"), ({k: "offset1" for k in base}, "all/offset1")]
    accepted, refused = [], []
    for forms, config in plans:
        inputs, hit = dict(base), False
        for k, form in forms.items():
            t = H.input_form(base[k], form, DEV)
            if t is not None:
                inputs[k], hit = t, True
        if not hit:
            continue
        try:
            got = call(inputs)
        except refusal as e:
            if "HIP error" in str(e) or "illegal" in str(e):   # a device fault is no refusal
                raise
            refused.append(config)
            continue
        _same(name, config, got, want, m)
        accepted.append(config)
    with capsys.disabled():
        print(f"\n{name}: accepted {' '.join(accepted) or '-'}; refused {' '.join(refused) or '-'}", end="")
    assert accepted, f"{name}: every form was refused, the contiguous offset views included"
