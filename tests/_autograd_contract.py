"""The autograd contract of the hand-written `torch.autograd.Function` nodes: what a node owes the engine in every
configuration a caller can legally produce, not only the one the models happen to use (every input needs a gradient, every
output is used, the cotangent is a fresh contiguous tensor, backward runs once).

A node is described once (`Node`): how to build its inputs, the call through its public wrapper, which inputs are
differentiable, and the same operation as a plain differentiable torch composition (the oracle modules / torch.nn.functional),
which this module evaluates on the CPU in fp64 and in fp32.  These checks run on that description:

    check_flags     all inputs / each input alone / all but each one require a gradient          (positional bookkeeping,
                    inputs that do not are created with requires_grad=False)                       NULL kernel outputs)
    check_unused    a loss that reads each single output alone, then all of them                  (None cotangents)
    check_forms     the same cotangent values as a fresh tensor, with a stride-0 dimension,       (strides and storage
                    in the other memory format, and as a view at a storage offset of 4k floats     offsets of grad_output)
    check_replay    autograd.grad(retain_graph=True) twice, .backward() twice into .grad,         (state that outlives one
                    then the node's module-level state must be clean                               backward pass)
    check_pruned_then_full   one backward over a pruned graph, then a full one over the same graph and over a new one
    check_input_forms   the same INPUT values in the other memory format, with the last two dimensions swapped      (strides, storage
                    in memory, as a slice of a larger NaN-filled buffer, and as contiguous views at storage         offsets and alignment
                    offsets 12 and 1: each input alone in each form, then all in `format`, all in `offset1`         of the inputs)

Comparison rules (none is fitted to what the code under test returns):

  * a gradient that ONE launch produces and that a reference module has an element-wise error model for is held to that
    model, fed with this harness' inputs and cotangents (Node.elementwise): cost_volume, softargmin, warp_gather,
    patch_reprojection, disp_loss, sequence_loss, spp_concat, costconv._Merge / _Assemble, gru._Conv3x3Bf16;
  * every other gradient (compositions of launches, plain torch sums) against fp64, per tensor (test_gpu_psmnet.py,
    G13): ||got - g64|| <= max(3 e_ref, 2e-4) ||g64|| with
    e_ref = ||g32 - g64|| / ||g64||, g32 / g64 the CPU fp32 / fp64 evaluations of the reference on the same inputs;
  * across configurations of one node, gradients of kernels without float atomics are equal as values (torch.equal);
    the ones named in `Node.atomic` are flushed with float atomics and are held to the fp64 rule in every configuration;
  * a gradient that was asked for is a tensor of its input's shape wherever the reference's is not identically zero (None is
    the engine's zero).  What a node hands into a slot whose flag is off is dropped by the engine before anyone can see it;
    a node that misplaces a gradient is caught by the slot that was asked for and comes back None, wrong or misshapen.

`device` is the switch between the GPU nodes (tests/test_gpu_autograd_contract.py) and the pure-torch mutants that prove on
the CPU that each check can fail (tests/test_autograd_contract_cpu.py).

Determinism class and nullable kernel outputs per node.  "atomic": the gradient is flushed with float atomics (or summed in an order the engine chooses) and is held to the fp64 rule only; every other
gradient must be equal as values across configurations.  "NULL": kernel pointers that are NULL in some flag subset or call
form, with the place that passes them and the guard in the kernel.

  conv_bn (conv3d._ConvBN), fork net
      atomic  weight: every az_conv3d_wgrad*.hip tile flush, az_wgrad_common.h:111.  x, gamma, beta, residual: none (az_bn3d.hip
              reduces through its workspace; the input-gradient kernels have no atomics; handover.GradSlot sums with az_sum4).
      NULL    az_bn3d_bwd dz_out (no residual or no ReLU, conv3d.py:540; guarded az_bn3d.hip:360,459), dx_amax (not f16x3,
              conv3d.py:546; az_bn3d.hip:472,659), y / scale / shift by the ReLU form (conv3d.py:552; az_bn3d.hip:650-651);
              az_bn3d_apply residual / y_amax.  No flag subset changes a pointer: needs_input_grad skips the two launches
              (conv3d.py:563,566) and picks the layout of d(raw) (_presplit_ok, conv3d.py:548).
  _convbn_unit = conv2d._ConvSame / _ConvS2Vol / _ConvS2Patches + bn2d._BNAct
      atomic  weight: az_conv2d_wgrad.hip:191 and the 3-D weight gradient of the stride-2 route.  Others: none.
      NULL    az_bn2d_bwd dz, y, scale, shift by the ReLU / residual form (bn2d.py:109,117-118; az_bn3d.hip bn2d_bwd_launch);
              az_bn2d_fwd partials (bn2d.py:79).  Flag subsets only skip launches (conv2d.py:316,319,373,376,422,428).
  conv_logits (conv3d._ConvLogits)
      atomic  weight: az_conv3d_c1.hip:318-321.  x, addend: none.
      NULL    az_conv3d_c1_fwd addend / scale / shift, az_conv3d_c1_wgrad scale / shift (conv3d.py:623,645; guarded
              az_conv3d_c1.hip:72,147,247,334,357).  Flag subsets skip launches (conv3d.py:635,639).
  add, fanout (conv3d._AddRelu, _FanOut)
      atomic  none.   NULL  az_sum4 c, d for fewer than four parts (handover.py:53; az_bn3d.hip:550-551,681).
  cost_volume, cost_volume_ndhwc: atomic none, NULL none (ops.py:83-86 always writes both gradients).
  softargmin: atomic logits (az_softargmin.hip:306).  NULL: az_softargmin_fwd stats when logits needs no gradient
              (ops.py:116; az_softargmin.hip:180) -- backward never runs then.
  warp_gather, torch.ops.azhip.warp_gather: atomic img (az_warp_gather.hip:100-103).  NULL: grad_img when img needs no
              gradient (ops.py:165, torch_ops.py:160; guarded az_warp_gather.hip:90,99).
  disp_loss, sequence_loss, patch_reprojection: atomic none -- backward is element-wise and divides by the forward's
              COUNT (az_disp_loss.hip:51, az_patch_reproj.hip:75,184), an integer accumulated in double, exact in any order.
              NULL: the mask (ops.py:185,198,270,286), by the call's form.
  convex_upsample (fp32 and fp16 mask): atomic none (az_convex_up.hip reduces through its workspace).  NULL none.
  spp_concat (_SppConcat): atomic none (az_spp.hip:10,72).  NULL none: an input that needs no gradient skips its launch
              (psmnet_submodule_3.py:184).
  costvol_conv (costconv._Merge, _Assemble): atomic weight (the 2-D weight gradients under it); NULL none.
  torch.ops.azhip.conv3d: as conv_bn's two convolution launches (torch_ops.py:262-263).
  CorrBlock1D (corr._Volume, _Pool, _Lookup): atomic f1, f2 -- the lookups of one pass add into one buffer per level in the
              order the engine runs them (az_corr1d.hip:343-356).  NULL: az_corr1d_volume_bwd grad_f1 / grad_f2
              (corr.py:48-49; guarded az_corr1d.hip:274,283); a level that needs no gradient skips its launch (corr.py:139).

  ConvGRU (gru._GRUStepBf16 in both operand formats, gru._Conv3x3Bf16 through the operator form): atomic wz, wr, wq
              (az_conv2d_wgrad.hip:191).  NULL none: needs_input_grad skips launches and slices (gru.py:316-345).
              Every gradient of the step -- all thirteen-plus slots -- against Node.vjp: forward and backward of the step
              chained in fp64 from split_reference (fwd / dgrad / wgrad with the operand rounding and the f16 amax
              scaling), gru_rh, gru_bwd1..3 of tests/_gru_fp64ref.py, per tensor with e_ref = 0.
  gru._Conv3x3Bf16 (called directly): atomic w (az_conv2d_wgrad.hip:191); NULL: the bias (gru.py:195).  x and w gradients
              are one launch each: held to tests/_gru_fp64ref.py's model (operand rounding in split_reference).
  costconv._Merge, _Assemble (called directly): atomic none (az_costconv.hip); NULL none.

The token slot of _ConvS2Patches (conv2d.py:393,433) runs with an armed overlap.Sink in
test_first_layer_token_and_the_sink_is_closed, which also asserts that the sink is joined and empty after backward.
"""
import torch

from tests._weights import seeded

RULE_FLOOR = 2e-4   # test_gpu_psmnet.py:317
RULE_FACTOR = 3.0


class Node:
    """name; make(device) -> {input name: fp32 tensor without grad}; call(inputs) -> output or tuple of outputs, through the
    public wrapper; diff: names of the differentiable inputs; ref(inputs) -> the same outputs from plain torch ops, for inputs
    of any dtype on the CPU (same layouts as `call`); atomic: names whose gradient a float-atomic flush produces;
    dirty(outputs) -> list of complaints about module-level state after a backward pass; images: outputs are 4-D / 5-D
    images, so the other memory format is a legal cotangent.
    elementwise(inputs, cotangents, got, key) -> {name: error / bound}: the node is one launch per gradient and a reference
    module holds its element-wise error model -- `inputs` the CPU fp32 inputs, `cotangents` {output index: CPU fp32 values},
    `got` {name: numpy gradient}, `key` names the (used outputs, cotangent kind) for the hook's own cache; the gradients it
    returns a ratio for are held to that bound INSTEAD of the per-tensor rule.
    half: names of inputs (and so gradients) that are fp16 tensors: the fp64 and fp32 references are rounded to fp16, so
    that the format's rounding is in the reference, not in the tolerance.
    vjp(inputs, cotangents) -> {name: fp64 gradient}: a node that is SPECIFIED to round its operands (the ConvGRU's one-part
    fp16 / bf16 convolutions) cannot be compared with the autograd of its unrounded formula; `vjp` is its chained fp64
    reference with that rounding IN the reference (tests/_gru_fp64ref.py's pieces).  It stands for both evaluations, so
    e_ref = 0 and the per-tensor rule is its floor, 2e-4.
    refuses: {input name: forms} -- the wrapper REFUSES that input in those memory forms (a `_chk` without `.contiguous()`):
    check_input_forms then asks for a RuntimeError, and a refusal is a pass.  "*" names every tensor input.
    unaligned: the documented route that the node takes for a pointer that is not 16-byte aligned (a sentence naming the
    switch in the kernel); it may change a summation order, so the two `offset1` arrangements -- and no other form -- are
    held to the fp64 rule instead of equality."""

    def __init__(self, name, make, call, diff, ref, atomic=(), dirty=None, images=True, elementwise=None, half=(), vjp=None,
                 refuses=None, unaligned=None):
        self.name, self.make, self.call, self.diff, self.ref = name, make, call, tuple(diff), ref
        self.atomic, self.dirty, self.images = frozenset(atomic), dirty, images
        self.elementwise, self.half, self.vjp = elementwise, frozenset(half), vjp
        self.refuses, self.unaligned = {k: frozenset(v) for k, v in (refuses or {}).items()}, unaligned
        self._ref = {}

    def __repr__(self):
        return self.name


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def leaves(node, device, need):
    """fresh inputs; the differentiable ones are leaves whose requires_grad is set at creation, never detached afterwards"""
    inp = node.make(device)
    for k in node.diff:
        inp[k] = inp[k].clone().requires_grad_(k in need)
    return inp


# ---- cotangents -----------------------------------------------------------------------------------------------------------
def cot_values(shape, k, kind="random"):
    """the cotangent VALUES of output k (CPU fp32).  "rows": constant along the last dimension, so that a stride-0 view can
    carry them; "scalar": one value everywhere, what `.sum().backward()` delivers."""
    shape = tuple(shape)
    if kind == "scalar" or not shape:
        return torch.full(shape, 0.75 - 0.25 * k)
    if kind == "rows":
        return seeded(shape[:-1] + (1,), 9100 + k).expand(shape).contiguous()
    return seeded(shape, 9000 + k)


FORMS = ("fresh", "stride0", "format", "offset")


def cot_form(values, form, device, kind):
    """the same values in one of the four memory forms; None where the form does not apply"""
    v = values.to(device)
    if form == "fresh" or v.dim() == 0:
        return v.clone() if form == "fresh" else None
    if form == "stride0":
        if kind == "scalar":
            return v.flatten()[0].clone().expand(v.shape)
        if kind == "rows":
            return v[..., :1].clone().expand(v.shape)
        return None
    if form == "format":
        if v.dim() not in (4, 5):
            return None
        if v.dim() == 4:  # [N,C,H,W]: the fresh one is NCHW-contiguous, this one channels_last
            return v.contiguous(memory_format=torch.channels_last)
        # [B,D,H,W,C] volumes are channels-last by shape: the other format is the memory of a contiguous [B,C,D,H,W]
        return v.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1)
    if form == "offset":
        buf = torch.full((v.numel() + 24,), float("nan"), device=device)
        buf[12:12 + v.numel()] = v.reshape(-1)
        t = buf[12:12 + v.numel()].view(v.shape)
        assert t.storage_offset() == 12
        return t
    raise ValueError(form)


# ---- the fp64 reference and the per-tensor rule -----------------------------------------------------------------------------
def reference(node, use=None, kind="random"):
    """({name: g64}, {name: g32}) of sum_k <ref output k, cotangent k> over the used outputs, every differentiable input
    requiring a gradient; computed once per (used outputs, cotangent kind) and shared"""
    key = (tuple(use) if use is not None else None, kind)
    if key not in node._ref and node.vjp is not None:
        inp = node.make("cpu")
        with torch.no_grad():
            outs = _tuple(node.ref(inp))
            idx = range(len(outs)) if use is None else use
            g = {k: v.double() for k, v in node.vjp(inp, {j: cot_values(outs[j].shape, j, kind) for j in idx}).items()}
        assert set(g) == set(node.diff)
        node._ref[key] = (g, g)
    if key not in node._ref:
        res = []
        for dt in (torch.float64, torch.float32):
            inp = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in node.make("cpu").items()}
            for k in node.diff:
                inp[k] = inp[k].clone().requires_grad_()
            outs = _tuple(node.ref(inp))
            idx = range(len(outs)) if use is None else use
            loss = sum((outs[k] * cot_values(outs[k].shape, k, kind).to(dt)).sum() for k in idx)
            gs = torch.autograd.grad(loss, [inp[k] for k in node.diff], allow_unused=True)
            gd = {k: (g if g is not None else torch.zeros_like(inp[k])) for k, g in zip(node.diff, gs)}
            res.append({k: (g.half() if k in node.half else g).double() for k, g in gd.items()})
        node._ref[key] = tuple(res)
    return node._ref[key]


def ratio(got, g64, g32):
    """(error / bound) of the per-tensor rule; <= 1 passes"""
    n64 = float(g64.norm())
    e_ref = float((g32 - g64).norm())
    bound = max(RULE_FACTOR * e_ref, RULE_FLOOR * n64)
    err = float((got.detach().double().cpu() - g64).norm())
    if bound == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / bound


class Report:
    """worst error/bound ratio per node and check (the first word of the configuration: needs / uses / cotangent / replay /
    pruned / full), with the configuration and the tensor it came from; printed in the project's record(...) style"""

    def __init__(self):
        self.worst, self.notes = {}, []

    def note(self, node, text):
        self.notes.append((str(node), text))

    def add(self, node, config, name, r):
        key = (str(node), config.split()[0].rstrip(":"))
        if r >= self.worst.get(key, (-1.0, ""))[0]:
            self.worst[key] = (r, f"d/d{name}, {config}")

    def lines(self, node=None):
        """the table, or the rows of one node"""
        return ([f"{n} [{c}]: worst error/bound {r:.4f} ({where})" for (n, c), (r, where) in self.worst.items()
                 if node is None or n == str(node)]
                + [f"{n} [{text}]" for n, text in self.notes if node is None or n == str(node)])


def check_fp64(node, grads, need, use, kind, report, config):
    g64, g32 = reference(node, use, kind)
    element = {}
    if node.elementwise is not None:
        inp = node.make("cpu")
        outs = _tuple(node.ref(inp))
        idx = range(len(outs)) if use is None else use
        cots = {j: cot_values(outs[j].shape, j, kind) for j in idx}
        got = {k: grads[k].detach().cpu().numpy() for k in need if grads[k] is not None}
        element = {k: r for k, r in node.elementwise(inp, cots, got, (tuple(idx), kind)).items() if k in got}
    for k in node.diff:
        g = grads[k]
        if k not in need:
            continue
        if g is None and not bool(g64[k].any()):
            continue  # no used output depends on this input: None is the engine's zero
        assert g is not None, f"{node} [{config}]: no gradient for {k}"
        assert tuple(g.shape) == tuple(g64[k].shape), f"{node} [{config}]: gradient of {k} has shape {tuple(g.shape)}"
        if k in element:
            continue
        r = ratio(g, g64[k], g32[k])
        report.add(node, config, k, r)
        assert r <= 1.0, f"{node} [{config}]: d/d{k} misses the fp64 rule, error/bound {r:.3f}"
    for k, r in element.items():
        report.add(node, config, k + " (element-wise)", r)
        assert r <= 1.0, f"{node} [{config}]: d/d{k} misses its element-wise bound, error/bound {r:.3f}"


def same(node, a, b, need, what):
    """across configurations: equal as values, except the float-atomic gradients (held to fp64 by the caller)"""
    for k in need:
        if k in node.atomic:
            continue
        assert a[k] is not None and b[k] is not None, f"{node} [{what}]: no gradient for {k}"
        assert torch.equal(a[k], b[k]), (f"{node} [{what}]: d/d{k} differs between two configurations, max "
                                         f"{float((a[k] - b[k]).abs().max()):.3e}")


# ---- one backward pass ----------------------------------------------------------------------------------------------------
def run(node, device, need=None, use=None, form="fresh", kind="random"):
    """gradients {name: tensor or None} of the inputs in `need` for a loss over the outputs in `use`"""
    need = node.diff if need is None else tuple(need)
    inp = leaves(node, device, need)
    outs = _tuple(node.call(inp))
    idx = list(range(len(outs))) if use is None else list(use)
    idx = [k for k in idx if outs[k].requires_grad]  # (an output that is an input without a gradient: nothing to ask)
    cots = [cot_form(cot_values(outs[k].shape, k, kind), form, device, kind) for k in idx]
    if any(c is None for c in cots):
        return None
    gs = torch.autograd.grad([outs[k] for k in idx], [inp[k] for k in need], cots, allow_unused=True)
    grads = {k: None for k in node.diff}
    grads.update(zip(need, gs))
    return grads


def flag_subsets(diff):
    out = [tuple(diff)]
    if len(diff) > 1:
        out += [(k,) for k in diff]
    if len(diff) > 2:
        out += [tuple(j for j in diff if j != k) for k in diff]
    return out


def check_flags(node, device, report):
    full = None
    for need in flag_subsets(node.diff):
        config = "needs " + ",".join(need)
        grads = run(node, device, need)
        check_fp64(node, grads, need, None, "random", report, config)
        if full is None:
            full = grads
        else:
            same(node, grads, full, need, config + " vs all")


def check_unused(node, device, report, n_out):
    """a loss that reads each single output alone, then all of them"""
    for use in [(k,) for k in range(n_out)] + [tuple(range(n_out))]:
        config = "uses " + ",".join(map(str, use))
        grads = run(node, device, None, use)
        check_fp64(node, grads, node.diff, use, "random", report, config)


def check_forms(node, device, report):
    """the four memory forms of one cotangent: values constant along the last dimension (every form can carry them, and
    no gradient degenerates), then one value everywhere (what .sum().backward() produces; a constant cotangent makes a
    train-mode BatchNorm gradient pure cancellation, so only the equality across forms is asked of it)"""
    for kind in ("rows", "scalar"):
        first = None
        for form in FORMS:
            if form == "format" and not node.images:
                continue
            grads = run(node, device, None, None, form, kind)
            if grads is None:
                continue
            config = f"cotangent {kind}/{form}"
            if kind == "rows":
                check_fp64(node, grads, node.diff, None, kind, report, config)
            if first is None:
                first = grads
            else:
                same(node, grads, first, node.diff, config + " vs fresh")


def check_replay(node, device, report):
    inp = leaves(node, device, node.diff)
    outs = _tuple(node.call(inp))
    cots = [cot_form(cot_values(o.shape, k), "fresh", device, "random") for k, o in enumerate(outs)]
    xs = [inp[k] for k in node.diff]
    g1 = dict(zip(node.diff, torch.autograd.grad(outs, xs, cots, retain_graph=True, allow_unused=True)))
    g2 = dict(zip(node.diff, torch.autograd.grad(outs, xs, cots, retain_graph=True, allow_unused=True)))
    check_fp64(node, g1, node.diff, None, "random", report, "replay: first grad()")
    check_fp64(node, g2, node.diff, None, "random", report, "replay: second grad()")
    same(node, g2, g1, node.diff, "replay: second grad() vs first")
    torch.autograd.backward(outs, cots, retain_graph=True)
    torch.autograd.backward(outs, cots)
    acc = {k: inp[k].grad for k in node.diff}
    for k in node.diff:
        assert acc[k] is not None, f"{node}: .grad of {k} is None after two backward passes"
    same(node, acc, {k: g1[k] + g1[k] for k in node.diff}, node.diff, "replay: .grad after two backward() vs twice the first")
    check_fp64(node, {k: acc[k] * 0.5 for k in node.diff}, node.diff, None, "random", report, "replay: .grad / 2")
    complaints = node.dirty(outs) if node.dirty is not None else []
    assert not complaints, f"{node}: state left behind by backward: {complaints}"


def check_pruned_then_full(node, device, report, first_use):
    """one backward pass that reads only `first_use` of the outputs (the engine prunes the rest), then a full pass over the
    SAME retained graph and one over a new graph: what the first pass left behind must not reach the others"""
    inp = leaves(node, device, node.diff)
    outs = _tuple(node.call(inp))
    xs = [inp[k] for k in node.diff]
    cots = [cot_form(cot_values(o.shape, k), "fresh", device, "random") for k, o in enumerate(outs)]
    gs = torch.autograd.grad([outs[k] for k in first_use], xs, [cots[k] for k in first_use], retain_graph=True, allow_unused=True)
    check_fp64(node, dict(zip(node.diff, gs)), node.diff, tuple(first_use), "random", report, "pruned pass")
    complaints = node.dirty(outs) if node.dirty is not None else []
    assert not complaints, f"{node}: state left behind by a pruned backward: {complaints}"
    gs = torch.autograd.grad(outs, xs, cots, allow_unused=True)
    check_fp64(node, dict(zip(node.diff, gs)), node.diff, None, "random", report, "full pass over the graph of a pruned one")
    complaints = node.dirty(outs) if node.dirty is not None else []
    assert not complaints, f"{node}: state left behind by the full pass after a pruned one: {complaints}"
    check_fp64(node, run(node, device), node.diff, None, "random", report, "full pass over a new graph after a pruned one")


# ---- the memory forms of the inputs ---------------------------------------------------------------------------------------
INPUT_FORMS = ("format", "transposed", "slice", "offset12", "offset1")
NOT_DENSE = ("format", "transposed", "slice")   # the forms that `is_contiguous()` can tell from a fresh tensor


def _filler(t):
    """what surrounds the values in a larger buffer: NaN, or the largest value of a format that has none"""
    return float("nan") if t.is_floating_point() else (True if t.dtype == torch.bool else torch.iinfo(t.dtype).max)


def input_form(values, form, device):
    """the same values, in the same logical shape, in one of the five memory forms; None where the form does not apply
    to the rank.  `values` is what Node.make returned for the input: contiguous or, for a 4-D image, channels_last."""
    v = values.to(device)
    if v.dim() == 0:
        return None
    if form == "format":
        if v.dim() == 4:  # the OTHER format: channels_last for an NCHW-contiguous image, NCHW for a channels_last one
            t = v.contiguous(memory_format=torch.channels_last) if v.is_contiguous() else v.contiguous()
            return t.clone(memory_format=torch.preserve_format)
        if v.dim() == 5:  # (as cot_form: the memory of a contiguous [B,C,D,H,W] viewed back)
            return v.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1)
        return None
    if form == "transposed":
        return v.transpose(-1, -2).contiguous().transpose(-1, -2) if v.dim() >= 2 else None
    if form == "slice":
        if v.dim() == 1:  # every other element of a buffer twice as long
            buf = torch.full((2 * v.numel() + 1,), _filler(v), dtype=v.dtype, device=device)
            t = buf[1::2]
        else:
            pad = [0] * v.dim()
            pad[1] += 2
            pad[-1] += 3
            buf = torch.full([n + p for n, p in zip(v.shape, pad)], _filler(v), dtype=v.dtype, device=device)
            idx = [slice(None)] * v.dim()
            idx[1], idx[-1] = slice(1, 1 + v.shape[1]), slice(2, 2 + v.shape[-1])   # (a matrix: one dimension is both)
            t = buf[tuple(idx)]
        t.copy_(v)
        assert t.shape == v.shape and (not t.is_contiguous() or v.numel() <= 1)
        return t
    if form in ("offset12", "offset1"):  # one element: 4 bytes past 16-byte alignment for fp32, 2 for fp16, 1 for bytes
        off, n = int(form[6:]), v.numel()
        dense = 1 + sum((sz - 1) * st for sz, st in zip(v.shape, v.stride())) == n or n == 0
        assert dense, "Node.make returns dense tensors"
        buf = torch.full((n + 2 * off + 12,), _filler(v), dtype=v.dtype, device=device)
        t = buf[off:off + n].as_strided(v.shape, v.stride())  # (the strides of the fresh input: its own layout, moved)
        t.copy_(v)
        assert t.storage_offset() == off and t.is_contiguous() == v.is_contiguous()
        return t
    raise ValueError(form)


def run_inputs(node, device, forms):
    """(outputs, gradients) with the inputs named in `forms` {name: form} in that memory form and every other one fresh;
    every differentiable input requires a gradient, the cotangents are fresh.  None where no named form applies."""
    inp = node.make(device)
    hit = False
    for k, form in forms.items():
        if not isinstance(inp.get(k), torch.Tensor):
            continue
        t = input_form(inp[k], form, device)
        if t is not None:
            inp[k], hit = t, True
    if forms and not hit:
        return None
    for k in node.diff:
        inp[k] = (inp[k] if k in forms else inp[k].clone(memory_format=torch.preserve_format)).requires_grad_()
        assert inp[k].is_leaf
    outs = _tuple(node.call(inp))
    idx = [k for k in range(len(outs)) if outs[k].requires_grad]
    if not node.diff:   # (a plain function, no autograd node: outputs only)
        return tuple(outs), {}
    cots = [cot_form(cot_values(outs[k].shape, k), "fresh", device, "random") for k in idx]
    gs = torch.autograd.grad([outs[k] for k in idx], [inp[k] for k in node.diff], cots, allow_unused=True)
    for k, g in zip(node.diff, gs):
        assert g is None or g.shape == inp[k].shape, f"{node}: gradient of {k} has shape {tuple(g.shape)}, its input {tuple(inp[k].shape)}"
    return tuple(outs), dict(zip(node.diff, gs))   # (the outputs still attached: Node.dirty walks their graph)


def out_reference(node):
    """the outputs of the reference on the CPU in fp64 and fp32 (for the `unaligned` routes, whose outputs may differ)"""
    if "outs" not in node._ref:
        res = []
        for dt in (torch.float64, torch.float32):
            with torch.no_grad():
                inp = {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in node.make("cpu").items()}
                res.append([o.double() for o in _tuple(node.ref(inp))])
        node._ref["outs"] = tuple(res)
    return node._ref["outs"]


def _tensor_inputs(node, device):
    return [k for k, v in node.make(device).items() if isinstance(v, torch.Tensor)]


def _refused(node, forms, device):
    """the inputs of this arrangement that the node declares it refuses -- where the form applies to the input's rank and
    its strides differ from the fresh input's (channels_last of one channel is the fresh tensor: nothing to refuse)"""
    probe, out = node.make(device), []
    for k, form in forms.items():
        if form in node.refuses.get(k, node.refuses.get("*", ())) and isinstance(probe.get(k), torch.Tensor):
            t = input_form(probe[k], form, device)
            if t is not None and (t.stride() != probe[k].stride() or t.storage_offset() != probe[k].storage_offset()):
                out.append(k)
    return out


def _device_fault(e):
    """a HIP error surfaces as a RuntimeError too"""
    return any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access"))


def check_input_forms(node, device, report):
    """each input alone in each memory form that applies to its rank, all inputs in `format`, all inputs in `offset1`,
    against the run on fresh inputs: every output and every gradient has the fresh one's logical shape (a gradient its
    input's) and, read logically, the fresh one's values -- torch.equal, except the float-atomic gradients (fp64 rule or
    element-wise model, as everywhere) and, for a node with a documented `unaligned` route, the two `offset1` arrangements
    (fp64 rule, outputs included).  A form that the node declares in `refuses` must raise RuntimeError; any other
    exception, and any undeclared one, fails.

    Measured on an MI355X (tests/test_gpu_autograd_contract.py and tests/test_gpu_torch_ops.py print the table): every output
    and every non-atomic gradient of every node equal in every accepted arrangement; no node needed `unaligned`.  Worst
    error / bound of the atomic gradients over all arrangements: 3-D weight gradients (conv_bn, azhip.conv3d, fork net,
    costvol_conv, conv_logits) 0.0004 .. 0.0021; 2-D weight gradients (convbn_unit, BasicBlock) 0.0006 .. 0.0015; softargmin
    and azhip.softargmin d/dlogits 0.0096 and warp_gather / azhip.warp_gather d/dimg 0.539 of their element-wise bounds;
    ConvGRU d/dwr 0.170 (f16x1) and 0.926 (bf16, bf16_ops), gru._Conv3x3Bf16 d/dw 0.196 -- the figures of the fresh run, the
    operand rounding dominates; CorrBlock1D d/df1 0.0068.  Refused, per node: Node.refuses in the two test files."""
    fresh = run_inputs(node, device, {})
    assert fresh is not None
    f_outs, f_grads = tuple(o.detach() for o in fresh[0]), fresh[1]
    names = _tensor_inputs(node, device)
    plans = [({k: form}, f"input {k}/{form}") for k in names for form in INPUT_FORMS]
    plans += [({k: "format" for k in names}, "input all/format"), ({k: "offset1" for k in names}, "input all/offset1")]
    atomic = tuple(k for k in node.diff if k in node.atomic)
    for forms, config in plans:
        refused = _refused(node, forms, device)
        if refused:
            try:
                run_inputs(node, device, forms)
            except RuntimeError as e:   # the wrapper's or the library's refusal -- a device fault is none
                assert not _device_fault(e), f"{node} [{config}]: a device fault where a refusal is declared: {e}"
            else:
                raise AssertionError(f"{node} [{config}]: DID NOT RAISE the RuntimeError it declares for {','.join(refused)}")
            report.note(node, f"{config}: refused ({','.join(refused)})")
            continue
        try:
            got = run_inputs(node, device, forms)
        except (RuntimeError, TypeError, ValueError) as e:
            if _device_fault(e):
                raise
            raise AssertionError(f"{node} [{config}]: raised {type(e).__name__} for a form it does not declare as refused: {e}") from e
        if got is None:
            continue
        outs, grads = got
        complaints = node.dirty(outs) if node.dirty is not None else []
        assert not complaints, f"{node} [{config}]: state left behind by backward: {complaints}"
        outs = tuple(o.detach() for o in outs)
        loose = node.unaligned is not None and config.endswith("/offset1")
        assert len(outs) == len(f_outs)
        for j, (o, f) in enumerate(zip(outs, f_outs)):
            assert o.shape == f.shape, f"{node} [{config}]: output {j} has shape {tuple(o.shape)}, fresh {tuple(f.shape)}"
            if loose:
                o64, o32 = out_reference(node)
                r = ratio(o, o64[j], o32[j])
                report.add(node, config, f"output {j}", r)
                assert r <= 1.0, f"{node} [{config}]: output {j} misses the fp64 rule, error/bound {r:.3f}"
            else:
                assert torch.equal(o.contiguous(), f.contiguous()), (
                    f"{node} [{config}]: output {j} differs from the fresh run, max {float((o - f).abs().max()):.3e}")
        for k in node.diff:
            g, f = grads[k], f_grads[k]
            assert (g is None) == (f is None), f"{node} [{config}]: gradient of {k} is {'None' if g is None else 'a tensor'}"
            if g is None:
                continue
            assert g.shape == f.shape, f"{node} [{config}]: gradient of {k} has shape {tuple(g.shape)}, fresh {tuple(f.shape)}"
            if k not in node.atomic and not loose:
                assert torch.equal(g.contiguous(), f.contiguous()), (
                    f"{node} [{config}]: d/d{k} differs from the fresh run, max {float((g - f).abs().max()):.3e}")
        held = node.diff if loose else atomic
        if held:
            check_fp64(node, grads, held, None, "random", report, config)
        else:
            report.add(node, config, "all (equal)", 0.0)


# ---- module-level state ---------------------------------------------------------------------------------------------------
def graph_nodes(outs):
    seen, stack = set(), [o.grad_fn for o in _tuple(outs) if o.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack.extend(f for f, _ in fn.next_functions)
    return seen


def slot_complaints(outs):
    """every handover.GradSlot reachable from the graph is as forward left it: left == expect, nothing parked"""
    out = []
    for fn in graph_nodes(outs):
        for attr in ("az_out_slot", "x_slot", "res_slot"):
            s = getattr(fn, attr, None)
            if s is not None and (s.left != s.expect or s.parts):
                out.append(f"{type(fn).__name__}.{attr}: left {s.left} expect {s.expect} parked {len(s.parts)}")
    return out
