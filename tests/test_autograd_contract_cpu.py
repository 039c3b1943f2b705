"""Proof on the CPU that the autograd-contract harness (tests/_autograd_contract.py) can fail: pure-torch mutants of a
two-input, two-output toy node, each wrong in one of the ways a hand-written autograd node can be wrong, each rejected by the
check named for it -- and the correct node passes every check."""
import pytest
import torch

from tests import _autograd_contract as H
from tests._weights import seeded

DEV = "cpu"
STATE = {"acc": None, "parked": []}   # the module-level state the stateful mutants keep


class _Toy(torch.autograd.Function):
    """y1 = a * g, y2 = a + g with a [2,3,4,8] and a per-channel g [8] (the shape of a BatchNorm gamma)"""

    @staticmethod
    def forward(ctx, a, g, flavour):
        ctx.flavour, ctx.runs = flavour, 0
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(a, g)
        if flavour == "input_read_linearly":   # hands the kernel the pointer of an input whose strides it never looked at
            a = torch.as_strided(a, a.shape, torch.empty(a.shape).stride())
        return a * g, a + g

    @staticmethod
    def backward(ctx, g1, g2):
        a_saved, g_saved = ctx.saved_tensors
        a, g = a_saved.contiguous(), g_saved.contiguous()   # (what the kernel reads)
        fl = ctx.flavour
        need_a, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        pruned = g2 is None
        if fl == "none_as_ones":
            g1 = torch.ones_like(a) if g1 is None else g1
            g2 = torch.ones_like(a) if g2 is None else g2
        if fl == "stride0_first":   # reads grad_output through its pointer as if it were dense
            g1, g2 = (torch.full_like(t, float(t.flatten()[0])) if (t is not None and 0 in t.stride()) else t for t in (g1, g2))
        if fl == "offset_ignored":  # reads the storage from its start
            g1, g2 = (torch.as_strided(t, t.shape, t.stride(), 0) if t is not None else t for t in (g1, g2))
        # (.contiguous() as the real nodes do: torch's own reductions order their sums by the strides)
        g1 = torch.zeros_like(a) if g1 is None else g1.contiguous()
        g2 = torch.zeros_like(a) if g2 is None else g2.contiguous()
        da = g1 * g + g2
        dg = (g1 * a + g2).sum(dim=(0, 1, 2))
        if fl == "unaligned_route" and a.data_ptr() % 16:   # a documented other route for a pointer off 16 bytes:
            dg = (g1 * a + g2).double().sum(dim=(0, 1, 2)).float()  # the same sum, accumulated otherwise
        if fl == "dgamma_zeroed":
            dg = torch.where(g != 0, dg, torch.zeros_like(dg))
        if fl == "acc_never_cleared":
            STATE["acc"] = da if STATE["acc"] is None else STATE["acc"] + da
            da = STATE["acc"]
        if fl == "acc_released":
            ctx.runs += 1
            if ctx.runs > 1:
                da, dg = torch.zeros_like(da), torch.zeros_like(dg)
        if fl == "dirty_after_pruned":
            if pruned:
                STATE["parked"].append(da)       # waits for a sibling that the engine pruned
            elif STATE["parked"]:
                da = da + sum(STATE["parked"])   # ... and reaches the next pass
                STATE["parked"] = []
        if fl == "grad_like_saved":   # torch_ops._warp_gather_bwd before its fix: the gradient is allocated *_like the CALLER'S
            out = torch.empty_like(a_saved)   # tensor (a dense permuted one keeps its strides) and written linearly
            out.as_strided((out.numel(),), (1,)).copy_(da.reshape(-1))
            da = out
        if fl == "grad_transposed" and not a_saved.is_contiguous() and a_saved.transpose(-1, -2).is_contiguous():
            da = da.transpose(-1, -2)     # "fixes" a transposed input by working on its transpose, and hands that back
        if fl == "swapped" and not (need_a and need_g):
            return (dg if need_g else None), (da if need_a else None), None
        if fl == "neighbour_flag":  # needs_input_grad[i + 1]
            return (da if need_g else None), (dg if need_g else None), None
        return (da if need_a else None), (dg if need_g else None), None


def _make(device):
    g = seeded((8,), 5002, 0.5, 1.5)
    g[1], g[2] = 0.0, -0.75
    return {"a": seeded((2, 3, 4, 8), 5001).to(device), "g": g.to(device)}


def toy(flavour):
    STATE["acc"], STATE["parked"] = None, []
    return H.Node("toy:" + flavour, _make, lambda i: _Toy.apply(i["a"], i["g"], flavour), ("a", "g"),
                  lambda i: (i["a"] * i["g"], i["a"] + i["g"]),
                  dirty=lambda outs: [f"{len(STATE['parked'])} parked"] if STATE["parked"] else [])


CHECKS = {
    "flags": lambda n, r: H.check_flags(n, DEV, r),
    "unused": lambda n, r: H.check_unused(n, DEV, r, 2),
    "forms": lambda n, r: H.check_forms(n, DEV, r),
    "replay": lambda n, r: H.check_replay(n, DEV, r),
    "pruned": lambda n, r: H.check_pruned_then_full(n, DEV, r, (0,)),
    "inputs": lambda n, r: H.check_input_forms(n, DEV, r),
}
INPUT_MUTANTS = ("grad_like_saved", "input_read_linearly", "grad_transposed")


def test_the_correct_node_passes_every_check():
    report = H.Report()
    for name, check in CHECKS.items():
        check(toy("correct"), report)
    assert report.worst and all(r <= 1.0 for r, _ in report.worst.values())


@pytest.mark.parametrize("flavour,check,words", [
    ("swapped", "flags", "no gradient for"),
    ("neighbour_flag", "flags", "no gradient for"),
    ("none_as_ones", "unused", "misses the fp64 rule"),
    ("stride0_first", "forms", "misses the fp64 rule"),
    ("offset_ignored", "forms", "misses the fp64 rule"),
    ("acc_never_cleared", "replay", "replay: second grad"),
    ("acc_released", "replay", "replay: second grad"),
    ("dirty_after_pruned", "pruned", "state left behind by a pruned backward"),
    ("dgamma_zeroed", "flags", "d/dg misses the fp64 rule"),
    ("grad_like_saved", "inputs", "d/da differs from the fresh run"),
    ("input_read_linearly", "inputs", "output 0 differs from the fresh run"),
    # (a gradient of another shape never leaves the ENGINE, which raises RuntimeError: check_input_forms turns that undeclared
    #  refusal into its failure; its own shape assertions stand behind the engine's)
    ("grad_transposed", "inputs", "raised RuntimeError for a form it does not declare as refused: Function _ToyBackward returned an invalid gradient"),
])
def test_each_mutant_is_rejected_by_its_check(flavour, check, words):
    with pytest.raises(AssertionError, match=words):
        CHECKS[check](toy(flavour), H.Report())


@pytest.mark.parametrize("flavour", INPUT_MUTANTS)
def test_input_form_mutants_pass_every_older_check(flavour):
    """... whose inputs are all fresh contiguous tensors: no weaker check rejects them"""
    for name, check in CHECKS.items():
        if name != "inputs":
            check(toy(flavour), H.Report())


@pytest.mark.parametrize("form", ["format", "transposed"])
def test_the_warp_gather_bwd_pattern_is_wrong_for_each_dense_permuted_input(form):
    """the defect of torch_ops._warp_gather_bwd in one line each: right for a fresh input and for a slice (empty_like of a
    tensor that is not dense is contiguous), a permuted gradient for channels_last and for a transposed input"""
    node = toy("grad_like_saved")
    fresh = H.run_inputs(node, DEV, {})[1]["a"]
    assert torch.equal(H.run_inputs(node, DEV, {"a": "slice"})[1]["a"], fresh)
    got = H.run_inputs(node, DEV, {"a": form})[1]["a"]
    assert got.shape == fresh.shape and not torch.equal(got, fresh)
    assert torch.equal(got.as_strided((got.numel(),), (1,)), fresh.reshape(-1))   # the right values, in the wrong places


def test_an_unaligned_route_is_held_to_the_fp64_rule_only_where_the_node_names_it():
    """a summation order that changes with the pointer's alignment fails the equality -- unless the node documents the route
    (Node.unaligned), and then only the offset1 arrangements are held to the fp64 rule: no other form is loosened"""
    with pytest.raises(AssertionError, match=r"input a/offset1\]: d/dg differs from the fresh run"):
        H.check_input_forms(toy("unaligned_route"), DEV, H.Report())
    node = toy("unaligned_route")
    node.unaligned = "the toy sums d/dg in fp64 when `a` is not 16-byte aligned"
    report = H.Report()
    H.check_input_forms(node, DEV, report)
    assert all(r <= 1.0 for r, _ in report.worst.values())
    node = toy("grad_like_saved")
    node.unaligned = "(names a route it does not have)"
    with pytest.raises(AssertionError, match="d/da differs from the fresh run"):
        H.check_input_forms(node, DEV, H.Report())


def test_a_declared_refusal_must_happen():
    """`refuses` is a claim about the wrapper: a node that declares a refusal and computes instead fails"""
    node = toy("correct")
    node.refuses = {"a": frozenset(H.NOT_DENSE)}
    with pytest.raises(BaseException, match="DID NOT RAISE"):
        H.check_input_forms(node, DEV, H.Report())


@pytest.mark.parametrize("flavour", ["swapped", "neighbour_flag"])
def test_positional_mutants_are_invisible_while_every_flag_is_true(flavour):
    """... which is why the flag subsets exist"""
    node = toy(flavour)
    H.check_fp64(node, H.run(node, DEV), node.diff, None, "random", H.Report(), "all")


def test_scalar_cotangent_alone_rejects_the_stride0_mutant():
    """the .sum().backward() form proper: equality across forms, no fp64 rule involved"""
    node = toy("stride0_first")
    a = H.run(node, DEV, form="fresh", kind="scalar")
    b = H.run(node, DEV, form="stride0", kind="scalar")
    H.same(node, a, b, node.diff, "scalar")   # one value everywhere: this mutant is right by accident ...
    a = H.run(node, DEV, form="fresh", kind="rows")
    b = H.run(node, DEV, form="stride0", kind="rows")
    with pytest.raises(AssertionError, match="differs between two configurations"):
        H.same(node, a, b, node.diff, "rows")  # ... and wrong as soon as one dimension carries values


def test_a_wrongly_shaped_gradient_is_refused():
    node = toy("correct")
    grads = H.run(node, DEV)
    grads["g"] = grads["g"][:4]
    with pytest.raises(AssertionError, match="has shape"):
        H.check_fp64(node, grads, node.diff, None, "random", H.Report(), "all")


def test_flag_subsets_of_a_wide_node_are_three_families():
    diff = tuple("abcdefgh")
    subsets = H.flag_subsets(diff)
    assert len(subsets) == 1 + 8 + 8 and subsets[0] == diff and ("a",) in subsets and diff[1:] in subsets


def test_cotangent_forms_carry_the_same_values():
    for shape in ((2, 3, 4, 8), (1, 3, 4, 5, 8)):
        for kind in ("rows", "scalar"):
            v = H.cot_values(shape, 0, kind)
            forms = {f: H.cot_form(v, f, DEV, kind) for f in H.FORMS}
            assert all(torch.equal(t, v) for t in forms.values())
            assert 0 in forms["stride0"].stride() and not forms["format"].is_contiguous()
            assert forms["offset"].storage_offset() % 4 == 0 and forms["offset"].storage_offset() > 0
    assert H.cot_form(H.cot_values((2, 3, 4, 8), 0), "stride0", DEV, "random") is None


def test_input_forms_carry_the_same_values():
    for v in (seeded((2, 3, 4, 8), 1), seeded((1, 3, 4, 5, 8), 2), seeded((8,), 3), seeded((6, 5), 4), seeded((2, 3, 4, 8), 5) > 0,
              seeded((2, 3, 4, 8), 6).half(), seeded((2, 3, 4, 8), 7).contiguous(memory_format=torch.channels_last)):
        forms = {f: H.input_form(v, f, DEV) for f in H.INPUT_FORMS}
        assert all(t is None or (t.shape == v.shape and t.dtype == v.dtype and torch.equal(t, v)) for t in forms.values())
        assert forms["offset12"].storage_offset() == 12 and forms["offset1"].storage_offset() == 1
        assert forms["offset1"].data_ptr() % 16 == v.element_size()   # one element past 16-byte alignment
        assert all(forms[f].stride() == v.stride() for f in ("offset12", "offset1"))
        assert not forms["slice"].is_contiguous()
        assert (forms["format"] is None) == (v.dim() not in (4, 5)) and (forms["transposed"] is None) == (v.dim() < 2)
        for f in ("format", "transposed"):
            if forms[f] is not None:   # dense and permuted: the case in which *_like keeps the strides
                assert forms[f].stride() != v.stride() and torch.empty_like(forms[f]).stride() == forms[f].stride()
        # the neighbours of the values in memory are NaN (or the format's largest value): a linear read finds them
        if v.is_floating_point():
            whole = torch.as_strided(forms["offset1"], (v.numel() + 2,), (1,), 0)
            assert bool(whole[0].isnan()) and bool(whole[-1].isnan())
            assert bool(torch.as_strided(forms["slice"], (1,), (1,), 0).isnan())
    assert H.input_form(torch.tensor(1.0), "offset1", DEV) is None
