"""CPU: the `azhip::*` dispatcher registration (activezero_amd/torch_ops.py): schemas exist, shape inference
runs on the meta device (what FakeTensor / torch.compile tracing uses) with no GPU, CPU tensors are refused."""
import pytest
import torch

import activezero_amd.torch_ops  # noqa: F401  (registers the operators)


def test_schemas_registered():
    for name in ("warp_scatter", "cost_volume", "softargmin", "softargmin_fwd", "softargmin_bwd", "warp_gather",
                 "warp_gather_bwd", "local_contrast_norm", "cost_volume_bwd", "conv3d", "conv3d_input_grad",
                 "conv3d_weight_grad", "bn3d", "patch_reproj", "patch_reproj_bwd"):
        assert hasattr(torch.ops.azhip, name), name
    assert "Tensor logits" in str(torch.ops.azhip.softargmin.default._schema)


def test_meta_shape_inference_without_a_gpu():
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    assert torch.ops.azhip.softargmin(m(2, 48, 34, 60)).shape == (2, 1, 136, 240)
    assert torch.ops.azhip.softargmin(m(2, 1, 48, 34, 60)).shape == (2, 1, 136, 240)
    assert torch.ops.azhip.cost_volume(m(2, 32, 34, 60), m(2, 32, 34, 60), 48).shape == (2, 64, 48, 34, 60)
    assert torch.ops.azhip.warp_gather(m(2, 3, 16, 24), m(2, 1, 16, 24)).shape == (2, 3, 16, 24)
    assert torch.ops.azhip.warp_scatter(m(2, 1, 16, 24), m(2, 1, 16, 24, dtype=torch.int32), 1).shape == (2, 1, 16, 24)
    n, s = torch.ops.azhip.local_contrast_norm(m(2, 1, 16, 24), 9, 1e-5)
    assert n.shape == s.shape == (2, 1, 16, 24)
    # K4/K5 on a channels-last volume: stride 1, stride 2, transposed stride 2 (psmnet_3.py:15-58)
    assert torch.ops.azhip.conv3d(m(2, 12, 34, 60, 32), m(32, 32, 3, 3, 3), 0).shape == (2, 12, 34, 60, 32)
    assert torch.ops.azhip.conv3d(m(2, 12, 34, 60, 32), m(64, 32, 3, 3, 3), 1).shape == (2, 6, 17, 30, 64)
    assert torch.ops.azhip.conv3d(m(2, 6, 17, 30, 64), m(64, 32, 3, 3, 3), 2).shape == (2, 12, 34, 60, 32)
    assert torch.ops.azhip.bn3d(m(2, 6, 17, 30, 64), m(64), m(64), None, True).shape == (2, 6, 17, 30, 64)
    assert torch.ops.azhip.patch_reproj(m(2, 1, 32, 48), m(2, 1, 32, 48), m(2, 1, 32, 48), None, 11).shape == ()


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError):
        torch.ops.azhip.softargmin(torch.zeros(1, 4, 3, 3))
    with pytest.raises(RuntimeError):
        torch.ops.azhip.warp_gather(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


# ---- memory forms and mismatched arguments on the meta device ---------------------------------------------------------------
def _m(*s, dtype=torch.float32):
    return torch.empty(*s, dtype=dtype, device="meta")


def _forms(t):
    """the dense permuted forms whose strides *_like would keep: the other memory format and the last two dimensions swapped"""
    out = [t.transpose(-1, -2).contiguous().transpose(-1, -2)]
    if t.dim() == 4:
        out.append(t.contiguous(memory_format=torch.channels_last))
    if t.dim() == 5:
        out.append(t.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1))
    assert all(f.shape == t.shape for f in out) and not out[0].is_contiguous()  # (channels_last of one channel is contiguous)
    return out


META_CALLS = {
    "warp_scatter": lambda f: torch.ops.azhip.warp_scatter(f(_m(2, 3, 4, 6)), f(_m(2, 1, 4, 6, dtype=torch.int32)), 1),
    "cost_volume": lambda f: torch.ops.azhip.cost_volume(f(_m(2, 8, 4, 6)), f(_m(2, 8, 4, 6)), 3),
    "cost_volume_bwd": lambda f: torch.ops.azhip.cost_volume_bwd(f(_m(2, 16, 3, 4, 6)), 3),
    "softargmin": lambda f: torch.ops.azhip.softargmin(f(_m(2, 6, 3, 5))),
    "softargmin_fwd": lambda f: torch.ops.azhip.softargmin_fwd(f(_m(2, 1, 6, 3, 5))),
    "softargmin_bwd": lambda f: torch.ops.azhip.softargmin_bwd(f(_m(2, 1, 12, 20)), f(_m(2, 6, 3, 5)), f(_m(2, 12, 20, 2)),
                                                               f(_m(2, 1, 12, 20))),
    "warp_gather": lambda f: torch.ops.azhip.warp_gather(f(_m(2, 3, 4, 6)), f(_m(2, 1, 4, 6))),
    "warp_gather_bwd": lambda f: torch.ops.azhip.warp_gather_bwd(f(_m(2, 3, 4, 6)), f(_m(2, 3, 4, 6)), f(_m(2, 1, 4, 6)), True),
    "local_contrast_norm": lambda f: torch.ops.azhip.local_contrast_norm(f(_m(2, 3, 4, 6)), 3, 1e-5),
    "conv3d": lambda f: torch.ops.azhip.conv3d(f(_m(2, 4, 6, 8, 32)), f(_m(64, 32, 3, 3, 3)), 1),
    "conv3d_input_grad": lambda f: torch.ops.azhip.conv3d_input_grad(f(_m(2, 2, 3, 4, 64)), f(_m(64, 32, 3, 3, 3)), 1),
    "conv3d_weight_grad": lambda f: torch.ops.azhip.conv3d_weight_grad(f(_m(2, 2, 3, 4, 64)), f(_m(2, 4, 6, 8, 32)),
                                                                       f(_m(64, 32, 3, 3, 3)), 2),
    "bn3d": lambda f: torch.ops.azhip.bn3d(f(_m(2, 4, 6, 8, 32)), _m(32), _m(32), f(_m(2, 4, 6, 8, 32)), True),
    "patch_reproj": lambda f: torch.ops.azhip.patch_reproj(f(_m(2, 1, 8, 12)), f(_m(2, 1, 8, 12)), f(_m(2, 1, 8, 12)), None, 3),
    "patch_reproj_bwd": lambda f: torch.ops.azhip.patch_reproj_bwd(_m(()), f(_m(2, 1, 8, 12)), f(_m(2, 1, 8, 12)),
                                                                   f(_m(2, 1, 8, 12)), f(_m(2, 1, 8, 12, dtype=torch.bool)), 3),
}


@pytest.mark.parametrize("name", sorted(META_CALLS))
def test_meta_outputs_are_contiguous_for_permuted_inputs(name):
    """the real implementations return fresh contiguous tensors whatever the inputs' strides are, so the fake ones must
    say so: empty_like of a channels_last or transposed input would trace strides that no kernel writes"""
    want = None
    for k in range(3):  # contiguous, transposed, the other memory format
        pick = (lambda t: t) if k == 0 else (lambda t, k=k: _forms(t)[min(k, len(_forms(t))) - 1])
        outs = META_CALLS[name](pick)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        for o in outs:
            assert o.is_contiguous() and o.stride() == torch.empty(o.shape, device="meta").stride(), (name, k, o.stride())
        shapes = [tuple(o.shape) for o in outs]
        want = want or shapes
        assert shapes == want


def test_meta_calls_cover_every_operator():
    """against what the library DEFINES (the dispatcher's own list: `dir(torch.ops.azhip)` only shows the names somebody has
    already touched), so this holds whatever ran before it"""
    defined = {n.split("::")[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("azhip::")}
    assert len(defined) == 15 and sorted(META_CALLS) == sorted(defined)


MISMATCHED = {
    "bn3d short scale": lambda: torch.ops.azhip.bn3d(_m(2, 4, 6, 8, 32), _m(16), _m(32), None, True),
    "bn3d short shift": lambda: torch.ops.azhip.bn3d(_m(2, 4, 6, 8, 32), _m(32), _m(31), None, False),
    "bn3d residual shape": lambda: torch.ops.azhip.bn3d(_m(2, 4, 6, 8, 32), _m(32), _m(32), _m(2, 4, 6, 4, 32), True),
    "cost_volume_bwd ndisp": lambda: torch.ops.azhip.cost_volume_bwd(_m(2, 16, 3, 4, 6), 4),
    "cost_volume_bwd odd channels": lambda: torch.ops.azhip.cost_volume_bwd(_m(2, 15, 3, 4, 6), 3),
    "softargmin_bwd stats": lambda: torch.ops.azhip.softargmin_bwd(_m(2, 1, 12, 20), _m(2, 6, 3, 5), _m(2, 12, 20, 1), _m(2, 1, 12, 20)),
    "softargmin_bwd disp": lambda: torch.ops.azhip.softargmin_bwd(_m(2, 1, 12, 20), _m(2, 6, 3, 5), _m(2, 12, 20, 2), _m(2, 1, 3, 5)),
    "softargmin_bwd grad": lambda: torch.ops.azhip.softargmin_bwd(_m(2, 1, 3, 5), _m(2, 6, 3, 5), _m(2, 12, 20, 2), _m(2, 1, 12, 20)),
    "warp_gather_bwd grad_out": lambda: torch.ops.azhip.warp_gather_bwd(_m(2, 1, 4, 6), _m(2, 3, 4, 6), _m(2, 1, 4, 6), True),
    "warp_gather disp": lambda: torch.ops.azhip.warp_gather(_m(2, 3, 4, 6), _m(2, 1, 4, 5)),
    "conv3d channels": lambda: torch.ops.azhip.conv3d(_m(2, 4, 6, 8, 16), _m(64, 32, 3, 3, 3), 0),
    "conv3d transposed channels": lambda: torch.ops.azhip.conv3d(_m(2, 4, 6, 8, 32), _m(64, 32, 3, 3, 3), 2),
    "conv3d_input_grad channels": lambda: torch.ops.azhip.conv3d_input_grad(_m(2, 4, 6, 8, 32), _m(64, 32, 3, 3, 3), 0),
    "conv3d_weight_grad x channels": lambda: torch.ops.azhip.conv3d_weight_grad(_m(2, 4, 6, 8, 16), _m(2, 4, 6, 8, 64), _m(64, 32, 3, 3, 3), 0),
    "conv3d_weight_grad grad channels": lambda: torch.ops.azhip.conv3d_weight_grad(_m(2, 4, 6, 8, 32), _m(2, 4, 6, 8, 32), _m(64, 32, 3, 3, 3), 0),
    "conv3d_weight_grad extent": lambda: torch.ops.azhip.conv3d_weight_grad(_m(2, 4, 6, 8, 32), _m(2, 4, 6, 8, 64), _m(64, 32, 3, 3, 3), 1),
    "patch_reproj disp": lambda: torch.ops.azhip.patch_reproj(_m(2, 1, 8, 12), _m(2, 1, 8, 12), _m(2, 1, 8, 6), None, 3),
    "patch_reproj mask": lambda: torch.ops.azhip.patch_reproj(_m(2, 1, 8, 12), _m(2, 1, 8, 12), _m(2, 1, 8, 12), _m(2, 1, 8, 6), 3),
}


@pytest.mark.parametrize("case", sorted(MISMATCHED))
def test_mismatched_arguments_are_refused_on_meta(case):
    """sizes come from one argument and pointers from another: what disagrees would be read past its end, so it is refused --
    on meta by the fake function, through the very helper that the CUDA implementation calls first"""
    with pytest.raises(RuntimeError):
        MISMATCHED[case]()


def test_the_cuda_implementations_call_the_checks_of_the_fakes():
    """one helper, two callers: each check named in a fake function's code is named in its CUDA implementation's too"""
    import activezero_amd.torch_ops as T

    pairs = [(T._cost_volume_bwd, T._cost_volume_bwd_fake), (T._softargmin_bwd, T._softargmin_bwd_fake),
             (T._warp_gather, T._warp_gather_fake), (T._warp_gather_bwd, T._warp_gather_bwd_fake), (T._conv3d, T._conv3d_fake),
             (T._conv3d_input_grad, T._conv3d_in_dims), (T._conv3d_weight_grad, T._conv3d_weight_grad_fake),
             (T._bn3d, T._bn3d_fake), (T._pr_args, T._patch_reproj_fake), (T._pr_args, T._patch_reproj_bwd_fake)]
    for impl, fake in pairs:
        checks = {n for n in fake.__code__.co_names if n.startswith("_check_")}
        assert checks and checks <= set(impl.__code__.co_names), (impl.__name__, checks)
    for impl in (T._patch_reproj, T._patch_reproj_bwd):
        assert "_pr_args" in impl.__code__.co_names
