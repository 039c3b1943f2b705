"""CPU: the host side of the fused optimizer step (activezero_amd/optim.py, csrc/az_optim.hip) -- the descriptor struct as
the C++ compiler lays it out against the table the Python side fills, argument checks that happen before any launch, the
options the constructor refuses, state_dict round trips with torch's own Adam / AdamW, and the refusal of CPU parameters."""
import copy
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from activezero_amd import _lib, build, optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("param", "grad", "exp_avg", "exp_avg_sq", "step", "n")


@pytest.fixture(scope="module")
def handle():
    build.build()
    return _lib.lib()


def test_struct_layout_is_what_the_compiler_sees(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the image is expected to have it")
    lines = ['std::printf("sizeof %zu\\n", sizeof(AzAdamDesc));']
    lines += [f'std::printf("{f} %zu+%zu\\n", offsetof(AzAdamDesc, {f}), sizeof(((AzAdamDesc *)0)->{f}));' for f in FIELDS]
    src, exe = tmp_path / "adam_desc.cpp", tmp_path / "adam_desc"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "azhip.h"\nint main() {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split(" ") for line in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    dtype = _lib.ADAM_DESC
    assert dtype.names == FIELDS and int(out["sizeof"]) == dtype.itemsize == 48
    for f in FIELDS:
        sub, offset = dtype.fields[f][:2]
        assert out[f] == f"{offset}+{sub.itemsize}", f


def test_table_bytes_are_the_struct_in_header_order():
    rows = [(0x7F0000001000, 0x7F0000002040, 0x7F0000003080, 0x7F00000040C0, 0x7F0000005004, 27648),
            (0xFFFF000011110000, 0x7E0000005004, 0x10, 0x20, 0x30, 1), (0x40, 0x50, 0x60, 0x70, 0x80, 1025),
            (0x90, 0xA0, 0xB0, 0xC0, 0xD0, (1 << 33) + 5)]
    descs, block_desc, first, nblocks = optim.adam_tables([dict(zip(FIELDS, r)) for r in rows])
    assert descs.view(np.uint8).tobytes() == b"".join(struct.pack("<QQQQQq", *r) for r in rows)
    nb = [27, 1, 2, (1 << 23) + 1]  # one workgroup per 1024 elements: 256 work items of four floats
    assert nblocks == sum(nb) and first.tolist() == [0, 27, 28, 30]
    assert block_desc.dtype == first.dtype == np.int32 and block_desc.size == nblocks
    assert block_desc[:31].tolist() == [0] * 27 + [1] + [2] * 2 + [3] and int(block_desc[-1]) == 3
    with pytest.raises(KeyError):
        optim.adam_tables([dict(zip(FIELDS[:-1], rows[0]))])


def test_argument_validation_happens_before_any_launch(handle):
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok, enull, einval = _lib.CONST["AZ_OK"], _lib.CONST["AZ_ENULL"], _lib.CONST["AZ_EINVAL"]
    assert (ok, enull, einval) == (0, -2, -1)
    # az_grad_sumsq_multi(partials, descs, block_desc, first_block, nd, nblocks, stream)
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert handle.az_grad_sumsq_multi(*args, 1, 1, None) == enull
    assert handle.az_grad_sumsq_multi(p, p, p, p, 0, 1, None) == einval
    assert handle.az_grad_sumsq_multi(p, p, p, p, 1, 0, None) == einval
    assert handle.az_grad_sumsq_multi(p, p, p, p, -3, 1, None) == einval
    # az_optim_begin(head, rec, descs, nd, partials, nblocks_norm, grad_scale, found_inf, lr, beta1, beta2, max_norm, stream)
    hp = (1e-3, 0.9, 0.999, 1.0)
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert handle.az_optim_begin(*args, 1, p, 1, None, None, *hp, None) == enull
    assert handle.az_optim_begin(p, p, p, 1, None, 1, None, None, *hp, None) == enull   # partials wanted, not given
    assert handle.az_optim_begin(p, p, p, 0, p, 1, None, None, *hp, None) == einval
    assert handle.az_optim_begin(p, p, p, 1, p, -1, None, None, *hp, None) == einval
    assert handle.az_optim_begin(p, p, p, 1, p, 1, None, None, 1e-3, 1.0, 0.999, 1.0, None) == einval   # beta1 = 1
    assert handle.az_optim_begin(p, p, p, 1, p, 1, None, None, 1e-3, 0.9, 0.999, float("nan"), None) == einval
    # az_adam_multi(descs, block_desc, first_block, nd, nblocks, head, rec, lr, beta1, beta2, eps, weight_decay, decoupled,
    #               use_mult, stream)
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    for k in range(5):
        args = [p, p, p, 1, 1, p, p]
        args[k + 2 if k >= 3 else k] = None
        assert handle.az_adam_multi(*args, *hp, None) == enull
    assert handle.az_adam_multi(p, p, p, 0, 1, p, p, *hp, None) == einval
    assert handle.az_adam_multi(p, p, p, 1, 0, p, p, *hp, None) == einval
    assert handle.az_adam_multi(p, p, p, 1, 1, p, p, 1e-3, 0.9, 0.999, -1e-8, 0.0, 0, 0, None) == einval
    assert handle.az_adam_multi(p, p, p, 1, 1, p, p, 1e-3, 0.9, 0.999, 1e-8, -0.1, 0, 0, None) == einval


def _params():
    torch.manual_seed(5)
    return [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))]


@pytest.mark.parametrize("option", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_constructor_refuses_unsupported_options(option):
    with pytest.raises(ValueError, match=option):
        optim.FusedAdam(_params(), **{option: True})
    with pytest.raises(ValueError, match=option):
        optim.FusedAdamW(_params(), **{option: True})
    optim.FusedAdam(_params(), **{option: False})


def test_constructor_refuses_other_dtypes_layouts_and_values():
    with pytest.raises(ValueError, match="float32"):
        optim.FusedAdam([torch.nn.Parameter(torch.randn(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="float32"):
        optim.FusedAdam([torch.nn.Parameter(torch.randn(4).to(torch.bfloat16))])
    with pytest.raises(ValueError, match="contiguous"):
        optim.FusedAdam([torch.nn.Parameter(torch.randn(4, 6).t())])
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0),
                dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            optim.FusedAdam(_params(), **bad)
    with pytest.raises(TypeError, match="momentum"):
        optim.FusedAdam(_params(), momentum=0.9)
    opt = optim.FusedAdam(_params())
    with pytest.raises(ValueError, match="float32"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.randn(3).double())]))


def test_defaults_are_torchs():
    a, w = optim.FusedAdam(_params()), optim.FusedAdamW(_params())
    ta, tw = torch.optim.Adam(_params()), torch.optim.AdamW(_params())
    for mine, theirs in ((a, ta), (w, tw)):
        for key in ("lr", "betas", "eps", "weight_decay"):
            assert mine.defaults[key] == theirs.defaults[key], key
    assert a.defaults["decoupled_weight_decay"] is False and w.defaults["decoupled_weight_decay"] is True
    assert a._step_supports_amp_scaling is True and a.max_grad_norm is None and a.last_grad_norm is None


def test_step_on_cpu_parameters_raises():
    ps = _params()
    opt = optim.FusedAdam(ps)
    opt.step()  # (no gradient anywhere: nothing to do, as in torch)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    assert all(torch.equal(a, p) for a, p in zip(before, ps)) and not opt.state


def _torch_state_after_two_steps(cls, **kw):
    ps = _params()
    opt = cls(ps, lr=2e-3, **kw)
    for k in range(2):
        for p in ps:
            p.grad = torch.full_like(p, 0.5 + k)
        opt.step()
    return ps, opt


@pytest.mark.parametrize("fused_cls, torch_cls", [(optim.FusedAdam, torch.optim.Adam), (optim.FusedAdamW, torch.optim.AdamW)])
def test_state_dict_round_trips_with_torch(fused_cls, torch_cls):
    ps, topt = _torch_state_after_two_steps(torch_cls, weight_decay=0.02)
    sd = copy.deepcopy(topt.state_dict())  # (as a saved file would be: torch's load shares tensors that need no cast)
    # torch -> fused
    mine = fused_cls(_params(), max_grad_norm=1.0)
    mine.load_state_dict(sd)
    assert mine.param_groups[0]["lr"] == 2e-3 and mine.param_groups[0]["weight_decay"] == 0.02
    for p, q in zip(mine.param_groups[0]["params"], ps):
        st, want = mine.state[p], topt.state[q]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], want["exp_avg"]) and torch.equal(st["exp_avg_sq"], want["exp_avg_sq"])
    # fused -> torch: the loaded optimizer steps on as the original does
    back = torch_cls(_params())
    back.load_state_dict(copy.deepcopy(mine.state_dict()))
    qs = back.param_groups[0]["params"]
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    for opt_, params in ((topt, ps), (back, qs)):
        for p in params:
            p.grad = torch.full_like(p, -0.25)
        opt_.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        assert float(back.state[q]["step"]) == 3.0
    # a state with an option this class refuses is refused at load
    bad = torch_cls(_params(), amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        fused_cls(_params()).load_state_dict(bad)
