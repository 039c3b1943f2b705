"""CPU: the rule of tests/_adam_ref.py, which tests/test_gpu_optim.py holds K27 / K28 to, (a) lets torch's own fp32 Adam and
AdamW through on every case -- and measures the K the rule's docstring records -- and (b) rejects every wrong kernel of
_adam_ref.MUTANTS, written in numpy, on the same inputs."""
import math

import numpy as np
import pytest
import torch

from tests import _adam_ref as R


class TorchCPU:
    """torch.optim.Adam / AdamW, fp32, foreach=False, on the CPU; clipping as clip_grad_norm_ does it (g *= float32 coefficient,
    in place) with the norm taken in fp64: the rule of the norm is K27's business, not ATen's"""

    def __init__(self, mode, clip=False):
        hp = R.MODES[mode]
        self.clip = clip
        self.params = [torch.from_numpy(p.copy()).reshape(s) for p, (s, _) in zip(R.initial_params(), R.TENSORS)]
        groups = [dict(params=[p for p, grp in zip(self.params, R.GROUP_OF) if grp == k], lr=R.LRS[k]) for k in (0, 1)]
        cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
        self.opt = cls(groups, betas=R.BETAS, eps=R.EPS, weight_decay=hp["weight_decay"], foreach=False)

    def state(self):
        out = []
        for p in self.params:
            st = self.opt.state.get(p, {})
            if not st:
                out.append((p.detach().numpy().ravel(), np.zeros(p.numel(), R.F32), np.zeros(p.numel(), R.F32), 0.0))
            else:
                out.append((p.detach().numpy().ravel(), st["exp_avg"].numpy().ravel(), st["exp_avg_sq"].numpy().ravel(),
                            float(st["step"])))
        return out

    def step(self, grads, lrs):
        res = None
        if self.clip:
            norm, _ = R.norm_ref(grads)
            coef = np.float32(min(1.0, R.MAX_NORM / (norm + 1e-6)))
            grads = [None if g is None else g * coef for g in grads]
            res = (norm, coef)
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else torch.from_numpy(np.ascontiguousarray(g, dtype=R.F32)).reshape(p.shape)
        for group, lr in zip(self.opt.param_groups, lrs):
            group["lr"] = lr
        self.opt.step()
        return res


CASES = [(mode, clip) for mode in R.MODES for clip in (False, True)]


@pytest.fixture(scope="module")
def measured():
    """{(mode, clip): worst ratios at K = 1} of torch's CPU step, each case driven once under a K no honest step reaches"""
    return {(mode, clip): R.drive(TorchCPU(mode, clip), mode, clip, k=1024.0) for mode, clip in CASES}


@pytest.mark.parametrize("mode, clip", CASES)
def test_torch_fp32_step_is_inside_the_rule(measured, mode, clip):
    worst = measured[(mode, clip)]
    print(f"torch CPU {mode}{' clipped' if clip else ''}: largest err / bound(K = 1): "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst["p"], worst["m"], worst["v"]) <= R.K


def test_k_is_twice_what_torch_reaches(measured):
    top = max(max(w["p"], w["m"], w["v"]) for w in measured.values())
    print(f"largest err / bound(K = 1) of torch's CPU step over all cases: {top:.4f}; K_TORCH {R.K_TORCH}, K {R.K}")
    assert R.K == 2.0 * R.K_TORCH
    # (another CPU's vector units may round a little differently: the recorded figure is held to a factor, the rule to K)
    assert R.K_TORCH / 2.0 < top <= R.K, "torch's own step is far from what the docstring of tests/_adam_ref.py records"


@pytest.mark.parametrize("mode, clip", CASES)
def test_the_kernel_restated_in_numpy_is_inside_the_rule(mode, clip):
    worst = R.drive(R.NumpyKernel(mode, clip), mode, clip)
    assert max(worst["p"], worst["m"], worst["v"]) <= R.K


@pytest.mark.parametrize("defect", R.MUTANTS)
def test_rule_rejects_the_wrong_kernel(defect):
    mode, clip = R.MUTANT_NEEDS.get(defect, ("adamw", False))
    with pytest.raises(AssertionError):
        R.drive(R.NumpyKernel(mode, clip, defect), mode, clip)
    R.drive(R.NumpyKernel(mode, clip), mode, clip)  # (the same case passes without the defect)


def test_inputs_cover_what_the_gpu_test_claims():
    assert len(R.TENSORS) == 14 and sorted(set(R.GROUP_OF)) == [0, 1]
    for t in range(R.STEPS):
        grads = R.gradients(t)
        assert (grads[R.I_NO_GRAD] is None) == (t in R.NO_GRAD_STEPS)
        for g, (shape, tag) in zip(grads, R.TENSORS):
            if g is None:
                continue
            zeros = float((g == 0).mean())
            assert zeros == 1.0 if tag == "zero_grad" else (g.size < 64 or 0.2 < zeros < 0.47)
    norms = [R.norm_ref(R.gradients(t, reg))[0] for t, reg in enumerate(R.CLIP_REGIMES)]
    assert norms[0] > 100 and norms[3] > 100 and norms[2] == 0.0
    assert all(0.98 < n < 0.995 for n in (norms[1], norms[4]))
    assert math.isclose(R.lr_at(2, 0), R.LRS[0]) and math.isclose(R.lr_at(3, 0), 0.5 * R.LRS[0])
