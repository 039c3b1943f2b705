"""GPU: the fused optimizer step (activezero_amd/optim.py; K27 az_grad_sumsq_multi, az_optim_begin, K28 az_adam_multi of
csrc/az_optim.hip) under the rule of tests/_adam_ref.py -- every element of p, exp_avg and exp_avg_sq of 14 tensors (sizes on
both sides of the 4-element vector, the 256-thread workgroup and its 1024 elements; a misaligned one, one without gradient at
two steps, one with all-zero gradients) in two parameter groups over five steps, Adam with and without coupled decay and
AdamW, plain and clipped; the skip on non-finite gradients; GradScaler's protocol; determinism; no host synchronisation; and
the version counters the packed weight images are keyed on."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import optim, packing  # noqa: E402
from tests import _adam_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)


class Fused:
    """optim.FusedAdam / FusedAdamW behind the interface of _adam_ref.drive; the gradients live in persistent tensors, as
    the gradient arena of a training run does"""

    def __init__(self, mode, clip=False, **kw):
        hp = R.MODES[mode]
        self.clip = clip
        self.params = []
        for p, (shape, tag) in zip(R.initial_params(), R.TENSORS):
            t = torch.from_numpy(p).to(DEV)
            if tag == "misaligned":
                buf = torch.zeros(p.size + 8, device=DEV)
                buf[1:1 + p.size] = t
                t = buf[1:1 + p.size]
                assert t.data_ptr() % 16 == 4
            self.params.append(torch.nn.Parameter(t.reshape(shape)))
        self.grads = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        groups = [dict(params=[p for p, grp in zip(self.params, R.GROUP_OF) if grp == k], lr=R.LRS[k]) for k in (0, 1)]
        cls = optim.FusedAdamW if hp["decoupled"] else optim.FusedAdam
        self.opt = cls(groups, betas=R.BETAS, eps=R.EPS, weight_decay=hp["weight_decay"],
                       max_grad_norm=R.MAX_NORM if clip else None, **kw)

    def state(self):
        out = []
        for p in self.params:
            st = self.opt.state.get(p, {})
            if not st:
                out.append((p.detach().cpu().numpy().ravel(), np.zeros(p.numel(), R.F32), np.zeros(p.numel(), R.F32), 0.0))
            else:
                assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].device == p.device
                out.append((p.detach().cpu().numpy().ravel(), st["exp_avg"].cpu().numpy().ravel(),
                            st["exp_avg_sq"].cpu().numpy().ravel(), float(st["step"])))
        return out

    def load(self, grads):
        for p, buf, g in zip(self.params, self.grads, grads):
            if g is None:
                p.grad = None
            else:
                buf.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=R.F32)).reshape(buf.shape))
                p.grad = buf

    def step(self, grads, lrs):
        self.load(grads)
        for group, lr in zip(self.opt.param_groups, lrs):
            group["lr"] = lr
        self.opt.step()
        if self.clip:
            return float(self.opt.last_grad_norm), float(self.opt.last_clip_coef)
        return None

    def bits(self):
        return [np.concatenate([a.view(np.uint32) for a in s[:3]] + [np.array([s[3]], np.float32).view(np.uint32)])
                for s in self.state()]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}: tensor {i} {R.TENSORS[i][0]}: {int((x != y).sum())} words differ"


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_every_element_is_inside_the_rule(mode, clip):
    impl = Fused(mode, clip)
    worst = R.drive(impl, mode, clip)
    print(f"{mode}{' clipped' if clip else ''}: largest err / bound(K = 1): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"  (K = {R.K})")
    steps = [s[3] for s in impl.state()]
    assert steps[R.I_NO_GRAD] == R.STEPS - len(R.NO_GRAD_STEPS)  # it lags
    assert all(s == R.STEPS for i, s in enumerate(steps) if i != R.I_NO_GRAD)  # torch's count: one per step with a gradient
    for s in impl.state():
        assert all(np.isfinite(a).all() for a in s[:3])  # (the clipped run has a step of all-zero gradients: no NaN)
    # at most three launches per group and step (sumsq, begin, update), two without a norm
    assert impl.opt.launches == R.STEPS * 2 * (3 if clip else 2)


def test_a_norm_just_below_max_norm_gives_the_bits_of_the_unclipped_run():
    a, b = Fused("adam_wd", clip=True), Fused("adam_wd", clip=False)
    for t in range(3):
        grads = R.gradients(t, "just_below")
        lrs = (R.lr_at(t, 0), R.lr_at(t, 1))
        norm, coef = a.step(grads, lrs)
        b.step(grads, lrs)
        assert 0.98 < norm < 1.0 and coef == 1.0
        _same(a.bits(), b.bits(), f"step {t}")


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan], ids=["inf", "-inf", "nan"])
def test_a_non_finite_gradient_skips_the_step_of_every_tensor(bad):
    impl = Fused("adamw", clip=True)
    impl.step(R.gradients(0), R.LRS)
    before = impl.bits()
    grads = R.gradients(2)  # (a step at which every tensor has a gradient)
    grads[7] = grads[7].copy()
    grads[7][513] = bad
    norm, _ = impl.step(grads, R.LRS)
    assert not math.isfinite(norm)
    _same(impl.bits(), before, f"the step with one {bad} in tensor 7")  # p, m, v and the step count of EVERY tensor
    norm, _ = impl.step(R.gradients(2), R.LRS)
    assert math.isfinite(norm)
    assert [s[3] for s in impl.state()] == [2.0] * len(R.TENSORS)  # counts on from where it was
    # ... and that step is the one a run without the bad step takes
    clean = Fused("adamw", clip=True)
    clean.step(R.gradients(0), R.LRS)
    clean.step(R.gradients(2), R.LRS)
    _same(impl.bits(), clean.bits(), "the step after the skipped one")


def test_found_inf_skips_and_grad_scale_unscales():
    impl = Fused("adam")
    impl.step(R.gradients(0), R.LRS)
    before = impl.bits()
    impl.opt.found_inf = 1
    impl.step(R.gradients(2), R.LRS)
    _same(impl.bits(), before, "found_inf = 1 with finite gradients")
    impl.opt.found_inf = torch.zeros(1, device=DEV)
    impl.opt.grad_scale = torch.full((1,), 1024.0, device=DEV)
    impl.step([g * R.F32(1024) for g in R.gradients(2)], R.LRS)
    scaled_norm = float(impl.opt.last_grad_norm)
    del impl.opt.found_inf, impl.opt.grad_scale
    plain = Fused("adam")
    plain.step(R.gradients(0), R.LRS)
    plain.step(R.gradients(2), R.LRS)
    _same(impl.bits(), plain.bits(), "grad_scale = 1024 on gradients multiplied by 1024")
    assert plain.opt.last_grad_norm is None
    R.check_norm(scaled_norm, R.gradients(2), "last_grad_norm under grad_scale")  # the norm of the UNSCALED gradients
    # a number for grad_scale is accepted as well
    impl.opt.grad_scale = 1024
    impl.step([g * R.F32(1024) for g in R.gradients(4)], R.LRS)
    plain.step(R.gradients(4), R.LRS)
    _same(impl.bits(), plain.bits(), "grad_scale = 1024 as a number")


def test_the_same_inputs_twice_give_the_same_bits():
    runs = []
    for _ in range(2):
        impl, norms = Fused("adam_wd", clip=True), []
        for t in range(3):
            norm, coef = impl.step(R.gradients(t, R.CLIP_REGIMES[t]), R.LRS)
            norms.append((np.float32(norm).view(np.uint32), np.float32(coef).view(np.uint32)))
        runs.append((impl.bits(), norms))
    _same(runs[0][0], runs[1][0], "second run")
    assert runs[0][1] == runs[1][1]


def test_a_steady_state_step_does_not_synchronise_and_bumps_the_versions():
    impl = Fused("adamw", clip=True)
    grads = [R.gradients(t) for t in (0, 2, 4)]  # (steps at which every tensor has a gradient: one set of addresses)
    impl.step(grads[0], R.LRS)
    impl.step(grads[1], R.LRS)
    impl.load(grads[2])
    impl.opt.param_groups[0]["lr"] = 5e-4  # a scheduler's write: read at the step, no table is rebuilt
    versions = [p._version for p in impl.params]
    launches = impl.opt.launches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        impl.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert impl.opt.launches - launches == 6
    assert all(p._version > v for p, v in zip(impl.params, versions))
    assert [s[3] for s in impl.state()] == [3.0] * len(R.TENSORS)


def test_prepack_packs_again_after_a_step():
    plan = packing.PackPlan(DEV)
    w = torch.nn.Parameter(torch.from_numpy(R.initial_params()[10]).reshape(32, 32, 3, 3, 3).to(DEV))
    plan.prepack([w])
    e, fresh = plan.lookup(w, packing.PACK_3D_ROLL, 32, 32, 32, 32, 32 * 27, 27, 27, False)
    assert e is not None and not fresh
    plan.prepack([w])
    assert plan.launches == 1
    image = e.packed.clone()
    plan.prepack([w])
    assert plan.launches == 1  # nothing moved
    opt = optim.FusedAdam([w], lr=1e-2)
    w.grad = torch.ones_like(w)
    opt.step()
    plan.prepack([w])
    assert plan.launches == 2, "the step wrote the weight through a raw pointer: its version counter must have moved"
    assert not torch.equal(e.packed.view(torch.int32), image.view(torch.int32))


def _amp_model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1, bias=False)).to(DEV)


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        z = np.zeros(p.numel(), R.F32)
        out.append((p.detach().cpu().numpy().ravel().copy(), st["exp_avg"].cpu().numpy().ravel() if st else z,
                    st["exp_avg_sq"].cpu().numpy().ravel() if st else z, float(st["step"]) if st else 0.0))
    return out


def test_grad_scaler_drives_it_as_it_drives_torchs_adamw():
    """scale(loss).backward(); unscale_(opt); step(opt); update() on a three-tensor model, the second step with an inf in one
    gradient: each optimizer's step is inside the rule against its own previous state and unscaled gradients, both skip the
    bad step, the scalers agree, and after the first step (same start) the two differ by at most both bounds"""
    hp = dict(lr=1e-2, betas=R.BETAS, eps=R.EPS, weight_decay=1e-2)
    runs = []
    for make in (lambda ps: optim.FusedAdamW(ps, **hp), lambda ps: torch.optim.AdamW(ps, **hp)):
        model = _amp_model(11)
        params = list(model.parameters())
        assert len(params) == 3
        opt, scaler = make(params), torch.amp.GradScaler("cuda", init_scale=2.0 ** 12)
        torch.manual_seed(12)
        log = []
        for t in range(3):
            x, y = torch.randn(32, 8, device=DEV), torch.randn(32, 1, device=DEV)
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.mse_loss(model(x), y)
            scaler.scale(loss).backward()
            if t == 1:
                params[0].grad[3, 2] = math.inf
            scaler.unscale_(opt)
            grads = [p.grad.detach().cpu().numpy().ravel().copy() for p in params]
            before = _snapshot(opt, params)
            scaler.step(opt)
            scaler.update()
            log.append((before, grads, _snapshot(opt, params), float(scaler.get_scale())))
        runs.append(log)
    for name, log in zip(("FusedAdamW", "torch.optim.AdamW"), runs):
        for t, (before, grads, after, scale) in enumerate(log):
            assert scale == (2.0 ** 12 if t == 0 else 2.0 ** 11)
            for i, (b, g, a) in enumerate(zip(before, grads, after)):
                what = f"{name} step {t} tensor {i}"
                if t == 1:
                    for x, y in zip(a[:3], b[:3]):
                        R.same_bits(x, y, what + " (skipped)")
                    assert a[3] == b[3]
                    continue
                assert a[3] == b[3] + 1.0
                args = (b[0], g, b[1], b[2], a[3], hp["lr"], hp["weight_decay"], True)
                ref, one = R.adam_f64(*args, k=R.K), R.adam_f64(*args, k=1.0)
                for key, j in (("m", 1), ("v", 2), ("p", 0)):
                    R.ratio(a[j], ref[key], ref["tol_" + key], one["tol_" + key], f"{what}: {key}")
    mine, theirs = runs[0][0], runs[1][0]
    for i, (b, g, a, th) in enumerate(zip(mine[0], mine[1], mine[2], theirs[2])):
        ref = R.adam_f64(b[0], g, b[1], b[2], 1.0, hp["lr"], hp["weight_decay"], True, k=R.K)
        for key, j in (("p", 0), ("m", 1), ("v", 2)):
            assert (np.abs(a[j].astype(np.float64) - th[j]) <= 2.0 * ref["tol_" + key]).all(), (i, key)
