"""What tests/test_gpu_optim.py holds the optimizer step to (numpy only): K27 az_grad_sumsq_multi, az_optim_begin and K28
az_adam_multi (csrc/az_optim.hip; activezero_amd/optim.py) -- the Adam / AdamW update restated in fp64 from the float32
inputs, the rule a result is compared by, the inputs of the comparison, and `drive`, which takes ANY implementation of the
step (the library's, torch's on the CPU, a wrong kernel written in numpy) through those inputs under the rule.
tests/test_adam_error_model_cpu.py proves on the CPU that torch's own fp32 step passes and that every wrong kernel of MUTANTS
is rejected.

Why not ulps of the result.  torch's own fp32 step is hundreds to thousands of ulps from fp64 in exp_avg wherever m and g
cancel, and in g + wd p.  The rule is a running-error bound on operand magnitudes, u = 2^-24, per element:
    g'  = g mult (+ wd p, coupled decay)          tol_g' = K u (|g mult| + wd |p|)
    m'  = m + (1 - beta1) (g' - m)                tol_m  = K u (|m| + |g'|) + (1 - beta1) tol_g'
    v'  = beta2 v + (1 - beta2) g'^2              tol_v  = K u v' + 2 (1 - beta2) |g'| tol_g'
    dp  = step_size m' / denom,  denom = sqrt(v') / bc2sqrt + eps,  p' = p (1 - lr wd, decoupled decay) - dp
    tol_p = K u (|p| + |dp|) + step_size tol_m / denom + |dp| min(tol_v / (2 sqrt(v')), sqrt(tol_v)) / (bc2sqrt denom)
(the last term is what tol_v does to sqrt(v'); sqrt(a + t) - sqrt(a) <= min(t / (2 sqrt(a)), sqrt(t)), so it stays bounded
through the eps in denom when v' = 0).  The restatement is fed the implementation's OWN previous float32 state at every step,
so errors do not pile up over steps; every element of every tensor takes part.

K is measured, not chosen: the largest err / bound(K = 1) that torch's own fp32 CPU step (foreach=False) reaches against the
restatement on these inputs, doubled -- hipcc may contract a multiply-add where ATen does not, which moves at most one
rounding per operation.  tests/test_adam_error_model_cpu.py measures it again at every run and prints it:
    measured 2.213  (the parameter under AdamW, clipped; exp_avg_sq reaches 2.151, exp_avg 0.982, the parameter under coupled
                     decay 1.362: float32(0.999), float32(0.001) and float32(1 - lr wd) are themselves up to u / 2 off)
    K_TORCH = 2.22, K = 4.44
Steps are exact: every parameter that had a gradient counts one more, the others stand still, bit for bit in p, m, v too.

The gradient norm is compared with sqrt(fsum(g^2)) (the squares exact in fp64) under the rule of tests/_reduce_ref.py for an
fp64 sum of m terms in any order, m 2^-52 sum|term| -- relative to the sum, so half of it relative to the norm -- plus the
fp64 roundings of sqrt and the scale and ONE float32 rounding of the stored value.  The clip coefficient is compared with
min(1, max_norm / (norm + 1e-6)) in fp64, with the norm's bound propagated through it plus 3 u relative; where the fp64
coefficient clamps to 1 with room to spare, the result must be exactly 1.
"""
import math

import numpy as np

from tests._reduce_ref import fsum, sum_bound

F32 = np.float32
U = 2.0 ** -24
K_TORCH = 2.22
K = 2.0 * K_TORCH

BETAS, EPS = (0.9, 0.999), 1e-8
MODES = {"adam": dict(weight_decay=0.0, decoupled=False), "adam_wd": dict(weight_decay=1e-2, decoupled=False),
         "adamw": dict(weight_decay=1e-2, decoupled=True)}
LRS = (1e-3, 3e-4)        # the two parameter groups: even / odd tensors
LR_CHANGE = (3, 0.5)      # before the step of index 3 (the fourth) every group's lr is halved
STEPS = 5
SCALES = (1e-6, 1e-2, 10.0)
# (shape, what is special about it): 14 tensors
TENSORS = [((1,), None), ((3,), None), ((4,), None), ((255,), None), ((256,), None), ((257,), None), ((1023,), None),
           ((1024,), None), ((1025,), None), ((4099,), None), ((32, 32, 3, 3, 3), None),
           ((2049,), "no_grad"),      # grad = None at the steps of index 1 and 3 (the second and the fourth)
           ((1027,), "misaligned"),   # starts one float past a 16-byte boundary
           ((513,), "zero_grad")]     # all-zero gradients at every step
NO_GRAD_STEPS = (1, 3)
GROUP_OF = [i % 2 for i in range(len(TENSORS))]
I_NO_GRAD = [i for i, (_, tag) in enumerate(TENSORS) if tag == "no_grad"][0]
MAX_NORM = 1.0
CLIP_REGIMES = ("far_above", "just_below", "zero", "far_above", "just_below")  # per step, when clipping


def numel(shape):
    return int(np.prod(shape))


def initial_params(seed=2700):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(numel(s)) * 0.2).astype(F32) for s, _ in TENSORS]


def gradients(step, regime=None, seed=2701):
    """the list of float32 gradients of one step (None: the parameter has no gradient): a third of the entries zero, the
    scale of tensor i at this step SCALES[(i + step) % 3]; regime (clipping): "far_above" as they are (norm >> 1),
    "just_below" all scaled to a global norm of 0.99, "zero" all zero"""
    rng = np.random.default_rng(seed + step)
    out = []
    for i, (shape, tag) in enumerate(TENSORS):
        n = numel(shape)
        g = rng.standard_normal(n) * SCALES[(i + step) % 3]
        g[rng.uniform(0, 1, n) < 1.0 / 3.0] = 0.0
        if tag == "zero_grad" or regime == "zero":
            g[:] = 0.0
        out.append(g.astype(F32))
    if regime == "just_below":
        norm = math.sqrt(sum(fsum(g.astype(np.float64) ** 2) for g in out))
        out = [(g.astype(np.float64) * (0.99 / norm)).astype(F32) for g in out]
    out[I_NO_GRAD] = None if step in NO_GRAD_STEPS else out[I_NO_GRAD]
    return out


def lr_at(step, group):
    return LRS[group] * (LR_CHANGE[1] if step >= LR_CHANGE[0] else 1.0)


# ---- the fp64 restatement and its bound ----------------------------------------------------------------------------------
def adam_f64(p, g, m, v, step, lr, weight_decay, decoupled, mult=1.0, k=1.0, betas=BETAS, eps=EPS):
    """one tensor's step from its float32 inputs, `step` the count AFTER this step: dict p, m, v (fp64) and tol_p, tol_m, tol_v
    at K = k"""
    b1, b2 = betas
    U = k * 2.0 ** -24
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gm = g * mult
    tol_g = U * (np.abs(gm) + weight_decay * np.abs(p))
    if decoupled:
        g1, p0 = gm, p * (1.0 - lr * weight_decay)
    else:
        g1, p0 = gm + weight_decay * p, p
    m1 = m + (1.0 - b1) * (g1 - m)
    tol_m = U * (np.abs(m) + np.abs(g1)) + (1.0 - b1) * tol_g
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    tol_v = U * v1 + 2.0 * (1.0 - b2) * np.abs(g1) * tol_g
    step_size = lr / (1.0 - b1 ** step)
    bc2sqrt = math.sqrt(1.0 - b2 ** step)
    root = np.sqrt(v1)
    denom = root / bc2sqrt + eps
    dp = step_size * m1 / denom
    with np.errstate(divide="ignore", invalid="ignore"):
        droot = np.where(v1 > 0, np.minimum(tol_v / (2.0 * root), np.sqrt(tol_v)), np.sqrt(tol_v))
    tol_p = U * (np.abs(p) + np.abs(dp)) + step_size * tol_m / denom + np.abs(dp) * droot / (bc2sqrt * denom)
    return dict(p=p0 - dp, m=m1, v=v1, tol_p=tol_p, tol_m=tol_m, tol_v=tol_v)


def ratio(got, want, tol, tol1, what):
    """the largest |got - want| / tol1 (the bound at K = 1) over all elements (0 / 0 = 0); AssertionError when one element
    exceeds tol, the bound at the K under test"""
    got = np.asarray(got, dtype=np.float64).ravel()
    err = np.abs(got - want.ravel())
    tol, tol1 = tol.ravel(), tol1.ravel()
    bad = ~(err <= tol)  # (NaN fails)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the rule; the first at {i}: got "
                             f"{got[i]!r}, {want.ravel()[i]!r} expected, |err| {err[i]:.6g} > bound {tol[i]:.6g}")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / tol1, 0.0)
    return float(r.max()) if r.size else 0.0


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=F32).ravel(), np.ascontiguousarray(want, dtype=F32).ravel()
    bad = got.view(np.uint32) != want.view(np.uint32)
    if got.shape != want.shape or bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements changed their bits; the first at {i}: "
                             f"{got[i]!r} vs {want[i]!r}")


# ---- the norm and the coefficient ------------------------------------------------------------------------------------------
def norm_ref(grads, inv_scale=1.0):
    """(norm in fp64 from the exact squares, its bound) over the gradients that are not None"""
    sq = np.concatenate([g.astype(np.float64).ravel() ** 2 for g in grads if g is not None])
    total = fsum(sq)
    if not math.isfinite(total):
        return total, 0.0
    norm = math.sqrt(total) * inv_scale
    rel = (0.5 * sum_bound(sq) / total if total > 0 else 0.0) + 4 * 2.0 ** -53 + U
    return norm, rel * norm


def check_norm(got, grads, what="last_grad_norm", inv_scale=1.0):
    want, bound = norm_ref(grads, inv_scale)
    got = float(got)
    if not math.isfinite(want):
        if math.isfinite(got):
            raise AssertionError(f"{what}: got {got}, a non-finite norm expected")
        return 0.0
    if not abs(got - want) <= bound:
        raise AssertionError(f"{what}: got {got!r}, {want!r} expected, |err| {abs(got - want):.6g} > bound {bound:.6g}")
    return abs(got - want) / bound if bound > 0 else 0.0


def coef_ref(norm, norm_bound, max_norm=MAX_NORM):
    """(min(1, max_norm / (norm + 1e-6)) in fp64, its bound, whether it must be exactly 1)"""
    raw = max_norm / (norm + 1e-6)
    bound = raw * norm_bound / (norm + 1e-6) + 3 * U * raw
    if raw - bound >= 1.0:
        return 1.0, 0.0, True
    return min(1.0, raw), bound, False


def check_coef(got, grads, what="clip coefficient", max_norm=MAX_NORM):
    norm, nb = norm_ref(grads)
    want, bound, exact = coef_ref(norm, nb, max_norm)
    got = float(got)
    if exact and got != 1.0:
        raise AssertionError(f"{what}: got {got!r} where the norm {norm!r} is below max_norm: exactly 1 expected")
    if not abs(got - want) <= bound:
        raise AssertionError(f"{what}: got {got!r}, {want!r} expected, |err| {abs(got - want):.6g} > bound {bound:.6g}")
    return want


# ---- the driver ------------------------------------------------------------------------------------------------------------
def drive(impl, mode, clip=False, k=K, steps=STEPS):
    """Take `impl` through the STEPS steps of one mode under the rule; the largest err / bound(K = 1) per quantity, dict with
    keys p, m, v (and norm when clipping).  AssertionError at the first violation.
    impl.state() -> [(p, m, v, step)] of the 14 tensors (float32 arrays in the tensors' order; step a number);
    impl.step(grads, lrs) -> None, or (norm, coefficient) when it clips: one optimizer step with these gradients
    (None: no gradient) and the two groups' learning rates."""
    hp = MODES[mode]
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
    before = [tuple(np.array(a, copy=True) for a in s) for s in impl.state()]
    for t in range(steps):
        grads = gradients(t, CLIP_REGIMES[t] if clip else None)
        lrs = tuple(lr_at(t, grp) for grp in (0, 1))
        res = impl.step(grads, lrs)
        mult = 1.0
        if clip:
            norm, coef = res
            worst["norm"] = max(worst["norm"], check_norm(norm, grads, f"{mode} step {t}: norm"))
            check_coef(coef, grads, f"{mode} step {t}: clip coefficient")
            mult = float(F32(coef))  # the implementation's own multiplier, just checked
        after = [tuple(np.array(a, copy=True) for a in s) for s in impl.state()]
        for i, ((p0, m0, v0, s0), (p1, m1, v1, s1), g) in enumerate(zip(before, after, grads)):
            what = f"{mode}{' clipped' if clip else ''} step {t} tensor {i} {TENSORS[i][0]}"
            if g is None:
                for name, a, b in (("p", p0, p1), ("exp_avg", m0, m1), ("exp_avg_sq", v0, v1)):
                    same_bits(b, a, f"{what} (no gradient): {name}")
                if float(s1) != float(s0):
                    raise AssertionError(f"{what} (no gradient): step moved from {float(s0)} to {float(s1)}")
                continue
            if float(s1) != float(s0) + 1.0:
                raise AssertionError(f"{what}: step {float(s1)}, exactly {float(s0) + 1.0} expected")
            args = (p0, g, m0, v0, float(s0) + 1.0, lrs[GROUP_OF[i]], hp["weight_decay"], hp["decoupled"], mult)
            ref, one = adam_f64(*args, k=k), adam_f64(*args, k=1.0)
            worst["m"] = max(worst["m"], ratio(m1, ref["m"], ref["tol_m"], one["tol_m"], f"{what}: exp_avg"))
            worst["v"] = max(worst["v"], ratio(v1, ref["v"], ref["tol_v"], one["tol_v"], f"{what}: exp_avg_sq"))
            worst["p"] = max(worst["p"], ratio(p1, ref["p"], ref["tol_p"], one["tol_p"], f"{what}: parameter"))
        before = after
    return worst


# ---- a kernel in numpy float32, right or wrong ------------------------------------------------------------------------------
MUTANTS = ("no_bias_correction1", "bc2_without_sqrt", "eps_inside_sqrt", "decay_swapped", "clip_not_clamped",
           "mult_on_m_only", "step_not_advanced", "record_of_previous_tensor", "last_block_untouched", "scalar_tail_skipped",
           "no_grad_updated")
MUTANT_NEEDS = {"decay_swapped": ("adam_wd", False), "clip_not_clamped": ("adam", True), "mult_on_m_only": ("adam", True)}


class NumpyKernel:
    """csrc/az_optim.hip restated in numpy float32 (`defect`: one of MUTANTS, None for the kernel as it is)"""

    def __init__(self, mode, clip=False, defect=None):
        self.hp, self.clip, self.defect = MODES[mode], clip, defect
        self.p = initial_params()
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.steps = [0.0] * len(self.p)

    def state(self):
        return list(zip(self.p, self.m, self.v, self.steps))

    def step(self, grads, lrs):
        d, hp = self.defect, self.hp
        mult, res = F32(1), None
        if self.clip:
            total = sum(fsum(g.astype(np.float64) ** 2) for g in grads if g is not None)
            norm = math.sqrt(total)
            coef = MAX_NORM / (norm + 1e-6)
            coef = coef if d == "clip_not_clamped" else min(1.0, coef)
            mult, res = F32(coef), (F32(norm), F32(min(1.0, MAX_NORM / (norm + 1e-6))))
        old_steps = list(self.steps)
        for i, g in enumerate(grads):
            if g is None:
                if d != "no_grad_updated":
                    continue
                g = np.zeros_like(self.p[i])
            step = self.steps[i] + 1.0
            if d != "step_not_advanced":
                self.steps[i] = step
            if d == "record_of_previous_tensor" and i == I_NO_GRAD + 1:
                step = old_steps[I_NO_GRAD] + (0.0 if grads[I_NO_GRAD] is None else 1.0)
            lr, (b1, b2), wd = lrs[GROUP_OF[i]], BETAS, hp["weight_decay"]
            decoupled = hp["decoupled"] != (d == "decay_swapped")
            step_size = F32(lr if d == "no_bias_correction1" else lr / (1.0 - b1 ** step))
            bc2 = 1.0 - b2 ** step
            bc2sqrt = F32(bc2 if d == "bc2_without_sqrt" else math.sqrt(bc2))
            n = g.size
            sel = slice(0, n)
            if d == "last_block_untouched":
                sel = slice(0, n - n % 1024)
            elif d == "scalar_tail_skipped":
                sel = slice(0, n - (n & 3))
            p, m, v, gg = self.p[i][sel], self.m[i][sel], self.v[i][sel], g[sel]
            with np.errstate(all="ignore"):
                gm = gg * mult
                gv = gg if d == "mult_on_m_only" else gm
                if wd != 0.0:
                    if decoupled:
                        p = p * F32(1.0 - lr * wd)
                    else:
                        gm = gm + F32(wd) * p
                        gv = gv + F32(wd) * p
                m = m + F32(1.0 - b1) * (gm - m)
                v = F32(b2) * v + (F32(1.0 - b2) * gv) * gv
                root = np.sqrt(v + F32(EPS)) / bc2sqrt if d == "eps_inside_sqrt" else np.sqrt(v) / bc2sqrt + F32(EPS)
                p = p - (step_size * m) / root
            self.p[i], self.m[i], self.v[i] = self.p[i].copy(), self.m[i].copy(), self.v[i].copy()
            self.p[i][sel], self.m[i][sel], self.v[i][sel] = p, m, v
        return res
