"""The optimizer step on this library's kernels (K27 / K28, csrc/az_optim.hip): Adam and AdamW over all tensors of a
parameter group in ONE launch, with clip_grad_norm_, GradScaler's unscale and its skip on non-finite gradients folded in.

    opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-5, max_grad_norm=1.0)
    scaler.scale(loss).backward(); scaler.unscale_(opt); scaler.step(opt); scaler.update()

A step() is, per device: az_grad_sumsq_multi per parameter group (only when a norm is wanted: max_grad_norm, a grad_scale
or a found_inf), then per group az_optim_begin (one workgroup: the norm over ALL groups of the device, the coefficient, the
per-tensor steps and bias corrections) and az_adam_multi -- at most three launches per device and group, two without
clipping or scaling.  What differs from torch:
  * gradients are read only: after the step they are NOT unscaled / clipped in memory (nothing reads them after it);
  * the norm is taken per device (torch's clip_grad_norm_ moves every device's norm to the first one);
  * last_grad_norm is a device scalar (total_norm of clip_grad_norm_, after unscaling): reading it is the caller's sync.
The state keys are torch's (`step` a 0-dim float32 device tensor, `exp_avg`, `exp_avg_sq`), so a state_dict() loads into
torch.optim.Adam / AdamW and the other way round.  There is no fallback: CPU parameters are an error at step().
"""
import numpy as np
import torch

from . import packing, profiler
from ._lib import ADAM_DESC
from .ops import _call, _p, _stream


def adam_tables(rows):
    """launch_tables (packing.py) of az_grad_sumsq_multi / az_adam_multi: one descriptor per tensor, dicts with param, grad,
    exp_avg, exp_avg_sq, step, n; a workgroup takes 256 work items of four floats"""
    return packing.launch_tables(ADAM_DESC, rows, lambda r: (r["n"] + 3) // 4)


class _GroupTable:
    __slots__ = ("descs", "block_desc", "first_block", "nd", "nblocks", "rec", "partial0", "params", "keep", "numel")


class _DeviceTable:
    __slots__ = ("groups", "partials", "head", "nblocks")


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (weight_decay added to the gradient) or, with decoupled_weight_decay, AdamW; max_grad_norm: the
    max_norm of a clip_grad_norm_(all parameters of this optimizer, max_norm) in front of the step, None for none"""

    _step_supports_amp_scaling = True  # GradScaler.step hands over grad_scale / found_inf instead of a host-side check

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False,
                 max_grad_norm=None, **unsupported):
        for name in ("amsgrad", "maximize", "capturable", "differentiable"):
            if unsupported.pop(name, False):
                raise ValueError(f"FusedAdam: {name}=True is not supported (the fused kernels have no such path)")
        for name in ("foreach", "fused"):
            unsupported.pop(name, None)  # (torch's implementation switches: this class is its own implementation)
        if unsupported:
            raise TypeError(f"FusedAdam: unknown arguments {sorted(unsupported)}")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a number (it is read from param_groups at every step, without a sync)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=bool(decoupled_weight_decay),
                        # torch's keys, so that a state_dict() loads into torch.optim.Adam / AdamW and back
                        amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None  # device scalar: the gradients' global norm of the last step (None: no norm was taken)
        self.last_clip_coef = None  # device scalar: min(1, max_grad_norm / (norm + 1e-6)) of the last step
        self.launches = 0           # kernel launches so far (tests)
        self._tables = {}           # key of the (param, grad) addresses -> [(device, _DeviceTable, [group])]
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                self._check_param(p)

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32:
            raise ValueError(f"FusedAdam: parameters must be float32, got {p.dtype}")
        if not p.is_contiguous():
            raise ValueError("FusedAdam: parameters must be contiguous")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):
            self._tables.clear()
        group = self.param_groups[-1]
        for name in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(name, False):
                raise ValueError(f"FusedAdam: {name}=True is not supported (the fused kernels have no such path)")
        for p in group["params"]:
            self._check_param(p)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()
        for group in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name, False):
                    raise ValueError(f"FusedAdam: the loaded state has {name}=True, which is not supported")
            for p in group["params"]:
                st = self.state.get(p)
                if st:  # torch's own Adam may keep `step` on the CPU, or as float64 under another default dtype
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())
                    for k in ("exp_avg", "exp_avg_sq"):
                        st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()

    # -- the device tables of one set of (param, grad) addresses
    def _state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _key(self):
        """the addresses of every parameter that has a gradient, and of that gradient: what a cached table is found by.
        This is the per-step host work, so it does nothing else; _build checks what it describes, once per key."""
        key = []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    key.append(p.data_ptr())
                    key.append(g.data_ptr() if g.layout is torch.strided else -1)
        return tuple(key)

    def _build(self, key):
        """[(device, _DeviceTable, [group])] for the parameters that have a gradient now: checked, their state created, the
        descriptor tables uploaded (the only blocking copies: once per set of addresses)"""
        per_dev = {}
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError(f"FusedAdam.step: parameters must live on the GPU (got {p.device}); the HIP path has "
                                       "no CPU fallback")
                if g.is_sparse or g.layout is not torch.strided:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError(f"FusedAdam.step: a gradient is {g.dtype} on {g.device}, its parameter float32 on {p.device}")
                self._check_param(p)
                if p.numel() == 0:
                    continue
                if not g.is_contiguous():
                    return None  # (made contiguous by the caller, which changes the key)
                groups = per_dev.setdefault(p.device, [])
                if not groups or groups[-1][0] is not group:
                    groups.append((group, []))
                groups[-1][1].append((p, g, self._state(p)))
        entry = []
        for dev, groups in per_dev.items():
            tab = _DeviceTable()
            tab.groups, tab.nblocks = [], 0
            for _, items in groups:
                descs, block_desc, first, nblocks = adam_tables([
                    dict(param=p.data_ptr(), grad=g.data_ptr(), exp_avg=st["exp_avg"].data_ptr(),
                         exp_avg_sq=st["exp_avg_sq"].data_ptr(), step=st["step"].data_ptr(), n=p.numel()) for p, g, st in items])
                gt = _GroupTable()
                gt.descs = torch.from_numpy(descs.view(np.uint8)).to(dev)
                gt.block_desc, gt.first_block = torch.from_numpy(block_desc).to(dev), torch.from_numpy(first).to(dev)
                gt.nd, gt.nblocks, gt.partial0 = len(items), nblocks, tab.nblocks
                gt.rec = torch.empty(2 * len(items), dtype=torch.float32, device=dev)
                gt.params = [p for p, _, _ in items]
                gt.numel = sum(p.numel() for p in gt.params)
                # the state tensors stay alive with the entry: the table holds their addresses
                gt.keep = [(st["exp_avg"], st["exp_avg_sq"], st["step"]) for _, _, st in items]
                tab.groups.append(gt)
                tab.nblocks += nblocks
            tab.partials = torch.empty(tab.nblocks, dtype=torch.float64, device=dev)
            tab.head = torch.zeros(4, dtype=torch.float32, device=dev)
            entry.append((dev, tab, [group for group, _ in groups]))
        if len(self._tables) >= 8:
            self._tables.clear()
        self._tables[key] = entry
        return entry

    def _entry(self):
        key = self._key()
        entry = self._tables.get(key)
        if entry is None:
            entry = self._build(key)
            if entry is None:  # a gradient that is not contiguous: replaced once, then the addresses are new ones
                for group in self.param_groups:
                    for p in group["params"]:
                        if p.grad is not None and not p.grad.is_contiguous():
                            p.grad = p.grad.contiguous()
                key = self._key()
                entry = self._tables.get(key) or self._build(key)
        return entry

    @staticmethod
    def _device_scalar(value, dev):
        """grad_scale / found_inf as a float32 device scalar (GradScaler passes tensors; a number is filled on the device)"""
        if value is None:
            return None
        if isinstance(value, torch.Tensor):
            return value.to(device=dev, dtype=torch.float32, non_blocking=True).reshape(-1)[:1].contiguous()
        return torch.full((1,), float(value), dtype=torch.float32, device=dev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        want_norm = self.max_grad_norm is not None or grad_scale is not None or found_inf is not None
        max_norm = -1.0 if self.max_grad_norm is None else float(self.max_grad_norm)
        for dev, tab, groups in self._entry():
            scale_t, inf_t = self._device_scalar(grad_scale, dev), self._device_scalar(found_inf, dev)
            with torch.cuda.device(dev):
                stream = _stream()
                if want_norm:
                    with profiler.scope("grad_sumsq", bytes=4.0 * sum(gt.numel for gt in tab.groups), bound="hbm"):
                        for gt in tab.groups:
                            _call("az_grad_sumsq_multi", tab.partials.data_ptr() + 8 * gt.partial0, _p(gt.descs),
                                  _p(gt.block_desc), _p(gt.first_block), gt.nd, gt.nblocks, stream)
                            self.launches += 1
                for group, gt in zip(groups, tab.groups):
                    lr, (beta1, beta2) = group["lr"], group["betas"]
                    if isinstance(lr, torch.Tensor):
                        raise RuntimeError("FusedAdam.step: lr must be a number, not a tensor (reading it would synchronise)")
                    _call("az_optim_begin", _p(tab.head), _p(gt.rec), _p(gt.descs), gt.nd,
                          _p(tab.partials) if want_norm else None, tab.nblocks if want_norm else 0, _p(scale_t), _p(inf_t),
                          float(lr), float(beta1), float(beta2), max_norm, stream)
                    with profiler.scope("adam", bytes=28.0 * gt.numel, bound="hbm"):
                        _call("az_adam_multi", _p(gt.descs), _p(gt.block_desc), _p(gt.first_block), gt.nd, gt.nblocks,
                              _p(tab.head), _p(gt.rec), float(lr), float(beta1), float(beta2), float(group["eps"]),
                              float(group["weight_decay"]), int(bool(group.get("decoupled_weight_decay", self.defaults["decoupled_weight_decay"]))),
                              int(want_norm), stream)
                    self.launches += 2
                    # the kernel wrote through raw pointers: the packed weight images and the inference memo are keyed on
                    # the version counters (packing.py)
                    packing.touched(*gt.params)
            if want_norm:
                self.last_grad_norm, self.last_clip_coef = tab.head[0], tab.head[3]
            else:
                self.last_grad_norm = self.last_clip_coef = None
        return loss


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: the decay multiplies the parameter (p *= 1 - lr * weight_decay) and stays out of the moments"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, **kw):
        kw.pop("decoupled_weight_decay", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True,
                         max_grad_norm=max_grad_norm, **kw)
