"""Cache coherence: one rule for every host-side table that stands between a parameter and a launch.

Between an nn.Parameter and the bytes a kernel reads there are about ten tables keyed by (address, version counter):
packing.PACK_CACHE / AFFINE_CACHE, conv2d._PACK2D_CACHE, costconv._MERGED_CACHE, amax._W_AMAX with the persistent rows of
prime_weight_amax, packing.PackPlan, and the ConvGRU's _PACK_CACHE / _CTX_CACHE / _ROWS_CACHE / _SEEN_ONCE.  A stale hit
launches a correct kernel on yesterday's weights and raises nothing.

THE RULE (no tolerance): after a write, the next call is bit-equal to the same call with nothing remembered -- every table
emptied, a fresh PackPlan, and a copy.deepcopy of the module (new addresses, same values).  Train-mode calls compare what
the launch was handed (image and amax array) with the per-tensor packer and a fresh az_absmax on the current weight
instead: their outputs pass through float atomics.  Every case must be able to fail: the fresh answers before and after
the write must differ, or the case proves nothing and is refused.

A `Site` is one small call through a public entry point; a `Write` is one way a user changes parameters.  `check` holds a
site to the rule for a write, `check_recycled` for an address handed from one parameter to another.
tests/test_cache_keys_cpu.py proves on toy sites that each check can fail; tests/test_gpu_cache_coherence.py runs the real ones.
"""
import contextlib
import copy

import torch

BN = (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)
CONV = (torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.ConvTranspose3d)


# ---- nothing remembered ---------------------------------------------------------------------------------------------------
def tables():
    """(module, attribute) of every dict the rule empties"""
    from activezero_amd import amax, conv2d, costconv, packing
    from activezero_amd.nets.raft import gru
    return [(packing, "PACK_CACHE"), (packing, "AFFINE_CACHE"), (conv2d, "_PACK2D_CACHE"), (costconv, "_MERGED_CACHE"),
            (amax, "_W_AMAX"), (amax, "_PRIME_ROWS"), (gru, "_PACK_CACHE"), (gru, "_CTX_CACHE"), (gru, "_ROWS_CACHE"),
            (gru, "_SEEN_ONCE"), (packing, "_PLANS")]  # (_PLANS empty: the next pack_plan() is a fresh PackPlan)


@contextlib.contextmanager
def nothing_remembered(monkeypatch):
    """inside: every table is empty and the pack plan is new; afterwards: what was remembered before is back"""
    from activezero_amd import amax
    with monkeypatch.context() as m:
        for mod, name in tables():
            m.setattr(mod, name, {})
        m.setattr(amax, "_PRIME", amax.MultiAbsmax())
        yield


# ---- sites ------------------------------------------------------------------------------------------------------------------
class Site:
    """name; make(device) -> (module, inputs); call(module, inputs) -> tuple of tensors (inputs are never written);
    weight(module) -> (owning module, attribute name) of the weight the recycled-address construction replaces;
    fresh(module, inputs) -> the same tuple with nothing remembered (default: call on a deepcopy -- train-mode sites give the
    per-tensor packer's bytes instead); train(module, inputs): a train-mode call that moves the running statistics"""

    def __init__(self, name, make, call, weight=None, fresh=None, train=None, skip=()):
        self.name, self.make, self.call, self.weight, self._fresh, self.train = name, make, call, weight, fresh, train
        self.skip = tuple(skip)  # names of writes that have no meaning here

    def __repr__(self):
        return self.name

    def fresh(self, module, inputs, monkeypatch):
        with nothing_remembered(monkeypatch):
            if self._fresh is not None:
                return _tuple(self._fresh(module, inputs))
            return _tuple(self.call(copy.deepcopy(module), inputs))


def _tuple(y):
    return tuple(t.detach().clone() for t in (y if isinstance(y, (tuple, list)) else (y,)))


def same(a, b):
    """bit-equal tuples of tensors (NaN-safe: compared as integers)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        x, y = x.contiguous(), y.contiguous()
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            return False
    return True


# ---- writes -----------------------------------------------------------------------------------------------------------------
def changes(module):
    """[(owner module, attribute, op, constant, is_parameter)]: writes that are certain to move the answer -- weights x 1.5,
    biases + 0.25, gamma x 1.5, beta + 0.25, running_mean + 0.25, running_var x 2"""
    out = []
    for m in module.modules():
        if isinstance(m, BN):
            out += [(m, "weight", "mul", 1.5, True), (m, "bias", "add", 0.25, True),
                    (m, "running_mean", "add", 0.25, False), (m, "running_var", "mul", 2.0, False)]
        elif isinstance(m, CONV) or getattr(m, "cache_coherence_weight", False):
            out.append((m, "weight", "mul", 1.5, True))
            if getattr(m, "bias", None) is not None:
                out.append((m, "bias", "add", 0.25, True))
    return [c for c in out if getattr(c[0], c[1], None) is not None]


def _new(t, op, c):
    return (t.detach() * c) if op == "mul" else (t.detach() + c)


def _inplace(t, op, c):
    return t.mul_(c) if op == "mul" else t.add_(c)


def w_inplace(module, device):
    with torch.no_grad():
        for m, a, op, c, _ in changes(module):
            _inplace(getattr(m, a), op, c)


def _grads(module):
    ps = [p for p in module.parameters()]
    for i, p in enumerate(ps):
        g = torch.ones_like(p)
        g.view(-1)[i % 2::2] = -1.0  # (both signs: Adam's first step moves every element by +-lr)
        p.grad = g
    return ps


def w_adam(module, device):
    torch.optim.Adam(_grads(module), lr=0.05).step()


def w_fused_adam(module, device):
    from activezero_amd import optim
    optim.FusedAdam(_grads(module), lr=0.05).step()


def w_load_state_dict(module, device):
    sd = {k: v.clone() for k, v in module.state_dict().items()}
    names = {id(m): n for n, m in module.named_modules()}
    for m, a, op, c, _ in changes(module):
        key = (names[id(m)] + "." if names[id(m)] else "") + a
        sd[key] = _new(sd[key], op, c)
    module.load_state_dict(sd)


def w_data_copy_touched(module, device):
    from activezero_amd import packing
    for m, a, op, c, _ in changes(module):
        t = getattr(m, a)
        t.data.copy_(_new(t, op, c))
        packing.touched(t)


def w_data_mul_touched(module, device):
    from activezero_amd import packing
    for m, a, op, c, _ in changes(module):
        t = getattr(m, a)
        _inplace(t.data, op, c)
        packing.touched(t)


def w_data_assign(module, device):
    for m, a, op, c, _ in changes(module):
        t = getattr(m, a)
        t.data = _new(t, op, c)


def w_vector_to_parameters(module, device):
    new = {id(getattr(m, a)): _new(getattr(m, a), op, c) for m, a, op, c, is_p in changes(module) if is_p}
    ps = list(module.parameters())
    vec = torch.cat([new.get(id(p), p.detach()).reshape(-1) for p in ps])
    torch.nn.utils.vector_to_parameters(vec, ps)


def w_cpu_and_back(module, device):
    """module.cpu(), new values assigned there, module.to(device): the device storage is freed and allocated again"""
    module.cpu()
    w_data_assign(module, device)
    module.to(device)


def w_bn_eps(module, device):
    for m in module.modules():
        if isinstance(m, BN):
            assert m.eps == 1e-5
            m.eps = 1e-3


def _scale_weights(module, c):
    with torch.no_grad():
        for m, a, _op, _c, is_p in changes(module):
            if a == "weight" and not isinstance(m, BN):
                getattr(m, a).mul_(c)


def w_amax_up(module, device):
    """max |w| four times larger: a stale amax would clip the f16x3 operands (the image's bytes do not move: only the amax
    array and the output tell)"""
    _scale_weights(module, 4.0)


def w_amax_down(module, device):
    """max |w| 2^-10 of what it was: a stale amax would throw ten of the operands' bits away"""
    _scale_weights(module, 2.0 ** -10)


def has_bn(module):
    return any(isinstance(m, BN) for m in module.modules())


WRITES = {  # name -> (function, needs a BatchNorm)
    "inplace_no_grad": (w_inplace, False),
    "adam_step": (w_adam, False),
    "fused_adam_step": (w_fused_adam, False),
    "load_state_dict": (w_load_state_dict, False),
    "data_copy_touched": (w_data_copy_touched, False),
    "data_mul_touched": (w_data_mul_touched, False),
    "data_assign": (w_data_assign, False),
    "vector_to_parameters": (w_vector_to_parameters, False),
    "cpu_and_back": (w_cpu_and_back, False),
    "bn_eps": (w_bn_eps, True),
    "amax_up_x4": (w_amax_up, False),
    "amax_down_x2pow-10": (w_amax_down, False),
}


# ---- the checks -------------------------------------------------------------------------------------------------------------
def check(site, write, device, monkeypatch, between=None):
    """the rule for one site and one write (a function of (module, device)); `between`: run after the write and before the
    call under test (eviction)"""
    with nothing_remembered(monkeypatch):
        module, inputs = site.make(device)
        before = site.fresh(module, inputs, monkeypatch)
        warm = _tuple(site.call(module, inputs))
        if site._fresh is None:
            assert same(warm, before), f"{site}: the first call differs from a call with nothing remembered"
            assert same(_tuple(site.call(module, inputs)), warm), f"{site}: the remembered call differs from the first"
        write(module, device)
        if between is not None:
            between()
        got = _tuple(site.call(module, inputs))
        after = site.fresh(module, inputs, monkeypatch)
        assert not same(before, after), f"{site}: this write does not change the answer, the case cannot fail"
        assert same(got, after), f"{site}: stale after the write -- the call differs from one with nothing remembered"
        if site._fresh is None:
            assert same(_tuple(site.call(module, inputs)), after), f"{site}: the second call after the write differs"


def check_unchanged(site, device, monkeypatch, between):
    """no write, but `between` (an eviction) runs between two calls: the answer stays what it was"""
    with nothing_remembered(monkeypatch):
        module, inputs = site.make(device)
        warm = _tuple(site.call(module, inputs))
        between()
        got = _tuple(site.call(module, inputs))
        assert same(got, warm), f"{site}: the answer moved across an eviction"
        assert same(got, site.fresh(module, inputs, monkeypatch)), f"{site}: differs from a call with nothing remembered"


def rebase(site, module, buf):
    """the site's weight becomes a parameter that is a view of the caller-owned buffer `buf` (which holds its values)"""
    owner, attr = site.weight(module)
    old = getattr(owner, attr)
    p = torch.nn.Parameter(buf[:old.numel()].view(old.shape), requires_grad=old.requires_grad)
    setattr(owner, attr, p)
    return p


def check_recycled(site, device, monkeypatch, prepare=None):
    """A recycled address, constructed: parameter A is a view of a caller-owned buffer and is remembered; `A.data =
    elsewhere`; the buffer gets new values; parameter B is a view of the same buffer -- same address, same version counter
    value.  The site on B must use B's values, and on A, again, A's.  `prepare(module)`: run before each call under test
    (PackPlan: prepack of that module's weights)"""
    with nothing_remembered(monkeypatch):
        mod_a, inputs = site.make(device)
        owner, attr = site.weight(mod_a)
        w0 = getattr(owner, attr).detach().clone()
        buf = torch.empty(w0.numel() + 64, dtype=w0.dtype, device=device)  # the caller's buffer
        buf[:w0.numel()] = w0.reshape(-1)
        a = rebase(site, mod_a, buf)
        assert a.data_ptr() == buf.data_ptr()
        if prepare is not None:
            prepare(mod_a)
        site.call(mod_a, inputs)  # remembered (twice: a planned route needs the second call)
        site.call(mod_a, inputs)
        ptr, version = a.data_ptr(), a._version
        a.data = a.detach().clone()                  # A moves elsewhere; nothing bumps its counter
        buf.data[:w0.numel()] = (w0 * 1.5).reshape(-1)   # new values at the old address
        mod_b = copy.deepcopy(mod_a)
        b = rebase(site, mod_b, buf)
        assert b.data_ptr() == ptr and b._version == version and a.data_ptr() != ptr and a._version == version
        for who, mod in (("B", mod_b), ("A", mod_a), ("B again", mod_b)):
            if prepare is not None:
                prepare(mod)
            got = _tuple(site.call(mod, inputs))
            want = site.fresh(mod, inputs, monkeypatch)
            assert same(got, want), f"{site}: {who} at a recycled address was answered with another tensor's entry"
        assert not same(site.fresh(mod_a, inputs, monkeypatch), site.fresh(mod_b, inputs, monkeypatch)), \
            f"{site}: A and B give the same answer, the case cannot fail"
