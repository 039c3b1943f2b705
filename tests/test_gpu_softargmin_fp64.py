"""GPU: the soft-argmin head -- K6 az_softargmin.hip, forward and backward -- against fp64, element-wise, per depth route and on
both backward paths.

The kernels are called through the C ABI; every output (disparity, saved statistics, grad_logits) lies inside a larger buffer
filled with a NaN sentinel: every output element must be written, nothing around it may be.  The reference and the bounds are
those of tests/_softargmin_fp64ref.py: a closed-form fp64 head and bounds that count the kernel's roundings.  Every check is a
ratio err / bound <= 1.0 over every element; tests/test_softargmin_error_model_cpu.py shows that these checks reject the
defects they are meant to see -- among them the backward kernel's former dead lanes, which read the statistics of pixel
(0, 0, 0) of batch 0 and turned column w - 1 of grad_logits into NaN on the `wide` set at every width with 4 w % 64 != 0.

Per shape and input set: the forward with and without a statistics buffer (the same bits), the saved (M, s) against the
reference, the backward on the saved-statistics path and on the recompute path (stats and disp_fwd both NULL), and the refusal
of one of the two being NULL."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from activezero_amd import _lib, ops  # noqa: E402
from activezero_amd.ops import _call, _p, _stream  # noqa: E402
from tests import _softargmin_fp64ref as SA  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x7FC0BEEF  # a NaN with a payload no arithmetic produces
GUARD = 4096
WORST = {}  # (pass, path, depth route, input set) -> largest ratio


def note(what, path, shape, which, r, capsys):
    key = (what, path, SA.route(shape[1]), which)
    WORST[key] = max(WORST.get(key, 0.0), r)
    with capsys.disabled():
        print(f"\nsoftargmin {what} [{path}] {shape} {which}: {r:.4f}")
    return r


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the shared inputs are read-only


class Guarded:
    """a float32 output of `shape` inside a buffer of NaN sentinels (GUARD elements before and after it), 16-byte aligned as a
    tensor of its own would be"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.out = self.buf[GUARD:GUARD + n].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 0

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())

    def settle(self):
        """the guards are untouched and every output element was written; returns the output as numpy"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all()), "guard band written"
        inner = self.buf[GUARD:GUARD + self.n]
        assert not bool((inner == SENTINEL).any()), f"{int((inner == SENTINEL).sum())} output elements not written"
        return self.out.cpu().numpy()


def bad_columns(grad):
    """the x-cells that hold a non-finite gradient (for the message of a failed check)"""
    return sorted(set(np.nonzero(~np.isfinite(grad))[-1].tolist()))


@functools.lru_cache(maxsize=None)
def device_inputs(shape, which):
    return tuple(dev(t) for t in SA.inputs(shape, which))


def forward(shape, lg, with_stats):
    b, d, h, w = shape
    out = Guarded((b, 4 * h, 4 * w))
    st = Guarded((b, 4 * h, 4 * w, 2)) if with_stats else None
    with torch.cuda.device(DEV):
        _call("az_softargmin_fwd", _p(out.out), _p(st.out) if st else None, _p(lg), b, d, h, w, _stream())
    return out, st


def backward(shape, lg, g, stats, disp):
    b, d, h, w = shape
    gl = Guarded(shape)
    with torch.cuda.device(DEV):
        _call("az_softargmin_bwd", _p(gl.out), _p(g), _p(lg), _p(stats), _p(disp), b, d, h, w, _stream())
    return gl.settle()


def test_shape_list_reaches_every_feature(capsys):
    feats = SA.features()
    with capsys.disabled():
        print("\nreached:", sorted(feats))
    assert SA.WANT <= feats, SA.WANT - feats
    assert {SA.route(s[1]) for s in SA.SHAPES} == {"d == 48 registers", "d == 16 registers", "generic depth"}


@pytest.mark.parametrize("shape", SA.SHAPES, ids=str)
@pytest.mark.parametrize("which", SA.SETS)
def test_forward_statistics_and_both_backward_paths(shape, which, capsys):
    b, d, h, w = shape
    lg, g = device_inputs(shape, which)
    SA.reference(shape, which)                    # on `wide` this asserts that the input arms the dead lanes
    plain, _ = forward(shape, lg, False)
    kept, st = forward(shape, lg, True)
    out, out_kept, stats = plain.settle(), kept.settle(), st.settle()
    assert np.array_equal(out.view(np.uint32), out_kept.view(np.uint32))       # the same bits with and without the statistics
    rs = {k: note(k, "-", shape, which, r, capsys) for k, r in SA.check_forward(shape, which, out_kept, stats).items()}
    saved = backward(shape, lg, g, st.out, kept.out)
    recomputed = backward(shape, lg, g, None, None)
    rs["backward saved"] = note("backward", "saved statistics", shape, which, SA.check_backward(shape, which, saved), capsys)
    rs["backward recompute"] = note("backward", "recompute", shape, which, SA.check_backward(shape, which, recomputed), capsys)
    if which in ("spike", "wide"):
        assert np.isfinite(out).all() and np.isfinite(stats).all()
        assert np.isfinite(saved).all(), f"non-finite grad_logits (saved statistics) in columns {bad_columns(saved)} of {w}"
        assert np.isfinite(recomputed).all(), f"non-finite grad_logits (recompute) in columns {bad_columns(recomputed)} of {w}"
    assert max(rs.values()) <= 1.0, rs
    # one of stats / disp_fwd missing: refused, nothing written
    lib, gl = _lib.lib(), Guarded(shape)
    with torch.cuda.device(DEV):
        assert lib.az_softargmin_bwd(_p(gl.out), _p(g), _p(lg), _p(st.out), None, b, d, h, w, _stream()) == _lib.CONST["AZ_EINVAL"]
        assert lib.az_softargmin_bwd(_p(gl.out), _p(g), _p(lg), None, _p(kept.out), b, d, h, w, _stream()) == _lib.CONST["AZ_EINVAL"]
    assert gl.untouched()


def test_depth_83_is_refused_by_both_entry_points():
    """(54 + 144) d floats of LDS: d == 82 is the largest depth that fits 64 KiB (it is in the shape list)"""
    assert max(s[1] for s in SA.SHAPES) == SA.MAX_D
    b, d, h, w = 1, SA.MAX_D + 1, 1, 3
    src = dev(np.zeros((b, d, 4 * h, 4 * w), dtype=np.float32))
    outs = [Guarded((b, d, 4 * h, 4 * w)) for _ in range(3)]
    lib, code = _lib.lib(), _lib.CONST["AZ_EUNSUPPORTED"]
    with torch.cuda.device(DEV):
        assert lib.az_softargmin_fwd(_p(outs[0].out), _p(outs[1].out), _p(src), b, d, h, w, _stream()) == code
        assert lib.az_softargmin_bwd(_p(outs[2].out), _p(src), _p(src), None, None, b, d, h, w, _stream()) == code
        assert lib.az_softargmin_bwd(_p(outs[2].out), _p(src), _p(src), _p(src), _p(src), b, d, h, w, _stream()) == code
    assert all(o.untouched() for o in outs)


@pytest.mark.parametrize("shape", [(1, 48, 3, 21), (3, 16, 1, 17), (1, 5, 4, 15)], ids=str)
def test_through_autograd(shape, capsys):
    """ops.softargmin: the forward is the C ABI's bits; its gradient (the saved-statistics path, float atomics in any order) is
    within the same bound; [B,1,d,h,w] and [B,d,h,w] logits are one and the same"""
    b, d, h, w = shape
    which = "wide"
    lg, g = device_inputs(shape, which)
    kept, st = forward(shape, lg, True)
    want = kept.settle()
    for view in ((b, d, h, w), (b, 1, d, h, w)):
        x = lg.clone().view(view).requires_grad_()
        out = ops.softargmin(x)
        assert tuple(out.shape) == (b, 1, 4 * h, 4 * w)
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32).reshape(want.shape), want.view(np.uint32))
        out.backward(g.view(b, 1, 4 * h, 4 * w))
        grad = x.grad.cpu().numpy()
        assert np.isfinite(grad).all(), f"non-finite gradient in columns {bad_columns(grad)} of {w}"
        assert note("backward", "autograd", shape, which, SA.check_backward(shape, which, grad), capsys) <= 1.0
    with torch.no_grad():
        out = ops.softargmin(lg)
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(want.shape), want.view(np.uint32))


def test_zz_largest_ratios(capsys):
    """the largest ratio of each check per pass, path, depth route and input set over the cases run"""
    with capsys.disabled():
        print()
        for (what, path, rt, which), r in sorted(WORST.items()):
            print(f"softargmin worst {what:10s} {path:17s} {rt:18s} {which:6s} {r:.3f}" + ("   > 0.5" if r > 0.5 else ""))
    assert all(r <= 1.0 for r in WORST.values())
