"""What tests/test_gpu_nonfinite.py asserts with (CPU only): the class of every element -- finite, NaN, +inf, -inf -- of a
kernel's output against the class of the same operation evaluated by torch in fp64, equality of bits where an output read
nothing that was poisoned, and which outputs of a convolution read a poisoned input element.  There is no tolerance here:
every assertion is equality of class maps or equality of bits.

The rule the kernels are held to (include/azhip.h, "Non-finite values"): a NaN read by an output is a NaN in that output,
through every fused activation; what an inf becomes is the reference's point-wise result."""
import torch

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
NAMES = ("finite", "nan", "+inf", "-inf")


def classes(t):
    """int8 map of t: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    t = t.detach()
    m = torch.zeros(t.shape, dtype=torch.int8, device=t.device)
    m[torch.isnan(t)] = NAN
    m[t == float("inf")] = PINF
    m[t == float("-inf")] = NINF
    return m


def counts(m):
    """elements per class of a class map, in the order of NAMES"""
    return [int((m == k).sum()) for k in range(4)]


def _fmt(c):
    return " ".join(f"{n} {v}" for n, v in zip(NAMES, c))


def same_classes(got, ref64, what):
    """prints the count of each class on both sides, then asserts that the class maps are equal"""
    assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    a, b = classes(got).cpu(), classes(ref64).cpu()
    print(f"\n  {what}: got [{_fmt(counts(a))}]  fp64 [{_fmt(counts(b))}]", end="")
    bad = a != b
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ in class; the first at {i}: got {NAMES[int(a[i])]} "
                             f"({float(got[i])}), fp64 {NAMES[int(b[i])]} ({float(ref64[i])})")


def all_nan(got, where, what):
    """prints how many of the elements selected by `where` (a bool map that broadcasts against got) are NaN, then asserts
    that all are"""
    sel = torch.isnan(got.detach().cpu())[where.expand(got.shape)]
    print(f"\n  {what}: {int(sel.sum())} of {sel.numel()} outputs that read a NaN are NaN", end="")
    assert sel.numel() > 0, what
    assert bool(sel.all()), f"{what}: {int((~sel).sum())} of {sel.numel()} outputs that read a NaN are not NaN"


def untouched(got, clean, keep, what):
    """the elements selected by `keep` (a bool map that broadcasts against got) hold the bits of `clean`: the same launch
    on the unpoisoned operands"""
    assert got.shape == clean.shape and got.dtype == clean.dtype == torch.float32, what
    keep = keep.expand(got.shape)
    assert bool(keep.any()), f"{what}: nothing is left to compare"
    a = got.detach().cpu().contiguous().view(torch.int32)[keep]
    b = clean.detach().cpu().contiguous().view(torch.int32)[keep]
    assert not bool(torch.isnan(clean).any()), f"{what}: the clean launch holds a NaN"
    n = int((a != b).sum())
    print(f"\n  {what}: {a.numel() - n} of {a.numel()} elements that read nothing poisoned hold the clean launch's bits", end="")
    assert n == 0, f"{what}: {n} of {a.numel()} elements that read nothing poisoned differ from the clean launch"


def reads(mask_in, fn):
    """the outputs that read a poisoned input element: fn(mask_in.double(), ones_weight) > 0.  mask_in: bool [B,1,*spatial],
    true where ANY channel of the input is poisoned; fn(x, w): the fp64 torch operator of the layer with its stride and
    padding (F.conv3d, F.conv_transpose3d, F.conv2d); the weight is one 3 x .. x 3 tap block of ones (one channel in, one
    out).  Returns bool [B,1,*output spatial]: it holds for every output channel."""
    ones = torch.ones((1, 1) + (3,) * (mask_in.dim() - 2), dtype=torch.float64)
    return fn(mask_in.double().cpu(), ones) > 0


def finite_amax(t):
    """the largest finite magnitude of t: what an amax array holds (csrc/az_common.h az_finite_abs_bits)"""
    a = t.detach().abs()
    return float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max())
