"""numpy restatement of Pillow's 8-bit two-pass BILINEAR resample (ImagingResample: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc), the yardstick of K21
(activezero_amd/csrc/az_resample.hip).  Written from the algorithm; it does not call the library.

    scale = in / out;  fs = max(scale, 1);  support = 1.0 * fs;  ss = 1 / fs;  ksize = (int)ceil(support) * 2 + 1
    per output index xx:  center = (xx + 0.5) * scale
                          first = max((int)(center - support + 0.5), 0);  last = min((int)(center + support + 0.5), in)
                          w[x] = tri((x + first - center + 0.5) * ss), x < count = last - first;  w /= sum(w) unless 0
                          coef[x] = (int)(0.5 + w[x] * 2^22)
    a pass:  v = clip(((1 << 21) + sum_k pixel[first + k] * coef[k]) >> 22, 0, 255)  -- horizontal first, a uint8 image
    between the two passes.
Python floats are IEEE doubles and every step below is one rounded operation, as in C without contraction."""
import math

import numpy as np

BITS = 22

# (Hin, Win) -> (Hout, Wout): the cases of tests/golden/g15_pil_resize.npz
GOLDEN_CASES = (((7, 9), (5, 6)), ((12, 16), (9, 12)), ((5, 5), (11, 13)), ((33, 47), (8, 10)), ((20, 31), (20, 17)),
                ((16, 8), (3, 8)), ((1, 1), (4, 4)), ((9, 13), (1, 1)), ((100, 3), (37, 7)))
STRIPES = np.array([[0, 255, 0, 255, 0, 255, 0, 255]], np.uint8)  # 1 x 8 -> 1 x 6 gives STRIPES_OUT
STRIPES_OUT = np.array([[76, 128, 162, 93, 128, 179]], np.uint8)


MAX_TAPS = 17  # the library's row width at its ratio cap of 8


def ksize(in_size, out_size):
    """Pillow's ksize; the library lays the rows of an axis of at most 17 pixels out with 17 taps where Pillow's ksize is
    larger (count <= in: nothing is lost, and neither pass looks at ksize)"""
    ks = int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1
    return MAX_TAPS if ks > MAX_TAPS and in_size <= MAX_TAPS else ks


def table(in_size, out_size):
    """[out_size, 2 + ksize] int32: first, count, coef[0 .. ksize) -- the layout of az_resample_bilinear_table"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ks = ksize(in_size, out_size)
    out = np.zeros((out_size, 2 + ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)  # int(): C truncation
        last = min(int(center + support + 0.5), in_size)
        w = []
        for x in range(last - first):
            a = abs((x + first - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out[xx, 0], out[xx, 1] = first, last - first
        out[xx, 2:2 + len(w)] = [int(0.5 + v * float(1 << BITS)) for v in w]
    return out


def _pass_columns(img, tab):
    """one pass along the last axis of a uint8 image -> uint8"""
    src = img.astype(np.int64)
    out = np.empty(img.shape[:-1] + (tab.shape[0],), np.uint8)
    for xx in range(tab.shape[0]):
        first, count = int(tab[xx, 0]), int(tab[xx, 1])
        acc = (1 << (BITS - 1)) + src[..., first:first + count] @ tab[xx, 2:2 + count].astype(np.int64)
        out[..., xx] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(img, size):
    """[..., Hin, Win] uint8 -> [..., Hout, Wout] uint8, size = (Hout, Wout): horizontal pass, then vertical"""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    hout, wout = size
    tmp = _pass_columns(img, table(img.shape[-1], wout))
    return np.swapaxes(_pass_columns(np.swapaxes(tmp, -1, -2), table(img.shape[-2], hout)), -1, -2).copy()


def unit(levels):
    """uint8 levels -> what the loader's np.array(img) / 255 becomes as a float32 tensor"""
    return (np.asarray(levels).astype(np.float64) / 255).astype(np.float32)


def make_image(seed, h, w, binary=False):
    rng = np.random.default_rng(1000 + seed)
    if binary:
        return (255 * (rng.random((h, w)) < 0.4)).astype(np.uint8)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)
