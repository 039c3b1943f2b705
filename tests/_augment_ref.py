"""numpy fp64 restatement of the reference's data_augmentation (datasets/dataset_utils.py:49-83) as its loader applies it
(datasets/messytable.py:264-280, 402-404), the per-element error bound of K20 (az_augment.hip) against it, and an fp32
emulation of the kernel's documented structure.  Shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py; a
helper module, not a conftest.  Only tests/ may import this file.

PARITY UNPINNED for torchvision: the transform is torchvision's GaussianBlur, ColorJitter, ToTensor and Normalize
(torchvision 0.9-0.11), a third-party dependency that is absent here, and the reference holds no fixture for it.  It is
restated from its published definition.  The reference feeds it np.array(img) / 255, a float64 [H,W,3] array of three equal
channels; ToTensor does not rescale a non-uint8 array and the result is cast to float32 only at the end, so fp64 IS the
reference's arithmetic:
    GaussianBlur   t = linspace(-(ks-1)/2, (ks-1)/2, ks), k = exp(-0.5 (t / sigma)^2), k /= k.sum(); the 2-D kernel is
                   outer(k, k); the image is padded by ks // 2 with mode="reflect" (the edge pixel is not repeated) and
                   correlated with it
    ColorJitter    brightness=[b,b], contrast=[c,c], saturation and hue off; the two adjustments run in a random order
                   per call.  brightness: clamp(b x, 0, 1).  contrast: m = mean over the image of 0.2989 r + 0.587 g +
                   0.114 b (the weights sum to 0.9999), clamp(c x + (1 - c) m, 0, 1), m taken of the image as it stands
    Normalize      (x - mean[ch]) / std[ch], ImageNet constants

THE BOUND (bound() below), u = 2^-24, counted per expression of the kernel, never fitted to an output.  x >= 0 everywhere,
so a partial sum never exceeds the finished one and every rounding of an accumulation is at most u times the finished value.
    input          1   a uint8 level becomes fl(v / 255); the restatement takes v / 255 in fp64 (0 for a float32 image)
    blur           2 ks + 2   V = the exact blurred value: the fp32 tap of either pass (the fp64 taps are rounded once: 2),
                   ks fused multiply-adds per pass (2 ks).  E_V = (2 ks + 2 + input) u V          ks = 9: 21 u V
    brightness     fl(b x): E <- b E + u b x                       (clamp is 1-Lipschitz and adds nothing)
    mean           per pixel the three-term grey value: the three fp32 weights and three roundings, 4 u g (the first
                   product's weight and rounding, then two fused steps whose weights are the other two: u (0.9999 x) for the
                   weights in all, 3 u g for the roundings); the tile sum: 8 values per thread one after the other, 6
                   butterfly steps, 3 adds over the waves = 17 u S; the tiles are added in fp64; the mean is rounded to fp32
                   once.  E_m = mean(E_x) + (4 + 17 + 1) u m = mean(E_x) + 22 u m
    contrast       fl(1 - c), its product with m, the fused c x + p: E <- |c| E + |1 - c| E_m + 2 u |1 - c| m + u |t|, t the
                   value before the clamp
    normalise      the fp32 constants (the restatement's are fp64: u mean, u |q| for std), the subtraction u |x - mean|,
                   the division u |q|:   E_out = (E + u mean + u |x - mean|) / std + 2 u |q|
All of it times SLACK = 1.001 for the second-order terms and the restatement's own fp64 error.  At b = 1.4, c = 1.2, ks = 9
and a pixel near 1 this is 30.8 u after brightness, about 43 u after contrast, 2.6e-6, and 1.2e-5 after the division by std.

Measured here (tests/test_augment_cpu.py prints them): the fp32 emulation below against the restatement, over the sizes
5 x 7 to 135 x 240, sigma 0.1 - 2.0, both orders, the four flag combinations, uint8 and float32 input.  With both stages on
its largest absolute difference per case is 2.9e-7 .. 1.4e-6 and its ratio to the bound 0.03 .. 0.21: the bound is the worst
case of 2 ks roundings of one sign, the emulation's accumulate like a random walk.  With both stages off only three or four
roundings are left and the ratio reaches EMU_WORST_RATIO = 0.67, the worst over all cases."""
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.001
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
TW, TH = 64, 32  # the kernel's tile (AUG_TW, AUG_TH)
# the cases of tests/test_gpu_augment.py: (H, W), ks, the generator seeds of the batch
CASES = (((5, 7), 9, (0,)), ((24, 29), 9, (0,)), ((40, 64), 9, (0,)), ((37, 53), 9, (0,)), ((16, 200), 31, (0,)),
         ((67, 93), 9, (0, 1, 2)), ((135, 240), 9, (0, 1)))
EMU_WORST_RATIO = 0.67  # a record of this module's emulation (see above), not a tolerance


def reflect(i, n):
    """"reflect" padding index (one reflection: -n < i < 2n - 1): the edge pixel is not repeated"""
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def weights(ks, sigma):
    t = np.linspace(-(ks - 1) / 2, (ks - 1) / 2, ks)
    k = np.exp(-0.5 * (t / sigma) ** 2)
    return k / k.sum()


def gaussian_blur(img, ks, sigma):
    """the 2-D kernel outer(k, k) correlated with the reflect-padded image: a double loop over taps"""
    h, w = img.shape
    r = ks // 2
    assert ks % 2 == 1 and h > r and w > r
    k1 = weights(ks, sigma)
    k2 = np.outer(k1, k1)
    pad = np.pad(np.asarray(img, dtype=np.float64), r, mode="reflect")
    out = np.zeros((h, w))
    for dy in range(ks):
        for dx in range(ks):
            out += k2[dy, dx] * pad[dy:dy + h, dx:dx + w]
    return out


def grey_mean(x):
    return float(np.mean(0.2989 * x + 0.587 * x + 0.114 * x))


def adjust_brightness(x, b):
    return np.clip(b * x, 0.0, 1.0)


def adjust_contrast(x, c):
    return np.clip(c * x + (1.0 - c) * grey_mean(x), 0.0, 1.0)


def normalise(x):
    return np.stack([(x - MEAN[ch]) / STD[ch] for ch in range(3)])


def unit(img):
    """the grey image in [0,1] as the reference sees it: uint8 levels / 255 in fp64, a float image as it is"""
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def augment(img, sigma=None, b=None, c=None, contrast_first=False, ks=9, stages=None):
    """[3,H,W] fp64.  sigma None: no blur; b, c None: no jitter.  Parameters are taken as the fp32 values the device holds.
    `stages`, a dict, receives the values before each clamp ("pre") and the intermediate images."""
    x = unit(img)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    if sigma is not None:
        x = gaussian_blur(x, ks, f32(sigma))
    pre = []
    if b is not None:
        b, c = f32(b), f32(c)
        for what in (("c", "b") if contrast_first else ("b", "c")):
            t = b * x if what == "b" else c * x + (1.0 - c) * grey_mean(x)
            pre.append(t)
            x = np.clip(t, 0.0, 1.0)
    if stages is not None:
        stages["pre"] = pre
    return normalise(x)


def clamp_shares(img, sigma, b, c, contrast_first, ks=9):
    """(share of pixels some clamp cut at 1, share some clamp cut at 0)"""
    st = {}
    augment(img, sigma, b, c, contrast_first, ks, st)
    hi = np.zeros(np.shape(img), bool)
    lo = np.zeros(np.shape(img), bool)
    for t in st["pre"]:
        hi |= t > 1.0
        lo |= t < 0.0
    return hi.mean(), lo.mean()


def bound(img, sigma=None, b=None, c=None, contrast_first=False, ks=9):
    """[3,H,W] per-element bound on |kernel - augment(...)|, from the module docstring"""
    x = unit(img)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    e = U * x if np.asarray(img).dtype == np.uint8 else np.zeros_like(x)
    if sigma is not None:
        x = gaussian_blur(x, ks, f32(sigma))
        e = gaussian_blur(e, ks, f32(sigma)) + (2 * ks + 2) * U * x
    if b is not None:
        b, c = f32(b), f32(c)
        for what in (("c", "b") if contrast_first else ("b", "c")):
            if what == "b":
                t = b * x
                e = abs(b) * e + U * np.abs(t)
            else:
                m = grey_mean(x)
                e_m = float(np.mean(e)) + 22 * U * abs(m)
                t = c * x + (1.0 - c) * m
                e = abs(c) * e + abs(1.0 - c) * e_m + 2 * U * abs((1.0 - c) * m) + U * np.abs(t)
            x = np.clip(t, 0.0, 1.0)
    out = []
    for ch in range(3):
        q = (x - MEAN[ch]) / STD[ch]
        out.append((e + U * MEAN[ch] + U * np.abs(x - MEAN[ch])) / STD[ch] + 2 * U * np.abs(q))
    return np.stack(out) * SLACK


def ratio(got, img, sigma=None, b=None, c=None, contrast_first=False, ks=9):
    """(largest |got - restatement| / bound, largest |got - restatement|); a non-finite output is ratio inf"""
    got = np.asarray(got, dtype=np.float64)
    want = augment(img, sigma, b, c, contrast_first, ks)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf"), float("inf")
    err = np.abs(got - want)
    return float((err / bound(img, sigma, b, c, contrast_first, ks)).max()), float(err.max())


def make_image(seed, h, w):
    """The input generator: 8 x 8 blocks of random level (they survive the blur, so both clamps are exercised), 6 % dots,
    a little noise; uint8 [h,w]."""
    rng = np.random.default_rng(200 + seed)
    blocks = rng.random((math.ceil(h / 8), math.ceil(w / 8)))
    base = np.kron(blocks, np.ones((8, 8)))[:h, :w]
    dots = (rng.random((h, w)) < 0.06) * rng.uniform(0.2, 0.5, (h, w))
    return np.rint(255 * np.clip(0.02 + 0.96 * base + dots + rng.normal(0, 0.01, (h, w)), 0, 1)).astype(np.uint8)


# ---- fp32 emulation of the kernel's documented structure (numpy; independent of the HIP code) ----------------------------
F = np.float32


def _fma(a, b, c):
    """fp32 fused multiply-add through fp64 (the product of two floats is exact in fp64)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _clamp(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def emu_unit(img):
    img = np.asarray(img)
    return img.astype(F) / F(255) if img.dtype == np.uint8 else img.astype(F)


def emu_blur(x, ks, sigma, mutant=None):
    """two 1-D passes of fused multiply-adds with the fp64 taps rounded to fp32 once; horizontal first"""
    h, w = x.shape
    r = ks // 2
    sigma = float(F(sigma))
    if sigma <= 0:
        return x
    t = np.arange(ks, dtype=np.float64) - r
    k = np.exp(-0.5 * (t / sigma) ** 2)
    taps = (k if mutant == "weights_not_normalised" else k / k.sum()).astype(F)
    pad = np.pad(x, r, mode="edge" if mutant == "edge_repeated" else "reflect")
    rows = np.zeros((h + 2 * r, w), F)
    for j in range(ks):
        term = pad[:, j:j + w]
        if mutant == "seam_tap_dropped" and j == 0:
            term = term.copy()
            term[:, TW::TW] = 0  # the first column of every tile but the left-most misses its left-most tap
        rows = _fma(taps[j], term, rows)
    if mutant == "horizontal_only":
        return rows[r:r + h]
    out = np.zeros((h, w), F)
    for j in range(ks):
        out = _fma(taps[j], rows[j:j + h], out)
    return out


def emu_mean(x, mutant=None):
    """one fp32 sum per 64 x 32 tile of the three-term grey value, the tiles added in slot order in fp64, rounded once"""
    h, w = x.shape
    if mutant == "grey_weights_sum_to_one":
        g = x
    else:
        g = _fma(F(0.114), x, _fma(F(0.587), x, F(0.2989) * x))
    parts = [np.sum(g[y:y + TH, c:c + TW], dtype=F) for y in range(0, h, TH) for c in range(0, w, TW)]
    if mutant == "tile_dropped":
        parts = parts[:-1]
    total = 0.0
    for p in parts:
        total += float(p)
    return F(total / (h * w))


def emulate(img, sigma=None, b=None, c=None, contrast_first=False, ks=9, mutant=None, other=None):
    """[3,H,W] fp32 as the kernel documents its arithmetic.  `other`: another image of the batch (mutant "mean_of_other")"""
    x = emu_unit(img)
    if sigma is not None:
        x = emu_blur(x, ks, sigma, mutant)
    if b is not None:
        b, c = F(b), F(c)
        if mutant == "orders_swapped":
            contrast_first = not contrast_first
        bright = lambda v: (b * v if mutant == "no_high_clamp" else                      # noqa: E731
                            np.minimum(b * v, F(1)) if mutant == "no_low_clamp" else _clamp(b * v))

        def contrast(v, src):
            m = emu_mean(src, mutant)
            t = _fma(c, v, (F(1) - c) * m)
            return (np.maximum(t, F(0)) if mutant == "no_high_clamp" else
                    np.minimum(t, F(1)) if mutant == "no_low_clamp" else _clamp(t))

        src = None
        if mutant == "mean_of_other":
            src = emu_unit(other) if sigma is None else emu_blur(emu_unit(other), ks, sigma)
        if contrast_first:
            x = bright(contrast(x, x if src is None else src))
        else:
            y = bright(x)
            if mutant == "mean_before_brightness":
                src = x
            elif src is not None:
                src = bright(src)
            x = contrast(y, y if src is None else src)
    mean, std = (MEAN, STD) if mutant != "channels_permuted" else (MEAN[::-1], STD[::-1])
    return np.stack([(x - F(mean[ch])) / F(std[ch]) for ch in range(3)])
