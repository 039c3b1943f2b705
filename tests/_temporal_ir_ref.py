"""numpy fp64 restatement of the reference's temporal IR pattern, tools/temporal_ir.py:91-114 with its helper
get_smoothed_ir_pattern (:35-40): the yardstick of K17 (az_temporal_ir.hip).  Written from the text -- the tool itself
cannot be imported (argparse runs at import; cv2 and matplotlib are absent).

PARITY UNPINNED for cv2: the helper's arithmetic is cv2.blur(diff, (ks, ks)) (opencv-python 4.5.x), a third-party
dependency that is absent here, and the reference holds no fixture for it.  cv2.blur is restated from its published
definition: the NORMALISED ks x ks box filter, anchor at the centre, default border BORDER_REFLECT_101 (index -i -> i,
n-1+i -> n-1-i: the edge pixel is not repeated).  Everything else (line fit, end-point difference, min-max
normalisation, threshold) is the reference's own numpy code.  Only tests/ may import this file."""
import numpy as np


def fit_diff(stack):
    """temporal_ir.py:93-111 for a [T,H,W] stack: |fit[T-1] - fit[0]| / 255 per pixel, before normalisation"""
    y = np.moveaxis(np.asarray(stack, dtype=np.float64), 0, -1)  # [H,W,D] like img_temp
    d = y.shape[-1]
    x = np.broadcast_to(np.linspace(0, d - 1, num=d, dtype=int).reshape(1, 1, -1), y.shape)
    x_avg = np.average(x, axis=-1)[..., None]
    y_avg = np.average(y, axis=-1)[..., None]
    numerator = np.sum((y - y_avg) * (x - x_avg), axis=-1)
    denominator = np.sum((x - x_avg) ** 2, axis=-1)
    slope = (numerator / denominator)[..., None]
    intercept = y_avg - slope * x_avg
    fit = slope * x + intercept
    return np.abs((fit[..., -1] - fit[..., 0]) / 255)


def reflect101(i, n):
    """BORDER_REFLECT_101 index (one reflection: -n < i < 2n - 1)"""
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def box_blur(img, ks):
    """normalised ks x ks box filter with reflect-101 borders, separably: row sums, then column sums, / ks^2"""
    h, w = img.shape
    r = ks // 2
    assert ks % 2 == 1 and h > r and w > r
    pad = np.pad(np.asarray(img, dtype=np.float64), r, mode="reflect")  # numpy's "reflect" does not repeat the edge
    rows = sum(pad[:, k:k + w] for k in range(ks))
    return sum(rows[k:k + h] for k in range(ks)) / (ks * ks)


def box_blur_bruteforce(img, ks):
    h, w = img.shape
    r = ks // 2
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            acc = 0.0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    acc += img[reflect101(y + dy, h), reflect101(x + dx, w)]
            out[y, x] = acc / (ks * ks)
    return out


def temporal_ir_pattern(stack, ks=11, threshold=0.005):
    """(pattern, margin) of one [T,H,W] stack: pattern = 1 where margin = d - blur(d) - threshold > 0, d the normalised
    end-point difference of the per-pixel line fit.  A constant difference image normalises to NaN as in the reference:
    every comparison is false, the pattern is all zeros (and the margin NaN)."""
    diff = fit_diff(stack)
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = (diff - np.min(diff)) / (np.max(diff) - np.min(diff))
        margin = np.abs(diff) - box_blur(np.abs(diff), ks) - threshold
        ir = np.zeros_like(diff)
        ir[margin > 0] = 1
    return ir, margin


def exposure_stack(seed, t, h, w):
    """The test generator: rng = default_rng(100 + seed); texture = integers(20, 120); dots = random < 0.06; frame
    k = clip(rint(texture + dots * k * (12 + 8 * random) + normal(0, 1.5)), 0, 255).  [t,h,w] float64 of integers."""
    rng = np.random.default_rng(100 + seed)
    tex = rng.integers(20, 120, size=(h, w)).astype(np.float64)
    dots = rng.random((h, w)) < 0.06
    frames = [np.clip(np.rint(tex + dots * k * (12 + 8 * rng.random((h, w))) + rng.normal(0, 1.5, (h, w))), 0, 255)
              for k in range(t)]
    return np.stack(frames)
