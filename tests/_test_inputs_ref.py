"""Restatements the K25 (az_depth_labels) and K26 (az_test_images) kernels of csrc/az_test_inputs.hip are compared with.
Test infrastructure: numpy only, never the product path.

K25 is the loader's own numpy arithmetic on whole arrays: millimetres / 1000 in float64, focal_length * baseline / depth
under the mask depth > 0 in float64, the crop, one cast to float32.  The kernel must give these bits.

K26 restates ATen's upsample_bilinear2d (align_corners=False, no antialiasing) followed by the zero pad: source indices and
weights in float32, every operation rounded on its own, exactly as the entry point's contract states them; the BLEND of the
four taps is evaluated in float64.  A float32 blend -- the kernel's, or torch's own -- differs from it by rounded float32
operations on weights <= 1: on the way to one output a value passes an inner product, an inner sum, an outer product and
the outer sum, the two halves of the outer sum each bring their own product and sum -- six roundings in all, each at most
2^-24 of a partial result no larger than M, the largest tap magnitude: |diff| <= 6 M 2^-24.  tests/test_test_inputs_cpu.py
holds torch's own CPU operator to the same bound, so the restatement is ATen's definition and not a private one.
"""
import numpy as np

F32 = np.float32
MEAN = (0.485, 0.456, 0.406)  # ImageNet constants, as dataset_utils.py:76-81 normalises
STD = (0.229, 0.224, 0.225)
SIZE_PAIRS = (((7, 9), (5, 6)), ((5, 6), (7, 9)), ((13, 17), (13, 17)), ((33, 47), (20, 31)), ((1, 5), (3, 2)))
PADS = ((2, 3), (0, 0), (4, 0), (1, 2), (0, 1))  # (top, right), one per size pair
LARGE = ((720, 1280), (540, 960), (4, 0))


# ---- K25 -----------------------------------------------------------------------------------------------------------
def depth_labels(mm_l, mm_r, focal_length, baseline, origin=None, window=None):
    """mm_l, mm_r integer arrays [B,H2,W2]; focal_length, baseline float64 [B] (or scalars); origin None (the whole map) or
    integers [B,2] of (y0, x0) with window = (h2, w2), clamped into the map as the entry point clamps a device-side origin
    -> (disp_l, depth_l, disp_r, depth_r) float32 [B,1,h2,w2]"""
    mm_l, mm_r = np.asarray(mm_l), np.asarray(mm_r)
    B, H2, W2 = mm_l.shape
    fl = np.broadcast_to(np.asarray(focal_length, dtype=np.float64).reshape(-1), (B,))
    bl = np.broadcast_to(np.asarray(baseline, dtype=np.float64).reshape(-1), (B,))
    h2, w2 = (H2, W2) if window is None else window
    outs = [np.empty((B, 1, h2, w2), dtype=F32) for _ in range(4)]
    for b in range(B):
        y0, x0 = (0, 0) if origin is None else (int(v) for v in np.asarray(origin)[b])
        y0, x0 = min(max(y0, 0), H2 - h2), min(max(x0, 0), W2 - w2)
        for k, mm in enumerate((mm_l, mm_r)):
            depth = np.array(mm[b]) / 1000            # float64: millimetres to metres
            mask = depth > 0
            disp = np.zeros_like(depth)
            disp[mask] = fl[b] * bl[b] / depth[mask]
            outs[2 * k][b, 0] = disp[y0:y0 + h2, x0:x0 + w2].astype(F32)
            outs[2 * k + 1][b, 0] = depth[y0:y0 + h2, x0:x0 + w2].astype(F32)
    return tuple(outs)


# ---- K26 -----------------------------------------------------------------------------------------------------------
def normalise(levels):
    """uint8 [N,H,W] -> float32 [N,3,H,W]: float32 v / 255, minus the mean, divided by the std, each rounded once"""
    v = np.asarray(levels).astype(F32) / F32(255)
    return np.stack([(v - F32(m)) / F32(s) for m, s in zip(MEAN, STD)], axis=1)


def axis(n_in, n_out):
    """(i0, i1 int64 [n_out]; l0, l1 float32 [n_out]) of one axis"""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32)
    src = np.maximum(scale * (dst + F32(0.5)) - F32(0.5), F32(0))
    assert src.dtype == F32
    i0 = src.astype(np.int64)
    assert i0.max() <= n_in - 1
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F32)
    l0 = F32(1) - l1
    assert l0.dtype == l1.dtype == F32
    return i0, i1, l0, l1


def resize_pad(src, size, pad=(0, 0)):
    """float32 [N,3,Hin,Win] -> float64 [N,3,H + top,W + right]: the float32 weights, the blend in float64, zeros around"""
    src = np.asarray(src, dtype=F32)
    (h, w), (top, right) = size, pad
    y0, y1, ly0, ly1 = axis(src.shape[2], h)
    x0, x1, lx0, lx1 = axis(src.shape[3], w)
    s = src.astype(np.float64)
    ly0, ly1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    lx0, lx1 = lx0.astype(np.float64), lx1.astype(np.float64)
    with np.errstate(invalid="ignore"):
        a, b = s[:, :, y0][:, :, :, x0], s[:, :, y0][:, :, :, x1]
        c, d = s[:, :, y1][:, :, :, x0], s[:, :, y1][:, :, :, x1]
        val = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    out = np.zeros(src.shape[:2] + (h + top, w + right), dtype=np.float64)
    out[:, :, top:, :w] = val
    return out


def bound(src):
    """6 M 2^-24, M the largest finite tap magnitude"""
    src = np.asarray(src)
    return 6.0 * float(np.abs(src[np.isfinite(src)]).max()) * 2.0 ** -24


def random_levels(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
