"""GPU twins of the reference's per-item pattern helpers (datasets/dataset_utils.py) -- SURVEY.md 8f-4.
The reference computes them with numpy / cv2 inside DataLoader workers, one image at a time; here a whole
batch is processed on the device by az_ir_pattern (csrc/az_ir_pattern.hip).  get_temporal_ir_pattern is the twin of the
reference's offline tool tools/temporal_ir.py (csrc/az_temporal_ir.hip): the pattern of a real view from its stack of
projector exposures, made per item on the device instead of by a pass over the dataset before training.
augment_images / data_augmentation are the twin of data_augmentation (dataset_utils.py:49-83: GaussianBlur, ColorJitter,
ToTensor, Normalize) on az_augment (csrc/az_augment.hip): a batch of grey images in, normalised 3-channel images out.
resize_bilinear is the twin of the PIL resize the real item goes through (messytable.py:324-341, 353-356, 410-420) on
az_resize_bilinear_u8 (csrc/az_resample.hip): 8-bit grey images in, PIL's bits out, cropped on the way if asked.
depth_to_labels is the twin of the loader's depth lines (messytable.py:197-213, 256-261, 281-284) on az_depth_labels
(csrc/az_test_inputs.hip): raw millimetre maps in, the four float32 disparity and depth labels out; stereo_constants gives
the two host scalars it needs from an item's metadata."""
import numpy as np
import torch

from activezero_amd import _lib, ops
from activezero_amd.ops import _call, _chk, _p, _stream


def _pair(img_ir, img):
    a = _chk(img_ir.reshape(-1, *img_ir.shape[-2:]).contiguous(), "img_ir")
    b_ = _chk(img.reshape(-1, *img.shape[-2:]).contiguous(), "img")
    if a.shape != b_.shape:
        raise RuntimeError("img_ir and img must have identical shapes")
    return a, b_


def _pattern_mode(img_ir, img, ks, threshold, mode, what):
    a, b_ = _pair(img_ir, img)
    n, h, w = a.shape
    ws_bytes = 8 * n + 64 if mode == 0 else _lib.lib().az_ir_pattern_workspace(n, h, w, int(ks))
    if ws_bytes < 0:
        raise RuntimeError(f"{what}: image smaller than the smoothing window")
    ws = a.new_empty((ws_bytes + 3) // 4)
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        _call("az_ir_pattern_mode", _p(out), _p(ws), ws_bytes, _p(a), _p(b_), n, h, w, int(ks), float(threshold), mode,
              _stream())
    return out[0] if img_ir.dim() == 2 else out.view(img_ir.shape)


def get_ir_pattern(img_ir, img, threshold=0.005):
    """dataset_utils.py:12-17 for [H,W] or [B,H,W] float32 CUDA tensors -> binary pattern of the same shape."""
    return _pattern_mode(img_ir, img, 1, threshold, 0, "get_ir_pattern")


def get_smoothed_ir_pattern(img_ir, img, ks=11):
    """dataset_utils.py:20-30 for [H,W] or [B,H,W] float32 CUDA tensors -> binary pattern of the same shape."""
    return _pattern_mode(img_ir, img, ks, 0.0, 1, "get_smoothed_ir_pattern")


def get_temporal_ir_pattern(stack, ks=11, threshold=0.005):
    """tools/temporal_ir.py:91-114 for a [T,H,W] or [B,T,H,W] CUDA stack of grey levels 0..255 (float32 or uint8, the
    exposures of one view along T) -> binary float32 pattern [H,W] or [B,H,W]."""
    if not isinstance(stack, torch.Tensor):
        raise TypeError("stack: expected a tensor")
    if stack.dim() not in (3, 4):
        raise RuntimeError("stack must be [T,H,W] or [B,T,H,W]")
    if stack.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"stack: expected torch.float32 or torch.uint8, got {stack.dtype}")
    s = _chk((stack[None] if stack.dim() == 3 else stack).contiguous(), "stack", stack.dtype)
    n, t, h, w = s.shape
    ws_bytes = _lib.lib().az_temporal_ir_workspace(n, t, h, w, int(ks))
    _lib.check(min(ws_bytes, 0), "az_temporal_ir_workspace")  # T, ks or the image size out of range: nothing is launched
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=s.device)
    out = torch.empty(n, h, w, dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        _call("az_temporal_ir", _p(out), _p(ws), ws_bytes, _p(s), int(s.dtype == torch.uint8), n, t, h, w, int(ks),
              float(threshold), _stream())
    return out[0] if stack.dim() == 3 else out


def get_smoothed_ir_pattern2(img_ir, img, ks=11, threshold=0.005):
    """dataset_utils.py:33-46 for [H,W] or [B,H,W] float32 CUDA tensors -> binary pattern of the same shape."""
    squeeze = img_ir.dim() == 2
    a = _chk(img_ir.reshape(-1, *img_ir.shape[-2:]).contiguous(), "img_ir")
    b_ = _chk(img.reshape(-1, *img.shape[-2:]).contiguous(), "img")
    if a.shape != b_.shape:
        raise RuntimeError("img_ir and img must have identical shapes")
    n, h, w = a.shape
    ws_bytes = _lib.lib().az_ir_pattern_workspace(n, h, w, int(ks))
    if ws_bytes < 0:
        raise RuntimeError("get_smoothed_ir_pattern2: image smaller than the smoothing window")
    ws = a.new_empty((ws_bytes + 3) // 4)
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        _call("az_ir_pattern", _p(out), _p(ws), ws_bytes, _p(a), _p(b_), n, h, w, int(ks), float(threshold), _stream())
    return out[0] if squeeze else out.view(img_ir.shape)


def _column(value, n, name, device):
    """one parameter of augment_images as n float32 values on the device, without a host round trip"""
    if isinstance(value, torch.Tensor):
        if value.device != device:
            raise RuntimeError(f"{name}: must live on the device of grey ({device}), got {value.device}")
        if value.numel() != n:
            raise RuntimeError(f"{name}: expected {n} values (one per image), got {value.numel()}")
        return value.reshape(n).to(torch.float32)
    return torch.full((n,), float(value), dtype=torch.float32, device=device)


def augment_images(grey, sigma=None, brightness=None, contrast=None, contrast_first=None, kernel_size=9):
    """The transform dataset_utils.py:49-83 builds, for [H,W] or [B,H,W] grey CUDA images (float32 in [0,1], or uint8
    levels taken as v / 255) -> [3,H,W] or [B,3,H,W] float32: GaussianBlur(kernel_size, sigma), ColorJitter with the fixed
    factors `brightness` and `contrast` in the order `contrast_first` says (torchvision draws it per call), then the
    ImageNet normalisation.  Each parameter is None (stage off), a number, or a CUDA tensor of B values; brightness and
    contrast come together (the reference only ever enables both).  With every stage off the result is bit for bit
    (grey - mean) / std.  sigma <= 0 leaves an image unblurred, factors are not range-checked (a device-side value cannot
    raise without a synchronisation), NaN propagates."""
    if not isinstance(grey, torch.Tensor):
        raise TypeError("grey: expected a tensor")
    if grey.dim() not in (2, 3):
        raise RuntimeError("grey must be [H,W] or [B,H,W]")
    if grey.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"grey: expected torch.float32 or torch.uint8, got {grey.dtype}")
    if (brightness is None) != (contrast is None):
        raise RuntimeError("brightness and contrast are given together or not at all")
    if contrast_first is not None and brightness is None:
        raise RuntimeError("contrast_first needs brightness and contrast")
    g = _chk((grey[None] if grey.dim() == 2 else grey).contiguous(), "grey", grey.dtype)
    n, h, w = g.shape
    flags = int(sigma is not None) | 2 * int(brightness is not None)
    params = None
    if flags:
        one = lambda v, name: _column(0.0 if v is None else v, n, name, g.device)  # noqa: E731
        params = torch.stack([one(sigma, "sigma"), one(brightness, "brightness"), one(contrast, "contrast"),
                              one(contrast_first, "contrast_first")], dim=1).contiguous()
    ws_bytes = _lib.lib().az_augment_workspace(n, h, w, int(kernel_size))
    _lib.check(min(ws_bytes, 0), "az_augment_workspace")  # kernel_size or the image size out of range: nothing is launched
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=g.device)
    out = torch.empty(n, 3, h, w, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _call("az_augment", _p(out), _p(ws), ws_bytes, _p(g), int(g.dtype == torch.uint8), _p(params), n, h, w,
              int(kernel_size), flags, _stream())
    return out[0] if grey.dim() == 2 else out


_RESAMPLE_TABLES = {}  # (in_size, out_size, device) -> [out_size, 2 + ksize] int32 on the device


def _resample_ksize(in_size, out_size, what):
    """taps per table row for one axis, from the library's host function; raises for a size it refuses"""
    ks = _lib.lib().az_resample_bilinear_ksize(int(in_size), int(out_size))
    if ks == _lib.CONST["AZ_EUNSUPPORTED"]:
        raise RuntimeError(f"resize_bilinear: {what} {in_size} -> {out_size}: a ratio above 8 is not supported")
    if ks < 0:
        raise RuntimeError(f"resize_bilinear: {what} {in_size} -> {out_size}: sizes must be positive")
    return ks


def _resample_table(in_size, out_size, device):
    """the device copy of the library's coefficient table for one axis: built on the host and copied once per
    (in, out, device), then served from the cache"""
    key = (int(in_size), int(out_size), torch.device(device))
    table = _RESAMPLE_TABLES.get(key)
    if table is None:
        ks = _resample_ksize(in_size, out_size, "size")
        host = torch.empty(key[1], 2 + ks, dtype=torch.int32)
        _call("az_resample_bilinear_table", host.data_ptr(), key[0], key[1])
        table = _RESAMPLE_TABLES[key] = host.to(key[2])
    return table


def resize_bilinear(grey, size, crop=None, dtype=torch.uint8):
    """PIL's Image.resize(size, resample=Image.BILINEAR) on 8-bit grey images, bit for bit (messytable.py:324-341, 353-356,
    410-420), for a [Hin,Win] or [B,Hin,Win] uint8 CUDA tensor; size = (Hout, Wout) -- rows first, where PIL takes
    (width, height).  crop = (y0, x0, h, w) returns only that window of the resized image (messytable.py:366-398), None the
    whole image.  dtype torch.uint8 gives the levels, torch.float32 the image v / 255 with the bits of
    torch.from_numpy(np.array(img) / 255).float().  Returns [h,w] or [B,h,w].  Sizes with in > 8 out are refused (unless in <= 17).  The two
    coefficient tables come from the library and are cached on the device per (in, out, device): the first call for a size
    pair copies them, every later call is one launch and synchronises nothing."""
    if not isinstance(grey, torch.Tensor):
        raise TypeError("grey: expected a tensor")
    if grey.dim() not in (2, 3):
        raise RuntimeError("grey must be [Hin,Win] or [B,Hin,Win]")
    if grey.dtype != torch.uint8:
        raise RuntimeError(f"grey: expected torch.uint8, got {grey.dtype}")
    if dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"dtype: expected torch.uint8 or torch.float32, got {dtype}")
    hin, win = grey.shape[-2:]
    hout, wout = (int(s) for s in size)
    _resample_ksize(hin, hout, "height")
    _resample_ksize(win, wout, "width")
    y0, x0, h, w = (0, 0, hout, wout) if crop is None else (int(c) for c in crop)
    if y0 < 0 or x0 < 0 or h <= 0 or w <= 0 or y0 + h > hout or x0 + w > wout:
        raise RuntimeError(f"crop {(y0, x0, h, w)} lies outside the {hout} x {wout} image")
    g = _chk((grey[None] if grey.dim() == 2 else grey).contiguous(), "grey", torch.uint8)
    n = g.shape[0]
    table_y, table_x = _resample_table(hin, hout, g.device), _resample_table(win, wout, g.device)
    out = torch.empty(n, h, w, dtype=dtype, device=g.device)
    u8, f32 = (out, None) if dtype == torch.uint8 else (None, out)
    with torch.cuda.device(g.device):
        _call("az_resize_bilinear_u8", _p(u8), _p(f32), _p(g), _p(table_y), _p(table_x), n, hin, win, hout, wout, y0, x0,
              h, w, _stream())
    return out[0] if grey.dim() == 2 else out


def stereo_constants(extrinsic_l, extrinsic_r, intrinsic_l):
    """messytable.py:205-206: (focal_length, baseline) of an item's metadata as float64 host scalars -- the focal length of
    the left IR camera at half resolution, intrinsic_l[0, 0] / 2, and the distance between the two IR cameras, the norm of the
    difference of the extrinsics' last columns.  Host arithmetic on a 3 x 3 and two 4 x 4 matrices: no device is touched."""
    extrinsic_l, extrinsic_r, intrinsic_l = (np.asarray(m, dtype=np.float64) for m in (extrinsic_l, extrinsic_r, intrinsic_l))
    baseline = np.linalg.norm(extrinsic_l[:, -1] - extrinsic_r[:, -1])
    focal_length = intrinsic_l[0, 0] / 2
    return focal_length, baseline


def depth_to_labels(depth_l_mm, depth_r_mm, focal_length, baseline, crop=None):
    """messytable.py:197-213, 256-261, 281-284 on az_depth_labels (csrc/az_test_inputs.hip): the two raw millimetre depth maps
    of a batch, [H2,W2] or [B,H2,W2] uint16 (a 16-bit PNG) or int32 (PIL's mode I) CUDA tensors -- uploaded as they are, a
    quarter of the bytes of the four float maps the reference's loader uploads -- -> (img_disp_l, img_depth_l, img_disp_r,
    img_depth_r), each [1,h2,w2] or [B,1,h2,w2] float32 with the bits of the reference's float64 arithmetic.  focal_length,
    baseline: stereo_constants' numbers, or B values on the device.  crop None: the whole maps (test mode); (y0, x0, h2, w2)
    integers: that window of every item; (origin, (h2, w2)) with origin an int32 [B,2] CUDA tensor of (y0, x0): a window per
    item -- the reference's 2x : 2(x + th), 2y : 2(y + tw) with y0 = 2x, x0 = 2y, h2 = 2th, w2 = 2tw.  Nothing synchronises."""
    if not isinstance(depth_l_mm, torch.Tensor) or not isinstance(depth_r_mm, torch.Tensor):
        raise TypeError("depth_l_mm, depth_r_mm: expected tensors")
    if depth_l_mm.dim() not in (2, 3):
        raise RuntimeError("depth_l_mm must be [H2,W2] or [B,H2,W2]")
    single = depth_l_mm.dim() == 2
    a, b_ = ((t[None] if single else t).contiguous() for t in (depth_l_mm, depth_r_mm))
    origin = window = None
    if crop is not None and len(crop) == 4:
        y0, x0, h2, w2 = (int(c) for c in crop)
        if y0 < 0 or x0 < 0 or h2 <= 0 or w2 <= 0 or y0 + h2 > a.shape[-2] or x0 + w2 > a.shape[-1]:
            raise RuntimeError(f"crop {(y0, x0, h2, w2)} lies outside the {a.shape[-2]} x {a.shape[-1]} map")
        origin = torch.empty(a.shape[0], 2, dtype=torch.int32, device=a.device)  # filled on the device: no host round trip
        origin[:, 0].fill_(y0)
        origin[:, 1].fill_(x0)
        window = (h2, w2)
    elif crop is not None:
        origin, window = crop
    outs = ops.depth_labels(a, b_, focal_length, baseline, origin, window)
    return tuple(o[0] for o in outs) if single else outs


class _Augmentation:
    """what data_augmentation returns: the drawn parameters (sigma, brightness, contrast: [items] float32 on the device, or
    None for a stage that is off) and the call that applies them"""

    def __init__(self, sigma, brightness, contrast, kernel_size, generator, device):
        self.sigma, self.brightness, self.contrast = sigma, brightness, contrast
        self.kernel_size, self.generator, self.device = kernel_size, generator, device
        self.last_order = None

    def draw_order(self, n):
        """n orders, 1 = contrast first: torchvision's ColorJitter permutes its adjustments at every application"""
        return (torch.rand(n, generator=self.generator, device=self.device) < 0.5).to(torch.float32)

    def __call__(self, grey):
        if not isinstance(grey, torch.Tensor) or grey.dim() not in (3, 4):
            raise RuntimeError("grey must be [B,H,W] or [B,V,H,W] (V views of B items)")
        b, v = grey.shape[0], (grey.shape[1] if grey.dim() == 4 else 1)
        items = next((p.numel() for p in (self.sigma, self.brightness) if p is not None), 1)
        if items not in (1, b):
            raise RuntimeError(f"parameters were drawn for {items} items, got {b}")
        # the views of an item share its parameters (messytable.py:264-270); one drawn set serves any number of items
        each = lambda p: None if p is None else p.expand(b)[:, None].expand(b, v).reshape(-1)  # noqa: E731
        order = None
        if self.brightness is not None:
            order = self.last_order = self.draw_order(b * v)
        out = augment_images(grey.reshape(b * v, *grey.shape[-2:]), each(self.sigma), each(self.brightness),
                             each(self.contrast), order, self.kernel_size)
        return out if grey.dim() == 3 else out.view(b, v, 3, *grey.shape[-2:])


def data_augmentation(gaussian_blur=False, color_jitter=False, *, kernel_size=9, sigma=(0.1, 2.0), brightness=(0.4, 1.4),
                      contrast=(0.8, 1.2), generator=None, items=1):
    """dataset_utils.py:49-83 with the values of configs/config.py:104-113 as defaults.  Like the reference it draws the
    parameters WHEN IT IS CALLED -- one (sigma, brightness, contrast) per item, uniform in the given ranges, with
    torch.rand(items, 3, generator=generator) on the generator's device (the current CUDA device without one) -- and returns
    a callable for [B,H,W] grey images, or [B,V,H,W] for V views per item which share the item's parameters; B = items, or
    any B when items = 1.  The jitter order is drawn anew, per image, at each application.  Nothing synchronises."""
    device = generator.device if generator is not None else torch.device("cuda", torch.cuda.current_device())
    u = torch.rand(items, 3, generator=generator, device=device)
    draw = lambda k, rng: rng[0] + (rng[1] - rng[0]) * u[:, k]  # noqa: E731
    return _Augmentation(draw(0, sigma) if gaussian_blur else None, draw(1, brightness) if color_jitter else None,
                         draw(2, contrast) if color_jitter else None, int(kernel_size), generator, device)
