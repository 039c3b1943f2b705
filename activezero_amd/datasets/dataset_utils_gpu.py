"""GPU twins of the reference's per-item pattern helpers (datasets/dataset_utils.py) -- SURVEY.md 8f-4.
The reference computes them with numpy / cv2 inside DataLoader workers, one image at a time; here a whole
batch is processed on the device by az_ir_pattern (csrc/az_ir_pattern.hip).  get_temporal_ir_pattern is the twin of the
reference's offline tool tools/temporal_ir.py (csrc/az_temporal_ir.hip): the pattern of a real view from its stack of
projector exposures, made per item on the device instead of by a pass over the dataset before training."""
import torch

from activezero_amd import _lib
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
