"""Torch-facing wrappers over the C ABI (include/azhip.h).

PyTorch is plumbing only here: it owns device memory and the current HIP
stream; every computation is a call into libazhip.so through raw pointers.
All wrappers validate like the reference does (contiguity / dtype / device /
sign, utils/warp_ops.py:69-77) and raise on violation -- there is no eager or
CPU fallback.
"""
import numpy as np
import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: must be contiguous")
    return t


def _call(name, *args):
    fn = getattr(_lib.lib(), name)
    _lib.check(fn(*args), name)


def _p(t):
    return t.data_ptr() if t is not None else None


# ----------------------------------------------------------------------------
# K1/K2 scatter warp
# ----------------------------------------------------------------------------
def warp_scatter(img, disp, sign):
    """dst[n,c,y,j+disp] = src[n,c,y,j] with the reference's collision rule."""
    _chk(img, "img")
    _chk(disp, "disp", torch.int32)
    n, c, h, w = img.shape
    if disp.numel() != n * h * w:
        raise RuntimeError("disp must be [N,H,W] or [N,1,H,W]")
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _call("az_warp_scatter", _p(out), _p(img), _p(disp), n, c, h, w, int(sign), _stream())
    return out


# ----------------------------------------------------------------------------
# K3 cost volume
# ----------------------------------------------------------------------------
class _CostVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_l, feat_r, ndisp, channels_last):
        feat_l = _chk(feat_l.contiguous(), "feat_l")
        feat_r = _chk(feat_r.contiguous(), "feat_r")
        if feat_l.shape != feat_r.shape:
            raise RuntimeError("feature maps must have identical shapes")
        ctx.ndisp, ctx.cl = ndisp, channels_last
        with torch.cuda.device(feat_l.device):
            if channels_last:
                b, h, w, c = feat_l.shape
                out = feat_l.new_empty(b, ndisp, h, w, 2 * c)
                _call("az_cost_volume_fwd_ndhwc", _p(out), _p(feat_l), _p(feat_r), b, c, ndisp, h, w, _stream())
            else:
                b, c, h, w = feat_l.shape
                out = feat_l.new_empty(b, 2 * c, ndisp, h, w)
                _call("az_cost_volume_fwd", _p(out), _p(feat_l), _p(feat_r), b, c, ndisp, h, w, _stream())
        ctx.dims = (b, c, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _chk(g.contiguous(), "grad_cost")
        b, c, h, w = ctx.dims
        shape = (b, h, w, c) if ctx.cl else (b, c, h, w)
        gl, gr = g.new_empty(shape), g.new_empty(shape)
        name = "az_cost_volume_bwd_ndhwc" if ctx.cl else "az_cost_volume_bwd"
        with torch.cuda.device(g.device):
            _call(name, _p(gl), _p(gr), _p(g), b, c, ctx.ndisp, h, w, _stream())
        return gl, gr, None, None


def cost_volume(feat_l, feat_r, ndisp):
    """[B,C,h,w] x2 -> [B,2C,ndisp,h,w] (reference layout)."""
    return _CostVolume.apply(feat_l, feat_r, int(ndisp), False)


def cost_volume_ndhwc(feat_l_nhwc, feat_r_nhwc, ndisp):
    """[B,h,w,C] x2 -> [B,ndisp,h,w,2C] (channels-last, internal layout)."""
    return _CostVolume.apply(feat_l_nhwc, feat_r_nhwc, int(ndisp), True)


# ----------------------------------------------------------------------------
# K6 soft-argmin head
# ----------------------------------------------------------------------------
class _SoftArgmin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        # logits: [B,1,d,h,w] or [B,d,h,w]
        lg = _chk(logits.contiguous(), "logits")
        if lg.dim() == 5:
            if lg.shape[1] != 1:
                raise RuntimeError("logits must have one channel")
            b, _, d, h, w = lg.shape
        else:
            b, d, h, w = lg.shape
        out = lg.new_empty(b, 1, 4 * h, 4 * w)
        # per-pixel softmax shift / normaliser (8 B per pixel) so that backward skips that pass
        stats = lg.new_empty(b, 4 * h, 4 * w, 2) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(lg.device):
            _call("az_softargmin_fwd", _p(out), _p(stats), _p(lg), b, d, h, w, _stream())
        if stats is not None:
            ctx.save_for_backward(lg, stats, out)
        else:
            ctx.save_for_backward(lg)
        ctx.dims = (b, d, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        lg, stats, out = (tuple(ctx.saved_tensors) + (None, None))[:3]
        g = _chk(g.contiguous(), "grad_disp")
        b, d, h, w = ctx.dims
        gl = torch.empty_like(lg)
        with torch.cuda.device(g.device):
            _call("az_softargmin_bwd", _p(gl), _p(g), _p(lg), _p(stats), _p(out), b, d, h, w, _stream())
        return gl


def softargmin(logits):
    """Fused trilinear x4 upsample + softmax over D=4d + expectation -> [B,1,4h,4w]."""
    return _SoftArgmin.apply(logits)


# ----------------------------------------------------------------------------
# K7 bilinear gather warp
# ----------------------------------------------------------------------------
class _WarpGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, disp):
        img = _chk(img.contiguous(), "img")
        disp = _chk(disp.contiguous(), "disp")
        b, c, h, w = img.shape
        if disp.numel() != b * h * w:
            raise RuntimeError("disp must be [B,1,H,W]")
        out = torch.empty_like(img)
        with torch.cuda.device(img.device):
            _call("az_warp_gather_fwd", _p(out), _p(img), _p(disp), b, c, h, w, _stream())
        ctx.save_for_backward(img, disp)
        return out

    @staticmethod
    def backward(ctx, g):
        img, disp = ctx.saved_tensors
        g = _chk(g.contiguous(), "grad_out")
        b, c, h, w = img.shape
        gd = torch.empty_like(disp)
        gi = torch.zeros_like(img) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(g.device):
            _call("az_warp_gather_bwd", _p(gd), _p(gi), _p(g), _p(img), _p(disp), b, c, h, w, _stream())
        return gi, gd


def warp_gather(img, disp):
    """apply_disparity: bilinear sample of img at x + disp, zero padding."""
    return _WarpGather.apply(img, disp)


# ----------------------------------------------------------------------------
# K8 fused patch reprojection loss
# ----------------------------------------------------------------------------
class _PatchReproj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pat_l, pat_r, disp, mask_u8, ps, sign):
        b, c, h, w = pat_l.shape
        acc = torch.empty(2, dtype=torch.float64, device=pat_l.device)
        with torch.cuda.device(pat_l.device):
            _call("az_patch_reproj_fwd", _p(acc), _p(pat_l), _p(pat_r), _p(disp), _p(mask_u8),
                  b, c, h, w, ps, float(sign), _stream())
        ctx.save_for_backward(pat_l, pat_r, disp, mask_u8, acc)
        ctx.ps, ctx.sign = ps, sign
        return (acc[0] / acc[1]).to(torch.float32)

    @staticmethod
    def backward(ctx, gloss):
        pat_l, pat_r, disp, mask_u8, acc = ctx.saved_tensors
        b, c, h, w = pat_l.shape
        gloss = gloss.to(torch.float32).contiguous()
        gd = torch.empty_like(disp)
        with torch.cuda.device(disp.device):
            _call("az_patch_reproj_bwd", _p(gd), _p(gloss), _p(acc), _p(pat_l), _p(pat_r),
                  _p(disp), _p(mask_u8), b, c, h, w, ctx.ps, float(ctx.sign), _stream())
        return None, None, gd, None, None, None


def patch_reprojection(input_l, input_r, pred_disp_l, mask=None, ps=5, want_vis=True):
    """get_reproj_error_patch -> (loss, warped_vis [B,C,H,W], mask [B,C,H,W] int32)."""
    pat_l = _chk(input_l.detach().contiguous(), "input_L")
    pat_r = _chk(input_r.detach().contiguous(), "input_R")
    disp = _chk(pred_disp_l.contiguous(), "pred_disp_l")
    b, c, h, w = pat_l.shape
    if disp.numel() != b * h * w:
        raise RuntimeError("pred_disp_l must be [B,1,H,W]")
    mask_u8 = None
    if mask is not None:
        if mask.numel() != b * h * w:
            raise RuntimeError("mask must be [B,1,H,W]")
        mask_u8 = _chk(mask.contiguous().to(torch.uint8), "mask", torch.uint8)
    loss = _PatchReproj.apply(pat_l, pat_r, disp, mask_u8, int(ps), -1.0)
    vis = None
    if want_vis:
        vis = torch.empty_like(pat_l)
        with torch.cuda.device(pat_l.device):
            _call("az_patch_reproj_vis", _p(vis), _p(pat_r), _p(disp.detach()), b, c, h, w, int(ps),
                  -1.0, _stream())
    if mask is None:
        mask_out = torch.ones(b, c, h, w, dtype=torch.int32, device=pat_l.device)
    else:
        mask_out = mask.reshape(b, 1, h, w).expand(b, c, h, w).to(torch.int32)
    return loss, vis, mask_out


# ----------------------------------------------------------------------------
# K9 local contrast normalisation
# ----------------------------------------------------------------------------
def local_contrast_norm(image, kernel_size=9, eps=1e-5):
    """image [B,1,H,W] (contiguous) -> (normed, std), both [B,1,H,W]."""
    img = _chk(image, "image")
    b, c, h, w = img.shape
    normed = img.new_empty(b, 1, h, w)
    std = img.new_empty(b, 1, h, w)
    with torch.cuda.device(img.device):
        _call("az_lcn", _p(normed), _p(std), _p(img), b, h, w, int(kernel_size), float(eps),
              c * h * w, _stream())
    return normed, std


# ----------------------------------------------------------------------------
# K12 disparity loss + error metrics (the step after the path)
# ----------------------------------------------------------------------------
def _mask_u8(mask, like, name="mask"):
    if mask is None:
        return None
    if mask.shape != like.shape:
        raise RuntimeError(f"{name}: shape {tuple(mask.shape)} != {tuple(like.shape)}")
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)  # same bytes, no copy
    return _chk(mask, name, torch.uint8)


class _DispLoss(torch.autograd.Function):
    WEIGHTS = (1.0, 0.7, 0.5)  # pred3, pred2, pred1 (utils/losses.py:9-14)

    @staticmethod
    def forward(ctx, pred3, pred2, pred1, gt, mask, lo, hi):
        p3, p2, p1 = (_chk(p.contiguous(), f"pred{k}") for p, k in ((pred3, 3), (pred2, 2), (pred1, 1)))
        gt = _chk(gt.contiguous(), "disp_gt")
        if not (p3.shape == p2.shape == p1.shape == gt.shape):
            raise RuntimeError("predictions and ground truth must have identical shapes")
        m = _mask_u8(mask, gt)
        acc = torch.zeros(4, dtype=torch.float64, device=gt.device)
        with torch.cuda.device(gt.device):
            _call("az_disp_loss_fwd", _p(acc), _p(p3), _p(p2), _p(p1), _p(gt), _p(m), float(lo), float(hi),
                  gt.numel(), _stream())
        w3, w2, w1 = _DispLoss.WEIGHTS
        loss = ((w3 * acc[0] + w2 * acc[1] + w1 * acc[2]) / acc[3]).to(torch.float32)  # 0/0 = nan, as the reference's empty mean
        ctx.save_for_backward(p3, p2, p1, gt, m if m is not None else gt.new_empty(0), acc)
        ctx.has_mask, ctx.lo, ctx.hi = m is not None, float(lo), float(hi)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        p3, p2, p1, gt, m, acc = ctx.saved_tensors
        gloss = _chk(gloss.contiguous().to(torch.float32).reshape(1), "grad_loss")
        g3, g2, g1 = torch.empty_like(p3), torch.empty_like(p2), torch.empty_like(p1)
        w3, w2, w1 = _DispLoss.WEIGHTS
        with torch.cuda.device(gt.device):
            _call("az_disp_loss_bwd", _p(g3), _p(g2), _p(g1), _p(p3), _p(p2), _p(p1), _p(gt),
                  _p(m) if ctx.has_mask else None, ctx.lo, ctx.hi, _p(gloss), _p(acc), w3, w2, w1,
                  gt.numel(), _stream())
        return g3, g2, g1, None, None, None, None


def disp_loss(pred3, pred2, pred1, gt, mask=None, lo=0.0, hi=float("inf")):
    """smooth_l1(pred3) + 0.7 smooth_l1(pred2) + 0.5 smooth_l1(pred1), each a mean over the valid
    pixels: `mask` (bool/uint8, same shape) or, when mask is None, lo < gt < hi.  One pass, no sync."""
    return _DispLoss.apply(pred3, pred2, pred1, gt, mask, lo, hi)


# ----------------------------------------------------------------------------
# K29 multi-scale disparity loss (dispnet_disp, default_disp)
# ----------------------------------------------------------------------------
MS_LOSS_MAX = _lib.CONST["AZ_MS_LOSS_MAX"]


def _ms_descs(ps, grads, shifts):
    """the AzMsLossDesc table of one call, in host memory (the library copies it into the kernel arguments)"""
    descs = np.zeros(len(ps), dtype=_lib.MS_LOSS_DESC)
    for k, (p, g, s) in enumerate(zip(ps, grads, shifts)):
        descs[k] = (p.data_ptr(), 0 if g is None else g.data_ptr(), s, p.shape[2], p.shape[3], 0)
    return descs


class _MsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, mask, shifts, weights, lo, hi, *preds):
        gt = _chk(gt.contiguous(), "disp_gt")
        if gt.dim() != 4 or gt.shape[1] != 1:
            raise RuntimeError(f"disp_gt: expected [B,1,H,W], got {tuple(gt.shape)}")
        m = _mask_u8(mask, gt)
        b, _, h, w = gt.shape
        ps = []
        for k, (p, s) in enumerate(zip(preds, shifts)):
            p = _chk(p.contiguous(), f"preds[{k}]")
            if (h >> s) < 1 or (w >> s) < 1:
                raise RuntimeError(f"preds[{k}]: a {h}x{w} map has no pixels at scale 1/{1 << s}")
            if tuple(p.shape) != (b, 1, h >> s, w >> s):
                raise RuntimeError(f"preds[{k}]: shape {tuple(p.shape)} != {(b, 1, h >> s, w >> s)} (scale 1/{1 << s})")
            ps.append(p)
        n = len(ps)
        acc = torch.zeros(n, 2, dtype=torch.float64, device=gt.device)
        descs = _ms_descs(ps, [None] * n, shifts)
        with torch.cuda.device(gt.device):
            _call("az_ms_loss_fwd", _p(acc), descs.ctypes.data, n, _p(gt), _p(m), float(lo), float(hi), b, h, w, _stream())
        # python-float weights: kernel arguments, no blocking copy.  0/0 = nan, as the reference's empty mean
        means = acc[:, 0] / acc[:, 1]
        loss = means[0] * weights[0]
        for k in range(1, n):
            loss = torch.add(loss, means[k], alpha=weights[k])
        ctx.save_for_backward(gt, m if m is not None else gt.new_empty(0), acc, *ps)
        ctx.has_mask, ctx.lo, ctx.hi, ctx.shifts, ctx.weights = m is not None, float(lo), float(hi), shifts, weights
        means = means.to(torch.float32)
        ctx.mark_non_differentiable(means)
        return loss.to(torch.float32), means

    @staticmethod
    def backward(ctx, gloss, _gmeans):
        gt, m, acc, *ps = ctx.saved_tensors
        gloss = _chk(gloss.contiguous().to(torch.float32).reshape(1), "grad_loss")
        grads = [torch.empty_like(p) if need else None for p, need in zip(ps, ctx.needs_input_grad[6:])]
        descs = _ms_descs(ps, grads, ctx.shifts)
        wts = np.asarray(ctx.weights, dtype=np.float32)
        b, _, h, w = gt.shape
        with torch.cuda.device(gt.device):
            _call("az_ms_loss_bwd", descs.ctypes.data, wts.ctypes.data, len(ps), _p(gt), _p(m) if ctx.has_mask else None,
                  ctx.lo, ctx.hi, _p(gloss), _p(acc), b, h, w, _stream())
        return (None,) * 6 + tuple(grads)


def multiscale_disp_loss(preds, gt, mask=None, shifts=None, weights=None, lo=0.0, hi=float("inf")):
    """sum_k weights[k] * mean of smooth_l1(preds[k] - gt at stride 2^shifts[k]) over the valid pixels of scale k.
    gt [B,1,H,W]; preds[k] [B,1,H >> shifts[k], W >> shifts[k]], its pixel (y, x) is compared with gt at
    (y << shifts[k], x << shifts[k]) -- F.interpolate(scale_factor=1 / 2^s), nearest.  Valid: `mask` (bool / uint8, gt's shape)
    at that pixel, or, when mask is None, lo < gt < hi.  shifts default to 0 (every prediction at full resolution), weights
    to 1; at most MS_LOSS_MAX predictions.  One autograd node, one forward and one backward launch, no boolean indexing and
    no host sync.  Returns the fp32 scalar; its attribute `scale_means` is the fp32 device tensor [len(preds)] of the
    per-scale means (nan for a scale without valid pixels, as the reference's empty mean), for logging without a sync."""
    preds = list(preds)
    n = len(preds)
    if not 1 <= n <= MS_LOSS_MAX:
        raise RuntimeError(f"multiscale_disp_loss takes 1..{MS_LOSS_MAX} predictions, got {n}")
    shifts = (0,) * n if shifts is None else tuple(int(s) for s in shifts)
    weights = (1.0,) * n if weights is None else tuple(float(x) for x in weights)
    if len(shifts) != n or len(weights) != n:
        raise RuntimeError(f"{n} predictions, {len(shifts)} shifts, {len(weights)} weights")
    if any(not 0 <= s <= 30 for s in shifts):
        raise RuntimeError(f"shifts must be in 0..30, got {shifts}")
    loss, means = _MsLoss.apply(gt, mask, shifts, weights, lo, hi, *preds)
    loss.scale_means = means
    return loss


def disp_metrics(disp_gt, depth_gt, disp_pred, mask, focal_x_baseline=None, depth_pred=None):
    """fp64 sums [sum|dd|, #(|dd|>1), #(|dd|>2), sum clip(|1000 dz|,0,100), #(|dz|>2e-3), #(|dz|>4e-3),
    #(|dz|>8e-3), count] over the masked pixels, on the device (no sync)."""
    dg = _chk(disp_gt.contiguous(), "disp_gt")
    zg = _chk(depth_gt.contiguous(), "depth_gt")
    dp = _chk(disp_pred.contiguous(), "disp_pred")
    if not (dg.shape == zg.shape == dp.shape):
        raise RuntimeError("disp_gt, depth_gt and disp_pred must have identical shapes")
    m = _mask_u8(mask, dg)
    if m is None:
        raise RuntimeError("mask is required")
    b = dg.shape[0]
    zp = _chk(depth_pred.contiguous(), "depth_pred") if depth_pred is not None else None
    fb = None
    if zp is None:
        fb = _chk(focal_x_baseline.contiguous().reshape(-1), "focal_x_baseline")
        if fb.numel() != b:
            raise RuntimeError("focal_x_baseline must hold one value per batch element")
    acc = torch.zeros(8, dtype=torch.float64, device=dg.device)
    with torch.cuda.device(dg.device):
        _call("az_disp_metrics", _p(acc), _p(dg), _p(zg), _p(dp), _p(zp), _p(fb), _p(m), b,
              dg.numel() // max(b, 1), _stream())
    return acc


# ----------------------------------------------------------------------------
# K22 metrics per image and object label, K23 the evaluation mask (test.py around the network)
# ----------------------------------------------------------------------------
MAX_LABELS = _lib.CONST["AZ_OBJ_MAX_LABELS"]


def _obj_metrics(disp_gt, depth_gt, disp_pred, mask, label, num_labels, focal_x_baseline, depth_pred):
    """the launch of obj_metrics -> (the fp64 buffer that holds its three outputs, B, L)"""
    dg = _chk(disp_gt.contiguous(), "disp_gt")
    zg = _chk(depth_gt.contiguous(), "depth_gt")
    dp = _chk(disp_pred.contiguous(), "disp_pred")
    if not (dg.shape == zg.shape == dp.shape):
        raise RuntimeError("disp_gt, depth_gt and disp_pred must have identical shapes")
    m = _mask_u8(mask, dg)
    if m is None:
        raise RuntimeError("mask is required")
    nl = int(num_labels)
    if not 1 <= nl <= MAX_LABELS:
        raise RuntimeError(f"num_labels must be in [1, {MAX_LABELS}], got {num_labels}")
    lb = None
    if label is not None:
        lb = _chk(label.contiguous(), "label", torch.int32)
        if lb.numel() != dg.numel() or lb.shape[0] != dg.shape[0]:
            raise RuntimeError(f"label: shape {tuple(lb.shape)} does not match {tuple(dg.shape)}")
    b = dg.shape[0]
    zp = _chk(depth_pred.contiguous(), "depth_pred") if depth_pred is not None else None
    fb = None
    if zp is None:
        if focal_x_baseline is None:
            raise RuntimeError("focal_x_baseline or depth_pred is required")
        fb = _chk(focal_x_baseline.contiguous().reshape(-1), "focal_x_baseline")
        if fb.numel() != b:
            raise RuntimeError("focal_x_baseline must hold one value per batch element")
    elif zp.shape != dg.shape:
        raise RuntimeError("depth_pred must have the shape of disp_pred")
    buf = torch.zeros(_obj_words(b, nl), dtype=torch.float64, device=dg.device)  # the three outputs: one zeroing, one copy
    acc, present, stats = _obj_views(buf, b, nl)
    with torch.cuda.device(dg.device):
        _call("az_obj_metrics", _p(acc), _p(present), _p(stats), _p(dg), _p(zg), _p(dp), _p(zp), _p(fb), _p(m), _p(lb),
              b, nl, dg.numel() // max(b, 1), _stream())
    return buf, b, nl


def obj_metrics(disp_gt, depth_gt, disp_pred, mask, label=None, num_labels=1, focal_x_baseline=None, depth_pred=None):
    """The eight sums of disp_metrics per image and per object label, in one launch: maps [B,1,H,W] (or any shape whose
    first axis is the batch), mask bool / uint8, label int32 of the same shape or None (every pixel has label 0).
    Returns (acc [B,L,8] float64, present [B,L] int32 -- pixels of image b with label l, masked or not --, stats [1] int32
    -- pixels whose label is outside [0, L)), L = num_labels <= MAX_LABELS, all on the device.  No host sync."""
    return _obj_views(*_obj_metrics(disp_gt, depth_gt, disp_pred, mask, label, num_labels, focal_x_baseline, depth_pred))


def obj_metrics_host(disp_gt, depth_gt, disp_pred, mask, label=None, num_labels=1, focal_x_baseline=None, depth_pred=None):
    """obj_metrics, its three results as numpy arrays: the launch and then ONE device->host copy (the only sync)."""
    buf, b, nl = _obj_metrics(disp_gt, depth_gt, disp_pred, mask, label, num_labels, focal_x_baseline, depth_pred)
    return _obj_views(buf.cpu().numpy(), b, nl)


def _obj_words(b, nl):
    """fp64 words of the buffer obj_metrics keeps its three outputs in: acc, then present and stats as int32 pairs"""
    return b * nl * 8 + (b * nl + 2) // 2


def _obj_views(buf, b, nl):
    """(acc [b,nl,8] float64, present [b,nl] int32, stats [1] int32) as views of that buffer -- a tensor or a numpy array"""
    i32 = torch.int32 if isinstance(buf, torch.Tensor) else "int32"
    ints = buf[b * nl * 8:].view(i32)
    return buf[:b * nl * 8].reshape(b, nl, 8), ints[:b * nl].reshape(b, nl), ints[b * nl:b * nl + 1]


def _aux_map(t, name, b, device):
    """an optional [B,h,w] / [B,1,h,w] map of float32 or float64 -> (tensor, is_f64, h, w)"""
    if t is None:
        return None, 0, 0, 0
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"{name}: expected a float32 or float64 tensor")
    t = _chk(t.contiguous(), name, t.dtype)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.shape[0] != b or t.device != device or t.numel() == 0:
        raise RuntimeError(f"{name}: shape {tuple(t.shape)}: expected [{b},h,w] or [{b},1,h,w] on {device}")
    return t, int(t.dtype == torch.float64), t.shape[1], t.shape[2]


def eval_mask(disp_l, depth_l, max_disp, exclude_bg=True, robot_mask=None, realsense_depth=None, depth_hi=1.25):
    """test.py:112-117, 162-193 in one launch: disp_l, depth_l [B,1,H,W] float32; robot_mask / realsense_depth optional maps
    [B,h,w] or [B,1,h,w] of their own size, float32 or float64, read at the nearest-resize indices in their own type.
    mask = (0 < disp_l < max_disp) & (0 < depth_l < depth_hi if exclude_bg) & ((int)robot == 0) & (realsense > 0).
    Returns (mask [B,1,H,W], a bool view of the byte tensor the kernel wrote, count int32 [1] on the device).  No host sync."""
    d = _chk(disp_l, "disp_l")
    z = _chk(depth_l, "depth_l")
    if d.dim() != 4 or d.shape[1] != 1 or z.shape != d.shape or z.device != d.device:
        raise RuntimeError("disp_l and depth_l must be [B,1,H,W] of one shape")
    b, _, h, w = d.shape
    if d.numel() == 0:
        raise RuntimeError("disp_l is empty")
    robot, r64, hr, wr = _aux_map(robot_mask, "robot_mask", b, d.device)
    rs, s64, hs, ws = _aux_map(realsense_depth, "realsense_depth", b, d.device)
    mask = torch.empty(b, 1, h, w, dtype=torch.uint8, device=d.device)
    count = torch.empty(1, dtype=torch.int32, device=d.device)
    with torch.cuda.device(d.device):
        _call("az_eval_mask", _p(mask), _p(count), _p(d), _p(z), _p(robot), r64, hr, wr, _p(rs), s64, hs, ws, b, h, w,
              float(max_disp), 1 if exclude_bg else 0, float(depth_hi), _stream())
    return mask.view(torch.bool), count


# ----------------------------------------------------------------------------
# K18 ground truth from the right view, K19 error colour images
# ----------------------------------------------------------------------------
def gt_from_right(disp_r, extra=None, keep=None, *, scale_factor=0.5, size=None, lo=0.0, hi=float("inf"), check=False):
    """train.py:255-272 / test.py:91-110 in one launch: nearest resize of the right view's disparity disp_r [N,1,Hin,Win]
    (by scale_factor, or to size=(H, W)), truncation to an integer shift, scatter to the left view (smallest source column
    wins, holes 0) and the mask lo < disp_l < hi.  extra [N,Ce,Hin,Win]: channels warped by the same shifts; keep
    [N,Ck,Hin,Win]: channels resized only.  Returns (disp_l, extra_l, keep_s, mask, stats): extra_l / keep_s are None where
    the input was; mask is a bool view of the byte tensor the kernel wrote; stats is an int32 device tensor
    [number of disparities that are <= -1 or not finite, number of mask pixels].  No host sync -- unless check=True, which
    reads stats[0] and raises AssertionError as the reference's sign assertion would."""
    d = _chk(disp_r, "disp_r")
    if d.dim() != 4 or d.shape[1] != 1:
        raise RuntimeError("disp_r must be [N,1,H,W]")
    n, _, hin, win = d.shape
    chans = []
    for t, name in ((extra, "extra"), (keep, "keep")):
        if t is not None:
            _chk(t, name)
            if t.dim() != 4 or t.shape[0] != n or tuple(t.shape[2:]) != (hin, win) or t.device != d.device:
                raise RuntimeError(f"{name}: shape {tuple(t.shape)} does not match disp_r {tuple(d.shape)}")
        chans.append(0 if t is None else t.shape[1])
    ce, ck = chans
    if size is not None:  # ATen: scale = in / out in float when a size is given
        h, w = (int(s) for s in size)
        if h < 1 or w < 1:
            raise RuntimeError(f"size {tuple(size)} must be positive")
        scale_h, scale_w = hin / h, win / w
    else:  # ... and 1 / scale_factor with recompute_scale_factor=False; the output size is floor(in * scale_factor)
        sh, sw = scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor)
        h, w = int(hin * float(sh)), int(win * float(sw))
        scale_h, scale_w = 1.0 / float(sh), 1.0 / float(sw)
    disp_l = d.new_empty(n, 1, h, w)
    extra_l = d.new_empty(n, ce, h, w) if ce else None
    keep_s = d.new_empty(n, ck, h, w) if ck else None
    mask = torch.empty(n, 1, h, w, dtype=torch.uint8, device=d.device)
    stats = torch.zeros(2, dtype=torch.int32, device=d.device)
    with torch.cuda.device(d.device):
        _call("az_gt_from_right", _p(disp_l), _p(extra_l), _p(keep_s), _p(mask), _p(stats), _p(d), _p(extra), _p(keep),
              n, ce, ck, hin, win, h, w, scale_h, scale_w, float(lo), float(hi), _stream())
    if check:  # the one host sync, on request
        bad = int(stats[0])
        if bad:
            raise AssertionError(f"gt_from_right: {bad} disparities are <= -1 or not finite (warp_ops.py:73-77 asserts one sign)")
    return disp_l, extra_l, keep_s, mask.view(torch.bool), stats


def error_img(est, gt, mask, kind="disp", abs_thres=None, rel_thres=0.05, channels_first=True):
    """utils/util.py:185-244 for every image of a batch, on the device: est, gt, mask of one shape with B * H * W elements
    ([B,H,W] or [B,1,H,W]; mask bool or uint8) -> [B,3,H,W] (channels_first, train.py:354-356) or [B,H,W,3] float32.
    kind "disp" (abs_thres 3.0, rel_thres 0.05) or "depth" (abs_thres 1.0).  No host sync."""
    if kind not in ("disp", "depth"):
        raise RuntimeError(f"kind must be 'disp' or 'depth', got {kind!r}")
    e = _chk(est, "est")
    g = _chk(gt, "gt")
    if e.shape != g.shape:
        raise RuntimeError(f"est {tuple(e.shape)} and gt {tuple(g.shape)} must have identical shapes")
    if mask is None:
        raise RuntimeError("mask is required")
    m = _mask_u8(mask, g)
    if not (e.dim() == 3 or (e.dim() == 4 and e.shape[1] == 1)):
        raise RuntimeError("est, gt and mask must be [B,H,W] or [B,1,H,W]")
    b, (h, w) = e.shape[0], e.shape[-2:]
    if abs_thres is None:
        abs_thres = 3.0 if kind == "disp" else 1.0
    out = e.new_empty((b, 3, h, w) if channels_first else (b, h, w, 3))
    with torch.cuda.device(e.device):
        _call("az_error_img", _p(out), _p(e), _p(g), _p(m), 0 if kind == "disp" else 1, float(abs_thres), float(rel_thres),
              1 if channels_first else 0, b, h, w, _stream())
    return out


# ----------------------------------------------------------------------------
# K24 the six result images of a test batch as RGBA bytes
# ----------------------------------------------------------------------------
RESULT_PANELS = ("pred_disp", "gt_disp", "pred_disp_abs_err_cmap", "pred_depth", "gt_depth", "pred_depth_abs_err_cmap")


def result_images(pred_disp, gt_disp, gt_depth, mask, focal_x_baseline, max_disp, depth_hi=1.25, disp_abs_thres=3.0,
                  disp_rel_thres=0.05, depth_scale=1000.0, depth_abs_thres=1.0, return_flags=False):
    """test.py:235-260 with utils/test_util.py:59-107 save_img for every image of a batch, on the device: the bytes plt.imsave
    writes for pred_disp, gt_disp, the disparity error image, pred_depth = focal_x_baseline / pred_disp, gt_depth and the depth
    error image (RESULT_PANELS, save_img's order) -> uint8 [B,6,H,W,4] RGBA.  pred_disp: any [B,1,H,W] float32 view whose last
    stride is 1 (the crop of a padded prediction, test.py:208, is not copied); gt_disp, gt_depth contiguous [B,1,H,W]; mask
    bool or uint8; focal_x_baseline one float32 per image.  return_flags: also the int32 [B] word of az_result_images (bit m:
    panel m of the image has a masked pixel).  No host sync."""
    if not isinstance(pred_disp, torch.Tensor) or pred_disp.dim() != 4 or pred_disp.shape[1] != 1:
        raise RuntimeError("pred_disp must be a [B,1,H,W] tensor")
    b, _, h, w = pred_disp.shape
    if pred_disp.numel() == 0:
        raise RuntimeError("pred_disp is empty")
    if w > 1 and pred_disp.stride(3) != 1:
        raise RuntimeError("pred_disp: the last dimension must have stride 1")
    if pred_disp.device.type != "cuda":
        raise RuntimeError(f"pred_disp: must live on the GPU (got {pred_disp.device}); the HIP path has no CPU fallback")
    if pred_disp.dtype != torch.float32:
        raise RuntimeError(f"pred_disp: expected torch.float32, got {pred_disp.dtype}")
    # a dimension of size 1 has no stride to speak of: give it the contiguous one
    row_stride = pred_disp.stride(2) if h > 1 else w
    img_stride = pred_disp.stride(0) if b > 1 else h * row_stride
    gd = _chk(gt_disp, "gt_disp")
    gz = _chk(gt_depth, "gt_depth")
    if gd.shape != pred_disp.shape or gz.shape != pred_disp.shape or gd.device != pred_disp.device or gz.device != gd.device:
        raise RuntimeError("pred_disp, gt_disp and gt_depth must be [B,1,H,W] of one shape on one device")
    if mask is None:
        raise RuntimeError("mask is required")
    m = _mask_u8(mask, gd)
    fb = _chk(focal_x_baseline.contiguous().reshape(-1), "focal_x_baseline")
    if fb.numel() != b:
        raise RuntimeError("focal_x_baseline must hold one value per batch element")
    out = torch.empty(b, 6, h, w, 4, dtype=torch.uint8, device=gd.device)
    flags = torch.empty(b, dtype=torch.int32, device=gd.device)
    with torch.cuda.device(gd.device):
        _call("az_result_images", _p(out), _p(flags), _p(pred_disp), row_stride, img_stride, _p(gd), _p(gz), _p(m), _p(fb),
              float(max_disp), float(depth_hi), float(disp_abs_thres), float(disp_rel_thres), float(depth_scale),
              float(depth_abs_thres), b, h, w, _stream())
    return (out, flags) if return_flags else out


# ----------------------------------------------------------------------------
# K25 millimetre depth maps to labels, K26 a test item's network inputs
# ----------------------------------------------------------------------------
_DEPTH_DTYPES = {torch.uint16: "AZ_DEPTH_U16", torch.int32: "AZ_DEPTH_I32"}


def _per_item_f64(value, b, name, device):
    """one float64 per item on the device, from a number (filled on the device: no host round trip) or a tensor of B values"""
    if isinstance(value, torch.Tensor):
        if value.device != device:
            raise RuntimeError(f"{name}: must live on the device of the depth maps ({device}), got {value.device}")
        if value.numel() != b:
            raise RuntimeError(f"{name}: expected {b} values (one per item), got {value.numel()}")
        return value.reshape(b).to(torch.float64).contiguous()
    return torch.full((b,), float(value), dtype=torch.float64, device=device)


def depth_labels(depth_l_mm, depth_r_mm, focal_length, baseline, origin=None, window=None):
    """messytable.py:197-213, 256-261, 281-284 in one launch: depth_l_mm, depth_r_mm [B,H2,W2] raw millimetres, uint16 or
    int32; focal_length, baseline a number or B values on the device (taken as float64) -> (disp_l, depth_l, disp_r, depth_r),
    each [B,1,h2,w2] float32 with numpy's bits: depth = v / 1000 and disp = focal_length * baseline / depth where v > 0, else
    0, in float64, rounded once.  origin None: the whole map; or int32 [B,2] on the device, (y0, x0) per item, with window =
    (h2, w2): the training crop, clamped into the map on the device.  No host sync."""
    if not isinstance(depth_l_mm, torch.Tensor) or depth_l_mm.dtype not in _DEPTH_DTYPES:
        raise RuntimeError("depth_l_mm: expected a torch.uint16 or torch.int32 tensor")
    a = _chk(depth_l_mm, "depth_l_mm", depth_l_mm.dtype)
    b_ = _chk(depth_r_mm, "depth_r_mm", a.dtype)
    if a.dim() != 3 or a.numel() == 0 or b_.shape != a.shape or b_.device != a.device:
        raise RuntimeError("depth_l_mm and depth_r_mm must be non-empty [B,H2,W2] of one shape on one device")
    n, hh, ww = a.shape
    if origin is None:
        if window is not None and tuple(int(s) for s in window) != (hh, ww):
            raise RuntimeError("window needs an origin")
        h2, w2 = hh, ww
    else:
        if window is None:
            raise RuntimeError("origin needs a window size (h2, w2)")
        h2, w2 = (int(s) for s in window)
        if not 0 < h2 <= hh or not 0 < w2 <= ww:
            raise RuntimeError(f"window {(h2, w2)} does not fit the {hh} x {ww} map")
        origin = _chk(origin, "origin", torch.int32)
        if tuple(origin.shape) != (n, 2) or origin.device != a.device:
            raise RuntimeError(f"origin: expected int32 [{n},2] on {a.device}, got {tuple(origin.shape)} on {origin.device}")
    fl = _per_item_f64(focal_length, n, "focal_length", a.device)
    bl = _per_item_f64(baseline, n, "baseline", a.device)
    outs = [torch.empty(n, 1, h2, w2, dtype=torch.float32, device=a.device) for _ in range(4)]
    with torch.cuda.device(a.device):
        _call("az_depth_labels", *(_p(o) for o in outs), _p(a), _p(b_), _lib.CONST[_DEPTH_DTYPES[a.dtype]], _p(fl), _p(bl),
              _p(origin), n, hh, ww, h2, w2, _stream())
    return tuple(outs)


def test_images(src, src_second=None, size=None, pad=(0, 0)):
    """test.py:118-131, 141-146 in one launch: src (and src_second, the other view, of the same form) either [N,3,Hin,Win]
    float32, normalised, or [N,Hin,Win] uint8 grey levels, normalised per tap as augment_images normalises them -> float32
    [N (+ N_second),3,H + top,W + right]: ATen's bilinear resize (align_corners=False) to size = (H, W) -- None: the
    source's size, the image is only padded -- below `top` rows and left of `right` columns of +0.0, pad = (top, right).
    src's images come first.  No host sync."""
    if not isinstance(src, torch.Tensor) or src.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError("src: expected a torch.float32 or torch.uint8 tensor")
    u8 = src.dtype == torch.uint8
    srcs = [_chk(src, "src", src.dtype)] + ([] if src_second is None else [_chk(src_second, "src_second", src.dtype)])
    for t in srcs:
        if t.dim() != (3 if u8 else 4) or (not u8 and t.shape[1] != 3) or t.numel() == 0:
            raise RuntimeError(f"a source of {src.dtype} must be a non-empty {'[N,Hin,Win]' if u8 else '[N,3,Hin,Win]'}, got "
                               f"{tuple(t.shape)}")
        if t.shape[-2:] != src.shape[-2:] or t.device != src.device:
            raise RuntimeError("src and src_second must have one image size and one device")
    hin, win = src.shape[-2:]
    h, w = (hin, win) if size is None else (int(s) for s in size)
    top, right = (int(s) for s in pad)
    if h < 1 or w < 1 or top < 0 or right < 0:
        raise RuntimeError(f"size {(h, w)} must be positive and pad {(top, right)} non-negative")
    n, n2 = srcs[0].shape[0], (srcs[1].shape[0] if len(srcs) == 2 else 0)
    out = torch.empty(n + n2, 3, h + top, w + right, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _call("az_test_images", _p(out), _p(srcs[0]), _p(srcs[1]) if n2 else None, int(u8), n, n2, hin, win, h, w, top,
              right, _stream())
    return out


test_images.__test__ = False  # (pytest would collect a function of this name from a test module that imports it)


# ----------------------------------------------------------------------------
# K15 RAFT-Stereo convex upsampling
# ----------------------------------------------------------------------------
def _chk_mask(mask, name="mask"):
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.float16:
        return _chk(mask, name, torch.float16)
    return _chk(mask, name)


class _ConvexUp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask, factor, d_out, sign):
        flow = _chk(flow.contiguous(), "flow")
        mask = _chk_mask(mask.contiguous())
        if flow.dim() != 4 or mask.dim() != 4:
            raise RuntimeError("flow must be [N,D,h,w] and mask [N,9*factor*factor,h,w]")
        n, d, h, w = flow.shape
        if mask.shape[0] != n or tuple(mask.shape[2:]) != (h, w):
            raise RuntimeError(f"mask {tuple(mask.shape)} does not match flow {tuple(flow.shape)}")
        up = flow.new_empty(n, d_out, factor * h, factor * w)
        ctx.args = (int(mask.dtype == torch.float16), n, d, d_out, h, w, factor, mask.shape[1], sign)
        with torch.cuda.device(flow.device):
            _call("az_convex_up_fwd", _p(up), _p(flow), _p(mask), *ctx.args, _stream())
        ctx.save_for_backward(flow, mask)  # the inputs only: the softmax is recomputed, nothing of mask size is kept
        return up

    @staticmethod
    def backward(ctx, g):
        flow, mask = ctx.saved_tensors
        g = _chk(g.contiguous(), "grad_up")
        if g.data_ptr() % 16:  # a contiguous view at an odd storage offset: the kernel reads g_up as float4
            g = g.clone()
        _, n, _, d_out, h, w = ctx.args[:6]
        gm, gf = torch.empty_like(mask), torch.empty_like(flow)
        nbytes = _lib.lib().az_convex_up_bwd_workspace(n, d_out, h, w)
        ws = flow.new_empty(nbytes // 4)
        with torch.cuda.device(flow.device):
            _call("az_convex_up_bwd", _p(gm), _p(gf), _p(ws), nbytes, _p(g), _p(flow), _p(mask), *ctx.args, _stream())
        return gf, gm, None, None, None


def convex_upsample(flow, mask, factor, channels=None, negate=False):
    """RAFTStereo.upsample_flow as one kernel: flow [N,D,h,w] fp32, mask [N,9*factor^2,h,w] fp32 or fp16 ->
    [N,channels,factor*h,factor*w] fp32, the softmax-weighted sum of the 3x3 neighbourhood of factor*flow.
    channels (default D) < D computes the leading channels only (`flow_up[:, :1]`); negate returns the
    negated result (`pred_disp = -output[-1]`).  One autograd node; nothing of mask size is saved."""
    d_out = flow.shape[1] if channels is None else int(channels)
    return _ConvexUp.apply(flow, mask, int(factor), d_out, -1 if negate else 1)


# ----------------------------------------------------------------------------
# K16 sequence loss
# ----------------------------------------------------------------------------
class _SeqLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, valid, weights, max_flow, tsign, check, *preds):
        gt = _chk(gt.contiguous(), "flow_gt")
        if valid.shape != gt.shape:
            raise RuntimeError(f"valid: shape {tuple(valid.shape)} != {tuple(gt.shape)}")
        if valid.dtype == torch.float32:
            valid = _chk(valid.contiguous(), "valid")
        else:
            valid = _mask_u8(valid.contiguous(), gt, "valid")
        ps = []
        for i, p in enumerate(preds):
            p = _chk(p.contiguous(), f"flow_preds[{i}]")
            if p.shape != gt.shape:
                raise RuntimeError(f"flow_preds[{i}]: shape {tuple(p.shape)} != {tuple(gt.shape)}")
            ps.append(p)
        n = len(ps)
        acc = torch.zeros(n, 3, dtype=torch.float64, device=gt.device)
        ctx.args = (int(valid.dtype == torch.uint8), float(max_flow), tsign)
        with torch.cuda.device(gt.device):
            for i, p in enumerate(ps):
                _call("az_seq_loss_fwd", acc.data_ptr() + 24 * i, _p(p), _p(gt), _p(valid), *ctx.args, gt.numel(),
                      _stream())
        if check:  # the one host sync, on request: losses.py:53-56 asserts every prediction finite
            bad = acc[:, 2].tolist()
            if any(bad):
                raise AssertionError(f"sequence_loss: non-finite values in flow_preds {[i for i, b in enumerate(bad) if b]}")
        # w_i from an on-device arange: a host list would be a blocking copy.  0/0 = nan, as the reference's empty mean
        gp, k = weights
        wts = torch.pow(gp, (k - torch.arange(n, device=gt.device)).to(torch.float64))
        loss = (wts * acc[:, 0] / acc[:, 1]).sum().to(torch.float32)
        ctx.save_for_backward(gt, valid, acc, *ps)
        ctx.weights = [gp ** (k - i) for i in range(n)]
        return loss

    @staticmethod
    def backward(ctx, gloss):
        gt, valid, acc, *ps = ctx.saved_tensors
        gloss = _chk(gloss.contiguous().to(torch.float32).reshape(1), "grad_loss")
        grads = [torch.empty_like(p) for p in ps]
        with torch.cuda.device(gt.device):
            for i, (p, g) in enumerate(zip(ps, grads)):
                _call("az_seq_loss_bwd", _p(g), _p(p), _p(gt), _p(valid), *ctx.args, _p(gloss),
                      acc.data_ptr() + 24 * i, ctx.weights[i], gt.numel(), _stream())
        return (None,) * 6 + tuple(grads)


def sequence_loss(flow_preds, flow_gt, valid, loss_gamma=0.9, max_flow=700, check=False, *, disparity=False):
    """sum_i w_i * mean |flow_preds[i] - (-flow_gt)| over the pixels with valid >= 0.5 and |flow_gt| < max_flow
    (utils/losses.py:34-69), w_i = g^(n-1-i), g = loss_gamma^(15/(n-1)).  For n = 1 the reference divides by zero;
    here the single prediction has weight 1.  All maps [B,1,H,W]; valid fp32, uint8 or bool.
    One autograd node for the whole list, one accumulator vector, n forward and n backward launches, no boolean
    indexing and no host sync -- unless check=True, which reads the non-finite counter (one sync) and raises
    AssertionError as the reference's assertions would.  disparity=True: the predictions already are
    disparities (convex_upsample(..., negate=True)), so the target is +flow_gt."""
    preds = list(flow_preds)
    n = len(preds)
    if n < 1:
        raise AssertionError("sequence_loss needs at least one prediction")
    gp = float(loss_gamma) ** (15.0 / (n - 1)) if n > 1 else 1.0
    return _SeqLoss.apply(flow_gt, valid, (gp, n - 1), max_flow, 1 if disparity else -1, bool(check), *preds)
