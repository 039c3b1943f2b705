"""RAFT-Stereo ConvGRU update on the MI355X convolution kernels -- drop-in for the class `ConvGRU` of the
reference module nets/raft/update.py:19-41 (same constructor, parameter names `convz / convr / convq` with
bias, so reference checkpoints load unchanged; same forward signature `(h, cz, cr, cq, *x_list)`).

The reference runs the update block under autocast (nets/raft/raft_stereo.py:142-172): convolution operands
are rounded to 16 bits, products accumulated in fp32.  Without autograd this module does the same on the plain
bf16 MFMA path (include/azhip.h `az_conv2d_bf16_fwd`) in TWO launches per update:

    zr = sigmoid(conv_{z|r}([h, x]) + bias + [cz, cr])          one 3x3 convolution, 2*hidden output channels
    h' = (1 - z) * h + z * tanh(conv_q([r*h, x]) + bias + cq)   gate arithmetic in the convolution's epilogue

The gates, context terms and the state itself stay fp32 (the reference keeps them in 16 bits between the
convolutions, so this path is the more accurate of the two; tests/test_gpu_raft_gru.py measures both against an
fp64 evaluation).  With autograd enabled (training) the convolutions keep that arithmetic in BOTH directions, as the
reference's autocast + GradScaler training does (train.py:303-309, configs/config.py:24 MIXED_PRECISION = True):
forward, input gradient (the same kernel on the flipped weight image) and weight gradient (az_conv2d_wgrad_bf16) round
their operands to bf16 once, one MFMA per block, fp32 accumulation; the gates are fp32 torch operators.
`ConvGRU.train_arithmetic = "bf16x6"` restores round 3's fp32-class convolutions (six MFMAs per product).

The file is deliberately not called update.py: the rest of that reference module (motion encoder, flow head,
multi-level block) is ordinary torch code outside this path and keeps resolving from the reference tree; the
one-line edit there is `from nets.raft.gru import ConvGRU`.
"""
import ctypes
import os
import weakref

import torch
import torch.nn as nn

from activezero_amd import amax, conv2d
from activezero_amd.packing import CACHE_LOCK, cache_get, cache_key, cache_put, memo
from activezero_amd.ops import _call, _chk, _p, _stream

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_GRU = range(5)
_ARITH = ("bf16", "f16x1")  # by `h1`: the names of the one-part arithmetics in profiler scopes and conv2d._WGRAD
_PACK_CACHE = {}
_CTX_CACHE = {}
CTX_CONVERSIONS = 0  # context-row conversions so far (tests: one per step and GRU level, whatever the inputs' dtype)


def _context_rows(cz, cr, cq):
    """fp32 rows [cz | cr] and cq of the context terms -- the same tensors in all 22 updates of a step
    (raft_stereo.py:142-172) -- converted once.  Keyed on the CALLER's tensors (under the reference's mixed precision they
    arrive as fp16, and a key taken after `.float()` would never hit); an entry holds detached rows and weak references:
    it neither keeps the step's autograd graph alive nor answers for a recycled address, and entries whose sources have
    died are dropped at the next conversion."""
    global CTX_CONVERSIONS
    key = cache_key(cz, cr, cq)
    hit = cache_get(_CTX_CACHE, key)
    if hit is not None and all(r() is t for r, t in zip(hit[1], (cz, cr, cq))):
        return hit[0]
    with torch.no_grad():
        czr = torch.cat([cz.detach().permute(0, 2, 3, 1), cr.detach().permute(0, 2, 3, 1)], -1).float().contiguous()
        cqr = _rows(cq.detach())
    CTX_CONVERSIONS += 1
    with CACHE_LOCK:
        for k in [k for k, v in _CTX_CACHE.items() if any(r() is None for r in v[1])]:
            del _CTX_CACHE[k]
    cache_put(_CTX_CACHE, key, ((czr, cqr), tuple(weakref.ref(t) for t in (cz, cr, cq))), 4)
    return czr, cqr


# ---- [h | x_0 | x_1 ..] rows in one launch (az_rows_concat) -----------------------------------------------------------------
# AZ_GRU_ASSEMBLE=0 (read once): one torch slice assignment per source, as in round 4 (A/B runs)
ASSEMBLE = os.environ.get("AZ_GRU_ASSEMBLE", "1") != "0"
_ROWS_CACHE = {}
_SEEN_ONCE = {}
ROW_CONVERSIONS = 0  # cached channels-last copies made so far (tests)


def _cached_rows(t):
    """a channels-last fp32 copy of an NCHW tensor that comes back update after update (the context features: the same tensor
    in all 22 updates of a step), made once; weak-referenced like _context_rows' entries"""
    global ROW_CONVERSIONS
    key = cache_key(t)
    hit = cache_get(_ROWS_CACHE, key)
    if hit is not None and hit[1]() is t:
        return hit[0]
    with torch.no_grad():
        r = t.detach().permute(0, 2, 3, 1).float().contiguous()
    ROW_CONVERSIONS += 1
    with CACHE_LOCK:
        for k in [k for k, v in _ROWS_CACHE.items() if v[1]() is None]:
            del _ROWS_CACHE[k]
    cache_put(_ROWS_CACHE, key, (r, weakref.ref(t)), 8)
    return r


def _source(t):
    """(tensor that owns the memory, kind) of one input for az_rows_concat: kind 0 = dense rows, 1 = dense NCHW image; None:
    neither (the caller falls back to torch)"""
    if t.dtype != torch.float32:
        return None
    if t.permute(0, 2, 3, 1).is_contiguous():
        return t, 0
    if not t.is_contiguous():
        return None
    if t.shape[1] <= 128:
        # an image the kernel can transpose on the way -- unless it is the same tensor as last time: then a cached copy is cheaper
        key = cache_key(t)
        seen, rows = cache_get(_SEEN_ONCE, key), cache_get(_ROWS_CACHE, key)
        # (an entry left by a dead tensor whose address this one has recycled answers for neither)
        if (seen is None or seen[0]() is not t) and (rows is None or rows[1]() is not t):
            cache_put(_SEEN_ONCE, key, (weakref.ref(t),), 8)
            return t, 1
    return _cached_rows(t), 0


def _assemble(h, xs):
    """hx rows [B,H,W,C_h + sum C_x] and, per x, whether it entered as an NCHW image (its gradient leaves the same way)"""
    b, c, hh, ww = h.shape
    ct = c + sum(t.shape[1] for t in xs)
    hx = h.new_empty(b, hh, ww, ct)
    srcs = [_source(t) for t in (h, *xs)] if (ASSEMBLE and len(xs) <= 3) else [None]
    if any(s is None for s in srcs) or any(t.shape[1] % 4 for t in (h, *xs)):
        hx[..., :c] = h.permute(0, 2, 3, 1)
        at = c
        for t in xs:
            hx[..., at:at + t.shape[1]] = t.permute(0, 2, 3, 1)
            at += t.shape[1]
        return hx, [False] * len(xs)
    n = len(srcs)
    ptrs = (ctypes.c_void_p * n)(*[s[0].data_ptr() for s in srcs])
    chans = (ctypes.c_int * n)(*[t.shape[1] for t in (h, *xs)])
    kinds = (ctypes.c_int * n)(*[s[1] for s in srcs])
    _call("az_rows_concat", _p(hx), b * hh * ww, hh * ww, n, ptrs, chans, kinds, _stream())
    return hx, [s[1] == 1 for s in srcs[1:]]


def _pack(weights, k, flipped=False, cache=True):
    """[Cout_i, Cin, 3, 3] weights (concatenated along Cout) -> the one-part image of kernel k (conv2d.ONE_BF16 / ONE_H1):
    the forward's, or with flipped = True the input gradient's (taps flipped, channel roles swapped); unscaled, as
    autocast casts them.  cache = False: not memoised (the call site has autograd on a derived weight)."""
    def make():
        w = torch.cat([x.detach().float() for x in weights], 0).contiguous()
        cout, cin = w.shape[0], w.shape[1]
        if not flipped and (cin % 16 or cout % 32):  # (the flipped image's counts: the library's own check)
            raise RuntimeError(f"ConvGRU: unsupported channel counts cin={cin} cout={cout} (need cin % 16 == 0, cout % 32 == 0)")
        if flipped:
            return conv2d._pack_image(k, w, cout, cin, 9, cin * 9, 3, 3, True)[0]
        return conv2d._pack_image(k, w, cin, cout, cin * 9, 9, 3, 3, False)[0]

    return memo(_PACK_CACHE, (k.fwd, bool(flipped)) + cache_key(*weights) if cache else None, make, tuple(weights), 64)


def _pack_bf16(weights, cache):
    return _pack(weights, conv2d.ONE_BF16, False, cache)


def conv3x3_bf16(xr, packed, cin, cout, bias=None, residual=None, act=ACT_NONE, gate_z=None, gate_h=None, h1=False,
                 in_amax=None):
    """xr [B,H,W,>=cin] fp32 rows -> act(conv3x3(xr[..., :cin]) + bias + residual) as [B,H,W,cout] rows.
    h1: one FP16 part per operand (az_conv2d_h1_fwd; `packed` from az_conv2d_pack_weights_h1) instead of one bf16 part;
    in_amax: amax array of xr for a power-of-two operand scale (gradient operands), None = rounded as it is."""
    k, am = (conv2d.ONE_H1, (in_amax, None)) if h1 else (conv2d.ONE_BF16, None)
    return conv2d._launch(k, xr, packed, cin, cout, amax=am, res=residual, bias=bias, act=act,
                          tag=f"gru_conv3x3_{_ARITH[h1]}", gates=(gate_z, gate_h))


def _rows(t):
    return _chk(t.float().permute(0, 2, 3, 1).contiguous(), "ConvGRU input")


class _Conv3x3Bf16(torch.autograd.Function):
    """conv3x3(x, w) + bias on [B,C,H,W] tensors in channels_last memory, every operand rounded to bf16 once (forward,
    input gradient, weight gradient), fp32 accumulation and fp32 results"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xr = _chk(conv2d.rows(x), "x")
        cout, cin = weight.shape[0], weight.shape[1]
        with torch.cuda.device(x.device):
            y = conv3x3_bf16(xr, _pack((weight,), conv2d.ONE_BF16, cache=False), cin, cout,
                             bias.detach().float().contiguous() if bias is not None else None)
        ctx.save_for_backward(xr, weight)
        ctx.has_bias = bias is not None
        return conv2d.image(y)

    @staticmethod
    def backward(ctx, gy):
        xr, weight = ctx.saved_tensors
        cout, cin = weight.shape[0], weight.shape[1]
        gr = _chk(conv2d.rows(gy), "grad_y")
        gx = gw = gb = None
        with torch.cuda.device(gy.device):
            if ctx.needs_input_grad[0]:  # the same convolution on gy with flipped taps and swapped channel roles
                gx = conv2d.image(conv3x3_bf16(gr, _pack((weight,), conv2d.ONE_BF16, True, cache=False), cout, cin))
            if ctx.needs_input_grad[1]:
                gw = conv2d._wgrad(gr, xr, cout, cin, cout, cin, 3, 3, 1, tag="gru_wgrad_bf16", arith="bf16")
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = gr.sum(dim=(0, 1, 2))
        return gx, gw, gb


class _GRUStepBf16(torch.autograd.Function):
    """One ConvGRU update (update.py:32-41) under autograd as ONE node: the two convolutions, their input and weight gradients
    in the reference's autocast arithmetic (bf16 operands, fp32 accumulation; `_Conv3x3Bf16`'s kernels), the gates in fp32
    in the convolution epilogues (forward) and in five streaming kernels (az_gru_gates.hip).  Same arithmetic as the
    operator-by-operator form ("bf16_ops"), a quarter of its launches and tensor passes."""

    @staticmethod
    def forward(ctx, h1, h, cz, cr, cq, czr, cqr, wz, wr, wq, bz, br, bq, *xs):
        """h1: True = "f16x1" (one fp16 part per operand: the reference's float16 autocast), False = "bf16".
        czr / cqr: the fp32 rows of the context terms (`_context_rows`; cz / cr / cq themselves only receive gradients)"""
        ctx.h1 = h1
        k = conv2d.ONE_H1 if h1 else conv2d.ONE_BF16
        c, ci = h.shape[1], sum(t.shape[1] for t in xs)
        with torch.cuda.device(h.device):
            b, _, hh, ww = h.shape
            npix = b * hh * ww
            hx, as_image = _assemble(h, xs)  # [h | x_0 | x_1 ..] rows in one launch (az_rows_concat)
            ctx.as_image = as_image
            bzr = torch.cat([bz, br]).detach().float().contiguous()
            zr = conv3x3_bf16(hx, _pack((wz, wr), k), c + ci, 2 * c, bzr, czr, ACT_SIGMOID, h1=h1)
            rhx = torch.empty_like(hx)
            _call("az_gru_rh", _p(rhx), _p(zr), _p(hx), npix, c, ci, _stream())
            q = conv3x3_bf16(rhx, _pack((wq,), k), c + ci, c, bq.detach().float().contiguous(), cqr, ACT_TANH, h1=h1)
            hn = torch.empty_like(q)
            _call("az_gru_out", _p(hn), _p(zr), _p(q), _p(hx), npix, c, ci, _stream())
        ctx.save_for_backward(hx, rhx, zr, q, wz, wr, wq)
        ctx.dims = (c, ci, tuple(t.shape[1] for t in xs))
        return conv2d.image(hn)

    @staticmethod
    def backward(ctx, g_hn):
        hx, rhx, zr, q, wz, wr, wq = ctx.saved_tensors
        c, ci, xsplit = ctx.dims
        b, hh, ww, ct = hx.shape
        npix = b * hh * ww
        need = ctx.needs_input_grad
        with torch.cuda.device(g_hn.device):
            # the incoming gradient: channels-last memory when it comes from the next update alone (a view of its dh), a dense NCHW
            # image as soon as a torch operator had a hand in it (the flow head, a loss term): transposed by one kernel then, and
            # dh leaves in the layout g_hn came in, so that the engine's sum with that other gradient stays a contiguous add
            g_is_image = ASSEMBLE and g_hn.dtype == torch.float32 and g_hn.is_contiguous() and not g_hn.permute(0, 2, 3, 1).is_contiguous() \
                and c <= 128 and c % 4 == 0
            if g_is_image:
                g = g_hn.new_empty(b, hh, ww, c)
                one = (ctypes.c_void_p * 1)(g_hn.data_ptr())
                _call("az_rows_concat", _p(g), npix, hh * ww, 1, one, (ctypes.c_int * 1)(c), (ctypes.c_int * 1)(1), _stream())
            else:
                g = _chk(conv2d.rows(g_hn), "grad")
            dq = torch.empty_like(q)
            dzr = torch.empty_like(zr)
            dh_acc = torch.empty_like(q)
            h1 = ctx.h1
            # f16x1: the gradient operands are scaled by a power of two from their amax (taken by the gate kernels that write
            # them) before the fp16 rounding -- the job GradScaler does for the reference (train.py:303-309)
            am_q = amax.ZEROS.take(q) if h1 else None
            am_z = amax.ZEROS.take(q) if h1 else None
            k = conv2d.ONE_H1 if h1 else conv2d.ONE_BF16
            _call("az_gru_bwd1", _p(dq), _p(dzr), _p(dh_acc), _p(g), _p(zr), _p(q), _p(hx), npix, c, ci, _p(am_q), _p(am_z), _stream())
            d_rhx = conv3x3_bf16(dq, _pack((wq,), k, True), c, ct, h1=h1, in_amax=am_q)
            _call("az_gru_bwd2", _p(dzr), _p(dh_acc), _p(d_rhx), _p(zr), _p(hx), npix, c, ci, _p(am_z), _stream())
            d_hx = conv3x3_bf16(dzr, _pack((wz, wr), k, True), 2 * c, ct, h1=h1, in_amax=am_z)
            dh = torch.empty_like(q)
            dx = hx.new_empty(b, hh, ww, ci)
            _call("az_gru_bwd3", _p(dh), _p(dx), _p(dh_acc), _p(d_rhx), _p(d_hx), npix, c, ci, _stream())

            def wgrad(go, xin, cout, go_amax):
                return conv2d._wgrad(go, xin, cout, ct, cout, ct, 3, 3, 1, tag=f"gru_wgrad_{_ARITH[h1]}",
                                     amax=(go_amax, None) if h1 else None, arith=_ARITH[h1])

            gwz = gwr = gwq = gbz = gbr = gbq = None
            if need[7] or need[8]:
                gwzr = wgrad(dzr, hx, 2 * c, am_z)
                gwz, gwr = gwzr[:c], gwzr[c:]
            if need[9]:
                gwq = wgrad(dq, rhx, c, am_q)
            if need[10] or need[11]:
                gbzr = dzr.sum(dim=(0, 1, 2))
                gbz, gbr = gbzr[:c], gbzr[c:]
            if need[12]:
                gbq = dq.sum(dim=(0, 1, 2))
            img = lambda t: t.permute(0, 3, 1, 2)
            gxs, at = [], 0
            for i, n in enumerate(xsplit):
                if need[13 + i] and ctx.as_image[i] and n <= 128:
                    # the input came as a dense NCHW image: its consumer takes the gradient that way (the lookup's backward calls
                    # .contiguous() on it): transposed here by one kernel instead of torch's strided copy
                    gi = dx.new_empty(b, n, hh, ww)
                    _call("az_rows_slice_to_image", _p(gi), _p(dx), npix, hh * ww, ci, at, n, _stream())
                    gxs.append(gi)
                else:
                    gxs.append(img(dx[..., at:at + n]) if need[13 + i] else None)
                at += n
            g_h = None
            if need[1]:
                if g_is_image:
                    g_h = dh.new_empty(b, c, hh, ww)
                    _call("az_rows_slice_to_image", _p(g_h), _p(dh), npix, hh * ww, c, 0, c, _stream())
                else:
                    g_h = img(dh)
            return (None, g_h, img(dzr[..., :c]) if need[2] else None, img(dzr[..., c:]) if need[3] else None,
                    img(dq) if need[4] else None, None, None, gwz, gwr, gwq, gbz, gbr, gbq, *gxs)


class ConvGRU(nn.Module):
    # Arithmetic of the convolutions under autograd (the gates are fp32 in every mode):
    #   "f16x1"    one FP16 part per operand, fp32 accumulation: what the reference's torch.cuda.amp.autocast computes on CUDA
    #              (raft_stereo.py:14; GradScaler's job done by a power-of-two scale from each gradient operand's amax); one fused
    #              autograd node per update.  Default since round 5.
    #   "bf16"     one BF16 part (round 4's default): the same node, operands rounded 8x COARSER than the reference does --
    #              its gradients sit 1.2-2.8e-3 from the fp64 ones where the reference's fp16 autocast sits 3-7e-4 (G12).
    #   "bf16_ops" the bf16 arithmetic operator by operator (first round-4 form); "bf16x6": fp32-class convolutions (round 3)
    train_arithmetic = "f16x1"

    def __init__(self, hidden_dim, input_dim, kernel_size=3):
        super().__init__()
        if kernel_size != 3:
            raise RuntimeError("ConvGRU: the reference only instantiates kernel_size=3 (update.py:119-126)")
        self.hidden_dim, self.input_dim = hidden_dim, input_dim
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)

    def forward(self, h, cz, cr, cq, *x_list):
        if h.device.type != "cuda":
            raise RuntimeError("ConvGRU: inputs must live on the GPU; the HIP path has no CPU fallback")
        needs_grad = torch.is_grad_enabled() and (
            any(t.requires_grad for t in (h, cz, cr, cq, *x_list)) or any(p.requires_grad for p in self.parameters()))
        if needs_grad:
            return self._forward_autograd(h, cz, cr, cq, *x_list)
        c, ct = self.hidden_dim, self.hidden_dim + self.input_dim
        if h.shape[1] != c or sum(x.shape[1] for x in x_list) != self.input_dim:
            raise RuntimeError("ConvGRU: channel counts do not match the constructor's hidden_dim / input_dim")
        with torch.cuda.device(h.device), torch.autocast("cuda", enabled=False):
            hr = _rows(h)
            b, hh, ww, _ = hr.shape
            hx = hr.new_empty(b, hh, ww, ct)
            hx[..., :c] = hr
            at = c
            for x in x_list:
                hx[..., at:at + x.shape[1]] = x.permute(0, 2, 3, 1)
                at += x.shape[1]
            czr = torch.cat([cz.permute(0, 2, 3, 1), cr.permute(0, 2, 3, 1)], -1).float().contiguous()
            bzr = torch.cat([self.convz.bias, self.convr.bias]).detach().float().contiguous()
            zr = conv3x3_bf16(hx, _pack((self.convz.weight, self.convr.weight), conv2d.ONE_BF16), ct, 2 * c, bzr, czr,
                              ACT_SIGMOID)
            hx[..., :c] = zr[..., c:] * hr
            out = conv3x3_bf16(hx, _pack((self.convq.weight,), conv2d.ONE_BF16), ct, c,
                               self.convq.bias.detach().float().contiguous(), _rows(cq), ACT_GRU, gate_z=zr, gate_h=hr)
        return out.permute(0, 3, 1, 2)

    def _forward_autograd(self, h, cz, cr, cq, *x_list):
        with torch.autocast("cuda", enabled=False):
            # (the fused node's convolutions need hidden % 32 == 0 and (hidden + input) % 32 == 0: the reference's 128 + 256;
            #  every input part a multiple of 4 channels for the float4 kernels -- RAFT's 36 correlation + 220 context do)
            if self.train_arithmetic in ("bf16", "f16x1") and h.shape[1] % 32 == 0 and (h.shape[1] + self.input_dim) % 32 == 0:
                with torch.cuda.device(h.device):
                    czr, cqr = _context_rows(cz, cr, cq)  # looked up on the caller's tensors, BEFORE any cast
                return _GRUStepBf16.apply(self.train_arithmetic == "f16x1", h.float(), cz, cr, cq, czr, cqr, self.convz.weight, self.convr.weight,
                                          self.convq.weight, self.convz.bias, self.convr.bias, self.convq.bias,
                                          *[t.float() for t in x_list])
            h, cz, cr, cq = h.float(), cz.float(), cr.float(), cq.float()
            x = torch.cat([t.float() for t in x_list], 1)
            hx = torch.cat([h, x], 1).contiguous(memory_format=torch.channels_last)

            if self.train_arithmetic in ("bf16", "bf16_ops", "f16x1"):
                def conv(m, t):
                    return _Conv3x3Bf16.apply(t, m.weight, m.bias)
            else:
                def conv(m, t):
                    return conv2d.conv_same(t, m.weight) + m.bias.view(1, -1, 1, 1)

            if self.train_arithmetic in ("bf16", "bf16_ops", "f16x1"):  # z and r read the same operand: one convolution with 2 x hidden outputs
                zr = _Conv3x3Bf16.apply(hx, torch.cat([self.convz.weight, self.convr.weight], 0),
                                        torch.cat([self.convz.bias, self.convr.bias], 0))
                z, r = torch.sigmoid(zr[:, :self.hidden_dim] + cz), torch.sigmoid(zr[:, self.hidden_dim:] + cr)
            else:
                z = torch.sigmoid(conv(self.convz, hx) + cz)
                r = torch.sigmoid(conv(self.convr, hx) + cr)
            rhx = torch.cat([r * h, x], 1).contiguous(memory_format=torch.channels_last)
            q = torch.tanh(conv(self.convq, rhx) + cq)
            return (1 - z) * h + z * q
