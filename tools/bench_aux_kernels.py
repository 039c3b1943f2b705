#!/usr/bin/env python3
"""Microbenchmarks of the bandwidth-class kernels at BASELINE.json's full size
(B=4, 544x960, D=192): time per launch (HIP events on the launch stream) against the
ALGORITHMIC bytes of SURVEY.md 8(d).  Prints a markdown table.

    python tools/bench_aux_kernels.py raft_head [out.json]
runs the RAFT-Stereo prediction head instead (K15 convex upsampling + K16 sequence loss, 22 iterations forward and
backward at mask [4,144,136,240]) beside the reference's arithmetic in PyTorch eager, and prints one JSON record.

    python tools/bench_aux_kernels.py temporal_ir [out.json]
runs the temporal IR pattern (K17) at B=8, T=7, 540x960, ks=11 for uint8 and float32 stacks and prints one JSON record.

    python tools/bench_aux_kernels.py gt_prep [out.json]
    python tools/bench_aux_kernels.py error_img [out.json]
time the step's ground-truth preparation (K18, B=4, 1080x1920 -> 540x960) against the operator chain of train.py:255-272, and
the error image (K19, 540x960) against the numpy restatement fed from device tensors; one JSON record each (with an output
path the record is merged into that file under its case name).  The chain of `gt_prep` runs through this library's own
apply_disparity_cu (the K1 scatter kernel): the reference's extension does not exist on this platform.  `error_img` takes its
numpy baseline and its input generator from the test infrastructure (tests/_gt_prep_ref.py, the restatement of
utils/util.py:185-244): a recorded measurement, not a product path.

    python tools/bench_aux_kernels.py augment [out.json]
times the loader's blur + colour jitter + normalisation (K20, both stages on, ks = 9) at B = 8, 540x960 and at the training
crop 256x512, for uint8 and float32 images: the kernel pair, the copy probe moving the same algorithmic bytes, and the plain
torch fp32 operator chain (reflect F.pad, F.conv2d with the 2-D kernel, the blends, the normalisation) on the same inputs.

    python tools/bench_aux_kernels.py resize [out.json]
times the real domain's resize (K21, Pillow's 8-bit BILINEAR, bit for bit) at B = 8, 720x1280 -> 540x960, whole and with the
256x512 crop (100, 200), for uint8 and float32 output: the kernel, the copy probe (az_hbm_copy_probe) moving the same
algorithmic bytes, and F.interpolate(mode="bilinear", antialias=True) on the float image (cropped afterwards) -- the nearest
stock operator, which is not bit-compatible; the record says how many levels differ.

    python tools/bench_aux_kernels.py result_images [out.json]
times the six result images of a test batch (K24) at B = 1 and 4, 540x960: the launch plus its one copy against the host chain
of test.py:235-272 up to the PNG encoder (four copies and matplotlib's to_rgba per image, two K19 images), and both kernels
against the copy probe; profiles/result_images.json.

    python tools/bench_aux_kernels.py test_inputs [out.json]
times a test item's labels (K25, B = 1 and 4, 1080x1920 uint16 maps) and network inputs (K26, N = 2 and 8, 720x1280 -> 540x960,
pad (4, 0), float and grey-level sources): each kernel against the copy probe moving the same bytes and against what it
replaces -- F.interpolate + F.pad per view on the device for K26, the loader's numpy lines plus the upload of the four float
maps for K25; profiles/test_inputs.json.  Recorded, not gated.

    python tools/bench_aux_kernels.py optim [out.json]
times the optimizer step on the full-size PSMNet parameter set (maxdisp 192) with synthetic gradients: torch.optim.Adam in
its default (foreach) and fused=True forms, activezero_amd.optim.FusedAdam (K28) without and with max_grad_norm=1.0 (K27), and
foreach Adam behind clip_grad_norm_, beside the copy probe moving the update's 28 B per parameter; back to back (the 80 MB of
p, g, m, v stay in the 256 MiB cache) and behind a 512 MiB fill (they arrive from HBM, as in a training step);
profiles/optim_step.json.  Recorded, not gated.

    python tools/bench_aux_kernels.py ms_loss [out.json]
times the multi-scale disparity loss (K29) forward + backward at B = 4, 256x512 and 544x960, as dispnet_disp (seven scales) and
as default_disp (one): the fused autograd node against the same formula written as the torch operator chain (F.interpolate,
casts, boolean indexing, smooth_l1_loss), with the device kernels and host syncs of one step of each, and the two kernels
alone against the copy probe moving the bytes they touch; profiles/ms_loss.json.  Recorded, not gated."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def raft_head(out_path=None):
    import json
    import statistics
    import bench as _bench
    from activezero_amd import ops
    dev = torch.device("cuda:0")
    B, h, w, f, iters, reps = 4, 136, 240, 4, 22, 20
    g = torch.Generator(device=dev).manual_seed(0)
    gt = 2.0 + 90.0 * torch.rand(B, 1, f * h, f * w, device=dev, generator=g)
    valid = (torch.rand(B, 1, f * h, f * w, device=dev, generator=g) > 0.1).float()
    flows = [torch.cat([-gt[:, :, ::f, ::f] / f + torch.randn(B, 1, h, w, device=dev, generator=g),
                        torch.zeros(B, 1, h, w, device=dev)], 1).contiguous().requires_grad_() for _ in range(iters)]
    masks = [(2.0 * torch.randn(B, 9 * f * f, h, w, device=dev, generator=g)).requires_grad_() for _ in range(iters)]

    # the reference's arithmetic, restated: softmax over the 9 taps of the [N,1,9,f,f,h,w] view, 3x3 unfold of f * flow,
    # materialised product, sum, permute; then the masked L1 means with their finiteness assertions
    def eager_up(flow, mask):
        n, d = flow.shape[:2]
        p = torch.softmax(mask.view(n, 1, 9, f, f, h, w), dim=2)
        u = torch.nn.functional.unfold(f * flow, [3, 3], padding=1).view(n, d, 9, 1, 1, h, w)
        return torch.sum(p * u, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, d, f * h, f * w)[:, :1]

    def eager_loss(preds, gt, valid, gamma=0.9, max_flow=700):
        t = -gt
        ok = (valid >= 0.5) & (t.abs() < max_flow)
        assert not torch.isinf(t[ok]).any()
        n, loss = len(preds), 0.0
        for i, p in enumerate(preds):
            assert not torch.isnan(p).any() and not torch.isinf(p).any()
            loss = loss + (gamma ** (15 / (n - 1))) ** (n - i - 1) * (p - t).abs()[ok].mean()
        return loss

    def ours():
        loss = ops.sequence_loss([ops.convex_upsample(a, b, f, channels=1) for a, b in zip(flows, masks)], gt, valid)
        loss.backward()

    def eager():
        eager_loss([eager_up(a, b) for a, b in zip(flows, masks)], gt, valid).backward()

    def leg(fn):
        for t in flows + masks:
            t.grad = None
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return {"ms_per_22_iterations": statistics.median(ms), "min_ms": min(ms), "repeats": reps,
                "peak_MB_above_resident": (torch.cuda.max_memory_allocated() - base) / 1e6}

    def kernel(fn, nbytes):
        """fn(i) launches on the i-th of the 22 buffer sets (1.65 GB of fp32 masks: no launch finds its mask in the 256 MiB
        cache, as in the training step); one event pair around the 22 launches"""
        for _ in range(2):
            for i in range(iters):
                fn(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                fn(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / iters)
        m = statistics.median(ms)
        return {"ms": m, "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6, "launches_per_timing": iters,
                "buffers": "rotated over %d sets" % iters}

    rec = {"case": "raft_head", "mask": [B, 9 * f * f, h, w], "iterations": iters, "ours": leg(ours), "eager": leg(eager)}
    for t in flows + masks:
        t.grad = None
    with torch.no_grad():
        fls, mks = [t.detach() for t in flows], [t.detach() for t in masks]
        mbytes, ubytes, fbytes = 4.0 * mks[0].numel(), 4.0 * B * f * h * f * w, 4.0 * fls[0].numel()
        ups = [torch.randn(B, 1, f * h, f * w, device=dev) for _ in range(iters)]
        gms = [torch.empty_like(m) for m in mks]
        gf = torch.empty_like(fls[0])
        ws = torch.empty(B * 9 * h * w, device=dev)
        wbytes = 4.0 * ws.numel()
        args = (0, B, 2, 1, h, w, f, 9 * f * f, 1)
        rec["K15_fwd"] = kernel(lambda i: ops._call("az_convex_up_fwd", ups[i].data_ptr(), fls[i].data_ptr(),
                                                    mks[i].data_ptr(), *args, ops._stream()), mbytes + fbytes + ubytes)
        rec["K15_bwd"] = kernel(lambda i: ops._call("az_convex_up_bwd", gms[i].data_ptr(), gf.data_ptr(), ws.data_ptr(),
                                                    4 * ws.numel(), ups[i].data_ptr(), fls[i].data_ptr(),
                                                    mks[i].data_ptr(), *args, ops._stream()),
                                2 * mbytes + ubytes + 2 * fbytes + 2 * wbytes)
        mhs = [m.half() for m in mks]
        del gms
        gmhs = [torch.empty_like(m) for m in mhs]
        args16 = (1,) + args[1:]
        rec["K15_fwd_fp16_mask"] = kernel(lambda i: ops._call("az_convex_up_fwd", ups[i].data_ptr(), fls[i].data_ptr(),
                                                              mhs[i].data_ptr(), *args16, ops._stream()),
                                          mbytes / 2 + fbytes + ubytes)
        rec["K15_bwd_fp16_mask"] = kernel(lambda i: ops._call("az_convex_up_bwd", gmhs[i].data_ptr(), gf.data_ptr(),
                                                              ws.data_ptr(), 4 * ws.numel(), ups[i].data_ptr(),
                                                              fls[i].data_ptr(), mhs[i].data_ptr(), *args16, ops._stream()),
                                          mbytes + ubytes + 2 * fbytes + 2 * wbytes)
    rec["copy_probe_GB/s"] = _bench.hbm_probe(dev)["GB/s"]
    rec["speedup_vs_eager"] = rec["eager"]["ms_per_22_iterations"] / rec["ours"]["ms_per_22_iterations"]
    rec["mask_sized_tensor_MB"] = 4.0 * B * 9 * f * f * h * w / 1e6
    line = json.dumps(rec)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


def temporal_ir(out_path=None):
    import json
    import statistics
    import bench as _bench
    from activezero_amd import _lib, ops
    dev = torch.device("cuda:0")
    B, T, H, W, ks, sets, reps = 8, 7, 540, 960, 11, 8, 20
    g = torch.Generator(device=dev).manual_seed(0)
    ws_bytes = _lib.lib().az_temporal_ir_workspace(B, T, H, W, ks)
    rec = {"case": "temporal_ir", "stack": [B, T, H, W], "ks": ks, "threshold": 0.005,
           "timing": "%d launches on %d rotated buffer sets (more than the 256 MiB cache) per event pair, median of %d"
                     % (sets, sets, reps)}
    for name, dtype, size in (("u8", torch.uint8, 1), ("f32", torch.float32, 4)):
        stacks = []
        for _ in range(sets):  # texture + k * dot gain + noise, as a loader renders it
            tex = 20 + 100 * torch.rand(B, 1, H, W, device=dev, generator=g)
            gain = (torch.rand(B, 1, H, W, device=dev, generator=g) < 0.06) * 15.0
            k = torch.arange(T, device=dev).view(1, T, 1, 1)
            stacks.append((tex + gain * k + 1.5 * torch.randn(B, T, H, W, device=dev, generator=g)).round().clamp(0, 255).to(dtype))
        wss = [torch.empty(ws_bytes // 4, device=dev) for _ in range(sets)]
        outs = [torch.empty(B, H, W, device=dev) for _ in range(sets)]

        def launch(i):
            ops._call("az_temporal_ir", outs[i].data_ptr(), wss[i].data_ptr(), ws_bytes, stacks[i].data_ptr(), int(size == 1),
                      B, T, H, W, ks, 0.005, ops._stream())

        for _ in range(2):
            for i in range(sets):
                launch(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                launch(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        m = statistics.median(ms)
        nbytes = float(B) * H * W * (T * size + 4 + 4 + 4)  # stack read, diff write, diff read, pattern write
        rec[name] = {"ms": m, "min_ms": min(ms), "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
                     "share_of_ones": float(outs[0].mean())}
        del stacks, wss, outs
    rec["copy_probe_GB/s"] = _bench.hbm_probe(dev)["GB/s"]
    for name in ("u8", "f32"):
        rec[name]["of_copy_probe"] = rec[name]["GB/s"] / rec["copy_probe_GB/s"]
    print(json.dumps(rec))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


def augment(out_path=None):
    import json
    import statistics
    import torch.nn.functional as F
    import bench as _bench
    from activezero_amd import _lib, ops
    dev = torch.device("cuda:0")
    B, ks, reps = 8, 9, 20
    g = torch.Generator(device=dev).manual_seed(0)
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev).view(1, 3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev).view(1, 3, 1, 1)
    rec = {"case": "augment", "batch": B, "ks": ks, "flags": "blur + jitter, brightness first in every image",
           "timing": "one call per buffer set, the sets rotated (together more than the 256 MiB cache), per event pair; "
                     "median of %d after two warm-up rounds" % reps}

    def events(fn, sets):
        for _ in range(2):
            for i in range(sets):
                fn(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                fn(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        return statistics.median(ms), min(ms)

    probe = _bench.hbm_probe(dev)["GB/s"]
    rec["copy_probe_GB/s"] = probe
    for H, W in ((540, 960), (256, 512)):
        ws_bytes = _lib.lib().az_augment_workspace(B, H, W, ks)
        for name, dtype, size in (("u8", torch.uint8, 1), ("f32", torch.float32, 4)):
            per_set = B * H * W * (size + 12)
            sets = max(8, -(-300 * (1 << 20) // per_set))
            level = [(255 * torch.rand(B, H, W, device=dev, generator=g)).round() for _ in range(sets)]
            imgs = [(v.to(torch.uint8) if size == 1 else v / 255) for v in level]
            del level
            u = torch.rand(B, 3, device=dev, generator=g)
            params = torch.stack([0.1 + 1.9 * u[:, 0], 0.4 + u[:, 1], 0.8 + 0.4 * u[:, 2], torch.zeros(B, device=dev)], 1).contiguous()
            wss = [torch.empty(ws_bytes // 4, device=dev) for _ in range(sets)]
            outs = [torch.empty(B, 3, H, W, device=dev) for _ in range(sets)]

            def launch(i):
                ops._call("az_augment", outs[i].data_ptr(), wss[i].data_ptr(), ws_bytes, imgs[i].data_ptr(), int(size == 1),
                          params.data_ptr(), B, H, W, ks, 3, ops._stream())

            t = torch.arange(ks, device=dev) - ks // 2
            k1 = torch.exp(-0.5 * (t[None] / params[:, :1]) ** 2)
            k1 = k1 / k1.sum(1, keepdim=True)
            k2 = (k1[:, :, None] * k1[:, None, :])[:, None]  # [B,1,ks,ks]: one 2-D kernel per image, a grouped convolution
            bright, contrast = params[:, 1].view(B, 1, 1), params[:, 2].view(B, 1, 1)

            def chain(i):
                x = imgs[i].float() / 255 if size == 1 else imgs[i]
                x = F.conv2d(F.pad(x[None], (ks // 2,) * 4, mode="reflect"), k2, groups=B)[0]
                x = (bright * x).clamp(0, 1)
                m = (0.2989 * x + 0.587 * x + 0.114 * x).mean((1, 2), keepdim=True)
                x = (contrast * x + (1 - contrast) * m).clamp(0, 1)
                return (x[:, None] - mean) / std

            launch(0)
            worst = float((outs[0] - chain(0)).abs().max())
            assert worst < 1e-4, worst  # the two compute the same thing (fp32 both; the tests hold the kernel to fp64)
            m, lo = events(launch, sets)
            cm, clo = events(chain, sets)
            nbytes = float(B) * H * W * (2 * size + 12)  # the image read by both passes, three planes written
            rec["%dx%d_%s" % (H, W, name)] = {
                "ms": m, "min_ms": lo, "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
                "copy_probe_ms_same_bytes": nbytes / probe / 1e6, "of_copy_probe": nbytes / m / 1e6 / probe,
                "torch_chain_ms": cm, "torch_chain_min_ms": clo, "speedup_vs_torch_chain": cm / m,
                "buffer_sets": sets, "max_abs_diff_vs_chain": worst}
            del imgs, wss, outs
    print(json.dumps(rec))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


def resize(out_path=None):
    import json
    import statistics
    import torch.nn.functional as F
    from activezero_amd import ops
    from activezero_amd.datasets import dataset_utils_gpu as du
    dev = torch.device("cuda:0")
    B, Hin, Win, Hout, Wout, reps = 8, 720, 1280, 540, 960, 20
    g = torch.Generator(device=dev).manual_seed(0)
    rec = {"case": "resize", "batch": B, "in": [Hin, Win], "out": [Hout, Wout],
           "timing": "one call per buffer set, the sets rotated (together more than the 256 MiB cache), per event pair; "
                     "median of %d after two warm-up rounds; the copy probe moves the same number of bytes (half in, half "
                     "out) through the same rotation" % reps}

    def events(fn, sets):
        for _ in range(2):
            for i in range(sets):
                fn(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                fn(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        return statistics.median(ms), min(ms)

    ty, tx = du._resample_table(Hin, Hout, dev), du._resample_table(Win, Wout, dev)
    for window in ((0, 0, Hout, Wout), (100, 200, 256, 512)):
        y0, x0, h, w = window
        # source rows / columns the window's taps span: what a cropped call has to read
        ylo, yhi = int(ty[y0, 0]), int(ty[y0 + h - 1, 0] + ty[y0 + h - 1, 1])
        xlo, xhi = int(tx[x0, 0]), int(tx[x0 + w - 1, 0] + tx[x0 + w - 1, 1])
        for name, dtype, size in (("u8", torch.uint8, 1), ("f32", torch.float32, 4)):
            nbytes = float(B) * ((yhi - ylo) * (xhi - xlo) + h * w * size)
            per_set = B * (Hin * Win + h * w * size)
            sets = max(8, -(-300 * (1 << 20) // per_set))
            imgs = [torch.randint(0, 256, (B, Hin, Win), device=dev, generator=g, dtype=torch.uint8) for _ in range(sets)]
            outs = [torch.empty(B, h, w, dtype=dtype, device=dev) for _ in range(sets)]

            def launch(i):
                ops._call("az_resize_bilinear_u8", outs[i].data_ptr() if size == 1 else None,
                          outs[i].data_ptr() if size == 4 else None, imgs[i].data_ptr(), ty.data_ptr(), tx.data_ptr(), B, Hin,
                          Win, Hout, Wout, y0, x0, h, w, ops._stream())

            def stock(i):  # the nearest stock operator: not bit-compatible with Pillow's fixed-point passes
                x = F.interpolate((imgs[i].float() / 255)[:, None], size=(Hout, Wout), mode="bilinear", antialias=True,
                                  align_corners=False)[:, 0, y0:y0 + h, x0:x0 + w]
                return (255 * x).round().to(torch.uint8) if size == 1 else x.contiguous()

            launch(0)
            assert torch.equal(outs[0], du.resize_bilinear(imgs[0], (Hout, Wout), crop=window, dtype=dtype))
            diff = (outs[0].float() * (1 if size == 1 else 255) - stock(0).float() * (1 if size == 1 else 255)).abs()
            m, lo = events(launch, sets)
            sm, slo = events(stock, sets)
            nf = int(nbytes) // 8  # floats the probe copies: 4 bytes in + 4 bytes out each
            src = [torch.empty(nf, device=dev).normal_() for _ in range(sets)]
            dst = [torch.empty(nf, device=dev) for _ in range(sets)]
            pm, plo = events(lambda i: ops._call("az_hbm_copy_probe", dst[i].data_ptr(), src[i].data_ptr(), nf, ops._stream()),
                             sets)
            rec["%dx%d_%s" % (h, w, name)] = {
                "window": list(window), "ms": m, "min_ms": lo, "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
                "copy_probe_ms_same_bytes": pm, "copy_probe_min_ms": plo, "of_copy_probe": pm / m,
                "interpolate_antialias_ms": sm, "interpolate_antialias_min_ms": slo, "speedup_vs_interpolate": sm / m,
                "levels_differing_from_interpolate": float((diff >= 0.5).float().mean()),
                "max_level_diff_vs_interpolate": float(diff.max()), "buffer_sets": sets}
            del imgs, outs, src, dst
    print(json.dumps(rec))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


def _write_case(rec, out_path):
    """print the record; merge it into out_path under its case name"""
    import json
    print(json.dumps(rec))
    if out_path:
        doc = {}
        if os.path.exists(out_path):
            with open(out_path) as fh:
                doc = json.load(fh)
        doc[rec["case"]] = rec
        with open(out_path, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


def gt_prep(out_path=None):
    import statistics
    import time
    import torch.nn.functional as F
    import bench as _bench
    from activezero_amd import ops
    from activezero_amd.utils.warp_ops import apply_disparity_cu
    dev = torch.device("cuda:0")
    B, Hin, Win, H, W, sets, reps, MAX_DISP = 4, 1080, 1920, 540, 960, 8, 20, 192
    g = torch.Generator(device=dev).manual_seed(0)
    # smooth disparity of 8..120 pixels with fractional parts, depth from it: 8 sets of 66 MB, more than the 256 MiB cache
    disps, depths = [], []
    for _ in range(sets):
        coarse = 8 + 112 * torch.rand(B, 1, 9, 16, device=dev, generator=g)
        d = F.interpolate(coarse, (Hin, Win), mode="bilinear", align_corners=False).contiguous()
        disps.append(d)
        depths.append((446.31 * 0.055 / d).contiguous())
    half = lambda t: F.interpolate(t, scale_factor=0.5, mode="nearest", recompute_scale_factor=False)  # noqa: E731

    def chain(i, sign):
        depth_gt = half(depths[i])
        r = half(disps[i])
        disp_gt_l = apply_disparity_cu(r, r.type(torch.int), sign)
        return disp_gt_l, depth_gt, (disp_gt_l < MAX_DISP) * (disp_gt_l > 0)

    def fused(i):
        disp_gt_l, _, depth_gt, mask, _ = ops.gt_from_right(disps[i], keep=depths[i], lo=0.0, hi=float(MAX_DISP))
        return disp_gt_l, depth_gt, mask

    for a, b in zip(fused(0), chain(0, None)):
        assert torch.equal(a, b)

    def wall(fn):
        """host wall time per call: `sets` calls back to back on rotated inputs, device drained at either end"""
        for i in range(sets):
            fn(i)
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(sets):
                fn(i)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / sets * 1e6)
        return {"us_per_call": statistics.median(us), "min_us": min(us)}

    rec = {"case": "gt_prep", "input": [B, 1, Hin, Win], "output": [B, 1, H, W],
           "timing": "host wall time around %d calls on %d rotated input sets, device drained before and after, median of %d"
                     % (sets, sets, reps),
           "fused": dict(wall(fused), launches=2, host_syncs=0, launches_are="the memset of the two counters, the kernel"),
           "chain_with_sign_check": dict(wall(lambda i: chain(i, None)), launches=11, host_syncs=1, launches_are=(
               "3 nearest resizes, the int cast, disp >= 0, all(), its 1-byte copy to the host (the sync), the scatter kernel, "
               "2 compares, their product; counted from the code")),
           "chain_sign_given": dict(wall(lambda i: chain(i, 1)), launches=8, host_syncs=0)}
    # the kernel alone on preallocated outputs
    outs = [(torch.empty(B, 1, H, W, device=dev), torch.empty(B, 1, H, W, device=dev),
             torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)) for _ in range(sets)]
    stats = torch.zeros(2, dtype=torch.int32, device=dev)

    def launch(i):
        ops._call("az_gt_from_right", outs[i][0].data_ptr(), None, outs[i][1].data_ptr(), outs[i][2].data_ptr(), stats.data_ptr(),
                  disps[i].data_ptr(), None, depths[i].data_ptr(), B, 0, 1, Hin, Win, H, W, 2.0, 2.0, 0.0, float(MAX_DISP),
                  ops._stream())

    for _ in range(2):
        for i in range(sets):
            launch(i)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(sets):
            launch(i)
        b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / sets)
    m = statistics.median(ms)
    # touched: every 64-byte line of the 540 selected rows of both sources (stride-2 dwords), 4 + 4 + 1 bytes written per pixel
    nbytes = float(B) * H * (2 * Win * 4) + float(B) * H * W * 9
    probe = _bench.hbm_probe(dev)["GB/s"]
    rec["kernel"] = {"ms": m, "min_ms": min(ms), "touched_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6, "copy_probe_GB/s": probe,
                     "of_copy_probe": nbytes / m / 1e6 / probe,
                     "bytes_are": "whole lines of the selected source rows (half of each is used) + disp_l, depth, mask written"}
    rec["speedup_vs_chain_with_sign_check"] = rec["chain_with_sign_check"]["us_per_call"] / rec["fused"]["us_per_call"]
    rec["speedup_vs_chain_sign_given"] = rec["chain_sign_given"]["us_per_call"] / rec["fused"]["us_per_call"]
    _write_case(rec, out_path)


def error_img(out_path=None):
    import statistics
    import time
    import numpy as np
    from activezero_amd import ops
    from activezero_amd.utils.error_images import disp_error_img, disp_error_img_tensor
    from tests import _gt_prep_ref as ref
    dev = torch.device("cuda:0")
    H, W, reps = 540, 960, 20
    est, gt, mask = (torch.tensor(x, device=dev)[None] for x in ref.error_case(0, 1, H, W, "disp"))  # [1,1,H,W], as train.py:353

    def host():  # utils/util.py:214-244 as train.py:353 runs it: three device-to-host copies, the numpy passes
        e, g, m = (t.squeeze(0).detach().cpu().numpy() for t in (est, gt, mask))
        return ref.error_img(e, g, m, "disp")[0]

    def ours():
        return disp_error_img(est, gt, mask)

    assert np.array_equal(host(), ours())

    def wall(fn):
        for _ in range(3):
            fn()
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        return {"us_per_call": statistics.median(us), "min_us": min(us)}

    rec = {"case": "error_img", "image": [1, H, W], "timing": "host wall time per call, device drained before and after, median of %d" % reps,
           "drop_in_kernel_plus_one_copy": dict(wall(ours), host_syncs=1, bytes_to_host=12 * H * W),
           "numpy_restatement_from_device_tensors": dict(wall(host), host_syncs=3, bytes_to_host=9 * H * W),
           "tensor_variant_no_copy": dict(wall(lambda: disp_error_img_tensor(est, gt, mask)), host_syncs=0)}
    e3, g3, m3 = est[0], gt[0], mask[0].view(torch.uint8)
    out = torch.empty(1, 3, H, W, device=dev)
    ms = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(8):
            ops._call("az_error_img", out.data_ptr(), e3.data_ptr(), g3.data_ptr(), m3.data_ptr(), 0, 3.0, 0.05, 1, 1, H, W, ops._stream())
        b.record(); torch.cuda.synchronize()
        if k >= 2:
            ms.append(a.elapsed_time(b) / 8)
    rec["kernel"] = {"ms": statistics.median(ms), "algorithmic_MB": 21.0 * H * W / 1e6, "GB/s": 21.0 * H * W / statistics.median(ms) / 1e6,
                     "note": "8 launches on one 11 MB buffer set per event pair: cache-resident, launch-bound at this size"}
    rec["speedup_drop_in_vs_numpy"] = (rec["numpy_restatement_from_device_tensors"]["us_per_call"]
                                       / rec["drop_in_kernel_plus_one_copy"]["us_per_call"])
    _write_case(rec, out_path)


def eval_epilogue(out_path=None):
    """K22 against the per-object loop it replaces and K23 against its torch chain, at B = 1 and B = 4, 540x960, 17 objects
    laid out as blobs; equality first, then host wall time and kernel time; launches and syncs counted from the code"""
    import json
    import statistics
    import time
    import numpy as np
    import torch.nn.functional as F
    import bench as _bench
    from activezero_amd import ops
    from activezero_amd.utils import cascade_metrics as cm
    dev = torch.device("cuda:0")
    H, W, L, reps, MAX_DISP = 540, 960, 17, 20, 192
    probe = _bench.hbm_probe(dev)["GB/s"]
    doc = {"case": "eval_epilogue", "copy_probe_GB/s": probe,
           "timing": "host wall time per call on rotated input sets, device drained before and after, median of %d; kernel time "
                     "by events around one pass over the sets (together larger than the 256 MiB cache)" % reps}

    def wall(fn, sets):
        for i in range(min(sets, 4)):
            fn(i)
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(sets):
                fn(i)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / sets * 1e6)
        return {"us_per_call": statistics.median(us), "min_us": min(us)}

    def kernel_ms(launch, sets):
        for _ in range(2):
            for i in range(sets):
                launch(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                launch(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        return statistics.median(ms), min(ms)

    for B in (1, 4):
        sets = 32 if B == 1 else 8
        g = torch.Generator(device=dev).manual_seed(B)
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        data = []
        for s in range(sets):
            # 17 objects as blobs of 135 x 160 pixels, shifted per set and image
            label = torch.stack([(((yy + 7 * (s + b)) // 135) * 6 + (xx + 11 * b) // 160) % L for b in range(B)])[:, None].to(torch.int32)
            disp_gt = (8 + 112 * torch.rand(B, 1, H, W, device=dev, generator=g)).contiguous()
            disp_pred = disp_gt + 3 * torch.randn(B, 1, H, W, device=dev, generator=g)
            focal = torch.full((B, 1, 1, 1), 446.31, device=dev)
            base = torch.full((B, 1, 1, 1), 0.055, device=dev)
            depth_gt = (focal * base / disp_gt).contiguous()
            mask = torch.rand(B, 1, H, W, device=dev, generator=g) > 0.2
            data.append((disp_gt, depth_gt, disp_pred.clamp_min(0.5).contiguous(), focal, base, label.contiguous(), mask))

        def chain(i):
            """utils/cascade_metrics.py:65-126 as torch operators, one image or the batch as one set"""
            disp_gt, depth_gt, disp_pred, focal, base, label, mask = data[i]
            depth_pred = focal * base / disp_pred
            out = np.zeros((4, L))
            for obj in label.unique():
                k = int(obj.item())
                own = label == k
                out[0, k] += F.l1_loss(disp_gt[own * mask], disp_pred[own * mask], reduction="mean").item()
                mm = torch.clip(torch.abs(depth_gt[own * mask] * 1000 - depth_pred[own * mask] * 1000), min=0, max=100)
                out[1, k] += torch.mean(mm).item()
                dz = torch.abs(depth_gt[own * mask] - depth_pred[own * mask])
                out[2, k] += dz[dz > 4e-3].numel() / dz.numel()
                out[3, k] += 1
            return out

        def k12_loop(i):
            """compute_obj_err as it ran before K22: one az_disp_metrics launch per object, one copy"""
            disp_gt, depth_gt, disp_pred, focal, base, label, mask = data[i]
            depth_pred = (focal * base / disp_pred).contiguous()
            accs = [ops.disp_metrics(disp_gt, depth_gt, disp_pred, (label == obj) & mask, None, depth_pred)
                    for obj in label.unique().tolist()]
            return torch.stack(accs).tolist()

        def fused(i):
            return cm.compute_obj_err(*data[i])

        got, want = fused(0), chain(0)
        assert np.array_equal(got[3], want[3]), "object counts differ"
        for k in (0, 1):  # float32 means of the chain against fp64 sums
            np.testing.assert_allclose(got[k], want[k], rtol=2e-5)
        # a ratio of counts: equal when torch's float32 division rounds as the kernel's does (recorded), else a pixel or two apart
        np.testing.assert_allclose(got[2], want[2], atol=1e-4)
        per = cm.compute_obj_err_per_image(*data[0])
        single = [cm.compute_obj_err(*(t[b:b + 1] for t in data[0])) for b in range(B)]
        for k in range(4):
            np.testing.assert_allclose(per[k], sum(s[k] for s in single), rtol=1e-12)
        objs = int(want[3].sum())
        rec = {"maps": [B, 1, H, W], "objects_present": objs, "depth_err4_equal_to_the_chain": bool(np.array_equal(got[2], want[2])),
               "k22_compute_obj_err": dict(wall(fused, sets), library_launches=1, host_syncs=1, launches_are=(
                   "az_obj_metrics; beside it the focal * baseline product and the zero fill of the 4.4 KB output buffer, then the one copy")),
               "per_object_operator_chain": dict(wall(chain, sets), launches_at_least=4 + 33 * objs, host_syncs=1 + 10 * objs, launches_are=(
                   "unique (a sort, a sync) and the depth division, then per object: item, the compare, 6 products, 6 boolean-index "
                   "compactions (nonzero with a sync, gather), 14 element-wise and reduction operators, 3 item(); counted from the code")),
               "per_object_k12_loop": dict(wall(k12_loop, sets), launches=3 + 4 * objs, host_syncs=2, launches_are=(
                   "unique + tolist (a sync), the depth division, per object a compare, an and, a zero fill and az_disp_metrics, "
                   "then stack and one copy"))}
        rec["speedup_vs_operator_chain"] = rec["per_object_operator_chain"]["us_per_call"] / rec["k22_compute_obj_err"]["us_per_call"]
        rec["speedup_vs_k12_loop"] = rec["per_object_k12_loop"]["us_per_call"] / rec["k22_compute_obj_err"]["us_per_call"]

        # the kernels alone on preallocated outputs
        fb = [(d[3] * d[4]).reshape(-1).contiguous() for d in data]
        m8 = [d[6].view(torch.uint8) for d in data]
        buf = torch.zeros(ops._obj_words(B, L), dtype=torch.float64, device=dev)
        acc, present, stats = ops._obj_views(buf, B, L)
        acc8 = torch.zeros(8, dtype=torch.float64, device=dev)
        P = H * W

        def k22(i, lab=True, nl=L):
            d = data[i]
            ops._call("az_obj_metrics", acc.data_ptr(), present.data_ptr(), stats.data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                      d[2].data_ptr(), None, fb[i].data_ptr(), m8[i].data_ptr(), d[5].data_ptr() if lab else None, B, nl, P, ops._stream())

        def k12(i):
            d = data[i]
            ops._call("az_disp_metrics", acc8.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, fb[i].data_ptr(),
                      m8[i].data_ptr(), B, P, ops._stream())

        for name, launch, per_px in (("k22_17_labels", k22, 17 + 4), ("k22_no_label", lambda i: k22(i, False, 1), 17), ("k12_whole_batch", k12, 17)):
            m, lo = kernel_ms(launch, sets)
            nbytes = float(per_px) * B * P
            rec[name] = {"ms": m, "min_ms": lo, "MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6, "of_copy_probe": nbytes / m / 1e6 / probe,
                         "copy_probe_ms_for_these_bytes": nbytes / probe / 1e6}

        # K23: the loader's robot mask and RealSense depth at 1080 x 1920, float64
        aux = [((torch.rand(B, 1080, 1920, device=dev, generator=g, dtype=torch.float64) > 0.8).double(),
                torch.rand(B, 1080, 1920, device=dev, generator=g, dtype=torch.float64).clamp_min(0.25) - 0.25) for _ in range(sets)]

        def mask_chain(i):
            """test.py:112-117, 162-193"""
            disp, depth = data[i][0], data[i][1]
            robot = F.interpolate(aux[i][0].unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False).type(torch.int) == 0
            ground = (depth > 0) & (depth < 1.25)
            m = (disp < MAX_DISP) * (disp > 0) * ground * robot
            rs = F.interpolate(aux[i][1].unsqueeze(1), (H, W), mode="nearest", recompute_scale_factor=False)
            return (m * (rs > 0)).type(torch.bool)

        def mask_fused(i):
            return ops.eval_mask(data[i][0], data[i][1], MAX_DISP, True, aux[i][0], aux[i][1])[0]

        assert torch.equal(mask_fused(0), mask_chain(0))
        rec["k23_eval_mask"] = dict(wall(mask_fused, sets), launches=2, host_syncs=0, launches_are="the memset of the counter, the kernel")
        rec["mask_operator_chain"] = dict(wall(mask_chain, sets), launches=14, host_syncs=0, launches_are=(
            "2 nearest resizes, the int cast, 6 compares, the and, 4 products; counted from the code"))
        rec["k23_speedup"] = rec["mask_operator_chain"]["us_per_call"] / rec["k23_eval_mask"]["us_per_call"]
        out_m = torch.empty(B, 1, H, W, dtype=torch.uint8, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)

        def k23(i):
            ops._call("az_eval_mask", out_m.data_ptr(), cnt.data_ptr(), data[i][0].data_ptr(), data[i][1].data_ptr(), aux[i][0].data_ptr(),
                      1, 1080, 1920, aux[i][1].data_ptr(), 1, 1080, 1920, B, H, W, float(MAX_DISP), 1, 1.25, ops._stream())

        m, lo = kernel_ms(k23, sets)
        # 4 + 4 read and 1 written per pixel, and of each float64 map every second element of every second row: whole 64-byte
        # lines of the 540 selected rows
        nbytes = float(B) * P * 9 + 2 * float(B) * H * 1920 * 8
        rec["k23_kernel"] = {"ms": m, "min_ms": lo, "touched_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6, "of_copy_probe": nbytes / m / 1e6 / probe,
                             "copy_probe_ms_for_these_bytes": nbytes / probe / 1e6, "includes": "the 4-byte memset of the counter"}
        doc["B%d" % B] = rec
        del data, aux
    print(json.dumps(doc))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


def result_images(out_path=None):
    """K24 against the host chain it replaces (test.py:235-272 up to the PNG encoder, per image: four device-to-host copies,
    [ground_mask] = -1, masked_where and matplotlib's to_rgba(bytes=True), and the two K19 error images copied to the host and
    scaled to bytes), at B = 1 and B = 4, 540x960; equality first, then host wall time and kernel time.  Without matplotlib the
    host chain is left out and the record says so."""
    import importlib.util
    import json
    import statistics
    import time
    import numpy as np
    import bench as _bench
    from activezero_amd import ops
    from activezero_amd.utils import error_images as ei
    dev = torch.device("cuda:0")
    H, W, reps, MAX_DISP = 540, 960, 20, 192
    have_mpl = importlib.util.find_spec("matplotlib") is not None
    probe = _bench.hbm_probe(dev)["GB/s"]
    doc = {"case": "result_images", "copy_probe_GB/s": probe, "matplotlib": have_mpl,
           "timing": "host wall time per call on rotated input sets, device drained before and after, median of %d; kernel time "
                     "by events around one pass over the sets (together larger than the 256 MiB cache)" % reps}
    if have_mpl:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.cm as mcm
        import matplotlib.pyplot as plt
        cmap = plt.get_cmap("viridis").copy()
        cmap.set_bad(color="red")

    def host_chain(d):
        pred, gt_disp, gt_depth, mask, fb = d
        pred_depth = fb.view(-1, 1, 1, 1) / pred
        out = np.empty((pred.shape[0], 6, H, W, 4), np.uint8)
        for b in range(pred.shape[0]):  # the reference has no batch
            ground = torch.logical_not(mask[b, 0]).cpu().numpy()
            for m, (x, vmax) in {0: (pred, MAX_DISP), 1: (gt_disp, MAX_DISP), 3: (pred_depth, 1.25), 4: (gt_depth, 1.25)}.items():
                a = x[b, 0].detach().cpu().numpy()
                a[ground] = -1
                sm = mcm.ScalarMappable(cmap=cmap)
                sm.set_clim(0, vmax)
                out[b, m] = sm.to_rgba(np.ma.masked_where(a == -1, a), bytes=True)  # what plt.imsave hands to the encoder
            s = slice(b, b + 1)
            out[b, 2, :, :, :3] = (ei.disp_error_img(pred[s], gt_disp[s], mask[s]) * 255).astype(np.uint8)
            out[b, 5, :, :, :3] = (ei.depth_error_img(pred_depth[s] * 1000, gt_depth[s] * 1000, mask[s]) * 255).astype(np.uint8)
            out[b, 2, :, :, 3] = out[b, 5, :, :, 3] = 255
        return out

    def wall(fn, sets):
        for i in range(min(sets, 2)):
            fn(i)
        us = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(sets):
                fn(i)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / sets * 1e6)
        return {"us_per_call": statistics.median(us), "min_us": min(us)}

    for B in (1, 4):
        sets = 16 if B == 1 else 4  # 37 bytes per pixel and set: 307 MB in all
        g = torch.Generator(device=dev).manual_seed(B)
        data = []
        for _ in range(sets):
            gt_disp = (8 + 112 * torch.rand(B, 1, H, W, device=dev, generator=g)).contiguous()
            pred = (gt_disp + 3 * torch.randn(B, 1, H, W, device=dev, generator=g)).contiguous()
            fb = torch.full((B,), 446.31, device=dev) * torch.full((B,), 0.055, device=dev)
            gt_depth = (fb.view(B, 1, 1, 1) / gt_disp).contiguous()
            mask = torch.rand(B, 1, H, W, device=dev, generator=g) > 0.3
            data.append((pred, gt_disp, gt_depth, mask, fb))

        def fused(i):
            return ops.result_images(*data[i][:4], data[i][4], MAX_DISP).cpu()  # the launch and ONE copy of finished bytes

        rec = {"shape": [B, 6, H, W, 4]}
        rec["k24_plus_one_copy"] = dict(wall(fused, sets), launches=3, host_syncs=1, bytes_to_host=24 * B * H * W,
                                        launches_are="the memset of the flags, the flags kernel, the render kernel")
        if have_mpl:
            differ = int((fused(0).numpy() != host_chain(data[0])).any(-1).sum())
            rec["pixels_that_differ_from_host_chain"] = differ  # (its depth is torch's own fb / pred on the device)
            rec["host_chain"] = dict(wall(lambda i: host_chain(data[i]), sets), host_syncs=7 * B, bytes_to_host=(17 + 24) * B * H * W,
                                     chain_is="per image: mask and four float maps copied, to_rgba(bytes=True) four times, two K19 images copied")
            rec["speedup"] = rec["host_chain"]["us_per_call"] / rec["k24_plus_one_copy"]["us_per_call"]
        outs = [torch.empty(B, 6, H, W, 4, dtype=torch.uint8, device=dev) for _ in range(sets)]
        flags = torch.empty(B, dtype=torch.int32, device=dev)

        def k24(i):
            pred, gt_disp, gt_depth, mask, fb = data[i]
            ops._call("az_result_images", outs[i].data_ptr(), flags.data_ptr(), pred.data_ptr(), W, H * W, gt_disp.data_ptr(),
                      gt_depth.data_ptr(), mask.view(torch.uint8).data_ptr(), fb.data_ptr(), float(MAX_DISP), 1.25, 3.0, 0.05, 1000.0,
                      1.0, B, H, W, ops._stream())

        for _ in range(2):
            for i in range(sets):
                k24(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                k24(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        m = statistics.median(ms)
        nbytes = 37.0 * B * H * W  # 13 read + 24 written per pixel; the flags kernel reads the 13 a first time
        rec["k24_kernels"] = {"ms": m, "min_ms": min(ms), "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
                              "of_copy_probe": nbytes / m / 1e6 / probe, "copy_probe_ms_for_these_bytes": nbytes / probe / 1e6,
                              "includes": "the memset of the flags and both kernels; the flags kernel's 13 B/pixel are not counted"}
        doc["B%d" % B] = rec
        del data, outs
    print(json.dumps(doc))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


def test_inputs(out_path=None):
    """K25 (B = 1 and 4, 1080x1920 uint16 maps) and K26 (N = 2 and 8, 720x1280 -> 540x960, pad (4, 0), both source forms):
    each kernel by events on rotated buffer sets against the copy probe moving the same algorithmic bytes, and against what it
    replaces -- for K26 the device chain of test.py:118-146 (F.interpolate and F.pad per view) by events, for K25 the loader's
    numpy lines plus the upload of their four float maps, by host wall time against the upload of the raw maps plus the
    launch.  Equality with the replaced chain is checked first."""
    import json
    import statistics
    import time
    import numpy as np
    import torch.nn.functional as F
    from activezero_amd import ops
    from activezero_amd.datasets import dataset_utils_gpu as du
    dev = torch.device("cuda:0")
    reps = 20
    doc = {"case": "test_inputs",
           "timing": "kernels: one call per buffer set, the sets rotated (together more than the 256 MiB cache), per event pair, "
                     "median of %d after two warm-up rounds; the copy probe moves the same number of bytes (half in, half out) "
                     "through the same rotation; host chains: wall time per call, device drained before and after, median of 5" % reps}

    def events(fn, sets):
        for _ in range(2):
            for i in range(sets):
                fn(i)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(sets):
                fn(i)
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / sets)
        return statistics.median(ms), min(ms)

    def wall(fn):
        fn()
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def probe(nbytes, sets):
        nf = int(nbytes) // 8  # floats the probe copies: 4 bytes in + 4 bytes out each
        src = [torch.empty(nf, device=dev).normal_() for _ in range(sets)]
        dst = [torch.empty(nf, device=dev) for _ in range(sets)]
        return events(lambda i: ops._call("az_hbm_copy_probe", dst[i].data_ptr(), src[i].data_ptr(), nf, ops._stream()), sets)

    def sets_for(per_set):
        return max(2, -(-300 * (1 << 20) // per_set))

    # ---- K25
    H2, W2, FOCAL, BASE = 1080, 1920, 446.31, 0.055
    rng = np.random.default_rng(0)
    for B in (1, 4):
        nbytes = float(B) * H2 * W2 * (2 * 2 + 4 * 4)
        sets = sets_for(int(nbytes))
        host = [rng.integers(0, 2000, (2, B, H2, W2)).astype(np.uint16) for _ in range(2)]
        mm = [torch.from_numpy(host[i % 2]).to(dev) for i in range(sets)]
        fl = torch.full((B,), FOCAL, dtype=torch.float64, device=dev)
        bl = torch.full((B,), BASE, dtype=torch.float64, device=dev)
        outs = [[torch.empty(B, 1, H2, W2, device=dev) for _ in range(4)] for _ in range(sets)]

        def k25(i):
            ops._call("az_depth_labels", *(o.data_ptr() for o in outs[i]), mm[i][0].data_ptr(), mm[i][1].data_ptr(), 0,
                      fl.data_ptr(), bl.data_ptr(), None, B, H2, W2, H2, W2, ops._stream())

        def numpy_chain(maps=host[0]):  # messytable.py:197-213, 281-284 per item, then the four uploads
            items = []
            for b in range(B):
                item = []
                for side in (0, 1):
                    depth = np.array(maps[side, b]) / 1000
                    mask = depth > 0
                    disp = np.zeros_like(depth)
                    disp[mask] = FOCAL * BASE / depth[mask]
                    item += [torch.tensor(disp, dtype=torch.float32).unsqueeze(0), torch.tensor(depth, dtype=torch.float32).unsqueeze(0)]
                items.append(item)
            return [torch.stack([it[k] for it in items]).to(dev) for k in range(4)]

        def raw_upload(maps=host[0]):
            return du.depth_to_labels(torch.from_numpy(maps[0]).to(dev), torch.from_numpy(maps[1]).to(dev), FOCAL, BASE)

        k25(0)
        assert all(torch.equal(a, b) for a, b in zip(outs[0], numpy_chain()))
        m, lo = events(k25, sets)
        pm, plo = probe(nbytes, sets)
        doc["k25_B%d" % B] = {
            "maps": [B, H2, W2], "ms": m, "min_ms": lo, "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
            "copy_probe_ms_same_bytes": pm, "copy_probe_min_ms": plo, "of_copy_probe": pm / m, "buffer_sets": sets,
            "numpy_lines_plus_upload_ms": wall(numpy_chain), "raw_upload_plus_k25_ms": wall(raw_upload),
            "upload_MB": {"float_labels": 16.0 * B * H2 * W2 / 1e6, "raw_uint16": 4.0 * B * H2 * W2 / 1e6}}
        del mm, outs

    # ---- K26
    Hin, Win, H, W, top, right = 720, 1280, 540, 960, 4, 0
    g = torch.Generator(device=dev).manual_seed(0)
    for N in (2, 8):
        for name, u8 in (("float", 0), ("levels", 1)):
            in_bytes = N * Hin * Win * (1 if u8 else 12)
            nbytes = float(in_bytes + N * 3 * (H + top) * (W + right) * 4)
            sets = sets_for(int(nbytes))
            levels = [torch.randint(0, 256, (N, Hin, Win), device=dev, generator=g, dtype=torch.uint8) for _ in range(sets)]
            srcs = levels if u8 else [du.augment_images(l) for l in levels]
            outs = [torch.empty(N, 3, H + top, W + right, device=dev) for _ in range(sets)]

            def k26(i):
                ops._call("az_test_images", outs[i].data_ptr(), srcs[i].data_ptr(), None, u8, N, 0, Hin, Win, H, W, top, right,
                          ops._stream())

            rec = {"images": N, "in": [Hin, Win], "out": [H + top, W + right], "buffer_sets": sets}
            k26(0)
            if not u8:
                floats = srcs

                def chain(i):  # test.py:118-146: the two views on their own
                    res = []
                    for view in (floats[i][:N // 2], floats[i][N // 2:]):
                        x = F.interpolate(view, (H, W), mode="bilinear", recompute_scale_factor=False, align_corners=False)
                        res.append(F.pad(x, (0, right, top, 0, 0, 0, 0, 0), mode="constant", value=0))
                    return res

                rec["max_abs_diff_vs_chain"] = float((outs[0] - torch.cat(chain(0))).abs().max())
                rec["largest_tap"] = float(floats[0].abs().max())
                assert rec["max_abs_diff_vs_chain"] <= 12 * rec["largest_tap"] * 2.0 ** -24  # two float32 blends, 6 M 2^-24 each
                cm, clo = events(chain, sets)
                rec.update({"chain_ms": cm, "chain_min_ms": clo, "chain_launches": 4})
            else:
                assert torch.equal(outs[0], ops.test_images(du.augment_images(levels[0]), size=(H, W), pad=(top, right)))
            m, lo = events(k26, sets)
            pm, plo = probe(nbytes, sets)
            rec.update({"ms": m, "min_ms": lo, "algorithmic_MB": nbytes / 1e6, "GB/s": nbytes / m / 1e6,
                        "copy_probe_ms_same_bytes": pm, "copy_probe_min_ms": plo, "of_copy_probe": pm / m})
            if "chain_ms" in rec:
                rec["speedup_vs_chain"] = rec["chain_ms"] / m
            doc["k26_N%d_%s" % (N, name)] = rec
            del levels, srcs, outs
    print(json.dumps(doc))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")



def optim_step(out_path=None):
    import statistics
    import time
    from activezero_amd import ops
    from activezero_amd.nets.psmnet.psmnet_3 import PSMNet
    from activezero_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in PSMNet(192).parameters()]
    n_param = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device=dev).manual_seed(1)

    def make(ctor, clip=False):
        ps = [torch.nn.Parameter(0.1 * torch.randn(s, device=dev, generator=g)) for s in shapes]
        for p in ps:
            p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=g)
        opt = ctor(ps)
        if clip:
            return lambda: (torch.nn.utils.clip_grad_norm_(ps, 1.0), opt.step()), opt
        return opt.step, opt

    variants = {
        "torch_adam_foreach": make(lambda ps: torch.optim.Adam(ps, lr=2e-4)),
        "torch_adam_fused": make(lambda ps: torch.optim.Adam(ps, lr=2e-4, fused=True)),
        "fused_adam": make(lambda ps: FusedAdam(ps, lr=2e-4)),
        "fused_adam_max_grad_norm": make(lambda ps: FusedAdam(ps, lr=2e-4, max_grad_norm=1.0)),
        "torch_adam_foreach_plus_clip_grad_norm": make(lambda ps: torch.optim.Adam(ps, lr=2e-4), clip=True),
    }
    n_copy = (int(3.5 * n_param) + 3) // 4 * 4  # a float copied is 8 bytes moved: 28 B per parameter
    src, dst = torch.randn(n_copy, device=dev, generator=g), torch.empty(n_copy, device=dev)
    variants["copy_probe_28B_per_param"] = (
        lambda: ops._call("az_hbm_copy_probe", dst.data_ptr(), src.data_ptr(), n_copy, ops._stream()), None)
    flush = torch.empty(1 << 27, device=dev)  # 512 MiB: twice the Infinity Cache
    inner, reps = 10, 15
    for fn, _ in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    warm = {k: [] for k in variants}
    cold_wall, cold_dev = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(reps):  # the variants alternate inside every repetition: drift hits all of them alike
        for k, (fn, _) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            warm[k].append((time.perf_counter() - t0) / inner * 1e3)
            flush.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            cold_wall[k].append((time.perf_counter() - t0) * 1e3)
            cold_dev[k].append(a.elapsed_time(b))
    med = statistics.median
    rec = {"case": "optim_step", "tensors": len(shapes), "parameters": n_param, "bytes_per_step_MB": 28.0 * n_param / 1e6,
           "timing": "ms per step.  back_to_back: host wall time around %d steps, device drained at either end, median of %d "
                     "(working set 16 B per parameter, cache-resident); cold: one step behind a 512 MiB fill, host wall time to "
                     "the drained device and the device events around it, median of %d; variants alternate inside every "
                     "repetition" % (inner, reps, reps),
           "variants": {k: {"back_to_back_ms": med(warm[k]), "back_to_back_min_ms": min(warm[k]), "cold_wall_ms": med(cold_wall[k]),
                            "cold_event_ms": med(cold_dev[k]), "cold_event_min_ms": min(cold_dev[k])} for k in variants}}
    for k in ("fused_adam", "fused_adam_max_grad_norm"):
        opt = variants[k][1]
        l0 = opt.launches
        opt.step()
        rec["variants"][k]["launches_per_step"] = opt.launches - l0
    v = rec["variants"]
    for k in ("fused_adam", "fused_adam_max_grad_norm"):
        v[k]["cold_GB/s"] = (28.0 + (4.0 if k.endswith("norm") else 0.0)) * n_param / v[k]["cold_event_ms"] / 1e6
    v["copy_probe_28B_per_param"]["cold_GB/s"] = 28.0 * n_param / v["copy_probe_28B_per_param"]["cold_event_ms"] / 1e6
    rec["back_to_back_speedup_vs_foreach"] = v["torch_adam_foreach"]["back_to_back_ms"] / v["fused_adam"]["back_to_back_ms"]
    rec["back_to_back_speedup_vs_torch_fused"] = v["torch_adam_fused"]["back_to_back_ms"] / v["fused_adam"]["back_to_back_ms"]
    rec["back_to_back_speedup_clipped_vs_foreach_plus_clip"] = (
        v["torch_adam_foreach_plus_clip_grad_norm"]["back_to_back_ms"] / v["fused_adam_max_grad_norm"]["back_to_back_ms"])
    _write_case(rec, out_path)


def ms_loss(out_path=None):
    import json
    import statistics
    import warnings
    import numpy as np
    import torch.nn.functional as F
    import bench as _bench
    from activezero_amd import ops
    from activezero_amd.utils import disp_losses
    dev = torch.device("cuda:0")
    reps = 30
    g = torch.Generator(device=dev).manual_seed(0)
    weights = disp_losses.DISPNET_WEIGHTS
    probe = _bench.hbm_probe(dev)["GB/s"]
    doc = {"case": "ms_loss", "copy_probe_GB/s": probe,
           "timing": "forward + backward of one loss per HIP event pair on the launch stream (host gaps and syncs of the "
                     "chain included: the stream idles while the host waits), median of %d after 3 warm-up steps; "
                     "kernels_only: az_ms_loss_fwd + az_ms_loss_bwd through the C ABI, 20 pairs per event pair; device "
                     "kernels counted by torch.profiler over one step, host syncs by set_sync_debug_mode('warn')" % reps}

    def chain_dispnet(ps, gt, mask):  # the formula of utils/losses.py:17-32 as the torch operator chain
        total = 0.0
        for s, (p, w) in enumerate(zip(ps, weights)):
            if s:
                dgt = F.interpolate(gt, scale_factor=1 / (2 ** s))
                m = F.interpolate(mask.float(), scale_factor=1 / (2 ** s)).bool()
            else:
                dgt, m = gt, mask
            total = total + w * F.smooth_l1_loss(p[m], dgt[m], reduction="mean")
        return total

    def chain_default(ps, gt, mask):  # utils/losses.py:71-72
        return F.smooth_l1_loss(ps[0][mask], gt[mask], reduction="mean")

    def step(fn, ps, gt, mask):
        for p in ps:
            p.grad = None
        fn(ps, gt, mask).backward()

    def events(fn, inner=1):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / inner)
        return statistics.median(ms), min(ms)

    def count(fn):
        """(device kernels of one step or None when the profiler is unavailable, launches per K29 kernel, host syncs)"""
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        syncs = sum("synchroniz" in str(c.message).lower() and "prototype" not in str(c.message).lower() for c in caught)
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                     and "memset" not in e.name.lower()]
            return len(names), {n.split("(")[0]: names.count(n) for n in sorted(set(names)) if "ms_loss" in n}, syncs
        except Exception as err:  # recorded, not hidden
            return None, {"profiler unavailable: %r" % (err,): 0}, syncs

    for H, W in ((256, 512), (544, 960)):
        B = 4
        gt = 2.0 + 90.0 * torch.rand(B, 1, H, W, device=dev, generator=g)
        gt[:, :, : H // 8] = 0.0
        mask = (gt > 0) & (gt < 64.0)
        for name, nd, fused, chain in (("dispnet_disp", 7, lambda ps, a, m: disp_losses.dispnet_disp(ps, a, m), chain_dispnet),
                                       ("default_disp", 1, lambda ps, a, m: disp_losses.default_disp(ps[0], a, m), chain_default)):
            ps = [(gt[:, :, ::1 << s, ::1 << s][:, :, :H >> s, :W >> s] + torch.randn(B, 1, H >> s, W >> s, device=dev, generator=g))
                  .contiguous().requires_grad_() for s in range(nd)]
            lf, lc = fused(ps, gt, mask), chain(ps, gt, mask)
            lf, lc = float(lf.detach()), float(lc.detach())
            assert abs(lf - lc) <= 1e-5 * abs(lc), (name, lf, lc)
            fm, flo = events(lambda: step(fused, ps, gt, mask))
            cm, clo = events(lambda: step(chain, ps, gt, mask))
            fk, fnames, fsync = count(lambda: step(fused, ps, gt, mask))
            ck, _, csync = count(lambda: step(chain, ps, gt, mask))
            # the two kernels alone, through the C ABI
            det = [p.detach() for p in ps]
            grads = [torch.empty_like(p) for p in det]
            acc = torch.zeros(nd, 2, dtype=torch.float64, device=dev)
            gloss = torch.ones(1, device=dev)
            m8 = mask.view(torch.uint8)
            d_f = ops._ms_descs(det, [None] * nd, range(nd))
            d_b = ops._ms_descs(det, grads, range(nd))
            wts = np.asarray(weights[:nd], dtype=np.float32)

            def pair():
                ops._call("az_ms_loss_fwd", acc.data_ptr(), d_f.ctypes.data, nd, gt.data_ptr(), m8.data_ptr(), 0.0, float("inf"),
                          B, H, W, ops._stream())
                ops._call("az_ms_loss_bwd", d_b.ctypes.data, wts.ctypes.data, nd, gt.data_ptr(), m8.data_ptr(), 0.0, float("inf"),
                          gloss.data_ptr(), acc.data_ptr(), B, H, W, ops._stream())

            km, klo = events(pair, inner=20)
            npix = sum(p.numel() for p in det)
            # per prediction pixel: forward 4 B read, backward 4 B read + 4 B written; gt (4 B) and mask (1 B) once per pass
            # at scale 0, by touched 64 B lines at the coarser scales (stride >= 16 floats: one line per pixel)
            gt_lines = sum(min(det[s].numel() * 64, gt.numel() * 4) if s else gt.numel() * 4 for s in range(nd))
            nbytes = 12.0 * npix + 2.0 * (gt_lines + gt.numel())
            nf = int(nbytes) // 8
            src, dst = torch.empty(nf, device=dev).normal_(), torch.empty(nf, device=dev)
            pm, plo = events(lambda: ops._call("az_hbm_copy_probe", dst.data_ptr(), src.data_ptr(), nf, ops._stream()), inner=20)
            doc["%s_%dx%d" % (name, H, W)] = {
                "batch": B, "predictions": nd, "prediction_pixels": npix,
                "fused_fwd_bwd_ms": fm, "fused_min_ms": flo, "chain_fwd_bwd_ms": cm, "chain_min_ms": clo, "speedup_vs_chain": cm / fm,
                "fused_device_kernels": fk, "fused_ms_loss_kernels": fnames, "fused_host_syncs": fsync,
                "chain_device_kernels": ck, "chain_host_syncs": csync,
                "kernels_only_fwd_plus_bwd_ms": km, "kernels_only_min_ms": klo, "touched_MB": nbytes / 1e6,
                "kernels_only_GB/s": nbytes / km / 1e6, "copy_probe_ms_same_bytes": pm, "copy_probe_min_ms": plo,
                "of_copy_probe": pm / km}
    print(json.dumps(doc))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


test_inputs.__test__ = False  # (a benchmark, not a test)
if len(sys.argv) > 1 and sys.argv[1] == "ms_loss":
    ms_loss(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "optim":
    optim_step(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "test_inputs":
    test_inputs(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "result_images":
    result_images(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "eval_epilogue":
    eval_epilogue(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] in ("gt_prep", "error_img"):
    {"gt_prep": gt_prep, "error_img": error_img}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "augment":
    augment(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "resize":
    resize(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "temporal_ir":
    temporal_ir(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "raft_head":
    raft_head(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

from activezero_amd import ops, conv3d
from activezero_amd.utils import reprojection as rp, warp_ops
from activezero_amd.nets.raft.corr import CorrBlock1D

dev = torch.device("cuda:0")
B, H, W, D = 4, 544, 960, 192
h, w, d, C = H // 4, W // 4, D // 4, 32


def timeit(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


rows = []
def row(name, ms, nbytes, note=""):
    rows.append(f"| {name} | {ms:.3f} | {nbytes / 1e6:.1f} | {nbytes / ms / 1e6:.0f} | {nbytes / ms / 1e6 / 8000 * 100:.0f} % | {note} |")

g = torch.Generator(device=dev).manual_seed(0)
# K1 scatter warp (C=1)
x = (40 * torch.rand(B, 1, H, W, device=dev, generator=g)).contiguous()
di = x.int()
row("K1 `az_warp_scatter` (C=1)", timeit(lambda: ops.warp_scatter(x, di, 1)), 4.0 * B * H * W * 3)
# K3 cost volume
fl, fr = torch.randn(B, C, h, w, device=dev), torch.randn(B, C, h, w, device=dev)
vol_bytes = 4.0 * B * (2 * C * h * w + 2 * C * d * h * w)
vol = ops.cost_volume(fl, fr, d)
row("K3 `az_cost_volume_fwd` (NCDHW)", timeit(lambda: ops.cost_volume(fl, fr, d)), vol_bytes)
gl, gr = torch.empty_like(fl), torch.empty_like(fr)
row("K3 `az_cost_volume_bwd` (NCDHW)", timeit(lambda: ops._call("az_cost_volume_bwd", gl.data_ptr(), gr.data_ptr(), vol.data_ptr(), B, C, d, h, w, ops._stream())), vol_bytes)
del vol
fln, frn = fl.permute(0, 2, 3, 1).contiguous(), fr.permute(0, 2, 3, 1).contiguous()
volc = ops.cost_volume_ndhwc(fln, frn, d)
row("K3 `az_cost_volume_fwd_ndhwc`", timeit(lambda: ops.cost_volume_ndhwc(fln, frn, d)), vol_bytes)
row("K3 `az_cost_volume_bwd_ndhwc`", timeit(lambda: ops._call("az_cost_volume_bwd_ndhwc", gl.data_ptr(), gr.data_ptr(), volc.data_ptr(), B, C, d, h, w, ops._stream())), vol_bytes)
del volc
# K6 soft-argmin
lg = (3 * torch.randn(B, 1, d, h, w, device=dev)).requires_grad_()
out = ops.softargmin(lg)
row("K6 `az_softargmin_fwd` (per head)", timeit(lambda: ops.softargmin(lg.detach())), 4.0 * B * (d * h * w + H * W), "VALU-issue bound: plane values in registers, one v_exp_f32 per disparity")
go = torch.randn_like(out)
glg = torch.empty_like(lg)
row("K6 `az_softargmin_bwd` (per head)", timeit(lambda: ops._call("az_softargmin_bwd", glg.data_ptr(), go.data_ptr(), lg.data_ptr(), None, None, B, d, h, w, ops._stream())), 4.0 * B * (2 * d * h * w + H * W), "recompute; per-wave private LDS gradient tiles, global float atomics")
# K7 gather warp
img = torch.randn(B, 1, H, W, device=dev)
dsp = (8 * torch.rand(B, 1, H, W, device=dev)).requires_grad_()
row("K7 `az_warp_gather_fwd` (C=1)", timeit(lambda: ops.warp_gather(img, dsp.detach())), 4.0 * B * H * W * 3)
# K8 patch reprojection ps=11
pl = (torch.rand(B, 1, H, W, device=dev) < 0.25).float()
pr = pl.roll(5, 3).contiguous()
mask = torch.rand(B, 1, H, W, device=dev) < 0.9
def k8f():
    return ops.patch_reprojection(pl, pr, dsp.detach(), mask, 11, want_vis=False)
row("K8 `az_patch_reproj_fwd` (ps=11)", timeit(k8f), 4.0 * B * H * W * 3.25, "band of rows at full width in LDS, four pixels per thread")
loss, _, _ = ops.patch_reprojection(pl, pr, dsp, mask, 11, want_vis=False)
def k8b():
    dsp.grad = None
    l, _, _ = ops.patch_reprojection(pl, pr, dsp, mask, 11, want_vis=False)
    l.backward()
tb = timeit(k8b)
row("K8 fwd+bwd (ps=11)", tb, 4.0 * B * H * W * (3.25 + 4.25))
row("K8 `az_patch_reproj_vis` (Fold image)", timeit(lambda: ops.patch_reprojection(pl, pr, dsp.detach(), mask, 11, want_vis=True)) - timeit(k8f), 4.0 * B * H * W * 3, "121 x 4 gathers per pixel; TensorBoard only")
# K9 LCN
im = torch.rand(B, 1, 540, 960, device=dev)
row("K9 `az_lcn` (k=11)", timeit(lambda: ops.local_contrast_norm(im, 11)), 4.0 * B * 540 * 960 * 3)
# BN passes on a V0 32-channel tensor
xv = torch.randn(B, d, h, w, C, device=dev)
yv = torch.empty_like(xv)
sc, sh = torch.ones(C, device=dev), torch.zeros(C, device=dev)
row("`az_bn3d_apply` (V0, 32 ch)", timeit(lambda: ops._call("az_bn3d_apply", yv.data_ptr(), xv.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, 1, xv.numel() // C, C, None, ops._stream())), 8.0 * xv.numel())
# BatchNorm backward of the same tensor (five tensor passes: 2 x (dy, raw) in, dx out) with max |dx| taken on the way
from activezero_amd import _lib  # noqa: E402
gy, raw = torch.randn_like(xv), torch.randn_like(xv)
nv = xv.numel() // C
mean, invstd, gamma = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.ones(C, device=dev)
dgm, dbt, coef, dxa = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(C, 3, device=dev), torch.zeros(1024, device=dev)
wsb = _lib.lib().az_bn3d_bwd_workspace(nv, C)
wsp = torch.empty(wsb // 4, device=dev)
row("`az_bn3d_bwd` (V0, 32 ch, ReLU mask recomputed, amax out)", timeit(lambda: ops._call(
    "az_bn3d_bwd", yv.data_ptr(), None, dgm.data_ptr(), dbt.data_ptr(), coef.data_ptr(), wsp.data_ptr(), wsb, gy.data_ptr(), None,
    raw.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, nv, C, dxa.data_ptr(), 0,
    ops._stream())), 20.0 * xv.numel(), "reduce + apply (partials merged in the apply prologue)")
row("`az_bn3d_bwd` (V0, 32 ch), dx written pre-split", timeit(lambda: ops._call(
    "az_bn3d_bwd", yv.data_ptr(), None, dgm.data_ptr(), dbt.data_ptr(), coef.data_ptr(), wsp.data_ptr(), wsb, gy.data_ptr(), None,
    raw.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, nv, C, dxa.data_ptr(), 1,
    ops._stream())), 20.0 * xv.numel(), "round 5: per-channel maxima in the reduce pass, bound + two fp16 parts in the apply pass")
row("`az_absmax` (V0, 32 ch)", timeit(lambda: ops._call("az_absmax", dxa.data_ptr(), xv.data_ptr(), xv.numel(), ops._stream())), 4.0 * xv.numel(), "the stand-alone amax pass (f16x3 operand scale) where no producer kernel took it")
import bench as _bench  # the SAME probe bench.py's roofline.measured_hbm_gbps comes from (one implementation, one size: VERDICT r4 item 9)
_hb = _bench.hbm_probe(dev)
row("`az_hbm_copy_probe` (float4 copy, 1 GiB in + 1 GiB out; bench.hbm_probe)", 2.0 * (1 << 30) / 1e6 / _hb["GB/s"], 2.0 * (1 << 30), "bench.py's measured_hbm kernel, median of 7 after 3 warm-up launches")
row("`az_hbm_copy_probe` on the V0 tensor above (0.8 GB in + 0.8 GB out), 10 launches behind 2", timeit(lambda: ops._call("az_hbm_copy_probe", yv.data_ptr(), xv.data_ptr(), xv.numel(), ops._stream())), 8.0 * xv.numel(), "the round-4 table's row: same kernel, this tool's generic timer")
# 32 -> 1 classifier convolution (VALU kernels)
wc = torch.randn(1, C, 3, 3, 3, device=dev) * 0.05
lo = torch.empty(B, d, h, w, device=dev); gxc = torch.empty_like(xv); gwc = torch.empty_like(wc)
row("K4c `az_conv3d_c1_fwd`", timeit(lambda: ops._call("az_conv3d_c1_fwd", lo.data_ptr(), xv.data_ptr(), wc.data_ptr(), None, None, None, B, d, h, w, ops._stream())), 4.0 * (xv.numel() + lo.numel()))
row("K4c `az_conv3d_c1_dgrad`", timeit(lambda: ops._call("az_conv3d_c1_dgrad", gxc.data_ptr(), lo.data_ptr(), wc.data_ptr(), B, d, h, w, ops._stream())), 4.0 * (xv.numel() + lo.numel()))
row("K4c `az_conv3d_c1_wgrad`", timeit(lambda: ops._call("az_conv3d_c1_wgrad", gwc.data_ptr(), xv.data_ptr(), lo.data_ptr(), None, None, B, d, h, w, ops._stream())), 4.0 * (xv.numel() + lo.numel()))
# K10/K11 RAFT
f1, f2 = torch.randn(B, 256, h, w, device=dev), torch.randn(B, 256, h, w, device=dev)
ms = timeit(lambda: CorrBlock1D(f1, f2), reps=5)
rows.append(f"| K10 `az_corr1d_volume` + 4 pools | {ms:.3f} | {2.0 * 256 * B * h * w * w / 1e9:.1f} GFLOP | {2.0 * 256 * B * h * w * w / ms / 1e9:.1f} TFLOP/s | {2.0 * 256 * B * h * w * w / ms / 1e9 / 157.3 * 100:.0f} % of fp32 MFMA | generic strided batched GEMM |")
blk = CorrBlock1D(f1, f2)
coords = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")[::-1], 0).float()[None].repeat(B, 1, 1, 1).to(dev)
coords[:, 0] -= 20
row("K11 lookup, 4 levels x 9 taps", timeit(lambda: blk(coords)), 4.0 * B * h * w * (36 + 1 + 2 * 36))
print("| kernel | ms/launch | algorithmic MB | GB/s | of 8 TB/s | note |\n|---|---|---|---|---|---|")
print("\n".join(rows))
