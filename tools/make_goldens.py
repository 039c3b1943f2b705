#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE, imported from
/root/reference in the build container (CPU, torch fp32).

Only data (inputs' seeds / inputs / expected outputs) is written; no reference
source travels.  Re-run:  python tools/make_goldens.py
Harness-side shims (none of them edits the reference):
  * torch.Tensor.cuda -> identity, because the reference hard-codes .cuda()
    (nets/psmnet/psmnet_3.py:150-154, psmnet_submodule_3.py:83-85);
  * empty stand-in modules for `cupy` / `pynvrtc` so that utils/reprojection.py
    (which imports utils/warp_ops.py at module level) can be imported; the
    NVRTC scatter warp itself is NOT run (it cannot be);
  * (G12 / G13 / G14 only) inert stand-ins for `opt_einsum` and `configs.config`: nets/raft/update.py,
    nets/raft/raft_stereo.py and utils/losses.py import them at module level, but neither `ConvGRU`
    (update.py:19-41), `psmnet_disp` (losses.py:7-15) nor `sequence_loss` (losses.py:34-69) reads anything from
    them; `RAFTStereo.upsample_flow` reads cfg.MODEL.N_DOWNSAMPLE, which G14 sets on the stand-in.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(1, REF)

from tests._weights import load_procedural, seeded  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self  # shim 1
for name in ("cupy", "cupy.cuda", "pynvrtc", "pynvrtc.compiler"):  # shim 2
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["cupy.cuda"].function = types.SimpleNamespace(Module=object)
sys.modules["pynvrtc.compiler"].Program = object

from nets.psmnet import psmnet as ref_psmnet6  # noqa: E402
from nets.psmnet import psmnet_3 as ref_psmnet3  # noqa: E402
from nets.raft.corr import CorrBlock1D  # noqa: E402
from utils import reprojection as ref_reproj  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  keys={list(out)}")


class _Stop(Exception):
    pass


class _Fn(torch.nn.Module):
    """wrap a callable so it can replace a registered child module"""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, *a):
        return self.fn(*a)


# ---------------------------------------------------------------- G1 cost volume
def g1_cost_volume():
    b, c, h, w, nd = 2, 32, 8, 40, 12
    feat_l = seeded((b, c, h, w), 101).requires_grad_()
    feat_r = seeded((b, c, h, w), 102).requires_grad_()
    cot = seeded((b, 2 * c, nd, h, w), 103)
    model = ref_psmnet3.PSMNet(maxdisp=4 * nd)
    feats = iter([feat_l, feat_r])
    model.feature_extraction = _Fn(lambda _img: next(feats))
    grabbed = {}

    def grab(_m, args):
        grabbed["cost"] = args[0]
        raise _Stop

    model.dres0.register_forward_pre_hook(grab)
    try:
        model(torch.zeros(1), torch.zeros(1))
    except _Stop:
        pass
    cost = grabbed["cost"]
    gl, gr = torch.autograd.grad(cost, (feat_l, feat_r), cot)
    save("g1_cost_volume", seeds=[101, 102, 103], shape=[b, c, h, w, nd], cost=cost,
         grad_l=gl, grad_r=gr)


# ---------------------------------------------------------------- G2 soft-argmin head
def g2_softargmin():
    b, d, h, w = 2, 6, 5, 7
    k1 = (4 * seeded((b, 1, d, h, w), 201)).requires_grad_()
    d2 = (4 * seeded((b, 1, d, h, w), 202)).requires_grad_()
    d3 = (4 * seeded((b, 1, d, h, w), 203)).requires_grad_()
    cots = [seeded((b, 1, 4 * h, 4 * w), 204 + i) for i in range(3)]
    stub = types.SimpleNamespace(
        maxdisp=4 * d, training=True,
        feature_extraction=lambda _x: torch.zeros(b, 32, h, w),
        dres0=lambda c: c, dres1=lambda c: c,
        dres2=lambda x, p, q: (x, None, None), dres3=lambda x, p, q: (x, None, None),
        dres4=lambda x, p, q: (x, None, None),
        classif1=lambda _x: k1, classif2=lambda _x: d2, classif3=lambda _x: d3)
    p3, p2, p1 = ref_psmnet3.PSMNet.forward(stub, torch.zeros(1), torch.zeros(1))
    c1 = k1.detach()
    c2 = d2.detach() + c1
    c3 = d3.detach() + c2
    g1 = torch.autograd.grad(p1, k1, cots[0], retain_graph=True)[0]
    g2 = torch.autograd.grad(p2, d2, cots[1], retain_graph=True)[0]
    g3 = torch.autograd.grad(p3, d3, cots[2])[0]
    stub.training = False
    p3_eval = ref_psmnet3.PSMNet.forward(stub, torch.zeros(1), torch.zeros(1))
    assert torch.equal(p3_eval, p3)
    save("g2_softargmin", maxdisp=4 * d, cost1=c1, cost2=c2, cost3=c3, pred1=p1, pred2=p2,
         pred3=p3, cot1=cots[0], cot2=cots[1], cot3=cots[2], grad1=g1, grad2=g2, grad3=g3)
    # a full-size-in-D case (D=192 -> d=48) on a tiny image, forward only
    b, d, h, w = 1, 48, 3, 4
    k = (6 * seeded((b, 1, d, h, w), 211)).requires_grad_()
    z = torch.zeros_like(k)
    stub = types.SimpleNamespace(
        maxdisp=192, training=False, feature_extraction=lambda _x: torch.zeros(b, 32, h, w),
        dres0=lambda c: c, dres1=lambda c: c, dres2=lambda x, p, q: (x, None, None),
        dres3=lambda x, p, q: (x, None, None), dres4=lambda x, p, q: (x, None, None),
        classif1=lambda _x: z, classif2=lambda _x: z, classif3=lambda _x: k)
    p = ref_psmnet3.PSMNet.forward(stub, torch.zeros(1), torch.zeros(1))
    cot = seeded(tuple(p.shape), 212)
    g = torch.autograd.grad(p, k, cot)[0]
    save("g2_softargmin_d192", maxdisp=192, cost=k, pred=p, cot=cot, grad=g)


# ---------------------------------------------------------------- G3 3-D blocks
def g3_blocks():
    x = seeded((1, 32, 8, 8, 12), 301)
    pre = seeded((1, 64, 4, 4, 6), 302)
    post = seeded((1, 64, 4, 4, 6), 303)
    cot = seeded((1, 32, 8, 8, 12), 304)
    out = {}
    for mode in ("eval", "train"):
        for skips in (False, True):
            hg = load_procedural(ref_psmnet3.hourglass(32), "g3.hg.")
            hg.train(mode == "train")
            xi = x.clone().requires_grad_()
            o, p, q = hg(xi, pre if skips else None, post if skips else None)
            loss = (o * cot).sum() + p.sum() * 0.25 + q.sum() * 0.5
            loss.backward()
            tag = f"{mode}_{'skip' if skips else 'noskip'}"
            out[f"{tag}_out"], out[f"{tag}_pre"], out[f"{tag}_post"] = o, p, q
            out[f"{tag}_gx"] = xi.grad
            out[f"{tag}_gw_conv1"] = hg.conv1[0][0].weight.grad[:8, :8]
            out[f"{tag}_gw_conv5"] = hg.conv5[0].weight.grad[:8, :8]
            out[f"{tag}_gw_conv6"] = hg.conv6[0].weight.grad[:8, :8]
            out[f"{tag}_ggamma_conv2"] = hg.conv2[1].weight.grad
            out[f"{tag}_gbeta_conv6"] = hg.conv6[1].bias.grad
            if mode == "train":
                out[f"{tag}_rm_conv1"] = hg.conv1[0][1].running_mean
                out[f"{tag}_rv_conv1"] = hg.conv1[0][1].running_var
    save("g3_hourglass", seeds=[301, 302, 303, 304], **out)

    # single convbn_3d layers (the unit the HIP conv kernels are tested against)
    out = {}
    for cin, cout, stride in ((64, 32, 1), (32, 32, 1), (32, 64, 2), (64, 64, 2), (64, 64, 1)):
        layer = load_procedural(ref_psmnet3.convbn_3d(cin, cout, 3, stride, 1),
                                f"g3.cb{cin}_{cout}_{stride}.")
        xin = seeded((2, cin, 4, 6, 8), 310 + cin + cout + stride).requires_grad_()
        for mode in ("eval", "train"):
            layer.train(mode == "train")
            y = layer(xin)
            ct = seeded(tuple(y.shape), 320)
            gx, gw, gg, gb = torch.autograd.grad(
                y, (xin, layer[0].weight, layer[1].weight, layer[1].bias), ct)
            tag = f"cb{cin}_{cout}_{stride}_{mode}"
            out[tag + "_y"], out[tag + "_gx"], out[tag + "_gw"] = y, gx, gw[:8, :8]
            out[tag + "_gg"], out[tag + "_gb"] = gg, gb
    save("g3_convbn3d", **out)


# ---------------------------------------------------------------- G4 full PSMNet
def g4_full():
    h = w = 256
    maxdisp = 32
    nb = 2  # train-mode BatchNorm after the 64x64 SPP pooling needs > 1 value per channel
    gt = 1.0 + 28.0 * torch.sigmoid(
        F.interpolate(seeded((nb, 1, 8, 8), 404, -3, 3), size=(h, w), mode="bilinear",
                      align_corners=False))
    gt[:, :, :40, :30] = 0.0  # invalid region -> exercised by the mask
    mask = (gt < maxdisp) * (gt > 0)
    for variant, mod, nin in (("psmnet3", ref_psmnet3, 3), ("psmnet6", ref_psmnet6, 6)):
        imgs = [seeded((nb, 3, h, w), 400 + i, -2.0, 2.0) for i in range(4)]
        args = imgs[:2] if nin == 3 else imgs
        model = load_procedural(mod.PSMNet(maxdisp=maxdisp), "g4.")
        nkeys = len(model.state_dict())
        # calibrate the BatchNorm running statistics with one momentum-1 training pass
        # (procedural running stats make the 28-layer eval net blow up into the chaotic,
        # saturated regime); the calibrated buffers travel in the golden file.
        bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        for m in bns:
            m.momentum = 1.0
        model.train()
        with torch.no_grad():
            model(*args)
        for m in bns:
            m.momentum = 0.1
        bufs0 = {"buf::" + k: v.clone() for k, v in model.state_dict().items()
                 if k.endswith("running_mean") or k.endswith("running_var")}
        model.eval()
        with torch.no_grad():
            pred_eval = model(*args)
        model.train()
        p3, p2, p1 = model(*args)
        sl1 = lambda p: F.smooth_l1_loss(p[mask], gt[mask], reduction="mean")
        loss = 0.5 * sl1(p1) + 0.7 * sl1(p2) + sl1(p3)  # utils/losses.py:7-15
        loss.backward()
        sd = dict(model.named_parameters())
        grads = {
            "g_dres0_0_0": sd["dres0.0.0.weight"].grad[:4, :4],
            "g_classif3_2": sd["classif3.2.weight"].grad,
            "g_dres4_conv5_0": sd["dres4.conv5.0.weight"].grad[:4, :4],
            "g_dres2_conv1_0_1_w": sd["dres2.conv1.0.1.weight"].grad,
            "g_fe_lastconv_2": sd["feature_extraction.lastconv.2.weight"].grad[:, :8, 0, 0],
            "g_fe_firstconv_0_0": sd["feature_extraction.firstconv.0.0.weight"].grad[:4],
        }
        bufs = dict(model.named_buffers())
        save(f"g4_{variant}", seeds=[400, 401, 402, 403, 404], maxdisp=maxdisp, nkeys=nkeys,
             keys=np.array(sorted(model.state_dict().keys())), gt=gt, pred_stride=2,
             pred_eval=pred_eval[..., ::2, ::2], pred3=p3[..., ::2, ::2],
             pred2=p2[..., ::2, ::2], pred1=p1[..., ::2, ::2], loss=loss,
             rm_dres0=bufs["dres0.0.1.running_mean"], rv_dres0=bufs["dres0.0.1.running_var"],
             **grads, **bufs0)


# ---------------------------------------------------------------- G6-G8 reprojection
def g6_apply_disparity():
    img = seeded((2, 3, 9, 17), 601)
    disp = seeded((2, 1, 9, 17), 602, -6.0, 6.0)
    disp[0, 0, 0, :4] = torch.tensor([30.0, -30.0, 16.5, -0.25])  # far out of range
    disp.requires_grad_()
    cot = seeded((2, 3, 9, 17), 603)
    out = ref_reproj.apply_disparity(img, disp)
    (g,) = torch.autograd.grad(out, disp, cot)
    save("g6_apply_disparity", img=img, disp=disp, out=out, cot=cot, grad=g)


def g7_patch():
    b, h, w = 2, 12, 20
    out = {}
    pat_l = (seeded((b, 1, h, w), 701, 0, 1) < 0.3).float()
    pat_r = (seeded((b, 1, h, w), 702, 0, 1) < 0.3).float()
    con_l, con_r = seeded((b, 1, h, w), 703), seeded((b, 1, h, w), 704)
    disp0 = seeded((b, 1, h, w), 705, 0.0, 6.0)
    mask = seeded((b, 1, h, w), 706, 0, 1) < 0.7
    out.update(pat_l=pat_l, pat_r=pat_r, con_l=con_l, con_r=con_r, disp=disp0, mask=mask)
    for kind, (l, r) in (("pat", (pat_l, pat_r)), ("con", (con_l, con_r))):
        for ps in (1, 3, 11):
            for use_mask in (False, True):
                d = disp0.clone().requires_grad_()
                loss, vis, m = ref_reproj.get_reproj_error_patch(
                    l, r, d, mask if use_mask else None, ps)
                loss.backward()
                tag = f"{kind}_ps{ps}_{'mask' if use_mask else 'nomask'}"
                out[tag + "_loss"], out[tag + "_vis"], out[tag + "_m"] = loss, vis, m
                out[tag + "_grad"] = d.grad
    # two-channel input (API allows c > 1)
    l2, r2 = seeded((1, 2, 8, 10), 707), seeded((1, 2, 8, 10), 708)
    d2 = seeded((1, 1, 8, 10), 709, 0.0, 4.0).requires_grad_()
    loss, vis, m = ref_reproj.get_reproj_error_patch(l2, r2, d2, None, 3)
    loss.backward()
    out.update(c2_l=l2, c2_r=r2, c2_disp=d2, c2_loss=loss, c2_vis=vis, c2_m=m, c2_grad=d2.grad)
    save("g7_reproj_patch", **out)

    # whole-image variants (API surface a10)
    img_l, img_r = seeded((2, 3, 16, 24), 711), seeded((2, 3, 16, 24), 712)
    d = seeded((2, 1, 16, 24), 713, 0.0, 5.0).requires_grad_()
    mk = seeded((2, 1, 16, 24), 714, 0, 1) < 0.6
    lo, wo, mo = ref_reproj.get_reprojection_error_old(img_l, img_r, d, mk)
    (go,) = torch.autograd.grad(lo, d)
    lo2, wo2, mo2 = ref_reproj.get_reprojection_error_old(img_l, img_r, d, None)
    tot, stages, parts = ref_reproj.get_reprojection_error_diff_ratio(img_l, img_r, d, mk)
    (gd,) = torch.autograd.grad(tot, d)
    save("g7_reproj_image", img_l=img_l, img_r=img_r, disp=d, mask=mk, old_loss=lo,
         old_warped=wo, old_mask=mo, old_grad=go, old_nomask_loss=lo2, old_nomask_mask=mo2,
         dr_total=tot, dr_grad=gd, dr_parts=np.array([parts[f"stage{i}"] for i in range(3)]),
         dr_warped0=stages["stage0"]["warped"], dr_warped2=stages["stage2"]["warped"],
         dr_mask1=stages["stage1"]["mask"], dr_disp0=stages["stage0"]["pred_disp"])


def g8_lcn():
    img = seeded((2, 1, 12, 20), 801, 0.0, 1.0)
    img3 = seeded((1, 3, 6, 9), 802, 0.0, 1.0)
    out = dict(img=img, img3=img3)
    for k in (3, 9):
        n, s = ref_reproj.local_contrast_norm(img, k)
        out[f"k{k}_normed"], out[f"k{k}_std"] = n, s
    n, s = ref_reproj.local_contrast_norm(img3, 5)
    out["c3_normed"], out["c3_std"] = n, s
    save("g8_lcn", **out)


# ---------------------------------------------------------------- G9 RAFT 1-D correlation
def g9_corr():
    f1 = seeded((1, 16, 6, 20), 901).requires_grad_()
    f2 = seeded((1, 16, 6, 20), 902).requires_grad_()
    coords = torch.stack(torch.meshgrid(torch.arange(6), torch.arange(20), indexing="ij")[::-1],
                         0).float()[None]
    coords = coords.clone()
    coords[:, 0] -= seeded((1, 6, 20), 903, 0.0, 9.0)
    blk = CorrBlock1D(f1, f2, num_levels=4, radius=4)
    out = blk(coords)
    cot = seeded(tuple(out.shape), 904)
    g1, g2 = torch.autograd.grad(out, (f1, f2), cot)
    save("g9_corr1d", fmap1=f1, fmap2=f2, coords=coords, out=out, cot=cot, grad1=g1, grad2=g2,
         **{f"pyr{i}": p for i, p in enumerate(blk.corr_pyramid[:4])})


# ---------------------------------------------------------------- G10 loss + error metrics
def g10_metrics():
    """compute_err_metric / compute_obj_err: the imported reference (utils/cascade_metrics.py).
    psmnet_disp: utils/losses.py is not importable here (its module imports the yacs config), so
    its three-line formula (losses.py:7-15) is evaluated with the same torch calls on boolean-
    indexed operands, as SURVEY.md 8c prescribes."""
    from utils import cascade_metrics as ref_metrics

    b, h, w = 2, 24, 40
    gt = seeded((b, 1, h, w), 1001, 0.0, 60.0)
    gt[:, :, :3] = 0.0          # invalid rows (gt == 0)
    gt[0, 0, 10, :5] = 70.0     # beyond maxdisp
    maxdisp = 64.0
    mask = (gt < maxdisp) & (gt > 0)
    preds = [(gt + seeded((b, 1, h, w), 1002 + k, -3.0, 3.0)).requires_grad_() for k in range(3)]
    p3, p2, p1 = preds
    loss = (0.5 * F.smooth_l1_loss(p1[mask], gt[mask], reduction="mean")
            + 0.7 * F.smooth_l1_loss(p2[mask], gt[mask], reduction="mean")
            + F.smooth_l1_loss(p3[mask], gt[mask], reduction="mean"))
    g3, g2, g1 = torch.autograd.grad(loss, (p3, p2, p1))
    focal = seeded((b, 1, 1, 1), 1010, 400.0, 500.0)
    base = seeded((b, 1, 1, 1), 1011, 0.05, 0.06)
    depth_gt = torch.where(gt > 0, focal * base / gt.clamp(min=1e-3), torch.zeros_like(gt))
    pred = p3.detach().clamp(min=0.5)
    m = ref_metrics.compute_err_metric(gt, depth_gt, pred, focal, base, mask)
    depth_pred = focal * base / pred + 1e-3
    m2 = ref_metrics.compute_err_metric(gt, depth_gt, pred, focal, base, mask, depth_pred=depth_pred)
    label = (seeded((1, 1, h, w), 1012, 0.0, 4.99)).floor()
    obj = ref_metrics.compute_obj_err(gt[:1], depth_gt[:1], pred[:1], focal[:1], base[:1], label, mask[:1])
    keys = sorted(m)
    save("g10_metrics", gt=gt, mask=mask, pred3=p3, pred2=p2, pred1=p1, maxdisp=maxdisp, loss=loss,
         grad3=g3, grad2=g2, grad1=g1, focal=focal, baseline=base, depth_gt=depth_gt, disp_pred=pred,
         depth_pred=depth_pred, metric_keys=np.array(keys), metrics=np.array([m[k] for k in keys]),
         metrics_dp=np.array([m2[k] for k in keys]), label=label, **{f"obj{i}": o for i, o in enumerate(obj)})


# ---------------------------------------------------------------- G11 full PSMNet at D = 192
def g11_full_d192():
    """nets/psmnet/psmnet_3.py:144-220 at the headline disparity range (maxdisp = 192, 0..191 px), where
    the 1e-3 px bar is hardest: one 256x512 pair, eval and train-mode predictions, evaluated by the
    imported reference in fp32 AND in fp64 (harness shim 3: torch.FloatTensor -> DoubleTensor while the
    fp64 pass runs, because forward() allocates the cost volume with torch.FloatTensor), plus one
    540->544x960 eval forward in both precisions.  The fp64 run is the yardstick that says how far ANY
    fp32 evaluation order may sit from the exact result (|ref32 - ref64|)."""
    maxdisp = 192
    il, ir = seeded((1, 3, 256, 512), 1101, -2.0, 2.0), seeded((1, 3, 256, 512), 1102, -2.0, 2.0)
    big = [F.pad(seeded((1, 3, 540, 960), 1103 + i, -2.0, 2.0), (0, 0, 4, 0)) for i in range(2)]  # test.py:137-146
    model = load_procedural(ref_psmnet3.PSMNet(maxdisp=maxdisp), "g11.")
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    for m in bns:
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(il, ir)
    for m in bns:
        m.momentum = 0.1
    bufs0 = {"buf::" + k: v.clone() for k, v in model.state_dict().items()
             if k.endswith("running_mean") or k.endswith("running_var")}
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    out = {}
    st, st_big = 3, 5
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        model.load_state_dict(sd0)
        model.to(dt)
        real_ft = torch.FloatTensor
        if dt == torch.float64:
            torch.FloatTensor = torch.DoubleTensor  # shim 3 (harness side)
        try:
            with torch.no_grad():
                model.eval()
                out["eval" + tag] = model(il.to(dt), ir.to(dt))[..., ::st, ::st]
                out["big_eval" + tag] = model(big[0].to(dt), big[1].to(dt))[..., ::st_big, ::st_big]
                model.train()  # batch statistics (running stats are restored from sd0 for the next pass)
                p3, p2, p1 = model(il.to(dt), ir.to(dt))
                out["pred3_" + tag], out["pred2_" + tag], out["pred1_" + tag] = (
                    p[..., ::st, ::st] for p in (p3, p2, p1))
        finally:
            torch.FloatTensor = real_ft
        print("g11", tag, "done", flush=True)
    for k in ("eval", "big_eval", "pred3_", "pred2_", "pred1_"):
        d = (out[k + "32"].double() - out[k + "64"]).abs()
        print(f"  |ref32 - ref64| {k}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    save("g11_psmnet3_d192", seeds=[1101, 1102, 1103, 1104], maxdisp=maxdisp, pred_stride=st,
         big_stride=st_big, **out, **bufs0)


# ---------------------------------------------------------------- G12 RAFT-Stereo ConvGRU
def _import_with_inert_stubs(modname):
    """import a reference module whose top-level imports name packages this image lacks but whose code
    under test never touches them (shim 4)"""
    import importlib
    if "opt_einsum" not in sys.modules:
        m = types.ModuleType("opt_einsum")
        m.contract = None
        sys.modules["opt_einsum"] = m
    if "configs.config" not in sys.modules:
        pkg = types.ModuleType("configs")
        pkg.__path__ = []
        m = types.ModuleType("configs.config")
        m.cfg = types.SimpleNamespace()
        pkg.config = m
        sys.modules["configs"], sys.modules["configs.config"] = pkg, m
    return importlib.import_module(modname)


def g12_convgru():
    """nets/raft/update.py:19-41 `ConvGRU.forward(h, cz, cr, cq, *x_list)`, the class itself imported from the
    reference: fp32 and fp64 evaluations and the reference's own arithmetic for this block (CPU
    autocast(bfloat16), raft_stereo.py:142 wraps the update block in autocast), one update and four chained
    updates; plus value / gradient goldens of the fp32 path for the autograd route."""
    upd = _import_with_inert_stubs("nets.raft.update")
    out = {}
    cases = [("a", 128, (128,), (34, 60), 2), ("b", 128, (128, 128), (17, 30), 2), ("c", 64, (32, 48), (9, 21), 1),
             ("d", 64, (64,), (12, 20), 1)]  # d: the gradient case (channel counts of the differentiable kernels)
    for tag, hidden, cx, (h, w), b in cases:
        mod = load_procedural(upd.ConvGRU(hidden, sum(cx)), f"g12{tag}.")
        for name in ("convz", "convr", "convq"):  # biases: procedural_tensor's 1-D rule is the BN-beta one
            assert getattr(mod, name).bias.abs().max() > 0
        sd = 1200 + 10 * (ord(tag) - ord("a"))
        hid = torch.tanh(seeded((b, hidden, h, w), sd, -2.0, 2.0))
        ctx = [seeded((b, hidden, h, w), sd + 1 + i, -0.8, 0.8) for i in range(3)]
        xs = [seeded((b, n, h, w), sd + 4 + i, -1.7, 1.7) for i, n in enumerate(cx)]
        # inputs are regenerated from the seeds by the test; outputs are stored on a channel / pixel lattice
        cs, ps = (1, 1) if tag in "cd" else (4, 2)
        lat = lambda t: t[:, ::cs, ::ps, ::ps]
        out[f"{tag}_meta"] = np.array([hidden, h, w, b, sd, cs, ps] + list(cx))
        with torch.no_grad():
            out[f"{tag}_out32"] = lat(mod(hid, *ctx, *xs))
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out[f"{tag}_outamp"] = lat(mod(hid, *ctx, *xs).float())
            # round 5: torch.cuda.amp.autocast (raft_stereo.py:14), the reference's own arithmetic for this
            # block, is FLOAT16 on CUDA (11-bit operands, GradScaler) -- the bfloat16 yardstick above is 8x coarser
            with torch.autocast("cpu", dtype=torch.float16):
                out[f"{tag}_outamp16"] = lat(mod(hid, *ctx, *xs).float())
            hh = hid
            for _ in range(4):
                hh = mod(hh, *ctx, *xs)
            out[f"{tag}_iter4_32"] = lat(hh)
            mod.double()
            out[f"{tag}_out64"] = lat(mod(hid.double(), *[c.double() for c in ctx], *[x.double() for x in xs]))
            hh = hid.double()
            for _ in range(4):
                hh = mod(hh, *[c.double() for c in ctx], *[x.double() for x in xs])
            out[f"{tag}_iter4_64"] = lat(hh)
            mod.float()
        if tag == "d":  # gradients of the fp32 path (the product's autograd route)
            cot = seeded((b, hidden, h, w), sd + 9)
            hr = hid.clone().requires_grad_(True)
            (mod(hr, *ctx, *xs) * cot).sum().backward()
            out["d_gh"] = hr.grad
            for name in ("convz", "convr", "convq"):
                out[f"d_gw_{name}"] = getattr(mod, name).weight.grad[:16, :32]
                out[f"d_gb_{name}"] = getattr(mod, name).bias.grad
            # round 4: the same gradients in the reference's TRAINING arithmetic -- the update block under autocast
            # (raft_stereo.py:142-172, train.py:303-309; bfloat16 on the CPU) -- and in fp64: the distance between the two
            # is what a valid 16-bit evaluation of these gradients may be off by (whole tensors: the norms matter)
            mod.zero_grad(set_to_none=True)
            hr = hid.clone().requires_grad_(True)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                o = mod(hr, *ctx, *xs)
            (o.float() * cot).sum().backward()
            out["d_gh_amp"] = hr.grad.float()
            for name in ("convz", "convr", "convq"):
                out[f"d_gwfull_amp_{name}"] = getattr(mod, name).weight.grad.float()
                out[f"d_gb_amp_{name}"] = getattr(mod, name).bias.grad.float()
            mod.zero_grad(set_to_none=True)
            hr = hid.clone().requires_grad_(True)
            with torch.autocast("cpu", dtype=torch.float16):  # (see _outamp16; unit cotangent scale: no GradScaler needed)
                o = mod(hr, *ctx, *xs)
            (o.float() * cot).sum().backward()
            out["d_gh_amp16"] = hr.grad.float()
            for name in ("convz", "convr", "convq"):
                out[f"d_gwfull_amp16_{name}"] = getattr(mod, name).weight.grad.float()
                out[f"d_gb_amp16_{name}"] = getattr(mod, name).bias.grad.float()
            mod.zero_grad(set_to_none=True)
            mod.double()
            hr = hid.double().requires_grad_(True)
            (mod(hr, *[c.double() for c in ctx], *[x.double() for x in xs]) * cot.double()).sum().backward()
            out["d_gh64"] = hr.grad
            for name in ("convz", "convr", "convq"):
                out[f"d_gwfull64_{name}"] = getattr(mod, name).weight.grad
                out[f"d_gb64_{name}"] = getattr(mod, name).bias.grad
            mod.float()
    save("g12_convgru", **out)


# ---------------------------------------------------------------- G13 configs[1] at full size, train mode
def g13_full_train_d192():
    """BASELINE.json configs[1] through the imported reference, one pair: nets/psmnet/psmnet_3.py:144-220 in
    TRAIN mode on a 540->544x960 pair at maxdisp 192, utils/losses.py:7-15 `psmnet_disp`, backward.  fp32 (the
    reference's own arithmetic) and fp64 (how far any fp32 evaluation of these predictions / gradients may sit
    from exact).  Stored: strided predictions, the loss, the mask count, whole small gradients and slices of
    the large ones, the updated running statistics of two BatchNorms."""
    import time
    losses = _import_with_inert_stubs("utils.losses")
    maxdisp, st = 192, 5
    il, ir = (F.pad(seeded((1, 3, 540, 960), 1103 + i, -2.0, 2.0), (0, 0, 4, 0)) for i in range(2))
    gt = seeded((1, 1, 544, 960), 1301, -12.0, 215.0)
    mask = (gt < maxdisp) * (gt > 0)  # train.py:272
    out = {"n_mask": int(mask.sum())}
    grads_of = {
        "classif3.2.weight": None, "classif1.2.weight": None,
        "dres0.0.0.weight": (slice(0, 4), slice(0, 8)), "dres1.2.0.weight": (slice(0, 4), slice(0, 4)),
        "dres2.conv1.0.0.weight": (slice(0, 4), slice(0, 4)), "dres3.conv5.0.weight": (slice(0, 4), slice(0, 4)),
        "dres4.conv6.0.weight": (slice(0, 4), slice(0, 4)), "dres4.conv2.0.weight": (slice(0, 2), slice(0, 4)),
        "feature_extraction.firstconv.0.0.weight": None,
        "feature_extraction.layer3.1.conv2.0.weight": (slice(0, 4), slice(0, 4)),
        "feature_extraction.lastconv.2.weight": (slice(0, 8), slice(0, 16)),
        "dres1.0.1.weight": None, "dres1.0.1.bias": None, "feature_extraction.layer1.0.conv1.0.1.weight": None,
    }
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        t0 = time.time()
        model = load_procedural(ref_psmnet3.PSMNet(maxdisp=maxdisp), "g11.").to(dt).train()
        real_ft = torch.FloatTensor
        if dt == torch.float64:
            torch.FloatTensor = torch.DoubleTensor  # shim 3
        try:
            assert all(n in dict(model.named_parameters()) for n in grads_of)
            preds = model(il.to(dt), ir.to(dt))
        finally:
            torch.FloatTensor = real_ft
        loss = losses.psmnet_disp(preds, gt.to(dt), mask)
        loss.backward()
        for p, k in zip(preds, ("pred3_", "pred2_", "pred1_")):
            out[k + tag] = p.detach()[..., ::st, ::st]
        out["loss" + tag] = loss.detach()
        params = dict(model.named_parameters())
        for name, sl in grads_of.items():
            g = params[name].grad
            out[f"g{tag}::{name}"] = g if sl is None else g[sl]
            out[f"gn{tag}::{name}"] = g.double().norm()  # L2 norm of the WHOLE gradient tensor
        bufs = dict(model.named_buffers())
        for name in ("dres0.0.1.running_var", "dres4.conv6.1.running_mean"):
            out[f"buf{tag}::{name}"] = bufs[name]
        del model, preds, loss, params
        print(f"g13 {tag} done in {time.time() - t0:.0f} s", flush=True)
    for k in ("pred3_", "pred2_", "pred1_"):
        d = (out[k + "32"].double() - out[k + "64"]).abs()
        print(f"  |ref32 - ref64| {k}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    print(f"  loss32 {out['loss32'].item():.7f} loss64 {out['loss64'].item():.7f}")
    for name in grads_of:
        a, b = out[f"g32::{name}"].double(), out[f"g64::{name}"]
        print(f"  grad rel-L2 ref32 vs ref64 {name}: {((a - b).norm() / b.norm()).item():.3e}")
    save("g13_psmnet3_train_d192", seeds=[1103, 1104, 1301], maxdisp=maxdisp, pred_stride=st, **out)


# ---------------------------------------------------------------- G14 RAFT-Stereo prediction head
def g14_raft_head():
    """nets/raft/raft_stereo.py:74-86 `RAFTStereo.upsample_flow` (called unbound: it reads nothing from self) and
    utils/losses.py:34-69 `sequence_loss`, both imported from the reference, in fp32 and fp64; the upsampling also with
    the mask rounded to fp16 and evaluated as under cfg.MODEL.MIXED_PRECISION (the mask head's output is fp16 there:
    softmax in fp16, product with the fp32 flow in fp32) beside fp64 of the same fp16-valued inputs.  Inputs are
    regenerated from the seeds by the tests; the large outputs are stored on lattices (`*_lat` = the strides)."""
    from tests._raft_head_ref import make_mask_logits
    rs = _import_with_inert_stubs("nets.raft.raft_stereo")
    losses = _import_with_inert_stubs("utils.losses")
    cfg = sys.modules["configs.config"].cfg
    out = {}
    # tag, factor, flow shape, zero the y channel, seed
    cases = [("a", 4, (2, 2, 9, 13), False, 1401), ("b", 8, (1, 2, 5, 7), True, 1411)]
    up_lat, gm_lat = (3, 3), (3, 4)  # 3 is coprime to both factors: every sub-pixel (i, j) is sampled
    for tag, f, shape, zero_y, sd in cases:
        cfg.MODEL = types.SimpleNamespace(N_DOWNSAMPLE={4: 2, 8: 3}[f])
        n, d, h, w = shape
        flow = seeded(shape, sd, -3.0, 3.0)
        if zero_y:
            flow[:, 1] = 0.0
        mask = make_mask_logits((n, 9 * f * f, h, w), sd + 1)
        cot = seeded((n, d, f * h, f * w), sd + 2)
        out[f"{tag}_meta"] = np.array([f, n, d, h, w, sd, int(zero_y)])

        def run(fl, mk, key):
            fl, mk = fl.clone().requires_grad_(True), mk.clone().requires_grad_(True)
            up = rs.RAFTStereo.upsample_flow(None, fl, mk)
            gf, gm = torch.autograd.grad(up, (fl, mk), cot.to(up.dtype))
            out[f"{tag}_up{key}"] = up[..., ::up_lat[0], ::up_lat[1]]
            out[f"{tag}_gflow{key}"] = gf
            out[f"{tag}_gmask{key}"] = gm[..., ::gm_lat[0], ::gm_lat[1]]
            return up, gf, gm

        r32 = run(flow, mask, "32")
        r64 = run(flow.double(), mask.double(), "64")
        m16 = mask.half()
        ramp = run(flow, m16, "_amp")  # fp16 softmax, fp32 product; g_mask comes back in fp16
        r64h = run(flow.double(), m16.double(), "64_h")
        for name, a, b in (("fp32", r32, r64), ("amp", ramp, r64h)):
            print(f"  g14 {tag} {name}: max |ref - ref64| up {(a[0].double() - b[0]).abs().max():.3e} "
                  f"gflow {(a[1].double() - b[1]).abs().max():.3e} gmask {(a[2].double() - b[2]).abs().max():.3e}")
    # sequence loss: [2,1,36,52], a zero region in valid, some |gt| >= max_flow
    shape, sd = (2, 1, 36, 52), 1421
    gt = seeded(shape, sd, -40.0, 820.0)
    valid = (seeded(shape, sd + 1, 0.0, 1.0) > 0.1).float()
    valid[:, :, 5:17, 20:41] = 0.0
    st = 2
    for n_pred in (4, 22):
        preds = [-gt + seeded(shape, sd + 10 + i, -3.0, 3.0) * (1.0 + 0.2 * (n_pred - i)) for i in range(n_pred)]
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            ps = [p.to(dt).requires_grad_(True) for p in preds]
            loss = losses.sequence_loss(ps, gt.to(dt), valid.to(dt), loss_gamma=0.9, max_flow=700)
            grads = torch.autograd.grad(loss, ps)
            out[f"s{n_pred}_loss{tag}"] = loss
            out[f"s{n_pred}_grads{tag}"] = torch.stack(grads)[..., ::st, ::st]
        print(f"  g14 seq n={n_pred}: loss32 {out[f's{n_pred}_loss32'].item():.7f} loss64 {out[f's{n_pred}_loss64'].item():.7f}")
    save("g14_raft_head", seeds=[1401, 1411, 1421], up_lat=up_lat, gmask_lat=gm_lat, seq_lat=st, max_flow=700.0,
         loss_gamma=0.9, **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for fn in (g1_cost_volume, g2_softargmin, g3_blocks, g4_full, g6_apply_disparity, g7_patch,
               g8_lcn, g9_corr, g10_metrics, g11_full_d192, g12_convgru, g13_full_train_d192,
               g14_raft_head):
        if not only or fn.__name__.split("_")[0] in only:
            fn()
